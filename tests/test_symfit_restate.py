"""The contract of mad_assembly_refine_symmetric restated in numpy (jointfit.symmetric_refine_numpy), the
python side's arguments and results, and the plan restated from csrc/mad_jointfit_plan.h.  No device."""
import os
import re

import numpy as np
import pytest

from mad_amd import _lib, jointfit, symmetry

import jointfit_cases as jc
import symfit_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING3_SEEDS = (1, 2, 3, 4)


def test_one_operator_is_joint_refine_numpy():
    """K = 1: every statement is joint_refine_numpy's, and every output the same bits."""
    s = jc.two_body_scene(10.0, 10)
    want = jc.restated((10.0, 10))
    got = jointfit.symmetric_refine_numpy(s["grid"], jc.ORIGIN, jc.VS, s["start"], s["masses"], np.identity(3)[None], np.zeros((1, 3)),
                                          s["resolution"], n_steps=jc.N_STEPS)
    assert sorted(got) == sorted(want)
    for k in ("coords", "R", "T"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[k], want[k]))
    assert got["converged"] == want["converged"] and got["last_step"] == want["last_step"] and got["n_rounds"] == want["n_rounds"]
    assert got["scale"].tobytes() == want["scale"].tobytes() and got["margin"] == want["margin"]


@pytest.mark.parametrize("seed", RING3_SEEDS)
def test_ring3_constrained_against_free(seed):
    """The unit ends closer to the truth than it started, and its images are exact copies; joint_refine_numpy on the three copies
    as free bodies gives a ring that is no ring any more.  Constrained RMSD to the truth <= the mean of the three free bodies':
    the restatement shows it for every seed tried (1 to 4: 0.049 / 0.080, 0.047 / 0.082, 0.038 / 0.047, 0.037 / 0.053 A), so it is
    asserted for all of them; there is no seed to name where it does not hold."""
    s, got, free = sc.scene("ring3", seed), sc.restated("ring3", seed), sc.restated_free("ring3", seed)
    ops = s["ops"]
    assert got["margin"] >= 1e-4 and got["converged"] == [True]
    end, begin = jc.rmsd(got["coords"][0], s["truth"][0]), jc.rmsd(s["start"][0], s["truth"][0])
    assert end < 0.2 < 2.5 < begin
    images = np.stack([jointfit.image_numpy(got["coords"][0], ops.R, ops.T, g) for g in range(3)])
    np.testing.assert_allclose(images, ops.copies(got["coords"][0]), rtol=0, atol=1e-9)
    assert images[0] is got["coords"][0] or np.array_equal(images[0], got["coords"][0])
    truth = ops.copies(s["truth"][0])
    free_rmsd = [jc.rmsd(free["coords"][g], truth[g]) for g in range(3)]
    dev = max(np.abs(free["coords"][g] - ops.copies(free["coords"][0])[g]).max() for g in (1, 2))
    print("ring3 seed %d: constrained %.4f A to the truth, free %s (mean %.4f), free bodies off their copies by %.3g A, margins %.3g / %.3g"
          % (seed, end, np.round(free_rmsd, 4), np.mean(free_rmsd), dev, got["margin"], free["margin"]))
    assert dev > 1e-6
    assert end <= np.mean(free_rmsd)


@pytest.mark.parametrize("name", sc.SCENES)
def test_scenes_meet_their_conditions(name):
    """Every scene decides its batches by 1e-4 A or more, moves every free unit towards the truth, and shows what it is there for."""
    s, got = sc.scene(name), sc.restated(name)
    K, U = len(s["ops"]), len(s["start"])
    print("%s: %d units x %d operators, margin %.3g, rounds %d, last_step %s" % (name, U, K, got["margin"], got["n_rounds"], got["last_step"]))
    assert got["margin"] >= 1e-4 and U * K <= jointfit.MAX_BODIES
    assert np.array_equal(s["ops"].R[0], np.identity(3)) and not s["ops"].T[0].any()
    for u in range(U):
        if s["fixed"] and s["fixed"][u]:
            assert np.array_equal(got["coords"][u], s["start"][u]) and got["last_step"][u] == -1
        else:
            assert jc.rmsd(got["coords"][u], s["truth"][u]) < jc.rmsd(s["start"][u], s["truth"][u])
    assert (U, K) == dict(ring3=(1, 3), d2pair=(2, 4), big2=(1, 2), ico=(1, 60), full64=(8, 8), overhang=(1, 2))[name]
    if name == "overhang":
        for c in (s["start"][0], got["coords"][0]):
            out = jc.outside_the_map(s["ops"].copies(c)[1], s["shape"])
            assert 20 <= out <= len(c) - 20 and jc.outside_the_map(c, s["shape"]) == 0
    elif name != "full64":      # every image inside the lattice
        assert all(jc.outside_the_map(im, s["shape"]) == 0 for c in s["start"] for im in s["ops"].copies(c))


def test_the_plan_restated():
    """G and the workgroups of every scene at 256 compute units, by jf_groups with the image count for the body count; the new
    constants against the header's."""
    text = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_jointfit_plan.h")).read()
    assert re.search(r"#define\s+JF_SYM_ORTHO_TOL\s+1e-6\b", text) and jointfit.ORTHO_TOL == 1e-6
    assert re.search(r"#define\s+JF_SYM_MAX_MEMBERS\s+\(JF_MAX_BODIES \* JF_MAX_G\)", text)
    want = dict(ring3=(1, 1, 3), d2pair=(1, 1, 8), big2=(2, 1, 4), ico=(1, 1, 60), full64=(1, 1, 64), overhang=(1, 1, 2))
    for name in sc.SCENES:
        s = sc.scene(name)
        plan = sc.expected_plan([len(c) for c in s["start"]], len(s["ops"]), 256)
        assert plan == want[name] and plan[2] <= 256
    assert sc.expected_plan([4100], 2, 256, split=1) == (1, 0, 2) and sc.expected_plan([4100], 2, 256, registers=0) == (2, 0, 4)
    assert sc.expected_plan([26000], 4, 256) == (8, 1, 32) and sc.expected_plan([1 << 20], 60, 256) == (4, 0, 240)
    assert sc.expected_plan([30, 30], 1, 256) == jc.expected_plan([30, 30], 256)


def test_arguments_of_the_python_side(tmp_path):
    a, b = np.zeros((4, 3)), np.ones((2, 3))
    coords, ms, src = jointfit.bodies_of("t", [a, b])
    assert [len(c) for c in coords] == [4, 2] and src == [None, None]
    c4 = symmetry.point_group("C4", centre=(1.0, 2.0, 3.0))
    assert jointfit.operators_of("t", c4) is c4
    pair = jointfit.operators_of("t", (c4.R, c4.T))
    assert np.array_equal(pair.R, c4.R) and np.array_equal(pair.T, c4.T)

    class Found(object):
        def operators(self):
            return c4
    assert jointfit.operators_of("t", Found()) is c4
    found = symmetry.Symmetry("C4", 4, (0.0, 0.0, 1.0), None, (1.0, 2.0, 3.0), 1.0, [], 10.0, 1)
    assert len(jointfit.operators_of("t", found)) == 4
    mirror = np.array([np.identity(3), np.diag([1.0, 1.0, -1.0])])
    for bad, match in (("C4", "symmetry must be"), ((c4.R, c4.T[:3]), "shape"), ((c4.R[[1, 0, 2, 3]], c4.T[[1, 0, 2, 3]]), "identity"),
                       ((c4.R * 1.001, c4.T * 0), "identity"), ((c4.R * np.array([1, 1.001, 1, 1])[:, None, None], c4.T), "orthonormal"),
                       ((mirror, np.zeros((2, 3))), "reflection"), ((np.zeros((0, 3, 3)), np.zeros((0, 3))), "no operator"),
                       ((c4.R, c4.T + np.array([[0.0, 0, 0], [np.inf, 0, 0], [0, 0, 0], [0, 0, 0]])), "finite")):
        with pytest.raises(ValueError, match=match):
            jointfit.operators_of("t", bad)
    with pytest.raises(ValueError, match="units x"):
        jointfit.symmetric_refine_numpy(np.zeros((8, 8, 8), np.float32), (0, 0, 0), 1.0, [a] * 17, [np.ones(4)] * 17, c4.R, c4.T, 6.0)
    # the result
    unit = np.arange(12.0).reshape(4, 3)
    fit = jointfit.SymmetricFit(c4, [unit], [unit + 1.0], np.identity(3)[None], np.ones((1, 3)), np.array([True]), np.array([7]), np.ones(2), [None])
    assert isinstance(fit, jointfit.JointFit) and len(fit) == 1 and fit.operators is c4
    im = fit.images(0)
    assert im.shape == (4, 4, 3) and np.array_equal(im[0], fit.coords[0])
    np.testing.assert_allclose(im, c4.copies(unit + 1.0), rtol=0, atol=1e-12)
    assert len(fit.assembly()) == 4 and np.array_equal(fit.assembly()[2], im[2])
    assert fit.write_pdb(str(tmp_path / "x")) == [] and abs(fit.rmsd()[0] - np.sqrt(3.0)) < 1e-12

    class Stub(object):      # a PDB as far as place and write_pdb go
        def __init__(self):
            self.c, self.written = unit.copy(), None

        def get_coords(self):
            return self.c

        def set_coords(self, c):
            self.c = c

        def write_pdb(self, path):
            open(path, "w").write("%r" % (self.c.tolist(),))
    stub = Stub()
    fit = jointfit.SymmetricFit(c4, [unit], [unit + 1.0], np.identity(3)[None], np.ones((1, 3)), np.array([True]), np.array([7]), np.ones(2), [stub])
    names = fit.write_pdb(str(tmp_path / "y"))
    assert [os.path.basename(n) for n in names] == ["y_0_%d.pdb" % g for g in range(4)] and all(os.path.exists(n) for n in names)
    assert eval(open(names[3]).read()) == fit.images(0)[3].tolist() and np.array_equal(stub.c, unit)


def test_header_and_wrapper_carry_the_entry():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_assembly_refine_symmetric\s*\(\s*mad_ctx\s*\*\s*ctx\s*,", text)
    assert _lib.PROTOTYPES["mad_assembly_refine_symmetric"] == ("i", tuple("pippppippdiddppppppp"))
    assert callable(_lib.Lib.assembly_refine_symmetric)
    from mad_amd.Dmap import Dmap
    assert callable(Dmap.refine_symmetric)
    src = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_jointfit.hip")).read()
    assert "k_jf_init_sym" in src and "k_jf_steps_sym" in src
