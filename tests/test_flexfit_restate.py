"""The numpy restatement of DESIGN.md section 4za (mad_amd/flexfit.py) on its own: the network against a double loop, the fit against
closed forms, and on the hinge scene flexible fitting is for.  Runs without a GPU."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mad_amd import _lib, flexfit, jointfit

import flexfit_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the network -------------------------------------------------------------------------------------------------------------
def test_network_against_a_double_loop():
    x = np.random.default_rng(3).uniform(-12.0, 14.0, size=(300, 3))
    first, nbr, rest = flexfit.network_numpy(x, 6.0)
    rows, rests = [], []
    for i in range(300):
        row = []
        for j in range(300):
            dx, dy, dz = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1], x[j, 2] - x[i, 2]
            s = (dx * dx + dy * dy) + dz * dz
            if j != i and s <= 6.0 * 6.0:
                row.append(j)
                rests.append(np.sqrt(s))
        rows.append(row)
    assert list(first) == list(np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    assert list(nbr) == [j for r in rows for j in r] and np.array_equal(rest, np.array(rests))
    assert first.dtype == np.int32 and nbr.dtype == np.int32 and rest.dtype == np.float64
    # symmetric: j in the row of i with the same rest length as i in the row of j
    owner = np.repeat(np.arange(300), np.diff(first))
    pairs = {(int(i), int(j)): r for i, j, r in zip(owner, nbr, rest)}
    assert all(pairs[(j, i)] == r for (i, j), r in pairs.items())


def test_a_pair_at_exactly_the_cutoff_is_a_spring_and_an_atom_alone_has_an_empty_row():
    x = np.array([[-3.0, 2.0, 1.0], [3.0, 2.0, 1.0], [3.0, 2.0, 1.0 + 6.0 + 1e-9]])      # on an axis: the sum is exact
    first, nbr, rest = flexfit.network_numpy(x, 6.0)
    assert list(first) == [0, 1, 2, 2] and list(nbr) == [1, 0] and list(rest) == [6.0, 6.0]
    first, nbr, rest = flexfit.network_numpy(x[:1], 6.0)
    assert list(first) == [0, 0] and len(nbr) == 0 == len(rest)


def test_the_degree_cap_is_refused():
    x = np.random.default_rng(6).normal(size=(flexfit.MAX_DEGREE + 2, 3)) * 0.3
    with pytest.raises(ValueError, match="atom 0 has 129 neighbours within cutoff = 6"):
        flexfit.network_numpy(x, 6.0)
    first, _, _ = flexfit.network_numpy(x[:-1], 6.0)
    assert np.all(np.diff(first) == flexfit.MAX_DEGREE)
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert int(re.search(r"^#define MAD_FLEX_MAX_DEGREE (\d+)", text, re.M).group(1)) == flexfit.MAX_DEGREE == _lib.FLEX_MAX_DEGREE
    plan = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_flexfit_plan.h")).read()
    assert int(re.search(r"^#define FX_MAX_DEGREE (\d+)", plan, re.M).group(1)) == flexfit.MAX_DEGREE
    assert int(re.search(r"^#define FX_BATCH (\d+)", plan, re.M).group(1)) == flexfit.BATCH


# -- the fit against closed forms ----------------------------------------------------------------------------------------------
SHAPE, VS, ORIGIN = (20, 20, 20), 2.0, np.array([4.0, -9.0, 2.5])


def ramp(slopes=(0.25, 0.5, -0.125)):
    """A map that rises by slopes[d] per voxel along axis d: every texel is `slopes`, at the faces too."""
    i, j, k = np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(20.0), indexing="ij")
    return (slopes[0] * i + slopes[1] * j + slopes[2] * k).astype(np.float32)


def test_on_a_linear_ramp_every_atom_takes_the_same_step_and_no_spring_is_strained():
    """The ramp runs along x and the atoms stand on multiples of 1/4 A, so every weight of the gather, every force (1, 0, 0) and every
    step of 0.5 A is exact: the springs keep their lengths to the bit and strain() is exactly 0."""
    x = ORIGIN + 0.25 * np.random.default_rng(1).integers(32, 56, size=(40, 3))
    x = np.unique(x, axis=0)
    net = flexfit.network_numpy(x, 5.0)
    assert len(net[1]) > 100
    out = flexfit.flex_fit_numpy(ramp((0.25, 0.0, 0.0)), ORIGIN, VS, x, net, stiffness=3.0, n_steps=6, max_step=0.5, min_step=0.01)
    assert np.array_equal(out["coords"], x + np.array([3.0, 0.0, 0.0]))
    assert out["g0"] == 0.25 and not out["converged"] and out["last_step"] == 5 and out["step"] == 0.5 and out["margin"] == 1.5
    fit = flexfit.FlexFit(x, out["coords"], out["converged"], out["last_step"], out["step"], out["g0"], net, np.array([0, len(x)]), [None])
    assert fit.strain() == 0.0 and np.all(fit.displacement() == 3.0)
    # a ramp in a general direction: the same force for every atom at the first step, to rounding
    tex = np.moveaxis(np.array(np.gradient(ramp())), 0, -1)
    F = flexfit.forces_numpy(tex, ORIGIN, VS, x + 0.1, np.ones(len(x)), 0.5, flexfit.network_numpy(x + 0.1, 5.0), 1.0)
    np.testing.assert_allclose(F, np.tile(np.array([0.25, 0.5, -0.125]) / 0.5, (len(x), 1)), rtol=0, atol=1e-14)


def test_stiffness_0_with_one_atom_is_gradient_ascent_on_the_gather():
    grid = fc.scene("mini", 1)["grid"]
    tex = np.moveaxis(np.array(np.gradient(grid)), 0, -1)
    x = (fc.ORIGIN + fc.VS * np.array([[14.3, 15.1, 16.7]]))
    net = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0))
    out = flexfit.flex_fit_numpy(grid, fc.ORIGIN, fc.VS, x, net, stiffness=0.0, n_steps=7, max_step=0.25, min_step=0.01)
    p, step, prev, batch = x.copy(), 0.25, x.copy(), 0
    g0 = None
    for s in range(7):
        g = jointfit._gather(tex, fc.ORIGIN, fc.VS, p)
        if g0 is None:
            g0 = float(np.sqrt(((g[0, 0] * g[0, 0] + g[0, 1] * g[0, 1]) + g[0, 2] * g[0, 2]) / 1.0))
        F = g / g0
        m = float(np.sqrt((F[0, 0] * F[0, 0] + F[0, 1] * F[0, 1]) + F[0, 2] * F[0, 2]))
        p = p + F * (step / m)
        batch += 1
        if batch == 4:
            if np.linalg.norm(p - prev) < step:
                step *= 0.5
            batch, prev = 0, p.copy()
    assert np.array_equal(out["coords"], p) and out["g0"] == g0 and out["step"] == step
    # every step is one step size long
    assert abs(np.linalg.norm(flexfit.flex_fit_numpy(grid, fc.ORIGIN, fc.VS, x, net, stiffness=0.0, n_steps=1)["coords"] - x) - 0.5) < 1e-12


def test_fixed_atoms_keep_their_bits_and_still_hold_their_neighbours():
    s, kw, net = fc.variant("fixed")
    out = fc.restated_variant("fixed")
    fx = kw["fixed"]
    assert np.array_equal(out["coords"][fx].view(np.uint64), s["start"][fx].view(np.uint64))
    assert np.any(out["coords"][~fx] != s["start"][~fx])
    free = fc.restated_variant("plain")
    assert np.any(free["coords"][fx] != s["start"][fx])


@pytest.mark.parametrize("n_steps", range(1, 10))
def test_runs_of_1_to_9_steps_end_at_the_right_batch_boundaries(n_steps):
    """A step size so large that the first look halves it: looks come after steps 3 and 7 and nowhere else."""
    s = fc.scene("mini", 1)
    x = s["start"][:1]
    net = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0))
    # the atom circles its density peak: in 4 steps of 8 A it ends less than 8 A from where it began
    out = flexfit.flex_fit_numpy(s["grid"], fc.ORIGIN, fc.VS, x, net, n_steps=n_steps, max_step=8.0, min_step=3.0)
    long_run = flexfit.flex_fit_numpy(s["grid"], fc.ORIGIN, fc.VS, x, net, n_steps=40, max_step=8.0, min_step=3.0)
    assert long_run["converged"] and long_run["last_step"] % 4 == 3      # convergence is seen at a look, never between two
    if n_steps > long_run["last_step"]:
        assert (out["converged"], out["last_step"], out["step"]) == (True, long_run["last_step"], long_run["step"])
        assert np.array_equal(out["coords"], long_run["coords"])
    else:
        looks = n_steps // 4
        assert not out["converged"] and out["last_step"] == n_steps - 1
        assert out["step"] in [8.0 * 0.5 ** k for k in range(looks + 1)]
        assert (out["margin"] == np.inf) == (looks == 0)
    plain = fc.restated_case(("mini", "plain"), n_steps)
    assert (plain["converged"], plain["last_step"], plain["step"]) == (False, n_steps - 1, 0.5) and (plain["margin"] == np.inf) == (n_steps < 4)


def test_a_run_ends_when_no_atom_feels_a_force_and_is_refused_when_none_feels_the_map():
    x = ORIGIN + np.array([[10.0, 10.0, 10.0], [13.0, 10.0, 10.0]])
    net = flexfit.network_numpy(x, 5.0)
    with pytest.raises(ValueError, match="no atom feels the map"):
        flexfit.flex_fit_numpy(np.ones(SHAPE, np.float32), ORIGIN, VS, x, net)
    # both atoms fixed: F = 0 for all, the run ends converged at step 0
    out = flexfit.flex_fit_numpy(ramp(), ORIGIN, VS, x, net, fixed=[True, True])
    assert out["converged"] and out["last_step"] == 0 and np.array_equal(out["coords"], x)
    # an atom outside the map feels its spring alone
    far = ORIGIN + np.array([[10.0, 10.0, 10.0], [-1.0, 10.0, 10.0]])
    net = (np.array([0, 0, 1], np.int32), np.array([0], np.int32), np.array([9.0]))
    out = flexfit.flex_fit_numpy(ramp(), ORIGIN, VS, far, net, n_steps=1, fixed=[True, False])
    assert np.array_equal(out["coords"][0], far[0]) and out["coords"][1, 0] > far[1, 0] and np.array_equal(out["coords"][1, 1:], far[1, 1:])


# -- the hinge scene -----------------------------------------------------------------------------------------------------------
def test_the_hinge_scene_ends_within_a_quarter_of_the_start_rmsd():
    """Two balls of 150 atoms and 8 linker atoms, the second ball turned 25 degrees, 8 A, 2 A per voxel, 36^3, noise 0.02, cutoff 6,
    stiffness 1.  Per seed: the final RMSD to the truth is at most a quarter of the start's and strain() is below 0.15 A; at least
    3 of the 4 seeds of flexfit_cases.HINGE_SEEDS must pass.  Restated figures (start -> end RMSD in A, strain in A, last step):
    seed 1: 4.28 -> 0.270, 0.105, 403; seed 2: 4.33 -> 0.208, 0.101, 339; seed 3: 4.38 -> 0.301, 0.098, 351; seed 4: 4.32 -> 0.251,
    0.098, 255.  All four pass."""
    passed = 0
    for seed in fc.HINGE_SEEDS:
        s, net, out = fc.scene("hinge", seed), fc.network("hinge", seed), fc.restated("hinge", seed)
        start, end = fc.rmsd(s["start"], s["truth"]), fc.rmsd(out["coords"], s["truth"])
        fit = flexfit.FlexFit(s["start"], out["coords"], out["converged"], out["last_step"], out["step"], out["g0"], net, np.array([0, len(s["start"])]), [None])
        print("seed %d: %.3f -> %.3f A, strain %.3f A, converged %s at step %d" % (seed, start, end, fit.strain(), out["converged"], out["last_step"]))
        assert fit.strain() == fc.strain(out["coords"], net) and fit.rmsd(s["truth"]) == end
        passed += end <= 0.25 * start and fit.strain() < 0.15
    assert passed >= 3


def test_the_flexible_result_is_closer_than_the_rigid_one():
    """The same scene through refine_pdb's restatement (jointfit.joint_refine_numpy with one body): seed 1 ends 1.372 A from the
    truth as a rigid body and 0.270 A on the elastic network."""
    s = fc.scene("hinge", fc.HINGE_SEEDS[0])
    rigid = jointfit.joint_refine_numpy(s["grid"], fc.ORIGIN, fc.VS, [s["start"]], [np.full(len(s["start"]), fc.CARBON)], s["resolution"], n_steps=fc.N_STEPS)
    flexible = fc.restated("hinge", fc.HINGE_SEEDS[0])
    print("rigid %.3f A, flexible %.3f A" % (fc.rmsd(rigid["coords"][0], s["truth"]), fc.rmsd(flexible["coords"], s["truth"])))
    assert fc.rmsd(flexible["coords"], s["truth"]) < fc.rmsd(rigid["coords"][0], s["truth"])


@pytest.mark.parametrize("key", fc.GPU_CASES, ids=lambda k: "%s_%s" % k)
def test_the_device_cases_were_chosen_by_their_margin(key):
    """Every case tests/test_gpu_flexfit.py runs to the end: no batch decision closer than 1e-4 A to its threshold."""
    assert fc.restated_case(key)["margin"] >= 1e-4


# -- the layers ----------------------------------------------------------------------------------------------------------------
def test_the_host_plan_under_the_sanitizers(tmp_path):
    """make check-flexfit-plan: mad_flexfit_plan.h in a stand-alone program under AddressSanitizer and UBSan."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mad_amd", "csrc"), "check-flexfit-plan", "BUILD=%s" % tmp_path],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0 and "check_flexfit_plan: ok" in out.stdout, out.stdout


def test_header_wrapper_and_makefile_carry_the_entries():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    for name in ("mad_flex_network", "mad_flex_fit", "mad_last_flex_plan"):
        assert re.search(r"\bint\s+%s\s*\(\s*mad_ctx\s*\*\s*ctx\s*," % name, text) and name in _lib.PROTOTYPES
    assert callable(_lib.Lib.flex_network) and callable(_lib.Lib.flex_fit) and callable(_lib.Lib.last_flex_plan)
    mk = open(os.path.join(ROOT, "mad_amd", "csrc", "Makefile")).read()
    assert "mad_flexfit.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "mad_flexfit_plan.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^check-flexfit-plan:", mk, re.M) and not re.search(r"^all:.*check-flexfit-plan", mk, re.M)
    names = re.search(r"k_timer_names\[MAD_T_COUNT\]\s*=\s*\{(.*?)\}", open(os.path.join(ROOT, "mad_amd", "csrc", "mad_ctx.hip")).read(), re.S).group(1)
    assert all(n in re.findall(r'"([a-z0-9_]+)"', names) for n in ("flex_network", "flex_steps"))
    src = inspect.getsource(flexfit)
    assert not re.search(r"^\s*(import|from)\s+(scipy|oracle)", src, re.M)      # the restatement is numpy alone
    kernels = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_flexfit.hip")).read()
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", kernels) and "fma(" not in kernels      # integer atomics only


def test_arguments_of_the_python_side():
    a, b = np.zeros((4, 3)), np.ones((2, 3))
    coords, first, src = flexfit.atoms_of("t", [a, b])
    assert coords.shape == (6, 3) and list(first) == [0, 4, 6] and src == [None, None]
    assert flexfit.atoms_of("t", a)[0].shape == (4, 3)
    for bad in ([], [np.zeros((3, 2))], [np.zeros((0, 3))], "x"):
        with pytest.raises(ValueError, match="structure"):
            flexfit.atoms_of("t", bad)
    ok = dict(cutoff=6.0, stiffness=1.0, n_steps=10, max_step=0.5, min_step=0.01)
    flexfit.check_steps("t", **ok)
    flexfit.check_steps("t", **dict(ok, stiffness=0.0, min_step=0.5))
    for key, value in (("cutoff", 0.0), ("cutoff", -1.0), ("cutoff", np.nan), ("stiffness", -1e-9), ("stiffness", np.inf), ("n_steps", 0),
                       ("n_steps", 2.5), ("min_step", 0.0), ("min_step", 0.6), ("max_step", np.inf)):
        with pytest.raises(ValueError, match="steps" if key in ("min_step", "max_step") else key):
            flexfit.check_steps("t", **dict(ok, **{key: value}))
    first, nbr, rest = np.array([0, 2, 3, 3, 4]), np.array([1, 3, 0, 0]), np.array([1.5, 2.0, 1.5, 2.0])
    got = flexfit.check_network("t", 4, (first, nbr, rest))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and list(got[0]) == list(first)

    def changed(which, i, v):
        arrays = [first.copy(), nbr.copy(), rest.copy()]
        arrays[which][i] = v
        return tuple(arrays)

    for net in (changed(0, 0, 1), changed(0, 2, 1), changed(1, 0, 4), changed(1, 1, -1), changed(1, 2, 1), changed(1, 0, 3), changed(2, 3, 0.0),
                changed(2, 0, np.nan), (first[:-1], nbr, rest), (first, nbr[:-1], rest), (first, nbr), None):
        if net is None:
            continue
        with pytest.raises(ValueError, match="network"):
            flexfit.check_network("t", 4, net)
    fit = flexfit.FlexFit(a, a + 1.0, True, 7, 0.0078125, 0.2, (np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0)), np.array([0, 4]), [None])
    assert len(fit) == 1 and abs(fit.rmsd() - np.sqrt(3.0)) < 1e-15 and fit.strain() == 0.0 and fit.write_pdb("unused") == []
    assert np.allclose(fit.displacement(), np.sqrt(3.0)) and fit.rmsd(a + 1.0) == 0.0
    with pytest.raises(ValueError, match="array"):
        fit.place()
    with pytest.raises(ValueError, match="shape"):
        fit.rmsd(b)


def test_dmap_flex_fit_checks_its_arguments_before_the_device_is_touched():
    from mad_amd.Dmap import Dmap
    d = Dmap.__new__(Dmap)
    d.grid3d, d.voxsp, d.xi, d.yi, d.zi = np.zeros((8, 8, 8), np.float32), 2.0, 0.0, 0.0, 0.0
    x = np.random.default_rng(0).uniform(2.0, 10.0, size=(5, 3))
    for kw, match in ((dict(cutoff=0.0), "cutoff"), (dict(stiffness=-1.0), "stiffness"), (dict(n_steps=0), "n_steps"), (dict(min_step=1.0), "steps"),
                      (dict(weights=np.ones(4)), "weights"), (dict(weights=[1, 1, np.nan, 1, 1]), "weights"), (dict(fixed=[True]), "fixed"),
                      (dict(network=(np.zeros(3, np.int32), [], [])), "network")):
        with pytest.raises(ValueError, match=match):
            d.flex_fit(x, **kw)
    bad = x.copy()
    bad[2, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        d.flex_fit(bad)
    with pytest.raises(ValueError, match="structure"):
        d.flex_fit([])
