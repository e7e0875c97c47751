"""Asymmetric units refined under a point group on the device (mad_assembly_refine_symmetric: k_jf_init_sym and k_jf_steps_sym of
mad_jointfit.hip) against mad_assembly_refine, bit for bit, where the two must agree, and against the numpy restatement of DESIGN.md
section 4z (jointfit.symmetric_refine_numpy) on the six scenes of symfit_cases.py.

Tolerances ("Measured differences"; each is 8 times the worst |device - restatement| measured over the six
scenes, the rule of test_gpu_jointfit.py):
  SYM_COORD_TOL  final coordinates of the units, Angstrom: measured 2.91e-13 (full64; d2pair 2.70e-13, big2 7.11e-14, ring3 5.68e-14,
                 overhang 4.97e-14, ico 1.42e-14): the sums of a unit's gradients are taken in another order on the device.
  SYM_SCALE_TOL  s per round, relative: measured 2.14e-13 (overhang; ring3 8.54e-14, d2pair 6.00e-14, ico 3.84e-14, full64
                 2.18e-14, big2 1.38e-14).
Every scene's restatement margin (2.69e-3 A or more) is at least 1000 times the measured coordinate difference.  No float32
rounding of a field value flipped in any scene; one that does moves the coordinates by about 1e-7 A (test_gpu_jointfit.py), so a
change of the scenes may need these figures measured again.
"""
import ctypes as C
import os

import numpy as np
import pytest

from mad_amd import _lib, jointfit, symmetry, synth
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from mad_amd._lib import MadBackendError

import jointfit_cases as jc
import symfit_cases as sc
from test_gpu_jointfit import dmap, hooks      # noqa: F401 (hooks is a fixture: it restores the two test hooks)

pytestmark = pytest.mark.gpu

MEASURED_COORD, MEASURED_SCALE = 2.91e-13, 2.14e-13
SYM_COORD_TOL = 8 * MEASURED_COORD
SYM_SCALE_TOL = 8 * MEASURED_SCALE
IDENTITY = (np.identity(3)[None], np.zeros((1, 3)))


@pytest.fixture(scope="module")
def n_cu(lib):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def same_bytes(a, b):
    for x, y in zip(a, b):
        for p, q in zip(x, y) if isinstance(x, list) else [(x, y)]:
            assert p.tobytes() == q.tobytes()


def run_scene(lib, name, **kw):
    s = sc.scene(name)
    lib.upload_density(s["grid"], sc.ORIGIN, sc.VS)
    return lib.assembly_refine_symmetric(s["start"], s["masses"], s["ops"].R, s["ops"].T, s["resolution"], n_steps=s["n_steps"], fixed=s["fixed"], **kw)


# -- one operator is mad_assembly_refine ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split, registers", [(8, 1), (8, 0), (1, 1)])
@pytest.mark.parametrize("key", list(jc.TWO_BODY_CASES) + ["pair"])
def test_one_operator_is_assembly_refine(hooks, n_cu, key, split, registers):
    """K = 1 runs k_jf_init_sym and k_jf_steps_sym (the entry point has no other path) and returns mad_assembly_refine's bytes in
    every output: on the register form, the global-memory form and with one workgroup per body; "pair" has two workgroups a body."""
    lib = hooks
    s = jc.plan_scene(key) if key == "pair" else jc.two_body_scene(*key)
    n_steps = s.get("n_steps", jc.N_STEPS)
    lib.set_option("jointfit_split", split)
    lib.set_option("jointfit_registers", registers)
    lib.upload_density(s["grid"], jc.ORIGIN, jc.VS)
    want = lib.assembly_refine(s["start"], s["masses"], s["resolution"], n_steps=n_steps)
    plan = lib.last_assembly_plan()
    lib.assembly_refine(s["start"][:1], s["masses"][:1], s["resolution"], n_steps=4)      # another plan in between
    assert lib.last_assembly_plan() != plan
    got = lib.assembly_refine_symmetric(s["start"], s["masses"], IDENTITY[0], IDENTITY[1], s["resolution"], n_steps=n_steps)
    print("%s split %d registers %d: plan %s, last_step %s" % (key, split, registers, lib.last_assembly_plan(), list(got[4])))
    assert lib.last_assembly_plan() == plan == sc.expected_plan([len(c) for c in s["start"]], 1, n_cu, split, registers)
    if key == "pair" and split == 8:
        assert plan[0] == 2
    same_bytes(want, got)
    assert max(np.abs(c - c0).max() for c, c0 in zip(got[0], s["start"])) > 0.5


def test_images_outside_the_map_equal_one_operator(lib):
    """ring3's unit under [identity, (R_120, T + 1e4), (R_240, T - 1e4)]: the far images splat nothing and gather nothing, their
    partials are +0, and every output is the K = 1 call's bytes while the K G reduction and the pull-back run."""
    s = sc.scene("ring3")
    R, T = s["ops"].R.copy(), s["ops"].T.copy()
    T[1] += 1e4
    T[2] -= 1e4
    lib.upload_density(s["grid"], sc.ORIGIN, sc.VS)
    one = lib.assembly_refine_symmetric(s["start"], s["masses"], IDENTITY[0], IDENTITY[1], s["resolution"], n_steps=s["n_steps"])
    far = lib.assembly_refine_symmetric(s["start"], s["masses"], R, T, s["resolution"], n_steps=s["n_steps"])
    assert lib.last_assembly_plan()[2] == 3
    same_bytes(one, far)
    near = run_scene(lib, "ring3")
    assert np.abs(near[0][0] - one[0][0]).max() > 1e-6      # the true images do count


# -- against the restatement ----------------------------------------------------------------------------------------------------------
def hold_to_restatement(got, ref, what):
    coords, R, T, conv, last, scale = got
    print("%s: converged %s / %s, last_step %s / %s, rounds %d / %d, margin %.3g" % (
        what, list(conv), ref["converged"], list(last), ref["last_step"], len(scale), ref["n_rounds"], ref["margin"]))
    assert [bool(c) for c in conv] == ref["converged"] and [int(v) for v in last] == ref["last_step"] and len(scale) == ref["n_rounds"]
    dc = max(np.abs(c - r).max() for c, r in zip(coords, ref["coords"]))
    ds = np.abs(scale / ref["scale"] - 1.0).max()
    print("%s: max |d coords| = %.3g A, max |ds| / |s| = %.3g" % (what, dc, ds))
    assert ref["margin"] >= 1000 * MEASURED_COORD
    assert dc <= SYM_COORD_TOL and ds <= SYM_SCALE_TOL
    for u in range(len(coords)):
        np.testing.assert_allclose(R[u], ref["R"][u], rtol=0, atol=1e-9)
        np.testing.assert_allclose(T[u], ref["T"][u], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", sc.SCENES)
def test_against_the_restatement(lib, name):
    """Discrete outcomes identical, s per round and coordinates within SYM_SCALE_TOL and SYM_COORD_TOL, R and T to 1e-9."""
    s = sc.scene(name)
    got = run_scene(lib, name)
    hold_to_restatement(got, sc.restated(name), name)
    moved = [u for u in range(len(s["start"])) if not (s["fixed"] and s["fixed"][u])]
    assert all(jc.rmsd(got[0][u], s["truth"][u]) < jc.rmsd(s["start"][u], s["truth"][u]) for u in moved)
    if name == "overhang":
        out = jc.outside_the_map(s["ops"].copies(got[0][0])[1], s["shape"])
        print("overhang: %d of %d atoms of image 1 do not count" % (out, len(got[0][0])))
        assert 20 <= out <= len(got[0][0]) - 20 and jc.outside_the_map(got[0][0], s["shape"]) == 0


@pytest.mark.parametrize("name", sc.SCENES)
def test_symmetry_kept(name):
    """Through Dmap.refine_symmetric: the images are the unit under the operators, and the assembly read back through
    Dmap.residual gives a finite positive scale; the map is not modified."""
    s = sc.scene(name)
    m = dmap(s["grid"].copy(), sc.ORIGIN, sc.VS)
    fit = m.refine_symmetric(s["start"], s["resolution"], s["ops"], n_steps=s["n_steps"], fixed=s["fixed"], masses=s["masses"])
    K = len(s["ops"])
    assert len(fit) == len(s["start"]) and len(fit.assembly()) == len(fit) * K and np.array_equal(m.grid3d, s["grid"])
    for u in range(len(fit)):
        im = fit.images(u)
        assert im.shape == (K,) + fit.coords[u].shape and np.array_equal(im[0], fit.coords[u])
        for g in range(K):
            np.testing.assert_allclose(im[g], fit.coords[u] @ s["ops"].R[g] + s["ops"].T[g], rtol=0, atol=1e-9)
        np.testing.assert_allclose(im, s["ops"].copies(fit.coords[u]), rtol=0, atol=1e-9)
    res = m.residual(fit.assembly(), s["resolution"], masses=[mm for mm in s["masses"] for _ in range(K)])
    print("%s: scale of the refined assembly %.6g (last round %.6g)" % (name, res.scale, fit.scale[-1]))
    assert np.isfinite(res.scale) and res.scale > 0 and np.isfinite(res.grid3d).all()


def test_fixed_units_and_the_same_bits_every_call(lib):
    """full64's two fixed units come back bit for bit with last_step -1; two calls give the same bytes in every output."""
    s = sc.scene("full64")
    got = run_scene(lib, "full64")
    for u in sc.FULL64_FIXED:
        assert got[0][u].tobytes() == np.ascontiguousarray(s["start"][u]).tobytes()
        assert not got[3][u] and got[4][u] == -1 and np.array_equal(got[1][u], np.identity(3)) and not got[2][u].any()
    assert all(got[4][u] == s["n_steps"] - 1 for u in range(8) if u not in sc.FULL64_FIXED)
    same_bytes(got, run_scene(lib, "full64"))
    first = run_scene(lib, "big2")
    same_bytes(first, run_scene(lib, "big2"))


# -- plans --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, split, registers", [("big2", 8, 1), ("ico", 8, 1), ("full64", 8, 1), ("big2", 1, 1), ("big2", 8, 0)])
def test_plans(hooks, n_cu, name, split, registers):
    lib = hooks
    s = sc.scene(name)
    lib.set_option("jointfit_split", split)
    lib.set_option("jointfit_registers", registers)
    got = run_scene(lib, name)
    plan, want = lib.last_assembly_plan(), sc.expected_plan([len(c) for c in s["start"]], len(s["ops"]), n_cu, split, registers)
    print("%s split %d registers %d: plan %s, restated %s" % (name, split, registers, plan, want))
    assert plan == want
    if (split, registers) == (8, 1):
        assert plan == dict(big2=(2, 1, 4), ico=(1, 1, 60), full64=(1, 1, 64))[name]
    else:      # another plan, the same contract
        hold_to_restatement(got, sc.restated(name), "%s split %d registers %d" % (name, split, registers))


# -- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """Every refusal of the C ABI raises, with the argument named."""
    grid = np.random.default_rng(2).random((16, 16, 16), dtype=np.float32)
    body = np.array([[8.0, 8.0, 8.0], [9.0, 8.0, 8.0]])
    mass = np.array([12.0, 12.0])
    c2 = symmetry.point_group("C2", centre=(8.0, 8.0, 8.0))
    fresh = _lib.Lib(0)
    try:
        with pytest.raises(MadBackendError, match="mad_upload_density"):
            fresh.assembly_refine_symmetric([body], [mass], c2.R, c2.T, 6.0)
    finally:
        fresh.close()
    lib.upload_density(grid, (0.0, 0.0, 0.0), 1.0)
    assert len(lib.assembly_refine_symmetric([body], [mass], c2.R, c2.T, 6.0, n_steps=8)[0]) == 1
    bad = body.copy()
    bad[1, 2] = np.nan
    turned = c2.R[[1, 0]], c2.T[[1, 0]]
    shifted = c2.R.copy(), c2.T + np.array([1e-300, 0.0, 0.0])
    scaled = c2.R * np.array([1.0, 1.0 + 1e-5])[:, None, None], c2.T
    mirror = np.array([np.identity(3), np.diag([1.0, 1.0, -1.0])]), np.zeros((2, 3))
    c5 = symmetry.point_group("C5", centre=(8.0, 8.0, 8.0))
    for kw, match in ((dict(R=turned[0], T=turned[1]), "op_rot.*identity"), (dict(R=shifted[0], T=shifted[1]), "op_trans.*identity"),
                      (dict(R=scaled[0], T=scaled[1]), "op_rot.*orthonormal"), (dict(R=mirror[0], T=mirror[1]), "op_rot.*reflection"),
                      (dict(R=np.zeros((0, 3, 3)), T=np.zeros((0, 3))), "n_ops"),
                      (dict(coords_list=[body] * 13, mass_list=[mass] * 13, R=c5.R, T=c5.T), "n_units x n_ops = 65"),
                      (dict(coords_list=[]), "n_units"), (dict(coords_list=[body] * 65, mass_list=[mass] * 65), "n_units"),
                      (dict(coords_list=[body, np.zeros((0, 3))], mass_list=[mass, np.zeros(0)]), "empty"),
                      (dict(coords_list=[bad]), "atoms"), (dict(mass_list=[np.array([12.0, np.inf])]), "mass"),
                      (dict(resolution=0.0), "resolution"), (dict(resolution=-3.0), "resolution"), (dict(resolution=1e4), "resolution"),
                      (dict(n_steps=0), "n_steps"), (dict(min_step=0.0), "min_step"), (dict(min_step=0.6), "min_step"),
                      (dict(max_step=np.nan), "max_step")):
        args = dict(coords_list=[body], mass_list=[mass], R=c2.R, T=c2.T, resolution=6.0)
        args.update(kw)
        if "mass_list" not in kw and "coords_list" in kw:
            args["mass_list"] = [mass] * len(kw["coords_list"])
        with pytest.raises(MadBackendError, match=match):
            lib.assembly_refine_symmetric(**args)
    # a NULL pointer where the ABI wants one
    first = np.array([0, 2], np.int64)
    out, rot, tr, cv, ls, nr = np.zeros((2, 3)), np.zeros(9), np.zeros(3), np.zeros(1, np.int32), np.zeros(1, np.int32), C.c_int32(0)
    p = _lib._p
    full = [lib.ctx, 1, p(body), p(mass), p(first), None, 2, p(c2.R), p(c2.T), 6.0, 10, 0.5, 0.01, p(out), p(rot), p(tr), p(cv), p(ls), None, C.byref(nr)]
    assert lib.dll.mad_assembly_refine_symmetric(*full) == 0
    for at, name in ((2, "atoms"), (3, "mass"), (4, "first_atom"), (7, "op_rot"), (8, "op_trans"), (13, "coords"), (14, "rot"), (15, "trans"),
                     (16, "converged"), (17, "last_step"), (19, "n_rounds")):
        a = list(full)
        a[at] = None
        assert lib.dll.mad_assembly_refine_symmetric(*a) == _lib.EINVAL and name in lib.last_error()
    m = dmap(grid, (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="fixed"):
        m.refine_symmetric([body], 6.0, c2, fixed=[True, False])
    with pytest.raises(ValueError, match="symmetry"):
        m.refine_symmetric([body], 6.0, "C2")
    with pytest.raises(ValueError, match="reflection"):
        m.refine_symmetric([body], 6.0, mirror)
    with pytest.raises(ValueError, match="65 images"):
        m.refine_symmetric([body] * 13, 6.0, c5)


# -- the public interface ---------------------------------------------------------------------------------------------------------------
def ring3_files(tmp_path):
    s = sc.scene("ring3")
    _, names, elems = synth.random_globule(200, 10.0, 10 * sc.SEEDS["ring3"] + 1)
    path = str(tmp_path / "unit.pdb")
    synth.write_pdb(path, np.round(s["start"][0], 3), names, elems)
    return s, path


def test_dmap_refine_symmetric_round_trip(tmp_path):
    s, path = ring3_files(tmp_path)
    pdb = PDB(path)
    m = dmap(s["grid"].copy(), sc.ORIGIN, sc.VS)
    fit = m.refine_symmetric(pdb, s["resolution"], s["ops"])
    pair = m.refine_symmetric([pdb.get_coords()], s["resolution"], (s["ops"].R, s["ops"].T), masses=[pdb.atom_masses()])
    assert isinstance(fit, jointfit.SymmetricFit) and isinstance(fit, jointfit.JointFit) and len(fit) == 1 and fit.operators is s["ops"]
    assert fit.coords[0].tobytes() == pair.coords[0].tobytes() and np.array_equal(m.grid3d, s["grid"])
    assert np.array_equal(pdb.get_coords(), np.round(s["start"][0], 3))      # the structure is not modified
    assert fit.converged.all() and fit.rmsd()[0] > 1.0 and jc.rmsd(fit.coords[0], s["truth"][0]) < 0.5
    assert np.array_equal(fit.place(0).get_coords(), fit.coords[0])
    names = fit.write_pdb(str(tmp_path / "fit"))
    assert [os.path.basename(n) for n in names] == ["fit_0_0.pdb", "fit_0_1.pdb", "fit_0_2.pdb"]
    for g, n in enumerate(names):
        np.testing.assert_allclose(PDB(n).get_coords(), fit.images(0)[g], rtol=0, atol=5.1e-4)
    assert pair.write_pdb(str(tmp_path / "none")) == []      # units that came from arrays have no PDB to write

    class Found(object):      # what find_symmetry returns has operators()
        def operators(self):
            return s["ops"]
    assert m.refine_symmetric(pdb, s["resolution"], Found()).coords[0].tobytes() == fit.coords[0].tobytes()


def test_refine_assembly_tool_with_a_group(tmp_path, capsys):
    import importlib.util
    from mad_amd import mapio
    spec = importlib.util.spec_from_file_location("refine_assembly", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "refine_assembly.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    s, path = ring3_files(tmp_path)
    src, res_out, prefix = str(tmp_path / "map.mrc"), str(tmp_path / "residual.mrc"), str(tmp_path / "out")
    mapio.write_volume(src, s["grid"], tuple(sc.ORIGIN), sc.VS)
    centre = jc._centre_of(s["shape"])
    tool.main([src, str(s["resolution"]), path, "--steps", "40", "--out-prefix", prefix, "--residual", res_out, "--group", "C3",
               "--axis"] + [repr(float(v)) for v in sc.TILT] + ["--centre"] + [repr(float(v)) for v in centre])
    m = Dmap.from_file_as_is(src)
    pdb = PDB(path)
    fit = m.refine_symmetric(pdb, s["resolution"], symmetry.point_group("C3", axis=sc.TILT, centre=centre), n_steps=40)
    for g in range(3):
        np.testing.assert_allclose(PDB("%s_0_%d.pdb" % (prefix, g)).get_coords(), fit.images(0)[g], rtol=0, atol=5.1e-4)
    want = m.residual(fit.assembly(), s["resolution"], masses=[pdb.atom_masses()] * 3)
    assert mapio.read_volume(res_out)[0].tobytes() == want.grid3d.tobytes()
    text = capsys.readouterr().out
    assert "1 units under C3 (3 images)" in text and "not converged after step 39" in text and "10 rounds" in text
    with pytest.raises(SystemExit, match="--group needs --axis and --centre"):
        tool.main([src, "10", path, "--group", "C3"])
    with pytest.raises(SystemExit, match="go with --group"):
        tool.main([src, "10", path, "--axis", "0", "0", "1"])
