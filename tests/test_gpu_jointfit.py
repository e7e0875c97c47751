"""The placed bodies of an assembly refined together on the device (mad_assembly_density, mad_assembly_refine: mad_jointfit.hip)
against the numpy restatement of DESIGN.md section 4x in mad_amd/jointfit.py.

Tolerances ("Measured differences"; each is 8 times the worst difference measured over the cases here):
  M_TOL      |M - restated| / max|M|, measured 2.64e-13 (the 63-atom body; max|M| = 23).  The splat accumulates in 2^-36 fixed point:
             each of an atom's 8 contributions is rounded to a multiple of 2^-36, an error of at most 2^-37 = 7.3e-12, so a voxel
             that c contributions reach is off by at most c 2^-37 before the blur, and the blur, a convex combination, does not
             enlarge that.  With c up to about 20 here the bound is 1.5e-10 absolute = 6e-12 of max|M|; the roundings have either
             sign and the blur averages 343 of them, which leaves the 6e-12 absolute that was measured.  The float64 sums on
             either side differ by 1e-16 relative only.
  S_TOL      |s - restated| / |s|, measured 1.32e-13: two sums over 13 440 voxels of M as above, in another order on the device.
  COORD_TOL  final coordinates of a joint run, Angstrom: measured 8.53e-13 (two bodies at 10 A, seed 12).  No float32 rounding of
             a field value flipped in any case; one that does moves a texel by 2^-24 of the map's range and the coordinates by
             about 1e-7 A, so a change of the cases may need this figure measured again.  Every case's restatement margin (the
             smallest |max displacement - step| over its batch decisions, 2.2e-4 A or more) is at least 1000 times 8.53e-13.
  SCALE_TOL  s per round of a joint run, relative: measured 8.13e-14.
"""
import os

import numpy as np
import pytest

from mad_amd import jointfit, synth
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from mad_amd._lib import MadBackendError

import jointfit_cases as jc

pytestmark = pytest.mark.gpu

M_TOL = 8 * 2.64e-13
S_TOL = 8 * 1.32e-13
COORD_TOL = 8 * 8.53e-13
SCALE_TOL = 8 * 8.13e-14
REFINE_PIN = 1e-8      # one body against Lib.refine: the g6 pin of the existing kernel


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


@pytest.fixture
def hooks(lib):
    yield lib
    lib.set_option("jointfit_split", 8)
    lib.set_option("jointfit_registers", 1)


# -- model and scale ---------------------------------------------------------------------------------------------------------
MODEL_SHAPE, MODEL_VS, MODEL_RES, MODEL_ORIGIN = (24, 20, 28), 1.5, 6.0, np.array([4.0, -9.0, 2.5])


def model_bodies():
    """Bodies of 1, 63, 64, 65 and 130 atoms: the single atom on a lattice point; the 63 next to the x = 0 face (its box is
    clipped); a third of the 64 beyond the y face; the 65 and the 130 side by side (their boxes overlap)."""
    rng = np.random.default_rng(11)
    span = MODEL_VS * (np.array(MODEL_SHAPE) - 1)

    def cloud(n, centre, radius):
        return np.asarray(centre) + MODEL_ORIGIN + rng.normal(size=(n, 3)) * radius / 2.0

    one = MODEL_ORIGIN + MODEL_VS * np.array([[12.0, 10.0, 14.0]])
    near_face = cloud(63, [2.5, 0.5 * span[1], 0.3 * span[2]], 4.0)
    beyond = cloud(64, [0.7 * span[0], span[1], 0.5 * span[2]], 4.0)
    beyond[:21, 1] = MODEL_ORIGIN[1] + span[1] + 0.5 + rng.random(21) * 3.0      # a third outside the lattice
    beyond[21:, 1] = np.minimum(beyond[21:, 1], MODEL_ORIGIN[1] + span[1] - 0.25)
    a = cloud(65, [0.45 * span[0], 0.45 * span[1], 0.75 * span[2]], 4.0)
    b = cloud(130, [0.6 * span[0], 0.5 * span[1], 0.65 * span[2]], 5.0)
    bodies = [one, near_face, beyond, a, b]
    masses = [12.0 + 20.0 * rng.random(len(c)) for c in bodies]
    return bodies, masses


def test_model_and_scale_against_the_restatement(lib):
    """M (float64) and s of mad_assembly_density against model_density_numpy within M_TOL and S_TOL (see the module's docstring
    for the arithmetic); the residual is bit-identical to the map wherever M is 0."""
    bodies, masses = model_bodies()
    rng = np.random.default_rng(5)
    grid = rng.random(MODEL_SHAPE, dtype=np.float32)
    lib.upload_density(grid, MODEL_ORIGIN, MODEL_VS)
    worst_m = worst_s = 0.0
    for pick in ([0], [1], [2], [3, 4], [0, 1, 2, 3, 4]):
        bs, ms = [bodies[i] for i in pick], [masses[i] for i in pick]
        M, s, res = lib.assembly_density(bs, ms, MODEL_RES)
        Mr, sr, _ = jointfit.model_density_numpy(grid, MODEL_ORIGIN, MODEL_VS, bs, ms, MODEL_RES)
        dm, ds = np.abs(M - Mr).max() / np.abs(Mr).max(), abs(s - sr) / abs(sr)
        print("bodies %s: max|M| %.4g, |dM| / max|M| = %.3g, s = %.6g, |ds| / |s| = %.3g" % (pick, np.abs(Mr).max(), dm, s, ds))
        worst_m, worst_s = max(worst_m, dm), max(worst_s, ds)
        zero = M == 0
        assert np.array_equal(zero, Mr == 0) and zero.any() and not zero.all()
        assert np.array_equal(res.view(np.uint32)[zero], grid.view(np.uint32)[zero])
        want = (grid.astype(np.float64) - s * M).astype(np.float32)
        assert np.array_equal(res.view(np.uint32), want.view(np.uint32))
    print("worst |dM| / max|M| = %.3g, worst |ds| / |s| = %.3g" % (worst_m, worst_s))
    assert worst_m <= M_TOL and worst_s <= S_TOL
    # the single atom on a lattice point: the outer product of the taps times its mass, up to the splat's fixed point
    M, _, _ = lib.assembly_density([bodies[0]], [masses[0]], MODEL_RES)
    r, taps = jointfit.blur_taps(MODEL_RES, MODEL_VS)
    want = masses[0][0] * taps[:, None, None] * taps[None, :, None] * taps[None, None, :]
    np.testing.assert_allclose(M[12 - r:12 + r + 1, 10 - r:10 + r + 1, 14 - r:14 + r + 1], want, rtol=0, atol=2.0 ** -36)
    assert np.count_nonzero(M) == (2 * r + 1) ** 3


# -- one body is Lib.refine --------------------------------------------------------------------------------------------------
def one_body_case(n):
    shape, vs, origin = (32, 32, 32), 2.0, np.array([10.0, -20.0, 5.0])
    centre = origin + 0.5 * vs * (np.array(shape) - 1)
    ref, _, elems = synth.random_globule(max(n, 40), max(6.0, 1.6 * n ** (1.0 / 3.0)), 100 + n)
    ref = ref - ref.mean(axis=0) + centre
    rho = jointfit.body_density_numpy(shape, origin, vs, ref, synth.masses(elems), 8.0)
    rng = np.random.default_rng(n)
    grid = (rho / rho.max() + rng.normal(0.0, 0.02, shape)).astype(np.float32)
    start = ref[:n] + np.array([2.5, -1.5, 2.0])
    return grid, origin, vs, start


@pytest.mark.parametrize("n, split, registers, plan", [(1, 8, 1, (1, 1, 1)), (64, 8, 1, (1, 1, 1)), (65, 8, 1, (1, 1, 1)), (513, 8, 1, (1, 1, 1)),
                                                       (4097, 8, 1, (2, 1, 2)), (4097, 1, 1, (1, 0, 1)), (4097, 8, 0, (2, 0, 2)), (513, 8, 0, (1, 0, 1))])
def test_one_body_is_lib_refine(hooks, n, split, registers, plan):
    """With one body F is the map: converged and last_step of mad_assembly_refine are mad_refine's and the coordinates agree to the
    pin of the existing kernel, on the register form, the global-memory form and with two workgroups per body."""
    lib = hooks
    grid, origin, vs, start = one_body_case(n)
    lib.upload_density(grid, origin, vs)
    want, wconv, wlast = lib.refine(start, n_steps=200)
    lib.set_option("jointfit_split", split)
    lib.set_option("jointfit_registers", registers)
    coords, R, T, conv, last, scale = lib.assembly_refine([start], [np.full(n, 12.011)], 8.0, n_steps=200)
    assert lib.last_assembly_plan() == plan
    nan = np.isnan(want)      # one atom: its farthest distance is 0, the first rotation's angle infinite, as in refine_pdb
    assert np.array_equal(np.isnan(coords[0]), nan) and nan.any() == (n == 1)
    d = np.abs(coords[0] - want)[~nan].max() if not nan.all() else 0.0
    print("n %d plan %s (mad_refine: %s): converged %s last_step %d, max |d coords| = %.3g, moved %.3f A" % (
        n, plan, lib.last_refine_plan(), conv[0], last[0], d, np.nanmax(np.abs(want - start), initial=0.0)))
    assert (bool(conv[0]), int(last[0])) == (wconv, wlast)
    assert d <= REFINE_PIN
    if not nan.any():
        assert np.abs(want - start).max() > 0.5
        c = start.mean(axis=0)
        np.testing.assert_allclose(np.dot(start - c, R[0]) + c + T[0], coords[0], rtol=0, atol=1e-9)
    assert len(scale) == (int(last[0]) + 4) // 4


# -- joint runs --------------------------------------------------------------------------------------------------------------
def run_scene(lib, scene, n_steps=jc.N_STEPS, without=None, extra=None):
    keep = [b for b in range(len(scene["start"])) if b != without]
    starts, masses = [scene["start"][b] for b in keep], [scene["masses"][b] for b in keep]
    fixed = [scene["fixed"][b] for b in keep] if "fixed" in scene else None
    if extra is not None:
        starts, masses = starts + [extra[0]], masses + [extra[1]]
        fixed = None if fixed is None else fixed + [False]
    lib.upload_density(scene["grid"], jc.ORIGIN, jc.VS)
    return lib.assembly_refine(starts, masses, scene["resolution"], n_steps=n_steps, fixed=fixed)


def hold_to_restatement(got, ref, what):
    coords, R, T, conv, last, scale = got
    print("%s: converged %s / %s, last_step %s / %s, rounds %d / %d, margin %.3g" % (
        what, list(conv), ref["converged"], list(last), ref["last_step"], len(scale), ref["n_rounds"], ref["margin"]))
    assert [bool(c) for c in conv] == ref["converged"] and [int(v) for v in last] == ref["last_step"] and len(scale) == ref["n_rounds"]
    dc = max(np.abs(c - r).max() for c, r in zip(coords, ref["coords"]))
    ds = np.abs(scale / ref["scale"] - 1.0).max() if len(scale) else 0.0
    print("%s: max |d coords| = %.3g A, max |ds| / |s| = %.3g" % (what, dc, ds))
    assert ref["margin"] >= 1000 * COORD_TOL / 8
    assert dc <= COORD_TOL and ds <= SCALE_TOL
    for b in range(len(coords)):
        np.testing.assert_allclose(R[b], ref["R"][b], rtol=0, atol=1e-9)
        np.testing.assert_allclose(T[b], ref["T"][b], rtol=0, atol=1e-9)
    return dc


@pytest.mark.parametrize("key", jc.TWO_BODY_CASES)
def test_two_bodies_against_the_restatement(lib, key):
    """700 + 90 atoms in a 48^3 map: discrete outcomes identical, s per round and coordinates within SCALE_TOL and COORD_TOL."""
    scene = jc.two_body_scene(*key)
    hold_to_restatement(run_scene(lib, scene), jc.restated(key), "two bodies %s" % (key,))


def test_three_bodies_one_fixed(lib):
    """The fixed body's coordinates come back bit for bit; the others' results differ from the run without it; two calls give the
    same bits in every output."""
    scene = jc.three_body_scene()
    got = run_scene(lib, scene)
    hold_to_restatement(got, jc.restated("three"), "three bodies")
    assert np.array_equal(got[0][2].view(np.uint64), np.ascontiguousarray(scene["start"][2]).view(np.uint64))
    assert not got[3][2] and got[4][2] == -1 and np.array_equal(got[1][2], np.identity(3)) and not got[2][2].any()
    pair = run_scene(lib, scene, without=2)
    hold_to_restatement(pair, jc.restated("three", without=2), "three bodies without the fixed one")
    for b in (0, 1):
        moved = np.abs(pair[0][b] - got[0][b]).max()
        print("body %d: with / without the fixed body differ by %.3g A" % (b, moved))
        assert moved > 1e-6
    again = run_scene(lib, scene)
    for a, b in zip(got, again):
        for x, y in zip(a, b) if isinstance(a, list) else [(a, b)]:
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("n_steps", [1, 2, 3, 4, 5, 9])
def test_step_counts(lib, n_steps):
    """An incomplete last batch, and no halving before a complete one."""
    key = jc.TWO_BODY_CASES[2]
    got = run_scene(lib, jc.two_body_scene(*key), n_steps=n_steps)
    hold_to_restatement(got, jc.restated(key, n_steps=n_steps), "n_steps %d" % n_steps)
    assert list(got[4]) == [n_steps - 1] * 2 and len(got[5]) == (n_steps + 3) // 4


def test_a_body_outside_the_map(lib):
    """It takes no translation, halves to convergence and reports what the restatement reports; the others' results are the bits
    of the run without it."""
    key = jc.TWO_BODY_CASES[3]
    scene = jc.two_body_scene(*key)
    far = scene["start"][1] + np.array([900.0, -400.0, 250.0])
    got = run_scene(lib, scene, extra=(far, scene["masses"][1]))
    ref = jointfit.joint_refine_numpy(scene["grid"], jc.ORIGIN, jc.VS, scene["start"] + [far], scene["masses"] + [scene["masses"][1]], scene["resolution"],
                                      n_steps=jc.N_STEPS)
    coords, R, T, conv, last, scale = got
    print("outside body: converged %s last_step %d, moved %.3g A" % (conv[2], last[2], np.abs(coords[2] - far).max()))
    hold_to_restatement(got, ref, "two bodies and one outside")
    assert conv[2] and last[2] == 4 * 6 - 1 and not T[2].any()      # 0.5 halves six times to below 0.01, once per batch
    assert np.abs(coords[2] - far).max() < 0.05
    pair = run_scene(lib, scene)
    for b in (0, 1):
        assert coords[b].tobytes() == pair[0][b].tobytes() and conv[b] == pair[3][b] and last[b] == pair[4][b]
    assert scale[:len(pair[5])].tobytes() == pair[5].tobytes()


# -- the public interface ----------------------------------------------------------------------------------------------------
def test_dmap_methods_round_trip(tmp_path):
    key = jc.TWO_BODY_CASES[2]
    scene = jc.two_body_scene(*key)
    pdbs = []
    for b, c in enumerate(scene["start"]):
        _, names, elems = synth.random_globule(len(c), 18.0 if b == 0 else 8.0, 10 * key[1] + 1 + b)
        path = str(tmp_path / ("body%d.pdb" % b))
        synth.write_pdb(path, np.round(c, 3), names, elems)
        pdbs.append(PDB(path))
    m = dmap(scene["grid"].copy(), jc.ORIGIN, jc.VS)
    fit = m.refine_together(pdbs, scene["resolution"])
    arr = m.refine_together([p.get_coords() for p in pdbs], scene["resolution"], masses=[p.atom_masses() for p in pdbs])
    assert np.array_equal(m.grid3d, scene["grid"]) and len(fit) == 2
    for b in range(2):
        assert fit.coords[b].tobytes() == arr.coords[b].tobytes()
        assert np.array_equal(pdbs[b].get_coords(), np.round(scene["start"][b], 3))      # the structures are not modified
        placed = fit.place(b)
        assert placed is not pdbs[b] and np.array_equal(placed.get_coords(), fit.coords[b])
    assert fit.rmsd()[1] > 1.0 and fit.converged.all() and len(fit.scale) == (fit.last_step.max() + 4) // 4
    names = fit.write_pdb(str(tmp_path / "fit"))
    assert [os.path.basename(n) for n in names] == ["fit_0.pdb", "fit_1.pdb"]
    np.testing.assert_allclose(PDB(names[1]).get_coords(), fit.coords[1], rtol=0, atol=5.1e-4)
    with pytest.raises(ValueError, match="came from an array"):
        arr.place(0)
    one = m.refine_together(pdbs[1], scene["resolution"])      # a single PDB is one body
    assert len(one) == 1
    res = m.residual(pdbs, scene["resolution"])
    res2 = m.residual([p.get_coords() for p in pdbs], scene["resolution"], masses=[p.atom_masses() for p in pdbs])
    assert res.grid3d.tobytes() == res2.grid3d.tobytes() and res.scale == res2.scale and res.scale > 0
    assert res.grid3d.shape == m.grid3d.shape and (res.xi, res.yi, res.zi, res.voxsp) == (m.xi, m.yi, m.zi, m.voxsp)
    Mr, sr, _ = jointfit.model_density_numpy(m.grid3d, jc.ORIGIN, jc.VS, [p.get_coords() for p in pdbs], [p.atom_masses() for p in pdbs], scene["resolution"])
    assert abs(res.scale / sr - 1) <= S_TOL
    np.testing.assert_allclose(res.grid3d, m.grid3d - sr * Mr, rtol=0, atol=2e-7 * np.abs(m.grid3d).max())
    assert np.array_equal(m.grid3d, scene["grid"])


def test_refine_assembly_tool(tmp_path, capsys):
    import importlib.util
    from mad_amd import mapio
    spec = importlib.util.spec_from_file_location("refine_assembly", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "refine_assembly.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    key = jc.TWO_BODY_CASES[2]
    scene = jc.two_body_scene(*key)
    src, res_out, prefix = str(tmp_path / "map.mrc"), str(tmp_path / "residual.mrc"), str(tmp_path / "out")
    mapio.write_volume(src, scene["grid"], tuple(jc.ORIGIN), jc.VS)
    files = []
    for b, c in enumerate(scene["start"]):
        _, names, elems = synth.random_globule(len(c), 18.0 if b == 0 else 8.0, 10 * key[1] + 1 + b)
        files.append(str(tmp_path / ("body%d.pdb" % b)))
        synth.write_pdb(files[-1], np.round(c, 3), names, elems)
    tool.main([src, str(scene["resolution"]), files[0], files[1], "--fixed", "0", "--steps", "40", "--out-prefix", prefix, "--residual", res_out])
    m = Dmap.from_file_as_is(src)      # as the tool reads it
    pdbs = [PDB(f) for f in files]
    fit = m.refine_together(pdbs, scene["resolution"], n_steps=40, fixed=[True, False])
    for b in range(2):
        np.testing.assert_allclose(PDB("%s_%d.pdb" % (prefix, b)).get_coords(), fit.coords[b], rtol=0, atol=5.1e-4)
    assert np.array_equal(fit.coords[0], pdbs[0].get_coords()) and fit.rmsd()[1] > 1.0
    want = m.residual([fit.place(0), fit.place(1)], scene["resolution"])
    assert mapio.read_volume(res_out)[0].tobytes() == want.grid3d.tobytes()
    text = capsys.readouterr().out
    assert "body 0 %s: moved 0.000 A (RMSD), fixed" % files[0] in text and "not converged after step 39" in text and "10 rounds" in text
    with pytest.raises(SystemExit, match="refine_assembly> --fixed 2"):
        tool.main([src, "10", files[0], files[1], "--fixed", "2"])


def test_refusals(lib):
    """Every refusal of the C ABI raises, with the argument named."""
    grid = np.random.default_rng(2).random((16, 16, 16), dtype=np.float32)
    body = np.array([[8.0, 8.0, 8.0], [9.0, 8.0, 8.0]])
    mass = np.array([12.0, 12.0])
    from mad_amd import _lib
    fresh = _lib.Lib(0)
    try:
        with pytest.raises(MadBackendError, match="mad_upload_density"):
            fresh.assembly_refine([body], [mass], 6.0)
        with pytest.raises(MadBackendError, match="mad_upload_density"):
            fresh.assembly_density([body], [mass], 6.0)
    finally:
        fresh.close()
    lib.upload_density(grid, (0.0, 0.0, 0.0), 1.0)
    bad = body.copy()
    bad[1, 2] = np.nan
    for kw, match in ((dict(coords_list=[]), "n_bodies"), (dict(coords_list=[body] * 65, mass_list=[mass] * 65), "n_bodies"),
                      (dict(coords_list=[body, np.zeros((0, 3))], mass_list=[mass, np.zeros(0)]), "empty"),
                      (dict(coords_list=[bad]), "atoms"), (dict(mass_list=[np.array([12.0, np.inf])]), "mass"),
                      (dict(resolution=0.0), "resolution"), (dict(resolution=-3.0), "resolution"), (dict(resolution=1e4), "resolution"),
                      (dict(n_steps=0), "n_steps"), (dict(min_step=0.0), "min_step"), (dict(min_step=0.6), "min_step"),
                      (dict(max_step=np.nan), "max_step")):
        args = dict(coords_list=[body], mass_list=[mass], resolution=6.0)
        args.update(kw)
        if "mass_list" not in kw and "coords_list" in kw:
            args["mass_list"] = [mass] * len(kw["coords_list"])
        with pytest.raises(MadBackendError, match=match):
            lib.assembly_refine(**args)
        if not set(kw) & {"n_steps", "min_step", "max_step"}:
            with pytest.raises(MadBackendError, match=match):
                lib.assembly_density(**args)
    # a NULL pointer where the ABI wants one
    import ctypes as C
    first = np.array([0, 2], np.int64)
    out, rot, tr, cv, ls, nr = np.zeros((2, 3)), np.zeros(9), np.zeros(3), np.zeros(1, np.int32), np.zeros(1, np.int32), C.c_int32(0)
    p = _lib._p
    full = [lib.ctx, 1, p(body), p(mass), p(first), None, 6.0, 10, 0.5, 0.01, p(out), p(rot), p(tr), p(cv), p(ls), None, C.byref(nr)]
    for at, name in ((2, "atoms"), (3, "mass"), (4, "first_atom"), (10, "coords"), (11, "rot"), (12, "trans"), (13, "converged"), (14, "last_step"), (16, "n_rounds")):
        a = list(full)
        a[at] = None
        assert lib.dll.mad_assembly_refine(*a) == _lib.EINVAL and name in lib.last_error()
    s = C.c_double(0)
    assert lib.dll.mad_assembly_density(lib.ctx, 1, p(body), p(mass), p(first), 6.0, None, None, None) == _lib.EINVAL and "scale" in lib.last_error()
    assert lib.dll.mad_assembly_density(lib.ctx, 1, p(body), p(mass), p(first), 6.0, None, C.byref(s), None) == 0 and s.value != 0
    with pytest.raises(ValueError, match="fixed"):
        dmap(grid, (0, 0, 0), 1.0).refine_together([body], 6.0, fixed=[True, False])
    with pytest.raises(ValueError, match="structures"):
        dmap(grid, (0, 0, 0), 1.0).refine_together([np.zeros((4, 2))], 6.0)
    with pytest.raises(ValueError, match="masses"):
        dmap(grid, (0, 0, 0), 1.0).residual([body], 6.0, masses=[np.ones(3)])
