"""mad_assembly_refine (mad_jointfit.hip) where its workgroups wait for one another and its indexing is not trivial: several
workgroups per body with more than one body, bodies of mixed sizes in both orders, up to 8 workgroups per body, 64 bodies, bodies
that stop in different windows of the host's poll, and cubes clipped by the map and shifted against a face.  Every run is held to
the numpy restatement (mad_amd/jointfit.py), which knows nothing of boxes, workgroups or kernel forms, and to the plan restated in
jointfit_cases.expected_plan from the bodies' atom counts, the device's CU count and the two hooks.

Plans covered, bodies x workgroups per body x form (256 CUs):
  pair           4100 + 4112 atoms     2 + 2 registers; 2 + 2 global (jointfit_registers = 0); 1 + 1 global (jointfit_split = 1)
  mixed          4100 + 90             2 + 1 registers; 1 + 1 global, the small body in 1024-thread workgroups (split 1)
  mixed_swapped  90 + 4100             1 + 2 registers (g0 = 1 for the split body, which is body 1); 1 + 1 global (split 1)
  g8             16 400 + 4100         8 + 2 registers; 5 + 2 registers (split 5); 3 + 2 global (split 3)
  g8, body 0     16 400                8 registers, 5 registers, 3 global, each against Lib.refine
  many64         64 x 28 - 33          64 x 1 registers, 4 bodies fixed, 10 rounds
  many16         16 x 28 - 33          16 x 1 registers, 62 rounds, the bodies stop in rounds 11 to 62
  slab           200 + 120             1 + 1 registers, 48 x 48 x 14 map: cubes of 14 voxels on z, one shifted against x = 0

Tolerances ("Measured differences"; each is 8 times the worst difference of its group of cases from the
restatement, measured on the MI355X on 2026-10-21 on top of 33afe56; `converged`, `last_step` and the rounds were identical in every
case).  No float32 rounding of a field value flipped in any of them (that shows as 1e-7 A): the coordinates differ by the order of the
sums over a body's atoms, and s by the splat's 2^-36 fixed point, which the restatement reproduces when it is given that splat:
  COORD_TOL_SPLIT, SCALE_TOL_SPLIT   pair, mixed, mixed_swapped on every plan: 1.56e-13 A (pair, split 8 in global memory), 2.62e-14
  COORD_TOL_G8, SCALE_TOL_G8         g8 at splits 8, 5 and 3: 1.14e-13 A (split 3), 1.51e-14.  The body alone against Lib.refine:
                                     0 at split 8 (the same plan), 5.68e-14 and 7.11e-14 A at 5 and 3, under REFINE_PIN
  COORD_TOL_MANY, SCALE_TOL_MANY     many64: 1.48e-11 A, 3.60e-14; many16: 1.51e-11 A, 7.19e-14.  Bodies of 30 atoms whose gradient sums
                                     nearly cancel: the restatement itself, given the atoms of every body in another order, moves by
                                     8.8e-11 A (many64, body 39; the median body by 5e-14) and 9.0e-12 A (many16, body 0): the
                                     bodies that differ most on the device, where the median body differs by 5.7e-14 and 9.9e-14 A
  COORD_TOL_SLAB, SCALE_TOL_SLAB     slab: 1.42e-14 A, 1.52e-13
Every scene's restatement margin (tests/test_jointfit_restate.py: 1e-4 A or more; the smallest is many16's 2.09e-4) is at least 1000
times its coordinate difference.
"""
import numpy as np
import pytest

import jointfit_cases as jc
from test_gpu_jointfit import REFINE_PIN, hooks      # noqa: F401 (hooks is a fixture: it restores the two test hooks)

pytestmark = pytest.mark.gpu

COORD_TOL_SPLIT, SCALE_TOL_SPLIT = 8 * 1.56e-13, 8 * 2.62e-14
COORD_TOL_G8, SCALE_TOL_G8 = 8 * 1.14e-13, 8 * 1.51e-14
COORD_TOL_MANY, SCALE_TOL_MANY = 8 * 1.51e-11, 8 * 7.19e-14
COORD_TOL_SLAB, SCALE_TOL_SLAB = 8 * 1.42e-14, 8 * 1.52e-13


@pytest.fixture(scope="module")
def n_cu(lib):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run(lib, name, n_cu, split=8, registers=1):
    """The scene refined on the plan the hooks force; the plan the library reports is the restated one."""
    s = jc.plan_scene(name)
    lib.set_option("jointfit_split", split)
    lib.set_option("jointfit_registers", registers)
    lib.upload_density(s["grid"], jc.ORIGIN, jc.VS)
    got = lib.assembly_refine(s["start"], s["masses"], s["resolution"], n_steps=s["n_steps"], fixed=s["fixed"])
    plan, want = lib.last_assembly_plan(), jc.expected_plan([len(c) for c in s["start"]], n_cu, split, registers)
    print("%s split %d registers %d: plan (G of body 0, registers, workgroups) %s, restated %s" % (name, split, registers, plan, want))
    assert plan == want
    return got


def hold(got, ref, what, coord_tol, scale_tol):
    """test_gpu_jointfit.hold_to_restatement with the group's tolerances."""
    coords, R, T, conv, last, scale = got
    print("%s: converged %d / %d of %d, last_step %s / %s, rounds %d / %d, margin %.3g" % (
        what, sum(conv), sum(ref["converged"]), len(conv), sorted(set(int(v) for v in last)), sorted(set(ref["last_step"])), len(scale), ref["n_rounds"],
        ref["margin"]))
    assert [bool(c) for c in conv] == ref["converged"] and [int(v) for v in last] == ref["last_step"] and len(scale) == ref["n_rounds"]
    per_body = [np.abs(c - r).max() for c, r in zip(coords, ref["coords"])]
    dc, ds = max(per_body), np.abs(scale / ref["scale"] - 1.0).max()
    print("%s: max |d coords| = %.3g A (body %d; the median body %.3g), max |ds| / |s| = %.3g" % (what, dc, int(np.argmax(per_body)), np.median(per_body), ds))
    assert ref["margin"] >= 1000 * coord_tol / 8 and ref["margin"] >= 1000 * dc
    assert dc <= coord_tol and ds <= scale_tol
    for b in range(len(coords)):
        np.testing.assert_allclose(R[b], ref["R"][b], rtol=0, atol=1e-9)
        np.testing.assert_allclose(T[b], ref["T"][b], rtol=0, atol=1e-9)


def discrete(got):
    return [bool(c) for c in got[3]], [int(v) for v in got[4]], len(got[5])


def same_bits(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y) if isinstance(x, list) else [(x, y)]:
            assert u.tobytes() == v.tobytes()


def test_two_bodies_of_two_workgroups_each(hooks, n_cu):
    """4100 + 4112 atoms to convergence: b = 1 publishes into its own slots and counts on its own word, g0 = 2 maps blocks 2 and 3 to
    it.  The register form, the same split in global memory, and one workgroup per body (which no longer fits the registers)."""
    ref, seen = jc.restated_plan("pair"), []
    for split, registers in ((8, 1), (8, 0), (1, 1)):
        got = run(hooks, "pair", n_cu, split, registers)
        hold(got, ref, "pair split %d registers %d" % (split, registers), COORD_TOL_SPLIT, SCALE_TOL_SPLIT)
        seen.append(discrete(got))
    assert seen[0] == seen[1] == seen[2] and all(seen[0][0])


@pytest.mark.parametrize("name", ["mixed", "mixed_swapped"])
@pytest.mark.parametrize("split", [8, 1])
def test_mixed_sizes_in_both_orders(hooks, n_cu, name, split):
    """4100 + 90 atoms: G = 2 and 1, so the split body's g0 is not 2 b, and first in one order, second in the other.  With split 1
    the large body takes the small one into the global form, 90 atoms in a workgroup of 1024 threads."""
    got = run(hooks, name, n_cu, split)
    hold(got, jc.restated_plan(name), "%s split %d" % (name, split), COORD_TOL_SPLIT, SCALE_TOL_SPLIT)
    assert all(got[3])


@pytest.mark.parametrize("split", [8, 5, 3])
def test_up_to_eight_workgroups_a_body(hooks, n_cu, split):
    """16 400 + 4100 atoms for 24 steps: 8 + 2, 5 + 2 workgroups in registers, 3 + 2 in global memory."""
    got = run(hooks, "g8", n_cu, split)
    hold(got, jc.restated_plan("g8"), "g8 split %d" % split, COORD_TOL_G8, SCALE_TOL_G8)


@pytest.mark.parametrize("split", [8, 5, 3])
def test_one_large_body_is_lib_refine(hooks, n_cu, split):
    """The 16 400 atoms alone against the same map: F is the map, the result mad_refine's to the pin of the existing kernel."""
    lib, s = hooks, jc.plan_scene("g8")
    start = s["start"][0]
    lib.upload_density(s["grid"], jc.ORIGIN, jc.VS)
    want, wconv, wlast = lib.refine(start, n_steps=200)
    lib.set_option("jointfit_split", split)
    coords, R, T, conv, last, scale = lib.assembly_refine([start], [s["masses"][0]], s["resolution"], n_steps=200)
    plan = lib.last_assembly_plan()
    d = np.abs(coords[0] - want).max()
    print("16 400 atoms split %d: plan %s (mad_refine: %s), converged %s last_step %d, max |d coords| = %.3g A, moved %.3f A" % (
        split, plan, lib.last_refine_plan(), conv[0], last[0], d, np.abs(want - start).max()))
    assert plan == jc.expected_plan([len(start)], n_cu, split) and plan[0] == split
    assert (bool(conv[0]), int(last[0])) == (wconv, wlast) and wconv
    assert d <= REFINE_PIN and np.abs(want - start).max() > 0.5
    assert len(scale) == (int(last[0]) + 4) // 4


def test_sixty_four_bodies(hooks, n_cu):
    """The most bodies the call takes, one workgroup each, four of them fixed, for 40 steps: the 10 rounds cross the host's poll
    after the 8th.  k_jf_accum's tables are full, and the outer sites' cubes are shifted against the map's faces."""
    s, ref = jc.plan_scene("many64"), jc.restated_plan("many64")
    got = run(hooks, "many64", n_cu)
    hold(got, ref, "64 bodies", COORD_TOL_MANY, SCALE_TOL_MANY)
    for b in jc.MANY_FIXED:
        assert got[0][b].tobytes() == np.ascontiguousarray(s["start"][b]).tobytes() and not got[3][b] and got[4][b] == -1
        assert np.array_equal(got[1][b], np.identity(3)) and not got[2][b].any()
    assert len(got[5]) == 10


def test_sixteen_bodies_stop_in_different_polling_windows(hooks, n_cu):
    """To convergence: the bodies leave the count of moving bodies between rounds 11 and 62, the last one runs 21 rounds alone, and
    the rounds enqueued after it stops return at once: s is reported for the 62 rounds that took steps and no more."""
    ref = jc.restated_plan("many16")
    got = run(hooks, "many16", n_cu)
    hold(got, ref, "16 bodies", COORD_TOL_MANY, SCALE_TOL_MANY)
    assert all(got[3]) and len(got[5]) == (int(max(got[4])) + 4) // 4


def test_cubes_at_the_faces(hooks, n_cu):
    """A 48 x 48 x 14 map: both cubes have the map's extent on z; the body at the x = 0 face has atoms beyond it that do not count,
    one-sided texel differences, and a cube shifted against the face and placed again every round.  The call raises nothing: no
    atom inside the map lies outside its body's cube."""
    s, ref = jc.plan_scene("slab"), jc.restated_plan("slab")
    got = run(hooks, "slab", n_cu)
    hold(got, ref, "slab", COORD_TOL_SLAB, SCALE_TOL_SLAB)
    shape = s["grid"].shape
    assert all(got[3]) and jc.outside_the_map(got[0][1], shape) == jc.outside_the_map(ref["coords"][1], shape) > 0


def test_the_same_bits_every_call(hooks, n_cu):
    """pair, mixed and mixed_swapped twice, and a third time after calls that use the same scratch at other sizes (the model of
    another map's bodies, a mad_refine): every output has the same bits."""
    lib, slab = hooks, jc.plan_scene("slab")
    for name in ("pair", "mixed", "mixed_swapped"):
        first = run(lib, name, n_cu)
        same_bits(first, run(lib, name, n_cu))
        lib.upload_density(slab["grid"], jc.ORIGIN, jc.VS)
        M, _, _ = lib.assembly_density(slab["start"], slab["masses"], slab["resolution"])
        assert M.max() > 0
        lib.refine(slab["start"][0], n_steps=20)
        same_bits(first, run(lib, name, n_cu))
