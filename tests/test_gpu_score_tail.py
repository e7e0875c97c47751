"""The tail of the pipeline on the device -- refinement (a13), density simulation (a14-a15), CCC (a16) -- on every code path the
sizing rules of mad_refine.hip can choose, against the CPU oracle and against the reference's own outputs on the edges
(tests/golden/g24_score_tail.npz, made by tests/golden/make_golden_g24.py; tests/test_score_tail_golden.py holds the oracle to it).

Refinement: `refine_device` splits a candidate over G workgroups (G = min(8, CUs / candidates), lowered while a workgroup would hold
fewer than 2048 atoms) and keeps the atoms in registers (k_refine<8>) when a thread holds at most 8, otherwise walks them in global
memory (k_refine<0>).  Every test here asserts the plan (G, in_registers) it was written for through `Lib.last_refine_plan()`, so a
change of the sizing rule fails loudly; the last refinement test checks that the module has run G = 1..8 in the register form and
G = 1, 2, 3, 8 in the global form, and prints per plan the largest device-oracle difference next to the oracle's own spread under a
permutation of the atoms (DESIGN.md section 2 keeps that table).

Tolerances are DESIGN.md section 2's: converged / last_step identical, coordinates within 1e-8 A after at most 8 steps and 1e-6 A after
up to 500; density 2e-7; CCC 1e-9 against the oracle on the same grids, 1e-5 relative against the reference (float32 sums) and
through the resident path.  A refinement case is admitted only if the oracle itself gives the same (converged, last_step) and the
same step sizes for the atoms in their order and in a seeded permutation (`_oracle`), so that "identical last_step" is a fair
demand; a case that fails it is a bad seed, to be replaced, never skipped.
"""
import os

import numpy as np
import pytest

from mad_amd import synth
from mad_amd._lib import MadBackendError
from mad_amd.math_utils import euler_rod_mat
from oracle import oracle as O

pytestmark = pytest.mark.gpu

G24 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_score_tail.npz")
AXIS = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
REG, GLOBAL = 1, 0

PLANS = {}      # (G, in_registers) -> [largest device-oracle difference, the oracle's permutation spread of that case, cases]


@pytest.fixture(scope="module")
def g24():
    with np.load(G24, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def n_cu(lib):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def base():
    """One large globule; a case of n atoms takes n of them spread evenly over it, so every case sits in the same maps."""
    coords, _, elems = synth.random_globule(33000, 36.0, 3)
    return coords, synth.masses(elems), {}


def _atoms(base, n):
    return np.ascontiguousarray(base[0][np.linspace(0, len(base[0]) - 1, n).astype(np.int64)])


def _map(base, vs, off=0.0, pad=8):
    """(grid, origin, vs): the globule's simulated density, zero-padded, its origin moved by `off` A off the voxel lattice (the
    atoms keep their place)."""
    key = (vs, off, pad)
    if key not in base[2]:
        grid, x0, y0, z0 = O.structure_to_density(base[0], base[1], 8.0, vs)
        base[2][key] = (np.pad(grid, pad), np.array([x0, y0, z0]) - pad * vs + off, vs)
    return base[2][key]


def _cut_map(base):
    """The globule's density at voxel 1.5 cut through the structure: every face of the map lies in the density."""
    key = "cut"
    if key not in base[2]:
        grid, x0, y0, z0 = O.structure_to_density(base[0], base[1], 8.0, 1.5)
        lo, n = (12, 11, 13), (36, 38, 35)
        cut = np.ascontiguousarray(grid[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]])
        assert all(np.abs(cut.take(i, axis=d)).max() > 0.1 for d in range(3) for i in (0, -1))
        base[2][key] = (cut, np.array([x0, y0, z0]) + np.array(lo) * 1.5, 1.5)
    return base[2][key]


def _pose(atoms, ang, shift):
    c = atoms.mean(0)
    return (atoms - c) @ euler_rod_mat(AXIS, ang) + c + np.asarray(shift, np.float64)


def _cands_for(n_cu, G):
    """The fewest candidates that hold the split at G workgroups each: G = min(8, CUs / candidates)."""
    n = n_cu // (G + 1) + 1
    assert n_cu // n == G, "no candidate count gives G = %d on %d CUs" % (G, n_cu)
    return n


def _oracle(m, start, n_steps, lim):
    """The oracle's run of one start and its spread under a seeded permutation of the atoms; refuses a knife-edge case."""
    grid, origin, vs = m
    ref, conv, last, tr = O.refine(grid, origin, vs, start, n_steps=n_steps, max_step=lim[0], min_step=lim[1], want_trace=True)
    perm = np.random.default_rng(len(start) + 7 * n_steps).permutation(len(start))
    ref2, conv2, last2, tr2 = O.refine(grid, origin, vs, start[perm], n_steps=n_steps, max_step=lim[0], min_step=lim[1], want_trace=True)
    assert (conv, last) == (conv2, last2) and np.array_equal(tr[:, 12], tr2[:, 12], equal_nan=True), \
        "knife-edge case (the oracle's own trajectory depends on the order of its sums): pick another seed"
    back = np.empty_like(ref2)
    back[perm] = ref2
    fin = np.isfinite(ref).all(1) & np.isfinite(back).all(1)
    return ref, conv, last, float(np.abs(ref[fin] - back[fin]).max()) if fin.any() else 0.0


def _run(lib, m, starts, n_steps, lim, plan, distinct=None, label=""):
    """Refine `starts` ((n_cand, n, 3)) in map `m`, assert the plan, compare every distinct start with the oracle and its copies with
    each other bit for bit; with G > 1 the whole batch again, bit-identical.  distinct[i] = the first candidate equal to i."""
    starts = np.ascontiguousarray(starts, np.float64)
    distinct = list(range(len(starts))) if distinct is None else list(distinct)
    lib.upload_density(*m)
    got, conv, last = lib.refine(starts, n_steps=n_steps, max_step=lim[0], min_step=lim[1])
    assert lib.last_refine_plan() == plan, (label, lib.last_refine_plan(), plan)
    tol = 1e-8 if n_steps <= 8 else 1e-6
    worst, spread = 0.0, 0.0
    for i in sorted(set(distinct)):
        ref, rconv, rlast, sp = _oracle(m, starts[i], n_steps, lim)
        assert (bool(conv[i]), int(last[i])) == (rconv, rlast), (label, i, bool(conv[i]), int(last[i]), rconv, rlast)
        d = float(np.abs(got[i] - ref).max())
        print("refine %-28s plan %s cand %3d n %6d steps %3d last %3d: device-oracle %.2e A, oracle permuted %.2e A" %
              (label, plan, i, starts.shape[1], n_steps, rlast, d, sp))
        np.testing.assert_allclose(got[i], ref, rtol=0, atol=tol, err_msg=str((label, i)))
        if d >= worst:
            worst, spread = d, sp
    for i, j in enumerate(distinct):
        if i != j:
            assert (conv[i], last[i]) == (conv[j], last[j]) and np.array_equal(got[i], got[j]), (label, "copies differ", i, j)
    if plan[0] > 1:
        again, conv2, last2 = lib.refine(starts, n_steps=n_steps, max_step=lim[0], min_step=lim[1])
        assert np.array_equal(again, got) and np.array_equal(conv2, conv) and np.array_equal(last2, last), (label, "run to run")
    rec = PLANS.setdefault(plan, [0.0, 0.0, 0])
    if n_steps > 8 and worst >= rec[0]:
        rec[0], rec[1] = worst, spread
    rec[2] += 1
    return got, conv, last


# ---------------------------------------------------------------------------------------------------------------------
# refinement over the plan matrix
# ---------------------------------------------------------------------------------------------------------------------

def test_refine_register_form_at_every_split(lib, base, n_cu):
    """One candidate of exactly 2048 G atoms runs in G workgroups, one atom fewer in G - 1: G = 1..8, registers.  The voxel size,
    the origin's place on the lattice and the step limits change from case to case."""
    assert n_cu >= 8
    maps = (_map(base, 1.5), _map(base, 1.2, 0.37), _map(base, 0.7, 0.123))
    lims = ((1.0, 0.1), (0.5, 0.01), (0.25, 0.001))
    k = 0
    for G in range(1, 9):
        for n, want in ((2048 * G, G), (2048 * G - 1, G - 1)):
            if want == 0:
                continue
            atoms = _atoms(base, n)
            start = _pose(atoms, 0.05 + 0.01 * G, (1.0, -0.8, 0.5))
            _run(lib, maps[k % 3], start[None], 500, lims[(k // 3) % 3], (want, REG), label="split n=%d" % n)
            k += 1


def test_refine_tier_boundary(lib, base, n_cu):
    """4096 G atoms fill the eighth register slot of every thread; one more atom goes to the global-memory form.  At G = 8 (one
    candidate) and at G = 3 (held there by the number of candidates)."""
    m = _map(base, 1.5)
    for n, plan in ((4096 * 8, (8, REG)), (4096 * 8 + 1, (8, GLOBAL))):
        start = _pose(_atoms(base, n), 0.1, (1.0, -0.8, 0.5))
        _run(lib, m, start[None], 500, (1.0, 0.1), plan, label="tier n=%d" % n)
    nc = _cands_for(n_cu, 3)
    for n, plan in ((4096 * 3, (3, REG)), (4096 * 3 + 1, (3, GLOBAL))):
        atoms = _atoms(base, n)
        kinds = [_pose(atoms, 0.1, (1.0, -0.8, 0.5)), _pose(atoms, 0.06, (-1.2, 0.4, 0.9)), _pose(atoms, 0.02, (55.0, 50.0, 45.0))]
        distinct = [i % 3 for i in range(nc)]
        _run(lib, m, np.stack([kinds[d] for d in distinct]), 500, (0.5, 0.01), plan, distinct, label="tier n=%d x %d" % (n, nc))


@pytest.mark.parametrize("G", [1, 2, 7])
def test_refine_global_form_many_candidates(lib, base, n_cu, G):
    """The global-memory form at the splits that only a large batch reaches (G = 3 and 8: test_refine_tier_boundary): just over 4096 G
    atoms per candidate, five distinct starts repeated -- two near the planted pose, one mostly outside the map, one entirely outside,
    one far off in angle -- whose copies must come back bit-identical; also with step counts that stop inside a batch of four."""
    nc = _cands_for(n_cu, G)
    n = 4096 * G + 4 + G
    atoms = _atoms(base, n)
    kinds = [_pose(atoms, 0.1, (1.0, -0.8, 0.5)), _pose(atoms, 0.05, (-0.9, 1.1, 0.3)), _pose(atoms, 0.02, (60.0, 55.0, 50.0)),
             _pose(atoms, 0.0, (400.0, 0.0, 0.0)), _pose(atoms, 0.3, (2.5, 2.0, -3.0))]
    distinct = [i % 5 for i in range(nc)]
    starts = np.stack([kinds[d] for d in distinct])
    m = _map(base, 1.5) if G != 2 else _map(base, 1.2, 0.37)
    _run(lib, m, starts, 500, (1.0, 0.1) if G != 2 else (0.5, 0.01), (G, GLOBAL), distinct, label="global G=%d x %d" % (G, nc))
    for n_steps in (1, 2, 3, 5, 7):
        _run(lib, m, starts, n_steps, (0.5, 0.01), (G, GLOBAL), distinct, label="global G=%d steps=%d" % (G, n_steps))


@pytest.mark.parametrize("vs,off", [(1.2, 0.37), (0.7, 0.123)])
def test_refine_other_voxels_limits_and_step_counts(lib, base, vs, off):
    """Voxel sizes whose lattice points are not exact in binary, the map's origin off that lattice (the kernel's grid-point search
    then differs from a plain floor), the reference's default step limits and a finer pair, step counts that end inside a batch."""
    m = _map(base, vs, off)
    for n, plan in ((700, (1, REG)), (5000, (2, REG))):
        start = _pose(_atoms(base, n), 0.12, (1.0, -0.8, 0.5))
        for n_steps in (1, 2, 3, 5, 7):
            _run(lib, m, start[None], n_steps, (0.5, 0.01), plan, label="vs=%.1f n=%d" % (vs, n))
        for lim in ((0.5, 0.01), (0.25, 0.001)):
            _run(lib, m, start[None], 500, lim, plan, label="vs=%.1f n=%d lim=%s" % (vs, n, lim))


@pytest.mark.parametrize("vs", [1.5, 1.2])
def test_refine_long_chain(lib, n_cu, vs):
    """Hundreds of dependent steps, hence of hand-offs between the workgroups of a candidate: a start 20 A and 0.5 rad away with small
    steps.  Register form at G = 4, global form at G = 2 (a batch)."""
    coords, _, elems = synth.random_globule(9000, 30.0, 6)
    grid, x0, y0, z0 = O.structure_to_density(coords, synth.masses(elems), 8.0, vs)
    m = (np.pad(grid, 14), np.array([x0, y0, z0]) - 14 * vs, vs)
    start = _pose(coords, 0.5, 20.0 * np.array([0.6, -0.64, 0.48]))
    lim = (0.25, 0.001)
    _, rconv, rlast, _ = O.refine(*m, start, n_steps=500, max_step=lim[0], min_step=lim[1])
    assert rlast >= 300, rlast      # the case must stay long
    got, _, _ = _run(lib, m, start[None], 500, lim, (4, REG), label="long vs=%.1f" % vs)
    assert np.sqrt(((got[0] - coords) ** 2).sum(1).mean()) < 0.05
    nc = _cands_for(n_cu, 2)
    other = _pose(coords, 0.45, 18.0 * np.array([0.6, -0.64, 0.48]))
    distinct = [i % 2 for i in range(nc)]
    _run(lib, m, np.stack([(start, other)[d] for d in distinct]), 500, lim, (2, GLOBAL), distinct, label="long vs=%.1f x %d" % (vs, nc))


def test_refine_degenerate_inputs(lib, base):
    """A flat map, one atom, atoms exactly on the planes of the strict inside test, and a NaN coordinate in one candidate of a batch,
    in one workgroup and split over two."""
    m = _map(base, 1.5)
    grid, origin, vs = m
    flat = (np.zeros_like(grid), origin, vs)
    for n, plan in ((600, (1, REG)), (5000, (2, REG))):
        atoms = _atoms(base, n)
        start = _pose(atoms, 0.1, (1.0, -0.8, 0.5))
        got, conv, last = _run(lib, flat, start[None], 500, (1.0, 0.1), plan, label="flat n=%d" % n)
        assert (bool(conv[0]), int(last[0])) == (True, 15)
        # on the planes o and o + (n - 1) vs an atom is outside (structure_utils.py:101-103: strict on both sides), a ulp further in
        # it is inside.  The map is cut through the density, so the outermost cells carry gradient and the decision shows.
        cg, co, _ = cut = _cut_map(base)
        hi = [co[d] + cg.shape[d] * vs - vs for d in range(3)]
        mid = co + 0.5 * np.array(cg.shape) * vs
        # All coordinates are multiples of 2^-10 A (the planes are multiples of 0.5): the centroid's sums are then exact in any order,
        # so device and oracle re-form (x - centroid) + centroid of a plane atom with the same bits and meet the same side.
        edge = np.round(start * 1024.0) / 1024.0
        for k in range(12):
            edge[k] = mid + np.array([3.125, -2.25, 1.75]) * (k % 5 - 2)
        for d in range(3):
            assert co[d] * 2 == round(co[d] * 2) and hi[d] * 2 == round(hi[d] * 2)
            edge[2 * d, d], edge[2 * d + 1, d] = co[d], hi[d]
            edge[6 + 2 * d, d], edge[7 + 2 * d, d] = co[d] + 2.0 ** -10, hi[d] - 2.0 ** -10
        for n_steps in (1, 2, 500):
            _run(lib, cut, edge[None], n_steps, (1.0, 0.1), plan, label="planes n=%d" % n)
        for n_steps in (1, 2):      # the case decides: one ulp inward of a plane moves everybody else by far more than the tolerance
            ref = O.refine(*cut, edge, n_steps=n_steps, max_step=1.0, min_step=0.1)[0]
            moved = 0
            for k in range(6):
                nudged = edge.copy()
                nudged[k, k // 2] = np.nextafter(edge[k, k // 2], np.inf if k % 2 == 0 else -np.inf)
                moved += np.abs(O.refine(*cut, nudged, n_steps=n_steps, max_step=1.0, min_step=0.1)[0][12:] - ref[12:]).max() > 1e-5
            assert moved >= 4, (n, n_steps, moved)      # (the oracle, like the reference, re-forms (x - centroid) + centroid: a plane atom may round off it)
        # a NaN in the middle candidate: it stops at once, its neighbours equal their solo runs bit for bit
        bad = _pose(atoms, 0.05, (0.3, 0.2, -0.4))
        bad[n // 2, 1] = np.nan
        other = _pose(atoms, 0.07, (-1.0, 0.6, 0.8))
        lib.upload_density(*m)
        got, conv, last = lib.refine(np.stack([start, bad, other]), n_steps=500, max_step=1.0, min_step=0.1)
        assert lib.last_refine_plan() == plan
        _, rconv, rlast, _ = O.refine(*m, bad, n_steps=500, max_step=1.0, min_step=0.1)
        assert (bool(conv[1]), int(last[1])) == (rconv, rlast) == (False, 0)
        for i, s in ((0, start), (2, other)):
            solo, sconv, slast = lib.refine(s, n_steps=500, max_step=1.0, min_step=0.1)
            assert lib.last_refine_plan() == plan
            assert np.array_equal(solo, got[i]) and (sconv, slast) == (bool(conv[i]), int(last[i])), i
            ref, rconv, rlast, _ = _oracle(m, s, 500, (1.0, 0.1))
            assert (sconv, slast) == (rconv, rlast)
            np.testing.assert_allclose(solo, ref, rtol=0, atol=1e-6)
    one = _pose(_atoms(base, 600), 0.1, (1.0, -0.8, 0.5))[300:301]
    got, conv, last = _run(lib, m, one[None], 500, (0.5, 0.01), (1, REG), label="one atom")
    assert (bool(conv[0]), int(last[0])) == (False, 2)      # the rotation angle is step / 0


def _dock_case(lib, m, structs, picks, plan, res=8.0, iso=(0.0, 0.0), label=""):
    """mad_dock_refine_score on candidates of several structures against the oracle chain.  picks: (structure, angle, shift) per
    candidate; equal picks must give bit-identical rows."""
    grid, origin, vs = m
    lib.upload_density(*m)
    hi_p, lo_p, rot, owner, starts = [], [], [], [], []
    for st, ang, shift in picks:
        atoms = structs[st][0]
        R = euler_rod_mat(AXIS, ang)
        hi = atoms[len(atoms) // 3] + 0.25
        lo = hi + np.asarray(shift)
        hi_p.append(hi); lo_p.append(lo); rot.append(R); owner.append(st)
        starts.append((atoms - hi) @ R + lo)      # MaD.py:566-569
    lim = (1.0, 0.1)
    args = ([a for a, _ in structs], [w for _, w in structs], np.array(hi_p), np.array(lo_p), np.array(rot), res)
    kw = dict(n_steps=500, max_step=lim[0], min_step=lim[1], density_isovalue=iso[0], ccc_isovalue=iso[1], cand_struct=np.array(owner))
    coords, conv, last, ccc = lib.dock_refine_score(*args, **kw)
    assert lib.last_refine_plan() == plan, (label, lib.last_refine_plan())
    first = {}
    worst, spread = 0.0, 0.0
    for c, pick in enumerate(picks):
        if pick in first:
            j = first[pick]
            assert np.array_equal(coords[c], coords[j]) and (conv[c], last[c]) == (conv[j], last[j]), (label, "copies differ", c, j)
            assert ccc[c] == ccc[j] or (np.isnan(ccc[c]) and np.isnan(ccc[j])), (label, c, j, ccc[c], ccc[j])
            continue
        first[pick] = c
        ref, rconv, rlast, sp = _oracle(m, starts[c], 500, lim)
        assert (bool(conv[c]), int(last[c])) == (rconv, rlast), (label, c)
        d = float(np.abs(coords[c] - ref).max())
        np.testing.assert_allclose(coords[c], ref, rtol=0, atol=1e-6, err_msg=str((label, c)))
        g2, x0, y0, z0 = O.structure_to_density(ref, structs[pick[0]][1], res, vs, isovalue=iso[0])
        want = O.ccc(grid.copy(), origin, g2, np.array([x0, y0, z0]), vs, iso[1])
        print("dock   %-28s plan %s cand %3d n %6d last %3d: device-oracle %.2e A (permuted %.2e), ccc %.9f oracle %.9f" %
              (label, plan, c, len(ref), rlast, d, sp, ccc[c], want))
        if np.isnan(want):
            assert np.isnan(ccc[c]), (label, c, ccc[c])
        else:
            assert abs(ccc[c] - want) <= 1e-5 * max(abs(want), 1e-3), (label, c, ccc[c], want)
        if d >= worst:
            worst, spread = d, sp
    coords2, conv2, last2, ccc2 = lib.dock_refine_score(*args, **kw)      # run to run
    assert np.array_equal(ccc2, ccc, equal_nan=True) and np.array_equal(conv2, conv) and np.array_equal(last2, last)
    for a, b in zip(coords, coords2):
        assert np.array_equal(a, b)
    rec = PLANS.setdefault(plan, [0.0, 0.0, 0])
    if worst >= rec[0]:
        rec[0], rec[1] = worst, spread
    rec[2] += 1


def test_dock_refine_score_mixed_sizes_split(lib, base, n_cu):
    """Candidates of different sizes in one call with G > 1: G is sized from the largest structure, so a small one leaves whole
    workgroups without an atom (they still publish, arrive and wait) and a middle one ends inside a workgroup.  Register form at
    G = 8, global form at G = 3; one candidate leaves the map; non-zero isovalues in the second."""
    m = _map(base, 1.5)
    w = base[1]

    def sub(n):
        idx = np.linspace(0, len(base[0]) - 1, n).astype(np.int64)
        return np.ascontiguousarray(base[0][idx]), np.ascontiguousarray(w[idx])
    structs = [sub(16500), sub(300), sub(5000)]
    picks = [(0, 0.08, (0.6, -0.3, 0.5)), (1, 0.1, (-0.5, 0.4, 0.3)), (2, 0.05, (0.4, 0.6, -0.5)), (1, 0.02, (70.0, 60.0, 65.0)),
             (0, 0.03, (-0.8, 0.2, 0.1)), (2, 0.0, (0.0, 0.0, 0.0))]
    _dock_case(lib, m, structs, picks, (8, REG), label="mixed registers")
    nc = _cands_for(n_cu, 3)
    structs = [sub(4096 * 3 + 100), sub(300), sub(5000)]
    kinds = [(0, 0.08, (0.6, -0.3, 0.5)), (1, 0.1, (-0.5, 0.4, 0.3)), (2, 0.05, (0.4, 0.6, -0.5)), (1, 0.02, (70.0, 60.0, 65.0))]
    _dock_case(lib, m, structs, [kinds[i % 4] for i in range(nc)], (3, GLOBAL), iso=(0.05, 0.1), label="mixed global")


def test_refine_plans_covered():
    """After the tests above (run the module as a whole): which plans were asserted, and the measured differences per plan."""
    print("\nplan (G, in_registers): largest device-oracle difference over full runs | the oracle's permutation spread there | cases")
    for plan in sorted(PLANS):
        print("  %s: %.2e A | %.2e A | %d" % ((plan,) + tuple(PLANS[plan])))
    assert {(G, REG) for G in range(1, 9)} <= set(PLANS), sorted(PLANS)
    assert {(G, GLOBAL) for G in (1, 2, 3, 8)} <= set(PLANS), sorted(PLANS)


# ---------------------------------------------------------------------------------------------------------------------
# the device against the reference's outputs on the edges (g24)
# ---------------------------------------------------------------------------------------------------------------------

def test_refine_against_reference_edges(lib, g24):
    g = g24
    for i, ((mi, s, n), (mx, mn)) in enumerate(zip(g["rf_case"], g["rf_lim"])):
        lib.upload_density(g["rf_map_%d" % mi], g["rf_map_origin_%d" % mi], float(g["rf_map_vs_%d" % mi]))
        got, conv, last = lib.refine(g["rf_start_" + str(g["rf_starts"][s])], n_steps=int(n), max_step=float(mx), min_step=float(mn))
        assert lib.last_refine_plan() == (1, REG)
        assert (conv, last) == (bool(g["rf_ret"][i][0]), int(g["rf_ret"][i][1])), (i, str(g["rf_starts"][s]))
        np.testing.assert_allclose(got, g["rf_final_%d" % i], rtol=0, atol=1e-8 if n <= 8 else 1e-6, equal_nan=True, err_msg=str((i, str(g["rf_starts"][s]))))


def _density_cases(g):
    for i, ((s, pad, pair), (res, vs, iso)) in enumerate(zip(g["dn_case"], g["dn_par"])):
        name = str(g["dn_structs"][s])
        key = "lattice_%d" % pair if name == "lattice" else name
        yield i, name, g["dn_atoms_" + key], synth.masses([str(e) for e in g["dn_elem_" + name]]), float(res), float(vs), float(iso), int(pad)


def test_density_against_reference_edges(lib, g24):
    for i, name, atoms, mass, res, vs, iso, pad in _density_cases(g24):
        got, x0, y0, z0 = lib.structure_to_density(atoms, mass, res, vs, isovalue=iso, pad=pad)
        ref = g24["dn_grid_%d" % i]
        assert got.shape == ref.shape, (i, name)
        np.testing.assert_array_equal([x0, y0, z0], g24["dn_origin"][i])
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-7, err_msg=str((i, name)))


def test_ccc_and_overlap_on_the_reference_box_table(lib, g24):
    """Every geometry of the table: against the reference where it gives a number (1e-5: it sums in float32), against the oracle
    everywhere (1e-9) -- also where the reference raised, on a half-voxel tie: there the oracle's rule, the smaller extent, is this
    project's definition.  Both grids come back clamped.  mad_grid_overlap on the same boxes against oracle.overlap."""
    g = g24
    vs, o1 = float(g["cc_vs"]), g["cc_o1"]
    for i, (k, off, iso) in enumerate(zip(g["cc_case"], g["cc_off"], g["cc_iso"])):
        o2 = o1 + off * vs
        a, b, a2, b2 = g["cc_g1"].copy(), g["cc_g2_%d" % k].copy(), g["cc_g1"].copy(), g["cc_g2_%d" % k].copy()
        want = O.ccc(a, o1, b, o2, vs, float(iso))
        got = lib.ccc(a2, o1, b2, o2, vs, float(iso))
        np.testing.assert_array_equal(a2, a)
        np.testing.assert_array_equal(b2, b)
        if np.isnan(want):
            assert np.isnan(got), (i, off, got)
        else:
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (i, off, got, want)
        if not g["cc_raised"][i]:
            ref = float(g["cc_val"][i])
            if np.isnan(ref):
                assert np.isnan(got), (i, off, got)
            elif ref == 0:
                assert got == 0, (i, off, got)
            else:
                assert abs(got - ref) <= 1e-5 * max(abs(ref), 1e-3), (i, off, got, ref)
        thr = max(float(iso), 1e-8)
        a, b, a2, b2 = g["cc_g1"].copy(), g["cc_g2_%d" % k].copy(), g["cc_g1"].copy(), g["cc_g2_%d" % k].copy()
        assert lib.grid_overlap(a2, o1, b2, o2, vs, thr) == O.overlap(a, o1, b, o2, vs, thr), (i, off)
        np.testing.assert_array_equal(a2, a)
        np.testing.assert_array_equal(b2, b)


def test_density_ccc_against_reference_chain(lib, g24):
    """The resident path (upload, simulate, score) against the reference's structure_to_density + get_CCC_with_grid on placements
    that leave the map at the low corner, the high corner, on one axis, touch it and miss it; isovalues zero and not."""
    g = g24
    lib.upload_density(g["rf_map_0"], g["rf_map_origin_0"], float(g["rf_map_vs_0"]))
    mass = synth.masses([str(e) for e in g["dc_elem"]])
    for (res, diso, ciso), atoms, ref in zip(g["dc_par"], g["dc_atoms"], g["dc_val"]):
        got = lib.density_ccc(atoms, mass, float(res), density_isovalue=float(diso), ccc_isovalue=float(ciso))[0]
        if np.isnan(ref):
            assert np.isnan(got), (got, ref)
        elif ref == 0:
            assert got == 0, (got, ref)
        else:
            assert abs(got - ref) <= 1e-5 * max(abs(ref), 1e-3), (got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# density and CCC against the oracle, beyond the fixture
# ---------------------------------------------------------------------------------------------------------------------

def _kernel_radius(res, vs):
    return int(np.ceil(3.0 * res / (np.pi * np.sqrt(2.0)) / vs))


def test_density_sweep_against_oracle(lib):
    """Voxel x resolution x padding x isovalue, on a globule near the origin, far from it (1e4 A: the lattice alignment works on
    large numbers) and at all-negative coordinates.  With an isovalue, a voxel within one float32 ulp of it may fall on either side:
    only voxels whose unthresholded oracle value is within 1e-6 of the isovalue would be exempt, at most 1 in 1e5 -- and the seed is
    one for which the oracle has no such voxel in any case of the sweep, which is asserted here, so nothing is exempt in fact."""
    iso = 0.05
    coords, _, elems = synth.random_globule(150, 8.0, 15)
    mass = synth.masses(elems)
    places = (np.zeros(3), np.array([1e4, -1e4, 3.0]), -coords.max(0) - 5.3)
    for vs in (0.7, 1.2, 1.5, 2.0):
        for res in (2.0, 5.0, 8.0, 15.0):
            for pad in (0, 2):
                for t in places:
                    atoms = coords + t
                    raw, rx, ry, rz = O.structure_to_density(atoms, mass, res, vs, isovalue=0.0, pad=pad)
                    near = np.abs(raw.astype(np.float64) - iso) <= 1e-6
                    assert near.sum() == 0 <= 1e-5 * raw.size, (vs, res, pad, t, int(near.sum()))      # a seed with such a voxel is replaced
                    for cut in (0.0, iso):
                        ref = raw if cut == 0 else O.structure_to_density(atoms, mass, res, vs, isovalue=cut, pad=pad)[0]
                        got, gx, gy, gz = lib.structure_to_density(atoms, mass, res, vs, isovalue=cut, pad=pad)
                        assert got.shape == ref.shape and (gx, gy, gz) == (rx, ry, rz), (vs, res, pad, cut, t)
                        bad = (np.abs(got.astype(np.float64) - ref) > 2e-7) & ~near
                        assert not bad.any(), (vs, res, pad, cut, t, int(bad.sum()), float(np.abs(got.astype(np.float64) - ref).max()))
                        if cut > 0:
                            assert (ref == 0).any() and (ref[ref > 0] >= np.float32(cut)).all()


def test_density_kernel_radius_limit(lib):
    """r = ceil(3 resolution / (pi sqrt 2) / voxel): 64 is the largest the device takes, 65 is refused."""
    atoms = np.array([[0.3, 1.1, -0.7], [2.9, -1.4, 0.2], [-1.6, 0.5, 2.2], [0.0, 0.0, 0.0]])
    mass = synth.masses(["C", "N", "O", "S"])
    assert _kernel_radius(94.7, 1.0) == 64 and _kernel_radius(94.9, 1.0) == 65
    ref, rx, ry, rz = O.structure_to_density(atoms, mass, 94.7, 1.0)
    got, gx, gy, gz = lib.structure_to_density(atoms, mass, 94.7, 1.0)
    assert got.shape == ref.shape and (gx, gy, gz) == (rx, ry, rz)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-7)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.structure_to_density(atoms, mass, 94.9, 1.0)


def test_ccc_box_table_scaled_up(lib):
    """The box geometries of the fixture on larger, non-cubic grids (the 64 partial sums of k_ccc_b all get work)."""
    rng = np.random.default_rng(77)
    vs, o1 = 1.5, np.array([-3.0, 4.5, 0.75])
    n1 = (40, 37, 45)
    g1 = (rng.random(n1) ** 2).astype(np.float32)
    g1[rng.random(n1) < 0.05] = -0.2
    for n2 in ((23, 50, 31), (40, 37, 45), (52, 41, 49)):
        g2 = (rng.random(n2) ** 2).astype(np.float32)
        g2[rng.random(n2) < 0.05] = -0.1
        xs = (-n2[0] - 3.0, -float(n2[0]), -7.5, -2.5, -0.5, -0.25, 0.0, 0.49, 0.5, 0.51, 1.5, 6.0, float(n1[0]), n1[0] + 4.0)
        for x in xs:
            for y in (0.0, 1.25, -3.0, n1[1] - 2.5):
                for iso in (0.0, 0.1):
                    o2 = o1 + np.array([x, y, -x / 2]) * vs
                    a, b, a2, b2 = g1.copy(), g2.copy(), g1.copy(), g2.copy()
                    want = O.ccc(a, o1, b, o2, vs, iso)
                    got = lib.ccc(a2, o1, b2, o2, vs, iso)
                    np.testing.assert_array_equal(a2, a)
                    np.testing.assert_array_equal(b2, b)
                    if np.isnan(want):
                        assert np.isnan(got), (n2, x, y, got)
                    else:
                        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (n2, x, y, got, want)


def _chain(m, atoms, mass, res, diso, ciso):
    grid, origin, vs = m
    g2, x0, y0, z0 = O.structure_to_density(atoms, mass, res, vs, isovalue=diso)
    return O.ccc(grid.copy(), origin, g2, np.array([x0, y0, z0]), vs, ciso), g2.shape, np.array([x0, y0, z0])


def _same(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), (what, got, want)
    elif want == 0:
        assert got == 0, (what, got, want)
    else:
        assert abs(got - want) <= 1e-5 * max(abs(want), 1e-3), (what, got, want)


def test_density_ccc_boxes_at_the_map_edges(lib):
    """The resident path with the simulated box sticking out of the uploaded map at the low corner, at the high corner, on one axis
    only, touching it, missing it, and containing it; isovalues zero and not; the uploaded map stays as it was."""
    coords, _, elems = synth.random_globule(500, 12.0, 8)
    mass = synth.masses(elems)
    vs, res = 1.5, 8.0
    grid, x0, y0, z0 = O.structure_to_density(coords, mass, res, vs)
    grid = np.pad(grid, 4)
    grid[3, 5, 7] = -0.4
    origin = np.array([x0, y0, z0]) - 4 * vs
    m = (grid, origin, vs)
    ext = np.array(grid.shape) * vs
    _, shape2, o2 = _chain(m, coords, mass, res, 0.0, 0.0)
    touch = (origin[0] - shape2[0] * vs) - o2[0]      # a multiple of the voxel: the box ends exactly where the map begins
    shifts = [(0, 0, 0), (1.1, -0.7, 0.4), tuple(-0.6 * ext), tuple(0.6 * ext), (0.7 * ext[0], 0, 0), (0, -0.65 * ext[1], 0.3),
              (touch, 0, 0), (touch - vs, 0, 0), (touch + vs, 0, 0), (3 * ext[0], 0, 0), (0.25 * vs, 0.5 * vs, -0.5 * vs)]
    cands = np.stack([coords + np.array(s) for s in shifts])
    lib.upload_density(*m)
    before = lib.density_ccc(cands, mass, res)
    kinds = set()
    for diso, ciso in ((0.0, 0.0), (0.05, 0.1), (0.0, 0.3), (0.2, 0.0)):
        got = lib.density_ccc(cands, mass, res, density_isovalue=diso, ccc_isovalue=ciso)
        for c, s in enumerate(shifts):
            want, _, _ = _chain(m, cands[c], mass, res, diso, ciso)
            kinds.add("nan" if np.isnan(want) else ("zero" if want == 0 else "value"))
            _same(got[c], want, (s, diso, ciso))
    assert kinds == {"nan", "zero", "value"}
    assert np.array_equal(lib.density_ccc(cands, mass, res), before, equal_nan=True)      # the map was clamped on the fly only
    assert before[0] > 0.9
    # a small map inside a large structure's box
    small = np.ascontiguousarray(grid[14:24, 15:24, 13:25])
    ms = (small, origin + np.array([14, 15, 13]) * vs, vs)
    lib.upload_density(*ms)
    for diso, ciso in ((0.0, 0.0), (0.05, 0.1)):
        got = lib.density_ccc(cands[:2], mass, res, density_isovalue=diso, ccc_isovalue=ciso)
        for c in range(2):
            _same(got[c], _chain(ms, cands[c], mass, res, diso, ciso)[0], ("inside", c, diso, ciso))


def test_density_ccc_more_than_one_chunk(lib):
    """density_batch cuts a batch into chunks of at most 512 Mi float64 voxels and re-bases offsets, maxima and partial sums per
    chunk: a 0.5 A map makes a candidate's volume millions of voxels, and enough candidates make two chunks.  Three poses round-robin,
    copies of each on both sides of the cut: bit-identical; each pose against the oracle.  About 8 GB of device scratch; last."""
    coords, _, elems = synth.random_globule(9000, 30.0, 6)
    mass = synth.masses(elems)
    vs, res = 0.5, 8.0
    grid, x0, y0, z0 = O.structure_to_density(coords, mass, res, vs)
    m = (grid, np.array([x0, y0, z0]), vs)
    poses = [coords, _pose(coords, 0.4, (3.0, -2.0, 1.0)), _pose(coords, 1.1, (-40.0, 10.0, 25.0))]
    want, vox = [], []
    for p in poses:
        w, shape, _ = _chain(m, p, mass, res, 0.0, 0.0)
        want.append(w)
        vox.append(int(np.prod(shape)))
    cap = 512 << 20
    n, tot = 0, 0
    while tot + vox[n % 3] <= cap:      # the first chunk, as density_batch fills it
        tot += vox[n % 3]
        n += 1
    n_first = n
    n += 7                              # ... and at least two copies of every pose behind the cut
    assert n_first >= 6 and sum(vox[i % 3] for i in range(n_first, n)) <= cap
    lib.upload_density(*m)
    got = lib.density_ccc(np.stack([poses[i % 3] for i in range(n)]), mass, res)
    assert lib.last_density_chunks() == 2
    assert lib.density_ccc(np.stack(poses), mass, res).tolist() == got[:3].tolist() and lib.last_density_chunks() == 1
    for i in range(n):
        assert got[i] == got[i % 3], (i, n_first, got[i], got[i % 3])
    for k in range(3):
        print("chunks: pose %d ccc %.9f oracle %.9f, %d voxels; %d candidates, %d in the first chunk" % (k, got[k], want[k], vox[k], n, n_first))
        _same(got[k], want[k], ("pose", k))
    assert want[0] > 0.99
