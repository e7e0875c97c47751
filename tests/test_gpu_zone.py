"""A map cut around a structure, or with the structure erased, on the device (mad_map_zone: k_zone_count / k_zone_scan / k_zone_fill,
k_map_zone) against the numpy restatement of DESIGN.md section 4i in tests/test_zone_restate.py.

Hard calls (soft = 0): the output equals the restatement bit for bit (uint32 views) and the counts are equal.  Soft calls:
|device - restated| <= ulp32(|restated|) + 1e-15 max|g| on every voxel -- the device's float64 cos may differ from glibc's in the last
ulp, float64 sqrt and the divisions are correctly rounded on both sides, so the product can land on the
neighbouring float32 --, voxels whose restated weight is exactly 0 or 1 are still bit-exact, and the counts are equal: the inputs
keep every voxel far more than an ulp from both bounds."""
import numpy as np
import pytest

from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_zone_restate import BASE_DIMS, BASE_ORIGIN, BASE_RADIUS, BASE_SOFT, BASE_VOXSP, base_atoms, base_grid, bits, chain, restate_zone, zone_d2

pytestmark = pytest.mark.gpu


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def make_grid(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


def hold(dev, dev_counts, g, D2, radius, soft, erase):
    """The device's output and counts against restate_zone on a D2 computed once for the case."""
    ref, counts, w = restate_zone(g, None, None, None, radius, soft, erase, D2=D2, weights=True)
    print("counts device %s restated %s" % (dev_counts, counts))
    assert tuple(dev_counts) == counts
    exact = (w == 0.0) | (w == 1.0)
    n_bad = int((bits(dev)[exact] != bits(ref)[exact]).sum())
    print("voxels of weight 0 or 1 whose bits differ: %d of %d" % (n_bad, int(exact.sum())))
    assert n_bad == 0
    if soft == 0:
        assert exact.all()
        return
    part = ~exact
    gmax = float(np.abs(g[np.isfinite(g)]).max()) if np.isfinite(g).any() else 0.0
    err = np.abs(dev[part].astype(np.float64) - ref[part].astype(np.float64))
    tol = np.spacing(np.abs(ref[part])).astype(np.float64) + 1e-15 * gmax
    print("soft voxels %d, max |device - restated| = %g, voxels off by one float32: %d" % (int(part.sum()), err.max() if err.size else 0.0,
                                                                                            int((err > 0).sum())))
    assert np.all(err <= tol)


def run(lib, g, origin, voxsp, atoms, radius, soft, erase, window=False):
    """One call of Lib.map_zone on a copy of g, held to the restatement.  -> (out, counts)"""
    D2 = zone_d2(g.shape, origin, voxsp, atoms, (radius + soft) if window else None)
    out = g.copy()
    counts = lib.map_zone(out, origin, voxsp, atoms, radius, soft, erase)
    hold(out, counts, g, D2, radius, soft, erase)
    return out, counts


@pytest.fixture(scope="module")
def base():
    g, inside, outside = base_grid()
    atoms = base_atoms()
    return dict(g=g, inside=inside, outside=outside, atoms=atoms, D2=zone_d2(BASE_DIMS, BASE_ORIGIN, BASE_VOXSP, atoms))


# ---- 1. the base case ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("erase", (False, True))
@pytest.mark.parametrize("soft", (0.0, BASE_SOFT))
@pytest.mark.parametrize("through", ("lib", "dmap"))
def test_base_case(lib, base, through, soft, erase):
    g = base["g"]
    if through == "lib":
        out = g.copy()
        counts = lib.map_zone(out, BASE_ORIGIN, BASE_VOXSP, base["atoms"], BASE_RADIUS, soft, erase)
    else:
        d = dmap(g.copy(), BASE_ORIGIN, BASE_VOXSP)
        counts = d.zone(base["atoms"], BASE_RADIUS, soft=soft, erase=erase)
        out = d.grid3d
    hold(out, counts, g, base["D2"], BASE_RADIUS, soft, erase)
    kept, zeroed = (base["outside"], base["inside"]) if erase else (base["inside"], base["outside"])
    for j in kept:      # NaN, -0.0, inf: every bit
        assert bits(out)[tuple(j)] == bits(g)[tuple(j)]
    for j in zeroed:      # all bits zero, NaN * 0 did not leak
        assert bits(out)[tuple(j)] == 0
    assert bits(g)[tuple(kept[0])] & 0x7fffffff > 0x7f800000 and bits(g)[tuple(kept[1])] == 0x80000000


def test_dmap_zone_copies_what_it_cannot_edit(lib, base):
    g64 = np.asfortranarray(base["g"].astype(np.float64))
    before = g64.copy()
    d = dmap(g64, BASE_ORIGIN, BASE_VOXSP)
    counts = d.zone(base["atoms"], BASE_RADIUS)
    assert d.grid3d is not g64 and d.grid3d.dtype == np.float32 and d.grid3d.flags.c_contiguous
    assert np.array_equal(bits(g64.astype(np.float32)), bits(before.astype(np.float32)))
    hold(d.grid3d, counts, base["g"], base["D2"], BASE_RADIUS, 0.0, False)
    ro = base["g"].copy()
    ro.flags.writeable = False
    d = dmap(ro, BASE_ORIGIN, BASE_VOXSP)
    counts = d.zone(base["atoms"], BASE_RADIUS, erase=True)
    assert d.grid3d is not ro and np.array_equal(bits(ro), bits(base["g"]))
    hold(d.grid3d, counts, base["g"], base["D2"], BASE_RADIUS, 0.0, True)


# ---- 2. ties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twice", (False, True))
def test_ties_are_inclusive(lib, twice):
    g = np.ones((12, 12, 12), np.float32)
    atoms = [[5.0, 5.0, 5.0]] * (2 if twice else 1)
    out, counts = run(lib, g, (0, 0, 0), 1.0, atoms, 5.0, 0.0, False)
    D2 = zone_d2(g.shape, (0, 0, 0), 1.0, atoms)
    assert counts == (515, 0) and int((out == 1).sum()) == 515 and np.all(out[D2 == 25.0] == 1) and int((D2 == 25.0).sum()) == 30
    out, counts = run(lib, g, (0, 0, 0), 1.0, atoms, 5.0, 0.0, True)
    assert counts == (515, 0) and int((out == 1).sum()) == g.size - 515 and np.all(out[D2 == 25.0] == 0)


def lattice_case(dims, origin, voxsp, atom_idx, seed):
    """A grid without zeros and atoms at origin + voxsp * index (indices may lie outside the grid).  With an origin and a spacing
    that are small multiples of a power of two every position, difference and square is exact, so a voxel k lattice steps from an
    atom along an axis has d2 == (k * voxsp)^2 bit for bit."""
    origin = np.asarray(origin, np.float64)
    g = make_grid(dims, seed)
    g[g == 0] = np.float32(0.5)
    return g, origin, origin + voxsp * np.asarray(atom_idx, np.float64).reshape(-1, 3)


def hold_ties(lib, g, origin, voxsp, atoms, radius, tie_voxels, n_inside):
    """Keep and erase at soft = 0, bits and counts against the restatement (run), and the named voxels are ties that are inside."""
    D2 = zone_d2(g.shape, origin, voxsp, atoms)
    for j in tie_voxels:
        assert D2[tuple(j)] == radius * radius      # the test's own premise
    keep, counts = run(lib, g, origin, voxsp, atoms, radius, 0.0, False)
    assert counts == (n_inside, 0) and int((keep != 0).sum()) == n_inside
    erased, counts = run(lib, g, origin, voxsp, atoms, radius, 0.0, True)
    assert counts == (n_inside, 0) and int((erased == 0).sum()) == n_inside
    for j in tie_voxels:
        assert bits(keep)[tuple(j)] == bits(g)[tuple(j)] and bits(erased)[tuple(j)] == 0


@pytest.mark.parametrize("origin,voxsp", (((0.0, 0.0, 0.0), 1.0), ((0.25, -1.5, 3.0), 0.5)))
def test_ties_on_the_first_layer_of_the_next_brick(lib, origin, voxsp):
    """The atom's own brick is not the tie's: the brick that holds the tie voxel sees the atom at exactly R from its box, which
    is where the staging test decides."""
    # x and y: bricks are 4 x 8 x 32 voxels; (8,5,5) and (5,8,5) open the bricks after the atom's
    g, o, atoms = lattice_case((12, 12, 12), origin, voxsp, [[5, 5, 5]], 21)
    hold_ties(lib, g, o, voxsp, atoms, 3.0 * voxsp, [(8, 5, 5), (5, 8, 5), (2, 5, 5), (5, 5, 8)], 123)
    # all three axes, towards the next brick (first atom) and towards the one before (second atom); nz > 32
    g, o, atoms = lattice_case((8, 12, 40), origin, voxsp, [[1, 5, 29], [6, 10, 34]], 22)
    ties = [(4, 5, 29), (1, 8, 29), (1, 5, 32), (3, 10, 34), (6, 7, 34), (6, 10, 31)]
    n_inside = int((zone_d2(g.shape, o, voxsp, atoms) <= (3.0 * voxsp) ** 2).sum())
    hold_ties(lib, g, o, voxsp, atoms, 3.0 * voxsp, ties, n_inside)


@pytest.mark.parametrize("atom,voxel", (((-5, 5, 5), (0, 5, 5)), ((16, 5, 5), (11, 5, 5)), ((5, -5, 5), (5, 0, 5)), ((5, 16, 5), (5, 11, 5)),
                                        ((5, 5, -5), (5, 5, 0)), ((5, 5, 16), (5, 5, 11))))
@pytest.mark.parametrize("origin,voxsp", (((0.0, 0.0, 0.0), 1.0), ((0.25, -1.5, 3.0), 0.5)))
def test_tie_of_an_atom_exactly_the_radius_outside_the_box(lib, origin, voxsp, atom, voxel):
    """One atom on a lattice line, exactly `radius` beyond a face of the map: it reaches one voxel, at d2 == r2, and the drop of
    atoms out of reach before binning must not take it."""
    g, o, atoms = lattice_case((12, 12, 12), origin, voxsp, [atom], 23)
    hold_ties(lib, g, o, voxsp, atoms, 5.0 * voxsp, [voxel], 1)


def test_radius_zero_with_an_edge_whose_square_underflows(lib):
    """radius 0 and soft 1e-200: R * R is 0, and the voxel an atom sits on (D2 = 0 <= r2) still has weight 1."""
    g, o, atoms = lattice_case((9, 10, 35), (0.25, -1.5, 3.0), 0.5, [[4, 7, 33], [20, 3, 3]], 24)
    for erase in (False, True):
        out, counts = run(lib, g, o, 0.5, atoms, 0.0, 1e-200, erase)
        assert counts == (1, 0) and (bits(out)[4, 7, 33] == 0) == erase and int((out != 0).sum()) == (g.size - 1 if erase else 1)


# ---- 3. shapes that break the lane layout --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", ((5, 7, 3), (1, 1, 1), (4, 8, 32), (9, 17, 33), (6, 9, 37)))
def test_shapes(lib, dims):
    origin, voxsp = np.array([-2.0, 0.7, 5.5]), 1.3
    n = np.array(dims)
    hi = origin + voxsp * (n - 1)
    rng = np.random.default_rng(sum(dims))
    centre = origin + voxsp * np.minimum(n - 1, (2, 3, 1)).astype(np.float64)      # a voxel centre, bit for bit
    atoms = np.concatenate([[centre, hi, origin + [0.0, 0.0, voxsp * (n[2] - 1)]], origin + rng.random((3, 3)) * (hi - origin + 3.0) - 1.5])
    g = make_grid(dims, 3)
    for radius, soft in ((2.0, 0.0), (2.0, 1.0)):
        for erase in (False, True):
            out, counts = run(lib, g, origin, voxsp, atoms, radius, soft, erase)
            assert counts[0] >= 1


# ---- 4. chunking and culling ---------------------------------------------------------------------------------------------------

def test_more_atoms_in_a_cell_than_a_chunk(lib):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(3000, 3))
    atoms = np.array([11.3, 9.1, 14.2]) + d / np.linalg.norm(d, axis=1)[:, None] * 0.5 * rng.random((3000, 1))
    g = make_grid((21, 19, 40), 4)
    for soft, erase in ((0.0, False), (1.5, True)):
        run(lib, g, (0.0, 0.0, 0.0), 1.1, atoms, 3.0, soft, erase)


def test_radius_beyond_the_box(lib):
    rng = np.random.default_rng(6)
    d = rng.normal(size=(6, 3)) + [3.0, 0.0, 0.0]      # all on one side, so that the radius ends inside the box
    atoms = np.array([10.0, 9.0, 11.0]) + d / np.linalg.norm(d, axis=1)[:, None] * (62.0 + 8.0 * rng.random((6, 1)))
    g = make_grid((20, 18, 22), 5)
    for soft, erase in ((0.0, False), (4.0, False), (4.0, True)):
        out, counts = run(lib, g, (0.0, 0.0, 0.0), 1.0, atoms, 60.0, soft, erase)
        assert 0 < counts[0] < g.size
    out, counts = run(lib, g, (0.0, 0.0, 0.0), 1.0, atoms, 200.0, 0.0, False)
    assert counts == (g.size, 0) and np.array_equal(bits(out), bits(g))


def test_cell_count_bound(lib):
    """radius 0.05 on a 64^3 grid: the cell edge is set by the bound on the cell count, not by the reach."""
    origin, voxsp = np.array([0.5, -3.0, 2.0]), 1.0
    rng = np.random.default_rng(8)
    j = rng.integers(0, 64, size=(20, 3))
    on = origin + voxsp * j.astype(np.float64)
    near = origin + voxsp * rng.integers(0, 64, size=(20, 3)).astype(np.float64) + 0.03 * np.array([1.0, 0.0, 0.0])
    atoms = np.concatenate([on, near, origin + 63.0 * rng.random((200, 3))])
    g = make_grid((64, 64, 64), 9)
    g[g == 0] = 0.5
    out, counts = run(lib, g, origin, voxsp, atoms, 0.05, 0.0, False)
    assert counts[0] >= len(np.unique(j, axis=0)) and counts[1] == 0
    run(lib, g, origin, voxsp, atoms, 0.05, 0.0, True)


def test_radius_zero_with_a_soft_edge(lib):
    origin, voxsp = np.array([1.0, 2.0, 3.0]), 0.9
    on = origin + voxsp * np.array([4.0, 5.0, 6.0])
    atoms = np.concatenate([[on], origin + 14.0 * np.random.default_rng(10).random((12, 3))])
    g = make_grid((17, 18, 19), 11)
    for erase in (False, True):
        out, counts = run(lib, g, origin, voxsp, atoms, 0.0, 1.5, erase)
        assert counts[0] == 1 and counts[1] > 0


@pytest.mark.parametrize("atoms", (np.array([[-40.0, 5.0, 5.0], [10.0, 60.0, 3.0], [1e4, 1e4, 1e4]]), np.zeros((0, 3))), ids=("far", "none"))
def test_nothing_in_reach(lib, atoms):
    g = make_grid((13, 14, 35), 12)
    g[2, 3, 4], g[5, 6, 7], g[1, 1, 1] = np.nan, -0.0, np.inf
    for soft in (0.0, 2.0):
        out, counts = run(lib, g, (0.0, 0.0, 0.0), 1.0, atoms, 4.0, soft, False)
        assert counts == (0, 0) and not bits(out).any()
        out, counts = run(lib, g, (0.0, 0.0, 0.0), 1.0, atoms, 4.0, soft, True)
        assert counts == (0, 0) and np.array_equal(bits(out), bits(g))


# ---- 5. more workgroups than the device holds at once --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    dims, voxsp, origin = (161, 129, 131), 1.1, np.array([-12.0, 4.0, 30.5])
    c = chain(2000, 17)
    c += origin + 0.5 * voxsp * (np.array(dims) - 1) - 0.5 * (c.min(0) + c.max(0))
    return dict(g=make_grid(dims, 13), origin=origin, voxsp=voxsp, atoms=c, D2=zone_d2(dims, origin, voxsp, c, window=6.0))


@pytest.mark.parametrize("erase", (False, True))
def test_large_grid(lib, big, erase):
    out = big["g"].copy()
    counts = lib.map_zone(out, big["origin"], big["voxsp"], big["atoms"], 4.0, 2.0, erase)
    assert counts[0] > 10000 and counts[1] > 10000
    hold(out, counts, big["g"], big["D2"], 4.0, 2.0, erase)


def test_more_bricks_than_one_launch(lib):
    """A row of 2^24 + 5 voxels along x is 2^22 + 2 bricks, more than one launch of k_map_zone takes."""
    dims, origin, voxsp = ((1 << 24) + 5, 1, 1), np.array([-7.0, 1.0, 2.0]), 0.5
    last = origin[0] + voxsp * (dims[0] - 1)
    atoms = np.array([[origin[0] + 3.2, 1.5, 2.0], [0.5 * (origin[0] + last), 1.0, 2.5], [last - 0.7, 1.0, 2.0], [last + 2.0, 1.0, 2.0]])
    g = make_grid(dims, 14)
    D2 = zone_d2(dims, origin, voxsp, atoms, window=4.5)
    for erase in (False, True):
        out = g.copy()
        counts = lib.map_zone(out, origin, voxsp, atoms, 3.0, 1.5, erase)
        hold(out, counts, g, D2, 3.0, 1.5, erase)


# ---- 6. repeatability ----------------------------------------------------------------------------------------------------------

def test_same_bits_after_another_call(lib, base):
    def call():
        out = base["g"].copy()
        return out, lib.map_zone(out, BASE_ORIGIN, BASE_VOXSP, base["atoms"], BASE_RADIUS, BASE_SOFT, False)
    a, ca = call()
    other = make_grid((50, 40, 70), 15)
    lib.map_zone(other, (0.0, 0.0, 0.0), 2.0, chain(5000, 3) + [50.0, 40.0, 70.0], 7.0, 1.0, True)
    b, cb = call()
    assert ca == cb and np.array_equal(bits(a), bits(b))


# ---- 7. several structures -----------------------------------------------------------------------------------------------------

def test_a_list_is_the_concatenation(lib, base):
    class Structure(object):      # what Dmap.zone asks of a PDB
        def __init__(self, c):
            self.c = c

        def get_coords(self):
            return self.c
    atoms = base["atoms"]
    one = dmap(base["g"].copy(), BASE_ORIGIN, BASE_VOXSP)
    c_one = one.zone(atoms, BASE_RADIUS, soft=BASE_SOFT, erase=True)
    for parts in ([atoms[:120], atoms[120:]], (Structure(atoms[:7]), atoms[7:]), [Structure(atoms[:200]), Structure(atoms[200:])]):
        two = dmap(base["g"].copy(), BASE_ORIGIN, BASE_VOXSP)
        assert two.zone(parts, BASE_RADIUS, soft=BASE_SOFT, erase=True) == c_one
        assert np.array_equal(bits(two.grid3d), bits(one.grid3d))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_grid(lib, base):
    g = base["g"].copy()
    bad = base["atoms"].copy()
    bad[17, 1] = np.nan
    inf = base["atoms"].copy()
    inf[3, 2] = np.inf
    for atoms, voxsp, radius, soft in ((bad, 1.2, 3.0, 0.0), (inf, 1.2, 3.0, 0.0), (base["atoms"], 1.2, -1.0, 2.0), (base["atoms"], 1.2, 0.0, 0.0),
                                       (base["atoms"], 0.0, 3.0, 0.0), (base["atoms"], -1.2, 3.0, 0.0), (base["atoms"], 1.2, 3.0, -0.5),
                                       (base["atoms"], 1.2, np.nan, 0.0)):
        with pytest.raises(MadBackendError):
            lib.map_zone(g, BASE_ORIGIN, voxsp, atoms, radius, soft)
        assert np.array_equal(bits(g), bits(base["g"]))


# ---- 9. far from zero ----------------------------------------------------------------------------------------------------------

def test_coordinates_far_from_zero(lib):
    shift = np.array([1e4, -1e4, 1e4])
    origin, voxsp = np.array([1.3, -0.4, 2.2]) + shift, 0.7
    c = chain(60, 19, step=1.0)
    c += origin + 0.5 * voxsp * 23 - 0.5 * (c.min(0) + c.max(0))
    g = make_grid((24, 24, 24), 16)
    for erase in (False, True):
        out, counts = run(lib, g, origin, voxsp, c, 2.5, 0.0, erase)
        assert 0 < counts[0] < g.size
