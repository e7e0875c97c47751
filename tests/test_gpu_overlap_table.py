"""The overlap table of assembly building (mad_overlap_matrix: density_batch without a map, k_clamp_count, k_overlap_pairs
driven by overlap_run, the division on the host) at sizes, spacings, isovalues and pair counts beyond the 12 structures of
g9_assembly.npz.  The oracle is oracle.structure_to_density + oracle.overlap_ratio, which reproduce the reference's table bit for
bit on that fixture; the comparison is assert_array_equal on the whole n x n table (two integers divided in float64 on both sides).

A voxel whose density sits on an isovalue may fall on either side of it on the device (2e-7 is what test_gpu_score_tail.py holds the
density to).  Nothing is exempted for that: every case is chosen so that the unthresholded oracle density has NO voxel within 1e-6
of an isovalue in use, and so that its table holds enough distinct non-zero values to tell a wrong entry from a right one.
test_inputs_keep_their_teeth asserts both for every case of the file and needs no GPU.

  1. sweep           8 structures of very different sizes (600 atoms, 150, 7, one atom, an identical copy, one inside another,
                     one 500 A away) x 3 placements x 4 voxels x 3 resolutions x 5 isovalue pairs: pool offsets and strides
                     differ per grid, k_clamp_count writes the pool when the overlap isovalue is not the default
  2. permutation     the reversed list: overlap(j, i) = common / npos[j] of the first table is an entry of the second
  3. single calls    the batched densities and the pair kernel against structure_to_density + grid_overlap one at a time, bit
                     for bit, and the table twice
  4. pair launches   260 structures, 33 670 pairs: the second launch of overlap_run's loop over 32 768 pairs, and density_batch
                     with hundreds of jobs in one chunk
  5. large           two structures of 17 M voxels: thousands of rounds per thread of k_overlap_pairs, pool index past 2^24
  6. density chunks  enough 17 M voxel structures for a second chunk of density_batch on the path without a host synchronisation
                     (test_gpu_score_tail.py has the path with one); about 8 GB of device scratch, last in the file
  7. refusals        the C entry's own argument checks and its n_struct 0 and 1 branches, which Lib.overlap_matrix never reaches
and assembly.overlap_table on PDB files against overlap_matrix at the assembly's settings."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from mad_amd import assembly, synth
from mad_amd._lib import _p
from mad_amd.PDB import PDB
from oracle import oracle as O

NEAR = 1e-6      # band of test_density_sweep_against_oracle: five times the 2e-7 the device's density is held to
DEFAULTS = (2.0, 5.0, 0.2, 1e-8)      # voxel, resolution, density isovalue, overlap isovalue (MaD.py:669, 760)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

def ball(n, radius, seed):
    """n points uniform in a ball, rounded to the PDB's 3 decimals (a random-walk globule piles its density into a small core and
    keeps too few voxels above an isovalue of 0.2 for pairs to overlap)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.round(d * (radius * rng.random(n) ** (1.0 / 3.0))[:, None], 3)


def _mass(n):
    return synth.masses([("C", "N", "O", "S")[i % 4] for i in range(n)])


def _with_mass(coords):
    return [(np.ascontiguousarray(c, dtype=np.float64), _mass(len(c))) for c in coords]


PLACES = ((0.0, 0.0, 0.0), (1e4, -1e4, 3.0), (-531.43, -83.29, -47.87))      # the last: every coordinate of the family negative
VOXELS = (1.0, 1.2, 2.0, 3.0)
RESOLUTIONS = (3.0, 5.0, 10.0)
ISOVALUES = ((0.2, 1e-8), (0.0, 1e-8), (0.05, 1e-8), (0.2, 0.3), (0.0, 0.05))
SEED = 40
SEED_FOR = {(0, 1.2, 3.0): 70, (1, 1.2, 5.0): 50, (1, 1.2, 10.0): 50}      # (place, voxel, resolution) -> seed, where SEED leaves a voxel near one of the isovalues


def family(seed, place):
    big, mid, tiny = ball(600, 14.0, seed), ball(150, 8.0, seed + 1), ball(7, 3.0, seed + 2)
    one = np.array([[0.3, -1.1, 2.2]])
    parts = [big, mid + (9.0, -4.0, 3.0), tiny + (-6.0, 5.0, 1.0), one, big.copy(), mid + (30.0, 0.0, 0.0), big + (500.0, 0.0, 0.0),
             tiny + (2.0, 2.0, -3.0)]
    return _with_mass([p + np.asarray(place) for p in parts])


def family6(seed):
    big, mid, tiny = ball(300, 10.0, seed), ball(150, 8.0, seed + 1), ball(7, 3.0, seed + 2)
    return _with_mass([big, mid + (9.0, -4.0, 3.0), tiny + (-6.0, 5.0, 1.0), np.array([[0.3, -1.1, 2.2]]), mid + (14.0, 0.5, -2.0),
                       big + (3.3, -2.1, 1.7)])


def sweep_cases():
    for place, vs, res, (d_iso, o_iso) in itertools.product(range(len(PLACES)), VOXELS, RESOLUTIONS, ISOVALUES):
        yield SEED_FOR.get((place, vs, res), SEED), place, vs, res, d_iso, o_iso


PERMUTED = ((SEED, 0) + DEFAULTS, (SEED, 2, 1.2, 3.0, 0.05, 1e-8))
SINGLE_SETTINGS = (DEFAULTS, (1.2, 3.0, 0.0, 0.05), (3.0, 10.0, 0.2, 0.3))
SINGLE_SEEDS = (40, 41, 42)


def many_small():
    """260 structures of 1 to 5 atoms: 33 670 pairs."""
    rng = np.random.default_rng(5)
    centres, counts = rng.normal(scale=3.0, size=(260, 3)), rng.integers(1, 6, size=260)
    return _with_mass([np.round(c + rng.normal(scale=1.5, size=(int(n), 3)), 3) for c, n in zip(centres, counts)])


LARGE = (0.5, 5.0, 0.2, 1e-8)
LARGE_SEED = 155
LARGE_ANGLE = 0.4


def three_poses():
    """ball(4000, 60), a rotated copy and a shifted copy: about 17 M voxels each at a voxel of 0.5."""
    a = ball(4000, 60.0, LARGE_SEED)
    c, s = np.cos(LARGE_ANGLE), np.sin(LARGE_ANGLE)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return _with_mass([a, np.round(a @ rot, 3), a + (7.0, -3.5, 11.0)])


def two_large():
    poses = three_poses()
    return [poses[0], poses[2]]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's table, computed once per case
# ---------------------------------------------------------------------------------------------------------------------

def oracle_table(structs, res, vs, d_iso, o_iso, both=False):
    """-> (table, near, geometry): the upper-triangular table of oracle.overlap_ratio between the oracle's densities (both: the
    lower triangle too, overlap(i, j) for i > j, which the device leaves 0), the number of voxels of the unthresholded densities
    within NEAR of an isovalue in use (1e-8, and a density isovalue of 0, are too small to matter), and every grid's
    (shape, origin)."""
    grids, near = [], 0
    bands = [v for v in (d_iso, o_iso) if v > 1e-7]
    for c, m in structs:
        g, x0, y0, z0 = O.structure_to_density(c, m, res, vs, isovalue=d_iso)
        grids.append((g, (x0, y0, z0)))
        if bands:
            raw = g if d_iso == 0 else O.structure_to_density(c, m, res, vs, isovalue=0.0)[0]
            for v in bands:
                close = raw[np.abs(raw - np.float32(v)) <= 2 * NEAR].astype(np.float64)      # float32 first: the grids can be large
                near += int(np.count_nonzero(np.abs(close - v) <= NEAR))
            del raw
    n = len(grids)
    table = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i < j or (both and i != j):
                table[i, j] = O.overlap_ratio(grids[i][0].copy(), grids[i][1], grids[j][0].copy(), grids[j][1], vs, o_iso)
    return table, near, [(g.shape, o) for g, o in grids]


@functools.lru_cache(maxsize=None)
def family_table(seed, place, vs, res, d_iso, o_iso, reverse=False):
    structs = family(seed, PLACES[place])
    return oracle_table(structs[::-1] if reverse else structs, res, vs, d_iso, o_iso)


@functools.lru_cache(maxsize=None)
def family6_table(seed, vs, res, d_iso, o_iso):
    return oracle_table(family6(seed), res, vs, d_iso, o_iso)


@functools.lru_cache(maxsize=None)
def many_small_table():
    vs, res, d_iso, o_iso = DEFAULTS
    return oracle_table(many_small(), res, vs, d_iso, o_iso)


@functools.lru_cache(maxsize=None)
def three_poses_table():
    """Both directions of every pair of poses; the two large structures of case 5 are poses 0 and 2 of it."""
    vs, res, d_iso, o_iso = LARGE
    return oracle_table(three_poses(), res, vs, d_iso, o_iso, both=True)


def _distinct(table):
    return len(set(table[table != 0].tolist()))


def _boxed(geom, vs):
    """Row-major list of the pairs i < j whose grids share a box of at least one voxel (structure_utils.py:181-243): the pairs
    overlap_run puts in its table, in its order."""
    out = []
    for i in range(len(geom)):
        for j in range(i + 1, len(geom)):
            (n1, o1), (n2, o2) = geom[i], geom[j]
            ok = True
            for d in range(3):
                lo1, hi1, lo2, hi2 = O._common_box(n1[d], o1[d] / vs, n2[d], o2[d] / vs)
                ok = ok and min(min(hi1, n1[d]) - lo1, min(hi2, n2[d]) - lo2) > 0
            if ok:
                out.append((i, j))
    return out


PAIRS_PER_LAUNCH = 32768      # overlap_run: gridDim.y of one launch of k_overlap_pairs


def _past_the_cut(table, geom, vs):
    boxed = _boxed(geom, vs)
    return len(boxed), np.array([table[i, j] for i, j in boxed[PAIRS_PER_LAUNCH:]])


def _chunk_counts(geom):
    """(structures in the first chunk of density_batch, structures in all) for the three poses dealt round-robin: the first chunk as
    density_batch fills it (512 Mi float64 voxels), then six more."""
    vox = [int(np.prod(shape)) for shape, _ in geom]
    cap = 512 << 20
    n = tot = 0
    while tot + vox[n % 3] <= cap:
        tot += vox[n % 3]
        n += 1
    return n, n + 6, vox


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the inputs are free of voxels on an isovalue and their tables are not vacuous
# ---------------------------------------------------------------------------------------------------------------------

def _teeth_sweep():
    changed = 0
    for case in sweep_cases():
        table, near, _ = family_table(*case)
        assert near == 0, (case, near)
        assert _distinct(table) >= 5, (case, _distinct(table))
        assert table[0, 4] == 1.0 and not table[6].any() and not table[:, 6].any(), case
        if case[5] != 1e-8:
            changed += int(np.any(table != family_table(*case[:5], 1e-8)[0]))
    assert changed >= 1      # the overlap isovalue moves entries: the clamp of k_clamp_count is seen
    for case in PERMUTED:
        fwd, near, _ = family_table(*case)
        rev, near_r, _ = family_table(*case, reverse=True)
        n = len(fwd)
        assert near == 0 and near_r == 0 and _distinct(rev) >= 5, case
        differ = sum(fwd[i, j] != rev[n - 1 - j, n - 1 - i] for i in range(n) for j in range(i + 1, n))
        assert differ >= 5, (case, differ)      # the direction matters
    for setting in SINGLE_SETTINGS:      # device against device, nothing can be near: only the floor applies
        for seed in SINGLE_SEEDS:
            assert _distinct(family6_table(seed, *setting)[0]) >= 5, (setting, seed)


def _teeth_many_small():
    table, near, geom = many_small_table()
    n_boxed, tail = _past_the_cut(table, geom, DEFAULTS[0])
    assert near == 0 and len(table) == 260
    assert n_boxed > PAIRS_PER_LAUNCH and _distinct(tail) >= 20, (n_boxed, _distinct(tail))


def _teeth_large():
    table, near, geom = three_poses_table()
    n_first, n_all, vox = _chunk_counts(geom)
    assert near == 0 and min(vox) > 15 << 20      # about 16 Mi voxels per grid: the pool index of the second passes 2^24
    assert n_first >= 6 and sum(vox[i % 3] for i in range(n_first, n_all)) <= 512 << 20
    cross = [table[i, j] for i in range(3) for j in range(3) if i != j]
    assert all(0 < v < 1 for v in cross) and len({table[i, j] for i in range(3) for j in range(i + 1, 3)}) == 3, cross


@pytest.mark.parametrize("which", [_teeth_sweep, _teeth_many_small, _teeth_large], ids=["family", "many_small", "large"])
def test_inputs_keep_their_teeth(which):
    which()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------

def _device_table(lib, structs, vs, res, d_iso, o_iso):
    return lib.overlap_matrix([c for c, _ in structs], [m for _, m in structs], resolution=res, voxsp=vs, density_isovalue=d_iso,
                              overlap_isovalue=o_iso)


@pytest.mark.gpu
def test_table_sweep_against_the_oracle(lib):
    changed = 0
    for case in sweep_cases():
        seed, place, vs, res, d_iso, o_iso = case
        want, near, _ = family_table(*case)
        assert near == 0 and _distinct(want) >= 5, case
        got = _device_table(lib, family(seed, PLACES[place]), vs, res, d_iso, o_iso)
        np.testing.assert_array_equal(got, want, err_msg=repr(case))      # lower triangle and diagonal: exactly 0 in both
        assert got[0, 4] == 1.0, case                                     # an identical copy
        assert not got[6].any() and not got[:, 6].any(), case             # 500 A away from everything
        if o_iso != 1e-8:
            changed += int(np.any(got != family_table(seed, place, vs, res, d_iso, 1e-8)[0]))
    assert changed >= 1


@pytest.mark.gpu
def test_both_directions_by_permutation(lib):
    for case in PERMUTED:
        seed, place, vs, res, d_iso, o_iso = case
        fwd = family_table(*case)[0]
        want, near, _ = family_table(*case, reverse=True)
        n = len(want)
        assert near == 0 and _distinct(want) >= 5, case
        assert sum(fwd[i, j] != want[n - 1 - j, n - 1 - i] for i in range(n) for j in range(i + 1, n)) >= 5, case
        got = _device_table(lib, family(seed, PLACES[place])[::-1], vs, res, d_iso, o_iso)
        np.testing.assert_array_equal(got, want, err_msg=repr(case))


@pytest.mark.gpu
def test_batched_table_equals_the_single_calls(lib):
    for (vs, res, d_iso, o_iso), seed in itertools.product(SINGLE_SETTINGS, SINGLE_SEEDS):
        structs = family6(seed)
        got = _device_table(lib, structs, vs, res, d_iso, o_iso)
        grids = []
        for c, m in structs:
            g, x0, y0, z0 = lib.structure_to_density(c, m, res, vs, isovalue=d_iso)
            grids.append((g, (x0, y0, z0)))
        want = np.zeros_like(got)
        for i in range(len(grids)):
            for j in range(i + 1, len(grids)):
                common, npos = lib.grid_overlap(grids[i][0].copy(), grids[i][1], grids[j][0].copy(), grids[j][1], vs, o_iso)
                assert npos > 0
                want[i, j] = common / npos
        np.testing.assert_array_equal(got, want, err_msg=repr((vs, res, d_iso, o_iso, seed)))
        assert _distinct(got) >= 5
        again = _device_table(lib, structs, vs, res, d_iso, o_iso)
        assert again.tobytes() == got.tobytes()


@pytest.mark.gpu
def test_more_pairs_than_one_launch(lib):
    vs, res, d_iso, o_iso = DEFAULTS
    want, near, geom = many_small_table()
    n_boxed, tail = _past_the_cut(want, geom, vs)
    assert near == 0
    assert n_boxed > PAIRS_PER_LAUNCH      # overlap_run launches k_overlap_pairs twice
    assert _distinct(tail) >= 20           # ... and the second launch has entries to get wrong
    got = _device_table(lib, many_small(), vs, res, d_iso, o_iso)
    assert lib.last_density_chunks() == 1
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_two_large_structures(lib):
    vs, res, d_iso, o_iso = LARGE
    table, near, geom = three_poses_table()
    assert near == 0 and min(np.prod(geom[k][0]) for k in (0, 2)) > 15 << 20
    structs = two_large()
    for a, b in ((0, 2), (2, 0)):      # both directions, by swapping the list
        assert 0 < table[a, b] < 1
        want = np.array([[0.0, table[a, b]], [0.0, 0.0]])
        np.testing.assert_array_equal(_device_table(lib, structs[::-1] if a else structs, vs, res, d_iso, o_iso), want)


@pytest.mark.gpu
def test_refusals_and_the_next_call_works(lib):
    vs, res, d_iso, o_iso = DEFAULTS
    structs = family(SEED, PLACES[0])
    before = _device_table(lib, structs, vs, res, d_iso, o_iso)
    np.testing.assert_array_equal(before, family_table(SEED, 0, vs, res, d_iso, o_iso)[0])
    atoms = np.ascontiguousarray(np.concatenate([c for c, _ in structs[:3]]))
    mass = np.ascontiguousarray(np.concatenate([m for _, m in structs[:3]]))
    first = np.zeros(4, np.int64)
    first[1:] = np.cumsum([len(c) for c, _ in structs[:3]])

    def call(n, a=atoms, m=mass, f=first, out=None, r=res, v=vs):
        out = np.full(9, 7.0) if out is None else out
        rc = lib.dll.mad_overlap_matrix(lib.ctx, _p(a), _p(m), _p(f), C.c_int(n), C.c_double(r), C.c_double(v), C.c_double(d_iso),
                                        C.c_double(o_iso), _p(out) if out is not False else None)
        return rc, out

    rc, out = call(0)
    assert rc == 0 and (out == 7.0).all()                          # a 0 x 0 table: nothing to write
    rc, out = call(1)
    assert rc == 0 and out[0] == 0.0 and (out[1:] == 7.0).all()    # a 1 x 1 table: zeroed
    EINVAL, EDOM = -22, -33
    assert call(-1)[0] == EINVAL
    assert call(3, a=None)[0] == EINVAL and call(3, m=None)[0] == EINVAL and call(3, f=None)[0] == EINVAL
    assert call(3, out=False)[0] == EINVAL
    assert call(3, v=0.0)[0] == EINVAL and call(3, r=0.0)[0] == EINVAL
    assert "voxsp" in lib.last_error()
    n = 4097
    ones, first_n = np.arange(3.0 * n).reshape(n, 3), np.arange(n + 1, dtype=np.int64)
    assert call(n, a=ones, m=_mass(n), f=first_n, out=np.zeros(n * n))[0] == EINVAL
    hole = first.copy()
    hole[2] = hole[1]      # the middle structure has no atoms
    assert call(3, f=hole)[0] == EINVAL and "no atoms" in lib.last_error()
    bad = atoms.copy()
    bad[int(first[1]) + 2, 1] = np.nan
    assert call(3, a=bad)[0] == EDOM
    assert call(3, r=94.9, v=1.0)[0] == EINVAL      # kernel radius 65
    with pytest.raises(ValueError):
        lib.overlap_matrix([c for c, _ in structs[:3]], [m for _, m in structs[:2]] + [structs[2][1][:-1]])
    rc, out = call(3)
    assert rc == 0
    np.testing.assert_array_equal(out.reshape(3, 3), before[:3, :3])
    np.testing.assert_array_equal(_device_table(lib, structs, vs, res, d_iso, o_iso), before)


@pytest.mark.gpu
def test_overlap_table_of_pdb_files(lib, tmp_path):
    files, coords, mass = [], [], []
    for k, (c, m) in enumerate(family(SEED, PLACES[0])):
        elems = [("C", "N", "O", "S")[i % 4] for i in range(len(c))]
        files.append(str(tmp_path / ("s%d.pdb" % k)))
        synth.write_pdb(files[-1], c, elems, elems)
        coords.append(np.array([[float("%8.3f" % v) for v in row] for row in c]))      # what the file holds
        mass.append(m)
        pdb = PDB(files[-1])
        np.testing.assert_array_equal(pdb.coords, coords[-1])
        np.testing.assert_array_equal(pdb.atom_masses(), m)
    got = assembly.overlap_table(files, lib=lib)
    want = lib.overlap_matrix(coords, mass, resolution=assembly.OVERLAP_RES, voxsp=assembly.OVERLAP_VOXSP,
                              density_isovalue=assembly.OVERLAP_ISO)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, family_table(SEED, 0, *DEFAULTS)[0])


@pytest.mark.gpu
def test_more_than_one_density_chunk(lib):
    """Last: about 8 GB of device scratch, like test_density_ccc_more_than_one_chunk."""
    vs, res, d_iso, o_iso = LARGE
    want, near, geom = three_poses_table()
    n_first, n_all, vox = _chunk_counts(geom)
    assert near == 0 and n_first >= 6 and sum(vox[i % 3] for i in range(n_first, n_all)) <= 512 << 20
    assert len({want[i, j] for i in range(3) for j in range(i + 1, 3)}) == 3
    poses = three_poses()
    got = _device_table(lib, [poses[i % 3] for i in range(n_all)], vs, res, d_iso, o_iso)
    assert lib.last_density_chunks() == 2
    # the 3 x 3 layout of the poses: (a, b) with a before b in the list, from the first entries on that side of the diagonal
    lay = np.zeros((3, 3))
    for i in range(6):
        for j in range(i + 1, 6):
            lay[i % 3, j % 3] = got[i, j]
    for i in range(n_all):
        for j in range(n_all):
            assert got[i, j] == (lay[i % 3, j % 3] if i < j else 0.0), (i, j, n_first, got[i, j], lay[i % 3, j % 3])
    assert lay[0, 0] == lay[1, 1] == lay[2, 2] == 1.0      # a pose against its own copy
    off = ~np.eye(3, dtype=bool)
    np.testing.assert_array_equal(lay[off], want[off])
    small = _device_table(lib, poses, vs, res, d_iso, o_iso)
    assert lib.last_density_chunks() == 1
    np.testing.assert_array_equal(small, np.triu(lay, 1))
