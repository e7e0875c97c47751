"""Patch sizes 20 and 24 (descriptor radius 10 and 12) without a GPU: the CPU oracle against what the REFERENCE computed at these
sizes (tests/golden/g19_patch_sizes.npz, written by tests/golden/make_golden_g19.py), a numpy model of the centred int8 encoding
the correlation of wide sets uses, the float32 candidate test in front of the exact threshold, and which patch sizes MaD.run
takes on the resident path."""
import os

import numpy as np
import pytest

from mad_amd import _lib, synth
from mad_amd.eqsp import EQSP_Sphere
from oracle import oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVELS, RAMP = 4095, (0.37e-6, 0.59e-6, 0.71e-6)      # make_golden_g19.py: the fields are stored in 12 bits and used with a tiny ramp


def load_g19():
    with np.load(os.path.join(G, "g19_patch_sizes.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def g19_gradient(g, octave):
    q = g["volq_%d" % octave]
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in q.shape], indexing="ij")
    vol = (q.astype(np.float64) / LEVELS + RAMP[0] * x + RAMP[1] * y + RAMP[2] * z).astype(np.float32)
    return synth.gradient_field(vol)


def test_fixture_is_small_and_meets_its_conditions():
    """The conditions the fixture was made under: no anchor rejected at the border; at patch 24 at least half of the rows of each
    octave hold a count above 127 (what makes the rows 'wide'); at patch 20 none does (5^3 = 125 samples per sub-region)."""
    assert os.path.getsize(os.path.join(G, "g19_patch_sizes.npz")) <= os.path.getsize(os.path.join(G, "g23_orient_describe.npz"))
    g = load_g19()
    for p in (20, 24):
        assert int(g["n_reject_%d" % p]) == 0
        for o in (1, 0):
            d = g["dsc_%d_%d" % (p, o)]
            assert len(np.unique(g["row_anchor_%d_%d" % (p, o)])) <= len(g["coords_%d_%d" % (p, o)]) == 12
            wide_rows = int((d.max(axis=1) > 127).sum())
            print("patch %d octave %d: %d rows, %d with a count above 127, max %d" % (p, o, len(d), wide_rows, d.max()))
            if p == 24:
                assert 2 * wide_rows >= len(d) and d.max() <= 216
            else:
                assert wide_rows == 0 and d.max() <= 125


@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("patch", [20, 24])
def test_oracle_reproduces_the_reference(patch, octave):
    g = load_g19()
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    grad = g19_gradient(g, octave)
    key = "_%d_%d" % (patch, octave)
    coords = g["coords" + key]
    got = O.orient(grad[..., 0], grad[..., 1], grad[..., 2], octave, coords, e112.sphere_eqsp, e112.p_centers_eqsp, r=patch // 2,
                   want_counts=False)
    assert got["n_reject"] == 0
    np.testing.assert_array_equal(got["anchor"], g["row_anchor" + key])
    np.testing.assert_array_equal(got["main"], g["row_main" + key])
    np.testing.assert_array_equal(got["sec"], g["row_sec" + key])
    np.testing.assert_allclose(np.asarray(got["R"]).reshape(-1, 3, 3), g["row_R" + key], rtol=0, atol=1e-14)
    dsc = O.describe(grad[..., 0], grad[..., 1], grad[..., 2], octave, coords[g["row_anchor" + key]], g["row_R" + key], e16.sphere_eqsp,
                     r=patch // 2)
    np.testing.assert_array_equal(dsc, g["dsc" + key])


# ---------------------------------------------------------------------------------------------------------------------------------
# the centred encoding (csrc/mad_common.h, MAD_WIDE_*): int8 rows of count - c, an int32 bias per row, the true dot product restored
# ---------------------------------------------------------------------------------------------------------------------------------
C8, D = _lib.WIDE_C, 1024


def encode(rows):
    rows = np.asarray(rows, np.int64)
    assert rows.min() >= 0 and rows.max() <= _lib.WIDE_MAX
    cen = rows - C8
    assert cen.min() >= -128 and cen.max() <= 127
    bias = C8 * rows.sum(axis=1) - (D // 2) * C8 * C8
    assert np.abs(bias).max() < 2 ** 31
    return cen.astype(np.int8), bias.astype(np.int32)


def pad_row():
    """What pads a set to a multiple of 128 rows, and what a dead row becomes: all -c, the bias of sum 0."""
    return np.full((1, D), -C8, np.int8), np.array([-(D // 2) * C8 * C8], np.int32)


def decode_dot(h8, hb, l8, lb):
    acc = h8.astype(np.int64) @ l8.astype(np.int64).T            # what the int8 matrix cores accumulate (int32 on the device)
    assert np.abs(acc).max() < 2 ** 31
    out = acc + hb.astype(np.int64)[:, None] + lb.astype(np.int64)[None, :]
    assert np.abs(out).max() < 2 ** 31                           # ... and every intermediate stays inside int32 in either order of the adds
    assert np.abs(acc + hb.astype(np.int64)[:, None]).max() < 2 ** 31 and np.abs(acc + lb.astype(np.int64)[None, :]).max() < 2 ** 31
    return out


def adversarial_rows():
    rows = []
    one_zone = np.zeros((64, 16), np.int64)
    one_zone[:, 3] = 216                      # all 216 samples of every region in one zone
    rows.append(one_zone.reshape(-1))
    other = np.zeros((64, 16), np.int64)
    other[:, 11] = 216                        # ... in another zone: true dot product 0 with the first
    rows.append(other.reshape(-1))
    rows.append(np.zeros(D, np.int64))        # nothing counted (every sample below the magnitude cut)
    rows.append(np.full(D, _lib.WIDE_MAX, np.int64))      # the largest row a load accepts
    spread = np.zeros((64, 16), np.int64)
    spread[:, :] = 13
    spread[:, 0] = 21                         # 216 samples spread evenly
    rows.append(spread.reshape(-1))
    return np.array(rows)


def test_centred_encoding_gives_the_exact_dot_product():
    rng = np.random.default_rng(19)
    rand = np.zeros((40, 64, 16), np.int64)
    for r in range(40):                       # rows as k_describe makes them: up to 216 samples per region over 16 zones
        for s in range(64):
            n = int(rng.integers(150, 217))
            rand[r, s] = np.bincount(rng.choice(16, size=n, p=rng.dirichlet(np.full(16, 0.3))), minlength=16)
    rows = np.concatenate([adversarial_rows(), rand.reshape(40, -1)])
    assert rows.max() > 127
    h8, hb = encode(rows)
    p8, pb = pad_row()
    a8, ab = np.concatenate([h8, p8]), np.concatenate([hb, pb])
    got = decode_dot(a8, ab, a8, ab)
    want = np.concatenate([rows, np.zeros((1, D), np.int64)])
    want = want @ want.T
    np.testing.assert_array_equal(got, want)
    assert (got[-1] == 0).all() and (got[:, -1] == 0).all()      # the pad row: true dot product 0 with everything, itself included
    assert got[0, 1] == 0 and got[0, 0] == 64 * 216 * 216 and got.max() == D * _lib.WIDE_MAX ** 2 < 2 ** 31


def test_float32_candidate_test_flags_a_superset_of_the_exact_threshold():
    """The GEMM's epilogue flags an entry when float32(dot) > float32(|h|) * (float32(cc |l|) (1 - 4e-6)) and only flagged entries see
    the float64 test dot / (|h| |l|) > cc.  Rows are built so that dot / (|h| |l|) sits within 1e-7 relative of cc, on both sides:
    every entry the float64 test passes must be flagged.  (Each float32 operation rounds by at most 2^-24 = 6e-8 relative: one for
    the dot product -- it passes 2^24 at these counts --, one per norm, two for cc |l| (1 - margin), one for the product: under
    4e-7 in all, a tenth of the margin.)"""
    rng = np.random.default_rng(24)
    f32 = np.float32
    n_close = n_true = 0
    for trial in range(4000):
        # a pair of wide-range rows: sparse large counts, so that dot, |h|^2 and |l|^2 are large integers (dot up to ~4e7 > 2^24)
        h = np.zeros(D, np.int64)
        l = np.zeros(D, np.int64)
        idx = rng.choice(D, size=int(rng.integers(64, 400)), replace=False)
        h[idx] = rng.integers(1, 217, size=len(idx))
        l[idx] = np.clip(h[idx] + rng.integers(-40, 41, size=len(idx)), 0, 216)
        extra = rng.choice(D, size=64, replace=False)
        l[extra] = rng.integers(0, 217, size=64)
        dot = int(h @ l)
        nh, nl = np.sqrt(float(h @ h)), np.sqrt(float(l @ l))
        if dot == 0 or nh == 0 or nl == 0:
            continue
        score = dot / (nh * nl)
        for rel in (-1e-7, -3e-8, -1e-9, 0.0, 1e-9, 3e-8, 1e-7):      # thresholds a hair below, at and above the score
            cc = score * (1.0 + rel)
            exact = dot / (nh * nl) > cc                        # MaD.py:423 in float64
            v = f32(cc * nl)                                    # sN[column] = (float)(cc * |l|)
            tl = f32(v - f32(f32(abs(v)) * f32(4e-6)))          # v - fabsf(v) * 4e-6f
            flagged = f32(dot) > f32(f32(nh) * tl)              # (float)acc > thv * tl
            n_close += 1
            n_true += bool(exact)
            assert flagged or not exact, (dot, nh, nl, cc)
            assert flagged                                      # within 1e-7 of the threshold the 4e-6 margin flags either side
        assert dot < 2 ** 31
    assert n_close > 20000 and 0 < n_true < n_close
    assert D * 216 ** 2 > 2 ** 24                               # the dot products of wide rows do pass float32's integer range


def test_resident_path_takes_the_even_radii_up_to_12():
    from mad_amd.MaD import MaD
    for p in (4, 8, 12, 16, 17, 20, 21, 24, 25):
        assert MaD.resident_unsupported(p) is None, p
    for p in (10, 22, 26, 2, 14):
        msg = MaD.resident_unsupported(p)
        assert msg is not None and "radius %d" % (p // 2) in msg, (p, msg)
