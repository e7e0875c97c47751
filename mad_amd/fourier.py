"""Fourier shell correlation of two maps and radial filters in Fourier space (section 4m): the host side.
The filters -- `filter_lattice`, `radial_gain`, the designs `gain_*` and the restatement `filter_numpy` -- have their contract
further down.

`plan_box` puts two grids of one spacing onto a common cubic lattice, `fsc_numpy` restates the contract of `mad_map_fsc` with
`numpy.fft.fftn` in float64 -- the checker of the GPU tests, and the one place the contract is spelled out in code -- and `FSC` is
what `Dmap.fsc` returns: the curve, the resolution at a threshold and a CSV writer.  Nothing here touches the device.

The contract.  Per axis, d = o2 / voxsp - o1 / voxsp, s = round(d) (half to even, `mad_map_mask`'s offset), delta = d - s in
[-0.5, 0.5].  The lattice begins min(0, s) voxels from grid 1's origin: grid 1 sits at index -min(0, s), grid 2 at s - min(0, s);
N is the smallest power of two >= the extent of the union box, 8 <= N <= 1024.  Z = FFT(g1 + i g2) over the zero-padded lattice
(forward, unnormalised, exp(-2 pi i k n / N)), F1(k) = (Z(k) + conj Z(-k)) / 2, F2(k) = (Z(k) - conj Z(-k)) / (2i).  A lattice
index a stands for the frequency i = a if a < N / 2 else a - N; the shell of (i, j, k) is floor(sqrt(i^2 + j^2 + k^2) + 0.5),
shells 0 .. N / 2 are kept.  Per shell P1 = sum |F1|^2, P2 = sum |F2|^2, C = sum Re(F1 conj(F2 phi)) with
phi = phi_x[a] phi_y[b] phi_z[c], phi_x[a] = exp(-2 pi i (i delta_x) / N): the ramp that moves grid 2 by its sub-voxel offset.
"""
import numpy as np

MIN_N, MAX_N = 8, 1024


def plan_box(dims1, o1, dims2, o2, voxsp):
    """-> (N, place1, place2, delta): the lattice edge, the lattice index of voxel (0, 0, 0) of either grid (int tuples) and the
    fractional offset of grid 2 in voxels (float64 array).  ValueError where `mad_map_fsc` refuses."""
    voxsp = float(voxsp)
    if not (voxsp > 0) or not np.isfinite(voxsp):
        raise ValueError("plan_box: voxsp %r (positive and finite)" % (voxsp,))
    o1, o2 = np.asarray(o1, np.float64).reshape(3), np.asarray(o2, np.float64).reshape(3)
    if not (np.isfinite(o1).all() and np.isfinite(o2).all()):
        raise ValueError("plan_box: an origin is not finite")
    place1, place2, delta, extent = [], [], np.zeros(3), 0
    for a in range(3):
        n1, n2 = int(dims1[a]), int(dims2[a])
        if n1 < 1 or n2 < 1:
            raise ValueError("plan_box: empty grid")
        d = float(o2[a]) / voxsp - float(o1[a]) / voxsp
        if not abs(d) < 1e15:
            raise ValueError("plan_box: origins %r voxels apart" % (d,))
        s = int(round(d))      # python's round: half to even
        lo = min(0, s)
        place1.append(-lo)
        place2.append(s - lo)
        delta[a] = d - s
        extent = max(extent, n1 - lo, n2 + s - lo)
    N = MIN_N
    while N < extent and N <= MAX_N:
        N *= 2
    if N > MAX_N:
        raise ValueError("plan_box: the union box is %d voxels long, more than %d" % (extent, MAX_N))
    return N, tuple(place1), tuple(place2), delta


def frequencies(N):
    """Signed frequency of every lattice index: a for a < N / 2, else a - N (the range [-N / 2, N / 2))."""
    a = np.arange(N)
    return np.where(a < N // 2, a, a - N)


def shell_index(N):
    """int64 [N, N, N]: floor(sqrt(i^2 + j^2 + k^2) + 0.5) of every lattice point."""
    f = frequencies(N).astype(np.float64)
    r2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, :] ** 2
    return np.floor(np.sqrt(r2) + 0.5).astype(np.int64)


def phase_tables(N, delta):
    """complex128 [3, N]: exp(-2 pi i (i delta_a) / N) per axis."""
    f = frequencies(N).astype(np.float64)
    ang = 2.0 * np.pi * (f[None, :] * np.asarray(delta, np.float64).reshape(3, 1)) / N
    return np.cos(ang) - 1j * np.sin(ang)


def pack_lattice(g1, o1, g2, o2, voxsp):
    """-> (complex128 [N, N, N] holding grid 1 in the real and grid 2 in the imaginary part, delta).  `g2` None: grid 1 alone."""
    g1 = np.asarray(g1)
    if g2 is None:
        N, p1, p2, delta = plan_box(g1.shape, o1, (1, 1, 1), o1, voxsp)
    else:
        g2 = np.asarray(g2)
        N, p1, p2, delta = plan_box(g1.shape, o1, g2.shape, o2, voxsp)
    Z = np.zeros((N, N, N), np.complex128)
    Z[p1[0]:p1[0] + g1.shape[0], p1[1]:p1[1] + g1.shape[1], p1[2]:p1[2] + g1.shape[2]] += g1.astype(np.float64)
    if g2 is not None:
        Z[p2[0]:p2[0] + g2.shape[0], p2[1]:p2[1] + g2.shape[1], p2[2]:p2[2] + g2.shape[2]] += 1j * g2.astype(np.float64)
    return Z, delta


def split_pair(Z):
    """The spectra of the real and of the imaginary part of the signal whose transform is Z: F1 = (Z(k) + conj Z(-k)) / 2,
    F2 = (Z(k) - conj Z(-k)) / (2i)."""
    Zm = Z
    for ax in range(Z.ndim):
        Zm = np.roll(np.flip(Zm, ax), 1, ax)      # index (N - a) % N on every axis
    Zm = np.conj(Zm)
    return (Z + Zm) / 2.0, (Z - Zm) / 2.0j


def shell_sums(F1, F2, delta, ramp=True):
    """-> (sums float64 [N / 2 + 1, 3] = P1, P2, C; count int64 [N / 2 + 1])."""
    N = F1.shape[0]
    sh = shell_index(N).ravel()
    keep = sh <= N // 2
    sh = sh[keep]
    if ramp:
        ph = phase_tables(N, delta)
        F2p = F2 * ((ph[0][:, None, None] * ph[1][None, :, None]) * ph[2][None, None, :])
    else:
        F2p = F2
    n = N // 2 + 1
    sums = np.zeros((n, 3))
    sums[:, 0] = np.bincount(sh, (F1.real ** 2 + F1.imag ** 2).ravel()[keep], n)
    sums[:, 1] = np.bincount(sh, (F2.real ** 2 + F2.imag ** 2).ravel()[keep], n)
    sums[:, 2] = np.bincount(sh, (F1 * np.conj(F2p)).real.ravel()[keep], n)
    return sums, np.bincount(sh, minlength=n).astype(np.int64)


def fsc_numpy(g1, o1, g2, o2, voxsp, ramp=True):
    """The contract of `mad_map_fsc` with numpy.fft.fftn in float64 -> `FSC`.  `ramp=False` leaves the phase ramp out (what the
    curve looks like when the sub-voxel offset is rounded away)."""
    Z, delta = pack_lattice(g1, o1, g2, o2, voxsp)
    F1, F2 = split_pair(np.fft.fftn(Z))
    sums, count = shell_sums(F1, F2, delta, ramp)
    return FSC(Z.shape[0], voxsp, sums, count)


# ---------------------------------------------------------------------------
# radial filters: the contract of `mad_map_filter`
#
# One or two float32 grids [x, y, z], each placed at lattice index (0, 0, 0) -- a radial filter is shift-invariant, the grids need
# no common frame.  N is the smallest power of two >= max(all dims) + pad, 8 <= N <= 1024; pad >= 0 is the zero margin between
# the far face of the box and its near face on the circular lattice.  Z = FFT(g1 + i g2); Z(k) *= gain[r2], r2 = i^2 + j^2 + k^2
# over the signed frequencies, a float64 table of 3 (N / 2)^2 + 1 entries; the inverse transform's real part over grid 1's box is
# the filtered grid 1, its imaginary part over grid 2's box the filtered grid 2 (the gain is real and even).
# ---------------------------------------------------------------------------

def filter_lattice(dims, pad=0, dims2=None):
    """-> N of `mad_map_filter` for grids of `dims` (and `dims2`) with `pad` voxels of zero margin.  ValueError beyond 1024."""
    pad = int(pad)
    if pad < 0:
        raise ValueError("filter_lattice: pad %d (0 or more)" % pad)
    longest = max(int(v) for v in tuple(dims) + (tuple(dims2) if dims2 is not None else ()))
    if min(int(v) for v in tuple(dims) + (tuple(dims2) if dims2 is not None else ())) < 1:
        raise ValueError("filter_lattice: empty grid")
    if longest + pad > MAX_N:
        raise ValueError("filter_lattice: the longest axis and the pad are %d + %d voxels, more than %d" % (longest, pad, MAX_N))
    N = MIN_N
    while N < longest + pad:
        N *= 2
    return N


def gain_len(N):
    """Entries of the gain table of a lattice of edge N: r2 = 0 .. 3 (N / 2)^2."""
    return 3 * (N // 2) ** 2 + 1


def radial_gain(N, voxsp, fn):
    """float64 [gain_len(N)]: `fn` evaluated at f = sqrt(r2) / (N voxsp) (1 / Angstrom) for every r2.  ValueError where the
    result is not finite (what `mad_map_filter` refuses)."""
    voxsp = float(voxsp)
    if not (voxsp > 0) or not np.isfinite(voxsp):
        raise ValueError("radial_gain: voxsp %r (positive and finite)" % (voxsp,))
    f = np.sqrt(np.arange(gain_len(N), dtype=np.float64)) / (N * voxsp)
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(fn(f), np.float64), f.shape))
    if not np.isfinite(g).all():
        raise ValueError("radial_gain: the gain is not finite at r2 = %d" % int(np.nonzero(~np.isfinite(g))[0][0]))
    return g


def gain_gaussian(f, d):
    """exp(-(f d)^2): the transform of the Gaussian `structure_to_density` blurs atoms with at resolution d, sigma = d / (pi sqrt 2)
    Angstrom.  A map low-passed to d and a model simulated at d carry the same envelope."""
    f = np.asarray(f, np.float64)
    return np.exp(-(f * d) ** 2)


def gain_cosine(r, r_c, w):
    """A raised-cosine edge in lattice units, r = sqrt(r2), r_c = N voxsp / d: 1 for r <= r_c - w / 2, 0 for r >= r_c + w / 2,
    0.5 + 0.5 cos(pi (r - (r_c - w / 2)) / w) between; w = 0 is the top hat (1 for r <= r_c)."""
    r = np.asarray(r, np.float64)
    if w == 0:
        return np.where(r <= r_c, 1.0, 0.0)
    lo = r_c - w / 2.0
    t = np.clip((r - lo) / w, 0.0, 1.0)
    return np.where(r <= lo, 1.0, np.where(r >= r_c + w / 2.0, 0.0, 0.5 + 0.5 * np.cos(np.pi * t)))


def gain_bfactor(f, B):
    """exp(-B f^2 / 4): a temperature factor of B square Angstrom applied; negative B sharpens."""
    f = np.asarray(f, np.float64)
    return np.exp(-B * f * f / 4.0)


def gain_curve(f, freq, gain):
    """A tabulated curve `gain` over `freq` (1 / Angstrom, increasing), interpolated linearly and constant beyond its ends."""
    return np.interp(np.asarray(f, np.float64), np.asarray(freq, np.float64), np.asarray(gain, np.float64))


def r2_index(N):
    """int64 [N, N, N]: i^2 + j^2 + k^2 of every lattice point, the index into a gain table."""
    f = frequencies(N).astype(np.int64)
    return f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, :] ** 2


def filter_numpy(g1, gain, pad=0, g2=None):
    """The contract of `mad_map_filter` with numpy.fft in float64 -> the filtered grid 1 (with `g2`: both) as float64, before the
    cast to float32: pack, fftn, multiply by gain[r2], ifftn, real / imaginary part, crop."""
    g1 = np.asarray(g1)
    g2 = None if g2 is None else np.asarray(g2)
    N = filter_lattice(g1.shape, pad, None if g2 is None else g2.shape)
    gain = np.asarray(gain, np.float64).reshape(-1)
    if len(gain) != gain_len(N):
        raise ValueError("filter_numpy: a gain table of %d entries, the %d^3 lattice needs %d" % (len(gain), N, gain_len(N)))
    Z = np.zeros((N, N, N), np.complex128)
    Z[:g1.shape[0], :g1.shape[1], :g1.shape[2]] = g1.astype(np.float64)
    if g2 is not None:
        Z[:g2.shape[0], :g2.shape[1], :g2.shape[2]] += 1j * g2.astype(np.float64)
    Y = np.fft.ifftn(np.fft.fftn(Z) * gain[r2_index(N)])
    out1 = np.ascontiguousarray(Y.real[:g1.shape[0], :g1.shape[1], :g1.shape[2]])
    if g2 is None:
        return out1
    return out1, np.ascontiguousarray(Y.imag[:g2.shape[0], :g2.shape[1], :g2.shape[2]])


class FSC(object):
    """A Fourier shell correlation curve: `N`, `voxsp`, and per shell 0 .. N / 2 `freq` (1 / Angstrom: s / (N voxsp)), `n` (lattice
    points), `power1`, `power2`, `cross` and `fsc` = cross / sqrt(power1 power2), 0 where power1 power2 == 0."""

    def __init__(self, N, voxsp, sums, count):
        self.N, self.voxsp = int(N), float(voxsp)
        sums = np.asarray(sums, np.float64).reshape(self.N // 2 + 1, 3)
        self.n = np.asarray(count, np.int64).reshape(self.N // 2 + 1)
        self.power1, self.power2, self.cross = sums[:, 0].copy(), sums[:, 1].copy(), sums[:, 2].copy()
        self.freq = np.arange(self.N // 2 + 1) / (self.N * self.voxsp)
        pp = self.power1 * self.power2
        ok = pp > 0
        self.fsc = np.zeros(len(pp))
        self.fsc[ok] = self.cross[ok] / np.sqrt(pp[ok])

    def resolution(self, threshold=0.143):
        """-> (Angstrom, reached): the first shell s >= 1 with fsc < threshold, interpolated linearly in frequency between shells
        s - 1 and s; (2 voxsp, False) when the curve never falls below the threshold."""
        below = np.nonzero(self.fsc[1:] < threshold)[0]
        if len(below) == 0:
            return 2.0 * self.voxsp, False
        s = int(below[0]) + 1
        a, b = self.fsc[s - 1], self.fsc[s]
        f = self.freq[s]
        if a >= threshold:      # (else shell s - 1 is below already, which only shell 0 can be: the crossing is taken at shell s)
            f = self.freq[s - 1] + (self.freq[s] - self.freq[s - 1]) * ((a - threshold) / (a - b))
        return 1.0 / f, True

    def write_csv(self, path):
        """Columns shell, freq (1 / Angstrom), resolution (Angstrom; inf for shell 0), n, fsc."""
        with open(path, "w") as f:
            f.write("shell,freq,resolution,n,fsc\n")
            for s in range(len(self.fsc)):
                res = "inf" if s == 0 else "%.6f" % (1.0 / self.freq[s])
                f.write("%d,%.9g,%s,%d,%.9g\n" % (s, self.freq[s], res, self.n[s], self.fsc[s]))
