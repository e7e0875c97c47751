"""Fourier shell correlation of two maps and radial filters in Fourier space (section 4m): the host side.
The filters -- `filter_lattice`, `radial_gain`, the designs `gain_*` and the restatement `filter_numpy` -- have their contract
further down, and so have the translation scan (section 4n): `scan_lattice`, the restatement `scan_numpy`, `peaks_numpy` and `Scan`,
and the rotational search (section 4o): `rotation_set`, the restatements `rotate_numpy`, `tree_sum` and `search_numpy`, and `Search`,
and local resolution (section 4p): `local_plan`, `hann_window`, the restatement `local_fsc_numpy` and `LocalResolution`;
local amplitude scaling (section 4v): the restatement `local_scale_numpy`, `LocalScale`, and `scale_curve` / `gain_shells` of
`Dmap.scale_to`;
a low-pass by local resolution (section 4q): the restatements `local_sigma_numpy` and `local_filter_numpy`;
the masked curve and its phase-randomised correction (section 4s): `splitmix_u`, the restatements `randomize_numpy` and
`fsc_masked_numpy`, and `MaskedFSC`.

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


# ---------------------------------------------------------------------------
# translation scan: the contract of `mad_map_scan`
#
# A map m (float32 [x, y, z], dims d1) and n_t >= 1 templates g_j of common dims d2 <= d1 per axis, each at lattice index (0, 0, 0) of
# a cubic lattice whose edge N is the smallest power of two >= max(d1), 8 <= N <= 1024.  Offsets u in [0, D), D = d1 - d2 + 1: the
# template's box lies wholly inside the map's, so no scored offset wraps around the lattice.  Per template, w = [g > iso], g^ = g w,
# n_w = sum w, G = sum g^2, gbar = sum g^ / n_w:  C(u) = sum_x m(u + x) g^(x), E(u) = sum_x m(u + x)^2 w(x), A(u) = sum_x m(u + x) w(x).
# mode 0: score = C / sqrt(E G) where E > e_min.  mode 1: C' = C - A gbar, E' = E - A^2 / n_w, G' = G - n_w gbar^2,
# score = C' / sqrt(E' G') where E' > e_min.  best = the greatest float32 score over the templates that scored an offset, best_t the
# lowest template that attains it; 0.0 and -1 where none scored.  Spectra: M, M2 = split_pair(FFT(m + i m^2)),
# G^, W = split_pair(FFT(g^ + i w)), ifft(M conj(G^) + i M2 conj(W)) = C + i E, ifft(M conj(W)) = A.
# ---------------------------------------------------------------------------

def scan_lattice(d1, d2):
    """-> (N, D) of `mad_map_scan`: the lattice edge and the box of offsets D = d1 - d2 + 1 (int tuple).  ValueError where the
    call refuses: an empty grid, max(d1) > 1024, or a template longer than the map on an axis."""
    d1, d2 = tuple(int(v) for v in d1), tuple(int(v) for v in d2)
    if len(d1) != 3 or len(d2) != 3 or min(d1 + d2) < 1:
        raise ValueError("scan_lattice: empty grid (%r, %r)" % (d1, d2))
    if max(d1) > MAX_N:
        raise ValueError("scan_lattice: the map's longest axis is %d voxels, more than %d" % (max(d1), MAX_N))
    for a in range(3):
        if d2[a] > d1[a]:
            raise ValueError("scan_lattice: the template is %d voxels long on axis %d, the map %d" % (d2[a], a, d1[a]))
    N = MIN_N
    while N < max(d1):
        N *= 2
    return N, tuple(d1[a] - d2[a] + 1 for a in range(3))


def scan_template(g, iso):
    """-> (g^ float64, w float64, n_w, G, gbar) of one template: w = [g > iso], g^ = g w."""
    g = np.asarray(g).astype(np.float64)
    w = (g > float(iso)).astype(np.float64)
    gh = g * w
    n_w = float(w.sum())
    if n_w == 0:
        raise ValueError("scan_template: no voxel above iso = %r" % (iso,))
    return gh, w, n_w, float((gh * gh).sum()), float(gh.sum()) / n_w


def scan_inverse(m, g, iso, mode=0):
    """-> (p, q): the full inverse lattices complex128 [N, N, N] of one template, p = ifft(M conj(G^) + i M2 conj(W)) = C + i E and,
    in mode 1, q = ifft(M conj(W)) = A (else None)."""
    m = np.asarray(m).astype(np.float64)
    N, _ = scan_lattice(m.shape, np.shape(g))
    gh, w = scan_template(g, iso)[:2]
    Zm, Zt = np.zeros((N, N, N), np.complex128), np.zeros((N, N, N), np.complex128)
    Zm[:m.shape[0], :m.shape[1], :m.shape[2]] = m + 1j * (m * m)
    Zt[:gh.shape[0], :gh.shape[1], :gh.shape[2]] = gh + 1j * w
    M, M2 = split_pair(np.fft.fftn(Zm))
    Gh, W = split_pair(np.fft.fftn(Zt))
    p = np.fft.ifftn(M * np.conj(Gh) + 1j * (M2 * np.conj(W)))
    return p, (np.fft.ifftn(M * np.conj(W)) if mode else None)


def scan_numpy(m, templates, iso, e_min, mode):
    """The contract of `mad_map_scan` with numpy.fft in float64 -> (best float64 [D] before the cast to float32 -- the maximum is
    taken on the float32 values, as the device takes it --, best_t int32 [D], and per template the lists C, E (C', E' in mode 1:
    what is scored), G (G' in mode 1) and n_w).  An offset is scored by a template where E > e_min."""
    if mode not in (0, 1):
        raise ValueError("scan_numpy: mode %r (0 un-centred, 1 centred)" % (mode,))
    e_min = float(e_min)
    if not (e_min >= 0) or not np.isfinite(e_min) or not np.isfinite(float(iso)):
        raise ValueError("scan_numpy: iso %r, e_min %r (finite, e_min 0 or more)" % (iso, e_min))
    templates = list(templates)
    if len(templates) < 1:
        raise ValueError("scan_numpy: no template")
    m = np.asarray(m)
    _, D = scan_lattice(m.shape, np.shape(templates[0]))
    best, best32, best_t = np.zeros(D), np.zeros(D, np.float32), np.full(D, -1, np.int32)
    Cs, Es, Gs, ns = [], [], [], []
    for j, g in enumerate(templates):
        if np.shape(g) != np.shape(templates[0]):
            raise ValueError("scan_numpy: template %d has shape %r, template 0 %r" % (j, np.shape(g), np.shape(templates[0])))
        _, _, n_w, G, gbar = scan_template(g, iso)
        p, q = scan_inverse(m, g, iso, mode)
        C = np.ascontiguousarray(p.real[:D[0], :D[1], :D[2]])
        E = np.ascontiguousarray(p.imag[:D[0], :D[1], :D[2]])
        if mode:
            A = q.real[:D[0], :D[1], :D[2]]
            C = C - A * gbar
            E = E - (A * A) / n_w
            G = G - n_w * (gbar * gbar)
            if not G > 0:
                raise ValueError("scan_numpy: template %d is constant under its mask (G' = %r)" % (j, G))
        scored = E > e_min
        s = np.zeros(D)
        s[scored] = C[scored] / np.sqrt(E[scored] * G)
        s32 = s.astype(np.float32)
        take = scored & ((best_t < 0) | (s32 > best32))
        best[take], best32[take], best_t[take] = s[take], s32[take], j
        Cs.append(C); Es.append(E); Gs.append(G); ns.append(n_w)
    return best, best_t, Cs, Es, Gs, ns


def peaks_numpy(best, best_t, min_score, k):
    """The peaks of a score volume -> (peaks float64 [min(k, n_found), 5] = ux, uy, uz, score, template; n_found).  An offset is a
    peak when best_t >= 0, best >= min_score and every one of the 26 neighbours inside the box is smaller, or equal with a larger
    linear index; sorted by score descending, then linear index ascending."""
    best, best_t = np.asarray(best), np.asarray(best_t)
    D = best.shape
    idx = np.arange(best.size, dtype=np.int64).reshape(D)
    ok = (best_t >= 0) & (best.astype(np.float64) >= float(min_score))
    pb = np.pad(best.astype(np.float64), 1, mode="constant", constant_values=-np.inf)      # outside the box: ignored
    pi = np.pad(idx, 1, mode="constant", constant_values=-1)
    for dx in (0, 1, 2):
        for dy in (0, 1, 2):
            for dz in (0, 1, 2):
                if (dx, dy, dz) == (1, 1, 1):
                    continue
                v = pb[dx:dx + D[0], dy:dy + D[1], dz:dz + D[2]]
                j = pi[dx:dx + D[0], dy:dy + D[1], dz:dz + D[2]]
                ok &= (j < 0) | (v < best) | ((v == best) & (j > idx))
    found = idx[ok]
    order = np.lexsort((found, -best[ok].astype(np.float64)))
    found = found[order][:max(int(k), 0)]
    out = np.zeros((len(found), 5))
    out[:, 0], out[:, 1], out[:, 2] = np.unravel_index(found, D) if len(found) else ((), (), ())
    out[:, 3] = best.reshape(-1)[found]
    out[:, 4] = best_t.reshape(-1)[found]
    return out, int(ok.sum())


class _Peaks(object):
    """What `Scan` and `Search` share: `peaks` float64 [n, 5] = ux, uy, uz, score, rotation, the best first; `n_found`: how many
    peaks there are (`peaks` holds the first k); `origin`, `voxsp`: the map's; `rotations` [n, 3, 3] and `centroid`: a point x of the
    structure goes to (x - centroid) @ R + centroid + T at a peak.  A subclass says what T is (`_shift`) and where its score volume
    `best` has its origin (`_write_origin`)."""

    def __init__(self, best, peaks, n_found, origin, voxsp, rotations, centroid, N, mode):
        self.best = best
        self.peaks = np.asarray(peaks, np.float64).reshape(-1, 5)
        self.n_found = int(n_found)
        self.origin = np.asarray(origin, np.float64).reshape(3)
        self.voxsp = float(voxsp)
        self.rotations = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
        self.centroid = np.asarray(centroid, np.float64).reshape(3)
        self.N, self.mode = int(N), int(mode)

    def pose(self, i):
        """-> (rotation index, R [3, 3], T [3], score) of peak i."""
        ux, uy, uz, score, j = self.peaks[i]
        j = int(j)
        return j, self.rotations[j], self._shift(np.array([ux, uy, uz]), j), float(score)

    def place(self, i, pdb):
        """The structure at peak i: a copy of `pdb` (a `PDB`: a new `PDB` with the coordinates moved; an (n, 3) array: a new array)."""
        _, R, T, _ = self.pose(i)
        if hasattr(pdb, "get_coords"):
            import copy
            out = copy.deepcopy(pdb)
            out.set_coords((np.asarray(pdb.get_coords(), np.float64) - self.centroid) @ R + self.centroid + T)
            return out
        return (np.asarray(pdb, np.float64) - self.centroid) @ R + self.centroid + T

    def write_peaks(self, path):
        """Columns rank, ux, uy, uz (voxels), score, rotation, tx, ty, tz (Angstrom)."""
        with open(path, "w") as f:
            f.write("rank,ux,uy,uz,score,rotation,tx,ty,tz\n")
            for i in range(len(self.peaks)):
                j, _, T, score = self.pose(i)
                f.write("%d,%d,%d,%d,%.9g,%d,%.6f,%.6f,%.6f\n" % ((i,) + tuple(int(v) for v in self.peaks[i][:3]) + (score, j) + tuple(T)))

    def write(self, outname):
        """The score volume as a map (.sit / .situs: Situs, anything else MRC)."""
        from . import mapio
        mapio.write_volume(outname, np.ascontiguousarray(self.best, np.float32), tuple(self._write_origin()), self.voxsp)


class Scan(_Peaks):
    """What `Dmap.scan` returns.  `best` float32 [D]: the best score over the rotations at every whole-voxel offset; `best_t` int32
    [D]: the rotation that attains it, -1 where none was scored; `peaks`: float64 [n, 5] = ux, uy, uz, score, rotation, the best
    first; `n_found`: how many peaks there are (`peaks` holds the first k).  `origin`, `voxsp`: where offset (0, 0, 0) puts the
    template's voxel (0, 0, 0), i.e. the map's origin and spacing.  `rotations` [n, 3, 3], `centroid` and `template_origins` [n, 3]
    (the grid origin of every rotated copy's box before it is moved) turn a peak into a placement: a point x of the structure goes to
    (x - centroid) @ R + centroid + T, T = origin + u voxsp - template_origins[rotation].  `write(outname)`: the score volume as a
    map whose origin is the map's origin: the value at a voxel is the best score of the template whose voxel (0, 0, 0) is placed there."""

    def __init__(self, best, best_t, peaks, n_found, origin, voxsp, rotations, centroid, template_origins, N=0, e_min=0.0, mode=0):
        _Peaks.__init__(self, best, peaks, n_found, origin, voxsp, rotations, centroid, N, mode)
        self.best_t, self.e_min = best_t, float(e_min)
        self.template_origins = np.asarray(template_origins, np.float64).reshape(-1, 3)

    def _shift(self, u, j):
        return self.origin + u * self.voxsp - self.template_origins[j]

    def _write_origin(self):
        return self.origin


# ---------------------------------------------------------------------------
# rotational search: the contract of `mad_map_search` and `mad_map_rotate`
#
# A map m (float32 [x, y, z], dims d1), ONE base template g0 (float32, any dims d0), a centre c0 (float64 [3], in g0's voxel
# coordinates, may be fractional), a cube edge e >= 1 with e <= d1 per axis, n_r >= 1 rotations R_j (row-major 3 x 3; the library
# moves points by y = (x - c) @ R + c, so the rotated density at y is the base density at (y - c) @ R^T + c), iso, e_fill >= 0, mode,
# min_score, k.
# Rotated template: c2 = (e - 1) / 2; for the cube's voxel x, d = x - c2 and p_a = c0_a + ((d_0 R[a][0] + d_1 R[a][1]) + d_2 R[a][2]);
# f = floor(p), t = p - f; the eight corners are read from g0, a corner outside g0 is 0 (a p at or beyond -1 or d0 on an axis has no
# corner inside and gives 0); lerp(a, b, t) = a + t (b - a) along z, then y, then x; float64 in exactly this order, no fused
# multiply-add; rounded to float32: the template voxel g_j(x).  With c0 - c2 integral the identity returns g0's bits, and a rotation
# whose entries are 0 and +-1 permutes voxels.
# Mask and sums: w = [g_j > iso] in float64, n_w = sum w, G = tree_sum(g^2 w), S = tree_sum(g w) over the cube in linear [x][y][z]
# order; mode 1: gbar = S / n_w, G' = G - n_w (gbar gbar).  A rotation is skipped (scores no offset; counted, not refused) when
# n_w = 0, G is not in (0, 1.7e308] or, in mode 1, G' <= 0.
# Scores: section 4n's over D = d1 - e + 1 with the floor e_min_j = e_fill n_w_j; best, best_r and the peaks as there.
# ---------------------------------------------------------------------------

def rotation_set(angle):
    """-> float64 [n, 3, 3]: rotations such that every rotation of SO(3) lies within `angle` degrees of a member.  Member 0 is the
    identity; deterministic.  Directions on a Fibonacci spiral from pole to pole, one per hexagonal cell of side `angle`
    (n_d = ceil(4 pi / (sqrt(3) / 2 angle^2))), each reached from +z by the shortest turn, after an in-plane turn about z by
    multiples of 360 / ceil(360 / angle) degrees: member i n_t + k is Rz(k step) followed by the turn to direction i (matrices for
    row vectors, x @ R).  45 / 30 / 20 / 15 degrees give 192 / 636 / 2160 / 5088 members."""
    angle = float(angle)
    if not (0.0 < angle <= 180.0):
        raise ValueError("rotation_set: angle %r (in (0, 180] degrees)" % (angle,))
    a = np.radians(angle)
    n_d = max(int(np.ceil(4.0 * np.pi / (np.sqrt(3.0) / 2.0 * a * a))), 2)
    n_t = int(np.ceil(360.0 / angle))
    golden = np.pi * (3.0 - np.sqrt(5.0))
    out = np.zeros((n_d * n_t, 3, 3))
    for i in range(n_d):
        z = 1.0 - 2.0 * i / (n_d - 1.0)
        r = np.sqrt(max(0.0, 1.0 - z * z))
        d = np.array([r * np.cos(golden * i), r * np.sin(golden * i), z])
        if i == 0:
            A = np.eye(3)
        elif i == n_d - 1:
            A = np.diag([1.0, -1.0, -1.0])      # +z to -z: half a turn about x
        else:      # Rodrigues about z x d: the column form, +z -> d
            ax = np.array([-d[1], d[0], 0.0]) / r
            K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
            A = np.eye(3) + r * K + (1.0 - z) * (K @ K)
        for k in range(n_t):
            psi = 2.0 * np.pi * k / n_t
            c, s = (1.0, 0.0) if k == 0 else (np.cos(psi), np.sin(psi))
            Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
            M = (A @ Rz).T      # row-vector form
            u, _, vt = np.linalg.svd(M)      # the nearest rotation: orthonormal to the last bit
            out[i * n_t + k] = np.eye(3) if (i == 0 and k == 0) else u @ vt
    return out


def rotation_distance(Q, members):
    """Degrees from the rotation `Q` [3, 3] to the nearest of `members` [n, 3, 3]."""
    tr = np.einsum("ab,nab->n", np.asarray(Q, np.float64), np.asarray(members, np.float64))
    return float(np.degrees(np.arccos(np.clip((tr.max() - 1.0) / 2.0, -1.0, 1.0))))


def rotate_numpy(g0, c0, e, R):
    """The rotated template of the contract -> float32 [e, e, e]."""
    g0 = np.asarray(g0)
    g64 = g0.astype(np.float64)
    e = int(e)
    if g0.ndim != 3 or g0.size == 0 or e < 1:
        raise ValueError("rotate_numpy: a grid of shape %r, edge %r" % (g0.shape, e))
    c0, R = np.asarray(c0, np.float64).reshape(3), np.asarray(R, np.float64).reshape(3, 3)
    if not (np.isfinite(c0).all() and np.isfinite(R).all()):
        raise ValueError("rotate_numpy: c0 or R is not finite")
    c2 = (float(e) - 1.0) / 2.0
    ax = np.arange(e, dtype=np.float64) - c2
    d = [ax[:, None, None], ax[None, :, None], ax[None, None, :]]
    p = [c0[a] + ((d[0] * R[a, 0] + d[1] * R[a, 1]) + d[2] * R[a, 2]) for a in range(3)]
    inside = np.ones((e, e, e), bool)
    for a in range(3):
        inside &= (p[a] > -1.0) & (p[a] < float(g0.shape[a]))
    p = [np.where(inside, v, 0.0) for v in p]
    f = [np.floor(v) for v in p]
    t = [p[a] - f[a] for a in range(3)]
    i = [f[a].astype(np.int64) for a in range(3)]

    def corner(da, db, dc):
        x, y, z = i[0] + da, i[1] + db, i[2] + dc
        ok = (x >= 0) & (x < g0.shape[0]) & (y >= 0) & (y < g0.shape[1]) & (z >= 0) & (z < g0.shape[2])
        return np.where(ok, g64[np.clip(x, 0, g0.shape[0] - 1), np.clip(y, 0, g0.shape[1] - 1), np.clip(z, 0, g0.shape[2] - 1)], 0.0)

    def lerp(a, b, w):
        return a + w * (b - a)

    v00, v01 = lerp(corner(0, 0, 0), corner(0, 0, 1), t[2]), lerp(corner(0, 1, 0), corner(0, 1, 1), t[2])
    v10, v11 = lerp(corner(1, 0, 0), corner(1, 0, 1), t[2]), lerp(corner(1, 1, 0), corner(1, 1, 1), t[2])
    v = lerp(lerp(v00, v01, t[1]), lerp(v10, v11, t[1]), t[0])
    return np.where(inside, v, 0.0).astype(np.float32)


def tree_sum(x):
    """The fixed pairing of the contract's sums: runs of 256 consecutive elements (the last zero-padded), each summed by halving
    (x[:128] + x[128:], then 64, ... 1), and the partial sums the same way until one value is left -> float."""
    x = np.asarray(x, np.float64).reshape(-1)
    if x.size == 0:
        return 0.0
    while True:
        n = -(-x.size // 256)
        r = np.zeros(n * 256)
        r[:x.size] = x
        r = r.reshape(n, 256)
        h = 128
        while h >= 1:
            r = r[:, :h] + r[:, h:2 * h]
            h //= 2
        x = r.reshape(-1)
        if x.size == 1:
            return float(x[0])


def search_stats(g, iso, mode=0):
    """-> (n_w int, G, S, G' (G in mode 0), skipped) of one rotated template by the contract's sums."""
    g = np.asarray(g).astype(np.float64).reshape(-1)
    w = (g > float(iso)).astype(np.float64)
    n_w, G, S = int(w.sum()), tree_sum(g * g * w), tree_sum(g * w)
    skipped = n_w == 0 or not (0.0 < G <= 1.7e308)
    Gp = G
    if mode and not skipped:
        gbar = S / n_w
        Gp = G - n_w * (gbar * gbar)
        skipped = not Gp > 0.0
    return n_w, G, S, Gp, skipped


def search_numpy(m, g0, c0, e, rotations, iso, e_fill, mode):
    """The contract of `mad_map_search` through `rotate_numpy` and, per rotation, `scan_numpy` -> (best float64 [D] before the cast
    to float32 -- the maximum is taken on the float32 values --, best_r int32 [D], n_skipped, and per rotation the tuple
    (n_w, G, S, G', skipped))."""
    if mode not in (0, 1):
        raise ValueError("search_numpy: mode %r (0 un-centred, 1 centred)" % (mode,))
    e_fill = float(e_fill)
    if not (e_fill >= 0) or not np.isfinite(e_fill) or not np.isfinite(float(iso)):
        raise ValueError("search_numpy: iso %r, e_fill %r (finite, e_fill 0 or more)" % (iso, e_fill))
    rot = np.asarray(rotations, np.float64)
    if rot.ndim != 3 or rot.shape[1:] != (3, 3) or len(rot) < 1:
        raise ValueError("search_numpy: rotations of shape %r, not (n, 3, 3) with n >= 1" % (rot.shape,))
    for j, R in enumerate(rot):
        if not np.isfinite(R).all() or np.abs(R @ R.T - np.eye(3)).max() > 1e-6:
            raise ValueError("search_numpy: rotation %d is not finite or not orthonormal" % j)
    m, e = np.asarray(m), int(e)
    _, D = scan_lattice(m.shape, (e, e, e))
    best, best32, best_r = np.zeros(D), np.zeros(D, np.float32), np.full(D, -1, np.int32)
    stats, n_skipped = [], 0
    for j, R in enumerate(rot):
        g = rotate_numpy(g0, c0, e, R)
        st = search_stats(g, iso, mode)
        stats.append(st)
        if st[4]:
            n_skipped += 1
            continue
        b, bt = scan_numpy(m, [g], iso, e_fill * st[0], mode)[:2]
        b32 = b.astype(np.float32)
        take = (bt >= 0) & ((best_r < 0) | (b32 > best32))
        best[take], best32[take], best_r[take] = b[take], b32[take], j
    return best, best_r, n_skipped, stats


def search_edge(g0, c0, iso):
    """The cube edge `Dmap.search` uses: the smallest odd integer >= 2 rho + 3, rho the largest distance in voxels from `c0` to a
    voxel of `g0` above `iso` (0 where there is none): the mask of every rotation fits with a voxel to spare."""
    g0, c0 = np.asarray(g0), np.asarray(c0, np.float64).reshape(3)
    idx = np.argwhere(g0.astype(np.float64) > float(iso))
    rho = float(np.sqrt(((idx - c0) ** 2).sum(axis=1).max())) if len(idx) else 0.0
    e = int(np.ceil(2.0 * rho + 3.0))
    return e if e % 2 else e + 1


class Search(_Peaks):
    """What `Dmap.search` returns.  `best` float32 [D]: the best score over the rotations at every whole-voxel offset; `best_r` int32
    [D]: the rotation that attains it, -1 where none was scored; `peaks`: float64 [n, 5] = ux, uy, uz, score, rotation, the best
    first; `n_found`: how many peaks there are (`peaks` holds the first k); `n_skipped`: rotations whose mask was empty (or, centred,
    flat).  `rotations` [n, 3, 3], `centroid`, `origin`, `voxsp` and `edge` turn a peak into a placement: at offset u the centre of the
    cube, voxel c2 = (edge - 1) / 2, carries the centroid, so a point x of the structure goes to (x - centroid) @ R + centroid + T,
    T = origin + (u + c2) voxsp - centroid.  Peaks are whole-voxel and no finer in angle than the set's spacing.  `write(outname)`:
    the score volume as a map whose origin is the map's origin + c2 voxsp: the value at a point is the best score of the structure
    with its centroid there."""

    def __init__(self, best, best_r, peaks, n_found, n_skipped, origin, voxsp, rotations, centroid, edge, N=0, e_fill=0.0, mode=0):
        _Peaks.__init__(self, best, peaks, n_found, origin, voxsp, rotations, centroid, N, mode)
        self.best_r, self.n_skipped, self.edge, self.e_fill = best_r, int(n_skipped), int(edge), float(e_fill)

    def _shift(self, u, j):
        return self.origin + (u + (self.edge - 1.0) / 2.0) * self.voxsp - self.centroid

    def _write_origin(self):
        return self.origin + (self.edge - 1.0) / 2.0 * self.voxsp


# ---------------------------------------------------------------------------
# local resolution: the contract of `mad_map_local_fsc`
#
# Two float32 grids [x, y, z] of one spacing, placed as in section 4l: per axis d = o2 / voxsp - o1 / voxsp, s = round(d) (half to
# even), delta = d - s; grid 2's voxel j sits at grid 1's index j + s; a voxel outside either grid is 0 for that grid.  Samples at the
# grid-1 voxels p_a = step m_a, m_a = 0 .. n_a - 1, n_a = (dims1[a] - 1) // step + 1.  The box of a sample has edge w in {8, 16, 32}:
# box index n stands for voxel p - w / 2 + n on every axis.  Both grids are multiplied by (h[nx] h[ny]) h[nz],
# h[n] = 0.5 - 0.5 cos(2 pi n / w) (the cosine of the exactly reduced angle, `unit_root`): the periodic Hann window, 1 at the sample.
# Z = FFT(w1 + i w2); F1, F2 = split_pair(Z); P1, P2, C per shell 0 .. w / 2 = shell_sums(F1, F2, delta) with N = w; the curve and its
# crossing with the threshold are `FSC`'s and `FSC.resolution`'s: the first shell s >= 1 with fsc_s < thr, interpolated in frequency
# against shell s - 1 where that one is at or above thr.  Not reached: 2 voxsp and shell 0.  Not selected: 0.0 and shell -1.
# ---------------------------------------------------------------------------

LOCAL_BOXES = (8, 16, 32)


def unit_root(k, N):
    """-> (cos, sin) of 2 pi k / N with the angle reduced exactly (in integers) to [0, pi / 4] first, as the library's host tables do;
    N a power of two >= 8."""
    import math
    k, N = int(k), int(N)
    quad = N // 4
    q, m = (k // quad) & 3, k % quad
    if m <= N // 8:
        cm, sm = math.cos(2.0 * math.pi * m / N), math.sin(2.0 * math.pi * m / N)
    else:
        cm, sm = math.sin(2.0 * math.pi * (quad - m) / N), math.cos(2.0 * math.pi * (quad - m) / N)
    if m == 0:
        cm, sm = 1.0, 0.0
    return ((cm, sm), (-sm, cm), (-cm, -sm), (sm, -cm))[q]


def hann_window(w):
    """float64 [w]: h[n] = 0.5 - 0.5 cos(2 pi n / w), the periodic Hann window: exactly 0 at n = 0, 0.5 at w / 4, 1 at w / 2."""
    return np.array([0.5 - 0.5 * unit_root(n, w)[0] for n in range(int(w))])


def shell_counts(N):
    """int64 [N / 2 + 1]: the lattice points of every kept shell of an N^3 lattice."""
    sh = shell_index(N).ravel()
    return np.bincount(sh[sh <= N // 2], minlength=N // 2 + 1).astype(np.int64)


def local_plan(dims1, o1, dims2, o2, voxsp, box, step, threshold):
    """-> (n (int tuple: the sample lattice), s (int tuple: grid 2's voxel j sits at grid 1's index j + s), delta float64 [3]).
    ValueError where `mad_map_local_fsc` refuses."""
    voxsp, threshold = float(voxsp), float(threshold)
    if box not in LOCAL_BOXES:
        raise ValueError("local_plan: box %r (8, 16 or 32)" % (box,))
    if int(step) != step or step < 1:
        raise ValueError("local_plan: step %r (a whole number, 1 or more)" % (step,))
    if not (-1.0 < threshold < 1.0):
        raise ValueError("local_plan: threshold %r (inside (-1, 1))" % (threshold,))
    if not (voxsp > 0) or not np.isfinite(voxsp):
        raise ValueError("local_plan: voxsp %r (positive and finite)" % (voxsp,))
    o1, o2 = np.asarray(o1, np.float64).reshape(3), np.asarray(o2, np.float64).reshape(3)
    if not (np.isfinite(o1).all() and np.isfinite(o2).all()):
        raise ValueError("local_plan: an origin is not finite")
    if len(dims1) != 3 or len(dims2) != 3 or min(tuple(dims1) + tuple(dims2)) < 1:
        raise ValueError("local_plan: empty grid (%r, %r)" % (tuple(dims1), tuple(dims2)))
    s, delta = [], np.zeros(3)
    for a in range(3):
        d = float(o2[a]) / voxsp - float(o1[a]) / voxsp
        if not abs(d) < 1e15:
            raise ValueError("local_plan: origins %r voxels apart" % (d,))
        s.append(int(round(d)))      # python's round: half to even
        delta[a] = d - s[a]
    return tuple((int(dims1[a]) - 1) // int(step) + 1 for a in range(3)), tuple(s), delta


def local_box(g, lo, w):
    """float64 [w, w, w]: the voxels lo .. lo + w - 1 (per axis) of `g`, 0 outside it."""
    out = np.zeros((w, w, w))
    a = [max(0, -int(lo[k])) for k in range(3)]
    b = [min(w, g.shape[k] - int(lo[k])) for k in range(3)]
    if all(b[k] > a[k] for k in range(3)):
        out[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = g[lo[0] + a[0]:lo[0] + b[0], lo[1] + a[1]:lo[1] + b[1], lo[2] + a[2]:lo[2] + b[2]]
    return out


def local_fsc_numpy(g1, o1, g2, o2, voxsp, box, step, threshold, select=None):
    """The contract of `mad_map_local_fsc` with numpy.fft.fftn in float64 -> `LocalResolution` (with `sums`).  `select`: anything
    that converts to a boolean array over the sample lattice, None for every sample."""
    g1, g2 = np.asarray(g1), np.asarray(g2)
    if g1.ndim != 3 or g2.ndim != 3:
        raise ValueError("local_fsc_numpy: 3-D grids")
    n, s, delta = local_plan(g1.shape, o1, g2.shape, o2, voxsp, box, step, threshold)
    w, step, voxsp, threshold = int(box), int(step), float(voxsp), float(threshold)
    sel = np.ones(n, bool) if select is None else np.asarray(select).astype(bool).reshape(n)
    h = hann_window(w)
    H = (h[:, None, None] * h[None, :, None]) * h[None, None, :]
    count = shell_counts(w)
    res, shell, sums = np.zeros(n), np.full(n, -1, np.int32), np.zeros(n + (w // 2 + 1, 3))
    for m in np.argwhere(sel):
        lo = [step * int(m[a]) - w // 2 for a in range(3)]
        w1 = local_box(g1, lo, w) * H
        w2 = local_box(g2, [lo[a] - s[a] for a in range(3)], w) * H
        F1, F2 = split_pair(np.fft.fftn(w1 + 1j * w2))
        sm, _ = shell_sums(F1, F2, delta)
        curve = FSC(w, voxsp, sm, count)
        r, reached = curve.resolution(threshold)
        res[tuple(m)] = r
        shell[tuple(m)] = int(np.nonzero(curve.fsc[1:] < threshold)[0][0]) + 1 if reached else 0
        sums[tuple(m)] = sm
    return LocalResolution(res, shell, sums, w, step, voxsp, o1, threshold)


class LocalResolution(object):
    """What `Dmap.local_resolution` returns.  `resolution` float64 [nx, ny, nz] (Angstrom): per sample the crossing of its box's FSC
    curve with `threshold`, 2 voxsp where the curve never falls below it, 0.0 where the sample was not selected; `shell` int32: the
    crossing shell, 0 (not reached) or -1 (not selected); `reached` = shell > 0, `computed` = shell >= 0; `sums` float64
    [nx, ny, nz, box / 2 + 1, 3] = P1, P2, C per shell, or None.  Sample (i, j, k) sits at `origin` + step voxsp (i, j, k)."""

    def __init__(self, resolution, shell, sums, box, step, voxsp, origin, threshold):
        self.resolution = np.asarray(resolution, np.float64)
        self.shell = np.asarray(shell, np.int32)
        self.sums = None if sums is None else np.asarray(sums, np.float64)
        self.box, self.step, self.voxsp, self.threshold = int(box), int(step), float(voxsp), float(threshold)
        self.origin = np.asarray(origin, np.float64).reshape(3).copy()
        self.reached, self.computed = self.shell > 0, self.shell >= 0

    def curve(self, i, j, k):
        """The `FSC` of the box of sample (i, j, k); needs `sums`, and a sample that was computed."""
        if self.sums is None:
            raise ValueError("LocalResolution.curve: made without sums (ask for sums=True)")
        if not self.computed[i, j, k]:
            raise ValueError("LocalResolution.curve: sample (%d, %d, %d) was not selected" % (i, j, k))
        return FSC(self.box, self.voxsp, self.sums[i, j, k], shell_counts(self.box))

    def median(self):
        """The median resolution (Angstrom) over the samples whose curve reached the threshold; nan where none did."""
        return float(np.median(self.resolution[self.reached])) if self.reached.any() else float("nan")

    def filled(self, fill=None):
        """float64 [nx, ny, nz]: the samples with every not-computed one (shell == -1, stored as 0.0) holding `fill` (Angstrom) -- what
        `Dmap.lowpass_local` filters by.  `fill=None`: the largest computed value: samples an isovalue left out are background, and
        filtering them hardest is the cautious choice.  ValueError where nothing was computed."""
        if not self.computed.any():
            raise ValueError("LocalResolution.filled: no sample was computed")
        v = float(self.resolution[self.computed].max()) if fill is None else float(fill)
        out = self.resolution.copy()
        out[~self.computed] = v
        return out

    def to_dmap(self):
        """The resolution volume as a `Dmap` of spacing step voxsp at the map's origin (float32); `resample(like=map)` brings it
        onto the map's own lattice."""
        from .Dmap import Dmap
        d = Dmap.__new__(Dmap)
        d.grid3d = np.ascontiguousarray(self.resolution, dtype=np.float32)
        d.voxsp = self.step * self.voxsp
        d.xi, d.yi, d.zi = (float(v) for v in self.origin)
        d.xb, d.yb, d.zb = d.grid3d.shape
        d.map_name, d.name = "", "local_resolution"
        return d

    def write(self, outname):
        """The resolution volume as a map (.sit / .situs: Situs, anything else MRC) of spacing step voxsp at the map's origin."""
        from . import mapio
        mapio.write_volume(outname, np.ascontiguousarray(self.resolution, np.float32), tuple(self.origin), self.step * self.voxsp)


# ---------------------------------------------------------------------------
# local amplitude scaling: the contract of `mad_map_local_scale`
#
# Sample lattice, whole-voxel shift s, boxes and window are those of local resolution above: the corner of a sample's box is
# step m - w / 2, so box index w / 2 on every axis is the sample's own voxel, and the window is exactly 1 there.  F1, F2 =
# split_pair(fftn(w1 + 1j w2)).  Shells sh = min(shell_index(w), w / 2): the corner points beyond shell w / 2 ride with shell w / 2
# (local resolution drops them), so that a map scaled against itself comes back unchanged.  P1_s, P2_s = the sums of |F1|^2, |F2|^2
# over that binning; gain_s = sqrt(P2_s / P1_s) where P1_s > 0 and the quotient is finite, else 0.0;
# out = Re ifftn(gain[sh] F1)[w / 2, w / 2, w / 2] = (1 / w^3) sum_s gain_s D_s, D_s = sum_{k in s} Re F1(k) (-1)^(a + b + c).
# ---------------------------------------------------------------------------

def scale_shells(w):
    """int64 [w, w, w]: min(shell_index(w), w / 2), the binning of local amplitude scaling -- the corners ride with the last shell."""
    return np.minimum(shell_index(w), w // 2)


def centre_signs(w):
    """float64 [w, w, w]: (-1)^(a + b + c) = exp(2 pi i k . (w / 2, w / 2, w / 2) / w), what the inverse transform multiplies the
    point (a, b, c) by at the centre of the box."""
    p = 1.0 - 2.0 * (np.arange(w) % 2)
    return (p[:, None, None] * p[None, :, None]) * p[None, None, :]


def scale_gains(P1, P2):
    """gain = sqrt(P2 / P1) where P1 > 0 and the quotient is finite, else 0.0 (float64, any shape)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = P2 / P1
        ok = (P1 > 0) & np.isfinite(q)
        return np.where(ok, np.sqrt(np.where(ok, q, 0.0)), 0.0)


def local_scale_box(w1, w2):
    """One box of local amplitude scaling: the windowed sub-cubes w1, w2 (float64 [w, w, w]) -> (out, gains [w / 2 + 1],
    sums [w / 2 + 1, 3] = P1, P2, D per shell)."""
    w = w1.shape[0]
    F1, F2 = split_pair(np.fft.fftn(w1 + 1j * w2))
    sh, n = scale_shells(w).ravel(), w // 2 + 1
    sums = np.zeros((n, 3))
    sums[:, 0] = np.bincount(sh, (F1.real ** 2 + F1.imag ** 2).ravel(), n)
    sums[:, 1] = np.bincount(sh, (F2.real ** 2 + F2.imag ** 2).ravel(), n)
    sums[:, 2] = np.bincount(sh, (F1.real * centre_signs(w)).ravel(), n)
    gains = scale_gains(sums[:, 0], sums[:, 1])
    return float((gains * sums[:, 2]).sum() / float(w) ** 3), gains, sums


def local_scale_numpy(g1, o1, g2, o2, voxsp, box, step, select=None):
    """The contract of `mad_map_local_scale` with numpy.fft.fftn in float64 -> `LocalScale` (with `gains` and `sums`).  The lattice,
    the whole-voxel shift, the boxes and the window are `local_fsc_numpy`'s.  The sub-voxel rest `delta` of grid 2's placement is
    NOT used: it is a phase ramp on F2, and amplitudes do not see a phase ramp -- a reference placed a whole voxel plus a fraction
    off gives the bits of the whole-voxel placement.  `select`: anything that converts to a boolean array over the sample lattice,
    None for every sample."""
    g1, g2 = np.asarray(g1), np.asarray(g2)
    if g1.ndim != 3 or g2.ndim != 3:
        raise ValueError("local_scale_numpy: 3-D grids")
    n, s, _ = local_plan(g1.shape, o1, g2.shape, o2, voxsp, box, step, 0.0)
    w, step, voxsp = int(box), int(step), float(voxsp)
    sel = np.ones(n, bool) if select is None else np.asarray(select).astype(bool).reshape(n)
    h = hann_window(w)
    H = (h[:, None, None] * h[None, :, None]) * h[None, None, :]
    value, gains, sums = np.zeros(n), np.zeros(n + (w // 2 + 1,)), np.zeros(n + (w // 2 + 1, 3))
    for m in np.argwhere(sel):
        lo = [step * int(m[a]) - w // 2 for a in range(3)]
        w1 = local_box(g1, lo, w) * H
        w2 = local_box(g2, [lo[a] - s[a] for a in range(3)], w) * H
        value[tuple(m)], gains[tuple(m)], sums[tuple(m)] = local_scale_box(w1, w2)
    return LocalScale(value, sel, gains, w, step, voxsp, o1, sums=sums)


class LocalScale(object):
    """What `Dmap.scale_local` returns.  `value` float64 [nx, ny, nz]: per sample the map's density there after the sample's box
    has been given the reference's power shell by shell, 0.0 where the sample was not selected; `computed` bool; `gains` float64
    [nx, ny, nz, box / 2 + 1] (the factor every shell of the box's spectrum was multiplied by) or None; `sums` (the restatement
    alone) float64 [nx, ny, nz, box / 2 + 1, 3] = P1, P2, D per shell, or None.  Sample (i, j, k) sits at `origin` +
    step voxsp (i, j, k)."""

    def __init__(self, value, computed, gains, box, step, voxsp, origin, sums=None):
        self.value = np.asarray(value, np.float64)
        self.computed = np.asarray(computed, bool).reshape(self.value.shape)
        self.gains = None if gains is None else np.asarray(gains, np.float64)
        self.sums = None if sums is None else np.asarray(sums, np.float64)
        self.box, self.step, self.voxsp = int(box), int(step), float(voxsp)
        self.origin = np.asarray(origin, np.float64).reshape(3).copy()

    def gain(self, i, j, k):
        """-> (freq [box / 2 + 1] in 1 / Angstrom: s / (box voxsp), gain [box / 2 + 1]) of the box of sample (i, j, k); needs
        `gains`, and a sample that was computed."""
        if self.gains is None:
            raise ValueError("LocalScale.gain: made without gains (ask for gains=True)")
        if not self.computed[i, j, k]:
            raise ValueError("LocalScale.gain: sample (%d, %d, %d) was not selected" % (i, j, k))
        return np.arange(self.box // 2 + 1) / (self.box * self.voxsp), self.gains[i, j, k].copy()

    def to_dmap(self):
        """The scaled values as a `Dmap` of spacing step voxsp at the map's origin (float32).  At step 1 that is the scaled map on
        the map's own lattice; at a larger step `resample(like=map)` brings the coarser volume back onto it."""
        from .Dmap import Dmap
        d = Dmap.__new__(Dmap)
        d.grid3d = np.ascontiguousarray(self.value, dtype=np.float32)
        d.voxsp = self.step * self.voxsp
        d.xi, d.yi, d.zi = (float(v) for v in self.origin)
        d.xb, d.yb, d.zb = d.grid3d.shape
        d.map_name, d.name = "", "local_scale"
        return d

    def write(self, outname):
        """The scaled values as a map (.sit / .situs: Situs, anything else MRC) of spacing step voxsp at the map's origin."""
        from . import mapio
        mapio.write_volume(outname, np.ascontiguousarray(self.value, np.float32), tuple(self.origin), self.step * self.voxsp)


def scale_curve(curve):
    """-> (freq, gain) that brings the first map of an `FSC` to the second's power shell by shell: sqrt(power2 / power1), 0.0 where
    power1 is 0 (`scale_gains`)."""
    return curve.freq.copy(), scale_gains(curve.power1, curve.power2)


def gain_shells(f, freq, gain):
    """A per-shell curve `gain` over the equally spaced `freq` (1 / Angstrom, from 0) as a staircase: the value of the shell
    nearest to f, floor(f / freq[1] + 0.5) -- the shell `shell_index` puts a lattice point of that frequency in --, the last
    shell's beyond the curve's end."""
    f, freq, gain = np.asarray(f, np.float64), np.asarray(freq, np.float64), np.asarray(gain, np.float64)
    s = np.floor(f / freq[1] + 0.5).astype(np.int64)
    return gain[np.clip(s, 0, len(gain) - 1)]


# ---------------------------------------------------------------------------
# a low-pass by local resolution: the contract of `mad_map_local_filter`
#
# A float32 grid [x, y, z] of n voxels per axis and a float64 field of resolutions d (Angstrom) on the lattice of every step-th voxel,
# m_a = (n_a - 1) // step + 1 samples per axis.  At voxel i of an axis: j0 = min(i // step, m - 1), j1 = min(j0 + 1, m - 1),
# f = (i - j0 step) / step, 0.0 where j1 == j0 (clamped beyond the last sample).  d = trilinear, lerp(a, b, f) = a + (b - a) f along z,
# then y, then x; sigma = d / (voxsp K) voxels, K = pi sqrt(2).  R = max(1, int(4 sigma + 0.5)) -- `Dmap.smooth`'s truncation --,
# q = -0.5 / (sigma sigma), w_k = exp(q (k k)), W = w_0 + 2 (w_R + ... + w_1) summed from R down to 1.  out = S / (W W W) with
# S = sum_dx w_|dx| (sum_dy w_|dy| (sum_dz w_|dz| g[i + dx, j + dy, k + dz])), each offset ascending from -R to R, 0.0 outside the
# grid: a gather with the OUTPUT voxel's weights.  float64 throughout.
# ---------------------------------------------------------------------------

LOCAL_FILTER_MAX_SIGMA = 6.0                      # voxels: the widest Gaussian `mad_map_local_filter` takes (R <= 24)
LOCAL_FILTER_K = np.pi * np.sqrt(2.0)             # sigma (Angstrom) = d / K: the envelope of `lowpass(kind="gaussian")`


def local_radius(sigma):
    """int array: R = max(1, int(4 sigma + 0.5)) for sigma in voxels."""
    return np.maximum(1, (4.0 * np.asarray(sigma, np.float64) + 0.5).astype(np.int64))


def _local_filter_field(dims, res, step, voxsp):
    """-> (dims, res float64 [m0, m1, m2], step, voxsp) checked; ValueError where `mad_map_local_filter` refuses."""
    who = "local_filter"
    if isinstance(step, bool) or int(step) != step or step < 1:
        raise ValueError("%s: step %r (a whole number, 1 or more)" % (who, step))
    step, voxsp = int(step), float(voxsp)
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError("%s: grid of %r voxels" % (who, dims))
    if not (voxsp > 0) or not np.isfinite(voxsp):
        raise ValueError("%s: voxsp %r (positive and finite)" % (who, voxsp))
    res = np.asarray(res, np.float64)
    want = tuple((n - 1) // step + 1 for n in dims)
    if res.shape != want:
        raise ValueError("%s: rdims %r, the samples at every %d-th voxel of %r are %r" % (who, res.shape, step, dims, want))
    bad = ~(np.isfinite(res) & (res > 0))
    wide = ~bad & ~(res / (voxsp * LOCAL_FILTER_K) <= LOCAL_FILTER_MAX_SIGMA)
    for m in np.argwhere(bad | wide)[:1]:      # the first in index order, as the entry reports it
        m = tuple(int(v) for v in m)
        if bad[m]:
            raise ValueError("%s: sample %r is %r A (positive and finite)" % (who, m, float(res[m])))
        raise ValueError("%s: sample %r is %r A, a Gaussian of sigma %r voxels wide (at most %r)"
                         % (who, m, float(res[m]), float(res[m] / (voxsp * LOCAL_FILTER_K)), LOCAL_FILTER_MAX_SIGMA))
    return dims, res, step, voxsp


def local_sigma_numpy(dims, res, step, voxsp):
    """float64 [n0, n1, n2]: sigma in voxels at every voxel of a grid of `dims` from the field `res` on the lattice of every `step`-th
    voxel -- the operations of the contract in its order, so the same bits as `mad_map_local_filter`'s `sigma`."""
    dims, res, step, voxsp = _local_filter_field(dims, res, step, voxsp)
    j0, j1, f = [], [], []
    for a in range(3):
        i, m = np.arange(dims[a]), res.shape[a]
        lo = np.minimum(i // step, m - 1)
        hi = np.minimum(lo + 1, m - 1)
        j0.append(lo)
        j1.append(hi)
        f.append(np.where(hi == lo, 0.0, (i - lo * step).astype(np.float64) / float(step)))
    a, b = res[:, :, j0[2]], res[:, :, j1[2]]
    c = a + (b - a) * f[2][None, None, :]
    a, b = c[:, j0[1], :], c[:, j1[1], :]
    c = a + (b - a) * f[1][None, :, None]
    a, b = c[j0[0]], c[j1[0]]
    c = a + (b - a) * f[0][:, None, None]
    return c / (voxsp * LOCAL_FILTER_K)


def local_filter_numpy(grid, res, step, voxsp, with_abs=False):
    """The contract of `mad_map_local_filter` with numpy in float64 -> (out64, sigma), both float64 of the grid's shape; with
    `with_abs` -> (out64, sigma, A), A the same sums over |grid| (what an error bound of out64 scales with), for the price of one
    pass.  Vectorised over the voxels of one R at a time: a loop over dx and dy, the taps along z as one window per voxel summed in
    ascending order (a cumulative sum).  A voxel beyond a kernel's R is never touched."""
    g = np.asarray(grid)
    if g.ndim != 3:
        raise ValueError("local_filter: a 3-D grid")
    sigma = local_sigma_numpy(g.shape, res, step, voxsp)
    R = local_radius(sigma)
    Rm = int(R.max())
    vols = [g.astype(np.float64)] + ([np.abs(g.astype(np.float64))] if with_abs else [])
    pad = np.zeros((len(vols),) + tuple(n + 2 * Rm for n in g.shape))
    for v, vol in enumerate(vols):
        pad[v, Rm:Rm + g.shape[0], Rm:Rm + g.shape[1], Rm:Rm + g.shape[2]] = vol
    flat = pad.reshape(len(vols), -1)
    outs = np.zeros((len(vols),) + g.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in (int(v) for v in np.unique(R)):
            i, j, k = np.nonzero(R == r)
            s = sigma[i, j, k]
            q = -0.5 / (s * s)
            w = np.stack([np.exp(q * float(t * t)) for t in range(r + 1)])      # [t][voxel]
            tail = np.zeros(len(s))
            for t in range(r, 0, -1):
                tail = tail + w[t]
            W = w[0] + 2.0 * tail
            wz = np.ascontiguousarray(w[np.abs(np.arange(-r, r + 1))].T)        # [voxel][dz]
            first = ((i + Rm) * pad.shape[2] + (j + Rm)) * pad.shape[3] + (k + (Rm - r))      # of the voxel's own row: tap dz = -r
            taps = first[:, None] + np.arange(2 * r + 1)[None, :]
            sx = np.zeros((len(vols), len(s)))
            for dx in range(-r, r + 1):
                if i.max() + dx < 0 or i.min() + dx >= g.shape[0]:
                    continue      # every tap of this plane lies outside the grid for every voxel: zeros, which change no sum
                sy = np.zeros((len(vols), len(s)))
                for dy in range(-r, r + 1):
                    if j.max() + dy < 0 or j.min() + dy >= g.shape[1]:
                        continue
                    rows = np.take(flat, taps + (dx * pad.shape[2] + dy) * pad.shape[3], axis=1)      # [volume][voxel][dz]
                    rows *= wz
                    sy = sy + w[abs(dy)] * np.cumsum(rows, axis=-1, out=rows)[..., -1]
                sx = sx + w[abs(dx)] * sy
            outs[:, i, j, k] = sx / (W * W * W)
    return (outs[0], sigma, outs[1]) if with_abs else (outs[0], sigma)


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


# ---------------------------------------------------------------------------
# the masked curve and its phase-randomised correction: the contract of `mad_map_fsc_masked`
#
# Lattice, placement, delta and the phase ramp are `plan_box`'s, from the two grids alone.  The mask is placed against grid 1 by whole
# voxels, round(om / voxsp - o1 / voxsp) per axis (half to even); what is left of its offset is rounded away, so a soft edge moves by
# at most half a voxel.  It multiplies both parts of the packed lattice; lattice points outside its box become 0.
#   1. Z = FFT(g1 + i g2): the unmasked shell sums.
#   2. shell_r: given, or the lowest shell s >= 1 whose unmasked fsc (FSC's convention) is below t_r; N / 2 + 1 when there is none.
#   3. `randomize_numpy` on F1 (which = 0) and F2 (which = 1), Z = F1' + i F2'.
#   4. inverse transform, times the mask, forward: the random shell sums.
#   5. the packed lattice times the mask, forward: the masked shell sums.
# ---------------------------------------------------------------------------

_MASK64 = (1 << 64) - 1


def splitmix_u(seed, n):
    """-> (u, z): u = (z >> 11) * 2^-53 in [0, 1) and the 64-bit z itself, z = splitmix64's finaliser on
    seed + 0x9E3779B97F4A7C15 * n (mod 2^64).  `n`: an integer or an array of them; the results are float64 / uint64 arrays."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _MASK64) + np.uint64(0x9E3779B97F4A7C15) * np.asarray(n).astype(np.uint64)
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, z


def mirror_index(N):
    """int64 [N, N, N]: the flat index L' of -k for every lattice point L = (a N + b) N + c."""
    m = (N - np.arange(N)) % N
    return ((m[:, None, None] * N + m[None, :, None]) * N + m[None, None, :]).astype(np.int64)


def randomize_numpy(F, shell_r, seed, which=0):
    """The spectrum F (complex128 [N, N, N]) with new phases from shell `shell_r` on, as k_fsc_randomize makes them: where L < L'
    (the index of -k) and shell(k) >= shell_r, F(k) = |F(k)| (cos t + i sin t), t = 6.283185307179586 * u,
    u = splitmix_u(seed, 2 L + which + 1), and F(-k) = conj F(k).  Everything else -- lower shells, self-conjugate points -- is
    returned as it came."""
    F = np.array(F, np.complex128)
    N = F.shape[0]
    L = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
    Lm = mirror_index(N)
    act = (L < Lm) & (shell_index(N) >= int(shell_r))
    la, lm = L[act], Lm[act]
    flat = F.reshape(-1)
    f = flat[la]
    mag = np.sqrt(f.real * f.real + f.imag * f.imag)
    t = 6.283185307179586 * splitmix_u(seed, 2 * la + int(which) + 1)[0]
    new = mag * np.cos(t) + 1j * (mag * np.sin(t))
    flat[la] = new
    flat[lm] = np.conj(new)
    return F


def mask_lattice(N, p1, o1, mask, om, voxsp):
    """float64 [N, N, N]: the mask on the lattice whose index p1 holds grid 1's voxel (0, 0, 0); 0 outside the mask's box (no
    wrap-around)."""
    mask = np.asarray(mask)
    M = np.zeros((N, N, N))
    lo, hi, src = [], [], []
    for a in range(3):
        p = p1[a] + int(round(float(om[a]) / float(voxsp) - float(o1[a]) / float(voxsp)))
        l, h = max(p, 0), min(p + mask.shape[a], N)
        if h <= l:
            return M
        lo.append(l); hi.append(h); src.append(l - p)
    M[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = mask[src[0]:src[0] + hi[0] - lo[0], src[1]:src[1] + hi[1] - lo[1],
                                                     src[2]:src[2] + hi[2] - lo[2]].astype(np.float64)
    return M


def randomize_shell(sums, t_r):
    """The shell the 0.8 rule picks: the lowest s >= 1 whose C / sqrt(P1 P2) (0 where P1 P2 is not positive) is below t_r, else
    N / 2 + 1 (= len(sums))."""
    sums = np.asarray(sums, np.float64)
    for s in range(1, len(sums)):
        pp = sums[s, 0] * sums[s, 1]
        if (sums[s, 2] / np.sqrt(pp) if pp > 0 else 0.0) < t_r:
            return s
    return len(sums)


def fsc_masked_numpy(g1, o1, g2, o2, voxsp, mask, om, shell_r=None, t_r=0.8, seed=0):
    """The contract of `mad_map_fsc_masked` with numpy.fft in float64 -> `MaskedFSC`."""
    Z0, delta = pack_lattice(g1, o1, g2, o2, voxsp)
    N = Z0.shape[0]
    _, p1, _, _ = plan_box(np.asarray(g1).shape, o1, np.asarray(g2).shape, o2, voxsp)
    M = mask_lattice(N, p1, o1, mask, om, voxsp)
    F1, F2 = split_pair(np.fft.fftn(Z0))
    su, count = shell_sums(F1, F2, delta)
    sr = randomize_shell(su, t_r) if shell_r is None or shell_r < 0 else int(shell_r)
    Zr = randomize_numpy(F1, sr, seed, 0) + 1j * randomize_numpy(F2, sr, seed, 1)
    sr_sums, _ = shell_sums(*split_pair(np.fft.fftn(np.fft.ifftn(Zr) * M)), delta)
    sm, _ = shell_sums(*split_pair(np.fft.fftn(Z0 * M)), delta)
    return MaskedFSC(N, voxsp, su, sm, sr_sums, count, sr, seed)


class MaskedFSC(FSC):
    """What `Dmap.fsc(mask=...)` returns: an `FSC` whose `fsc` is the masked curve corrected for the mask's own contribution (Chen et
    al. 2013).  `fsc_unmasked`, `fsc_masked` and `fsc_random` are the three measured curves (each an `FSC`'s: 0 where a power is 0),
    `shell_r` the shell the phases were randomised from, `seed` the seed.  fsc = fsc_masked for s < shell_r + 2 and
    (fsc_masked - fsc_random) / (1 - fsc_random) from there on; where 1 - fsc_random is 0 the masked value stands.  `power1`,
    `power2`, `cross` and `n` are the masked sums."""

    def __init__(self, N, voxsp, sums_unmasked, sums_masked, sums_random, count, shell_r, seed=0):
        FSC.__init__(self, N, voxsp, sums_masked, count)
        self.sums_unmasked, self.sums_masked, self.sums_random = (np.array(s, np.float64).reshape(self.N // 2 + 1, 3)
                                                                  for s in (sums_unmasked, sums_masked, sums_random))
        self.fsc_masked = self.fsc
        self.fsc_unmasked = FSC(N, voxsp, sums_unmasked, count).fsc
        self.fsc_random = FSC(N, voxsp, sums_random, count).fsc
        self.shell_r, self.seed = int(shell_r), int(seed)
        self.fsc = self.corrected(self.fsc_masked, self.fsc_random, self.shell_r)

    @staticmethod
    def corrected(masked, random, shell_r):
        masked, random = np.asarray(masked, np.float64), np.asarray(random, np.float64)
        out = masked.copy()
        den = 1.0 - random
        use = (np.arange(len(masked)) >= shell_r + 2) & (den != 0) & np.isfinite(den) & np.isfinite(masked)
        out[use] = (masked[use] - random[use]) / den[use]
        return out

    def write_csv(self, path):
        """Columns shell, freq (1 / Angstrom), resolution (Angstrom; inf for shell 0), n, fsc (corrected), fsc_unmasked, fsc_masked,
        fsc_random."""
        with open(path, "w") as f:
            f.write("shell,freq,resolution,n,fsc,fsc_unmasked,fsc_masked,fsc_random\n")
            for s in range(len(self.fsc)):
                res = "inf" if s == 0 else "%.6f" % (1.0 / self.freq[s])
                f.write("%d,%.9g,%s,%d,%.9g,%.9g,%.9g,%.9g\n" % (s, self.freq[s], res, self.n[s], self.fsc[s], self.fsc_unmasked[s],
                                                              self.fsc_masked[s], self.fsc_random[s]))
