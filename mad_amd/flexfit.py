"""Flexible fitting: atoms moved up the map's gradient on an elastic network.

`Dmap.flex_fit` runs on the device (`mad_flex_network`, `mad_flex_fit`); there is no CPU path.  `network_numpy` and
`flex_fit_numpy` restate the contract with numpy, statement by statement, for the tests: they are slow and nothing in the
package calls them.
"""
import copy

import numpy as np

from . import fourier
from .jointfit import _gather, _map_args

BATCH = 4              # FX_BATCH of csrc/mad_flexfit_plan.h: steps between two looks at the displacement
MAX_DEGREE = 128       # MAD_FLEX_MAX_DEGREE of include/mad_amd.h (a convention: all-atom protein has 45 - 80 neighbours within 6 A)


# -- arguments ---------------------------------------------------------------------------------------------------------------
def atoms_of(who, structure):
    """`structure` -- a PDB, an (n, 3) array, or a list / tuple of those -- as (coords (N, 3) float64 of all of them, first_atom
    (parts + 1), [the PDB or None per part])."""
    if hasattr(structure, "get_coords") or (not isinstance(structure, (list, tuple)) and np.ndim(structure) == 2):
        structure = [structure]
    if not isinstance(structure, (list, tuple)) or len(structure) == 0:
        raise ValueError("%s: structure must be a PDB, an (n, 3) array or a non-empty list of those" % who)
    parts, src = [], []
    for b, s in enumerate(structure):
        pdb = s if hasattr(s, "get_coords") else None
        c = np.array(pdb.get_coords() if pdb is not None else s, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != 3 or len(c) == 0:
            raise ValueError("%s: structure: part %d has coordinates of shape %s, not (n, 3)" % (who, b, c.shape))
        parts.append(c); src.append(pdb)
    first = np.zeros(len(parts) + 1, np.int64)
    first[1:] = np.cumsum([len(c) for c in parts])
    return np.ascontiguousarray(np.concatenate(parts, axis=0)), first, src


def check_steps(who, cutoff, stiffness, n_steps, max_step, min_step):
    if cutoff is not None and not (cutoff > 0.0 and np.isfinite(cutoff)):
        raise ValueError("%s: cutoff %r (positive)" % (who, cutoff))
    if not (stiffness >= 0.0 and np.isfinite(stiffness)):
        raise ValueError("%s: stiffness %r (0 or more)" % (who, stiffness))
    if int(n_steps) != n_steps or n_steps < 1:
        raise ValueError("%s: n_steps %r (1 or more)" % (who, n_steps))
    if not (0.0 < min_step <= max_step and np.isfinite(max_step)):
        raise ValueError("%s: steps: 0 < min_step <= max_step, not %r and %r" % (who, min_step, max_step))


def check_network(who, n, network):
    """A caller's network (first, nbr, rest) as mad_flex_fit takes it -> the three arrays (int32, int32, float64)."""
    if not isinstance(network, (list, tuple)) or len(network) != 3:
        raise ValueError("%s: network must be (first, nbr, rest)" % who)
    first, nbr, rest = np.asarray(network[0]), np.asarray(network[1]), np.asarray(network[2], np.float64)
    if first.shape != (n + 1,) or first[0] != 0 or np.any(np.diff(first) < 0):
        raise ValueError("%s: network: first must ascend from 0 over %d + 1 entries" % (who, n))
    if nbr.shape != (int(first[-1]),) or rest.shape != nbr.shape:
        raise ValueError("%s: network: nbr and rest must hold first[-1] = %d entries" % (who, int(first[-1])))
    first, nbr = first.astype(np.int32), nbr.astype(np.int32)
    owner = np.repeat(np.arange(n), np.diff(first))
    if np.any(nbr < 0) or np.any(nbr >= n) or np.any(nbr == owner):
        raise ValueError("%s: network: a neighbour is out of range or the atom itself" % who)
    inner = np.ones(len(nbr), bool)
    inner[first[:-1][np.diff(first) > 0]] = False      # the first entry of every row
    if np.any(nbr[1:][inner[1:]] <= nbr[:-1][inner[1:]]):
        raise ValueError("%s: network: a row does not ascend" % who)
    if not np.all(np.isfinite(rest)) or np.any(rest <= 0.0):
        raise ValueError("%s: network: rest lengths must be finite and positive" % who)
    return first, nbr, rest


# -- the numpy restatement ---------------------------------------------------------------------------------------------------
def network_numpy(coords, cutoff, max_degree=MAX_DEGREE):
    """Every pair with (dx dx + dy dy) + dz dz <= cutoff cutoff (float64, dx = x_j - x_i) is a spring -> (first int32 [n + 1],
    nbr int32 in ascending atom index per row, rest float64 = sqrt of that sum).  Brute force, a block of rows at a time."""
    x = np.asarray(coords, np.float64).reshape(-1, 3)
    n = len(x)
    if n < 1 or not np.all(np.isfinite(x)):
        raise ValueError("network_numpy: coords must be finite (n, 3) with n >= 1")
    if not cutoff > 0.0:
        raise ValueError("network_numpy: cutoff %r (positive)" % cutoff)
    c2 = cutoff * cutoff
    deg, rows, rests = np.zeros(n, np.int64), [], []
    for i0 in range(0, n, 512):
        i1 = min(n, i0 + 512)
        dx = x[None, :, 0] - x[i0:i1, None, 0]
        dy = x[None, :, 1] - x[i0:i1, None, 1]
        dz = x[None, :, 2] - x[i0:i1, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        near = d2 <= c2
        near[np.arange(i1 - i0), np.arange(i0, i1)] = False
        deg[i0:i1] = near.sum(axis=1)
        ii, jj = np.nonzero(near)      # row-major: ascending j within a row
        rows.append(jj); rests.append(np.sqrt(d2[ii, jj]))
    if deg.max() > max_degree:
        i = int(np.argmax(deg > max_degree))
        raise ValueError("network_numpy: atom %d has %d neighbours within cutoff = %g (%d at most)" % (i, deg[i], cutoff, max_degree))
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum(deg)
    return first, np.concatenate(rows).astype(np.int32), np.concatenate(rests)


def _length(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def forces_numpy(tex, origin, vs, x, w, g0, network, stiffness):
    """F_i = (w_i g_i) / g0 + sum over j in nbr(i), ascending, of ((stiffness (d - d0)) / d) (x_j - x_i); g0 = None: w_i g_i alone."""
    n = len(x)
    hi = origin + np.array(tex.shape[:3]) * vs - vs
    inside = ((x[:, 0] > origin[0]) & (x[:, 0] < hi[0]) & (x[:, 1] > origin[1]) & (x[:, 1] < hi[1]) & (x[:, 2] > origin[2]) & (x[:, 2] < hi[2]))
    g = np.zeros((n, 3))
    g[inside] = _gather(tex, origin, vs, x[inside])
    F = w[:, None] * g
    if g0 is None:
        return F
    F = F / g0
    first, nbr, rest = network
    deg = np.diff(first)
    for k in range(int(deg.max()) if n else 0):      # the k-th neighbour of every atom that has one: ascending j per atom
        i = np.nonzero(deg > k)[0]
        e = first[i] + k
        d3 = x[nbr[e]] - x[i]
        d = _length(d3)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (stiffness * (d - rest[e])) / d
        live = d != 0.0      # a term with d == 0 contributes nothing
        F[i[live]] = F[i[live]] + t[live, None] * d3[live]
    return F


def flex_fit_numpy(grid, origin, vs, coords, network, stiffness=1.0, n_steps=2000, max_step=0.5, min_step=0.01, weights=None, fixed=None):
    """The contract of `mad_flex_fit`, restated.  -> dict(coords, converged, last_step, step, g0, margin): margin is the smallest
    |max displacement - step| over all batch decisions of the run (inf when there was none)."""
    grid = np.asarray(grid, np.float32)
    origin = np.asarray(origin, np.float64)
    x = np.array(coords, np.float64).reshape(-1, 3)
    n = len(x)
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    free = np.ones(n, bool) if fixed is None else ~np.asarray(fixed, bool).reshape(-1)
    network = check_network("flex_fit_numpy", n, network)
    check_steps("flex_fit_numpy", None, stiffness, n_steps, max_step, min_step)
    tex = np.moveaxis(np.array(np.gradient(grid)), 0, -1)      # float32, as k_density_grad
    wg = forces_numpy(tex, origin, vs, x, w, None, network, stiffness)
    g0 = float(np.sqrt(fourier.tree_sum((wg[:, 0] * wg[:, 0] + wg[:, 1] * wg[:, 1]) + wg[:, 2] * wg[:, 2]) / float(n)))
    if g0 == 0.0:
        raise ValueError("flex_fit_numpy: no atom feels the map")
    prev = x.copy()
    step, batch, margin = float(max_step), 0, np.inf
    converged, last = False, n_steps - 1
    for s in range(n_steps):
        F = forces_numpy(tex, origin, vs, x, w, g0, network, stiffness)
        F[~free] = 0.0
        length = _length(F)
        if np.any(np.isnan(length)) or np.any(np.isnan(x)):
            converged, last = False, s
            break
        m = float(np.max(length))
        if m == 0.0:
            converged, last = True, s
            break
        scale = step / m
        x[free] = x[free] + F[free] * scale
        batch += 1
        if batch == BATCH:
            mx = float(np.fmax.reduce(_length(x[free] - prev[free]), initial=0.0))
            margin = min(margin, abs(mx - step))
            if mx < step:
                step *= 0.5
            batch = 0
            prev = x.copy()
        if step < min_step:
            converged, last = True, s
            break
    return dict(coords=x, converged=converged, last_step=last, step=step, g0=g0, margin=float(margin))


# -- the result --------------------------------------------------------------------------------------------------------------
class FlexFit(object):
    """What `Dmap.flex_fit` returns: `coords` (N, 3) of all atoms, `start`, `converged`, `last_step`, the final `step`, `g0`,
    `network` = (first, nbr, rest), and `first_atom` (where every part of a list begins)."""

    def __init__(self, start, coords, converged, last_step, step, g0, network, first_atom, sources):
        self.start, self.coords = start, coords
        self.converged, self.last_step, self.step, self.g0 = converged, last_step, step, g0
        self.network, self.first_atom = network, first_atom
        self._sources = sources

    def __len__(self):
        return len(self._sources)

    def part(self, b):
        """The fitted coordinates of part b of the list that was given."""
        return self.coords[self.first_atom[b]:self.first_atom[b + 1]]

    def strain(self):
        """RMS of d - d0 over all springs (0 for a network without springs)."""
        first, nbr, rest = self.network
        if len(nbr) == 0:
            return 0.0
        owner = np.repeat(np.arange(len(self.coords)), np.diff(first))
        d = _length(self.coords[nbr] - self.coords[owner]) - rest
        return float(np.sqrt(np.sum(d * d) / len(d)))

    def displacement(self):
        """Per atom, how far it ended from where it started."""
        return _length(self.coords - self.start)

    def rmsd(self, other=None):
        """RMSD of the fitted coordinates to `other` (N, 3); default: to the start."""
        other = self.start if other is None else np.asarray(other, np.float64).reshape(-1, 3)
        if other.shape != self.coords.shape:
            raise ValueError("FlexFit.rmsd: other has shape %s, the fit %s" % (other.shape, self.coords.shape))
        return float(np.sqrt(np.sum((self.coords - other) ** 2) / len(other)))

    def place(self, pdb=None, b=0):
        """A copy of `pdb` (default: the PDB part b came from) carrying part b's fitted coordinates."""
        pdb = self._sources[b] if pdb is None else pdb
        if pdb is None:
            raise ValueError("FlexFit.place: part %d came from an array: give the PDB to place" % b)
        if len(pdb.get_coords()) != len(self.part(b)):
            raise ValueError("FlexFit.place: the PDB has %d atoms, part %d has %d" % (len(pdb.get_coords()), b, len(self.part(b))))
        out = copy.copy(pdb)
        out.set_coords(self.part(b))
        return out

    def write_pdb(self, prefix):
        """`<prefix>_<b>.pdb` for every part that came from a PDB -> the names written."""
        names = []
        for b, src in enumerate(self._sources):
            if src is not None:
                names.append("%s_%d.pdb" % (prefix, b))
                self.place(b=b).write_pdb(names[-1])
        return names


def flex_fit(dmap, structure, cutoff=6.0, stiffness=1.0, n_steps=2000, max_step=0.5, min_step=0.01, weights=None, fixed=None, network=None):
    from . import _lib, structure_utils
    who = "Dmap.flex_fit"
    coords, first_atom, src = atoms_of(who, structure)
    n = len(coords)
    check_steps(who, cutoff if network is None else None, stiffness, n_steps, max_step, min_step)
    if not np.all(np.isfinite(coords)):
        raise ValueError("%s: structure: a coordinate is not finite" % who)
    if weights is not None:
        weights = np.asarray(weights, np.float64).reshape(-1)
        if len(weights) != n or not np.all(np.isfinite(weights)):
            raise ValueError("%s: weights must be %d finite numbers" % (who, n))
    if fixed is not None:
        fixed = np.asarray(fixed, bool).reshape(-1)
        if len(fixed) != n:
            raise ValueError("%s: fixed has %d entries for %d atoms" % (who, len(fixed), n))
    if network is not None:
        network = check_network(who, n, network)
    g, origin, vs = _map_args(who, dmap)
    lib = _lib.get_lib()
    if network is None:
        network = lib.flex_network(coords, cutoff)
    lib.upload_density(g, origin, vs)
    structure_utils.invalidate_density()
    out, conv, last, step, g0 = lib.flex_fit(coords, network, stiffness=stiffness, n_steps=n_steps, max_step=max_step, min_step=min_step,
                                             weights=weights, fixed=fixed)
    return FlexFit(coords, out, conv, last, step, g0, network, first_atom, src)
