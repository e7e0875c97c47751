"""End-to-end MaD.run() on a bench workload: the resident path against the stage path (MAD_STAGE_PATH=1), cold and warm.

    python tools/run_mad_e2e.py --workload c3

The workload (bench/configs/<name>.json) is written into a temporary folder the way bench.py builds it -- the subunits with
mad_amd.synth, the map = their placed copies simulated on the device, padded to N^3, plus the workload's noise -- as an MRC map and
one PDB per subunit.  Then, for each path in its own folder, MaD.run() twice: cold (no descriptor cache) and warm (the cache of
the cold run).  One JSON line on stdout: wall seconds, mad.timings, mad.timings_detail (the filter stage split into clustering and
candidate list) with the matches whose clustering fell back to the host loop, correlations / wall, and the seconds outside MapSpace,
Detector, file preparation, cache I/O and solution writing.  MaD's own messages go to stderr.  MAD_FILTER_HOST=1 in the
environment keeps the filter's host loop (the stage as it was before the device clustering).
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_workload(lib, W, folder):
    """bench.build_inputs' map and subunits, as files: map.mrc and subNN.pdb."""
    from mad_amd import mapio, synth
    rng = np.random.default_rng(1234)
    sp = 2.2 * W["radius"]
    cells = [(i, j, k) for i in range(W["grid"][0]) for j in range(W["grid"][1]) for k in range(W["grid"][2])]
    centre = (np.array(W["grid"]) - 1) * sp / 2
    placed, mass, subs = [], [], []
    for s, seed in enumerate(W["seeds"]):
        atoms, names, elems = synth.random_globule(W["n_atoms"], W["radius"], seed=seed)
        name = "sub%02d" % s
        synth.write_pdb(os.path.join(folder, name + ".pdb"), atoms, names, elems)
        subs.append(name + ".pdb")
        for c in range(W["copies"]):
            placed.append(synth.place(atoms, synth.random_rotation(rng), np.array(cells[s * W["copies"] + c]) * sp - centre + rng.normal(scale=2.0, size=3)))
            mass.append(synth.masses(elems))
    grid, x0, y0, z0 = lib.structure_to_density(np.concatenate(placed), np.concatenate(mass), W["res"], W["vs"])
    origin = np.array([x0, y0, z0])
    N = W["N"]
    lo = [(N - s) // 2 for s in grid.shape]
    big = np.zeros((N, N, N), np.float32)
    big[lo[0]:lo[0] + grid.shape[0], lo[1]:lo[1] + grid.shape[1], lo[2]:lo[2] + grid.shape[2]] = grid
    grid, origin = big, origin - np.array(lo) * W["vs"]
    if W.get("noise", 0.0) > 0.0:
        grid = (grid + np.random.default_rng(4321).normal(0.0, W["noise"] * float(grid.max()), grid.shape)).astype(np.float32)
    mapio.write_mrc(os.path.join(folder, "map.mrc"), grid, origin, W["vs"])
    return subs


def run_once(folder, inputs, subs, W):
    from mad import MaD
    cwd = os.getcwd()
    os.chdir(folder)
    try:
        mad = MaD.MaD()
        with contextlib.redirect_stdout(sys.stderr):
            mad.add_map(os.path.join(inputs, "map.mrc"), W["res"])
            for s in subs:
                mad.add_subunit(os.path.join(inputs, s), n_copies=W["copies"])
            t0 = time.perf_counter()
            mad.run(cc_threshold=W["cc_threshold"], n_samples=W["n_samples"])
            wall = time.perf_counter() - t0
    finally:
        os.chdir(cwd)
    t = {k: round(v, 4) for k, v in mad.timings.items()}
    outside = wall - sum(mad.timings[k] for k in ("prep", "mapspace", "detector", "cache_io", "write"))
    detail = {k: round(v, 4) for k, v in mad.timings_detail.items()}
    return dict(wall_s=round(wall, 4), timings_s=t, timings_detail_s=detail, filter_undecided=int(mad.filter_undecided), correlations=int(mad.n_correlations),
                correlations_per_s=mad.n_correlations / wall if wall > 0 else None,
                outside_mapspace_detector_io_s=round(outside, 4), solutions=sum(len(v[1]) for v in mad.buildable_subunits.values()))


def main():
    import bench
    from mad_amd import _lib
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workload", default="c3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--paths", default="resident,stage", help="comma-separated: resident, stage")
    args = ap.parse_args()
    W = bench.WORKLOADS[args.workload]
    lib = _lib.get_lib()
    out = dict(tool="run_mad_e2e", workload=args.workload, config=W["file"])
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs")
        os.makedirs(inputs)
        subs = write_workload(lib, W, inputs)
        for path in args.paths.split(","):
            folder = os.path.join(tmp, path)
            os.makedirs(folder)
            if path == "stage":
                os.environ["MAD_STAGE_PATH"] = "1"
            else:
                os.environ.pop("MAD_STAGE_PATH", None)
            out[path] = dict(cold=run_once(folder, inputs, subs, W), warm=run_once(folder, inputs, subs, W))
        os.environ.pop("MAD_STAGE_PATH", None)
    print(json.dumps(out))
    lib.synchronize()


if __name__ == "__main__":
    main()
