#!/usr/bin/env python3
"""Example driver, same calls as the reference's run_MaD.py:64-76.

    python run_MaD.py <map.mrc|map.sit|map.pdb> <resolution> <subunit.pdb>[:n_copies] [more subunits...]
                      [--patch-size N] [--cc-threshold X] [--n-samples N]

The options are the arguments of MaD.run() the reference's own examples change: patch_size=24 for its low-resolution case,
cc_threshold=0.5 and n_samples=80 for others.  An option that is not given keeps run()'s default.

Without arguments it docks a small synthetic dimer (written to ./synthetic_example) so
that the flow can be tried without the lab's data set.  Needs an MI355X: the hot path
has no CPU fallback.
"""
import os
import sys

from mad import MaD


def _synthetic_example(folder="synthetic_example"):
    import numpy as np
    from mad_amd import synth
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(7)
    coords, names, elems = synth.random_globule(1500, 16.0, seed=1)
    sub = os.path.join(folder, "subunit.pdb")
    synth.write_pdb(sub, coords, names, elems)
    parts = [synth.place(coords, synth.random_rotation(rng), t) for t in ([0, 0, 0], [38, 6, -4])]
    asm = os.path.join(folder, "assembly.pdb")
    synth.write_pdb(asm, np.concatenate(parts), names * 2, elems * 2)
    return asm, 10.0, [(sub, 2)]


RUN_OPTIONS = {"--patch-size": ("patch_size", int), "--cc-threshold": ("cc_threshold", float), "--n-samples": ("n_samples", int)}


def _take_options(argv):
    """Splits `--name value` / `--name=value` run() options from the positional arguments: (positional, {run() keyword: value})."""
    rest, opts = [], {}
    i = 0
    while i < len(argv):
        name, eq, value = argv[i].partition("=")
        if name in RUN_OPTIONS:
            if not eq:
                i += 1
                if i >= len(argv):
                    sys.exit("run_MaD.py: %s needs a value" % name)
                value = argv[i]
            key, kind = RUN_OPTIONS[name]
            try:
                opts[key] = kind(value)
            except ValueError:
                sys.exit("run_MaD.py: %s %r is not %s" % (name, value, "an integer" if kind is int else "a number"))
        elif argv[i].startswith("--"):
            sys.exit("run_MaD.py: unknown option %s (known: %s)" % (argv[i], ", ".join(sorted(RUN_OPTIONS))))
        else:
            rest.append(argv[i])
        i += 1
    return rest, opts


if __name__ == "__main__":
    args, run_options = _take_options(sys.argv[1:])
    if len(args) >= 3:
        map_file, resolution = args[0], float(args[1])
        subunits = [(a.split(":")[0], int(a.split(":")[1]) if ":" in a else 1) for a in args[2:]]
    else:
        map_file, resolution, subunits = _synthetic_example()

    # Make a MaD instance
    mad = MaD.MaD()

    # Add map, specify its resolution
    mad.add_map(map_file, resolution)

    # Add components
    for path, n_copies in subunits:
        mad.add_subunit(path, n_copies=n_copies)

    # Get solutions per component
    mad.run(**run_options)

    # Build assembly models from solutions
    mad.build_assembly()
