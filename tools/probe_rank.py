#!/usr/bin/env python
"""Times the device heads of the assembly ranking (assembly.rank_copies_head / rank_models_head) on seeded tables and, where
the host loops finish, checks them against assembly.rank_copies / rank_models.  Prints one JSON line: per case the seconds of
the device call, the items it evaluated and the items it jumped over (mad_last_rank_plan), and the host's seconds where run.
DESIGN.md section 4f's table comes from this.

    python tools/probe_rank.py                      # every case; the host loops up to --host-max-items
    python tools/probe_rank.py --unpruned           # also with MAD_RANK_NO_PRUNE=1: the rate the launch range is sized from
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, assembly      # noqa: E402


def table(n, seed, p_zero):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, n))
    m = n * (n - 1) // 2
    t[np.triu_indices(n, 1)] = np.where(rng.random(m) < p_zero, 0.0, rng.random(m))
    return t


def groups_of(g, size):
    return [list(range(i * size, (i + 1) * size)) for i in range(g)]


def same(a, b):
    return len(a) == len(b) and all(tuple(x[0]) == tuple(y[0]) and [float(v).hex() for v in x[1:]] == [float(v).hex() for v in y[1:]] for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-max-items", type=int, default=600000)
    ap.add_argument("--unpruned", action="store_true")
    ap.add_argument("--cap", type=int, default=10)
    a = ap.parse_args()
    lib = _lib.get_lib()
    cases = [("copies", n, c, 0.5) for n, c in ((16, 6), (20, 6), (24, 6), (30, 6), (40, 6))] + [("copies", 60, 8, 0.7)]
    cases += [("models", g, 10, 0.5) for g in (4, 5, 6, 8)]
    if a.unpruned:      # spaces large enough to read a rate from
        cases += [("copies", 60, 6, 0.5), ("copies", 48, 8, 0.5), ("copies", 36, 12, 0.5), ("copies", 32, 16, 0.5), ("models", 9, 8, 0.5), ("models", 16, 3, 0.5)]
    out = []
    for kind, x, y, p_zero in cases:
        if kind == "copies":
            t, items = table(x, 100 + x, p_zero), math.comb(x, y)
            dev = lambda: assembly.rank_copies_head(t, y, cap=a.cap, lib=lib)
            host = lambda: assembly.rank_copies(t, y)[:a.cap]
        else:
            t, items = table(x * y, 200 + x, p_zero), y ** x
            dev = lambda: assembly.rank_models_head(t, groups_of(x, y), a.cap, lib=lib)
            host = lambda: assembly.rank_models(t, groups_of(x, y))[:a.cap]
        rec = {"case": "%s %d/%d" % (kind, x, y), "items": items}
        for tag in ("pruned", "unpruned") if a.unpruned and items <= 2 ** 31 else ("pruned",):
            os.environ["MAD_RANK_NO_PRUNE"] = "1" if tag == "unpruned" else "0"
            dev()      # (the first call sizes the scratch buffer)
            t0 = time.perf_counter()
            got = dev()
            dt = time.perf_counter() - t0
            launches, evaluated, skipped, extra = lib.last_rank_plan()
            rec[tag] = {"seconds": round(dt, 6), "launches": launches, "evaluated": evaluated, "skipped": skipped, "band_extra": extra,
                        "items_per_s": round(evaluated / dt)}
        os.environ["MAD_RANK_NO_PRUNE"] = "0"
        if items <= a.host_max_items:
            t0 = time.perf_counter()
            want = host()
            rec["host_seconds"] = round(time.perf_counter() - t0, 3)
            rec["equal"] = same(got, want)
        out.append(rec)
    print(json.dumps({"probe": "rank", "cap": a.cap, "cases": out}))
    return 0 if all(r.get("equal", True) for r in out) else 1


if __name__ == "__main__":
    sys.exit(main())
