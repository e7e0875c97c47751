#!/usr/bin/env python3
"""Host time of one sharded match (dist.ShardedMatchAsync: constructor = everything enqueued, finish = the one wait + unpacking) on
one GPU, through torch.distributed (`--path torch`: RCCL of torch on an ExternalStream, the records merged on the host) or through
the library's communicator (`--path lib`: mad_dist_*, the records merged by k_shard_merge).

  --mode world1   a group of ONE rank with real RCCL collectives (the only size at which RCCL runs on one GPU)
  --mode rank3    the rehearsal of rank 2 of 3: no link traffic; torch path = local=True (no collective, its own record only),
                  lib path = the rehearsal communicator (its record into slot 2 of 3, all three merged on the device)

One JSON line.  The sets are those of tests/test_gpu_dist_lib.py.  A sibling of tools/probe_collective.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=("torch", "lib"), required=True)
    ap.add_argument("--mode", choices=("world1", "rank3"), required=True)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--k", type=int, default=40)
    a = ap.parse_args()
    import torch
    from mad_amd import _lib, synth
    from mad_amd import dist as mdist
    from mad_amd.eqsp import EQSP_Sphere
    from mad_amd.orient_tables import orientation_matrices
    lib = _lib.Lib(0)
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    dom, adj = orientation_matrices(e112)
    lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, e16.sphere_eqsp)
    shape = (56, 60, 64)
    slot = lib.new_slot()
    lib.upload_field(slot, synth.gradient_field(synth.blob_volume(shape, n_blobs=60, seed=9, sigma=(1.5, 3.5))))
    rng = np.random.default_rng(3)
    sets = []
    for n in (150, 60):
        coords = synth.interior_anchors(shape, n, 12, 100 + n)
        sets.append(lib.set_build([-1, slot], coords, np.ones(n, np.int32), coords.astype(np.float64) * 1.5 + rng.normal(scale=0.2, size=(n, 3)), np.arange(n)))
    lo, hi = sets
    cc, dist_, k = 0.45, 4.0, a.k
    n_lo = lo.size()[0]
    part, parts = (0, 1) if a.mode == "world1" else (2, 3)
    kw, comm, pg = {}, None, False
    if a.path == "torch":
        if a.mode == "world1":
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29545")
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
            pg = True
            kw = dict(group=None, local=False)
        else:
            kw = dict(local=True)
    else:
        comm = mdist.LibComm(lib, part, parts, rehearsal=a.mode == "rank3")
        kw = dict(comm=comm)
        if a.mode == "rank3":      # the peers' records in their slots (this rank's own, thrice: the cost does not depend on the values)
            rec = lib.match_shard_record_doubles(k)
            h = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, part, parts, n_lo, **kw)
            h.finish()
            d_all = comm.match_buffers(hi.lane(), hi.n_anchors + lo.n_anchors, rec)[2]
            mine = lib.dist_download(d_all + 2 * rec * 8, rec)
            lib.dist_upload(d_all, np.concatenate([mine, mine, mine]))
    tb, tf = [], []
    m = None
    for it in range(a.reps + 20):
        lib.synchronize()
        t0 = time.perf_counter()
        h = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, part, parts, n_lo, **kw)
        t1 = time.perf_counter()
        res = h.finish()
        t2 = time.perf_counter()
        assert res is not None
        m = len(res[0])
        if it >= 20:
            tb.append(t1 - t0)
            tf.append(t2 - t1)
    tot = [x + y for x, y in zip(tb, tf)]
    us = lambda v: round(1e6 * statistics.median(v), 1)      # noqa: E731
    print(json.dumps(dict(path=a.path, mode=a.mode, k=k, rows=m, reps=a.reps, lib=os.path.basename(_lib.LIB_PATH), begin_us=us(tb), finish_us=us(tf),
                          total_us=us(tot), total_mean_us=round(1e6 * statistics.mean(tot), 1), total_p10_us=round(1e6 * sorted(tot)[len(tot) // 10], 1),
                          total_p90_us=round(1e6 * sorted(tot)[9 * len(tot) // 10], 1))))
    sys.stdout.flush()
    if comm is not None:
        comm.close()
    for s in sets:
        s.close()
    if pg:
        import torch.distributed as dist
        mdist.ShardedMatchAsync._pool.clear()
        torch.cuda.synchronize()
        dist.destroy_process_group()
    lib.close()


if __name__ == "__main__":
    main()
