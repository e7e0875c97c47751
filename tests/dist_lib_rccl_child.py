"""Child process of tests/test_gpu_dist_lib.py::test_rccl_world_of_one_in_a_child_process: the RCCL branch of the library's
communicator at world size 1 -- the only size at which it can run on one GPU -- in a process that has torch imported."""
import os
import sys

import numpy as np
import torch      # noqa: F401  (on purpose: the process keeps torch's copy of RCCL, and must still exit cleanly)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_amd import _lib, synth      # noqa: E402
from mad_amd import dist as mdist      # noqa: E402
from mad_amd.eqsp import EQSP_Sphere      # noqa: E402
from mad_amd.orient_tables import orientation_matrices      # noqa: E402


def main():
    lib = _lib.Lib(0)
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    dom, adj = orientation_matrices(e112)
    lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, e16.sphere_eqsp)
    shape = (56, 60, 64)
    slot = lib.new_slot()
    lib.upload_field(slot, synth.gradient_field(synth.blob_volume(shape, n_blobs=60, seed=9, sigma=(1.5, 3.5))))
    rng = np.random.default_rng(1)
    sets, anchors = [], []
    for n in (150, 60):
        coords = synth.interior_anchors(shape, n, 12, 100 + n)
        subv = coords.astype(np.float64) * 1.5 + rng.normal(scale=0.2, size=(n, 3))
        anchors.append((coords, subv))
        sets.append(lib.set_build([-1, slot], coords, np.ones(n, np.int32), subv, np.arange(n)))
    lo, hi = sets
    cc, dist_, k = 0.45, 4.0, 40
    n_lo = lo.size()[0]

    comm = mdist.LibComm(lib, 0, 1)      # mad_dist_unique_id -> mad_dist_init(1, 0, id)
    assert lib.dist_info() == (1, 0, False)
    try:
        lib.dist_init(1, 0, lib.dist_unique_id())
    except _lib.MadBackendError as e:
        assert "EINVAL" in str(e), e
    else:
        raise AssertionError("a second mad_dist_init without mad_dist_destroy went through")

    # the two plain collectives are identities at world size 1
    lane, stream = hi.lane(), hi.stream()
    flags = rng.integers(0, 2, size=777).astype(np.uint8)
    d_flags = lib.dist_scratch(lane, _lib.DIST_BUF_FLAGS, flags.size)
    lib.dist_upload(d_flags, flags)
    lib.dist_or_allreduce(stream, d_flags, flags.size)
    lib.synchronize()
    assert np.array_equal(lib.dist_download(d_flags, flags.size, np.uint8), flags)
    block = rng.integers(0, 256, size=100003).astype(np.uint8)
    d_send, d_recv = comm.wire_buffers(lane, block.size)
    lib.dist_upload(d_send, block)
    lib.dist_upload(d_recv, np.zeros_like(block))
    lib.dist_allgather(stream, d_send, d_recv, block.size)
    lib.synchronize()
    assert np.array_equal(lib.dist_download(d_recv, block.size, np.uint8), block)

    # the sharded match through the communicator = the one without any collective
    want = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, 0, 1, n_lo, local=True).finish()
    got = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, 0, 1, n_lo, comm=comm).finish()
    assert len(want[0]) == k
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    assert mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, 0, 1, n_lo - 1, comm=comm).finish() is None

    # the sharded build of one share through the communicator = mad_set_build
    coords, subv = anchors[0]
    n = len(coords)
    b = mdist.ShardedSetBuild(lib, [-1, slot], coords, np.ones(n, np.int32), subv, np.arange(n), 0, 1, force=True, comm=comm)
    assert b.sharded and b.backend == "lib"
    ref = lo.download()
    for it in range(2):
        full = b.enqueue()
        d = full.download()
        for key in ("anchor", "main", "sec", "R", "dsc"):
            assert np.array_equal(d[key], ref[key]), key
    b.close()

    comm.close()      # mad_dist_destroy ...
    comm = mdist.LibComm(lib, 0, 1)      # ... and a second communicator on the same context
    lib.dist_upload(d_flags, flags)
    lib.dist_or_allreduce(stream, d_flags, flags.size)
    lib.synchronize()
    assert np.array_equal(lib.dist_download(d_flags, flags.size, np.uint8), flags)
    comm.close()
    for s in sets:
        s.close()
    lib.close()
    print("rccl child OK")


if __name__ == "__main__":
    main()
