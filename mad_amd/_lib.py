"""ctypes binding of libmad_amd.so (the C-ABI in include/mad_amd.h).

This is the ONLY compute back-end of the package: there is no CPU fallback.  If the
shared library is missing, or no gfx950 device can be opened, the first call raises
`MadBackendError` -- loudly, as a drop-in for a hot path must.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MAD_LIB_PATH: another build of the same library (diagnostic builds with other compiler flags; tools/build_variant.sh)
LIB_PATH = os.environ.get("MAD_LIB_PATH") or os.path.join(_HERE, "libmad_amd.so")
# mirrors of include/mad_amd.h (tests/test_host.py compares each with the header's #define)
RESULT_COLS = 23
RANK_MAX_N, RANK_MAX_K, RANK_MAX_TOP, RANK_MAX_OUT = 96, 16, 512, 4096      # MAD_RANK_*
RANK_TOP, RANK_BELOW = 0, 1
SHARD_MERGE_MAX = 8192      # MAD_SHARD_MERGE_MAX: records x k one workgroup of k_shard_merge sorts
SHARD_FLAG_MISMATCH = 32    # MAD_SHARD_FLAG_MISMATCH
DIST_ID_BYTES = 128         # MAD_DIST_ID_BYTES
DIST_BUF_FLAGS, DIST_BUF_MINE, DIST_BUF_ALL, DIST_BUF_MERGED, DIST_BUF_WIRE, DIST_BUF_GATHER = range(6)      # MAD_DIST_BUF_*
POSE_CLUSTER_MAX_N = 4096      # MAD_POSE_CLUSTER_MAX_N: rows of one match in pose_cluster_many
EINVAL, ENOMEM, ENOSPC, ENODEV, EDOM, EHIP = -22, -12, -28, -19, -33, -5      # MAD_E*
ERRORS = {EINVAL: "EINVAL", ENOMEM: "ENOMEM", ENOSPC: "ENOSPC", ENODEV: "ENODEV", EDOM: "EDOM", EHIP: "EHIP"}
# mirrors of headers under csrc/ (no test compares these)
# wide sets (include/mad_amd.h; MAD_WIDE_* of csrc/mad_common.h): from this descriptor radius on a set's int8 rows hold count - WIDE_C
WIDE_FROM_R = 11
WIDE_C = 108
WIDE_MAX = WIDE_C + 127
QSCORE_CHUNK = 256          # QS_CHUNK of csrc/mad_qscore_plan.h: neighbours of one LDS chunk of k_qscore
QSCORE_MAX_SHELLS, QSCORE_MAX_TRIES = 64, 64      # QS_MAX_R, QS_MAX_TRIES
SYMMETRIZE_MAX_OPS = 64     # SYMZ_MAX_OPS of csrc/mad_resample.hip
TAB_ZBINS, TAB_PBINS, TAB_BELTS = 2048, 2048, 4      # MAD_TAB_* of csrc/mad_common.h
FLEX_MAX_DEGREE = 128       # MAD_FLEX_MAX_DEGREE of include/mad_amd.h: springs of one atom that flex_network builds at most

# The C ABI, stated once: every function of include/mad_amd.h as name=return(arguments), one letter per type.  load_library() sets
# restype and argtypes from it, so a call passes plain Python numbers and ctypes refuses a wrapper of another width.  A new function
# of the header gets its entry here; tests/test_host.py parses the header and says where the two disagree.
_CTYPE = {"p": C.c_void_p,      # any pointer: handles, arrays, byref results, ctypes arrays of pointers, None
          "i": C.c_int,         # int, int32_t
          "q": C.c_int64, "Q": C.c_uint64, "d": C.c_double, "f": C.c_float,
          "s": C.c_char_p,      # const char *
          "v": None}            # void (return only)
PROTOTYPES = {entry[:entry.index("=")]: (entry[entry.index("=") + 1], tuple(entry[entry.index("(") + 1:-1])) for entry in """
mad_init=i(ip) mad_destroy=v(p) mad_last_error=s(p) mad_synchronize=i(p) mad_stream=p(p) mad_set_overlap=i(pi)
mad_timing_enable=i(pi) mad_timing_reset=i(p) mad_timing_get=i(pspp) mad_last_ms=d(ps) mad_probe_peaks=i(ppp)
mad_set_eqsp=i(piippp) mad_eqsp_tab_build=i(pipp) mad_upload_field=i(pipppiii) mad_upload_field_device=i(pipiii)
mad_free_field=i(pi) mad_field_download=i(pipp) mad_set_orient_window=i(pd) mad_orient=i(piipiiiippppppqp)
mad_describe=i(piippqip) mad_describe_sized=i(piippqiip) mad_correlate=i(ppqpqidppppq) mad_pose_score=i(ppppqpppqpppqpqpqdpp)
mad_topk=i(ppqqp) mad_set_create=i(pp) mad_set_destroy=v(pp) mad_set_build=i(pppppppiiii) mad_set_build_many=i(pipppppppiii)
mad_set_mark_wide=i(ppi) mad_set_is_wide=i(pp) mad_set_load=i(ppqppppipppi) mad_set_size=i(pppp) mad_set_download=i(ppppppp)
mad_match_topk=i(pppddqpppp) mad_match_topk_many=i(pippddqpppp) mad_match_topk_many_begin=i(pippddqpppp)
mad_match_topk_many_finish=i(p) mad_match_topk_many_begin2=i(pippddqpppppp) mad_match_topk_many2=i(pippddqpppppp)
mad_set_batching=i(pi) mad_set_option=i(psd) mad_last_pose_kernel=i(p) mad_last_pose_plan=i(pp) mad_last_pose_selected=q(p)
mad_device_allocations=q(p) mad_match_fetch=i(pppppq) mad_match_results=i(ppppq) mad_match_used=i(ppipi)
mad_upload_density=i(ppiiidddd) mad_refine=i(ppiqiddpp) mad_last_refine_plan=i(ppp) mad_last_density_chunks=i(p)
mad_structure_to_density=i(pppqdddippp) mad_ccc=i(pppppppddp) mad_map_mask=i(pppppppd) mad_map_multiply=i(pppppppd)
mad_map_ccc=i(ppppipppddp) mad_map_resample=i(ppppdppippdp) mad_map_zone=i(ppppdpqddip) mad_map_envelope=i(pppddddppp)
mad_map_group_fit=i(pppppppdppiddpp) mad_map_qscore=i(ppppdpqpqppipippppp) mad_map_smooth=i(pppdp)
mad_map_segment=i(pppdidqpppppqppp) mad_map_components=i(pppdipppqp) mad_map_dust=i(pppdiqqfpp) mad_map_sort=i(ppqp)
mad_map_kth=i(ppqqpp) mad_map_confidence=i(pppipdipppppppp) mad_map_fsc=i(pppppppdpppq)
mad_map_fsc_masked=i(pppppppdpppidQpppppp) mad_map_phase_randomize=i(ppiiQ) mad_map_fft=i(pppppppdpp)
mad_map_filter=i(pppppipqppp) mad_map_ifft=i(ppip) mad_map_scan=i(pppippddidqpppppp) mad_map_search=i(ppppppipiddidqppppppp)
mad_map_rotate=i(ppppipdpp) mad_map_local_fsc=i(pppppppdiidppppp) mad_map_local_scale=i(pppppppdiipppp)
mad_map_local_filter=i(pppdppippp) mad_match_shard_pairs=i(pppqqdppp) mad_match_shard_topk=i(pppppdqppppp)
mad_match_shard_record_doubles=q(q) mad_match_shard_begin=i(pppqqqdp) mad_match_shard_score=i(ppppdqp)
mad_match_shard_collect=i(pppqp) mad_match_shard_wait=i(pipq) mad_match_shard_merge=i(pppiqp) mad_dist_unique_id=i(pp)
mad_dist_init=i(piip) mad_dist_destroy=i(p) mad_dist_info=i(pppp) mad_dist_rehearse_flags=i(ppq) mad_dist_or_allreduce=i(pppq)
mad_dist_allgather=i(ppppq) mad_dist_allgather_topk=i(ppppqp) mad_dist_scratch=i(piiqp) mad_dist_copy=i(pppqi)
mad_set_wire_bytes=q(iq) mad_set_export=i(pppiq) mad_set_import=i(pppiiqppppi) mad_set_lane=i(pp) mad_set_stream=p(pp)
mad_set_bind_lane=i(ppi) mad_density_ccc=i(pppiqdddp) mad_dock_refine_score=i(pipppippppidddddpppp)
mad_grid_overlap=i(pppppppddpp) mad_overlap_matrix=i(ppppiddddp) mad_space_create=i(pp) mad_space_destroy=v(pp)
mad_space_build=i(pppiiiiiippidpipppii) mad_space_info=i(pppppp) mad_space_download=i(ppiip) mad_space_peaks=i(ppidippqp)
mad_space_patches=i(ppipiip) mad_space_localize=i(ppipippppp) mad_localize_volume=i(ppiiiipippppp)
mad_pose_cluster_many=i(pippppdpppp) mad_rank_copies=i(ppiiidqqqpppppp) mad_rank_models=i(ppipiqqqqpppppp)
mad_last_rank_plan=i(ppppp) mad_assembly_density=i(pipppdppp) mad_assembly_refine=i(pippppdiddppppppp)
mad_assembly_refine_symmetric=i(pippppippdiddppppppp)
mad_last_assembly_plan=i(pppp) mad_map_symmetry_score=i(ppppdpdiippp) mad_map_symmetrize=i(ppppdippip)
mad_last_symmetry_plan=i(pppp) mad_flex_network=i(pqpdpqppp) mad_flex_fit=i(pqppppppdiddppppp) mad_last_flex_plan=i(ppppp)
mad_model_density_b=i(pppdqpppddpp) mad_bfactor_refine=i(ppppdqppqpppdddiddppppp) mad_last_bfactor_plan=i(pppppppp)
""".split()}
SYMBOLS = list(PROTOTYPES)      # every symbol include/mad_amd.h declares (tests check the library exports all of them)


class MadBackendError(RuntimeError):
    pass


_dll = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 next to its extension modules.  Two HIP runtimes in one process do not share a
    device: whichever is loaded second finds "no HIP GPUs".  So when torch is installed, its copy of the runtime is loaded first
    and libmad_amd.so binds to that one (same soname), whatever the import order of torch and this package.  torch itself is
    neither imported nor needed."""
    import importlib.util
    if os.environ.get("MAD_OWN_HIP_RUNTIME", "0") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        path = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load_library():
    """dlopen the HIP library (works without a GPU; opening a device does not) and give every function of PROTOTYPES its types."""
    global _dll
    if _dll is None:
        if not os.path.exists(LIB_PATH):
            raise MadBackendError(
                "MaD> %s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C mad_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        _share_torch_hip_runtime()
        try:
            dll = C.CDLL(LIB_PATH)
        except OSError as e:
            raise MadBackendError("MaD> cannot load %s: %s" % (LIB_PATH, e))
        for name, (ret, args) in PROTOTYPES.items():
            try:
                fn = getattr(dll, name)
            except AttributeError:
                raise MadBackendError("MaD> %s does not export %s, which include/mad_amd.h declares: rebuild it" % (LIB_PATH, name))
            fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[a] for a in args]
        _dll = dll
    return _dll


class _PosePlanInfo(C.Structure):      # mad_pose_plan_info of include/mad_amd.h
    _fields_ = [("kernel", C.c_int32), ("hi_in_lds", C.c_int32), ("pruned", C.c_int32), ("split", C.c_int32), ("nbv", C.c_int32),
                ("inner_plane", C.c_int32), ("grid_dim", C.c_int32 * 3), ("own_selection", C.c_int32), ("topk_one_wg", C.c_int32),
                ("sel_repeat", C.c_int32), ("fine_grown", C.c_int32), ("search_wgs", C.c_int32), ("fine_dim", C.c_int32 * 3),
                ("reserved", C.c_int32), ("fine_h", C.c_double), ("coarse_h", C.c_double), ("fine_mn", C.c_double * 3),
                ("bits_rad", C.c_double), ("bits_rad_in", C.c_double), ("lds64", C.c_int64), ("lds32", C.c_int64), ("lds32_hi", C.c_int64)]


def eqsp_tab_build(bounds):
    """The table classifier of the 4-byte texels as the library builds it for the zone table `bounds` (Z x 4), on the host: no
    device is opened.  Returns (ok, zbelt[2048], ptab[4, 2048]) as uint8, 255 = undecided; ok is False when the zone table does
    not fit the classifier (then every entry is 255)."""
    dll = load_library()
    b = _c(bounds, np.float64).reshape(-1, 4)
    zbelt, ptab = np.empty(TAB_ZBINS, np.uint8), np.empty((TAB_BELTS, TAB_PBINS), np.uint8)
    rc = dll.mad_eqsp_tab_build(_p(b), len(b), _p(zbelt), _p(ptab))
    if rc < 0:
        raise ValueError("mad_eqsp_tab_build: %s" % ERRORS.get(rc, rc))
    return rc == 1, zbelt, ptab


# -- arguments: what every wrapper checks and converts the same way ---------------------------------------------------------
def _p(a):
    """The address of an array, or NULL for None (the pointer keeps its array alive)."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _dims(g):
    """The int32[3] shape argument of a grid."""
    return np.array(g.shape, np.int32)


def _vec(x, n):
    """A contiguous float64[n]: origins, centres, R (9), T."""
    return _c(np.asarray(x, np.float64).reshape(n), np.float64)


def _grid(who, g, ndim=3, writable=False, what="grid"):
    """`g` as the library reads it in place: a C-contiguous float32 array, `ndim`-dimensional (None: any), writable where the call
    writes into it.  -> g"""
    if not isinstance(g, np.ndarray) or g.dtype != np.float32 or not g.flags.c_contiguous or (writable and not g.flags.writeable):
        raise ValueError("%s needs a %sC-contiguous float32 %s" % (who, "writable " if writable else "", what))
    if ndim is not None and g.ndim != ndim:
        raise ValueError("%s needs a %d-D %s" % (who, ndim, what))
    return g


def _placed(who, g, origin, writable=False, what="grid"):
    """The three arguments (grid, dims[3], origin[3]) of a map with its place; three NULLs for a `g` of None."""
    if g is None:
        return None, None, None
    return _p(_grid(who, g, writable=writable, what=what)), _p(_dims(g)), _p(_vec(origin, 3))


def _countable(who, g):
    if g.size < 1 or g.size >= 2 ** 31:
        raise ValueError("%s: %d voxels (1 .. 2^31 - 1)" % (who, g.size))


def _out(who, out, shape, dtype=np.float32, of="the grid's shape", new=np.empty, name="out"):
    """The array a call fills: a fresh one, or the caller's `out` once it is a writable C-contiguous `dtype` array of `shape`."""
    if out is None:
        return new(shape, dtype)
    if (not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous
            or not out.flags.writeable):
        raise ValueError("%s: %s must be a writable C-contiguous %s array of %s" % (who, name, np.dtype(dtype).name, of))
    return out


def _whole(who, name, v, lo=-2 ** 31, hi=2 ** 31):
    """`v` as an int when it is a whole number in [lo, hi)."""
    i = int(v)
    if i != v or not lo <= i < hi:
        raise ValueError("%s: %s %r" % (who, name, v))
    return i


def _retry_enospc(lib, call, cap, grow=True, slack=0):
    """One C call whose tables may be too small: `call(cap)` makes it with tables of capacity `cap` and returns (rc, needed).  On
    MAD_ENOSPC with needed > cap the call is made again at needed + slack; with grow=False (the caller fixed the capacity) it is
    not, and the answer is False.  Any other failure raises.  -> True when the tables of the last call hold the result."""
    while True:
        rc, needed = call(cap)
        if rc != ENOSPC or needed <= cap:
            lib._chk(rc)
            return True
        if not grow:
            return False
        cap = needed + slack


def _pad_rows(dsc, to=128):
    """Descriptor rows zero-padded to a multiple of 128 counts: the correlation kernel consumes K in steps of 128 bytes, and zeros
    change neither a dot product nor a norm (row lengths 432 and 16 of Descriptor(dsc_size=27 | 1))."""
    d = dsc.shape[1] if dsc.ndim == 2 else 0
    if d == 0 or d % to == 0:
        return dsc
    out = np.zeros((dsc.shape[0], (d + to - 1) // to * to), dsc.dtype)
    out[:, :d] = dsc
    return out


class BuildBatch(object):
    """The argument tables of one `mad_set_build_many` call (several structures, one launch per stage), kept alive between steps."""

    def __init__(self, lib, jobs, r, lim_main, lim_sec, gw_sig=0.0):
        self.lib, self.r, self.lim_main, self.lim_sec, self.gw_sig = lib, int(r), int(lim_main), int(lim_sec), float(gw_sig)
        n = len(jobs)
        self.sets = [job[5] if len(job) > 5 and job[5] is not None else DeviceSet(lib) for job in jobs]
        self._keep = []
        coords, octave, subv, index, counts, slots = [], [], [], [], [], []
        for job in jobs:
            c, o = _c(job[1], np.int32).reshape(-1, 3), _c(job[2], np.int32)
            v, i = _c(job[3], np.float64).reshape(-1, 3), _c(job[4], np.int32)
            if not (len(c) == len(o) == len(v) == len(i)):
                raise ValueError("set_build_many: anchor arrays of different lengths")
            self._keep += [c, o, v, i]
            coords.append(c.ctypes.data); octave.append(o.ctypes.data); subv.append(v.ctypes.data); index.append(i.ctypes.data)
            counts.append(len(o))
            slots += [int(job[0][0]), int(job[0][1])]
        self.counts = counts
        self._h = (C.c_void_p * max(n, 1))(*[s.h.value for s in self.sets])
        self._slots = (C.c_int * max(2 * n, 1))(*slots)
        self._coords = (C.c_void_p * max(n, 1))(*coords)
        self._octave = (C.c_void_p * max(n, 1))(*octave)
        self._subv = (C.c_void_p * max(n, 1))(*subv)
        self._index = (C.c_void_p * max(n, 1))(*index)
        self._n = (C.c_int * max(n, 1))(*counts)

    def run(self):
        self.lib.set_orient_window(self.gw_sig)      # the window is state of the context: every build states its own, as set_build does
        for s, n in zip(self.sets, self.counts):
            s.n_anchors = n
        self.lib._chk(self.lib.dll.mad_set_build_many(self.lib.ctx, len(self.sets), self._h, self._slots, self._coords, self._octave,
                                                      self._subv, self._index, self._n, self.r, self.lim_main, self.lim_sec))
        return self.sets


class DeviceSet(object):
    """Device-resident oriented-anchor rows of one structure (mad_set)."""

    def __init__(self, lib, lane=None):
        self.lib = lib
        self.h = C.c_void_p()
        lib._chk(lib.dll.mad_set_create(lib.ctx, C.byref(self.h)))
        self.n_anchors = 0
        if lane is not None:
            self.bind_lane(lane)

    def lane(self):
        return int(self.lib.dll.mad_set_lane(self.lib.ctx, self.h))

    def is_wide(self):
        """True when the set holds the centred int8 rows of a wide set (built at r >= 11, or loaded with wide=True)."""
        return int(self.lib.dll.mad_set_is_wide(self.lib.ctx, self.h)) == 1

    def bind_lane(self, lane):
        """Put the set on lane `lane` (0..7): sets of one lane run in order on one stream.  Synchronises the context."""
        self.lib._chk(self.lib.dll.mad_set_bind_lane(self.lib.ctx, self.h, int(lane)))

    def stream(self):
        """The HIP stream (as an integer handle) the set's kernels are enqueued on."""
        return self.lib.dll.mad_set_stream(self.lib.ctx, self.h)

    def size(self):
        n = C.c_int64(0)
        a = C.c_int32(0)
        self.lib._chk(self.lib.dll.mad_set_size(self.lib.ctx, self.h, C.byref(n), C.byref(a)))
        return n.value, a.value

    def download(self, want_dsc=True, D=1024):
        n, _ = self.size()
        out = dict(anchor=np.zeros(n, np.int32), main=np.zeros(n, np.int32), sec=np.zeros(n, np.int32),
                   R=np.zeros((n, 3, 3)), dsc=np.zeros((n, D), np.int16) if want_dsc else None)
        self.lib._chk(self.lib.dll.mad_set_download(self.lib.ctx, self.h, _p(out["anchor"]), _p(out["main"]), _p(out["sec"]),
                                                    _p(out["R"]), _p(out["dsc"])))
        return out

    def close(self):
        if self.h and self.lib.ctx:
            self.lib.dll.mad_set_destroy(self.lib.ctx, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _localize(lib, dtype, coords, call):
    """Shared body of DeviceSpace.localize and Lib.localize_volume: output arrays, one C call, the project's error codes."""
    coords = np.asarray(coords)
    if coords.size == 0:
        coords = coords.reshape(0, 3)
    if coords.ndim != 2 or coords.shape[1] != 3 or not np.issubdtype(coords.dtype, np.integer):
        raise ValueError("localize: coords must be an integer (n, 3) array, got %s %s" % (coords.dtype, coords.shape))
    if len(coords) and (coords.min() < np.iinfo(np.int32).min or coords.max() > np.iinfo(np.int32).max):
        raise ValueError("localize: coordinates outside int32")
    c = _c(coords, np.int32)
    n = len(c)
    status, coord = np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    H, G = np.zeros((n, 3, 3), dtype), np.zeros((n, 3), dtype)
    nu = C.c_int64(0)
    lib._chk(call(_p(c), n, _p(status), _p(coord), _p(H), _p(G), C.byref(nu)))
    return status, coord, H, G, int(nu.value)


class DeviceSpace(object):
    """Device-resident scale space of one structure (mad_space): the volumes of MapSpace.build_space."""

    GRID, LOG, GAUSS = 0, 1, 2

    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p()
        lib._chk(lib.dll.mad_space_create(lib.ctx, C.byref(self.h)))
        self.shapes, self.kinds, self.dtypes = [], [], []

    def build(self, grid, pad=9, oct_mode="both", sig_init=2, sig_presmooth=1, slot_up=-1, slot_base=-1):
        """grid: float32 or float64 (X, Y, Z).  Fills the field slots with the gradient texels."""
        from . import scale_tables as st
        g = np.asarray(grid)
        if g.ndim != 3 or g.dtype not in (np.float32, np.float64):
            raise ValueError("density grid must be a 3-D float32 or float64 array")
        g = np.ascontiguousarray(g)
        self.shapes, self.kinds, self.dtypes = [], [], []      # a failed build leaves the space empty, as mad_space_build does
        mode = {"base": 1, "up": 2, "both": 3}[oct_mode]
        R = st.kernel_radius(sig_init)
        g0 = np.ascontiguousarray(st.gaussian_kernel1d(sig_init, 0, R)[::-1])
        g2 = np.ascontiguousarray(st.gaussian_kernel1d(sig_init, 2, R)[::-1])
        pre_R = st.kernel_radius(sig_presmooth) if (sig_presmooth and mode & 2) else 0
        pre = np.ascontiguousarray(st.gaussian_kernel1d(sig_presmooth, 0, pre_R)[::-1]) if pre_R else None
        P3 = C.c_void_p * 3
        lu = ev_w = ev_i = None
        keep = []
        if mode & 2 and min(g.shape) + 2 * pad >= 4:      # shorter lines: mad_space_build refuses them (MAD_EINVAL)
            tabs = [st.spline_tables(int(n) + 2 * pad) for n in g.shape]
            keep = tabs
            lu = P3(*[t[0].ctypes.data for t in tabs])
            ev_w = P3(*[t[1].ctypes.data for t in tabs])
            ev_i = P3(*[t[2].ctypes.data for t in tabs])
        self.lib._chk(self.lib.dll.mad_space_build(
            self.lib.ctx, self.h, _p(g), 1 if g.dtype == np.float64 else 0, g.shape[0], g.shape[1], g.shape[2], pad, mode,
            _p(g0), _p(g2), R, float(sig_init) ** 2, _p(pre), pre_R, lu, ev_w, ev_i, slot_up, slot_base))
        del keep
        n = C.c_int(0)
        dims, kind, f64 = np.zeros(6, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
        self.lib._chk(self.lib.dll.mad_space_info(self.lib.ctx, self.h, C.byref(n), _p(dims), _p(kind), _p(f64)))
        self.shapes = [tuple(int(v) for v in dims[3 * o:3 * o + 3]) for o in range(n.value)]
        self.kinds = [int(kind[o]) for o in range(n.value)]
        self.dtypes = [np.float64 if f64[o] else np.float32 for o in range(n.value)]
        for shape, kind in zip(self.shapes, self.kinds):
            slot = slot_up if kind == 0 else slot_base
            if slot >= 0:
                self.lib._field_dims[slot] = shape
        return self

    def download(self, entry, what):
        out = np.empty(self.shapes[entry], self.dtypes[entry])
        self.lib._chk(self.lib.dll.mad_space_download(self.lib.ctx, self.h, entry, what, _p(out)))
        return out

    def peaks(self, entry, threshold=5e-2, border=12, cap0=1 << 16):
        """-> (coords int (n, 3), values float64 (n,)) in skimage's order: descending value, row-major among equals.
        A float32 entry compares with float32(threshold), as numpy does; cap0 is the first capacity tried (it grows on MAD_ENOSPC)."""
        idx = val = None
        n = C.c_int64(0)

        def call(cap):
            nonlocal idx, val
            idx, val = np.zeros(cap, np.int64), np.zeros(cap, np.float64)
            return self.lib.dll.mad_space_peaks(self.lib.ctx, self.h, entry, threshold, border, _p(idx), _p(val), cap, C.byref(n)), n.value

        _retry_enospc(self.lib, call, int(cap0), slack=1024)
        idx, val = idx[:n.value], val[:n.value]
        order = np.argsort(idx, kind="stable")              # row-major, like np.nonzero
        idx, val = idx[order], val[order]
        order = np.argsort(-val, kind="stable")
        idx, val = idx[order], val[order]
        _, ny, nz = self.shapes[entry]
        coords = np.stack([idx // (ny * nz), (idx // nz) % ny, idx % nz], 1).astype(np.int64)
        return coords, val

    def patches(self, entry, coords, r):
        coords = _c(coords, np.int32).reshape(-1, 3)
        side = 2 * r + 1
        out = np.zeros((len(coords), side, side, side), self.dtypes[entry])
        self.lib._chk(self.lib.dll.mad_space_patches(self.lib.ctx, self.h, entry, _p(coords), len(coords), r, _p(out)))
        return out

    def localize(self, entry, coords):
        """Detector.check_localize of every voxel in `coords` (n, 3) on map_space[entry], on the device (mad_space_localize).
        -> (status int32 (n,): 0 rejected / 1 accepted / 2 undecided, coord int32 (n, 3), H (n, 3, 3), G (n, 3), n_undecided);
        H and G in the storage type of the entry."""
        entry = int(entry)
        dtype = self.dtypes[entry] if 0 <= entry < len(self.dtypes) else np.float32      # a bad entry: MAD_EINVAL from the library
        return _localize(self.lib, dtype, coords,
                         lambda c, n, st, co, H, G, nu: self.lib.dll.mad_space_localize(self.lib.ctx, self.h, entry, c, n, st, co, H, G, nu))

    def close(self):
        if self.h and self.lib.ctx:
            self.lib.dll.mad_space_destroy(self.lib.ctx, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lib(object):
    """One mad_ctx on one GPU."""

    def __init__(self, device=0):
        self.dll = load_library()
        self.ctx = C.c_void_p()
        rc = self.dll.mad_init(device, C.byref(self.ctx))
        if rc != 0:
            msg = self.dll.mad_last_error(None)
            self.ctx = None
            raise MadBackendError("MaD> mad_init(device=%d) failed (%s): %s -- the hot path runs on an MI355X only"
                                  % (device, ERRORS.get(rc, rc), msg.decode() if msg else ""))
        self.device = device
        self._fields = {}      # id(array) -> slot bookkeeping is done by the callers
        self._field_dims = {}  # slot -> (X, Y, Z) of the texels it holds (download_field)
        self._next_slot = 0
        self._free_slots = []
        self._eq_loaded = {}

    # -- plumbing -----------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            msg = self.dll.mad_last_error(self.ctx)
            raise MadBackendError("MaD> %s: %s" % (ERRORS.get(rc, rc), msg.decode() if msg else ""))

    def close(self):
        if self.ctx:
            self.dll.mad_destroy(self.ctx)
        self.ctx = None

    def synchronize(self):
        self._chk(self.dll.mad_synchronize(self.ctx))

    def stream(self):
        return self.dll.mad_stream(self.ctx)

    def set_overlap(self, on=True):
        """False: kernels of all lanes run one at a time (per-kernel timing); True (default): lanes overlap."""
        self._chk(self.dll.mad_set_overlap(self.ctx, 1 if on else 0))

    def timing_enable(self, on=True):
        self._chk(self.dll.mad_timing_enable(self.ctx, 1 if on else 0))

    def timing_reset(self):
        self._chk(self.dll.mad_timing_reset(self.ctx))

    def set_batching(self, on):
        """One GEMM launch for all matches of a `match_topk_many` bracket (True) or one per match (False, default)."""
        self._chk(self.dll.mad_set_batching(self.ctx, 1 if on else 0))

    def set_option(self, name, value):
        """Tuning values that change speed, never results (`mad_set_option`)."""
        self._chk(self.dll.mad_set_option(self.ctx, name.encode(), float(value)))

    def probe_peaks(self):
        """(device copy GB/s, int8 MFMA TOP/s) measured now on this device (mad_probe_peaks)."""
        c, m = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.dll.mad_probe_peaks(self.ctx, C.byref(c), C.byref(m)))
        return c.value, m.value

    def timing_get(self, what):
        t = C.c_double(0)
        n = C.c_int64(0)
        self._chk(self.dll.mad_timing_get(self.ctx, what.encode(), C.byref(t), C.byref(n)))
        return t.value, n.value

    # -- tables and fields ----------------------------------------------------------
    def set_eqsp(self, which, bounds, to_dom=None, adj_sec=None):
        bounds = _c(bounds, np.float64)
        to_dom = None if to_dom is None else _c(to_dom, np.float64)
        adj_sec = None if adj_sec is None else _c(adj_sec, np.float64)
        self._chk(self.dll.mad_set_eqsp(self.ctx, which, len(bounds), _p(bounds), _p(to_dom), _p(adj_sec)))

    def set_orient_window(self, gw_sig=0.0):
        """Orientator(gw_sig): Gaussian window on the orientation histogram (0 = none) for the following `orient` calls.  The window is
        state of the context; `set_build`, `set_build_many` and `BuildBatch.run` set it themselves for every build (their `gw_sig`,
        default 0), so what is set here does not reach them.  A change of window waits for the device (mad_synchronize)."""
        if getattr(self, "_gw_sig", 0.0) != float(gw_sig):
            self._chk(self.dll.mad_set_orient_window(self.ctx, float(gw_sig)))
            self._gw_sig = float(gw_sig)

    def new_slot(self):
        if self._free_slots:
            return self._free_slots.pop()
        s = self._next_slot
        self._next_slot += 1
        if s >= 64:
            raise MadBackendError("MaD> out of gradient-field slots; free some with free_field()")
        return s

    def localize_volume(self, vol, coords):
        """Detector.check_localize of every voxel in `coords` on a host LoG volume (float32 or float64, (X, Y, Z)), on the device
        (mad_localize_volume).  Same result tuple as DeviceSpace.localize."""
        v = np.asarray(vol)
        if v.ndim != 3 or v.dtype not in (np.float32, np.float64):
            raise ValueError("localize_volume: volume must be a 3-D float32 or float64 array, got %s %s" % (v.dtype, v.shape))
        v = np.ascontiguousarray(v)
        return _localize(self, v.dtype.type, coords,
                         lambda c, n, st, co, H, G, nu: self.dll.mad_localize_volume(
                             self.ctx, _p(v), 1 if v.dtype == np.float64 else 0, v.shape[0], v.shape[1], v.shape[2], c, n, st, co, H, G, nu))

    def upload_field(self, slot, grad):
        """grad: the reference's grad_list entry, shape (X, Y, Z, 3), any strides; or a (3, X, Y, Z) array."""
        g = np.asarray(grad)
        if g.ndim != 4:
            raise ValueError("gradient field must be 4-D")
        if g.shape[-1] == 3:
            g = np.moveaxis(g, -1, 0)
        elif g.shape[0] != 3:
            raise ValueError("gradient field must be (X, Y, Z, 3) or (3, X, Y, Z)")
        planes = [_c(g[i], np.float32) for i in range(3)]
        nx, ny, nz = planes[0].shape
        self._chk(self.dll.mad_upload_field(self.ctx, slot, _p(planes[0]), _p(planes[1]), _p(planes[2]), nx, ny, nz))
        self._field_dims[slot] = (nx, ny, nz)

    def upload_field_device(self, slot, dev_ptr, nx, ny, nz):
        self._chk(self.dll.mad_upload_field_device(self.ctx, slot, dev_ptr, nx, ny, nz))
        self._field_dims[slot] = (int(nx), int(ny), int(nz))

    def download_field(self, slot):
        """Diagnostic (mad_field_download): the texels of a slot as the kernels read them
        -> (float32 (X, Y, Z, 4) {gx, gy, gz, |g|}, uint32 (X, Y, Z) packed 4-byte texels)."""
        dims = self._field_dims.get(slot)
        if dims is None:      # nothing known to be there: the library says so
            self._chk(self.dll.mad_field_download(self.ctx, slot, None, None))
            raise MadBackendError("MaD> download_field: the size of slot %d is unknown to this binding" % slot)
        tex, tex4 = np.empty(tuple(dims) + (4,), np.float32), np.empty(tuple(dims), np.uint32)
        self._chk(self.dll.mad_field_download(self.ctx, slot, _p(tex), _p(tex4)))
        return tex, tex4

    def free_field(self, slot):
        self._chk(self.dll.mad_free_field(self.ctx, slot))
        self._field_dims.pop(slot, None)
        if slot not in self._free_slots:
            self._free_slots.append(slot)

    # -- stage API --------------------------------------------------------------------
    def orient(self, slot, octave, coords, r=8, lim_main=6, lim_sec=6, want_counts=True, Z=112):
        coords = _c(coords, np.int32).reshape(-1, 3)
        n = len(coords)
        cap = max(1, n * lim_main * lim_sec)
        ra, rm, rs = (np.zeros(cap, np.int32) for _ in range(3))
        R = np.zeros((cap, 9))
        cnt = np.zeros((cap, Z), np.int32) if want_counts else None
        nrows = C.c_int64(0)
        nrej = C.c_int32(0)
        self._chk(self.dll.mad_orient(self.ctx, slot, octave, _p(coords), n, r, lim_main, lim_sec, _p(ra), _p(rm), _p(rs), _p(R), _p(cnt),
                                      C.byref(nrows), cap, C.byref(nrej)))
        k = nrows.value
        return dict(anchor=ra[:k].copy(), main=rm[:k].copy(), sec=rs[:k].copy(), R=R[:k].reshape(k, 3, 3).copy(),
                    counts=None if cnt is None else cnt[:k].copy(), n_reject=nrej.value)

    def describe(self, slot, octave, coords, R, r=8, Zd=16, dsc_size=64):
        coords = _c(coords, np.int32).reshape(-1, 3)
        R = _c(R, np.float64).reshape(-1, 9)
        n = len(coords)
        out = np.zeros((n, dsc_size * Zd), np.int16)
        self._chk(self.dll.mad_describe_sized(self.ctx, slot, octave, _p(coords), _p(R), n, r, dsc_size, _p(out)))
        return out

    def correlate(self, hi, lo, cc):
        hi, lo = _pad_rows(_c(hi, np.int16)), _pad_rows(_c(lo, np.int16))
        n_hi, D = hi.shape
        n_lo = lo.shape[0]
        npairs = C.c_int64(0)
        ph = pl = ps = None

        def call(cap):
            nonlocal ph, pl, ps
            ph, pl, ps = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
            return self.dll.mad_correlate(self.ctx, _p(hi), n_hi, _p(lo), n_lo, D, cc, _p(ph), _p(pl), _p(ps), C.byref(npairs), cap), npairs.value

        _retry_enospc(self, call, 1 << 16)
        k = npairs.value
        return ph[:k].copy(), pl[:k].copy(), ps[:k].copy()

    def pose_score(self, pair_hi, pair_lo, pair_score, hi_p, hi_R, hi_meta, lo_p, lo_R, lo_meta, hi_cloud, lo_cloud,
                   dist=4.0, want_results=True):
        pair_hi, pair_lo = _c(pair_hi, np.int32), _c(pair_lo, np.int32)
        pair_score = _c(pair_score, np.float64)
        hi_p, lo_p = _c(hi_p, np.float64), _c(lo_p, np.float64)
        hi_R, lo_R = _c(hi_R, np.float64).reshape(-1, 9), _c(lo_R, np.float64).reshape(-1, 9)
        hi_meta, lo_meta = _c(hi_meta, np.int32), _c(lo_meta, np.int32)
        hi_cloud, lo_cloud = _c(hi_cloud, np.float64), _c(lo_cloud, np.float64)
        n = len(pair_hi)
        res = np.zeros((n, RESULT_COLS)) if want_results else None
        cnt = np.zeros(n, np.int32)
        self._chk(self.dll.mad_pose_score(self.ctx, _p(pair_hi), _p(pair_lo), _p(pair_score), n,
                                          _p(hi_p), _p(hi_R), _p(hi_meta), len(hi_p), _p(lo_p), _p(lo_R), _p(lo_meta), len(lo_p),
                                          _p(hi_cloud), len(hi_cloud), _p(lo_cloud), len(lo_cloud), dist, _p(res), _p(cnt)))
        return res, cnt

    def topk(self, counts, k):
        counts = _c(counts, np.int32)
        k = min(int(k), len(counts))
        order = np.zeros(max(k, 1), np.int64)
        self._chk(self.dll.mad_topk(self.ctx, _p(counts), len(counts), k, _p(order)))
        return order[:k]

    # -- device-resident pipeline -------------------------------------------------------
    def set_build(self, slots, anc_coords, anc_octave, anc_subv, anc_index, r=8, lim_main=6, lim_sec=6, into=None, gw_sig=0.0):
        """Orient + describe the anchors into a device-resident set.  Asynchronous; pass `into` to rebuild an
        existing set in place (its device buffers are reused).  `gw_sig`: the Gaussian window of Orientator(gw_sig) for THIS
        build (the window is state of the context: it is set here for every build, so that an Orientator object used earlier on
        the same context cannot leak its window into a set)."""
        self.set_orient_window(gw_sig)
        s = into if into is not None else DeviceSet(self)
        slots = (C.c_int * 2)(int(slots[0]), int(slots[1]))
        anc_coords = _c(anc_coords, np.int32).reshape(-1, 3)
        anc_octave = _c(anc_octave, np.int32)
        anc_subv = _c(anc_subv, np.float64).reshape(-1, 3)
        anc_index = _c(anc_index, np.int32)
        s.n_anchors = len(anc_octave)
        self._chk(self.dll.mad_set_build(self.ctx, s.h, slots, _p(anc_coords), _p(anc_octave), _p(anc_subv), _p(anc_index),
                                         len(anc_octave), r, lim_main, lim_sec))
        return s

    def prepare_build_many(self, jobs, r=8, lim_main=6, lim_sec=6, gw_sig=0.0):
        """jobs: [(slots, anc_coords, anc_octave, anc_subv, anc_index, into-or-None), ...] -> a BuildBatch whose `run()` enqueues
        orientation + description of all of them with one launch per stage (`mad_set_build_many`) and returns the sets.
        Prepared once, run every step: the argument arrays are converted and pinned down here."""
        return BuildBatch(self, jobs, r, lim_main, lim_sec, gw_sig)

    def set_build_many(self, jobs, r=8, lim_main=6, lim_sec=6, gw_sig=0.0):
        return self.prepare_build_many(jobs, r, lim_main, lim_sec, gw_sig).run()

    def set_load(self, row_anchor, row_main, row_R, dsc, anc_subv, anc_index, anc_octave, wide=False):
        """wide: the rows were described at a radius of 11 or more (patch sizes 22 .. 25) and hold counts up to 216: the set is
        marked wide before the load (include/mad_amd.h, "Wide sets") and matches wide sets only."""
        s = DeviceSet(self)
        if wide:
            self._chk(self.dll.mad_set_mark_wide(self.ctx, s.h, 1))
        row_anchor, row_main = _c(row_anchor, np.int32), _c(row_main, np.int32)
        row_R = _c(row_R, np.float64).reshape(-1, 9)
        dsc = _c(dsc, np.int16)
        if dsc.ndim != 2:
            dsc = dsc.reshape(len(row_anchor), -1)
        dsc = _pad_rows(dsc)
        anc_subv = _c(anc_subv, np.float64).reshape(-1, 3)
        anc_index, anc_octave = _c(anc_index, np.int32), _c(anc_octave, np.int32)
        s.n_anchors = len(anc_index)
        self._chk(self.dll.mad_set_load(self.ctx, s.h, len(row_anchor), _p(row_anchor), _p(row_main), _p(row_R), _p(dsc),
                                        dsc.shape[1] if len(dsc) else 1024, _p(anc_subv), _p(anc_index), _p(anc_octave), len(anc_index)))
        return s

    def match_topk(self, hi, lo, cc, dist, k):
        k = int(k)
        res = np.zeros((max(k, 1), RESULT_COLS))
        idx = np.zeros(max(k, 1), np.int64)
        n_out = C.c_int64(0)
        stats = np.zeros(4, np.int64)
        self._chk(self.dll.mad_match_topk(self.ctx, hi.h, lo.h, cc, dist, k, _p(res), _p(idx), C.byref(n_out), _p(stats)))
        g = n_out.value
        return res[:g], idx[:g], dict(n_pairs=int(stats[0]), l_hi=int(stats[1]), l_lo=int(stats[2]), n_corr=int(stats[3]))

    def _many_call(self, plain, with_used, his, lo, cc, dist, k, want_used):
        """One bracket through `plain`, or with want_used through `with_used`, which also takes the two flag arrays -> its arrays."""
        h = self._many_args(his, lo, k, want_used)
        used = (_p(h["used_hi"]), _p(h["used_lo"])) if want_used else ()
        self._chk((with_used if want_used else plain)(self.ctx, h["n"], h["arr"], lo.h, cc, dist, h["k"], _p(h["res"]), _p(h["idx"]),
                                                      _p(h["n_out"]), _p(h["stats"]), *used))
        return h

    def match_topk_many(self, his, lo, cc, dist, k, want_used=False):
        """[(rows, pair_index, stats)] for every subunit set of `his` against `lo`; see mad_match_topk_many.  want_used=True:
        [(rows, pair_index, stats, used_hi, used_lo)], each match's anchor-use flags as bool arrays (mad_match_topk_many2)."""
        return self._many_unpack(self._many_call(self.dll.mad_match_topk_many, self.dll.mad_match_topk_many2, his, lo, cc, dist, k, want_used))

    @staticmethod
    def _many_args(his, lo, k, want_used):
        """Output arrays of one bracket (and, with want_used, its flag arrays: hi flags back to back, lo flags n x anchors of lo)."""
        k = int(k)
        n = len(his)
        h = dict(n=n, k=k, res=np.zeros((max(n, 1), max(k, 1), RESULT_COLS)), idx=np.zeros((max(n, 1), max(k, 1)), np.int64),
                 n_out=np.zeros(max(n, 1), np.int64), stats=np.zeros((max(n, 1), 4), np.int64), sets=(list(his), lo),
                 arr=(C.c_void_p * max(n, 1))(*[x.h.value for x in his]), want_used=bool(want_used))
        if want_used:
            h["hi_off"] = np.concatenate([[0], np.cumsum([x.n_anchors for x in his], dtype=np.int64)]).astype(np.int64)
            h["used_hi"] = np.zeros(max(int(h["hi_off"][-1]), 1), np.uint8)
            h["used_lo"] = np.zeros((max(n, 1), max(lo.n_anchors, 1)), np.uint8)
        return h

    @staticmethod
    def _many_unpack(h):
        out = []
        for i in range(h["n"]):
            g = int(h["n_out"][i])
            st = h["stats"][i]
            row = (h["res"][i, :g], h["idx"][i, :g], dict(n_pairs=int(st[0]), l_hi=int(st[1]), l_lo=int(st[2]), n_corr=int(st[3])))
            if h["want_used"]:
                a, b = int(h["hi_off"][i]), int(h["hi_off"][i + 1])
                n_lo = h["sets"][1].n_anchors
                row += (h["used_hi"][a:b].astype(bool), h["used_lo"][i, :n_lo].astype(bool))
            out.append(row)
        return out

    def last_pose_kernel(self):
        """0 k_pose_lds, 1 k_pose_lds32, 2 k_pose (global cell list): the kernel of the most recently enqueued match."""
        return int(self.dll.mad_last_pose_kernel(self.ctx))

    def last_pose_plan(self):
        """What the host chose for the most recently enqueued pose stage (mad_last_pose_plan), as a dict; every value is -1 before
        the first one.  Read it before match_fetch / match_results: completing a pruned match enqueues a pose stage of its own."""
        info = _PosePlanInfo()
        self._chk(self.dll.mad_last_pose_plan(self.ctx, C.byref(info)))
        out = {}
        for name, _ in _PosePlanInfo._fields_:
            if name == "reserved":
                continue
            v = getattr(info, name)
            out[name] = tuple(v) if hasattr(v, "__len__") else v
        return out

    def last_pose_selected(self):
        """Pairs of the last completed match that went through the exact pose search (the rest were excluded by their bounds)."""
        return int(self.dll.mad_last_pose_selected(self.ctx))

    def device_allocations(self):
        """Device buffers (re)allocated by this context so far (mad_device_allocations): 0 new ones across a steady-state region."""
        return int(self.dll.mad_device_allocations(self.ctx))

    def match_topk_many_begin(self, his, lo, cc, dist, k, want_used=False):
        """Enqueue every match and return a handle; `match_topk_many_finish(handle)` waits and unpacks.  In between
        the caller may build the sets of its next batch (not the ones this bracket reads).  want_used=True: every match also
        hands back its anchor-use flags (mad_match_topk_many_begin2), and finish returns 5-tuples."""
        h = self._many_call(self.dll.mad_match_topk_many_begin, self.dll.mad_match_topk_many_begin2, his, lo, cc, dist, k, want_used)
        self._open_brackets = getattr(self, "_open_brackets", []) + [h]      # at most three (MAD_BRACKETS); they finish in the order they began
        return h

    def match_topk_many_finish(self, h):
        pending = getattr(self, "_open_brackets", [])
        if not pending or pending[0] is not h:
            raise MadBackendError("MaD> match_topk_many_finish: brackets finish in the order they were begun")
        self._open_brackets = pending[1:]      # the library closes the bracket whether or not one of its matches failed
        self._chk(self.dll.mad_match_topk_many_finish(self.ctx))
        return self._many_unpack(h)

    def match_shard_pairs(self, hi, lo, lo_begin, lo_end, cc):
        """Stage B of a sharded match -> (used_hi flags, used_lo flags, n_pairs) of the lo-row block [lo_begin, lo_end)."""
        used_hi, used_lo = np.zeros(max(hi.n_anchors, 1), np.uint8), np.zeros(max(lo.n_anchors, 1), np.uint8)
        n = C.c_int64(0)
        self._chk(self.dll.mad_match_shard_pairs(self.ctx, hi.h, lo.h, lo_begin, lo_end, cc, _p(used_hi), _p(used_lo), C.byref(n)))
        return used_hi[:hi.n_anchors], used_lo[:lo.n_anchors], n.value

    def match_shard_topk(self, hi, lo, used_hi_all, used_lo_all, dist, k):
        """Stage C -> (rows (m, 23), counts (m,), global pair ranks (m,), l_hi) with m <= k."""
        uh, ul = _c(used_hi_all, np.uint8), _c(used_lo_all, np.uint8)
        assert len(uh) == hi.n_anchors and len(ul) == lo.n_anchors
        res = np.zeros((k, RESULT_COLS))
        rank, cnt = np.zeros(k, np.int64), np.zeros(k, np.int32)
        n, l_hi = C.c_int64(0), C.c_int64(0)
        self._chk(self.dll.mad_match_shard_topk(self.ctx, hi.h, lo.h, _p(uh), _p(ul), dist, k, _p(res), _p(rank), _p(cnt), C.byref(n),
                                                C.byref(l_hi)))
        m = n.value
        return res[:m].copy(), cnt[:m].copy(), rank[:m].copy(), l_hi.value

    def match_shard_record_doubles(self, k):
        return int(self.dll.mad_match_shard_record_doubles(int(k)))

    def match_shard_begin(self, hi, lo, lo_begin, lo_end, n_lo, cc, flags_ptr):
        """Stage B, asynchronous on hi's lane: the shard's flags go to device memory at `flags_ptr` (hi.n_anchors + lo.n_anchors bytes)."""
        self._chk(self.dll.mad_match_shard_begin(self.ctx, hi.h, lo.h, int(lo_begin), int(lo_end), int(n_lo), cc, int(flags_ptr)))

    def match_shard_score(self, hi, lo, flags_all_ptr, dist, k, out_ptr):
        """Stage C, asynchronous: the shard's record (match_shard_record_doubles(k) float64) goes to device memory at `out_ptr`."""
        self._chk(self.dll.mad_match_shard_score(self.ctx, hi.h, lo.h, int(flags_all_ptr), dist, int(k), int(out_ptr)))

    def match_shard_collect(self, hi, all_ptr, n):
        """The n float64 at device address `all_ptr` on their way to the host, behind everything enqueued on hi's lane -> ticket."""
        t = C.c_int(0)
        self._chk(self.dll.mad_match_shard_collect(self.ctx, hi.h, int(all_ptr), int(n), C.byref(t)))
        return t.value

    def match_shard_wait(self, ticket, n):
        out = np.zeros(int(n))
        self._chk(self.dll.mad_match_shard_wait(self.ctx, int(ticket), _p(out), int(n)))
        return out

    def match_shard_merge(self, hi, all_ptr, nranks, k, merged_ptr):
        """k_shard_merge on hi's lane: the `nranks` records at device address `all_ptr` -> one record at `merged_ptr` (the order of
        dist.merge_topk).  nranks * k > SHARD_MERGE_MAX raises (EDOM)."""
        self._chk(self.dll.mad_match_shard_merge(self.ctx, hi.h, int(all_ptr), int(nranks), int(k), int(merged_ptr)))

    # -- the exchanges of a sharded step inside the library (mad_dist.hip; mad_amd/dist.py::LibComm drives them) ---------
    def dist_unique_id(self):
        """The 128 bytes rank 0 hands to every rank of the communicator (loads RCCL)."""
        buf = C.create_string_buffer(DIST_ID_BYTES)
        self._chk(self.dll.mad_dist_unique_id(self.ctx, buf))
        return buf.raw

    def dist_init(self, nranks, rank, unique_id=None):
        """unique_id None: the rehearsal communicator (one rank of nranks alone on its GPU, RCCL not loaded)."""
        if unique_id is not None and len(unique_id) != DIST_ID_BYTES:
            raise ValueError("dist_init: a unique id has %d bytes" % DIST_ID_BYTES)
        self._chk(self.dll.mad_dist_init(self.ctx, int(nranks), int(rank), unique_id))

    def dist_destroy(self):
        self._chk(self.dll.mad_dist_destroy(self.ctx))

    def dist_info(self):
        """-> (nranks, rank, rehearsal)"""
        n, r, e = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.dll.mad_dist_info(self.ctx, C.byref(n), C.byref(r), C.byref(e)))
        return n.value, r.value, bool(e.value)

    def dist_rehearse_flags(self, peer_ptr, n):
        self._chk(self.dll.mad_dist_rehearse_flags(self.ctx, int(peer_ptr) if peer_ptr else None, int(n)))

    def dist_or_allreduce(self, stream, flags_ptr, n):
        self._chk(self.dll.mad_dist_or_allreduce(self.ctx, stream, int(flags_ptr), int(n)))

    def dist_allgather(self, stream, send_ptr, recv_ptr, bytes_per_rank):
        self._chk(self.dll.mad_dist_allgather(self.ctx, stream, int(send_ptr), int(recv_ptr), int(bytes_per_rank)))

    def dist_allgather_topk(self, hi, mine_ptr, all_ptr, k, merged_ptr):
        self._chk(self.dll.mad_dist_allgather_topk(self.ctx, hi.h, int(mine_ptr), int(all_ptr), int(k), int(merged_ptr)))

    def dist_scratch(self, lane, which, nbytes):
        """Device address of the grow-only buffer `which` (DIST_BUF_*) of `lane`, at least nbytes long."""
        p = C.c_void_p()
        self._chk(self.dll.mad_dist_scratch(self.ctx, int(lane), int(which), int(nbytes), C.byref(p)))
        return int(p.value)

    def dist_upload(self, dev_ptr, array):
        """Host array -> device memory at `dev_ptr`, synchronous (set-up, rehearsals, tests)."""
        a = np.ascontiguousarray(array)
        self._chk(self.dll.mad_dist_copy(self.ctx, int(dev_ptr), _p(a), a.nbytes, 0))

    def dist_download(self, dev_ptr, n, dtype=np.float64):
        out = np.zeros(int(n), dtype)
        self._chk(self.dll.mad_dist_copy(self.ctx, _p(out), int(dev_ptr), out.nbytes, 1))
        return out

    # -- a structure's rows built in shares (SURVEY.md 8(e) stage A; the all-gather is mad_amd/dist.py's, or mad_dist_allgather) --------
    def set_wire_bytes(self, cap_rows, D=1024):
        n = int(self.dll.mad_set_wire_bytes(int(D), int(cap_rows)))
        if n < 0:
            raise ValueError("set_wire_bytes(%r, %r)" % (cap_rows, D))
        return n

    def set_export(self, share, cap_rows, wire=None, device_ptr=None):
        """Wire image of a built set.  device_ptr: address of device memory of set_wire_bytes(cap_rows) bytes (asynchronous
        on the set's stream); otherwise a host uint8 array is filled (and returned)."""
        if device_ptr is not None:
            self._chk(self.dll.mad_set_export(self.ctx, share.h, int(device_ptr), 1, int(cap_rows)))
            return None
        nbytes = self.set_wire_bytes(cap_rows)
        if wire is None:
            wire = np.zeros(nbytes, np.uint8)
        if wire.dtype != np.uint8 or wire.size != nbytes or not wire.flags.c_contiguous:
            raise ValueError("set_export: wire must be a contiguous uint8 array of %d bytes" % nbytes)
        self._chk(self.dll.mad_set_export(self.ctx, share.h, _p(wire), 0, int(cap_rows)))
        return wire

    def set_import(self, n_shares, cap_rows, anc_coords, anc_octave, anc_subv, anc_index, wires=None, device_ptr=None, into=None):
        """The full set of a structure from the wire images of its n_shares shares (anchor a was built in share a % n_shares).
        wires: host uint8 array (n_shares x set_wire_bytes), or device_ptr: the same bytes in device memory (asynchronous)."""
        s = into if into is not None else DeviceSet(self)
        anc_octave = _c(anc_octave, np.int32)
        anc_subv = _c(anc_subv, np.float64).reshape(-1, 3)
        anc_index = _c(anc_index, np.int32)
        anc_coords = None if anc_coords is None else _c(anc_coords, np.int32).reshape(-1, 3)
        n = len(anc_octave)
        if len(anc_subv) != n or len(anc_index) != n or (anc_coords is not None and len(anc_coords) != n):
            raise ValueError("set_import: anchor arrays of different lengths")
        if device_ptr is not None:
            src, on_dev = int(device_ptr), 1
        else:
            wires = np.ascontiguousarray(wires, dtype=np.uint8)
            if wires.size != n_shares * self.set_wire_bytes(cap_rows):
                raise ValueError("set_import: %d bytes for %d shares of %d" % (wires.size, n_shares, self.set_wire_bytes(cap_rows)))
            src, on_dev = _p(wires), 0
        s.n_anchors = n
        self._chk(self.dll.mad_set_import(self.ctx, s.h, src, on_dev, int(n_shares), int(cap_rows), _p(anc_coords), _p(anc_octave),
                                          _p(anc_subv), _p(anc_index), n))
        return s

    def match_fetch(self, n_pairs):
        ph, pl = np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32)
        ps, cn = np.zeros(n_pairs), np.zeros(n_pairs, np.int32)
        self._chk(self.dll.mad_match_fetch(self.ctx, _p(ph), _p(pl), _p(ps), _p(cn), n_pairs))
        return ph, pl, ps, cn

    def match_results(self, hi, lo, n_pairs):
        res = np.zeros((max(n_pairs, 1), RESULT_COLS))
        self._chk(self.dll.mad_match_results(self.ctx, hi.h, lo.h, _p(res), n_pairs))
        return res[:n_pairs]

    def match_used(self, n_hi_anchors, n_lo_anchors):
        uh, ul = np.zeros(max(n_hi_anchors, 1), np.uint8), np.zeros(max(n_lo_anchors, 1), np.uint8)
        self._chk(self.dll.mad_match_used(self.ctx, _p(uh), n_hi_anchors, _p(ul), n_lo_anchors))
        return uh[:n_hi_anchors].astype(bool), ul[:n_lo_anchors].astype(bool)

    def pose_cluster_many(self, rows_list, clouds, n_samples_list, rmsd_thresh=10.0):
        """The greedy cloud-RMSD clustering of MaD._filter_dsc_pairs for several matches in one call (mad_pose_cluster_many).
        rows_list[m]: the match's result rows, float64 (len, 23), sorted as _filter_dsc_pairs sorts them; clouds[m]: its hi cloud
        (N, 3); n_samples_list[m]: rows that take part (min(len, n_samples) do).  Per match (owner int32 [n], d2min float64 [n],
        n_done, status): owner[i] = the row that leads row i's cluster; status 1 = row n_done lies inside the guard band, run the
        host loop for this match (owner is -1 from there on).  More than POSE_CLUSTER_MAX_N rows in a match: MadBackendError (EDOM)."""
        nm = len(rows_list)
        if not (len(clouds) == len(n_samples_list) == nm):
            raise ValueError("pose_cluster_many: %d row lists, %d clouds, %d sample counts" % (nm, len(clouds), len(n_samples_list)))
        rows, cl, ns = [], [], []
        for r, c, k in zip(rows_list, clouds, n_samples_list):
            r = _c(r, np.float64).reshape(-1, RESULT_COLS)
            if int(k) < 0:
                raise ValueError("pose_cluster_many: n_samples = %d" % int(k))
            rows.append(r)
            cl.append(_c(c, np.float64).reshape(-1, 3))
            ns.append(min(len(r), int(k)))
        owner = [np.zeros(n, np.int32) for n in ns]
        d2min = [np.zeros(n, np.float64) for n in ns]
        n_rows, n_cloud = np.array(ns, np.int32), np.array([len(c) for c in cl], np.int32)
        n_done, status = np.zeros(max(nm, 1), np.int32), np.zeros(max(nm, 1), np.int32)
        PP = C.c_void_p * max(nm, 1)
        ptrs = [PP(*[a.ctypes.data if a.size else None for a in arrs]) for arrs in (rows, cl, owner, d2min)]
        self._chk(self.dll.mad_pose_cluster_many(self.ctx, nm, ptrs[0], _p(n_rows), ptrs[1], _p(n_cloud), float(rmsd_thresh),
                                                 ptrs[2], ptrs[3], _p(n_done), _p(status)))
        return [(owner[m], d2min[m], int(n_done[m]), int(status[m])) for m in range(nm)]

    # -- assembly ranking ------------------------------------------------------------------
    def _rank_result(self, rc, width, idx, key, rank, n_out, n_total, status):
        """(status, entries, n_total) of a mad_rank_* call: status "ok" with entries = (idx [m][width], key [m], rank [m]), or
        "edom" / "enospc" / "budget" with entries None -- the three answers after which the caller runs the host loop."""
        if rc == EDOM:
            return "edom", None, 0
        if rc == ENOSPC:
            return "enospc", None, int(n_total.value)
        self._chk(rc)
        if status.value:
            return "budget", None, 0
        m = int(n_out.value)
        return "ok", (idx[:m * width].reshape(m, width).copy(), key[:m].copy(), rank[:m].copy()), int(n_total.value)

    def rank_copies(self, overlap, n_copies, cap, max_overlap=None, launch_items=0, budget=0):
        """The head of assembly.rank_copies(overlap, n_copies) (mad_rank_copies).  max_overlap None: the first `cap` entries (TOP);
        else every entry whose maximum is <= max_overlap, up to `cap` of them (BELOW).  launch_items: ranks per kernel launch
        (0: the default), budget: items the call may evaluate (0: the default).  Returns (status, (idx, max, rank), n_total), see
        _rank_result; last_error() has the reason of an "edom"."""
        t = _c(overlap, np.float64)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("rank_copies: overlap has shape %s" % (t.shape,))
        n, c, cap = len(t), int(n_copies), max(int(cap), 0)
        room = max(min(cap, RANK_MAX_OUT), 1)
        idx, key, rank = np.zeros(room * max(c, 1), np.int32), np.zeros(room, np.float64), np.zeros(room, np.int64)
        n_out, n_total, status = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        mode = RANK_TOP if max_overlap is None else RANK_BELOW
        rc = self.dll.mad_rank_copies(self.ctx, _p(t), n, c, mode, 0.0 if max_overlap is None else float(max_overlap), min(cap, room),
                                      int(launch_items), int(budget), _p(idx), _p(key), _p(rank), C.byref(n_out), C.byref(n_total),
                                      C.byref(status))
        return self._rank_result(rc, c, idx, key, rank, n_out, n_total, status)

    def rank_models(self, overlap, groups, cap, out_cap=None, launch_items=0, budget=0):
        """Candidates for the head of assembly.rank_models(overlap, groups) (mad_rank_models): every pick whose device sum lies
        within the band of the cap-th smallest, in (device sum, rank) order -- a superset of the reference's first `cap` entries.
        groups: lists of consecutive rows, together 0 .. n - 1 (what build_models makes); anything else is an "edom".
        Returns (status, (picks, device sums, ranks), n_total)."""
        t = _c(overlap, np.float64)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("rank_models: overlap has shape %s" % (t.shape,))
        n, g, cap = len(t), len(groups), max(int(cap), 0)
        first, at = [0], 0
        for grp in groups:
            if list(grp) != list(range(at, at + len(grp))):
                return "edom", None, 0
            at += len(grp)
            first.append(at)
        out_cap = RANK_MAX_OUT if out_cap is None else max(int(out_cap), cap)
        room = max(min(out_cap, RANK_MAX_OUT), 1)
        idx, key, rank = np.zeros(room * max(g, 1), np.int32), np.zeros(room, np.float64), np.zeros(room, np.int64)
        n_out, n_total, status = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        first = np.array(first, np.int32)
        rc = self.dll.mad_rank_models(self.ctx, _p(t), n, _p(first), g, min(cap, room), room, int(launch_items), int(budget),
                                      _p(idx), _p(key), _p(rank), C.byref(n_out), C.byref(n_total), C.byref(status))
        return self._rank_result(rc, g, idx, key, rank, n_out, n_total, status)

    def last_rank_plan(self):
        """(launches, evaluated, skipped, band_extra) of the most recent rank_copies / rank_models (mad_last_rank_plan): kernel
        launches over rank ranges, items whose key was formed, items jumped over by prefix pruning, and whether the band of
        rank_models held more than `cap` candidates."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._chk(self.dll.mad_last_rank_plan(self.ctx, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, bool(d.value)

    def last_error(self):
        msg = self.dll.mad_last_error(self.ctx)
        return msg.decode() if msg else ""

    # -- refinement / density / ccc --------------------------------------------------------
    def upload_density(self, grid, origin, voxsp):
        grid = _c(grid, np.float32)
        nx, ny, nz = grid.shape
        self._chk(self.dll.mad_upload_density(self.ctx, _p(grid), nx, ny, nz, origin[0], origin[1], origin[2], voxsp))
        self._density_dims = (nx, ny, nz)

    def density_dims(self):
        """Shape of the map given to upload_density, or None."""
        return getattr(self, "_density_dims", None)

    def refine(self, coords, n_steps=500, max_step=0.5, min_step=0.01):
        """coords: (n_cand, n_atoms, 3) or (n_atoms, 3).  Returns (coords, converged[], last_step[])."""
        c = _c(coords, np.float64).copy()
        single = c.ndim == 2
        if single:
            c = c[None]
        n_cand, n_atoms, _ = c.shape
        conv, last = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32)
        self._chk(self.dll.mad_refine(self.ctx, _p(c), n_cand, n_atoms, n_steps, max_step, min_step, _p(conv), _p(last)))
        if single:
            return c[0], bool(conv[0]), int(last[0])
        return c, conv.astype(bool), last

    def last_refine_plan(self):
        """(G, in_registers) of the most recent refinement (mad_last_refine_plan): workgroups per candidate, and whether the atoms
        stayed in registers (k_refine<8>) or were walked in global memory (k_refine<0>); (-1, -1) before the first."""
        g, reg = C.c_int(-1), C.c_int(-1)
        self._chk(self.dll.mad_last_refine_plan(self.ctx, C.byref(g), C.byref(reg)))
        return g.value, reg.value

    @staticmethod
    def _bodies(who, coords_list, mass_list):
        """Bodies as the assembly calls take them: (atoms (N, 3), mass (N), first_atom (B + 1) int64)."""
        if len(coords_list) != len(mass_list):
            raise ValueError("%s: %d bodies, %d mass arrays" % (who, len(coords_list), len(mass_list)))
        parts = [_c(c, np.float64).reshape(-1, 3) for c in coords_list]
        ms = [_c(m, np.float64).reshape(-1) for m in mass_list]
        for b, (c, m) in enumerate(zip(parts, ms)):
            if len(c) != len(m):
                raise ValueError("%s: mass: body %d has %d masses for %d atoms" % (who, b, len(m), len(c)))
        first = np.zeros(len(parts) + 1, np.int64)
        first[1:] = np.cumsum([len(c) for c in parts])
        atoms = np.concatenate(parts, axis=0) if parts else np.zeros((0, 3))
        mass = np.concatenate(ms) if ms else np.zeros(0)
        return np.ascontiguousarray(atoms), np.ascontiguousarray(mass), first

    def assembly_density(self, coords_list, mass_list, resolution, want_model=True, want_residual=True):
        """The model of placed bodies on the lattice of the map given to upload_density (mad_assembly_density) -> (M float64 or
        None, s, map - s M float32 or None)."""
        atoms, mass, first = self._bodies("assembly_density", coords_list, mass_list)
        dims = self.density_dims()
        model = np.empty(dims, np.float64) if want_model and dims else None
        res = np.empty(dims, np.float32) if want_residual and dims else None
        s = C.c_double(0.0)
        self._chk(self.dll.mad_assembly_density(self.ctx, len(first) - 1, _p(atoms), _p(mass), _p(first), resolution, _p(model), C.byref(s), _p(res)))
        return model, s.value, res

    def assembly_refine(self, coords_list, mass_list, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None):
        """The bodies refined together against the map given to upload_density (mad_assembly_refine) -> ([coords (n_b, 3)],
        R (B, 3, 3), T (B, 3), converged (B) bool, last_step (B), s of every round that ran)."""
        atoms, mass, first = self._bodies("assembly_refine", coords_list, mass_list)
        B = len(first) - 1
        fx = None
        if fixed is not None:
            fx = _c(np.asarray(fixed, bool), np.uint8).reshape(-1)
            if len(fx) != B:
                raise ValueError("assembly_refine: fixed has %d entries for %d bodies" % (len(fx), B))
        n_steps = _whole("assembly_refine", "n_steps", n_steps)
        out = np.empty_like(atoms)
        rot, trans = np.zeros((B, 3, 3)), np.zeros((B, 3))
        conv, last = np.zeros(B, np.int32), np.zeros(B, np.int32)
        scale = np.zeros(max((n_steps + 3) // 4, 1))
        rounds = C.c_int32(0)
        self._chk(self.dll.mad_assembly_refine(self.ctx, B, _p(atoms), _p(mass), _p(first), _p(fx), resolution, n_steps, max_step, min_step,
                                               _p(out), _p(rot), _p(trans), _p(conv), _p(last), _p(scale), C.byref(rounds)))
        return ([out[first[b]:first[b + 1]].copy() for b in range(B)], rot, trans, conv.astype(bool), last, scale[:rounds.value].copy())

    def assembly_refine_symmetric(self, coords_list, mass_list, R, T, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None):
        """The units refined under the operators x -> x @ R[g] + T[g] (R (K, 3, 3), T (K, 3), operator 0 the identity) against the
        map given to upload_density (mad_assembly_refine_symmetric) -> per UNIT what assembly_refine returns per body."""
        who = "assembly_refine_symmetric"
        atoms, mass, first = self._bodies(who, coords_list, mass_list)
        U = len(first) - 1
        rot_in, tr_in = _c(R, np.float64), _c(T, np.float64)
        if rot_in.ndim != 3 or rot_in.shape[1:] != (3, 3) or tr_in.shape != (len(rot_in), 3):
            raise ValueError("%s: R of shape %s and T of shape %s, not (K, 3, 3) and (K, 3)" % (who, rot_in.shape, tr_in.shape))
        fx = None
        if fixed is not None:
            fx = _c(np.asarray(fixed, bool), np.uint8).reshape(-1)
            if len(fx) != U:
                raise ValueError("%s: fixed has %d entries for %d units" % (who, len(fx), U))
        n_steps = _whole(who, "n_steps", n_steps)
        out = np.empty_like(atoms)
        rot, trans = np.zeros((U, 3, 3)), np.zeros((U, 3))
        conv, last = np.zeros(U, np.int32), np.zeros(U, np.int32)
        scale = np.zeros(max((n_steps + 3) // 4, 1))
        rounds = C.c_int32(0)
        self._chk(self.dll.mad_assembly_refine_symmetric(self.ctx, U, _p(atoms), _p(mass), _p(first), _p(fx), len(rot_in), _p(rot_in), _p(tr_in),
                                                         resolution, n_steps, max_step, min_step, _p(out), _p(rot), _p(trans), _p(conv),
                                                         _p(last), _p(scale), C.byref(rounds)))
        return ([out[first[b]:first[b + 1]].copy() for b in range(U)], rot, trans, conv.astype(bool), last, scale[:rounds.value].copy())

    def last_assembly_plan(self):
        """(G of body 0, in_registers, workgroups) of the most recent assembly_refine or assembly_refine_symmetric
        (mad_last_assembly_plan); -1 before the first."""
        g, reg, wgs = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        self._chk(self.dll.mad_last_assembly_plan(self.ctx, C.byref(g), C.byref(reg), C.byref(wgs)))
        return g.value, reg.value, wgs.value

    def flex_network(self, coords, cutoff):
        """The elastic network of (n, 3) coordinates (mad_flex_network) -> (first int32 [n + 1], nbr int32, rest float64): every pair
        within `cutoff`, a row per atom, ascending; bit for bit flexfit.network_numpy's."""
        x = _c(coords, np.float64).reshape(-1, 3)
        n = len(x)
        first = np.zeros(n + 1, np.int32)
        held = {}

        def call(cap):
            held["nbr"], held["rest"] = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)
            total = C.c_int64(0)
            rc = self.dll.mad_flex_network(self.ctx, n, _p(x), float(cutoff), _p(first), cap, _p(held["nbr"]), _p(held["rest"]), C.byref(total))
            held["total"] = total.value
            return rc, total.value

        _retry_enospc(self, call, 64 * max(n, 1))
        return first, held["nbr"][:held["total"]].copy(), held["rest"][:held["total"]].copy()

    def flex_fit(self, coords, network, stiffness=1.0, n_steps=2000, max_step=0.5, min_step=0.01, weights=None, fixed=None):
        """The atoms moved on their elastic network against the map given to upload_density (mad_flex_fit) -> (coords (n, 3),
        converged, last_step, step, g0).  network: (first, nbr, rest)."""
        x = _c(coords, np.float64).reshape(-1, 3)
        n = len(x)
        first, nbr, rest = (_c(network[0], np.int32).reshape(-1), _c(network[1], np.int32).reshape(-1), _c(network[2], np.float64).reshape(-1))
        if len(first) != n + 1:
            raise ValueError("flex_fit: network: first has %d entries for %d atoms" % (len(first), n))
        if len(nbr) != len(rest) or (len(first) and int(first[-1]) != len(nbr)):
            raise ValueError("flex_fit: network: first ends at %d, nbr has %d and rest %d entries" % (int(first[-1]), len(nbr), len(rest)))
        w = fx = None
        if weights is not None:
            w = _c(weights, np.float64).reshape(-1)
            if len(w) != n:
                raise ValueError("flex_fit: weights has %d entries for %d atoms" % (len(w), n))
        if fixed is not None:
            fx = _c(np.asarray(fixed, bool), np.uint8).reshape(-1)
            if len(fx) != n:
                raise ValueError("flex_fit: fixed has %d entries for %d atoms" % (len(fx), n))
        n_steps = _whole("flex_fit", "n_steps", n_steps)
        out = np.empty_like(x)
        conv, last = C.c_int32(0), C.c_int32(-1)
        step, g0 = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.dll.mad_flex_fit(self.ctx, n, _p(x), _p(w), _p(fx), _p(first), _p(nbr) if len(nbr) else None, _p(rest) if len(rest) else None,
                                        float(stiffness), n_steps, float(max_step), float(min_step), _p(out), C.byref(conv), C.byref(last),
                                        C.byref(step), C.byref(g0)))
        return out, bool(conv.value), int(last.value), step.value, g0.value

    def last_flex_plan(self):
        """(workgroups, threads, atoms per thread, springs) of the most recent flex_fit (mad_last_flex_plan); -1 before the first."""
        g, t, a, s = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
        self._chk(self.dll.mad_last_flex_plan(self.ctx, C.byref(g), C.byref(t), C.byref(a), C.byref(s)))
        return g.value, t.value, a.value, s.value

    def model_density_b(self, dims, origin, voxsp, coords, masses, b_atom, resolution, b_max=None):
        """The density of a model whose atom a has the variance (resolution / (pi sqrt 2))^2 + b_atom[a] / (8 pi^2), on the lattice
        (dims, origin, voxsp) (mad_model_density_b) -> (rho float64 [x][y][z], zero outside the box; box = (lo[3], dim[3])).
        b_max (default: the largest of b_atom) sets the box and the cell grid."""
        x = _c(coords, np.float64).reshape(-1, 3)
        n = len(x)
        m, b = _c(masses, np.float64).reshape(-1), _c(b_atom, np.float64).reshape(-1)
        if len(m) != n or len(b) != n:
            raise ValueError("model_density_b: %d masses and %d B-factors for %d atoms" % (len(m), len(b), n))
        d = np.array([_whole("model_density_b", "dims", v) for v in dims], np.int32)
        if d.shape != (3,) or np.any(d < 1):
            raise ValueError("model_density_b: dims %r" % (dims,))
        b_max = float(b.max()) if b_max is None and n else float(b_max if b_max is not None else 0.0)
        rho = np.empty(tuple(int(v) for v in d), np.float64)
        box = np.zeros(6, np.int32)
        self._chk(self.dll.mad_model_density_b(self.ctx, _p(d), _p(_vec(origin, 3)), float(voxsp), n, _p(x), _p(m), _p(b), float(resolution), b_max,
                                               _p(rho), _p(box)))
        return rho, (tuple(int(v) for v in box[:3]), tuple(int(v) for v in box[3:]))

    def bfactor_refine(self, grid, origin, voxsp, coords, masses, first_atom, b0, resolution, b_min=0.0, b_max=400.0, n_cycles=400, max_step=32.0,
                       min_step=0.25, fixed=None, want_density=False):
        """One B-factor per group of atoms refined against the map `grid` (mad_bfactor_refine) -> dict(b, scale, scale0, loss0, loss,
        cc0, cc, step, converged, last_cycle, rho).  The atoms come sorted by group, group g = first_atom[g] .. first_atom[g + 1] - 1;
        b0 one value per group; fixed one flag per group; rho (want_density) the unscaled float64 density at the final B."""
        g = _c(grid, np.float32)
        if g.ndim != 3:
            raise ValueError("bfactor_refine: the grid has shape %r" % (g.shape,))
        x = _c(coords, np.float64).reshape(-1, 3)
        n = len(x)
        m = _c(masses, np.float64).reshape(-1)
        if len(m) != n:
            raise ValueError("bfactor_refine: masses has %d entries for %d atoms" % (len(m), n))
        first = _c(first_atom, np.int64).reshape(-1)
        ng = len(first) - 1
        if ng < 1:
            raise ValueError("bfactor_refine: first_atom has %d entries" % len(first))
        b = _c(b0, np.float64).reshape(-1)
        if len(b) != ng:
            raise ValueError("bfactor_refine: b0 has %d entries for %d groups" % (len(b), ng))
        fx = None
        if fixed is not None:
            fx = _c(np.asarray(fixed, bool), np.uint8).reshape(-1)
            if len(fx) != ng:
                raise ValueError("bfactor_refine: fixed has %d entries for %d groups" % (len(fx), ng))
        n_cycles = _whole("bfactor_refine", "n_cycles", n_cycles)
        out, stats = np.empty(ng, np.float64), np.zeros(7, np.float64)
        conv, last = C.c_int32(0), C.c_int32(-1)
        rho = np.empty(g.shape, np.float64) if want_density else None
        self._chk(self.dll.mad_bfactor_refine(self.ctx, _p(g), _p(_dims(g)), _p(_vec(origin, 3)), float(voxsp), n, _p(x), _p(m), ng, _p(first), _p(b),
                                              _p(fx), float(resolution), float(b_min), float(b_max), n_cycles, float(max_step), float(min_step),
                                              _p(out), _p(stats), C.byref(conv), C.byref(last), _p(rho)))
        return dict(b=out, scale=stats[0], loss0=stats[1], loss=stats[2], cc0=stats[3], cc=stats[4], step=stats[5], scale0=stats[6],
                    converged=bool(conv.value), last_cycle=int(last.value), rho=rho)

    def last_bfactor_plan(self):
        """dict(box_lo, box_dim, bricks, cells, chunk, threads, cycles, kept) of the most recent model_density_b / bfactor_refine
        (mad_last_bfactor_plan); -1 before the first."""
        box, bricks, cells = np.zeros(6, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        chunk, threads, cycles, kept = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
        self._chk(self.dll.mad_last_bfactor_plan(self.ctx, _p(box), _p(bricks), _p(cells), C.byref(chunk), C.byref(threads), C.byref(cycles), C.byref(kept)))
        return dict(box_lo=tuple(int(v) for v in box[:3]), box_dim=tuple(int(v) for v in box[3:]), bricks=tuple(int(v) for v in bricks),
                    cells=tuple(int(v) for v in cells), chunk=chunk.value, threads=threads.value, cycles=cycles.value, kept=kept.value)

    def last_density_chunks(self):
        """Chunks the most recent density simulation cut its batch into (mad_last_density_chunks); -1 before the first."""
        return int(self.dll.mad_last_density_chunks(self.ctx))

    def structure_to_density(self, atoms, mass, resolution, voxsp, isovalue=0.0, pad=0):
        atoms, mass = _c(atoms, np.float64), _c(mass, np.float64)
        dims = np.zeros(3, np.int32)
        org = np.zeros(3)
        args = (self.ctx, _p(atoms), _p(mass), len(atoms), resolution, voxsp, isovalue, pad, _p(dims), _p(org))
        self._chk(self.dll.mad_structure_to_density(*args, None))
        grid = np.zeros(tuple(int(d) for d in dims), np.float32)
        self._chk(self.dll.mad_structure_to_density(*args, _p(grid)))
        return grid, float(org[0]), float(org[1]), float(org[2])

    def density_ccc(self, coords, mass, resolution, density_isovalue=0.0, ccc_isovalue=0.0):
        """coords: (n_cand, n_atoms, 3) placed copies of one structure -> CCC of each copy's simulated density with the
        map given to upload_density (PDB.structure_to_density + Dmap.get_CCC_with_grid, on the device end to end)."""
        c = _c(coords, np.float64)
        if c.ndim == 2:
            c = c[None]
        n_cand, n_atoms, _ = c.shape
        mass = _c(mass, np.float64)
        out = np.zeros(n_cand, np.float64)
        self._chk(self.dll.mad_density_ccc(self.ctx, _p(c), _p(mass), n_cand, n_atoms, resolution, density_isovalue, ccc_isovalue, _p(out)))
        return out

    def dock_refine_score(self, base_atoms, mass, hi_p, lo_p, rot, resolution, n_steps=500, max_step=0.5, min_step=0.01,
                          density_isovalue=0.0, ccc_isovalue=0.0, want_coords=True, cand_struct=None):
        """Candidate poses -> (refined coords or None, converged, last_step, ccc), device-resident from the poses to the scores
        (mad_dock_refine_score): start_c = (atoms - hi_p[c]) @ rot[c] + lo_p[c], refined against the uploaded map, turned into a
        simulated density and scored by CCC.  One structure: base_atoms (n, 3), mass (n) -> coords (n_cand, n, 3).  Several: lists of
        them + cand_struct[c] = the structure candidate c is a pose of -> coords = list of (n_of_c, 3) arrays."""
        many = isinstance(base_atoms, (list, tuple))
        bases = [_c(a, np.float64).reshape(-1, 3) for a in (base_atoms if many else [base_atoms])]
        masses = [_c(m, np.float64).reshape(-1) for m in (mass if many else [mass])]
        assert len(bases) == len(masses) and all(len(a) == len(m) for a, m in zip(bases, masses))
        first = np.zeros(len(bases) + 1, np.int64)
        first[1:] = np.cumsum([len(a) for a in bases])
        base_all, mass_all = np.concatenate(bases), np.concatenate(masses)
        hi_p, lo_p = _c(hi_p, np.float64).reshape(-1, 3), _c(lo_p, np.float64).reshape(-1, 3)
        rot = _c(rot, np.float64).reshape(-1, 9)
        n_cand = len(hi_p)
        cs = np.zeros(n_cand, np.int32) if cand_struct is None else _c(cand_struct, np.int32).reshape(-1)
        assert len(lo_p) == n_cand and len(rot) == n_cand and len(cs) == n_cand
        sizes = (first[1:] - first[:-1])[cs] if n_cand else np.zeros(0, np.int64)
        flat = np.zeros((int(sizes.sum()), 3)) if want_coords else None
        conv, last = np.zeros(max(n_cand, 1), np.int32), np.zeros(max(n_cand, 1), np.int32)
        ccc = np.zeros(max(n_cand, 1))
        self._chk(self.dll.mad_dock_refine_score(self.ctx, len(bases), _p(base_all), _p(mass_all), _p(first), n_cand, _p(cs),
                                                 _p(hi_p), _p(lo_p), _p(rot), int(n_steps), max_step, min_step, resolution, density_isovalue,
                                                 ccc_isovalue, _p(flat), _p(conv), _p(last), _p(ccc)))
        coords = None
        if want_coords:
            if many:
                ends = np.cumsum(sizes)
                coords = [flat[e - n:e] for e, n in zip(ends, sizes)]
            else:
                coords = flat.reshape(n_cand, len(bases[0]), 3)
        return coords, conv[:n_cand].astype(bool), last[:n_cand], ccc[:n_cand]

    def grid_overlap(self, g1, o1, g2, o2, voxsp, isovalue=1e-8):
        """-> (common, positives of g1); both grids (writable C-contiguous float32) are clamped in place."""
        common, npos = C.c_int64(0), C.c_int64(0)
        self._chk(self.dll.mad_grid_overlap(self.ctx, *_placed("grid_overlap", g1, o1, True), *_placed("grid_overlap", g2, o2, True),
                                            voxsp, isovalue, C.byref(common), C.byref(npos)))
        return common.value, npos.value

    def overlap_matrix(self, coords_list, mass_list, resolution=5.0, voxsp=2.0, density_isovalue=0.2, overlap_isovalue=1e-8):
        """Upper-triangular table of get_overlap between the simulated densities of the given structures."""
        n = len(coords_list)
        out = np.zeros((n, n), np.float64)
        if n < 2:
            return out
        first = np.zeros(n + 1, np.int64)
        first[1:] = np.cumsum([len(c) for c in coords_list])
        atoms = _c(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in coords_list]), np.float64)
        mass = _c(np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in mass_list]), np.float64)
        if len(mass) != len(atoms):
            raise ValueError("overlap_matrix: %d masses for %d atoms" % (len(mass), len(atoms)))
        self._chk(self.dll.mad_overlap_matrix(self.ctx, _p(atoms), _p(mass), _p(first), n, resolution, voxsp, density_isovalue,
                                              overlap_isovalue, _p(out)))
        return out

    def ccc(self, g1, o1, g2, o2, voxsp, isovalue=0.0):
        """Both grids must be writable C-contiguous float32; they are clamped in place like the reference."""
        out = C.c_double(0)
        self._chk(self.dll.mad_ccc(self.ctx, *_placed("ccc", g1, o1, True), *_placed("ccc", g2, o2, True), voxsp, isovalue, C.byref(out)))
        return out.value

    def map_mask(self, g1, o1, mask, o2, voxsp):
        """Dmap.mask_with: g1 (writable C-contiguous float32) is zeroed in place outside `mask` and where `mask` is below 1e-8;
        the mask (C-contiguous float32) is only read."""
        self._chk(self.dll.mad_map_mask(self.ctx, *_placed("map_mask", g1, o1, True), *_placed("map_mask", mask, o2, what="mask"), voxsp))

    def map_multiply(self, g1, o1, mask, o2, voxsp):
        """g1 (writable C-contiguous float32) times the soft mask (C-contiguous float32, only read) in place: the mask sits at the
        whole-voxel offset round(o2 / voxsp - o1 / voxsp), a voxel under a mask value of 1 keeps its bits, one outside the mask's
        box becomes +0 (mad_map_multiply)."""
        self._chk(self.dll.mad_map_multiply(self.ctx, *_placed("map_multiply", g1, o1, True),
                                            *_placed("map_multiply", mask, o2, what="mask"), voxsp))

    def map_envelope(self, g, voxsp, threshold, extend, soft, want_d2=False, out=None):
        """A soft mask from the map `g` (C-contiguous float32 [x, y, z], not modified) itself: 1 within `extend` Angstrom of a voxel
        above `threshold`, a raised cosine over the next `soft` Angstrom, 0 beyond -> (mask float32, d2 int32 or None, (seeds,
        core, edge)); d2, with `want_d2`, is the squared distance in voxels to the nearest seed, 2^31 - 1 beyond the window
        (mad_map_envelope).  `out`: a float32 array to take the mask instead of a new one; it stays as it is
        when the call is refused."""
        _grid("map_envelope", g)
        out = _out("map_envelope", out, g.shape)
        d2 = np.empty(g.shape, np.int32) if want_d2 else None
        counts = np.zeros(3, np.int64)
        self._chk(self.dll.mad_map_envelope(self.ctx, _p(g), _p(_dims(g)), voxsp, threshold, extend, soft, _p(out), _p(d2), _p(counts)))
        return out, d2, (int(counts[0]), int(counts[1]), int(counts[2]))

    def map_ccc(self, g1, o1, seconds, voxsp, isovalue=0.0):
        """Dmap.get_CCC_with_dmap of g1 against every (grid, origin) of `seconds` in one call -> float64 array.
        All grids C-contiguous float32; none is modified."""
        seconds = list(seconds)
        for g in [g1] + [g for g, _ in seconds]:
            _grid("map_ccc", g)
        n = len(seconds)
        out = np.zeros(n, np.float64)
        if n == 0:
            return out
        d2 = np.array([g.shape for g, _ in seconds], np.int32).reshape(n, 3)
        o2 = _c(np.array([_vec(o, 3) for _, o in seconds]), np.float64)
        ptrs = (C.c_void_p * n)(*[g.ctypes.data for g, _ in seconds])
        self._chk(self.dll.mad_map_ccc(self.ctx, *_placed("map_ccc", g1, o1), n, ptrs, _p(d2), _p(o2), voxsp, isovalue, _p(out)))
        return out

    def map_resample(self, g, origin, voxsp, out_dims, out_origin, out_voxsp, R=None, T=None, order=3):
        """`g` (C-contiguous float32 [x, y, z] with `origin` and `voxsp`) sampled on the lattice (`out_dims`, `out_origin`,
        `out_voxsp`) -> a new float32 array.  `R`, `T` (both or neither) move the source first: a point x goes to x @ R + T.
        order 1 is trilinear, order 3 cubic B-spline interpolation; outside the source the result is 0 (mad_map_resample)."""
        source = _placed("map_resample", g, origin)
        md =np.array([int(v) for v in out_dims], np.int64).reshape(3)
        if np.any(md < -2 ** 31) or np.any(md >= 2 ** 31):
            raise ValueError("map_resample: out_dims %s" % (tuple(md),))
        md = md.astype(np.int32)
        Rp = None if R is None else _vec(R, 9)
        Tp = None if T is None else _vec(T, 3)
        n_out = int(np.prod(np.maximum(md.astype(np.int64), 0)))
        out = np.empty(tuple(int(v) for v in md) if 0 < n_out < 2 ** 32 else (0,), np.float32)      # (a refused call writes nothing)
        self._chk(self.dll.mad_map_resample(self.ctx, *source, voxsp, _p(Rp), _p(Tp), order, _p(md),
                                            _p(_vec(out_origin, 3)), out_voxsp, _p(out)))
        return out

    @staticmethod
    def _operators(who, R, T):
        """The operator table of a call: R (n, 3, 3) and T (n, 3), or anything with fields `R` and `T` in the first place."""
        if T is None and hasattr(R, "R") and hasattr(R, "T") and not isinstance(R, np.ndarray):
            R, T = R.R, R.T
        R, T = _c(np.asarray(R, np.float64), np.float64), _c(np.asarray(T, np.float64), np.float64)
        if R.ndim != 3 or R.shape[1:] != (3, 3) or T.shape != (len(R), 3):
            raise ValueError("%s: operators of shapes %r and %r, not (n, 3, 3) and (n, 3)" % (who, R.shape, T.shape))
        if not 0 <= len(R) < 2 ** 31:
            raise ValueError("%s: %d operators" % (who, len(R)))
        return R, T

    def map_symmetry_score(self, g, origin, voxsp, centre, radius, R, T=None, stride=1, out=None):
        """The sums of `g` against itself moved by every operator (R[i], T[i]) over the lattice points of the ball (`centre`,
        `radius`, Angstrom) at every `stride`-th index -> float64 [n, 6] = n, sum a, sum b, sum a^2, sum b^2, sum a b
        (mad_map_symmetry_score; `symmetry.score_numpy` restates it bit for bit).  Nothing is modified."""
        who = "map_symmetry_score"
        placed = _placed(who, g, origin)
        R, T = self._operators(who, R, T)
        out = _out(who, out, (len(R), 6), np.float64, of="shape (n, 6)")
        self._chk(self.dll.mad_map_symmetry_score(self.ctx, *placed, float(voxsp), _p(_vec(centre, 3)), float(radius), _whole(who, "stride", stride),
                                                  len(R), _p(R), _p(T), _p(out)))
        return out

    def map_symmetrize(self, g, origin, voxsp, R, T=None, order=3, out=None):
        """`g` averaged over the operators (R[i], T[i]) on its own lattice -> a new float32 array (mad_map_symmetrize; DESIGN.md
        section 4y; `symmetry.symmetrize_numpy` restates it).  1 .. 64 operators; order 1 or 3 as `map_resample`."""
        who = "map_symmetrize"
        placed = _placed(who, g, origin)
        R, T = self._operators(who, R, T)
        out = _out(who, out, g.shape)
        self._chk(self.dll.mad_map_symmetrize(self.ctx, *placed, float(voxsp), len(R), _p(R), _p(T), _whole(who, "order", order), _p(out)))
        return out

    def last_symmetry_plan(self):
        """-> (operators per workgroup of the score kernel, chunks of operators, bytes of partial records) of the most recent
        `map_symmetry_score` (mad_last_symmetry_plan; the last two -1 before the first call)."""
        w, c, b = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._chk(self.dll.mad_last_symmetry_plan(self.ctx, C.byref(w), C.byref(c), C.byref(b)))
        return int(w.value), int(c.value), int(b.value)

    def map_fsc(self, g1, o1, g2, o2, voxsp):
        """Fourier shell correlation sums of two maps of one spacing -> (N, sums float64 [N / 2 + 1, 3] = P1, P2, C per shell,
        count int64 [N / 2 + 1]) (mad_map_fsc; `fourier.FSC(N, voxsp, sums, count)` makes the curve).
        Both grids C-contiguous float32 [x, y, z]; neither is modified."""
        cap = 1024 // 2 + 1
        n, sums, count = C.c_int32(0), np.zeros((cap, 3), np.float64), np.zeros(cap, np.int64)
        self._chk(self.dll.mad_map_fsc(self.ctx, *_placed("map_fsc", g1, o1), *_placed("map_fsc", g2, o2), voxsp, C.byref(n),
                                       _p(sums), _p(count), cap))
        sh = n.value // 2 + 1
        return int(n.value), sums[:sh].copy(), count[:sh].copy()

    def map_fsc_masked(self, g1, o1, g2, o2, voxsp, mask, om, shell_r=None, t_r=0.8, seed=0):
        """The Fourier shell correlation of two maps under a soft mask and what corrects it for the mask -> (N, sums_unmasked,
        sums_masked, sums_random -- each float64 [N / 2 + 1, 3] = P1, P2, C --, count int64 [N / 2 + 1], shell_r): the phases are
        randomised from shell `shell_r` on, or with None from the lowest shell whose unmasked curve is below `t_r`
        (mad_map_fsc_masked; `fourier.fsc_masked_numpy` restates it, `fourier.MaskedFSC` makes the curves).
        All three grids C-contiguous float32 [x, y, z]; none is modified."""
        who = "map_fsc_masked"
        maps = _placed(who, g1, o1) + _placed(who, g2, o2) + (voxsp,)
        masked = _placed(who, mask, om)
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("map_fsc_masked: seed %r (0 .. 2^64 - 1)" % (seed,))
        sr = -1 if shell_r is None else int(shell_r)
        if shell_r is not None and not 0 <= sr < 2 ** 31:
            raise ValueError("map_fsc_masked: shell_r %r (0 or more, or None)" % (shell_r,))
        n = C.c_int32(0)
        self._chk(self.dll.mad_map_fft(self.ctx, *maps, C.byref(n), None))
        sh = n.value // 2 + 1
        su, sm, sr_sums, count = np.zeros((sh, 3)), np.zeros((sh, 3)), np.zeros((sh, 3)), np.zeros(sh, np.int64)
        got = C.c_int32(0)
        self._chk(self.dll.mad_map_fsc_masked(self.ctx, *maps, *masked, sr, float(t_r), seed, _p(su), _p(sm), _p(sr_sums), _p(count),
                                              C.byref(n), C.byref(got)))
        return int(n.value), su, sm, sr_sums, count, int(got.value)

    def map_phase_randomize(self, spectrum, shell_r, seed=0):
        """A copy of `spectrum` (complex128 [N, N, N], N a power of two from 8 to 1024) with new phases from shell `shell_r` on and
        F(-k) = conj F(k) there (mad_map_phase_randomize; `fourier.randomize_numpy` restates it)."""
        s = np.array(spectrum, np.complex128, order="C")
        if s.ndim != 3 or s.shape[0] != s.shape[1] or s.shape[0] != s.shape[2]:
            raise ValueError("map_phase_randomize needs a cubic 3-D spectrum, got %r" % (s.shape,))
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("map_phase_randomize: seed %r (0 .. 2^64 - 1)" % (seed,))
        self._chk(self.dll.mad_map_phase_randomize(self.ctx, _p(s), s.shape[0], int(shell_r), seed))
        return s

    @staticmethod
    def _selection(who, select, shape):
        """`select` over the sample lattice of `shape` as the uint8 flags the library reads, or None."""
        if select is None:
            return None
        sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
        if sel.shape != shape:
            raise ValueError("%s: select of shape %r, the sample lattice is %r" % (who, sel.shape, shape))
        return sel

    def map_local_fsc(self, g1, o1, g2, o2, voxsp, box=16, step=2, threshold=0.143, select=None, sums=False):
        """Local resolution by windowed Fourier shell correlation -> (resolution float64 [nx, ny, nz], shell int32 [nx, ny, nz],
        sums float64 [nx, ny, nz, box / 2 + 1, 3] or None) over the samples at every `step`-th voxel of `g1` (mad_map_local_fsc;
        DESIGN.md section 4p; `fourier.local_fsc_numpy` restates it).  `select`: an array over the sample lattice, a sample where it
        is 0 gets 0.0 / -1 and is not computed.  Both grids C-contiguous float32 [x, y, z]; neither is modified."""
        n = np.zeros(3, np.int32)
        args = (self.ctx,) + _placed("map_local_fsc", g1, o1) + _placed("map_local_fsc", g2, o2) + (voxsp, int(box), int(step), float(threshold))
        self._chk(self.dll.mad_map_local_fsc(*args, None, None, None, None, _p(n)))      # the size query
        shape = tuple(int(v) for v in n)
        sel = self._selection("map_local_fsc", select, shape)
        res, shell = np.empty(shape, np.float64), np.empty(shape, np.int32)
        sm = np.empty(shape + (int(box) // 2 + 1, 3), np.float64) if sums else None
        self._chk(self.dll.mad_map_local_fsc(*args, _p(sel), _p(res), _p(shell), _p(sm), _p(n)))
        return res, shell, sm

    def map_local_scale(self, g1, o1, g2, o2, voxsp, box=16, step=1, select=None, gains=False):
        """The amplitudes of `g1` scaled to those of `g2` box by box -> (value float64 [nx, ny, nz], computed bool [nx, ny, nz],
        gains float64 [nx, ny, nz, box / 2 + 1] or None) over the samples at every `step`-th voxel of `g1` (mad_map_local_scale;
        DESIGN.md section 4v; `fourier.local_scale_numpy` restates it).  `select`: an array over the sample lattice, a sample where
        it is 0 gets 0.0 and is not computed.  Both grids C-contiguous float32 [x, y, z]; neither is modified."""
        n = np.zeros(3, np.int32)
        args = (self.ctx,) + _placed("map_local_scale", g1, o1) + _placed("map_local_scale", g2, o2) + (voxsp, int(box), int(step))
        self._chk(self.dll.mad_map_local_scale(*args, None, None, None, _p(n)))      # the size query
        shape = tuple(int(v) for v in n)
        sel = self._selection("map_local_scale", select, shape)
        value = np.empty(shape, np.float64)
        gn = np.empty(shape + (int(box) // 2 + 1,), np.float64) if gains else None
        self._chk(self.dll.mad_map_local_scale(*args, _p(sel), _p(value), _p(gn), _p(n)))
        return value, (np.ones(shape, bool) if sel is None else sel.astype(bool)), gn

    def map_local_filter(self, grid, res, step, voxsp, out=None, out64=False, sigma=False):
        """`grid` (C-contiguous float32 [x, y, z]) low-passed voxel by voxel: every output voxel is the map under the Gaussian of its
        own resolution, sigma = d / (voxsp pi sqrt(2)) voxels, d interpolated trilinearly from `res` (float64, Angstrom) on the
        lattice of every `step`-th voxel, shape ((n - 1) // step + 1 per axis) (mad_map_local_filter; DESIGN.md section 4q;
        `fourier.local_filter_numpy` restates it).  -> the float32 result (a new array, or `out`, which may be `grid` itself); with
        `out64` and / or `sigma` a tuple (out, out64 or None, sigma or None): the float64 result before rounding and the per-voxel
        sigma in voxels.  The results do not depend on which of the two were asked for."""
        _grid("map_local_filter", grid)
        r = _c(np.asarray(res), np.float64)
        if r.ndim != 3:
            raise ValueError("map_local_filter needs a 3-D field of resolutions")
        step = _whole("map_local_filter", "step", step)
        out = _out("map_local_filter", out, grid.shape)
        o64 = np.empty(grid.shape, np.float64) if out64 else None
        sg = np.empty(grid.shape, np.float64) if sigma else None
        self._chk(self.dll.mad_map_local_filter(self.ctx, _p(grid), _p(_dims(grid)), float(voxsp), _p(r), _p(_dims(r)), step, _p(out),
                                                _p(o64), _p(sg)))
        return (out, o64, sg) if (out64 or sigma) else out

    def map_fft(self, g1, o1, g2=None, o2=None, voxsp=1.0):
        """The transform `map_fsc` works on, for testing it alone -> complex128 [N, N, N]: the FFT of the lattice that holds `g1`
        in the real and `g2` (may be None) in the imaginary part (mad_map_fft)."""
        args = (self.ctx,) + _placed("map_fft", g1, o1) + _placed("map_fft", g2, o2) + (voxsp,)
        n = C.c_int32(0)
        self._chk(self.dll.mad_map_fft(*args, C.byref(n), None))
        out = np.empty((n.value,) * 3, np.complex128)
        self._chk(self.dll.mad_map_fft(*args, C.byref(n), _p(out)))
        return out

    def map_filter(self, g1, gain, pad=0, g2=None):
        """A radial filter in Fourier space -> out1, or (out1, out2) with `g2`: new float32 arrays of the grids' shapes
        (mad_map_filter; `fourier.filter_numpy` restates it).  `gain`: float64 [3 (N / 2)^2 + 1] by
        r2 = i^2 + j^2 + k^2 (`fourier.radial_gain`), N = `fourier.filter_lattice(g1.shape, pad, g2.shape)`.  The grids
        (C-contiguous float32 [x, y, z]) need no common frame; neither is modified."""
        _grid("map_filter", g1)
        d2 = None if g2 is None else _dims(_grid("map_filter", g2))
        gain = _vec(gain, -1)
        out1 = np.empty(g1.shape, np.float32)
        out2 = None if g2 is None else np.empty(g2.shape, np.float32)
        n = C.c_int32(0)
        self._chk(self.dll.mad_map_filter(self.ctx, _p(g1), _p(_dims(g1)), _p(g2), _p(d2), int(pad), _p(gain), len(gain), C.byref(n),
                                          _p(out1), _p(out2)))
        return out1 if g2 is None else (out1, out2)

    def map_ifft(self, spectrum):
        """The inverse transform `map_filter` works with, for testing it alone -> complex128 [N, N, N] = ifft(spectrum), normalised by
        1 / N^3 (mad_map_ifft).  `spectrum`: complex128 [N, N, N], N a power of two from 8 to 1024."""
        s = _c(np.asarray(spectrum), np.complex128)
        if s.ndim != 3 or s.shape[0] != s.shape[1] or s.shape[0] != s.shape[2]:
            raise ValueError("map_ifft needs a cubic 3-D spectrum, got %r" % (s.shape,))
        out = np.empty(s.shape, np.complex128)
        self._chk(self.dll.mad_map_ifft(self.ctx, _p(s), s.shape[0], _p(out)))
        return out

    def map_scan_lattice(self, d1, d2):
        """N of `map_scan` for a map of dims `d1` and templates of dims `d2`: the size query of mad_map_scan (nothing is allocated
        or launched; it refuses what `fourier.scan_lattice` refuses)."""
        d1, d2 = np.array(d1, np.int32).reshape(3), np.array(d2, np.int32).reshape(3)
        n = C.c_int32(0)
        self._chk(self.dll.mad_map_scan(self.ctx, None, _p(d1), 1, None, _p(d2), 0.0, 0.0, 0, 0.0, 0, None, None, None, None, None, C.byref(n)))
        return int(n.value)

    def _corr_outputs(self, who, k, shape, ext):
        """What `map_scan` / `map_search` fill, over the offsets D = shape - ext + 1 -> (k, best, best_i, peaks, n_peaks, n_found, n_skipped, n)."""
        k = int(k)
        if k < 0:
            raise ValueError("%s: k = %d (0 or more)" % (who, k))
        D = tuple(max(int(a) - int(b) + 1, 1) for a, b in zip(shape, ext))
        return k, np.zeros(D, np.float32), np.full(D, -1, np.int32), np.zeros((max(k, 1), 5), np.float64), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)

    def map_scan(self, m, templates, iso=0.0, e_min=0.0, mode=0, min_score=0.0, k=20):
        """Every whole-voxel translation of the templates inside the map `m`, scored by fast local correlation -> (best float32 [D],
        best_t int32 [D], peaks float64 [min(k, n_found), 5] = ux, uy, uz, score, template; n_found, N) (mad_map_scan; DESIGN.md
        section 4n; `fourier.scan_numpy` and `fourier.peaks_numpy` restate it).  `m` and the `templates` (a list of grids of one
        shape, no longer than the map on any axis): C-contiguous float32 [x, y, z]; D = m.shape - template shape + 1.  mode 0: the
        un-centred score C / sqrt(E G); 1: the centred one.  An offset is scored where E (E') > `e_min`.  Nothing is modified."""
        templates = list(templates)
        if len(templates) < 1:
            raise ValueError("map_scan needs one template or more")
        _grid("map_scan", m)
        for g in templates:
            if _grid("map_scan", g).shape != templates[0].shape:
                raise ValueError("map_scan needs templates of one shape, got %r and %r" % (templates[0].shape, g.shape))
        k, best, best_t, peaks, n_peaks, n_found, _, n = self._corr_outputs("map_scan", k, m.shape, templates[0].shape)
        ptrs = (C.c_void_p * len(templates))(*[g.ctypes.data for g in templates])
        self._chk(self.dll.mad_map_scan(self.ctx, _p(m), _p(_dims(m)), len(templates), ptrs, _p(_dims(templates[0])), float(iso), float(e_min),
                                        int(mode), float(min_score), k, _p(best), _p(best_t), _p(peaks), C.byref(n_peaks), C.byref(n_found),
                                        C.byref(n)))
        return best, best_t, peaks[:n_peaks.value].copy(), int(n_found.value), int(n.value)

    def map_rotate(self, base, c0, edge, R, iso=0.0):
        """One rotated template of `map_search` and its sums -> (g float32 [e, e, e], n_w, G, S) (mad_map_rotate; DESIGN.md section
        4o; `fourier.rotate_numpy` and `fourier.tree_sum` restate it bit for bit).  `base`: C-contiguous float32 [x, y, z]; `c0`: the
        centre of rotation in its voxel coordinates; `R`: 3 x 3."""
        e = int(edge)
        out, stats = np.zeros((max(e, 0),) * 3 if e <= 1024 else (0,), np.float32), np.zeros(3, np.float64)
        self._chk(self.dll.mad_map_rotate(self.ctx, *_placed("map_rotate", base, c0), e, _p(_vec(R, 9)), float(iso), _p(out), _p(stats)))
        return out, int(stats[0]), float(stats[1]), float(stats[2])

    def map_search(self, m, base, c0, edge, rotations, iso=0.0, e_fill=0.0, mode=0, min_score=0.0, k=20):
        """Every rotation in `rotations` and every whole-voxel translation of the template `base` inside the map `m`, scored by fast
        local correlation -> (best float32 [D], best_r int32 [D], peaks float64 [min(k, n_found), 5] = ux, uy, uz, score, rotation;
        n_found, n_skipped, N) (mad_map_search; `fourier.search_numpy` restates it).  `m`, `base`: C-contiguous
        float32 [x, y, z]; `c0`: the centre of rotation in `base`'s voxel coordinates; the rotated templates are cubes of `edge`
        voxels, D = m.shape - edge + 1; `rotations`: (n, 3, 3).  An offset is scored by a rotation where E (E') > e_fill n_w.  A
        rotation whose mask is empty (or, centred, flat) is skipped and counted in n_skipped.  Nothing is modified."""
        _grid("map_search", m)
        template = _placed("map_search", base, c0)
        rot =_c(np.asarray(rotations, np.float64), np.float64)
        if rot.ndim != 3 or rot.shape[1:] != (3, 3) or len(rot) < 1:
            raise ValueError("map_search: rotations of shape %r, not (n, 3, 3) with n >= 1" % (rot.shape,))
        e = int(edge)
        k, best, best_r, peaks, n_peaks, n_found, n_skipped, n = self._corr_outputs("map_search", k, m.shape, (e, e, e))
        self._chk(self.dll.mad_map_search(self.ctx, _p(m), _p(_dims(m)), *template, e, _p(rot), len(rot), float(iso),
                                          float(e_fill), int(mode), float(min_score), k, _p(best), _p(best_r), _p(peaks), C.byref(n_peaks),
                                          C.byref(n_found), C.byref(n_skipped), C.byref(n)))
        return best, best_r, peaks[:n_peaks.value].copy(), int(n_found.value), int(n_skipped.value), int(n.value)

    def map_zone(self, g, origin, voxsp, atoms, radius, soft=0.0, erase=False):
        """`g` (writable C-contiguous float32 [x, y, z] with `origin` and `voxsp`) cut around `atoms` in place: a voxel within
        `radius` of an atom keeps its bits, one `radius + soft` away or farther becomes 0, a raised cosine in between;
        `erase=True` takes one minus that weight.  `atoms`: anything np.asarray(..., float64).reshape(-1, 3) accepts.
        -> (voxels within radius, voxels in the soft edge) (mad_map_zone)."""
        placed = _placed("map_zone", g, origin, True)
        a = _vec(atoms, (-1, 3))
        counts = np.zeros(2, np.int64)
        self._chk(self.dll.mad_map_zone(self.ctx, *placed, voxsp, _p(a) if len(a) else None, len(a), radius, soft, 1 if erase else 0,
                                        _p(counts)))
        return int(counts[0]), int(counts[1])

    def map_group_fit(self, g1, o1, g2, o2, voxsp, atoms, first_atom, radius, isovalue=0.0, out=None):
        """A placed model scored per group of atoms: `g1` (the map) and `g2` (the model's density), C-contiguous float32
        [x, y, z] with origins `o1`, `o2` and the common spacing `voxsp`; group g owns atoms first_atom[g] .. first_atom[g + 1] - 1.
        -> (n_vox int64 [G], sums float64 [G, 5]): per group the voxels of g1 within `radius` of one of its atoms, and over them
        sum a*a, sum b*b, sum a*b, sum a, sum b with a, b the two densities clamped at `isovalue`, b = 0 beyond g2
        (mad_map_group_fit).  Nothing is modified.  `out`: a pair of arrays to fill instead of new ones."""
        who = "map_group_fit"
        maps = _placed(who, g1, o1) + _placed(who, g2, o2)
        a = _vec(atoms, (-1, 3))
        first = _c(np.asarray(first_atom, np.int64).reshape(-1), np.int64)
        if len(first) < 1:
            raise ValueError("map_group_fit: first_atom needs n_groups + 1 entries")
        n_groups = len(first) - 1
        if n_groups >= 2 ** 31:
            raise ValueError("map_group_fit: %d groups" % n_groups)
        if int(first[-1]) > len(a):
            raise ValueError("map_group_fit: first_atom ends at %d, there are %d atoms" % (int(first[-1]), len(a)))
        n_vox, sums = (None, None) if out is None else out
        n_vox = _out(who, n_vox, (n_groups,), np.int64, "[G] entries", np.zeros, "out[0]")
        sums = _out(who, sums, (n_groups, 5), np.float64, "shape [G, 5]", np.zeros, "out[1]")
        self._chk(self.dll.mad_map_group_fit(self.ctx, *maps, voxsp, _p(a) if len(a) else None, _p(first), n_groups, radius, isovalue,
                                             _p(n_vox), _p(sums)))
        return n_vox, sums

    def map_qscore(self, g, origin, voxsp, atoms, radii, ref, dirs, tries, index=None, details=False):
        """The Q-score per atom: `g` (C-contiguous float32 [x, y, z] with `origin` and `voxsp`) sampled around `atoms` (n x 3, the
        environment) on the shells `radii` and correlated with `ref`; `dirs`: the point sets 1 .. `tries`, set t with 8 t unit
        vectors (`localfit.qscore_tables` makes the three).  `index`: the atoms to score (int64; None: all).
        -> (q float64 [m], n_samples int32 [m]), with `details` also (tries_used int32 [m, n_r], picked int32 [m, n_r, 8], values
        float64 [m, n_r, 8]) (mad_map_qscore).  Nothing is modified."""
        placed = _placed("map_qscore", g, origin)
        a, radii, ref, dirs = _vec(atoms, (-1, 3)), _vec(radii, -1), _vec(ref, -1), _vec(dirs, (-1, 3))
        tries, n_r = int(tries), len(radii)
        if len(ref) != n_r:
            raise ValueError("map_qscore: %d ref values for %d radii" % (len(ref), n_r))
        if not 1 <= n_r <= QSCORE_MAX_SHELLS or not 1 <= tries <= QSCORE_MAX_TRIES:
            raise ValueError("map_qscore: %d shells, %d point sets (1 .. %d, 1 .. %d)" % (n_r, tries, QSCORE_MAX_SHELLS, QSCORE_MAX_TRIES))
        if len(dirs) != 4 * tries * (tries + 1):
            raise ValueError("map_qscore: %d directions, %d point sets need %d" % (len(dirs), tries, 4 * tries * (tries + 1)))
        if index is not None:
            index = _c(np.asarray(index).reshape(-1), np.int64)
            if len(index) and (index.min() < 0 or index.max() >= len(a)):
                raise ValueError("map_qscore: index holds an atom outside 0 .. %d" % (len(a) - 1))
        m = len(a) if index is None else len(index)
        q, n_samples = np.full(m, np.nan), np.zeros(m, np.int32)
        det = (np.zeros((m, n_r), np.int32), np.full((m, n_r, 8), -1, np.int32), np.zeros((m, n_r, 8), np.float64)) if details else (None, None, None)
        self._chk(self.dll.mad_map_qscore(self.ctx, *placed, voxsp, _p(a) if len(a) else None, len(a), _p(index), m if index is not None else 0,
                                          _p(radii), _p(ref), n_r, _p(dirs), tries, _p(q), _p(n_samples), _p(det[0]), _p(det[1]), _p(det[2])))
        return (q, n_samples) + (det if details else ())

    def map_smooth(self, g, sigma_vox, out=None):
        """`g` (C-contiguous float32 [x, y, z]) smoothed with a Gaussian of `sigma_vox` voxels, zero beyond the grid, float64 inside
        -> a new float32 array, or `out` (which may be `g` itself) (mad_map_smooth)."""
        _grid("map_smooth", g)
        out = _out("map_smooth", out, g.shape)
        self._chk(self.dll.mad_map_smooth(self.ctx, _p(g), _p(_dims(g)), sigma_vox, _p(out)))
        return out

    SEGMENT_CAP0 = 1 << 16      # regions the tables of map_segment hold at first (they grow on MAD_ENOSPC, at the price of a second call)

    def _tables(self, g, cap, dtypes, call):
        """The per-region tables of map_segment / map_components: `call(tabs, cap, n)` makes the C call that fills arrays of `dtypes`
        and the count n.  By default they grow until they fit; a given `cap` that is too small -> (None, n needed)."""
        tabs, n = None, C.c_int64(0)

        def attempt(try_cap):
            nonlocal tabs
            tabs = tuple(np.zeros(max(try_cap, 0), dt) for dt in dtypes)
            return call(tabs, try_cap, n), n.value

        fits = _retry_enospc(self, attempt, int(cap) if cap is not None else max(1, min(g.size, self.SEGMENT_CAP0)), grow=cap is None)
        n = int(n.value)
        return (tuple(t[:n].copy() for t in tabs) if fits else None), n

    def map_segment(self, g, threshold=0.0, steps=4, step=1.0, stop_at=0, cap=None):
        """Watershed regions of `g` (C-contiguous float32 [x, y, z]; foreground: value > threshold), grouped by following their maxima
        through `steps` copies of the map smoothed with sigma = step, 2 step, ... voxels, stopping early once no more than `stop_at`
        groups are left (0: never) (mad_map_segment).  -> dict: `labels` int32 (the group of every voxel, 0 for
        background), per region `root` (int64 linear index), `peak` (float32), `size` (int64), `group` (int32), and `history` (groups
        after step 0 .. steps_done), `steps_done`, `n_regions`, `n_groups`.  `cap`: the capacity of the region tables; by default it
        grows until they fit, with a given one that is too small the four tables come back as None and `n_regions` says what is needed."""
        _grid("map_segment", g)
        steps = _whole("map_segment", "steps", steps)
        stop_at = _whole("map_segment", "stop_at", stop_at, -2 ** 63, 2 ** 63)
        d = _dims(g)
        labels = np.zeros(g.shape, np.int32)
        history = np.zeros(max(steps, 0) + 1, np.int64)
        done = C.c_int32(0)      # on MAD_ENOSPC labels and history are valid all the same
        tabs, n = self._tables(g, cap, (np.int64, np.float32, np.int64, np.int32), lambda t, try_cap, n: self.dll.mad_map_segment(
            self.ctx, _p(g), _p(d), threshold, steps, step, stop_at, _p(labels), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), try_cap,
            C.byref(n), _p(history), C.byref(done)))
        done = int(done.value)
        hist = history[:done + 1].copy()
        out = dict(labels=labels, history=hist, steps_done=done, n_regions=n, n_groups=int(hist[-1]))
        for k, name in enumerate(("root", "peak", "size", "group")):
            out[name] = None if tabs is None else tabs[k]
        return out

    def map_components(self, g, threshold, connectivity=26, cap=None):
        """The connected components of the voxels of `g` (C-contiguous float32 [x, y, z], not modified) above `threshold` (strict),
        neighbours by `connectivity` 6, 18 or 26, no wrap-around (mad_map_components).  -> dict: `labels` int32
        (the component of every voxel, 1 .. n by ascending smallest linear index, 0 for background), per component `root` (int64, that
        index) and `size` (int64, its voxels), and `n`.  `cap`: the capacity of the two tables; by default it grows until they fit,
        with a given one that is too small they come back as None and `n` says what is needed."""
        _grid("map_components", g)
        conn = _whole("map_components", "connectivity", connectivity)
        d = _dims(g)
        labels = np.zeros(g.shape, np.int32)      # on MAD_ENOSPC the labels are valid all the same
        tabs, n = self._tables(g, cap, (np.int64, np.int64), lambda t, try_cap, n: self.dll.mad_map_components(
            self.ctx, _p(g), _p(d), threshold, conn, _p(labels), _p(t[0]), _p(t[1]), try_cap, C.byref(n)))
        return dict(labels=labels, n=n, root=None if tabs is None else tabs[0], size=None if tabs is None else tabs[1])

    def map_dust(self, g, threshold, connectivity=26, min_size=1, keep=0, fill=None, out=None):
        """`g` (C-contiguous float32 [x, y, z]) without its dust: the components of `map_components` are ranked by size descending,
        root ascending, one is kept where its size is `min_size` or more and (`keep` == 0 or its rank < `keep`), and every foreground
        voxel of one that is not kept becomes `fill` (None: 0.0 for a threshold of 0 or more, else the largest float32 not above the
        threshold); every other voxel keeps its bits (mad_map_dust).  -> (out float32, (components, kept
        components, foreground voxels, kept voxels)).  `out`: a float32 array to take the result instead of a new one; it may be `g`,
        and stays as it is when the call is refused."""
        from .components import default_fill
        _grid("map_dust", g)
        conn = _whole("map_dust", "connectivity", connectivity)
        min_size = _whole("map_dust", "min_size", min_size, -2 ** 31, 2 ** 63)
        keep = _whole("map_dust", "keep", keep, -2 ** 31, 2 ** 63)
        out =_out("map_dust", out, g.shape)
        fill = default_fill(threshold) if fill is None else np.float32(fill)
        counts = np.zeros(4, np.int64)
        self._chk(self.dll.mad_map_dust(self.ctx, _p(g), _p(_dims(g)), threshold, conn, min_size, keep, fill, _p(out), _p(counts)))
        return out, tuple(int(v) for v in counts)

    def map_sort(self, g, out=None):
        """The values of `g` (C-contiguous float32 of any shape, not modified) in descending order, -0.0 as +0.0 -> float32 [g.size]
        (mad_map_sort; DESIGN.md section 4w: a radix sort of the keys on the device).  A voxel that is not finite is refused, and `out`
        (a float32 array to take the result) then stays as it is."""
        _countable("map_sort", _grid("map_sort", g, None, what="array"))
        out = _out("map_sort", out, (g.size,), of="g.size values")
        self._chk(self.dll.mad_map_sort(self.ctx, _p(g), g.size, _p(out)))
        return out

    def map_kth(self, g, k, out=None):
        """The `k`-th largest values of `g` (C-contiguous float32 of any shape), 1-based: k = 1 the maximum, k = g.size the minimum; `k`
        a whole number or several -> float32 [len(k)] (mad_map_kth)."""
        _countable("map_kth", _grid("map_kth", g, None, what="array"))
        ka = np.atleast_1d(np.asarray(k))
        if ka.ndim != 1 or len(ka) < 1 or not np.issubdtype(ka.dtype, np.integer):
            raise ValueError("map_kth: ranks must be whole numbers, got %s %s" % (ka.dtype, ka.shape))
        ka = _c(ka, np.int64)
        if ka.min() < 1 or ka.max() > g.size:
            raise ValueError("map_kth: ranks %d .. %d of %d voxels (1 is the largest)" % (ka.min(), ka.max(), g.size))
        out = _out("map_kth", out, (len(ka),), of="len(k) values")
        self._chk(self.dll.mad_map_kth(self.ctx, _p(g), g.size, len(ka), _p(ka), _p(out)))
        return out

    def map_confidence(self, g, boxes, c, levels=(0.01,), want_q=True, details=False, out=None):
        """The confidence map of `g` (C-contiguous float32 [x, y, z], not modified): noise from the cubes `boxes` (whole numbers (n, 4):
        x, y, z of the corner, edge; inside the grid), one-sided p-values under normal noise, q-values by the step-up rule with the
        constant `c` (1: Benjamini-Hochberg; `confidence.harmonic(g.size)`: Benjamini-Yekutieli), and per false discovery rate of
        `levels` the voxels whose q is at or below it and the least density among them (mad_map_confidence) ->
        dict: `confidence` float32 (1 - q), `q` float64 (None unless want_q), `mean`, `var`, `n` of the noise, `count` int64 and `value`
        float32 per level (NaN where count is 0), and with details=True `sorted` (float32, the densities descending) and `q_sorted`.
        `out`: a float32 array of the grid's shape to take the confidence; it stays as it is when the call is refused."""
        from .confidence import check_boxes
        _countable("map_confidence", _grid("map_confidence", g, what="array"))
        b = _c(check_boxes("map_confidence", g.shape, boxes), np.int32)
        c = float(c)
        if not (c >= 1.0) or not np.isfinite(c):
            raise ValueError("map_confidence: c = %r (1, or the harmonic number of the voxels)" % (c,))
        lv = _c(np.atleast_1d(np.asarray(levels, np.float64)), np.float64)
        if lv.ndim != 1 or len(lv) > 256 or not ((lv >= 0) & (lv <= 1)).all():
            raise ValueError("map_confidence: levels %r (at most 256 false discovery rates, 0 .. 1)" % (levels,))
        out = _out("map_confidence", out, g.shape)
        q = np.empty(g.shape, np.float64) if want_q else None
        srt = np.empty(g.size, np.float32) if details else None
        qs = np.empty(g.size, np.float64) if details else None
        count, value, stats = np.zeros(max(len(lv), 1), np.int64), np.zeros(max(len(lv), 1), np.float32), np.zeros(3, np.float64)
        self._chk(self.dll.mad_map_confidence(self.ctx, _p(g), _p(_dims(g)), len(b), _p(b), c, len(lv), _p(lv), _p(out), _p(q), _p(srt),
                                              _p(qs), _p(count), _p(value), _p(stats)))
        r = dict(confidence=out, q=q, mean=float(stats[0]), var=float(stats[1]), n=int(stats[2]), count=count[:len(lv)].copy(), value=value[:len(lv)].copy())
        if details:
            r.update(sorted=srt, q_sorted=qs)
        return r


_default = None


def get_lib(device=None):
    """Process-wide default context (device from MAD_DEVICE / LOCAL_RANK / 0)."""
    global _default
    if _default is None:
        if device is None:
            device = int(os.environ.get("MAD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default = Lib(device)
    return _default


def reset_lib():
    global _default
    if _default is not None:
        _default.close()
    _default = None
