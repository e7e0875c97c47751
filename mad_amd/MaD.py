"""Orchestrator with the reference's entry points (mad/MaD.py:25-99):

    mad = MaD.MaD(); mad.add_map(path, resolution); mad.add_subunit(path, n_copies=k); mad.run()

On the hot path: `_describe_struct` (orientation + description on
the GPU), `_match_dsc` (int8-MFMA correlation, pose scoring, top-k on the GPU) and
`_refine_filtered_solutions` (batched persistent refinement, density simulation and CCC
on the GPU).  The greedy cloud clustering that picks which poses get refined
(`_filter_dsc_pairs`, MaD.py:456-553) is decided on the device (`Lib.pose_cluster_many`: one call
per bracket chunk, float64 with a guard band) and turned into the candidate list by
`_filter_from_owner`; a match with a decision inside the band, or with more than 4 096 rows
(n_samples * n_copies beyond what the entry takes), goes through the host loop of
`_filter_dsc_pairs`, and MAD_FILTER_HOST=1 sends every match there.  Both give the same list.

Several GPUs (round 3): started under a launcher (`torchrun --nproc-per-node N run_MaD.py ...`: WORLD_SIZE / RANK / LOCAL_RANK in
the environment), `run()` deals the structures to describe and then the subunits / ensemble frames to dock round-robin over the
ranks -- the reference's loops over them are independent iterations (MaD.py:116-190) -- every rank works on its GPU, the
solution files land in the one results folder rank 0 created, and the lists of solutions are all-gathered so that every rank
ends with the reference's `buildable_subunits`; `build_assembly` runs on rank 0.  The exchanges are a few python objects over a
gloo group (names, file lists): control plane, nothing of the data path crosses ranks.

Resident path (the default): `_describe_struct` runs MapSpace and Detector as above and then builds the structure's rows straight
into a device set (`Lib.set_build`: orientation + description, one call); the rows stay on the device as a `DescriptorRows`
(mad_amd/rows.py) and become host objects only when somebody reads them.  The cache is written from and read into arrays
(`set_load`, no row objects).  `get_solutions` matches every subunit and ensemble frame of this rank against the resident map set in
`match_topk_many_begin` / `_finish` brackets, each match handing back its own clouds (`mad_match_topk_many_begin2`), then filters,
refines and writes subunit by subunit in the reference's order.  MAD_STAGE_PATH=1 keeps the stage-by-stage path (Orientator ->
Descriptor -> _RowSet -> one match_topk per subunit / frame); both write the same files.

`run()` options and the resident path: ori_eqsp_size, dsc_eqsp_size and dsc_subregions are accepted and ignored on both paths, as
the reference ignores them (only patch_size reaches the stages), and run() has no gw_sig (Orientator's default, 0,
is what both paths use).  patch_size gives r = patch_size // 2 (an odd size loses one, as Orientator / Descriptor print); the
resident path covers r = 2, 4, 6, 8, 10, 12 (patch_size 4-5, 8-9, 12-13, 16-17, 20-21, 24-25), the radii the description kernel is
built for.  Any other patch_size falls back to the stage path with a one-line message (the stage path then reports the kernel's
own error).  At r = 12 (patch_size 24, 25: the reference's low-resolution example) a count can pass 127 and the sets are "wide"
(include/mad_amd.h): built sets know it by their radius, sets loaded from the descriptor cache or from stage rows are told by
`get_descriptors`, which has the patch size; results are the same, the match runs on one device per subunit as always.
`mad.timings`: wall seconds per stage of the last run() (prep, mapspace, detector, build, cache_io, match, filter, refine_ccc, write).
`mad.timings_detail`: the filter stage split into filter_cluster (the clustering: device call or host loop) and filter_place (the
candidate list: reading the PDB, placing and copying the chain where a caller wants it), summed over the subunits;
`mad.filter_undecided`: matches of the last run() the device left to the host loop.

Kept from the reference: method names, argument order and defaults, the
`results/<map>_<comps>_res..._iso...` folder layout, the `Solutions_refined_<k>.csv`
header and the descriptor cache file name (MaD.py:118).  Replaced: the h5py cache
becomes an `.npz` with the same four datasets when h5py is missing; the map is written
with the built-in MRC writer.  Assembly building (MaD.py:632-843) is out of scope for
the hot path; `build_assembly` is provided by mad_amd.assembly when present.
"""
import os
import time
from copy import deepcopy
from operator import itemgetter

import numpy as np

from . import _lib
from .DensityFeature import DensityFeature
from .Descriptor import Descriptor
from .Detector import Detector
from .Dmap import Dmap
from .MapSpace import MapSpace
from .math_utils import get_rototrans_SVD
from .Orientator import Orientator
from .PDB import PDB
from .rows import DescriptorRows
from .structure_utils import dock_refine_score_many, move_copy_structure

try:      # optional: the reference's cache format
    import h5py
except Exception:      # pragma: no cover - h5py is absent in the build image
    h5py = None

# result-row columns of MaD.py:451 / :461-474
D_CC, REPEAT, LO_IDX, LO_OCT, LO_BIN, HI_IDX, HI_OCT, HI_BIN = range(8)
HI_COORD, LO_COORD = slice(8, 11), slice(11, 14)
R1, R2, R3 = slice(14, 17), slice(17, 20), slice(20, 23)

TIMING_KEYS = ("prep", "mapspace", "detector", "build", "cache_io", "match", "filter", "refine_ccc", "write")
DETAIL_KEYS = ("filter_cluster", "filter_place")
RMSDCLOUD_THRESH = 10      # MaD.py:476
BRACKET_MAX = 16      # matches per bracket: two per lane of the context (MAD_RES); a chunk's ensemble frames are closed behind it


class _RowSet(object):
    """Host view of a descriptor list + its device-resident twin (mad_set)."""

    def __init__(self, lib, dsc_list, wide=False):
        n = len(dsc_list)
        self.n_rows = n
        subv = np.array([df.subv_map_coords for df in dsc_list], dtype=np.float64).reshape(-1, 3)
        # anchors = unique sub-voxel coordinates, lexicographically sorted like np.unique (MaD.py:427-428)
        if n:
            self.anchors, self.row_anchor = np.unique(subv, axis=0, return_inverse=True)
            self.row_anchor = np.asarray(self.row_anchor, dtype=np.int32).reshape(-1)
        else:
            self.anchors, self.row_anchor = np.zeros((0, 3)), np.zeros(0, np.int32)
        first = np.zeros(len(self.anchors), np.int64)
        first[self.row_anchor[::-1]] = np.arange(n)[::-1]
        idx = np.array([df.index for df in dsc_list], dtype=np.int32)
        octv = np.array([df.oct_scale for df in dsc_list], dtype=np.int32)
        main = np.array([df.main_bin for df in dsc_list], dtype=np.int32)
        R = np.array([df.Rfinal for df in dsc_list], dtype=np.float64).reshape(-1, 9)
        dsc = np.array([df.lin_ar_subeqsp for df in dsc_list], dtype=np.int16).reshape(n, -1)
        self.dev = lib.set_load(self.row_anchor, main, R, dsc, self.anchors, idx[first] if n else idx, octv[first] if n else octv,
                                wide=wide)


class MaD(object):
    def __init__(self):
        self.input_map = None
        self.input_subunits = {}
        self.input_ensembles = {}
        self.processed_map = None
        self.processed_subunits = {}
        self.processed_ensembles = {}
        self.buildable_subunits = {}
        self.out_folder = None
        self.dsc_dict = {}
        self._rowsets = {}
        self.timings = dict.fromkeys(TIMING_KEYS, 0.0)
        self.timings_detail = dict.fromkeys(DETAIL_KEYS, 0.0)
        self.filter_undecided = 0  # matches of the last run() whose clustering the device left to the host loop
        self.n_correlations = 0    # descriptor pairs correlated by the matches of the last run() (rows x rows per match)
        self._fallback = None      # why the last run() took the stage path although MAD_STAGE_PATH is not set (None: it did not)
        self._pending = []         # resident path: this rank's matches not yet run, [(key, n_copies, is_frame)]
        self._matched = {}         # ... and their outcome, key -> (top rows, map cloud, structure cloud, clustering or None)

    def _stage(self):
        """True when this run takes the stage-by-stage path (MAD_STAGE_PATH=1, or options the resident path does not cover)."""
        return os.environ.get("MAD_STAGE_PATH", "0") == "1" or self._fallback is not None

    def _tick(self, key, t0):
        self.timings[key] = self.timings.get(key, 0.0) + time.perf_counter() - t0

    def _tick_detail(self, key, seconds):
        self.timings_detail[key] = self.timings_detail.get(key, 0.0) + seconds

    @staticmethod
    def _cluster_on_device(n_rows):
        """Whether a match with n_rows rows to cluster goes to Lib.pose_cluster_many: not under MAD_FILTER_HOST=1, not when it is
        empty, and not beyond the rows the entry takes (POSE_CLUSTER_MAX_N; the host loop has no limit)."""
        return os.environ.get("MAD_FILTER_HOST", "0") != "1" and 0 < n_rows <= _lib.POSE_CLUSTER_MAX_N

    @staticmethod
    def resident_unsupported(patch_size=16):
        """Why mad_set_build cannot serve these run() options (None when it can); see the module docstring."""
        r = int(patch_size) // 2
        if r not in (2, 4, 6, 8, 10, 12):
            return "patch_size %s (radius %d): the resident build describes r = 2, 4, 6, 8, 10, 12 only" % (patch_size, r)
        return None

    # ------------------------------------------------------------------ inputs
    def add_subunit(self, sub_filename_folder, n_copies=1, identifier=""):
        assert os.path.exists(sub_filename_folder), "MaD> subunit or ensemble not found: %s" % sub_filename_folder
        if os.path.isfile(sub_filename_folder):
            filename = os.path.splitext(os.path.split(sub_filename_folder)[-1])[0]
            key = identifier if identifier != "" else filename
            if key in self.input_subunits:
                print("MaD> subunit %s already added; overwriting" % filename)
            self.input_subunits[key] = [sub_filename_folder, n_copies]
            print("MaD> Added: subunit %s" % sub_filename_folder)
        elif os.path.isdir(sub_filename_folder):
            folder = os.path.basename(os.path.normpath(sub_filename_folder))
            key = identifier if identifier != "" else folder
            frames = [os.path.join(sub_filename_folder, x) for x in os.listdir(sub_filename_folder) if x.split(".")[-1] in ("pdb", "PDB")]
            if not frames:
                print("MaD> No PDB files found in ensemble folder %s" % sub_filename_folder)
                return
            self.input_ensembles[key] = {}
            for frame in frames:
                fkey = os.path.splitext(os.path.split(frame)[-1])[0]
                print("      > Added frame: ", fkey)
                self.input_ensembles[key][fkey] = [frame, n_copies]
            print("MaD> Added: ensemble %s of %i frames" % (key, len(frames)))
        else:
            print("MaD> Error: %s not a valid structure or ensemble" % sub_filename_folder)

    def add_map(self, input_map, resolution, isovalue=0):
        assert os.path.exists(input_map), "MaD> Exp. map not found: %s" % input_map
        assert resolution > 0, "MaD> Map cannot have a negative resolution"
        self.resolution = resolution
        self.isovalue = isovalue
        self.input_map = input_map
        self.map_name = os.path.splitext(os.path.split(input_map)[-1])[0]
        print("MaD> Added: density map %s, resolution %.2f A" % (self.map_name, self.resolution))

    # ------------------------------------------------------------------ ranks
    def _ranks(self):
        """(rank, world, torch.distributed or None).  More than one rank only under a launcher (WORLD_SIZE > 1)."""
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world <= 1:
            return 0, 1, None
        import torch.distributed as dist
        if not dist.is_initialized():
            import datetime
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29544")      # (a launcher sets its own; this is the fallback of a hand-started job)
            # a rank that died must not hold the others for the backend's default half hour
            dist.init_process_group(os.environ.get("MAD_CONTROL_BACKEND", "gloo"),
                                    timeout=datetime.timedelta(seconds=int(os.environ.get("MAD_DIST_TIMEOUT_S", "600"))))
        return dist.get_rank(), dist.get_world_size(), dist

    def _all_ranks(self, dist, work):
        """Runs `work()` on this rank and agrees with the others on the outcome BEFORE the exchange that follows: the helpers of the
        reference print and sys.exit(1) on bad input (Dmap.py:45-49, PDB.py:13-15), and a rank that leaves alone would hold the
        others in the next barrier until the group's timeout.  Every rank raises when any rank failed."""
        err, out = None, None
        try:
            out = work()
        except BaseException as e:      # SystemExit included
            err = "%s: %s" % (type(e).__name__, e)
        seen = [None] * dist.get_world_size()
        dist.all_gather_object(seen, err)
        bad = [(r, e) for r, e in enumerate(seen) if e is not None]
        if bad:
            raise RuntimeError("MaD> rank %d failed (%s); stopping all %d ranks" % (bad[0][0], bad[0][1], len(seen)))
        return out

    # ------------------------------------------------------------------ driver
    def run(self, transform_subunits=False, detect_sigma=2.0, presmooth_sigma=1, ori_eqsp_size=112, dsc_eqsp_size=16,
            dsc_subregions=64, patch_size=16, cc_threshold=0.6, weight_threshold=4, n_samples=60):
        self.transform_subunits = transform_subunits
        self.timings = dict.fromkeys(TIMING_KEYS, 0.0)
        self.timings_detail = dict.fromkeys(DETAIL_KEYS, 0.0)
        self.filter_undecided = 0
        self.n_correlations = 0
        self._fallback = None
        if os.environ.get("MAD_STAGE_PATH", "0") != "1":
            self._fallback = self.resident_unsupported(patch_size)
            if self._fallback is not None:
                print("MaD> %s; taking the stage path" % self._fallback)
        t0 = time.perf_counter()
        ok = self.check_preprocess_data()
        self._tick("prep", t0)
        if not ok:
            return
        self.get_descriptors(detect_sigma=detect_sigma, presmooth_sigma=presmooth_sigma, patch_size=patch_size,
                             ori_eqsp_size=ori_eqsp_size, dsc_eqsp_size=dsc_eqsp_size, dsc_subregions=dsc_subregions)
        self.get_solutions(cc_threshold=cc_threshold, weight_threshold=weight_threshold, n_samples=n_samples)

    def check_preprocess_data(self):
        if self.input_map is None or not (len(self.input_subunits) + len(self.input_ensembles)):
            print("MaD> Make sure you have defined at least one component and a density map")
            if self.input_map is not None:
                print("     > Map: %s" % self.input_map)
            for k in self.input_subunits:
                print("     > Subunit: %s" % k)
            return False      # the reference falls through and crashes later (MaD.py:104-113)
        rank, world, dist = self._ranks()
        if world == 1:
            self._prep_files_folders()
            return True
        # one results folder for the job: rank 0 prepares it, everybody learns its name and the processed inputs
        state = [None]
        if rank == 0:
            self._all_ranks(dist, self._prep_files_folders)
            state = [(self.out_folder, self.processed_map, getattr(self, "voxsp", None), self.processed_subunits, self.processed_ensembles)]
        else:
            self._all_ranks(dist, lambda: None)
        dist.broadcast_object_list(state, src=0)
        self.out_folder, self.processed_map, self.voxsp, self.processed_subunits, self.processed_ensembles = state[0]
        return True

    def _cache_name(self, key, detect_sigma, presmooth_sigma, patch_size, ori_eqsp_size, dsc_eqsp_size):
        # MaD.py:118 (the trailing 64 is a literal in the reference)
        return (f"dsc_db/{key}_res{self.resolution}_iso{self.isovalue}_detSig{detect_sigma}_presmooth{presmooth_sigma}"
                f"_patch{patch_size}_orieqsp{ori_eqsp_size}_dsceqsp{dsc_eqsp_size}_subregions{64}.h5")

    def get_descriptors(self, detect_sigma=2.0, presmooth_sigma=1, ori_eqsp_size=112, dsc_eqsp_size=16, dsc_subregions=64, patch_size=16):
        self._wide = int(patch_size) // 2 >= 11      # what sets loaded from rows of this patch size are marked as (Lib.set_load)
        def described(key, struct, what):
            name = self._cache_name(key, detect_sigma, presmooth_sigma, patch_size, ori_eqsp_size, dsc_eqsp_size)
            if self._cache_exists(name):
                t0 = time.perf_counter()
                rows = self._load_descriptors(name)
                self._tick("cache_io", t0)
                print("MaD> %i descriptors for %s found in database" % (len(rows), key))
                return rows, name
            print("\nMaD> Processing %s %s" % (what, key))
            rows = self._describe_struct(struct, detect_sigma, presmooth_sigma, ori_eqsp_size, dsc_eqsp_size, dsc_subregions, patch_size)
            t0 = time.perf_counter()
            self._save_descriptors(rows, name)
            self._tick("cache_io", t0)
            return rows, name

        rank, world, dist = self._ranks()
        if world > 1:
            # the structures to describe, in the reference's order, dealt round-robin; a rank describes its own (into the cache:
            # dsc_db/ is the hand-over), then everybody loads the map's rows and refers to the others by cache name
            jobs = [(self.map_name, self.processed_map, "map")] + [(k, v[0], "subunit") for k, v in self.processed_subunits.items()]
            for ek in self.processed_ensembles:
                jobs += [(fk, v[0], "frame") for fk, v in self.processed_ensembles[ek].items()]
            names = {}
            for key, struct, what in jobs:
                names[key] = self._cache_name(key, detect_sigma, presmooth_sigma, patch_size, ori_eqsp_size, dsc_eqsp_size)
            self._all_ranks(dist, lambda: [described(key, struct, what) for i, (key, struct, what) in enumerate(jobs) if i % world == rank])
            dist.barrier()
            t0 = time.perf_counter()
            self.map_dsc = self._load_descriptors(names[self.map_name])
            self._tick("cache_io", t0)
            for k in self.processed_subunits:
                self.dsc_dict[k] = names[k]
            for ek in self.processed_ensembles:
                self.dsc_dict[ek] = {}
                for fk in self.processed_ensembles[ek]:
                    self.dsc_dict[fk] = names[fk]
            return
        self.map_dsc, _ = described(self.map_name, self.processed_map, "map")
        for k in self.processed_subunits:
            self.dsc_dict[k], _ = described(k, self.processed_subunits[k][0], "subunit")
        for ek in self.processed_ensembles:
            self.dsc_dict[ek] = {}
            print("\nMaD> Describing ensemble %s" % ek)
            for fk in self.processed_ensembles[ek]:
                rows, name = described(fk, self.processed_ensembles[ek][fk][0], "frame")
                # stage path: frames are re-loaded when matched (MaD.py:158-162); resident path: a frame's rows stay where they are
                # (a built set on the device, or the cache's arrays, loaded into a set by its bracket) until its match has run
                self.dsc_dict[fk] = name if self._stage() else rows

    def get_solutions(self, cc_threshold=0.6, weight_threshold=4, n_samples=120):
        rank, world, dist = self._ranks()
        if world > 1:
            # MaD.py:165-190: one independent docking per subunit / frame -> dealt round-robin (mad_amd.dist.shard_round_robin); the
            # file lists come back in the reference's order on every rank
            from .dist import shard_round_robin
            jobs = [("sub", k, k) for k in self.processed_subunits]
            for ek in self.processed_ensembles:
                jobs += [("frame", ek, fk) for fk in self.processed_ensembles[ek]]
            mine = {}
            self._plan_matches([(key, (self.processed_subunits[key] if kind == "sub" else self.processed_ensembles[owner_key][key])[1], kind == "frame")
                                for kind, owner_key, key in shard_round_robin(jobs, rank, world)])

            def dock_mine():
                for kind, owner_key, key in shard_round_robin(jobs, rank, world):
                    pdbfile, n_copies = self.processed_subunits[key] if kind == "sub" else self.processed_ensembles[owner_key][key]
                    mine[(kind, owner_key, key)] = self._match_filter_refine(pdbfile, n_copies, key, cc_threshold, weight_threshold, n_samples)

            self._all_ranks(dist, dock_mine)
            everyone = [None] * world
            dist.all_gather_object(everyone, mine)
            files_of = {}
            for part in everyone:
                files_of.update(part)
            for kind, owner_key, key in jobs:
                files = files_of[(kind, owner_key, key)]
                if kind == "sub":
                    if len(files):
                        self.buildable_subunits[key] = [self.processed_subunits[key][1], files]
                else:
                    ensemble = self.processed_ensembles[owner_key]
                    if owner_key not in self.buildable_subunits:
                        self.buildable_subunits[owner_key] = [ensemble[list(ensemble.keys())[0]][1], []]
                    self.buildable_subunits[owner_key][1].extend(files)
            return
        self._plan_matches([(k, v[1], False) for k, v in self.processed_subunits.items()] +
                           [(fk, v[1], True) for ek in self.processed_ensembles for fk, v in self.processed_ensembles[ek].items()])
        for k in self.processed_subunits:
            pdbfile, n_copies = self.processed_subunits[k]
            files = self._match_filter_refine(pdbfile, n_copies, k, cc_threshold, weight_threshold, n_samples)
            if len(files):
                self.buildable_subunits[k] = [n_copies, files]
        for ek in self.processed_ensembles:
            ensemble = self.processed_ensembles[ek]
            n_copies = ensemble[list(ensemble.keys())[0]][1]
            self.buildable_subunits[ek] = [n_copies, []]
            for fk in ensemble:
                pdbfile, n_copies = ensemble[fk]
                self.buildable_subunits[ek][1].extend(self._match_filter_refine(pdbfile, n_copies, fk, cc_threshold, weight_threshold, n_samples))

    def build_assembly(self, max_models=10, max_overlap_complex=0.1):
        """MaD.py:192-222; the overlap table and the model CCCs are device calls (mad_amd/assembly.py)."""
        from . import assembly
        rank, world, dist = self._ranks()
        if world > 1:      # one rank builds the models (the combinatorics are sequential); the others wait for its files
            out = self._all_ranks(dist, lambda: assembly.build_assembly(self, max_models=max_models, max_overlap_complex=max_overlap_complex) if rank == 0 else None)
            dist.barrier()
            return out
        return assembly.build_assembly(self, max_models=max_models, max_overlap_complex=max_overlap_complex)

    def _build_from_single(self, sub_key, homomultimer=False):
        from . import assembly
        return assembly.build_from_single(self, sub_key, homomultimer=homomultimer)

    def _build_models(self, sub_sol_dict):
        from . import assembly
        return assembly.build_models(self, sub_sol_dict)

    def _write_complex_from_components(self, components, outname):
        from . import assembly
        assembly.write_complex(components, outname)

    def score_ensembles(self):
        if not self.processed_ensembles:
            print("MaD> No ensembles were provided and/or processed")
            return
        if self._ranks()[0] != 0:      # the tables are printed once
            return
        import csv
        for ek, ensemble in self.processed_ensembles.items():
            ranking = []
            for fk in sorted(ensemble):
                path = os.path.join(self.out_folder, "Solutions_refined_%s.csv" % fk)
                if not os.path.exists(path):
                    continue
                with open(path) as fh:
                    rows = list(csv.DictReader(fh))
                if rows:
                    ranking.append([fk] + [float(np.mean([float(r[c]) for r in rows])) for c in ("Repeatability", "Weight", "mCC", "RWmCC")])
            print("MaD> Ranking for ensemble %s: " % ek)
            for col, title in ((1, "Repeatability"), (2, "Weight"), (3, "Cross-corr."), (4, "MaD score")):
                print("%s     Top 3 - %s:" % ("" if col == 1 else "\n", title))      # blank line between the tables (MaD.py:267-273)
                for i, r in enumerate(sorted(ranking, key=itemgetter(col), reverse=True)[:3]):
                    print("     %i: %6.2f %s" % (i + 1, r[col], r[0]))

    # ------------------------------------------------------------------ files and folders
    def _prep_files_folders(self):
        for d in ("results", "dsc_db"):
            if not os.path.exists(d):
                os.mkdir(d)
        subs = ["%sx%i" % (k, self.input_subunits[k][1]) for k in sorted(self.input_subunits)]
        ens = ["%sx%i" % (k, self.input_ensembles[k][list(self.input_ensembles[k].keys())[0]][1]) for k in sorted(self.input_ensembles)]
        out = f"results/{self.map_name}_{'.'.join(subs + ens)}_res{self.resolution:.3f}_iso{self.isovalue:.3f}"
        if os.path.exists(out):
            i = 1
            while os.path.exists("%s_%i" % (out, i)):
                i += 1
            out = "%s_%i" % (out, i)
        os.mkdir(out)
        self.out_folder = out
        print("MaD> Created output folder: %s" % out)
        init_path = os.path.join(out, "initial_files")
        os.mkdir(init_path)
        ext = os.path.splitext(self.input_map)[-1].lower()
        if ext in (".sit", ".situs", ".mrc", ".map"):
            lo_map = Dmap(self.input_map, isovalue=self.isovalue)
            lo_map.reduce_void()
            self.voxsp = lo_map.voxsp
            self.processed_map = os.path.join(init_path, "%s_mad.mrc" % self.map_name)
            lo_map.write_to_mrc(self.processed_map)
        elif ext == ".pdb":
            print("MaD> PDB provided for density map: %s" % self.input_map)
            print("     Simulating at specified resolution and voxel spacing of 1.2 angstroms")
            self.voxsp = 1.2
            self.processed_map = os.path.join(init_path, "%s_simulated_map.mrc" % self.map_name)
            PDB(self.input_map).structure_to_density(self.resolution, self.voxsp, outname=self.processed_map)
        else:
            print("MaD> ERROR: density map not understood (either sit/mrc/map format or PDB for simulated density): %s" % self.input_map)
        for k, (pdb_file, n_copies) in self.input_subunits.items():
            out_name = os.path.join(init_path, "%s.pdb" % k)
            move_copy_structure(pdb_file, out_name, transform=self.transform_subunits)
            self.processed_subunits[k] = [out_name, n_copies]
        for ek, ensemble in self.input_ensembles.items():
            self.processed_ensembles[ek] = {}
            for fk, (pdb_file, n_copies) in ensemble.items():
                out_name = os.path.join(init_path, os.path.split(pdb_file)[-1])
                move_copy_structure(pdb_file, out_name, transform=self.transform_subunits)
                self.processed_ensembles[ek][fk] = [out_name, n_copies]

    # ------------------------------------------------------------------ hot path
    def _describe_struct(self, struct, detect_sigma, presmooth_sigma, ori_eqsp_size, dsc_eqsp_size, dsc_subregions, patch_size):
        """MaD.py:358-368.  As in the reference, only patch_size reaches the stages.  Resident path: a DescriptorRows
        over a set built by Lib.set_build; stage path: the list of DensityFeature rows of Orientator + Descriptor."""
        ms = MapSpace(struct, resolution=self.resolution, voxelsp=self.voxsp, sig_init=detect_sigma, sig_presmooth=presmooth_sigma)
        det = Detector()
        t0 = time.perf_counter()
        ms.build_space()
        self._tick("mapspace", t0)
        t0 = time.perf_counter()
        anchors = det.find_anchors(ms)
        self._tick("detector", t0)
        t0 = time.perf_counter()
        if self._stage():
            ori = Orientator(ori_radius=patch_size)
            dsc = Descriptor(dsc_radius=patch_size)
            oriented = ori.assign_orientations(ms, anchors)
            rows = dsc.generate_descriptors(ms, oriented)
        else:
            rows = self._build_rows(ms, anchors, patch_size)
        self._tick("build", t0)
        ms.release_device()
        return rows

    @staticmethod
    def _bind_tables(lib):
        """The EQSP tables of Orientator() / Descriptor() (112 orientation zones with their matrices, 16 descriptor zones), loaded
        the way their _bind does, and no orientation window."""
        if lib._eq_loaded.get(0) != ("ori", 112):
            Orientator()._bind(lib)
        if lib._eq_loaded.get(1) != ("dsc", 16):
            Descriptor()._bind(lib)
        lib.set_orient_window(0.0)

    def _build_rows(self, ms, anchors, patch_size):
        """Orientation + description of the detector's anchors into one device set (mad_set_build): the rows of
        Orientator(ori_radius=patch_size) + Descriptor(dsc_radius=patch_size), in their order, without a row object."""
        lib = _lib.get_lib()
        self._bind_tables(lib)
        print("MaD> Orienting and describing %i anchors on the device..." % len(anchors))
        slots = ms.device_slots(lib)
        kinds = ms.space.kinds      # list entry -> 0 upsampled / 1 base: the octave the kernels sample with
        slot_of_octave = [-1, -1]
        for e, kd in enumerate(kinds):
            slot_of_octave[kd] = slots[e]
        n = len(anchors)
        entry = np.array([df.oct_scale for df in anchors], np.int64)
        coords = np.array([df.coords for df in anchors], np.int64).reshape(n, 3)
        map_coords = np.array([df.map_coords for df in anchors], np.float64).reshape(n, 3)
        subv = np.array([df.subv_map_coords for df in anchors], np.float64).reshape(n, 3)
        index = np.array([df.index for df in anchors], np.int64)
        octave = np.array(kinds, np.int32)[entry] if n else np.zeros(0, np.int32)
        dev = lib.set_build(slot_of_octave, coords, octave, subv, index, r=int(patch_size) // 2, lim_main=6, lim_sec=6, gw_sig=0.0)
        dev.size()      # waits for the build: it reads the MapSpace fields, which are freed next
        return DescriptorRows.built(dev, index, entry, coords, map_coords, subv, eqsp_size=112, subeqsp_size=16, D=1024)

    def _rowset(self, lib, dsc_list):
        key = id(dsc_list)
        hit = self._rowsets.get(key)
        if hit is None or hit[0] is not dsc_list or hit[1].dev.lib is not lib:
            hit = (dsc_list, _RowSet(lib, dsc_list, wide=getattr(self, "_wide", False)))
            self._rowsets[key] = hit
        return hit[1]

    def _match_device(self, lo_dsc_list, hi_dsc_list, anchor_dist_thresh, cc_threshold, k):
        lib = _lib.get_lib()
        lo, hi = self._rowset(lib, lo_dsc_list), self._rowset(lib, hi_dsc_list)
        top, idx, stats = lib.match_topk(hi.dev, lo.dev, cc_threshold, anchor_dist_thresh, k)
        self.n_correlations = getattr(self, "n_correlations", 0) + stats["n_corr"]
        if stats["n_pairs"]:
            uh, ul = lib.match_used(len(hi.anchors), len(lo.anchors))
            hi_cloud, lo_cloud = hi.anchors[uh], lo.anchors[ul]
        else:
            hi_cloud, lo_cloud = np.zeros((0, 3)), np.zeros((0, 3))
        return lib, lo, hi, top, idx, stats, lo_cloud, hi_cloud

    def _match_dsc(self, lo_dsc_list, hi_dsc_list, anchor_dist_thresh=4, cc_threshold=0.65):
        """MaD.py:414-453: (list of float64[23] rows in row-major pair order, lo_mapcoords, hi_mapcoords)."""
        lib, lo, hi, _, _, stats, lo_cloud, hi_cloud = self._match_device(lo_dsc_list, hi_dsc_list, anchor_dist_thresh, cc_threshold, 1)
        res = lib.match_results(hi.dev, lo.dev, stats["n_pairs"]) if stats["n_pairs"] else np.zeros((0, 23))
        return list(res), lo_cloud, hi_cloud

    def _match_dsc_topk(self, lo_dsc_list, hi_dsc_list, k, anchor_dist_thresh=4, cc_threshold=0.65):
        """The first k rows of sorted(_match_dsc(...)[0], key=repeatability, reverse=True) (MaD.py:480),
        selected and ordered on the device, plus the two clouds."""
        _, _, _, top, _, _, lo_cloud, hi_cloud = self._match_device(lo_dsc_list, hi_dsc_list, anchor_dist_thresh, cc_threshold, k)
        return top, lo_cloud, hi_cloud

    def _plan_matches(self, jobs):
        """Resident path: the matches this rank will ask _match_filter_refine for, [(key, n_copies, is_frame)] in that order.  The
        first request runs them all, in brackets (_run_brackets)."""
        self._pending = [] if self._stage() else list(jobs)
        self._matched = {}

    def _as_rows(self, x):
        """DescriptorRows of a structure, whichever form dsc_dict / map_dsc hold it in (rows, a cache name, a list of rows)."""
        if isinstance(x, DescriptorRows):
            return x
        if isinstance(x, str):
            t0 = time.perf_counter()
            rows = self._load_descriptors(x)
            self._tick("cache_io", t0)
            return rows if isinstance(rows, DescriptorRows) else DescriptorRows.from_arrays(self._list_arrays(rows), wide=getattr(self, "_wide", False))
        return DescriptorRows.from_arrays(self._list_arrays(x), wide=getattr(self, "_wide", False))

    def _run_brackets(self, cc_threshold, n_samples):
        """Every planned match against the resident map set, up to BRACKET_MAX per match_topk_many bracket, all at
        k = the largest n_samples * n_copies: a subunit keeps its first n_samples * n_copies rows, which are its own top-k because the
        device order is a total order (repeatability descending, then row-major pair rank -- the stable sort of MaD.py:480).  Each
        match's clouds come from its own anchor-use flags, in np.unique(..., axis=0) order (MaD.py:427-428).  A chunk's ensemble
        frames are closed behind its bracket."""
        lib = _lib.get_lib()
        jobs, self._pending = self._pending, []
        if not jobs:
            return
        lo = self._as_rows(self.map_dsc)
        self.map_dsc = lo
        K = max(int(n_samples * n) for _, n, _ in jobs)
        for c0 in range(0, len(jobs), BRACKET_MAX):
            chunk = jobs[c0:c0 + BRACKET_MAX]
            rows = [self._as_rows(self.dsc_dict[key]) for key, _, _ in chunk]
            t0 = time.perf_counter()
            h = lib.match_topk_many_begin([r.dev for r in rows], lo.dev, cc_threshold, 4.0, K, want_used=True)
            out = lib.match_topk_many_finish(h)
            done = []
            for (key, n_copies, frame), r, (top, _, st, uh, ul) in zip(chunk, rows, out):
                self.n_correlations += st["n_corr"]
                if st["n_pairs"]:
                    hi_cloud, lo_cloud = np.unique(r.anchor_subv[uh], axis=0), np.unique(lo.anchor_subv[ul], axis=0)
                else:
                    hi_cloud, lo_cloud = np.zeros((0, 3)), np.zeros((0, 3))
                done.append((key, top[:int(n_samples * n_copies)], lo_cloud, hi_cloud))
                if frame:      # one frame resident only until its match has run (MaD.py:158-162, 379-380)
                    r.close()
            self._tick("match", t0)
            # the chunk's pose clustering in one call: the clouds exist only now
            t0 = time.perf_counter()
            todo = [d for d in done if self._cluster_on_device(len(d[1]))]
            clusters = self._cluster_matches(lib, [d[1] for d in todo], [d[3] for d in todo]) if todo else []
            by_key = {d[0]: c for d, c in zip(todo, clusters)}
            for key, top, lo_cloud, hi_cloud in done:
                self._matched[key] = (top, lo_cloud, hi_cloud, by_key.get(key))
            self._tick("filter", t0)
            self._tick_detail("filter_cluster", time.perf_counter() - t0)

    @staticmethod
    def _cluster_matches(lib, tops, hi_clouds):
        """Lib.pose_cluster_many on the rows of several matches (each already cut to its n_samples * n_copies rows, in the order
        _filter_dsc_pairs gives them) -> per match (owner, d2min, n_done, status)."""
        return lib.pose_cluster_many([np.asarray(t, np.float64) for t in tops], hi_clouds, [len(t) for t in tops], rmsd_thresh=float(RMSDCLOUD_THRESH))

    def _match_filter_refine(self, pdbfile, n_copies, k, cc_threshold, weight_threshold, n_samples):
        n_samples_sub = int(n_samples * n_copies)
        print("MaD> Matching descriptors (%s vs. %s) (cc = %.2f)..." % (self.map_name, k, cc_threshold))
        if not self._stage() and (k in self._matched or any(j[0] == k for j in self._pending)):
            if k not in self._matched:
                self._run_brackets(cc_threshold, n_samples)
            top, map_anchors, comp_anchors, cluster = self._matched.pop(k)
        else:
            t0 = time.perf_counter()
            from_cache = isinstance(self.dsc_dict[k], str)
            hi_list = self._load_descriptors(self.dsc_dict[k]) if from_cache else self.dsc_dict[k]
            top, map_anchors, comp_anchors = self._match_dsc_topk(self.map_dsc, hi_list, n_samples_sub, cc_threshold=cc_threshold)
            if from_cache:      # an ensemble frame re-loaded for this match (MaD.py:158-162, 379-380): one frame resident at a time
                hit = self._rowsets.pop(id(hi_list), None)
                if hit is not None:
                    hit[1].dev.close()
            self._tick("match", t0)
            cluster = None
            if self._cluster_on_device(min(len(top), n_samples_sub)):      # the same entry as the resident path, with one match
                t0 = time.perf_counter()
                cluster = self._cluster_matches(_lib.get_lib(), [top[:n_samples_sub]], [comp_anchors])[0]
                self._tick("filter", t0)
                self._tick_detail("filter_cluster", time.perf_counter() - t0)
        if not len(top):
            print("MaD> No descriptor pair above the threshold for %s" % k)
            return []
        print("MaD> Filtering descriptor pairs (map %s vs. structure %s) (weight=%i, n_samples=%i*%i)..." % (self.map_name, k, weight_threshold, n_samples, n_copies))
        t0 = time.perf_counter()
        filtered = self._filter_match(pdbfile, top, map_anchors, comp_anchors, cluster, weight_threshold, n_samples_sub)
        self._tick("filter", t0)
        print("MaD> Refining %s in %s..." % (self.map_name, k))
        t0 = time.perf_counter()
        refined = self._refine_filtered_solutions(pdbfile, filtered, map_anchors, comp_anchors)
        self._tick("refine_ccc", t0)
        t0 = time.perf_counter()
        files = self._save_solutions_refined(refined, k)
        self._tick("write", t0)
        return files

    def _filter_match(self, pdbfile, top, map_anchors, comp_anchors, cluster, weight_threshold, n_samples_sub):
        """The candidate list of one match for the run: from the device's clustering `cluster` = (owner, d2min, n_done, status) when it
        decided every row, else (None: MAD_FILTER_HOST=1 or more rows than the entry takes; status 1: a decision inside the guard band)
        from the host loop.  The run
        reads poses, weights and members of a candidate, never its placed chain (_refine_filtered_solutions reads elements 0, 1, 2, 4
        and 8), so the device path does not read the PDB, place or copy it."""
        t0 = time.perf_counter()
        if cluster is not None and cluster[3] == 0:
            filtered = self._filter_from_owner(pdbfile, top, cluster[0], weight_threshold, place=False)
            self._tick_detail("filter_place", time.perf_counter() - t0)
            return filtered
        self.filter_undecided += cluster is not None
        detail = {}
        filtered = self._filter_dsc_pairs(pdbfile, top, map_anchors, comp_anchors, wthresh=weight_threshold, n_samples=n_samples_sub,
                                          presorted=True, _detail=detail)
        self._tick_detail("filter_cluster", detail["cluster"])
        self._tick_detail("filter_place", time.perf_counter() - t0 - detail["cluster"])
        return filtered

    def _filter_dsc_pairs(self, pdbfile, match_data, lo_cloud, hi_cloud, wthresh=4, n_samples=200, presorted=False, _detail=None):
        """Greedy clustering of the best poses by cloud RMSD (MaD.py:456-553).  Host, float64.  _detail: a dict that receives the
        seconds of the clustering loop under "cluster"."""
        rmsdcloud_thresh = RMSDCLOUD_THRESH
        data = np.array(match_data if presorted else sorted(match_data, key=itemgetter(REPEAT), reverse=True))
        chain = PDB(pdbfile)
        chain_init = chain.get_coords().copy()
        init_hi_cloud = hi_cloud.copy()

        def moved_cloud(s):
            return np.dot(init_hi_cloud - s[HI_COORD], np.array([s[R1], s[R2], s[R3]]).T) + s[LO_COORD]

        best = data[0]
        cand_ids = [0]
        cand_clouds = [moved_cloud(best)]
        weights = {0: 1}
        members = {0: [[best[HI_COORD], best[LO_COORD], best[HI_BIN], best[LO_BIN]]]}
        counter = 1
        t_loop = time.perf_counter()
        for s in data[1:n_samples]:
            cur = moved_cloud(s)
            rmsd = np.sqrt(np.sum(np.square(cand_clouds - cur), axis=(1, 2)) / len(cur))
            if np.amin(rmsd) > rmsdcloud_thresh:
                cand_ids.append(counter)
                cand_clouds.append(cur)
                weights[counter] = 1
                members[counter] = [[s[HI_COORD], s[LO_COORD], s[HI_BIN], s[LO_BIN]]]
            else:
                owner = cand_ids[int(np.argmin(rmsd))]
                weights[owner] += 1
                members[owner].append([s[HI_COORD], s[LO_COORD], s[HI_BIN], s[LO_BIN]])
            counter += 1
        if _detail is not None:
            _detail["cluster"] = time.perf_counter() - t_loop
        rep_thresh = max(5, best[REPEAT] * 0.3)
        out = []
        for cand in cand_ids:
            s = data[cand]
            w = weights[cand]
            if w < wthresh or s[REPEAT] < rep_thresh:
                continue
            Rt = np.array([s[R1], s[R2], s[R3]]).T
            chain.set_coords(chain_init)
            chain.translate_atoms(-s[HI_COORD])
            chain.rotate_atoms(Rt)
            chain.translate_atoms(s[LO_COORD])
            out.append([s[HI_COORD], s[LO_COORD], Rt, s[D_CC], w, s[REPEAT], s[REPEAT] * w, deepcopy(chain), members[cand]])
        return sorted(out, key=itemgetter(6), reverse=True)

    def _filter_from_owner(self, pdbfile, data, owner, wthresh, place=True):
        """The list _filter_dsc_pairs returns, from its sorted rows `data` and the clustering `owner` (owner[i] = the row that leads
        row i's cluster, owner[i] == i for a leader; len(owner) rows took part): weights = rows per leader, members in row order,
        the weight and repeatability thresholds, the chain placed per kept candidate, and the stable sort by repeat * weight with
        the leaders going in in row order.  place=False leaves the chain (element 7) None and does not read the PDB."""
        data = np.array(data)
        owner = np.asarray(owner)
        n = len(owner)
        best = data[0]
        weights = np.bincount(owner, minlength=n)
        members = {}
        for i in range(n):
            s = data[i]
            members.setdefault(int(owner[i]), []).append([s[HI_COORD], s[LO_COORD], s[HI_BIN], s[LO_BIN]])
        if place:
            chain = PDB(pdbfile)
            chain_init = chain.get_coords().copy()
        rep_thresh = max(5, best[REPEAT] * 0.3)
        out = []
        for cand in np.flatnonzero(owner == np.arange(n)):
            s = data[cand]
            w = int(weights[cand])
            if w < wthresh or s[REPEAT] < rep_thresh:
                continue
            Rt = np.array([s[R1], s[R2], s[R3]]).T
            placed = None
            if place:
                chain.set_coords(chain_init)
                chain.translate_atoms(-s[HI_COORD])
                chain.rotate_atoms(Rt)
                chain.translate_atoms(s[LO_COORD])
                placed = deepcopy(chain)
            out.append([s[HI_COORD], s[LO_COORD], Rt, s[D_CC], w, s[REPEAT], s[REPEAT] * w, placed, members[int(cand)]])
        return sorted(out, key=itemgetter(6), reverse=True)

    def _refine_filtered_solutions(self, pdbfile, filtered_candidate_list, lo_cloud, hi_cloud):
        """MaD.py:556-629 with all candidates refined in ONE launch (one workgroup each)."""
        from scipy.spatial import cKDTree
        hi_pdb = PDB(pdbfile)
        hi_init = hi_pdb.get_coords().copy()
        dmap = Dmap(self.processed_map)
        if not len(filtered_candidate_list):
            return []
        # placement, refinement, density simulation and CCC of every candidate in ONE device call (MaD.py:566-575, 613-616): the poses go
        # in, the refined coordinates and one score per candidate come back
        n_c = len(filtered_candidate_list)
        coords, _, _, ccc_all = dock_refine_score_many(dmap, hi_init, hi_pdb.atom_masses(), np.array([c[0] for c in filtered_candidate_list]),
                                                       np.array([c[1] for c in filtered_candidate_list]),
                                                       np.array([c[2] for c in filtered_candidate_list]).reshape(n_c, 9), self.resolution,
                                                       n_steps=500, max_step_size=1, min_step_size=0.1)
        tree = cKDTree(lo_cloud)
        refined = []
        for cand, xyz, ccc in zip(filtered_candidate_list, coords, ccc_all):
            weight, clustered = cand[4], cand[8]
            if np.any(np.isnan(xyz)):
                continue
            R, T = get_rototrans_SVD(hi_init, xyz)
            moved = np.dot(hi_cloud, R) + T
            dist, _ = tree.query(moved, distance_upper_bound=dmap.voxsp * 1.5)
            repeat = 100 * np.count_nonzero(dist < dmap.voxsp * 2) / hi_cloud.shape[0]
            if repeat > 0:
                sol = deepcopy(hi_pdb)
                sol.set_coords(xyz)
                refined.append([sol, moved[dist < dmap.voxsp * 2], repeat, weight, clustered, float(ccc)])
        final = []
        for sol, corresp, repeat, weight, clustered, ccc in refined:
            if final:
                rmsds = [sol.get_rmsdCA_with(f[0]) for f in final]
                if np.min(rmsds) < 6:      # a clone of an earlier solution: merge (MaD.py:609-612)
                    j = int(np.argmin(rmsds))
                    final[j][3] += weight
                    final[j][5].extend(clustered)
                    continue
            final.append([sol, corresp, repeat, weight, ccc, clustered])
        for sol in final:
            sol.append(sol[2] * sol[3] * sol[4])
        return sorted(final, key=itemgetter(-1), reverse=True)

    # ------------------------------------------------------------------ I/O
    @staticmethod
    def _npz_name(name):
        return name[:-3] + ".npz" if name.endswith(".h5") else name + ".npz"

    def _cache_exists(self, name):
        return (h5py is not None and os.path.exists(name)) or os.path.exists(self._npz_name(name))

    @staticmethod
    def _list_arrays(df_list):
        """The four cache datasets of a list of DensityFeature rows."""
        return dict(
            dsc=np.array([df.lin_ar_subeqsp for df in df_list], dtype=np.int16),
            info=np.array([[df.index, df.main_bin, df.sec_bin, df.oct_scale, df.eqsp_size, df.subeqsp_size] for df in df_list]).astype(np.uint16),
            coords=np.array([[df.coords, df.map_coords, df.subv_map_coords] for df in df_list], dtype=np.float64),
            rot=np.array([df.Rfinal for df in df_list], dtype=np.float64))

    def _save_descriptors(self, df_list, outname):
        """MaD.py:849-858.  A DescriptorRows is written from its arrays(), without row objects; the file is the same."""
        data = df_list.arrays() if isinstance(df_list, DescriptorRows) else self._list_arrays(df_list)
        if h5py is not None:
            with h5py.File(outname, "w") as hf:
                for k, v in data.items():
                    hf.create_dataset(k, data=v)
        else:
            np.savez(self._npz_name(outname), **data)

    def _load_descriptors(self, input_name):
        if h5py is not None and os.path.exists(input_name):
            with h5py.File(input_name, "r") as hf:
                data = {k: np.array(hf.get(k)) for k in ("dsc", "info", "coords", "rot")}
        else:
            with np.load(self._npz_name(input_name)) as z:
                data = {k: z[k] for k in ("dsc", "info", "coords", "rot")}
        if not self._stage():      # resident path: the arrays as they are; the set is loaded from them (set_load) when first matched
            return DescriptorRows.from_arrays(data, wide=getattr(self, "_wide", False))
        rows = []
        for d, c, i, r in zip(data["dsc"], data["coords"], data["info"], data["rot"]):
            df = DensityFeature()
            df.set_from_file_dsc(int(i[0]), int(i[1]), int(i[2]), int(i[3]), int(i[4]), int(i[5]), c[0], c[1], c[2], r, d)
            rows.append(df)
        return rows

    def _save_solutions_refined(self, refined_solutions, sub_key):
        sol_path = os.path.join(self.out_folder, "individual_solutions")
        anchor_path = os.path.join(sol_path, "anchor_files")
        os.makedirs(anchor_path, exist_ok=True)
        sep = "------------------------------------------"
        print("\n" + sep + "\n|  # | Repeat | Weight |   mCC  |  RWmCC |\n" + sep)
        table, files = [], []
        for idx, (pdb, corresp, repeat, weight, ccc, clustered, score) in enumerate(refined_solutions):
            fname = os.path.join(sol_path, "sol_%s_%i.pdb" % (sub_key, idx))
            pdb.write_pdb(fname)
            files.append(fname)
            self._save_coords_as_pdb(corresp, os.path.join(anchor_path, "corresp_anchors_%s_%i.pdb" % (sub_key, idx)))
            print("| %2i | %6.2f | %6i | %6.2f | %6.2f |" % (idx, repeat, weight, ccc, score))
            table.append([idx, repeat, weight, ccc, score])
        print(sep + "\n")
        if table:
            with open(os.path.join(self.out_folder, "Solutions_refined_%s.csv" % sub_key), "w") as fh:
                fh.write("ID,Repeatability,Weight,mCC,RWmCC\n")
                def num(v):      # as pandas.to_csv prints it: shortest repr in the value's own precision
                    return str(v) if isinstance(v, (np.floating, np.integer)) else repr(v)
                for row in table:
                    fh.write("%i,%s,%s,%s,%s\n" % (row[0], num(row[1]), num(row[2]), num(row[3]), num(row[4])))
        return files

    def _save_coords_as_pdb(self, coords, outname):
        with open(outname, "w") as fh:
            for i, c in enumerate(coords):
                fh.write("%-6s%5i  %-3s %3s%2s%4i    %8.3f%8.3f%8.3f%6.2f%6.2f          %-2s\n"
                         % ("ATOM", i % 100000, "O", "EPC", "E", i % 10000, c[0], c[1], c[2], 1.0, i / len(coords), "O"))      # B = rank in the list (MaD.py:1001)
