/*
 * mad_amd.h -- C-ABI of libmad_amd.so, the MI355X (gfx950) implementation of the
 * MaD anchor-matching hot path.
 *
 * The reference (LBM-EPFL/MaD) has no FFI: its boundary is a set of Python
 * methods.  Each entry point below replaces the *body* of one of them; the
 * Python mirror in mad_amd/ keeps the reference's names and signatures and calls
 * these through ctypes.  See INTEGRATION.md for the binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MAD_E* code; nothing
 *     throws across the ABI; mad_last_error(ctx) gives the message;
 *   - unless a parameter says "device", buffers are caller-owned HOST memory
 *     (numpy arrays) and the call is synchronous on return;
 *   - the library owns only what lives inside a mad_ctx / mad_set;
 *   - one ctx per GPU; a ctx is not thread-safe, distinct ctxs may be driven
 *     from distinct threads;
 *   - 3x3 matrices are row-major double[9]; volumes are [nx][ny][nz], z fastest;
 *   - variable-length outputs take a capacity; on overflow the call returns
 *     MAD_ENOSPC and stores the needed size in the count argument.
 *
 * File:line references are into the reference checkout (mad/...).
 */
#ifndef MAD_AMD_H
#define MAD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAD_OK        0
#define MAD_EINVAL   -22   /* bad argument */
#define MAD_ENOMEM   -12   /* device allocation failed */
#define MAD_ENOSPC   -28   /* output capacity too small */
#define MAD_ENODEV   -19   /* no usable gfx950 device */
#define MAD_EDOM     -33   /* input outside the supported range */
#define MAD_EHIP     -5    /* HIP runtime error */

#define MAD_MAX_Z      128 /* zones per EQSP table */
#define MAD_MAX_FIELDS 64  /* gradient-field slots per ctx */
#define MAD_POSE_CLUSTER_MAX_N 4096 /* rows of one match in mad_pose_cluster_many (a d2 triangle of 64 MiB) */
#define MAD_RANK_MAX_N 96    /* rows of the overlap table in mad_rank_copies / mad_rank_models (LDS: DESIGN.md section 4f) */
#define MAD_RANK_MAX_K 16    /* copies of a subunit / groups of a model, at most */
#define MAD_RANK_MAX_TOP 512 /* entries a MAD_RANK_TOP call may ask for (the workgroups' lists in LDS) */
#define MAD_RANK_MAX_OUT 4096 /* entries a MAD_RANK_BELOW call, or the band of mad_rank_models, may return */
#define MAD_RANK_TOP 0
#define MAD_RANK_BELOW 1
#define MAD_RESULT_COLS 23 /* row width of MaD._match_dsc results, MaD.py:451 */

typedef struct mad_ctx mad_ctx;
typedef struct mad_set mad_set;   /* device-resident oriented-anchor rows of one structure */

/* ---- context ----------------------------------------------------------- */

int mad_init(int device, mad_ctx **out);
void mad_destroy(mad_ctx *ctx);
const char *mad_last_error(const mad_ctx *ctx);   /* ctx may be NULL: last init error */
int mad_synchronize(mad_ctx *ctx);
/*
 * A ctx owns 8 "lanes" (a HIP stream + its scratch buffers each).  Independent work -- the builds of different
 * mad_sets, the matches of one mad_match_topk_many call -- is enqueued on different lanes and overlaps on the
 * device; every entry point still returns only results that are complete.  mad_stream returns the stream of
 * lane 0 (the one the stage API uses), for callers that time with events.
 * mad_set_overlap(ctx, 0) makes every lane enqueue on that one stream, so kernels run one at a time: the mode in
 * which the duration of a launch is a property of the kernel alone (profiling, per-kernel rooflines).
 */
void *mad_stream(mad_ctx *ctx);
int mad_set_overlap(mad_ctx *ctx, int on);
/*
 * Per-kernel-group timing with HIP events recorded on the ctx stream around each launch.
 * Groups: "orient", "describe", "correlate", "pairs", "pose", "topk", "refine", "density", "ccc".
 * mad_assembly_density / mad_assembly_refine: "jf_model" (splat and blur), "jf_field" (M, s, texels or residual), "jf_steps".
 * Off by default; mad_timing_get drains pending events (a sync) and returns the accumulated
 * device time and launch count since the last reset; mad_last_ms = total / launches (<0 if none).
 */
int mad_timing_enable(mad_ctx *ctx, int on);
int mad_timing_reset(mad_ctx *ctx);
int mad_timing_get(mad_ctx *ctx, const char *what, double *total_ms, int64_t *launches);
double mad_last_ms(mad_ctx *ctx, const char *what);

/*
 * Measurement aid (bench.py, SURVEY.md 8(d) "confirm with a device copy microbenchmark in the same run"): the rate of a
 * streaming device copy of 1 GiB (read + write bytes per second, GB/s) and the issue rate of v_mfma_i32_16x16x64_i8 with
 * register operands (the instruction of the correlation kernel, int8 TOP/s), measured on this ctx's device now.  Either
 * pointer may be NULL.  No reference counterpart.
 */
int mad_probe_peaks(mad_ctx *ctx, double *copy_gbs, double *i8_tops);

/*
 * EQSP zone tables.  which = 0: orientation sphere (Orientator.py:16, 112 zones);
 * which = 1: descriptor sphere (Descriptor.py:17, 16 zones).  bounds = Z x
 * [theta_min, phi_min, theta_max, phi_max] (eqsp.py:16-20).  For which = 0 also
 * pass the 3x3 matrices the reference derives from the zone centres:
 * to_dom[a] = rotation bringing the centre of zone a onto +z (Orientator.py:198-205,
 * identity for a = 0) and adj_sec[a] = z-rotation of Orientator.py:259-263.
 */
int mad_set_eqsp(mad_ctx *ctx, int which, int Z, const double *bounds,
                 const double *to_dom, const double *adj_sec);
/*
 * The table classifier k_describe reads for the 4-byte texels, built from a zone table alone: host arithmetic, no context and no
 * device (mad_set_eqsp calls it).  zbelt_out: 2048 bytes, z bin -> belt; ptab_out: 4 x 2048 bytes, belt x pseudo-angle bin -> zone;
 * 255 = the table does not decide.  Returns 1 when built, 0 when this zone table does not fit the classifier (more than 4 belts or
 * more than 127 zones: every entry is 255 and k_describe takes its other form), MAD_EINVAL otherwise.  No reference counterpart.
 */
int mad_eqsp_tab_build(const double *bounds, int Z, unsigned char *zbelt_out, unsigned char *ptab_out);

/* ---- gradient fields (input of the path; produced by MapSpace.py:178-189) ---- */

/*
 * Upload one octave's gradient field into slot (0..MAD_MAX_FIELDS-1): three planar
 * float32 volumes, the layout of the reference's grad_list view (MapSpace.py:187).
 * On the device the field is repacked to one 16-byte texel per voxel
 * {gx, gy, gz, |g|}.
 */
int mad_upload_field(mad_ctx *ctx, int slot, const float *gx, const float *gy, const float *gz,
                     int nx, int ny, int nz);
/* Same, from a DEVICE buffer holding the three planes back to back ([3][nx][ny][nz]). */
int mad_upload_field_device(mad_ctx *ctx, int slot, const float *g3_device, int nx, int ny, int nz);
int mad_free_field(mad_ctx *ctx, int slot);
/*
 * Diagnostic: copies a slot's texels back to the host, tex_xyzw = [nx*ny*nz][4] float32 {gx, gy, gz, |g|} and
 * tex4 = [nx*ny*nz] packed 4-byte texels, both in linear [nx][ny][nz] order (on the device the 4-byte texels lie in padded
 * bricks of 4x4x2 voxels; they are taken apart here and exactly nx*ny*nz words are written); either pointer may be NULL.
 * Waits for the stream.  MAD_EINVAL for an empty or out-of-range slot.  Nothing on the path calls it.
 */
int mad_field_download(mad_ctx *ctx, int slot, float *tex_xyzw, uint32_t *tex4);

/* ---- a1-a8: Orientator.assign_orientations (Orientator.py:68-110) ------------ */

/*
 * coords: n x 3 integer voxel positions in the octave of `slot` (DensityFeature.coords).
 * octave: 1 = base grid (unit stride), 0 = upsampled grid (stride 2), Orientator.py:128-158.
 * r = box_side (8 for the default patch of 16).  Rows are emitted in anchor order
 * x main bin ascending x secondary bin ascending (Orientator.py:90-106).
 * row_count (nullable): Z quantised zone counts per row (DensityFeature.ar_count).
 * n_reject (nullable): anchors refused by the border test (Orientator.py:131-135).
 */
/*
 * Orientator(gw_sig = sigma) (Orientator.py:49-54): a Gaussian window exp(-d^2 / (2 sigma^2)) on the orientation histogram,
 * d = a voxel's offset from the anchor in voxels of the box.  0 (the default, and what MaD.run uses) = no window.  Applies
 * to mad_orient and mad_set_build from the next call on.  The reference truncates each zone's float64 weight sum to
 * int32 before it quantises; the kernel sums the weights in 2^-50 fixed point (deterministic, |error| < 1.2e-12 per
 * sum), so a zone count can differ from the reference's only where its weight sum lies that close to an integer.
 */
int mad_set_orient_window(mad_ctx *ctx, double gw_sig);
/* r = box_side 1 .. 12 (Orientator(ori_radius = 2 .. 25)); with a window (gw_sig != 0) 1 .. 10.  Beyond: MAD_EINVAL. */
int mad_orient(mad_ctx *ctx, int slot, int octave, const int32_t *coords, int n, int r,
               int lim_main, int lim_sec,
               int32_t *row_anchor, int32_t *row_main, int32_t *row_sec, double *row_R,
               int32_t *row_count, int64_t *n_rows, int64_t cap, int32_t *n_reject);

/* ---- a9-a10: Descriptor.generate_descriptors (Descriptor.py:106-202) --------- */

/*
 * coords: n_rows x 3 anchor voxel positions, R: n_rows x 9 Rfinal.  dsc: n_rows x
 * (64 * Zd) int16, sub-cube major (id j*16+i*4+k, Descriptor.py:44-64), zone minor.
 * A row whose sample cube leaves the grid is all zero (Descriptor.py:140-149).
 * r = dsc_radius / 2: 2, 4, 6, 8, 10 or 12 (odd radii and larger ones: MAD_EINVAL).  At r = 12 a sub-region holds
 * 6^3 = 216 samples, so a count may exceed 127: see "wide" sets below for what that means for a match.
 */
int mad_describe(mad_ctx *ctx, int slot, int octave, const int32_t *coords, const double *R,
                 int64_t n_rows, int r, int16_t *dsc);
/*
 * The same with another partition of the sample cube, Descriptor(dsc_size = 64 | 27 | 8 | 1) (Descriptor.py:44-93):
 * dsc is n_rows x (dsc_size * Zd), sub-regions in the order of the reference's sub_slices lists.  MaD.run never selects
 * them (it constructs Descriptor(dsc_radius=patch_size) only, MaD.py:362); 27, 8 and 1 exist for r = 8, and r = 10, 12
 * for 64 regions of 16 zones only.
 */
int mad_describe_sized(mad_ctx *ctx, int slot, int octave, const int32_t *coords, const double *R,
                       int64_t n_rows, int r, int dsc_size, int16_t *dsc);

/* ---- a11: MaD._match_dsc part 1 (MaD.py:416-424) ----------------------------- */

/*
 * hi: n_hi x D, lo: n_lo x D int16 descriptor counts (D = 1024; every |count| <= 127,
 * else MAD_EDOM).  Emits every (hi, lo) with normalised correlation > cc, row-major,
 * with its score.
 */
int mad_correlate(mad_ctx *ctx, const int16_t *hi, int64_t n_hi, const int16_t *lo, int64_t n_lo,
                  int D, double cc, int32_t *pair_hi, int32_t *pair_lo, double *pair_score,
                  int64_t *n_pairs, int64_t cap);

/* ---- a12: MaD._match_dsc part 2 (MaD.py:426-451) ----------------------------- */

/*
 * Per-row inputs: p = subv_map_coords (n x 3), R = Rfinal (n x 9), meta = {index,
 * oct_scale, main_bin} (n x 3 int32).  hi_cloud / lo_cloud: the unique sub-voxel
 * coordinates of rows present in at least one pair (MaD.py:427-428).
 * results (nullable): n_pairs x 23 as MaD.py:451.  counts (nullable): number of
 * hi cloud points brought within `dist` of a lo cloud point (repeatability =
 * 100 * count / l_hi).  dist > 0, any size: a dist too small for the float32 tier's band only makes that tier test
 * every candidate in float64.
 * Coordinates (p of both sides, both clouds) must lie within +-10 000 A (the range of the PDB format and a little more):
 * the search maps absolute coordinates to the voxels of its occupancy bitmaps in float32, with an error below
 * 1.87e-6 A + 1.2e-4 Angstrom for coordinates up to A, and the bitmaps allow for 0.02 ("The float32 voxel map").
 * Beyond: MAD_EDOM (also for a NaN).
 */
int mad_pose_score(mad_ctx *ctx, const int32_t *pair_hi, const int32_t *pair_lo, const double *pair_score,
                   int64_t n_pairs,
                   const double *hi_p, const double *hi_R, const int32_t *hi_meta, int64_t n_hi,
                   const double *lo_p, const double *lo_R, const int32_t *lo_meta, int64_t n_lo,
                   const double *hi_cloud, int64_t l_hi, const double *lo_cloud, int64_t l_lo,
                   double dist, double *results, int32_t *counts);

/*
 * Indices of the first k pairs in the order of MaD._filter_dsc_pairs' stable sort
 * (MaD.py:480): count descending, ties in input order.
 */
int mad_topk(mad_ctx *ctx, const int32_t *counts, int64_t n, int64_t k, int64_t *order);

/* ---- device-resident pipeline (same kernels, no host round trips) -------------- */

/*
 * A mad_set holds the oriented-anchor rows of one structure (map or subunit) on
 * the device: descriptors, Rfinal, anchor ids and the anchors' sub-voxel
 * coordinates.  mad_set_build runs a1-a10 for the anchors of both octaves:
 *   slot_of_octave[o] = field slot of octave o (or -1),
 *   anc_coords n x 3 int32, anc_octave n int32, anc_subv n x 3 double (Angstrom),
 *   anc_index n int32 (DensityFeature.index).
 * Row order = anchor order (as given) x main x sec, exactly the reference's list.
 * r = 2, 4, 6, 8, 10 or 12 (what mad_orient and mad_describe both take).
 *
 * Wide sets.  A set built at r >= 11 (i.e. 12) is WIDE: its counts reach 216, beyond an int8, so its int8 rows hold
 * count - 108 and every row carries c * sum(counts) - (D / 2) c^2 as int32; the correlation adds the two rows' terms to
 * the int8 dot product and so hands the exact int32 dot product of the counts to everything behind it.  Results are those
 * of the counts themselves.  A wide set matches wide sets only (against a narrow one: MAD_EINVAL), is matched whole on one
 * device (mad_set_export and the mad_match_shard_* calls refuse it with MAD_EINVAL), and takes counts 0 .. 235.
 */
int mad_set_create(mad_ctx *ctx, mad_set **out);
void mad_set_destroy(mad_ctx *ctx, mad_set *set);
int mad_set_build(mad_ctx *ctx, mad_set *set, const int *slot_of_octave,
                  const int32_t *anc_coords, const int32_t *anc_octave, const double *anc_subv,
                  const int32_t *anc_index, int n_anchors, int r, int lim_main, int lim_sec);
/* The same for n_sets structures at once -- the map and the subunits of a MaD.run step, which the reference describes one
 * after the other (MaD._describe_struct, MaD.py:358-368, called per structure from get_descriptors, MaD.py:116-163): ONE k_orient grid, one
 * scan, one row expansion and ONE k_describe grid over the anchors / rows of all of them, so that small structures do not each
 * pay a launch that cannot fill 256 CUs.  Arrays of n_sets entries; slot_of_octave has 2 per set.  Each set comes out exactly as
 * mad_set_build would have made it.  Asynchronous, on the lane of sets[0]; every set's consumers wait for its own event. */
int mad_set_build_many(mad_ctx *ctx, int n_sets, mad_set *const *sets, const int *slot_of_octave,
                       const int32_t *const *anc_coords, const int32_t *const *anc_octave,
                       const double *const *anc_subv, const int32_t *const *anc_index, const int *n_anchors,
                       int r, int lim_main, int lim_sec);
/* Load rows computed earlier (descriptor cache, MaD.py:861-875): anchor = row -> anchor id.
 * The rows are taken for narrow ones (counts -128 .. 127, else MAD_EDOM) unless the set has been marked with
 * mad_set_mark_wide(set, 1) before: then for those of a wide set (counts 0 .. 235, else MAD_EDOM).  The mark stays until it
 * is changed; mad_set_build does not look at it (it goes by r).  mad_set_is_wide: what the set holds now (1 / 0). */
int mad_set_mark_wide(mad_ctx *ctx, mad_set *set, int wide);
int mad_set_is_wide(mad_ctx *ctx, const mad_set *set);
int mad_set_load(mad_ctx *ctx, mad_set *set, int64_t n_rows, const int32_t *row_anchor,
                 const int32_t *row_main, const double *row_R, const int16_t *dsc, int D,
                 const double *anc_subv, const int32_t *anc_index, const int32_t *anc_octave, int n_anchors);
int mad_set_size(mad_ctx *ctx, const mad_set *set, int64_t *n_rows, int32_t *n_anchors);
/* Any of the output pointers may be NULL.  A set built on the device keeps its rows as int8 only (what a match reads): its int16
 * rows are materialised here, by one small kernel, the first time `dsc` is asked for after a build -- the count is the int8 value
 * (narrow sets) or the int8 value + 108 (wide sets), a row that left the grid is all zero.  A loaded or imported set hands out the
 * int16 rows it was given. */
int mad_set_download(mad_ctx *ctx, const mad_set *set, int32_t *row_anchor, int32_t *row_main,
                     int32_t *row_sec, double *row_R, int16_t *dsc);

/*
 * a11 + a12 + top-k for one (subunit = hi, map = lo) pair of sets, entirely on the
 * device.  results: k x 23 rows of MaD.py:451 in the order of MaD.py:480 (fewer if
 * n_pairs < k: *n_out).  pair_index (nullable): k row-major pair ranks.
 * stats (nullable) int64[4] = {n_pairs, l_hi, l_lo, n_correlations}.
 * dist > 0.  The anchors' sub-voxel coordinates lie within +-10 000 A: mad_set_build*, mad_set_load and mad_set_import refuse
 * others with MAD_EDOM, because the pose search maps absolute coordinates to bitmap voxels in float32 (error below
 * 1.87e-6 A + 1.2e-4 Angstrom for coordinates up to A, against the 0.02 the bitmaps allow for; see mad_pose_score).
 */
int mad_match_topk(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, double cc, double dist,
                   int64_t k, double *results, int64_t *pair_index, int64_t *n_out, int64_t *stats);
/*
 * The same for n subunit sets against one map set, with up to 4 matches in flight before the host waits for
 * the oldest.  results: n x k x 23; pair_index (nullable): n x k; n_out: n; stats (nullable): n x 4.
 * mad_match_fetch / _results / _used afterwards refer to the LAST match of the batch (every match's flags: mad_match_topk_many2).
 */
int mad_match_topk_many(mad_ctx *ctx, int n, const mad_set *const *hi, const mad_set *lo, double cc, double dist,
                        int64_t k, double *results, int64_t *pair_index, int64_t *n_out, int64_t *stats);

/*
 * The same call in two halves, for callers that keep the device fed: _begin enqueues every match and returns
 * (the output arrays belong to the bracket until _finish returns: _finish fills them; _begin itself only does so for a
 * match whose lane it has to reuse, n > 8).  Between the two the caller may enqueue other work -- typically
 * mad_set_build of the NEXT batch into other sets: sets read by the open bracket must not be rebuilt or destroyed, and
 * no other match call may be made.  Up to three brackets may be open at once (each has its own pinned result staging);
 * _finish completes the older one.
 */
int mad_match_topk_many_begin(mad_ctx *ctx, int n, const mad_set *const *hi, const mad_set *lo, double cc, double dist,
                              int64_t k, double *results, int64_t *pair_index, int64_t *n_out, int64_t *stats);
int mad_match_topk_many_finish(mad_ctx *ctx);
/*
 * The same two calls, and mad_match_topk_many, with every match's anchor-use flags -- what mad_match_used returns after a single
 * mad_match_topk -- for MaD.run, whose filter and refinement need each match's clouds (MaD.py:427-428).  Both arrays are nullable and
 * belong to the bracket until _finish returns, like the other outputs:
 *   used_hi: one byte per anchor of hi[0], then of hi[1], ... (sum of the hi sets' anchor counts); match i at the sum of the counts
 *            of hi[0 .. i-1];
 *   used_lo: n x (anchors of lo); match i at i * (anchors of lo).
 * 1 = the anchor is in at least one pair above cc.  Flags are per canonical anchor, as in mad_match_used: anchors with identical
 * sub-voxel coordinates count once, on the first of them in the set's anchor list; the others stay 0.  A match that is not run (an
 * empty set) leaves 0.  Each match's flags are copied on its own lane, in stream order, into pinned staging of the bracket before the
 * lane can take another match: no host synchronisation inside the bracket, and no device allocation.
 */
int mad_match_topk_many_begin2(mad_ctx *ctx, int n, const mad_set *const *hi, const mad_set *lo, double cc, double dist,
                               int64_t k, double *results, int64_t *pair_index, int64_t *n_out, int64_t *stats,
                               uint8_t *used_hi, uint8_t *used_lo);
int mad_match_topk_many2(mad_ctx *ctx, int n, const mad_set *const *hi, const mad_set *lo, double cc, double dist,
                         int64_t k, double *results, int64_t *pair_index, int64_t *n_out, int64_t *stats,
                         uint8_t *used_hi, uint8_t *used_lo);
/* on != 0: mad_match_topk_many(_begin) computes the score tiles of all matches of a bracket (first match of every lane) in ONE
 * GEMM grid -- fewer, fuller launches (C3: 0.151 -> 0.106 ms of device time per step) at the price of every match waiting for
 * the slowest set; off (default): one GEMM per match, each on its own lane, which overlaps better when several lanes are busy
 * (1.07 against 1.21 ms per overlapped C3 step).  Results are identical either way. */
int mad_set_batching(mad_ctx *ctx, int on);
/* Tuning values that change speed, never results.  "pose_split" (-1 auto: subunits of more than 512 anchors; 0 off; 1 on): the
 * pose search of mad_match_topk* brackets the best-scoring pairs first and, in a second launch, abandons every other pair as
 * soon as its running upper bound falls below the k-th lower bound of the first batch.  "pose_split_min": that first batch
 * holds at least this many pairs (default 4096) and at least 64 k.  "ori_queue" / "dsc_queue": entries in use of the queues through
 * which k_orient / k_describe hand the directions their fast classifiers cannot decide to the exact one (defaults: all 512 / 768);
 * a small value drives the kernels' full-queue paths for every anchor / row -- a test hook, the results are the same.  "fft_bpt"
 * (0 default, 1, 2, 4): butterflies per thread of k_fft_lines, i.e. which of its three forms mad_map_fft / mad_map_fsc / mad_map_filter / mad_map_ifft / mad_map_scan launch (by
 * default 1 up to N = 256, 2 at 512, 4 at 1024; a value below that is raised to it) -- a test hook, the bits are the same.
 * "search_prune" (1 default, 0): 0 makes mad_map_search run full line passes instead of the pruned ones -- a test hook, it changes
 * speed, never numbers.  "symmetry_scratch" (bytes, default 64 MiB): what the partial records of one chunk of operators of
 * mad_map_symmetry_score may take -- it changes the chunks, never numbers. */
int mad_set_option(mad_ctx *ctx, const char *name, double value);

/*
 * Which pose-scoring kernel the most recently enqueued match used: 0 = k_pose_lds (both clouds in LDS as float64),
 * 1 = k_pose_lds32 (lo cloud as float32 offsets in LDS), 2 = k_pose (global cell list), -1 = none yet.  For tests and
 * diagnostics: the three give identical counts, so only this tells when a sizing change has demoted a workload.
 */
int mad_last_pose_kernel(mad_ctx *ctx);
/*
 * Everything the host chose for the most recently ENQUEUED pose stage of the context (mad_pose_score, a match of
 * mad_match_topk*, mad_match_shard_topk / _score, or the completion of a pruned match by mad_match_fetch / mad_match_results):
 * the plan follows from the cloud sizes, the lo cloud's bounding box and dist alone, the last three flags also from what the
 * previous match of the lane selected.  Host-only: it launches nothing and changes no decision.  Every field is -1 before the first
 * pose stage.  For tests and diagnostics: all plans give identical counts, so only this tells which one a workload reached.
 */
typedef struct mad_pose_plan_info {
    int32_t kernel;          /* as mad_last_pose_kernel: 0 k_pose_lds, 1 k_pose_lds32, 2 k_pose (global cell list) */
    int32_t hi_in_lds;       /* the hi cloud sits in LDS: 1 for kernel 0 and k_pose_lds32<true>, 0 for k_pose_lds32<false> and kernel 2 */
    int32_t pruned;          /* the bounds pass (k_pose_bounds) ran and the exact search saw the selected pairs only */
    int32_t split;           /* the bounds pass ran as two launches; 0 when not pruned */
    int32_t nbv;             /* width of k_pose_bounds<NB, .> in sets of 64 hi points: 2, 4, 6, 8, 10, 12 or 16; 0 when not pruned */
    int32_t inner_plane;     /* the fine bitmap has its inner plane (bits_rad_in > 0.5); 0 for kernel 2 */
    int32_t grid_dim[3];     /* cells of the search grid per axis (kernel 2: of the global cell list) */
    int32_t own_selection;   /* k_pose_lds selected its own pairs (no k_prune_select launch) */
    int32_t topk_one_wg;     /* the k rows came from k_topk_selected (one workgroup); 0: the general top-k, or no top-k in this stage */
    int32_t sel_repeat;      /* this enqueue repeats the match because the selection outgrew the own / one-workgroup forms */
    int32_t fine_grown;      /* the fine voxel was enlarged to keep the bitmap within 16 MB */
    int32_t search_wgs;      /* workgroups of the exact search */
    int32_t fine_dim[3];     /* voxels of the fine bitmap per axis; 0 for kernel 2 */
    int32_t reserved;
    double fine_h, coarse_h; /* voxel edges of the fine bitmap and of the coarse one of the bounds pass (A); 0 for kernel 2 */
    double fine_mn[3];       /* origin of the fine bitmap (A) */
    double bits_rad, bits_rad_in;      /* radii of the outer and inner plane around a lo point (A) */
    int64_t lds64, lds32, lds32_hi;    /* LDS bytes the plan computed for k_pose_lds, k_pose_lds32<false>, k_pose_lds32<true> */
} mad_pose_plan_info;
int mad_last_pose_plan(mad_ctx *ctx, mad_pose_plan_info *out);
/*
 * How many pairs of the most recently COMPLETED match went through the exact search.  mad_match_topk* only report the k best
 * pairs (MaD.py:480,502), so the pose search first brackets every pair's count with the occupancy bitmaps alone (lower bound =
 * points certainly within dist, upper bound = those plus the points in the uncertain shell) and searches exactly only the pairs
 * whose upper bound reaches the k-th largest lower bound; the k rows and their order are those of the full search.  Equal to
 * n_pairs when nothing could be pruned.  mad_match_fetch(counts) / mad_match_results complete the other pairs on demand.
 */
int64_t mad_last_pose_selected(mad_ctx *ctx);
/* Device buffers the context has (re)allocated since mad_init (scratch and set storage grow on demand and never shrink).  Each is a
 * hipMalloc -- and, when it replaces a smaller buffer, a hipFree that waits for every stream.  A caller that pipelines steps can
 * check that its steady state shows none (bench.py: config.device_allocations_in_timed_region). */
int64_t mad_device_allocations(mad_ctx *ctx);
/* After mad_match_topk: all pairs of that call (for MaD._match_dsc's full return value). */
int mad_match_fetch(mad_ctx *ctx, int32_t *pair_hi, int32_t *pair_lo, double *pair_score,
                    int32_t *counts, int64_t cap);
/* After mad_match_topk(hi, lo, ...): the MaD.py:451 rows of ALL pairs, row-major pair order (n_pairs x 23). */
int mad_match_results(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, double *results, int64_t cap);
/* After mad_match_topk: which anchors of each set appear in a pair (uint8 flags). */
int mad_match_used(mad_ctx *ctx, uint8_t *hi_anchor_used, int32_t n_hi_anchors,
                   uint8_t *lo_anchor_used, int32_t n_lo_anchors);

/* ---- a13: structure_utils.refine_pdb (structure_utils.py:58-161) --------------- */

/*
 * Upload the density map the candidates are refined in (Dmap.grid3d, float32
 * [nx][ny][nz], origin and voxel spacing in Angstrom).  The library derives the
 * np.gradient field (structure_utils.py:80) once and keeps both.
 */
int mad_upload_density(mad_ctx *ctx, const float *grid, int nx, int ny, int nz,
                       double ox, double oy, double oz, double voxsp);
/*
 * Refine n_cand rigid placements of the same n_atoms-atom structure at once.  Each candidate
 * runs in G persistent workgroups that share its atoms and meet at every reduction (G from 1 to 8,
 * sized so that all n_cand x G workgroups are resident together); the atoms stay in registers when
 * a thread holds at most 8 of them, otherwise the kernel walks them in global memory.
 * coords: n_cand x n_atoms x 3, updated in place.  converged / last_step: per candidate, the
 * reference's return values.
 */
int mad_refine(mad_ctx *ctx, double *coords, int n_cand, int64_t n_atoms, int n_steps,
               double max_step, double min_step, int32_t *converged, int32_t *last_step);
/*
 * What the most recent refinement (mad_refine or mad_dock_refine_score) chose: *G = workgroups per candidate, *in_registers = 1 for
 * the register-resident kernel form, 0 for the one over global memory; both -1 before the first.  For tests and diagnostics: the
 * results of the plans agree to the last bits only, so only this tells when a sizing change has moved a workload to another plan.
 */
int mad_last_refine_plan(mad_ctx *ctx, int *G, int *in_registers);
/* Into how many chunks (of at most 512 Mi float64 voxels) the most recent density simulation cut its batch; -1 before the first. */
int mad_last_density_chunks(mad_ctx *ctx);

/* ---- next to a13: the placed bodies of an assembly refined together (mad_jointfit.hip) ---- */

/*
 * The model of n_bodies placed bodies (1 .. 64) on the lattice of the map given to mad_upload_density, and what the map holds
 * beyond it.  Body b's atoms are rows first_atom[b] .. first_atom[b + 1] - 1 of atoms (x 3, Angstrom) and mass; first_atom has
 * n_bodies + 1 entries, the first 0.  rho_b: the atoms splatted trilinearly, mass-weighted, onto the lattice (voxel (i, j, k) at
 * origin + vs (i, j, k); an atom counts when its cell index is 0 .. n - 2 on every axis) and blurred by the separable Gaussian of
 * mad_structure_to_density (sig = resolution / (pi sqrt 2) / vs, r = ceil(3 sig), taps of sum 1, zero beyond the lattice), float64,
 * neither normalised nor thresholded.  M = the sum of the rho_b in ascending b; *scale = s = <map, M> / <M, M> over the lattice (0
 * when <M, M> is 0).  model (nullable): M, float64 [nx][ny][nz].  residual (nullable): map - s M as float32.
 * MAD_EINVAL with a message for a NULL pointer, n_bodies outside 1 .. 64, an empty body, a coordinate or mass that is not finite,
 * resolution <= 0 (or a blur of more than 64 voxels) and a ctx without a map.
 */
int mad_assembly_density(mad_ctx *ctx, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                         double resolution, double *model, double *scale, float *residual);
/*
 * The bodies refined together.  Every body carries the state of refine_pdb (structure_utils.py:58-161: start coordinates and
 * their centre, the farthest atom, translation, rotation, step size, the coordinates at the last batch boundary).  A round is one
 * batch of refine_pdb: 4 steps, fewer in the last round when n_steps is no multiple of 4.  Before a round M and s are formed as
 * mad_assembly_density forms them from where the bodies stand; body b then takes the round's steps of refine_pdb against
 * F_b = float32(map - s (M - rho_b)), unless fixed[b] (nullable: none is) or converged.  The run ends when no body moves or
 * n_steps are taken.  With one body F is the map and the call is mad_refine.
 * coords: all atoms x 3, the refined coordinates.  rot (n_bodies x 9) and trans (n_bodies x 3): coords = (start - centre) rot +
 * centre + trans up to the rounding of the last step.  converged / last_step: refine_pdb's return values per body (a fixed body:
 * 0 and -1).  scale_per_round (nullable, (n_steps + 3) / 4 entries): s of every round that ran, 0 behind them.  *n_rounds: rounds
 * in which steps were taken.  Refusals as mad_assembly_density, and n_steps < 1 or steps that are not 0 < min_step <= max_step.
 */
int mad_assembly_refine(mad_ctx *ctx, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                        const uint8_t *fixed, double resolution, int n_steps, double max_step, double min_step, double *coords,
                        double *rot, double *trans, int32_t *converged, int32_t *last_step, double *scale_per_round,
                        int32_t *n_rounds);
/*
 * n_units asymmetric units refined under a point group.  The units are given as mad_assembly_refine's bodies
 * (atoms, mass, first_atom, fixed: per unit).  The n_ops operators are op_rot (n_ops x 9, row-major, for row vectors) and op_trans
 * (n_ops x 3): image (u, g) of unit u is x -> x op_rot[g] + op_trans[g], each component ((x R[0][j] + y R[1][j]) + z R[2][j]) + T[j],
 * and it is body u n_ops + g of the model; image 0 is the unit itself.  Operator 0 must be the identity bit for bit, every op_rot[g]
 * orthonormal (|R R^T - I| <= 1e-6 in every entry) with a positive determinant, and n_units n_ops at most 64.  A round is
 * mad_assembly_refine's over the images as bodies, except that the images of a unit take ONE common step: the force is the sum over
 * images and atoms of the gathered gradients pulled back into the unit's frame (h = g R^T), the torque that of cross(h, x - centre)
 * over the unit's own coordinates x, and the batch decision is taken on the unit's coordinates.  With n_ops = 1 every output is
 * mad_assembly_refine's, bit for bit.  coords (all unit atoms x 3), rot, trans, converged, last_step: per UNIT, as
 * mad_assembly_refine gives them per body.  Refusals as mad_assembly_refine, and the operator conditions above, each by name.
 */
int mad_assembly_refine_symmetric(mad_ctx *ctx, int n_units, const double *atoms, const double *mass, const int64_t *first_atom,
                                  const uint8_t *fixed, int n_ops, const double *op_rot, const double *op_trans, double resolution,
                                  int n_steps, double max_step, double min_step, double *coords, double *rot, double *trans,
                                  int32_t *converged, int32_t *last_step, double *scale_per_round, int32_t *n_rounds);
/*
 * What the most recent mad_assembly_refine or mad_assembly_refine_symmetric chose: *G = workgroups of body 0 (per image of unit 0),
 * *in_registers = the form of k_jf_steps / k_jf_steps_sym (1: a thread keeps its atoms in registers for the round; 0: global
 * memory), *workgroups = workgroups of all bodies (of all images).  -1 before the first.
 * mad_set_option "jointfit_split" (1 .. 8: workgroups per body at most) and "jointfit_registers" (0: never) are the tests' hooks.
 */
int mad_last_assembly_plan(mad_ctx *ctx, int *G, int *in_registers, int *workgroups);

/* ---- a14-a15: PDB.structure_to_density (PDB.py:131-292) ------------------------ */

/*
 * atoms n x 3 (Angstrom), mass n.  Call with grid = NULL to get dims (output grid
 * shape) and origin; then with grid = float32[dims0*dims1*dims2] ([x][y][z]).
 */
int mad_structure_to_density(mad_ctx *ctx, const double *atoms, const double *mass, int64_t n,
                             double resolution, double voxsp, double isovalue, int pad,
                             int32_t dims[3], double origin[3], float *grid);

/* ---- a16: Dmap.get_CCC_with_grid (Dmap.py:153-258) ----------------------------- */

/*
 * Both grids float32 [x][y][z]; voxels below isovalue are zeroed IN PLACE in both,
 * as the reference does (Dmap.py:160-161).  *ccc = <a,b>/sqrt(<a,a><b,b>) over the
 * overlap box, 0 if the boxes do not overlap.
 */
int mad_ccc(mad_ctx *ctx, float *grid1, const int32_t dims1[3], const double origin1[3],
            float *grid2, const int32_t dims2[3], const double origin2[3],
            double voxsp, double isovalue, double *ccc);

/* ---- next to a16: a map against a map (mad_mapops.hip) ---------------------------- */

/*
 * Dmap.mask_with (Dmap.py:99-151).  Host pointers, synchronous.  grid1 (float32 [x][y][z]) is updated IN PLACE: a voxel outside
 * the planes the reference's slices keep -- s = round(origin2 / voxsp - origin1 / voxsp) per axis (half to even), min = max(s, 0),
 * max = min(n1, n2 + s), `grid[:min] = 0`, `grid[max:] = 0` with python's slice semantics: a negative max zeroes the last -max
 * planes only -- or over a mask voxel < (float)1e-8 becomes 0; every other voxel keeps its bits.  The mask is read only.  Where
 * the reference raises IndexError (the mask begins behind the map's last plane: it has zeroed the whole map by then) this returns
 * MAD_OK with the map zeroed.  MAD_EINVAL: NULL, a dimension < 1, voxsp <= 0, a grid of 2^32 voxels or more.
 */
int mad_map_mask(mad_ctx *ctx, float *grid1, const int32_t dims1[3], const double origin1[3],
                 const float *mask, const int32_t dims2[3], const double origin2[3], double voxsp);

/*
 * A map times a soft mask (no counterpart in the reference).  Host pointers, synchronous.  grid1 (float32
 * [x][y][z]) is updated IN PLACE, the mask is read only.  The mask sits at the whole-voxel offset s = round(origin2 / voxsp -
 * origin1 / voxsp) per axis (half to even: mad_map_mask's expression), mask voxel j under grid voxel j + s; what is left of the offset
 * is rounded away, so a soft edge lands up to half a voxel from where its origin puts it.  Under the mask's box
 * g = (float)((double)g * (double)m), except that a voxel under m == 1 is not written (every bit stays); a voxel of grid 1 outside the
 * mask's box becomes +0.0f.  Where the boxes do not meet the whole grid becomes +0.0f and the call returns MAD_OK.
 * MAD_EINVAL: as mad_map_mask.
 */
int mad_map_multiply(mad_ctx *ctx, float *grid1, const int32_t dims1[3], const double origin1[3],
                     const float *mask, const int32_t dims2[3], const double origin2[3], double voxsp);

/*
 * Dmap.get_CCC_with_dmap (Dmap.py:260-372) of grid 1 against n second maps: grids2[j] float32 [x][y][z] with dims2[3 j ..] and
 * origins2[3 j ..].  Grid 1 is uploaded once and its voxels above the isovalue are counted once; the call with one map is the
 * n = 1 case of the same path (same bits).  No grid is modified.  With n1 / n2 = voxels of the whole grids above the isovalue and,
 * over the common box of mad_ccc (on a half-voxel tie the smaller extent, where the reference raises ValueError),
 * common = voxels with m2 != 0, m2 > isovalue, m1 > isovalue, S1 = sum m1^2 where m2 > 0, S2 = sum m2^2 where m1 > 0, D = sum m1 m2
 * (float32 comparisons, float64 sums in a fixed order):
 *     out[j] = 0 if common = 0 or min(n1, n2) = 0, else D / (sqrt(S1) sqrt(S2)) common / min(n1, n2)      (inf / NaN if S1 S2 = 0)
 * MAD_EINVAL: NULL, n < 1 or > 32767, a dimension < 1, voxsp <= 0, a grid of 2^32 voxels or more.
 */
int mad_map_ccc(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], int n,
                const float *const *grids2, const int32_t *dims2, const double *origins2,
                double voxsp, double isovalue, double *out);

/*
 * A map sampled on another lattice (mad_resample.hip).  Host pointers, synchronous.  grid: float32 [x][y][z]
 * with dims, origin (Angstrom, centre of voxel (0,0,0)) and spacing voxsp; out: float32 [x][y][z] with out_dims, out_origin,
 * out_voxsp, every voxel of it written.  R9 / T3 (both or neither; NULL, NULL: no motion) move the source rigidly before it is
 * sampled, in the convention of get_rototrans_SVD / PDB.rotate_atoms: R9 is the 3 x 3 matrix R row-major, R9[3 a + k] = R[a][k],
 * and a point x of the source (a row vector) moves to x @ R + T, i.e. x'_k = sum_a x_a R[a][k] + T_k.  Output voxel j lies at
 * y = out_origin + out_voxsp j and takes the source value at index u = ((y - T) @ R^T - origin) / voxsp, folded on the host into
 * u = b + A j with A[a][k] = (R[a][k] out_voxsp) / voxsp and
 * b[a] = ((((y0_0 - T_0) R[a][0] + (y0_1 - T_1) R[a][1]) + (y0_2 - T_2) R[a][2]) - origin[a]) / voxsp  (y0 = out_origin), and
 * evaluated as ((b_a + A_a0 jx) + A_a1 jy) + A_a2 jz in float64.  Where 0 <= u_a <= dims[a] - 1 on all three axes (both ends
 * included) the output is the interpolated value, elsewhere exactly 0.0f.  order 1: trilinear; order 3: cubic B-spline
 * interpolation (prefilter with pole sqrt(3) - 2, mirror boundary about the first and last sample); float64 sums, rounded to
 * float32 once: scipy.ndimage.map_coordinates(grid as float64, u, order, mode="constant", cval=0, prefilter=True).  No low-pass
 * filter before coarsening, no other boundary mode, no other order.  Without motion (or with R the identity bit for bit) the
 * volume is done as three 1-D passes from per-axis tables unless MAD_RESAMPLE_GENERAL=1 is set in the environment at the call.
 * MAD_EINVAL, with nothing launched: NULL, order other than 1 or 3, a source axis shorter than 2, an output dimension < 1,
 * voxsp or out_voxsp <= 0, 2^32 voxels or more in either grid, a number that is not finite, max|R R^T - I| > 1e-9 or det R < 0,
 * one of R9 / T3 without the other.
 */
int mad_map_resample(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                     const double *R9, const double *T3,          /* NULL, NULL: no motion */
                     int order, const int32_t out_dims[3], const double out_origin[3], double out_voxsp, float *out);

/*
 * The self-correlation of a map under a batch of rigid motions, and the average of a map over a set of them (mad_symmetry.hip,
 * mad_resample.hip; mad_amd/symmetry.py restates both with numpy).  Host pointers, synchronous, the grid is
 * not modified.  An operator g is a pair (R, T) in mad_map_resample's convention: R9[9 g + 3 a + k] = R_g[a][k], T3[3 g + k], a
 * point x (a row vector, Angstrom) moves to x @ R + T.
 *
 * mad_map_symmetry_score: out[6 g ..] = (n, sum a, sum b, sum a^2, sum b^2, sum a b) over the sample points j.  Candidates are the
 * lattice indices j_a = stride k_a; with c = (ball_centre - origin) / voxsp and r = radius / voxsp the box holds per axis the k_a
 * with |j_a - c_a| <= r and 0 <= j_a <= dims[a] - 1, and a point of the box counts when ((dx dx + dy dy) + dz dz) <= r r
 * (d = j - c, float64).  a = (double)grid[j]; b = the float32 that mad_map_resample(order 1, R_g, T_g, onto the map's own
 * lattice) writes at voxel j in its general form (the same fold into u = b + A j, the same expressions, 0 outside
 * 0 <= u <= dims - 1).  The box is walked in linear [x][y][z] order in runs of 256, points that do not count enter every sum as
 * +0.0, and every sum is paired as fourier.tree_sum pairs it (a run by halving, then level after level): the same call gives the
 * same bits, whatever the chunking.  An empty box gives n = 0 and zero sums.  The operators are scored in chunks whose partial
 * records fit mad_set_option "symmetry_scratch" bytes (default 64 MiB; one operator's records at least); all operators of a chunk
 * are one grid.  MAD_EINVAL, with nothing launched and out untouched: NULL, n_ops < 1, stride < 1, radius < 0, a dimension < 2,
 * 2^32 voxels or more, voxsp <= 0, a number that is not finite, an R that mad_map_resample refuses.
 *
 * mad_map_symmetrize: out[j] = (float)((sum over g of v_g) / n_ops) on the map's own lattice, v_g the float64 interpolated value
 * of the map moved by operator g at voxel j before any rounding to float32 (0 outside the source), the sum from +0.0 in the order
 * g = 0, 1, ...  order 1: trilinear; order 3: the cubic B-spline of mad_map_resample, prefiltered once per call.  n_ops = 1 gives
 * mad_map_resample's bits (general form).  MAD_EINVAL as mad_map_resample, and for n_ops outside 1 .. 64.
 *
 * mad_last_symmetry_plan: operators per workgroup of the score kernel (a constant), and the chunks and the bytes of partial records
 * of the most recent mad_map_symmetry_score (-1 before the first).  Any pointer may be NULL.
 */
int mad_map_symmetry_score(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                           const double ball_centre[3], double radius, int32_t stride, int32_t n_ops, const double *R9,
                           const double *T3, double *out);
int mad_map_symmetrize(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, int32_t n_ops,
                       const double *R9, const double *T3, int order, float *out);
int mad_last_symmetry_plan(mad_ctx *ctx, int32_t *ops_per_workgroup, int32_t *n_chunks, int64_t *scratch_bytes);

/*
 * Flexible fitting: the atoms of a model moved one by one up the gradient of the map given to mad_upload_density, held together
 * by an elastic network (mad_flexfit.hip; DESIGN.md section 4za, restated in mad_amd/flexfit.py).  Host pointers, synchronous.
 *
 * mad_flex_network: every pair of the n_atoms coordinates (n x 3 float64) with (dx dx + dy dy) + dz dz <= cutoff cutoff in float64,
 * dx = x_j - x_i, is a spring, stored for both atoms: first[n_atoms + 1] (a row per atom), nbr[] (a row's neighbours in ascending
 * atom index) and rest[] (the square root of that sum), bit for bit flexfit.network_numpy's.  *n_springs receives first[n_atoms];
 * MAD_ENOSPC when it exceeds cap_springs, the capacity of nbr and rest (then only *n_springs is written).  MAD_EDOM when an atom
 * has more than MAD_FLEX_MAX_DEGREE neighbours (a convention: all-atom protein has 45 - 80 within 6 A); the message names the atom,
 * its degree and the cutoff.  MAD_EINVAL: NULL, n_atoms outside 1 .. 2^24 - 1, a coordinate that is not finite, cutoff <= 0.
 *
 * mad_flex_fit: n_steps steps at most of x_i += F_i step / max_j |F_j|, F_i = (w_i g_i) / g0 + sum over the row of atom i of
 * ((stiffness (d - d0)) / d) (x_j - x_i): g_i k_refine's gather of the gradient texels (0 unless the atom lies strictly inside
 * the map), g0 = sqrt(sum |w_i g_i|^2 / n) at the start, d the length of x_j - x_i now and d0 the rest length.  weights (n, NULL:
 * all 1) and fixed (n bytes, NULL: none; a fixed atom keeps its bits) are optional.  The network is the caller's: mad_flex_network's,
 * or any with first[0] = 0, ascending first, rows that may be empty and need not be symmetric, neighbours in range and strictly
 * ascending within a row, no atom its own neighbour, finite positive rest lengths.  After every 4 steps the step size halves
 * when no atom moved as far as one step size since the last look; a step size below min_step is convergence, and so is a step in
 * which no atom feels a force.  *last_step: the step that ended the run (refine_pdb's meaning); *step: the final step size; a NaN
 * in a coordinate or a force ends the run with *converged = 0.  The same bits on every plan and in every call.
 * MAD_EDOM when g0 is 0 (no atom feels the map).  MAD_EINVAL: NULL, n_atoms < 1, a coordinate or weight that is not finite,
 * stiffness < 0, n_steps < 1, not 0 < min_step <= max_step, no map, a malformed network.
 *
 * mad_last_flex_plan: the workgroups, the threads of each, the atoms a thread owns at most and the springs of the most recent
 * mad_flex_fit (-1 before the first).  Any pointer may be NULL.  mad_set_option "flex_groups" (0: by the atom count; never more than
 * the compute units) and "flex_threads" (0: the default; a multiple of 64 up to 1024) are the tests' hooks.
 * Timing groups: "flex_network", "flex_steps".
 */
#define MAD_FLEX_MAX_DEGREE 128
int mad_flex_network(mad_ctx *ctx, int64_t n_atoms, const double *coords, double cutoff, int32_t *first, int64_t cap_springs,
                     int32_t *nbr, double *rest, int64_t *n_springs);
int mad_flex_fit(mad_ctx *ctx, int64_t n_atoms, const double *coords, const double *weights, const uint8_t *fixed, const int32_t *first,
                 const int32_t *nbr, const double *rest, double stiffness, int n_steps, double max_step, double min_step,
                 double *coords_out, int32_t *converged, int32_t *last_step, double *step, double *g0);
int mad_last_flex_plan(mad_ctx *ctx, int32_t *workgroups, int32_t *threads, int32_t *atoms_per_thread, int64_t *springs);

/*
 * A model's density with a Gaussian width per atom, and the B-factors of a placed model refined against a map (mad_bfactor.hip;
 * DESIGN.md section 4zb, restated in mad_amd/bfactor.py).  Host pointers, synchronous, nothing modified.
 *
 * The contract: K = 8 pi^2, v0 = (resolution / (pi sqrt 2))^2, an atom of B-factor B has the variance v = v0 + B / K.  Voxel j sits at
 * origin + voxsp j, d2 = (dx dx + dy dy) + dz dz in float64 without fused multiply-add.  The atom reaches the voxel iff d2 <= 9 v and
 * adds e = (m / ((2 pi v) sqrt(2 pi v))) exp(-(d2 / (2 v))) to it.  The box is the union, over the atoms that reach the lattice, of
 * floor((x - rmax - o) / voxsp) .. ceil((x + rmax - o) / voxsp) per axis, rmax = 3 sqrt(v0 + b_max / K), clipped to the lattice.
 *
 * mad_model_density_b: rho (float64 [x][y][z] of dims, zero outside the box) for n_atoms coordinates (n x 3 float64), masses and
 * B-factors b_atom (0 <= b <= b_max).  A voxel's sum runs over the cells of a grid over the atoms in ascending order, atoms ascending
 * within a cell, in float64: the same bits whatever "bf_chunk" and "bf_threads" are.  box (nullable) receives lo[3], dim[3].
 *
 * mad_bfactor_refine: the atoms come sorted by group, group g = first_atom[g] .. first_atom[g + 1] - 1 (first_atom[0] = 0,
 * first_atom[n_groups] = n_atoms, a group may be empty), one B per group starting from b0 (within [b_min, b_max]); fixed (n_groups
 * bytes, NULL: none) keeps a group's B.  A cycle: rho at the present B, s = <D, rho> / <rho, rho> over the box in fourier.tree_sum's
 * pairing (D the map), r = s rho - D, g_a = (s sum_p (r e_a)(d2 / (2 v v) - 1.5 / v)) / K, a group's gradient the sum of its atoms'
 * in ascending order, mx the largest |g| of the free groups (0: converged), B <- clip(B - step (g / mx), b_min, b_max).  Every
 * fourth cycle the step halves when no B moved as far as one step since the last look; a step below min_step is convergence; a NaN
 * ends the run with *converged = 0.  All cycles are queued at once and a flag on the device empties those after the end.
 * b_out: n_groups.  stats[7]: the scale s, the loss <r, r> at b0 and at the end, the un-centred correlation at b0 and at the end, the
 * final step, the scale at b0.  *last_cycle: the cycle that ended the run.  rho (nullable): as mad_model_density_b, at the final B,
 * not scaled.
 * MAD_EINVAL: NULL, resolution <= 0, a coordinate or mass that is not finite, b0 outside [b_min, b_max], a group table that does not
 * cover the atoms, n_cycles < 1, not 0 < min_step <= max_step.  MAD_EDOM: no atom reaches the lattice, or <rho, rho> == 0.
 *
 * mad_last_bfactor_plan: the box (lo[3], dim[3]), the bricks and the cells per axis, the atoms per LDS chunk, the threads of a gather
 * workgroup, the cycles queued (0 for mad_model_density_b) and the atoms that reach the lattice, of the most recent call of either
 * (-1 before the first).  Any pointer may be NULL.  mad_set_option "bf_chunk" (0, or 64 .. 1024) and "bf_threads" (0, or a multiple of
 * 64 up to 512) are the tests' hooks.  Timing groups: "bf_gather", "bf_sums", "bf_grad", "bf_step".
 */
int mad_model_density_b(mad_ctx *ctx, const int32_t dims[3], const double origin[3], double voxsp, int64_t n_atoms, const double *coords,
                        const double *masses, const double *b_atom, double resolution, double b_max, double *rho, int32_t box[6]);
int mad_bfactor_refine(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, int64_t n_atoms,
                       const double *coords, const double *masses, int64_t n_groups, const int64_t *first_atom, const double *b0,
                       const uint8_t *fixed, double resolution, double b_min, double b_max, int n_cycles, double max_step, double min_step,
                       double *b_out, double *stats, int32_t *converged, int32_t *last_cycle, double *rho);
int mad_last_bfactor_plan(mad_ctx *ctx, int32_t box[6], int32_t bricks[3], int32_t cells[3], int32_t *chunk, int32_t *threads, int32_t *cycles,
                          int64_t *kept);

/*
 * A map cut around a structure, or with the structure erased (mad_zone.hip).  Host pointers, synchronous.
 * grid: float32 [x][y][z] with dims, origin (Angstrom, centre of voxel (0,0,0)) and spacing voxsp, updated IN PLACE; atoms:
 * n_atoms x 3 float64 (Angstrom), read only, NULL allowed when n_atoms == 0.  Voxel j sits at p_a = origin_a + voxsp * j_a
 * (float64, one multiply and one add, no FMA); its squared distance to an atom is d2 = (dx*dx + dy*dy) + dz*dz with
 * dx = p_x - a_x, and D2 is the minimum of d2 over all atoms.  With r2 = radius * radius, R = radius + soft, R2 = R * R the weight
 * is w = 1 where D2 <= r2, w = 0 where D2 >= R2 or n_atoms == 0, and w = 0.5 + 0.5 * cos(pi * ((sqrt(D2) - radius) / soft)) in
 * between (float64); erase != 0 takes 1 - w.  A voxel of final weight exactly 1 is not written (every bit stays), one of final
 * weight exactly 0 becomes +0.0f whatever it held, any other becomes (float)((double)g * w).  counts (may be NULL): counts[0] =
 * voxels with D2 <= r2, counts[1] = voxels with r2 < D2 < R2.  The same call gives the same bits alone or after any other call.
 * MAD_EINVAL, with nothing launched and the grid untouched: NULL (atoms only when n_atoms == 0), a dimension < 1, voxsp <= 0,
 * 2^32 voxels or more, n_atoms < 0 (or 2^31 and more), radius < 0, soft < 0, radius + soft == 0, a number that is not finite
 * (atom coordinates included; also a box that, grown by radius + soft, leaves float64).
 */
int mad_map_zone(mad_ctx *ctx, float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                 const double *atoms, int64_t n_atoms, double radius, double soft, int erase,
                 int64_t counts[2] /* may be NULL */);

/*
 * A soft mask made from the map itself: threshold, grow, raised-cosine edge (mad_envelope.hip; DESIGN.md section 4r;
 * mad_amd/envelope.py::envelope_numpy restates the contract).  Host pointers, synchronous; grid (float32 [x][y][z]) is read only.
 *   Seeds.  A voxel is a seed where (double)g > threshold.
 *   Distance.  d2(v) is the squared Euclidean distance in whole voxels from v to the nearest seed, exact wherever it is at most Rv^2
 *   with Rv = min(floor((extend + soft) / voxsp) + 1, max(dims) - 1); anything farther, and everything when there is no seed, is the
 *   sentinel INT32_MAX.  (Where max(dims) - 1 is the smaller term, voxels farther than that from every seed hold the sentinel although
 *   extend + soft would reach them.)
 *   Weight.  mad_map_zone's expressions with D2 = (double)d2 * (voxsp * voxsp), r2 = extend * extend, R = extend + soft, R2 = R * R:
 *   w = 1 where D2 <= r2, w = 0 where D2 >= R2 or d2 is the sentinel, else w = 0.5 + 0.5 * cos(pi * ((sqrt(D2) - extend) / soft)), in
 *   float64, stored as float32.  extend = soft = 0 is legal: the mask is the seed set.
 * mask_out: float32 [x][y][z], every voxel written.  d2_out (may be NULL): int32 [x][y][z].  counts (may be NULL): [0] seeds, [1]
 * voxels with D2 <= r2 (seeds included), [2] voxels with r2 < D2 < R2 -- by the branch taken, as mad_map_zone counts, so they do not
 * depend on how cos rounds.  The same call gives the same bits alone or after any other call.
 * MAD_EINVAL, nothing launched: NULL, a dimension < 1, 2^31 voxels or more, voxsp not positive and finite, a NaN threshold, extend or
 * soft negative or not finite.  MAD_EDOM, outputs untouched: Rv > 255 (the figure is in the message); a voxel that is not finite.
 */
int mad_map_envelope(mad_ctx *ctx, const float *grid, const int32_t dims[3], double voxsp,
                     double threshold, double extend, double soft,
                     float *mask_out, int32_t *d2_out /* may be NULL */, int64_t counts[3] /* may be NULL */);

/*
 * A placed model scored per group of atoms -- residue, chain, any partition -- against a map (mad_groupfit.hip; DESIGN.md section
 * 4k).  Host pointers, synchronous, nothing modified but the two outputs.  grid1 (the map) and grid2 (the model's density): float32
 * [x][y][z] with their dims and origins (Angstrom, centre of voxel (0,0,0)) and the common spacing voxsp.  Group g owns the atoms
 * first_atom[g] .. first_atom[g + 1] - 1 of atoms (n x 3 float64, Angstrom; the layout of mad_overlap_matrix), n_atoms =
 * first_atom[n_groups]; atoms may be NULL when n_atoms == 0.
 *   Membership: mad_map_zone's expressions on grid 1's lattice.  Voxel j sits at p_a = origin1_a + voxsp * j_a (float64, one
 *     multiply and one add, no FMA), d2 = (dx*dx + dy*dy) + dz*dz with dx = p_x - a_x, and j is a member of group g iff some atom
 *     of g has d2 <= radius * radius (inclusive).  Groups may overlap: a voxel counts in every group that reaches it.
 *   Values: a = g1[j] < (float)isovalue ? 0.0 : (double)g1[j] (a float32 compare).  With s_a = round-half-even(origin2_a / voxsp -
 *     origin1_a / voxsp) and k = j - s: b = 0.0 where k lies outside grid 2, else the same expression on g2[k].  The sums are not
 *     restricted to the common box of the two grids.
 *   Outputs: n_vox[g] = the members of g (exact); sums[5 g ..] = {sum a*a, sum b*b, sum a*b, sum a, sum b} over them, float64 (every
 *     term is exact; the order of the additions is fixed).  An empty group, or one that reaches no voxel, has
 *     n_vox = 0 and five zero sums.  A voxel that is not finite is no error: it propagates as IEEE says.  The same call gives the
 *     same bits alone or after any other call.  n_groups == 0 returns MAD_OK and writes nothing.
 * MAD_EINVAL, with nothing launched and the outputs untouched: NULL (atoms only when n_atoms == 0), a dimension < 1, voxsp <= 0,
 * 2^32 voxels or more in either grid, n_groups < 0, first_atom[0] != 0 or first_atom decreasing, n_atoms >= 2^31, radius < 0,
 * isovalue < 0, a number that is not finite (atom coordinates, origins and the offset between the grids in voxels included), a work
 * list of 2^31 bricks or more (one brick of 8 x 8 x 16 voxels per group and part of the group's reach).
 */
int mad_map_group_fit(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                      const float *grid2, const int32_t dims2[3], const double origin2[3], double voxsp,
                      const double *atoms, const int64_t *first_atom, int32_t n_groups, double radius, double isovalue,
                      int64_t *n_vox /* [n_groups] */, double *sums /* [n_groups][5] */);

/*
 * The Q-score of Pintilie et al. 2020 per atom of a placed model (mad_qscore.hip; DESIGN.md section 4u;
 * mad_amd/localfit.py::qscore_numpy restates the contract).  Host pointers, synchronous, nothing modified but the outputs.  grid:
 * float32 [x][y][z] with dims, origin and voxsp; atoms: n_atoms x 3 float64, the environment (every atom counts as "another atom");
 * index: the n_index atoms to score, or NULL to score all (then n_index is ignored); radii, ref: n_r shells, the radii strictly
 * ascending from a first >= 0, and the reference profile per shell; dirs: unit vectors (|d|^2 <= 1 + 2^-20), the sets t = 1 ..
 * n_tries one after the other, set t with 8 t of them: 4 n_tries (n_tries + 1) x 3 float64.  All arithmetic is float64 without
 * fused multiply-adds.
 *   Points of a shell R > 0: a candidate is p_a = x_a + R * dir_a; it is kept iff every other atom b (other by index) has
 *     D2 = (dx*dx + dy*dy) + dz*dz > R * R with dx = p_x - b_x.  The sets are tried in order; the first with 8 kept candidates or
 *     more gives the shell its points, the first 8 kept in table order; if none does, the shell takes the kept candidates of the
 *     last set (0 .. 7).  A shell with R = 0 is 8 copies of the sample at the atom's centre.
 *   Sampling: f_a = (p_a - origin_a) / voxsp; a point with any f_a outside [-1, n_a] is 0; else i_a = floor(f_a), t_a = f_a - i_a, the
 *     eight corners (0 outside the grid) blended along z, then y, then x as c0 + t * (c1 - c0).
 *   Score: over the slots [shell][point] (a slot without a point adds 0 to every sum): lane l = 0 .. 63 adds the slots l, l + 64, ...
 *     in this order, then the 64 partial sums are folded as s_l += s_(l xor 32), then xor 16, 8, 4, 2, 1.  So the sums of the
 *     samples u and of their shells' ref values v, the means (divided by the number n of points), and, the same way, the sums of du
 *     dv, du du and dv dv; q = S_uv / (sqrt(S_uu) * sqrt(S_vv)), NaN when n < 2 or either sum of squares is 0.
 * Outputs per scored atom, in the order of index: q float64, n_samples int32, and where the pointer is not NULL tries_used int32
 * [n_r] (the set that gave the shell its points, 0 for R = 0), picked int32 [n_r][8] (the row of dirs, -1 for no point and in a shell
 * with R = 0), values float64 [n_r][8] (0 for no point).  The same call gives the same bits alone or after any other call.
 * n_atoms == 0, or nothing to score, returns MAD_OK and writes nothing.
 * MAD_EINVAL, with nothing launched and the outputs untouched: NULL (atoms only when n_atoms == 0; index and the last three
 * outputs may be), a dimension < 1, 2^32 voxels or more, voxsp <= 0, a number that is not finite (origin, spacing, coordinates,
 * radii, ref, dirs), radii that do not ascend or a negative one, n_r outside 1 .. 64, n_tries outside 1 .. 64, a direction longer
 * than a unit vector, an index outside [0, n_atoms), 2^31 atoms or indices or more.
 */
int mad_map_qscore(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                   const double *atoms, int64_t n_atoms, const int64_t *index /* may be NULL */, int64_t n_index,
                   const double *radii, const double *ref, int32_t n_r, const double *dirs, int32_t n_tries,
                   double *q, int32_t *n_samples, int32_t *tries_used /* may be NULL */, int32_t *picked /* may be NULL */,
                   double *values /* may be NULL */);

/*
 * A Gaussian on a map, and a map cut into segments (mad_segment.hip).  Host pointers, synchronous.  Both work
 * in voxels: grid is float32 [x][y][z] with dims, the linear index of a voxel is L = (x * ny + y) * nz + z, neither origin nor
 * spacing enters.
 *
 * mad_map_smooth: out = grid smoothed with a Gaussian of sigma_vox voxels; out may be grid.  R = (int)(4 sigma + 0.5); the taps are
 * w_k = exp(-0.5 * k * k / (sigma * sigma)), k = 0 .. R, float64 with libm's exp on the host, divided by w_0 + 2 * (w_1 + w_2 + ...)
 * (that sum accumulated for k = 1, 2, ... in this order).  Three passes, over axis 0, then 1, then 2, float64 in between; an output
 * of a pass is a = c * w_0, then for k = R, R - 1, ..., 1: a += (in[-k] + in[+k]) * w_k, products and sums rounded separately (no
 * FMA), a tap outside the grid being 0.0 (zero extension: scipy.ndimage.gaussian_filter(mode="constant", truncate=4.0)).  The last
 * pass rounds to float32.  A voxel that is not finite is no error here: it propagates as IEEE says.
 * MAD_EINVAL, with nothing launched and out untouched: NULL, a dimension < 1, 2^31 voxels or more, sigma_vox <= 0 or not finite
 * (or 2^18 voxels and more).
 *
 * mad_map_segment: a watershed of the density, whose regions are then grouped by following their maxima through smoothed copies of
 * the map.
 *   Order.  Voxel a is above voxel b iff v_a > v_b, or v_a == v_b and L_a < L_b (IEEE compares: -0.0 == +0.0).  A strict total order.
 *   Watershed.  A voxel is foreground iff (double)v > threshold (strict; threshold = -inf is allowed).  The parent of a foreground
 *     voxel is the greatest, in the order, among itself and its foreground neighbours (up to 26, those inside the grid).  A root is
 *     its own parent; a foreground voxel belongs to the root its chain of parents ends in.  The regions are numbered 1 .. n by
 *     ascending L of their roots; a background voxel has label 0.
 *   Grouping.  point_r starts as the root of region r.  For s = 1 .. steps: S_s = the map smoothed as by mad_map_smooth with sigma =
 *     s * step voxels (always from the original grid; the same bits), the parents of S_s are taken with every voxel foreground, and
 *     point_r becomes the root of point_r in S_s.  Regions with equal points are one group (equal points stay equal: groups only
 *     merge).  history[s] = the number of groups after step s, history[0] = n.  The steps stop after the first one with
 *     history[s] <= stop_at (stop_at = 0: never early).  The groups are numbered 1 .. m by ascending smallest member region.
 * Outputs: labels int32 [x][y][z], the group of every voxel (0: background; with steps = 0 the region); per region r (0-based,
 * region r + 1) root[r] int64 = L of its root, peak[r] float32 = the value there (the region's maximum), size[r] int64 = its voxels,
 * group[r] int32 = its group -- each of the four may be NULL --; history int64 [steps + 1], of which [0 .. *steps_done] are
 * written; *steps_done = smoothing steps run (0 when n = 0); *n_regions = n.  cap = entries each region table holds: with n > cap
 * the call returns MAD_ENOSPC with *n_regions = n (the capacity needed), the tables untouched, and labels, history and *steps_done
 * as valid as otherwise.  The same call gives the same bits alone or after any other call.
 * MAD_EDOM, nothing written: a voxel that is not finite (found by the first pass over the map on the device).
 * MAD_EINVAL, nothing launched or written: NULL (other than a table), a dimension < 1, 2^31 voxels or more, a NaN threshold,
 * steps < 0, step <= 0 or not finite, stop_at < 0, cap < 0, steps * step of 2^18 voxels and more.
 */
int mad_map_smooth(mad_ctx *ctx, const float *grid, const int32_t dims[3], double sigma_vox, float *out);
int mad_map_segment(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t steps, double step,
                    int64_t stop_at, int32_t *labels, int64_t *root, float *peak, int64_t *size, int32_t *group, int64_t cap,
                    int64_t *n_regions, int64_t *history, int32_t *steps_done);

/*
 * The connected components of a map above a threshold, and the map with its small components ("dust") replaced by a fill value
 * (mad_components.hip; mad_amd/components.py::components_numpy / dust_numpy restate the contract).  Host
 * pointers, synchronous.  Both work in voxels: grid is float32 [x][y][z] with dims, read only, the linear index of a voxel is
 * L = (x * ny + y) * nz + z as in mad_map_segment, neither origin nor spacing enters.
 *   Foreground.  A voxel is foreground iff (double)v > threshold (strict, as mad_map_segment and mad_map_envelope; threshold = -inf is
 *     allowed: every voxel).
 *   Neighbours.  connectivity 6, 18 or 26: the offsets in {-1, 0, 1}^3 with 1, at most 2, or at most 3 components that are not 0.  Only
 *     neighbours inside the grid count: no wrap-around.
 *   Components.  A component is a class of the transitive closure of "foreground voxels that are neighbours".  Its root is its member
 *     with the smallest L.  The components are numbered 1 .. n by ascending root; a background voxel has label 0.
 * mad_map_components writes labels (int32 [x][y][z]), per component c (0-based, component c + 1) root[c] int64 = L of its root and
 * size[c] int64 = its voxels -- either table may be NULL --, and *n_components = n.  cap = entries each table holds: with n > cap the
 * call returns MAD_ENOSPC with *n_components = n (the capacity needed), the tables untouched and labels as valid as otherwise.
 * mad_map_dust ranks the components by size descending, root ascending (a strict order); a component is kept iff size >= min_size and
 * (keep == 0 or its rank, from 0, is < keep).  out (float32 [x][y][z]; may be grid): a background voxel keeps its bits, a voxel of a
 * kept component keeps its bits, a foreground voxel of a component that is not kept becomes fill.  counts (may be NULL) = {components,
 * kept components, foreground voxels, kept voxels}.
 * The same call gives the same bits alone or after any other call (labels by comparisons and integer atomics whose order cannot
 * show; ids by a scan; sizes are integer sums).
 * MAD_EINVAL, nothing launched or written: NULL (other than a table or counts), a dimension < 1, 2^31 voxels or more, a NaN threshold,
 * a connectivity other than 6, 18 or 26, cap < 0, min_size < 1, keep < 0, fill not finite or (double)fill > threshold (a fill above
 * the threshold would turn dust back into foreground).
 * MAD_EDOM, nothing written: a voxel that is not finite (found by the first pass over the map on the device).
 */
int mad_map_components(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t connectivity,
                       int32_t *labels, int64_t *root /* may be NULL */, int64_t *size /* may be NULL */,
                       int64_t cap, int64_t *n_components);
int mad_map_dust(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t connectivity,
                 int64_t min_size, int64_t keep, float fill, float *out /* may be grid */, int64_t counts[4] /* may be NULL */);

/*
 * A map's voxels sorted, its order statistics, and its confidence map: thresholds that control the false discovery rate (Beckers,
 * Jakobi and Sachse, IUCrJ 2019) (mad_confidence.hip; mad_amd/confidence.py::sort_numpy / kth_numpy /
 * confidence_numpy restate the contract).  Host pointers, synchronous, lane 0; grid is float32, read only; neither origin nor spacing
 * enters.
 *   Order.  The n values descending.  -0.0 counts as, and comes back as, +0.0: the output is a function of the values alone.  (A radix
 *     sort of the keys only, 8 bits x 4 passes, stable; integer work throughout.)
 * mad_map_sort writes out_desc[0 .. n) = the values in that order.  mad_map_kth writes out[i] = the k[i]-th largest value, 1-based:
 * out_desc[k[i] - 1].
 * mad_map_confidence, with N = the voxels of dims and s[0 .. N) = the values in that order:
 *   Noise.  boxes[b] = {x, y, z, edge}: the cube of edge^3 voxels whose corner of least indices is (x, y, z), inside the grid.  The
 *     samples are the voxels of box 0 in linear [x][y][z] order, then box 1, ... (a voxel in two boxes counts twice), n of them, as
 *     float64.  mean = tree_sum(samples) / n, var = tree_sum((samples - mean)^2) / (n - 1), sd = sqrt(var); tree_sum is the fixed
 *     pairing of mad_map_search (runs of 256 by halving, the partial sums the same way).  stats = {mean, var, n}.
 *   p and q.  In float64, without fused multiply-add: t = ((double)s[j] - mean) / sd, p[j] = 0.5 erfc(t / sqrt 2),
 *     r[j] = (p[j] (N c)) / (j + 1), q_sorted[j] = min(1, min over j' >= j of r[j']) -- the step-up rule of Benjamini and Hochberg
 *     with c = 1 and of Benjamini and Yekutieli with c = 1 + 1/2 + ... + 1/N, which the caller passes.  q_sorted ascends with j, and
 *     equal values have equal q.  Everything but erfc is correctly rounded arithmetic and minima: only the device's erfc can differ from
 *     another library's.
 *   Outputs.  out_q [x][y][z] (may be NULL) = q_sorted at a j with s[j] equal to the voxel; out_confidence [x][y][z] = (float)(1 - q);
 *     out_sorted (may be NULL) = s; out_q_sorted (may be NULL).  Per level l < n_levels: out_level_count[l] = the number of j with
 *     q_sorted[j] <= levels[l], out_level_value[l] = s[count - 1], the least density at which the rate is met, NaN where count is 0.
 * The same call gives the same bits alone or after any other call.
 * MAD_EINVAL, nothing launched or written: NULL (other than those named), n < 1 or a dimension < 1, 2^31 voxels or more, n_k < 1 or
 * above 2^20, a rank below 1 or above n, n_boxes < 1 or above 4096, a box with edge < 1 or not inside the grid, fewer than 2 or 2^31
 * and more samples, c not finite or below 1, n_levels < 0 or above 256, a level outside 0 .. 1.
 * MAD_EDOM, nothing written: a voxel that is not finite (counted by the first pass over the map on the device); for
 * mad_map_confidence also a variance of the samples that is not positive -- a map already masked to a constant has no noise in its
 * corners: the caller must name boxes that lie in the solvent.
 */
int mad_map_sort(mad_ctx *ctx, const float *grid, int64_t n, float *out_desc);
int mad_map_kth(mad_ctx *ctx, const float *grid, int64_t n, int64_t n_k, const int64_t *k, float *out);
int mad_map_confidence(mad_ctx *ctx, const float *grid, const int32_t dims[3], int32_t n_boxes, const int32_t *boxes, double c,
                       int32_t n_levels, const double *levels, float *out_confidence, double *out_q /* may be NULL */,
                       float *out_sorted /* may be NULL */, double *out_q_sorted /* may be NULL */, int64_t *out_level_count,
                       float *out_level_value, double stats[3] /* mean, var, n */);

/*
 * Fourier shell correlation of two maps, and the 3-D transform under it (mad_fourier.hip; restated with numpy
 * in mad_amd/fourier.py).  Host pointers, synchronous, nothing modified but the outputs.  grid1, grid2: float32 [x][y][z] with
 * their dims and origins (Angstrom, centre of voxel (0,0,0)) and the common spacing voxsp.
 *   Lattice.  Per axis d = origin2 / voxsp - origin1 / voxsp, s = round(d) (half to even, mad_map_mask's expression), delta = d - s
 *     in [-0.5, 0.5].  The lattice begins min(0, s) voxels from grid 1's origin: voxel (0,0,0) of grid 1 has lattice index -min(0, s),
 *     that of grid 2 s - min(0, s).  N is the smallest power of two >= the extent of the union box on every axis, 8 <= N <= 1024.
 *     The lattice is complex128 [N][N][N]: grid 1 in the real part, grid 2 in the imaginary part, zero elsewhere.
 *   Transform.  Z(k) = sum over the lattice of (g1 + i g2)(n) exp(-2 pi i k.n / N), unnormalised, float64 throughout (radix-4
 *     Stockham passes along z, y, x; twiddles from a host table; the same input gives the same bits every run).
 *   Shells.  F1(k) = (Z(k) + conj Z(-k)) / 2, F2(k) = (Z(k) - conj Z(-k)) / (2i), -k taken modulo N per axis.  Lattice index a stands
 *     for the frequency i = a (a < N / 2) or a - N; the shell of (i, j, k) is floor(sqrt(i*i + j*j + k*k) + 0.5); shells 0 .. N / 2
 *     are kept, the corners beyond are dropped.  Per shell: sums[3 s] = P1 = sum |F1|^2, sums[3 s + 1] = P2 = sum |F2|^2,
 *     sums[3 s + 2] = C = sum Re(F1 conj(F2 phi)), phi = (phi_x[a] phi_y[b]) phi_z[c], phi_x[a] = exp(-2 pi i (i delta_x) / N)
 *     (cos and sin of 2 pi (i delta_x) / N with the host's libm); count[s] = the lattice points of the shell.  The sums are added in
 *     a fixed order without floating-point atomics: the same call gives the same bits alone or after any other call.
 * mad_map_fsc writes *N_out (may be NULL), sums [(N / 2 + 1)][3] and count [N / 2 + 1]; cap_shells = the shells both hold: with
 * cap_shells < N / 2 + 1 the call returns MAD_ENOSPC with *N_out set and nothing else written.  It allocates the N^3 x 16 byte lattice
 * for the call and frees it.
 * mad_map_fft (a diagnostic, like mad_field_download) returns Z: spectrum = N^3 complex128, interleaved (re, im), [x][y][z].  grid2
 * may be NULL (dims2, origin2 are then ignored): grid 1 alone, N from its dims.  spectrum NULL: only *N_out is written (the size to
 * allocate), nothing is launched.
 * MAD_EINVAL: NULL, a dimension < 1, voxsp <= 0 or not finite, an origin that is not finite (or 1e15 voxels and more from 0), a grid
 * of 2^32 voxels or more.  MAD_EDOM: a union box longer than 1024 voxels on an axis.  MAD_ENOMEM: less free device memory than the
 * lattice, the grids and the tables need (judged before anything is allocated), or the allocation fails.  Each leaves the outputs
 * untouched (but *N_out with MAD_ENOSPC), launches nothing, and the next call works.
 */
int mad_map_fsc(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                const float *grid2, const int32_t dims2[3], const double origin2[3], double voxsp,
                int32_t *N_out, double *sums /* [N / 2 + 1][3]: P1, P2, C */, int64_t *count /* [N / 2 + 1] */, int64_t cap_shells);

/*
 * The Fourier shell correlation of two maps under a soft mask, with what it takes to correct the curve for the mask's own
 * contribution (Chen et al. 2013; mad_fourier.hip; restated with numpy as fourier.fsc_masked_numpy).  Host
 * pointers, synchronous, nothing modified but the outputs.  Lattice, placement, delta and phase ramp are mad_map_fsc's, from grid 1 and
 * grid 2 alone.  The mask (float32 [x][y][z] with dimsm, originm) is placed against grid 1 by whole voxels, its voxel j at lattice index
 * p1 + round(originm / voxsp - origin1 / voxsp) + j (half to even; no wrap-around); it multiplies both parts of the packed lattice at
 * the same lattice index, lattice points outside its box become 0.  What is left of its offset to either grid is rounded away: a soft
 * edge moves by at most half a voxel.
 *   1. Z = FFT(g1 + i g2); its shell sums are sums_unmasked (= mad_map_fsc's, bit for bit).
 *   2. shell_r >= 0 is taken as given.  shell_r < 0: the lowest shell s >= 1 whose unmasked C / sqrt(P1 P2) (0 where P1 P2 is not
 *      positive) is below t_r, N / 2 + 1 when there is none; found on the host.  *shell_r_out (may be NULL) receives it.
 *   3. k_fsc_randomize, in place on Z, one thread per lattice point L = (a N + b) N + c, acting where L < L', the index of -k; a
 *      self-conjugate point is never touched.  F1, F2 as above; where shell(k) >= shell_r (corners beyond N / 2 included) each becomes
 *      |F| (cos t + i sin t), |F| = sqrt(re*re + im*im), t = 6.283185307179586 * u, u = (z >> 11) * 2^-53, z = seed +
 *      0x9E3779B97F4A7C15 * (2 L + which + 1) (which: 0 for F1, 1 for F2) put through z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
 *      z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).  Z(k) = F1' + i F2', Z(-k) = conj(F1') + i conj(F2').
 *   4. The inverse transform (mad_map_ifft's passes); the mask times real and imaginary part, with the 1 / N^3; forward; the shell sums
 *      are sums_random.
 *   5. The lattice packed again, times the mask, forward; the shell sums are sums_masked.
 * Each table is [N / 2 + 1][3] = P1, P2, C, count [N / 2 + 1] as mad_map_fsc's (mad_map_fft's size query gives N beforehand).  No
 * floating-point atomics: the same call with the same seed gives the same bits.  MAD_EINVAL / MAD_EDOM / MAD_ENOMEM as mad_map_fsc, the
 * mask's dims and origin judged like a grid's; MAD_EINVAL also for shell_r < 0 with a NaN t_r.
 * mad_map_phase_randomize is step 3 alone on a spectrum the caller brings (complex128 [N][N][N] on the host, interleaved, N a power
 * of two in 8 .. 1024, updated IN PLACE), the sibling of mad_map_ifft: F1 is the spectrum itself, F2 is absent, Z(-k) = conj(F1').
 * MAD_EINVAL: NULL, such an N, shell_r < 0.
 */
int mad_map_fsc_masked(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                       const float *grid2, const int32_t dims2[3], const double origin2[3], double voxsp,
                       const float *mask, const int32_t dimsm[3], const double originm[3],
                       int32_t shell_r /* < 0: from t_r */, double t_r, uint64_t seed,
                       double *sums_unmasked, double *sums_masked, double *sums_random /* each [N / 2 + 1][3] */,
                       int64_t *count, int32_t *N_out, int32_t *shell_r_out);
int mad_map_phase_randomize(mad_ctx *ctx, double *spectrum, int32_t N, int32_t shell_r, uint64_t seed);
int mad_map_fft(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                const float *grid2 /* may be NULL */, const int32_t dims2[3], const double origin2[3], double voxsp,
                int32_t *N_out, double *spectrum /* N^3 complex128, interleaved; NULL: size query */);

/*
 * A radial filter on one or two maps in Fourier space, and the inverse transform under it (mad_fourier.hip; DESIGN.md section 4m;
 * restated with numpy in mad_amd/fourier.py::filter_numpy).  Host pointers, synchronous.
 *   Lattice.  grid1 and grid2 (float32 [x][y][z]) are each placed at lattice index (0, 0, 0): a radial filter is shift-invariant, the
 *     grids need no common frame.  N is the smallest power of two >= max(all dims) + pad, 8 <= N <= 1024; pad >= 0 is the zero margin
 *     between the far face of the box and its near face on the circular lattice.  Grid 1 in the real, grid 2 in the imaginary part.
 *   Spectrum.  Z = FFT(g1 + i g2), as mad_map_fft.
 *   Gain.  gain[r2], float64, r2 = i*i + j*j + k*k over the signed frequencies (a if a < N / 2, else a - N): n_gain = 3 (N / 2)^2 + 1
 *     entries, finite, negative values allowed.  It depends on r2 alone, so it is real and even, and the real and imaginary parts of
 *     the inverse are the filtered grid 1 and grid 2: one pair of transforms serves two maps.
 *   Inverse.  ifft(X) = conj(FFT(conj(X))) / N^3: Z(k) <- (Re Z g, -(Im Z g)), the same three forward passes, then
 *     out1 = (float)(Re Z 2^(-3 log2 N)) over grid 1's box and out2 = (float)(-(Im Z) 2^(-3 log2 N)) over grid 2's.  Float64 throughout,
 *     no fused multiply-add, no atomics: the same bits every run and after any other call.
 * mad_map_filter.  gain == NULL: the size query -- *N_out set, nothing allocated or launched.  grid2 / dims2 / out2 may be NULL
 * together.  out1 may be grid1 and out2 may be grid2 (host memory: the grids are uploaded before anything is written).
 * mad_map_ifft (a diagnostic, like mad_map_fft).  spectrum, out: complex128 [N][N][N] on the host, interleaved (re, im);
 * out = ifft(spectrum), normalised by 1 / N^3.  For testing the inverse alone.
 * MAD_EINVAL: NULL, a dimension < 1, a grid of 2^32 voxels or more, pad < 0, n_gain != 3 (N / 2)^2 + 1 (with *N_out set), a gain that
 * is not finite (its index is in the message), grid2 without out2 or out2 without grid2, mad_map_ifft with N not a power of two in
 * 8 .. 1024.  MAD_EDOM: max(dims) + pad > 1024.  MAD_ENOMEM: as mad_map_fsc (the lattice, both grids and the gain table are judged
 * before anything is allocated).  Each leaves the outputs untouched, launches nothing, and the next call works.
 */
int mad_map_filter(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const float *grid2 /* may be NULL */, const int32_t dims2[3],
                   int32_t pad, const double *gain /* NULL: size query */, int64_t n_gain, int32_t *N_out, float *out1, float *out2);
int mad_map_ifft(mad_ctx *ctx, const double *spectrum, int32_t N, double *out);

/*
 * A model scanned over every whole-voxel translation of a map by fast local correlation (Roseman's scheme; mad_fourier.hip; DESIGN.md
 * section 4n; restated with numpy in mad_amd/fourier.py::scan_numpy).  Host pointers, synchronous, lane 0; nothing is modified and no
 * state survives the call.
 *   Inputs.  map: float32 [x][y][z] of dims1.  templates: n_t >= 1 pointers to float32 grids, all of dims2, dims2[a] <= dims1[a].
 *     mode 0: the un-centred score (the library's convention everywhere else); mode 1: the centred one (Roseman's local correlation).
 *   Lattice.  N is the smallest power of two >= max(dims1), 8 <= N <= 1024; map and template each sit at lattice index (0, 0, 0).
 *   Offsets.  u in [0, D[a]) per axis, D = dims1 - dims2 + 1: the template's box lies wholly inside the map's, no scored offset wraps
 *     around the circular lattice.  best and best_t are [D[0]][D[1]][D[2]].
 *   Per template, with w(x) = 1 where g(x) > iso else 0, g^ = g w, n_w = sum w, G = sum g^2, gbar = sum g^ / n_w (float64, in voxel
 *     order): C(u) = sum_x m(u + x) g^(x), E(u) = sum_x m(u + x)^2 w(x), mode 1 also A(u) = sum_x m(u + x) w(x).
 *     mode 0: score = C / sqrt(E G) where E > e_min.  mode 1: C' = C - A gbar, E' = E - A^2 / n_w, G' = G - n_w gbar^2,
 *     score = C' / sqrt(E' G') where E' > e_min.  Elsewhere the offset is not scored: in empty regions E is round-off.
 *   Across templates.  best(u) = the greatest float32 score of the templates that scored u, best_t(u) = the lowest template index
 *     that attains it; 0.0 and -1 where none scored.
 *   Peaks.  u is a peak when best_t(u) >= 0, best(u) >= min_score and every one of its 26 neighbours v inside the offset box has
 *     best(v) < best(u), or best(v) == best(u) and a larger linear index.  Sorted by score descending, then linear index ascending;
 *     the first k go to peaks[p] = (ux, uy, uz, score, template), *n_peaks = how many were written, *n_found = how many there are.
 *   Spectra.  One transform of m + i m^2 serves all templates; per template one of g^ + i w, the product
 *     M conj(G^) + i M2 conj(W) in place, and one inverse by the same line passes whose real part is C and imaginary part E; mode 1
 *     adds M conj(W) on a third lattice and a second inverse for A.  Float64, no fused multiply-add, no floating-point atomics: two
 *     calls return the same bits.
 * best == NULL with N_out: the size query -- *N_out set, nothing allocated or launched (map and templates are not read).
 * peaks may be NULL with k = 0.  N_out may be NULL otherwise.
 * MAD_EINVAL: NULL (a template's pointer included), n_t < 1, a dimension < 1, iso, e_min or min_score not finite, e_min < 0, k < 0, a
 * mode other than 0 or 1, a template with no voxel above iso, in mode 1 a template that is constant under its mask (G' <= 0) -- the
 * template's index is in the message.  MAD_EDOM: max(dims1) > 1024, or dims2[a] > dims1[a].  MAD_ENOMEM: as mad_map_fsc (two
 * lattices, in mode 1 three, both grids and the outputs are judged before anything is allocated).  Each leaves the outputs
 * untouched, launches nothing, and the next call works.
 */
int mad_map_scan(mad_ctx *ctx, const float *map, const int32_t dims1[3], int32_t n_t, const float *const *templates, const int32_t dims2[3],
                 double iso, double e_min, int32_t mode, double min_score, int64_t k, float *best, int32_t *best_t,
                 double *peaks /* [k][5]: ux, uy, uz, score, template; may be NULL with k = 0 */, int64_t *n_peaks, int64_t *n_found,
                 int32_t *N_out);

/*
 * A model searched over rotations and every whole-voxel translation of a map: mad_map_scan's scores with the templates made on the
 * device, one per rotation of ONE base template (mad_fourier.hip; restated with numpy in
 * mad_amd/fourier.py::search_numpy, rotate_numpy and tree_sum).  Host pointers, synchronous, lane 0; nothing is modified and no state
 * survives the call.  Between the first rotation and the last nothing comes back to the host.
 *   Inputs.  map: float32 [x][y][z] of dims1.  base: float32 of dims0 (any shape).  c0: the centre of rotation in base's voxel
 *     coordinates (may be fractional).  edge e >= 1, e <= dims1[a]: the rotated template is a cube of e^3 voxels.  rotations: n_r >= 1
 *     row-major 3 x 3 matrices R_j (the library moves points by y = (x - c) @ R + c).
 *   Rotated template.  c2 = (e - 1) / 2; for the cube's voxel x, d = x - c2 and p_a = c0_a + ((d_0 R[a][0] + d_1 R[a][1]) + d_2 R[a][2]);
 *     f = floor(p), t = p - f; the eight corners f, f + 1 are read from base, a corner outside it is 0 (so a p at or beyond -1 or
 *     dims0[a] gives 0); lerp(a, b, t) = a + t (b - a) along z, then y, then x; float64 in exactly this order without fused
 *     multiply-add; the result rounded to float32 is the template voxel g_j(x).
 *   Mask and sums.  w = [g_j > iso] (compared in float64), n_w = sum w, G = tree_sum(g^2 w), S = tree_sum(g w) over the cube in linear
 *     [x][y][z] order.  tree_sum: runs of 256 consecutive elements (the last zero-padded) are each summed by halving -- x[0:128] +
 *     x[128:256], then 64, ... 1 --, and the partial sums the same way until one value is left.  mode 1: gbar = S / n_w,
 *     G' = G - n_w (gbar gbar).
 *   Skipped rotations.  A rotation with n_w = 0, G not in (0, 1.7e308] or, in mode 1, G' <= 0 scores no offset; *n_skipped counts
 *     them.  That is not an error (the sums exist only on the device): with every rotation skipped best is 0.0, best_r -1, *n_found 0.
 *   Scores, best, best_r and peaks: as mad_map_scan over D = dims1 - e + 1 with the floor e_min_j = e_fill n_w_j (one float64
 *     product); peaks[p] = (ux, uy, uz, score, rotation).
 *   Line passes.  With the option "search_prune" (default 1) the forward passes skip the lines and elements that are zero (the
 *     template fills e^3 of N^3) and the inverse passes the lines no scored offset reads; 0 runs full passes: the same numbers.
 * best == NULL with N_out: the size query -- *N_out set, nothing allocated or launched.  peaks may be NULL with k = 0.
 * MAD_EINVAL: NULL, n_r < 1, edge < 1, a dimension < 1, c0, iso, e_fill or min_score not finite, e_fill < 0, k < 0, a mode other than
 * 0 or 1, a rotation with an entry that is not finite or with max |R R^T - I| > 1e-6 (its index is in the message).  MAD_EDOM:
 * max(dims1) > 1024, or edge > dims1[a].  MAD_ENOMEM: as mad_map_scan.  Each is decided before anything is allocated or launched,
 * leaves the outputs untouched, and the next call works.
 */
int mad_map_search(mad_ctx *ctx, const float *map, const int32_t dims1[3], const float *base, const int32_t dims0[3], const double c0[3],
                   int32_t edge, const double *rotations /* [n_r][9] */, int32_t n_r, double iso, double e_fill, int32_t mode, double min_score,
                   int64_t k, float *best, int32_t *best_r, double *peaks /* [k][5]: ux, uy, uz, score, rotation; may be NULL with k = 0 */,
                   int64_t *n_peaks, int64_t *n_found, int32_t *n_skipped, int32_t *N_out);

/* One rotated template of mad_map_search and its sums, for testing them alone: out float32 [edge^3] = g_j(x) (before the mask),
 * stats = (n_w, G, S).  MAD_EINVAL as above; MAD_EDOM: edge > 1024. */
int mad_map_rotate(mad_ctx *ctx, const float *base, const int32_t dims0[3], const double c0[3], int32_t edge, const double R[9], double iso,
                   float *out /* float32 [e^3] */, double stats[3] /* n_w, G, S */);

/*
 * Local resolution of a map by windowed Fourier shell correlation.  DESIGN.md section 4p has the contract; mad_amd/fourier.py restates
 * it as local_fsc_numpy.  No reference counterpart.
 *   Placement.  As mad_map_fsc: per axis d = o2 / voxsp - o1 / voxsp, s = round(d) (half to even), delta = d - s; grid 2's voxel j
 *     sits at grid 1's index j + s, delta goes into the phase ramp with N = box.  The dims need not be equal; a voxel outside either
 *     grid is 0 for that grid.
 *   Samples.  n_a = (dims1[a] - 1) / step + 1 points per axis at grid-1 voxel p_a = step m_a; the outputs are volumes [n_x][n_y][n_z]
 *     with grid 1's origin and spacing step voxsp.  select (uint8 over that lattice, NULL: every sample): a sample whose byte is 0 gets
 *     resolution 0.0, shell -1 and zero sums, and nothing is computed for it.
 *   Box.  Box index n in 0 .. box - 1 stands for voxel p - box / 2 + n on every axis.  Both grids are multiplied by the periodic Hann
 *     window (h[nx] h[ny]) h[nz], h[n] = 0.5 - 0.5 cos(2 pi n / box) (the cosine of an exactly reduced angle): it peaks at the sample.
 *   Sums.  Z = FFT(w1 + i w2), forward, unnormalised; F1, F2, the shells 0 .. box / 2 and P1, P2, C as mad_map_fsc with N = box.
 *   Crossing.  fsc_s = C_s / sqrt(P1_s P2_s), 0 where P1_s P2_s is not > 0; the first shell s >= 1 with fsc_s < threshold; with
 *     a = fsc_(s-1), b = fsc_s, freq_s = s / (box voxsp): f = freq_(s-1) + (freq_s - freq_(s-1)) ((a - threshold) / (a - b)) when
 *     a >= threshold, else f = freq_s; resolution = 1 / f, shell = s.  No such shell: resolution = 2 voxsp, shell = 0.
 *   float64, no fused multiply-add, no atomics, every sum in an order fixed by indices: the same bits every run and after any other call.
 * resolution == NULL: the size query -- the checks and n_out only, nothing allocated or launched.  Otherwise resolution and shell hold
 * n_x n_y n_z entries, sums (may be NULL) n_x n_y n_z (box / 2 + 1) 3.
 * MAD_EINVAL: NULL (other than select, sums, and resolution with shell), a box other than 8, 16 or 32, step < 1, a threshold outside
 * (-1, 1) or not finite, voxsp <= 0 or not finite, a dimension < 1, a grid of 2^32 voxels or more, an origin that is not finite.
 * MAD_EDOM: origins 1e15 voxels or more apart, 2^31 selected samples or more.  MAD_ENOMEM: less device memory free than the grids, the
 * outputs and (box 32) the 32 MiB scratch buffer need, judged before anything is allocated.  Each leaves the outputs untouched,
 * launches nothing, and the next call works.
 */
int mad_map_local_fsc(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                      const float *grid2, const int32_t dims2[3], const double origin2[3], double voxsp,
                      int32_t box, int32_t step, double threshold, const uint8_t *select /* may be NULL: every sample */,
                      double *resolution /* [nx][ny][nz]; NULL: size query */, int32_t *shell /* same */,
                      double *sums /* may be NULL; [nx][ny][nz][box / 2 + 1][3] = P1, P2, C */, int32_t n_out[3]);

/*
 * A map's amplitudes scaled to a reference, box by box: every sample gets the value, at its own voxel, of its box of grid 1 after
 * each shell of that box's spectrum has been given the power the same box of grid 2 holds there; grid 1 keeps its phases (the local
 * amplitude scaling of Jakobi, Wilmanns and Sachse 2017).  DESIGN.md section 4v has the contract; mad_amd/fourier.py restates it as
 * local_scale_numpy.  No reference counterpart.
 *   Placement, samples, select, box and window.  As mad_map_local_fsc, whose front end this call shares: s = round(d) places grid 2 by
 *     whole voxels; the rest delta is NOT used -- amplitudes do not see a phase ramp.  Box index box / 2 on every axis is the sample's
 *     own voxel, and the window is exactly 1 there.
 *   Sums.  Z = FFT(w1 + i w2), F1 and F2 as mad_map_fsc with N = box.  Shells sh = min(shell index, box / 2): the corner points
 *     beyond shell box / 2 ride with shell box / 2 (unlike mad_map_local_fsc, which drops them), so that a map scaled against itself
 *     comes back unchanged.  P1_s = sum |F1|^2, P2_s = sum |F2|^2, D_s = sum Re F1(k) (-1)^(a + b + c) over the points (a, b, c) of
 *     shell s.
 *   Gain and value.  gain_s = sqrt(P2_s / P1_s) where P1_s > 0 and the quotient is finite, else 0.0.
 *     out = (gain_0 D_0 + ... + gain_(box/2) D_(box/2)) / box^3, added in shell order: the real part of the inverse transform of
 *     gain[sh] F1 at the centre of the box.
 *   float64, no fused multiply-add, no atomics, every sum in an order fixed by indices: the same bits every run and after any other call.
 * out == NULL: the size query -- the checks and n_out only, nothing allocated or launched.  Otherwise out holds n_x n_y n_z entries
 * (0.0 where select is 0) and gains (may be NULL) n_x n_y n_z (box / 2 + 1) (zeros where select is 0).  The values do not depend on
 * whether gains was asked for.
 * MAD_EINVAL, MAD_EDOM, MAD_ENOMEM: those of mad_map_local_fsc, without the threshold's.  Each leaves the outputs untouched, launches
 * nothing, and the next call works.
 */
int mad_map_local_scale(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3],
                        const float *grid2, const int32_t dims2[3], const double origin2[3], double voxsp,
                        int32_t box, int32_t step, const uint8_t *select /* may be NULL: every sample */,
                        double *out /* float64 [nx][ny][nz]; NULL: size query */,
                        double *gains /* may be NULL; float64 [nx][ny][nz][box / 2 + 1] */, int32_t n_out[3]);

/*
 * A low-pass whose width varies from voxel to voxel: every output voxel is the map under the Gaussian of its own resolution
 * (mad_localfilter.hip).  DESIGN.md section 4q has the contract; mad_amd/fourier.py restates it as local_sigma_numpy and
 * local_filter_numpy.  No reference counterpart.  grid float32 [nx][ny][nz]; res float64 (Angstrom) on the sample lattice of step
 * s >= 1, rdims m_a = (n_a - 1) / s + 1 (the lattice mad_map_local_fsc writes; s = 1: a full-size field).
 *   Resolution at voxel (i, j, k).  Per axis j0 = min(i / s, m - 1), j1 = min(j0 + 1, m - 1), f = (i - j0 * s) / s as a float64
 *     division, 0.0 where j1 == j0 (beyond the last sample the field is clamped, not extrapolated).  Trilinear with
 *     lerp(a, b, f) = a + (b - a) * f along z first, then y, then x.  sigma = d / (voxsp * K) voxels, K = pi * sqrt(2) formed once on
 *     the host in float64.  These IEEE operations in this order, none fused: sigma is the same bits on the device and in numpy.
 *   Taps.  R = max(1, (int)(4 sigma + 0.5)) (mad_map_smooth's truncation), q = -0.5 / (sigma * sigma), w_k = exp(q * (k * k)) for
 *     k = 0 .. R, W = w_0 + 2 * (w_R + ... + w_1), summed from R down to 1.
 *   Output.  out = S / (W * W * W), S = sum_dx w_|dx| * (sum_dy w_|dy| * (sum_dz w_|dz| * g[i + dx, j + dy, k + dz])), each offset
 *     from -R to R, a voxel outside the grid being 0.0.  A gather: the width is the OUTPUT voxel's.  float64 throughout, no atomics;
 *     the order of summation depends on nothing but the inputs: two calls give the same bits.  A voxel beyond a kernel's R never
 *     enters its sum: a voxel that is not finite spoils the outputs whose kernel covers it and no other.
 * out = the float32 rounding of the float64 result, may be grid itself; out64 (may be NULL) = that result before rounding; sigma (may
 * be NULL) = the per-voxel sigma in voxels.  The results do not depend on which optional outputs were asked for.
 * MAD_EINVAL, naming the sample: a sample that is not finite or not > 0.  MAD_EDOM ("... voxels wide"): a sample whose sigma exceeds
 * 6.0 voxels (fourier.LOCAL_FILTER_MAX_SIGMA; R <= 24) -- the interpolation is convex, so the samples alone are checked.  MAD_EINVAL:
 * NULL (other than out64, sigma), step < 1, rdims other than the formula's, a dimension < 1, 2^31 voxels or more, voxsp not positive
 * and finite.  Each is found on the host: nothing is allocated or launched, the outputs are untouched, and the next call works.
 */
int mad_map_local_filter(mad_ctx *ctx, const float *grid, const int32_t dims[3], double voxsp, const double *res,
                         const int32_t rdims[3], int32_t step, float *out, double *out64 /* may be NULL */,
                         double *sigma /* may be NULL */);

/* ---- one subunit's pair grid sharded over GPUs by blocks of map rows (the exchange steps -- OR of the flag vectors,
 *      all-gather of the per-shard top-k -- are the caller's, mad_amd/dist.py::sharded_match, or the library's own:
 *      mad_dist_or_allreduce / mad_dist_allgather_topk below) ------------------------------------------------- */

/*
 * Stage B of a sharded match: correlate hi against the lo rows [lo_begin, lo_end) (MaD.py:416-424 on that block of
 * `preds`), keep the pairs on the device, return this shard's flags "anchor takes part in a pair" (one byte per
 * anchor of hi / of lo).  The OR of the flags over all shards defines the global clouds of MaD.py:427-428.
 */
int mad_match_shard_pairs(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, int64_t lo_begin, int64_t lo_end, double cc,
                          uint8_t *used_hi, uint8_t *used_lo, int64_t *n_pairs);

/*
 * Stage C: score the shard's pairs against the global clouds (MaD.py:433-451) and return its k best in the order of
 * MaD.py:480 restricted to the shard: result rows [k][23], match counts, and pair_rank = hi_row * N_lo + lo_row, the
 * position of the pair in the unsharded row-major list.  *l_hi = size of the global hi cloud.  Must follow
 * mad_match_shard_pairs for the same sets on the same ctx.
 */
int mad_match_shard_topk(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, const uint8_t *used_hi_all,
                         const uint8_t *used_lo_all, double dist, int64_t k, double *results, int64_t *pair_rank,
                         int32_t *counts, int64_t *n_out, int64_t *l_hi);

/*
 * Stages B and C without a host round trip (MaD.py:420-451 for one block of map rows; the loop it shards is serial over subunits,
 * MaD.py:165-190).  Everything is enqueued on the lane of `hi`; the flags and the shard's list live in DEVICE memory of the caller,
 * who orders the two exchanges of SURVEY.md 8(e) -- the OR all-reduce of the flags, the all-gather of the lists -- on that lane's
 * stream (mad_set_stream(hi)) between and behind the two calls.
 *   mad_match_shard_begin: hi against the lo rows [lo_begin, lo_end) of a lo set ASSUMED to have n_lo rows (the caller cut the blocks
 *     from that number; the device checks it).  d_flags: hi->n_anchors + lo->n_anchors bytes, hi's flags first.
 *   mad_match_shard_score: the shard's pairs against the global clouds (d_flags_all: the OR over the shards, same layout); d_out:
 *     mad_match_shard_record_doubles(k) float64 = [rows m, flags, |hi cloud|, pairs][k x 23 result rows][k counts][k pair ranks].
 *     flags != 0 (1 score-matrix capacity, 2 pair capacity, 4 n_lo was wrong, 8 selection list, 16 the describe launch of hi or lo
 *     fell short -- a set rebuilt in place with more rows than its previous build, not yet repaired by a host read of its size):
 *     m = 0, repeat the shard through mad_match_shard_pairs / mad_match_shard_topk (which repair the sets).
 */
int64_t mad_match_shard_record_doubles(int64_t k);
int mad_match_shard_begin(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, int64_t lo_begin, int64_t lo_end, int64_t n_lo,
                          double cc, uint8_t *d_flags);
int mad_match_shard_score(mad_ctx *ctx, const mad_set *hi, const mad_set *lo, const uint8_t *d_flags_all, double dist, int64_t k,
                          double *d_out);
/*
 * The records of a group's shards (n float64 in device memory: what the caller's all-gather left behind mad_match_shard_score) to
 * the host: copied into pinned memory of the library on the lane of `hi`; *ticket names the copy.  mad_match_shard_wait blocks
 * until it has arrived and copies it to `out` (host).  At most 8 copies of one lane may be pending.
 */
int mad_match_shard_collect(mad_ctx *ctx, const mad_set *hi, const double *d_all, int64_t n, int *ticket);
int mad_match_shard_wait(mad_ctx *ctx, int ticket, double *out, int64_t n);
/*
 * The merge of a group's records on the device (k_shard_merge; the order of mad_amd/dist.py::merge_topk): d_all holds nranks
 * records of mad_match_shard_record_doubles(k) float64 back to back, d_merged (another buffer) receives ONE record of the same
 * layout, enqueued on the lane of `hi`:
 *   - its first m = min(k, sum of the shards' m) entries are the shards' entries in the stable order of MaD.py:480 -- count
 *     descending, global pair rank ascending -- rows copied bit for bit, the rest of the record zero;
 *   - flags = the OR of the shards' flags; m = 0 when that is non-zero (the whole group repeats the match synchronously);
 *   - |hi cloud| is the first record's, pairs the sum of the shards'.
 *   - flag 32 (beside 1 / 2 / 4 / 8 / 16 above): the records do not belong together or are malformed -- they disagree on
 *     |hi cloud|, or an m lies outside 0 .. k, a count outside 0 .. 2^24 - 1, a pair rank outside 0 .. 2^40 - 1 (the sort key
 *     is (max count - count) << 40 | pair rank; the ranks live in device memory, so it is the kernel that checks them).
 * One workgroup sorts nranks x k keys in LDS: nranks x k > MAD_SHARD_MERGE_MAX is MAD_EDOM (merge on the host then).
 */
#define MAD_SHARD_MERGE_MAX 8192
#define MAD_SHARD_FLAG_MISMATCH 32
int mad_match_shard_merge(mad_ctx *ctx, const mad_set *hi, const double *d_all, int nranks, int64_t k, double *d_merged);

/* ---- the exchanges between the GPUs of a sharded step, inside the library (mad_dist.hip) -------------------------------
 *      One communicator per ctx.  RCCL is resolved at run time (dlopen of librccl.so.1, then librccl.so, and dlsym of the six
 *      entry points used) by mad_dist_unique_id / mad_dist_init and by nothing else: libmad_amd.so does not depend on it, a
 *      process that never calls these never loads it, and a process that has it mapped already (one that imported torch) keeps
 *      that one copy.  When it cannot be loaded the call returns MAD_ENODEV and the message names what was tried; an RCCL error
 *      is MAD_EHIP with ncclGetErrorString in mad_last_error.  Every collective is enqueue-only: none blocks the host.
 *      The RCCL branch has run at world size 1 only; more than one rank on hardware is unmeasured. ------------------------ */

#define MAD_DIST_ID_BYTES 128      /* sizeof(ncclUniqueId) */
/* Rank 0 takes an id and hands it to the other ranks by whatever means the caller has (a file, MPI, a socket). */
int mad_dist_unique_id(mad_ctx *ctx, void *id128);
/*
 * Creates the communicator of rank `rank` of `nranks` (collective over the ranks when id128 != NULL).  id128 == NULL: a
 * REHEARSAL communicator -- one rank of nranks alone on its GPU, RCCL not loaded: the OR-reduce is the identity (or adds the
 * peers' flags registered with mad_dist_rehearse_flags), the all-gathers copy this rank's block into slot `rank` of the
 * receive buffer and leave every other slot as the caller filled it.  What a rehearsal reports is a per-rank cost without
 * link traffic, never a multi-GPU measurement.  A second mad_dist_init without mad_dist_destroy in between: MAD_EINVAL.
 */
int mad_dist_init(mad_ctx *ctx, int nranks, int rank, const void *id128);
int mad_dist_destroy(mad_ctx *ctx);      /* mad_destroy calls it; without a communicator it does nothing */
int mad_dist_info(mad_ctx *ctx, int *nranks, int *rank, int *rehearsal);      /* MAD_EINVAL without a communicator */
/* Rehearsal only: d_peer_or (n bytes 0 / 1 in device memory, NULL to forget them) is what the absent ranks would contribute
 * to every later mad_dist_or_allreduce of n flags; the buffer stays the caller's and must outlive those calls. */
int mad_dist_rehearse_flags(mad_ctx *ctx, const uint8_t *d_peer_or, int64_t n);
/* In place on n bytes 0 / 1 in device memory, on `stream` (a stream of the library: mad_set_stream, mad_stream): ncclMax on
 * uint8 -- RCCL has no bitwise-OR reduction. */
int mad_dist_or_allreduce(mad_ctx *ctx, void *stream, uint8_t *d_flags, int64_t n);
/* d_recv: nranks x bytes_per_rank, rank r's block at r * bytes_per_rank (the wire images of mad_set_export for mad_set_import). */
int mad_dist_allgather(mad_ctx *ctx, void *stream, const void *d_send, void *d_recv, int64_t bytes_per_rank);
/*
 * Exchange 2 of a sharded match on the lane of `hi`: the all-gather of the shards' records (d_mine: this rank's, what
 * mad_match_shard_score wrote; d_all: nranks records) and then mad_match_shard_merge into d_merged -- one record, ready for
 * mad_match_shard_collect.  nranks x k > MAD_SHARD_MERGE_MAX: MAD_EDOM, nothing enqueued (gather with mad_dist_allgather and
 * merge on the host).
 */
int mad_dist_allgather_topk(mad_ctx *ctx, const mad_set *hi, const double *d_mine, double *d_all, int64_t k, double *d_merged);
/*
 * Device memory for the buffers of these calls, for callers that have no allocator of their own on the device: buffer `which`
 * of lane `lane`, at least `bytes` long, grow-only and counted by mad_device_allocations (a steady state shows none).  A
 * buffer that grows is a NEW buffer: ask again for the address before every use, and not while work that uses it is in flight.
 * mad_dist_copy moves bytes between host memory and such a buffer, synchronously (kind 0: host to device, 1: device to host);
 * it waits for the device first.  For set-up, rehearsals and tests, not for the steady state.
 */
#define MAD_DIST_BUF_FLAGS  0
#define MAD_DIST_BUF_MINE   1
#define MAD_DIST_BUF_ALL    2
#define MAD_DIST_BUF_MERGED 3
#define MAD_DIST_BUF_WIRE   4
#define MAD_DIST_BUF_GATHER 5
int mad_dist_scratch(mad_ctx *ctx, int lane, int which, int64_t bytes, void **d_out);
int mad_dist_copy(mad_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind);

/* ---- one structure's rows built in shares on several GPUs (stage A).  Orientation and description
 *      are independent per anchor (Orientator.py:80-108, Descriptor.py:106-116): anchor a of the structure's list goes
 *      to share a % n_shares (local position a / n_shares), every rank runs mad_set_build on its share, the shares
 *      travel as fixed-size "wire images" (one all-gather, issued by the caller: mad_amd/dist.py) and every rank
 *      assembles the full set, rows in the reference's order (anchor x main x sec, Orientator.py:90-106) -- bit for bit
 *      the set mad_set_build makes from the whole list. ------------------------------------------------------------ */

/* Bytes of a wire image with room for cap_rows rows of D counts (header + main / sec / local anchor / norm / int8 rows). */
int64_t mad_set_wire_bytes(int D, int64_t cap_rows);
/*
 * Packs the rows of a built set into a wire image.  wire_on_device != 0: `wire` is device memory (e.g. the tensor
 * handed to the all-gather) and the call is asynchronous on the set's lane (mad_set_stream); otherwise host memory
 * and synchronous.  A share with more than cap_rows rows is sent as an empty image whose header carries its row count;
 * the import then fails with MAD_ENOSPC at the first call that needs the set's size.
 */
int mad_set_export(mad_ctx *ctx, const mad_set *share, void *wire, int wire_on_device, int64_t cap_rows);
/*
 * Assembles `set` from n_shares wire images laid out back to back (share r at wires + r * mad_set_wire_bytes).  The
 * anchors are those of the WHOLE structure in the reference's order; anc_coords may be NULL (an imported set is never
 * described again).  Rfinal, inv(Rfinal), the int16 counts and the result metadata are re-derived on the importing
 * GPU with the builder's own expressions.  wires_on_device as above (asynchronous on the set's lane).
 */
int mad_set_import(mad_ctx *ctx, mad_set *set, const void *wires, int wires_on_device, int n_shares, int64_t cap_rows,
                   const int32_t *anc_coords, const int32_t *anc_octave, const double *anc_subv, const int32_t *anc_index,
                   int n_anchors);
/*
 * The lane a set is built on, its HIP stream (for callers that order a collective against the export / import
 * kernels: hipStreamWaitEvent or a torch ExternalStream), and a way to put two sets on one lane so that
 * build -> export -> all-gather -> import is one in-order stream.  mad_set_bind_lane synchronises the ctx.
 */
int mad_set_lane(mad_ctx *ctx, const mad_set *set);
void *mad_set_stream(mad_ctx *ctx, const mad_set *set);
int mad_set_bind_lane(mad_ctx *ctx, mad_set *set, int lane);

/*
 * a14-a16 for a batch of placed copies of one structure, on the device end to end: candidate c's atoms
 * (atoms + c*n*3, float64) -> simulated density at the voxel spacing of the map uploaded with
 * mad_upload_density (PDB.structure_to_density(resolution, voxsp, isovalue = density_isovalue)) ->
 * ccc[c] = Dmap.get_CCC_with_grid(grid, x0, y0, z0, isovalue = ccc_isovalue) against that map.  The uploaded
 * map is clamped on the fly, not modified.  One read-back at the end (MaD.py:613-616 per solution).
 */
int mad_density_ccc(mad_ctx *ctx, const double *atoms, const double *mass, int n_cand, int64_t n,
                    double resolution, double density_isovalue, double ccc_isovalue, double *ccc);

/*
 * MaD._refine_filtered_solutions (MaD.py:556-629) for a batch of candidate poses, on the device from the poses to the scores -- what
 * mad_refine + mad_density_ccc do with a host round trip of all coordinates in between.  The candidates may belong to several
 * structures (the subunits of a run: the reference refines them one subunit after the other, MaD.py:165-190): structure s =
 * base_atoms[first_atom[s] .. first_atom[s + 1]) (float64 xyz) with masses alongside, candidate c is a pose of structure cand_struct[c]:
 *   start_c = (atoms - hi_p[c]) @ rot[c] + lo_p[c]             (MaD.py:566-569: translate_atoms(-hi), rotate_atoms(R), translate_atoms(lo);
 *                                                               rot[c] row-major 3x3 in PDB.rotate_atoms' convention coords @ R)
 *   refine_pdb(map, start_c, n_steps, max_step, min_step)      (structure_utils.py:58-161, against the map of mad_upload_density)
 *   ccc[c] = map.get_CCC_with_grid(structure_to_density(refined_c, resolution, voxsp of the map, density_isovalue), ccc_isovalue)
 * converged / last_step: refine_pdb's return values per candidate.  coords (nullable): the refined coordinates of candidate 0, 1, ...
 * back to back; NULL leaves them on the device (15 doubles per candidate in and ~1.6 KB per candidate out cross the bus).  A
 * candidate whose refinement ends in NaN coordinates (structure_utils.py:97-98) gets ccc = NaN.
 */
int mad_dock_refine_score(mad_ctx *ctx, int n_struct, const double *base_atoms, const double *mass, const int64_t *first_atom,
                          int n_cand, const int32_t *cand_struct, const double *hi_p, const double *lo_p, const double *rot,
                          int n_steps, double max_step, double min_step, double resolution, double density_isovalue,
                          double ccc_isovalue, double *coords, int32_t *converged, int32_t *last_step, double *ccc);

/* ---- next to the path, downstream: occupancy overlap for assembly building ------------ */

/*
 * structure_utils.get_overlap(g1, g2, voxsp, isovalue) (structure_utils.py:163-259): both grids
 * (host, float32 [x][y][z], z fastest) are clamped in place (values < isovalue -> 0), the common box
 * follows from the origins (Angstrom) in voxel units with python's round(), *common = voxels of the
 * box where both grids are > 0, *n_pos1 = voxels of grid1 that are > 0.  The reference's return value
 * is common / n_pos1 (0 when n_pos1 == 0 or the boxes do not meet).
 */
int mad_grid_overlap(mad_ctx *ctx, float *grid1, const int32_t d1[3], const double o1[3], float *grid2,
                     const int32_t d2[3], const double o2[3], double voxsp, double isovalue, int64_t *common,
                     int64_t *n_pos1);

/*
 * The overlap table of MaD._build_from_single / _build_models (MaD.py:667-686, 760-783) in one call:
 * structure s = atoms[first_atom[s] .. first_atom[s+1]) (float64 xyz, masses alongside) is turned into
 * PDB.structure_to_density(resolution, voxsp, isovalue = density_isovalue) on the device, the grids stay
 * there, and overlap[i * n_struct + j] = get_overlap(grid_i, grid_j, voxsp, overlap_isovalue) for i < j
 * (0 elsewhere, as the reference leaves its table).  One read-back of the counts.
 */
int mad_overlap_matrix(mad_ctx *ctx, const double *atoms, const double *mass, const int64_t *first_atom,
                       int n_struct, double resolution, double voxsp, double density_isovalue,
                       double overlap_isovalue, double *overlap);

/* ---- next to the path, upstream: MapSpace.build_space (MapSpace.py:116-189) and
 *      Detector.find_anchors (Detector.py:28-123) --------------------------------------- */

typedef struct mad_space mad_space;

int mad_space_create(mad_ctx *ctx, mad_space **out);
void mad_space_destroy(mad_ctx *ctx, mad_space *s);

/*
 * Builds the scale space of one density grid on the device.
 *   grid      host, [x][y][z] z fastest, float32 (is_f64 = 0; PDB / MRC input) or float64
 *             (is_f64 = 1; Situs input, MapSpace.py:93-96); padded with `pad` zero voxels
 *             per face (MapSpace.py:117-118).
 *   oct_mode  1 = base, 2 = upsampled, 3 = both (MapSpace.py:147-163).  List entry 0 is the
 *             upsampled octave when it exists, as in the reference.
 *   g0, g2    order-0 and order-2 Gaussian kernels of sigma_init, 2*radius+1 taps each, as
 *             scipy.ndimage computes them (the host passes numpy's values so that the
 *             weights are identical); sig2 = sigma_init^2 (MapSpace.py:171).
 *   pre       order-0 kernel of the pre-smoothing sigma (MapSpace.py:144), pre_radius = 0
 *             to skip it.
 *   lu, ev_w, ev_i   per axis a (padded length n_a): banded LU factors [5][n_a] of the
 *             not-a-knot cubic collocation matrix, and for the 2 n_a - 1 half-integer
 *             sites the 4 basis weights + first coefficient index (interp1d(kind="cubic"),
 *             MapSpace.py:206-214).  Only read when the upsampled octave is built.
 *   slot_up, slot_base   field slots that receive the gradient texels of np.gradient(
 *             gaussian_filter(grid, sigma_init)) (MapSpace.py:182-187); -1 = do not fill.
 * Filter passes reproduce scipy.ndimage's summation order and per-pass rounding; the
 * spline agrees with scipy to ~4e-16 relative (see mad_space.hip).  A build that fails, a
 * refused argument included, leaves the space empty.
 */
int mad_space_build(mad_ctx *ctx, mad_space *s, const void *grid, int is_f64, int nx, int ny, int nz, int pad,
                    int oct_mode, const double *g0, const double *g2, int radius, double sig2,
                    const double *pre, int pre_radius, const double *const *lu, const double *const *ev_w,
                    const int32_t *const *ev_i, int slot_up, int slot_base);

/* n_octaves list entries; dims6 = [entry][3]; kind2[entry] = 0 upsampled / 1 base; is_f64_2[entry]. */
int mad_space_info(mad_ctx *ctx, const mad_space *s, int *n_octaves, int32_t *dims6, int32_t *kind2, int32_t *is_f64_2);

/* what: 0 = grid_list[entry], 1 = map_space[entry] (LoG), 2 = gauss_list[entry]; storage type of the entry. */
int mad_space_download(mad_ctx *ctx, const mad_space *s, int entry, int what, void *out);

/*
 * skimage.feature.peak_local_max(map_space[entry], exclude_border=border, threshold_abs=
 * threshold) as Detector.py:29 calls it: voxels equal to the maximum of their zero-extended
 * 3x3x3 neighbourhood and strictly above the threshold, compared in the storage type of the entry
 * as numpy does: a float32 entry against (float)threshold (round to nearest), a float64 entry
 * against threshold.  Returns linear indices
 * ((x*ny + y)*nz + z) and values in NO particular order; the host sorts (row-major, then by
 * descending value).  MAD_ENOSPC with *n_out = required capacity if cap is too small.
 */
int mad_space_peaks(mad_ctx *ctx, const mad_space *s, int entry, double threshold, int border, int64_t *lin_index,
                    double *value, int64_t cap, int64_t *n_out);

/* (2r+1)^3 LoG neighbourhoods of n voxels (zero outside), storage type of the entry: the input of
 * Detector.check_localize (Detector.py:53-123) on the host, for the candidates mad_space_localize
 * leaves undecided. */
int mad_space_patches(mad_ctx *ctx, const mad_space *s, int entry, const int32_t *coords, int n, int r, void *out);

/*
 * Detector.check_localize (Detector.py:53-123) for n candidate voxels of map_space[entry], on the
 * device and in place: the walk of at most 5 quadratic fits, the moves with the border limits
 * x - 1 > 0 and x + 1 < shape - 1 per axis (:87-99), the stop when every |offset| < 0.6 (:84), and
 * the rejection of a fit whose Hessian has a positive eigenvalue (:104-108).
 *   cand      [n][3] starting voxels, each inside [1, shape - 2] on every axis (else MAD_EDOM)
 *   status    [n]: 0 rejected, 1 accepted, 2 undecided
 *   coord     [n][3]: the voxel the walk ended on (the anchor's voxel when status = 1)
 *   H, G      [n][9] and [n][3] in the storage type of the entry: Hessian and gradient of the last
 *             fit, built from the same voxel reads in the same operation order as the reference
 *   n_undecided   number of status-2 candidates (may be NULL)
 * H and G are exact; the decisions are taken from a float64 solve only outside a guard band that
 * covers the rounding of numpy's -dot(inv(H), G) in the storage type and of geev (DESIGN.md section
 * 4b).  Status 1: the caller finishes offset = -dot(inv(H), G) itself.  Status 2 (inside the band, or
 * H near-singular, where numpy may or may not raise): the caller runs check_localize on that
 * candidate.  Status 0 is final.  n = 0 is a no-op.  Results come back in one copy.
 */
int mad_space_localize(mad_ctx *ctx, const mad_space *s, int entry, const int32_t *cand, int n, int32_t *status,
                       int32_t *coord, void *H, void *G, int64_t *n_undecided);

/* The same kernel on a host volume [nx][ny][nz] (z fastest), float32 (is_f64 = 0) or float64 (1),
 * uploaded for the call: for volumes that are not a mad_space, such as test fixtures. */
int mad_localize_volume(mad_ctx *ctx, const void *vol, int is_f64, int nx, int ny, int nz, const int32_t *cand, int n,
                        int32_t *status, int32_t *coord, void *H, void *G, int64_t *n_undecided);

/* ---------------------------------------------------------------------------
 * Pose filter: the greedy clustering of MaD._filter_dsc_pairs (mad/MaD.py:456-553) for n_match matches in one call.
 *   rows[m]       float64 [>= n_rows[m]][23], the result rows sorted as _filter_dsc_pairs sorts them (repeatability
 *                 descending, stable); the first n_rows[m] = min(len, n_samples) are read
 *   cloud[m]      float64 [n_cloud[m]][3], the match's hi cloud
 *   rmsd_thresh   the reference's rmsdcloud_thresh (10)
 *   owner_out[m]  int32 [n_rows[m]]: the row index of the row's cluster leader (owner[i] == i: row i leads a new cluster)
 *   d2min_out[m]  float64 [n_rows[m]]: the smallest sum((cloud(c) - cloud(i))**2) / N over the leaders c before row i (row 0: 0)
 *   n_done_out[m] rows decided, from row 0;  status_out[m]  0 = all n rows decided, 1 = row n_done is undecided
 * Row 0 leads cluster 0; row i leads a new one when sqrt(min d2) > rmsd_thresh and otherwise joins the leader with the
 * smallest d2 (the earliest on a tie).  The device decides only outside a guard band around rmsd_thresh^2 and between
 * the two nearest leaders that covers the rounding of numpy's expression and its own.  The first
 * row inside the band ends the match: status 1, rows from n_done on have owner -1 and d2min NaN (d2min[n_done] = the
 * doubtful minimum), and the caller runs the host loop for that match -- later rows depend on the undecided one.
 * n = 0 does nothing (n_done 0, status 0), n = 1 leads trivially; N = 0 with n > 1 (the reference divides by zero) and
 * non-finite input are undecided at row 1.  MAD_EINVAL: null pointers, negative sizes, a negative or non-finite
 * threshold; MAD_EDOM: n_rows[m] > MAD_POSE_CLUSTER_MAX_N.  Host pointers, synchronous, on lane 0 (mad_stream); the d2
 * triangles (n (n - 1) / 2 doubles per match) live in grow-only scratch of the context: a call is split into launches of at
 * most 16 matches and 256 MiB of triangles, so the scratch never grows beyond that.
 * Two calls on the same input return the same bits (fixed reduction trees, no atomics).
 */
int mad_pose_cluster_many(mad_ctx *ctx, int n_match, const double *const *rows, const int32_t *n_rows,
                          const double *const *cloud, const int32_t *n_cloud, double rmsd_thresh, int32_t *const *owner_out,
                          double *const *d2min_out, int32_t *n_done_out, int32_t *status_out);

/* ---------------------------------------------------------------------------
 * Assembly ranking: the HEAD of the two sorted lists MaD.build_assembly searches, by ordered enumeration with prefix
 * pruning on the device.  overlap is the n x n float64 table of mad_overlap_matrix (host).
 *
 * mad_rank_copies serves mad/MaD.py:684-694: every n_copies-subset of the n solutions of one subunit, keyed by the
 * maximum of overlap[a, b] over its pairs a < b, in the order of the reference's stable sort (maximum ascending, then
 * itertools.combinations order).  A maximum is exact, so the result is that order bit for bit.
 *   mode MAD_RANK_TOP    the first min(cap, C(n, n_copies)) entries (at most MAD_RANK_MAX_TOP, else MAD_EDOM)
 *   mode MAD_RANK_BELOW  every entry with maximum <= max_overlap, *n_total of them; more than min(cap, MAD_RANK_MAX_OUT):
 *                        MAD_ENOSPC with *n_total = the count
 *   idx_out  int32 [cap][n_copies]   key_out  float64 [cap]: the maximum   rank_out  int64 [cap]: position in combinations order
 *   (key_out is +0 for a maximum of -0: the table is read as overlap + 0.0, which changes no comparison)
 *
 * mad_rank_models serves mad/MaD.py:797-807: one row out of each of n_groups contiguous groups (group l = rows
 * group_first[l] .. group_first[l + 1] - 1, group_first[0] = 0, group_first[n_groups] = n), keyed by the sum of the FULL
 * k x k block overlap[pick][:, pick] (no triangular table assumed), in itertools.product order on ties.  The sum is a rounded
 * one, so the device returns a SUPERSET: with T the cap-th smallest device sum by (sum, rank), every pick whose device sum is
 * <= T (1 + 8 k^2 2^-53), in (device sum, rank) order; the reference's first cap entries are among them (derivation: DESIGN.md
 * section 4f) and the caller decides with numpy's own sum.  T = 0 returns exactly cap entries (a sum of 0 has only zero terms).
 *   cap <= MAD_RANK_MAX_TOP (after min with the size of the product), cap <= out_cap; more than min(out_cap, MAD_RANK_MAX_OUT)
 *   candidates: MAD_ENOSPC with *n_total = the count
 *   idx_out  int32 [out_cap][n_groups]: rows   key_out  float64 [out_cap]: device sums   rank_out  int64 [out_cap]
 *
 * Both: launch_items = ranks covered by one kernel launch (<= 0: the default), budget = items a call may evaluate (<= 0: the
 * default); past it, with ranks still to visit, *status = 1, *n_out = 0 and the call returns MAD_OK (no partial result); *status = 0 otherwise.
 * MAD_EDOM (the caller runs the host loop): an entry that is negative or not finite, a NaN max_overlap, n > MAD_RANK_MAX_N,
 * n_copies outside 2 .. min(n, MAD_RANK_MAX_K), n_groups outside 1 .. MAD_RANK_MAX_K, groups that do not tile 0 .. n, a
 * space beyond int64.  MAD_RANK_NO_PRUNE=1 in the environment (read per call) turns the prefix jumps off; the result does not
 * depend on it.  Host pointers, synchronous, lane 0; two calls return the same bits.
 */
int mad_rank_copies(mad_ctx *ctx, const double *overlap, int n, int n_copies, int mode, double max_overlap, int64_t cap,
                    int64_t launch_items, int64_t budget, int32_t *idx_out, double *key_out, int64_t *rank_out,
                    int64_t *n_out, int64_t *n_total, int32_t *status);
int mad_rank_models(mad_ctx *ctx, const double *overlap, int n, const int32_t *group_first, int n_groups, int64_t cap,
                    int64_t out_cap, int64_t launch_items, int64_t budget, int32_t *idx_out, double *key_out,
                    int64_t *rank_out, int64_t *n_out, int64_t *n_total, int32_t *status);
/* The last mad_rank_* call: kernel launches over rank ranges, items whose key was evaluated, items jumped over by prefix
 * pruning, and whether the band of mad_rank_models held more than cap candidates. */
int mad_last_rank_plan(mad_ctx *ctx, int64_t *launches, int64_t *evaluated, int64_t *skipped, int32_t *band_extra);

#ifdef __cplusplus
}
#endif
#endif /* MAD_AMD_H */
