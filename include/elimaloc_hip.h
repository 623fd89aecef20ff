/*
 * elimaloc_hip.h -- C ABI of the MI355X-native pcm_matching registration hot path.
 *
 * This is the drop-in boundary: every entry point replaces one in-process C++ call of the reference
 * (ELiMaLoc @ 2025-02-27).  Citations are relative to /root/reference/src/app/localization/ :
 *   reg.hpp/reg.cpp = pcm_matching/{include,src}/registration.{hpp,cpp}
 *   vhm.hpp/vhm.cpp = pcm_matching/{include,src}/voxel_hash_map.{hpp,cpp}
 *   pcm.hpp/pcm.cpp = pcm_matching/{include,src}/pcm_matching.{hpp,cpp}
 *
 * Conventions
 *   - plain pointers and sizes only; 4x4 / 6x6 / 3x3 matrices are column-major doubles (Eigen's default).
 *   - every function returns an int status: 0 = ok, <0 = error (see elm_strerror); the status is SEPARATE
 *     from the algorithmic is_success flag of RunRegister.
 *   - a context owns one GPU (one process per GPU), one HIP stream and all scratch memory.  Calls on one
 *     context must be serialised by the caller (the reference serialises them with mutex_pcl_, pcm.cpp:199,357).
 *   - no CPU fallback exists: without a gfx950 device elm_ctx_create fails.
 */
#ifndef ELIMALOC_HIP_H
#define ELIMALOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELM_OK 0
#define ELM_ERR_INVALID -1     /* bad argument */
#define ELM_ERR_DEVICE -2      /* HIP runtime error (elm_last_error has the text) */
#define ELM_ERR_NO_DEVICE -3   /* no usable gfx950 device */
#define ELM_ERR_COMM -4        /* RCCL error / not initialised */
#define ELM_ERR_UNSUPPORTED -5 /* e.g. a host-fed stream with a communicator attached; a search index that cannot be built */
#define ELM_ERR_IO -6          /* file missing / unreadable */
#define ELM_ERR_ALLOC -7       /* host allocation failed */

#define ELM_MAX_ITER_TRACE 64

typedef struct elm_ctx elm_ctx;
typedef struct elm_map elm_map;   /* VoxelHashMap, device resident (vhm.hpp:89-335) */
typedef struct elm_scan elm_scan; /* one source scan (sensor frame), device resident */

/* IcpMethod (reg.hpp:60) */
enum { ELM_P2P = 0, ELM_GICP = 1, ELM_VGICP = 2, ELM_AVGICP = 3 };

/* POD mirror of RegistrationConfig (reg.hpp:62-85), same field names. */
typedef struct elm_reg_config {
    int32_t i_max_thread;        /* unused on the GPU; kept for API parity */
    int32_t icp_method;          /* ELM_P2P .. ELM_AVGICP */
    int32_t voxel_search_method; /* parsed but unused by the reference (pcm.cpp:175) */
    int32_t use_radar_cov;       /* reg.hpp:186-217: first iteration adds CalPointCov of the point under the initial guess, later ones I */
    int32_t max_iteration;
    int32_t b_debug_print;
    double gicp_cov_search_dist;
    double max_search_dist;
    double lm_lambda;
    double icp_termination_threshold_m;
    double min_overlap_ratio;
    double max_fitness_score;
    double doppler_trans_lambda;
    double range_variance_m;
    double azimuth_variance_deg;
    double elevation_variance_deg;
    double ego_to_lidar_trans[3];
    double ego_to_lidar_rot[9];
    double ego_to_imu_rot[9];
} elm_reg_config;

/* Fills the shipped defaults of config/localization.ini:80-105. */
void elm_reg_config_default(elm_reg_config* cfg);

/* Per-iteration record (optional; see elm_reg_result.trace). */
typedef struct elm_iter_trace {
    double JTJ[36]; /* column-major, before damping */
    double JTr[6];
    double residual_sum;
    double n_corr;
    double x[6];
    double step_norm;
    double T[16];
} elm_iter_trace;

/* elm_reg_result.path: the accumulate kernels of the call.  GRID (dense / two-level cell grid: P2P, GICP) and VOXEL_LISTS (VGICP, AVGICP)
 * are the fast kernels; LISTS / WALK are the fall-back index forms of maps no grid can hold (or ELM_KERNEL); PAIRS = the per-pair kernels
 * (use_radar_cov, ELM_CHECK=strict_pairs, or -- with one warning per map on stderr -- asymmetric covariances where the search is the plain
 * walk: 12-27 times slower); | SIDE_RECORDS: the map holds asymmetric covariances and the fast kernels carried their antisymmetric sums. */
#define ELM_PATH_GRID 1
#define ELM_PATH_LISTS 2
#define ELM_PATH_VOXEL_LISTS 3
#define ELM_PATH_WALK 4
#define ELM_PATH_PAIRS 5
#define ELM_PATH_SIDE_RECORDS 16

/* Outputs of one RunRegister (reg.cpp:274-418). */
typedef struct elm_reg_result {
    double T[16];         /* returned pose (column-major) */
    double fitness_score; /* written only on success, as the reference's out-param (reg.cpp:415); else 0 */
    double d_fitness;     /* Registration::d_fitness_score_ at return */
    double local_cov[36]; /* I unless GICP (reg.cpp:280,142) */
    int32_t is_success;
    int32_t iterations; /* executed iterations */
    int32_t gate;       /* 0 none, 1 empty map, 2 overlap ratio (reg.cpp:352), 3 fitness (reg.cpp:405) */
    int32_t path;       /* which kernels ran (ELM_PATH_*; 0: nothing iterated) */
    double n_corr_last; /* correspondences of the last executed iteration */
    double point_iterations; /* scan points processed x iterations */
    /* work counters summed over the executed iterations (for the algorithmic-bytes model): 0 unless
     * elm_ctx_set_work_counters(ctx, 1) */
    double n_cand_total;     /* candidate map points (P2P/GICP) or voxel means (VGICP/AVGICP) distance-tested */
    double n_occ_total;      /* occupied neighbour voxels visited */
    double fallback_blocks;  /* workgroup launches that took the un-staged path */
    double n_tested_total;   /* candidates whose distance was actually evaluated (after exact cell pruning) */
} elm_reg_result;

typedef struct elm_map_info {
    uint64_t n_input_points;
    uint64_t n_points; /* retained by AddPoints' spacing rule */
    uint64_t n_voxels;
    uint64_t hash_capacity;
    double voxel_size;
    int32_t max_points_per_voxel;
    int32_t has_voxel_cov;
    int32_t has_point_cov;
    int32_t layout_flags; /* bit 0: GICP payload as 64-byte {mean, normal, k} records (a point covariance of the form I - 0.999 n n^T
                           * has its inverse rebuilt as I + k n n^T; a point outside that form is flagged and reads its stored inverse),
                           * bit 1: the same for the voxel covariances of VGICP / AVGICP (clear: ELM_CHECK=full_records, all stored inverses),
                           * bit 2: the P2P / GICP cell grid is the two-level (tiled) form (box too large / sparse for one dense table),
                           * bit 3: no point covariance is flagged: GICP runs the kernels without the stored-inverse fallback and gathers its
                           *        pair fused, A = w I + (w k) n n^T (clear with ELM_CHECK=pair_nine at map build: nine entries of w C^-1),
                           * bit 4: the same for the voxel covariances (VGICP's pair; AVGICP gathers sum w and sum (w k) n n^T per point),
                           * bit 5: the face sublists are written for AVGICP's fused walk,
                           * bit 6: ... and some voxel is flagged: the fused walk skips its pairs and a fix-up launch over the marked
                           *        workgroups adds them (ELM_CHECK=avg_inline at map build: the nine-entry walk with its in-line fallback instead),
                           * bit 7: some flagged POINT covariance has an asymmetric stored inverse (rank-deficient neighbourhood, U != V in its
                           *        SVD): GICP's kernels on this map also write the 15 antisymmetric side sums per workgroup and the solve restores
                           *        all 36 entries of J^T M J (LDLT on the lower triangle, as the reference); ELM_CHECK=strict_pairs runs
                           *        the reference's per-pair arithmetic instead (the in-product checker, 12-27 times slower),
                           * bit 8: the same for the voxel covariances (VGICP / AVGICP),
                           * bit 9: the cell grid of this map was built on the device (elm_map_set_index_build; set only when the device
                           *        producer ran to the end). */
    uint64_t device_bytes;
    uint64_t n_query_voxels; /* cell grid: voxels of the dense statistics box; neighbourhood lists: query voxels (0 until built) */
    uint64_t nbr_entries;    /* cell grid: == n_points (every map point once); neighbourhood lists: ~27 x n_points */
    uint64_t index_bytes;    /* device bytes of the search structures the accumulate kernels read (built on first use) */
    uint64_t index_part_bytes[4]; /* ... by structure: [0] cell grid (blocks + offsets: P2P / GICP), [1] voxel-mean lists + per-voxel records
                                   * (VGICP; AVGICP without a face table), [2] AVGICP's face sublists + their table, [3] neighbourhood lists (the
                                   * fall-back index of P2P / GICP) */
    uint64_t n_list_voxels;       /* query voxels of the voxel-mean lists (0 until built) */
} elm_map_info;

/* ---------------------------------------------------------------- run-time switches --------------- */
/* The library reads FIVE environment variables (+ ELM_DEVICES, read by the C++ shims in include/elimaloc/).  None is needed in
 * production: the defaults are what every number in DESIGN.md is measured with; the others select shipping code paths that other maps
 * reach by themselves (so that tests can force them onto small maps) or run the in-product checkers of the fast forms.
 *   ELM_KERNEL          grid (default: dense / two-level cell grid for P2P / GICP, voxel-mean lists for VGICP / AVGICP) | lists (the
 *                       fall-back index of maps no grid can hold: per-query-voxel neighbourhood lists) | direct (the plain walk -- 27 hash
 *                       probes, every bucket point, float64: the in-kernel reference of the parity tests).  Read at elm_ctx_create.
 *   ELM_GRID            comma-separated: dense | tiled (forbid / force the two-level form), max_cells=N (cell budget of the dense offset
 *                       table, default 1.5e9), max_block_bytes=N (block arrays beyond N bytes are addressed in 16-byte units, default 4 GB).
 *                       Read when a map's search index is built.
 *   ELM_CHECK           comma-separated in-product checkers: strict_pairs (covariance methods run the reference's per-pair arithmetic: all
 *                       36 entries of J^T M J, 3x3 products and an inverse per pair), full_records (pairs read the stored 3x3 inverses
 *                       instead of the compact {mean, normal, k} records), pair_nine / avg_nine (nine entries of w C^-1 per pair instead of
 *                       the fused gathers), avg_inline / avg_fixup (AVGICP on maps with flagged voxels: in-line fallback / fix-up launch,
 *                       whatever the map's share of flagged voxels), query_direct (elm_map_get_correspondences by the plain walk),
 *                       free_wave (elm_map_check_free_space: a wave per ray instead of a lane per ray; the same counts),
 *                       ray_poses=N (elm_map_raycast: N = 1 .. 16 poses per workgroup instead of the shipped block; the same outputs).
 *   ELM_SCAN_ORDER      none: elm_scan_upload keeps the caller's point order (default: Hilbert order over 2 m cells, on the device).
 *   ELM_GROUP_EXCHANGE  host | rccl: the exchange of a device group (default: RCCL when every rank has a device of its own).
 *   ELM_DEVICES         (shims) "0,1,2,3": the process-wide context of the C++ shims is a device group over these GPUs.
 * Measured-negative experiments of rounds 2-5 (fused reduction, half-set streams, graph replay, wave-level reduction, previous-winner
 * bound, patch table ...) are not in the library any more: profiles/r06_removed_*.patch re-adds each. */

/* ---------------------------------------------------------------- context ------------------------- */
int elm_ctx_create(int device_id, elm_ctx** out);
void elm_ctx_destroy(elm_ctx* ctx);
const char* elm_last_error(const elm_ctx* ctx); /* text of the last ELM_ERR_DEVICE / ELM_ERR_COMM */
const char* elm_strerror(int status);
int elm_ctx_synchronize(elm_ctx* ctx);
/* native hipStream_t of the context (for hipEvent timing by the caller) */
void* elm_ctx_stream(elm_ctx* ctx);

/* Optional per-kernel timing with hipEvents recorded on the context stream around every accumulate launch and
 * every solve(+exchange) step of elm_register_batch* / _stream.  Totals accumulate until reset. */
typedef struct elm_profile {
    uint64_t accumulate_launches;
    uint64_t solve_steps;
    double accumulate_ms; /* sum of the spans of the main accumulate kernel (k_accumulate_cell / _vnbr / _direct) */
    double solve_ms;      /* sum of the reduce/solve (+ all-reduce, + slot refill) spans */
} elm_profile;
int elm_ctx_set_profiling(elm_ctx* ctx, int enable);
/* Work counters of elm_reg_result (n_cand_total, n_occ_total, n_tested_total, fallback_blocks): OFF by default -- the registration
 * launches then carry no instrumentation and those fields read 0; on: the same kernels with
 * the counters compiled in (~1 % slower).  poses, flags, iteration counts and point_iterations do not depend on the switch. */
int elm_ctx_set_work_counters(elm_ctx* ctx, int enable);
int elm_ctx_get_profile(elm_ctx* ctx, elm_profile* out, int reset);

/* ---------------------------------------------------------------- map ----------------------------- */
/* VoxelHashMap::Init + AddPoints (vhm.cpp:26-29, 270-285; call site pcm.cpp:87-88).  xyz: n*3 float32 map
 * points in file order (the PCD is float32, pcm.hpp:205-215).  Serial insertion semantics (trunc keys,
 * min-spacing rule, <= max_points) are reproduced per voxel; buckets are uploaded to the device. */
int elm_map_build(elm_ctx* ctx, const float* xyz, size_t n, double voxel_size, int max_points_per_voxel,
                  elm_map** out);
void elm_map_destroy(elm_map* map);
/* VoxelHashMap::CalVoxelCovAll (vhm.hpp:183-193), HIP kernel over voxels */
int elm_map_cal_voxel_cov_all(elm_map* map);
/* VoxelHashMap::CalPointCovAll (vhm.hpp:252-257), HIP kernel over map points */
int elm_map_cal_point_cov_all(elm_map* map, double d_search_dist);
/* Build the search index of the P2P / GICP correspondence search now instead of on the first registration (an init-time cost of about
 * 0.3 s on a 10 M-point map with the host build, 4 ms with the device index build below): the dense half-voxel CELL GRID -- the map
 * points once more, sorted by cell in 48-byte blocks of four,
 * plus one offset per cell of the bounding box -- when the box fits the cell and byte budgets; its two-level form (tiles of 8 x 8 columns
 * with their own z range) when it does not; the round-1 neighbourhood lists (per query voxel the points of its 27 buckets, 27x the map)
 * only when neither can be built or ELM_KERNEL=lists asks for them.  Results do not depend on which index is in use (the reference's
 * visiting order -- vhm.cpp:234-240, insertion order inside a bucket -- settles exact ties in all of them). */
int elm_map_build_neighbourhoods(elm_map* map);
int elm_map_get_info(const elm_map* map, elm_map_info* info);
/* VoxelHashMap::Empty (vhm.hpp:325) */
int elm_map_empty(const elm_map* map);
/* VoxelHashMap::Pointcloud (vhm.cpp:245-255): xyz[3n] doubles; optional per-point cov (9, col-major) and mean (3).
 * Order is bucket order (the reference's order is unordered_map iteration order; only the set is contractual). */
int elm_map_download_points(const elm_map* map, double* xyz, double* cov9, double* mean3, size_t cap);
/* all voxels: stored key (3 ints), point count, cov (9) and mean (3); Covariances() (vhm.cpp:257-265) is the
 * subset with count > 2 */
int elm_map_download_voxels(const elm_map* map, int32_t* key3, int32_t* npts, double* cov9, double* mean3,
                            size_t cap);
/* VoxelHashMap::GetCorrespondencePoints (what = 0; voxel_hash_map.cpp:31-88), ::GetCorrespondencesCov (1; :90-151) and
 * ::GetCorrespondencesAllCov (2; :153-206) as calls of their own -- Registration::RunRegister (registration.cpp:317-334) never needs them
 * (its iterations search and accumulate in one kernel), a caller of the map's public interface may.  xyz: n points in the MAP frame
 * (PointStruct::pose after TransformPoints), column order x, y, z.  Pairs come back in input order (the reference's vectors: ranges joined
 * in order): src_index[k] = the query point of pair k, tgt_index[k] = its target -- what 0: position of the map point in
 * elm_map_download_points order, what 1 / 2: position of the voxel in elm_map_download_voxels order; -1 = the reference's default target at
 * the origin (no neighbour bucket at all around the point, voxel_hash_map.cpp:37 / :105; never for what 2).  what 2 yields up to seven
 * pairs per point in the reference's neighbour order (0, +x, -x, +y, -y, +z, -z).  At most `cap` pairs are written; *n_pairs is the full
 * count.  The search is the accumulate kernels' own (their QUERY instantiations); ELM_CHECK=query_direct runs the plain 27-probe walk instead. */
int elm_map_get_correspondences(elm_ctx* ctx, const elm_map* map, int what, const double* xyz, size_t n, double max_dist,
                                uint32_t* src_index, int32_t* tgt_index, size_t cap, size_t* n_pairs);

/* Registration::AlignCloudsLocal (method ELM_P2P; registration.cpp:15-66), ::AlignCloudsLocalPointCov (ELM_GICP; :68-152) and
 * ::AlignCloudsLocalVoxelCov (ELM_VGICP / ELM_AVGICP; :154-225) on pairs the CALLER holds (RunRegister pairs and accumulates in one kernel and
 * never calls them): src_local = PointStruct::local of the n source points (sensor frame), tgt_xyz = the targets' positions in the map
 * frame -- PointStruct::pose for P2P, covariance.mean for the covariance methods (registration.cpp:97, 172) --, tgt_cov9 = their 3x3
 * covariances (column-major; NULL for P2P), src_cov9 = the source points' covariance terms, added when cfg->use_radar_cov (NULL: none).
 * T_out = the step as a column-major 4x4 (the reference's return value), local_cov = the inverse of the damped normal matrix (written
 * for ELM_GICP only, like the reference's out-parameter), *fitness_score = d_fitness_score_ (residual sum / n).  cfg: lm_lambda and
 * use_radar_cov are read (NULL: the defaults).  The pairs are accumulated on the device with the reference's per-pair arithmetic
 * (all 36 entries of J^T M J for the covariance methods: a non-symmetric covariance behaves as in the reference). */
int elm_align_clouds_local(elm_ctx* ctx, int method, const double* src_local, const double* tgt_xyz, const double* tgt_cov9,
                           const double* src_cov9, size_t n, const double last_icp_pose[16], double trans_th,
                           const elm_reg_config* cfg, double T_out[16], double local_cov[36], double* fitness_score);

/* VoxelHashMap::FindGroundHeight (vhm.hpp:285-322); *found = 0/1 */
int elm_map_find_ground_height(const elm_map* map, double x, double y, double* ground_z, int* found);

/* ---------------------------------------------------------------- scans --------------------------- */
/* Upload one source scan (sensor frame, packed float32 xyz, 12 bytes per point; PointStruct.local == .pose, pcm.hpp:205-220).
 * n_total is the size of the whole scan when this context holds only a shard of it (multi-GPU; the overlap
 * ratio of reg.cpp:351 is taken against n_total); pass n_total = n on one GPU.  The points go to HBM as they are and are
 * re-ordered ON THE DEVICE along a Hilbert curve over 2 m sensor-frame cells for locality (source order is not contractual:
 * the reference's own VoxelDownsample emits unordered_map order, vhm.hpp:278-280; ELM_SCAN_ORDER=none keeps the caller's). */
int elm_scan_upload(elm_ctx* ctx, const float* xyz, size_t n, size_t n_total, elm_scan** out);
void elm_scan_destroy(elm_scan* scan);
size_t elm_scan_size(const elm_scan* scan);
/* The resident points of a scan (xyz[3 * min(cap, size)] float32, in the device order): e.g. the undistorted, downsampled
 * cloud elm_deskew_downsample produced -- what the node publishes as its debug clouds (pcm.cpp:308-316). */
int elm_scan_download(const elm_scan* scan, float* xyz, size_t cap);

/* ---------------------------------------------------------------- registration -------------------- */
/* Registration::RunRegister (reg.hpp:122-124, reg.cpp:274-418; call sites pcm.cpp:280-282, 412-414) on host
 * buffers: uploads the scan, iterates on the device, downloads the result.  trace may be NULL or an array of
 * ELM_MAX_ITER_TRACE entries. */
int elm_register(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T0[16],
                 const elm_reg_config* cfg, double T_out[16], int* is_success, double* fitness_score,
                 double local_cov[36], elm_reg_result* result, elm_iter_trace* trace);
/* What Registration::RunRegister writes to stdout for one call (reg.cpp:291-295, 343-356, 393-413), rebuilt from the call's result:
 * the warnings the reference prints whatever the configuration -- "VOXEL MAP EMPTY!", "[RunRegister] Small corresponding  ratio. r",
 * "[RunRegister] ICP Fitness Score Low f" -- and, with cfg->b_debug_print, its per-iteration line "[Registration] Total Correspondence
 * Time for: i in X ms, and cores num: N", the totals "[Registration] Total Correspondence Time: X ms" and "[Registration] RunRegister:
 * iteration N executed in Y ms", the corresponding ratio and the fitness score, with the reference's colour codes
 * (localization_functions.hpp:78-85) and stream formatting.  trace (per-iteration n_corr) and corr_ms (per-iteration correspondence
 * time in ms: the accumulate launch, which IS the correspondence search + the sums here) may be NULL: the per-iteration lines are then
 * left out.  Writes at most cap bytes including the terminating NUL; returns the length the whole text needs.  elm_register prints this
 * text itself (debug lines only with b_debug_print: the default adds no event, no trace and no output on success). */
size_t elm_format_register_log(const elm_reg_config* cfg, const elm_reg_result* res, size_t n_points, const elm_iter_trace* trace,
                               const double* corr_ms, double total_ms, char* buf, size_t cap);

/* The same on B device-resident scans against one map, all iterated together (one accumulate launch, one
 * optional all-reduce and one solve launch per ICP iteration for the whole batch).  T0: 16*B doubles.
 * results: B entries.  trace: NULL or B*ELM_MAX_ITER_TRACE entries. */
int elm_register_batch(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch, const double* T0,
                       const elm_reg_config* cfg, elm_reg_result* results, elm_iter_trace* trace);
/* Continuous batching: `count` registrations through `slots` device slots.  Finished slots are refilled on the device with
 * the next pending registration after every ICP iteration, so every launch stays full until the queue is empty (throughput
 * mode for many more registrations than can usefully iterate in lockstep).  Results are bit-identical to
 * elm_register_batch on the same resident scans (which slot serves a registration may vary from call to call on one
 * rank -- the solve kernel hands out the queue positions -- but a registration's arithmetic does not depend on its slot; with a
 * communicator attached the assignment is in slot order, identical on every rank).  elm_register keeps the caller's point order
 * while elm_scan_upload orders the points: the two agree up to the order of the summation (1e-9 on every sum), not bit for bit.
 * trace: NULL or count*ELM_MAX_ITER_TRACE entries.  use_radar_cov = 1 with a covariance method: the registrations run as lockstep
 * batches of `slots` (same results as elm_register_batch; with a communicator attached the all-reduce then carries 64 sums per scan). */
int elm_register_stream(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int count, const double* T0,
                        const elm_reg_config* cfg, int slots, elm_reg_result* results, elm_iter_trace* trace);
/* The same with the scans still in HOST memory when the call starts -- RunRegister's per-call contract (reg.cpp:274-290: the
 * caller hands over a point vector): scan_xyz[i] = packed float32 xyz of registration i, n_pts[i] points.  Uploads (DMA on a copy
 * stream, in groups of ~32 MB), the device-side ordering kernel and the ICP iterations of the registrations that have already
 * arrived overlap; a slot starts a registration as soon as its scan has landed.  Page-locked sources (elm_host_alloc or
 * hipHostRegister) are read by the DMA engines directly and reach the PCIe rate; pageable ones are staged by the runtime.  HBM
 * needed: every scan of the call (12 bytes per point) + THREE staging sets of one upload group (~32 MB of packed xyz) each + 4 bytes
 * per staged point of ordering scratch.  Results are bit-identical to elm_register_stream on
 * the same scans uploaded with elm_scan_upload.  One rank only: ELM_ERR_UNSUPPORTED with a communicator or hook attached. */
int elm_register_stream_host(elm_ctx* ctx, const elm_map* map, const float* const* scan_xyz, const uint32_t* n_pts, int count,
                             const double* T0, const elm_reg_config* cfg, int slots, elm_reg_result* results, elm_iter_trace* trace);
/* page-locked host memory for the sources of elm_register_stream_host / elm_scan_upload (NULL on failure) */
void* elm_host_alloc(size_t bytes);
void elm_host_free(void* p);
/* diagnostic: GB/s of one plain host-to-device copy of `bytes` from `host` on this box (median of reps) -- the PCIe rate a
 * host-fed stream sits under */
int elm_ctx_measure_h2d(elm_ctx* ctx, const void* host, size_t bytes, int reps, double* gb_per_s);
/* Asynchronous halves of elm_register_batch: enqueue everything on the context stream / wait and fetch results.  enqueue returns
 * without waiting for the device on the first batch of a context; afterwards it polls the device-side count of still-iterating
 * scans (one 4-byte read-back where the previous batch finished, then every second iteration) so that it can stop enqueueing
 * iterations early -- i.e. it may block for the iterations enqueued so far.  Exactly one batch may be in flight per context. */
int elm_register_batch_enqueue(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch,
                               const double* T0, const elm_reg_config* cfg, int want_trace);
int elm_register_batch_finish(elm_ctx* ctx, elm_reg_result* results, elm_iter_trace* trace);

/* ---------------------------------------------------------------- relocalization ------------------ */
/* Recovery from a coarse pose (the clicked pose of CallbackInitialPose, pcm.cpp:356-447, metres / tens of degrees off): every pose of an
 * xy x yaw grid around the guess is scored on the device by voxel occupancy, the best ones after non-maximum suppression are refined by ICP.
 * score(T) = the number of COUNTED scan points -- ((x*x + y*y) + z*z) <= score_max_range_m^2 in float64 -- whose stored key
 * (int)(q / voxel_size) (truncation, vhm.cpp:275) under q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r (float64, this association) is a voxel of
 * the map: exact, deterministic and independent of the map's search index (it reads only the voxel set). */
typedef struct elm_reloc_config {
    double radius_xy_m, step_xy_m;      /* square xy window around the guess: offsets i * step, |i| <= floor(radius / step + 1e-9) */
    double yaw_range_deg, step_yaw_deg; /* |dyaw| <= range (k = 0: 0, then +step, -step, +2 step, ...); range >= 180: k * step,
                                         * k in [0, ceil(360 / step - 1e-9)) */
    double score_max_range_m;           /* r_max of the score */
    int32_t max_score_points;           /* elm_relocalize scores every ceil(n / cap)-th point of the caller's order */
    int32_t top_k;                      /* hypotheses refined by ICP after non-maximum suppression */
    double nms_xy_m, nms_yaw_deg;       /* a hypothesis within nms_xy_m in xy AND nms_yaw_deg in yaw of a better kept one is suppressed */
    int64_t lds_budget_bytes, bitmap_max_bytes; /* the occupancy bitmap of the hypotheses' key box goes to LDS when it fits the first (at most
                                                 * 64 KiB are used), is read from global memory when it fits the second, else every key is a
                                                 * hash probe; 0 disables the LDS form / both bitmap forms.  The counts are the same in all. */
} elm_reloc_config;
typedef struct elm_reloc_candidate {
    double T0[16], T[16]; /* hypothesis pose and ICP result (column-major) */
    uint32_t score;
    int32_t hyp_index, is_success, iterations;
    double fitness_score;
} elm_reloc_candidate;
/* 5 m / 0.5 m, 180 deg / 2 deg, 50 m, 8192, 16, 1.0 m / 6 deg, 64 KiB, 64 MiB */
void elm_reloc_config_default(elm_reloc_config* c);
/* Hypotheses around T_guess (lidar frame, column-major): T_h = [Rz(dyaw_k) R0 | t0 + (i step, j step, 0)], h = (k W + (i + m)) W + (j + m),
 * W = 2 m + 1.  Writes min(cap, count) column-major poses (poses16 may be NULL when cap = 0), *n = count.  Host function, no GPU needed. */
int elm_reloc_make_hypotheses(const double T_guess[16], const elm_reloc_config* c, double* poses16, size_t cap, size_t* n);
/* scores[h] = score(poses16[h]) of the resident scan against the map (c: score_max_range_m and the two byte budgets are read).  An empty map
 * scores 0 everywhere.  ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached. */
int elm_map_score_poses(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                        const elm_reloc_config* c, uint32_t* scores);
/* Relocalize from T_guess: uploads the score subsample and the scan, scores every hypothesis, sorts them by (score desc, index asc), keeps
 * top_k after greedy non-maximum suppression and refines those with ONE elm_register_batch (the scan repeated, T0 = T_h, config reg).  The
 * winner is the first successful one with the lowest fitness_score (ties: rank); without success, rank 0.  T_out / result = the winner's;
 * cands (cap entries, may be NULL) = the kept hypotheses in rank order, *n_cands = their count.  Empty map: result.gate = 1. */
int elm_relocalize(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_guess[16],
                   const elm_reloc_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                   elm_reloc_candidate* cands, int cap, int* n_cands);

/* ---------------------------------------------------------------- global relocalization ----------- */
/* Relocalization without a guess: an xy lattice over the map x the whole turn of yaw, every pose standing on the
 * map's ground, searched exactly by branch-and-bound on the device; the best ones are refined as elm_relocalize refines its hypotheses.
 * Lattice: x_i = x_min + i * step_xy (i < NX = floor((x_max - x_min) / step_xy + 1e-9) + 1), y_j likewise; yaw_k = k * step_yaw_deg,
 * k in [0, ceil(360 / step_yaw_deg - 1e-9)), cos / sin as elm_reloc_make_hypotheses' full-turn mode.  Pose (k, i, j):
 * T = [Rz(yaw_k) R0 | (x_i, y_j, fl(g(x_i, y_j) + h))] where T_tilt = [R0 | (0, 0, h)] (sensor roll / pitch and height above the ground;
 * a T_tilt with a non-zero x or y translation is ELM_ERR_INVALID) and g is the ground field of elm_map_ground_heights.  A node without
 * ground is not a pose.  Index hyp = (k NX + i) NY + j; a lattice above 2^31 - 1 poses is ELM_ERR_INVALID.
 * Score: elm_map_score_poses' contract, over the counted points that also satisfy (R0 p)_z + h >= score_min_height_m (float64,
 * ((R0_20 x + R0_21 y) + R0_22 z) + h; -INFINITY counts every point).  Result: the lattice sorted by (score desc, hyp asc), greedy NMS
 * (xy distance <= nms_xy_m AND wrapped |dyaw| <= nms_yaw_deg of a kept pose suppresses) down to top_k -- identical to scoring every
 * valid pose of the lattice -- then ONE elm_register_batch and elm_relocalize's winner rule. */
typedef struct elm_reloc_global_config {
    double x_min, x_max, y_min, y_max; /* the lattice's rectangle; all four NaN: the xy bounds of the map's stored points */
    double step_xy_m, step_yaw_deg;
    double score_max_range_m;   /* r_max of the score */
    double score_min_height_m;  /* counted points below this height above the ground are not counted (-INFINITY: all are) */
    int32_t max_score_points;   /* the score subsample: every ceil(n / cap)-th point of the caller's order */
    int32_t top_k;              /* kept poses, refined by ICP */
    double nms_xy_m, nms_yaw_deg;
    int32_t pool_min;           /* the first pruning threshold is the pool_min-th best score of the greedy descent's leaves */
    int32_t max_kz_span;        /* a bound whose z-key range exceeds this counts the point as a hit */
    int64_t bitmap_max_bytes;   /* the occupancy bitmap and its level windows together; more: ELM_ERR_UNSUPPORTED */
} elm_reloc_global_config;
typedef struct elm_reloc_global_stats {
    int64_t lattice_poses, valid_leaves;   /* NX NY K; the poses with ground */
    int32_t nx, ny, n_yaw, levels;         /* lattice dims; the top level of the search */
    int32_t n_counted, passes;             /* counted score points; search passes (a pass lowers the threshold when NMS keeps < top_k) */
    uint32_t tau, _pad;                    /* the last pass's pruning threshold */
    int64_t nodes_bounded[24], nodes_kept[24]; /* per level (index = level, 1 .. levels), summed over passes */
    int64_t leaves_scored;                 /* exact leaf scores, over passes (the greedy descent's included) */
    int64_t point_evals;                   /* counted points x (nodes bounded + leaves scored) */
    double ms_ground, ms_search, ms_refine; /* host wall time: ground field, search (bitmaps included), ICP */
} elm_reloc_global_stats;
/* full map rectangle, 0.5 m / 2 deg, 50 m, min height 1.0 m, 8192, 16, 1.0 m / 6 deg, pool 64, kz span 64, 256 MiB */
void elm_reloc_global_config_default(elm_reloc_global_config* c);
/* Ground heights of n xy queries (xy[2 q], xy[2 q + 1]) on the device: bit for bit elm_map_find_ground_height -- the mean of the (up to) 5
 * lowest z among the map points with dx*dx + dy*dy <= 25 (float64), summed in ascending order; found only with more than 3 such points.
 * z[q] = 0 where not found.  A 2-D bin index of the map's points is built at the first call and kept with the map.  One rank only. */
int elm_map_ground_heights(elm_ctx* ctx, const elm_map* map, const double* xy, size_t n, double* z, int32_t* found);
/* The lattice poses of elm_relocalize_global (column-major, min(cap, count) written; poses16 / valid may be NULL when cap = 0), valid[h] =
 * the node has ground, *n = NX NY K.  Invalid poses carry z = h.  With cap = 0 and an explicit rectangle only *n is computed: ctx and map
 * may then be NULL (no device needed); the arguments are checked as elm_relocalize_global checks them. */
int elm_reloc_global_hypotheses(elm_ctx* ctx, const elm_map* map, const double T_tilt[16], const elm_reloc_global_config* c,
                                double* poses16, int32_t* valid, size_t cap, size_t* n);
/* Global relocalization of a scan (sensor frame).  Outputs as elm_relocalize's (hyp_index = the lattice index); stats may be NULL.  No valid
 * pose (an empty map, a rectangle off the map): result.gate = 1, *n_cands = 0, T_out = T_tilt.  One rank only (ELM_ERR_UNSUPPORTED). */
int elm_relocalize_global(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_tilt[16],
                          const elm_reloc_global_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                          elm_reloc_candidate* cands, int cap, int* n_cands, elm_reloc_global_stats* stats);

/* ---------------------------------------------------------------- free-space check ---------------- */
/* Ray test of a scan against the map at a pose: the space between the sensor and every end point was empty when the scan was taken, so a
 * ray that passes through mapped structure before its end point is evidence against the pose (or, at a trusted pose, of a changed map).
 * Fine occupancy: cell = voxel_size / sub (float64); the fine cell of a STORED map point (elm_map_download_points' float32 coordinates as
 * float64) is f_r = (int)floor(q_r / cell) per axis -- floor, not the map's truncated keys; the occupancy is the set of these cells.
 * Per scan point p (float32 -> float64), origin o and pose T = [R | t]:
 *   d = p - o, L2 = (d_x d_x + d_y d_y) + d_z d_z, L = sqrt(L2); the ray is COUNTED when min_range_m^2 <= L2 <= max_range_m^2 and L2 > 0;
 *   reach = L - max(end_margin_m, end_margin_frac L); K = (int)floor(reach / step_m) when reach > 0, else 0, capped at max_samples;
 *   k0 = (int)floor(start_m / step_m) + 1; u = d / L; sample k in [k0, K]: a_r = o_r + u_r (k step_m),
 *   q_r = ((R_r0 a_x + R_r1 a_y) + R_r2 a_z) + t_r (float64, no contraction), fine cell floor(q_r / cell);
 *   hits = the samples whose fine cell is occupied; the ray is PIERCED when hits >= min_hits;
 *   the end point q(p) (the same transform of p itself) is END-OCCUPIED when its fine cell is occupied and SUPPORTED when that cell or one
 *   of its 26 neighbours is.  Only counted rays enter any field.  All results are integers: the same on every run and every index form. */
typedef struct elm_freespace_config {
    int32_t sub;            /* fine cells per voxel edge: 1, 2 or 4 */
    int32_t min_hits;       /* occupied samples that make a ray pierced (>= 1) */
    int32_t max_samples;    /* cap of K (1 .. 65536) */
    int32_t _pad;
    double step_m;          /* sample spacing along the ray; 0: cell / 2 of the map the call is made on */
    double start_m;         /* samples start beyond this distance from the origin (>= 0) */
    double min_range_m, max_range_m; /* counted rays: min^2 <= L2 <= max^2 */
    double end_margin_m, end_margin_frac; /* samples stop max(end_margin_m, end_margin_frac L) before the end point */
    double origin[3];       /* the ray origin in the scan frame */
} elm_freespace_config;
typedef struct elm_freespace_stats {
    uint32_t n_counted, n_pierced, n_end_occupied, n_supported;
    uint64_t n_samples, n_hit_samples;
} elm_freespace_stats;
/* sub 4, step_m 0 (= cell / 2), start 1 m, range 2 .. 50 m, margins 1 m / 0.2 L, min_hits 2, max_samples 1024, origin 0.  Why a fractional
 * margin: from height h over flat ground a ray stays within one cell c of the ground over the last c / h of its length at any range. */
void elm_freespace_config_default(elm_freespace_config* c);
/* The occupied fine cells of the map for `sub` as int32 triples in ascending (x, y, z) order: min(cap, count) written, *n = count
 * (cells3 may be NULL when cap = 0).  sub other than 1, 2, 4: ELM_ERR_INVALID. */
int elm_map_fine_cells(elm_ctx* ctx, const elm_map* map, int sub, int32_t* cells3, size_t cap, size_t* n);
/* The free-space statistics of a resident scan at n_poses poses (column-major, 16 doubles each, as elm_map_score_poses): stats[n_poses],
 * and, when hits is not NULL, hits[n_poses][elm_scan_size(scan)] = the occupied samples of every ray (saturating at 65535; 0 for a ray that
 * is not counted).  n_poses = 0 is allowed (nothing is written).  The fine occupancy table is built at the first call per (map, sub) and
 * kept with the map.  An empty map: nothing pierced, nothing supported.  ELM_ERR_UNSUPPORTED on a device group's lead or with a
 * communicator / hook attached. */
int elm_map_check_free_space(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                             const elm_freespace_config* c, elm_freespace_stats* stats, uint16_t* hits);

/* ---------------------------------------------------------------- ray casting --------------------- */
/* Standing at this pose, what range should this beam return?  An exact traversal of the map's fine cells (the occupancy of the free-space
 * check: cell = voxel_size / sub, the cells of elm_map_fine_cells) along every beam of a resident scan, at one or many poses.  Beam i starts
 * at `origin` o (scan frame) and passes through scan point p_i (float32 -> float64): a sensor model is a scan of unit vectors, a real scan
 * gives its own beams and, with them, its measured ranges L.  All arithmetic float64 without contraction; q / cell below is formed as the
 * fine occupancy forms it (q * (1 / cell) where cell is a power of two, the same bits).  Per beam and pose T = [R | t]:
 *   d = p - o, L2 = (d_x d_x + d_y d_y) + d_z d_z, L = sqrt(L2), u = d / L; the beam is CAST when L2 > 0 and finite;
 *   s_r = ((R_r0 o_x + R_r1 o_y) + R_r2 o_z) + t_r (world origin), w_r = (R_r0 u_x + R_r1 u_y) + R_r2 u_z (world direction);
 *   start: t_in = min_range_m, a_r = s_r + w_r t_in, cell c_r = (int)floor(a_r / cell);
 *   per axis sg_r = +1 / -1 / 0 by the sign of w_r and the exit parameter of the current cell
 *     tx_r = ((double)(c_r + (sg_r > 0 ? 1 : 0)) cell - s_r) / w_r, +inf when sg_r = 0 -- formed from the integer cell every time that axis
 *     steps, never accumulated;
 *   the walk: TEST the current cell; then STEP: the axis with the smallest tx (ties: x before y before z), t_next = fmax(t_in, tx_axis);
 *     if t_next > max_range_m the walk ends BY RANGE; else if max_steps steps were already taken it ends BY STEPS; else t_in = t_next,
 *     c_axis += sg_axis, tx_axis is formed anew, one step is counted; test, step, ...  (The first cell, at min_range_m, is tested like
 *     any other; max_steps steps test max_steps + 1 cells.)
 *   the first occupied cell is the HIT: range_in = its t_in, cell = c.  The walk goes on through the OCCUPIED RUN: range_out = the t_in of
 *     the first unoccupied cell after the hit, or max_range_m when the walk ends by range inside the run, or the last t_in when it ends
 *     by steps there.  A walk that ends by range without a hit is a MISS, one that ends by steps without a hit is TRUNCATED.
 *   n_steps counts the steps up to the hit or the end of the walk (the run's steps are not included: the count does not depend on what
 *     lies behind a surface).
 *   comparison with the measurement, for the cast beams with cmp_min_range_m^2 <= L2 <= cmp_max_range_m^2 (the COMPARED beams):
 *     tol = fmax(tol_m, tol_frac L); MATCH when hit and range_in - tol <= L <= range_out + tol; THROUGH when hit and L > range_out + tol
 *     (the map has a surface in front of the measurement: the free-space check's "pierced", with a position); FRONT otherwise (a miss,
 *     a truncation, or L < range_in - tol: the measurement ends before anything mapped).
 *   Why the run and not the entry alone: from height h over flat ground a beam runs inside the occupied ground layer of cells over the
 *     last cell / h of its length, so the entry of the first occupied cell lies metres before a return at 40 m; [range_in, range_out] is
 *     what a voxel map can say about where the return lies.
 * Every count is an integer and every range one IEEE division result (or a config value): the same on every run and every index form.
 * The tolerance defaults are a starting point (two fine cells of a 1 m map: a stored point lies up to cell sqrt(3) inside its cell), not
 * a measured optimum. */
typedef struct elm_raycast_config {
    int32_t sub;            /* fine cells per voxel edge: 1, 2 or 4 */
    int32_t max_steps;      /* cap of the steps of one walk (1 .. 1048576) */
    double min_range_m, max_range_m;         /* the walk covers [min_range_m, max_range_m] along the beam (0 <= min <= max) */
    double cmp_min_range_m, cmp_max_range_m; /* compared beams: min^2 <= L2 <= max^2 */
    double tol_m, tol_frac; /* tol = max(tol_m, tol_frac L) */
    double origin[3];       /* the beam origin in the scan frame */
} elm_raycast_config;
typedef struct elm_raycast_stats {
    uint32_t n_cast, n_hit, n_miss, n_truncated, n_compared, n_match, n_through, n_front;
    uint64_t n_steps;
} elm_raycast_stats;
/* sub 4, max_steps 4096, range 1 .. 100 m, compared 2 .. 50 m, tol_m 0.5, tol_frac 0.02, origin 0 */
void elm_raycast_config_default(elm_raycast_config* c);
/* The ray cast of a resident scan's beams at n_poses poses (column-major, 16 doubles each, as elm_map_score_poses): stats[n_poses] and,
 * each when not NULL, per-beam arrays [n_poses][elm_scan_size(scan)] in the resident scan's order: range_in, range_out (-1.0 for a beam
 * that did not hit), cell (int32 x 3, the hit cell; zeros when no hit), flag (0 not cast, 1 hit, 2 miss, 3 truncated).  n_poses = 0 is
 * allowed (nothing is written).  The fine occupancy table is built at the first call per (map, sub) and kept with the map.  An empty
 * map: every cast beam misses (or is truncated).  ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached. */
int elm_map_raycast(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses, const elm_raycast_config* c,
                    elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag);

/* ---------------------------------------------------------------- map evidence -------------------- */
/* Given poses we trust, which parts of the map are no longer there?  An evidence object holds two uint32 counters per occupied fine cell
 * of a map (the cells of elm_map_fine_cells(map, sub)): THROUGH, the beams that passed through the cell on the way to a farther end point,
 * and HIT, the beams that ended in it.  It lives on the device between calls and is fed by many (scan, pose) observations in one launch.
 * The walk is the ray cast's (see "ray casting"), stopped a margin before the measured end point, as the free-space check stops its samples.
 * All arithmetic float64 without contraction; q / cell below is formed as the fine occupancy forms it (q * (1 / cell) where cell is a power
 * of two, the same bits).  One OBSERVATION is one resident scan at one pose T = [R | t].  Per beam i (scan point p, float32 -> float64,
 * origin o):
 *   d = p - o, L2 = (d_x d_x + d_y d_y) + d_z d_z, L = sqrt(L2), u = d / L;
 *   the beam is CAST when L2 > 0 and finite;
 *   it is OBSERVING when cast and obs_min_range_m^2 <= L2 <= obs_max_range_m^2; only observing beams touch any counter;
 *   end point: q_r = ((R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r, e_r = (int)floor(q_r / cell);
 *     if e is an occupied cell then hit[e] += 1 and the beam is END-HIT, else it is END-FREE;
 *   reach = L - fmax(end_margin_m, end_margin_frac L); the beam WALKS when reach > min_range_m;
 *   the walk is the ray cast's with reach in the place of max_range_m:
 *     s_r = ((R_r0 o_x + R_r1 o_y) + R_r2 o_z) + t_r, w_r = (R_r0 u_x + R_r1 u_y) + R_r2 u_z;
 *     t_in = min_range_m, start cell c_r = (int)floor((s_r + w_r t_in) / cell);
 *     sg_r = +1 / -1 / 0 by the sign of w_r, tx_r = ((double)(c_r + (sg_r > 0 ? 1 : 0)) cell - s_r) / w_r, +inf when sg_r = 0, formed from
 *       the integer cell every time that axis steps;
 *     STEP: the axis with the smallest tx (ties: x before y before z), t_next = fmax(t_in, tx_axis);
 *     if t_next > reach the walk ends BY REACH; else if max_steps steps were already taken it ends BY STEPS (the beam is TRUNCATED);
 *     else the current cell is LEFT: t_in = t_next, c_axis += sg_axis, tx_axis is formed anew, one step is counted; step again;
 *   every occupied cell that the walk leaves by a step is SEEN THROUGH: through[c] += 1, one through EVENT of the beam;
 *     the cell in which the walk ends is not counted;
 *   a beam visits a cell at most once (the walk is monotone on every axis), so one beam adds at most 1 to any one counter.
 * Why the margins: from height h over flat ground a beam stays within one cell c of the ground over the last c / h of its length at any
 * range (the free-space check's grazing argument); without a fractional margin every ground return would see through the ground before it.
 * Every result is an integer and integer addition commutes: the counters and stats are the same on every run, for every job order and
 * every search-index form. */
typedef struct elm_evidence elm_evidence;
typedef struct elm_evidence_config {
    int32_t sub;            /* fine cells per voxel edge: 1, 2 or 4; must equal the evidence object's */
    int32_t max_steps;      /* cap of the steps of one walk (1 .. 1048576) */
    double min_range_m;     /* the walk starts here along the beam (>= 0) */
    double obs_min_range_m, obs_max_range_m; /* observing beams: min^2 <= L2 <= max^2 */
    double end_margin_m, end_margin_frac;    /* the walk stops max(end_margin_m, end_margin_frac L) before the end point */
    double origin[3];       /* the beam origin in the scan frame */
} elm_evidence_config;
typedef struct elm_evidence_stats {
    uint32_t n_cast, n_observing, n_walked, n_truncated;
    uint32_t n_through_beams;    /* observing beams with at least one through event */
    uint32_t n_end_hit, n_end_free, _pad;
    uint64_t n_through_events, n_steps;
} elm_evidence_stats;
/* The rule that turns counters into "stale": a cell is stale when through >= min_through and through >= through_per_hit * hit (the product
 * in 64 bits).  The defaults are a starting point, not a measured optimum. */
typedef struct elm_evidence_rule {
    uint32_t min_through;       /* default 3 */
    uint32_t through_per_hit;   /* default 4 */
} elm_evidence_rule;
/* sub 4, max_steps 4096, min_range 1 m, observing 2 .. 50 m, margins 1 m / 0.2 L, origin 0 */
void elm_evidence_config_default(elm_evidence_config* c);
/* min_through 3, through_per_hit 4 */
void elm_evidence_rule_default(elm_evidence_rule* r);
/* An evidence object bound to (map, sub), sub in {1, 2, 4}, all counters zero.  The map's fine occupancy table is built when it is not there
 * yet.  The object is destroyed before its map (it is not used after elm_map_destroy of that map; destroying it later only releases its
 * own memory, as a map or scan destroyed after its context does).  An empty map gives zero cells: accumulation runs and counts nothing.
 * ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached, here and in every call below that takes ctx. */
int elm_evidence_create(elm_ctx* ctx, const elm_map* map, int sub, elm_evidence** out);
void elm_evidence_destroy(elm_evidence* ev);
/* All counters and the object's beam total back to zero. */
int elm_evidence_reset(elm_ctx* ctx, elm_evidence* ev);
/* One observation: the resident scan at pose T16 (column-major).  stats (may be NULL): the observation's counts.  events (may be NULL):
 * events[elm_scan_size(scan)], the through events of every beam in the resident scan's order, saturating at 65535, 0 for a beam that does
 * not observe.  ELM_ERR_INVALID: cfg.sub differs from the object's, a non-finite pose entry, a scan or evidence of another context, a
 * batch in flight.  The object keeps a 64-bit total of the beams accumulated; a call that would carry it beyond 2^32 - 1 is refused with
 * ELM_ERR_UNSUPPORTED before anything is launched, so no counter can wrap. */
int elm_evidence_accumulate(elm_ctx* ctx, elm_evidence* ev, const elm_scan* scan, const double T16[16], const elm_evidence_config* cfg,
                            elm_evidence_stats* stats, uint16_t* events);
/* n_jobs (1 .. 4096) observations in one launch: scans[j] at poses16 + 16 j.  Jobs may have any sizes, 0 included; the same scan may appear
 * several times.  stats (may be NULL): stats[n_jobs].  The counters afterwards are those of the same jobs accumulated one by one, in any
 * order. */
int elm_evidence_accumulate_batch(elm_ctx* ctx, elm_evidence* ev, const elm_scan* const* scans, const double* poses16, int n_jobs,
                                  const elm_evidence_config* cfg, elm_evidence_stats* stats);
/* The counters, entry for entry in elm_map_fine_cells' ascending (x, y, z) order: min(cap, count) written, *n = count (through / hit may
 * each be NULL). */
int elm_evidence_counts(elm_ctx* ctx, const elm_evidence* ev, uint32_t* through, uint32_t* hit, size_t cap, size_t* n);
/* flags: one uint8 per stored point in elm_map_download_points order, 1 when the point's fine cell is stale by `rule`; min(cap, count)
 * written, *n = count (flags may be NULL when cap = 0). */
int elm_evidence_stale_points(elm_ctx* ctx, const elm_evidence* ev, const elm_evidence_rule* rule, uint8_t* flags, size_t cap, size_t* n);

/* ---------------------------------------------------------------- map growth ---------------------- */
/* Given poses we trust, what stands there that the map does not hold?  The other half of "map evidence": a growth object holds, per
 * CANDIDATE fine cell -- a cell the map does not occupy and in which beams ended -- HIT, the beams that ended in it, THROUGH, the beams
 * that later passed through it, and a fixed-point sum of where in the cell the end points lay.  The candidate cells are not known in
 * advance: the object owns a table on the device that the accumulate calls fill.  It is fed by many (scan, pose) observations per call.
 * Beam, CAST, OBSERVING, the end point q and its cell e, reach, and the walk with its tie rule, t_next, BY REACH and BY STEPS are exactly
 * those of "map evidence", in the same float64 arithmetic without contraction; they are not restated here.
 * END CLASS of an observing beam, the first that applies:
 *   END-HIT   e is an occupied cell of the map;
 *   END-OUT   some |e_r| >= 2^20 (what lets a cell pack into one 64-bit key);
 *   END-NEAR  clearance_cells > 0 and some occupied cell e' has max_r |e'_r - e_r| <= clearance_cells (clearance_cells is 0, 1 or 2;
 *             0: never NEAR);
 *   END-NEW   every other observing beam.
 *   HIT, OUT and NEAR beams enter the stats only.  Why a clearance: without it the sensor noise next to every mapped surface would fill
 *   the table with cells that are the old surface.  The default of 1 is a starting point, not a measured optimum.
 * One CALL (elm_growth_accumulate is a batch of one job) has two phases.
 * RECORD (phase 1), for every END-NEW beam of every job of the call: e becomes a candidate if it is not one yet; hit[e] += 1; per axis
 *   sum_r[e] += k_r (uint64), with v_r = q_r / cell formed as the fine occupancy forms it and
 *   k_r = min(65535, (uint32)floor((v_r - floor(v_r)) * 65536.0)).  The clamp is part of the contract: a tiny negative v_r gives a
 *   fraction of exactly 1.0.
 * WALK (phase 2), after the end points of ALL jobs of the call are recorded: every walking beam walks the evidence walk; every candidate
 *   cell that the walk leaves by a step gets through[c] += 1, one through EVENT of the beam.  A beam never leaves its own end cell before
 *   reach: the walk is monotone and stands at a parameter <= reach < L, the parameter of the end point (in exact arithmetic; the counters
 *   are those of the walk as computed).  A beam visits a cell at most once, so it adds at most 1 to any one counter.
 * ORDER.  Inside one call the counters do not depend on the order of the jobs.  Across calls they do, by definition: a beam counts against
 *   the candidates that exist after phase 1 of its own call, not against cells created by later calls.
 * RULE.  A cell has APPEARED when hit >= min_hit and hit >= hit_per_through * through (the product in 64 bits).
 * POINT of a cell: m_r = ((double)e_r + ((double)sum_r / (double)hit + 0.5) / 65536.0) * cell, float64, formed on the host: the mean end
 *   point to half a fixed-point step.
 * Every stored quantity is an integer fed by integer atomics: the result is the same on every run, for every job order inside a call and
 * every search-index form. */
typedef struct elm_growth elm_growth;
typedef struct elm_growth_config {
    int32_t sub;            /* fine cells per voxel edge: 1, 2 or 4; must equal the growth object's */
    int32_t max_steps;      /* cap of the steps of one walk (1 .. 1048576) */
    double min_range_m;     /* the walk starts here along the beam (>= 0) */
    double obs_min_range_m, obs_max_range_m; /* observing beams: min^2 <= L2 <= max^2 */
    double end_margin_m, end_margin_frac;    /* the walk stops max(end_margin_m, end_margin_frac L) before the end point */
    double origin[3];       /* the beam origin in the scan frame */
    int32_t clearance_cells; /* END-NEAR: an occupied cell within this Chebyshev distance of e (0, 1 or 2) */
    int32_t _pad;
} elm_growth_config;
typedef struct elm_growth_stats {
    uint32_t n_cast, n_observing, n_walked, n_truncated;
    uint32_t n_end_hit, n_end_near, n_end_new, n_end_out;   /* they add up to n_observing */
    uint32_t n_through_beams;    /* observing beams with at least one through event */
    uint32_t n_dropped;          /* END-NEW beams that found no slot: always 0 (the capacity guard below) */
    uint64_t n_through_events, n_steps;
} elm_growth_stats;
/* The rule that turns counters into "appeared".  The defaults are a starting point, not a measured optimum. */
typedef struct elm_growth_rule {
    uint32_t min_hit;           /* default 3 */
    uint32_t hit_per_through;   /* default 4 */
} elm_growth_rule;
/* the evidence defaults (sub 4, max_steps 4096, min_range 1 m, observing 2 .. 50 m, margins 1 m / 0.2 L, origin 0), clearance_cells 1 */
void elm_growth_config_default(elm_growth_config* c);
/* min_hit 3, hit_per_through 4 */
void elm_growth_rule_default(elm_growth_rule* r);
/* A growth object bound to (map, sub), sub in {1, 2, 4}, without candidates.  capacity (1 .. 2^30): the most candidate cells it can hold;
 * its tables are sized once, a power of two >= 2 * capacity slots.  The map's fine occupancy table is built when it is not there yet.  The
 * object is destroyed before its map (destroying it later only releases its own memory).  ELM_ERR_UNSUPPORTED on a device group's lead or
 * with a communicator / hook attached, here and in every call below that takes ctx. */
int elm_growth_create(elm_ctx* ctx, const elm_map* map, int sub, size_t capacity, elm_growth** out);
void elm_growth_destroy(elm_growth* g);
/* No candidates, all counters and the object's beam total back to zero. */
int elm_growth_reset(elm_ctx* ctx, elm_growth* g);
/* One observation (a call of one job): the resident scan at pose T16 (column-major).  stats (may be NULL): the observation's counts.
 * events (may be NULL): events[elm_scan_size(scan)], the through events of every beam in the resident scan's order, saturating at 65535.
 * ELM_ERR_INVALID: cfg.sub differs from the object's, a non-finite pose entry, a scan or object of another context, a batch in flight.
 * The object knows its exact candidate count after every call (elm_growth_cells with cap 0 returns it without a download).  A call with
 * count + (beams of the call) > capacity is refused with ELM_ERR_UNSUPPORTED before anything is launched, and so is a call that would
 * carry the 64-bit total of beams accumulated beyond 2^32 - 1: the table can never fill and no counter can wrap. */
int elm_growth_accumulate(elm_ctx* ctx, elm_growth* g, const elm_scan* scan, const double T16[16], const elm_growth_config* cfg,
                          elm_growth_stats* stats, uint16_t* events);
/* One call of n_jobs (1 .. 4096) observations: scans[j] at poses16 + 16 j.  Jobs may have any sizes, 0 included; the same scan may appear
 * several times.  stats (may be NULL): stats[n_jobs].  The counters afterwards do not depend on the order of the jobs. */
int elm_growth_accumulate_batch(elm_ctx* ctx, elm_growth* g, const elm_scan* const* scans, const double* poses16, int n_jobs,
                                const elm_growth_config* cfg, elm_growth_stats* stats);
/* The candidate cells in ascending (x, y, z) order (sorted on the host after the download): cells3 int32 [.][3], hit, through, sums3
 * uint64 [.][3]; min(cap, count) written, *n = count; each array may be NULL. */
int elm_growth_cells(elm_ctx* ctx, const elm_growth* g, int32_t* cells3, uint32_t* hit, uint32_t* through, uint64_t* sums3, size_t cap,
                     size_t* n);
/* The POINT of every appeared cell by `rule`, in the same order: xyz64 float64 [.][3]; min(cap, count) written, *n = count (xyz64 may be
 * NULL when cap = 0). */
int elm_growth_appeared_points(elm_ctx* ctx, const elm_growth* g, const elm_growth_rule* rule, double* xyz64, size_t cap, size_t* n);

/* ---------------------------------------------------------------- map growth: objects ------------- */
/* Which of the appeared cells belong together?  "map growth" ends at a bag of cells; here the cells are grouped into objects on the
 * device, against the growth object's own tables, and two maps lead back to the objects: candidate cell -> object and beam -> object.
 * Fed one scan into a fresh growth object and asked with the rule {1, 0, 26, 1}, the objects are the clusters of that scan's returns that
 * the map does not explain, and the beam map is the segmentation of the scan.
 *   MEMBER     a candidate cell with hit >= min_hit and hit >= hit_per_through * through (the product in 64 bits): elm_growth_rule's rule.
 *   ADJACENT   two cells a != b with d = b - a and max_r |d_r| <= 1 are adjacent under connectivity 6 when |d_x| + |d_y| + |d_z| <= 1,
 *              under 18 when that sum is <= 2, under 26 when it is <= 3.
 *   COMPONENT  an equivalence class of the member cells under the transitive closure of ADJACENT.  A cell that is not a member connects
 *              nothing.
 *   LABEL      of a component: its smallest member cell in (x, y, z) order.
 *   OBJECT     a component with n_cells >= min_cells.  A component below min_cells is SMALL: counted, not listed.
 *   ORDER      the objects are listed in ascending label order; an object's INDEX is its place in that list.
 * Every result is an integer and depends only on the set of candidate cells and their counters: not on the slot a cell occupies in the
 * table (which varies from run to run), the capacity, the order of the jobs that filled the table, or the search-index form. */
typedef struct elm_growth_object_rule {
    uint32_t min_hit, hit_per_through; /* which candidates are members: elm_growth_rule's rule */
    uint32_t connectivity;             /* 6, 18 or 26 */
    uint32_t min_cells;                /* >= 1; smaller components are SMALL */
} elm_growth_object_rule;
typedef struct elm_growth_object {     /* 80 bytes */
    int32_t  label[3];                 /* smallest member cell */
    uint32_t n_cells;
    int32_t  lo[3], hi[3];             /* bounding box in cells, inclusive */
    uint64_t hit, through;             /* sums over the member cells */
    uint64_t cell_sum[3];              /* sum over the member cells of (e_r + 2^20): the cell centroid, exactly */
} elm_growth_object;
typedef struct elm_growth_object_stats {
    uint32_t n_members;                /* member cells */
    uint32_t n_objects;                /* components listed */
    uint32_t n_small, n_small_cells;   /* small components and their cells: the objects' n_cells and n_small_cells add up to n_members */
    uint32_t max_cells;                /* n_cells of the largest component, listed or small; 0 without members */
    uint32_t _pad;
} elm_growth_object_stats;
/* min_hit 3, hit_per_through 4, connectivity 26, min_cells 1 -- starting points, not measured optima; with min_cells 1 the objects
 * partition the appeared cells */
void elm_growth_object_rule_default(elm_growth_object_rule* r);
/* Labels the member cells on the device and keeps the result with the growth object until the next elm_growth_accumulate,
 * elm_growth_accumulate_batch, elm_growth_reset or elm_growth_find_objects on it; while no result is held the three read calls below
 * return ELM_ERR_INVALID with a last_error text.  stats may be NULL.  The state it needs is allocated at the first call and freed by
 * elm_growth_destroy: a growth object that never asks pays nothing.  An object without candidates gives zero members and zero objects.
 * ELM_ERR_INVALID: a connectivity outside {6, 18, 26}, min_cells = 0, an object of another context, a batch in flight. */
int elm_growth_find_objects(elm_ctx* ctx, elm_growth* g, const elm_growth_object_rule* rule, elm_growth_object_stats* stats);
/* The objects in ascending label order: min(cap, count) written, *n = count (objs may be NULL when cap = 0). */
int elm_growth_objects(elm_ctx* ctx, const elm_growth* g, elm_growth_object* objs, size_t cap, size_t* n);
/* One value per candidate cell, in elm_growth_cells' order: the index of the object the cell is a member of, -2 for a member of a small
 * component, -1 for a cell that is not a member; min(cap, count) written, *n = count (obj may be NULL when cap = 0). */
int elm_growth_cell_objects(elm_ctx* ctx, const elm_growth* g, int32_t* obj, size_t cap, size_t* n);
/* One value per beam of the resident scan at pose T16, in the resident scan's order: obj[elm_scan_size(scan)].  The beam's end cell e is
 * formed exactly as "map growth" forms it.  If the beam is OBSERVING (cfg's window and origin, as in "map evidence"), every |e_r| < 2^20
 * and e is a member of a listed object, the value is that object's index; if e is a member of a small component, -2; otherwise -1.  The
 * map's table is not read.  ELM_ERR_INVALID: cfg.sub differs from the object's, a non-finite pose entry, a scan or object of another
 * context, a batch in flight. */
int elm_growth_beam_objects(elm_ctx* ctx, const elm_growth* g, const elm_scan* scan, const double T16[16], const elm_growth_config* cfg,
                            int32_t* obj);

/* ---------------------------------------------------------------- device map build ---------------- */
/* AddPoints, a prune and an incremental add as ONE build on the device.  The result is the map that
 *   elm_map_build(ctx, P, |P|, voxel_size, max_points_per_voxel, out)
 * returns, where P = the stored points of `base` with drop[i] == 0, in bucket order (voxels in first-seen order, insertion order inside a
 * voxel: the order of elm_map_download_points), followed by the n points of xyz -- the same elm_map_get_info, elm_map_download_points and
 * elm_map_download_voxels, byte for byte and in the same order, hence the same covariances, search indices and registrations afterwards.
 * The stored points of a map survive their own replay (all of them are kept, in their order, and so is any subset), and
 * AddPoints(A); AddPoints(B) equals one AddPoints(stored(A) ++ B): base and no drop is the reference's Update(points), base and drop a
 * prune.  base's points are read from HBM and never downloaded; base is not modified; voxel_size and the cap need not be base's.
 *   base   may be NULL (a build from xyz alone)
 *   drop   host, one byte per stored point of base in elm_map_download_points order; NULL: keep all; must be NULL when base is NULL
 *   xyz    host, packed float32, n points (may be NULL when n = 0)
 * The build's scratch memory (about 100 bytes per point of P) is released before return and is not part of device_bytes.
 * ELM_ERR_INVALID: ctx or out NULL, voxel_size <= 0 or NaN, max_points_per_voxel <= 0, drop without base, a base of another context,
 * a batch in flight.  ELM_ERR_UNSUPPORTED with a text in elm_last_error: a coordinate of P that is not finite or whose quotient by
 * voxel_size is not inside (-2^20, 2^20) (three 21-bit key fields; elm_map_build's cast of such a quotient is undefined or beyond any
 * map in use), more than 2^31 - 1 points in P, the lead of a device group, a context with a communicator or hook attached.  After any
 * refusal *out is NULL, nothing stays allocated and the context is usable. */
int elm_map_build_device(elm_ctx* ctx, const elm_map* base, const uint8_t* drop, const float* xyz, size_t n, double voxel_size,
                         int max_points_per_voxel, elm_map** out);
/* Device milliseconds (hipEvents on the context's stream) of the stages of the last successful elm_map_build_device or
 * elm_map_build_device_from of this thread on ctx: ms[0] base points compacted and xyz uploaded (or transformed), [1] key and insert, [2] voxel ids, [3] raw counts, [4] grouping (the sort), [5]
 * replay, [6] kept points and ranges written; the host's share (slot table, transfers of keys and ranges) is the call's wall clock less
 * their sum.  ELM_ERR_INVALID: no such build. */
#define ELM_BUILD_STAGES 7
int elm_map_build_device_stages(const elm_ctx* ctx, double ms[ELM_BUILD_STAGES]);

/* ---------------------------------------------------------------- device map build from resident sources */
/* The device build with both of its inputs produced on the device: which stored points of `base` stay is decided by a sphere, and the new
 * points are resident scans at their poses.  Nothing but the job table crosses the bus.  The result is the map that
 *   elm_map_build_device(ctx, base, drop, xyz, n, voxel_size, max_points_per_voxel, out)
 * returns -- byte for byte, in every sense given above -- for these drop and xyz:
 *   drop[i] = 0 iff keep_within == 0, or ((dx dx + dy dy) + dz dz) <= r2 with dx = x - keep_center[0], dy = y - keep_center[1],
 *       dz = z - keep_center[2] in float64, (x, y, z) the stored point's float32 coordinates widened, r2 = keep_radius_m * keep_radius_m
 *       computed once on the host; no fused multiply-add.  The sphere is closed.
 *   xyz = every job's resident points in device order (the order of elm_scan_download), the jobs in their order; each point becomes
 *       q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in float64 (the association of elm_evidence_accumulate's end points), rounded to float32
 *       (to nearest).
 *   base       may be NULL (a build from the scans alone); it is not modified
 *   scans      n_jobs resident scans; the same scan may appear several times; may be NULL when n_jobs = 0
 *   poses16    n_jobs column-major 4 x 4, map <- scan frame (what elm_evidence_accumulate takes); only [R | t] is read
 *   stats      may be NULL: the stored points of base kept / dropped, the points of all jobs, the points and voxels of the result
 * ELM_ERR_INVALID: ctx, src or out NULL, scans or poses16 NULL with n_jobs > 0, a NULL scan, voxel_size <= 0 or NaN,
 * max_points_per_voxel <= 0, a base or scan of another context, a batch in flight, n_jobs outside 0 .. 4096, a non-finite entry of
 * poses16, keep_center or keep_radius_m, a negative radius, keep_within not 0 or 1, keep_within == 1 without a base.
 * ELM_ERR_UNSUPPORTED with a text in elm_last_error: as elm_map_build_device, applied to the transformed points (a coordinate that is
 * not finite or whose quotient by voxel_size is not inside (-2^20, 2^20), more than 2^31 - 1 points, the lead of a device group, a
 * communicator or hook attached).  After any refusal *out is NULL, nothing stays allocated and the context is usable. */
typedef struct elm_build_sources {
    const elm_map* base;             /* may be NULL */
    int32_t keep_within;             /* 0: keep every stored point of base; 1: keep those within keep_radius_m of keep_center */
    double keep_center[3];
    double keep_radius_m;
    const elm_scan* const* scans;    /* n_jobs resident scans (may repeat) */
    const double* poses16;           /* n_jobs column-major 4x4, map <- scan frame */
    int32_t n_jobs;                  /* 0 .. 4096 */
} elm_build_sources;
typedef struct elm_build_sources_stats { uint64_t n_base_kept, n_base_dropped, n_scan_points, n_points, n_voxels; } elm_build_sources_stats;
int elm_map_build_device_from(elm_ctx* ctx, const elm_build_sources* src, double voxel_size, int max_points_per_voxel, elm_map** out,
                              elm_build_sources_stats* stats);

/* ---------------------------------------------------------------- LiDAR odometry on a rolling local map */
/* One object holds one local map (owned, device resident) and the pose history.  Every scan is registered against the local map
 * (elm_register_batch of the one resident scan) and, when it is a keyframe, inserted by elm_map_build_device_from: base = the current map,
 * the stored points farther than max_range_m from the new pose's translation forgotten, the scan added at the new pose.  No point crosses
 * the bus after the scan's own upload.  Poses are column-major 4 x 4, map <- scan frame.  The rules:
 *   first scan     no registration: registered = 0, is_success = 1, the pose is the guess (identity when T_guess is NULL), inserted = 1.
 *   later scans    one elm_register_batch against the current map from the guess (elm_odometry_predict when T_guess is NULL):
 *                  registered = 1, reg = its result.  is_success == 0: the step returns ELM_OK with that result and T = the result's
 *                  pose, inserts nothing and leaves the pose history untouched.
 *   keyframe test  insert iff sqrt((dx dx + dy dy) + dz dz) >= key_min_trans_m or ((R00 + R11) + R22 - 1) / 2 <= cos(key_min_rot_rad),
 *                  d = t_new - t_key and R = R_key^T R_new (R_ii = (K_0i N_0i + K_1i N_1i) + K_2i N_2i) against the last INSERTED pose.
 *                  With both thresholds 0 every scan is inserted; a threshold that should never fire alone is set large (pi for the
 *                  rotation), not 0.
 *   insert         elm_map_build_device_from(base = the map, keep_within = 1, keep_center = the new translation, keep_radius_m =
 *                  max_range_m, the one scan at the new pose); on the new map elm_map_set_index_build(ELM_INDEX_BUILD_DEVICE), then
 *                  elm_map_cal_point_cov_all(reg.gicp_cov_search_dist) for GICP, elm_map_cal_voxel_cov_all for VGICP / AVGICP; then the
 *                  old map is destroyed.  A failed build (its status is returned) leaves the old map and the history in place.
 *   history        the poses of the steps that succeeded, inserted or not.  Prediction is constant velocity in float64 on the host:
 *                  T_{k-1} (T_{k-2}^-1 T_{k-1}) with the rigid inverse [R^T, -R^T t]; with one pose that pose, with none the identity.
 *   scope          one rank only, as every query object: no device group's lead, no communicator or hook.
 * ELM_ERR_INVALID: a NULL argument (T_guess may be NULL), voxel_size <= 0 or NaN, max_points_per_voxel <= 0, max_range_m / key_min_trans_m
 * / key_min_rot_rad negative or not finite, reg.icp_method outside the four methods, a scan of another context, a non-finite guess, a
 * batch in flight, an object whose context is gone. */
typedef struct elm_odometry elm_odometry;
typedef struct elm_odometry_config {
    double voxel_size; int32_t max_points_per_voxel;   /* of the local map */
    double max_range_m;                                /* stored points farther than this from the new pose's translation are forgotten at an insert */
    double key_min_trans_m, key_min_rot_rad;           /* insert only when the pose moved this far from the last inserted one (0, 0: every scan) */
    elm_reg_config reg;                                /* method, gates, search distances: all four methods are legal */
} elm_odometry_config;
typedef struct elm_odometry_step {
    double T[16]; int32_t registered, is_success, inserted; elm_reg_result reg; elm_build_sources_stats build;
} elm_odometry_step;
/* voxel 1.0 m, cap 30, max_range_m 100, both key thresholds 0, reg = elm_reg_config_default */
void elm_odometry_config_default(elm_odometry_config* cfg);
int  elm_odometry_create(elm_ctx* ctx, const elm_odometry_config* cfg, elm_odometry** out);
void elm_odometry_destroy(elm_odometry* odom);
/* forgets the map and the history: the next scan is a first scan */
int  elm_odometry_reset(elm_odometry* odom);
int  elm_odometry_predict(const elm_odometry* odom, double T_guess[16]);
int  elm_odometry_step_scan(elm_odometry* odom, const elm_scan* scan, const double T_guess[16] /* NULL: predict */, elm_odometry_step* out);
/* owned by the object, valid until the next inserting step / reset / destroy; NULL before the first */
const elm_map* elm_odometry_map(const elm_odometry* odom);

/* ---------------------------------------------------------------- place recognition --------------- */
/* Have I been here before?  A places object holds, resident on the device, a database of binary scan DESCRIPTORS with a caller-given
 * int64 id each, and answers a query descriptor with the top entries of an EXACT search: every entry at every one of the 64 yaw shifts,
 * no prefilter and no tree.  One rank only.
 * THE DESCRIPTOR.  W = n_rings * n_layers words of 64 bits; word = ring * n_layers + layer, bit = sector (ELM_PLACES_SECTORS = 64, so a
 * yaw shift of the scan is a 64-bit rotate of every word).  Three float64 tables, computed once on the host (elm_places_tables):
 *   ring_edge2[i] = e_i * e_i, e_i = r_min_m + ((r_max_m - r_min_m) * i) / n_rings for i = 0 .. n_rings, e_n = r_max_m exactly;
 *   z_edge[j]     = z_min_m + ((z_max_m - z_min_m) * j) / n_layers for j = 0 .. n_layers, the last = z_max_m exactly;
 *   dir[k]        = (cos, sin)(2 pi k / 64): dir[0] = (1, 0); dir[1 .. 7] from libm; dir[8] = (c, c), c = cos(pi / 4) from libm;
 *                   dir[16 - k] = (dir[k].y, dir[k].x) for k = 0 .. 7; dir[k] = (-dir[k - 16].y, dir[k - 16].x) for k = 17 .. 63; zeros
 *                   are stored as +0.0.  So dir[k + 16] is exactly dir[k] turned a quarter, and an exact quarter turn of a scan,
 *                   (x, y) -> (-y, x), rotates every word of its descriptor left by exactly 16 bits.
 * A table that is not finite or not strictly increasing is ELM_ERR_INVALID.
 * One job is one resident scan with a LEVELLING pose T_level = [R | t] (sensor roll and pitch, and height: relocalization's T_tilt;
 * NULL: identity).  Per point p (float32 -> float64), all arithmetic float64 without contraction:
 *   q_r = ((R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r (the association of "map evidence");
 *   r2 = q_x q_x + q_y q_y; the ring is the i with ring_edge2[i] <= r2 < ring_edge2[i + 1];
 *   the layer is the j with z_edge[j] <= q_z < z_edge[j + 1];
 *   the sector is the smallest k with cross(dir[k], q) >= 0 and cross(dir[(k + 1) & 63], q) < 0, cross(d, q) = d_x q_y - d_y q_x;
 *   a point without a ring, a layer or a sector (a NaN, q_x = q_y = 0) is dropped; every other point sets its bit.
 * THE MATCH, in integers.  For a query a and an entry b and a shift k in 0 .. 63: inter(k) = sum over the words of
 * popcount(a_w & rotl64(b_w, k)).  The pair's result is the largest inter at the smallest such k, and
 *   dice_q16 = ((uint64)inter << 17) / (n_bits(a) + n_bits(b)), 0 when that sum is 0 (65536 = identical);
 *   yaw_rad  = -2 pi k / 64 wrapped to (-pi, pi]: -(2 pi k) / 64 for k < 32, (2 pi (64 - k)) / 64 otherwise; the yaw of the query's
 *              sensor relative to the entry's, T_query ~ T_entry * Rz(yaw_rad).
 * THE SELECTION, per query: of the entries with dice_q16 >= min_dice_q16 whose id lies outside the closed range [exclude_id_lo,
 * exclude_id_hi] (lo > hi excludes nothing), the first top_k by dice descending, then entry index ascending.
 * OR, integer sums and maxima of distinct keys have no order to protect: the same bytes on every run and for every job order. */
#define ELM_PLACES_SECTORS 64
#define ELM_PLACES_MAX_TOP_K 16
typedef struct elm_places elm_places;
typedef struct elm_places_config {
    int32_t n_rings;        /* 1 .. 32 */
    int32_t n_layers;       /* 1 .. 16 */
    double r_min_m, r_max_m; /* the rings cut [r_min_m, r_max_m) evenly in the levelled xy range */
    double z_min_m, z_max_m; /* the layers cut [z_min_m, z_max_m) evenly in the levelled height */
} elm_places_config;
typedef struct elm_places_stats {
    uint32_t n_points;      /* the scan's points */
    uint32_t n_used;        /* the points that set a bit */
    uint32_t n_bits;        /* the popcount of the descriptor */
} elm_places_stats;
typedef struct elm_places_query_config {
    int32_t top_k;          /* 1 .. ELM_PLACES_MAX_TOP_K */
    uint32_t min_dice_q16;
    int64_t exclude_id_lo, exclude_id_hi;
} elm_places_query_config;
typedef struct elm_place_match {
    uint32_t dice_q16;
    uint16_t inter, shift;
} elm_place_match;
typedef struct elm_place_candidate {
    uint32_t entry;         /* index in the database */
    uint32_t dice_q16;
    int64_t id;
    uint16_t inter, shift;
    uint32_t _pad;
    double yaw_rad;
} elm_place_candidate;
/* 16 rings over 2 .. 42 m, 8 layers over -3 .. 9 m */
void elm_places_config_default(elm_places_config* c);
/* The tables of cfg, each when not NULL: ring_edge2[n_rings + 1], z_edge[n_layers + 1], dir[64][2].  Host only. */
int elm_places_tables(const elm_places_config* cfg, double* ring_edge2, double* z_edge, double* dir);
/* An empty database of `capacity` entries (1 .. 65536), fixed for its life.  ELM_ERR_UNSUPPORTED on a device group's lead or with a
 * communicator / hook attached, here and in every call below that takes ctx. */
int elm_places_create(elm_ctx* ctx, const elm_places_config* cfg, int capacity, elm_places** out);
void elm_places_destroy(elm_places* pl);
/* the database empty again */
int elm_places_reset(elm_ctx* ctx, elm_places* pl);
int elm_places_size(elm_ctx* ctx, const elm_places* pl, size_t* n);
/* The descriptors of n_jobs (1 .. 4096) resident scans, scans[j] levelled by levels16 + 16 j (column-major; levels16 NULL: identity),
 * into words_out[n_jobs][W] and, when not NULL, stats[n_jobs].  The database is not touched.  Jobs may have any sizes, 0 included; the
 * same scan may appear several times.  ELM_ERR_INVALID: a non-finite level entry, a scan or object of another context, a batch in flight. */
int elm_places_describe(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, int n_jobs, uint64_t* words_out,
                        elm_places_stats* stats);
/* The same descriptors appended as n_jobs entries in job order with ids[j].  A call that would overfill the database is refused with
 * ELM_ERR_UNSUPPORTED and leaves it as it was. */
int elm_places_add(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, const int64_t* ids, int n_jobs,
                   elm_places_stats* stats);
/* n descriptors from the host, words[n][W], appended (a saved database loaded again; n = 0 is allowed). */
int elm_places_add_words(elm_ctx* ctx, elm_places* pl, const uint64_t* words, const int64_t* ids, size_t n);
/* Entries first .. first + count - 1, each output when not NULL: words[count][W], ids[count], n_bits[count].  ELM_ERR_INVALID beyond
 * the database's size. */
int elm_places_download(elm_ctx* ctx, const elm_places* pl, size_t first, size_t count, uint64_t* words, int64_t* ids, uint32_t* n_bits);
/* n_queries (1 .. 4096) descriptors words[n_queries][W] against every entry: cands[n_queries][ELM_PLACES_MAX_TOP_K] of which the first
 * n_cands[q] are written for query q under query_cfg[q]; matches, when not NULL: [n_queries][size], every (query, entry) pair.  An
 * empty database answers no candidates. */
int elm_places_match_words(elm_ctx* ctx, elm_places* pl, const uint64_t* words, int n_queries, const elm_places_query_config* query_cfg,
                           elm_place_candidate* cands, int32_t* n_cands, elm_place_match* matches);
/* The same on resident scans: described into scratch (stats, when not NULL: [n_queries]), then matched. */
int elm_places_query(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, int n_queries,
                     const elm_places_query_config* query_cfg, elm_place_candidate* cands, int32_t* n_cands, elm_place_match* matches,
                     elm_places_stats* stats);

/* ---------------------------------------------------------------- pose graph ---------------------- */
/* Given odometry constraints and loop constraints, the corrected poses.  A pose graph object holds, resident on the device, NODES (poses)
 * and relative-pose EDGES, linearizes them on the GPU, solves the damped normal equations by block-Jacobi preconditioned conjugate
 * gradients on the GPU, and runs Levenberg-Marquardt around that.  One rank only.  Everything is float64 without contraction.
 * NODES.  T_v = [R_v | t_v], world <- node, column-major 4 x 4 here, the twelve pose rows on the device; a `fixed` flag each.
 * TANGENT AND RETRACTION.  x = [v; w], translation first: R <- R Exp(w), t <- t + R v, Exp = Rodrigues (zero -> identity).
 * EDGES.  (i, j, Z, Omega): Z ~ T_i^-1 T_j; Omega 6 x 6, symmetric, row-major, in the order of x.  i == j, an index past the node count,
 * a non-finite entry or an Omega that is not exactly symmetric is ELM_ERR_INVALID; duplicate edges and i > j are legal.
 * RESIDUAL.  d = R_i^T (t_j - t_i), R_E = R_Z^T (R_i^T R_j), r = [r_t; r_R] = [R_Z^T (d - t_Z); Log(R_E)].
 * LOG goes through the unit quaternion (w, vec) of the matrix, signed to w >= 0: n = |vec|, theta = 2 atan2(n, w),
 * phi = vec (theta / n); below n = 1e-8, phi = 2 vec.  Log(I) is exactly 0.
 * JACOBIANS, rows in the order of r, columns in the order of x:
 *   A = dr/dx_i = [ -R_Z^T   R_Z^T [d]x ;  0  -J^-1(phi) R_j^T R_i ]      B = dr/dx_j = [ R_E  0 ;  0  J^-1(phi) ]
 *   J^-1(phi) = I + [phi]x / 2 + c(theta) [phi]x^2,  c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta).
 * Built: the second term of c is evaluated as w / (2 theta n) with the quaternion's w = cos(theta / 2), n = sin(theta / 2) -- the same
 * number, (1 + cos) / sin = cot(theta / 2), without the cancellation of 1 + cos theta near pi; below theta = 1e-2 c is its series
 * 1/12 + theta^2/720 + theta^4/30240 (both branches good to 1e-11 relative there).  The formulas agree with central differences of the
 * residual (tests/test_posegraph_abi.py).
 * ROBUST WEIGHT.  Huber on s_e = r^T Omega r: w_e = 1 if s_e <= k^2 else k / sqrt(s_e); cost rho_e = s_e if s_e <= k^2 else
 * 2 k sqrt(s_e) - k^2.  huber_k = 0 turns it off.  s_e == k^2 is an inlier.
 * NORMAL EQUATIONS.  H_vv = sum_e w_e X^T Omega X, H_ij = w_e A^T Omega B, g_v = sum_e w_e X^T Omega r (X = A for v = i, B for v = j);
 * every per-node sum runs over the node's incident edges IN ASCENDING EDGE INDEX, one addition per edge.  That order makes the results
 * the same bytes from run to run; they are NOT invariant under a permutation of the edges.
 * FIXED NODES have delta = 0 and their rows and columns are left out; a free node whose diagonal block is all zero (no edges) is
 * treated as fixed for the solve and stays where it is.  A connected component without a fixed node is the caller's business: with
 * lambda > 0 the damping keeps the solve defined and the component's gauge floats; with lambda = 0 the system is singular.
 * STEP.  (H + lambda diag(H)) delta = -g by preconditioned conjugate gradients from delta = 0, the preconditioner the inverse of the
 * node's damped diagonal block; it stops at sqrt(r^T M^-1 r) <= pcg_rel_tol sqrt(r0^T M^-1 r0) or at pcg_max_iterations;
 * pcg_rel_tol = 0 runs exactly pcg_max_iterations.  Every inner product is a fixed tree over partial sums whose number and order depend
 * on the node count and the edge set alone.
 * OUTER LOOP (elm_posegraph_optimize).  F = sum rho_e at the poses; F == 0 stops at once.  Per solve: solve, retract into trial poses,
 * F_new there.  F_new < F: accept, lambda <- max(lambda lambda_down, lambda_min), then stop on F_new == 0, on
 * F - F_new <= cost_rel_tol F, on max |delta| <= step_tol, on the solve count, else linearize again.  Otherwise: reject, the poses and
 * the linearization stay; stop on max |delta| <= step_tol or when lambda is already lambda_max; else lambda <- min(lambda lambda_up,
 * lambda_max) and only the damped diagonal and its inverses are redone.
 * PRECONDITIONER.  The block-Jacobi M above is the default.  The CHAIN preconditioner -- M block tridiagonal over the index chain
 * v, v + 1, applied by a parallel block cyclic reduction on the GPU -- is chosen per object; its definition and its two calls,
 * elm_posegraph_set_preconditioner / elm_posegraph_get_preconditioner, are in elimaloc_hip_posegraph_precond.h, included below.  With
 * the default every result of every call here is what it was before that choice existed, byte for byte.
 * INITIALIZATION.  A start far from the linear regime is first brought near it by two linear problems, rotations and then translations,
 * solved by the same conjugate gradients: elm_posegraph_initialize, in elimaloc_hip_posegraph_init.h, included below.
 * PRIORS.  Besides the relative-pose edges a node may carry absolute factors -- a measured pose or position in the world frame, with a
 * lever arm and a positive semi-definite information (GNSS, map matches): elimaloc_hip_posegraph_prior.h, included below.  With no
 * prior in the object every result of every call here is what it was before they existed, byte for byte.  The initialization that
 * uses them (a graph held by priors alone, without a fixed node): elimaloc_hip_posegraph_init_prior.h, included below.
 * LIMITS.  node_capacity 1 .. 2^20, edge_capacity 1 .. 2^22, fixed for the object's life; device memory about 1.8 KB per node (1.2 KB
 * of it the chain preconditioner's factor: per node and level of the reduction the inverse pivot block, the two coupling blocks and
 * the running coupling, the levels above the first adding 1/255) and 1.7 KB per edge of capacity. */
typedef struct elm_posegraph elm_posegraph;
#define ELM_POSEGRAPH_MAX_NODES (1 << 20)
#define ELM_POSEGRAPH_MAX_EDGES (1 << 22)
#define ELM_PG_STOP_MAX_ITERATIONS 1
#define ELM_PG_STOP_COST_TOL 2
#define ELM_PG_STOP_STEP_TOL 3
#define ELM_PG_STOP_LAMBDA_MAX 4
#define ELM_PG_STOP_COST_ZERO 5
typedef struct elm_posegraph_config {
    int32_t max_iterations;     /* solves, >= 1 */
    int32_t pcg_max_iterations; /* >= 1 */
    int32_t pcg_check_every;    /* PCG iterations queued between two reads of the device's done word, >= 1 */
    int32_t _pad;
    double lambda_init, lambda_up, lambda_down, lambda_min, lambda_max;
    double cost_rel_tol, step_tol, pcg_rel_tol, huber_k;
} elm_posegraph_config;
typedef struct elm_posegraph_linearize_stats {
    double chi2;          /* sum s_e */
    double cost;          /* sum rho_e */
    double grad_inf_norm; /* max |g_v| over the nodes the solve moves */
    int64_t n_outliers;   /* edges with w_e < 1 */
} elm_posegraph_linearize_stats;
typedef struct elm_posegraph_solve_stats {
    int32_t iterations;
    int32_t converged;    /* the stop test was met (never with pcg_rel_tol = 0) */
    double rel_residual;  /* sqrt(r^T M^-1 r) / sqrt(r0^T M^-1 r0) of the recurrence; 0 when the right-hand side is 0 */
} elm_posegraph_solve_stats;
typedef struct elm_posegraph_result {
    int32_t solves, accepted, rejected, stop_reason; /* ELM_PG_STOP_* */
    double cost_initial, cost_final, lambda_final;
    int64_t pcg_iterations_total;
} elm_posegraph_result;
typedef struct elm_posegraph_trace {
    double cost;    /* F_new of the solve's trial poses */
    double lambda;  /* the solve's damping */
    int32_t accepted, pcg_iterations;
} elm_posegraph_trace;
/* 20 solves, lambda 1e-4 (x 10 up, x 0.1 down, in [1e-12, 1e8]), cost_rel_tol 1e-12, step_tol 1e-10, PCG to 1e-8 in at most 2000
 * iterations checked every 32, Huber off */
void elm_posegraph_config_default(elm_posegraph_config* c);
/* An empty graph.  ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached, here and in every call below
 * that takes ctx; ELM_ERR_INVALID while a batch is in flight. */
int elm_posegraph_create(elm_ctx* ctx, int node_capacity, int edge_capacity, elm_posegraph** out);
void elm_posegraph_destroy(elm_posegraph* pg);
/* no nodes, no edges */
int elm_posegraph_reset(elm_ctx* ctx, elm_posegraph* pg);
int elm_posegraph_size(elm_ctx* ctx, const elm_posegraph* pg, size_t* n_nodes, size_t* n_edges);
/* n nodes appended: poses16[n][16] column-major, finite; fixed[n] (NULL: all free).  A call that would overfill is ELM_ERR_UNSUPPORTED
 * and changes nothing (as for edges). */
int elm_posegraph_add_nodes(elm_ctx* ctx, elm_posegraph* pg, const double* poses16, const uint8_t* fixed, size_t n);
int elm_posegraph_set_poses(elm_ctx* ctx, elm_posegraph* pg, size_t first, size_t count, const double* poses16);
int elm_posegraph_get_poses(elm_ctx* ctx, const elm_posegraph* pg, size_t first, size_t count, double* poses16);
int elm_posegraph_set_fixed(elm_ctx* ctx, elm_posegraph* pg, size_t first, size_t count, const uint8_t* fixed);
/* n edges appended: i[n], j[n], Z16[n][16] column-major, info36[n][36] row-major */
int elm_posegraph_add_edges(elm_ctx* ctx, elm_posegraph* pg, const int32_t* i, const int32_t* j, const double* Z16, const double* info36, size_t n);
/* Residuals, Jacobians, weights and the normal equations' blocks at the current poses; stats when not NULL.  huber_k >= 0. */
int elm_posegraph_linearize(elm_ctx* ctx, elm_posegraph* pg, double huber_k, elm_posegraph_linearize_stats* stats);
/* The current linearization, each output when not NULL: r[E][6], A[E][36], B[E][36], s[E], w[E], grad[N][6] (g_v as summed, for
 * fixed nodes too), diag[N][36] (H_vv undamped).  ELM_ERR_INVALID without one (the graph changed since, or never linearized). */
int elm_posegraph_download_linearization(elm_ctx* ctx, const elm_posegraph* pg, double* r, double* A, double* B, double* s, double* w,
                                         double* grad, double* diag);
/* The step of the current linearization: delta[N][6] (when not NULL) and stats (when not NULL).  lambda >= 0, pcg_rel_tol >= 0,
 * pcg_max_iterations >= 1.  The PCG iterations are queued pcg_check_every = 32 at a time. */
int elm_posegraph_solve(elm_ctx* ctx, elm_posegraph* pg, double lambda, double pcg_rel_tol, int pcg_max_iterations, double* delta,
                        elm_posegraph_solve_stats* stats);
/* Levenberg-Marquardt from the current poses, which it replaces.  ELM_ERR_INVALID: no fixed node at all, a bad config.  trace, when not
 * NULL: the first trace_cap solves. */
int elm_posegraph_optimize(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_config* cfg, elm_posegraph_result* result,
                           elm_posegraph_trace* trace, int trace_cap);
/* The residual and Jacobians of one edge, each output when not NULL: r[6], A[36], B[36] row-major.  Host only: the same code the kernel
 * runs, compiled for the host. */
int elm_posegraph_edge_terms(const double Ti16[16], const double Tj16[16], const double Z16[16], double* r, double* A, double* B);
#ifdef __cplusplus
}
#endif
#include "elimaloc_hip_posegraph_precond.h"
#include "elimaloc_hip_posegraph_init.h"
#include "elimaloc_hip_loops.h"
#include "elimaloc_hip_loopcov.h"
#include "elimaloc_hip_posegraph_cov.h"
#include "elimaloc_hip_posegraph_prior.h"
#include "elimaloc_hip_posegraph_init_prior.h"
#include "elimaloc_hip_reginfo.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- device index build -------------- */
/* The P2P / GICP cell grid of a map (dense or two-level) is laid out on the host by default: the stored points come down, are
 * counting-sorted by cell on one thread and go up again.  With ELM_INDEX_BUILD_DEVICE the same grid is built on the device from the stored
 * points where they lie: the box of half-voxel cells (six words come down), the entry of every point, the counts, a stable radix sort
 * of (entry, point number) by entry, the block starts (one word comes down: the block count), padding and fill.  The arrays it leaves
 * -- block starts, blocks, slot points, tile table -- and every field of the map's view are byte for byte the host build's, so
 * elm_map_get_info (but for layout_flags bit 9), registrations and elm_map_get_correspondences are too.  WHICH form a map gets is decided
 * by the same host arithmetic on the same numbers (ELM_GRID as ever); the device producer drops the host-memory term of the byte budget
 * and adds its scratch (16 bytes per point, 1 KB per 1024 points for the sort's histogram, 12 bytes per tile of the two-level form; no
 * word per entry beyond the table that becomes grid_start).  When that scratch is not affordable, a device allocation fails, or a size
 * passes the device kernels' 32-bit indices (2^31 - 1 points, 0xF0000000 entries), the host producer builds the same form and bit 9 stays
 * clear.  The preference is stored on the map and governs every later build of its P2P / GICP search index (the lazy build at the first
 * registration and elm_map_build_neighbourhoods); the voxel-mean lists and the neighbourhood lists are host builds either way.
 *   ELM_OK               also when the index is already built: nothing changes
 *   ELM_ERR_INVALID      map NULL, where not one of the two values
 *   ELM_ERR_UNSUPPORTED  (text in elm_last_error) a map with replicas, the lead of a device group, a communicator or hook attached */
#define ELM_INDEX_BUILD_HOST 0
#define ELM_INDEX_BUILD_DEVICE 1
int elm_map_set_index_build(elm_map* map, int where);
/* Device milliseconds of the stages of the map's device index build: [0] box, [1] entries and counts (two-level form: with the tile
 * table), [2] sort, [3] block starts, [4] padding and fill.  ELM_ERR_INVALID: the map's grid was not built on the device. */
#define ELM_INDEX_STAGES 5
int elm_map_index_build_stages(const elm_map* map, double ms[ELM_INDEX_STAGES]);
/* The cell grid as it lies on the device (whoever built it).  desc gets the fields of the map's view and the full counts; each array
 * may be NULL, and at most its cap entries are written: start n_start_words words, blocks12 n_blocks x 12 floats (x[4] y[4] z[4]; cap
 * in blocks), slot_point 4 * n_blocks words (cap in words), tiles2 n_tiles x 2 words (cap in tiles; n_tiles = 0 for the dense form).
 * Does not build anything: ELM_ERR_UNSUPPORTED when the map has no cell grid (not built yet, or it has neighbourhood lists). */
typedef struct elm_cell_grid_desc {
    int32_t gx0, gy0, gz0, gnx, gny, gnz; /* the box of cells (two-level form: gnx, gny rounded up to whole tiles) */
    int32_t vx0, vy0, vz0, vnx, vny, vnz; /* dense form: the statistics box of voxels */
    int32_t gtny;
    int32_t grid_tiled;
    int32_t grid_wide;
    uint32_t grid_nslots;
    uint64_t n_start_words;
    uint64_t n_blocks;
    uint64_t n_tiles;
} elm_cell_grid_desc;
int elm_map_download_cell_grid(const elm_map* map, elm_cell_grid_desc* desc, uint32_t* start, size_t start_cap, float* blocks12, size_t block_cap,
                               uint32_t* slot_point, size_t slot_cap, uint32_t* tiles2, size_t tile_cap);

/* ---------------------------------------------------------------- deskew -------------------------- */
/* Tables produced by ImuDeskewInfo / OdomDeskewInfo (pcm.cpp:533-729). */
typedef struct elm_deskew_tables {
    double d_time_scan_cur;     /* pcm.cpp:474/481 */
    double d_time_scan_end;     /* pcm.cpp:475/480 */
    int32_t i_imu_pointer_cur;  /* last valid table index (pcm.cpp:580) */
    int32_t b_run_deskew;       /* loc.ini:86 */
    int32_t b_is_imu_available; /* pcm.cpp:584 */
    int32_t b_is_odom_available;/* pcm.cpp:728 */
    float f_odom_incre_x, f_odom_incre_y, f_odom_incre_z; /* pcm.cpp:725 */
    float _pad;
    const double* vec_d_imu_time;  /* [i_imu_pointer_cur + 1] host pointers */
    const double* vec_d_imu_rot_x;
    const double* vec_d_imu_rot_y;
    const double* vec_d_imu_rot_z;
} elm_deskew_tables;

/* The per-point loop of DeskewPointCloud (pcm.cpp:498-525 -> DeskewPoint :780-824) as one HIP kernel.
 * xyz: n*3 float32, rel_time: n float32 (already rebased as pcm.cpp:483-485), xyz_out: n*3 float32 (host).
 * Returns ELM_OK and *ok = 0 when IMU or odom tables are unavailable (pcm.cpp:494-496, nothing written). */
int elm_deskew(elm_ctx* ctx, const float* xyz, const float* rel_time, size_t n, const elm_deskew_tables* tab,
               float* xyz_out, int* ok);
/* The same per-point loop followed by VoxelHashMap::VoxelDownsample (vhm.hpp:260-283: the first point of every floor-keyed
 * voxel of edge voxel_size) fused on the device: the undistorted cloud never leaves HBM and comes back as a resident scan
 * (kept points in input order) for elm_register_batch; release it with elm_scan_destroy.  *ok as elm_deskew (*scan_out is
 * NULL when 0).  ELM_ERR_UNSUPPORTED when |coordinate / voxel_size| >= 2^20 (use elm_deskew + elm_voxel_downsample). */
int elm_deskew_downsample(elm_ctx* ctx, const float* xyz, const float* rel_time, size_t n, const elm_deskew_tables* tab,
                          double voxel_size, elm_scan** scan_out, int* ok);
/* Host-side table preparation, same arithmetic as the reference (doubles for the IMU table, float32
 * PCL/Eigen transforms for the odometry increment).
 * imu: n_imu rows (t, wx, wy, wz) already rotated into the ego frame (pcm.cpp:328).
 * odom: n_odom rows of 14 doubles (t, px,py,pz, qx,qy,qz,qw, vx,vy,vz, wx,wy,wz).
 * front_time/back_time: time field of the first/last raw point; stamp: message stamp - lidar_time_delay. */
int elm_deskew_prepare(const double* imu4, size_t n_imu, const double* odom14, size_t n_odom, double stamp,
                       float front_time, float back_time, int lidar_scan_time_end, int run_deskew,
                       double* tab_time, double* tab_rx, double* tab_ry, double* tab_rz, size_t tab_cap,
                       elm_deskew_tables* out);

/* ---------------------------------------------------------------- caller glue (host) -------------- */
/* The steps of PcmMatching::CallbackPointCloud / CallbackInitialPose either side of the device path (SURVEY.md 8
 * rows f2 / f4), in the reference's float32 / float64 arithmetic.  Host functions, no GPU needed. */
/* FilterPointsByDistance (pcm.cpp:451-465): drops points farther than max_dist (float norm). time may be NULL. */
int elm_filter_points_by_distance(const float* xyz, const float* time, size_t n, double max_dist, float* xyz_out,
                                  float* time_out, size_t* n_out);
/* VoxelHashMap::VoxelDownsample (vhm.hpp:260-283): index of the first point of every floor-keyed voxel, in input
 * order (the reference emits unordered_map order; only the set is contractual). */
int elm_voxel_downsample(const float* xyz, size_t n, double voxel_size, int64_t* keep_idx, size_t* n_keep);
/* GetInterpolatedPose (pcm.cpp:933-1045): odom rows as in elm_deskew_prepare; T_out = Eigen::Affine3f matrix,
 * column-major; *ok = 0 when no odometry at or before the time exists. */
int elm_get_interpolated_pose(const double* odom14, size_t n_odom, double d_cur_time, float T_out[16], int* ok);
/* Registration::CalFramePointCov / CalPointCov (registration.hpp:186-217; called at registration.cpp:302-305 under use_radar_cov): the
 * covariance term R S of every source point from its position (map frame under the initial guess at the call site) and the range /
 * azimuth / elevation spreads.  cov9: n column-major 3x3 (not symmetric).  Host arithmetic (glibc sin / cos / atan2); elm_register
 * evaluates the same formula inside its radar kernel with the device's math library: the two agree to a few ulp, not bit for bit, so a
 * RunRegister re-assembled from this call + GetCorrespondences* + AlignCloudsLocal* under use_radar_cov follows elm_register to the
 * tolerance of the sums (1e-9; an ill-conditioned first-iteration metric amplifies the difference), not to the last bit. */
int elm_cal_frame_point_cov(const double* xyz, size_t n, double range_var_m, double azim_var_deg, double ele_var_deg, double* cov9);

/* Covariance of the published odometry (PublishPcmOdom pcm.cpp:1082-1098, NormalizeCovariance pcm.hpp:248-268):
 * cov_out is the row-major 6x6 of nav_msgs/Odometry.pose.covariance. */
int elm_shape_odom_covariance(const double local_cov[36], const double icp_ego_pose[16], double d_icp_pose_std_m,
                              double cov_out[36]);

/* ---------------------------------------------------------------- CPU EKF (host) ------------------ */
/* Plain-CPU counterpart of the reference's 27-state EKF (ekf_localization/src/ekf_algorithm.cpp) -- SURVEY.md 8 row f1.
 * north_star keeps the filter on the CPU; these calls close the config-5 stream (ICP pose -> EKF update -> next seed).
 * Built: Init, RunPredictionImu (+ ComplementaryKalmanFilter), RunGnssUpdate (all sources incl. PCM / PCM_INIT),
 * GetCurrentState, and the node's CallbackPcmOdom / GnssTimeCompensation / state deque.  ZUPT, CAN update and IMU-mount
 * calibration (off in the shipped localization.ini) return ELM_ERR_UNSUPPORTED. */
typedef struct elm_ekf elm_ekf;
enum { ELM_GNSS_NOVATEL = 0, ELM_GNSS_NAVSATFIX = 1, ELM_GNSS_BESTPOS = 2, ELM_GNSS_PCM = 3, ELM_GNSS_PCM_INIT = 4 }; /* ls.hpp:28 */
typedef struct elm_ekf_config { /* [ekf_localization] keys of config/localization.ini:15-75 */
    double imu_gravity;
    int32_t imu_estimate_gravity, imu_estimate_calibration, use_zupt, use_complementary_filter, gps_type, _pad;
    double ekf_init_x_m, ekf_init_y_m, ekf_init_z_m, ekf_init_roll_deg, ekf_init_pitch_deg, ekf_init_yaw_deg;
    double state_std_pos_m, state_std_rot_deg, state_std_vel_mps, state_std_gyro_dps, state_std_acc_mps;
    double imu_std_gyro_dps, imu_std_acc_mps, ekf_imu_bias_cov_gyro, ekf_imu_bias_cov_acc;
    double gnss_min_cov_x_m, gnss_min_cov_y_m, gnss_min_cov_z_m, gnss_min_cov_roll_deg, gnss_min_cov_pitch_deg, gnss_min_cov_yaw_deg;
    double can_vel_scale_factor, ekf_can_meas_uncertainty_vel_mps, ekf_can_meas_uncertainty_yaw_rate_deg; /* RunCanUpdate */
} elm_ekf_config;
typedef struct elm_ekf_state { /* EkfState (ls.hpp) + covariance, state order of ekf_algorithm.hpp:41-69 */
    double x[27];            /* rotation slots (3..5, 24..26) are 0: the attitude lives in the quaternions */
    double rot_xyzw[4], imu_rot_xyzw[4];
    double P[27 * 27];       /* row-major */
    double timestamp;
    int32_t b_state_initialized, b_yaw_initialized, b_rotation_stabilized, b_state_stabilized, b_pcm_init_on_going, _pad;
} elm_ekf_state;
typedef struct elm_ego_state { /* the EgoState fields GetCurrentState fills (ekfa.cpp:778-833) */
    double timestamp, x_m, y_m, z_m, roll_rad, pitch_rad, yaw_rad, roll_vel, pitch_vel, yaw_vel, vx, vy, vz, ax, ay, az;
    double x_cov_m, y_cov_m, z_cov_m, roll_cov_rad, pitch_cov_rad, yaw_cov_rad;
} elm_ego_state;
void elm_ekf_config_default(elm_ekf_config* cfg);
int elm_ekf_create(const elm_ekf_config* cfg, elm_ekf** out);
void elm_ekf_destroy(elm_ekf* ekf);
/* RunPredictionImu (ekfa.cpp:167-316): gyro / acc already rotated into the ego frame (ImuStructConverter) */
int elm_ekf_predict_imu(elm_ekf* ekf, double timestamp, const double gyro[3], const double acc[3], int* predicted);
/* RunPrediction (ekfa.cpp:81-165): the constant-velocity model of use_imu = 0 (ekfl.cpp:204-216) */
int elm_ekf_predict(elm_ekf* ekf, double timestamp, int* predicted);
/* RunCanUpdate + ZuptCan (ekfa.cpp:434-506, 567-587): vehicle-frame velocity and angular rate (the node fills vel[0], gyro[2]) */
int elm_ekf_update_can(elm_ekf* ekf, double timestamp, const double vel[3], const double gyro[3], int* updated);
/* RunGnssUpdate (ekfa.cpp:318-432): pos_cov / rot_cov row-major 3x3 */
int elm_ekf_update_pose(elm_ekf* ekf, double timestamp, const double pos[3], const double quat_xyzw[4], const double pos_cov[9],
                        const double rot_cov[9], int source, int* updated);
/* CallbackPcmOdom / CallbackPcmInitOdom (ekfl.cpp:147-220): odometry pose + row-major 6x6 covariance, time-compensated
 * against the published state history (GnssTimeCompensation ekfl.cpp:323-394) */
int elm_ekf_update_pcm_odom(elm_ekf* ekf, double stamp, const double pos[3], const double quat_xyzw[4],
                            const double covariance36[36], int source, int* updated);
/* GeographicLib::LocalCartesian(ref).Forward (ekfl.cpp:643-648): WGS84 geodetic -> east / north / up metres at the reference point */
int elm_gps_project(double ref_lat_deg, double ref_lon_deg, double ref_alt_m, double lat_deg, double lon_deg, double alt_m, double xyz[3]);
/* CallbackNavsatFix (ekfl.cpp:92-125): position_covariance = the message's row-major 3x3 (its diagonal holds standard deviations, which
 * the node squares); use_gps / gnss_uncertainty_max_m = the [ekf_localization] keys use_gps / gnss_uncertainy_max_m */
int elm_ekf_update_navsatfix(elm_ekf* ekf, double stamp, double lat_deg, double lon_deg, double alt_m, const double position_covariance[9],
                             double ref_lat_deg, double ref_lon_deg, double ref_alt_m, int use_gps, double gnss_uncertainty_max_m,
                             double pos_out[3], int* updated);
int elm_ekf_get_state(elm_ekf* ekf, elm_ekf_state* out);
/* GetCurrentState + the state-history upkeep of PublishInThread (ekfl.cpp:397-410); call after every prediction */
int elm_ekf_publish(elm_ekf* ekf, elm_ego_state* out);

/* ---------------------------------------------------------------- formats (host) ------------------ */
/* On-disk / wire formats either side of the path so the reference's own map, localization.ini and
 * calibration.ini drive the drop-in. */
typedef struct elm_ini elm_ini;
/* IniParser::ParseConfig rules (bsw/system/ini_parser/ini_parser.cpp:41-225 over SimpleIni): getters return 1 = found,
 * 0 = key missing (output untouched), <0 = error.  Numbers use atoi/atof, so "5.0 ; comment" reads as 5.0. */
int elm_ini_load(const char* path, elm_ini** out);
void elm_ini_destroy(elm_ini* ini);
int elm_ini_get_string(const elm_ini* ini, const char* section, const char* key, char* buf, size_t cap);
int elm_ini_get_int(const elm_ini* ini, const char* section, const char* key, int* out);
int elm_ini_get_bool(const elm_ini* ini, const char* section, const char* key, int* out); /* atoi(v) > 0 */
int elm_ini_get_double(const elm_ini* ini, const char* section, const char* key, double* out);
int elm_ini_get_array(const elm_ini* ini, const char* section, const char* key, double* out, size_t cap, size_t* n);

typedef struct elm_pcm_node_config { /* PcmMatchingConfig fields the pipeline reads (pcm_matching_config.hpp; pcm.cpp:152-170) */
    char lidar_type[32];          /* "ouster" selects OusterCloudmsg2cloud */
    int32_t lidar_scan_time_end, pcm_voxel_max_point, run_deskew, input_index_sampling;
    double lidar_time_delay, pcm_voxel_size, input_max_dist, input_voxel_ds_m;
    double tf_ego_to_lidar[16];   /* column-major */
} elm_pcm_node_config;
void elm_pcm_node_config_default(elm_pcm_node_config* cfg);
/* ProcessINI (pcm.cpp:121-196): reads [common_variable] + [pcm_matching] from localization.ini and the "Rear To Main
 * LiDAR" / "Rear To Imu" rows of calibration.ini (ZYX Euler, lf.hpp:340-345).  Call the *_default functions first; keys
 * missing from the file leave their fields unchanged.  Either path may be NULL. */
int elm_load_pcm_config(const char* localization_ini, const char* calibration_ini, elm_pcm_node_config* node,
                        elm_reg_config* reg);
int elm_load_ekf_config(const char* localization_ini, elm_ekf_config* cfg); /* ekfl.cpp:250-316 */

/* pcl::io::loadPCDFile<PointXYZINormal> as used for the map (pcm.cpp:72-79): ascii / binary / binary_compressed PCD,
 * x y z (float32, matched by field name) -> freshly malloc'ed xyz[3n]; release with elm_free. */
int elm_pcd_load_xyz(const char* path, float** xyz_out, size_t* n_out);
void elm_free(void* p);

/* PointCloud2-style record unpack (pcm.hpp:81-106; pcm.cpp:900-930). */
enum { ELM_FIELD_UINT16 = 4, ELM_FIELD_UINT32 = 6, ELM_FIELD_FLOAT32 = 7 }; /* sensor_msgs/PointField datatypes */
typedef struct elm_cloud_field { char name[24]; uint32_t offset; int32_t datatype; } elm_cloud_field;
/* is_ouster = 0: PointXYZIT (x y z intensity time, float32).  is_ouster = 1: OusterPointXYZIRT -- every
 * index_sampling-th record, intensity = reflectivity, time = t * 1e-9f, and the output holds n/index_sampling + 1 slots
 * (a trailing default point when n is a multiple of index_sampling, as in the reference).  cap = capacity of the outputs
 * in points; intensity / rel_time may be NULL. */
int elm_scan_from_cloud(const void* data, size_t n_points, size_t point_step, const elm_cloud_field* fields, int n_fields,
                        int is_ouster, int index_sampling, float* xyz, float* intensity, float* rel_time, size_t cap,
                        size_t* n_out);

/* ---------------------------------------------------------------- the node callback ---------------- */
/* PcmMatching::CallbackPointCloud (pcm.cpp:198-324) as ONE call: stamp -= lidar_time_delay, FilterPointsByDistance,
 * DeskewPointCloud (tables on the host, per-point loop on the GPU), GetInterpolatedPose at the scan end, VoxelDownsample,
 * lidar pose = sync ego pose * tf_ego_to_lidar, RunRegister, ego pose = result * tf_ego_to_lidar^-1, covariance shaping.
 * imu4 / odom14: the node's deq_imu_ / deq_odom_ contents as in elm_deskew_prepare.  *published = 0 reproduces the
 * reference's silent returns (empty input, deskew data missing, no synced pose, registration failure: pcm.cpp:226-229,
 * 238-241, 249-251, 289-292); the other outputs are then undefined except result. */
typedef struct elm_pcm_scan_output {
    double pose_ego[16];     /* icp_ego_pose, column-major */
    double pose_lidar[16];   /* registration result, column-major */
    double covariance[36];   /* nav_msgs/Odometry.pose.covariance, row-major (PublishPcmOdom) */
    double fitness_score;
    double time_scan_end;    /* d_time_scan_end_ = stamp of the published odometry */
    uint64_t n_filtered;     /* points after the distance filter */
    uint64_t n_source;       /* points after VoxelDownsample = registration source size */
    elm_reg_result result;
} elm_pcm_scan_output;
int elm_pcm_callback_point_cloud(elm_ctx* ctx, const elm_map* map, const elm_pcm_node_config* node, const elm_reg_config* reg,
                                 const float* xyz, const float* point_time, size_t n, double stamp, const double* imu4,
                                 size_t n_imu, const double* odom14, size_t n_odom, elm_pcm_scan_output* out, int* published);

/* ---------------------------------------------------------------- multi-GPU ----------------------- */
/* (a) ONE process, N GPUs -- a device group (elm_ctx_create(device_ids[], n, &ctx); the reference's pcm_matching node is
 * one process that calls Registration::RunRegister, pcm.cpp:280-282).  elm_ctx_create_multi creates one context per entry of device_ids
 * and returns the first as the group's LEAD context; everything else keeps its signature.  On the lead:
 *   elm_map_build / elm_map_cal_voxel_cov_all / elm_map_cal_point_cov_all / elm_map_build_neighbourhoods   the map is REPLICATED on every
 *       device (the handle is rank 0's replica: read-backs, elm_map_get_correspondences, elm_map_find_ground_height work on it);
 *   elm_scan_upload          the scan is ordered along the ordering kernel's Hilbert curve and cut into N contiguous SHARDS, one per
 *       device (locality-aware sharding: a rank holds a compact sector of the scan at full density); elm_scan_size = the whole scan;
 *   elm_register             RunRegister on host buffers: the caller's point order cut into N contiguous shards;
 *   elm_register_batch / elm_register_stream   on scans uploaded through the lead;
 *   every ICP iteration all-reduces the ranks' packed normal equations (ONE ncclAllReduce(double, sum) of ELM_PACKED_SUMS doubles per
 *       scan over the communicators the ranks form among themselves -- RCCL over xGMI -- each rank driven by its own host thread) and
 *       every rank solves the same sums; the ranks' results are compared bit for bit (ELM_ERR_COMM if they differ);
 *   elm_ctx_destroy          destroys the group.
 * Not available on a group (ELM_ERR_UNSUPPORTED): elm_register_stream_host, elm_register_batch_enqueue / _finish.
 * elm_pcm_callback_point_cloud on a group takes its stage-by-stage path (deskew + downsample on the lead device, the registration
 * sharded): same results; the fused one-pass form is a plain context's (the callback registers ~10 k downsampled points).
 * A device id may repeat ({0, 0}: two ranks on one GPU).  RCCL refuses two ranks on one device; such a group exchanges through
 * page-locked host memory (sum in rank order) -- the form a one-GPU box can test.  ELM_GROUP_EXCHANGE=host | rccl forces either.
 * n = 1 returns a plain context (with ELM_GROUP_EXCHANGE=rccl: a group of ONE rank -- worker thread, one-rank communicator, one
 * ncclAllReduce per iteration: what a one-GPU box can run of the group's RCCL path). */
int elm_ctx_create_multi(const int* device_ids, int n, elm_ctx** out);
/* ranks of the group a context leads (1: a plain context), its exchange (0 none, 1 RCCL, 2 host memory), its devices */
int elm_ctx_group_info(elm_ctx* ctx, int* n_ranks, int* exchange, int* device_ids, int cap);
/* RunRegister on ONE RANK's shard of an n_total-point scan (host buffers, the caller's point order): what a rank of a process-per-GPU
 * job (b) calls where the one-GPU caller calls elm_register -- the sums are exchanged over the context's communicator / hook, the overlap
 * gate (reg.cpp:351) is taken against n_total.  quiet != 0: RunRegister's log text is not printed (one rank of a job prints it). */
int elm_register_shard(elm_ctx* ctx, const elm_map* map, const float* shard_xyz, size_t n, size_t n_total, const double T0[16],
                       const elm_reg_config* cfg, elm_reg_result* result, elm_iter_trace* trace, int quiet);

/* (b) One process per GPU.  Rank 0 obtains an id, the host distributes its bytes (e.g. torch.distributed
 * broadcast), every rank calls elm_comm_init.  Afterwards elm_register_batch* sums the packed normal
 * equations of every scan over all ranks with ONE ncclAllReduce(double, sum) per ICP iteration (RCCL/xGMI).
 * RCCL is dlopen'ed ("librccl.so.1") on first use, a single-GPU process never needs it. */
#define ELM_COMM_ID_BYTES 128
int elm_comm_get_unique_id(void* id_bytes /* ELM_COMM_ID_BYTES */);
int elm_comm_init(elm_ctx* ctx, int rank, int nranks, const void* id_bytes);
int elm_comm_destroy(elm_ctx* ctx);
/* rank / size as the RCCL communicator itself reports them (ncclCommUserRank / ncclCommCount); nranks = 0 without a communicator */
int elm_comm_info(elm_ctx* ctx, int* rank, int* nranks);
/* Alternative exchange hook (e.g. a torch.distributed all_reduce from Python): called between the accumulate
 * and the solve launches with the device pointer of the packed sums. Pass NULL to remove. */
typedef int (*elm_allreduce_fn)(void* dev_ptr, size_t n_doubles, void* hip_stream, void* user);
int elm_comm_set_hook(elm_ctx* ctx, elm_allreduce_fn fn, void* user);

/* number of doubles all-reduced per scan per iteration: 21 (upper JTJ) + 6 (JTr) + 1 (residual) + 1 (n_corr)
 * padded to 32 */
#define ELM_PACKED_SUMS 32

#ifdef __cplusplus
}
#endif
#endif /* ELIMALOC_HIP_H */
