// elm_internal.hpp -- device-side data layout shared by the kernels (elm_k_*.hip) and the host units behind the C ABI
// (elm_ctx.cpp, elm_map.cpp, elm_index.cpp, elm_scan.cpp, elm_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/elimaloc_hip.h"

namespace elm {

// ---- map in HBM -------------------------------------------------------------------------------------
// Open-addressing table keyed by the STORED voxel key (truncation toward zero, vhm.cpp:275).  One 32-byte slot
// carries everything a probe needs (key, voxel id, bucket range), so a hit costs one 32-B access.
struct __attribute__((aligned(32))) HashSlot {
    int32_t kx, ky, kz;
    int32_t vid; // -1 = empty
    uint32_t start;
    uint32_t cnt;
    uint32_t pad0, pad1;
};

struct __attribute__((packed, aligned(4))) Pt3 { // 12-byte point: scan points (one global_load_dwordx3), candidates of the neighbourhood lists
    float x, y, z;
};

struct __attribute__((aligned(16))) GridBlk { // four candidates of the cell grid, structure of arrays (48 bytes = three 16-byte loads)
    float x[4], y[4], z[4];
};

// One occupied neighbour voxel of a query voxel (VGICP / AVGICP lists), ONE 64-byte record = one memory sector per pair: the mean
// (float64, vhm.hpp:114-148), the plane normal and k of its regularised covariance U diag(1, 1, 1e-3) V^T = I - 0.999 n n^T, whose
// inverse is I + k n n^T with k = 999 (k = 0: the identity of voxels with fewer than two points) -- the 72-byte inverse covariance is
// rebuilt in registers instead of being fetched.  Maps with a covariance that is NOT of that form (rank-deficient neighbourhoods:
// round-off decides the signs of U against V, vhm.hpp:141) are found at map build and keep reading vox_cinv[vid].
struct __attribute__((aligned(64))) VoxRec {
    double mx, my, mz;
    double nx, ny, nz;
    double k;
    int32_t vid;
    int32_t pad; // position code of the neighbour (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)
};

// Four slots of a voxel-mean list (VGICP / AVGICP): the float32 means (the filter of the VGICP search) and, per slot, the voxel's id
// with the neighbour's position code (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) above it -- 64 bytes, one memory sector, never straddling a
// 128-byte line.  Padding slots: mean 1e18, word -1.  The float64 record of a voxel lives ONCE in DevMap::vox_rec.
constexpr uint32_t kVidBits = 26;                    // voxel ids of the lists: < 2^26 voxels (a 1.6 G-point map at 25 points per voxel)
constexpr uint32_t kVidMask = (1u << kVidBits) - 1u;
struct __attribute__((aligned(64))) VoxBlk {
    GridBlk g;
    int32_t vc[4];
};

struct DevMap {
    const HashSlot* slots;
    uint32_t mask; // capacity - 1 (capacity is a power of two >= 4 * n_voxels)
    uint32_t n_vox;
    uint32_t n_pts;
    uint32_t _pad;
    const float4* pts;      // bucket-ordered map points, xyz + pad (w unused), insertion order inside a bucket
    const double* vox_mean; // [n_vox][3]            CalVoxelCov (vhm.hpp:114-148)
    const double* vox_cov;  // [n_vox][9] row-major (read-backs: Covariances())
    const double* vox_cinv; // [n_vox][9] its inverse: what the VGICP / AVGICP pairs use (add_pair_world)
    const double* vox_nk;   // [n_vox][4] unit plane normal + k of the inverse's compact form I + k n n^T (see VoxRec)
    // GICP payload of a map point, ONE 128-byte record (a matched point costs one cache line instead of three scattered
    // ones): [0..2] neighbourhood mean, [3..11] INVERSE of the covariance of ProcessVoxelBlock (vhm.hpp:195-250), row-major,
    // [12..14] eigenvector of the covariance's smallest eigenvalue (reg.cpp:89-91, precomputed once), [15] pad
    const double* pt_gicp;  // [n_pts][16]
    const double* pt_cov;   // [n_pts][9] the covariance itself, row-major (read-backs; the use_radar_cov kernel inverts R^-1 C R^-T + C_source)
    double voxel_size;
    double inv_vs_exact; // 1 / voxel_size when voxel_size is a power of two (g * inv == g / voxel_size bit for bit), else 0
    // neighbourhood lists (optional): for every FLOOR-keyed query voxel that has at least one stored neighbour, the
    // points of its 27 trunc-keyed neighbour buckets concatenated in the reference's visiting order (x-major ..
    // z-minor, insertion order inside a bucket).  27x duplication of the map points, laid out for streaming.
    const HashSlot* qslots; // key = query voxel, vid = query id, start/cnt = its list, pad0 = occupied neighbours
    uint32_t qmask;
    uint32_t n_q;
    const Pt3* nbr_pts;       // candidate coordinates, 12 bytes each
    const uint32_t* nbr_idx;  // global point index of every candidate (read only for a GICP winner)
    // voxel-mean lists (VGICP, optional): the occupied voxels among the 27 neighbours of every query voxel in the
    // reference's visiting order (vhm.cpp:208-243), 32-byte records; vqslots: query key -> (start, cnt)
    const HashSlot* vqslots;
    uint32_t vqmask;
    uint32_t _pad2;
    const VoxRec* vox_rec;    // [n_vox] the float64 record {mean, normal, k, vid} of every voxel, ONCE (round 6; rounds 2-5 replicated it into
                              // every query list: 27 copies, 4.3 GB on the 50 M-point map)
    const uint32_t* vq_dense; // optional: the same (start << 5 | cnt) addressed by the dense floor-key box (vq_x0.., no hash probe)
    const VoxBlk* vnbr_blk;     // the lists: blocks of four slots {float32 mean, vid | code}: list q starts at block
                                // start(q) / 4 (list starts are multiples of four slots), padding slots 1e18 / -1
    uint32_t vnbr_pad_blk;      // index of the all-padding block at the end of vnbr_blk
    const VoxRec* vface;        // optional (with vq_dense): the FACE neighbours (+ the voxel itself) of every query voxel, in list order --
                                // what AVGICP pairs with (vhm.cpp:153-206) -- and
    const uint32_t* vqf_dense;  // (start << 3 | count) of those, addressed like vq_dense
    int32_t vq_x0, vq_y0, vq_z0;
    int32_t vq_nx, vq_ny, vq_nz;
    const uint16_t* nbr_cell_off; // [n_q][224]: every list is sorted by half-voxel cell (6x6x6 grid, clamped); cell c =
                                  // entries [off[c], off[c+1]) of the list
    // dense half-voxel cell grid over the map's bounding box (optional; default search index when it fits the memory budget):
    // the map points ONCE, sorted by cell (x-major, y, z fastest -- the cells iz0..iz1 of one (ix, iy) column are one contiguous
    // run), in 48-byte blocks of four (x[4], y[4], z[4]); every cell is padded to whole blocks with far-away points (1e18), so a
    // block never straddles cells and no candidate needs masking.  grid_start[linear cell] = first BLOCK of the cell, the next
    // entry = its end.  Candidate id = block * 4 + slot.  Cells follow the
    // STORED (truncated) voxel keys: bucket k > 0 is cells {2k, 2k+1}, bucket 0 (two voxels wide) is {-2,-1,0,1}, bucket k < 0 is
    // {2k-2, 2k-1}; geometrically cell c is [c h, (c+1) h], h = voxel_size / 2.
    const GridBlk* grid_blk;    // [n_blk]; block 0 is all padding (the target of masked-off loads), cells start at block 1
    const uint32_t* grid_idx;   // [4 * n_blk] bucket-order index of every candidate slot (GICP payload, insertion order for exact
                                // ties); 0xFFFFFFFF in padding slots
    const uint32_t* grid_start; // [gnx * gny * gnz + 4]
    // two-level form of the same grid (maps whose bounding box is too large or too sparse for one dense offset table): the box is cut
    // into tiles of kTile x kTile (x, y) cells; grid_tiles[tile] = {first offset entry, z0 | nz << 16}: the tile stores offsets only for
    // the cells z0 .. z0 + nz - 1 that hold points, (nz + 1) entries per column (its cell starts + the column end), columns (x, y)-major.
    // Blocks are sorted (tile, column, z), so the cells of a column are still one contiguous run.  Empty tiles share 64 zero entries.
    const uint2* grid_tiles;    // [gnx / kTile][gny / kTile] (gnx, gny are multiples of kTile)
    int32_t grid_tiled;         // 1: grid_start is addressed through grid_tiles
    int32_t gtny;               // tiles along y
    int32_t grid_wide;          // 1: the block array is 4 GB or more -- stage 1 addresses it in 16-byte units (template flag WIDE)
    uint32_t grid_nslots;       // 4 * n_blk: candidate slots of the block array
    const double* grid_gicp;    // [4 * n_blk][16]: pt_gicp gathered into slot order -- a GICP match reads its record without the index hop
                                // (only for maps with a covariance outside the compact form)
    const double* grid_gicp8;   // [4 * n_blk][8]: the compact record {mean[3], unit normal[3], k, -}: 64 bytes = one memory sector per match;
                                // the inverse covariance I + k n n^T is rebuilt in registers (k = 999: U diag(1, 1, 1e-3) V^T of
                                // vhm.hpp:238-246 with U = V up to rounding, checked per point at map build; k = 0: identity)
    int32_t gicp_compact;       // 1: grid_gicp8 is what the grid kernel reads (k = NaN flags a point outside the compact form: its full
                                // record is read from pt_gicp by the index in word 7); 2: the same and no point is flagged -- the kernel
                                // instantiation without the fallback, its pair gathered fused (pair_sum_compact)
    int32_t vox_compact;        // 1: the VoxRec's own normal / k are used (k = NaN: vox_cinv[vid] is read for that voxel); 2: no voxel flagged
    int32_t vface_plain;        // 1: the face sublists are written for the fused AVGICP walk (identity covariances as zero normals), which gathers
                                // sum w and sum (w k) n n^T instead of nine entries per pair
    int32_t vface_flagged;      // 1: some voxel of this map is outside the compact form (its records carry NaN in the normal): the fused walk
                                // skips those pairs and a fix-up launch adds them (RegParams::flagged)
    int32_t gx0, gy0, gz0;      // cell coordinates of grid entry (0, 0, 0)
    int32_t gnx, gny, gnz;
    // dense voxel box of the floor keys a query can have near the map: cnt27 | nocc27 << 16 of the reference's 27-voxel walk
    // (the work counters, and cnt27 == 0 -> no neighbour bucket at all -> the reference's origin default, vhm.cpp:37)
    const uint32_t* vox_stat;   // [vnx * vny * vnz]
    int32_t vx0, vy0, vz0;
    int32_t vnx, vny, vnz;
};

__host__ __device__ __forceinline__ uint32_t hash3(int32_t x, int32_t y, int32_t z) {
    uint32_t h = (uint32_t)x * 73856093u ^ (uint32_t)y * 19349669u ^ (uint32_t)z * 83492791u;
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// ---- scans / per-registration state -----------------------------------------------------------------
struct ScanDesc {
    const Pt3* pts;    // sensor-frame points, packed xyz (12 bytes: what the LiDAR driver / the caller holds, no repack on upload)
    uint32_t n;        // points resident on this GPU
    uint32_t n_total;  // points of the whole scan (== n on one GPU)
    uint32_t blk_begin; // first logical block of this scan in the batch launch
    uint32_t blk_end;
};

// one per scan of the batch, lives in HBM for the whole registration
struct ScanState {
    double T[16];    // current pose, column-major
    double Rinv[9];  // row-major inverse of the rotation block (3x3 cofactor inverse, reg.cpp:79)
    double tinv[3];  // -Rinv t
    double fitness;  // d_fitness_score_
    double local_cov[36]; // column-major == row-major (symmetric)
    double n_corr_last;
    double pt_iters, cand_total, occ_total, fallback_blocks, tested_total; // work counters over the executed iterations
    int32_t done;
    int32_t success;
    int32_t gate;
    int32_t iters;
    int32_t reg;  // registration this slot works on (== slot index in a lockstep batch; -1 = idle slot of a stream)
    int32_t _pad;
};

// continuous batching (elm_register_stream): pending registrations and the device-side bookkeeping
struct QueueItem {
    const Pt3* pts;
    uint32_t n, n_total;
};
struct StreamCtrl {
    int32_t next;      // first registration not yet assigned to a slot
    int32_t completed; // registrations whose final state has been saved
    int32_t total;
    int32_t ready;     // host-fed streams: registrations whose scan has arrived in HBM (uploaded + ordered); a slot only takes r < ready
    int32_t done_iter; // iteration (0-based) whose solve finished the LAST registration, -1 while the stream runs: what the next call of the
                       // same shape enqueues before it first looks (the host's own count only says when it LOOKED)
};

// in-solve refill of finished slots (single-rank streams, see finish_slot in elm_k_solve.hip)
struct StreamArgs {
    ScanDesc* scans;
    const QueueItem* queue;
    const double* qT0;
    ScanState* out_state;
    StreamCtrl* ctrl; // nullptr: no refill in the solve
    int32_t hostfed;  // 1: the queue fills while the stream runs (ctrl->ready grows): idle slots look for work at every solve
    int32_t save_only; // 1 (multi-rank streams with the refill launch): the solve saves a finished registration's state and counts it, the slot
                       // stays free for k_stream_refill to hand it the next registration in slot order
    int32_t stride;   // > 0 (multi-rank streams): slot s serves the registrations s, s + stride, s + 2 stride, ... -- an assignment that
                      // is a function of the slot alone, hence identical on every rank without any exchange; 0: first come, first served
    int32_t iter;     // index of this iteration in the call (StreamCtrl::done_iter)
};

struct RegParams {
    double th;  // max_search_dist
    double th2; // th * th
    double lm_lambda;
    double term_thr;
    double min_overlap;
    double max_fitness;
    int32_t method;
    int32_t max_iter;
    uint32_t uniform_blocks; // > 0: every scan / slot owns exactly that many consecutive workgroups (scan = block / uniform_blocks)
    int32_t radar;           // use_radar_cov with a covariance method: k_accumulate_radar's 64-double partial records, full JTJ
    int32_t _reserved0;
    int32_t stats;           // elm_ctx_set_work_counters: the grid / voxel-list kernels also sum the three work counters (STATS = 1)
    uint32_t* flagged;   // [workgroups] AVGICP on a map with flagged voxels: set by a workgroup of the fused walk that met (and skipped) a flagged
                         // record, read and cleared by the fix-up launch that adds those pairs to the workgroup's partial record (nullptr: the
                         // map runs the nine-entry walk with its fallback instead)
    int32_t rank_check;  // 1 (several ranks, production kernels): slots 29..31 of every scan's exchanged sums -- the work counters, zero in
                         // production -- carry (1, id, id^2), id = 16 (registration + 1) + (iteration & 15): after the all-reduce every rank
                         // verifies sum(id) == n id and sum(id^2) == n id^2, i.e. that all ranks iterate the SAME registration in this slot
                         // (the refill launch hands registrations out from flags every rank computes for itself); a mismatch sets active[1]
                         // and the call returns ELM_ERR_COMM instead of adding up unrelated normal equations
    int32_t _pad_rc;
    double* asym;        // [workgroups][16] side records of a map with an asymmetric flagged covariance (the strict lower triangle of
                         // H_w - H_w^T, see asym_side_store in elm_dev_reduce.hpp): written by every workgroup of such a launch, reduced by
                         // k_solve, which restores all 36 entries of J^T M J before the congruence; nullptr on every other map
    double* asym_sums;   // [scans][16] the scans' reduced side sums when the iteration is split around an exchange (modes 1 / 2 of k_solve;
                         // laid out right behind the packed sums, so ONE all-reduce carries both)
    double radar_var[3]; // range_variance_m, azimuth_variance_deg, elevation_variance_deg (reg.hpp:77-79)
    // correspondence queries (elm_map_get_correspondences: the reference's public VoxelHashMap::GetCorrespondence* calls, vhm.cpp:31-206):
    // the QUERY instantiations of the grid / voxel-list kernels (template STATS = 2) take point i of their one "scan" from query[3 i ..]
    // (GLOBAL frame, float64: what Registration hands the map after TransformPoints) instead of T * p, run the production search and
    // write the pair(s) instead of sums: q_out[i] = the map point (bucket order) / voxel id of the pair, -1 = the reference's default
    // target at the origin (no neighbour bucket at all, vhm.cpp:37 / :105), -2 = no pair (beyond max_dist); GetCorrespondencesAllCov:
    // q_out[8 i + r] = voxel id of the pair with the r-th voxel of the reference's visiting order (vhm.cpp:224-230), -2 = none
    const double* query;
    int32_t* q_out;
};
constexpr int kAsymRecord = 16; // doubles per side record (15 used)
constexpr int kRadarRecord = 64; // doubles per partial record of k_accumulate_radar

constexpr int kTileShift = 3, kTile = 1 << kTileShift; // two-level grid: tiles of 8 x 8 columns
constexpr int kBlock = 256;
constexpr int kInitPack = 8; // batches up to this size are initialised from kernel arguments (k_init_pack)
struct InitPack {
    ScanDesc d[kInitPack];
    double T0[kInitPack][16];
};
constexpr int kSums = ELM_PACKED_SUMS; // 21 + 6 + 1 + 1 (+ n_cand, n_occ, pad)

// ---- launchers (elm_k_*.hip) ----------------------------------------------------------------------
void launch_init_state(hipStream_t s, ScanState* st, const double* T0, int batch, int map_empty, int* active);
void launch_init_pack(hipStream_t s, ScanDesc* scans, ScanState* st, const InitPack& pack, int batch, int map_empty, int* active, const unsigned* n_dev);
void launch_stream_refill(hipStream_t s, ScanDesc* scans, ScanState* st, int slots, const QueueItem* queue, const double* qT0,
                          /* first: initial fill; save: copy finished states out + count them (0: the solve has done that) */
                          ScanState* out_state, StreamCtrl* ctrl, int first, int save = 1);
void launch_accumulate_radar(hipStream_t s, const DevMap& m, const ScanDesc* scans, int batch, int total_blocks, ScanState* st, double* partials,
                             const RegParams& rp); // use_radar_cov = 1, methods GICP / VGICP / AVGICP
void launch_accumulate_direct(hipStream_t s, const DevMap& m, const ScanDesc* scans, int batch, int total_blocks,
                              ScanState* st, double* partials, const RegParams& rp);
// mode 0: reduce + solve (single GPU); 1: reduce only -> sums; 2: solve only from sums
void launch_solve(hipStream_t s, const ScanDesc* scans, int batch, ScanState* st, const double* partials,
                  double* sums, const RegParams& rp, elm_iter_trace* trace, int mode, int* active, const StreamArgs* refill = nullptr);
void launch_nbr_count(hipStream_t s, const DevMap& m, const int32_t* qkeys, uint32_t n_q, uint32_t* counts, uint32_t* nocc);
void launch_accumulate_vnbr(hipStream_t s, const DevMap& m, const ScanDesc* scans, int batch, int total_blocks,
                            ScanState* st, double* partials, const RegParams& rp);
void launch_vnbr_fill(hipStream_t s, const DevMap& m, const int32_t* qkeys, uint32_t n_q, const uint32_t* offsets, VoxBlk* out_blk);
void launch_vox_rec_fill(hipStream_t s, const DevMap& m, VoxRec* out);
// face-neighbour sublists of the voxel-mean lists: counts (out == nullptr) or the records at face_off
void launch_vface(hipStream_t s, const DevMap& m, const uint32_t* offsets, const uint32_t* counts, uint32_t n_q, uint32_t* face_cnt,
                  const uint32_t* face_off, VoxRec* out, int plain);
void launch_accumulate_cell(hipStream_t s, const DevMap& m, const ScanDesc* scans, int batch, int total_blocks,
                            ScanState* st, double* partials, const RegParams& rp);
int stream_max_slots(); // slots one elm_register_stream call can iterate concurrently
void launch_accumulate_grid(hipStream_t s, const DevMap& m, const ScanDesc* scans, int batch, int total_blocks,
                            ScanState* st, double* partials, const RegParams& rp);
// Registration::AlignCloudsLocal / AlignCloudsLocalPointCov / AlignCloudsLocalVoxelCov (reg.cpp:15-225) on explicit pairs (elm_align_clouds_local)
struct AlignArgs {
    double Rinv[9], tinv[3]; // inverse of last_icp_pose: rotation block (row-major) and -Rinv t
    double th, th2;          // trans_th
    double lm_lambda;
    int32_t method;          // ELM_P2P / ELM_GICP / ELM_VGICP (= AVGICP)
    int32_t use_src_cov;     // use_radar_cov: the source points' covariance terms are added (reg.cpp:109-111 / 188-190)
};
constexpr int kAlignOut = 16 + 36 + 1 + 6 + 36 + 6 + 1; // T (column-major), local_cov (row-major), fitness, x, J^T M J (row-major), J^T M r, pair count
void launch_align_pairs(hipStream_t s, const double* src_local, const double* tgt_xyz, const double* tgt_cov, const double* src_cov, size_t n,
                        const AlignArgs& a, double* partials, double* out);
void launch_query_direct(hipStream_t s, const DevMap& m, int what, const double* query, size_t n, double th2, int32_t* q_out); // the plain walk (27 / 7 hash probes, float64): the query form of k_accumulate_direct
void launch_vox_stat(hipStream_t s, const DevMap& m, uint32_t* out); // fills DevMap::vox_stat's box (m.vx0.., m.vnx..)
void launch_gather_gicp(hipStream_t s, const DevMap& m, size_t n_slots, double* out, int compact); // pt_gicp[grid_idx[slot]] -> out[slot] (16 or 8 doubles)
// half-voxel cell of a stored coordinate (host + device; the binning of DevMap::grid_pts)
__host__ __device__ inline int grid_cell_of(double a, double voxel_size) {
    const double t = a / voxel_size; // the reference's own key arithmetic (vhm.cpp:275), truncated below
    const int k = (int)t;
    if (k > 0) return 2 * k + ((t - (double)k >= 0.5) ? 1 : 0);
    if (k < 0) return 2 * k - 2 + ((t - (double)k > -0.5) ? 1 : 0);
    if (t >= 0.0) return (t >= 0.5) ? 1 : 0;
    return (t > -0.5) ? -1 : -2;
}
void launch_nbr_cellsort(hipStream_t s, const DevMap& m, const int32_t* qkeys, uint32_t n_q, const uint32_t* offsets,
                         const uint32_t* counts, Pt3* pts, uint32_t* idx, uint16_t* cell_off);
size_t nbr_cell_stride();
void launch_nbr_fill(hipStream_t s, const DevMap& m, const int32_t* qkeys, uint32_t n_q, const uint32_t* offsets, Pt3* out,
                     uint32_t* out_idx);
// *bad counts the covariances whose inverse is not I + k n n^T to 1e-10 relative (the compact records are then not used)
void launch_voxel_cov(hipStream_t s, const DevMap& m, const uint2* ranges, double* vox_mean, double* vox_cov, double* vox_cinv, double* vox_nk, unsigned* bad);
void launch_point_cov(hipStream_t s, const DevMap& m, double d2max, double* pt_gicp, double* pt_cov, unsigned* bad); // pt_cov [n_pts][9]: read-backs

// relocalization scores (elm_k_reloc.hip): the key box of the occupancy bitmap, cells (cx * ny + cy) * nz + cz
struct RelocBox {
    int32_t x0, y0, z0;
    uint32_t nx, ny, nz;
};
constexpr int kRelocPPL = 8;                    // scan points per lane of k_reloc_score
constexpr int kRelocChunk = kBlock * kRelocPPL; // points per workgroup
constexpr int kRelocHyp = 32;                   // hypotheses per workgroup
void launch_reloc_bitmap(hipStream_t s, const DevMap& m, const RelocBox& b, uint64_t n_cells, unsigned long long* bits);
// form 0: bitmap in LDS (n_words 32-bit words), 1: bitmap in global memory, 2: hash probes only.  partial: [n_poses][chunks] scratch
void launch_reloc_score(hipStream_t s, int form, const DevMap& m, const float* pts, uint32_t n, const double* poses, uint32_t n_poses,
                        const RelocBox& b, const uint32_t* bits, uint32_t n_words, uint32_t* partial, uint32_t* scores);

// global relocalization (elm_k_reloc.hip)
// 2-D bin index of the map's points for the ground field: bin (bx, by) = (floor((x - x0) / bin), floor((y - y0) / bin)) in float64, points
// sorted by bin (bx * nby + by), start[b] .. start[b + 1]; 2 bin > 5 m, so a query reads the 5 x 5 bins around its own
struct GroundIndex {
    const float4* pts;
    const uint32_t* start; // [nbx * nby + 1]
    double x0, y0, bin;
    int32_t nbx, nby;
};
constexpr double kGroundBin = 2.75;
void launch_ground_heights(hipStream_t s, const GroundIndex& gi, const double* xy, uint32_t n, double* z, int32_t* found);
// level windows of the occupancy bitmap: columns of nzw 32-bit words (cell (cx, cy) at word (cx * ny + cy) * nzw); out(c) = OR of in over the
// window [c, c + w) along axis (0: x, 1: y) read as windows of width wp of in (reads past the box are empty)
void launch_reloc_window_or(hipStream_t s, const uint32_t* in, uint32_t* out, uint32_t nx, uint32_t ny, uint32_t nzw, int axis, uint32_t wp, uint32_t w);
// a search node: the x / y range of its lattice nodes, the z range of fl(g + h) over its valid leaves, its yaw row
struct RelocNode {
    double xlo, xhi, ylo, yhi, zlo, zhi;
    int32_t k, _pad;
};
// bounds[n] = the counted points whose window at the node is occupied (rot: [K][9] row-major Rz(yaw_k) R0; bits: the level's windows of
// width w over the box b, columns of b.nz / 32 words)
void launch_reloc_bound(hipStream_t s, const DevMap& m, const float* pts, uint32_t n, const RelocNode* nodes, uint32_t n_nodes, const double* rot,
                        const RelocBox& b, const uint32_t* bits, uint32_t w, uint32_t kz_cap, uint32_t* partial, uint32_t* bounds);
// rows[12 l] of lattice pose hyps[l] = (k NX + i) NY + j: rot row k, t = (x_min + i step, y_min + j step, gz[i NY + j])
void launch_reloc_leaf_rows(hipStream_t s, const uint32_t* hyps, uint32_t n, const double* rot, double x_min, double y_min, double step,
                            uint32_t NX, uint32_t NY, const double* gz, double* rows);

// free-space check (elm_k_free.hip): the fine occupancy of a map as an open-addressing table of coarse cells
// (fine cell >> 2 per axis, arithmetic), each with the 64-bit mask of its 4 x 4 x 4 fine cells, bit ((f_x & 3) * 4 + (f_y & 3)) * 4 + (f_z & 3)
struct FineTable {
    const int4* keys;                // [mask + 1] coarse cell in x, y, z; w = 1 used, 0 empty (load factor <= 0.5: a probe always ends)
    const unsigned long long* masks; // [mask + 1]
    uint32_t mask;
    uint32_t n_coarse;
    double cell, inv_cell_exact; // voxel_size / sub; 1 / cell where cell is a power of two (q * inv gives q / cell's bits), else 0
};
struct FreeParams { // elm_freespace_config resolved for one map
    double ox, oy, oz, step, min_r2, max_r2, margin_m, margin_frac;
    int32_t k0, max_samples, min_hits, _pad;
};
constexpr int kFreePoses = 16;  // poses per workgroup of k_free_rays
constexpr int kFreeWords = 6;   // a partial: counted, pierced, end-occupied, supported, samples, hit samples of one (pose, chunk)
// form 0: one ray per lane, the last coarse cell's mask kept in registers; form 1: a wave walks its 64 rays one after the other, its lanes
// taking consecutive samples (the A/B of DESIGN.md section 13).  rows: 12 doubles per pose (R_r0, R_r1, R_r2, t_r); partial:
// [n_poses][chunks][kFreeWords] scratch; hits: [n_poses][n] or nullptr
void launch_free_space(hipStream_t s, int form, const FineTable& ft, const FreeParams& fp, const float* pts, uint32_t n, const double* rows,
                       uint32_t n_poses, uint32_t* partial, elm_freespace_stats* stats, uint16_t* hits);

// ray casting (elm_k_ray.hip): exact traversal of the fine cells (FineTable) along every beam of a scan at many poses
struct RayParams { // elm_raycast_config resolved for one call
    double ox, oy, oz, t_min, t_max, cmp_min_r2, cmp_max_r2, tol_m, tol_frac;
    int32_t max_steps, _pad;
};
constexpr int kRayMaxPoses = 16;    // the largest pose block of k_ray_cast (its LDS is sized for it)
constexpr int kRayPosesDefault = 1; // the pose block that measured fastest; ELM_CHECK=ray_poses=N overrides it
constexpr int kRayWords = 9;        // a partial: cast, hit, miss, truncated, compared, match, through, front, steps of one (pose, chunk)
constexpr int kRayMaxSteps = 1 << 20; // cap of max_steps: 256 beams x 2^20 steps fit a 32-bit partial
// rows: 12 doubles per pose (R_r0, R_r1, R_r2, t_r); partial: [n_poses][chunks][kRayWords] scratch; range_in / range_out [n_poses][n],
// cell [n_poses][n][3], flag [n_poses][n]: each nullptr or a device array; pose_block: 1 .. kRayMaxPoses poses per workgroup
void launch_ray_cast(hipStream_t s, uint32_t pose_block, const FineTable& ft, const RayParams& rp, const float* pts, uint32_t n, const double* rows,
                     uint32_t n_poses, uint32_t* partial, elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag);

// map evidence (elm_k_evid.hip): the ray cast's walk stopped before the measured end point, counting per occupied
// fine cell the beams that passed through it and the beams that ended in it
struct EvidParams { // elm_evidence_config resolved for one call
    double ox, oy, oz, t_min, obs_min_r2, obs_max_r2, margin_m, margin_frac;
    int32_t max_steps, _pad;
};
struct EvidJob { // one observation: a resident scan at a pose
    const float* pts; // packed xyz
    uint32_t n;       // beams
    uint32_t chunk0;  // the job's first 256-beam chunk among all chunks of the launch
    double rows[12];  // (R_r0, R_r1, R_r2, t_r) per row r
};
constexpr int kEvidMaxJobs = 4096;
constexpr int kEvidWords = 9; // a partial: cast, observing, walked, truncated, through beams, end hit, end free, through events, steps of a chunk
// jobs [n_jobs] with ascending chunk0, n_chunks = all chunks of the launch (> 0); base [ft.mask + 1]: the first counter of every table slot
// (prefix of the masks' popcounts in slot order); through / hit: the counters; partial [n_chunks][kEvidWords] scratch; stats [n_jobs];
// events [jobs[0].n] or nullptr (one job only)
void launch_evid_walk(hipStream_t s, const FineTable& ft, const EvidParams& ep, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks,
                      const uint32_t* base, uint32_t* through, uint32_t* hit, uint32_t* partial, elm_evidence_stats* stats, uint16_t* events);

// place recognition (elm_k_place.hip): scan descriptors of n_rings x n_layers words of 64 sector bits, their exact
// match at all 64 yaw shifts and the top-k selection
constexpr int kPlaceSectors = ELM_PLACES_SECTORS;
constexpr int kPlaceMaxWords = 512; // 32 rings x 16 layers: 4 KB of LDS per describing workgroup
constexpr int kPlaceMaxTopK = ELM_PLACES_MAX_TOP_K;
struct PlaceParams {
    int32_t n_rings, n_layers;
    const double* tables; // device: ring_edge2 [n_rings + 1], z_edge [n_layers + 1], dir [64][2]
};
// jobs / n_chunks as launch_evid_walk (the rows are the levelling poses); words [n_jobs][W] zero before the call, n_bits [n_jobs],
// stats [n_jobs] zero before the call
void launch_pl_describe(hipStream_t s, const PlaceParams& pp, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks, unsigned long long* words,
                        uint32_t* n_bits, elm_places_stats* stats);
void launch_pl_bits(hipStream_t s, const unsigned long long* words, uint32_t W, uint32_t n_desc, uint32_t* n_bits);
// matches [n_queries][n_entries], cands [n_queries][kPlaceMaxTopK], n_cands [n_queries]; nothing is launched without queries or entries
void launch_pl_match(hipStream_t s, const unsigned long long* qwords, const uint32_t* q_bits, uint32_t n_queries, const unsigned long long* dwords,
                     const uint32_t* d_bits, const long long* ids, uint32_t W, uint32_t n_entries, const elm_places_query_config* cfgs,
                     elm_place_match* matches, elm_place_candidate* cands, int32_t* n_cands);

// pose graph (elm_k_pgraph.hip): the device's view of one graph.  Edge arrays are component-major with the stride
// e_stride (array[component * e_stride + edge]); node arrays are node-major.
constexpr uint32_t kPgLanesPerEdge = 8;   // k_pg_linearize: the lane of a group is the column
constexpr uint32_t kPgNodesPerBlock = 32; // k_pg_spmv: a lane group of 8 per node, the lane is the row
constexpr uint32_t kPgHubDegree = 64;     // a node with more incident edges takes a whole wavefront of k_pg_spmv_hub
constexpr uint32_t kPgBlock = 256;        // the per-node and per-edge kernels, and the lanes that reduce partial slots
struct PgState {
    double rz[2];     // r^T z before the iteration of that parity
    double rz0;
    uint32_t stop[2]; // the solve is over for the launches of the iteration of that parity
    uint32_t iters, converged;
};
struct PgOut {
    double chi2, cost, n_outliers, dmax, grad_inf;
};
struct PgDev {
    uint32_t N, E, e_stride, n_hubs;
    const int32_t *ei, *ej;
    const double *Z, *info;          // [E][12] pose rows, [E][36]
    const uint8_t* fixed;            // [N]
    double *r, *A, *B, *s, *w;       // [6], [36], [36], [1], [1] components
    double *gi, *gj, *Hii, *Hij, *Hjj; // [6], [6], [36], [36], [36] components
    const uint32_t *inc_start, *inc; // CSR: [N + 1]; edge << 1 | side (0: the node is i, 1: j), ascending edge per node
    const uint32_t* hubs;            // the nodes of degree > kPgHubDegree, ascending
    double *Hd, *g, *Minv;           // [N][36], [N][6], [N][36]
    uint8_t* active;                 // [N]: the solve moves the node
    double *x, *rr, *z, *p, *q;      // [N][6]
    double *part_pq, *part_rz, *part_cost, *part_max;
    PgState* state;
    PgOut* out;
};
constexpr uint32_t pg_pq_slots(uint32_t N, uint32_t n_hubs) { return (N + kPgNodesPerBlock - 1) / kPgNodesPerBlock + n_hubs; }
constexpr uint32_t pg_blocks(uint32_t n) { return (n + kPgBlock - 1) / kPgBlock; }
void launch_pg_linearize(hipStream_t s, const PgDev& d, const double* poses, double huber_k);
// sum != 0: H_vv and g_v summed from the edges' contributions first; always: the active rule, the damping and the inverses
void launch_pg_nodes(hipStream_t s, const PgDev& d, double lambda, int sum);
// The conjugate gradients on (H + lambda diag H) x = -g, composed once for every preconditioner.  chain == nullptr: block Jacobi, the
// kernels apply Minv themselves; else the chain factor of launch_pgc_factor at the same lambda, applied by launch_pgc_apply.
struct PgcDev;
void launch_pg_pcg_begin(hipStream_t s, const PgDev& d, const PgcDev* chain, double tol);
void launch_pg_pcg_iteration(hipStream_t s, const PgDev& d, const PgcDev* chain, double lambda, double tol, uint32_t it);
void launch_pg_retract(hipStream_t s, const PgDev& d, const double* poses, double* trial);
// pose graph, priors (elm_k_pgprior.hip; the contract is include/elimaloc_hip_posegraph_prior.h): the device's
// view of a graph's priors, a second allocation.  Prior arrays are component-major with the stride p_stride, the prior capacity.
constexpr uint32_t kPgLanesPerPrior = 8; // k_pgp_linearize: the lane of a group is the column
struct PgPriorDev {
    uint32_t P, p_stride, n_rows;
    const int32_t* node;              // [P]
    const double *Z, *lever, *info;   // [P][12] pose rows, [P][3], [P][36]
    double *r, *J, *s, *w, *g, *H;    // [6], [36], [1], [1], [6], [36] components: g = w J^T Omega r, H = w J^T Omega J
    // the nodes that have priors, ascending: row k is node row_node[k] with the priors order[row_first[k] .. row_first[k + 1]),
    // ascending prior index
    const uint32_t *row_node, *row_first, *order;
    double* part_cost;                // [3][pg_blocks(P)]
};
// r, J, s, w, g, H of every prior at `poses`; P >= 1
void launch_pgp_linearize(hipStream_t s, const PgPriorDev& p, const double* poses, double huber_k);
// onto Hd and g as launch_pg_nodes(sum = 1) left them, each node's priors one by one; n_rows >= 1
void launch_pgp_nodes(hipStream_t s, const PgDev& d, const PgPriorDev& p);
// chi2, cost and outliers at `poses` into d.out, with the largest |x| of the last retraction; want_grad: also max |g_v| over active
// nodes.  prior: null, or the priors (P >= 1) whose three totals, under their own threshold, are added onto the edges' in d.out
void launch_pg_cost(hipStream_t s, const PgDev& d, const PgPriorDev* prior, const double* poses, double huber_k, double prior_huber_k, int want_grad);
// the priors' part of it (elm_k_pgprior.hip), queued after the edges' record is written
void launch_pgp_cost(hipStream_t s, const PgDev& d, const PgPriorDev& p, const double* poses, double huber_k);

// pose graph, chain preconditioner (elm_k_pgchain.hip): M^-1 of the block-tridiagonal M of the contract by
// block cyclic reduction in levels.  A level of n nodes is cut into segments of kPgcSeg consecutive nodes, one workgroup each; a
// workgroup eliminates every node of its segment but the last in odd-even order (log2 kPgcSeg steps), the last nodes of the segments
// are the next level's nodes, and the level of one segment ends the recursion.  Per node and level the factor keeps the inverse pivot
// block G and the two coupling blocks A = G M[p][left], B = G M[p][right].
// kPgcSeg = 256 = kPgBlock: a workgroup's nodes at level 0 are those of one r^T z slot, so the last launch of an apply writes the
// slots k_pg_update<true> writes and k_pg_direction serves both preconditioners; the apply holds only the segment's right-hand side in LDS
// (257 x 6 doubles, 12 KB), the factor works in global memory and holds 64 inversion workspaces (36 KB), so neither is bound by LDS;
// and 2^20 nodes are three levels (five launches per apply), 65 536 two (three launches), 256 one (one launch).
constexpr uint32_t kPgcSeg = 256;
constexpr uint32_t kPgcSteps = 8;        // log2 kPgcSeg
constexpr uint32_t kPgcMaxLevels = 3;    // 256^3 >= 2^20 nodes >= ELM_POSEGRAPH_MAX_NODES
constexpr uint32_t kPgcNoEdge = 0xffffffffu;
static_assert(kPgcSeg == kPgBlock && (1u << kPgcSteps) == kPgcSeg, "the level-0 segments are the r^T z slots");
struct PgcLevel {
    uint32_t n, nseg; // the level's nodes and segments
    uint32_t off;     // its first node in G, A, B, Lw, y (every level padded to whole segments)
    uint32_t soff;    // its first segment in De, bl, be
};
struct PgcDev {
    const uint32_t* ce;     // [N - 1]: the chain edge of v, edge << 1 | (1: stored v + 1 -> v), or kPgcNoEdge
    double *G, *A, *B, *Lw; // [padded nodes of all levels][36]; G holds the running diagonal block until the node is eliminated,
                            // Lw the running coupling to the node's left neighbour
    double* De;             // [segments][36]: what a segment's eliminations add to the diagonal block of the segment before's last node
    double* y;              // [padded nodes][6]: the reduced right-hand side, then the solution
    double *bl, *be;        // [segments][6]: the reduced right-hand side of the segment's last node, and its addition to the one before
};
// the levels of n nodes -> their count
inline uint32_t pgc_levels(uint32_t n, PgcLevel* lv) {
    uint32_t k = 0, off = 0, soff = 0;
    for (;;) {
        const uint32_t nseg = (n + kPgcSeg - 1) / kPgcSeg;
        lv[k++] = PgcLevel{n, nseg, off, soff};
        off += nseg * kPgcSeg;
        soff += nseg;
        if (nseg <= 1 || k == kPgcMaxLevels) return k;
        n = nseg;
    }
}
// the factor of M = chain part of H + lambda diag H (after launch_pg_nodes with the same lambda); N >= 1
void launch_pgc_factor(hipStream_t s, const PgDev& d, const PgcDev& c, double lambda);
// z = M^-1 r of the current residual, and the workgroups' partials of r^T z in the r^T z slots; first: p = z too; gate: nothing is done
// once the stop word of iteration `it` is set.  What launch_pg_pcg_begin and launch_pg_pcg_iteration queue for a chain; N >= 1
void launch_pgc_apply(hipStream_t s, const PgDev& d, const PgcDev& c, uint32_t it, int gate, int first);

// pose graph, covariance columns (elm_k_pgcov.hip; the contract is include/elimaloc_hip_posegraph_cov.h): the
// device's view of one pass of elm_posegraph_covariance, G groups of 64 columns solved together.  Column col0 + 64 g + lane of the call
// is lane `lane` of group g; the vectors are [G][N][6][64], the per-column words [G][64] (rz and stop twice, by the iteration's parity).
constexpr uint32_t kPgcovLanes = 64;         // the columns of a group: the lane is the column
constexpr uint32_t kPgcovNodesPerWave = 4;   // the nodes a wavefront of the per-node kernels takes one after another
constexpr uint32_t kPgcovNodesPerBlock = 4 * kPgcovNodesPerWave;
constexpr uint32_t kPgcovReduceWaves = 16;   // the wavefronts that add a group's slots
constexpr uint32_t kPgcovMaxGroups = 65535;  // grid.y of the per-node kernels
struct PgCovDev {
    uint32_t G, col0, n_cols;     // the pass's groups, its first column (a multiple of 64), the call's columns (6 m)
    const int32_t* col_nodes;     // [m]
    double *x, *r, *z, *p, *q;    // [G][N][6][64]
    double *slot_pq, *slot_rz;    // [pgcov_blocks(N)][G][64]
    double *alpha, *beta, *rz0, *rzf; // [G][64]; rzf: r^T z after the column's last iteration
    double* rz;                   // [2][G][64]
    uint32_t* stop;               // [2][G][64]
    uint32_t *iters, *converged;  // [G][64]
    uint32_t* gstop;              // [2][G]: all 64 columns of the group have stopped
    uint32_t* all_stop;           // [2]: every group has (what the host reads)
    // the chain preconditioner's apply (null with block Jacobi): the reduced right-hand side, then the solution, of every level, and what
    // a segment's eliminations add to the last node of the segment before
    double* y;                    // [G][y_pad][6][64], y_pad the padded nodes of all levels (PgcLevel::off)
    double* be;                   // [G][y_segs][6][64], y_segs the segments of all levels (PgcLevel::soff)
    uint32_t y_pad, y_segs;
};
constexpr uint32_t kPgccovWaves = 16;        // the wavefronts of a (segment, group) workgroup of the chain apply
constexpr uint32_t pgcov_blocks(uint32_t N) { return (N + kPgcovNodesPerBlock - 1) / kPgcovNodesPerBlock; }
// after launch_pg_nodes at the same lambda and a memset of the pass's vectors to zero; N >= 1, 1 <= G <= kPgcovMaxGroups
// chain: null for block Jacobi, else the factor of launch_pgc_factor at the same lambda (c.y and c.be are then set)
void launch_pgcov_begin(hipStream_t s, const PgDev& d, const PgCovDev& c, const PgcDev* chain, double tol);
void launch_pgcov_iteration(hipStream_t s, const PgDev& d, const PgCovDev& c, const PgcDev* chain, double lambda, double tol, uint32_t it);
// out [n_pairs][36]: block k is Sigma(row[k], col_nodes[ci[k]]) as solved; only the entries whose column is in the pass are written
void launch_pgcov_gather(hipStream_t s, const PgDev& d, const PgCovDev& c, const uint32_t* ci, const int32_t* row, uint32_t n_pairs, double* out);

// pose graph, linear initialization (elm_k_pginit.hip; the contract is include/elimaloc_hip_posegraph_init.h).
// The two term kernels fill gi, gj, Hii, Hij, Hjj of the view as launch_pg_linearize does, for launch_pg_nodes (sum = 1, lambda = 0)
// and the conjugate gradients to follow; the apply kernels read the solve's x and the active flags.
constexpr double kPgInitDegenerate = 1e-6; // a node with |rho1|, |rho2|, |u + v| or |u - v| below it keeps its rotation
void launch_pgi_rot_terms(hipStream_t s, const PgDev& d, const double* poses);
void launch_pgi_trans_terms(hipStream_t s, const PgDev& d, const double* poses);
// rows [N][6]: the rows before the projection; slots [pg_blocks(N)]: the workgroups' degenerate counts; trial: every node's pose
void launch_pgi_rot_apply(hipStream_t s, const PgDev& d, const double* poses, double* trial, double* rows, double* slots);
// t <- t + R v of the active nodes, in place
void launch_pgi_trans_apply(hipStream_t s, const PgDev& d, double* trial);
// pose graph, linear initialization with priors (elm_k_pginitp.hip; the contract is
// include/elimaloc_hip_posegraph_init_prior.h).  The term kernel fills g and H of the priors' view as launch_pgp_linearize does, for
// launch_pgp_nodes to follow; weight [P] is the stage's weight of every prior (0: not in the stage); stage 0: rotations, 1: translations.
// P >= 1
void launch_pgip_terms(hipStream_t s, const PgPriorDev& p, const double* poses, const double* weight, int stage);
// out [n_comps][16] = c_a, c_b, S row-major, W of each aligned component from its priors list[first[c] .. first[c + 1]); n_comps >= 1
// and no list empty
void launch_pgip_align_sums(hipStream_t s, const PgPriorDev& p, const double* poses, const double* weight, const uint32_t* first,
                            const uint32_t* list, uint32_t n_comps, double* out);
// comp [N]: the aligned component of the node or -1; xf [n_comps][21] = G row-major, c_a, c_b; in place on trial; N >= 1
void launch_pgip_align_apply(hipStream_t s, uint32_t N, const int32_t* comp, const double* xf, double* trial);

// loop consistency (elm_k_loops.hip; the contract is include/elimaloc_hip_loops.h): the device's view of one call.
// adj is [L][W] with W = lc_words(L); the greedy step `it` reads cand and stop of parity it & 1 and writes those of the other parity.
struct LcState {
    uint32_t stop[2]; // the greedy loop is over for the launches of the step of that parity
    uint32_t size;    // members so far (written by k_lc_pick, read by the host alone)
    uint32_t pad;
};
struct LcDev {
    uint32_t L, W, n, pad;
    const double* poses;            // [n][12] pose rows
    const int32_t *a, *b;           // [L]
    const double *Z, *var_t, *var_r; // [L][12], [L], [L]
    unsigned long long* adj;        // [L][W]
    double* s;                      // [L][L] or null
    unsigned long long* cand;       // [2][W]
    int32_t *deg0, *deg;            // [L]: the degrees of step 0 (the call's degree_out) and of every later step
    uint8_t* member;                // [L]
    LcState* state;
};
constexpr uint32_t lc_words(uint32_t L) { return (L + 63u) / 64u; }
void launch_lc_adjacency(hipStream_t s, const LcDev& d, double q_t, double q_r, double gamma);
// one greedy step: the degrees inside cand, then the pick
void launch_lc_step(hipStream_t s, const LcDev& d, uint32_t it);

// loop consistency with a propagated covariance (elm_k_loopcov.hip; the contract is include/elimaloc_hip_loopcov.h).
// Symmetric 6 x 6 matrices are 21 entries (elm_dev_loopcov.hpp); Wc and rec are component-major: entry c of item i at [c * stride + i].
constexpr uint32_t kLcvScanBlock = 1024; // elements of one block of the prefix sum: two levels reach 2^20 poses
constexpr uint32_t kLcvRecYa = 0, kLcvRecYb = 12, kLcvRecZ = 24, kLcvRecWa = 36, kLcvRecWb = 57, kLcvRecSigma = 78, kLcvRecWords = 99;
struct LcvChain {
    uint32_t n, q_count, nb, pad; // nb: blocks of the scan
    const double* poses;          // [n][12] pose rows
    const double* Q;              // [q_count][21]
    double* Wc;                   // [21][n]
    double* tot;                  // [21][nb] the block totals, scanned in place
};
struct LcvDev {
    uint32_t L, W, Lp, pad;       // Lp: the stride of rec
    const int32_t *a, *b;         // [L]
    const double* Z;              // [L][12]
    const double* Sigma;          // [L][21]
    double* rec;                  // [kLcvRecWords][Lp]
    unsigned long long* adj;      // [L][W]
    uint8_t* nanc;                // [L][W] the pairs of each word whose s is NaN
    int32_t* nan_row;             // [L] their sum per row
    double* s;                    // [L][L] or null
};
// W of the chain, component-major
void launch_lcv_chain(hipStream_t s, const LcvChain& c);
// W_out [n][36] and, when not null, S_out [n][36]
void launch_lcv_expand(hipStream_t s, const LcvChain& c, double* W_out, double* S_out);
// the per-loop records, then the pair terms
void launch_lcv_adjacency(hipStream_t s, const LcvChain& c, const LcvDev& d, double gamma);

// map growth (elm_k_grow.hip): the evidence walk against a table of candidate cells that the end points of the same
// call fill -- cells the map does not occupy and in which beams ended
struct GrowTables { // two open-addressing tables of `mask + 1` slots each, keys packed by grow_key (0 = empty), filled by k_grow_end
    unsigned long long* ckeys;  // coarse cell (fine cell >> 2 per axis)
    unsigned long long* cmasks; // the 64-bit mask of its candidate fine cells (fine_bit), as FineTable's
    unsigned long long* fkeys;  // candidate fine cell
    uint32_t* hit;              // [slots]
    uint32_t* through;          // [slots]
    unsigned long long* sums;   // [slots][3] fixed-point sums of the end points' fractions
    uint32_t* count;            // [1] the candidates
    uint32_t mask;
    int32_t clearance;          // elm_growth_config::clearance_cells
};
constexpr int kGrowLim = 1 << 20; // a cell packs into one 64-bit key when every |c_r| < 2^20 (grow_key, elm_dev_fine.hpp)
constexpr int kGrowEndWords = 7;  // k_grow_end's partial of a chunk: cast, observing, end hit, near, new, out, dropped
constexpr int kGrowWalkWords = 5; // k_grow_walk's: walked, truncated, through beams, through events, steps
constexpr int kGrowWords = kGrowEndWords + kGrowWalkWords;
// jobs / n_chunks as launch_evid_walk; partial [n_chunks][kGrowWords] scratch; stats [n_jobs]; events [jobs[0].n] or nullptr (one job only).
// Three launches on the stream: the end points of all jobs, the walks, the sums -- the kernel boundary is what makes every walk see
// every candidate of its call.
void launch_grow(hipStream_t s, const FineTable& ft, const EvidParams& ep, const GrowTables& gt, const EvidJob* jobs, uint32_t n_jobs,
                 uint32_t n_chunks, uint32_t* partial, elm_growth_stats* stats, uint16_t* events);

// map growth: objects (elm_k_obj.hip): the member cells of a growth object's fine table grouped into connected
// components by a lock-free union-find over its slots, one record per component, and the way back from a slot to its object
struct ObjRecord { // one component while it is on the device; the host turns the listed ones into elm_growth_object
    unsigned long long label;     // the smallest grow_key of the component
    uint32_t n_cells, _pad;
    int32_t lo[3], hi[3];
    unsigned long long hit, through, cell_sum[3];
};
constexpr uint32_t kObjNone = 0xFFFFFFFFu; // parent of a slot that holds no member
constexpr int kObjCounters = 8; // members, roots, listed, small, small cells, max cells, roots beyond the records (always 0), spare
struct ObjTables {
    uint32_t* parent;   // [slots] kObjNone, or a slot of the same component with a smaller index (itself: the root)
    uint32_t* root_id;  // [slots] of a root slot: its record
    ObjRecord* rec;     // [rec_cap] one per root, in the order the roots were met
    uint32_t* listed;   // [rec_cap] the records with n_cells >= min_cells, in the order they were met
    int32_t* rank;      // [rec_cap] of a record: the index of its object in ascending label order, -2 for a small component (host-made)
    uint32_t* counters; // [kObjCounters], zero before launch_obj_find
    uint32_t rec_cap;
};
// The launches of one labelling on the stream: the members by the rule, the unions along the forward half of the neighbourhood
// (connectivity 6, 18 or 26), every member's parent set to its root and the roots numbered, the records reduced, the objects listed.
// max_roots: the candidate count, which bounds the roots (<= rec_cap).
void launch_obj_find(hipStream_t s, const GrowTables& gt, const ObjTables& ot, uint32_t min_hit, uint32_t hit_per_through, uint32_t connectivity,
                     uint32_t min_cells, uint32_t max_roots);
// out[j] = rec[listed[j]], j < n_listed
void launch_obj_gather(hipStream_t s, const ObjTables& ot, uint32_t n_listed, ObjRecord* out);
// out[i] for every beam i < job.n of the scan at the job's pose: the rank of the object its end cell is a member of, -2 in a small
// component, -1 otherwise (ft: the cell size only)
void launch_obj_beams(hipStream_t s, const FineTable& ft, const EvidParams& ep, const GrowTables& gt, const ObjTables& ot, const EvidJob& job,
                      int32_t* out);

// device map build (elm_k_build.hip): the stages elm_build.cpp queues.  All indices are 32-bit (at most 2^31 - 1
// points); every array is the caller's scratch.
constexpr unsigned kBdBadInput = 1u;  // flags: a coordinate is not finite, or its quotient by the voxel size is outside (-2^20, 2^20)
constexpr unsigned kBdTableFull = 2u; // flags: the scratch table took no more keys (cannot happen at its load <= 0.5)
// in-place exclusive scan of a[0 .. n); blk: ceil(n / 1024) words of scratch; *total = the sum
void launch_bd_scan(hipStream_t s, unsigned* a, unsigned n, unsigned* blk, unsigned* total);
// pos[i] = 1 where drop[i] == 0 (scan it); then out[pos[i]] = pts[i] for those points (drop == nullptr: out[i] = pts[i])
void launch_bd_keep(hipStream_t s, const uint8_t* drop, unsigned n, unsigned* pos);
// without drop but with pos (scanned marks, total their sum): out[pos[i]] = pts[i] for the marked points
void launch_bd_compact(hipStream_t s, const float4* pts, const uint8_t* drop, const unsigned* pos, unsigned n, unsigned total, Pt3* out);
// device producers of the same input: pos[i] = 1 where stored point i lies within sqrt(r2) of c (scan it);
// out[pt0[j] + i] = float32(pose of job j applied to its point i), jobs / n_chunks as launch_evid_walk, pt0[n_jobs] the jobs' first points
void launch_bd_keep_within(hipStream_t s, const float4* pts, unsigned n, const double c[3], double r2, unsigned* pos);
void launch_bd_transform(hipStream_t s, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks, const uint32_t* pt0, Pt3* out);
// table / first: 2^cap_log2 >= 2 n entries, all ones before the call; slot: n entries; flags: zero before the call
void launch_bd_insert(hipStream_t s, const Pt3* in, unsigned n, double vs, unsigned long long* table, unsigned* first, unsigned cap_log2,
                      unsigned* slot, unsigned* flags);
// opens[i] = 1 for the first point of every voxel (scan it: the voxel ids in first-seen order, the sum = n_vox)
void launch_bd_opens(hipStream_t s, const unsigned* first, const unsigned* slot, unsigned n, unsigned* opens);
// keys[n_vox][3]; key[i] = voxel id of point i, val[i] = i; raw_cnt[n_vox] (zero before the call) = points per voxel
void launch_bd_vid(hipStream_t s, const unsigned* first, const unsigned* slot, unsigned n, const unsigned* opens, const unsigned long long* table,
                   unsigned* slot_vid, int32_t* keys, unsigned* key, unsigned* val, unsigned* raw_cnt);
// one stable 8-bit pass of the sort by key: histogram (bd_rx_hist_words(n) words), its scan by launch_bd_scan, scatter
size_t bd_rx_hist_words(unsigned n);
void launch_bd_rx_hist(hipStream_t s, const unsigned* key, unsigned n, unsigned shift, unsigned* hist);
void launch_bd_rx_scatter(hipStream_t s, const unsigned* key, const unsigned* val, unsigned n, unsigned shift, const unsigned* start,
                          unsigned* key_out, unsigned* val_out);
// order: the indices grouped by voxel (kept ones compacted to the front of every group on return); off: start of every group;
// kcnt = kstart = kept points per voxel (scan kstart)
void launch_bd_replay(hipStream_t s, const Pt3* in, unsigned* order, const unsigned* off, unsigned n_vox, unsigned n, unsigned cap, double res,
                      unsigned* kcnt, unsigned* kstart);
void launch_bd_emit(hipStream_t s, const Pt3* in, const unsigned* order, const unsigned* vid, const unsigned* off, const unsigned* kcnt,
                    const unsigned* kstart, unsigned n_vox, unsigned n, float4* out, uint2* ranges);

// device build of the cell grid (elm_k_gridbuild.hip): the stages elm_index.cpp queues.  At most 2^31 - 1 points and
// entries; every array but blk / idx / the tile table is the caller's scratch.
// box: lo[3] (INT32_MAX before the call), hi[3] (INT32_MIN): the half-voxel cells of the stored points, without the margin
void launch_gb_box(hipStream_t s, const float4* pts, unsigned n, double vs, int* box);
// key[i] = entry of point i, val[i] = i, cnt[entry] (zero before the call) += 1.  lo: the box with its margin; ny, nz: its cells along y, z
void launch_gb_entry_dense(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t ny, uint64_t nz, unsigned* key,
                           unsigned* val, unsigned* cnt);
// two-level form: zmin (all ones before the call) / zmax (zero) per tile; tcnt[t] = 64 * (nz + 1) or 0, *total (zero before) their 64-bit
// sum; tiles from the exclusive scan of tcnt; then the entries through the tile table
void launch_gb_tile_z(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t tny, unsigned* zmin, unsigned* zmax);
void launch_gb_tile_cnt(hipStream_t s, const unsigned* zmin, const unsigned* zmax, unsigned n_tiles, unsigned* tcnt, unsigned long long* total);
void launch_gb_tiles(hipStream_t s, const unsigned* zmin, const unsigned* zmax, const unsigned* tcnt, unsigned n_tiles, uint2* tiles);
void launch_gb_entry_tiled(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t tny, const uint2* tiles,
                           unsigned* key, unsigned* val, unsigned* cnt);
// a[e] = blocks of entry e (from its count); after launch_bd_scan over the entries: a = grid_start (zero_head: entries forced to 0)
void launch_gb_blocks(hipStream_t s, unsigned* a, unsigned entries);
void launch_gb_start_fin(hipStream_t s, unsigned* a, unsigned entries, unsigned zero_head, const unsigned* total);
void launch_gb_pad(hipStream_t s, GridBlk* blk, uint32_t* idx, uint64_t n_blk);
// skey / sval: the points sorted by entry (stable); every point to slot 4 * start[entry] + its rank in the entry
void launch_gb_fill(hipStream_t s, const float4* pts, const unsigned* skey, const unsigned* sval, unsigned n, const unsigned* start, GridBlk* blk,
                    uint32_t* idx);

struct DeskewDev {
    double time_scan_cur, time_scan_end;
    int32_t imu_pointer_cur;
    int32_t odom_available;
    float incre_x, incre_y, incre_z;
    float _pad;
    const double* imu_time;
    const double* rot_x;
    const double* rot_y;
    const double* rot_z;
};
// ordered device-side VoxelDownsample: table / first sized 2^cap_log2 (table = all ones, first = all ones before the call),
// slot n entries, block_count ceil(n / 1024) entries; *total = kept points, *overflow = 1 when a key does not pack
void launch_voxel_downsample(hipStream_t s, const float* xyz, uint32_t n, double vs, unsigned long long* table, unsigned* first,
                             unsigned cap_log2, unsigned* slot, unsigned* block_count, unsigned* total, int* overflow, Pt3* out);
// Scan ordering on the device (k_scan_order): one workgroup per scan sorts its points along a Hilbert curve over 2 m sensor-frame
// cells (deterministic counting sort, no atomics on the data path).  jobs[j] = {src, dst, n, tmp}; src == dst is not allowed.
struct OrderJob {
    const Pt3* src; // caller's order
    Pt3* dst;       // Hilbert order
    uint32_t* tmp;  // n words of scratch
    uint32_t n;
    uint32_t _pad;
};
void launch_scan_order(hipStream_t s, const OrderJob* jobs, int n_jobs, const uint16_t* hilbert_lut);
// one scan ordered by many workgroups (three launches, the same bytes as k_scan_order); scratch = order_wide_scratch_bytes(n) bytes
unsigned order_wide_groups(unsigned n);
size_t order_wide_scratch_bytes(unsigned n);
void launch_scan_order_wide(hipStream_t s, const OrderJob* job, unsigned n, const uint16_t* hilbert_lut, void* scratch);
void launch_publish_ready(hipStream_t s, StreamCtrl* ctrl, int ready);
void launch_slots_idle(hipStream_t s, ScanDesc* scans, ScanState* st, int slots, unsigned cap_blocks);
constexpr int kOrderCells = 64; // cells per axis of the ordering grid (2 m cells: +-64 m around the sensor, clamped beyond)
void launch_deskew(hipStream_t s, const float* xyz, const float* rel_time, uint32_t n, const DeskewDev& d,
                   float* xyz_out);

// registration information (elm_k_reginfo.hip; the contract is include/elimaloc_hip_reginfo.h)
struct RegInfoJob { // one job: a resident scan at a pose
    const float* pts; // packed xyz
    uint32_t n;       // points
    uint32_t chunk0;  // the job's first 256-point chunk among all chunks of the call
    uint64_t pt0;     // the job's first point among all points of the call (the query points are the jobs' points back to back)
    double rows[12];  // (R_r0, R_r1, R_r2, t_r) per row r
};
// jobs [n_jobs] with ascending chunk0, n_chunks = all chunks of the call (> 0); query [points][3]: g = T p of every point
void launch_reginfo_transform(hipStream_t s, const RegInfoJob* jobs, uint32_t n_jobs, uint32_t n_chunks, double* query);
// pairs: RegParams::q_out of the search at `query` (one word per point; eight for AVGICP); partial [n_chunks][32]
void launch_reginfo_terms(hipStream_t s, const DevMap& m, int method, int metric, double th, const RegInfoJob* jobs, uint32_t n_jobs, uint32_t n_chunks,
                          const int32_t* pairs, double* partial);
// results [n_jobs] from the chunks' partials
void launch_reginfo_finish(hipStream_t s, const RegInfoJob* jobs, uint32_t n_jobs, const double* partial, const elm_reginfo_config& cfg,
                           elm_reginfo_result* results);

} // namespace elm
