// elm_hostapi.hpp -- internal entry points shared by the host translation units (not part of the C ABI): the node callback in
// elm_glue.cpp, the device groups in elm_multi.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/elimaloc_hip.h"

namespace elm { struct DevMap; struct GroundIndex; struct FineTable; }
struct elm_group; // a lead context's group of per-device contexts inside one process (elm_multi.cpp)

namespace elm_host {
constexpr size_t kCbTableRows = 2000;                            // capacity of the IMU deskew tables (pcm.cpp:533-585 caps the queue likewise)
constexpr size_t kCbTableBytes = 65536;                          // 4 tables x 2000 doubles = 64 000 bytes, rounded up
void* callback_staging(elm_ctx* ctx, size_t bytes);
int callback_register(elm_ctx* ctx, const elm_map* map, const void* stage, const float* rel_time, size_t n, const elm_deskew_tables* tab,
                      double voxel_size, const double T0[16], const elm_reg_config* cfg, elm_reg_result* result, uint64_t* n_source,
                      int* unpackable);
// (the structs behind the handles are in elm_host_types.hpp, which needs HIP; what follows DOES something and stays a function)
// ... for elm_multi.cpp
void ctx_set_error(elm_ctx* ctx, const std::string& text);
// ... for elm_reloc.cpp and the map queries (elm_query.hpp)
// The context's query scratch, one grow-only device buffer per role: asking a slot for more bytes than it holds frees what it held, so a
// pointer into a slot is good until the next call that takes that slot.  A call takes its slots, queues its work and joins its stream
// before it returns; nothing is held between calls.
// A global search (elm_relocalize_global) HOLDS kScrPoints, kScrRows (its rotations), kScrBitmap, kScrGroundField and kScrLevelWindows
// from search_setup to its end, over many launches: nothing that runs during a search may take one of those five.  Its batches take
// kScrNodes, kScrNodePartials, kScrNodeOut, kScrLeafIds and kScrLeafRows, and never kScrPartials or kScrStats.
enum ScratchSlot {
    kScrPoints,       // the counted points of a score call or a search
    kScrRows,         // pose rows, or the job table of an accumulate call; a search's rotations (held)
    kScrBitmap,       // the level-0 occupancy bitmap
    kScrPartials,     // per-chunk partial sums
    kScrStats,        // per-pose / per-job stats, or scores
    kScrGroundXY, kScrGroundZ, kScrGroundFound, // elm_map_ground_heights: queries, heights, flags
    kScrNodes, kScrNodePartials, kScrNodeOut,   // a search's batch of nodes, its partials, its bounds or leaf scores
    kScrLeafIds, kScrLeafRows,                  // a search's batch of leaves and their pose rows
    kScrBeamArrays,   // per-beam outputs of a query, per-beam events, elm_growth_beam_objects' output
    kScrWindowTmp,    // search_setup's temporary between the two window passes
    kScrGroundField,  // a search's ground field (held)
    kScrLevelWindows, // a search's level windows (held)
    kScrPlaceWords,   // place recognition: the query descriptors (or a describe call's), then their n_bits
    kScrPlaceMatches, // ... every (query, entry) pair
    kScrPlaceCands,   // ... the query configs, the candidates and their counts
    kScrCount
};
void* ctx_reloc_scratch(elm_ctx* ctx, ScratchSlot slot, size_t bytes, int* rc); // the slot with at least `bytes` (nullptr: *rc)
// the map's ground-field bin index (built at the first call, kept with the map) and the xy bounds of its stored points {x_lo, x_hi, y_lo, y_hi}
int map_ground_index(const elm_map* m, const elm::GroundIndex** gi, double bounds[4]);
// ... for elm_free.cpp
// the map's fine-occupancy table for sub in {1, 2, 4} (built at the first call per sub, kept with the map); info, when given: the host
// milliseconds and device bytes of that build
int map_fine_table(const elm_map* m, int sub, const elm::FineTable** ft, double info[2]);
// the stored points' fine cells for sub, sorted ascending by (x, y, z), duplicates removed
int map_fine_cells(const elm_map* m, int sub, std::vector<int32_t>& cells3);
int free_space_form(); // 0: one ray per lane; 1: ELM_CHECK=free_wave, a wave per ray (the A/B of DESIGN.md section 13)
// ... for elm_ray.cpp
int ray_pose_block(int dflt); // poses per workgroup of k_ray_cast: dflt, or N of ELM_CHECK=ray_poses=N (1 .. 16; the sweep of DESIGN.md section 14)
// ... for elm_evid.cpp
bool ctx_is_alive(const elm_ctx* ctx, uint64_t id); // the context with this unique id still exists (a child may outlive its context)
// the fine cell of every stored point for sub, in elm_map_download_points order: [n_points][3]
int map_point_fine_cells(const elm_map* m, int sub, std::vector<int32_t>& cells3);
// ... for elm_build.cpp
// A map handle around arrays that a device build left in HBM: d_pts float4[n_pts] (w = 0), d_ranges uint2[n_vox], d_keys int32[n_vox][3],
// each allocated with at least 256 bytes.  Keys and ranges come down, the slot table is filled on the host as elm_map_build fills it.
// The arrays are the map's from the call on, released with it or on failure (a failed host allocation throws std::bad_alloc).
int map_adopt(elm_ctx* ctx, void* d_pts, void* d_ranges, void* d_keys, size_t n_pts, size_t n_vox, size_t n_input, double voxel_size,
              int max_points_per_voxel, elm_map** out);
} // namespace elm_host

// Device groups: N per-device contexts inside ONE process behind one lead context (elm_ctx_create_multi; SURVEY 8(b): the reference node is
// one process calling RunRegister).  The public entry points hand a call on the lead context to these; every rank's share runs on that
// rank's worker thread through the same public entry points on its own plain context.
namespace elm_multi {
bool in_worker(); // this thread is a group's worker: the entry points take their single-device path
void destroy(elm_group* g);
int set_work_counters(elm_ctx* lead, int enable);
int map_build(elm_ctx* lead, const float* xyz, size_t n, double voxel_size, int max_points_per_voxel, elm_map** out);
int map_call(elm_map* lead_map, int which, double arg); // 0 CalVoxelCovAll, 1 CalPointCovAll(arg), 2 the search index
int scan_upload(elm_ctx* lead, const float* xyz, size_t n, elm_scan** out);
int reg(elm_ctx* lead, const elm_map* map, const float* scan_xyz, size_t n, const double T0[16], const elm_reg_config* cfg, double T_out[16],
        int* is_success, double* fitness_score, double local_cov[36], elm_reg_result* result, elm_iter_trace* trace);
int reg_batch(elm_ctx* lead, const elm_map* map, elm_scan* const* scans, int count, const double* T0, const elm_reg_config* cfg, int slots,
              elm_reg_result* results, elm_iter_trace* trace); // slots = 0: the lockstep batch
} // namespace elm_multi
