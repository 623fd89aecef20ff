// elm_k_obj.hip -- map growth: objects.  The member cells of a growth object (the candidates that the rule calls appeared) grouped into
// connected components on the device, against the object's own fine table (elm_growth_find_objects / _beam_objects; the contract is in
// include/elimaloc_hip.h, "map growth: objects").  Everything works slot-wise over the tables of elm_k_grow.hip,
// which are stable during these launches (plain loads); the only words that change under other lanes' eyes are the union-find's parents,
// read and written with relaxed device-scope atomics.  Every quantity is an integer; a slot index never leaves the device as an identity.
//   K10a k_obj_init     one lane per slot: parent = the slot itself for a member, kObjNone for every other slot
//   K10b k_obj_link     one lane per member: the forward half of its neighbourhood looked up, the two slots united (lock-free)
//   K10c k_obj_flatten  parent = root for every member; every root draws a record and clears it
//   K10d k_obj_reduce   one lane per member: integer atomics on its root's record
//   K10e k_obj_list     one lane per record: the objects (n_cells >= min_cells) appended through one counter, the small ones counted
//   K10f k_obj_gather   the listed records side by side for the download
//   K10g k_obj_beams    one beam per lane: its end cell as k_grow_end forms it, the slot, the root, the root's rank
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

__device__ __forceinline__ uint32_t par_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void par_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of slot x while other lanes unite: a parent is always a slot of the same component with a smaller index, or the slot itself,
// so the way up is strictly descending and ends.  Every slot on the way is pointed at its grandparent (path halving: still an ancestor,
// whatever another lane stores there at the same time).  The loop is bounded by the slot count all the same.
__device__ __forceinline__ uint32_t obj_root(uint32_t* parent, uint32_t x, uint32_t mask) {
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        const uint32_t p = par_load(parent + x);
        if (p == x) return x;
        const uint32_t gp = par_load(parent + p);
        if (gp != p) par_store(parent + x, gp);
        x = gp;
    }
    return x;
}

// the root of slot x once no union runs any more; nothing is written, so that the one store of k_obj_flatten's lane stands
__device__ __forceinline__ uint32_t obj_root_final(const uint32_t* parent, uint32_t x, uint32_t mask) {
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        const uint32_t p = par_load(parent + x);
        if (p == x) return x;
        x = p;
    }
    return x;
}

// Slots a and b become one component: the larger root is hooked under the smaller by one compare-and-swap on the larger root's own word,
// which succeeds only while it still is a root.  A lane that loses looks both roots up again; it never waits for another lane (a lost
// swap means another lane's swap went through, and there are fewer swaps than members).
__device__ __forceinline__ void obj_unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t mask) {
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        a = obj_root(parent, a, mask);
        b = obj_root(parent, b, mask);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
    }
}

__device__ __forceinline__ void key_cell(unsigned long long key, int& x, int& y, int& z) {
    x = (int)((key >> 42) & 0x1FFFFFull) - kGrowLim;
    y = (int)((key >> 21) & 0x1FFFFFull) - kGrowLim;
    z = (int)(key & 0x1FFFFFull) - kGrowLim;
}

// what a slot's member stands for once the objects are ranked: -1 no member, -2 a member of a small component, else the object's index
__device__ __forceinline__ int32_t obj_of_slot(const ObjTables& ot, uint32_t slot) {
    const uint32_t root = ot.parent[slot];
    return root == kObjNone ? -1 : ot.rank[ot.root_id[root]];
}

} // namespace

// K10a
__global__ __launch_bounds__(256) void k_obj_init(const GrowTables gt, const ObjTables ot, uint32_t min_hit, uint32_t hit_per_through) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    bool member = false;
    if (s <= gt.mask) {
        const uint32_t h = gt.hit[s], t = gt.through[s];
        member = gt.fkeys[s] != 0ull && h >= min_hit && (unsigned long long)h >= (unsigned long long)hit_per_through * (unsigned long long)t;
        ot.parent[s] = member ? s : kObjNone;
    }
    const uint32_t n = wave_count(member);
    if ((threadIdx.x & 63u) == 0 && n) (void)atomicAdd(ot.counters + 0, n);
}

// K10b.  The forward half of the neighbourhood: the 13 offsets d > 0 in (x, y, z) order, of which connectivity 6 keeps the 3 with
// |d|_1 = 1 and connectivity 18 the 9 with |d|_1 <= 2 (l1_max).  A neighbour beyond the key range is in no table: it is neither packed
// nor probed.
__global__ __launch_bounds__(256) void k_obj_link(const GrowTables gt, const ObjTables ot, int l1_max) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > gt.mask || ot.parent[s] == kObjNone) return; // (kObjNone is written by k_obj_init only: a plain load)
    int x, y, z;
    key_cell(gt.fkeys[s], x, y, z);
#pragma unroll
    for (int k = 14; k < 27; ++k) { // offset k = (dx + 1) 9 + (dy + 1) 3 + (dz + 1); 13 is the cell itself
        const int dx = k / 9 - 1, dy = (k / 3) % 3 - 1, dz = k % 3 - 1;
        const int l1 = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
        if (l1 > l1_max) continue;
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (!grow_in_range(nx, ny, nz)) continue;
        uint32_t ns = 0;
        if (grow_find(gt.fkeys, gt.mask, hash3(nx, ny, nz), grow_key(nx, ny, nz), ns) && ot.parent[ns] != kObjNone)
            obj_unite(ot.parent, s, ns, gt.mask);
    }
}

// K10c.  No union runs any more: the roots are final.  A root draws the next record and clears it for k_obj_reduce.
__global__ __launch_bounds__(256) void k_obj_flatten(const GrowTables gt, const ObjTables ot, uint32_t max_roots) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > gt.mask || par_load(ot.parent + s) == kObjNone) return;
    const uint32_t root = obj_root_final(ot.parent, s, gt.mask);
    if (root != s) {
        par_store(ot.parent + s, root);
        return;
    }
    const uint32_t id = atomicAdd(ot.counters + 1, 1u);
    if (id >= max_roots || id >= ot.rec_cap) { // more roots than candidates: the host's count is wrong; nothing is written beyond the records
        (void)atomicAdd(ot.counters + 6, 1u);
        ot.root_id[s] = 0u;
        return;
    }
    ot.root_id[s] = id;
    ObjRecord r;
    r.label = ~0ull;
    r.n_cells = 0u;
    r._pad = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.lo[k] = 0x7FFFFFFF;
        r.hi[k] = -0x7FFFFFFF - 1;
        r.cell_sum[k] = 0ull;
    }
    r.hit = 0ull;
    r.through = 0ull;
    ot.rec[id] = r;
}

// K10d
__global__ __launch_bounds__(256) void k_obj_reduce(const GrowTables gt, const ObjTables ot) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > gt.mask) return;
    const uint32_t root = ot.parent[s];
    if (root == kObjNone || ot.counters[6]) return;
    ObjRecord* r = ot.rec + ot.root_id[root];
    const unsigned long long key = gt.fkeys[s];
    int c[3];
    key_cell(key, c[0], c[1], c[2]);
    (void)atomicMin(&r->label, key);
    (void)atomicAdd(&r->n_cells, 1u);
    (void)atomicAdd(&r->hit, (unsigned long long)gt.hit[s]);
    (void)atomicAdd(&r->through, (unsigned long long)gt.through[s]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (void)atomicMin(&r->lo[k], c[k]);
        (void)atomicMax(&r->hi[k], c[k]);
        (void)atomicAdd(&r->cell_sum[k], (unsigned long long)(uint32_t)(c[k] + kGrowLim));
    }
}

// K10e.  One lane per record.  The order of the list is the order in which the lanes arrive: the host sorts by label.
__global__ __launch_bounds__(256) void k_obj_list(const ObjTables ot, uint32_t min_cells, uint32_t max_roots) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_roots = ot.counters[1] < max_roots ? ot.counters[1] : max_roots;
    const bool have = i < n_roots && i < ot.rec_cap && !ot.counters[6];
    const uint32_t n = have ? ot.rec[i].n_cells : 0u;
    const bool listed = have && n >= min_cells, small = have && n < min_cells;
    if (listed) ot.listed[atomicAdd(ot.counters + 2, 1u)] = i;
    const uint32_t n_small = wave_count(small), small_cells = wave_sum(small ? n : 0u);
    uint32_t mx = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (n_small) {
            (void)atomicAdd(ot.counters + 3, n_small);
            (void)atomicAdd(ot.counters + 4, small_cells);
        }
        if (mx) (void)atomicMax(ot.counters + 5, mx);
    }
}

// K10f
__global__ __launch_bounds__(256) void k_obj_gather(const ObjTables ot, uint32_t n_listed, ObjRecord* __restrict__ out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_listed) return;
    const uint32_t i = ot.listed[j];
    if (i < ot.rec_cap) out[j] = ot.rec[i];
}

// K10g.  The beam, the window and the end cell exactly as in k_grow_end; then the fine table, the root and its rank.  The map's own
// table is not read (ft: the cell size only).
__global__ __launch_bounds__(256) void k_obj_beams(const FineTable ft, const EvidParams ep, const GrowTables gt, const ObjTables ot, const EvidJob job,
                                                   int32_t* __restrict__ out) {
    const PoseRows P = load_pose_rows(job.rows);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const Beam b = load_beam(job.pts, i, job.n, ep.ox, ep.oy, ep.oz);
    const bool obs = b.cast && in_window(b.L2, ep.obs_min_r2, ep.obs_max_r2);
    int32_t v = -1;
    if (obs) {
        double q0, q1, q2;
        pose_apply(P, b.px, b.py, b.pz, q0, q1, q2);
        const bool ex = ft.inv_cell_exact != 0.0;
        const double v0 = ex ? q0 * ft.inv_cell_exact : q0 / ft.cell, v1 = ex ? q1 * ft.inv_cell_exact : q1 / ft.cell;
        const double v2 = ex ? q2 * ft.inv_cell_exact : q2 / ft.cell;
        const int e0 = (int)floor(v0), e1 = (int)floor(v1), e2 = (int)floor(v2);
        uint32_t slot = 0;
        if (grow_in_range(e0, e1, e2) && grow_find(gt.fkeys, gt.mask, hash3(e0, e1, e2), grow_key(e0, e1, e2), slot)) v = obj_of_slot(ot, slot);
    }
    if (b.valid) out[i] = v;
}

void launch_obj_find(hipStream_t s, const GrowTables& gt, const ObjTables& ot, uint32_t min_hit, uint32_t hit_per_through, uint32_t connectivity,
                     uint32_t min_cells, uint32_t max_roots) {
    const dim3 grid((gt.mask + 256u) / 256u), block(256);
    const int l1_max = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    hipLaunchKernelGGL(k_obj_init, grid, block, 0, s, gt, ot, min_hit, hit_per_through);
    hipLaunchKernelGGL(k_obj_link, grid, block, 0, s, gt, ot, l1_max);
    hipLaunchKernelGGL(k_obj_flatten, grid, block, 0, s, gt, ot, max_roots);
    hipLaunchKernelGGL(k_obj_reduce, grid, block, 0, s, gt, ot);
    if (max_roots) hipLaunchKernelGGL(k_obj_list, dim3((max_roots + 255u) / 256u), block, 0, s, ot, min_cells, max_roots);
}

void launch_obj_gather(hipStream_t s, const ObjTables& ot, uint32_t n_listed, ObjRecord* out) {
    if (n_listed) hipLaunchKernelGGL(k_obj_gather, dim3((n_listed + 255u) / 256u), dim3(256), 0, s, ot, n_listed, out);
}

void launch_obj_beams(hipStream_t s, const FineTable& ft, const EvidParams& ep, const GrowTables& gt, const ObjTables& ot, const EvidJob& job,
                      int32_t* out) {
    if (job.n) hipLaunchKernelGGL(k_obj_beams, dim3((job.n + 255u) / 256u), dim3(256), 0, s, ft, ep, gt, ot, job, out);
}

} // namespace elm
