// elm_k_reginfo.hip -- registration information (include/elimaloc_hip_reginfo.h): k_ri_transform (the jobs' points
// as float64 query points in the map frame), k_ri_terms (the pairs' terms, one partial per 256-point chunk) and k_ri_finish (a job's sums
// in the fixed order of the contract, the 6 x 6 Jacobi and the information).  The pair search between the first two is the QUERY
// instantiation of the production search, launched by the host as elm_map_get_correspondences launches it.
#include <hip/hip_runtime.h>

#include "elm_internal.hpp"
#include "elm_la.hpp"
#include "elm_dev_pairs.hpp"
#include "elm_dev_reginfo.hpp"

namespace elm {

__device__ __forceinline__ const RegInfoJob* ri_job_of_chunk(const RegInfoJob* __restrict__ jobs, uint32_t n_jobs, uint32_t chunk) {
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].chunk0 <= chunk) lo = mid;
        else hi = mid;
    }
    return jobs + lo;
}

// g = T p with the association of k_accumulate_direct
__global__ __launch_bounds__(256) void k_ri_transform(const RegInfoJob* __restrict__ jobs, uint32_t n_jobs, double* __restrict__ query) {
    const RegInfoJob* J = ri_job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    if (i >= J->n) return;
    const double px = J->pts[3 * (size_t)i], py = J->pts[3 * (size_t)i + 1], pz = J->pts[3 * (size_t)i + 2];
    double* q = query + 3 * (J->pt0 + i);
    q[0] = ((J->rows[0] * px + J->rows[1] * py) + J->rows[2] * pz) + J->rows[3];
    q[1] = ((J->rows[4] * px + J->rows[5] * py) + J->rows[6] * pz) + J->rows[7];
    q[2] = ((J->rows[8] * px + J->rows[9] * py) + J->rows[10] * pz) + J->rows[11];
}

template <int METHOD, int METRIC>
__device__ __forceinline__ void ri_add(double* acc, const double* rows, double px, double py, double pz, double mx, double my, double mz,
                                       const double* S, const double* nrm, double th, bool dflt) {
    RegInfoPair t;
    if (!reginfo_pair<METHOD, METRIC>(rows, px, py, pz, mx, my, mz, S, nrm, th, t)) return;
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[kRiH + k] += t.w * t.Ht[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[kRiG + k] += t.w * t.gt[k];
    acc[kRiChi2] += t.w * t.chi;
    acc[kRiSw] += t.w;
    acc[kRiSwr2] += t.w * ((px * px + py * py) + pz * pz);
    acc[kRiPairs] += 1.0;
    if (dflt) acc[kRiDefault] += 1.0;
}

// One thread per point of a chunk; up to seven pairs per point for AVGICP.  pairs as RegParams::q_out.
template <int METHOD, int METRIC>
__global__ __launch_bounds__(256) void k_ri_terms(const DevMap m, const double th, const RegInfoJob* __restrict__ jobs, uint32_t n_jobs,
                                                  const int32_t* __restrict__ pairs, double* __restrict__ partial) {
    constexpr bool PLANE = METRIC == ELM_REGINFO_METRIC_PLANE;
    const RegInfoJob* J = ri_job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    double acc[kRiWords];
#pragma unroll
    for (int k = 0; k < kRiWords; ++k) acc[k] = 0.0;
    if (i < J->n) {
        double rows[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) rows[k] = J->rows[k];
        const double px = J->pts[3 * (size_t)i], py = J->pts[3 * (size_t)i + 1], pz = J->pts[3 * (size_t)i + 2];
        const size_t gi = (size_t)(J->pt0 + i);
        if (METHOD == ELM_P2P || METHOD == ELM_GICP) {
            const int32_t t = pairs[gi];
            if (t >= 0 && (uint32_t)t < m.n_pts) {
                const double* rec = (METHOD == ELM_GICP || PLANE) ? m.pt_gicp + (size_t)t * 16 : nullptr;
                double mx, my, mz;
                if (METHOD == ELM_GICP) { mx = rec[0]; my = rec[1]; mz = rec[2]; }
                else { const float4 q = m.pts[t]; mx = q.x; my = q.y; mz = q.z; }
                ri_add<METHOD, METRIC>(acc, rows, px, py, pz, mx, my, mz, METHOD == ELM_GICP ? rec + 3 : nullptr, PLANE ? rec + 12 : nullptr, th, false);
            } else if (t == -1 && !PLANE) {
                ri_add<METHOD, ELM_REGINFO_METRIC_METHOD>(acc, rows, px, py, pz, 0.0, 0.0, 0.0, nullptr, nullptr, th, true);
            }
        } else if (METHOD == ELM_VGICP) {
            const int32_t v = pairs[gi];
            if (v >= 0 && (uint32_t)v < m.n_vox)
                ri_add<METHOD, METRIC>(acc, rows, px, py, pz, m.vox_mean[(size_t)v * 3], m.vox_mean[(size_t)v * 3 + 1], m.vox_mean[(size_t)v * 3 + 2],
                                       m.vox_cinv + (size_t)v * 9, nullptr, th, false);
            else if (v == -1)
                ri_add<METHOD, METRIC>(acc, rows, px, py, pz, 0.0, 0.0, 0.0, nullptr, nullptr, th, true);
        } else {
            for (int r = 0; r < 7; ++r) {
                const int32_t v = pairs[8 * gi + r];
                if (v >= 0 && (uint32_t)v < m.n_vox)
                    ri_add<METHOD, METRIC>(acc, rows, px, py, pz, m.vox_mean[(size_t)v * 3], m.vox_mean[(size_t)v * 3 + 1], m.vox_mean[(size_t)v * 3 + 2],
                                           m.vox_cinv + (size_t)v * 9, nullptr, th, false);
            }
        }
    }
    __shared__ double red[4][kRiWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kRiWords; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)kRiWords)
        partial[(size_t)blockIdx.x * kRiWords + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// One wavefront per job: lane k < 32 adds word k of the job's chunks in ascending order onto a sum that starts at 0, lane 0 finishes.
__global__ __launch_bounds__(64) void k_ri_finish(const RegInfoJob* __restrict__ jobs, uint32_t n_jobs, const double* __restrict__ partial,
                                                  const elm_reginfo_config cfg, elm_reginfo_result* __restrict__ results) {
    const uint32_t j = blockIdx.x;
    if (j >= n_jobs) return;
    const RegInfoJob& J = jobs[j];
    const uint32_t nc = (J.n + 255u) / 256u;
    __shared__ double sums[kRiWords];
    if (threadIdx.x < (unsigned)kRiWords) {
        double s = 0.0;
        for (uint32_t c = 0; c < nc; ++c) s += partial[(size_t)(J.chunk0 + c) * kRiWords + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        elm_reginfo_result r;
        reginfo_finish(sums, cfg, cfg.metric == ELM_REGINFO_METRIC_PLANE ? 1 : 3, (int32_t)J.n, r);
        results[j] = r;
    }
}

void launch_reginfo_transform(hipStream_t s, const RegInfoJob* jobs, uint32_t n_jobs, uint32_t n_chunks, double* query) {
    hipLaunchKernelGGL(k_ri_transform, dim3(n_chunks), dim3(256), 0, s, jobs, n_jobs, query);
}

void launch_reginfo_terms(hipStream_t s, const DevMap& m, int method, int metric, double th, const RegInfoJob* jobs, uint32_t n_jobs, uint32_t n_chunks,
                          const int32_t* pairs, double* partial) {
    const dim3 g(n_chunks), b(256);
#define ELM_LAUNCH(M, Q) hipLaunchKernelGGL((k_ri_terms<M, Q>), g, b, 0, s, m, th, jobs, n_jobs, pairs, partial)
    if (metric == ELM_REGINFO_METRIC_PLANE) {
        if (method == ELM_P2P) ELM_LAUNCH(ELM_P2P, ELM_REGINFO_METRIC_PLANE);
        else ELM_LAUNCH(ELM_GICP, ELM_REGINFO_METRIC_PLANE);
    } else {
        switch (method) {
        case ELM_P2P: ELM_LAUNCH(ELM_P2P, ELM_REGINFO_METRIC_METHOD); break;
        case ELM_GICP: ELM_LAUNCH(ELM_GICP, ELM_REGINFO_METRIC_METHOD); break;
        case ELM_VGICP: ELM_LAUNCH(ELM_VGICP, ELM_REGINFO_METRIC_METHOD); break;
        default: ELM_LAUNCH(ELM_AVGICP, ELM_REGINFO_METRIC_METHOD); break;
        }
    }
#undef ELM_LAUNCH
}

void launch_reginfo_finish(hipStream_t s, const RegInfoJob* jobs, uint32_t n_jobs, const double* partial, const elm_reginfo_config& cfg,
                           elm_reginfo_result* results) {
    hipLaunchKernelGGL(k_ri_finish, dim3(n_jobs), dim3(64), 0, s, jobs, n_jobs, partial, cfg, results);
}

} // namespace elm
