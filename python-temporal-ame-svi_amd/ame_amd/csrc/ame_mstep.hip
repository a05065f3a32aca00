// State statistics of the M-step (ame_mstep_stats, include/ame_amd.h):
//   P_t = sum_i (m_it m_it' + S_it),   C_t = sum_i m_it m_i,t-1'   (C_t = 0 at global slice 0)
// per local slice, d x d fp64.  d is a runtime value: one kernel serves every r.
//
// K1 ame_mstep_state_kernel: one workgroup per (slice, chunk of AME_MS_CHUNK
//    nodes).  The chunk's means of slices t and t-1 are staged in LDS once;
//    thread `tid` owns matrix elements tid, tid + 256, ... (K of them, at most 18
//    at d = 66) and keeps their P and C partials in fp64 registers while the
//    workgroup streams the chunk's covariances node by node, each a contiguous
//    run of d^2 floats read once with coalesced loads (one node prefetched into
//    registers ahead of the sums).  Every product and every sum is fp64.  The
//    partials go to `work`.
// K2 ame_col_sum_kernel (ame_tile.h): one thread per output element adds the
//    chunk partials in chunk order.
// The chunk size is a constant, so the summation order of a slice's row does
// not depend on T_local, t_begin or how the caller splits slices over calls.
// Bandwidth-bound by design: the covariances are the only large read (4 d^2
// bytes per node and slice) and nothing of that size is written.
#include "ame_tile.h"
#include "ame_internal.h"

#define AME_MS_CHUNK 32                      // nodes per workgroup
#define AME_MS_MAXD (2 + 2 * AME_MAX_R)      // 66

template <int K>
__global__ void __launch_bounds__(AME_NT)
ame_mstep_state_kernel(const float* __restrict__ x, const float* __restrict__ cov,
                       const float* __restrict__ prev_final, int n, int d, int nchunk, int t_begin,
                       double* __restrict__ partial) {
    __shared__ float sm[AME_MS_CHUNK * AME_MS_MAXD], sp[AME_MS_CHUNK * AME_MS_MAXD];
    const int dd = d * d, tid = threadIdx.x;
    const int tl = blockIdx.x / nchunk, ch = blockIdx.x - tl * nchunk;
    const int i0 = ch * AME_MS_CHUNK;
    const int cnt = (n - i0 < AME_MS_CHUNK) ? n - i0 : AME_MS_CHUNK;
    const bool has_prev = t_begin + tl > 0;   // uniform over the workgroup
    const float* xs = x + ((size_t)tl * n + i0) * d;
    const float* xp = (tl > 0) ? x + ((size_t)(tl - 1) * n + i0) * d
                               : (has_prev ? prev_final + (size_t)i0 * d : nullptr);
    for (int e = tid; e < cnt * d; e += AME_NT) {
        sm[e] = xs[e];
        sp[e] = has_prev ? xp[e] : 0.f;
    }
    __syncthreads();

    int ra[K], rb[K];
    double P[K], C[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + AME_NT * k;
        const int a = (e < dd) ? e / d : 0;
        ra[k] = a;
        rb[k] = (e < dd) ? e - a * d : 0;
        P[k] = 0.0;
        C[k] = 0.0;
    }
    const float* cv = cov + ((size_t)tl * n + i0) * (size_t)dd;
    // The next node's covariance loads are issued before this node's sums, so
    // every wave always has loads in flight: 0.24 -> 0.16 ms at n = 1024,
    // T = 128, r = 16 for K more registers (66 VGPRs at d = 34, 7 waves per
    // SIMD).  Four nodes ahead cost 124 VGPRs (4 waves per SIMD) and measured
    // 0.39 ms.
    float c[K], cn[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + AME_NT * k;
        cn[k] = (e < dd) ? cv[e] : 0.f;
    }
    for (int i = 0; i < cnt; ++i) {
        const float* ci = cv + (size_t)(i + 1) * dd;
        const float* mi = sm + i * d;
        const float* pi = sp + i * d;
#pragma unroll
        for (int k = 0; k < K; ++k) {   // the next node's loads fly during this node's sums
            const int e = tid + AME_NT * k;
            c[k] = cn[k];
            cn[k] = (i + 1 < cnt && e < dd) ? ci[e] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double ma = (double)mi[ra[k]], mb = (double)mi[rb[k]];
            P[k] += (double)c[k] + ma * mb;
            if (has_prev) C[k] += ma * (double)pi[rb[k]];
        }
    }
    double* o = partial + ((size_t)tl * nchunk + ch) * 2 * (size_t)dd;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + AME_NT * k;
        if (e < dd) {
            o[e] = P[k];
            o[dd + e] = C[k];
        }
    }
}

static inline int mstep_chunks(int n) { return (n + AME_MS_CHUNK - 1) / AME_MS_CHUNK; }

long long ame_mstep_state_work_doubles(const ame_dims* dm) {
    const long long d = 2 + 2 * dm->r;
    return (long long)dm->T_local * mstep_chunks(dm->n) * 2 * d * d;
}

long long ame_mstep_state_blocks(const ame_dims* dm) {
    return (long long)dm->T_local * mstep_chunks(dm->n);
}

int ame_mstep_state_dispatch(const ame_dims* dm, const ame_mstep_args* a, hipStream_t st) {
    const int n = dm->n, d = 2 + 2 * dm->r, dd = d * d, nchunk = mstep_chunks(n);
    const unsigned grid = (unsigned)((long long)dm->T_local * nchunk);
    const int K = (dd + AME_NT - 1) / AME_NT;
#define AME_MS_LAUNCH(KK)                                                                          \
    hipLaunchKernelGGL(ame_mstep_state_kernel<KK>, dim3(grid), dim3(AME_NT), 0, st, a->x, a->cov, \
                       a->prev_final, n, d, nchunk, dm->t_begin, a->work)
    if (K <= 1) AME_MS_LAUNCH(1);
    else if (K <= 2) AME_MS_LAUNCH(2);
    else if (K <= 5) AME_MS_LAUNCH(5);
    else if (K <= 10) AME_MS_LAUNCH(10);
    else if (K <= 18) AME_MS_LAUNCH(18);
    else return -1;
#undef AME_MS_LAUNCH
    // out[tl][which][e] = sum over chunks, in chunk order
    ame_col_sum(a->work, nchunk, 2 * dd, 0, 2 * dd, dm->T_local, a->state, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
