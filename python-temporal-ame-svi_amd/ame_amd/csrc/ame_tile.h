// The dyad-tile machinery shared by ame_predict.hip (scoring, dense blocks, the
// M-step dyad statistics), ame_covar.hip and ame_missing.hip, and the slice
// mapping and final reductions they share with ame_elbo.hip and ame_mstep.hip.
//
// Everything here fixes an order or a layout that results depend on bit for
// bit: the tile size and the tile order, which workgroup takes which (slice,
// tile), which lane holds which dyad, and the order in which partial rows are
// added.  A slice's result is the same under any split of the slices over
// calls and under either slice mapping.
#pragma once
#include "ame_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define AME_DT 64   // dyad tile edge = bits of one packed mask word

__host__ __device__ constexpr int ame_pad4(int k) { return (k + 3) & ~3; }   // K of v_mfma_f32_16x16x4_f32
// 64-bit words of one row of the packed mask Mt
__host__ __device__ constexpr int ame_mask_row_words(int n) { return (n + 63) / 64; }

// LDS row stride of the small-K operand tiles (K <= 36 floats, staged whole):
// a lane reads float lq of row li, and 6 li + lq hits 32 distinct banks per
// half wave.
#define AME_SK_LD 38
static_assert(ame_pad4(AME_MAX_R + 2) <= AME_SK_LD, "a padded [a, 1, u] or U row must fit the LDS row stride");

// ---- tile enumeration ----
// AME_DT x AME_DT tiles of the upper triangle, diagonal tiles included,
// row-major: (0,0) (0,1) .. (1,1) ..
__host__ __device__ inline long long ame_tri_tiles(int n) {
    const long long nb = (n + AME_DT - 1) / AME_DT;
    return nb * (nb + 1) / 2;
}
__host__ __device__ __forceinline__ void ame_tri_tile_origin(int tile, int n, int& I0, int& J0) {
    const int nb = (n + AME_DT - 1) / AME_DT;
    int I = 0, rem = tile;
    while (rem >= nb - I) { rem -= nb - I; ++I; }
    I0 = I * AME_DT;
    J0 = (I + rem) * AME_DT;
}

// ---- slice mapping ----
// Workgroup b of a launch of S slices x per_slice items -> (slice tl, item).
// Workgroup b runs on XCD b % 8: when S is a multiple of 8, all workgroups of
// one slice share an XCD, so the slice's rows are fetched into one L2 instead
// of eight (slice tl sits on XCD tl / (S / 8)).  Otherwise slice-major.
__host__ __device__ __forceinline__ void ame_slice_block(int b, int S, int per_slice, int& tl, int& item) {
    if ((S & 7) == 0) {
        const int k = b >> 3, q = k / per_slice;
        tl = (b & 7) * (S >> 3) + q;
        item = k - q * per_slice;
    } else {
        tl = b / per_slice;
        item = b - tl * per_slice;
    }
}

// ---- lane -> dyad ----
// A workgroup of 4 waves holds a tile's products as v_mfma_f32_16x16x4_f32
// accumulators: wave w owns tile rows 16 w .. 16 w + 15, as four 16 x 16 column
// blocks s.  Element g of block s's accumulator in this lane is the dyad
//   i = I0 + 16 w + 4 lq + g,   j = J0 + 16 s + li,   li = lane & 15, lq = lane >> 4,
// and the lane's MFMA operands are float lq (+ 4 per K step) of row 16 w + li
// (i side) and of row 16 s + li (j side).
struct AmeLaneDyad {
    int I0, J0, li, lq, w;
    __device__ __forceinline__ AmeLaneDyad(int I0_, int J0_) : I0(I0_), J0(J0_) {
        const int lane = threadIdx.x & 63;
        w = threadIdx.x >> 6;
        li = lane & 15;
        lq = lane >> 4;
    }
    __device__ __forceinline__ int i(int g) const { return I0 + 16 * w + 4 * lq + g; }
    __device__ __forceinline__ int j(int s) const { return J0 + 16 * s + li; }
    __device__ __forceinline__ int row(int g) const { return 16 * w + 4 * lq + g; }   // i - I0
    __device__ __forceinline__ int col(int s) const { return 16 * s + li; }           // j - J0
    // float offset of the lane's i-side / j-side operand in a tile of row stride ld
    __device__ __forceinline__ int i_op(int ld) const { return (16 * w + li) * ld + lq; }
    __device__ __forceinline__ int j_op(int s, int ld) const { return (16 * s + li) * ld + lq; }
};
// (i, j) is a pair of the upper triangle of an n-node network
__device__ __forceinline__ bool ame_upper_pair(int i, int j, int n) { return i < n && j < n && i < j; }

// ---- small-K strip product ----
// One 16 x 16 block of the two products m0 = AI . BJ', m1 = BI . AJ' over
// operand tiles staged whole in LDS: ro / co are the lane's i-side / j-side
// operand offsets, k4 the padded K in MFMA steps.
__device__ __forceinline__ void ame_smallk_products(const float* AI, const float* BJ, const float* BI,
                                                    const float* AJ, int ro, int co, int k4, f32x4& m0,
                                                    f32x4& m1) {
    m0 = f32x4{0.f, 0.f, 0.f, 0.f};
    m1 = m0;
    for (int kk = 0; kk < k4; ++kk) {
        m0 = __builtin_amdgcn_mfma_f32_16x16x4f32(AI[ro + 4 * kk], BJ[co + 4 * kk], m0, 0, 0, 0);
        m1 = __builtin_amdgcn_mfma_f32_16x16x4f32(BI[ro + 4 * kk], AJ[co + 4 * kk], m1, 0, 0, 0);
    }
}

// ---- final reductions ----
// Block tree: one workgroup per slice adds its ntile partial rows of NS doubles,
// thread t rows t, t + AME_NT, .. in order, then block_sum.
template <int NS>
static __global__ void __launch_bounds__(AME_NT)
ame_tile_sum_kernel(const double* __restrict__ partial, int ntile, double* __restrict__ out) {
    __shared__ double red[4 * NS];
    const double* ps = partial + (size_t)blockIdx.x * ntile * NS;
    double v[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) v[q] = 0.0;
    for (int b = threadIdx.x; b < ntile; b += AME_NT) {
#pragma unroll
        for (int q = 0; q < NS; ++q) v[q] += ps[(size_t)b * NS + q];
    }
    block_sum<NS>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) out[(size_t)blockIdx.x * NS + q] = v[q];
    }
}

// Serial column sum: out[tl][q] = sum_b partial[(tl rows + b) stride + q0 + q],
// q < nq, one thread per (tl, q) in workgroups of NT, rows added in order from 0.0.
template <int NT>
static __global__ void __launch_bounds__(NT)
ame_col_sum_kernel(const double* __restrict__ partial, int rows, int stride, int q0, int nq, long long total,
                   double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= total) return;
    const long long tl = t / nq;
    const int q = (int)(t - tl * nq);
    const double* p = partial + (size_t)tl * rows * stride + q0 + q;
    double s = 0.0;
    for (int b = 0; b < rows; ++b) s += p[(size_t)b * stride];
    out[t] = s;
}
template <int NT = AME_NT>
static inline void ame_col_sum(const double* partial, int rows, int stride, int q0, int nq, int S, double* out,
                               hipStream_t st) {
    const long long total = (long long)S * nq;
    hipLaunchKernelGGL(ame_col_sum_kernel<NT>, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st,
                       partial, rows, stride, q0, nq, total, out);
}
