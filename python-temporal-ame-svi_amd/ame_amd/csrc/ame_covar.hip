// Dyadic-covariate statistics and the residual network (ame_covar_stats,
// ame_covar_resid, include/ame_amd.h).
//
// With y_ij = mu_ij + sum_k beta_k w_k,ij + eps, the M-step for beta needs, per
// slice and over the upper triangle i < j (Yt[t][i][j], Wt[k][t][i][j] as the
// observation 2-vectors),
//   G[k][a][b]    = sum w_k[a] e[b],       e = y~ - E[mu_ij]  (y~: the residual Yt)
//   H[k][l][a][b] = sum w_k[a] w_l[b]
//
// K1 ame_covar_g_kernel<P>: one workgroup per (slice, 64 x 64 tile of the upper
//    triangle, diagonal tiles included).  The tile's node rows are staged in
//    LDS as Ma = [a, 1, u] and Mb = [1, b, v] (K zero-padded to a multiple of 4)
//    and the two products Ma_I.Mb_J' = E[mu_ij[0]], Mb_I.Ma_J' = E[mu_ij[1]] run
//    on v_mfma_f32_16x16x4_f32 (ame_tile.h: tile order, lane -> dyad layout,
//    small-K strip product), 16 dyads per lane.  e is formed in fp32 from the
//    Yt tile (0 where i >= j or beyond n); the P covariate tiles are read once
//    each and w[a] e[b] is accumulated in fp64 registers (products of fp32
//    values are exact in fp64).
// K1h ame_covar_h_kernel<P>: the same tiles for H, without the means; see there.
// K2 ame_col_sum_kernel (ame_tile.h): one thread per statistic adds a slice's
//    tile partials in tile order, G and H each in a launch of their own.
// K3 ame_covar_resid_kernel: Yt = Yt_raw - sum_k beta_k Wt[k], elementwise over
//    the packed layout, float4 per thread, fp64 with every product and sum
//    rounded on its own, one rounding to fp32.
// The tile size is a constant and every sum has a fixed order: a slice's row has
// the same bits under any split of the slices over calls.  No atomics, no
// waits, nothing of size n^2 written by K1 / K2.
#include "ame_tile.h"
#include "ame_internal.h"

// doubles of one partial / output row: G (4 p) then H (4 p^2)
__host__ __device__ constexpr int ame_covar_row(int p) { return 4 * p + 4 * p * p; }

template <int P>
__global__ void __launch_bounds__(AME_NT)
ame_covar_g_kernel(const float* __restrict__ x, const float* __restrict__ Yt,
                   const float* __restrict__ Wt, int n, int r, int T_local, int ntile,
                   double* __restrict__ partial) {
    constexpr int NG = 4 * P;
    __shared__ float MaI[AME_DT * AME_SK_LD], MbI[AME_DT * AME_SK_LD];
    __shared__ float MaJ[AME_DT * AME_SK_LD], MbJ[AME_DT * AME_SK_LD];
    __shared__ double red[4 * NG];

    const int tl = blockIdx.x / ntile, tile = blockIdx.x - tl * ntile;
    int I0, J0;
    ame_tri_tile_origin(tile, n, I0, J0);
    const int d = 2 + 2 * r, mp = ame_pad4(r + 2);
    const AmeLaneDyad ld(I0, J0);

    // stage Ma = [a, 1, u, 0..], Mb = [1, b, v, 0..] of the tile's row and column nodes
    {
        const int row = threadIdx.x >> 2;
        const int ni = I0 + row, nj = J0 + row;
        const float* xi = x + ((size_t)tl * n + (ni < n ? ni : 0)) * d;
        const float* xj = x + ((size_t)tl * n + (nj < n ? nj : 0)) * d;
        for (int c = threadIdx.x & 3; c < mp; c += 4) {
            float ai, bi, aj, bj;
            if (c == 0) {
                ai = xi[0]; bi = 1.f; aj = xj[0]; bj = 1.f;
            } else if (c == 1) {
                ai = 1.f; bi = xi[1]; aj = 1.f; bj = xj[1];
            } else if (c < r + 2) {
                ai = xi[c]; bi = xi[c + r]; aj = xj[c]; bj = xj[c + r];
            } else {
                ai = bi = aj = bj = 0.f;
            }
            if (ni >= n) ai = bi = 0.f;
            if (nj >= n) aj = bj = 0.f;
            MaI[row * AME_SK_LD + c] = ai;
            MbI[row * AME_SK_LD + c] = bi;
            MaJ[row * AME_SK_LD + c] = aj;
            MbJ[row * AME_SK_LD + c] = bj;
        }
    }
    __syncthreads();

    // The wave's 16 x 64 strip goes by 16 x 16 blocks (s): the block's two MFMA
    // products, then its 4 dyads per lane.  The s loop is not unrolled, so the
    // loads in flight are one block's (4 (P + 1) float2 per lane).
    const int ny = ame_ystride(n);
    const size_t plane = (size_t)T_local * n * ny * 2;   // floats of one packed plane
    const size_t sbase = (size_t)tl * n * ny * 2;
    const int ro = ld.i_op(AME_SK_LD);
    double acc[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const int j = ld.j(s);
        f32x4 m0, m1;
        ame_smallk_products(MaI, MbJ, MbI, MaJ, ro, ld.j_op(s, AME_SK_LD), mp >> 2, m0, m1);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = ld.i(g);
            const bool ok = ame_upper_pair(i, j, n);
            const size_t o = sbase + ((size_t)(ok ? i : 0) * ny + (ok ? j : 0)) * 2;
            float2 wk[P];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                wk[k] = *(const float2*)(Wt + k * plane + o);
                if (!ok) wk[k] = make_float2(0.f, 0.f);
            }
            const float2 y = *(const float2*)(Yt + o);
            const float e0f = ok ? y.x - m0[g] : 0.f, e1f = ok ? y.y - m1[g] : 0.f;
            const double e0 = (double)e0f, e1 = (double)e1f;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double w0 = (double)wk[k].x, w1 = (double)wk[k].y;
                acc[4 * k + 0] += w0 * e0;
                acc[4 * k + 1] += w0 * e1;
                acc[4 * k + 2] += w1 * e0;
                acc[4 * k + 3] += w1 * e1;
            }
        }
    }
    block_sum<NG>(acc, red);
    if (threadIdx.x == 0) {
        double* o = partial + (size_t)blockIdx.x * ame_covar_row(P);
#pragma unroll
        for (int q = 0; q < NG; ++q) o[q] = acc[q];
    }
}

// H of one tile.  H depends on the data alone and the engine asks for it once,
// so this kernel is kept small instead of sharing the G kernel's pass: the row
// blocks H[k][k..P-1] are summed one k at a time (4 P fp64 sums per lane; all
// 2 P (P + 1) at once need more registers than a wave has at P = 8).  Plane k
// comes from HBM when its row block is summed, planes l > k are read again, by
// the same workgroup, right after it first read them.  The k <= l half is
// summed and mirrored: H[k][l][a][b] == H[l][k][b][a] bit for bit (on k == l the
// two off-diagonal sums add the same products in the same order).
template <int P>
__global__ void __launch_bounds__(AME_NT)
ame_covar_h_kernel(const float* __restrict__ Wt, int n, int T_local, int ntile,
                   double* __restrict__ partial) {
    constexpr int NH = 4 * P;
    __shared__ double red[4 * NH];
    const int tl = blockIdx.x / ntile, tile = blockIdx.x - tl * ntile;
    int I0, J0;
    ame_tri_tile_origin(tile, n, I0, J0);
    const AmeLaneDyad ld(I0, J0);
    const int ny = ame_ystride(n);
    const size_t plane = (size_t)T_local * n * ny * 2;
    const size_t sbase = (size_t)tl * n * ny * 2;
    double* H = partial + (size_t)blockIdx.x * ame_covar_row(P) + 4 * P;   // [P][P][2][2]
#pragma unroll 1
    for (int k = 0; k < P; ++k) {
        double acc[NH];
#pragma unroll
        for (int q = 0; q < NH; ++q) acc[q] = 0.0;
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                const bool ok = ame_upper_pair(i, j, n);
                const size_t o = sbase + ((size_t)(ok ? i : 0) * ny + (ok ? j : 0)) * 2;
                float2 wk = *(const float2*)(Wt + k * plane + o);
                if (!ok) wk = make_float2(0.f, 0.f);
                const double w0 = (double)wk.x, w1 = (double)wk.y;
#pragma unroll
                for (int l = 0; l < P; ++l) {
                    if (l >= k) {   // uniform over the workgroup
                        float2 wl = *(const float2*)(Wt + l * plane + o);
                        if (!ok) wl = make_float2(0.f, 0.f);
                        const double v0 = (double)wl.x, v1 = (double)wl.y;
                        acc[4 * l + 0] += w0 * v0;
                        acc[4 * l + 1] += w0 * v1;
                        acc[4 * l + 2] += w1 * v0;
                        acc[4 * l + 3] += w1 * v1;
                    }
                }
            }
        }
        block_sum<NH>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int l = 0; l < P; ++l) {
                if (l >= k) {
                    double* kl = H + (size_t)(k * P + l) * 4;
                    double* lk = H + (size_t)(l * P + k) * 4;
                    kl[0] = lk[0] = acc[4 * l + 0];
                    kl[1] = lk[2] = acc[4 * l + 1];
                    kl[2] = lk[1] = acc[4 * l + 2];
                    kl[3] = lk[3] = acc[4 * l + 3];
                }
            }
        }
        __syncthreads();   // `red` is reused by the next row block
    }
}

struct CovarBeta {
    double b[AME_MAX_COVARIATES];
};

// s + b * w and y - s with the product, the sum and the difference each rounded
// to fp64 on its own: plain operators inside the pragma's scope, as mul_add_rn
// (ame_common.h) -- __dmul_rn / __dadd_rn are header inlines compiled under
// -ffp-contract=fast, which the pragma of a caller does not reach.
__device__ __forceinline__ double covar_mul_then_add(double s, double b, double w) {
#pragma clang fp contract(off)
    const double t = b * w;
    return s + t;
}
__device__ __forceinline__ float covar_sub_round(float y, double s) {
#pragma clang fp contract(off)
    const double d = (double)y - s;
    return (float)d;
}

template <int P>
__global__ void __launch_bounds__(AME_NT)
ame_covar_resid_kernel(const float4* __restrict__ Yraw, const float4* __restrict__ Wt, CovarBeta beta,
                       long long plane4, float4* __restrict__ out) {
    const long long e = (long long)blockIdx.x * AME_NT + threadIdx.x;
    if (e >= plane4) return;
    float4 wv[P];
#pragma unroll
    for (int k = 0; k < P; ++k) wv[k] = Wt[(size_t)k * plane4 + e];
    const float4 y = Yraw[e];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        s0 = covar_mul_then_add(s0, beta.b[k], (double)wv[k].x);
        s1 = covar_mul_then_add(s1, beta.b[k], (double)wv[k].y);
        s2 = covar_mul_then_add(s2, beta.b[k], (double)wv[k].z);
        s3 = covar_mul_then_add(s3, beta.b[k], (double)wv[k].w);
    }
    float4 o;
    o.x = covar_sub_round(y.x, s0);
    o.y = covar_sub_round(y.y, s1);
    o.z = covar_sub_round(y.z, s2);
    o.w = covar_sub_round(y.w, s3);
    out[e] = o;
}

long long ame_covar_work_doubles(const ame_dims* dm, int p) {
    return (long long)dm->T_local * ame_tri_tiles(dm->n) * ame_covar_row(p);
}

long long ame_covar_blocks(const ame_dims* dm) { return (long long)dm->T_local * ame_tri_tiles(dm->n); }

// float4 elements of one packed plane (ny is even: a plane is whole float4s)
long long ame_covar_plane4(const ame_dims* dm) {
    return (long long)dm->T_local * dm->n * ame_ystride(dm->n) / 2;
}

template <int P>
static void launch_covar_tile(const ame_dims* dm, const ame_covar_args* a, int ntile, hipStream_t st) {
    const unsigned grid = (unsigned)((long long)dm->T_local * ntile);
    if (a->G)
        hipLaunchKernelGGL(ame_covar_g_kernel<P>, dim3(grid), dim3(AME_NT), 0, st, a->x, a->Yt, a->Wt, dm->n,
                           dm->r, dm->T_local, ntile, a->work);
    if (a->H)
        hipLaunchKernelGGL(ame_covar_h_kernel<P>, dim3(grid), dim3(AME_NT), 0, st, a->Wt, dm->n, dm->T_local,
                           ntile, a->work);
}

int ame_covar_stats_dispatch(const ame_dims* dm, const ame_covar_args* a, hipStream_t st) {
    const int ntile = (int)ame_tri_tiles(dm->n), p = a->p;
    switch (p) {
#define X(PP) \
    case PP: launch_covar_tile<PP>(dm, a, ntile, st); break;
        AME_FOR_EACH_P(X)
#undef X
        default: return -1;
    }
    const int row = ame_covar_row(p), ng = 4 * p;
    if (a->G) ame_col_sum(a->work, ntile, row, 0, ng, dm->T_local, a->G, st);
    if (a->H) ame_col_sum(a->work, ntile, row, ng, row - ng, dm->T_local, a->H, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int ame_covar_resid_dispatch(const ame_dims* dm, const float* Yraw, const float* Wt, const double* beta,
                             int p, float* out, hipStream_t st) {
    CovarBeta b;
    for (int k = 0; k < AME_MAX_COVARIATES; ++k) b.b[k] = k < p ? beta[k] : 0.0;
    const long long plane4 = ame_covar_plane4(dm);
    const unsigned grid = (unsigned)((plane4 + AME_NT - 1) / AME_NT);
    switch (p) {
#define X(PP)                                                                                         \
    case PP:                                                                                          \
        hipLaunchKernelGGL(ame_covar_resid_kernel<PP>, dim3(grid), dim3(AME_NT), 0, st,               \
                           (const float4*)Yraw, (const float4*)Wt, b, plane4, (float4*)out);          \
        break;
        AME_FOR_EACH_P(X)
#undef X
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
