// Binary networks: the probit working network (ame_probit_fill,
// include/ame_amd.h).
//
// The sweep stays Gaussian: it reads a working network whose entry (i, j) is
// node i's own-perspective mean plus the pair's correction d = E_q[z] - m,
//   Yt[t][i][j] = (a_i + p + d0, b_i + q + d1)    Yt[t][j][i] = (a_j + q + d1, b_j + p + d0)
//   p = u_i.v_j, q = u_j.v_i,  m = (a_i + b_j + p, a_j + b_i + q),
// rewritten from the new means after every sweep.
//
// K1 ame_probit_fill_kernel: one workgroup per (slice, 64 x 64 tile of the upper
//    triangle), in ame_tile.h's tile order and slice mapping.  The tie words of
//    the tile's row nodes (word J0 >> 6: ties i -> j) and of its column nodes
//    (word I0 >> 6: ties j -> i) and the hidden-pair words of the row nodes are
//    staged first; U, V, (a, b) of both node sets as in ame_fill_kernel; p and q
//    on v_mfma_f32_16x16x4_f32.  Each lane then runs the fp64 recursion of its 16
//    pairs (AME_PROBIT_STEPS alternating truncated-normal steps, one code path
//    for every rho) and adds the four statistics.  No early return: every pair
//    is written.  The tile is finished in four strips of 16 columns (the MFMA
//    column blocks): a strip's upper entries are staged in LDS as [64][16] and
//    written as row segments of the rows I, its lower entries transposed as
//    [16][64] and written as 512-byte row segments of the rows J.  A
//    lane-per-column store of the lower triangle would be a 64-way strided
//    write.  The diagonal, the pad column and rows >= n are never written.
// K2 ame_col_sum_kernel (ame_tile.h): tile partials in tile order.
// The tile size is a constant and every sum has a fixed order: a slice's row
// has the same bits under any split of the slices over calls.  No atomics, no
// waits between workgroups.
#include "ame_tile.h"
#include "ame_internal.h"
#include "ame_probit.h"

#define AME_PB_ULD 17   // LDS row stride of a strip's upper entries [64][16] (float2)
#define AME_PB_LLD 65   // LDS row stride of a strip's lower entries [16][64] (float2)

long long ame_probit_fill_work_doubles(const ame_dims* dm) {
    return (long long)dm->T_local * ame_tri_tiles(dm->n) * AME_PROBIT_STATS;
}
long long ame_probit_fill_blocks(const ame_dims* dm) { return (long long)dm->T_local * ame_tri_tiles(dm->n); }

struct ProbitParams {
    int n, r, S, ny, nw, ntile;
    const float* x;
    const unsigned long long* Bt;
    const unsigned long long* Mt;   // or nullptr
    float* Yt;
    double rho, sd, inv_sd, half_log, inv_1mr2;   // sqrt(1 - rho^2), its inverse, log(1 - rho^2) / 2, 1 / (1 - rho^2)
    double* partial;                              // [S][ntile][AME_PROBIT_STATS]
};

__global__ void __launch_bounds__(AME_NT)
ame_probit_fill_kernel(ProbitParams p) {
    __shared__ __attribute__((aligned(16))) float sm[4 * AME_DT * AME_SK_LD];
    __shared__ float abI[AME_DT * 2], abJ[AME_DT * 2];
    __shared__ unsigned long long bwI[AME_DT], bwJ[AME_DT], mwI[AME_DT];
    __shared__ double red[4 * AME_PROBIT_STATS];
    __shared__ float2 tu[AME_DT * AME_PB_ULD], tl2[16 * AME_PB_LLD];   // one 64 x 16 strip of the tile
    float* UI = sm;
    float* VI = sm + AME_DT * AME_SK_LD;
    float* UJ = sm + 2 * AME_DT * AME_SK_LD;
    float* VJ = sm + 3 * AME_DT * AME_SK_LD;

    const int n = p.n, ntile = p.ntile;
    int tl, tile, I0, J0;
    ame_slice_block(blockIdx.x, p.S, ntile, tl, tile);
    ame_tri_tile_origin(tile, n, I0, J0);

    if (threadIdx.x < AME_DT) {   // tie and mask words of the tile's nodes
        const int i = I0 + (int)threadIdx.x, j = J0 + (int)threadIdx.x;
        unsigned long long bi = 0ull, bj = 0ull, mi = 0ull;
        if (i < n) {
            bi = p.Bt[((size_t)tl * n + i) * p.nw + (J0 >> 6)];
            if (p.Mt) mi = p.Mt[((size_t)tl * n + i) * p.nw + (J0 >> 6)];
        }
        if (j < n) bj = p.Bt[((size_t)tl * n + j) * p.nw + (I0 >> 6)];
        bwI[threadIdx.x] = bi;
        bwJ[threadIdx.x] = bj;
        mwI[threadIdx.x] = mi;
    }

    const int r = p.r, d = 2 + 2 * r, kp = ame_pad4(r);
    const AmeLaneDyad ld(I0, J0);
    {   // stage (a, b), U, V of the tile's row and column nodes, K zero-padded
        const int row = threadIdx.x >> 2;
        const int ni = I0 + row, nj = J0 + row;
        const float* xi = p.x + ((size_t)tl * n + (ni < n ? ni : 0)) * d;
        const float* xj = p.x + ((size_t)tl * n + (nj < n ? nj : 0)) * d;
        for (int c = threadIdx.x & 3; c < kp; c += 4) {
            float ui = 0.f, vi = 0.f, uj = 0.f, vj = 0.f;
            if (c < r) {
                if (ni < n) { ui = xi[2 + c]; vi = xi[2 + r + c]; }
                if (nj < n) { uj = xj[2 + c]; vj = xj[2 + r + c]; }
            }
            UI[row * AME_SK_LD + c] = ui;
            VI[row * AME_SK_LD + c] = vi;
            UJ[row * AME_SK_LD + c] = uj;
            VJ[row * AME_SK_LD + c] = vj;
        }
        if ((threadIdx.x & 3) < 2) {
            const int c = threadIdx.x & 3;
            abI[row * 2 + c] = ni < n ? xi[c] : 0.f;
            abJ[row * 2 + c] = nj < n ? xj[c] : 0.f;
        }
    }
    __syncthreads();

    const int ro = ld.i_op(AME_SK_LD);
    const double rho = p.rho, sd = p.sd, inv_sd = p.inv_sd;
    const int ny = p.ny;
    float2* ys = (float2*)p.Yt + (size_t)tl * n * ny;
    const bool diag = I0 == J0;
    double st[AME_PROBIT_STATS] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const int cj = ld.col(s), j = J0 + cj;
        f32x4 pp, qq;
        ame_smallk_products(UI, VJ, VI, UJ, ro, ld.j_op(s, AME_SK_LD), kp >> 2, pp, qq);
        const float aj = abJ[cj * 2], bj = abJ[cj * 2 + 1];
        const unsigned long long wj = bwJ[cj];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ri = ld.row(g), i = I0 + ri;
            float2 uv = make_float2(0.f, 0.f), lv = uv;
            if (ame_upper_pair(i, j, n)) {
                const float ai = abI[ri * 2], bi = abI[ri * 2 + 1];
                const float pf = pp[g], qf = qq[g];
                if ((mwI[ri] >> cj) & 1ull) {   // hidden: ame_fill_missing's fp32 adds, no sums
                    uv = make_float2(ai + pf, bi + qf);
                    lv = make_float2(aj + qf, bj + pf);
                } else {
                    const double pv = (double)pf, qv = (double)qf;
                    const bool y0 = (bwI[ri] >> cj) & 1ull, y1 = (wj >> ri) & 1ull;
                    const double s0 = y0 ? 1.0 : -1.0, s1 = y1 ? 1.0 : -1.0;
                    const double m0 = (double)ai + (double)bj + pv;
                    const double m1 = (double)aj + (double)bi + qv;
                    double k0, k1, l0, l1;
                    ame_probit_kl(s0 * m0, k0, l0);
                    ame_probit_kl(s1 * m1, k1, l1);
                    const double lp = l0 + l1;   // sum_a log Phi(s_a m_a)
                    double e0 = m0 + s0 * k0, e1 = m1 + s1 * k1;
#pragma unroll 1
                    for (int it = 0; it < AME_PROBIT_STEPS; ++it) {
                        const double eta0 = m0 + rho * (e1 - m1);
                        ame_probit_kl(s0 * eta0 * inv_sd, k0, l0);
                        e0 = eta0 + s0 * sd * k0;
                        const double eta1 = m1 + rho * (e0 - m0);
                        ame_probit_kl(s1 * eta1 * inv_sd, k1, l1);
                        e1 = eta1 + s1 * sd * k1;
                    }
                    const double d0 = e0 - m0, d1 = e1 - m1;
                    const double f0 = (y0 ? 1.0 : 0.0) - ame_probit_phi(m0);
                    const double f1 = (y1 ? 1.0 : 0.0) - ame_probit_phi(m1);
                    st[0] += 1.0;
                    st[1] += p.half_log - 0.5 * ((d0 * d0 - 2.0 * rho * d0 * d1 + d1 * d1) * p.inv_1mr2) +
                             ((l0 + 0.5 * k0 * k0) + (l1 + 0.5 * k1 * k1));
                    st[2] += f0 * f0 + f1 * f1;
                    st[3] += lp;
                    // rounded once
                    uv = make_float2((float)((double)ai + pv + d0), (float)((double)bi + qv + d1));
                    lv = make_float2((float)((double)aj + qv + d1), (float)((double)bj + pv + d0));
                }
            }
            tu[ri * AME_PB_ULD + ld.li] = uv;    // upper entries [row][column of the strip]
            tl2[ld.li * AME_PB_LLD + ri] = lv;   // lower entries, transposed [column][row]
        }
        __syncthreads();
        // rows I: 64 segments of the strip's 16 columns
#pragma unroll
        for (int it = 0; it < AME_DT * 16 / AME_NT; ++it) {
            const int idx = threadIdx.x + AME_NT * it, a = idx >> 4, b = 16 * s + (idx & 15);
            const int gi = I0 + a, gj = J0 + b;
            if (gi < n && gj < n && (!diag || a < b)) ys[(size_t)gi * ny + gj] = tu[a * AME_PB_ULD + (idx & 15)];
        }
        // rows J: the strip's 16 rows, segments of 64 columns
#pragma unroll
        for (int it = 0; it < AME_DT * 16 / AME_NT; ++it) {
            const int idx = threadIdx.x + AME_NT * it, a = idx >> 6, b = idx & 63;
            const int gi = J0 + 16 * s + a, gj = I0 + b;
            if (gi < n && gj < n && (!diag || b < 16 * s + a)) ys[(size_t)gi * ny + gj] = tl2[a * AME_PB_LLD + b];
        }
        __syncthreads();   // the strip buffers are rewritten by the next strip
    }

    block_sum<AME_PROBIT_STATS>(st, red);
    if (threadIdx.x == 0) {
        double* out = p.partial + ((size_t)tl * ntile + tile) * AME_PROBIT_STATS;
#pragma unroll
        for (int q = 0; q < AME_PROBIT_STATS; ++q) out[q] = st[q];
    }
}

int ame_probit_fill_dispatch(const ame_dims* dm, const ame_probit_fill_args* a, hipStream_t st) {
    ProbitParams p;
    p.n = dm->n;
    p.r = dm->r;
    p.S = dm->T_local;
    p.ny = ame_ystride(dm->n);
    p.nw = ame_mask_row_words(dm->n);
    p.ntile = (int)ame_tri_tiles(dm->n);
    p.x = a->x;
    p.Bt = (const unsigned long long*)a->Bt;
    p.Mt = (const unsigned long long*)a->Mt;
    p.Yt = a->Yt;
    const double om = (1.0 - a->rho) * (1.0 + a->rho);   // 1 - rho^2
    p.rho = a->rho;
    p.sd = sqrt(om);
    p.inv_sd = 1.0 / p.sd;
    p.half_log = 0.5 * log(om);
    p.inv_1mr2 = 1.0 / om;
    p.partial = a->work;
    hipLaunchKernelGGL(ame_probit_fill_kernel, dim3((unsigned)((long long)p.S * p.ntile)), dim3(AME_NT), 0, st, p);
    ame_col_sum<64>(a->work, p.ntile, AME_PROBIT_STATS, 0, AME_PROBIT_STATS, p.S, a->stat, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
