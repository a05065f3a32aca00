// Goodness of fit: raw sums of the five network statistics and networks
// simulated from the fitted states (ame_net_moments, ame_net_triads,
// ame_simulate, include/ame_amd.h).
//
// K1 ame_net_moments_kernel: one wave per (slice, row) streams the row once as
//    float4 (two pairs) and adds row_i, col_i, sum y^2, sum y_ij y_ji in fp64
//    (lane-strided, then the wave butterfly); the diagonal, j >= n and the pad
//    pair are skipped by index, so what they hold never reaches a sum.
// K2 ame_tile_sum_kernel<2> (ame_tile.h): a slice's row partials in row order.
// K3 ame_net_triads_kernel: one workgroup per (slice, 128 x 128 output tile
//    (I, J)), all nb x nb tiles, in ame_tile.h's slice mapping.  k is walked in
//    chunks of 32; per chunk the rows I and J of the float2 network are read once
//    (float4 = two k) and de-interleaved into three LDS panels
//      PA[i][k] = E_ik (rows I, entry [0])    PC[j][k] = E_kj (rows J, entry [1])
//      PT[j][k] = E_jk (rows J, entry [0])
//    with the centre subtracted and the diagonal, k >= n and rows >= n set to
//    zero by selection; the next chunk's rows are loaded into registers before
//    the products of the current one.  Wave (wr, wc) owns the 64 x 64 quadrant
//    as 2 x 2 blocks of v_mfma_f32_32x32x2_f32; the cycle and the transitive
//    accumulators share the A fragment.  The k order inside a chunk is the MFMA's: step s multiplies
//    k = s (lanes 0-31) and k = 16 + s (lanes 32-63), so a lane's 16 operands of
//    a panel row are contiguous: four ds_read_b128 per row block.  Row stride 36
//    floats: the 16-byte slot of (row, half) is 9 row + 4 half mod 16, distinct
//    over each of ds_read_b128's 16-lane groups.  The epilogue multiplies by E_ji
//    (row i's entry [1]) in fp64, block_sum, one partial row per tile.
// K4 ame_col_sum_kernel (ame_tile.h): tile partials in tile order.
// K5 ame_simulate_kernel: one workgroup per (slice, 64 x 64 tile of the upper
//    triangle).  Ma = [a, 1, u], Mb = [1, b, v] staged as in ame_covar_g_kernel,
//    the two products on v_mfma_f32_16x16x4_f32, Philox4x32-10 and Box-Muller
//    per pair, then the tile goes through LDS (the operand panels' space, row
//    stride 65 float2: a column read by 32 lanes covers 64 banks once) so that
//    the upper rows and the transposed, swapped lower rows are both written as
//    512-byte row segments.
// Tile and chunk sizes are constants: the bits depend on them.
#include "ame_tile.h"
#include "ame_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define AME_GOF_TT 128   // triad output tile edge
#define AME_GOF_KC 32    // triad k chunk
#define AME_GOF_LD 36    // LDS row stride of the triad panels (floats)
#define AME_GOF_TLD 65   // LDS row stride of the simulated tile (float2)
static_assert(AME_DT * AME_GOF_TLD * 2 <= 4 * AME_DT * AME_SK_LD, "the simulated tile reuses the operand panels");

__host__ __device__ inline long long ame_gof_tiles(int n) {
    const long long nb = (n + AME_GOF_TT - 1) / AME_GOF_TT;
    return nb * nb;
}

long long ame_net_moments_work_doubles(const ame_dims* dm) { return (long long)dm->T_local * dm->n * 2; }
long long ame_net_moments_blocks(const ame_dims* dm) { return ((long long)dm->T_local * dm->n + 3) / 4; }
long long ame_net_triads_work_doubles(const ame_dims* dm) { return (long long)dm->T_local * ame_gof_tiles(dm->n) * 2; }
long long ame_net_triads_blocks(const ame_dims* dm) { return (long long)dm->T_local * ame_gof_tiles(dm->n); }
long long ame_simulate_blocks(const ame_dims* dm) { return (long long)dm->T_local * ame_tri_tiles(dm->n); }

// ---------------------------------------------------------------------------
// K1: row and column sums, sum of squares, sum of within-dyad products
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(AME_NT)
ame_net_moments_kernel(const float* __restrict__ Yt, int n, long long rows, double* __restrict__ node,
                       double* __restrict__ partial) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // tl * n + i
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(row % n), ny = ame_ystride(n);
    const float4* p = (const float4*)(Yt + (size_t)row * ny * 2);
    double sr = 0.0, sc = 0.0, s2 = 0.0, s11 = 0.0;
    for (int c = lane; c < (ny >> 1); c += 64) {
        const float4 v = p[c];
        const int j = 2 * c;
        if (j != i) {   // j < n: j is even and below ny
            const double a = (double)v.x, b = (double)v.y;
            sr += a;
            sc += b;
            s2 += a * a;
            s11 += a * b;
        }
        if (j + 1 < n && j + 1 != i) {
            const double a = (double)v.z, b = (double)v.w;
            sr += a;
            sc += b;
            s2 += a * a;
            s11 += a * b;
        }
    }
    sr = wave_sum(sr);
    sc = wave_sum(sc);
    s2 = wave_sum(s2);
    s11 = wave_sum(s11);
    if (lane == 0) {
        node[row * 2] = sr;
        node[row * 2 + 1] = sc;
        partial[row * 2] = s2;
        partial[row * 2 + 1] = s11;
    }
}

int ame_net_moments_dispatch(const ame_dims* dm, const ame_moments_args* a, hipStream_t st) {
    const long long rows = (long long)dm->T_local * dm->n;
    hipLaunchKernelGGL(ame_net_moments_kernel, dim3((unsigned)ame_net_moments_blocks(dm)), dim3(AME_NT), 0, st,
                       a->Yt, dm->n, rows, a->node, a->work);
    hipLaunchKernelGGL(ame_tile_sum_kernel<2>, dim3((unsigned)dm->T_local), dim3(AME_NT), 0, st, a->work, dm->n,
                       a->slice);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---------------------------------------------------------------------------
// K3: the two triad sums
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(AME_NT)
ame_net_triads_kernel(const float* __restrict__ Yt, const float* __restrict__ center, int n, int S, int nb,
                      double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float PA[AME_GOF_TT * AME_GOF_LD];
    __shared__ __attribute__((aligned(16))) float PC[AME_GOF_TT * AME_GOF_LD];
    __shared__ __attribute__((aligned(16))) float PT[AME_GOF_TT * AME_GOF_LD];
    __shared__ double red[4 * 2];

    int tl, tile;
    ame_slice_block(blockIdx.x, S, nb * nb, tl, tile);
    const int I0 = (tile / nb) * AME_GOF_TT, J0 = (tile % nb) * AME_GOF_TT;
    const int ny = ame_ystride(n);
    const float* ys = Yt + (size_t)tl * n * ny * 2;
    const float c = center[tl];

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = w >> 1, wc = w & 1, l31 = lane & 31, h = lane >> 5;

    f32x16 accC[2][2], accT[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q = 0; q < 16; ++q) accC[mi][ni][q] = accT[mi][ni][q] = 0.f;

    // a chunk's 128 rows x 16 float4 (two k each) of the rows I and of the rows J: 16 float4 per thread
    float4 vi[8], vj[8];
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = threadIdx.x + AME_NT * q, row = idx >> 4, k = k0 + 2 * (idx & 15);
            const int i = I0 + row, j = J0 + row;
            const bool ki = k < n;   // k is even: k + 1 <= ny - 1 stays inside the row
            vi[q] = *(const float4*)(ys + ((size_t)(i < n ? i : 0) * ny + (ki ? k : 0)) * 2);
            vj[q] = *(const float4*)(ys + ((size_t)(j < n ? j : 0) * ny + (ki ? k : 0)) * 2);
        }
    };
    load_chunk(0);
    for (int k0 = 0; k0 < n; k0 += AME_GOF_KC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = threadIdx.x + AME_NT * q, row = idx >> 4, c4 = idx & 15, k = k0 + 2 * c4;
            const int i = I0 + row, j = J0 + row;
            const bool i0 = i < n && k < n && k != i, i1 = i < n && k + 1 < n && k + 1 != i;
            const bool j0 = j < n && k < n && k != j, j1 = j < n && k + 1 < n && k + 1 != j;
            const int o = row * AME_GOF_LD + 2 * c4;
            *(float2*)(PA + o) = make_float2(i0 ? vi[q].x - c : 0.f, i1 ? vi[q].z - c : 0.f);
            *(float2*)(PT + o) = make_float2(j0 ? vj[q].x - c : 0.f, j1 ? vj[q].z - c : 0.f);
            *(float2*)(PC + o) = make_float2(j0 ? vj[q].y - c : 0.f, j1 ? vj[q].w - c : 0.f);
        }
        __syncthreads();
        // the next chunk's rows are in flight while this one is multiplied
        if (k0 + AME_GOF_KC < n) load_chunk(k0 + AME_GOF_KC);

        f32x4 af[2][4];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const f32x4* pa = (const f32x4*)(PA + (wr * 64 + mi * 32 + l31) * AME_GOF_LD + 16 * h);
#pragma unroll
            for (int v = 0; v < 4; ++v) af[mi][v] = pa[v];
        }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int ro = (wc * 64 + ni * 32 + l31) * AME_GOF_LD + 16 * h;
            const f32x4* pc = (const f32x4*)(PC + ro);
            const f32x4* pt = (const f32x4*)(PT + ro);
            f32x4 bc[4], bt[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                bc[v] = pc[v];
                bt[v] = pt[v];
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const float a = af[mi][s >> 2][s & 3];
                    accC[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bc[s >> 2][s & 3], accC[mi][ni], 0, 0, 0);
                    accT[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt[s >> 2][s & 3], accT[mi][ni], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // the panels are rewritten by the next chunk
    }

    // epilogue: register q of a 32 x 32 block is row (q & 3) + 8 (q >> 2) + 4 h, column l31
    double sm[2] = {0.0, 0.0};
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int j = J0 + wc * 64 + ni * 32 + l31;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = I0 + wr * 64 + mi * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                const bool ok = i < n && j < n && i != j;
                const float yji = ys[((size_t)(ok ? i : 0) * ny + (ok ? j : 0)) * 2 + 1];
                const double e = ok ? (double)(yji - c) : 0.0;
                sm[0] += (double)accC[mi][ni][q] * e;
                sm[1] += (double)accT[mi][ni][q] * e;
            }
        }
    }
    block_sum<2>(sm, red);
    if (threadIdx.x == 0) {
        double* o = partial + ((size_t)tl * nb * nb + tile) * 2;
        o[0] = sm[0];
        o[1] = sm[1];
    }
}

int ame_net_triads_dispatch(const ame_dims* dm, const ame_triads_args* a, hipStream_t st) {
    const int nb = (dm->n + AME_GOF_TT - 1) / AME_GOF_TT;
    hipLaunchKernelGGL(ame_net_triads_kernel, dim3((unsigned)ame_net_triads_blocks(dm)), dim3(AME_NT), 0, st,
                       a->Yt, a->center, dm->n, dm->T_local, nb, a->work);
    ame_col_sum<64>(a->work, nb * nb, 2, 0, 2, dm->T_local, a->tri, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---------------------------------------------------------------------------
// K5: one simulated network
// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011): words 0 and 1 of the output block
__device__ __forceinline__ void ame_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                  uint32_t k1, uint32_t& w0, uint32_t& w1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w0 = c0;
    w1 = c1;
}

// (float(w >> 8) + 0.5f) * 2^-24: in (0, 1], every step an fp32 operation
__device__ __forceinline__ float ame_uniform24(uint32_t w) {
    return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f;
}

struct SimParams {
    int n, r, t_begin, ntile;
    const float* x;
    float* out;
    double l00, l10, l11;
    uint32_t key0, key1, sample;
};

__global__ void __launch_bounds__(AME_NT)
ame_simulate_kernel(SimParams p) {
    __shared__ __attribute__((aligned(16))) float sm[4 * AME_DT * AME_SK_LD];
    float* MaI = sm;
    float* MbI = sm + AME_DT * AME_SK_LD;
    float* MaJ = sm + 2 * AME_DT * AME_SK_LD;
    float* MbJ = sm + 3 * AME_DT * AME_SK_LD;
    float2* tb = (float2*)sm;   // the finished tile [AME_DT][AME_GOF_TLD], after the products

    const int n = p.n, r = p.r;
    const int tl = blockIdx.x / p.ntile, tile = blockIdx.x - tl * p.ntile;
    int I0, J0;
    ame_tri_tile_origin(tile, n, I0, J0);
    const int d = 2 + 2 * r, mp = ame_pad4(r + 2);
    const AmeLaneDyad ld(I0, J0);

    {   // Ma = [a, 1, u, 0..], Mb = [1, b, v, 0..] of the tile's row and column nodes
        const int row = threadIdx.x >> 2;
        const int ni = I0 + row, nj = J0 + row;
        const float* xi = p.x + ((size_t)tl * n + (ni < n ? ni : 0)) * d;
        const float* xj = p.x + ((size_t)tl * n + (nj < n ? nj : 0)) * d;
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

    const uint32_t tg = (uint32_t)(p.t_begin + tl);
    const int ro = ld.i_op(AME_SK_LD);
    float2 yv[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int j = ld.j(s);
        f32x4 m0, m1;
        ame_smallk_products(MaI, MbJ, MbI, MaJ, ro, ld.j_op(s, AME_SK_LD), mp >> 2, m0, m1);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = ld.i(g);
            float2 y = make_float2(0.f, 0.f);
            if (ame_upper_pair(i, j, n)) {
                uint32_t w0, w1;
                ame_philox4x32_10((uint32_t)i, (uint32_t)j, tg, p.sample, p.key0, p.key1, w0, w1);
                const float u1 = ame_uniform24(w0), u2 = ame_uniform24(w1);
                const float rad = sqrtf(-2.0f * logf(u1));
                float sn, cs;
                sincospif(2.0f * u2, &sn, &cs);
                const double z0 = (double)(rad * cs), z1 = (double)(rad * sn);
                y.x = (float)((double)m0[g] + p.l00 * z0);
                y.y = (float)((double)m1[g] + (p.l10 * z0 + p.l11 * z1));
            }
            yv[s][g] = y;
        }
    }
    __syncthreads();   // every wave is done with the operand panels
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) tb[ld.row(g) * AME_GOF_TLD + ld.col(s)] = yv[s][g];
    __syncthreads();

    // a wave writes one row segment of 64 pairs per step
    const int ny = ame_ystride(n);
    float2* ys = (float2*)p.out + (size_t)tl * n * ny;
    const bool diag = I0 == J0;
    const float2 zero = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int it = 0; it < AME_DT * AME_DT / AME_NT; ++it) {
        const int idx = threadIdx.x + AME_NT * it, a = idx >> 6, b = idx & 63;
        const int gi = I0 + a, gj = J0 + b;
        if (gi < n && gj < ny) {   // rows I: the upper entries; on a diagonal tile the whole block
            float2 v = zero;
            if (!diag || a < b) {
                v = tb[a * AME_GOF_TLD + b];
            } else if (a > b) {
                const float2 u = tb[b * AME_GOF_TLD + a];
                v = make_float2(u.y, u.x);
            }
            if (gj >= n) v = zero;   // the pad pair of odd n
            ys[(size_t)gi * ny + gj] = v;
        }
        if (!diag && J0 + a < n && I0 + b < n) {   // rows J: the swapped transposes
            const float2 u = tb[b * AME_GOF_TLD + a];
            ys[(size_t)(J0 + a) * ny + I0 + b] = make_float2(u.y, u.x);
        }
    }
}

int ame_simulate_dispatch(const ame_dims* dm, const ame_simulate_args* a, hipStream_t st) {
    SimParams p;
    p.n = dm->n;
    p.r = dm->r;
    p.t_begin = dm->t_begin;
    p.ntile = (int)ame_tri_tiles(dm->n);
    p.x = a->x;
    p.out = a->Yt_out;
    p.l00 = a->lr[0];
    p.l10 = a->lr[1];
    p.l11 = a->lr[2];
    p.key0 = (uint32_t)(a->seed & 0xFFFFFFFFull);
    p.key1 = (uint32_t)(a->seed >> 32);
    p.sample = a->sample;
    hipLaunchKernelGGL(ame_simulate_kernel, dim3((unsigned)ame_simulate_blocks(dm)), dim3(AME_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
