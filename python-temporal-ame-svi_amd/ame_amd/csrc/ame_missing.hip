// Missing dyads: the packed mask and the working network (ame_pack_mask,
// ame_fill_missing, include/ame_amd.h).
//
// The sweep reads y_ij as J_j x_i + noise with J_j x_i = (a_i + u_i.v_j,
// b_i + v_i.u_j).  A hidden pair {i, j} contributes nothing to node i's update
// exactly when row i of the working network holds J_j m_i, node i's own mean of
// that entry, so the two rows of a hidden pair hold different values:
//   Yt[t][i][j] = (a_i + p, b_i + q)    Yt[t][j][i] = (a_j + q, b_j + p)
//   p = u_i.v_j, q = u_j.v_i.
//
// K1 ame_pack_mask_kernel: one workgroup per (slice, row).  Lane j of a wave
//    votes M[i][j][t] != 0 (and j != i, j < n): the ballot is the row's word
//    j >> 6.  Integer counts only: hidden pairs i < j of the slice, observed
//    partners of the row, entries whose transpose disagrees.
// K2 ame_fill_kernel: one workgroup per (slice, 64 x 64 tile of the upper
//    triangle), in ame_tile.h's tile order and slice mapping.  The tile's 64
//    mask words are read first (on a diagonal tile only bits j > i are kept); a
//    tile with nothing hidden writes zero partials and returns before any mean
//    is loaded.  Otherwise U and V of the tile's row and column nodes are
//    staged in LDS (K = r zero-padded to a multiple of 4) and the two products
//    run on v_mfma_f32_16x16x4_f32 (ame_tile.h: lane -> dyad layout, small-K
//    strip product); each hidden pair gets its two entries (fp32 adds) and adds
//    its correction terms in fp64.  No other element of Yt is written.
// K3 ame_col_sum_kernel (ame_tile.h): one thread per (slice, statistic) adds the
//    tile partials in tile order.
// The tile size is a constant and every sum has a fixed order: a slice's row
// has the same bits under any split of the slices over calls.  No atomics in
// the floating-point sums, no waits between workgroups.
#include "ame_tile.h"
#include "ame_internal.h"

#define AME_MS_NC 2     // correction sums per slice

long long ame_mask_words_count(const ame_dims* dm) {
    return (long long)dm->T_local * dm->n * ame_mask_row_words(dm->n);
}
long long ame_fill_work_doubles(const ame_dims* dm) {
    return (long long)dm->T_local * ame_tri_tiles(dm->n) * AME_MS_NC;
}
long long ame_fill_blocks(const ame_dims* dm) { return (long long)dm->T_local * ame_tri_tiles(dm->n); }

// ---------------------------------------------------------------------------
// K1: pack the mask
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(AME_NT)
ame_pack_mask_kernel(const uint8_t* __restrict__ M, unsigned long long* __restrict__ Mt, int n, int T_total,
                     int t_begin, unsigned long long* __restrict__ pairs, uint32_t* __restrict__ deg,
                     unsigned long long* __restrict__ asym) {
    __shared__ unsigned int cnt[3];   // hidden in the row, hidden with j > i, asymmetric
    const int tl = blockIdx.x / n, i = blockIdx.x - tl * n;
    const int tg = t_begin + tl, nw = ame_mask_row_words(n);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int c_all = 0u, c_up = 0u, c_as = 0u;
    // every wave walks whole words: j0 is a multiple of 64, so the ballot of a
    // wave is word j0 >> 6 (lanes at j >= n vote 0)
    for (int j0 = (int)(threadIdx.x & ~63u); j0 < nw * 64; j0 += AME_NT) {
        const int j = j0 + lane;
        bool h = false, as = false;
        if (j < n && j != i) {
            h = M[((size_t)i * n + j) * T_total + tg] != 0;
            as = h != (M[((size_t)j * n + i) * T_total + tg] != 0);
        }
        const unsigned long long word = __ballot(h);
        if (lane == 0) {
            Mt[((size_t)tl * n + i) * nw + (j0 >> 6)] = word;
            c_all += (unsigned int)__popcll(word);
            // bits of this word at j > i
            unsigned long long up = word;
            if (i >= j0 + 63) up = 0ull;
            else if (i >= j0) up &= ~0ull << (i - j0 + 1);
            c_up += (unsigned int)__popcll(up);
        }
        const unsigned long long aw = __ballot(as);
        if (lane == 0) c_as += (unsigned int)__popcll(aw);
    }
    if (lane == 0) {
        atomicAdd(&cnt[0], c_all);
        atomicAdd(&cnt[1], c_up);
        atomicAdd(&cnt[2], c_as);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        deg[(size_t)tl * n + i] = (uint32_t)(n - 1) - cnt[0];
        if (cnt[1]) atomicAdd(pairs + tl, (unsigned long long)cnt[1]);
        if (cnt[2]) atomicAdd(asym, (unsigned long long)cnt[2]);
    }
}

int ame_pack_mask_dispatch(const uint8_t* M, unsigned long long* Mt, const ame_dims* dm,
                           unsigned long long* pairs, uint32_t* deg, unsigned long long* asym,
                           hipStream_t st) {
    if (hipMemsetAsync(pairs, 0, sizeof(unsigned long long) * (size_t)dm->T_local, st) != hipSuccess) return -2;
    if (hipMemsetAsync(asym, 0, sizeof(unsigned long long), st) != hipSuccess) return -2;
    hipLaunchKernelGGL(ame_pack_mask_kernel, dim3((unsigned)((long long)dm->T_local * dm->n)), dim3(AME_NT), 0,
                       st, M, Mt, dm->n, dm->T_total, dm->t_begin, pairs, deg, asym);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---------------------------------------------------------------------------
// K2: fill the hidden entries of the working network, correction partials
// ---------------------------------------------------------------------------
struct FillParams {
    int n, r, S, ny, nw, ntile;
    const float* x;
    const unsigned long long* Mt;
    float* Yt;
    double r00, r01, r10, r11;
    double* partial;   // [S][ntile][AME_MS_NC]
};

__global__ void __launch_bounds__(AME_NT)
ame_fill_kernel(FillParams p) {
    __shared__ float UI[AME_DT * AME_SK_LD], VI[AME_DT * AME_SK_LD];
    __shared__ float UJ[AME_DT * AME_SK_LD], VJ[AME_DT * AME_SK_LD];
    __shared__ float abI[AME_DT * 2], abJ[AME_DT * 2];
    __shared__ unsigned long long mw[AME_DT];
    __shared__ double red[4 * AME_MS_NC];

    const int n = p.n, ntile = p.ntile;
    int tl, tile, I0, J0;
    ame_slice_block(blockIdx.x, p.S, ntile, tl, tile);
    ame_tri_tile_origin(tile, n, I0, J0);
    double* out = p.partial + ((size_t)tl * ntile + tile) * AME_MS_NC;

    // the tile's mask words: row I0 + k, word J0 >> 6
    bool any = false;
    if (threadIdx.x < AME_DT) {
        const int i = I0 + (int)threadIdx.x;
        unsigned long long wd = 0ull;
        if (i < n) {
            wd = p.Mt[((size_t)tl * n + i) * p.nw + (J0 >> 6)];
            if (I0 == J0) wd = threadIdx.x >= 63 ? 0ull : wd & (~0ull << (threadIdx.x + 1));
            const int left = n - J0;   // columns of this word inside the network (>= 1)
            if (left < 64) wd &= (1ull << left) - 1ull;
        }
        mw[threadIdx.x] = wd;
        any = wd != 0ull;
    }
    if (!__syncthreads_or(any ? 1 : 0)) {
        if (threadIdx.x < AME_MS_NC) out[threadIdx.x] = 0.0;
        return;
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

    float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
    const int ro = ld.i_op(AME_SK_LD);
    double sm[AME_MS_NC] = {0.0, 0.0};
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const int cj = ld.col(s), j = J0 + cj;
        // this lane's four rows: does any hold the bit of column j?  (uniform skip per wave)
        unsigned int bits = 0u;
#pragma unroll
        for (int g = 0; g < 4; ++g) bits |= (unsigned int)((mw[ld.row(g)] >> cj) & 1ull) << g;
        if (__ballot(bits != 0u) == 0ull) continue;
        f32x4 pp, qq;
        ame_smallk_products(UI, VJ, VI, UJ, ro, ld.j_op(s, AME_SK_LD), kp >> 2, pp, qq);
        const float aj = abJ[cj * 2], bj = abJ[cj * 2 + 1];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ri = ld.row(g), i = I0 + ri;
            if (((bits >> g) & 1u) && ame_upper_pair(i, j, n)) {
                const float ai = abI[ri * 2], bi = abI[ri * 2 + 1];
                const float pv = pp[g], qv = qq[g];
                const float2 up = make_float2(ai + pv, bi + qv);
                const float2 lo = make_float2(aj + qv, bj + pv);
                *(float2*)(ys + ((size_t)i * p.ny + j) * 2) = up;
                *(float2*)(ys + ((size_t)j * p.ny + i) * 2) = lo;
                // residuals of the two stored entries against E[mu_ij] and its swap
                const double m0 = (double)ai + (double)bj + (double)pv;
                const double m1 = (double)aj + (double)bi + (double)qv;
                const double u0 = (double)up.x - m0, u1 = (double)up.y - m1;
                const double l0 = (double)lo.x - m1, l1 = (double)lo.y - m0;
                sm[0] += u0 * (p.r00 * u0 + p.r01 * u1) + u1 * (p.r10 * u0 + p.r11 * u1);
                sm[1] += (u0 * u0 + u1 * u1) + (l0 * l0 + l1 * l1);
            }
        }
    }
    block_sum<AME_MS_NC>(sm, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < AME_MS_NC; ++q) out[q] = sm[q];
    }
}

int ame_fill_missing_dispatch(const ame_dims* dm, const ame_fill_args* a, hipStream_t st) {
    FillParams p;
    p.n = dm->n;
    p.r = dm->r;
    p.S = dm->T_local;
    p.ny = ame_ystride(dm->n);
    p.nw = ame_mask_row_words(dm->n);
    p.ntile = (int)ame_tri_tiles(dm->n);
    p.x = a->x;
    p.Mt = (const unsigned long long*)a->Mt;
    p.Yt = a->Yt;
    p.r00 = a->rinv[0];
    p.r01 = a->rinv[1];
    p.r10 = a->rinv[2];
    p.r11 = a->rinv[3];
    p.partial = a->work;
    hipLaunchKernelGGL(ame_fill_kernel, dim3((unsigned)((long long)p.S * p.ntile)), dim3(AME_NT), 0, st, p);
    // K3: corr[tl][q] = a slice's tile partials in tile order
    ame_col_sum<64>(a->work, p.ntile, AME_MS_NC, 0, AME_MS_NC, p.S, a->corr, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
