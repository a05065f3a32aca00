// Posterior-predictive dyad moments and scoring (ame_predict, include/ame_amd.h).
//
// Every term of V0(i,j), V0(j,i), C01(i,j) and of the two means is an inner
// product of a per-node feature of i with a per-node feature of j, so a 64 x 64
// tile of dyads is five small GEMMs over node-feature rows:
//
//   segment  length            i-side row . j-side row
//   Ma, Mb   r + 2             Ma_i.Mb_j = E[mu_ij[0]],  Mb_i.Ma_j = E[mu_ij[1]]
//   F, G     2 + 2P + 2r       F_i.G_j = V0(i,j),        G_i.F_j = V0(j,i)     P = r(r+1)/2
//   Pc, Qc   2 + 4r + 2r^2     Pc_i.Qc_j = C01(i,j)
//
//   Ma = [a, 1, u]                       Mb = [1, b, v]
//   F  = [S_aa, 1, pk(S_UU), pk(u u'), 2 S_aU, u]
//   G  = [1, S_bb, sy(S_VV + v v'), sy(S_VV), v, 2 S_bV]
//   Pc = [S_ab, 1, S_aV, v, S_bU, u, C, u v']          C = S_UV (rows U, columns V)
//   Qc = [1, S_ab, u, S_bU, v, S_aV, C' + v u', C']
// pk() packs a symmetric r x r block to its upper triangle with the two
// off-diagonal entries added, sy() with their mean, so pk(A).sy(B) = <A, B>.
// Each segment is zero-padded to a multiple of 4 (the K of v_mfma_f32_16x16x4_f32).
//
// K1 ame_predict_feat_kernel: one workgroup per (slice, node) writes the six
//    segments once (row of PredictCfg<R>::L floats) into `work`.
// K2 ame_predict_pairs_kernel: one workgroup per (slice, 64 x 64 tile; ame_tile.h
//    holds the tile order, the slice mapping and the lane -> dyad layout); the
//    five products stream K in chunks of 32 through LDS (both 64-row operand
//    tiles, next chunk prefetched into registers during the MFMAs), each wave
//    keeps its 16 x 64 part of the five results in registers (20 accumulators
//    of 4) and runs the epilogue on them: scoring in fp64 against Y, read once
//    from the upper triangle (MODE 0, tiles I <= J), or the dense block (MODE 1).
// K3 ame_tile_sum_kernel (ame_tile.h): fixed-order sum of a slice's tile partials.
// MODE 2 of K2 (ame_mstep_stats): the same tiles, products and K3, with the
//    M-step's residual second moments as the epilogue.
// MODE 3 of K2 (ame_probit_score): the same again with a Bernoulli epilogue,
//    pi = Phi(E[mu] / sqrt(1 + V0)) against a 0 / 1 network (C01 is not needed:
//    its product is skipped).
// MODE 4 of K2 (ame_probit_rank): MODE 3's products; the epilogue bins the score
//    t = E[mu] / sqrt(1 + V0) of both entries into a per-workgroup uint32
//    [2][nbins] histogram in LDS (LDS integer atomics) and adds its non-zero
//    bins to the slice's uint64 histogram with global integer atomics.
// MODE 5 of K2 (ame_probit_select): the same pass; entries at or above the
//    slice's threshold bin are appended to the slice's region of records (one
//    global integer atomic per workgroup reserves its run).
// MODE 6 of K2 (ame_resid_nodes): MODE 0's products and per-pair quantities; the
//    epilogue adds them per node, a few slots at a time so that the sums fit
//    beside the 20 accumulators: a row node's 64 pairs in the lane and across its
//    16-lane row, a column node's in the lane, across the lane quarters and (LDS)
//    across the waves, each result stored once into its own slot of a
//    [S][nb + 1][n][AME_NODE_SUMS] partial that ame_col_sum adds in slot order.
// MODE 7 of K2 (ame_resid_hist): the same pairs; m^2 binned as MODE 4 bins t
//    (one uint32 [nbins] histogram in LDS), a NaN into the last bin.
// MODE 8 of K2 (ame_resid_select): MODE 5's reservation scheme for the pairs at
//    or above the slice's threshold bin of m^2.
// Modes 0 - 3, 6: no atomics, no spin, no O(n^2) intermediate.  Modes 4, 5, 7, 8:
// integer atomics only (order-independent sums / a free order the host sorts away).
#include <type_traits>

#include "ame_tile.h"
#include "ame_internal.h"
#include "ame_probit.h"

#define AME_PKB 32       // K chunk in floats
#define AME_PLD 34       // LDS row stride: 2 li + lq hits 32 distinct banks per half wave
#define AME_PNS AME_PREDICT_SUMS
#define AME_MS_DYAD 4    // M-step dyad statistics per slice: pairs, Rss00, Rss11, Rss01

// floats of one node's feature row for latent dim r
__host__ __device__ constexpr int ame_predict_row(int r) {
    return 2 * ame_pad4(r + 2) + 2 * ame_pad4(2 + r * (r + 1) + 2 * r) + 2 * ame_pad4(2 + 4 * r + 2 * r * r);
}

template <int R>
struct PredictCfg {
    static constexpr int D = 2 + 2 * R, P = R * (R + 1) / 2;
    static constexpr int KM = R + 2, MP = ame_pad4(KM);
    static constexpr int KV = 2 + 2 * P + 2 * R, KVP = ame_pad4(KV);
    static constexpr int KC = 2 + 4 * R + 2 * R * R, KCP = ame_pad4(KC);
    static constexpr int oMa = 0, oMb = MP, oF = 2 * MP, oG = oF + KVP, oP = oG + KVP, oQ = oP + KCP;
    static constexpr int L = oQ + KCP;
    static_assert(L == ame_predict_row(R), "feature row length");
};

struct PredictParams {
    int n, S, ny, ntile, ntj, n_levels;
    int i0, i1, j0, j1;
    const float* feat;
    const float* Yt;
    double n00, n01, n11;
    double zsq[AME_PREDICT_MAX_LEVELS], csq[AME_PREDICT_MAX_LEVELS];
    double* partial;   // [S][ntile][AME_PNS]
    float* dense;
    const unsigned long long* Mt;   // [S][n][nw] packed mask, or nullptr
    int nw, mask_select;            // 0: every pair i < j; AME_MASK_OBSERVED / AME_MASK_HIDDEN
    // MODE 4, 5: the bin rule; MODE 4: hist [S][2][nbins]; MODE 5: the selection
    int nbins, tie_filter, slice0;
    double t_max, scale;
    unsigned long long* hist;
    const int* bin_min;             // [S]
    const long long* offset;        // [S + 1] record offsets of the slices' regions
    unsigned long long* count;      // [S] entries that passed (also those beyond a region)
    ame_link_record* rec;
    // MODE 6: node partial [S][nb + 1][n][AME_NODE_SUMS]; MODE 8: the records
    double* node_partial;
    ame_resid_record* rrec;
};

// whether pair (i, j), i < j < n, of slice tl is selected (MODE 0 scoring, MODE 2 statistics)
__device__ __forceinline__ bool predict_pair_selected(const PredictParams& p, int tl, int i, int j) {
    if (p.mask_select == 0) return true;
    const unsigned long long wd = p.Mt[((size_t)tl * p.n + i) * p.nw + (j >> 6)];
    const bool hidden = (wd >> (j & 63)) & 1ull;
    return hidden == (p.mask_select == AME_MASK_HIDDEN);
}

// the histogram bin of a score (include/ame_amd.h): an add, then a multiply, then
// floor, clamped to [0, nbins - 1]; a NaN score goes to bin 0
__device__ __forceinline__ int predict_rank_bin(const PredictParams& p, double t) {
    const double fb = floor((t + p.t_max) * p.scale);
    return !(fb >= 0.0) ? 0 : (fb > (double)(p.nbins - 1) ? p.nbins - 1 : (int)fb);
}

// the histogram bin of a pair's m^2 (include/ame_amd.h): one multiply, then floor,
// clamped to [0, nbins - 1]; a NaN m^2 goes to bin nbins - 1 (not 0 as above)
__device__ __forceinline__ int resid_bin(const PredictParams& p, double m2) {
    const double fb = floor(m2 * p.scale);
    return !(fb <= (double)(p.nbins - 1)) ? p.nbins - 1 : (fb < 0.0 ? 0 : (int)fb);
}

// MODE 0's per-pair quantities (modes 6 - 8), from the pair's observation and its
// five products
struct ResidPair {
    double e0, e1, v0, v1, c, det, q0, q1, m2;
    __device__ __forceinline__ ResidPair(const PredictParams& p, float2 y, float a0, float a1, float a2, float a3,
                                         float a4) {
        e0 = (double)y.x - (double)a0;
        e1 = (double)y.y - (double)a1;
        v0 = (double)a2 + p.n00;
        v1 = (double)a3 + p.n11;
        c = (double)a4 + p.n01;
        det = v0 * v1 - c * c;
        q0 = e0 * e0;
        q1 = e1 * e1;
        m2 = (v1 * q0 - 2.0 * c * e0 * e1 + v0 * q1) / det;
    }
};

// ---------------------------------------------------------------------------
// K1: feature rows
// ---------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(AME_NT)
ame_predict_feat_kernel(const float* __restrict__ x, const float* __restrict__ cov, float* __restrict__ feat) {
    using C = PredictCfg<R>;
    constexpr int D = C::D, P = C::P, iU = 2, iV = 2 + R;
    __shared__ float sc[D * D];
    __shared__ float sm[D];
    const size_t node = blockIdx.x;   // slice * n + i
    const float* cv = cov + node * (size_t)(D * D);
    for (int e = threadIdx.x; e < D * D; e += AME_NT) sc[e] = cv[e];
    if (threadIdx.x < D) sm[threadIdx.x] = x[node * D + threadIdx.x];
    __syncthreads();
    float* f = feat + node * (size_t)C::L;
    float* Ma = f + C::oMa;
    float* Mb = f + C::oMb;
    float* F = f + C::oF;
    float* G = f + C::oG;
    float* Pc = f + C::oP;
    float* Qc = f + C::oQ;
    auto Sg = [&](int a, int b) { return sc[a * D + b]; };
    const int t = threadIdx.x;
    if (t == 0) {
        Ma[0] = sm[0]; Ma[1] = 1.f;
        Mb[0] = 1.f;   Mb[1] = sm[1];
        F[0] = Sg(0, 0); F[1] = 1.f;
        G[0] = 1.f;      G[1] = Sg(1, 1);
        const float sab = 0.5f * (Sg(0, 1) + Sg(1, 0));
        Pc[0] = sab; Pc[1] = 1.f;
        Qc[0] = 1.f; Qc[1] = sab;
        for (int k = C::KM; k < C::MP; ++k) Ma[k] = Mb[k] = 0.f;
        for (int k = C::KV; k < C::KVP; ++k) F[k] = G[k] = 0.f;
        for (int k = C::KC; k < C::KCP; ++k) Pc[k] = Qc[k] = 0.f;
    }
    if (t < R) {
        const int k = t;
        const float u = sm[iU + k], v = sm[iV + k];
        const float saU = Sg(0, iU + k), saV = Sg(0, iV + k), sbU = Sg(1, iU + k), sbV = Sg(1, iV + k);
        Ma[2 + k] = u;
        Mb[2 + k] = v;
        F[2 + 2 * P + k] = 2.f * saU;
        F[2 + 2 * P + R + k] = u;
        G[2 + 2 * P + k] = v;
        G[2 + 2 * P + R + k] = 2.f * sbV;
        Pc[2 + k] = saV;
        Pc[2 + R + k] = v;
        Pc[2 + 2 * R + k] = sbU;
        Pc[2 + 3 * R + k] = u;
        Qc[2 + k] = u;
        Qc[2 + R + k] = sbU;
        Qc[2 + 2 * R + k] = v;
        Qc[2 + 3 * R + k] = saV;
    }
    for (int e = t; e < R * R; e += AME_NT) {
        const int a = e / R, b = e - a * R;
        const float ua = sm[iU + a], ub = sm[iU + b], va = sm[iV + a], vb = sm[iV + b];
        const float cba = Sg(iU + b, iV + a);          // C[b][a]
        Pc[2 + 4 * R + e] = Sg(iU + a, iV + b);        // C[a][b]
        Pc[2 + 4 * R + R * R + e] = ua * vb;
        Qc[2 + 4 * R + e] = cba + va * ub;
        Qc[2 + 4 * R + R * R + e] = cba;
        if (a <= b) {
            const int pos = a * R - (a * (a - 1)) / 2 + (b - a);
            const float w = (a == b) ? 1.f : 2.f;
            const float suu = (a == b) ? Sg(iU + a, iU + a) : Sg(iU + a, iU + b) + Sg(iU + b, iU + a);
            const float svv = (a == b) ? Sg(iV + a, iV + a) : 0.5f * (Sg(iV + a, iV + b) + Sg(iV + b, iV + a));
            F[2 + pos] = suu;
            F[2 + P + pos] = w * ua * ub;
            G[2 + pos] = svv + va * vb;
            G[2 + P + pos] = svv;
        }
    }
}

// ---------------------------------------------------------------------------
// K2: tiled pair kernel
// ---------------------------------------------------------------------------
template <int R, int MODE>
__global__ void __launch_bounds__(AME_NT, 2)
ame_predict_pairs_kernel(PredictParams p) {
    using C = PredictCfg<R>;
    constexpr int L = C::L;
    const int n = p.n, ntile = p.ntile;
    int tl, tile, I0, J0, ilim, jlim;
    ame_slice_block(blockIdx.x, p.S, ntile, tl, tile);
    if (MODE != 1) {   // scoring and the M-step dyad statistics: upper-triangle tiles
        ame_tri_tile_origin(tile, n, I0, J0);
        ilim = jlim = n;
    } else {
        const int ti = tile / p.ntj, tj = tile - ti * p.ntj;
        I0 = p.i0 + ti * AME_DT;
        J0 = p.j0 + tj * AME_DT;
        ilim = p.i1;
        jlim = p.j1;
    }
    const AmeLaneDyad ld(I0, J0);

    __shared__ __attribute__((aligned(16))) float Il[AME_DT * AME_PLD], Jl[AME_DT * AME_PLD];
    __shared__ double red[4 * AME_PNS];

    const float* fs = p.feat + (size_t)tl * n * L;
    // the two float4 of each operand tile this thread stages per chunk
    const int row0 = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;   // rows row0, row0 + 32
    const float* gi[2];
    const float* gj[2];
    bool oki[2], okj[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ri = I0 + row0 + 32 * h, rj = J0 + row0 + 32 * h;
        oki[h] = ri < ilim;
        okj[h] = rj < jlim;
        gi[h] = fs + (size_t)(oki[h] ? ri : 0) * L + c4;
        gj[h] = fs + (size_t)(okj[h] ? rj : 0) * L + c4;
    }

    f32x4 acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[q][s] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto product = [&](auto pidx, int segI, int segJ, int len) {
        constexpr int PI = decltype(pidx)::value;
        const int nch = (len + AME_PKB - 1) / AME_PKB;
        float4 ri[2], rj[2];
        auto gload = [&](int c) {
            const int k0 = c * AME_PKB;
            const bool in = k0 + c4 < len;   // len is a multiple of 4: a float4 is in or out
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ri[h] = (oki[h] && in) ? *(const float4*)(gi[h] + segI + k0) : z;
                rj[h] = (okj[h] && in) ? *(const float4*)(gj[h] + segJ + k0) : z;
            }
        };
        gload(0);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();   // the previous chunk's fragments have been read
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float* di = &Il[(row0 + 32 * h) * AME_PLD + c4];
                float* dj = &Jl[(row0 + 32 * h) * AME_PLD + c4];
                *(float2*)di = make_float2(ri[h].x, ri[h].y);
                *(float2*)(di + 2) = make_float2(ri[h].z, ri[h].w);
                *(float2*)dj = make_float2(rj[h].x, rj[h].y);
                *(float2*)(dj + 2) = make_float2(rj[h].z, rj[h].w);
            }
            __syncthreads();
            if (c + 1 < nch) gload(c + 1);
            const int left = (len - c * AME_PKB) >> 2;
            const int ks = left < AME_PKB / 4 ? left : AME_PKB / 4;
            const float* ia = &Il[ld.i_op(AME_PLD)];
            const float* jb = &Jl[ld.j_op(0, AME_PLD)];
#pragma unroll 2
            for (int kk = 0; kk < ks; ++kk) {
                const float a = ia[4 * kk];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float b = jb[16 * s * AME_PLD + 4 * kk];
                    acc[PI][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[PI][s], 0, 0, 0);
                }
            }
        }
    };
    product(std::integral_constant<int, 0>{}, C::oMa, C::oMb, C::MP);
    product(std::integral_constant<int, 1>{}, C::oMb, C::oMa, C::MP);
    product(std::integral_constant<int, 2>{}, C::oF, C::oG, C::KVP);
    product(std::integral_constant<int, 3>{}, C::oG, C::oF, C::KVP);
    constexpr bool NEED_C01 = MODE < 3 || MODE >= 6;   // the Bernoulli modes 3 - 5 skip C01
    if (NEED_C01) product(std::integral_constant<int, 4>{}, C::oP, C::oQ, C::KCP);

    // accumulator element (s, g) of this lane: dyad (ld.i(g), ld.j(s))
    if (MODE == 2) {   // pairs, e0^2 + V0(i,j), e1^2 + V0(j,i), e0 e1 + C01 (no noise), fp64
        double sm[AME_MS_DYAD];
#pragma unroll
        for (int q = 0; q < AME_MS_DYAD; ++q) sm[q] = 0.0;
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                    const double e0 = (double)y.x - (double)acc[0][s][g];
                    const double e1 = (double)y.y - (double)acc[1][s][g];
                    sm[0] += 1.0;
                    sm[1] += e0 * e0 + (double)acc[2][s][g];
                    sm[2] += e1 * e1 + (double)acc[3][s][g];
                    sm[3] += e0 * e1 + (double)acc[4][s][g];
                }
            }
        }
        block_sum<AME_MS_DYAD>(sm, red);
        if (threadIdx.x == 0) {
            double* o = p.partial + ((size_t)tl * ntile + tile) * AME_MS_DYAD;
#pragma unroll
            for (int q = 0; q < AME_MS_DYAD; ++q) o[q] = sm[q];
        }
        return;
    }
    if (MODE == 3) {   // pairs, log score, Brier, hits, ties, sum of pi over both entries, fp64
        double sm[AME_PROBIT_SUMS];
#pragma unroll
        for (int q = 0; q < AME_PROBIT_SUMS; ++q) sm[q] = 0.0;
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                    sm[0] += 1.0;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const bool tie = (c ? y.y : y.x) > 0.5f;
                        const double t = (double)acc[c][s][g] / sqrt(1.0 + (double)acc[2 + c][s][g]);
                        const double pi = ame_probit_phi(t), yv = tie ? 1.0 : 0.0;
                        sm[1] += ame_probit_logphi(tie ? t : -t);
                        sm[2] += (yv - pi) * (yv - pi);
                        sm[3] += ((pi > 0.5) == tie) ? 1.0 : 0.0;
                        sm[4] += yv;
                        sm[5] += pi;
                    }
                }
            }
        }
        block_sum<AME_PROBIT_SUMS>(sm, red);
        if (threadIdx.x == 0) {
            double* o = p.partial + ((size_t)tl * ntile + tile) * AME_PROBIT_SUMS;
#pragma unroll
            for (int q = 0; q < AME_PROBIT_SUMS; ++q) o[q] = sm[q];
        }
        return;
    }
    if (MODE == 4) {   // class histograms of t = E[mu] / sqrt(1 + V0), both entries of every selected pair
        __shared__ unsigned hl[2 * AME_RANK_MAX_BINS];
        const int nb = p.nbins;
        for (int e = threadIdx.x; e < 2 * nb; e += AME_NT) hl[e] = 0u;
        __syncthreads();
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const bool tie = (c ? y.y : y.x) > 0.5f;
                        const double t = (double)acc[c][s][g] / sqrt(1.0 + (double)acc[2 + c][s][g]);
                        atomicAdd(&hl[(tie ? nb : 0) + predict_rank_bin(p, t)], 1u);
                    }
                }
            }
        }
        __syncthreads();
        unsigned long long* hs = p.hist + (size_t)tl * 2 * nb;
        for (int e = threadIdx.x; e < 2 * nb; e += AME_NT) {
            const unsigned v = hl[e];
            if (v) atomicAdd(&hs[e], (unsigned long long)v);
        }
        return;
    }
    if (MODE == 5) {   // records of the entries at or above the slice's threshold bin
        __shared__ unsigned lcnt;
        __shared__ unsigned long long gbase;
        if (threadIdx.x == 0) lcnt = 0u;
        __syncthreads();
        const int bmin = p.bin_min[tl], tf = p.tie_filter;
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
        unsigned take = 0u, ties = 0u;   // bit 8 s + 2 g + c of this lane's 32 entries
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const bool tie = (c ? y.y : y.x) > 0.5f;
                        const double t = (double)acc[c][s][g] / sqrt(1.0 + (double)acc[2 + c][s][g]);
                        const unsigned bit = 1u << (8 * s + 2 * g + c);
                        if (tie) ties |= bit;
                        if (predict_rank_bin(p, t) >= bmin && (tf < 0 || (int)tie == tf)) take |= bit;
                    }
                }
            }
        }
        const unsigned mine = __popc(take);
        const unsigned lbase = mine ? atomicAdd(&lcnt, mine) : 0u;
        __syncthreads();
        if (threadIdx.x == 0 && lcnt) gbase = atomicAdd(&p.count[tl], (unsigned long long)lcnt);
        __syncthreads();
        if (!mine) return;
        const long long off = p.offset[tl];
        const long long cap = p.offset[tl + 1] - off;   // <= 0: nothing is written
        long long pos = (long long)(gbase + lbase);
        ame_link_record* rs = p.rec + off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const unsigned bit = 1u << (8 * s + 2 * g + c);
                    if (take & bit) {
                        if (pos < cap) {   // beyond the region: counted, not written
                            ame_link_record rc;
                            rc.t = (double)acc[c][s][g] / sqrt(1.0 + (double)acc[2 + c][s][g]);
                            rc.slice = p.slice0 + tl;
                            rc.sender = c ? j : i;
                            rc.receiver = c ? i : j;
                            rc.tie = (ties & bit) ? 1 : 0;
                            rs[pos] = rc;
                        }
                        ++pos;
                    }
                }
            }
        }
        return;
    }
    if (MODE == 6) {   // per-node sums of MODE 0's per-pair quantities, a few slots per pass
        constexpr int KMAX = 4;
        __shared__ double cl[4][AME_DT][KMAX];   // column partials of the four waves
        constexpr double LOG2PI2 = 2.0 * 1.8378770664093454835606594728112;
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
        const int nb = (n + AME_DT - 1) / AME_DT;
        // row nodes of tile (I, J) own slot J + 1, column nodes slot I
        double* rowp = p.node_partial + ((size_t)tl * (nb + 1) + (J0 / AME_DT + 1)) * n * AME_NODE_SUMS;
        double* colp = p.node_partial + ((size_t)tl * (nb + 1) + I0 / AME_DT) * n * AME_NODE_SUMS;
        unsigned sel = 0u;   // bit 4 s + g: the lane's pair (s, g) is selected
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (ame_upper_pair(ld.i(g), ld.j(s), n) && predict_pair_selected(p, tl, ld.i(g), ld.j(s)))
                    sel |= 1u << (4 * s + g);
        // K slots from q0 on; f(rp, v) fills the pair's K values as the row node i
        // takes them; SWAP: the column node j takes them with sent and received
        // (k, k ^ 1) exchanged
        auto pass = [&](auto kc, auto swap, int q0, auto&& f) {
            constexpr int K = decltype(kc)::value;
            constexpr bool SWAP = decltype(swap)::value;
            double rs[4][K], cs[4][K];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) rs[a][k] = cs[a][k] = 0.0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (sel & (1u << (4 * s + g))) {
                        const float2 y = *(const float2*)(ys + ((size_t)ld.i(g) * p.ny + ld.j(s)) * 2);
                        const ResidPair rp(p, y, acc[0][s][g], acc[1][s][g], acc[2][s][g], acc[3][s][g],
                                           acc[4][s][g]);
                        double v[K];
                        f(rp, v);
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            rs[g][k] += v[k];
                            cs[s][k] += v[SWAP ? (k ^ 1) : k];
                        }
                    }
                }
            }
            // row node 16 w + 4 lq + g: across the 16 lanes li of its row
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    double x = rs[g][k];
                    x += __shfl_xor(x, 1);
                    x += __shfl_xor(x, 2);
                    x += __shfl_xor(x, 4);
                    x += __shfl_xor(x, 8);
                    if (ld.li == 0 && ld.i(g) < n) rowp[(size_t)ld.i(g) * AME_NODE_SUMS + q0 + k] = x;
                }
            }
            // column node 16 s + li: across the lane quarters lq, then the waves in order
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    double x = cs[s][k];
                    x += __shfl_xor(x, 16);
                    x += __shfl_xor(x, 32);
                    if (ld.lq == 0) cl[ld.w][ld.col(s)][k] = x;
                }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < AME_DT * K; e += AME_NT) {
                const int cidx = e / K, k = e - cidx * K;
                if (J0 + cidx < n)
                    colp[(size_t)(J0 + cidx) * AME_NODE_SUMS + q0 + k] =
                        ((cl[0][cidx][k] + cl[1][cidx][k]) + cl[2][cidx][k]) + cl[3][cidx][k];
            }
            __syncthreads();   // cl is free for the next pass
        };
        pass(std::integral_constant<int, 3>{}, std::false_type{}, 0, [&](const ResidPair& rp, double* v) {
            v[0] = 1.0;
            v[1] = -0.5 * (log(rp.det) + rp.m2 + LOG2PI2);
            v[2] = rp.m2;
        });
        pass(std::integral_constant<int, 2>{}, std::true_type{}, 3, [&](const ResidPair& rp, double* v) {
            v[0] = rp.q0 / rp.v0;
            v[1] = rp.q1 / rp.v1;
        });
        pass(std::integral_constant<int, 4>{}, std::true_type{}, 5, [&](const ResidPair& rp, double* v) {
            v[0] = rp.e0;
            v[1] = rp.e1;
            v[2] = rp.q0;
            v[3] = rp.q1;
        });
        return;
    }
    if (MODE == 7) {   // histogram of m^2, one count per selected pair
        __shared__ unsigned hl[AME_RANK_MAX_BINS];
        const int nb = p.nbins;
        for (int e = threadIdx.x; e < nb; e += AME_NT) hl[e] = 0u;
        __syncthreads();
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                    const ResidPair rp(p, y, acc[0][s][g], acc[1][s][g], acc[2][s][g], acc[3][s][g], acc[4][s][g]);
                    atomicAdd(&hl[resid_bin(p, rp.m2)], 1u);
                }
            }
        }
        __syncthreads();
        unsigned long long* hs = p.hist + (size_t)tl * nb;
        for (int e = threadIdx.x; e < nb; e += AME_NT) {
            const unsigned v = hl[e];
            if (v) atomicAdd(&hs[e], (unsigned long long)v);
        }
        return;
    }
    if (MODE == 8) {   // records of the pairs at or above the slice's threshold bin of m^2
        __shared__ unsigned lcnt;
        __shared__ unsigned long long gbase;
        if (threadIdx.x == 0) lcnt = 0u;
        __syncthreads();
        const int bmin = p.bin_min[tl];
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
        unsigned take = 0u;   // bit 4 s + g of this lane's 16 pairs
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                    const ResidPair rp(p, y, acc[0][s][g], acc[1][s][g], acc[2][s][g], acc[3][s][g], acc[4][s][g]);
                    if (resid_bin(p, rp.m2) >= bmin) take |= 1u << (4 * s + g);
                }
            }
        }
        const unsigned mine = __popc(take);
        const unsigned lbase = mine ? atomicAdd(&lcnt, mine) : 0u;
        __syncthreads();
        if (threadIdx.x == 0 && lcnt) gbase = atomicAdd(&p.count[tl], (unsigned long long)lcnt);
        __syncthreads();
        if (!mine) return;
        const long long off = p.offset[tl];
        const long long cap = p.offset[tl + 1] - off;   // <= 0: nothing is written
        long long pos = (long long)(gbase + lbase);
        ame_resid_record* rs = p.rrec + off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (take & (1u << (4 * s + g))) {
                    if (pos < cap) {   // beyond the region: counted, not written
                        const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                        const ResidPair rp(p, y, acc[0][s][g], acc[1][s][g], acc[2][s][g], acc[3][s][g],
                                           acc[4][s][g]);
                        ame_resid_record rc;
                        rc.m2 = rp.m2;
                        rc.z0 = rp.e0 / sqrt(rp.v0);
                        rc.z1 = rp.e1 / sqrt(rp.v1);
                        rc.slice = p.slice0 + tl;
                        rc.i = i;
                        rc.j = j;
                        rc.pad = 0;
                        rs[pos] = rc;
                    }
                    ++pos;
                }
            }
        }
        return;
    }
    if (MODE == 0) {
        double sm[AME_PNS];
#pragma unroll
        for (int q = 0; q < AME_PNS; ++q) sm[q] = 0.0;
        const float* ys = p.Yt + (size_t)tl * n * p.ny * 2;
        constexpr double LOG2PI2 = 2.0 * 1.8378770664093454835606594728112;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (ame_upper_pair(i, j, n) && predict_pair_selected(p, tl, i, j)) {
                    const float2 y = *(const float2*)(ys + ((size_t)i * p.ny + j) * 2);
                    const double e0 = (double)y.x - (double)acc[0][s][g];
                    const double e1 = (double)y.y - (double)acc[1][s][g];
                    const double v0 = (double)acc[2][s][g] + p.n00, v1 = (double)acc[3][s][g] + p.n11;
                    const double c = (double)acc[4][s][g] + p.n01;
                    const double det = v0 * v1 - c * c;
                    const double q0 = e0 * e0, q1 = e1 * e1;
                    const double m2 = (v1 * q0 - 2.0 * c * e0 * e1 + v0 * q1) / det;
                    const double z0 = q0 / v0, z1 = q1 / v1;
                    sm[0] += 1.0;
                    sm[1] += -0.5 * (log(det) + m2 + LOG2PI2);
                    sm[2] += m2;
                    sm[3] += z0;
                    sm[4] += z1;
                    sm[5] += v0;
                    sm[6] += v1;
                    sm[7] += q0;
                    sm[8] += q1;
#pragma unroll
                    for (int l = 0; l < AME_PREDICT_MAX_LEVELS; ++l) {
                        if (l < p.n_levels) {
                            sm[9 + 3 * l] += (z0 <= p.zsq[l]) ? 1.0 : 0.0;
                            sm[10 + 3 * l] += (z1 <= p.zsq[l]) ? 1.0 : 0.0;
                            sm[11 + 3 * l] += (m2 <= p.csq[l]) ? 1.0 : 0.0;
                        }
                    }
                }
            }
        }
        block_sum<AME_PNS>(sm, red);
        if (threadIdx.x == 0) {
            double* o = p.partial + ((size_t)tl * ntile + tile) * AME_PNS;
#pragma unroll
            for (int q = 0; q < AME_PNS; ++q) o[q] = sm[q];
        }
    } else {
        const int ni = p.i1 - p.i0, nj = p.j1 - p.j0;
        const float n00 = (float)p.n00, n01 = (float)p.n01, n11 = (float)p.n11;
        const float qnan = __builtin_nanf("");
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = ld.j(s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ld.i(g);
                if (i < ilim && j < jlim) {
                    float* o = p.dense + (((size_t)tl * ni + (i - p.i0)) * nj + (j - p.j0)) * 5;
                    const bool dg = i == j;
                    o[0] = acc[0][s][g];
                    o[1] = acc[1][s][g];
                    o[2] = dg ? qnan : acc[2][s][g] + n00;
                    o[3] = dg ? qnan : acc[3][s][g] + n11;
                    o[4] = dg ? qnan : acc[4][s][g] + n01;
                }
            }
        }
    }
}

static inline long long predict_feat_doubles(const ame_dims* dm) {
    return ((long long)dm->T_local * dm->n * ame_predict_row(dm->r) + 1) / 2;
}

#if AME_PART0
long long ame_predict_work_doubles(const ame_dims* dm) {
    return predict_feat_doubles(dm) + (long long)dm->T_local * ame_tri_tiles(dm->n) * AME_PNS;
}

// workgroups of the largest launch ame_predict would make (the caller checks it fits a grid)
long long ame_predict_max_blocks(const ame_dims* dm, const ame_predict_args* a) {
    long long m = (long long)dm->T_local * dm->n;
    if (a->sums) {
        const long long b = (long long)dm->T_local * ame_tri_tiles(dm->n);
        m = b > m ? b : m;
    }
    if (a->dense) {
        const long long b = (long long)dm->T_local * ((a->i1 - a->i0 + AME_DT - 1) / AME_DT) *
                            ((a->j1 - a->j0 + AME_DT - 1) / AME_DT);
        m = b > m ? b : m;
    }
    return m;
}

// the dyad part of ame_mstep_stats' work buffer: feature rows, then tile partials
long long ame_mstep_dyad_work_doubles(const ame_dims* dm) {
    return predict_feat_doubles(dm) + (long long)dm->T_local * ame_tri_tiles(dm->n) * AME_MS_DYAD;
}
long long ame_probit_score_work_doubles(const ame_dims* dm) {
    return predict_feat_doubles(dm) + (long long)dm->T_local * ame_tri_tiles(dm->n) * AME_PROBIT_SUMS;
}
// ame_probit_rank / ame_probit_select keep nothing per tile: the feature rows only
long long ame_probit_rank_work_doubles(const ame_dims* dm) { return predict_feat_doubles(dm); }
// ame_resid_nodes: the feature rows, then one [n][AME_NODE_SUMS] row per slice and slot
long long ame_resid_nodes_work_doubles(const ame_dims* dm) {
    const long long nb = (dm->n + AME_DT - 1) / AME_DT;
    return predict_feat_doubles(dm) + (long long)dm->T_local * (nb + 1) * dm->n * AME_NODE_SUMS;
}
long long ame_mstep_dyad_blocks(const ame_dims* dm) {
    const long long a = (long long)dm->T_local * dm->n, b = (long long)dm->T_local * ame_tri_tiles(dm->n);
    return a > b ? a : b;
}
#endif

// What ame_predict and the M-step dyad statistics share: the feature kernel into
// the head of `work`, and the pair kernel's parameters for the upper-triangle
// tiles, with no noise, no levels and no dense block
template <int R>
static PredictParams predict_common(const ame_dims* dm, const float* x, const float* cov, const float* Yt,
                                    const void* Mt, int mask_select, double* work, hipStream_t st) {
    const int S = dm->T_local, n = dm->n;
    float* feat = (float*)work;
    hipLaunchKernelGGL(ame_predict_feat_kernel<R>, dim3((unsigned)((long long)S * n)), dim3(AME_NT), 0, st,
                       x, cov, feat);
    PredictParams p;
    p.n = n;
    p.S = S;
    p.ny = ame_ystride(n);
    p.ntile = (int)ame_tri_tiles(n);
    p.n_levels = 0;
    p.i0 = p.i1 = p.j0 = p.j1 = 0;
    p.ntj = 1;
    p.feat = feat;
    p.Yt = Yt;
    p.n00 = p.n01 = p.n11 = 0.0;
    for (int l = 0; l < AME_PREDICT_MAX_LEVELS; ++l) p.zsq[l] = p.csq[l] = 0.0;
    p.partial = work + predict_feat_doubles(dm);
    p.dense = nullptr;
    p.Mt = (const unsigned long long*)Mt;
    p.nw = ame_mask_row_words(n);
    p.mask_select = mask_select;
    p.nbins = 1;
    p.tie_filter = -1;
    p.slice0 = 0;
    p.t_max = p.scale = 1.0;
    p.hist = nullptr;
    p.bin_min = nullptr;
    p.offset = nullptr;
    p.count = nullptr;
    p.rec = nullptr;
    p.node_partial = nullptr;
    p.rrec = nullptr;
    return p;
}

template <int R>
static int launch_predict(const ame_dims* dm, const ame_predict_args* a, hipStream_t st) {
    const int S = dm->T_local;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    p.n_levels = a->n_levels;
    p.n00 = a->noise[0];
    p.n01 = 0.5 * (a->noise[1] + a->noise[2]);
    p.n11 = a->noise[3];
    for (int l = 0; l < a->n_levels; ++l) {
        p.zsq[l] = a->zsq[l];
        p.csq[l] = a->csq[l];
    }
    if (a->sums) {
        hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 0>), dim3((unsigned)((long long)S * p.ntile)),
                           dim3(AME_NT), 0, st, p);
        hipLaunchKernelGGL(ame_tile_sum_kernel<AME_PNS>, dim3((unsigned)S), dim3(AME_NT), 0, st, p.partial,
                           p.ntile, a->sums);
    }
    if (a->dense) {
        p.i0 = a->i0; p.i1 = a->i1; p.j0 = a->j0; p.j1 = a->j1;
        const int nti = (a->i1 - a->i0 + AME_DT - 1) / AME_DT;
        p.ntj = (a->j1 - a->j0 + AME_DT - 1) / AME_DT;
        p.ntile = nti * p.ntj;
        p.dense = a->dense;
        hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 1>), dim3((unsigned)((long long)S * p.ntile)),
                           dim3(AME_NT), 0, st, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 2: the feature kernel and the five tile products of ame_predict with the
// M-step epilogue; `work` is the dyad part of ame_mstep_args.work
template <int R>
static int launch_mstep_dyad(const ame_dims* dm, const ame_mstep_args* a, double* work, hipStream_t st) {
    const int S = dm->T_local;
    const PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, work, st);
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 2>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    hipLaunchKernelGGL(ame_tile_sum_kernel<AME_MS_DYAD>, dim3((unsigned)S), dim3(AME_NT), 0, st, p.partial,
                       p.ntile, a->dyad);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 3: Bernoulli scoring of a 0 / 1 network
template <int R>
static int launch_probit_score(const ame_dims* dm, const ame_probit_score_args* a, hipStream_t st) {
    const int S = dm->T_local;
    const PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 3>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    hipLaunchKernelGGL(ame_tile_sum_kernel<AME_PROBIT_SUMS>, dim3((unsigned)S), dim3(AME_NT), 0, st, p.partial,
                       p.ntile, a->sums);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 4: class histograms of the scores; hist is zeroed on the stream first
template <int R>
static int launch_probit_rank(const ame_dims* dm, const ame_probit_rank_args* a, hipStream_t st) {
    const int S = dm->T_local;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    p.nbins = a->nbins;
    p.t_max = a->t_max;
    p.scale = a->scale;
    p.hist = (unsigned long long*)a->hist;
    if (hipMemsetAsync(a->hist, 0, (size_t)S * 2 * a->nbins * sizeof(uint64_t), st) != hipSuccess) return -3;
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 4>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 5: records at or above bin_min; count is zeroed on the stream first
template <int R>
static int launch_probit_select(const ame_dims* dm, const ame_probit_select_args* a, hipStream_t st) {
    const int S = dm->T_local;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    p.nbins = a->nbins;
    p.t_max = a->t_max;
    p.scale = a->scale;
    p.bin_min = a->bin_min;
    p.tie_filter = a->tie_filter;
    p.slice0 = a->slice0;
    p.offset = (const long long*)a->offset;
    p.count = (unsigned long long*)a->count;
    p.rec = a->records;
    if (hipMemsetAsync(a->count, 0, (size_t)S * sizeof(uint64_t), st) != hipSuccess) return -3;
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 5>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

static void resid_noise(PredictParams& p, const double* noise) {
    p.n00 = noise[0];
    p.n01 = 0.5 * (noise[1] + noise[2]);
    p.n11 = noise[3];
}

// MODE 6: per-node sums; the partial's slots are all written, then added in slot order
template <int R>
static int launch_resid_nodes(const ame_dims* dm, const ame_resid_nodes_args* a, hipStream_t st) {
    const int S = dm->T_local, n = dm->n, nb = (n + AME_DT - 1) / AME_DT;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    resid_noise(p, a->noise);
    p.node_partial = p.partial;
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 6>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    ame_col_sum(p.node_partial, nb + 1, n * AME_NODE_SUMS, 0, n * AME_NODE_SUMS, S, a->node, st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 7: histogram of m^2; hist is zeroed on the stream first
template <int R>
static int launch_resid_hist(const ame_dims* dm, const ame_resid_hist_args* a, hipStream_t st) {
    const int S = dm->T_local;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    resid_noise(p, a->noise);
    p.nbins = a->nbins;
    p.scale = a->scale;
    p.hist = (unsigned long long*)a->hist;
    if (hipMemsetAsync(a->hist, 0, (size_t)S * a->nbins * sizeof(uint64_t), st) != hipSuccess) return -3;
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 7>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// MODE 8: records at or above bin_min; count is zeroed on the stream first
template <int R>
static int launch_resid_select(const ame_dims* dm, const ame_resid_select_args* a, hipStream_t st) {
    const int S = dm->T_local;
    PredictParams p = predict_common<R>(dm, a->x, a->cov, a->Yt, a->Mt, a->mask_select, a->work, st);
    resid_noise(p, a->noise);
    p.nbins = a->nbins;
    p.scale = a->scale;
    p.bin_min = a->bin_min;
    p.slice0 = a->slice0;
    p.offset = (const long long*)a->offset;
    p.count = (unsigned long long*)a->count;
    p.rrec = a->records;
    if (hipMemsetAsync(a->count, 0, (size_t)S * sizeof(uint64_t), st) != hipSuccess) return -3;
    hipLaunchKernelGGL((ame_predict_pairs_kernel<R, 8>), dim3((unsigned)((long long)S * p.ntile)),
                       dim3(AME_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int AME_PFN(ame_resid_nodes_dispatch)(const ame_dims* dm, const ame_resid_nodes_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_resid_nodes<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_resid_hist_dispatch)(const ame_dims* dm, const ame_resid_hist_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_resid_hist<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_resid_select_dispatch)(const ame_dims* dm, const ame_resid_select_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_resid_select<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_probit_rank_dispatch)(const ame_dims* dm, const ame_probit_rank_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_probit_rank<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_probit_select_dispatch)(const ame_dims* dm, const ame_probit_select_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_probit_select<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_probit_score_dispatch)(const ame_dims* dm, const ame_probit_score_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_probit_score<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_mstep_dyad_dispatch)(const ame_dims* dm, const ame_mstep_args* a, double* work,
                                     hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_mstep_dyad<RR>(dm, a, work, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}

int AME_PFN(ame_predict_dispatch)(const ame_dims* dm, const ame_predict_args* a, hipStream_t st) {
    switch (dm->r) {
#define X(RR) \
    case RR: return launch_predict<RR>(dm, a, st);
        AME_FOR_EACH_R(X)
#undef X
        default: return -1;
    }
}
