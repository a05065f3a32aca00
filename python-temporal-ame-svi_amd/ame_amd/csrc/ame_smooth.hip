// Exact per-node smoothing across time (ame_smooth, include/ame_amd.h).
//
// Given the current means of all other nodes, node i's Gaussian posterior over
// its whole trajectory has the block-tridiagonal precision
//   D_t = P_obs(i,t) + [t = 0] S0inv + [t > 0] Qinv + [t < T-1] PtQiP,   O = -QiPhi  (block (t, t-1))
// and the linear term h_t = h_obs(i,t).  One forward / backward block solve per
// node returns mu_t, S_tt and X_t = S[t, t-1].  d = 2 + 2r is a runtime value:
// one set of kernels serves every r.  Everything is fp64; the three outputs are
// rounded to fp32 once.
//
// Unlike the sweep's per-step inverse there is no 1e-6 jitter, no "bad" masking
// and no naive diagonal (the variant is not read), and P_obs uses the symmetric
// part of R_inv (h_obs keeps R_inv as given).
//
// Observation stage
//  K1 ame_smooth_gram_kernel: per slice the Gram matrix G = sum_j w_j w_j' of
//     w_j = [1, U_j, V_j] (count, sum U, sum V, UU', VV', VU' are its blocks), one
//     workgroup per slice, nodes in ascending order.  P_obs(i,t) is G minus node
//     i's own w_i w_i', scaled by the entries of sym(R_inv).
//  K2 ame_smooth_h_kernel: h_obs for 32 nodes x one slice per workgroup; the row
//     of Y is read once, z_ij = R_inv y_ij in fp64 (zero at j = i), and the (U, V)
//     block streams through LDS in tiles of 64 nodes, so it never has to fit.
//  K2m ame_smooth_hgram_kernel (with a mask only): one wave per (slice, node),
//     four per workgroup.  The wave walks the set bits of the node's mask words
//     in ascending j, four partners to a chunk, and adds one step of
//     v_mfma_f64_16x16x4_f64 per lower-triangle tile of the 2r x 2r (U, V) Gram
//     matrix (operands and lane mapping of p0_gram_mfma, ame_sweep_dev.h: lane l
//     holds partner l >> 4 of the chunk, column 16 I + (l & 15); rows gathered
//     from x in fp32 and widened, so the products are exact; lanes of an
//     incomplete last chunk and columns >= 2r hold zero).  Column sums come
//     from the same registers by a fixed shuffle tree, the count is the
//     popcount.  H(i,t) = sum_{j hidden} w_j w_j' goes to `work` in G's index
//     order, both triangles, and P_obs over the observed partners is
//     sym(R_inv) (.) ((G - w_i w_i') - H).  K2 then takes z_ij = 0 at a hidden j.
//     The order of the sum is a property of the (slice, node) alone.
// Solve stage
//  K3 ame_smooth_solve_kernel: one workgroup per node, sequential in t.
//     Forward:  J_t = D_t - QiPhi J_{t-1}^-1 QiPhi',  g_t = h_t + QiPhi J_{t-1}^-1 g_{t-1};
//               J_t = L D L' without pivoting (a non-positive pivot marks the
//               node failed), J_t^-1 = (D^-1/2 L^-1)' (D^-1/2 L^-1).
//     Backward: B_t = -J_t^-1 QiPhi',  W = S_{t+1} B_t',  X_{t+1} = -W,
//               S_t = J_t^-1 + B_t W,  mu_t = J_t^-1 g_t - B_t mu_{t+1}.
//     J_t^-1 and J_t^-1 g_t of every step go to `work` for the backward pass;
//     the slot of step t+1 is reused for the fp64 X_{t+1}.
//     LDS: four d x (d+1) fp64 matrices (odd row stride: column reads are
//     conflict-free) and 6 d-vectors: 38.6 KB at d = 34, 144.7 KB at d = 66.
//  K4 ame_smooth_lag_kernel: lag_sum[t] += chunk partials of the fp64 X_t in
//     fixed chunks of 32 nodes, chunk by chunk in node order.
// No atomics in any sum, no waits between workgroups.
#include "ame_internal.h"
#include "ame_tile.h"   // ame_mask_row_words: the row layout of ame_pack_mask

#define AME_SM_CHUNK 32    // nodes per lag_sum partial, rows per h workgroup
#define AME_SM_JT 64        // nodes per (U, V) tile of the h kernel
#define AME_SM_HW 4         // waves, one (slice, node) each, per hidden-Gram workgroup
#define AME_SM_MAXD (2 + 2 * AME_MAX_R)

__host__ __device__ inline long long ame_smooth_lds(int r) {
    const long long d = 2 + 2 * r;
    return 8LL * (4 * d * (d + 1) + 6 * d);
}

// ---- K1: per-slice Gram matrix of w = [1, U, V] ----
template <int K>
__global__ void __launch_bounds__(AME_NT)
ame_smooth_gram_kernel(const float* __restrict__ x, int n, int r, double* __restrict__ G) {
    __shared__ float sw[AME_SM_CHUNK][2 * AME_MAX_R + 2];
    const int d = 2 + 2 * r, W = 1 + 2 * r, WW = W * W, tid = threadIdx.x, t = blockIdx.x;
    int pa[K], qa[K];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + AME_NT * k;
        const int p = (e < WW) ? e / W : 0;
        pa[k] = p;
        qa[k] = (e < WW) ? e - p * W : 0;
        acc[k] = 0.0;
    }
    const float* xs = x + (size_t)t * n * d;
    for (int j0 = 0; j0 < n; j0 += AME_SM_CHUNK) {
        for (int e = tid; e < AME_SM_CHUNK * W; e += AME_NT) {
            const int jj = e / W, c = e - jj * W, j = j0 + jj;
            sw[jj][c] = (j < n) ? (c == 0 ? 1.f : xs[(size_t)j * d + 1 + c]) : 0.f;
        }
        __syncthreads();
        const int cnt = (n - j0 < AME_SM_CHUNK) ? n - j0 : AME_SM_CHUNK;
        for (int jj = 0; jj < cnt; ++jj) {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += (double)sw[jj][pa[k]] * (double)sw[jj][qa[k]];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + AME_NT * k;
        if (e < WW) G[(size_t)t * WW + e] = acc[k];
    }
}

// ---- K2: h_obs of 32 nodes x one slice ----
// column c of h: 0 -> sum z0, 1 -> sum z1, U block -> sum z0 V_j, V block -> sum z1 U_j
__global__ void __launch_bounds__(AME_NT)
ame_smooth_h_kernel(const float* __restrict__ Yt, const float* __restrict__ x, int n, int ny, int r,
                    int T, int i0, int nc, double r00, double r01, double r10, double r11,
                    double* __restrict__ hbuf, const unsigned long long* __restrict__ Mt, int nw) {
    __shared__ double z[AME_SM_CHUNK][2 * AME_SM_JT + 2];
    __shared__ float wt[AME_SM_JT][AME_SM_MAXD + 1];
    const int d = 2 + 2 * r, tid = threadIdx.x;
    const int nrb = (nc + AME_SM_CHUNK - 1) / AME_SM_CHUNK;
    const int t = blockIdx.x / nrb, rb = blockIdx.x - t * nrb;
    const int ib = i0 + rb * AME_SM_CHUNK, iend = i0 + nc;
    const int row = tid >> 3, sub = tid & 7;
    constexpr int NQ = (AME_SM_MAXD + 7) / 8;
    double acc[NQ];
    bool one[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int c = sub + 8 * q;
        acc[q] = 0.0;
        one[q] = !(c == 0 || (c >= 2 && c < 2 + r));
    }
    const float* xs = x + (size_t)t * n * d;
    for (int j0 = 0; j0 < n; j0 += AME_SM_JT) {
        for (int e = tid; e < AME_SM_JT * d; e += AME_NT) {
            const int jj = e / d, c = e - jj * d, j = j0 + jj;
            float v = 0.f;
            if (j < n) v = (c < 2) ? 1.f : (c < 2 + r ? xs[(size_t)j * d + c + r] : xs[(size_t)j * d + c - r]);
            wt[jj][c] = v;
        }
        for (int e = tid; e < AME_SM_CHUNK * AME_SM_JT; e += AME_NT) {
            const int rr = e / AME_SM_JT, jj = e - rr * AME_SM_JT, i = ib + rr, j = j0 + jj;
            double z0 = 0.0, z1 = 0.0;
            bool on = i < iend && j < n && j != i;
            // rr is the same for the 64 lanes of a wave and j0 a multiple of 64: one word per wave
            if (Mt && on) on = !((Mt[((size_t)t * n + i) * nw + (j0 >> 6)] >> jj) & 1ull);
            if (on) {
                const float2 y = *reinterpret_cast<const float2*>(Yt + (((size_t)t * n + i) * ny + j) * 2);
                z0 = r00 * (double)y.x + r01 * (double)y.y;
                z1 = r10 * (double)y.x + r11 * (double)y.y;
            }
            z[rr][2 * jj] = z0;
            z[rr][2 * jj + 1] = z1;
        }
        __syncthreads();
        for (int jj = 0; jj < AME_SM_JT; ++jj) {
            const double z0 = z[row][2 * jj], z1 = z[row][2 * jj + 1];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = sub + 8 * q;
                if (c < d) acc[q] += (one[q] ? z1 : z0) * (double)wt[jj][c];
            }
        }
        __syncthreads();
    }
    const int i = ib + row;
    if (i < iend) {
        double* o = hbuf + ((size_t)(i - i0) * T + t) * d;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = sub + 8 * q;
            if (c < d) o[c] = acc[q];
        }
    }
}

// ---- K2m: Gram matrix of the hidden partners of one (slice, node) per wave ----
typedef double ame_smd4 __attribute__((ext_vector_type(4)));
template <int NT>
__global__ void __launch_bounds__(64 * AME_SM_HW)
ame_smooth_hgram_kernel(const float* __restrict__ x, const unsigned long long* __restrict__ Mt, int n,
                        int nw, int r, int T, int i0, int nc, double* __restrict__ H) {
    constexpr int NTL = NT * (NT + 1) / 2;
    const int lane = threadIdx.x & 63;
    // the wave's index as a scalar: the walk over the mask words below is wave-uniform
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long g = (long long)blockIdx.x * AME_SM_HW + wv;
    if (g >= (long long)T * nc) return;   // a whole wave; the kernel has no barrier
    const int t = (int)(g / nc), ii = (int)(g - (long long)t * nc), node = i0 + ii;
    const int d = 2 + 2 * r, M2 = 2 * r, W = 1 + 2 * r;
    const int ci = lane & 15, ck = lane >> 4;
    ame_smd4 acc[NTL];
#pragma unroll
    for (int q = 0; q < NTL; ++q) acc[q] = ame_smd4{0.0, 0.0, 0.0, 0.0};
    double cs[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) cs[I] = 0.0;
    const float* xs = x + (size_t)t * n * d;
    const unsigned long long* row = Mt + ((size_t)t * n + node) * nw;

    // one chunk: lane (ck, ci) holds partner p[ck]'s columns 16 I + ci, zero past `cnt` partners
    auto chunk = [&](int p0, int p1, int p2, int p3, int cnt) {
        const int j = ck == 0 ? p0 : ck == 1 ? p1 : ck == 2 ? p2 : p3;
        const bool ok = ck < cnt;
        double xd[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            const int col = 16 * I + ci;
            xd[I] = (double)((ok && col < M2) ? xs[(size_t)j * d + 2 + col] : 0.f);
            cs[I] += xd[I];
        }
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J) {
                const int q = I * (I + 1) / 2 + J;
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xd[I], xd[J], acc[q], 0, 0, 0);
            }
    };

    int p0 = 0, p1 = 0, p2 = 0, cnt = 0, total = 0;   // wave-uniform
    for (int w = 0; w < nw; ++w) {
        const unsigned long long raw = row[w];
        // (the builtin returns a signed int: widen each half as unsigned)
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)raw);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(raw >> 32));
        unsigned long long word = ((unsigned long long)hi << 32) | (unsigned long long)lo;
        // partners are j < n, j != node whatever the words hold
        const int left = n - 64 * w;
        if (left < 64) word &= (1ull << left) - 1ull;
        if ((node >> 6) == w) word &= ~(1ull << (node & 63));
        total += __builtin_popcountll(word);
        while (word) {
            const int j = 64 * w + __builtin_ctzll(word);
            word &= word - 1ull;
            if (cnt == 0) p0 = j;
            else if (cnt == 1) p1 = j;
            else if (cnt == 2) p2 = j;
            if (++cnt == 4) {
                chunk(p0, p1, p2, j, 4);
                cnt = 0;
            }
        }
    }
    if (cnt) chunk(p0, p1, p2, 0, cnt);

    // column sums: the 4 partner lanes of a column, fixed tree
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        const double s1 = cs[I] + __shfl_xor(cs[I], 16);
        cs[I] = s1 + __shfl_xor(s1, 32);
    }
    double* Hn = H + ((size_t)ii * T + t) * W * W;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J) {
            const int q = I * (I + 1) / 2 + J;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int a = 16 * I + ck + 4 * v, b = 16 * J + ci;
                if (a >= M2 || b >= M2) continue;
                Hn[(1 + a) * W + 1 + b] = acc[q][v];
                if (I != J) Hn[(1 + b) * W + 1 + a] = acc[q][v];
            }
        }
    if (ck == 0) {
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            const int a = 16 * I + ci;
            if (a < M2) {
                Hn[1 + a] = cs[I];
                Hn[(1 + a) * W] = cs[I];
            }
        }
    }
    if (lane == 0) Hn[0] = (double)total;
}

// ---- K3 helpers ----
// C = (acc ? C : 0) + alpha * op(A) op(B) on d x d LDS matrices of row stride DS,
// 2 x 2 register tiles (d is even); C aliases neither A nor B.
template <bool TA, bool TB>
__device__ __forceinline__ void sm_mm(double* __restrict__ C, const double* A, const double* B, int d,
                                      int DS, double alpha, bool acc) {
    const int h = d >> 1, nt = h * h;
    for (int tile = threadIdx.x; tile < nt; tile += AME_NT) {
        const int it = tile / h, i = 2 * it, j = 2 * (tile - it * h);
        double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double a0 = TA ? A[k * DS + i] : A[i * DS + k];
            const double a1 = TA ? A[k * DS + i + 1] : A[(i + 1) * DS + k];
            const double b0 = TB ? B[j * DS + k] : B[k * DS + j];
            const double b1 = TB ? B[(j + 1) * DS + k] : B[k * DS + j + 1];
            c00 += a0 * b0;
            c01 += a0 * b1;
            c10 += a1 * b0;
            c11 += a1 * b1;
        }
        double* c0 = C + i * DS + j;
        double* c1 = c0 + DS;
        if (acc) {
            c0[0] += alpha * c00;
            c0[1] += alpha * c01;
            c1[0] += alpha * c10;
            c1[1] += alpha * c11;
        } else {
            c0[0] = alpha * c00;
            c0[1] = alpha * c01;
            c1[0] = alpha * c10;
            c1[1] = alpha * c11;
        }
    }
}

// state index k -> which row of J_j it belongs to (0: e0 = [1, 0, V, 0], 1: e1 =
// [0, 1, 0, U]) and the index of its value in w = [1, U, V]
__device__ __forceinline__ void sm_index(int k, int r, int& sel, int& wi) {
    if (k < 2) {
        sel = k;
        wi = 0;
    } else if (k < 2 + r) {
        sel = 0;
        wi = 1 + r + (k - 2);
    } else {
        sel = 1;
        wi = 1 + (k - 2 - r);
    }
}

// ---- K3: forward / backward block solve of one node ----
__global__ void __launch_bounds__(AME_NT)
ame_smooth_solve_kernel(const float* __restrict__ x, const double* __restrict__ consts,
                        const double* __restrict__ G, const double* __restrict__ hbuf,
                        double* mfbuf, double* fac, int n, int r, int T, int i0, double rs00,
                        double rs01, double rs11, float* __restrict__ mean, float* __restrict__ cov,
                        float* __restrict__ cross, uint32_t* fail, const double* __restrict__ Hb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_bad[2];
    const int d = 2 + 2 * r, DS = d + 1, W = 1 + 2 * r, dd = d * d, tid = threadIdx.x;
    const int ii = blockIdx.x, node = i0 + ii;
    double* M0 = reinterpret_cast<double*>(smem);
    double* M1 = M0 + d * DS;
    double* M2 = M1 + d * DS;
    double* M3 = M2 + d * DS;
    double* g = M3 + d * DS;
    double* mfp = g + d;
    double* mu = mfp + d;
    double* mun = mu + d;
    double* dinv = mun + d;
    double* wi = dinv + d;
    const double* qiphi = consts + 3 * (size_t)dd;
    double* facn = fac + (size_t)ii * T * dd;
    double* mfn = mfbuf + (size_t)ii * T * d;
    const double* hn = hbuf + (size_t)ii * T * d;
    const double* Hn = Hb ? Hb + (size_t)ii * T * W * W : nullptr;   // hidden partners' Gram, or no mask
    const int tx = tid & 15, ty = tid >> 4;

    if (tid == 0) {
        s_bad[0] = 0;
        s_bad[1] = 0;
    }
    for (int e = tid; e < dd; e += AME_NT) {
        const int k = e / d, m = e - k * d;
        M3[k * DS + m] = qiphi[e];
    }
    __syncthreads();

    // ---- forward: M3 = QiPhi, M0 = J_{t-1}^-1, M1 = J_t, M2 = scratch ----
    for (int t = 0; t < T; ++t) {
        const float* xi = x + ((size_t)t * n + node) * d;
        if (tid < W) wi[tid] = (tid == 0) ? 1.0 : (double)xi[1 + tid];
        if (tid >= 64 && tid < 64 + d) g[tid - 64] = hn[(size_t)t * d + tid - 64];
        __syncthreads();
        const double* Gt = G + (size_t)t * W * W;
        for (int e = tid; e < dd; e += AME_NT) {
            const int k = e / d, m = e - k * d;
            int sk, wk, sm, wm;
            sm_index(k, r, sk, wk);
            sm_index(m, r, sm, wm);
            const double rsv = (sk == sm) ? (sk ? rs11 : rs00) : rs01;
            double gv = Gt[wk * W + wm] - wi[wk] * wi[wm];
            if (Hn) gv -= Hn[(size_t)t * W * W + wk * W + wm];
            M1[k * DS + m] = pconst_entry(consts, d, k, m, t, T) + rsv * gv;
        }
        __syncthreads();
        if (t > 0) {
            sm_mm<false, false>(M2, M3, M0, d, DS, 1.0, false);   // QiPhi J_{t-1}^-1
            if (tid < d) {
                double s = 0.0;
                for (int k = 0; k < d; ++k) s += M3[tid * DS + k] * mfp[k];
                g[tid] += s;
            }
            __syncthreads();
            sm_mm<false, true>(M1, M2, M3, d, DS, -1.0, true);    // J_t = D_t - (..) QiPhi'
            __syncthreads();
        }
        // J_t = L D L' in the lower triangle of M1, no pivoting
        for (int k = 0; k < d; ++k) {
            const double p = M1[k * DS + k];
            if (!(p > 0.0) && tid == 0 && s_bad[0] == 0) {
                s_bad[0] = 1;
                s_bad[1] = t;
            }
            const double pinv = 1.0 / p;
            for (int i = k + 1 + ty; i < d; i += 16) {
                const double aik = M1[i * DS + k] * pinv;
                for (int j = k + 1 + tx; j <= i; j += 16) M1[i * DS + j] -= aik * M1[j * DS + k];
            }
            __syncthreads();
        }
        for (int e = tid; e < dd; e += AME_NT) {
            const int i = e / d, k = e - i * d;
            if (i > k) M1[i * DS + k] *= 1.0 / M1[k * DS + k];
        }
        if (tid < d) dinv[tid] = 1.0 / M1[tid * DS + tid];
        __syncthreads();
        // column c of D^-1/2 L^-1 into M2 (upper part zero)
        if (tid < d) {
            const int c = tid;
            for (int i = 0; i < c; ++i) M2[i * DS + c] = 0.0;
            M2[c * DS + c] = 1.0;
            for (int i = c + 1; i < d; ++i) {
                double s = 0.0;
                for (int k = c; k < i; ++k) s += M1[i * DS + k] * M2[k * DS + c];
                M2[i * DS + c] = -s;
            }
            for (int i = c; i < d; ++i) M2[i * DS + c] *= sqrt(dinv[i]);
        }
        __syncthreads();
        sm_mm<true, false>(M0, M2, M2, d, DS, 1.0, false);        // J_t^-1
        __syncthreads();
        if (tid < d) {
            double s = 0.0;
            for (int k = 0; k < d; ++k) s += M0[tid * DS + k] * g[k];
            mfp[tid] = s;
            mfn[(size_t)t * d + tid] = s;
        }
        for (int e = tid; e < dd; e += AME_NT) {
            const int k = e / d, m = e - k * d;
            facn[(size_t)t * dd + e] = M0[k * DS + m];
        }
        __syncthreads();
    }

    // ---- backward: Sn = S_{t+1}, Jt = J_t^-1 then S_t, M2 = B_t, M3 = QiPhi then W ----
    double* Sn = M0;
    double* Jt = M1;
    {
        const size_t o = (size_t)(T - 1) * n + node;
        for (int e = tid; e < dd; e += AME_NT) {
            const int k = e / d, m = e - k * d;
            cov[o * dd + e] = (float)Sn[k * DS + m];
        }
        if (tid < d) {
            mu[tid] = mfp[tid];
            mean[o * d + tid] = (float)mfp[tid];
        }
    }
    __syncthreads();
    for (int t = T - 2; t >= 0; --t) {
        for (int e = tid; e < dd; e += AME_NT) {
            const int k = e / d, m = e - k * d;
            Jt[k * DS + m] = facn[(size_t)t * dd + e];
            M3[k * DS + m] = qiphi[e];
        }
        if (tid < d) g[tid] = mfn[(size_t)t * d + tid];
        __syncthreads();
        sm_mm<false, true>(M2, Jt, M3, d, DS, -1.0, false);       // B_t = -J_t^-1 QiPhi'
        __syncthreads();
        sm_mm<false, true>(M3, Sn, M2, d, DS, 1.0, false);        // W = S_{t+1} B_t'
        if (tid < d) {
            double s = 0.0;
            for (int k = 0; k < d; ++k) s += M2[tid * DS + k] * mu[k];
            mun[tid] = g[tid] - s;
        }
        __syncthreads();
        {
            const size_t o = (size_t)(t + 1) * n + node;
            for (int e = tid; e < dd; e += AME_NT) {
                const int k = e / d, m = e - k * d;
                const double v = -M3[k * DS + m];                 // X_{t+1} = S[t+1, t]
                cross[o * dd + e] = (float)v;
                facn[(size_t)(t + 1) * dd + e] = v;
            }
        }
        sm_mm<false, false>(Jt, M2, M3, d, DS, 1.0, true);        // S_t = J_t^-1 + B_t W
        __syncthreads();
        for (int e = tid; e < dd; e += AME_NT) {
            const int k = e / d, m = e - k * d;
            if (k < m) {
                const double a = 0.5 * (Jt[k * DS + m] + Jt[m * DS + k]);
                Jt[k * DS + m] = a;
                Jt[m * DS + k] = a;
            }
        }
        __syncthreads();
        {
            const size_t o = (size_t)t * n + node;
            for (int e = tid; e < dd; e += AME_NT) {
                const int k = e / d, m = e - k * d;
                cov[o * dd + e] = (float)Jt[k * DS + m];
            }
            if (tid < d) mean[o * d + tid] = (float)mun[tid];
        }
        double* sw = Sn;
        Sn = Jt;
        Jt = sw;
        sw = mu;
        mu = mun;
        mun = sw;
        __syncthreads();
    }
    for (int e = tid; e < dd; e += AME_NT) {
        cross[(size_t)node * dd + e] = 0.f;
        facn[e] = 0.0;
    }
    if (s_bad[0]) {   // uniform over the workgroup (last written before many barriers)
        const float qn = __builtin_nanf("");
        const double qd = __builtin_nan("");
        for (int t = 0; t < T; ++t) {
            const size_t o = (size_t)t * n + node;
            for (int e = tid; e < dd; e += AME_NT) {
                cov[o * dd + e] = qn;
                cross[o * dd + e] = qn;
                if (t > 0) facn[(size_t)t * dd + e] = qd;
            }
            if (tid < d) mean[o * d + tid] = qn;
        }
        if (tid == 0) {
            atomicAdd(fail, 1u);
            if (atomicCAS(fail + 1, 0u, 1u) == 0u) {
                fail[2] = (uint32_t)node;
                fail[3] = (uint32_t)s_bad[1];
            }
        }
    }
}

// ---- K4: lag_sum[t] (+)= sum over the call's nodes of the fp64 X_t, 32-node partials in order ----
static __global__ void __launch_bounds__(AME_NT)
ame_smooth_lag_kernel(const double* __restrict__ fac, int nc, int T, int dd, int first,
                      double* __restrict__ lag) {
    const long long g = (long long)blockIdx.x * AME_NT + threadIdx.x;
    if (g >= (long long)T * dd) return;
    const int t = (int)(g / dd);
    double s = first ? 0.0 : lag[g];
    if (t > 0) {
        for (int c0 = 0; c0 < nc; c0 += AME_SM_CHUNK) {
            const int c1 = (c0 + AME_SM_CHUNK < nc) ? c0 + AME_SM_CHUNK : nc;
            double p = 0.0;
            for (int i = c0; i < c1; ++i) p += fac[(size_t)i * T * dd + g];
            s += p;
        }
    }
    lag[g] = s;
}

// work layout (doubles): G [T][W][W] | h [nc][T][d] | J^-1 g [nc][T][d] | factors [nc][T][d][d]
long long ame_smooth_work_doubles(const ame_dims* dm, int nodes) {
    const long long d = 2 + 2 * dm->r, W = 1 + 2 * dm->r, T = dm->T_local;
    return T * W * W + (long long)nodes * T * (2 * d + d * d);
}

// with a mask, appended: H [nc][T][W][W]
long long ame_smooth_hidden_doubles(const ame_dims* dm, int nodes) {
    const long long W = 1 + 2 * dm->r;
    return (long long)nodes * dm->T_local * W * W;
}

long long ame_smooth_lds_bytes_r(int r) { return ame_smooth_lds(r); }

int ame_smooth_dispatch(const ame_dims* dm, const ame_smooth_args* a, hipStream_t st) {
    const int n = dm->n, r = dm->r, T = dm->T_local, d = 2 + 2 * r, W = 1 + 2 * r, dd = d * d;
    const int i0 = a->i0, nc = a->i1 - a->i0;
    double* G = a->work;
    double* hbuf = G + (size_t)T * W * W;
    double* mfbuf = hbuf + (size_t)nc * T * d;
    double* fac = mfbuf + (size_t)nc * T * d;
    double* Hb = a->Mt ? fac + (size_t)nc * T * dd : nullptr;
    const unsigned long long* Mt = (const unsigned long long*)a->Mt;
    const int nw = ame_mask_row_words(n);
    const int stages = a->stages ? a->stages : (AME_SMOOTH_STAGE_OBS | AME_SMOOTH_STAGE_SOLVE);
    if (stages & AME_SMOOTH_STAGE_OBS) {
        const int K = (W * W + AME_NT - 1) / AME_NT;
#define AME_SM_GRAM(KK) \
    hipLaunchKernelGGL(ame_smooth_gram_kernel<KK>, dim3(T), dim3(AME_NT), 0, st, a->x, n, r, G)
        if (K <= 1) AME_SM_GRAM(1);
        else if (K <= 2) AME_SM_GRAM(2);
        else if (K <= 5) AME_SM_GRAM(5);
        else if (K <= 10) AME_SM_GRAM(10);
        else if (K <= 17) AME_SM_GRAM(17);
        else return -1;
#undef AME_SM_GRAM
        const int nrb = (nc + AME_SM_CHUNK - 1) / AME_SM_CHUNK;
        hipLaunchKernelGGL(ame_smooth_h_kernel, dim3((unsigned)((long long)T * nrb)), dim3(AME_NT), 0, st,
                           a->Yt, a->x, n, ame_ystride(n), r, T, i0, nc, a->rinv[0], a->rinv[1],
                           a->rinv[2], a->rinv[3], hbuf, Mt, nw);
        if (Mt) {
            const dim3 grid((unsigned)(((long long)T * nc + AME_SM_HW - 1) / AME_SM_HW));
#define AME_SM_HGRAM(NT) \
    hipLaunchKernelGGL(ame_smooth_hgram_kernel<NT>, grid, dim3(64 * AME_SM_HW), 0, st, a->x, Mt, n, nw, r, \
                       T, i0, nc, Hb)
            switch ((2 * r + 15) / 16) {
                case 1: AME_SM_HGRAM(1); break;
                case 2: AME_SM_HGRAM(2); break;
                case 3: AME_SM_HGRAM(3); break;
                case 4: AME_SM_HGRAM(4); break;
                default: return -1;
            }
#undef AME_SM_HGRAM
        }
    }
    if (stages & AME_SMOOTH_STAGE_SOLVE) {
        const int lds = (int)ame_smooth_lds(r);
        if (hipFuncSetAttribute((const void*)ame_smooth_solve_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return -2;
        hipLaunchKernelGGL(ame_smooth_solve_kernel, dim3(nc), dim3(AME_NT), (size_t)lds, st, a->x,
                           a->consts, G, hbuf, mfbuf, fac, n, r, T, i0, a->rinv[0],
                           0.5 * (a->rinv[1] + a->rinv[2]), a->rinv[3], a->mean, a->cov, a->cross,
                           a->fail, Hb);
        const long long total = (long long)T * dd;
        hipLaunchKernelGGL(ame_smooth_lag_kernel, dim3((unsigned)((total + AME_NT - 1) / AME_NT)),
                           dim3(AME_NT), 0, st, fac, nc, T, dd, i0 == 0 ? 1 : 0, a->lag_sum);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
