/*
 * ame_amd.h — C ABI of the MI355X (gfx950) implementation of the temporal-AME
 * structured / naive mean-field VI hot path.
 *
 * Drop-in boundary.  The reference (Alfieriek/Python-Temporal-AME-SVI) is pure
 * Python: its "interface" for this path is the template-method hooks of
 * BaseVariationalInference (src/inference/base.py:84-125) that fit()
 * (base.py:127-208) calls once per iteration.  Each entry point below replaces
 * one of those hooks (or the loop nest inside it); the Python host classes in
 * ame_amd/inference mirror the reference classes on top of this ABI.
 *
 *   ame_pack_y        replaces nothing in the reference: relayout of the
 *                     observed network Y (n,n,T,2) (temporal_ame.py:174) into
 *                     the time-major (T,n,n,2) layout the kernels stream.
 *   ame_sweep         replaces _update_step -> _update_node_i ->
 *                     _compute_observation_terms (structured_mf.py:211-326,
 *                     naive_mf.py:193-376): the sequential Gauss-Seidel sweep,
 *                     new means AND new (damped) covariances.
 *   ame_cov           the per-(node,time) covariance terms of the ELBO
 *                     (_compute_entropy :202-209, trace terms :142-144, :166,
 *                     :193) of the stored covariances.
 *   ame_elbo          replaces _compute_elbo (structured_mf.py:115-209,
 *                     naive_mf.py:89-191) and
 *                     compute_temporal_reconstruction_error
 *                     (temporal_ame.py:255-291): returns the sufficient sums
 *                     from which the host assembles ELBO and MSE.
 *   ame_predict       replaces nothing in the reference: posterior-predictive
 *                     mean and 2x2 covariance of every dyad from (means,
 *                     covariances), scored against the observed network
 *                     (the input metrics.py:350-518 expects and nothing there
 *                     produces), as per-slice sums or a dense block.
 *   ame_mstep_stats   replaces nothing in the reference: the sufficient
 *                     statistics of q from which the closed-form M-step of
 *                     variational EM re-estimates Phi, Q, R, Sigma and Psi.
 *   ame_smooth        replaces nothing in the reference: each node's exact
 *                     Gaussian posterior across time given the other nodes'
 *                     means (block-tridiagonal solve): smoothed means, marginal
 *                     covariances and lag-one cross-covariances.
 *   ame_covar_stats,  replace nothing in the reference: the regression on dyadic
 *   ame_covar_resid   covariates (all-pairs sums for the closed-form M-step of
 *                     beta; the residual network every other entry point reads).
 *   ame_pack_mask,    replace nothing in the reference: partially observed
 *   ame_fill_missing  networks (the packed mask of hidden pairs; the working
 *                     network the sweep and the ELBO kernels read in their place).
 *   ame_net_moments,  replace nothing in the reference: goodness of fit by network
 *   ame_net_triads,   statistics (row / column heterogeneity, reciprocity, cycles,
 *   ame_simulate      transitivity) of the observed network and of networks
 *                     simulated from the fitted states.
 *   ame_probit_fill,  replace nothing in the reference: binary networks with a
 *   ame_probit_score  probit link (the working network the sweep reads in place of
 *                     a 0 / 1 network; Bernoulli scores of held-out links).
 *   ame_probit_rank,  replace nothing in the reference: ranking the links of a binary
 *   ame_probit_select network (per-slice class histograms of the scores for ROC / AUC;
 *                     the records of the highest-scoring entries for a top-k list).
 *   ame_resid_nodes,  replace nothing in the reference: residual diagnostics of a
 *   ame_resid_hist,   Gaussian fit (per-node sums of the dyad scores; the per-slice
 *   ame_resid_select  histogram of the Mahalanobis distance m^2; the records of the
 *                     most surprising pairs for a top-k list).
 *
 * Conventions: all pointers are DEVICE pointers (hipMalloc / torch CUDA
 * tensors) unless the field says otherwise; `stream` is a hipStream_t (NULL =
 * default stream); no entry point allocates, frees or synchronises.  Return
 * value 0 = launched; negative = argument error (see ame_last_error()).
 * Device-side failures (spin timeout, non-finite pivot) are reported through
 * the `status` word, which the host reads after the iteration.
 *
 * Layouts (row-major, fp32 unless stated):
 *   Yt      [T_local][n][ny][2]   Yt[t][i][j] = Y[i][j][t0+t] of the reference for j < n;
 *                                 ny = n rounded up to even (rows 16-byte aligned), the
 *                                 pad pair j = n (odd n) is zero; ame_pack_y_size()
 *   X mean  [T_local][n][d]       d = 2 + 2r, x = [a, b, U(r), V(r)]
 *   X cov   [T_local][n][d][d]
 *   consts  fp64 [5][d][d]: S0inv, Qinv, PhiT*Qinv*Phi, Qinv*Phi, PhiT*Qinv
 */
#ifndef AME_AMD_H
#define AME_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ame_variant { AME_GOOD = 0, AME_BAD = 1, AME_NAIVE = 2 };

/* status word bits (device-written) */
#define AME_STATUS_SPIN_TIMEOUT 1u
#define AME_STATUS_HALO_TIMEOUT 2u
#define AME_STATUS_LDS_TIMEOUT 4u   /* intra-workgroup hand-off timed out (internal error) */
/* a hand-off word (done flag, back-channel done word, {epoch, value} granule)
 * carried an epoch the protocol cannot have produced yet: a stale buffer or an
 * unordered host write; the word is not consumed as if it were current */
#define AME_STATUS_STALE_EPOCH 8u

/* The status block: AME_STATUS_WORDS uint32 words (the caller zeroes it once
 * and again after reading a failure).
 *   [0]  AME_STATUS_* bits
 *   [1]  1 once the FIRST failing wait has written its record into [2..8]
 *   [2]  wait site (enum ame_wait_site)     [3] global time slice of the waiter
 *   [4]  node index (0xFFFFFFFF: before the node loop)
 *   [5]  word observed (epoch tag, done value, LDS count)   [6] value expected
 *   [7]  microseconds waited                [8] the sweep's epoch
 *   [9]  device bookkeeping: workgroups inside a cross-rank wait right now
 *   [10] waits that gave up quietly because [0] was already non-zero
 *   [11] microseconds the rank's first slice spun on the left rank's granules
 *   [12] microseconds its last slice spun on the right rank's back channel
 *        ([11], [12] accumulate over sweeps; the caller reads differences)
 * Wait rules (every kernel that spins): a wait gives up quietly -- no bit of its
 * own -- once [0] is non-zero (one failure does not manufacture more); a wait
 * on this GPU (slice -> slice, done flags, LDS counters) restarts its 2 s
 * budget while [9] > 0, since its producer may then sit behind a neighbouring
 * rank, whose own wait has the 10 s budget; a workgroup that failed or gave up
 * stores no done flag, back channel or current-epoch hand-off granule. */
#define AME_STATUS_WORDS 16
enum ame_wait_site {
    AME_WAIT_DONE_SELF = 1,     /* pipelined prologue: done[t] of the previous sweep */
    AME_WAIT_DONE_RIGHT = 2,    /* pipelined prologue: done[t+1] (or the next group's first slice) */
    AME_WAIT_BACK = 3,          /* pipelined prologue: the right rank's back-channel done word */
    AME_WAIT_GRAN_LOCAL = 4,    /* hand-off granule of slice t-1 on this GPU */
    AME_WAIT_GRAN_HALO = 5,     /* hand-off granule of the left rank's last slice */
    AME_WAIT_LDS = 6,           /* intra-workgroup LDS counter */
    AME_WAIT_WORKER_GRAN = 7,   /* GEMV worker: new-mean granule of its slice */
    AME_WAIT_PARTIAL = 8        /* slice workgroup: a GEMV worker's partial */
};

/* float offset of the done word in a back channel of n*d floats */
#define AME_BACK_DONE_OFFSET(nd) ((((nd) + 63) / 64) * 64)

/* Sweep kernels.  Concrete kinds (what ame_sweep launches):
 *   AME_SWEEP_V3          one 512-thread workgroup per slice (solver wave + 7
 *                         helper waves, slice (U,V) in registers/LDS); the slice's
 *                         state must fit one CU's 160 KiB LDS, which holds for
 *                         r <= 23 only: n <= 3456 up to r = 6, falling to
 *                         n <= 1344 at r = 16, 896 at r = 20, 768 at r = 21,
 *                         384 at r = 22 and 128 at r = 23 (ame_sweep_kind tells;
 *                         tests/test_every_r_guard.py pins the bound)
 *   AME_SWEEP_V2_LDS      one 256-thread workgroup per slice, (U,V) block in LDS
 *   AME_SWEEP_V2_HBM      same, (U,V) block in HBM (args.work)
 *   AME_SWEEP_V2_WORKERS  v2 plus seven GEMV worker workgroups per slice holding
 *                         the (U,V) block in registers (partial ring in args.work)
 *   AME_SWEEP_V2_PIPE     v2 plus four GEMV worker workgroups per slice (5 per
 *                         slice): two launches of up to half the co-resident
 *                         slices fit at once and the kernel orders itself slice
 *                         by slice (done flags, wait_epoch), so sweeps and slice
 *                         groups pipeline like AME_SWEEP_V3; d > 64, n <= 4096
 *   AME_SWEEP_V2_W6       v2 plus six GEMV worker workgroups per slice (7 per
 *                         slice), not pipelined: BASELINE config 5's 32 slices
 *                         hold 224 CUs, so the ELBO kernels can run beside the
 *                         next sweep on the other 32 (CU-masked streams,
 *                         ame_stream_create_cu_range); n <= 4224
 * Requests (resolved by ame_sweep_kind for given dims):
 *   AME_SWEEP_AUTO        V3 when the shape fits it, else AME_SWEEP_V2_AUTO
 *   AME_SWEEP_V2_AUTO     V2_WORKERS when their workgroups are co-resident, else
 *                         AME_SWEEP_V2_SINGLE
 *   AME_SWEEP_V2_SINGLE   V2_LDS when the block fits one CU's LDS, else V2_HBM
 * A concrete kind is also a valid request (resolved to itself or rejected). */
enum ame_sweep_kind_code {
    AME_SWEEP_AUTO = 0,
    AME_SWEEP_V2_SINGLE = 1,
    AME_SWEEP_V2_AUTO = 2,
    AME_SWEEP_V3 = 3,
    AME_SWEEP_V2_LDS = 20,
    AME_SWEEP_V2_HBM = 21,
    AME_SWEEP_V2_WORKERS = 22,
    AME_SWEEP_V2_PIPE = 23,
    AME_SWEEP_V2_W6 = 24
};

/* ame_sweep_args.flags */
#define AME_SWEEP_FLAG_NEXT_GROUP 1u   /* done[T_local] is the next slice group's first slice
                                          (same rank): with wait_epoch, the last slice also
                                          waits for it, as for any other right neighbour */
#define AME_SWEEP_FLAG_PREV_GROUP 2u   /* halo_in is the previous slice group's hand-off
                                          buffer on this GPU, not a neighbouring rank's: the
                                          first slice's wait on it is a local wait (2 s
                                          budget, not counted in status words 9 / 11) */

/* ELBO pair kernels (ame_elbo_args.pairs_kernel): AUTO = V2 (LDS-DMA rows). */
enum ame_pairs_kernel_code { AME_PAIRS_AUTO = 0, AME_PAIRS_V1 = 1, AME_PAIRS_V2 = 2 };

typedef struct ame_dims {
    int32_t n;        /* nodes */
    int32_t r;        /* latent_dim; d = 2 + 2r */
    int32_t T_local;  /* time slices held by this rank */
    int32_t t_begin;  /* global index of local slice 0 */
    int32_t T_total;  /* global number of time steps */
    int32_t variant;  /* enum ame_variant */
} ame_dims;

typedef struct ame_sweep_args {
    const float* Yt;             /* [T_local][n][ny][2] */
    const float* x_old;          /* [T_local][n][d] means before the sweep */
    float* x_new;                /* [T_local][n][d] means after the sweep */
    const float* next_old;       /* [n][d] old means at global slice t_begin+T_local
                                    (right halo), NULL if this rank holds T-1 */
    uint64_t* hand;              /* [T_local][n][d] {epoch,value} granules, lane hand-off */
    const uint64_t* halo_in;     /* [n][d] granules of slice t_begin-1 (left rank), or NULL */
    uint64_t* halo_out;          /* [n][d] granules of slice t_begin+T_local-1 for the right
                                    rank (its peer buffer, ame_peer_open), or NULL */
    float* cov;                  /* [T_local][n][d][d] covariances before the sweep (damped in
                                    place when cov_new is NULL) */
    const double* consts;        /* fp64 [5][d][d] */
    double rinv[4];              /* R_inv row-major (host values) */
    float lr;                    /* learning_rate (damping) */
    float one_minus_lr;          /* (float)(1 - lr) computed in double on the host */
    uint32_t epoch;              /* sweep counter, >= 1, identical on every rank */
    uint32_t* status;            /* [AME_STATUS_WORDS] status block (bits + first-failure record) */
    double* work;                /* scratch, >= ame_sweep_work_size() doubles: 0 for the v3
                                    sweep; the GEMV workers' partial ring (zeroed by the call
                                    itself) and the right-neighbour AR terms (filled by the call)
                                    for v2 with workers (kinds 22 / 23: n = 4096, r = 32, ...);
                                    [T_local][n][2r] fp32 (U,V) copy when v2 keeps the slice in
                                    HBM without workers (kind 21); may be NULL
                                    when the size is 0 */
    float* cov_new;              /* [T_local][n][d][d] damped covariances after the sweep, or NULL
                                    (in place).  A separate buffer lets ame_cov / ame_elbo read
                                    `cov` while the next sweep already runs (engine speculation) */
    uint32_t* done;              /* [T_local] per-slice "finished sweep <epoch>" words (zeroed once by
                                    the caller), or NULL */
    uint32_t wait_epoch;         /* 0, or: slice t starts only once done[t] and done[t+1] reach this
                                    epoch, so the next sweep can be queued while the previous one
                                    (epoch wait_epoch) still runs.  Needs ame_sweep_orders_slices()
                                    and room for both sweeps' workgroups (2 T_local <= max_slices) */
    float* back_out;             /* time-sharded, rank with a left neighbour: that rank's peer
                                    buffer [n*d floats | done word at AME_BACK_DONE_OFFSET] the first
                                    slice fills with its new means when it finishes, or NULL */
    const float* back_in;        /* the right neighbour's back_out: in a pipelined launch
                                    (wait_epoch != 0) it replaces next_old */
    int32_t kind;                /* enum ame_sweep_kind_code: the kernel the caller sized the
                                    buffers for (normally the concrete kind ame_sweep_kind
                                    returned); a request it does not resolve to is rejected */
    uint32_t flags;              /* AME_SWEEP_FLAG_* (0 for one launch over all local slices) */
    uint64_t work_doubles;       /* size of `work` in doubles, checked against
                                    ame_sweep_work_size(dims, kind) */
} ame_sweep_args;

typedef struct ame_cov_args {
    const float* cov;            /* [T_local][n][d][d] */
    const double* consts;        /* fp64 [5][d][d] */
    double* cov_terms;           /* [T_local][n][4] fp64: logdet, trace, tr(Qinv S), tr(S0inv S) */
} ame_cov_args;

typedef struct ame_elbo_args {
    const float* Yt;             /* [T_local][n][ny][2] */
    const float* x;              /* [T_local][n][d] means */
    const float* prev_final;     /* [n][d] means at global slice t_begin-1 (left halo) or NULL */
    const double* cov_terms;     /* [T_local][n][4] from ame_cov */
    const double* consts;        /* fp64 [5][d][d] */
    const double* phi;           /* fp64 [d][d] Phi */
    double rinv[4];
    int32_t swap_consistent;     /* 1: Y[j][i] == swap(Y[i][j]) for all pairs (checked at pack) */
    double* work;                /* scratch, >= ame_elbo_work_size() doubles */
    double* out;                 /* [8] sufficient sums (see ame_elbo doc) */
    int32_t pairs_kernel;        /* enum ame_pairs_kernel_code (0 = default) */
} ame_elbo_args;

/* Relayout Y [n][n][T_total][2] -> Yt [T_local][n][ny][2] for slices
 * [t_begin, t_begin+T_local), and count pairs with Y[j][i] != swap(Y[i][j])
 * into *mismatch (device uint64, caller zeroes it). */
int ame_pack_y(const float* Y, float* Yt, const ame_dims* dims,
               unsigned long long* mismatch, void* stream);

/* Floats of Yt for these dims (T_local * n * ny * 2), -1 on bad dims. */
long long ame_pack_y_size(const ame_dims* dims);

/* One Gauss-Seidel sweep over all n nodes for the local slices: new means and
 * new (damped) covariances.  One workgroup per local slice; all T_local
 * workgroups must be co-resident (see ame_sweep_max_slices).  Reproduces the
 * reference node order exactly: step (i,t) sees new means of nodes j<i at t
 * and of node i at t-1, and old means of nodes j>i at t and of node i at t+1. */
int ame_sweep(const ame_dims* dims, const ame_sweep_args* args, void* stream);

/* 1 when the sweep kernel `kind` (concrete) honours done / wait_epoch, else 0. */
int ame_sweep_orders_slices(int n, int r, int kind);

/* The concrete kernel (enum ame_sweep_kind_code) a request resolves to for
 * these dims, or -1 (unsupported dims, or the requested kernel cannot run
 * them; see ame_last_error).  Nothing in the library reads the environment:
 * the kind is chosen here, by the caller's request, once. */
int ame_sweep_kind(const ame_dims* dims, int request);

/* Scratch doubles ame_sweep needs in args->work for a concrete kind (see the
 * field); -1 on bad dims / kind. */
long long ame_sweep_work_size(const ame_dims* dims, int kind);

/* Largest T_local one ame_sweep launch can hold for (n, r) and a request on
 * this device (all its workgroups co-resident), 0 if the per-slice state does
 * not fit.  For AME_SWEEP_AUTO / V2_AUTO with v2 this counts the slice
 * workgroups alone (workers are then used when they fit, ame_sweep_kind). */
int ame_sweep_max_slices(int n, int r, int request);

/* Workgroups one slice occupies in a launch of a concrete kind (the slice's
 * own plus its GEMV workers; each is one CU's worth of LDS), -1 for a request
 * or an unknown kind.  A caller that confines the sweep to a CU range
 * (ame_stream_create_cu_range) sizes the launch with it. */
int ame_sweep_slice_workgroups(int kind);

/* Dynamic LDS bytes per slice workgroup of a concrete kind (0 = unsupported). */
long long ame_sweep_lds_bytes(int n, int r, int kind);

/* Per-(node, local slice) covariance terms of the ELBO (log|S|, tr S,
 * tr(Qinv S), tr(S0inv S)), fully parallel: 64/(2r) covariances per wave. */
int ame_cov(const ame_dims* dims, const ame_cov_args* args, void* stream);

/* ELBO / reconstruction sufficient sums over the local slices:
 *  out[0] sum_{t, i<j} r^T Rinv r          out[1] sum_{i,t} tr(S_it)
 *  out[2] sum_i mu_i0^T S0inv mu_i0        out[3] sum_i tr(S0inv S_i0)
 *  out[4] sum_{i,t>=1} e^T Qinv e          out[5] sum_{i,t>=1} tr(Qinv S_it)
 *  out[6] sum_{i,t} logdet S_it            out[7] sum_{t, i!=j} |Y_ij - m_ij|^2
 * (slice-0 / t>=1 terms use global time; the host adds the constants). */
int ame_elbo(const ame_dims* dims, const ame_elbo_args* args, void* stream);

/* Scratch doubles ame_elbo needs. */
long long ame_elbo_work_size(const ame_dims* dims);

/* Diagnostic (timing) entry point: launches ONLY the pair kernel of ame_elbo
 * (its per-workgroup partials land in args->work; args->out is NOT written).
 * Not part of an iteration; bench.py times the pair kernel alone with it. */
int ame_elbo_pairs_diag(const ame_dims* dims, const ame_elbo_args* args, void* stream);

/* ---- posterior-predictive dyad moments and scoring ---------------------------
 * Replaces nothing the reference computes: it supplies what its
 * calibration_error / compute_coverage / temporal_prediction_metrics
 * (src/utils/metrics.py:350-518) take as input, predictive intervals of the
 * dyads, from the means AND covariances of q.  With q(x_i) = N(m_i, S_i)
 * independent across nodes and mu_ij = (a_i + b_j + U_i.V_j, a_j + b_i + U_j.V_i)
 * (static_ame.py:189-238), for i != j
 *   E[mu_ij[0]]  = m_i[a] + m_j[b] + u_i.v_j
 *   V0(i,j)      = Var[mu_ij[0]] = S_i[aa] + S_j[bb] + v_j' S_i[UU] v_j
 *                  + u_i' S_j[VV] u_i + tr(S_i[UU] S_j[VV]) + 2 S_i[aU].v_j + 2 u_i.S_j[bV]
 *   Var[mu_ij[1]] = V0(j,i)
 *   C01(i,j)     = Cov[mu_ij[0], mu_ij[1]] = S_i[ab] + S_j[ab] + u_j.S_i[aV] + S_j[bU].v_i
 *                  + S_i[bU].v_j + u_i.S_j[aV] + tr(C_i C_j) + v_j' C_i u_j + v_i' C_j u_i,
 *                  C = S[UV] (rows U, columns V)
 * and the predictive covariance of (y_ij, y_ji) is [[V0(i,j), C01], [C01, V0(j,i)]] + N
 * (N = `noise`, symmetric: model.R for observations, zeros for the mean).  Any
 * variant's covariances are read as full d x d matrices.  The slices are
 * independent: dims.t_begin / T_total / variant are only range-checked, so a
 * caller may pass any [S][n][..] stack (forecast states) with T_local = S.
 *
 * Scoring (sums != NULL, needs Yt): unordered pairs i < j with the upper
 * triangle Yt[t][i][j] as the observation (structured_mf.py:136-137),
 * e = y - E[mu_ij], z_c^2 = e_c^2 / Sigma_cc, m^2 = e' Sigma^-1 e.  Per slice:
 *   [0] pairs scored   [1] sum log N(y; E[mu], Sigma)   [2] sum m^2
 *   [3],[4] sum z_0^2, z_1^2   [5],[6] sum Sigma_00, Sigma_11   [7],[8] sum e_0^2, e_1^2
 *   [9+3l],[10+3l],[11+3l] counts of z_0^2 <= zsq[l], z_1^2 <= zsq[l], m^2 <= csq[l]
 * (slots of levels >= n_levels are 0).  The sums are per-workgroup fp64
 * partials reduced in a fixed order: bit-identical from run to run.
 * Dense (dense != NULL): the five moments of every ordered pair of the block
 * rows [i0, i1) x columns [j0, j1); on the diagonal i == j the means are
 * compute_mean's and the three second moments are NaN (the independence the
 * formulas rest on does not hold there). */
#define AME_PREDICT_MAX_LEVELS 4
#define AME_PREDICT_SUMS (9 + 3 * AME_PREDICT_MAX_LEVELS)
/* mask_select of ame_predict_args / ame_mstep_args (missing dyads, below) */
#define AME_MASK_OBSERVED 1
#define AME_MASK_HIDDEN 2
typedef struct ame_predict_args {
    const float* x;      /* [S][n][d] means              (S = dims.T_local)           */
    const float* cov;    /* [S][n][d][d] covariances                                  */
    const float* Yt;     /* [S][n][ny][2] packed observations (ame_pack_y), or NULL:
                            no scoring, sums not written                              */
    double noise[4];     /* N, row-major; zeros = moments of the mean                 */
    int32_t n_levels;    /* 0..AME_PREDICT_MAX_LEVELS                                 */
    double zsq[AME_PREDICT_MAX_LEVELS];  /* marginal thresholds on z^2                */
    double csq[AME_PREDICT_MAX_LEVELS];  /* joint thresholds on the Mahalanobis^2     */
    double* sums;        /* [S][AME_PREDICT_SUMS] fp64, or NULL                       */
    float* dense;        /* [S][i1-i0][j1-j0][5] = mean0, mean1, var0, var1, cov01
                            (noise included as given), or NULL                        */
    int32_t i0, i1, j0, j1;              /* dense block, ignored when dense == NULL   */
    double* work;        /* >= ame_predict_work_size() doubles                        */
    const uint64_t* Mt;  /* [S][n][nw] packed mask (ame_pack_mask), or NULL           */
    int32_t mask_select; /* 0: every pair; AME_MASK_OBSERVED / AME_MASK_HIDDEN: only
                            the pairs i < j whose mask bit is 0 / 1 are scored, and
                            sums[0] counts those (needs Mt and sums)                  */
} ame_predict_args;
int ame_predict(const ame_dims* dims, const ame_predict_args* args, void* stream);
/* Scratch doubles ame_predict needs (per-node feature rows and per-workgroup
 * partials; nothing of size n^2 per slice beyond 21 doubles per 64 x 64 tile). */
long long ame_predict_work_size(const ame_dims* dims);

/* ---- M-step sufficient statistics (variational EM) ---------------------------
 * Replaces nothing the reference computes: it never estimates Phi, Q, R, Sigma
 * or Psi.  With q(x_it) = N(m_it, S_it) independent across nodes and time and
 * E_it = m_it m_it' + S_it, the expected complete-data log-likelihood
 *   F = -1/2 [ Np log|R| + tr(R^-1 Rss) ] - 1/2 [ n log|S0| + tr(S0^-1 A0) ]
 *       -1/2 [ n (T-1) log|Q| + tr(Q^-1 (A11 - Phi A10' - A10 Phi' + Phi A00 Phi')) ]
 * depends on q only through
 *   A0  = sum_i E_i0                 A11 = sum_i sum_{t>=1} E_it
 *   A00 = sum_i sum_{t>=1} E_i,t-1   A10 = sum_i sum_{t>=1} m_it m_i,t-1'
 *   Rss = sum_t sum_{i<j} ( e e' + [[V0(i,j), C01(i,j)], [C01(i,j), V0(j,i)]] )
 * with e = y_ij - E[mu_ij], V0 and C01 as under ame_predict (no noise added) and
 * the upper triangle Yt[t][i][j] as the observation.  ame_mstep_stats returns
 * them per local slice; the host adds slices in global time order in fp64:
 *   state [t][0] = P_t = sum_i E_it,   state [t][1] = C_t = sum_i m_it m_i,t-1'
 *         (C_t = 0 at global slice 0; d x d row-major fp64)
 *         A0 = P_0, A11 = sum_{t>=1} P_t, A00 = sum_{t<=T-2} P_t, A10 = sum_{t>=1} C_t
 *   dyad  [t] = { pairs, Rss00, Rss11, Rss01 } of the slice
 * State pass: one workgroup per (slice, chunk of 32 nodes) streams the chunk's
 * covariances once, every product and sum in fp64, and a second kernel adds the
 * chunk partials in chunk order.  The chunk size is a constant, so a slice's
 * row has the same bits under any time sharding and any split of the slices
 * over calls.  Dyad pass: ame_predict's feature rows and five tile products
 * with an fp64 epilogue and a fixed-order reduce.  No atomics, no spin. */
typedef struct ame_mstep_args {
    const float* x;          /* [T_local][n][d] means */
    const float* cov;        /* [T_local][n][d][d] */
    const float* prev_final; /* [n][d] means of global slice t_begin-1; required iff t_begin > 0 */
    const float* Yt;         /* packed observations (ame_pack_y), or NULL: no dyad statistics */
    double* state;           /* [T_local][2][d][d] fp64: P_t, C_t, or NULL */
    double* dyad;            /* [T_local][4] fp64: pairs, Rss00, Rss11, Rss01, or NULL */
    double* work;            /* >= ame_mstep_work_size() doubles */
    const uint64_t* Mt;      /* [T_local][n][nw] packed mask (ame_pack_mask), or NULL */
    int32_t mask_select;     /* 0, AME_MASK_OBSERVED or AME_MASK_HIDDEN: the pairs the dyad
                                statistics run over (dyad[0] counts them); needs Mt */
} ame_mstep_args;
int ame_mstep_stats(const ame_dims* dims, const ame_mstep_args* args, void* stream);
/* Scratch doubles ame_mstep_stats needs (chunk partials, feature rows, tile
 * partials), -1 on bad dims. */
long long ame_mstep_work_size(const ame_dims* dims);

/* ---- exact per-node smoothing across time --------------------------------------
 * Replaces nothing the reference computes.  The sweep leaves a posterior that is
 * mean-field across nodes AND time: each covariance is the inverse of one
 * diagonal block of a node's precision.  Given the current means of the other
 * nodes, node i's exact Gaussian posterior over its whole trajectory has the
 * block-tridiagonal precision
 *   D_t = P_obs(i,t) + [t = 0] S0inv + [t > 0] Qinv + [t < T-1] PtQiP      (d x d)
 *   O   = -QiPhi                   block (t, t-1), t >= 1; O' is block (t-1, t)
 *   h_t = h_obs(i,t) = sum_{j != i} J_j' R_inv y_ij
 *   Lambda_i = blocktridiag(D, O),  mu_i = Lambda_i^-1 h,  S_i = Lambda_i^-1
 * with P_obs, h_obs as the sweep builds them (structured_mf.py:289-326) from
 * the means `x`.  ame_smooth returns, for the nodes [i0, i1), the means mu_it,
 * the marginals S_i[t,t] and the lag-one blocks X_it = S_i[t,t-1] (X_i0 = 0).
 * Three differences from the sweep's per-step inverse:
 *   - no 1e-6 jitter is added;
 *   - no "bad" masking and no naive diagonal: the smoother is the same for every
 *     variant (dims.variant is only range-checked, as in ame_predict);
 *   - P_obs is built from the symmetric part of R_inv, so Lambda_i is symmetric
 *     for an asymmetric R_inv too; h_obs keeps R_inv as given.
 * Lambda_i is positive definite whenever S0 and Q are: the factorisation does
 * not pivot.  Time sharding is not supported: t_begin = 0 and T_local = T_total.
 *
 * Two stages (kernels in csrc/ame_smooth.hip), all sums and products fp64:
 * the observation stage (per-slice Gram statistics of (U, V) and h_obs, one pass
 * over the rows [i0, i1) of Yt) and the solve stage (one workgroup per node, a
 * forward and a backward pass over t; the per-step factors live in `work`).
 * mean / cov / cross are rounded to fp32 once.  lag_sum[t] = sum_i X_it is added
 * from the fp64 values in fixed chunks of 32 nodes, chunk by chunk in node
 * order: a call with i0 = 0 starts it from zero, a call with i0 > 0 continues
 * it, so calls over consecutive node ranges (i0 a multiple of 32, in ascending
 * order on one stream) give the same bits as one call over all nodes.
 * No atomics in the sums and no waits between workgroups.
 *
 * Observed partners only (missing dyads).  With `Mt` set (the words of
 * ame_pack_mask, bit j of row i = pair {i, j} hidden) the sums of P_obs and
 * h_obs run over obs(i,t) = { j != i : bit j of row i of slice t clear }:
 *   P_obs^m(i,t) = sum_{j in obs(i,t)} J_j' sym(R_inv) J_j
 *   h_t          = sum_{j in obs(i,t)} J_j' R_inv y_ij
 * the exact posterior of node i's trajectory given the other nodes' means and
 * only the dyads it has observed.  `Yt` is then the RAW packed network (never the
 * working network of ame_fill_missing): hidden entries are not read into h.
 * The observation stage gains one kernel: per (node, slice) the Gram matrix
 * H = sum_{j hidden} w_j w_j', w = [1, U_j, V_j], gathered in ascending j in
 * chunks of four partners on fp64 MFMA (fp32 rows widened, products exact), one
 * wave per (node, slice), into `work`; the solve stage assembles
 * sym(R_inv) (.) ((G - w_i w_i') - H).  A node with every partner hidden in a
 * slice keeps the prior blocks only.  An all-zero mask gives the bits of the
 * Mt = NULL call; the bits do not depend on how the nodes are split over calls.
 * `work` then needs ame_smooth_masked_work_size doubles.
 *
 * Failure: a non-positive (or NaN) pivot does not fault; that node's outputs
 * (and lag_sum) become NaN and `fail` records it: [0] nodes that failed, [1]
 * claim word, [2] node and [3] slice of the first to report.  The caller zeroes
 * `fail` and reads it after the stream has finished. */
#define AME_SMOOTH_STAGE_OBS 1
#define AME_SMOOTH_STAGE_SOLVE 2
#define AME_SMOOTH_FAIL_WORDS 4
typedef struct ame_smooth_args {
    const float* x;          /* [T][n][d] means of ALL nodes (conditioning values) */
    const float* Yt;         /* [T][n][ny][2] packed observations (ame_pack_y) */
    const double* consts;    /* fp64 [5][d][d] */
    double rinv[4];          /* R_inv row-major, exactly as the sweep receives it */
    int32_t i0, i1;          /* nodes [i0, i1) of this call; i0 a multiple of 32 */
    int32_t stages;          /* 0 = both; AME_SMOOTH_STAGE_* bits run one stage alone (timing:
                                the solve stage then reads what an observation stage of the
                                same dims and node range left in `work`) */
    float* mean;             /* [T][n][d]    rows [i0, i1) of every slice are written */
    float* cov;              /* [T][n][d][d] */
    float* cross;            /* [T][n][d][d] X_it = S_i[t,t-1]; slice 0 is zero */
    double* lag_sum;         /* [T][d][d] fp64 */
    uint32_t* fail;          /* [AME_SMOOTH_FAIL_WORDS] */
    double* work;            /* >= ame_smooth_work_size(dims, i1 - i0) doubles */
    uint64_t work_doubles;   /* size of `work` in doubles, checked */
    const uint64_t* Mt;      /* [T][n][nw] hidden-pair words (ame_pack_mask) or NULL: sums over
                                the observed partners only; Yt is then the raw network and
                                work holds >= ame_smooth_masked_work_size doubles */
} ame_smooth_args;
int ame_smooth(const ame_dims* dims, const ame_smooth_args* args, void* stream);
/* Scratch doubles one ame_smooth call over `nodes` nodes needs: T (1+2r)^2 Gram
 * statistics + nodes T (d^2 + 2d) (h_obs, J_t^-1 g_t, J_t^-1); -1 on bad
 * dims or nodes outside [1, n]. */
long long ame_smooth_work_size(const ame_dims* dims, int nodes);
/* The same with `Mt` set: ame_smooth_work_size + nodes T (1+2r)^2 (the hidden
 * partners' Gram matrices); -1 in the same cases. */
long long ame_smooth_masked_work_size(const ame_dims* dims, int nodes);
/* Dynamic LDS bytes of the solve workgroup at latent dim r (four d x (d+1) fp64
 * matrices and six d-vectors), -1 for an r that is not compiled in. */
long long ame_smooth_lds_bytes(int r);

/* ---- dyadic covariates ---------------------------------------------------------
 * Replaces nothing the reference computes: it has no regression term.  With
 *   y_ij,t = mu_ij,t + sum_k beta_k w_k,ij,t + eps,   eps ~ N(0, R)
 * every other entry point runs unchanged on the residual network
 * Y~ = Y - sum_k beta_k W_k (ame_covar_resid), and the closed-form M-step for
 * beta needs, per slice and over the upper triangle i < j with Yt[t][i][j] and
 * Wt[k][t][i][j] as the observation 2-vectors (ame_mstep_stats' convention),
 *   G[k][a][b]    = sum_{i<j} w_k[a] e[b],    e = y~_ij - E[mu_ij]
 *   H[k][l][a][b] = sum_{i<j} w_k[a] w_l[b]   (H[k][l][a][b] == H[l][k][b][a], bit for bit)
 * ame_covar_stats: one workgroup per (slice, 64 x 64 tile of the upper triangle)
 * forms E[mu_ij] on fp32 MFMA and e in fp32, reads each covariate tile once and
 * adds the products w e' in fp64 (exact products of fp32 values); a second kernel
 * adds the tile partials in tile order.  H depends on the data alone (a caller
 * asks for it once): it has a kernel of its own over the same tiles, which sums
 * the row blocks H[k][k..p-1] one k at a time, reading plane k from memory and
 * planes l > k again from cache.  No atomics, no waits; a slice's row has the
 * same bits under any split of the slices over calls (dims.t_begin / T_total /
 * variant are only range-checked).
 * ame_covar_resid: Yt_out = Yt_raw - sum_k beta[k] Wt[k] over the packed layout;
 * per element s = 0, s += beta[k] * w_k for k ascending, y - s, every product and
 * sum rounded to fp64 on its own (no FMA), one rounding to fp32.  The pad column
 * of odd n stays what ame_pack_y wrote.  beta is p HOST doubles, read by the call. */
#define AME_MAX_COVARIATES 8
typedef struct ame_covar_args {
    const float* x;      /* [T_local][n][d] means                                   */
    const float* Yt;     /* [T_local][n][ny][2] packed residual observations        */
    const float* Wt;     /* [p][T_local][n][ny][2], each plane packed by ame_pack_y */
    int32_t p;           /* 1..AME_MAX_COVARIATES                                   */
    double* G;           /* [T_local][p][2][2] fp64, or NULL                        */
    double* H;           /* [T_local][p][p][2][2] fp64, or NULL (not both)          */
    double* work;        /* >= ame_covar_work_size() doubles                        */
    uint64_t work_doubles; /* size of `work` in doubles, checked                    */
} ame_covar_args;
int ame_covar_stats(const ame_dims* dims, const ame_covar_args* args, void* stream);
/* Scratch doubles ame_covar_stats needs (4p + 4p^2 per tile), -1 on bad dims or p. */
long long ame_covar_work_size(const ame_dims* dims, int p);
/* Yt_raw, Wt and Yt_out are 16-byte aligned; Yt_out overlaps neither Yt_raw nor
 * any plane of Wt (checked). */
int ame_covar_resid(const ame_dims* dims, const float* Yt_raw, const float* Wt, const double* beta,
                    int p, float* Yt_out, void* stream);

/* ---- missing dyads ---------------------------------------------------------------
 * Replaces nothing the reference computes: it assumes every dyad observed.  The
 * unit is the unordered pair {i, j} of one slice.  ame_sweep, ame_cov and
 * ame_elbo take no mask: they run on a working network in which the two
 * entries of a hidden pair hold each node's own-perspective mean,
 *   Yt[t][i][j] = (a_i + u_i.v_j, b_i + v_i.u_j),
 *   Yt[t][j][i] = (a_j + u_j.v_i, b_j + v_j.u_i),
 * the value J_j m_i at which y_ij drops out of node i's update
 * (structured_mf.py:289-326 treats y_ij as J_j x_i + noise).  Refilled from the
 * new means after every sweep, the damped iteration converges to the fixed
 * point of the reference's rule restricted to observed partners (up to its 1e-6
 * jitter).  The covariances stay those of the fully observed precision.
 *
 * Mask layout: Mt[T_local][n][nw] uint64, nw = ceil(n / 64); bit j & 63 of word
 * j >> 6 in row i is 1 when {i, j} is hidden at that slice; bits at j >= n and
 * at j == i are 0.
 * ame_pack_mask: M is uint8 [n][n][T_total] (non-zero = hidden; the diagonal is
 * ignored); the slices [t_begin, t_begin + T_local) are packed.  pairs[T_local]
 * (uint64) = hidden pairs i < j per slice, deg[T_local][n] (uint32) = observed
 * partners of each node, *asym (uint64) = ordered entries i != j of the packed
 * slices with M[i][j] != M[j][i] as booleans (two per disagreeing pair).  The
 * call zeroes pairs and asym itself (on the stream).  Integer counts only: the
 * same bits on every run.
 * ame_fill_missing: one workgroup per (slice, 64 x 64 tile of the upper
 * triangle).  A tile with no hidden pair returns after reading its 64 mask
 * words.  Otherwise p = u_i.v_j and q = u_j.v_i of the tile run on fp32 MFMA and
 * every hidden pair i < j gets Yt[t][i][j] = (a_i + p, b_i + q) and Yt[t][j][i]
 * = (a_j + q, b_j + p), fp32 adds; no other element of Yt is written.  Per slice
 *   corr[t][0] = sum_{hidden i<j} r_up' R_inv r_up
 *   corr[t][1] = sum_{hidden i<j} (|r_up|^2 + |r_lo|^2)
 * in fp64, r_up = Yt[t][i][j] - (a_i + b_j + p, a_j + b_i + q) and r_lo =
 * Yt[t][j][i] - (a_j + b_i + q, a_i + b_j + p) of the values just stored: what
 * ame_elbo's out[0] and out[7] accumulate at the hidden entries.  Tile partials
 * are added by a second kernel in tile order: no atomics, no waits, the same
 * bits from run to run and for any split of the slices over calls (dims.t_begin
 * / T_total / variant are only range-checked). */
typedef struct ame_fill_args {
    const float* x;      /* [T_local][n][d] means                                        */
    const uint64_t* Mt;  /* [T_local][n][nw] packed mask                                 */
    float* Yt;           /* [T_local][n][ny][2] working network, hidden entries written  */
    double rinv[4];      /* R_inv row-major                                              */
    double* corr;        /* [T_local][2] fp64                                            */
    double* work;        /* >= ame_fill_work_size() doubles                              */
} ame_fill_args;
/* Words of Mt for these dims (T_local * n * ceil(n / 64)), -1 on bad dims. */
long long ame_mask_words(const ame_dims* dims);
int ame_pack_mask(const uint8_t* M, uint64_t* Mt, const ame_dims* dims, uint64_t* pairs, uint32_t* deg,
                  uint64_t* asym, void* stream);
int ame_fill_missing(const ame_dims* dims, const ame_fill_args* args, void* stream);
/* Scratch doubles ame_fill_missing needs (2 per tile), -1 on bad dims. */
long long ame_fill_work_size(const ame_dims* dims);

/* ---- goodness of fit: network statistics and simulated networks --------------------
 * Replaces nothing the reference computes.  The posterior-predictive check of
 * AME models compares five statistics of the observed network with those of
 * networks simulated from the fit.  For one slice, y_ij = Yt[t][i][j][0] (i != j;
 * the diagonal and the pad pair of odd n are never read as data), N = n (n - 1),
 *   ybar = sum y / N,   s^2 = sum (y - ybar)^2 / (N - 1),   E = Y - ybar off the diagonal,
 *   sd_rowmean, sd_colmean   sample sd over i of row_i / (n - 1), col_i / (n - 1)
 *   dyad_dep                 correlation of (y_ij, y_ji) over ordered pairs
 *   cycle_dep, trans_dep     tr(E E E), tr(E E' E) over n (n - 1) (n - 2) s^3
 * Row i of Yt also holds y_ji = Yt[t][i][j][1]: the kernels read it there, so the
 * network must be swap-consistent (ame_pack_y's mismatch count is 0).  The three
 * entry points return raw fp64 sums; the host finishes the statistics.
 * dims.t_begin / T_total / variant are only range-checked by the first two; a
 * slice's output has the same bits under any split of the slices over calls and
 * from run to run (fixed tiles, fixed orders, no atomics, no waits).
 *
 * ame_net_moments: one streaming pass, one wave per (slice, row), every sum fp64
 * (products of fp32 values are exact):
 *   node[t][i]  = { row_i = sum_{j != i} y_ij,  col_i = sum_{j != i} y_ji }
 *   slice[t]    = { sum y_ij^2,  sum y_ij y_ji }  over ordered pairs i != j
 * (the row partials of `slice` are added by ame_tile_sum_kernel, rows in order).
 *
 * ame_net_triads: with e = y - center[t] formed in fp32 (zero on the diagonal),
 *   tri[t] = { sum_{i != j} (E E)_ij E_ji,  sum_{i != j} (E E')_ij E_ji }
 * One workgroup per (slice, 128 x 128 output tile) walks k in chunks of 32; per
 * chunk three operand panels are staged in LDS from the float2 rows (rows I
 * entry [0] = E_ik, rows J entry [1] = E_kj, rows J entry [0] = E_jk; diagonal,
 * k >= n and rows >= n zeroed, centre subtracted) and two sets of
 * v_mfma_f32_32x32x2_f32 accumulators share the A operand.  The epilogue
 * multiplies by E_ji in fp64; tile partials are added in tile order.  The n x n
 * products are never written.  `center` is an input so that a reference can
 * centre by the same fp32 number.
 *
 * ame_simulate: one network from one set of states x = [a, b, U, V],
 *   Yt_out[t][i][j] = (mu_ij + eps_0, mu_ji + eps_1),  Yt_out[t][j][i] its swap, i < j,
 *   mu_ij = a_i + b_j + u_i.v_j on fp32 MFMA (K order [a, 1, u], zero-padded to 4),
 *   eps = (l00 z0, l10 z0 + l11 z1),  lr = { l00, l10, l11 } the lower Cholesky
 *   factor of the noise covariance (zeros: the mean alone),
 * the diagonal and the pad pair written as zero.  (z0, z1) of pair i < j of global
 * slice t come from Philox4x32-10 with key = (seed low, seed high) and counter =
 * (i, j, t, sample): w0, w1 of the output give u = (float(w >> 8) + 0.5f) * 2^-24
 * (fp32 operations) and z0 = rad cos(2 pi u2), z1 = rad sin(2 pi u2),
 * rad = sqrt(-2 log u1), in fp32 with the accurate library functions; eps and
 * the sum with mu are formed in fp64 and rounded to fp32 once.  The counter
 * names the dyad: the same bits for any slice split and any t_begin that keeps
 * t_begin + tl.  Both triangles are written in row segments (the tile is
 * staged in LDS). */
typedef struct ame_moments_args {
    const float* Yt;       /* [T_local][n][ny][2] packed network                       */
    double* node;          /* [T_local][n][2] fp64: row_i, col_i                       */
    double* slice;         /* [T_local][2] fp64: sum y^2, sum y_ij y_ji                */
    double* work;          /* >= ame_net_moments_work_size() doubles                   */
    uint64_t work_doubles; /* size of `work` in doubles, checked                       */
} ame_moments_args;
typedef struct ame_triads_args {
    const float* Yt;       /* [T_local][n][ny][2] packed network, 16-byte aligned      */
    const float* center;   /* [T_local] fp32, subtracted from every off-diagonal entry */
    double* tri;           /* [T_local][2] fp64: cycle sum, transitive sum             */
    double* work;          /* >= ame_net_triads_work_size() doubles                    */
    uint64_t work_doubles; /* size of `work` in doubles, checked                       */
} ame_triads_args;
typedef struct ame_simulate_args {
    const float* x;        /* [T_local][n][d] one draw of the states (or the means)    */
    double lr[3];          /* l00, l10, l11 of the noise covariance's Cholesky factor  */
    uint64_t seed;         /* Philox key                                               */
    uint32_t sample;       /* Philox counter word 3                                    */
    float* Yt_out;         /* [T_local][n][ny][2], 16-byte aligned                     */
} ame_simulate_args;
int ame_net_moments(const ame_dims* dims, const ame_moments_args* args, void* stream);
int ame_net_triads(const ame_dims* dims, const ame_triads_args* args, void* stream);
int ame_simulate(const ame_dims* dims, const ame_simulate_args* args, void* stream);
/* Scratch doubles: 2 per (slice, row) / 2 per (slice, 128 x 128 tile); -1 on bad dims. */
long long ame_net_moments_work_size(const ame_dims* dims);
long long ame_net_triads_work_size(const ame_dims* dims);

/* ---- binary networks: probit working network and link scoring ------------------------
 * Replaces nothing the reference computes: it is Gaussian only.  The model is
 *   z_pair = (z_ij, z_ji) ~ N(mu_pair, [[1, rho], [rho, 1]]),  y = 1[z > 0],  s = 2 y - 1
 * (the noise scale is not identified).  q(z_ij) q(z_ji) are truncated normals that
 * depend on q(x) only through m = E[mu_pair] = (a_i + b_j + u_i.v_j, a_j + b_i + u_j.v_i).
 * With sd = sqrt(1 - rho^2) and kappa(x) = phi(x) / Phi(x): e = m + s kappa(s m), then
 * AME_PROBIT_STEPS times (a constant; one code path for every rho, 0 included)
 *   eta0 = m0 + rho (e1 - m1),  e0 = eta0 + s0 sd kappa(s0 eta0 / sd)
 *   eta1 = m1 + rho (e0 - m0),  e1 = eta1 + s1 sd kappa(s1 eta1 / sd)
 * and with d = e - m, x_a = s_a eta_a / sd the pair's part of the bound is
 *   l = 1/2 log(1 - rho^2) - 1/2 d' R^-1 d + sum_a [ log Phi(x_a) + 1/2 kappa(x_a)^2 ]
 * (<= the log orthant probability for any number of steps; sum_a log Phi(s_a m_a)
 * at rho = 0).  The sweep reads row i's entry as J_j x_i + noise and never takes
 * the partner's additive effects off (see missing dyads above), so the working
 * network holds each node's own-perspective mean plus the correction d:
 *   Yt[t][i][j] = (a_i + p + d0, b_i + q + d1),   Yt[t][j][i] = (a_j + q + d1, b_j + p + d0),
 *   p = u_i.v_j, q = u_j.v_i.
 * A hidden pair (Mt) gets d = 0, bit for bit what ame_fill_missing writes, and is
 * left out of every sum.
 *
 * ame_probit_fill: Bt is packed by ame_pack_mask itself from B (uint8 [n][n][T],
 * B[i][j][t] != 0 = the tie i -> j): bit j of row i is the tie i -> j.  B need not be
 * symmetric; ame_pack_mask's pairs / deg / asym of it mean nothing.  One workgroup
 * per (slice, 64 x 64 tile of the upper triangle), ame_fill_missing's tile order
 * and slice mapping, no early return: every pair i < j is written.  p and q run on
 * fp32 MFMA; everything from m on is fp64 (m0 = (double)a_i + (double)b_j +
 * (double)p, kappa(x) = sqrt(2 / pi) / erfcx(-x / sqrt 2), log Phi(x) =
 * log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 for x < 0 and log1p(-erfc(x / sqrt 2) / 2)
 * otherwise); a stored value is (float)((double)a_i + (double)p + d0), rounded
 * once.  The tile is staged in LDS and both triangles are written in row segments.
 * The diagonal, the pad column of odd n and rows >= n are never written.  Per slice
 *   stat[t][0] = observed pairs i < j          stat[t][1] = sum l
 *   stat[t][2] = sum over both entries of (y - Phi(m))^2
 *   stat[t][3] = sum over both entries of log Phi(s m)
 * tile partials added in tile order by a second kernel: no atomics, no waits, the
 * same bits from run to run, for any split of the slices over calls and for both
 * slice mappings (dims.t_begin / T_total / variant are only range-checked).
 *
 * ame_probit_score: ame_predict's feature rows and tile products with a Bernoulli
 * epilogue.  Per pair i < j selected by Mt / mask_select exactly as in ame_predict's
 * scoring, and for both entries, pi = Phi(E[mu] / sqrt(1 + V0)), the exact marginal
 * P(y = 1) under q (V0 as under ame_predict); the observation is y = Yt > 1/2 of a
 * 0 / 1 network.  Per slice, fp64, fixed-order reduce:
 *   [0] pairs   [1] sum log pi(y)   [2] sum (y - pi)^2
 *   [3] entries with (pi > 1/2) == y   [4] ties (y = 1)   [5] sum pi */
#define AME_PROBIT_STEPS 2
#define AME_PROBIT_STATS 4
#define AME_PROBIT_SUMS 6
typedef struct ame_probit_fill_args {
    const float* x;        /* [T_local][n][d] means                                     */
    const uint64_t* Bt;    /* [T_local][n][nw] packed ties (ame_pack_mask of B)         */
    const uint64_t* Mt;    /* [T_local][n][nw] packed mask of hidden pairs, or NULL     */
    double rho;            /* |rho| < 1                                                 */
    float* Yt;             /* [T_local][n][ny][2] working network, every pair written   */
    double* stat;          /* [T_local][AME_PROBIT_STATS] fp64                          */
    double* work;          /* >= ame_probit_fill_work_size() doubles                    */
    uint64_t work_doubles; /* size of `work` in doubles, checked                        */
} ame_probit_fill_args;
typedef struct ame_probit_score_args {
    const float* x;        /* [S][n][d] means              (S = dims.T_local)           */
    const float* cov;      /* [S][n][d][d] covariances                                  */
    const float* Yt;       /* [S][n][ny][2] packed 0 / 1 network (ame_pack_y)           */
    double* sums;          /* [S][AME_PROBIT_SUMS] fp64                                 */
    double* work;          /* >= ame_probit_score_work_size() doubles                   */
    uint64_t work_doubles; /* size of `work` in doubles, checked                        */
    const uint64_t* Mt;    /* [S][n][nw] packed mask (ame_pack_mask), or NULL           */
    int32_t mask_select;   /* 0, AME_MASK_OBSERVED or AME_MASK_HIDDEN (needs Mt)        */
} ame_probit_score_args;
int ame_probit_fill(const ame_dims* dims, const ame_probit_fill_args* args, void* stream);
int ame_probit_score(const ame_dims* dims, const ame_probit_score_args* args, void* stream);
/* Scratch doubles: 4 per tile / the feature rows of ame_predict plus 6 per tile;
 * -1 on bad dims. */
long long ame_probit_fill_work_size(const ame_dims* dims);
long long ame_probit_score_work_size(const ame_dims* dims);

/* ---- binary networks: ranking links (ROC / AUC histograms, top-k selection) -----------
 * Replaces nothing the reference computes.  The score of a directed entry is
 *   t = E[mu] / sqrt(1 + V0),
 * the fp64 quantity ame_probit_score forms (pi = Phi(t) is monotone in it, and t keeps
 * its resolution where pi rounds to 0 or 1); class 1 is a tie (Yt > 1/2 of a 0 / 1
 * network).  Pairs i < j are selected by Mt / mask_select exactly as in
 * ame_probit_score, and both entries of a selected pair are taken: entry 0 of pair
 * (i, j) is i -> j, entry 1 is j -> i.  The bin of an entry is, in fp64,
 *   b = floor((t + t_max) * scale)   clamped to [0, nbins - 1]   (a NaN t: bin 0),
 * an add, then a multiply (nothing a compiler can contract), with scale = nbins /
 * (2 t_max) computed once by the caller in fp64 and passed in: a host reference given
 * the same t gets the same bin.
 *
 * ame_probit_rank: hist[s][c][b] = entries of slice s and class c in bin b, uint64.
 * The call zeroes hist on its stream, every workgroup (one per slice and 64 x 64 tile)
 * counts its tile into a uint32 [2][nbins] histogram in LDS with LDS integer atomics
 * and adds the non-zero bins to hist with global 64-bit integer atomics.  Integer adds
 * do not depend on their order: the same bits from run to run, for any split of the
 * slices over calls and for both slice mappings.
 *
 * ame_probit_select: the same pass; every selected entry with b >= bin_min[s], and,
 * when tie_filter is 0 or 1, of that class (-1: both), becomes a record in slice s's
 * region records[offset[s] .. offset[s + 1]).  count[s] (zeroed by the call on its
 * stream) receives the number of entries that passed; one beyond the region's capacity
 * is counted and not written, so count[s] > offset[s + 1] - offset[s] tells the caller.
 * A workgroup reserves its run of the region with one global integer atomic, so the
 * order of the records inside a region is free; their content is not.  slice0 is added
 * to the slice index a record carries (a caller that passes its slices in chunks).
 * No floating-point atomics anywhere. */
#define AME_RANK_MAX_BINS 2048
typedef struct ame_probit_rank_args {
    const float* x;        /* [S][n][d] means              (S = dims.T_local)           */
    const float* cov;      /* [S][n][d][d] covariances                                  */
    const float* Yt;       /* [S][n][ny][2] packed 0 / 1 network (ame_pack_y)           */
    uint64_t* hist;        /* [S][2][nbins] uint64, overwritten                         */
    double* work;          /* >= ame_probit_rank_work_size() doubles                    */
    uint64_t work_doubles; /* size of `work` in doubles, checked                        */
    const uint64_t* Mt;    /* [S][n][nw] packed mask (ame_pack_mask), or NULL           */
    int32_t mask_select;   /* 0, AME_MASK_OBSERVED or AME_MASK_HIDDEN (needs Mt)        */
    int32_t nbins;         /* 1 .. AME_RANK_MAX_BINS                                    */
    double t_max;          /* > 0: the bins cover [-t_max, t_max), the end bins the rest */
    double scale;          /* nbins / (2 t_max) in fp64                                 */
} ame_probit_rank_args;
typedef struct ame_link_record {
    double t;              /* the score                                                 */
    int32_t slice;         /* slice0 + the slice's index in the call                    */
    int32_t sender, receiver;
    int32_t tie;           /* 0 / 1: the entry's class                                  */
} ame_link_record;
typedef struct ame_probit_select_args {
    const float* x;        /* as ame_probit_rank_args                                   */
    const float* cov;
    const float* Yt;
    double* work;          /* >= ame_probit_select_work_size() doubles                  */
    uint64_t work_doubles;
    const uint64_t* Mt;
    int32_t mask_select;
    int32_t nbins;
    double t_max;
    double scale;
    const int32_t* bin_min; /* [S] smallest bin taken                                   */
    int32_t tie_filter;    /* -1: both classes; 0 / 1: that class only                  */
    int32_t slice0;        /* added to the slice index of a record                      */
    const int64_t* offset; /* [S + 1] non-decreasing record offsets of the regions      */
    uint64_t* count;       /* [S] entries that passed, overwritten                      */
    ame_link_record* records; /* offset[S] records                                      */
} ame_probit_select_args;
int ame_probit_rank(const ame_dims* dims, const ame_probit_rank_args* args, void* stream);
int ame_probit_select(const ame_dims* dims, const ame_probit_select_args* args, void* stream);
/* Scratch doubles: the feature rows of ame_predict; -1 on bad dims. */
long long ame_probit_rank_work_size(const ame_dims* dims);
long long ame_probit_select_work_size(const ame_dims* dims);

/* ---- residual diagnostics: per-node sums, the distribution of m^2, the top residuals ----
 * Replaces nothing the reference computes.  The Gaussian counterpart of the link
 * ranking above: three more epilogues of ame_predict's tile kernel, on its feature
 * rows and all five products.  Pairs i < j are selected by Mt / mask_select exactly
 * as in ame_predict's scoring, and the per-pair quantities are the ones it forms, in
 * fp64, with `noise` as in ame_predict_args:
 *   e = Yt[s][i][j] - E[mu_pair],  Sigma = [[V0(i,j) + n00, C01 + n01], [., V0(j,i) + n11]],
 *   m^2 = e' Sigma^-1 e,  z^2_c = e_c^2 / Sigma_cc,  log N(y; E[mu], Sigma).
 * Entry 0 of pair (i, j) is i -> j: i sends it and j receives it; entry 1 is the reverse.
 *
 * ame_resid_nodes: node[s][i][AME_NODE_SUMS], fp64, sums over the selected pairs that
 * contain node i (a node with none gets exact zeros):
 *   [0] pairs   [1] sum log N of the pair   [2] sum m^2
 *   [3], [4] sum z^2 of the entries i sends / receives
 *   [5], [6] sum e   of the entries i sends / receives (signed: the bias)
 *   [7], [8] sum e^2 of the entries i sends / receives
 * No atomics.  In tile (I, J) a row node's 64 pairs are added in the lane and across
 * its 16-lane row, a column node's in the lane, across the four lane quarters and, in
 * wave order, across the four waves, all in a fixed order.  With nb = ceil(n / 64) a
 * node of block B gets exactly nb + 1 contributions: as a column node of tiles
 * (I' <= B, B), slot I', and as a row node of tiles (B, J >= B), slot J + 1.  Each is
 * stored once into a [S][nb + 1][n][AME_NODE_SUMS] partial in `work` (zeros where
 * nothing is selected; nothing is cleared) and a second kernel adds a node's slots in
 * slot order: the same bits from run to run, for any split of the slices over calls
 * and for both slice mappings.
 *
 * ame_resid_hist: hist[s][b] = selected pairs of slice s whose m^2 falls into bin b,
 * uint64.  The bin is, in fp64,
 *   b = floor(m2 * scale)   clamped to [0, nbins - 1],   scale = nbins / m2_max
 * computed once by the caller: one multiply, nothing a compiler can contract.  A NaN
 * m^2 goes to bin nbins - 1, NOT to bin 0 as a NaN score of ame_probit_rank does, on
 * purpose: a broken pair must surface among the most surprising ones instead of
 * hiding among the best fitted.  The mechanism is ame_probit_rank's (the call zeroes
 * hist on its stream; a uint32 histogram per workgroup in LDS, LDS integer atomics,
 * non-zero bins added with global 64-bit integer atomics).
 *
 * ame_resid_select: the same pass; every selected pair with b >= bin_min[s] becomes a
 * record in records[offset[s] .. offset[s + 1]), by ame_probit_select's reservation
 * scheme (count[s] zeroed by the call; one global integer atomic per workgroup; plain
 * stores; a pair beyond the region is counted and not written; the order inside a
 * region is free).  z_c = e_c / sqrt(Sigma_cc), signed.  No floating-point atomics
 * anywhere. */
#define AME_NODE_SUMS 9
typedef struct ame_resid_nodes_args {
    const float* x;        /* [S][n][d] means              (S = dims.T_local)           */
    const float* cov;      /* [S][n][d][d] covariances                                  */
    const float* Yt;       /* [S][n][ny][2] packed network (ame_pack_y)                 */
    double noise[4];       /* N row-major, as ame_predict_args                          */
    double* node;          /* [S][n][AME_NODE_SUMS] fp64, overwritten                   */
    double* work;          /* >= ame_resid_nodes_work_size() doubles                    */
    uint64_t work_doubles; /* size of `work` in doubles, checked                        */
    const uint64_t* Mt;    /* [S][n][nw] packed mask (ame_pack_mask), or NULL           */
    int32_t mask_select;   /* 0, AME_MASK_OBSERVED or AME_MASK_HIDDEN (needs Mt)        */
} ame_resid_nodes_args;
typedef struct ame_resid_hist_args {
    const float* x;        /* as ame_resid_nodes_args                                   */
    const float* cov;
    const float* Yt;
    double noise[4];
    uint64_t* hist;        /* [S][nbins] uint64, overwritten                            */
    double* work;          /* >= ame_resid_hist_work_size() doubles                     */
    uint64_t work_doubles;
    const uint64_t* Mt;
    int32_t mask_select;
    int32_t nbins;         /* 1 .. AME_RANK_MAX_BINS                                    */
    double scale;          /* nbins / m2_max in fp64, > 0                               */
} ame_resid_hist_args;
typedef struct ame_resid_record {
    double m2;             /* e' Sigma^-1 e                                             */
    double z0, z1;         /* e_c / sqrt(Sigma_cc), signed                              */
    int32_t slice;         /* slice0 + the slice's index in the call                    */
    int32_t i, j;          /* the pair, i < j                                           */
    int32_t pad;           /* 0                                                         */
} ame_resid_record;
typedef struct ame_resid_select_args {
    const float* x;        /* as ame_resid_hist_args                                    */
    const float* cov;
    const float* Yt;
    double noise[4];
    double* work;          /* >= ame_resid_select_work_size() doubles                   */
    uint64_t work_doubles;
    const uint64_t* Mt;
    int32_t mask_select;
    int32_t nbins;
    double scale;
    const int32_t* bin_min; /* [S] smallest bin taken                                   */
    int32_t slice0;        /* added to the slice index of a record                      */
    int32_t reserved;      /* 0                                                         */
    const int64_t* offset; /* [S + 1] non-decreasing record offsets of the regions      */
    uint64_t* count;       /* [S] pairs that passed, overwritten                        */
    ame_resid_record* records; /* offset[S] records                                     */
} ame_resid_select_args;
int ame_resid_nodes(const ame_dims* dims, const ame_resid_nodes_args* args, void* stream);
int ame_resid_hist(const ame_dims* dims, const ame_resid_hist_args* args, void* stream);
int ame_resid_select(const ame_dims* dims, const ame_resid_select_args* args, void* stream);
/* Scratch doubles: the feature rows of ame_predict, for ame_resid_nodes plus
 * T_local (nb + 1) n AME_NODE_SUMS; -1 on bad dims. */
long long ame_resid_nodes_work_size(const ame_dims* dims);
long long ame_resid_hist_work_size(const ame_dims* dims);
long long ame_resid_select_work_size(const ame_dims* dims);

/* A HIP stream whose kernels run only on compute units [first_cu, first_cu +
 * num_cus) of the current device (hipExtStreamCreateWithCUMask); *stream
 * receives the hipStream_t.  With AME_SWEEP_V2_W6 the engine puts the sweep on
 * one CU range and the ELBO kernels on the rest, so they run side by side
 * instead of queueing behind the sweep's workgroups.  Replaces nothing in the
 * reference (CPU).  ame_stream_destroy releases it. */
int ame_stream_create_cu_range(int first_cu, int num_cus, void** stream);
int ame_stream_destroy(void* stream);

/* Pin + map host memory for device access; *dev receives the device address
 * (utility; the multi-GPU path uses the peer buffers below). */
int ame_host_register(void* host, unsigned long long bytes, void** dev);
int ame_host_unregister(void* host);

/* Peer hand-off buffers of the time-sharded multi-GPU path (one process per
 * GPU, all on one node, xGMI).  ame_peer_alloc: zeroed fine-grained device
 * memory on the current device plus its IPC handle (AME_PEER_HANDLE_BYTES
 * bytes written to *handle); a neighbour process maps it with ame_peer_open and
 * writes boundary means into it with system-scope stores while the owner's
 * sweep polls it locally.  No host memory is involved.  Replaces nothing in the
 * reference (single process, structured_mf.py:240 loops over all T). */
#define AME_PEER_HANDLE_BYTES 64
int ame_peer_alloc(unsigned long long bytes, void** dev, void* handle);
int ame_peer_free(void* dev);
int ame_peer_open(const void* handle, void** dev);
int ame_peer_close(void* dev);
/* Setup-time pre-flight of one peer link (no sweep involved): ame_peer_probe
 * stores `value` into the first 8 bytes of a MAPPED neighbour buffer from a
 * one-lane kernel on the caller's device (system-scope store + release, the
 * store the sweep's hand-off uses) and waits for it; ame_peer_read_u64 copies
 * the first 8 bytes of an OWNED buffer to the host; ame_peer_clear zeroes an
 * owned buffer again (sentinels must never look like a sweep epoch).  A rank
 * pair whose probe value does not arrive is named before the first sweep
 * instead of the sweep spinning into AME_STATUS_HALO_TIMEOUT. */
int ame_peer_probe(void* peer_dev, unsigned long long value);
int ame_peer_read_u64(const void* own_dev, unsigned long long* out);
int ame_peer_clear(void* own_dev, unsigned long long bytes);

/* ---- post-fit alignment -------------------------------
 * Replaces the per-time-step loops of src/utils/alignment.py:
 * align_temporal_states (:224-321) and compute_alignment_error (:324-385).
 * x_est, x_true: (n, T, d) fp32 device arrays, d = 2 + 2r.
 * ame_align_cross: global_mode = 0 -> cross[T][2][r][r] = U_true^T U_est and
 *   V_true^T V_est per time step (alignment.py:76, called from :211-212);
 *   global_mode = 1 -> cross[2r][2r] = Mbar_true^T Mbar_est of the time-averaged
 *   (U,V) blocks (:293-303), using work (ame_align_work_size doubles).
 * The caller turns each cross block into R = U Vt (svd, det(R) < 0 -> last
 * row of Vt negated, :79-87) and passes the rotations to
 * ame_align_apply: x_out = sign-aligned x_est (additive pair by row sign,
 *   (U,V) rotated then sign-aligned per row, :275-289 / :306-319) and
 *   partials[ame_align_partials_size] = fp64 partial sums of |x_out - x_true|^2. */
long long ame_align_work_size(int n, int T, int r);
long long ame_align_cross_size(int n, int T, int r, int global_mode);
long long ame_align_partials_size(int n, int T);
int ame_align_cross(const float* x_est, const float* x_true, int n, int T, int r, int global_mode,
                    double* cross, double* work, void* stream);
int ame_align_apply(const float* x_est, const float* x_true, int n, int T, int r, int global_mode,
                    const double* rot, float* x_out, double* partials, void* stream);

/* Latent dims compiled into this library (fills up to cap entries, returns count). */
int ame_supported_r(int* out, int cap);

/* Human-readable message for the last argument error on this thread. */
const char* ame_last_error(void);

/* Build/version string (includes the offload arch). */
const char* ame_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AME_AMD_H */
