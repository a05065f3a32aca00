// Entry points between the library's translation units: each kernel file
// defines its dispatch and sizing functions, ame_capi.hip (the extern "C"
// boundary) calls them, and ame_parts.hip routes the r-dependent ones of the
// split build.  Declared once, here; every file that defines or calls one
// includes this header, so a signature that drifts fails to compile.
#pragma once
#include "ame_common.h"

// r-dependent entry points of the split sources (build.py SPLIT): NAME in a
// one-part build; in the split build part p defines NAME_p<p> (AME_PFN,
// ame_common.h) and ame_parts.hip defines NAME, which routes by r.
#define AME_SPLIT_FN(RET, NAME, ARGS) \
    RET NAME ARGS;                    \
    RET NAME##_p0 ARGS;               \
    RET NAME##_p1 ARGS;               \
    RET NAME##_p2 ARGS;

// ame_sweep.hip (v2, kinds 20-24)
AME_SPLIT_FN(int, ame_sweep_dispatch, (const ame_dims*, const ame_sweep_args*, hipStream_t))
AME_SPLIT_FN(int, ame_sweep_blocks_per_cu, (int n, int r, int mode))
AME_SPLIT_FN(int, ame_sweep_workers_fit, (const ame_dims*, int mode))   // mode 2: kind 22, 3: kind 23, 4: kind 24
// ame_sweep3.hip (v3, kind 3)
AME_SPLIT_FN(int, ame_sweep3_dispatch, (const ame_dims*, const ame_sweep_args*, hipStream_t))
AME_SPLIT_FN(int, ame_sweep3_supported, (int n, int r))
AME_SPLIT_FN(int, ame_sweep3_blocks_per_cu, (int n, int r))
AME_SPLIT_FN(int, ame_sweep3_lds, (int n, int r))
long long ame_sweep3_work_doubles(const ame_dims*);
// ame_cov.hip
int ame_cov_dispatch(const ame_dims*, const ame_cov_args*, hipStream_t);
// ame_elbo.hip
AME_SPLIT_FN(int, ame_elbo_dispatch, (const ame_dims*, const ame_elbo_args*, hipStream_t, int pairs_only))
long long ame_elbo_work_doubles(const ame_dims*);
int ame_pack_dispatch(const float* Y, float* Yt, const ame_dims*, unsigned long long* mismatch, hipStream_t);
// ame_align.hip
int ame_align_cross_dispatch(const float* est, const float* tru, int n, int T, int r, int global_mode,
                             double* cross, double* work, hipStream_t);
int ame_align_apply_dispatch(const float* est, const float* tru, int n, int T, int r, int global_mode,
                             const double* rot, float* out, double* partials, hipStream_t);
long long ame_align_partials_count(int n, int T);
// ame_predict.hip (prediction, and the M-step's dyad statistics)
AME_SPLIT_FN(int, ame_predict_dispatch, (const ame_dims*, const ame_predict_args*, hipStream_t))
long long ame_predict_work_doubles(const ame_dims*);
long long ame_predict_max_blocks(const ame_dims*, const ame_predict_args*);
AME_SPLIT_FN(int, ame_mstep_dyad_dispatch, (const ame_dims*, const ame_mstep_args*, double* work, hipStream_t))
long long ame_mstep_dyad_work_doubles(const ame_dims*);
long long ame_mstep_dyad_blocks(const ame_dims*);
// ame_mstep.hip
int ame_mstep_state_dispatch(const ame_dims*, const ame_mstep_args*, hipStream_t);
long long ame_mstep_state_work_doubles(const ame_dims*);
long long ame_mstep_state_blocks(const ame_dims*);
// ame_smooth.hip
int ame_smooth_dispatch(const ame_dims*, const ame_smooth_args*, hipStream_t);
long long ame_smooth_work_doubles(const ame_dims*, int nodes);
long long ame_smooth_hidden_doubles(const ame_dims*, int nodes);
long long ame_smooth_lds_bytes_r(int r);
// ame_covar.hip
int ame_covar_stats_dispatch(const ame_dims*, const ame_covar_args*, hipStream_t);
int ame_covar_resid_dispatch(const ame_dims*, const float* Yraw, const float* Wt, const double* beta, int p,
                             float* out, hipStream_t);
long long ame_covar_work_doubles(const ame_dims*, int p);
long long ame_covar_blocks(const ame_dims*);
long long ame_covar_plane4(const ame_dims*);
// ame_missing.hip
int ame_pack_mask_dispatch(const uint8_t* M, unsigned long long* Mt, const ame_dims*, unsigned long long* pairs,
                           uint32_t* deg, unsigned long long* asym, hipStream_t);
int ame_fill_missing_dispatch(const ame_dims*, const ame_fill_args*, hipStream_t);
long long ame_mask_words_count(const ame_dims*);
long long ame_fill_work_doubles(const ame_dims*);
long long ame_fill_blocks(const ame_dims*);
// ame_gof.hip
int ame_net_moments_dispatch(const ame_dims*, const ame_moments_args*, hipStream_t);
int ame_net_triads_dispatch(const ame_dims*, const ame_triads_args*, hipStream_t);
int ame_simulate_dispatch(const ame_dims*, const ame_simulate_args*, hipStream_t);
long long ame_net_moments_work_doubles(const ame_dims*);
long long ame_net_moments_blocks(const ame_dims*);
long long ame_net_triads_work_doubles(const ame_dims*);
long long ame_net_triads_blocks(const ame_dims*);
long long ame_simulate_blocks(const ame_dims*);
// ame_binary.hip
int ame_probit_fill_dispatch(const ame_dims*, const ame_probit_fill_args*, hipStream_t);
long long ame_probit_fill_work_doubles(const ame_dims*);
long long ame_probit_fill_blocks(const ame_dims*);
// ame_predict.hip (MODE 3: Bernoulli scoring)
AME_SPLIT_FN(int, ame_probit_score_dispatch, (const ame_dims*, const ame_probit_score_args*, hipStream_t))
long long ame_probit_score_work_doubles(const ame_dims*);
// ame_predict.hip (MODE 4, 5: score histograms and top-scoring records)
AME_SPLIT_FN(int, ame_probit_rank_dispatch, (const ame_dims*, const ame_probit_rank_args*, hipStream_t))
AME_SPLIT_FN(int, ame_probit_select_dispatch, (const ame_dims*, const ame_probit_select_args*, hipStream_t))
long long ame_probit_rank_work_doubles(const ame_dims*);
// ame_predict.hip (MODE 6 - 8: per-node residual sums, the histogram of m^2, the top residuals)
AME_SPLIT_FN(int, ame_resid_nodes_dispatch, (const ame_dims*, const ame_resid_nodes_args*, hipStream_t))
AME_SPLIT_FN(int, ame_resid_hist_dispatch, (const ame_dims*, const ame_resid_hist_args*, hipStream_t))
AME_SPLIT_FN(int, ame_resid_select_dispatch, (const ame_dims*, const ame_resid_select_args*, hipStream_t))
long long ame_resid_nodes_work_doubles(const ame_dims*);

#undef AME_SPLIT_FN
