// extern "C" boundary of libame_amd.so (declared in include/ame_amd.h).
// Argument validation lives here so a bad call fails loudly with a message
// instead of faulting on the GPU.
#include <stdio.h>
#include <string.h>

#include "ame_internal.h"
#include "ame_tile.h"

static thread_local char g_err[512] = "";

static int fail(const char* fmt, int a = 0, int b = 0) {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return -1;
}

static bool r_supported(int r) {
    switch (r) {
#define X(RR) \
    case RR: return true;
        AME_FOR_EACH_R(X)
#undef X
        default: return false;
    }
}

static int check_dims(const ame_dims* d) {
    if (d == nullptr) return fail("ame: dims is NULL");
    if (d->n < 2) return fail("ame: n must be >= 2 (got %d)", d->n);
    if (!r_supported(d->r)) return fail("ame: latent_dim r=%d not compiled into this library", d->r);
    if (d->T_local < 1 || d->T_total < 1) return fail("ame: bad T_local=%d T_total=%d", d->T_local, d->T_total);
    if (d->t_begin < 0 || d->t_begin + d->T_local > d->T_total)
        return fail("ame: slice range [%d, +T_local) outside T_total", d->t_begin);
    if (d->variant < AME_GOOD || d->variant > AME_NAIVE) return fail("ame: bad variant %d", d->variant);
    return 0;
}

static int launched(int rc, const char* what) {
    if (rc == 0) return 0;
    hipError_t e = hipGetLastError();
    snprintf(g_err, sizeof(g_err), "ame: %s launch failed (rc=%d, hip=%s)", what, rc,
             hipGetErrorString(e));
    return -1;
}

extern "C" {

const char* ame_last_error(void) { return g_err; }

// AME_SRC_HASH: SHA-256 prefix of every source, header and build flag that
// went into this library (ame_amd/build.py source_hash()); build() compares it
// with the tree and rebuilds on a mismatch, and tests / bench report it
#ifndef AME_SRC_HASH
#define AME_SRC_HASH "unknown"
#endif
const char* ame_version(void) { return "ame_amd 0.4 gfx950 src=" AME_SRC_HASH; }

// test hook (not in the header): the GEMV-worker partial tag (ame_common.h)
unsigned int ame_debug_gw_tag(unsigned int epoch, int m) { return ame_gw_tag(epoch, m); }
// test hooks (not in the header): ame_tile.h's tile enumeration (returns the
// tile count of n) and slice mapping, run on the host
long long ame_debug_tri_tile(int tile, int n, int* I0, int* J0) {
    ame_tri_tile_origin(tile, n, *I0, *J0);
    return ame_tri_tiles(n);
}
void ame_debug_slice_block(int b, int S, int per_slice, int* tl, int* item) {
    ame_slice_block(b, S, per_slice, *tl, *item);
}

int ame_supported_r(int* out, int cap) {
    int c = 0;
#define X(RR)                       \
    if (c < cap && out) out[c] = RR; \
    ++c;
    AME_FOR_EACH_R(X)
#undef X
    return c;
}

#define AME_MAX_CUS 1024
static int device_cus();
int ame_stream_create_cu_range(int first_cu, int num_cus, void** stream) {
    if (!stream) return fail("ame_stream_create_cu_range: NULL");
    const int cus = device_cus();
    if (first_cu < 0 || num_cus < 1 || first_cu + num_cus > cus)
        return fail("ame_stream_create_cu_range: CUs [%d, %d) outside the device", first_cu,
                    first_cu + num_cus);
    uint32_t mask[(AME_MAX_CUS + 31) / 32] = {0};
    if (cus > AME_MAX_CUS) return fail("ame_stream_create_cu_range: %d CUs", cus);
    for (int c = first_cu; c < first_cu + num_cus; ++c) mask[c / 32] |= 1u << (c % 32);
    hipStream_t s = nullptr;
    const hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)((cus + 31) / 32), mask);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_stream_create_cu_range: %s", hipGetErrorString(e));
        return -1;
    }
    *stream = (void*)s;
    return 0;
}

int ame_stream_destroy(void* stream) {
    if (!stream) return fail("ame_stream_destroy: NULL");
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? 0 : fail("ame_stream_destroy failed");
}

int ame_host_register(void* host, unsigned long long bytes, void** dev) {
    if (!host || !dev || bytes == 0) return fail("ame_host_register: bad arguments");
    hipError_t e = hipHostRegister(host, (size_t)bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_host_register: hipHostRegister: %s", hipGetErrorString(e));
        return -1;
    }
    e = hipHostGetDevicePointer(dev, host, 0);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_host_register: hipHostGetDevicePointer: %s",
                 hipGetErrorString(e));
        return -1;
    }
    return 0;
}

int ame_host_unregister(void* host) {
    if (!host) return fail("ame_host_unregister: NULL");
    return hipHostUnregister(host) == hipSuccess ? 0 : fail("ame_host_unregister failed");
}

int ame_peer_alloc(unsigned long long bytes, void** dev, void* handle) {
    if (!dev || !handle || bytes == 0) return fail("ame_peer_alloc: bad arguments");
    hipError_t e = hipExtMallocWithFlags(dev, (size_t)bytes, hipDeviceMallocFinegrained);
    if (e == hipSuccess) e = hipMemset(*dev, 0, (size_t)bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipIpcGetMemHandle((hipIpcMemHandle_t*)handle, *dev);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_peer_alloc: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

int ame_peer_free(void* dev) {
    if (!dev) return fail("ame_peer_free: NULL");
    return hipFree(dev) == hipSuccess ? 0 : fail("ame_peer_free failed");
}

int ame_peer_open(const void* handle, void** dev) {
    if (!handle || !dev) return fail("ame_peer_open: bad arguments");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    hipError_t e = hipIpcOpenMemHandle(dev, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_peer_open: hipIpcOpenMemHandle: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

int ame_peer_close(void* dev) {
    if (!dev) return fail("ame_peer_close: NULL");
    return hipIpcCloseMemHandle(dev) == hipSuccess ? 0 : fail("ame_peer_close failed");
}

__global__ void ame_peer_probe_kernel(unsigned long long* dst, unsigned long long v) {
    if (threadIdx.x == 0) {
        __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    }
}

int ame_peer_probe(void* peer_dev, unsigned long long value) {
    if (!peer_dev) return fail("ame_peer_probe: NULL");
    hipLaunchKernelGGL(ame_peer_probe_kernel, dim3(1), dim3(64), 0, 0,
                       (unsigned long long*)peer_dev, value);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_peer_probe: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

int ame_peer_read_u64(const void* own_dev, unsigned long long* out) {
    if (!own_dev || !out) return fail("ame_peer_read_u64: NULL");
    hipError_t e = hipMemcpy(out, own_dev, sizeof(*out), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_peer_read_u64: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

int ame_peer_clear(void* own_dev, unsigned long long bytes) {
    if (!own_dev || bytes == 0) return fail("ame_peer_clear: bad arguments");
    hipError_t e = hipMemset(own_dev, 0, (size_t)bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ame_peer_clear: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

static int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}

static bool v2_block_in_lds(int n, int r) { return !sweep_lds_layout(n, r, 0).m_global; }
static bool v2_single_fits(int n, int r) { return sweep_lds_layout(n, r, 1).total <= AME_LDS_MAX; }

// The concrete sweep kinds: the mode of the v2 kernel (ame_sweep.hip; modes
// >= 2 have ame_v2_nworkers(mode) GEMV-worker workgroups beside each slice's
// own) or V3_KERNEL, whether the kernel orders its slices on the device, and
// the message of a request that does not fit (n and r; worker kinds: n and
// T_local).  Every query below reads the mapping from here.
#define V3_KERNEL (-1)
struct sweep_kind_row {
    int kind, mode;
    bool orders_slices;
    const char* nofit;
};
static const sweep_kind_row g_kinds[] = {
    {AME_SWEEP_V3, V3_KERNEL, true, "ame_sweep: the v3 sweep does not fit n=%d, r=%d"},
    {AME_SWEEP_V2_LDS, 0, false, "ame_sweep: the (U,V) block of n=%d, r=%d does not fit in LDS"},
    {AME_SWEEP_V2_HBM, 1, false, "ame_sweep: the v2 sweep does not fit n=%d, r=%d"},
    {AME_SWEEP_V2_WORKERS, 2, false, "ame_sweep: GEMV workers do not fit n=%d, T_local=%d"},
    {AME_SWEEP_V2_PIPE, 3, true,
     "ame_sweep: the pipelined GEMV-worker sweep does not fit n=%d, T_local=%d"},
    {AME_SWEEP_V2_W6, 4, false, "ame_sweep: the six-worker sweep does not fit n=%d, T_local=%d"},
};

static const sweep_kind_row* kind_row(int kind) {
    for (const sweep_kind_row& k : g_kinds)
        if (k.kind == kind) return &k;
    return nullptr;
}
static bool is_concrete(int k) { return kind_row(k) != nullptr; }

static bool kind_fits(const sweep_kind_row& k, const ame_dims* d) {
    if (k.mode == V3_KERNEL) return ame_sweep3_supported(d->n, d->r);
    if (k.mode == 0) return v2_block_in_lds(d->n, d->r);
    if (k.mode == 1) return v2_single_fits(d->n, d->r);
    return ame_sweep_workers_fit(d, k.mode);
}

// Request -> concrete kernel for these dims (-1 + message when it cannot run).
// The choice depends only on the request and the shape: nothing reads the
// environment, so a caller that sized its buffers for a kind gets that kind.
static int resolve_kind(const ame_dims* d, int request) {
    const int n = d->n, r = d->r;
    switch (request) {
        case AME_SWEEP_AUTO:
            if (ame_sweep3_supported(n, r)) return AME_SWEEP_V3;
            // fall through
        case AME_SWEEP_V2_AUTO:
            if (ame_sweep_workers_fit(d, 2)) return AME_SWEEP_V2_WORKERS;
            // fall through
        case AME_SWEEP_V2_SINGLE:
            if (v2_block_in_lds(n, r)) return AME_SWEEP_V2_LDS;
            if (v2_single_fits(n, r)) return AME_SWEEP_V2_HBM;
            return fail("ame_sweep: no sweep kernel fits n=%d, r=%d", n, r);
        default: {
            const sweep_kind_row* k = kind_row(request);
            if (!k) return fail("ame_sweep: unknown sweep kind request %d", request);
            if (kind_fits(*k, d)) return k->kind;
            return fail(k->nofit, n, k->mode >= 2 ? d->T_local : r);
        }
    }
}

long long ame_sweep_lds_bytes(int n, int r, int kind) {
    if (!r_supported(r) || n < 1) return 0;
    const sweep_kind_row* k = kind_row(kind);
    if (!k) return 0;
    if (k->mode == V3_KERNEL) return ame_sweep3_supported(n, r) ? ame_sweep3_lds(n, r) : 0;
    return ame_v2_mode_lds(n, r, k->mode);
}

int ame_sweep_max_slices(int n, int r, int request) {
    if (!r_supported(r) || n < 2) return 0;
    const int cus = device_cus();
    switch (request) {
        case AME_SWEEP_AUTO:
            if (ame_sweep3_supported(n, r)) return ame_sweep3_blocks_per_cu(n, r) * cus;
            // fall through
        case AME_SWEEP_V2_AUTO:
        case AME_SWEEP_V2_SINGLE:
            if (v2_block_in_lds(n, r)) return ame_sweep_blocks_per_cu(n, r, 0) * cus;
            return v2_single_fits(n, r) ? ame_sweep_blocks_per_cu(n, r, 1) * cus : 0;
        default: {
            const sweep_kind_row* k = kind_row(request);
            if (!k) return 0;
            // kind 22 answers what the chip holds whether or not one slice's
            // launch fits (resolve_kind decides that per launch); every other
            // kind answers 0 when a one-slice launch does not fit
            ame_dims one = {n, r, 1, 0, 1, 0};
            if (k->kind != AME_SWEEP_V2_WORKERS && !kind_fits(*k, &one)) return 0;
            if (k->mode == V3_KERNEL) return ame_sweep3_blocks_per_cu(n, r) * cus;
            const int per_slice = k->mode >= 2 ? 1 + ame_v2_nworkers(k->mode) : 1;
            return ame_sweep_blocks_per_cu(n, r, k->mode) * cus / per_slice;
        }
    }
}

int ame_sweep_slice_workgroups(int kind) {
    const sweep_kind_row* k = kind_row(kind);
    if (!k) return fail("ame_sweep_slice_workgroups: %d is not a concrete sweep kind", kind);
    return k->mode >= 2 ? 1 + ame_v2_nworkers(k->mode) : 1;
}

int ame_sweep_orders_slices(int n, int r, int kind) {
    if (!r_supported(r) || n < 2) return 0;
    const sweep_kind_row* k = kind_row(kind);
    ame_dims one = {n, r, 1, 0, 1, 0};
    return k && k->orders_slices && kind_fits(*k, &one) ? 1 : 0;
}

int ame_sweep_kind(const ame_dims* dims, int request) {
    if (check_dims(dims)) return -1;
    return resolve_kind(dims, request);
}

long long ame_sweep_work_size(const ame_dims* dims, int kind) {
    if (check_dims(dims)) return -1;
    const sweep_kind_row* k = kind_row(kind);
    if (!k) return fail("ame_sweep_work_size: %d is not a concrete sweep kind", kind);
    if (k->mode == V3_KERNEL) return ame_sweep3_work_doubles(dims);
    if (k->mode == 0) return 0;
    // [T_local][n][2r] fp32 (U,V) copy
    if (k->mode == 1) return ((long long)dims->T_local * dims->n * 2 * dims->r + 1) / 2;
    // partial ring, then the precomputed right AR terms
    return ame_v2_ring_doubles(dims, k->mode) + ame_v2_arr_doubles(dims);
}

long long ame_pack_y_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return (long long)dims->T_local * dims->n * ame_ystride(dims->n) * 2;
}

int ame_pack_y(const float* Y, float* Yt, const ame_dims* dims, unsigned long long* mismatch,
               void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!Y || !Yt) return fail("ame_pack_y: NULL buffer");
    return launched(ame_pack_dispatch(Y, Yt, dims, mismatch, (hipStream_t)stream), "pack");
}

int ame_sweep(const ame_dims* dims, const ame_sweep_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->Yt || !a->x_old || !a->x_new || !a->cov || !a->hand || !a->consts || !a->status)
        return fail("ame_sweep: NULL buffer");
    if (a->epoch == 0) return fail("ame_sweep: epoch must be >= 1");
    if (dims->t_begin > 0 && !a->halo_in)
        return fail("ame_sweep: t_begin=%d > 0 needs halo_in", dims->t_begin);
    if (dims->t_begin + dims->T_local < dims->T_total && !a->next_old && !(a->wait_epoch && a->back_in))
        return fail("ame_sweep: rank does not hold T-1 and next_old is NULL");
    const int kind = resolve_kind(dims, a->kind);
    if (kind < 0) return -1;
    if (is_concrete(a->kind) && kind != a->kind)
        return fail("ame_sweep: requested kind %d resolves to %d", a->kind, kind);
    const long long need = ame_sweep_work_size(dims, kind);
    if (need > 0 && (!a->work || a->work_doubles < (unsigned long long)need))
        return fail("ame_sweep: the work buffer holds %d doubles, kind %d needs more", (int)a->work_doubles, kind);
    if (a->wait_epoch != 0 && (!ame_sweep_orders_slices(dims->n, dims->r, kind) || !a->done))
        return fail("ame_sweep: wait_epoch needs a kernel that orders slices (kind %d) and a done array", kind);
    const int maxs = kind_row(kind)->mode >= 2
                          ? dims->T_local   // resolve_kind checked that the launch co-resides
                          : ame_sweep_max_slices(dims->n, dims->r, kind);
    if (dims->T_local > maxs)
        return fail("ame_sweep: T_local=%d exceeds co-resident workgroups (%d)", dims->T_local, maxs);
    ame_sweep_args c = *a;
    c.kind = kind;
    if (kind == AME_SWEEP_V3) return launched(ame_sweep3_dispatch(dims, &c, (hipStream_t)stream), "sweep3");
    return launched(ame_sweep_dispatch(dims, &c, (hipStream_t)stream), "sweep");
}

int ame_cov(const ame_dims* dims, const ame_cov_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->cov || !a->consts || !a->cov_terms) return fail("ame_cov: NULL buffer");
    return launched(ame_cov_dispatch(dims, a, (hipStream_t)stream), "cov");
}

long long ame_elbo_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_elbo_work_doubles(dims);
}

int ame_elbo(const ame_dims* dims, const ame_elbo_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->Yt || !a->x || !a->cov_terms || !a->consts || !a->phi || !a->work || !a->out)
        return fail("ame_elbo: NULL buffer");
    if (dims->t_begin > 0 && !a->prev_final)
        return fail("ame_elbo: t_begin=%d > 0 needs prev_final", dims->t_begin);
    if (a->pairs_kernel < AME_PAIRS_AUTO || a->pairs_kernel > AME_PAIRS_V2)
        return fail("ame_elbo: bad pairs_kernel %d", a->pairs_kernel);
    return launched(ame_elbo_dispatch(dims, a, (hipStream_t)stream, 0), "elbo");
}

int ame_elbo_pairs_diag(const ame_dims* dims, const ame_elbo_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->Yt || !a->x || !a->work) return fail("ame_elbo_pairs_diag: NULL buffer");
    if (a->pairs_kernel < AME_PAIRS_AUTO || a->pairs_kernel > AME_PAIRS_V2)
        return fail("ame_elbo_pairs_diag: bad pairs_kernel %d", a->pairs_kernel);
    return launched(ame_elbo_dispatch(dims, a, (hipStream_t)stream, 1), "elbo_pairs");
}

// mask_select of ame_predict_args / ame_mstep_args: a known value, and a mask when it selects
static int check_mask_select(const char* who, int sel, const void* Mt) {
    if (sel != 0 && sel != AME_MASK_OBSERVED && sel != AME_MASK_HIDDEN) {
        snprintf(g_err, sizeof(g_err), "%s: unknown mask_select %d", who, sel);
        return -1;
    }
    if (sel != 0 && !Mt) {
        snprintf(g_err, sizeof(g_err), "%s: mask_select=%d needs the packed mask Mt (NULL)", who, sel);
        return -1;
    }
    return 0;
}

long long ame_mask_words(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_mask_words_count(dims);
}

int ame_pack_mask(const uint8_t* M, uint64_t* Mt, const ame_dims* dims, uint64_t* pairs, uint32_t* deg,
                  uint64_t* asym, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!M || !Mt || !pairs || !deg || !asym)
        return fail("ame_pack_mask: NULL buffer (M, Mt, pairs, deg, asym)");
    if (((uintptr_t)Mt | (uintptr_t)pairs | (uintptr_t)asym) & 7)
        return fail("ame_pack_mask: Mt, pairs and asym must be 8-byte aligned");
    if ((uintptr_t)deg & 3) return fail("ame_pack_mask: deg must be 4-byte aligned");
    if ((long long)dims->T_local * dims->n > 0x7FFFFFFFLL)
        return fail("ame_pack_mask: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_pack_mask_dispatch(M, (unsigned long long*)Mt, dims, (unsigned long long*)pairs, deg,
                                           (unsigned long long*)asym, (hipStream_t)stream), "pack_mask");
}

long long ame_fill_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_fill_work_doubles(dims);
}

int ame_fill_missing(const ame_dims* dims, const ame_fill_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_fill_missing: args is NULL");
    if (!a->x || !a->Mt || !a->Yt || !a->corr || !a->work)
        return fail("ame_fill_missing: NULL buffer (x, Mt, Yt, corr, work)");
    if (((uintptr_t)a->Mt | (uintptr_t)a->Yt | (uintptr_t)a->corr | (uintptr_t)a->work) & 7)
        return fail("ame_fill_missing: Mt, Yt, corr and work must be 8-byte aligned");
    if (ame_fill_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_fill_missing: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_fill_missing_dispatch(dims, a, (hipStream_t)stream), "fill_missing");
}

long long ame_predict_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_predict_work_doubles(dims);
}

int ame_predict(const ame_dims* dims, const ame_predict_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->x || !a->cov || !a->work) return fail("ame_predict: NULL buffer (x, cov, work)");
    if (a->n_levels < 0 || a->n_levels > AME_PREDICT_MAX_LEVELS)
        return fail("ame_predict: n_levels=%d outside [0, %d]", a->n_levels, AME_PREDICT_MAX_LEVELS);
    if (a->sums && !a->Yt) return fail("ame_predict: sums need the observations Yt (NULL)");
    if (int e = check_mask_select("ame_predict", a->mask_select, a->Mt)) return e;
    if (a->mask_select != 0 && !a->sums) return fail("ame_predict: mask_select=%d without sums", a->mask_select);
    if (a->dense) {
        if (a->i0 < 0 || a->i0 >= a->i1 || a->i1 > dims->n)
            return fail("ame_predict: dense rows [%d, %d) outside [0, n]", a->i0, a->i1);
        if (a->j0 < 0 || a->j0 >= a->j1 || a->j1 > dims->n)
            return fail("ame_predict: dense columns [%d, %d) outside [0, n]", a->j0, a->j1);
    }
    if (ame_predict_max_blocks(dims, a) > 0x7FFFFFFFLL)
        return fail("ame_predict: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_predict_dispatch(dims, a, (hipStream_t)stream), "predict");
}

long long ame_mstep_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_mstep_state_work_doubles(dims) + ame_mstep_dyad_work_doubles(dims);
}

int ame_mstep_stats(const ame_dims* dims, const ame_mstep_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a || !a->x || !a->cov || !a->work) return fail("ame_mstep_stats: NULL buffer (x, cov, work)");
    if (!a->state && !a->dyad) return fail("ame_mstep_stats: state and dyad are both NULL");
    if (a->dyad && !a->Yt) return fail("ame_mstep_stats: dyad statistics need the observations Yt (NULL)");
    if (int e = check_mask_select("ame_mstep_stats", a->mask_select, a->Mt)) return e;
    if (a->mask_select != 0 && !a->dyad) return fail("ame_mstep_stats: mask_select=%d without dyad", a->mask_select);
    if (a->state && dims->t_begin > 0 && !a->prev_final)
        return fail("ame_mstep_stats: t_begin=%d > 0 needs prev_final", dims->t_begin);
    if ((a->state && ame_mstep_state_blocks(dims) > 0x7FFFFFFFLL) ||
        (a->dyad && ame_mstep_dyad_blocks(dims) > 0x7FFFFFFFLL))
        return fail("ame_mstep_stats: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    if (a->state)
        if (int e = launched(ame_mstep_state_dispatch(dims, a, (hipStream_t)stream), "mstep_state")) return e;
    if (a->dyad)
        return launched(ame_mstep_dyad_dispatch(dims, a, a->work + ame_mstep_state_work_doubles(dims),
                                                (hipStream_t)stream), "mstep_dyad");
    return 0;
}

static int check_covar_p(const char* who, int p) {
    if (p < 1 || p > AME_MAX_COVARIATES) {
        snprintf(g_err, sizeof(g_err), "%s: p=%d covariates outside [1, %d]", who, p, AME_MAX_COVARIATES);
        return -1;
    }
    return 0;
}

long long ame_covar_work_size(const ame_dims* dims, int p) {
    if (check_dims(dims) || check_covar_p("ame_covar_work_size", p)) return -1;
    return ame_covar_work_doubles(dims, p);
}

int ame_covar_stats(const ame_dims* dims, const ame_covar_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_covar_stats: args is NULL");
    if (int e = check_covar_p("ame_covar_stats", a->p)) return e;
    if (!a->x || !a->Yt || !a->Wt || !a->work) return fail("ame_covar_stats: NULL buffer (x, Yt, Wt, work)");
    if (!a->G && !a->H) return fail("ame_covar_stats: G and H are both NULL");
    if ((long long)a->work_doubles < ame_covar_work_doubles(dims, a->p))
        return fail("ame_covar_stats: work holds fewer doubles than ame_covar_work_size (p=%d)", a->p);
    if (ame_covar_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_covar_stats: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_covar_stats_dispatch(dims, a, (hipStream_t)stream), "covar_stats");
}

int ame_covar_resid(const ame_dims* dims, const float* Yt_raw, const float* Wt, const double* beta, int p,
                    float* Yt_out, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (int e = check_covar_p("ame_covar_resid", p)) return e;
    if (!Yt_raw || !Wt || !beta || !Yt_out) return fail("ame_covar_resid: NULL buffer (Yt_raw, Wt, beta, Yt_out)");
    {   // the kernel reads and writes float4: 16-byte aligned, Yt_out apart from every input plane
        const uintptr_t o = (uintptr_t)Yt_out, y = (uintptr_t)Yt_raw, w = (uintptr_t)Wt;
        const uintptr_t pb = (uintptr_t)ame_covar_plane4(dims) * 16;
        if ((o | y | w) & 15) return fail("ame_covar_resid: Yt_raw, Wt and Yt_out must be 16-byte aligned");
        if (o < y + pb && y < o + pb) return fail("ame_covar_resid: Yt_out aliases Yt_raw");
        if (o < w + (uintptr_t)p * pb && w < o + pb) return fail("ame_covar_resid: Yt_out aliases Wt");
    }
    if ((ame_covar_plane4(dims) + AME_NT - 1) / AME_NT > 0x7FFFFFFFLL)
        return fail("ame_covar_resid: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_covar_resid_dispatch(dims, Yt_raw, Wt, beta, p, Yt_out, (hipStream_t)stream),
                    "covar_resid");
}

long long ame_net_moments_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_net_moments_work_doubles(dims);
}

long long ame_net_triads_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_net_triads_work_doubles(dims);
}

int ame_net_moments(const ame_dims* dims, const ame_moments_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_net_moments: args is NULL");
    if (!a->Yt || !a->node || !a->slice || !a->work)
        return fail("ame_net_moments: NULL buffer (Yt, node, slice, work)");
    if ((uintptr_t)a->Yt & 15) return fail("ame_net_moments: Yt must be 16-byte aligned");
    if (((uintptr_t)a->node | (uintptr_t)a->slice | (uintptr_t)a->work) & 7)
        return fail("ame_net_moments: node, slice and work must be 8-byte aligned");
    if ((long long)a->work_doubles < ame_net_moments_work_doubles(dims))
        return fail("ame_net_moments: work holds fewer doubles than ame_net_moments_work_size");
    if (ame_net_moments_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_net_moments: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_net_moments_dispatch(dims, a, (hipStream_t)stream), "net_moments");
}

int ame_net_triads(const ame_dims* dims, const ame_triads_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_net_triads: args is NULL");
    if (!a->Yt || !a->center || !a->tri || !a->work)
        return fail("ame_net_triads: NULL buffer (Yt, center, tri, work)");
    if ((uintptr_t)a->Yt & 15) return fail("ame_net_triads: Yt must be 16-byte aligned");
    if ((uintptr_t)a->center & 3) return fail("ame_net_triads: center must be 4-byte aligned");
    if (((uintptr_t)a->tri | (uintptr_t)a->work) & 7)
        return fail("ame_net_triads: tri and work must be 8-byte aligned");
    if ((long long)a->work_doubles < ame_net_triads_work_doubles(dims))
        return fail("ame_net_triads: work holds fewer doubles than ame_net_triads_work_size");
    if (ame_net_triads_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_net_triads: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_net_triads_dispatch(dims, a, (hipStream_t)stream), "net_triads");
}

int ame_simulate(const ame_dims* dims, const ame_simulate_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_simulate: args is NULL");
    if (!a->x || !a->Yt_out) return fail("ame_simulate: NULL buffer (x, Yt_out)");
    if ((uintptr_t)a->x & 3) return fail("ame_simulate: x must be 4-byte aligned");
    if ((uintptr_t)a->Yt_out & 15) return fail("ame_simulate: Yt_out must be 16-byte aligned");
    if (!(a->lr[0] == a->lr[0] && a->lr[1] == a->lr[1] && a->lr[2] == a->lr[2]))
        return fail("ame_simulate: lr holds a NaN");
    if (ame_simulate_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_simulate: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_simulate_dispatch(dims, a, (hipStream_t)stream), "simulate");
}

long long ame_probit_fill_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_fill_work_doubles(dims);
}

int ame_probit_fill(const ame_dims* dims, const ame_probit_fill_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_probit_fill: args is NULL");
    if (!a->x || !a->Bt || !a->Yt || !a->stat || !a->work)
        return fail("ame_probit_fill: NULL buffer (x, Bt, Yt, stat, work)");
    if (!(a->rho > -1.0 && a->rho < 1.0)) return fail("ame_probit_fill: rho must lie inside (-1, 1)");
    if ((uintptr_t)a->x & 3) return fail("ame_probit_fill: x must be 4-byte aligned");
    if (((uintptr_t)a->Bt | (uintptr_t)a->Mt | (uintptr_t)a->Yt | (uintptr_t)a->stat | (uintptr_t)a->work) & 7)
        return fail("ame_probit_fill: Bt, Mt, Yt, stat and work must be 8-byte aligned");
    if ((long long)a->work_doubles < ame_probit_fill_work_doubles(dims))
        return fail("ame_probit_fill: work holds fewer doubles than ame_probit_fill_work_size");
    if (ame_probit_fill_blocks(dims) > 0x7FFFFFFFLL)
        return fail("ame_probit_fill: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                    dims->T_local, dims->n);
    return launched(ame_probit_fill_dispatch(dims, a, (hipStream_t)stream), "probit_fill");
}

long long ame_probit_score_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_score_work_doubles(dims);
}

int ame_probit_score(const ame_dims* dims, const ame_probit_score_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_probit_score: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->sums || !a->work)
        return fail("ame_probit_score: NULL buffer (x, cov, Yt, sums, work)");
    if (int e = check_mask_select("ame_probit_score", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->sums | (uintptr_t)a->work) & 7)
        return fail("ame_probit_score: Yt, Mt, sums and work must be 8-byte aligned");
    if ((long long)a->work_doubles < ame_probit_score_work_doubles(dims))
        return fail("ame_probit_score: work holds fewer doubles than ame_probit_score_work_size");
    {
        const long long b1 = (long long)dims->T_local * dims->n, b2 = (long long)dims->T_local * ame_tri_tiles(dims->n);
        if ((b1 > b2 ? b1 : b2) > 0x7FFFFFFFLL)
            return fail("ame_probit_score: T_local=%d slices of n=%d exceed one launch; pass fewer slices",
                        dims->T_local, dims->n);
    }
    return launched(ame_probit_score_dispatch(dims, a, (hipStream_t)stream), "probit_score");
}

long long ame_probit_rank_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_rank_work_doubles(dims);
}

long long ame_probit_select_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_rank_work_doubles(dims);
}

// what ame_probit_rank and ame_probit_select share: the bin rule and the launch size
static int check_rank_common(const char* who, const ame_dims* dims, int nbins, double t_max, double scale,
                             unsigned long long work_doubles) {
    const long long b1 = (long long)dims->T_local * dims->n, b2 = (long long)dims->T_local * ame_tri_tiles(dims->n);
    if (nbins < 1 || nbins > AME_RANK_MAX_BINS)
        snprintf(g_err, sizeof(g_err), "%s: nbins=%d outside [1, %d]", who, nbins, AME_RANK_MAX_BINS);
    else if (!(t_max > 0.0) || !(t_max < 1e300))
        snprintf(g_err, sizeof(g_err), "%s: t_max must be positive and finite", who);
    else if (!(scale > 0.0) || !(scale < 1e300))
        snprintf(g_err, sizeof(g_err), "%s: scale must be positive and finite", who);
    else if ((long long)work_doubles < ame_probit_rank_work_doubles(dims))
        snprintf(g_err, sizeof(g_err), "%s: work holds fewer doubles than %s_work_size", who, who);
    else if ((b1 > b2 ? b1 : b2) > 0x7FFFFFFFLL)
        snprintf(g_err, sizeof(g_err), "%s: T_local=%d slices of n=%d exceed one launch; pass fewer slices", who,
                 dims->T_local, dims->n);
    else
        return 0;
    return -1;
}

int ame_probit_rank(const ame_dims* dims, const ame_probit_rank_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_probit_rank: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->hist || !a->work)
        return fail("ame_probit_rank: NULL buffer (x, cov, Yt, hist, work)");
    if (int e = check_mask_select("ame_probit_rank", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->hist | (uintptr_t)a->work) & 7)
        return fail("ame_probit_rank: Yt, Mt, hist and work must be 8-byte aligned");
    if (int e = check_rank_common("ame_probit_rank", dims, a->nbins, a->t_max, a->scale, a->work_doubles)) return e;
    return launched(ame_probit_rank_dispatch(dims, a, (hipStream_t)stream), "probit_rank");
}

int ame_probit_select(const ame_dims* dims, const ame_probit_select_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_probit_select: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->work || !a->bin_min || !a->offset || !a->count || !a->records)
        return fail("ame_probit_select: NULL buffer (x, cov, Yt, work, bin_min, offset, count, records)");
    if (int e = check_mask_select("ame_probit_select", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->work | (uintptr_t)a->offset | (uintptr_t)a->count |
         (uintptr_t)a->records) & 7)
        return fail("ame_probit_select: Yt, Mt, work, offset, count and records must be 8-byte aligned");
    if ((uintptr_t)a->bin_min & 3) return fail("ame_probit_select: bin_min must be 4-byte aligned");
    if (a->tie_filter < -1 || a->tie_filter > 1)
        return fail("ame_probit_select: tie_filter=%d, expected -1, 0 or 1", a->tie_filter);
    if (int e = check_rank_common("ame_probit_select", dims, a->nbins, a->t_max, a->scale, a->work_doubles))
        return e;
    return launched(ame_probit_select_dispatch(dims, a, (hipStream_t)stream), "probit_select");
}

long long ame_resid_nodes_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_resid_nodes_work_doubles(dims);
}

long long ame_resid_hist_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_rank_work_doubles(dims);
}

long long ame_resid_select_work_size(const ame_dims* dims) {
    if (check_dims(dims)) return -1;
    return ame_probit_rank_work_doubles(dims);
}

// what the three residual entry points share: the noise, the scratch and the launch size
static int check_resid_common(const char* who, const ame_dims* dims, const double* noise, long long need,
                              unsigned long long work_doubles) {
    const long long b1 = (long long)dims->T_local * dims->n, b2 = (long long)dims->T_local * ame_tri_tiles(dims->n);
    if (!(noise[0] == noise[0] && noise[1] == noise[1] && noise[2] == noise[2] && noise[3] == noise[3]))
        snprintf(g_err, sizeof(g_err), "%s: noise holds a NaN", who);
    else if ((long long)work_doubles < need)
        snprintf(g_err, sizeof(g_err), "%s: work holds fewer doubles than %s_work_size", who, who);
    else if ((b1 > b2 ? b1 : b2) > 0x7FFFFFFFLL)
        snprintf(g_err, sizeof(g_err), "%s: T_local=%d slices of n=%d exceed one launch; pass fewer slices", who,
                 dims->T_local, dims->n);
    else
        return 0;
    return -1;
}

// the bin rule of ame_resid_hist / ame_resid_select
static int check_resid_bins(const char* who, int nbins, double scale) {
    if (nbins < 1 || nbins > AME_RANK_MAX_BINS)
        snprintf(g_err, sizeof(g_err), "%s: nbins=%d outside [1, %d]", who, nbins, AME_RANK_MAX_BINS);
    else if (!(scale > 0.0) || !(scale < 1e300))
        snprintf(g_err, sizeof(g_err), "%s: scale must be positive and finite", who);
    else
        return 0;
    return -1;
}

int ame_resid_nodes(const ame_dims* dims, const ame_resid_nodes_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_resid_nodes: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->node || !a->work)
        return fail("ame_resid_nodes: NULL buffer (x, cov, Yt, node, work)");
    if (int e = check_mask_select("ame_resid_nodes", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->node | (uintptr_t)a->work) & 7)
        return fail("ame_resid_nodes: Yt, Mt, node and work must be 8-byte aligned");
    if (int e = check_resid_common("ame_resid_nodes", dims, a->noise, ame_resid_nodes_work_doubles(dims),
                                   a->work_doubles))
        return e;
    return launched(ame_resid_nodes_dispatch(dims, a, (hipStream_t)stream), "resid_nodes");
}

int ame_resid_hist(const ame_dims* dims, const ame_resid_hist_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_resid_hist: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->hist || !a->work)
        return fail("ame_resid_hist: NULL buffer (x, cov, Yt, hist, work)");
    if (int e = check_mask_select("ame_resid_hist", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->hist | (uintptr_t)a->work) & 7)
        return fail("ame_resid_hist: Yt, Mt, hist and work must be 8-byte aligned");
    if (int e = check_resid_bins("ame_resid_hist", a->nbins, a->scale)) return e;
    if (int e = check_resid_common("ame_resid_hist", dims, a->noise, ame_probit_rank_work_doubles(dims),
                                   a->work_doubles))
        return e;
    return launched(ame_resid_hist_dispatch(dims, a, (hipStream_t)stream), "resid_hist");
}

int ame_resid_select(const ame_dims* dims, const ame_resid_select_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_resid_select: args is NULL");
    if (!a->x || !a->cov || !a->Yt || !a->work || !a->bin_min || !a->offset || !a->count || !a->records)
        return fail("ame_resid_select: NULL buffer (x, cov, Yt, work, bin_min, offset, count, records)");
    if (int e = check_mask_select("ame_resid_select", a->mask_select, a->Mt)) return e;
    if (((uintptr_t)a->Yt | (uintptr_t)a->Mt | (uintptr_t)a->work | (uintptr_t)a->offset | (uintptr_t)a->count |
         (uintptr_t)a->records) & 7)
        return fail("ame_resid_select: Yt, Mt, work, offset, count and records must be 8-byte aligned");
    if ((uintptr_t)a->bin_min & 3) return fail("ame_resid_select: bin_min must be 4-byte aligned");
    if (a->slice0 < 0) return fail("ame_resid_select: slice0=%d is negative", a->slice0);
    if (int e = check_resid_bins("ame_resid_select", a->nbins, a->scale)) return e;
    if (int e = check_resid_common("ame_resid_select", dims, a->noise, ame_probit_rank_work_doubles(dims),
                                   a->work_doubles))
        return e;
    return launched(ame_resid_select_dispatch(dims, a, (hipStream_t)stream), "resid_select");
}

long long ame_smooth_work_size(const ame_dims* dims, int nodes) {
    if (check_dims(dims)) return -1;
    if (nodes < 1 || nodes > dims->n) return fail("ame_smooth_work_size: nodes=%d outside [1, n]", nodes);
    return ame_smooth_work_doubles(dims, nodes);
}

long long ame_smooth_masked_work_size(const ame_dims* dims, int nodes) {
    if (check_dims(dims)) return -1;
    if (nodes < 1 || nodes > dims->n)
        return fail("ame_smooth_masked_work_size: nodes=%d outside [1, n]", nodes);
    return ame_smooth_work_doubles(dims, nodes) + ame_smooth_hidden_doubles(dims, nodes);
}

long long ame_smooth_lds_bytes(int r) {
    if (!r_supported(r)) return fail("ame_smooth_lds_bytes: latent_dim r=%d not compiled into this library", r);
    return ame_smooth_lds_bytes_r(r);
}

int ame_smooth(const ame_dims* dims, const ame_smooth_args* a, void* stream) {
    if (int e = check_dims(dims)) return e;
    if (!a) return fail("ame_smooth: args is NULL");
    if (dims->t_begin != 0 || dims->T_local != dims->T_total)
        return fail("ame_smooth: needs every slice on this rank (t_begin=%d, T_local=%d): time "
                    "sharding is not supported", dims->t_begin, dims->T_local);
    if (!a->x || !a->Yt || !a->consts || !a->work)
        return fail("ame_smooth: NULL input buffer (x, Yt, consts, work)");
    if (!a->mean || !a->cov || !a->cross || !a->lag_sum || !a->fail)
        return fail("ame_smooth: NULL output buffer (mean, cov, cross, lag_sum, fail)");
    if (a->i0 < 0 || a->i0 >= a->i1 || a->i1 > dims->n)
        return fail("ame_smooth: nodes [%d, %d) outside [0, n]", a->i0, a->i1);
    if (a->i0 % 32 != 0) return fail("ame_smooth: i0=%d is not a multiple of 32", a->i0);
    if (a->stages < 0 || a->stages > (AME_SMOOTH_STAGE_OBS | AME_SMOOTH_STAGE_SOLVE))
        return fail("ame_smooth: bad stages %d", a->stages);
    const long long need = ame_smooth_work_doubles(dims, a->i1 - a->i0);
    if ((long long)a->work_doubles < need)
        return fail("ame_smooth: work holds fewer doubles than ame_smooth_work_size (%d nodes)",
                    a->i1 - a->i0);
    if (a->Mt) {
        if ((uintptr_t)a->Mt & 7) return fail("ame_smooth: Mt must be 8-byte aligned");
        if ((long long)a->work_doubles < need + ame_smooth_hidden_doubles(dims, a->i1 - a->i0))
            return fail("ame_smooth: with Mt set, work holds fewer doubles than "
                        "ame_smooth_masked_work_size (%d nodes)", a->i1 - a->i0);
        if (((long long)dims->T_local * (a->i1 - a->i0) + 3) / 4 > 0x7FFFFFFFLL)
            return fail("ame_smooth: T_local=%d slices of %d nodes exceed one launch; pass fewer nodes",
                        dims->T_local, a->i1 - a->i0);
    }
    if ((long long)dims->T_local * ((a->i1 - a->i0 + 31) / 32) > 0x7FFFFFFFLL)
        return fail("ame_smooth: T_local=%d slices of %d nodes exceed one launch; pass fewer nodes",
                    dims->T_local, a->i1 - a->i0);
    return launched(ame_smooth_dispatch(dims, a, (hipStream_t)stream), "smooth");
}

static int check_align(int n, int T, int r) {
    if (n < 1 || T < 1) return fail("ame_align: bad n=%d T=%d", n, T);
    if (!r_supported(r)) return fail("ame_align: latent_dim r=%d not compiled into this library", r);
    return 0;
}

long long ame_align_work_size(int n, int T, int r) {
    if (check_align(n, T, r)) return -1;
    return 2LL * n * 2 * r;
}

long long ame_align_cross_size(int n, int T, int r, int global_mode) {
    if (check_align(n, T, r)) return -1;
    return global_mode ? 4LL * r * r : 2LL * T * r * r;
}

long long ame_align_partials_size(int n, int T) {
    if (n < 1 || T < 1) return fail("ame_align: bad n=%d T=%d", n, T);
    return ame_align_partials_count(n, T);
}

int ame_align_cross(const float* x_est, const float* x_true, int n, int T, int r, int global_mode,
                    double* cross, double* work, void* stream) {
    if (int e = check_align(n, T, r)) return e;
    if (!x_est || !x_true || !cross || (global_mode && !work)) return fail("ame_align_cross: NULL buffer");
    return launched(ame_align_cross_dispatch(x_est, x_true, n, T, r, global_mode, cross, work,
                                             (hipStream_t)stream), "align_cross");
}

int ame_align_apply(const float* x_est, const float* x_true, int n, int T, int r, int global_mode,
                    const double* rot, float* x_out, double* partials, void* stream) {
    if (int e = check_align(n, T, r)) return e;
    if (!x_est || !x_true || !rot || !x_out || !partials) return fail("ame_align_apply: NULL buffer");
    return launched(ame_align_apply_dispatch(x_est, x_true, n, T, r, global_mode, rot, x_out,
                                             partials, (hipStream_t)stream), "align_apply");
}

}  // extern "C"
