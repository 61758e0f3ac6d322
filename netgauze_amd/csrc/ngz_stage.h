// What the post-decode stages share (ngz_renorm.hip, ngz_enrich.hip, ngz_options.hip; included by
// those units only): the device helpers of their set and row kernels, and the host scaffold of a
// stage handle.  Header only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ngz_host.h"

namespace ngzs {

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Block-wide add of per-lane counts: a wave reduction, one LDS atomic per wave, one global atomic
// per block and counter.  Every thread of the block calls it; acc is the block's, N words.
template <int N>
__device__ __forceinline__ void block_add(unsigned long long *acc, const uint64_t (&v)[N], unsigned long long *const (&dst)[N]) {
    if (threadIdx.x < N) acc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[i], (unsigned long long)s);
    }
    __syncthreads();
    if (threadIdx.x < N && acc[threadIdx.x]) atomicAdd(dst[threadIdx.x], acc[threadIdx.x]);
}

// Four consecutive rows of a 1-, 2- or 4-byte column (r0 a multiple of 4: one aligned vector load
// that stays inside the column, whose capacity is a multiple of 4 rows)
__device__ __forceinline__ void load4(const uint8_t *col, uint32_t w, uint32_t r0, uint32_t v[4]) {
    if (w == 4) {
        const uint4 x = *(const uint4 *)(col + 4ull * r0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else if (w == 2) {
        const uint2 x = *(const uint2 *)(col + 2ull * r0);
        v[0] = x.x & 0xFFFFu; v[1] = x.x >> 16; v[2] = x.y & 0xFFFFu; v[3] = x.y >> 16;
    } else {
        const uint32_t x = *(const uint32_t *)(col + r0);
        v[0] = x & 0xFFu; v[1] = (x >> 8) & 0xFFu; v[2] = (x >> 16) & 0xFFu; v[3] = x >> 24;
    }
}

// The set pass of a stage, one thread per data set (grid-stride): body(set index, set, its
// datagram's header) for every set that has records and lies inside the batch's tables; a set
// outside them sets err bit 0 (fail_sets below) and is skipped.
template <class Body>
__device__ __forceinline__ void for_each_set(const ngz_set_info *__restrict__ sets, uint32_t n_sets,
                                             const ngz_dgram_hdr *__restrict__ hdr, uint32_t n_dgrams, uint32_t n_slots,
                                             const uint32_t *__restrict__ slot_rows, unsigned int *__restrict__ err, Body &&body) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sets; s += gridDim.x * blockDim.x) {
        const ngz_set_info si = sets[s];
        if (!si.n) continue;
        if (si.dgram >= n_dgrams || si.slot >= n_slots || (uint64_t)si.rec0 + si.n > slot_rows[si.slot]) {
            atomicOr(err, 1u);
            continue;
        }
        body(s, si, hdr[si.dgram]);
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// What every stage handle is: the handle structs inherit it
struct Stage {
    explicit Stage(int n_events) : n_ev(n_events) {}
    Stage(const Stage &) = delete;
    Stage &operator=(const Stage &) = delete;
    ~Stage() {  // the destroy functions select the device first
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
    int device = 0;
    std::string last_error;
    bool device_ready = false;
    int n_cus = 256;
    const int n_ev;  // events the stage times with, at most 4
    hipEvent_t ev[4]{};
};

inline int fail(Stage *s, int rc, const std::string &msg) {
    if (s) s->last_error = msg;
    return rc;
}

#define NGZ_STAGE_HIP(s, x)                                                                     \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return ngzs::fail(s, NGZ_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// First use of the stage's device: the CU count its grids are sized by, and its events
inline int device_init(Stage *s) {
    if (s->device_ready) return NGZ_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || s->device < 0 || s->device >= n) return fail(s, NGZ_E_DEVICE, "no such device");
    NGZ_STAGE_HIP(s, hipSetDevice(s->device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cus = prop.multiProcessorCount;
    for (int i = 0; i < s->n_ev; ++i) NGZ_STAGE_HIP(s, hipEventCreate(&s->ev[i]));
    s->device_ready = true;
    return NGZ_OK;
}

// Pinned host memory that grows on demand and frees itself (with its stage, after the destroy
// function selected the device)
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p) hipHostFree(p);
    }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        if (p) hipHostFree(p);
        p = nullptr;
        cap = 0;
        if (hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) return -1;
        cap = n;
        return 0;
    }
};

// What a stage asks of the context before it looks at a batch
inline int check_ctx(Stage *s, const ngz_ctx *ctx) {
    if (ctx->device != s->device) return fail(s, NGZ_E_INVALID, "the context is on another device");
    if (ctx->async.pending.load()) return fail(s, NGZ_E_INVALID, "a submitted decode is pending on the context");
    return NGZ_OK;
}

inline bool slot_table_ok(const ngz_batch_out *out) { return out->n_slots <= NGZ_MAX_SLOTS && (!out->n_slots || out->slots); }

// The fields of slot s of the context's last batch into fi; their number, or NGZ_E_INVALID
inline int slot_fields(Stage *st, ngz_ctx *ctx, uint32_t s, std::vector<ngz_field_info> &fi) {
    const int nf = ngz_slot_fields(ctx, s, nullptr, 0);
    if (nf < 0) return fail(st, NGZ_E_INVALID, "ngz_slot_fields: not the context's last batch");
    fi.resize(std::max(nf, 1));
    ngz_slot_fields(ctx, s, fi.data(), (uint32_t)nf);
    return nf;
}

// err bit 0 of a set pass read back set
inline int fail_sets(Stage *s) {
    return fail(s, NGZ_E_INVALID, "a data set outside the batch's tables: `out` is not the context's last decode");
}

// Rows of a slot that are records of decoded messages, given the rows its set pass counted as not
inline uint64_t ok_rows(uint32_t slot_rows, unsigned long long bad_rows) {
    return slot_rows - std::min<uint64_t>(slot_rows, bad_rows);
}

}  // namespace ngzs
