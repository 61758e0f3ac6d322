// The resolve pass of ngz_agg_push_enriched (include/ngz/flow_aggregate.h): the record the
// aggregation sees is the record's own fields, then the enrichment's added fields present in the
// row, then the writer id (crates/collector/src/flow/enrichment/actor.rs:141-153, :176-187), and a
// FieldRef's index counts the IE's occurrences over that list (flow/types.rs:82-100,
// aggregation/aggregator.rs:308-330).  Which added column holds occurrence i therefore depends on
// the row's presence mask.  One launch per slot in which a selected field resolves past the
// template's own columns: per row two presence words (bit k: key k is Some, bit v: aggregated field
// v is Some; own columns folded in as constants), and, for a field with several candidate columns
// or the writer id, the chosen candidate's cell in a resolved column of the aggregator's scratch.
// The reduction kernels (ngz_agg.hip) read the words and the columns; a field with one candidate
// column is read in place.
#include <hip/hip_runtime.h>

#include "ngz_agg_enrich.h"

namespace {

constexpr int RS_THREADS = 256;

__device__ __forceinline__ void copy_cell(uint8_t *dst, const uint8_t *src, uint32_t w) {
    switch (w) {
    case 16: *(uint4 *)dst = *(const uint4 *)src; break;
    case 8: *(uint2 *)dst = *(const uint2 *)src; break;
    case 4: *(uint32_t *)dst = *(const uint32_t *)src; break;
    case 2: *(uint16_t *)dst = *(const uint16_t *)src; break;
    default:
        for (uint32_t b = 0; b < w; ++b) dst[b] = src[b];
        break;
    }
}

__device__ __forceinline__ void zero_cell(uint8_t *dst, uint32_t w) {
    switch (w) {
    case 16: *(uint4 *)dst = make_uint4(0, 0, 0, 0); break;
    case 8: *(uint2 *)dst = make_uint2(0, 0); break;
    case 4: *(uint32_t *)dst = 0u; break;
    case 2: *(uint16_t *)dst = (uint16_t)0; break;
    default:
        for (uint32_t b = 0; b < w; ++b) dst[b] = 0;
        break;
    }
}

// Four consecutive rows per lane (as k_renorm and k_enrich): the mask loads as one 16-byte load and
// the presence words leave as one 16-byte store each.  Nothing is written past n_rows.
__global__ __launch_bounds__(RS_THREADS) void k_agg_resolve(const ngza::ResolvePlan P) {
    const uint32_t quads = (P.n_rows + 3) / 4;
    for (uint32_t q = blockIdx.x * RS_THREADS + threadIdx.x; q < quads; q += gridDim.x * RS_THREADS) {
        const uint32_t r0 = 4 * q;
        const uint4 mk = *(const uint4 *)(P.mask + r0);  // the mask buffer is padded to a quad
        const uint32_t m[4] = {mk.x, mk.y, mk.z, mk.w};
        uint32_t kp[4], vp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kp[j] = P.own_keys;
            vp[j] = P.own_vals;
        }
        for (uint32_t s = 0; s < P.n_sel; ++s) {
            const ngza::ResolveSel &sl = P.sel[s];  // wave-uniform: read with scalar loads
            const uint32_t kbit = sl.is_value ? 0u : 1u << sl.bit, vbit = sl.is_value ? 1u << sl.bit : 0u;
            uint32_t pick[4];  // the chosen candidate's mask bit, 0: none
            bool writer[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t have = m[j] & sl.cand;
                uint32_t c = have;  // drop the `ordinal` lowest present candidates
                for (uint32_t o = 0; o < sl.ordinal && c; ++o) c &= c - 1;
                pick[j] = c & (0u - c);
                writer[j] = !c && sl.writer_after && (uint32_t)__popc(have) == sl.ordinal;
                const bool some = c || writer[j];
                kp[j] |= some ? kbit : 0u;
                vp[j] |= some ? vbit : 0u;
            }
            if (!sl.resolved) continue;
            const uint32_t w = sl.width;
            // one candidate column at a time (a uniform pointer), the rows that chose it copy their cell
            for (uint32_t rest = sl.cand; rest; rest &= rest - 1) {
                const uint32_t cb = rest & (0u - rest);
                const uint8_t *col = P.col[__ffs(rest) - 1];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pick[j] == cb && r0 + j < P.n_rows) copy_cell(sl.resolved + (uint64_t)(r0 + j) * w, col + (uint64_t)(r0 + j) * w, w);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pick[j] || r0 + j >= P.n_rows) continue;
                uint8_t *dst = sl.resolved + (uint64_t)(r0 + j) * w;
                if (writer[j] && w == 16) *(uint4 *)dst = make_uint4(0, 0, sl.wid_len, ngza::CELL_WRITER);
                else zero_cell(dst, w);
            }
        }
        if (r0 + 3 < P.n_rows) {
            *(uint4 *)(P.kpres + r0) = make_uint4(kp[0], kp[1], kp[2], kp[3]);
            *(uint4 *)(P.vpres + r0) = make_uint4(vp[0], vp[1], vp[2], vp[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r0 + j < P.n_rows) {
                    P.kpres[r0 + j] = kp[j];
                    P.vpres[r0 + j] = vp[j];
                }
        }
    }
}

}  // namespace

int ngza::resolve_launch(const ResolvePlan &p, void *stream) {
    const uint64_t quads = ((uint64_t)p.n_rows + 3) / 4;
    if (!quads) return 0;
    // memory-bound: a bounded grid that strides the rest
    const uint32_t nb = (uint32_t)((quads + RS_THREADS - 1) / RS_THREADS < 2048 ? (quads + RS_THREADS - 1) / RS_THREADS : 2048);
    hipLaunchKernelGGL(k_agg_resolve, dim3(nb), dim3(RS_THREADS), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// ngz_agg_resolve_rows (flow_aggregate.h): the resolve pass of one selected field over a mask and
// columns given on the host
extern "C" int ngz_agg_resolve_rows(int device, const uint32_t *mask, uint32_t n_rows, const uint8_t *cols, uint32_t n_cols,
                                    uint32_t width, uint32_t cand, uint32_t ordinal, int writer_after, uint32_t writer_len,
                                    uint32_t *present, uint8_t *cells) {
    if (!mask || !present || !cells || !n_rows || n_cols > NGZ_AGG_ENRICH_MAX_COLUMNS || (n_cols && !cols) || !width ||
        width > 16 || ordinal > 255 || (n_cols < 32 && (cand >> n_cols)) || (writer_after && width != 16))
        return NGZ_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return NGZ_E_DEVICE;
    const uint64_t rows4 = ((uint64_t)n_rows + 3) & ~3ull, colb = (rows4 * width + 255) & ~255ull, wb = (rows4 * 4 + 255) & ~255ull;
    const uint64_t total = 3 * wb + (n_cols + 1) * colb;
    uint8_t *d = nullptr;
    if (hipMalloc(&d, total) != hipSuccess) return NGZ_E_NOMEM;
    int rc = NGZ_OK;
    ngza::ResolvePlan p{};
    p.mask = (const uint32_t *)d;
    p.kpres = (uint32_t *)(d + wb);
    p.vpres = (uint32_t *)(d + 2 * wb);
    p.n_rows = n_rows;
    p.n_sel = 1;
    ngza::ResolveSel &sl = p.sel[0];
    sl.cand = cand;
    sl.ordinal = (uint8_t)ordinal;
    sl.writer_after = writer_after ? 1 : 0;
    sl.width = width;
    sl.wid_len = writer_len;
    sl.resolved = d + 3 * wb + n_cols * colb;
    bool ok = hipMemset(d, 0, total) == hipSuccess &&
              hipMemcpy(d, mask, 4ull * n_rows, hipMemcpyHostToDevice) == hipSuccess;
    for (uint32_t c = 0; ok && c < n_cols; ++c) {
        p.col[c] = d + 3 * wb + c * colb;
        ok = hipMemcpy(d + 3 * wb + c * colb, cols + (uint64_t)c * n_rows * width, (uint64_t)n_rows * width, hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && ngza::resolve_launch(p, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(present, p.kpres, 4ull * n_rows, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(cells, sl.resolved, (uint64_t)n_rows * width, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) rc = NGZ_E_DEVICE;
    hipFree(d);
    return rc;
}
