// What the stages over aggregated rows share (ngz_agg_output.hip, ngz_agg_json.hip; included by those
// units only): the ngz_agg_row offsets, the little-endian reader, the wave's staging of its tile of rows
// into LDS, and the value-sorted view of a set dictionary.  Header only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ngz/flow_aggregate.h"

namespace ngzrow {

// Rows are array-of-structures: a lane reads its own row, so in LDS a row takes row_bytes + 4: with a
// stride of an odd number of dwords the 64 lanes' reads of one field fall into 64 different banks (at
// a stride of 128 or 256 bytes they would all hit one).
constexpr uint32_t AO_PAD = 4;
constexpr uint32_t BVAL_INLINE = 32;  // bytes of a byte value a row holds (flow_aggregate.h, kkind 3)

// ngz_agg_row offsets
constexpr uint32_t R_WINDOW = 0, R_FLOW_TYPE = 4, R_PEER = 6, R_KEYP = 8, R_VALP = 12, R_COUNT = 16, R_MIN_EXPORT = 24, R_MAX_EXPORT = 28,
                   R_SYS_UP = 32, R_TAKE = 36, R_MAX_COLL = 48, R_TEMPLATES = 56, R_PORTS = 64, R_DOMAINS = 72;
static_assert(sizeof(ngz_agg_row) == 88 && offsetof(ngz_agg_row, take_id) == R_TAKE && offsetof(ngz_agg_row, domain_bits) == R_DOMAINS &&
                  offsetof(ngz_agg_row, flow_type) == R_FLOW_TYPE && offsetof(ngz_agg_row, max_sys_up_time) == R_SYS_UP, "");

__device__ __forceinline__ uint64_t ld_le(const uint8_t *p, uint32_t w) {  // p: 4-byte aligned for w >= 4
    if (w == 8) return (uint64_t)*(const uint32_t *)p | ((uint64_t)*(const uint32_t *)(p + 4) << 32);
    if (w == 4) return *(const uint32_t *)p;
    return w == 2 ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) : p[0];
}
__host__ __device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;
}

// The wave's tile of rows into its stage: 16-byte global loads over the contiguous rows (16-byte
// aligned), the lanes consecutive; row r at stage + r * (row_bytes + AO_PAD)
__device__ __forceinline__ void stage_rows(const uint8_t *rows, uint32_t row_bytes, uint32_t row0, uint32_t nt, uint8_t *stage, uint32_t lane) {
    const uint4 *g = (const uint4 *)(rows + (uint64_t)row0 * row_bytes);
    const uint32_t per_row = row_bytes / 16u, n16 = nt * per_row;
    for (uint32_t i = lane; i < n16; i += 64u) {
        const uint4 v = g[i];
        uint32_t *d = (uint32_t *)(stage + (i / per_row) * (row_bytes + AO_PAD) + (i % per_row) * 16u);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// A set dictionary (entry i <-> bit i, -1 free), ascending by masked value: bit order is not value order
struct SetEntry {
    uint32_t value, bit;
};
inline uint32_t sorted_set(const std::vector<int64_t> &dict, uint32_t mask, SetEntry *out, uint32_t cap) {
    std::vector<SetEntry> e;
    for (uint32_t i = 0; i < dict.size() && i < cap; ++i)
        if (dict[i] >= 0) e.push_back(SetEntry{(uint32_t)dict[i] & mask, i});
    std::sort(e.begin(), e.end(), [](const SetEntry &a, const SetEntry &b) { return a.value != b.value ? a.value < b.value : a.bit < b.bit; });
    std::copy(e.begin(), e.end(), out);
    return (uint32_t)e.size();
}

constexpr uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

}  // namespace ngzrow
