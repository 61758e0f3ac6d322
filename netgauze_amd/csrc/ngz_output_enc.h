// The Avro writers and encoders of the output stages (ngz_output.hip over decoded columns,
// ngz_agg_output.hip over aggregated rows): a counting and a storing writer, one set of encoders
// templated on them, so that a size pass and a pack pass run the same code and the sizes are the packed
// bytes by construction, and the pack pass's LDS image and copy-out over one wave's rows, which the JSON
// and wire stages pack with too (ngz_agg_json.hip and ngz_flow_json.hip through ngz_json_dev.h,
// ngz_wire.hip).  Included by those five units only.  Device only, header only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ngz_output_plan.h"

namespace ngzenc {

struct CountW {
    static constexpr bool counting = true;
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t) { ++n; }
    __device__ __forceinline__ void bytes(const uint8_t *, uint32_t len) { n += len; }
};
struct PutW {  // nothing is stored at or past `end`
    static constexpr bool counting = false;
    uint8_t *p, *end;
    __device__ __forceinline__ void put(uint32_t b) {
        if (p < end) *p = (uint8_t)b;
        ++p;
    }
    __device__ __forceinline__ void bytes(const uint8_t *s, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) put(s[i]);
    }
};

template <class W>
__device__ __forceinline__ void put_varint(W &w, uint64_t z) {
    if constexpr (W::counting) {
        w.n += (70u - (uint32_t)__clzll((long long)(z | 1))) / 7u;
    } else {
        while (z >= 0x80) {
            w.put((uint32_t)z | 0x80u);
            z >>= 7;
        }
        w.put((uint32_t)z);
    }
}
template <class W>
__device__ __forceinline__ void put_long(W &w, int64_t v) {
    put_varint(w, ((uint64_t)v << 1) ^ (uint64_t)(v >> 63));
}
template <class W>
__device__ __forceinline__ void put_dec(W &w, uint64_t v) {
    uint8_t buf[20];
    uint32_t n = 0;
    do {
        buf[n++] = (uint8_t)('0' + v % 10);
        v /= 10;
    } while (v);
    if constexpr (W::counting) w.n += n;
    else
        while (n) w.put(buf[--n]);
}
template <class W>
__device__ __forceinline__ void put_ip4(W &w, uint32_t v) {
    for (int i = 3; i >= 0; --i) {
        put_dec(w, (v >> (8 * i)) & 255u);
        if (i) w.put('.');
    }
}
template <class W>
__device__ __forceinline__ void put_hex(W &w, uint32_t d) { w.put(d < 10 ? '0' + d : 'a' + d - 10); }
template <class W>
__device__ __forceinline__ void put_seg(W &w, uint32_t s) {  // {:x} of one 16-bit segment
    if (s >> 12) put_hex(w, s >> 12);
    if (s >> 8) put_hex(w, (s >> 8) & 15u);
    if (s >> 4) put_hex(w, (s >> 4) & 15u);
    put_hex(w, s & 15u);
}
// core::net::Ipv6Addr Display: ::ffff:a.b.c.d for a v4-mapped address, else the longest run of two
// or more zero segments (the first of equals) as "::"
template <class W>
__device__ __forceinline__ void put_ip6(W &w, const uint8_t *b) {
    uint32_t s[8];
    for (int i = 0; i < 8; ++i) s[i] = ((uint32_t)b[2 * i] << 8) | b[2 * i + 1];
    if (!(s[0] | s[1] | s[2] | s[3] | s[4]) && s[5] == 0xFFFFu) {
        const char pre[7] = {':', ':', 'f', 'f', 'f', 'f', ':'};
        for (int i = 0; i < 7; ++i) w.put(pre[i]);
        put_ip4(w, (s[6] << 16) | s[7]);
        return;
    }
    int best_s = 0, best_l = 0, cur_s = 0, cur_l = 0;
    for (int i = 0; i < 8; ++i) {
        if (s[i]) {
            cur_l = 0;
            continue;
        }
        if (!cur_l) cur_s = i;
        if (++cur_l > best_l) {
            best_s = cur_s;
            best_l = cur_l;
        }
    }
    if (best_l < 2) best_l = 0;
    for (int i = 0; i < 8; ++i) {
        if (best_l && i == best_s) {
            w.put(':');
            w.put(':');
            i += best_l - 1;
            continue;
        }
        if (i && !(best_l && i == best_s + best_l)) w.put(':');
        put_seg(w, s[i]);
    }
}
// An Avro string whose text `body` writes: its length, then the text
template <class W, class F>
__device__ __forceinline__ void put_text(W &w, F &&body) {
    CountW c;
    body(c);
    put_varint(w, (uint64_t)c.n << 1);
    if constexpr (W::counting) w.n += c.n;
    else body(w);
}

struct Cell {
    uint64_t v;        // an integer, float or IPv4 value, zero-extended
    const uint8_t *p;  // any other value's bytes
    uint32_t n;
};

__device__ __forceinline__ bool enc_numeric(uint32_t enc) {
    return enc == ngzout::ENC_INT_U || enc == ngzout::ENC_INT_S || enc == ngzout::ENC_RAW || enc == ngzout::ENC_BOOL ||
           enc == ngzout::ENC_IP4 || enc == ngzout::ENC_DEC_U || enc == ngzout::ENC_DEC_S || enc == ngzout::ENC_BOOLSTR;
}

// One value in the encoding S.enc; S: any source descriptor with `enc`, `width` (the bytes of an
// integer or float in c.v) and `aux` (ENC_MPLS_ITEM: n)
template <class W, class S>
__device__ __forceinline__ void encode_value(W &w, const S &src, const Cell &c) {
    const int shift = 64 - 8 * (int)src.width;
    switch (src.enc) {
    case ngzout::ENC_INT_U: put_long(w, (int64_t)c.v); break;
    case ngzout::ENC_INT_S: put_long(w, (int64_t)(c.v << shift) >> shift); break;
    case ngzout::ENC_RAW:
        for (uint32_t b = 0; b < src.width; ++b) w.put((uint32_t)(c.v >> (8 * b)) & 255u);
        break;
    case ngzout::ENC_BOOL: w.put(c.v ? 1 : 0); break;
    case ngzout::ENC_STR:
    case ngzout::ENC_BYTES:
        put_varint(w, (uint64_t)c.n << 1);
        w.bytes(c.p, c.n);
        break;
    case ngzout::ENC_MAC:
        put_text(w, [&](auto &t) {
            for (int i = 0; i < 6; ++i) {
                if (i) t.put(':');
                put_hex(t, c.p[i] >> 4);
                put_hex(t, c.p[i] & 15u);
            }
        });
        break;
    case ngzout::ENC_IP4: put_text(w, [&](auto &t) { put_ip4(t, (uint32_t)c.v); }); break;
    case ngzout::ENC_IP6: put_text(w, [&](auto &t) { put_ip6(t, c.p); }); break;
    case ngzout::ENC_DEC_U: put_text(w, [&](auto &t) { put_dec(t, c.v); }); break;
    case ngzout::ENC_DEC_S: {
        const int64_t sv = (int64_t)(c.v << shift) >> shift;
        put_text(w, [&](auto &t) {
            if (sv < 0) t.put('-');
            put_dec(t, sv < 0 ? 0ull - (uint64_t)sv : (uint64_t)sv);
        });
        break;
    }
    case ngzout::ENC_BOOLSTR:
        put_text(w, [&](auto &t) {
            const char *s = c.v ? "true" : "false";
            for (uint32_t i = 0; i < (c.v ? 4u : 5u); ++i) t.put(s[i]);
        });
        break;
    case ngzout::ENC_MPLS_ITEM:
        put_text(w, [&](auto &t) {
            put_dec(t, src.aux);
            t.put('-');
            put_dec(t, ((uint32_t)c.p[0] << 16) | ((uint32_t)c.p[1] << 8) | c.p[2]);
        });
        break;
    }
}

// The wave's image of `len` bytes at img + mis out to dst, mis = dst mod 16: the ragged head and the tail by
// bytes (at most 15 each, a lane a byte), the 16-byte aligned middle in 16-byte stores
__device__ __forceinline__ void copy_out(const uint8_t *img, uint32_t mis, uint8_t *dst, uint32_t len, uint32_t lane) {
    const uint32_t head = min(len, (16u - mis) & 15u);
    const uint32_t n16 = (len - head) / 16u, tail0 = head + 16u * n16;
    if (lane < head) dst[lane] = img[mis + lane];
    if (lane < len - tail0) dst[tail0 + lane] = img[mis + tail0 + lane];
    for (uint32_t i = lane; i < n16; i += 64u) *(uint4 *)(dst + head + 16u * i) = *(const uint4 *)(img + mis + head + 16u * i);
}

// The pack pass over one wave's tile of at most 64 consecutive rows.  Lane l < nt owns row l, whose datum
// fills out[base + rel0, base + rel1) (the scanned offsets, relative to the tile's first).  The wave encodes
// the rows [g0, g1) whose bytes fit the image together into `img`, IMG + 16 bytes of LDS laid out like
// their output range (image byte i of a group lies at img[mis + i], mis the group's first output address
// mod 16: a 16-byte aligned run of the image is a 16-byte aligned run of the output), and copies it out
// in 16-byte stores; a row longer than the image goes straight out.  encode(w) writes the calling lane's
// row into the writer w: a WImg{begin, end} over the image, a WOut{begin, end} over the output for a row
// that goes straight out.  Every lane of the wave calls it; nothing is written at or past out + total.
template <uint32_t IMG, class WImg = PutW, class WOut = PutW, class Encode>
__device__ __forceinline__ void pack_tile(uint32_t lane, uint32_t nt, unsigned long long base, uint32_t rel0, uint32_t rel1, uint8_t *out,
                                          unsigned long long total, uint8_t *img, Encode &&encode) {
    const unsigned long long o0 = base + rel0, o1 = base + rel1;
    for (uint32_t g0 = 0; g0 < nt;) {
        const uint32_t gb = __shfl(rel0, g0, 64);
        const bool fits = lane >= g0 && lane < nt && rel1 - gb <= IMG;
        const unsigned long long rest = ~__ballot(fits) >> g0;
        const uint32_t cnt = rest ? (uint32_t)__ffsll((long long)rest) - 1u : 64u - g0;
        if (!cnt) {  // row g0 alone is longer than the image
            if (lane == g0 && o1 <= total) {
                WOut w{out + o0, out + o1};
                encode(w);
            }
            ++g0;
            continue;
        }
        const uint32_t g1 = g0 + cnt;
        const uint32_t len = (uint32_t)__shfl(rel1, g1 - 1, 64) - gb;
        uint8_t *const dst = out + base + gb;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
        if (lane >= g0 && lane < g1 && rel1 > rel0) {
            WImg w{img + mis + (rel0 - gb), img + mis + (rel1 - gb)};
            encode(w);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        if (base + gb + len <= total) copy_out(img, mis, dst, len, lane);
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        g0 = g1;
    }
}

}  // namespace ngzenc
