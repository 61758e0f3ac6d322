// The serde-JSON writers and value renderers of the device JSON stages (ngz_agg_json.hip over aggregated
// rows, ngz_flow_json.hip over decoded columns; included by those units only): a counting writer, a byte
// writer and the accumulating dword writer, one set of renderers templated on them, so that a size pass
// and a pack pass run the same code and the sizes are the packed bytes by construction; the constant-text
// pool and the value-sorted sub-registry name table the host side of both units builds.  Header only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "ngz_agg_rows.h"
#include "ngz_host.h"
#include "ngz_output_enc.h"
#include "ngz_subreg.h"

namespace ngzjson {

using ngzrow::floor_div;

struct JText {  // constant text in the pool: off a multiple of four, zero padded to a whole dword
    uint32_t off, len;
};
struct JName {
    uint32_t value;
    JText text;
};
struct JSub {  // a sub-registry IE's variants in the name table, ascending by value, and a nested one's groups
    uint32_t sub0, sub_n, grp0, grp_n;
};

// ---------------------------------------------------------------------------------------------
// writers: put(byte), push(up to four characters, the first in the low byte, the rest zero),
// text(constant pool text), finish()
// ---------------------------------------------------------------------------------------------
struct JCount {
    static constexpr bool counting = true;
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t) { ++n; }
    __device__ __forceinline__ void push(uint32_t, uint32_t k) { n += k; }
    __device__ __forceinline__ void text(const uint32_t *, uint32_t len) { n += len; }
    __device__ __forceinline__ void finish() {}
};
struct JByte {  // the plain byte writer; nothing is stored at or past `end`
    static constexpr bool counting = false;
    uint8_t *p, *end;
    __host__ __device__ __forceinline__ void put(uint32_t b) {
        if (p < end) *p = (uint8_t)b;
        ++p;
    }
    __host__ __device__ __forceinline__ void push(uint32_t d, uint32_t k) {
        for (uint32_t i = 0; i < k; ++i) put(d >> (8u * i));
    }
    __host__ __device__ __forceinline__ void text(const uint32_t *s, uint32_t len) {
        const uint8_t *b = (const uint8_t *)s;
        for (uint32_t i = 0; i < len; ++i) put(b[i]);
    }
    __host__ __device__ __forceinline__ void finish() {}
};
// The accumulating writer over [begin, end) of an LDS image.  acc holds `fill` < 4 pending bytes in its
// low end; whatever comes in is shifted up by 8 * fill and ORed in, and each time four bytes are
// there the low dword goes to *p, a dword-aligned address.  A row that starts at byte phase h of a dword
// starts with fill = h: the dword's first h bytes are its neighbour's, so that one dword (`head`) and
// the last partial one (finish) are stored by bytes.  Nothing is stored at or past `end`.
struct JAcc {
    static constexpr bool counting = false;
    uint64_t acc;
    uint32_t fill, head;
    uint32_t *p, *lim;
    uint8_t *end;
    __device__ __forceinline__ JAcc(uint8_t *begin, uint8_t *e) : acc(0), end(e) {
        head = fill = (uint32_t)(uintptr_t)begin & 3u;
        p = (uint32_t *)(begin - fill);
        lim = (uint32_t *)(e - ((uint32_t)(uintptr_t)e & 3u));
    }
    __device__ __forceinline__ void emit(uint32_t d) {
        if (p < lim) {
            if (head) {
                uint8_t *b = (uint8_t *)p;
                for (uint32_t i = head; i < 4u; ++i) b[i] = (uint8_t)(d >> (8u * i));
            } else {
                *p = d;
            }
        }
        head = 0;
        ++p;
    }
    __device__ __forceinline__ void push(uint32_t d, uint32_t k) {
        acc |= (uint64_t)d << (8u * fill);
        fill += k;
        if (fill >= 4u) {
            emit((uint32_t)acc);
            acc >>= 32;
            fill -= 4u;
        }
    }
    __device__ __forceinline__ void put(uint32_t b) { push(b & 255u, 1); }
    __device__ __forceinline__ void text(const uint32_t *s, uint32_t len) {  // a dword: one shift, one store
        const uint32_t nd = len >> 2;
        for (uint32_t i = 0; i < nd; ++i) {
            acc |= (uint64_t)s[i] << (8u * fill);
            emit((uint32_t)acc);
            acc >>= 32;
        }
        if (len & 3u) push(s[nd], len & 3u);
    }
    __device__ __forceinline__ void finish() {
        uint8_t *b = (uint8_t *)p;
        for (uint32_t i = head; i < fill; ++i)
            if (b + i < end) b[i] = (uint8_t)(acc >> (8u * i));
    }
};
struct JHost {  // the head texts, on the host
    static constexpr bool counting = false;
    std::string s;
    void push(uint32_t d, uint32_t k) {
        for (uint32_t i = 0; i < k; ++i) s += (char)(d >> (8u * i));
    }
};

// ---------------------------------------------------------------------------------------------
// renderers, the counterparts of put_u64 / put_datetime / put_str / put_list / put_subreg of ngz_json.cpp
// ---------------------------------------------------------------------------------------------
// Decimal text of v, zero padded to min_digits.  The digits come out last first; each is shifted in
// below the ones before it, so the finished text lies in c0, c1, c2 first character lowest: the order
// push wants.
template <class W>
__host__ __device__ __forceinline__ void put_dec(W &w, uint64_t v, uint32_t min_digits = 1) {
    uint64_t c0 = 0, c1 = 0;
    uint32_t c2 = 0, n = 0;
    if (!(v >> 32)) {
        uint32_t x = (uint32_t)v;
        do {
            if constexpr (!W::counting) {
                c1 = (c1 << 8) | (c0 >> 56);
                c0 = (c0 << 8) | ('0' + x % 10u);
            }
            x /= 10u;
            ++n;
        } while (x || n < min_digits);
    } else {
        do {
            if constexpr (!W::counting) {
                c2 = (c2 << 8) | (uint32_t)(c1 >> 56);
                c1 = (c1 << 8) | (c0 >> 56);
                c0 = (c0 << 8) | ('0' + (uint32_t)(v % 10u));
            }
            v /= 10u;
            ++n;
        } while (v || n < min_digits);
    }
    if constexpr (W::counting) {
        w.n += n;
    } else {
        while (n) {
            const uint32_t k = n < 4u ? n : 4u;
            w.push((uint32_t)c0, k);
            c0 = (c0 >> 32) | (c1 << 32);
            c1 = (c1 >> 32) | ((uint64_t)c2 << 32);
            c2 = 0;
            n -= k;
        }
    }
}
__host__ __device__ __forceinline__ uint32_t two(uint32_t x) { return ('0' + x / 10u) | (('0' + x % 10u) << 8); }

// chrono's DateTime<Utc> serde text: RFC 3339, 'Z', the fraction in 0 / 3 / 6 / 9 digits, nanos >= 10^9
// as second 60, a year outside 0..9999 signed
template <class W>
__host__ __device__ __forceinline__ void put_datetime(W &w, int64_t secs, uint32_t nanos) {
    const int64_t days = floor_div(secs, 86400);
    const uint32_t sod = (uint32_t)(secs - days * 86400);
    const int64_t z = days + 719468;
    const int64_t era = floor_div(z, 146097);
    const uint32_t doe = (uint32_t)(z - era * 146097);
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    int64_t y = (int64_t)yoe + era * 400;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const uint32_t mp = (5u * doy + 2u) / 153u;
    const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
    const uint32_t m = mp < 10u ? mp + 3u : mp - 9u;
    if (m <= 2u) ++y;
    uint32_t ss = sod % 60u;
    if (nanos >= 1000000000u) {
        ss += 1u;
        nanos -= 1000000000u;
    }
    const uint32_t hh = sod / 3600u, mi = sod % 3600u / 60u;
    if (y >= 0 && y <= 9999) {
        w.push('"', 1);
        put_dec(w, (uint64_t)y, 4);
    } else {
        w.push('"' | ((y < 0 ? '-' : '+') << 8), 2);
        put_dec(w, y < 0 ? 0ull - (uint64_t)y : (uint64_t)y, 4);
    }
    w.push('-' | (two(m) << 8) | ('-' << 24), 4);
    w.push(two(d) | ('T' << 16) | (('0' + hh / 10u) << 24), 4);
    w.push(('0' + hh % 10u) | (':' << 8) | (two(mi) << 16), 4);
    w.push(':' | (two(ss) << 8), 3);
    if (nanos) {
        w.push('.', 1);
        if (nanos % 1000000u == 0) put_dec(w, nanos / 1000000u, 3);
        else if (nanos % 1000u == 0) put_dec(w, nanos / 1000u, 6);
        else put_dec(w, nanos, 9);
    }
    w.push('Z' | ('"' << 8), 2);
}

template <class W>
__device__ __forceinline__ void put_bool(W &w, bool b) {
    if (b) {
        w.push('t' | ('r' << 8) | ('u' << 16) | ('e' << 24), 4);
    } else {
        w.push('f' | ('a' << 8) | ('l' << 16) | ('s' << 24), 4);
        w.push('e', 1);
    }
}

// [1,2,3]: an item and the comma or bracket after it are at most four characters, one push
template <class W>
__device__ __forceinline__ void put_list(W &w, const uint8_t *p, uint32_t n) {
    if (!n) {
        w.push('[' | (']' << 8), 2);
        return;
    }
    w.push('[', 1);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = p[i], term = i + 1 == n ? ']' : ',';
        if (b >= 100u) w.push(('0' + b / 100u) | (('0' + b / 10u % 10u) << 8) | (('0' + b % 10u) << 16) | (term << 24), 4);
        else if (b >= 10u) w.push(('0' + b / 10u) | (('0' + b % 10u) << 8) | (term << 16), 3);
        else w.push(('0' + b) | (term << 8), 2);
    }
}

// serde_json's string: '"', '\\' and the C0 controls escaped, everything else as it is
template <class W>
__device__ __forceinline__ void put_str(W &w, const uint8_t *s, uint32_t n) {
    w.push('"', 1);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = s[i];
        if (c >= 0x20u && c != '"' && c != '\\') {
            w.push(c, 1);
            continue;
        }
        uint32_t e = 0;
        switch (c) {
        case '"': e = '"'; break;
        case '\\': e = '\\'; break;
        case '\b': e = 'b'; break;
        case '\f': e = 'f'; break;
        case '\n': e = 'n'; break;
        case '\r': e = 'r'; break;
        case '\t': e = 't'; break;
        }
        if (e) {
            w.push('\\' | (e << 8), 2);
        } else {
            const uint32_t hi = c >> 4, lo = c & 15u;
            w.push('\\' | ('u' << 8) | ('0' << 16) | ('0' << 24), 4);
            w.push(('0' + hi) | ((lo < 10u ? '0' + lo : 'a' + lo - 10u) << 8), 2);  // c < 0x20: hi is 0 or 1
        }
    }
    w.push('"', 1);
}

// TCPHeaderFlags: its eight named booleans
template <class W>
__device__ __forceinline__ void put_tcp(W &w, uint32_t bits) {
    constexpr uint32_t nm[8] = {'F' | ('I' << 8) | ('N' << 16), 'S' | ('Y' << 8) | ('N' << 16), 'R' | ('S' << 8) | ('T' << 16),
                                'P' | ('S' << 8) | ('H' << 16), 'A' | ('C' << 8) | ('K' << 16), 'U' | ('R' << 8) | ('G' << 16),
                                'E' | ('C' << 8) | ('E' << 16), 'C' | ('W' << 8) | ('R' << 16)};
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        w.push((i ? ',' : '{') | ('"' << 8), 2);
        w.push(nm[i] | ('"' << 24), 4);
        w.push(':', 1);
        put_bool(w, (bits >> i) & 1u);
    }
    w.push('}', 1);
}

// "a.b.c.d" of the address in v, and core::net::Ipv6Addr's Display text, quoted
template <class W>
__device__ __forceinline__ void put_ip4_str(W &w, uint64_t v) {
    w.push('"', 1);
    for (int i = 3; i >= 0; --i) {
        put_dec(w, (v >> (8 * i)) & 255u);
        if (i) w.push('.', 1);
    }
    w.push('"', 1);
}
template <class W>
__device__ __forceinline__ void put_ip6_str(W &w, const uint8_t *p) {
    w.push('"', 1);
    ngzenc::put_ip6(w, p);
    w.push('"', 1);
}

// The first variant of value v among names[first, first + n), ascending; n when there is none
__device__ __forceinline__ uint32_t find_name(const JName *names, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (names[mid].value < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && names[lo].value == v ? lo : n;
}

// unassigned: the pool text {"Unassigned":
template <class W>
__device__ __forceinline__ void put_unassigned(W &w, const uint32_t *pool, JText unassigned, uint64_t v) {
    w.text(pool + unassigned.off / 4u, unassigned.len);
    put_dec(w, v);
    w.push('}', 1);
}

// The variant name, {"Unassigned":v}, or for a nested registry {"Group":"Reason"} / {"Group":{"Unassigned":v}}
template <class W>
__device__ __forceinline__ void put_subreg(W &w, const JName *all, const uint32_t *pool, JText unassigned, const JSub &s, bool nested,
                                           uint64_t v) {
    const JName *names = all + s.sub0;
    const uint32_t at = find_name(names, s.sub_n, v);
    if (nested && v / 64u >= s.grp_n) {
        put_unassigned(w, pool, unassigned, v);
        return;
    }
    if (nested) {
        const JText g = all[s.grp0 + (uint32_t)(v / 64u)].text;
        w.push('{' | ('"' << 8), 2);
        w.text(pool + g.off / 4u, g.len);
        w.push('"' | (':' << 8), 2);
    }
    if (at < s.sub_n) {
        const JText t = names[at].text;
        w.push('"', 1);
        w.text(pool + t.off / 4u, t.len);
        w.push('"', 1);
    } else {
        put_unassigned(w, pool, unassigned, v);
    }
    if (nested) w.push('}', 1);
}

// ---------------------------------------------------------------------------------------------
// host: the pool, the name table, the tag texts
// ---------------------------------------------------------------------------------------------
struct Pool {  // constant text, each at a dword offset and zero padded to a whole dword
    std::vector<uint8_t> b;
    JText add(const std::string &t) {
        const JText r{(uint32_t)b.size(), (uint32_t)t.size()};
        b.insert(b.end(), t.begin(), t.end());
        b.resize((b.size() + 3) & ~(size_t)3, 0);
        return r;
    }
};

// The sub-registry of (pen, id) into the name table: subreg_kind (0: it has none, nothing is added)
inline int add_subreg(uint32_t pen, uint16_t id, Pool &pool, std::vector<JName> &names, JSub *s) {
    std::vector<ngzh::SubregName> vals;
    std::vector<const char *> groups;
    const int sk = ngzh::subreg_names(pen, id, &vals, &groups);
    if (!sk) return 0;
    s->sub0 = (uint32_t)names.size();
    s->sub_n = (uint32_t)vals.size();
    for (const ngzh::SubregName &v : vals) names.push_back(JName{v.value, pool.add(v.name)});
    s->grp0 = (uint32_t)names.size();
    s->grp_n = (uint32_t)groups.size();
    for (size_t g = 0; g < groups.size(); ++g) names.push_back(JName{(uint32_t)g, pool.add(groups[g])});
    return sk;
}

// The four tag shapes of put_field around a value
inline void tag_text(const ngzh::Spec &s, std::string *pre, std::string *suf) {
    switch (s.kind) {
    case ngzh::IK_IANA:
        *pre = std::string("{\"") + s.name + "\":";
        *suf = "}";
        break;
    case ngzh::IK_VENDOR:
        *pre = std::string("{\"") + s.vendor + "\":{\"" + s.name + "\":";
        *suf = "}}";
        break;
    case ngzh::IK_VENDOR_UNKNOWN:
        *pre = std::string("{\"") + s.vendor + "\":{\"Unknown\":{\"id\":" + std::to_string(s.id) + ",\"value\":";
        *suf = "}}}";
        break;
    default:
        *pre = "{\"Unknown\":{\"pen\":" + std::to_string(s.pen) + ",\"id\":" + std::to_string(s.id) + ",\"value\":";
        *suf = "}}";
        break;
    }
}

}  // namespace ngzjson
