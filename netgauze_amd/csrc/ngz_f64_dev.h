// serde_json's text of a float64 on the device and on the host: the shortest decimal that reads back as the
// same double (f64_shortest) and ryu's five print shapes round it (put_f64), templated on the writers of
// ngz_json_dev.h.  Integer arithmetic only: no double operation, and every division is a multiply-high by a
// constant.
//
// The derivation is Ryu's (Adams, PLDI 2018).  With the double as m2 * 2^e2', the value v = 4 m2 and the
// halfway points to its neighbours v + 2 and v - 1 - s (s = 0 below a power of two, where the lower gap is
// half as wide) are all scaled by one power of 5 and one shift into the decimal vr, vp, vm with the exponent
// e10; digits are then removed from all three while vp and vm still differ above them.  What is written here
// on its own account:
//   - the three scaled values come from one 64 x 128 -> 192-bit product P = v * pow: vp's is P + 2 pow, vm's
//     P - (1 + s) pow, exactly, so the eight 32 x 32 partial products are formed once per value, not three
//     times, and the two neighbours cost an add and a subtract with carry;
//   - the powers lie in one table in global memory (ngz_f64_table.h, 618 rows of 16 bytes), a row read in one
//     16-byte load at a lane's own index;
//   - the digit loop removes two digits per step while it can, then one;
//   - the text is built in registers last character first and pushed four characters at a time; a counting
//     writer gets the length from the digit count and builds no character.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ngzjson {

constexpr uint32_t F64_N_INV = 292, F64_N_POW = 326, F64_POW_BITS = 125;

// The table twice: device code reads global memory, the host entry point (ngz_flow_json_f64_text) its own copy
__device__ static const __attribute__((aligned(16))) uint64_t kF64PowDev[F64_N_INV + F64_N_POW][2] = {
#include "ngz_f64_table.h"
};
static const uint64_t kF64PowHost[F64_N_INV + F64_N_POW][2] = {
#include "ngz_f64_table.h"
};

__host__ __device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);  // four v_mad_u64_u32
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
__host__ __device__ __forceinline__ uint64_t div10(uint64_t v) { return mulhi64(v, 0xCCCCCCCCCCCCCCCDull) >> 3; }
__host__ __device__ __forceinline__ uint64_t div100(uint64_t v) { return mulhi64(v >> 2, 0x28F5C28F5C28F5C3ull) >> 2; }
__host__ __device__ __forceinline__ uint32_t div10_32(uint32_t x) { return (uint32_t)(((uint64_t)x * 0xCCCCCCCDu) >> 35); }

// 5^p divides v: v * 5^-1 (mod 2^64) stays at or below (2^64 - 1) / 5 exactly when 5 divides v
__host__ __device__ __forceinline__ bool multiple_of_pow5(uint64_t v, uint32_t p) {
    for (uint32_t i = 0; i < p; ++i) {
        v *= 0xCCCCCCCCCCCCCCCDull;
        if (v > 0x3333333333333333ull) return false;
    }
    return true;
}

// floor((w2:w1:w0) >> j) for 64 < j < 128, a value below 2^64
__host__ __device__ __forceinline__ uint64_t shift192(uint64_t w1, uint64_t w2, uint32_t j) {
    return (w1 >> (j - 64u)) | (w2 << (128u - j));
}

// vr = floor(v * pow >> j) and the same of v + 2 (vp) and v - 1 - s (vm), from one product
__host__ __device__ __forceinline__ uint64_t mul_shift_all(uint64_t v, uint32_t row, uint32_t j, uint32_t s, uint64_t *vp, uint64_t *vm) {
#ifdef __HIP_DEVICE_COMPILE__
    const ulonglong2 pw = *(const ulonglong2 *)kF64PowDev[row];
    const uint64_t lo = pw.x, hi = pw.y;
#else
    const uint64_t lo = kF64PowHost[row][0], hi = kF64PowHost[row][1];
#endif
    const uint64_t p0 = v * lo, t = v * hi;
    uint64_t p1 = mulhi64(v, lo) + t, p2 = mulhi64(v, hi);
    p2 += p1 < t;
    // + 2 pow (pow < 2^126: the doubling stays in 128 bits)
    const uint64_t a0 = lo << 1, a1 = (hi << 1) | (lo >> 63);
    const uint64_t q0 = p0 + a0, c0 = q0 < a0;
    const uint64_t q1 = p1 + a1, q1c = q1 + c0;
    *vp = shift192(q1c, p2 + (q1 < a1) + (q1c < c0), j);
    // - (1 + s) pow
    const uint64_t b0 = s ? a0 : lo, b1 = s ? a1 : hi;
    const uint64_t bw0 = p0 < b0;
    const uint64_t r1 = p1 - b1, r1b = r1 - bw0;
    *vm = shift192(r1b, p2 - (p1 < b1) - (r1 < bw0), j);
    return shift192(p1, p2, j);
}

// The shortest decimal digits * 10^exp10 inside the rounding interval of the finite non-zero double `bits`
// (its sign is ignored): the interval's bounds belong to it when the mantissa is even; among the shortest
// candidates the closest to the value, a tie to the even digit.  The loops leave no trailing zero.
__host__ __device__ __forceinline__ void f64_shortest(uint64_t bits, uint64_t *digits, int32_t *exp10) {
    const uint64_t mant = bits & ((1ull << 52) - 1);
    const uint32_t expo = (uint32_t)(bits >> 52) & 0x7FFu;
    const int32_t e2 = (expo ? (int32_t)expo : 1) - 1023 - 52 - 2;
    const uint64_t m2 = expo ? mant | (1ull << 52) : mant;
    const bool accept = !(m2 & 1u);
    const uint64_t mv = 4 * m2;
    const uint32_t s = mant != 0 || expo <= 1;  // mm_shift: 0 only below a power of two
    uint64_t vr, vp, vm;
    int32_t e10;
    bool vm_zeros = false, vr_zeros = false;  // what was cut off below vm / vr so far is zero
    if (e2 >= 0) {
        const uint32_t q = (((uint32_t)e2 * 78913u) >> 18) - (e2 > 3);  // floor(log10(2^e2)), one less
        e10 = (int32_t)q;
        const uint32_t pow5bits = ((q * 1217359u) >> 19) + 1u;
        vr = mul_shift_all(mv, q, (uint32_t)(-e2 + (int32_t)q + (int32_t)(F64_POW_BITS + pow5bits - 1u)), s, &vp, &vm);
        if (q <= 21) {  // only then can 5^q divide a 55-bit value
            const uint32_t mod5 = (uint32_t)mv - 5u * (uint32_t)(mulhi64(mv, 0xCCCCCCCCCCCCCCCDull) >> 2);
            if (mod5 == 0) vr_zeros = multiple_of_pow5(mv, q);
            else if (accept) vm_zeros = multiple_of_pow5(mv - 1 - s, q);
            else vp -= multiple_of_pow5(mv + 2, q);
        }
    } else {
        const uint32_t ne = (uint32_t)-e2;
        const uint32_t q = ((ne * 732923u) >> 20) - (ne > 1);  // floor(log10(5^-e2)), one less
        e10 = (int32_t)q + e2;
        const uint32_t i = ne - q;
        const int32_t k = (int32_t)(((i * 1217359u) >> 19) + 1u) - (int32_t)F64_POW_BITS;
        vr = mul_shift_all(mv, F64_N_INV + i, (uint32_t)((int32_t)q - k), s, &vp, &vm);
        if (q <= 1) {  // mv = 4 m2 has its low two bits clear
            vr_zeros = true;
            if (accept) vm_zeros = s == 1;
            else --vp;
        } else if (q < 63) {
            vr_zeros = !(mv & ((1ull << q) - 1));
        }
    }
    uint32_t removed = 0;
    uint64_t out;
    if (vm_zeros || vr_zeros) {  // rare: exact halves and zeros have to be told apart, a digit at a time
        uint32_t last = 0;
        for (;;) {
            const uint64_t vp10 = div10(vp), vm10 = div10(vm);
            if (vp10 <= vm10) break;
            const uint64_t vr10 = div10(vr);
            vm_zeros &= vm == vm10 * 10;
            vr_zeros &= last == 0;
            last = (uint32_t)(vr - vr10 * 10);
            vr = vr10, vp = vp10, vm = vm10;
            ++removed;
        }
        if (vm_zeros) {
            for (;;) {
                const uint64_t vm10 = div10(vm);
                if (vm != vm10 * 10) break;
                const uint64_t vr10 = div10(vr);
                vr_zeros &= last == 0;
                last = (uint32_t)(vr - vr10 * 10);
                vr = vr10, vp = div10(vp), vm = vm10;
                ++removed;
            }
        }
        if (vr_zeros && last == 5 && !(vr & 1u)) last = 4;  // exactly half: to even
        out = vr + ((vr == vm && (!accept || !vm_zeros)) || last >= 5);
    } else {
        bool up = false;
        for (;;) {  // two digits per step
            const uint64_t vp100 = div100(vp), vm100 = div100(vm);
            if (vp100 <= vm100) break;
            const uint64_t vr100 = div100(vr);
            up = (uint32_t)(vr - vr100 * 100) >= 50u;
            vr = vr100, vp = vp100, vm = vm100;
            removed += 2;
        }
        const uint64_t vp10 = div10(vp), vm10 = div10(vm);
        if (vp10 > vm10) {  // vp / 100 == vm / 100: at most one more
            const uint64_t vr10 = div10(vr);
            up = (uint32_t)(vr - vr10 * 10) >= 5u;
            vr = vr10, vm = vm10;
            ++removed;
        }
        out = vr + (vr == vm || up);
    }
    *digits = out;
    *exp10 = e10 + (int32_t)removed;
}

// Decimal digits of v < 10^17
__host__ __device__ __forceinline__ uint32_t dec_len17(uint64_t v) {
    uint32_t n = 1;
    uint64_t p = 10;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        n += v >= p;
        p *= 10;
    }
    return n;
}

// serde_json's f64: null for NaN and the infinities, 0.0 / -0.0, otherwise with n digits, value = digits *
// 10^k and kk = n + k, one of ryu's shapes: d..d0..0.0 (0 <= k, kk <= 16), d..d.d..d (0 < kk <= 16),
// 0.0..0d..d (-5 < kk <= 0), de<x>, d.d..de<x> with x = kk - 1.  At most 24 characters.
template <class W>
__host__ __device__ __forceinline__ void put_f64(W &w, uint64_t bits) {
    const uint32_t neg = (uint32_t)(bits >> 63);
    if (((bits >> 52) & 0x7FFu) == 0x7FFu) {
        w.push('n' | ('u' << 8) | ('l' << 16) | ('l' << 24), 4);
        return;
    }
    if (!(bits << 1)) {
        if (neg) w.push('-' | ('0' << 8) | ('.' << 16) | ('0' << 24), 4);
        else w.push('0' | ('.' << 8) | ('0' << 16), 3);
        return;
    }
    uint64_t dg;
    int32_t k;
    f64_shortest(bits, &dg, &k);
    const int32_t n = (int32_t)dec_len17(dg), kk = n + k;
    const bool sci = kk > 16 || kk <= -5;
    const int32_t ex = kk - 1;
    const uint32_t ax = (uint32_t)(ex < 0 ? -ex : ex);
    if constexpr (W::counting) {
        uint32_t len = neg;
        if (sci) len += (uint32_t)n + (n > 1) + 1u + (ex < 0) + 1u + (ax >= 10u) + (ax >= 100u);
        else if (k >= 0) len += (uint32_t)kk + 2u;
        else if (kk > 0) len += (uint32_t)n + 1u;
        else len += 2u + (uint32_t)(-kk) + (uint32_t)n;
        w.n += len;
    } else {
        // the text last character first, each shifted in below the ones before it: c0, c1, c2 hold it first
        // character lowest, the order push wants
        uint64_t c0 = 0, c1 = 0, c2 = 0;
        uint32_t len = 0;
        auto pre = [&](uint32_t ch) {
            c2 = (c2 << 8) | (c1 >> 56);
            c1 = (c1 << 8) | (c0 >> 56);
            c0 = (c0 << 8) | ch;
            ++len;
        };
        int32_t dot = 0;  // digits after the point, 0: no point among them
        if (sci) {
            uint32_t x = ax;
            do {
                const uint32_t x10 = div10_32(x);
                pre('0' + x - x10 * 10u);
                x = x10;
            } while (x);
            if (ex < 0) pre('-');
            pre('e');
            dot = n - 1;
        } else if (k >= 0) {
            pre('0');
            pre('.');
            for (int32_t i = 0; i < k; ++i) pre('0');
        } else if (kk > 0) {
            dot = -k;
        }
        // the digits from the last: the low eight of them, then the rest, each below 2^32
        const uint64_t top = mulhi64(dg, 0xABCC77118461CEFDull) >> 26;  // dg / 10^8
        uint32_t x = (uint32_t)(dg - top * 100000000ull);
        for (int32_t i = 0; i < n; ++i) {
            if (i == 8) x = (uint32_t)top;
            if (i == dot && i) pre('.');
            const uint32_t x10 = div10_32(x);
            pre('0' + x - x10 * 10u);
            x = x10;
        }
        if (!sci && kk <= 0) {
            for (int32_t i = 0; i < -kk; ++i) pre('0');
            pre('.');
            pre('0');
        }
        if (neg) pre('-');
        while (len) {
            const uint32_t m = len < 4u ? len : 4u;
            w.push((uint32_t)c0, m);
            c0 = (c0 >> 32) | (c1 << 32);
            c1 = (c1 >> 32) | (c2 << 32);
            c2 >>= 32;
            len -= m;
        }
    }
}

}  // namespace ngzjson
