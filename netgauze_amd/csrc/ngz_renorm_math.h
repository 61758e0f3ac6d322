// Per-record arithmetic of the flow renormalization (include/ngz/flow_renormalize.h): the
// reference's calculate_renormalization_factor and count scaling
// (crates/collector/src/flow/renormalization/logic.rs:30-261, 346-374) restated for host and
// device.  Used by the kernel (ngz_renorm.hip), by the host paths of the same unit and by the
// stand-alone check tests/native/renorm_math_check.cpp.  IEEE f64 with plain / and *: the
// library is built with -ffp-contract=off and without fast-math.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGZ_RN_HD __host__ __device__ inline
#else
#define NGZ_RN_HD inline
#endif

// parameter index -> IE (ngz_renorm_plan.param_field order)
#define NGZ_RN_P34 0   // samplingInterval
#define NGZ_RN_P35 1   // samplingAlgorithm
#define NGZ_RN_P49 2   // samplerMode
#define NGZ_RN_P50 3   // samplerRandomInterval
#define NGZ_RN_P304 4  // selectorAlgorithm
#define NGZ_RN_P305 5  // samplingPacketInterval
#define NGZ_RN_P306 6  // samplingPacketSpace
#define NGZ_RN_P309 7  // samplingSize
#define NGZ_RN_P310 8  // samplingPopulation
#define NGZ_RN_P311 9  // samplingProbability (f64 bits)
#define NGZ_RN_NPARAMS 10

// SamplingParameters (logic.rs:90-105): `present` bit i = parameter i is Some
struct NgzRenormParams {
    uint32_t present;
    uint32_t interval34, algorithm35, mode49, interval50, selector304, interval305, space306, size309, population310;
    double probability311;
};

struct NgzRenormFactor {
    double k;
    uint8_t has_k;     // Some(k)
    uint8_t invalid;   // ie_missing_or_invalid increments (0 / 1)
    uint8_t inferred;  // sampling_algorithm_inferred increments (0 / 1)
};

// calculate_renormalization_factor (logic.rs:107-261)
NGZ_RN_HD NgzRenormFactor ngz_renorm_factor(const NgzRenormParams &p) {
    NgzRenormFactor r;
    r.k = 0.0;
    r.has_k = r.invalid = r.inferred = 0;
    const uint32_t m = p.present;
    auto has = [m](int i) { return (m >> i) & 1u; };
    // calculate_count_based_k (:30-48), _random_n_out_of_n_k (:50-68), _probabilistic_k (:70-88)
    auto count_based = [&]() {
        if (p.interval305 == 0) r.invalid = 1;
        else { r.k = ((double)p.space306 + (double)p.interval305) / (double)p.interval305; r.has_k = 1; }
    };
    auto n_out_of_n = [&]() {
        if (p.size309 == 0) r.invalid = 1;
        else { r.k = (double)p.population310 / (double)p.size309; r.has_k = 1; }
    };
    auto probabilistic = [&]() {
        if (p.probability311 > 0.0 && p.probability311 <= 1.0) { r.k = 1.0 / p.probability311; r.has_k = 1; }
        else r.invalid = 1;
    };
    if (has(NGZ_RN_P304)) {  // :114-176
        if (p.selector304 == 1) {
            if (has(NGZ_RN_P305) && has(NGZ_RN_P306)) count_based();
            else r.invalid = 1;
        } else if (p.selector304 == 3) {
            if (has(NGZ_RN_P309) && has(NGZ_RN_P310)) n_out_of_n();
            else r.invalid = 1;
        } else if (p.selector304 == 4) {
            if (has(NGZ_RN_P311)) probabilistic();
            else r.invalid = 1;
        } else {
            r.invalid = 1;
        }
    } else if (has(NGZ_RN_P49)) {  // :177-204
        if ((p.mode49 == 1 || p.mode49 == 2) && has(NGZ_RN_P50)) { r.k = (double)p.interval50; r.has_k = 1; }
        else r.invalid = 1;
    } else if (has(NGZ_RN_P35)) {  // :205-233
        if ((p.algorithm35 == 1 || p.algorithm35 == 2) && has(NGZ_RN_P34)) { r.k = (double)p.interval34; r.has_k = 1; }
        else r.invalid = 1;
    } else if (has(NGZ_RN_P305) && has(NGZ_RN_P306)) {  // :236-256, the inferred chain
        r.inferred = 1;
        count_based();
    } else if (has(NGZ_RN_P309) && has(NGZ_RN_P310)) {
        r.inferred = 1;
        n_out_of_n();
    } else if (has(NGZ_RN_P311)) {
        r.inferred = 1;
        probabilistic();
    } else if (has(NGZ_RN_P50)) {
        r.inferred = 1;
        r.k = (double)p.interval50;
        r.has_k = 1;
    } else if (has(NGZ_RN_P34)) {
        r.inferred = 1;
        r.k = (double)p.interval34;
        r.has_k = 1;
    }
    return r;
}

// `(count as f64 * k) as u64` (logic.rs:353-365): the conversion to f64 rounds to nearest even,
// the cast back truncates toward zero and saturates (NaN -> 0), as Rust's `as` does.  A C++ cast
// of an out-of-range double is undefined, hence the explicit clamps.
NGZ_RN_HD uint64_t ngz_renorm_scale(uint64_t count, double k) {
    const double x = (double)count * k;
    if (!(x > 0.0)) return 0;  // NaN, zero and negatives
    if (x >= 18446744073709551616.0) return ~0ull;
    return (uint64_t)x;
}
