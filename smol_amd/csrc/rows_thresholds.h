// Float32 thresholds of the accept pre-test from ONE word of the acceptance uniform, without float64 (the straight
// rows swap kernels of mc_lean.h compute them per 16-step random batch; tests/test_gpu_rows_thresholds.py probes the
// same functions through libsmolmc_probe.so).
//
// The float64 rule accepts a step when dH < thr = log(u) / -beta with u = philox_u53(w2, w3); the pre-test is certain
// below thr - fast_eps and above thr + fast_eps.  With m = w2 >> 8 the uniform lies in [m 2^-24, (m + 1) 2^-24), both
// ends exact in float32, and with c = ln 2 / -beta < 0 and T(x) = log2(x 2^-24) c (decreasing in x, T(2^24) = 0)
//     T(m + 1) < thr <= T(m).
// thr_hi is the float32 evaluation of T(m) widened upward, thr_lo that of T(m + 1) widened downward, so that
//     thr_lo <= thr - fast_eps   and   thr + fast_eps <= thr_hi
// whatever w3 is: every step the pre-test decides is decided as the float64 rule decides it.
//
// Error budget of one evaluation T_eval = fl(log2_hw(x 2^-24) * c_f), relative to the exact T (x 2^-24 is exact):
//     hardware log2          K ulp <= K 2^-23   (measured, see below)
//     c_f = (float)(ln2 / -beta)   2^-24  (the float64 product and quotient before it: 3e-16, inside the slack)
//     the product's rounding       2^-24
// and the widening fma rounds once more (2^-24 of its result), so 1 + rh >= 1 / ((1 - (K + 1) 2^-23)(1 - 2^-24)) is
// needed: rh = (W + 2) 2^-23 with W >= 2 K leaves (K + 1/2) 2^-23 to spare.  fast_eps enters rounded up by 2^-20
// relative, which covers its own float32 rounding and that of the fma on either side of zero.
//
// MEASURED on the MI355X (tests/test_gpu_rows_thresholds.py, exhaustive over the integers 1 .. 2^24, against NumPy
// float64, in ulp of the result): v_log_f32 of m 2^-24, the form used here, is off by at most 0.9994 ulp (at m = 64457);
// of the bare integer m by at most 0.9999 ulp (at m = 16205731); log2(1) = 0 exactly.  The scaled form matters: log2(m) - 24
// in float32 would cancel for u near 1, the hardware's result for m 2^-24 is relative to the small logarithm itself.
// K = SMOLMC_ROWS_LOG2_MEASURED_ULP = 1 bounds both; W = SMOLMC_ROWS_LOG2_WIDEN_ULP = 3 is at least twice that (the test
// holds both against the device it runs on).
//
// Width of the band: thr_hi - thr_lo <= 2 fast_eps (1 + 2^-18) + 2 (rh + (K + 1) 2^-23 + 2^-24) |thr| + (T(m) - T(m + 1)).
// The factor of |thr| is 2 * 7.5 * 2^-23 = 1.8e-6 (the other kernels: 2e-6); the last term = kT ln(1 + 1/m) <= kT / m is
// the price of not reading w3: for m >= 2^20 at most 2^-20 kT, 1.7e-7 |thr| at u = 1/2 (for u = 2^-10 it is 9e-6 |thr|:
// one step in a thousand has a band that wide).  The exact path then runs about once in 1e5 steps, as before.
#pragma once
#include <stdint.h>
#include <math.h>

#define SMOLMC_ROWS_LOG2_MEASURED_ULP 1.0f
#define SMOLMC_ROWS_LOG2_WIDEN_ULP 3

// c_f: the scale of the thresholds, from 1 / -beta (negative)
__device__ __forceinline__ float rows_threshold_scale(double inv_nbeta) {
    return (float)(0.69314718055994530942 * inv_nbeta);
}

// fast_eps rounded up for float32 (see above); a band of zero selects the exact path on every step (thresholds -+inf)
__device__ __forceinline__ float rows_threshold_eps(double fast_eps) {
    return fast_eps > 0.0 ? (float)(fast_eps * (1.0 + 0x1p-20)) : INFINITY;
}

// thr_lo / thr_hi of the step whose acceptance uniform has w2 as its first word (Philox block 0, word 2)
__device__ __forceinline__ void rows_thresholds(uint32_t w2, float c_f, float eps_f, float &thr_lo, float &thr_hi) {
    constexpr float rel = (float)(SMOLMC_ROWS_LOG2_WIDEN_ULP + 2) * 0x1p-23f;
    const float x = (float)(w2 >> 8);                       // m, exact
    const float u_lo = x * 0x1p-24f;                        // m 2^-24, exact
    const float u_hi = __builtin_fmaf(x, 0x1p-24f, 0x1p-24f); // (m + 1) 2^-24, exact
    const float t_hi = __builtin_amdgcn_logf(u_lo) * c_f;   // T(m) >= 0; m = 0: +inf
    const float t_lo = __builtin_amdgcn_logf(u_hi) * c_f;   // T(m + 1) >= 0; m + 1 = 2^24: 0
    thr_hi = __builtin_fmaf(t_hi, 1.0f + rel, eps_f);
    thr_lo = __builtin_fmaf(t_lo, 1.0f - rel, -eps_f);
}

// the bare hardware log2, for the exhaustive measurement of its error (scaled != 0: of m 2^-24, as used above)
__device__ __forceinline__ float rows_log2_hw(uint32_t m, int scaled) {
    const float x = (float)m;
    return __builtin_amdgcn_logf(scaled ? x * 0x1p-24f : x);
}
