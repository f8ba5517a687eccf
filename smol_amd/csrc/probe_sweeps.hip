// probe_sweeps.hip -- TEST-ONLY probe of the Ewald potential-field sweeps of smolmc_common.h
// (libsmolmc_probe.so; never linked into the engine libraries, tests/test_gpu_ewald_sweeps.py drives it).
//
// The sweeps switch code on the NUMBER of field entries na (small masked path, batches of U groups, the shifted
// last batch, chunks of NB batches, ragged tail), not on the template instantiation, and an engine test reaches one
// na per Ewald table it builds.  Here one launch runs one sweep instantiation on a whole ladder of na: workgroup b
// (one wave) sweeps its own slice of phi with na = na_list[b], on synthetic tables.  Every instantiation below is
// one that a kernel calls; the call site stands beside it.
#include "smolmc_common.h"
#include "rows_thresholds.h" // (second probe, at the bottom: the float32 thresholds of the straight rows swap kernels)

thread_local std::string smolmc_g_err; // (smolmc_common.h's error plumbing: unused here, defined for the linker)

#define SMOLMC_PROBE_GUARD 128 // doubles behind every phi slice (the test checks that they come back unchanged)
#define SMOLMC_PROBE_SLACK (27 * 64) // LDS doubles behind the largest slice's guard, never touched by a correct sweep

enum ProbeVariant {
    PV_MULTI_1_2 = 0, // field_sweep_gx_multi<NF, FOOT> ...
    PV_MULTI_1_1,
    PV_MULTI_1_0,
    PV_MULTI_2_1,
    PV_MULTI_2_0,
    PV_MULTI_3_1,
    PV_MULTI_3_0,
    PV_MULTI_4_1,
    PV_MULTI_4_0,
    PV_MULTI_4_M1,
    PV_PRE27,
    PV_GROUPS_1_16,
    PV_GROUPS_2_16,
    PV_DENSE_1,   // field_sweep<false>
    PV_DENSE_2,   // field_sweep<true>
    PV_DENSE_1_6, // field_sweep<false, 6>
    PV_DENSE_2_4, // field_sweep<true, 4>
    PV_COUNT
};

struct ProbeFlips {
    uint32_t s8[4];
    double dq[4];
};

template <int NF, int FOOT>
__device__ __forceinline__ void probe_multi(double *phi, const uint32_t *E8, const unsigned char *gx, int lane, int na,
                                            const ProbeFlips &F) {
    uint32_t s8[NF];
    double dq[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        s8[f] = F.s8[f];
        dq[f] = F.dq[f];
    }
    field_sweep_gx_multi<NF, FOOT>(phi, E8, gx, lane, na, s8, dq);
}

template <int NF>
__device__ __forceinline__ void probe_groups16(double *phi, const uint32_t *E8, const unsigned char *gx, int lane,
                                               const ProbeFlips &F) {
    // the E8 offsets of a lane's 16 entries from registers, as mc_lean_multi.h:332 loads them
    uint32_t e0w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) e0w[u] = E8[64 * u + lane];
    uint32_t s8[NF];
    double dq[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        s8[f] = F.s8[f];
        dq[f] = F.dq[f];
    }
    field_sweep_gx_groups<NF, 16>(phi + lane, e0w, gx, s8, dq, 0);
}

template <int V>
__device__ __forceinline__ void probe_sweep(double *phi, const uint32_t *E8, const unsigned char *gx, const double *ga,
                                            const double *gb, int lane, int na, const ProbeFlips &F) {
    // single flips
    if (V == PV_MULTI_1_2) probe_multi<1, 2>(phi, E8, gx, lane, na, F);   // mc_lean.h:106 from field_apply<2, EPRE> (mc_lean.h:1079)
    if (V == PV_MULTI_1_1) probe_multi<1, 1>(phi, E8, gx, lane, na, F);   // mc_lean.h:106 from field_apply<1> (mc_lean_multi.h:807, mc_wl.h:589); mc_lean.h:165 (field_apply_flips<1, true>)
    if (V == PV_MULTI_1_0) probe_multi<1, 0>(phi, E8, gx, lane, na, F);   // mc_lean.h:106 from field_apply<0> (mc_lean_multi.h:819); mc_lean.h:165 from field_apply_flips<0> (mc_lean_multi.h:2065)
    // swaps
    if (V == PV_MULTI_2_1) probe_multi<2, 1>(phi, E8, gx, lane, na, F);   // mc_lean.h:195 from field_apply2<1> (mc_lean.h:1077, mc_wl.h:587, mc_lean_multi.h:805); mc_lean.h:169 (field_apply_flips<1, true>)
    if (V == PV_MULTI_2_0) probe_multi<2, 0>(phi, E8, gx, lane, na, F);   // mc_lean.h:195 from field_apply2<0> (mc_lean_multi.h:817); mc_lean.h:169 from field_apply_flips<0>
    // TableFlip steps, up to four flips at a time
    if (V == PV_MULTI_3_1) probe_multi<3, 1>(phi, E8, gx, lane, na, F);   // mc_lean.h:161 and :173 from field_apply_flips<1, true> (mc_lean.h:2351)
    if (V == PV_MULTI_3_0) probe_multi<3, 0>(phi, E8, gx, lane, na, F);   // mc_lean.h:173 from field_apply_flips<0> (mc_lean_multi.h:2065)
    if (V == PV_MULTI_4_1) probe_multi<4, 1>(phi, E8, gx, lane, na, F);   // mc_lean.h:175 from field_apply_flips<1, true> (mc_lean.h:2351)
    if (V == PV_MULTI_4_0) probe_multi<4, 0>(phi, E8, gx, lane, na, F);   // mc_lean.h:175 from field_apply_flips<0>; mc_lean_multi.h:307, pending flush of the swap kernels
    if (V == PV_MULTI_4_M1) probe_multi<4, -1>(phi, E8, gx, lane, na, F); // mc_lean_multi.h:307, pending flush of the flip kernels
    if (V == PV_PRE27) { // mc_lean.h:105, with the E8 entries of the first 27 groups preloaded as at mc_lean.h:462
        uint32_t e0[27];
#pragma unroll
        for (int u = 0; u < 27; ++u) e0[u] = E8[64 * u + lane];
        const uint32_t s8[1] = {F.s8[0]};
        const double dq[1] = {F.dq[0]};
        field_sweep_gx_pre27(phi, E8, gx, lane, na, s8, dq, e0);
    }
    if (V == PV_GROUPS_1_16) probe_groups16<1>(phi, E8, gx, lane, F); // mc_lean_multi.h:798 (na == 1024 only)
    if (V == PV_GROUPS_2_16) probe_groups16<2>(phi, E8, gx, lane, F); // mc_lean_multi.h:793 (na == 1024 only)
    // rows of the full site kernel
    if (V == PV_DENSE_1) field_sweep<false>(phi, ga, ga, lane, na, F.dq[0], 0.0);      // mc_lean.h:109, mc_lean.h:143
    if (V == PV_DENSE_2) field_sweep<true>(phi, ga, gb, lane, na, F.dq[0], F.dq[1]);   // mc_lean.h:203
    if (V == PV_DENSE_1_6) field_sweep<false, 6>(phi, ga, ga, lane, na, F.dq[0], 0.0); // mc_general.h:190
    if (V == PV_DENSE_2_4) field_sweep<true, 4>(phi, ga, gb, lane, na, F.dq[0], F.dq[1]); // mc_general.h:202
}

// Workgroup b = one wave: phi slice at phi_all + phi_off[b] (na + SMOLMC_PROBE_GUARD doubles), E8 / row slices at
// tab_off[b].  LDS: the slice is staged in LDS, guard included, swept there through the same generic pointer, and copied back.
template <int V, bool LDS>
__global__ __launch_bounds__(64) void probe_kernel(double *phi_all, const long long *phi_off, const long long *tab_off,
                                                   const int *na_list, const uint32_t *E8_all, const unsigned char *gx,
                                                   const double *ga_all, const double *gb_all, ProbeFlips F) {
    extern __shared__ double s_phi[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int na = na_list[b];
    double *slice = phi_all + phi_off[b];
    const uint32_t *E8 = E8_all ? E8_all + tab_off[b] : nullptr;
    const double *ga = ga_all ? ga_all + tab_off[b] : nullptr, *gb = gb_all ? gb_all + tab_off[b] : nullptr;
    double *phi = slice;
    if (LDS) {
        for (int j = lane; j < na + SMOLMC_PROBE_GUARD; j += 64) s_phi[j] = slice[j];
        __syncthreads();
        phi = s_phi;
    }
    probe_sweep<V>(phi, E8, gx, ga, gb, lane, na, F);
    if (LDS) {
        __syncthreads();
        for (int j = lane; j < na + SMOLMC_PROBE_GUARD; j += 64) slice[j] = s_phi[j];
    }
}

template <int V>
static hipError_t probe_launch(bool lds, int nblocks, int na_max, double *phi_all, const long long *phi_off,
                               const long long *tab_off, const int *na_list, const uint32_t *E8_all, const unsigned char *gx,
                               const double *ga_all, const double *gb_all, const ProbeFlips &F, hipStream_t stream) {
    if (lds) {
        const size_t bytes = (size_t)(na_max + SMOLMC_PROBE_GUARD + SMOLMC_PROBE_SLACK) * sizeof(double);
        hipLaunchKernelGGL((probe_kernel<V, true>), dim3(nblocks), dim3(64), bytes, stream, phi_all, phi_off, tab_off, na_list,
                           E8_all, gx, ga_all, gb_all, F);
    } else {
        hipLaunchKernelGGL((probe_kernel<V, false>), dim3(nblocks), dim3(64), 0, stream, phi_all, phi_off, tab_off, na_list,
                           E8_all, gx, ga_all, gb_all, F);
    }
    return hipGetLastError();
}

extern "C" {

int smolmc_probe_variant_count(void) { return PV_COUNT; }
int smolmc_probe_guard(void) { return SMOLMC_PROBE_GUARD; }

// Runs sweep `variant` on `nblocks` slices and waits for it.  The pointers are device buffers the caller filled, but for
// s8 and dq (host arrays of four: the flips go to the kernel by value); na_min / na_max are the smallest and largest
// na_list entry (host-side copies, for the LDS size and the checks).  Returns 0, or a negative
// argument error, or a positive hipError_t.
int smolmc_probe_sweep(int variant, int lds, int nblocks, int na_min, int na_max, double *phi_all, const long long *phi_off,
                       const long long *tab_off, const int *na_list, const uint32_t *E8_all, const unsigned char *gx,
                       const double *ga_all, const double *gb_all, const uint32_t *s8, const double *dq) {
    if (variant < 0 || variant >= PV_COUNT || nblocks <= 0 || na_min < 1 || na_max < na_min) return -1;
    const bool dense = variant >= PV_DENSE_1;
    if (!phi_all || !phi_off || !tab_off || !na_list || !s8 || !dq) return -2;
    if (dense ? (!ga_all || !gb_all) : (!E8_all || !gx)) return -2;
    if (variant == PV_PRE27 && na_min < 27 * 64) return -3;                                  // (the preload reads 27 groups)
    if ((variant == PV_GROUPS_1_16 || variant == PV_GROUPS_2_16) && (na_min != 1024 || na_max != 1024)) return -3;
    if (lds && (size_t)(na_max + SMOLMC_PROBE_GUARD + SMOLMC_PROBE_SLACK) * sizeof(double) > 64 * 1024) return -4; // (the default LDS limit)
    ProbeFlips F;
    for (int f = 0; f < 4; ++f) {
        F.s8[f] = s8[f];
        F.dq[f] = dq[f];
    }
    hipError_t e = hipSuccess;
#define PROBE_CASE(V)                                                                                                      \
    case V:                                                                                                                \
        e = probe_launch<V>(lds != 0, nblocks, na_max, phi_all, phi_off, tab_off, na_list, E8_all, gx, ga_all, gb_all, F, 0); \
        break;
    switch (variant) {
        PROBE_CASE(PV_MULTI_1_2)
        PROBE_CASE(PV_MULTI_1_1)
        PROBE_CASE(PV_MULTI_1_0)
        PROBE_CASE(PV_MULTI_2_1)
        PROBE_CASE(PV_MULTI_2_0)
        PROBE_CASE(PV_MULTI_3_1)
        PROBE_CASE(PV_MULTI_3_0)
        PROBE_CASE(PV_MULTI_4_1)
        PROBE_CASE(PV_MULTI_4_0)
        PROBE_CASE(PV_MULTI_4_M1)
        PROBE_CASE(PV_PRE27)
        PROBE_CASE(PV_GROUPS_1_16)
        PROBE_CASE(PV_GROUPS_2_16)
        PROBE_CASE(PV_DENSE_1)
        PROBE_CASE(PV_DENSE_2)
        PROBE_CASE(PV_DENSE_1_6)
        PROBE_CASE(PV_DENSE_2_4)
    }
#undef PROBE_CASE
    if (e != hipSuccess) return (int)e;
    e = hipDeviceSynchronize();
    return (int)e;
}

} // extern "C"

// ---- the float32 thresholds of the straight rows swap kernels (rows_thresholds.h; tests/test_gpu_rows_thresholds.py) ----
// The kernels below call the functions mc_lean_kernel calls, on words the test supplies; the walker's constants are
// derived as the kernel derives them (nbeta = -beta, inv_nbeta = 1 / nbeta).
__global__ __launch_bounds__(256) void probe_rows_thresholds_kernel(const uint32_t *w2, long long n, double beta,
                                                                    double fast_eps, float *lo, float *hi) {
    const double nbeta = -beta;
    const double inv_nbeta = 1.0 / nbeta;
    const float c_f = rows_threshold_scale(inv_nbeta), eps_f = rows_threshold_eps(fast_eps);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float a, b;
        rows_thresholds(w2[i], c_f, eps_f, a, b);
        lo[i] = a;
        hi[i] = b;
    }
}

__global__ __launch_bounds__(256) void probe_rows_log2_kernel(uint32_t first, long long n, int scaled, float *out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = rows_log2_hw(first + (uint32_t)i, scaled);
}

extern "C" {

// W of rows_thresholds.h (ulp of the hardware log2 the thresholds are widened by) and the measured worst case it rests on
int smolmc_probe_rows_widen_ulp(void) { return SMOLMC_ROWS_LOG2_WIDEN_ULP; }
double smolmc_probe_rows_measured_ulp(void) { return (double)SMOLMC_ROWS_LOG2_MEASURED_ULP; }

// lo[i], hi[i] = the thresholds of a step whose acceptance uniform begins with the word w2[i] (device buffers of n entries)
int smolmc_probe_rows_thresholds(const uint32_t *w2, long long n, double beta, double fast_eps, float *lo, float *hi) {
    if (!w2 || !lo || !hi || n <= 0) return -1;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(probe_rows_thresholds_kernel, dim3(blocks), dim3(256), 0, 0, w2, n, beta, fast_eps, lo, hi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

// out[i] = v_log_f32 of the integer first + i (scaled: of (first + i) 2^-24), i < n (device buffer of n floats)
int smolmc_probe_rows_log2(uint32_t first, long long n, int scaled, float *out) {
    if (!out || n <= 0 || (unsigned long long)first + (unsigned long long)n > (1ull << 24) + 1ull) return -1;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(probe_rows_log2_kernel, dim3(blocks), dim3(256), 0, 0, first, n, scaled, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

} // extern "C"
