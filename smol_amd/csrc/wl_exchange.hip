// Replica-exchange Wang-Landau (smolmc_exchange_wl, engine.hip): the exchange between walkers of neighbouring energy
// windows, decided and applied on the device.  A translation unit of its own, like grid_exchange.hip: a kernel added to
// engine.hip would move the descriptors of all of its kernels.
//
// Estimator s = (window [vmin_s, vmax_s), density-of-states copy S_s).  Walker a holds s, walker b holds t, Ea / Eb their
// enthalpies.  The pair is rejected unless Ea lies in t's window and Eb in s's; else, with ia(E) = floor((E - vmin_s) /
// bin) and ib likewise with vmin_t (floordiv_exact, the sampling kernels' own bin function),
//   ex = ((S_s[ia(Ea)] - S_s[ia(Eb)]) + S_t[ib(Eb)]) - S_t[ib(Ea)],   accept iff ex >= 0 or log u < ex
// (Vogel, Li, Wuest, Landau, PRL 110, 210603).  On acceptance the walkers swap their ESTIMATORS -- the window records
// {vmin, vmax, estimator} the sampling kernels read, and the inverse map -- and nothing else: occupancies, features,
// enthalpies, Ewald fields and every Wang-Landau array stay where they are ("swap the state point, not the
// configuration", as in grid_exchange.hip), so an attempt costs the same for 64 bins and for 4096.  S, histogram and
// occurrences are not touched: the post-step of the next sampling step records the walker in its new estimator.
// parallel.WLWindows.decide is the same arithmetic in NumPy, operation by operation: the same decisions bit for bit.
// The exponent is three separate roundings; the pragma keeps the compiler from contracting anything around them (the
// only f64 fma of the ISA are floordiv_exact's explicit remainder and the expansion of its division; check after a
// change).
#include "smolmc_common.h"

#define WLX_WAVES 4 // pairs (waves) per workgroup

struct WlExchangeArgs {
    WlWindow *win;           // [R] the walkers' records
    int32_t *walker_at;      // [R] estimator -> walker
    const double *enthalpy;  // [R]
    const double *entropy;   // [R][L], rows by estimator
    const int32_t *pairs;    // [npairs][2] estimators
    const double *log_u;     // [npairs]
    int32_t *accepted;       // [npairs] out
    double bin;
    int npairs, L;
};

// bin of E in the window that starts at vmin; an in-window E gives 0 .. L - 1, the clamp is the memory-safety net the
// sampling kernels have in their guard entries (it never changes an index that is in range)
__device__ __forceinline__ int wlx_bin(const double E, const double vmin, const double bin, const int L) {
    return min(max((int)floordiv_exact(E - vmin, bin), 0), L - 1);
}

// one wave per pair; the pairs of a call are disjoint, so no two waves touch the same walker or estimator
__global__ void __launch_bounds__(64 * WLX_WAVES) wl_exchange_kernel(const WlExchangeArgs A) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * WLX_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= A.npairs) return;
    const int s = A.pairs[2 * p], t = A.pairs[2 * p + 1];
    const int a = A.walker_at[s], b = A.walker_at[t];
    const WlWindow wa = A.win[a], wb = A.win[b]; // (wa.est == s, wb.est == t)
    const double Ea = A.enthalpy[a], Eb = A.enthalpy[b];
    bool acc = Ea >= wb.vmin && Ea < wb.vmax && Eb >= wa.vmin && Eb < wa.vmax;
    if (acc) {
        const double *Ss = A.entropy + (size_t)s * A.L, *St = A.entropy + (size_t)t * A.L;
        const int iaa = wlx_bin(Ea, wa.vmin, A.bin, A.L), iab = wlx_bin(Eb, wa.vmin, A.bin, A.L);
        const int iba = wlx_bin(Ea, wb.vmin, A.bin, A.L), ibb = wlx_bin(Eb, wb.vmin, A.bin, A.L);
        const double ex = ((Ss[iaa] - Ss[iab]) + St[ibb]) - St[iba];
        acc = ex >= 0.0 || A.log_u[p] < ex;
    }
    if (lane == 0) {
        if (acc) {
            A.win[a] = wb;
            A.win[b] = wa;
            A.walker_at[s] = b;
            A.walker_at[t] = a;
        }
        A.accepted[p] = acc ? 1 : 0;
    }
}

int smolmc_wl_exchange_launch(smolmc_handle *h, int npairs, const int32_t *pairs, const double *log_u, int32_t *accepted) {
    WlExchangeArgs A;
    memset(&A, 0, sizeof(A));
    A.win = h->d_wl_win; A.walker_at = h->d_wl_walker_at;
    A.enthalpy = h->kp.enthalpy; A.entropy = h->kp.wl_entropy;
    A.pairs = pairs; A.log_u = log_u; A.accepted = accepted;
    A.bin = h->cfg.wl_bin_size; A.npairs = npairs; A.L = h->L;
    hipLaunchKernelGGL(wl_exchange_kernel, dim3((unsigned)((npairs + WLX_WAVES - 1) / WLX_WAVES)), dim3(64 * WLX_WAVES), 0,
                       h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
