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
//
// The same kernel has a second mode, uniform over a launch (smolmc_wl_synchronise, engine.hip): the merge of the copies
// of a window, the second half of the method.  Group g is the estimators g * copies .. g * copies + copies - 1; one
// workgroup per group.  If the copies' factors are not all bitwise equal: status 2.  Else a copy is flat iff, over its
// visited bins V = {i : S[i] > 0}, n = |V| >= 2 and every (double) hist[i] > flat * ((double) sum_V hist / (double) n)
// (the sum in integers; the criterion of wl_multi_flatness_check, mc_lean.h); some copy not flat: status 0.  Else
// status 1: for every bin, visited or not, a = S_e0[i], a = a + S_e0+c[i] for c = 1 .. copies - 1 in that order,
// S_e[i] = a / (double) copies in every copy, every histogram 0, every factor m / div.  parallel.WLWindows.synchronise
// is the same arithmetic in NumPy: the same arrays bit for bit.  A mode and not a kernel of its own: every __global__
// symbol of the library is classified and counted (tests/dispatch_matrix.py).
#include "smolmc_common.h"

#define WLX_WAVES 4 // pairs (exchange) or copies in flight (merge): the waves of a workgroup

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
    // merge mode (the fields above but L are unused then)
    int merge, copies;       // merge != 0: one workgroup per group of `copies` estimators
    double *S;               // [R][L] the entropies again, to be written
    long long *hist;         // [R][L]
    double *m;               // [R] modification factors
    int32_t *status;         // [R / copies] out, or null
    double *factor;          // [R / copies] out: the groups' factors after the call (copy 0's), or null
    double flat, div;
};

// The merge of one group by one workgroup of WLX_WAVES waves.  Not inlined: the exchange mode keeps its registers.
__device__ __noinline__ void wlx_merge_group(double *S, long long *hist, double *m, int32_t *status, double *factor,
                                             const double flat, const double div, const int L, const int copies) {
#pragma clang fp contract(off)
    __shared__ int s_verdict; // bit 0: a copy is not flat, bit 1: the factors differ
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t e0 = (size_t)g * copies;
    if (threadIdx.x == 0) s_verdict = 0;
    __syncthreads();
    const long long m0 = __double_as_longlong(m[e0]);
    int bad = 0;
    for (int c = w; c < copies; c += WLX_WAVES) { // (wave-uniform trip count: the ballot below sees whole waves)
        if (__double_as_longlong(m[e0 + c]) != m0) bad |= 2;
        const double *Se = S + (e0 + c) * L;
        const long long *he = hist + (e0 + c) * L;
        int n = 0;
        long long sum = 0;
        for (int i = lane; i < L; i += 64)
            if (Se[i] > 0) { n++; sum += he[i]; }
        for (int o = 32; o; o >>= 1) {
            n += __shfl_xor(n, o);
            sum += __shfl_xor(sum, o);
        }
        bool flat_copy = n >= 2;
        if (flat_copy) {
            const double mean = (double)sum / (double)n;
            const double thr = flat * mean;
            int below = 0;
            for (int i = lane; i < L; i += 64)
                if (Se[i] > 0 && !((double)he[i] > thr)) below = 1;
            flat_copy = __ballot(below) == 0ull;
        }
        if (!flat_copy) bad |= 1;
    }
    if (bad && lane == 0) atomicOr(&s_verdict, bad);
    __syncthreads();
    const int verdict = s_verdict;
    const int st = (verdict & 2) ? 2 : (verdict & 1) ? 0 : 1;
    double m_new = __longlong_as_double(m0);
    if (st == 1) {
        const double ncopies = (double)copies;
        for (int i = threadIdx.x; i < L; i += 64 * WLX_WAVES) { // (lanes on neighbouring bins: coalesced rows)
            double a = S[e0 * L + i];
            for (int c = 1; c < copies; ++c) a = a + S[(e0 + c) * L + i];
            a = a / ncopies;
            for (int c = 0; c < copies; ++c) {
                S[(e0 + c) * L + i] = a;
                hist[(e0 + c) * L + i] = 0;
            }
        }
        m_new = m_new / div;
        for (int c = threadIdx.x; c < copies; c += 64 * WLX_WAVES) m[e0 + c] = m_new; // (every read of m is in front of the barrier)
    }
    if (threadIdx.x == 0) {
        if (status) status[g] = st;
        if (factor) factor[g] = m_new;
    }
}

// bin of E in the window that starts at vmin; an in-window E gives 0 .. L - 1, the clamp is the memory-safety net the
// sampling kernels have in their guard entries (it never changes an index that is in range)
__device__ __forceinline__ int wlx_bin(const double E, const double vmin, const double bin, const int L) {
    return min(max((int)floordiv_exact(E - vmin, bin), 0), L - 1);
}

// exchange: one wave per pair; the pairs of a call are disjoint, so no two waves touch the same walker or estimator.
// merge: one workgroup per group (the mode branch comes first: the early return of a surplus wave below must not sit in
// front of the barriers of the merge).
__global__ void __launch_bounds__(64 * WLX_WAVES) wl_exchange_kernel(const WlExchangeArgs A) {
#pragma clang fp contract(off)
    if (A.merge) {
        wlx_merge_group(A.S, A.hist, A.m, A.status, A.factor, A.flat, A.div, A.L, A.copies);
        return;
    }
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

// the merge mode: R / copies groups (the caller has checked that copies divides R), one workgroup each
int smolmc_wl_merge_launch(smolmc_handle *h, int copies, int32_t *status, double *factor) {
    WlExchangeArgs A;
    memset(&A, 0, sizeof(A));
    A.merge = 1; A.copies = copies; A.L = h->L;
    A.S = h->kp.wl_entropy; A.hist = h->kp.wl_hist; A.m = h->kp.wl_m;
    A.status = status; A.factor = factor;
    A.flat = h->cfg.wl_flatness; A.div = h->cfg.wl_mod_divisor;
    hipLaunchKernelGGL(wl_exchange_kernel, dim3((unsigned)(h->R / copies)), dim3(64 * WLX_WAVES), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
