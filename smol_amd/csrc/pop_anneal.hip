// Population annealing (smolmc_anneal_resample, smolmc_anneal_adaptive, smolmc_resample; engine.hip): the weights, the systematic resampling and
// the walker clone on the device.  A translation unit of its own, like grid_exchange.hip: a kernel added to engine.hip
// would move the descriptors of all of its kernels.
//
// One step takes a population of n walkers (a contiguous block of slots, one temperature) from beta to beta', db =
// beta' - beta.  The move is defined in integers (parallel.PopulationAnnealing is the same in NumPy):
//   H_ref = min H (db > 0) or max H (otherwise);   w_j = exp(-(db * (H_j - H_ref)));   q_j = (u64) floor(w_j 2^40)
//   Q = sum q_j;   off = (word * Q) >> 64;   C_j = q_0 + ... + q_j
//   child m (0 <= m < n) descends from the smallest j with n C_j > m Q + off (128-bit on both sides)
//   cnt_j children; every survivor (cnt > 0) keeps its slot, the k-th dead slot takes the k-th surplus copy, of the
//   donors repeat(arange(n), max(cnt - 1, 0)):  parent[m], with parent[parent[m]] == parent[m]
// The only floating-point operations are the product, the negation, the exp and the exact scaling: with contraction
// off (there is nothing to contract, the pragma says so) they round as NumPy's do, exp up to its last bit.
//
// An adaptive step (smolmc_anneal_adaptive) chooses beta' first, in a phase in front of the same kernel: the largest step
// towards a limit at which the energy histograms at beta and beta' still overlap by a target (pa_choose_step below).
#include "smolmc_common.h"

#define PA_THREADS 256
#define PA_WAVES (PA_THREADS / 64)

struct PopParentArgs {
    const double *enthalpy, *beta; // [R]
    const double *beta_new;        // [npop]
    const uint64_t *word;          // [npop]
    int32_t *parent;               // [R] out (slot numbers of the handle, not of the population)
    uint64_t *q, *qsum;            // [R], [npop] out
    double *href;                  // [npop] out
    uint64_t *C;                   // [R] scratch: inclusive sums of q
    uint32_t *cnt, *sur, *drank;   // [R] scratch: children, inclusive sums of the surplus copies, rank among the dead slots
    int n;                         // walkers per population
    // the adaptive step (n_iter > 0): beta_new is chosen here, towards beta_limit = 1 / (kB T_limit)
    int n_iter, npop;
    uint32_t target;               // the target overlap is target / 2^32
    double T_limit, beta_limit, kB;
    double *beta_out, *T_out;      // [npop], [1] out, written by workgroup 0
    int32_t *flags_out;            // [1] out: bit 0 reached, bit 1 forced
};

template <typename T> __device__ __forceinline__ T pa_wave_scan(T v, const int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
// inclusive scan of one chunk of PA_THREADS values behind `carry` (uniform; it gains the chunk's total): wave scans, the
// wave totals through LDS.  Every thread of the workgroup calls it.
template <typename T> __device__ __forceinline__ T pa_block_scan(T v, T *tot, T &carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = pa_wave_scan(v, lane);
    if (lane == 63) tot[wave] = v;
    __syncthreads();
    T before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) {
        if (w < wave) before += tot[w];
        all += tot[w];
    }
    __syncthreads();
    carry += all;
    return v + before;
}

// H_ref of one population: the enthalpy of the largest weight (a min / max: exact, whatever the order).  Every thread of
// the workgroup calls it; red is free again once the workgroup has passed its next barrier.
__device__ __forceinline__ double pa_block_ref(const double *H, const int n, const bool cool, double *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double ref = H[0];
    for (int j = tid; j < n; j += PA_THREADS) ref = cool ? fmin(ref, H[j]) : fmax(ref, H[j]);
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const double o = __shfl_xor(ref, d);
        ref = cool ? fmin(ref, o) : fmax(ref, o);
    }
    if (lane == 0) red[wave] = ref;
    __syncthreads();
    ref = red[0];
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) ref = cool ? fmin(ref, red[w]) : fmax(ref, red[w]);
    return ref;
}
__device__ __forceinline__ uint64_t pa_weight(const double db, const double Hj, const double ref) {
#pragma clang fp contract(off)
    const double w = exp(-(db * (Hj - ref)));
    return (uint64_t)(w * 1099511627776.0); // 2^40: the scaling is exact, the conversion truncates
}

// ---- the adaptive step: the largest step towards beta_limit that keeps the overlap of the energy histograms --------
// overlap_ok(db) of one population, in integers (PopulationAnnealing.overlap_ok is the same in NumPy):
//   s = sum_j min(Q, n q_j) = c Q + n U, c walkers with n q_j >= Q, U the sum of the other q_j;  ok iff s 2^32 >= t n Q
// Q is needed before c and U: the first chunk's q_j stays in a register, those of later chunks are evaluated twice (the
// enthalpies are read again, from L2).  The sums are integers: the same whatever the order.
template <typename T> __device__ __forceinline__ T pa_block_sum(T v, T *tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) tot[wave] = v;
    __syncthreads();
    T all = 0;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) all += tot[w];
    __syncthreads();
    return all;
}
__device__ __forceinline__ bool pa_overlap_ok(const double *H, const int n, const double ref, const double db, const uint32_t target,
                                              uint64_t *red_q, uint32_t *red_a) {
    const int tid = threadIdx.x;
    uint64_t q0 = 0, part = 0;
    for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        const uint64_t qj = j < n ? pa_weight(db, H[j], ref) : 0;
        if (j0 == 0) q0 = qj;
        part += qj; // (at most 2^14 terms of at most 2^40)
    }
    const uint64_t Q = pa_block_sum(part, red_q);
    uint32_t c = 0;
    uint64_t U = 0;
    for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        if (j < n) {
            const uint64_t qj = j0 == 0 ? q0 : pa_weight(db, H[j], ref);
            if ((uint64_t)n * qj >= Q) ++c; // (n <= 2^22: below 2^63)
            else U += qj;
        }
    }
    c = pa_block_sum(c, red_a);
    U = pa_block_sum(U, red_q);
    // uniform values from here on: every thread takes the same decision
    const unsigned __int128 s = (unsigned __int128)c * Q + (unsigned __int128)(uint64_t)n * U; // < 2^85
    return (s << 32) >= (unsigned __int128)((uint64_t)target * (uint64_t)n) * Q;             // both sides < 2^117
}
// The choice for all populations (PopulationAnnealing.next_temperature): per population the whole step D if it is ok,
// else a bisection of [0, D] that keeps ok(lo) and not ok(hi); the step of smallest magnitude wins.  Every workgroup runs
// the search of every population -- the same code on the same inputs, so all arrive at the same beta' without a
// reduction across workgroups -- and writes nothing to global memory but workgroup 0, which owns the three outputs.
// Returns beta'.
__device__ __forceinline__ double pa_choose_step(const PopParentArgs &A, double *red_d, uint64_t *red_q, uint32_t *red_a) {
#pragma clang fp contract(off)
    const int n = A.n;
    const double beta = A.beta[0]; // (one temperature over all populations: the host refuses anything else)
    const double D = A.beta_limit - beta;
    const bool cool = D > 0.0; // (every step that is evaluated has the sign of D)
    double db = D;
    bool reached = true, forced = false;
    for (int pp = 0; pp < A.npop; ++pp) {
        const double *H = A.enthalpy + (size_t)pp * n;
        const double ref = pa_block_ref(H, n, cool, red_d);
        double db_p = D;
        bool forced_p = false;
        if (!pa_overlap_ok(H, n, ref, D, A.target, red_q, red_a)) {
            reached = false;
            double lo = 0.0, hi = D;
            for (int it = 0; it < A.n_iter; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (mid == lo || mid == hi) break;
                if (pa_overlap_ok(H, n, ref, mid, A.target, red_q, red_a)) lo = mid;
                else hi = mid;
            }
            forced_p = lo == 0.0; // (the target is not met at this resolution: the schedule moves all the same)
            db_p = forced_p ? hi : lo;
        }
        if (pp == 0 || fabs(db_p) < fabs(db)) {
            db = db_p;
            forced = forced_p;
        }
    }
    const double T_new = reached ? A.T_limit : 1.0 / (A.kB * (beta + db));
    const double b_new = 1.0 / (A.kB * T_new); // (as set_betas: d_beta == 1 / (kB point_T) stays true)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int pp = 0; pp < A.npop; ++pp) A.beta_out[pp] = b_new;
        *A.T_out = T_new;
        *A.flags_out = (reached ? 1 : 0) | (forced ? 2 : 0);
    }
    return b_new;
}

// one workgroup per population
__global__ void __launch_bounds__(PA_THREADS) pop_parent_kernel(const PopParentArgs A) {
#pragma clang fp contract(off)
    __shared__ double red_d[PA_WAVES];
    __shared__ uint64_t red_q[PA_WAVES];
    __shared__ uint32_t red_a[PA_WAVES], red_b[PA_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, n = A.n;
    const size_t base = (size_t)p * n;
    const double *H = A.enthalpy + base;
    uint64_t *q = A.q + base, *C = A.C + base;
    uint32_t *cnt = A.cnt + base, *sur = A.sur + base, *drank = A.drank + base;
    // (A.n_iter is a launch argument: uniform over the grid; a fixed-schedule call reads the beta' it was given)
    const double b_new = A.n_iter > 0 ? pa_choose_step(A, red_d, red_q, red_a) : A.beta_new[p];
    const double db = b_new - A.beta[base];
    const bool cool = db > 0.0;

    const double ref = pa_block_ref(H, n, cool, red_d);

    // q_j and their inclusive sums, chunk by chunk
    uint64_t carry = 0;
    for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        uint64_t qj = 0;
        if (j < n) {
            qj = pa_weight(db, H[j], ref);
            q[j] = qj;
        }
        const uint64_t c = pa_block_scan(qj, red_q, carry);
        if (j < n) C[j] = c;
    }
    const uint64_t Q = carry;
    const uint64_t off = __umul64hi(A.word[p], Q);
    if (tid == 0) {
        A.qsum[p] = Q;
        A.href[p] = ref;
    }
    __syncthreads(); // (the scratch rows of this population are written and read by this workgroup alone)

    // children of j: child m descends from the smallest j with n C_j > m Q + off, so M_j = #{m < n: m Q + off < n C_j}
    // children descend from 0 .. j and cnt_j = M_j - M_{j-1}.  m Q + off grows with m: a binary search over m, no
    // division.  (C_{n-1} = Q and off < Q: M_{n-1} = n, every child has an ancestor.)
    for (int j = tid; j < n; j += PA_THREADS) {
        uint32_t M[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            M[e] = 0;
            if (j - e < 0) continue;
            const unsigned __int128 lhs = (unsigned __int128)(uint64_t)n * C[j - e];
            int lo = 0, hi = n; // the smallest m in 0 .. n with m Q + off >= n C
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((unsigned __int128)(uint64_t)mid * Q + off >= lhs) hi = mid;
                else lo = mid + 1;
            }
            M[e] = (uint32_t)lo;
        }
        cnt[j] = M[0] - M[1];
    }
    __syncthreads();

    // rank of every dead slot among the dead, and the inclusive sums of the surplus copies
    uint32_t dead_before = 0, sur_before = 0;
    for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        const uint32_t c = j < n ? cnt[j] : 1u;
        const uint32_t dr = pa_block_scan<uint32_t>(c == 0 ? 1u : 0u, red_a, dead_before);
        const uint32_t su = pa_block_scan<uint32_t>(c > 1 ? c - 1 : 0u, red_b, sur_before);
        if (j < n) {
            drank[j] = dr - 1; // (read for dead slots only: there dr >= 1)
            sur[j] = su;
        }
    }
    __syncthreads();

    // survivors keep their slot; the k-th dead slot takes the k-th surplus copy: of the smallest i with sur_i > k
    // (sum cnt = n: as many surplus copies as dead slots, sur_{n-1} > k for every dead rank k)
    for (int j = tid; j < n; j += PA_THREADS) {
        int src = j;
        if (cnt[j] == 0) {
            const uint32_t k = drank[j];
            int lo = 0, hi = n - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sur[mid] > k) hi = mid;
                else lo = mid + 1;
            }
            src = lo;
        }
        A.parent[base + j] = (int32_t)(base + src);
    }
}

// ---- the clone: slot m takes every per-walker row of slot parent[m] -----------------------------------------------
struct PopRow { // one per-walker array: row r at base + r * stride, `bytes` of it in use
    unsigned char *base;
    size_t stride, bytes;
};
#define PA_MAX_ROWS 10
struct PopCloneArgs {
    const int32_t *parent; // [R]
    double *beta;          // [R], or null: temperatures stay
    const double *beta_new; // [npop]
    int n;                 // walkers per population
    int nrows;
    PopRow rows[PA_MAX_ROWS];
};

// Rows are multiples of 8 bytes at 8-byte strides, or shorter than that (the accepted flag); the rows of two slots
// share their alignment modulo 16 when the stride is a multiple of 16 (the occupancy rows always, rows of doubles when
// their length is even, or when the two slots are an even distance apart).  16-byte accesses then, 8-byte or single
// bytes otherwise; four of a lane in flight before the first store.
__device__ __forceinline__ void pa_copy_row(unsigned char *__restrict__ dst, const unsigned char *__restrict__ src, const size_t bytes,
                                            const int tid) {
    if (((((uintptr_t)dst) | ((uintptr_t)src) | bytes) & 15) == 0) {
        const size_t nv = bytes >> 4;
        const uint4 *s = (const uint4 *)src;
        uint4 *d = (uint4 *)dst;
        size_t i = tid;
        for (; i + 3 * PA_THREADS < nv; i += 4 * PA_THREADS) {
            const uint4 a = s[i], b = s[i + PA_THREADS], c = s[i + 2 * PA_THREADS], e = s[i + 3 * PA_THREADS];
            d[i] = a; d[i + PA_THREADS] = b; d[i + 2 * PA_THREADS] = c; d[i + 3 * PA_THREADS] = e;
        }
        for (; i < nv; i += PA_THREADS) d[i] = s[i];
    } else if (((((uintptr_t)dst) | ((uintptr_t)src) | bytes) & 7) == 0) {
        const size_t nv = bytes >> 3;
        const uint64_t *s = (const uint64_t *)src;
        uint64_t *d = (uint64_t *)dst;
        size_t i = tid;
        for (; i + 3 * PA_THREADS < nv; i += 4 * PA_THREADS) {
            const uint64_t a = s[i], b = s[i + PA_THREADS], c = s[i + 2 * PA_THREADS], e = s[i + 3 * PA_THREADS];
            d[i] = a; d[i + PA_THREADS] = b; d[i + 2 * PA_THREADS] = c; d[i + 3 * PA_THREADS] = e;
        }
        for (; i < nv; i += PA_THREADS) d[i] = s[i];
    } else {
        for (size_t i = tid; i < bytes; i += PA_THREADS) dst[i] = src[i];
    }
}

// one workgroup per slot; a source is never a destination (parent[parent[m]] == parent[m]), so the copy is in place
__global__ void __launch_bounds__(PA_THREADS) pop_clone_kernel(const PopCloneArgs A) {
    const int m = blockIdx.x, tid = threadIdx.x;
    if (A.beta && tid == 0) A.beta[m] = A.beta_new[m / A.n];
    const int src = A.parent[m];
    if (src == m) return;
    for (int k = 0; k < A.nrows; ++k) {
        const PopRow &r = A.rows[k];
        pa_copy_row(r.base + (size_t)m * r.stride, r.base + (size_t)src * r.stride, r.bytes, tid);
    }
}

int smolmc_pop_parent_launch(smolmc_handle *h, int npop, const SmolmcPopScratch &S, const SmolmcPopSearch *search) {
    PopParentArgs A;
    memset(&A, 0, sizeof(A));
    A.enthalpy = h->kp.enthalpy; A.beta = h->d_beta; A.beta_new = S.beta_new; A.word = S.word;
    A.parent = S.parent; A.q = S.q; A.qsum = S.qsum; A.href = S.href;
    A.C = S.C; A.cnt = S.cnt; A.sur = S.sur; A.drank = S.drank;
    A.n = h->R / npop;
    A.npop = npop;
    if (search) {
        A.n_iter = search->n_iter; A.target = search->target;
        A.T_limit = search->T_limit; A.beta_limit = search->beta_limit; A.kB = SMOLMC_KB;
        A.beta_out = S.beta_new; A.T_out = S.T_new; A.flags_out = S.flags;
    }
    hipLaunchKernelGGL(pop_parent_kernel, dim3((unsigned)npop), dim3(PA_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}

int smolmc_pop_clone_launch(smolmc_handle *h, const int32_t *parent, int npop, const double *beta_new) {
    const KParams &kp = h->kp;
    PopCloneArgs A;
    memset(&A, 0, sizeof(A));
    A.parent = parent;
    A.beta = beta_new ? h->d_beta : nullptr;
    A.beta_new = beta_new;
    A.n = h->R / npop;
    auto row = [&](void *base, size_t stride, size_t bytes) {
        if (base && bytes) A.rows[A.nrows++] = PopRow{(unsigned char *)base, stride, bytes};
    };
    // every per-walker array the handle keeps in HBM between launches, but the slot's own: seeds, nsteps, nacc (its
    // position in the random stream) and the temperature
    row(kp.occ, (size_t)h->Npad, (size_t)h->Npad);
    row(kp.features, (size_t)h->F * 8, (size_t)h->F * 8);
    if (h->d_lazy_scal) { // (the scalar features the lean kernels of a lazy handle carry: rows of nscal doubles)
        const size_t ns = (size_t)(h->rt.has_ewald ? 1 : 0) + (h->rt.has_mu ? 1 : 0);
        row(h->d_lazy_scal, ns * 8, ns * 8);
    }
    row(kp.enthalpy, 8, 8);
    row(kp.last_acc, 1, 1);
    if (kp.bias_type) {
        row(kp.bias, 8, 8);
        row(kp.charge, (size_t)SMOLMC_MAX_BIAS_ROWS * 8, (size_t)SMOLMC_MAX_BIAS_ROWS * 8);
    }
    if (kp.ew_field) row(kp.ew_phi, (size_t)kp.ew_nact * 8, (size_t)kp.ew_nact * 8);
    static_assert(PA_MAX_ROWS >= 8, "one entry per array above");
    hipLaunchKernelGGL(pop_clone_kernel, dim3((unsigned)h->R), dim3(PA_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
