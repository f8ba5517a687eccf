// Population annealing (smolmc_anneal_resample, smolmc_resample; engine.hip): the weights, the systematic resampling and
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

// one workgroup per population
__global__ void __launch_bounds__(PA_THREADS) pop_parent_kernel(const PopParentArgs A) {
#pragma clang fp contract(off)
    __shared__ double red_d[PA_WAVES];
    __shared__ uint64_t red_q[PA_WAVES];
    __shared__ uint32_t red_a[PA_WAVES], red_b[PA_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n;
    const size_t base = (size_t)p * n;
    const double *H = A.enthalpy + base;
    uint64_t *q = A.q + base, *C = A.C + base;
    uint32_t *cnt = A.cnt + base, *sur = A.sur + base, *drank = A.drank + base;
    const double db = A.beta_new[p] - A.beta[base];
    const bool cool = db > 0.0;

    // H_ref: the enthalpy of the largest weight (a min / max: exact, whatever the order)
    double ref = H[0];
    for (int j = tid; j < n; j += PA_THREADS) ref = cool ? fmin(ref, H[j]) : fmax(ref, H[j]);
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const double o = __shfl_xor(ref, d);
        ref = cool ? fmin(ref, o) : fmax(ref, o);
    }
    if (lane == 0) red_d[wave] = ref;
    __syncthreads();
    ref = red_d[0];
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) ref = cool ? fmin(ref, red_d[w]) : fmax(ref, red_d[w]);

    // q_j and their inclusive sums, chunk by chunk
    uint64_t carry = 0;
    for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        uint64_t qj = 0;
        if (j < n) {
            const double w = exp(-(db * (H[j] - ref)));
            qj = (uint64_t)(w * 1099511627776.0); // 2^40: the scaling is exact, the conversion truncates
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

int smolmc_pop_parent_launch(smolmc_handle *h, int npop, const SmolmcPopScratch &S) {
    PopParentArgs A;
    A.enthalpy = h->kp.enthalpy; A.beta = h->d_beta; A.beta_new = S.beta_new; A.word = S.word;
    A.parent = S.parent; A.q = S.q; A.qsum = S.qsum; A.href = S.href;
    A.C = S.C; A.cnt = S.cnt; A.sur = S.sur; A.drank = S.drank;
    A.n = h->R / npop;
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
