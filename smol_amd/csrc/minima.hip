// The lowest recorded states, kept on the device (smolmc_set_minima, SMOLMC_SAMPLE_MINIMA, smolmc_update_minima;
// include/smolmc.h states the rule, smol_amd/minima.py is the same in NumPy).  A translation unit of its own, like
// observables.hip: nothing here touches a Monte-Carlo kernel, the reduction reads the rows of the sample ring (or the
// walkers' state arrays) when the block's launches are through.
//
// Three passes with kernel boundaries between them -- nothing relies on visibility between workgroups inside a launch:
//   1 rows     one thread per row: the value as a 64-bit key that orders the way doubles do, the slot; both are stored
//              for pass 2, and the slot's candidate is lowered with a 64-bit atomicMin.  A wave whose rows all go to one
//              slot (a canonical run keyed by composition) reduces across its lanes first and issues one atomic.
//   2 winners  one thread per row: a row whose key equals the candidate AND is strictly below the recorded value lowers
//              the slot's winner with its row index -- the lowest row is the earliest sample, then the lowest walker.
//   3 copy     one workgroup per slot: without a winner it only rearms the scratch; with one it copies the row into the
//              entry, the occupancy 16 bytes a lane.
// A per-walker record runs minima_companions_kernel between 2 and 3 (see there).
// cand and win are all ones between launches (pass 3 rearms what passes 1 and 2 lowered).
#include "smolmc_common.h"

#define MIN_THREADS 256
#define MIN_NOKEY 0xffffffffffffffffull
#define MIN_NOROW 0xffffffffu

struct MinArgs {
    // the rows
    const double *H, *feat;    // [rows], [rows x F]
    const uint8_t *occ;        // rows of Npad bytes
    const int32_t *counts;     // [rows x K] or null
    const uint64_t *nsteps;    // [R]: the walkers' step counters when the launches are through
    uint64_t *key;             // [rows] scratch: ordered values (MIN_NOKEY: the row makes no offer)
    int32_t *slot;             // [rows] scratch: the slot (-1: none)
    // the record
    double *value, *enthalpy, *features;
    uint64_t *step;
    int64_t *sample;
    int32_t *walker, *rcounts;
    uint8_t *rocc;
    uint8_t *comp;             // per-walker record: the companions of entry 0 [R x Npad], else null
    uint64_t *cand;
    uint32_t *win;
    // the spec
    const double *weights;
    const int32_t *axis_w;     // [n_axes x K]
    int32_t bin[SMOLMC_MAX_MINIMA_AXES], extent[SMOLMC_MAX_MINIMA_AXES];
    int n_weights, n_axes;
    int R, F, K, Npad, n_slots;
    uint32_t rows;
    long long nsamples, thin_by, offer0;
};

// doubles -> unsigned keys of the same order (minima.ordered_bits): sign bit set gives ~bits, else bits | 1 << 63
__device__ __forceinline__ uint64_t min_ordered(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double min_unordered(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(MIN_THREADS) minima_rows_kernel(const MinArgs A) {
    // Every product and every sum of the value is rounded on its own, as NumPy does it.  (__dmul_rn / __dadd_rn do not
    // say that to this compiler: they are the plain operators, inlined with the contraction the build allows, and
    // came out as one v_fmac_f64.)
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * MIN_THREADS + threadIdx.x;
    const bool in = i < A.rows;
    uint64_t key = MIN_NOKEY;
    int slot = -1;
    if (in) {
        double v;
        if (A.n_weights == 0) {
            v = A.H[i];
        } else {
            v = weighted_value_rn(A.weights, A.feat + (size_t)i * A.F, A.n_weights);
        }
        v = v + 0.0; // (-0.0 -> +0.0)
        if (v == v) key = min_ordered(v);
        if (A.n_axes == 0) {
            slot = (int)(i % (uint32_t)A.R);
        } else {
            const int32_t *c = A.counts + (size_t)i * A.K;
            long long k = 0;
            for (int a = 0; a < A.n_axes; ++a) {
                long long d = 0;
                for (int j = 0; j < A.K; ++j) d += (long long)A.axis_w[a * A.K + j] * c[j];
                const long long b = A.bin[a];
                long long q = d / b;
                if (d % b != 0 && d < 0) --q; // floor
                if (q < 0 || q >= A.extent[a]) k = -1;
                if (k >= 0) k = k * A.extent[a] + q;
            }
            slot = (int)k; // (n_slots <= 2^20)
        }
        if (key == MIN_NOKEY) slot = -1;
        A.key[i] = key;
        A.slot[i] = slot;
    }
    // one slot for the whole wave: reduce across the lanes, one atomic
    const bool offers = slot >= 0;
    const unsigned long long m = __ballot(offers);
    if (!m) return;
    const int first = __shfl(slot, __ffsll((long long)m) - 1);
    if (__ballot(offers && slot != first) == 0) {
        uint64_t k = offers ? key : MIN_NOKEY;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(k, d);
            k = o < k ? o : k;
        }
        if ((threadIdx.x & 63) == 0) atomicMin((unsigned long long *)&A.cand[first], (unsigned long long)k);
    } else if (offers) {
        atomicMin((unsigned long long *)&A.cand[slot], (unsigned long long)key);
    }
}

__global__ void __launch_bounds__(MIN_THREADS) minima_winners_kernel(const MinArgs A) {
    const uint32_t i = blockIdx.x * MIN_THREADS + threadIdx.x;
    if (i >= A.rows) return;
    const int slot = A.slot[i];
    if (slot < 0) return;
    const uint64_t key = A.key[i];
    if (key == A.cand[slot] && key < min_ordered(A.value[slot])) atomicMin(&A.win[slot], i);
}

// Per-walker record, between passes 2 and 3 (pass 3 rearms the winners): when walker 0's entry is about to be replaced,
// every walker's row of that sample is kept next to it -- what get_minimum_*_occupancy(flat=False) of the reference
// returns.  One workgroup per walker; it only reads the winner of slot 0.
__global__ void __launch_bounds__(MIN_THREADS) minima_companions_kernel(const MinArgs A) {
    const uint32_t w = A.win[0];
    if (w == MIN_NOROW) return;
    const size_t r = blockIdx.x, row = (size_t)(w / (uint32_t)A.R) * A.R + r; // (w < rows: row < rows)
    const uint4 *src = (const uint4 *)(A.occ + row * A.Npad);
    uint4 *dst = (uint4 *)(A.comp + r * A.Npad);
    for (int i = threadIdx.x; i < A.Npad / 16; i += MIN_THREADS) dst[i] = src[i];
}

__global__ void __launch_bounds__(MIN_THREADS) minima_copy_kernel(const MinArgs A) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    const uint32_t w = A.win[slot];
    __syncthreads(); // (every thread has read the winner before it is rearmed)
    if (tid == 0) {
        A.cand[slot] = MIN_NOKEY;
        A.win[slot] = MIN_NOROW;
    }
    if (w == MIN_NOROW) return;
    const size_t row = w;
    {
        const uint4 *src = (const uint4 *)(A.occ + row * A.Npad);
        uint4 *dst = (uint4 *)(A.rocc + (size_t)slot * A.Npad);
        for (int i = tid; i < A.Npad / 16; i += MIN_THREADS) dst[i] = src[i];
    }
    for (int i = tid; i < A.F; i += MIN_THREADS) A.features[(size_t)slot * A.F + i] = A.feat[row * A.F + i];
    if (A.counts)
        for (int i = tid; i < A.K; i += MIN_THREADS) A.rcounts[(size_t)slot * A.K + i] = A.counts[row * A.K + i];
    if (tid == 0) {
        const long long s = (long long)(w / (uint32_t)A.R);
        const int r = (int)(w % (uint32_t)A.R);
        A.value[slot] = min_unordered(A.key[row]);
        A.enthalpy[slot] = A.H[row];
        A.walker[slot] = r;
        A.sample[slot] = A.offer0 + s;
        A.step[slot] = A.nsteps[r] - (uint64_t)((A.nsamples - 1 - s) * A.thin_by);
    }
}

// an empty record: value +inf, walker and sample -1, zeros elsewhere; the scratch armed
__global__ void __launch_bounds__(MIN_THREADS) minima_clear_kernel(const MinArgs A) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    uint4 *o = (uint4 *)(A.rocc + (size_t)slot * A.Npad);
    for (int i = tid; i < A.Npad / 16; i += MIN_THREADS) o[i] = make_uint4(0, 0, 0, 0);
    if (A.comp) { // (per walker: n_slots == R)
        uint4 *c = (uint4 *)(A.comp + (size_t)slot * A.Npad);
        for (int i = tid; i < A.Npad / 16; i += MIN_THREADS) c[i] = make_uint4(0, 0, 0, 0);
    }
    for (int i = tid; i < A.F; i += MIN_THREADS) A.features[(size_t)slot * A.F + i] = 0.0;
    for (int i = tid; i < A.K; i += MIN_THREADS) A.rcounts[(size_t)slot * A.K + i] = 0;
    if (tid == 0) {
        A.value[slot] = __longlong_as_double(0x7ff0000000000000ll);
        A.enthalpy[slot] = 0.0;
        A.walker[slot] = -1;
        A.sample[slot] = -1;
        A.step[slot] = 0;
        A.cand[slot] = MIN_NOKEY;
        A.win[slot] = MIN_NOROW;
    }
}

static void min_record_args(const smolmc_handle *h, MinArgs &A) {
    const SmolmcMin &M = h->minima;
    memset(&A, 0, sizeof(A));
    A.value = M.value; A.enthalpy = M.enthalpy; A.features = M.features; A.step = M.step; A.sample = M.sample;
    A.walker = M.walker; A.rcounts = M.counts; A.rocc = M.occ; A.comp = M.companions; A.cand = M.cand; A.win = M.win;
    A.weights = M.weights; A.axis_w = M.axis_w;
    for (int a = 0; a < SMOLMC_MAX_MINIMA_AXES; ++a) { A.bin[a] = M.bin[a]; A.extent[a] = M.extent[a]; }
    A.n_weights = M.n_weights; A.n_axes = M.n_axes;
    A.R = h->R; A.F = h->F; A.K = M.K; A.Npad = h->Npad; A.n_slots = M.n_slots;
}

int smolmc_min_launch(smolmc_handle *h, const double *d_H, const double *d_feat, const uint8_t *d_occ8, const int32_t *d_counts,
                      uint64_t *d_key, int32_t *d_slot, long long nsamples, long long thin_by) {
    SmolmcMin &M = h->minima;
    if (!M.n_slots) return fail("no minima record set (smolmc_set_minima)");
    if (M.n_axes && !d_counts) return fail("minima: a record keyed by composition needs the kind counts of the rows");
    const size_t rows = (size_t)nsamples * h->R;
    if (rows > 0x7fffffffull) return fail("minima: more than 2^31 rows in one launch");
    MinArgs A;
    min_record_args(h, A);
    A.H = d_H; A.feat = d_feat; A.occ = d_occ8; A.counts = d_counts; A.nsteps = (const uint64_t *)h->kp.nsteps;
    A.key = d_key; A.slot = d_slot;
    A.rows = (uint32_t)rows; A.nsamples = nsamples; A.thin_by = thin_by; A.offer0 = M.offers;
    if (!M.ev[0])
        for (hipEvent_t &e : M.ev) HIPCHK(hipEventCreate(&e));
    const unsigned nb = (unsigned)((rows + MIN_THREADS - 1) / MIN_THREADS);
    HIPCHK(hipEventRecord(M.ev[0], h->stream));
    hipLaunchKernelGGL(minima_rows_kernel, dim3(nb), dim3(MIN_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(M.ev[1], h->stream));
    hipLaunchKernelGGL(minima_winners_kernel, dim3(nb), dim3(MIN_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(M.ev[2], h->stream));
    if (A.comp) {
        hipLaunchKernelGGL(minima_companions_kernel, dim3((unsigned)h->R), dim3(MIN_THREADS), 0, h->stream, A);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(minima_copy_kernel, dim3((unsigned)M.n_slots), dim3(MIN_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(M.ev[3], h->stream));
    M.offers += nsamples;
    return 0;
}

void smolmc_min_free(smolmc_handle *h) {
    SmolmcMin &M = h->minima;
    if (M.arena) hipFree(M.arena);
    for (hipEvent_t e : M.ev)
        if (e) hipEventDestroy(e);
    M = SmolmcMin();
}

static int min_clear(smolmc_handle *h) {
    MinArgs A;
    min_record_args(h, A);
    hipLaunchKernelGGL(minima_clear_kernel, dim3((unsigned)h->minima.n_slots), dim3(MIN_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    h->minima.offers = 0;
    return 0;
}

extern "C" int smolmc_set_minima(smolmc_handle *h, const smolmc_minima *m) {
    if (!h) return fail("null handle");
    if (h->dist) return fail("minima: a distance handle keeps its own best states (smolmc_get_best)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream)); // (queued blocks still write the record)
    if (!m) {
        smolmc_min_free(h);
        return 0;
    }
    const int K = h->obs.K, F = h->F;
    char msg[256];
    if (m->n_weights < 0 || (m->n_weights > 0 && !m->weights)) return fail("minima: null weights");
    if (m->n_weights > F) {
        snprintf(msg, sizeof msg, "minima: n_weights = %d is larger than the handle's %d features", m->n_weights, F);
        return fail(msg);
    }
    if (m->n_axes < 0 || m->n_axes > SMOLMC_MAX_MINIMA_AXES) {
        snprintf(msg, sizeof msg, "minima: n_axes must be 0..%d, got %d", SMOLMC_MAX_MINIMA_AXES, m->n_axes);
        return fail(msg);
    }
    if (m->n_axes > 0 && !K) return fail("minima: a record keyed by composition needs observables: call smolmc_set_observables first");
    if (m->n_axes > 0 && (!m->axis_weights || !m->axis_bin || !m->axis_extent)) return fail("minima: null axis argument");
    size_t n_slots = m->n_axes ? 1 : (size_t)h->R;
    for (int a = 0; a < m->n_axes; ++a) {
        if (m->axis_bin[a] < 1 || m->axis_extent[a] < 1) {
            snprintf(msg, sizeof msg, "minima: axis %d has bin %d and extent %d: each must be >= 1", a, (int)m->axis_bin[a],
                     (int)m->axis_extent[a]);
            return fail(msg);
        }
        n_slots *= (size_t)m->axis_extent[a];
        if (n_slots > ((size_t)1 << 20)) break;
    }
    if (n_slots > ((size_t)1 << 20)) {
        snprintf(msg, sizeof msg, "minima: %s slots, larger than the limit of 2^20", m->n_axes ? "the extents give more than 2^20" : "one per walker gives more than 2^20");
        return fail(msg);
    }
    const size_t per_slot = (size_t)h->Npad + 8 * (size_t)F + 4 * (size_t)K + 40;
    if (n_slots * per_slot > ((size_t)1 << 30)) {
        snprintf(msg, sizeof msg, "minima: a record of %zu slots x %zu bytes is larger than 1 GiB", n_slots, per_slot);
        return fail(msg);
    }
    // one arena: the entry arrays first (a fetch copies them in one piece), then the scratch and the spec
    SmolmcMin M;
    M.n_slots = (int)n_slots; M.n_axes = m->n_axes; M.n_weights = m->n_weights; M.K = K;
    for (int a = 0; a < m->n_axes; ++a) { M.bin[a] = m->axis_bin[a]; M.extent[a] = m->axis_extent[a]; }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
    const size_t R = (size_t)h->R;
    const size_t o_value = take(n_slots * 8), o_H = take(n_slots * 8), o_feat = take(n_slots * F * 8), o_step = take(n_slots * 8),
                 o_sample = take(n_slots * 8), o_walker = take(n_slots * 4), o_counts = take(n_slots * K * 4),
                 o_occ = take(n_slots * h->Npad);
    M.entry_bytes = at;
    const size_t o_cand = take(n_slots * 8), o_win = take(n_slots * 4), o_w = take((size_t)m->n_weights * 8),
                 o_aw = take((size_t)m->n_axes * K * 4), o_comp = take(m->n_axes ? 0 : R * h->Npad), o_ukey = take(R * 8), o_uslot = take(R * 4), o_ucnt = take(R * K * 4);
    M.arena_bytes = at;
    HIPCHK(hipMalloc((void **)&M.arena, at));
    unsigned char *d = M.arena;
    M.value = (double *)(d + o_value); M.enthalpy = (double *)(d + o_H); M.features = (double *)(d + o_feat);
    M.step = (uint64_t *)(d + o_step); M.sample = (int64_t *)(d + o_sample); M.walker = (int32_t *)(d + o_walker);
    M.counts = (int32_t *)(d + o_counts); M.occ = d + o_occ; M.cand = (uint64_t *)(d + o_cand); M.win = (uint32_t *)(d + o_win);
    M.companions = m->n_axes ? nullptr : d + o_comp;
    M.weights = (double *)(d + o_w); M.axis_w = (int32_t *)(d + o_aw);
    M.u_key = (uint64_t *)(d + o_ukey); M.u_slot = (int32_t *)(d + o_uslot); M.u_counts = (int32_t *)(d + o_ucnt);
    hipError_t e = hipSuccess;
    if (m->n_weights) e = hipMemcpy(M.weights, m->weights, (size_t)m->n_weights * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && m->n_axes) e = hipMemcpy(M.axis_w, m->axis_weights, (size_t)m->n_axes * K * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(M.arena);
        return fail(std::string("minima upload: ") + hipGetErrorString(e));
    }
    smolmc_min_free(h);
    h->minima = M;
    return min_clear(h);
}

extern "C" int smolmc_minima_shape(smolmc_handle *h, int *n_slots, int *n_axes) {
    if (!h) return fail("null handle");
    if (n_slots) *n_slots = h->minima.n_slots;
    if (n_axes) *n_axes = h->minima.n_axes;
    return 0;
}

extern "C" int smolmc_reset_minima(smolmc_handle *h) {
    if (!h) return fail("null handle");
    if (!h->minima.n_slots) return fail("no minima record set: call smolmc_set_minima first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return min_clear(h);
}

extern "C" int smolmc_get_minima(smolmc_handle *h, double *value, double *enthalpy, double *features, int32_t *occ,
                                 int32_t *counts, int32_t *walker, int64_t *sample, uint64_t *step) {
    if (!h) return fail("null handle");
    const SmolmcMin &M = h->minima;
    if (!M.n_slots) return fail("no minima record set: call smolmc_set_minima first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)M.n_slots, F = (size_t)h->F, K = (size_t)M.K, N = (size_t)h->N, Npad = (size_t)h->Npad;
    if (value) HIPCHK(hipMemcpy(value, M.value, n * 8, hipMemcpyDeviceToHost));
    if (enthalpy) HIPCHK(hipMemcpy(enthalpy, M.enthalpy, n * 8, hipMemcpyDeviceToHost));
    if (features && F) HIPCHK(hipMemcpy(features, M.features, n * F * 8, hipMemcpyDeviceToHost));
    if (counts && K) HIPCHK(hipMemcpy(counts, M.counts, n * K * 4, hipMemcpyDeviceToHost));
    if (walker) HIPCHK(hipMemcpy(walker, M.walker, n * 4, hipMemcpyDeviceToHost));
    if (sample) HIPCHK(hipMemcpy(sample, M.sample, n * 8, hipMemcpyDeviceToHost));
    if (step) HIPCHK(hipMemcpy(step, M.step, n * 8, hipMemcpyDeviceToHost));
    if (occ) {
        std::vector<uint8_t> rows(n * Npad);
        HIPCHK(hipMemcpy(rows.data(), M.occ, n * Npad, hipMemcpyDeviceToHost));
        const int32_t *new_of = h->relabelled ? h->new_of.data() : nullptr; // (column p of the caller's row is byte new_of[p])
        for (size_t s = 0; s < n; ++s) {
            const uint8_t *src = rows.data() + s * Npad;
            int32_t *dst = occ + s * N;
            for (size_t p = 0; p < N; ++p) dst[p] = (int32_t)src[new_of ? (size_t)new_of[p] : p];
        }
    }
    return 0;
}

extern "C" int smolmc_get_minima_companions(smolmc_handle *h, int32_t *occ) {
    if (!h || !occ) return fail("null argument");
    const SmolmcMin &M = h->minima;
    if (!M.n_slots) return fail("no minima record set: call smolmc_set_minima first");
    if (!M.companions) return fail("minima: the companions of walker 0's entry are kept by a per-walker record only");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t R = (size_t)h->R, N = (size_t)h->N, Npad = (size_t)h->Npad;
    std::vector<uint8_t> rows(R * Npad);
    HIPCHK(hipMemcpy(rows.data(), M.companions, R * Npad, hipMemcpyDeviceToHost));
    const int32_t *new_of = h->relabelled ? h->new_of.data() : nullptr;
    for (size_t r = 0; r < R; ++r)
        for (size_t p = 0; p < N; ++p) occ[r * N + p] = (int32_t)rows[r * Npad + (new_of ? (size_t)new_of[p] : p)];
    return 0;
}

// elapsed device time of the three passes of the last reduction in ms (tools/minima_timing.py); a measuring hook like
// smolmc_debug_obs_kernel_ms, not part of the C-ABI
extern "C" int smolmc_debug_minima_kernel_ms(smolmc_handle *h, float *ms /* [3] */) {
    if (!h || !ms) return fail("null argument");
    const SmolmcMin &M = h->minima;
    if (!M.ev[0]) return fail("the minima kernels have not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(M.ev[3]));
    for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(ms + k, M.ev[k], M.ev[k + 1]));
    return 0;
}
