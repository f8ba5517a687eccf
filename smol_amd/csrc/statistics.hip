// Running moments, blocking sums and a histogram of the recorded samples, kept on the device (smolmc_set_statistics,
// SMOLMC_SAMPLE_STATISTICS, smolmc_update_statistics; include/smolmc.h states the rule, smol_amd/statistics.py is the
// same in NumPy).  A translation unit of its own, like observables.hip and minima.hip: nothing here touches a
// Monte-Carlo kernel, the reduction reads the rows of the sample ring (or the walkers' state arrays) when the block's
// launches are through.
//
// One kernel, one workgroup per key.  Both key modes are permutations of the walkers, so a key gets exactly one row per
// sample and every accumulator has ONE owner thread that walks the block's samples in order: no atomics, no tie rules,
// the same bits on every run.
//   stage    the key's C column values of ST_CHUNK samples go to LDS once (all threads load), instead of C^2 threads
//            reading them from the ring
//   consume  thread p owns the entries p, p + 256, p + 512 of the upper triangle s2 (C (C + 1) / 2 <= 528); thread
//            c < C also owns s1[c] and column c's blocking chain (pend and b2 live in LDS for the launch; thread 0 counts
//            nb); the last thread owns the histogram
// d = x - shift is formed where it is used (one subtraction, the same bits everywhere).
#include "smolmc_common.h"

#define ST_THREADS 256
#define ST_CHUNK 32 // samples staged at a time
#define ST_MAXC SMOLMC_MAX_STAT_COLUMNS
#define ST_MAXL SMOLMC_MAX_STAT_LEVELS
#define ST_OWN 3    // s2 entries a thread owns at most: ceil(528 / 256)

struct StatArgs {
    // the rows
    const double *H, *feat;    // [rows], [rows x F]
    const int32_t *counts;     // [rows x K] or null
    const double *inten;       // [rows x I] or null: the intensities of the structure-factor spec in force
    const long long *conn;     // [rows x CS] or null: the stats of the connectivity spec in force, 24 per graph
    const int32_t *pat;        // [rows x PC] or null: the cells of the pattern spec in force
    const int32_t *env;        // [rows x EC] or null: the cells of the environment spec in force
    const int32_t *walker_at;  // key -> walker, or null: the identity
    // the record
    long long *n, *nb, *hist, *under, *over;
    double *shift, *s1, *s2, *pend, *b2;
    uint64_t *has;
    // the spec
    const int32_t *columns;    // [C]
    const double *weights;     // [n_weights]
    double hist_min, hist_bin;
    int C, L, n_bins, hist_column, n_weights;
    int R, F, K, I, CS, PC, EC;
    long long nsamples;
};

// column source `src` of row `row`: 0 the enthalpy, 1 + i feature i, 1 + F + k kind count k, 1 + F + K the weighted sum,
// 2 + F + K + i intensity i, 2 + F + K + I + c connectivity number c (24 per graph) as a double, 2 + F + K + I + CS + c
// pattern cell c as a double, 2 + F + K + I + CS + PC + c environment cell c as a double
__device__ __forceinline__ double stat_column(const StatArgs &A, size_t row, int src) {
    if (src == 0) return A.H[row];
    if (src <= A.F) return A.feat[row * A.F + (src - 1)];
    if (src <= A.F + A.K) return (double)A.counts[row * A.K + (src - 1 - A.F)];
    if (src > 1 + A.F + A.K + A.I + A.CS + A.PC) return (double)A.env[row * A.EC + (src - 2 - A.F - A.K - A.I - A.CS - A.PC)];
    if (src > 1 + A.F + A.K + A.I + A.CS) return (double)A.pat[row * A.PC + (src - 2 - A.F - A.K - A.I - A.CS)];
    if (src > 1 + A.F + A.K + A.I) return (double)A.conn[row * A.CS + (src - 2 - A.F - A.K - A.I)];
    if (src > 1 + A.F + A.K) return A.inten[row * A.I + (src - 2 - A.F - A.K)];
    return weighted_value_rn(A.weights, A.feat + row * A.F, A.n_weights);
}

__global__ void __launch_bounds__(ST_THREADS) statistics_kernel(const StatArgs A) {
    // Every product and every sum is rounded on its own, as NumPy does it (see weighted_value_rn, smolmc_common.h).
#pragma clang fp contract(off)
    __shared__ double s_x[ST_CHUNK * ST_MAXC];
    __shared__ double s_shift[ST_MAXC];
    __shared__ double s_pend[ST_MAXL * ST_MAXC], s_b2[ST_MAXL * ST_MAXC];
    __shared__ long long s_nb[ST_MAXL];
    const int key = blockIdx.x, tid = threadIdx.x;
    const int C = A.C, L = A.L, P = C * (C + 1) / 2;
    const size_t walker = A.walker_at ? (size_t)A.walker_at[key] : (size_t)key;
    const long long n0 = A.n[key];
    // the key's accumulators: s2 in registers, the blocking arrays in LDS
    double acc[ST_OWN];
    int ia[ST_OWN], ib[ST_OWN];
#pragma unroll
    for (int j = 0; j < ST_OWN; ++j) {
        const int p = tid + j * ST_THREADS;
        ia[j] = -1;
        ib[j] = 0;
        acc[j] = 0.0;
        if (p < P) { // entry p of the upper triangle, row-major: row a starts at a C - a (a - 1) / 2
            int a = 0, q = p;
            while (q >= C - a) {
                q -= C - a;
                ++a;
            }
            ia[j] = a;
            ib[j] = a + q;
            acc[j] = A.s2[(size_t)key * P + p];
        }
    }
    double my_s1 = 0.0;
    uint64_t my_has = 0;
    if (tid < C) {
        s_shift[tid] = A.shift[(size_t)key * C + tid];
        my_s1 = A.s1[(size_t)key * C + tid];
        my_has = A.has[(size_t)key * C + tid];
    }
    for (int i = tid; i < L * C; i += ST_THREADS) {
        s_pend[i] = A.pend[(size_t)key * L * C + i];
        s_b2[i] = A.b2[(size_t)key * L * C + i];
    }
    if (tid < L) s_nb[tid] = A.nb[(size_t)key * L + tid];
    const bool hist_owner = tid == ST_THREADS - 1 && A.n_bins > 0;
    long long under = 0, over = 0;
    if (hist_owner) {
        under = A.under[key];
        over = A.over[key];
    }
    for (long long s0 = 0; s0 < A.nsamples; s0 += ST_CHUNK) {
        const int m = (int)(A.nsamples - s0 < ST_CHUNK ? A.nsamples - s0 : ST_CHUNK);
        __syncthreads(); // (the chunk before is consumed; the loads above are done)
        for (int e = tid; e < m * C; e += ST_THREADS) {
            const int s = e / C, c = e - s * C;
            s_x[s * ST_MAXC + c] = stat_column(A, (size_t)(s0 + s) * A.R + walker, A.columns[c]);
        }
        __syncthreads();
        if (n0 == 0 && s0 == 0) { // (uniform over the workgroup) the key's first offered value
            if (tid < C) s_shift[tid] = s_x[tid];
            __syncthreads();
        }
        for (int s = 0; s < m; ++s) {
            const double *x = s_x + s * ST_MAXC;
#pragma unroll
            for (int j = 0; j < ST_OWN; ++j)
                if (ia[j] >= 0) {
                    const double da = x[ia[j]] - s_shift[ia[j]], db = x[ib[j]] - s_shift[ib[j]];
                    const double p = da * db;
                    acc[j] = acc[j] + p;
                }
            if (tid < C) {
                const double d = x[tid] - s_shift[tid];
                my_s1 = my_s1 + d;
                double carry = d;
                for (int l = 0; l < L; ++l) {
                    const double c2 = carry * carry;
                    s_b2[l * C + tid] = s_b2[l * C + tid] + c2;
                    if (tid == 0) s_nb[l] += 1;
                    if (!((my_has >> l) & 1)) {
                        s_pend[l * C + tid] = carry;
                        my_has |= (uint64_t)1 << l;
                        break;
                    }
                    carry = s_pend[l * C + tid] + carry;
                    my_has &= ~((uint64_t)1 << l);
                }
            }
            if (hist_owner) {
                const double xv = x[A.hist_column];
                const double q = floordiv_exact(xv - A.hist_min, A.hist_bin);
                if (!(fabs(xv) <= 1.7976931348623157e308) || !(q == q)) ++over; // (not finite)
                else if (q < 0.0) ++under;
                else if (q >= (double)A.n_bins) ++over;
                else A.hist[(size_t)key * A.n_bins + (size_t)q] += 1;
            }
        }
    }
    __syncthreads(); // (the blocking arrays in LDS are final)
#pragma unroll
    for (int j = 0; j < ST_OWN; ++j)
        if (ia[j] >= 0) A.s2[(size_t)key * P + tid + j * ST_THREADS] = acc[j];
    if (tid < C) {
        A.shift[(size_t)key * C + tid] = s_shift[tid];
        A.s1[(size_t)key * C + tid] = my_s1;
        A.has[(size_t)key * C + tid] = my_has;
    }
    for (int i = tid; i < L * C; i += ST_THREADS) {
        A.pend[(size_t)key * L * C + i] = s_pend[i];
        A.b2[(size_t)key * L * C + i] = s_b2[i];
    }
    if (tid < L) A.nb[(size_t)key * L + tid] = s_nb[tid];
    if (hist_owner) {
        A.under[key] = under;
        A.over[key] = over;
    }
    if (tid == 0) A.n[key] = n0 + A.nsamples;
}

int smolmc_stat_launch(smolmc_handle *h, const double *d_H, const double *d_feat, const int32_t *d_counts, const double *d_inten,
                       const long long *d_conn, const int32_t *d_pat, const int32_t *d_env, long long nsamples) {
    SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("no statistics record set (smolmc_set_statistics)");
    if (S.n_count_cols && !d_counts) return fail("statistics: a record with count columns needs the kind counts of the rows");
    if (S.n_inten_cols && !d_inten) return fail("statistics: a record with intensity columns needs the intensities of the rows");
    if (S.n_conn_cols && !d_conn) return fail("statistics: a record with connectivity columns needs the connectivity stats of the rows");
    if (S.n_pat_cols && !d_pat) return fail("statistics: a record with pattern columns needs the pattern cells of the rows");
    if (S.n_env_cols && !d_env) return fail("statistics: a record with environment columns needs the environment cells of the rows");
    if (S.key == SMOLMC_STAT_BY_STATE_POINT && !h->wl_win_min.empty())
        return fail("statistics: a record keyed by state point on a Wang-Landau handle with per-walker windows");
    if (nsamples <= 0 || (size_t)nsamples * h->R > 0x7fffffffull) return fail("statistics: 1 .. 2^31 rows in one launch");
    StatArgs A;
    memset(&A, 0, sizeof(A));
    A.H = d_H; A.feat = d_feat; A.counts = d_counts; A.inten = d_inten; A.conn = d_conn; A.pat = d_pat; A.env = d_env;
    // (the maps exist once smolmc_exchange_grid has run; both are permutations of 0 .. R - 1 at every kernel boundary)
    A.walker_at = S.key == SMOLMC_STAT_BY_STATE_POINT ? h->d_walker_at : nullptr;
    A.n = S.n; A.nb = S.nb; A.hist = S.hist; A.under = S.under; A.over = S.over;
    A.shift = S.shift; A.s1 = S.s1; A.s2 = S.s2; A.pend = S.pend; A.b2 = S.b2; A.has = S.has;
    A.columns = S.columns; A.weights = S.weights; A.hist_min = S.hist_min; A.hist_bin = S.hist_bin;
    A.C = S.C; A.L = S.L; A.n_bins = S.n_bins; A.hist_column = S.hist_column; A.n_weights = S.n_weights;
    A.R = h->R; A.F = h->F; A.K = S.K; A.I = S.I; A.CS = S.CS; A.PC = S.PC; A.EC = S.EC;
    A.nsamples = nsamples;
    if (!S.ev[0])
        for (hipEvent_t &e : S.ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(S.ev[0], h->stream));
    hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)S.n_keys), dim3(ST_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], h->stream));
    return 0;
}

void smolmc_stat_free(smolmc_handle *h) {
    SmolmcStat &S = h->stats;
    if (S.arena) hipFree(S.arena);
    for (hipEvent_t e : S.ev)
        if (e) hipEventDestroy(e);
    S = SmolmcStat();
}

extern "C" int smolmc_set_statistics(smolmc_handle *h, const smolmc_statistics *s) {
    if (!h) return fail("null handle");
    if (h->dist) return fail("statistics: a distance handle samples no thermodynamic ensemble");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream)); // (queued blocks still write the record)
    if (!s) {
        smolmc_stat_free(h);
        return 0;
    }
    const int K = h->obs.K, F = h->F, I = h->sfac.I; // (no structure-factor spec: I = 0, the range ends at the weighted sum)
    const int CS = h->conn.G * SMOLMC_CONN_STATS;    // (no connectivity spec: 0, the range ends where it ends without)
    const int PC = (int)h->obs.pat.n_cells;          // (no pattern spec: 0, likewise)
    const int EC = (int)h->obs.env.n_cells;          // (no environment spec: 0, likewise)
    char msg[320];
    if (s->key != SMOLMC_STAT_BY_WALKER && s->key != SMOLMC_STAT_BY_STATE_POINT) {
        snprintf(msg, sizeof msg, "statistics: key must be 0 (by walker) or 1 (by state point), got %d", s->key);
        return fail(msg);
    }
    if (s->key == SMOLMC_STAT_BY_STATE_POINT && !h->wl_win_min.empty())
        return fail("statistics: a record keyed by state point on a Wang-Landau handle with per-walker windows (its walkers "
                    "exchange estimators, not state points)");
    if (s->n_columns < 1 || s->n_columns > SMOLMC_MAX_STAT_COLUMNS) {
        snprintf(msg, sizeof msg, "statistics: n_columns must be 1..%d, got %d", SMOLMC_MAX_STAT_COLUMNS, s->n_columns);
        return fail(msg);
    }
    if (!s->columns) return fail("statistics: null columns");
    if (s->n_weights < 0 || (s->n_weights > 0 && !s->weights)) return fail("statistics: null weights");
    if (s->n_weights > F) {
        snprintf(msg, sizeof msg, "statistics: n_weights = %d is larger than the handle's %d features", s->n_weights, F);
        return fail(msg);
    }
    const int C = s->n_columns;
    int n_count_cols = 0, n_inten_cols = 0, n_conn_cols = 0, n_pat_cols = 0, n_env_cols = 0;
    for (int c = 0; c < C; ++c) {
        const int src = s->columns[c];
        if (src < 0 || src > 1 + F + K + I + CS + PC + EC) {
            char tail[176] = "";
            if (I && CS) snprintf(tail, sizeof tail, ", %d intensities, %d connectivity numbers", I, CS);
            else if (I) snprintf(tail, sizeof tail, ", %d intensities", I);
            else if (CS) snprintf(tail, sizeof tail, ", %d connectivity numbers", CS);
            if (PC) snprintf(tail + strlen(tail), sizeof tail - strlen(tail), ", %d pattern cells", PC);
            if (EC) snprintf(tail + strlen(tail), sizeof tail - strlen(tail), ", %d environment cells", EC);
            snprintf(msg, sizeof msg, "statistics: column %d has source %d, outside 0..%d (the enthalpy, %d features, %d kinds, the "
                     "weighted sum%s)%s", c, src, 1 + F + K + I + CS + PC + EC, F, K, tail,
                     !K && src > 1 + F ? "; a kind count needs observables: call smolmc_set_observables first" : "");
            return fail(msg);
        }
        for (int b = 0; b < c; ++b)
            if (s->columns[b] == src) {
                snprintf(msg, sizeof msg, "statistics: source %d is named twice (columns %d and %d)", src, b, c);
                return fail(msg);
            }
        n_count_cols += src > F && src <= F + K;
        n_inten_cols += src > 1 + F + K && src <= 1 + F + K + I;
        n_conn_cols += src > 1 + F + K + I && src <= 1 + F + K + I + CS;
        n_pat_cols += src > 1 + F + K + I + CS && src <= 1 + F + K + I + CS + PC;
        n_env_cols += src > 1 + F + K + I + CS + PC;
    }
    if (s->n_levels < 0 || s->n_levels > SMOLMC_MAX_STAT_LEVELS) {
        snprintf(msg, sizeof msg, "statistics: n_levels must be 0..%d, got %d", SMOLMC_MAX_STAT_LEVELS, s->n_levels);
        return fail(msg);
    }
    if (s->n_bins < 0 || s->n_bins > SMOLMC_MAX_STAT_BINS) {
        snprintf(msg, sizeof msg, "statistics: n_bins must be 0..%d, got %d", SMOLMC_MAX_STAT_BINS, s->n_bins);
        return fail(msg);
    }
    if (s->n_bins > 0) {
        if (!(s->hist_bin > 0.0) || !std::isfinite(s->hist_bin) || !std::isfinite(s->hist_min))
            return fail("statistics: hist_bin must be a positive finite number and hist_min finite");
        if (s->hist_column < 0 || s->hist_column >= C) {
            snprintf(msg, sizeof msg, "statistics: hist_column = %d is no index into the %d columns", s->hist_column, C);
            return fail(msg);
        }
    }
    const size_t nk = (size_t)h->R, L = (size_t)s->n_levels, B = (size_t)s->n_bins, P = (size_t)C * (C + 1) / 2;
    const size_t per_key = 8 * (3 + 3 * (size_t)C + P + 2 * L * C + L + B);
    if (nk * per_key > ((size_t)1 << 30)) {
        snprintf(msg, sizeof msg, "statistics: a record of %zu keys x %zu bytes is larger than 1 GiB", nk, per_key);
        return fail(msg);
    }
    // one arena: the accumulators first (a reset zeroes them in one piece), then the spec and the scratch
    SmolmcStat S;
    S.n_keys = (int)nk; S.key = s->key; S.C = C; S.L = (int)L; S.n_bins = (int)B; S.hist_column = B ? s->hist_column : 0;
    S.n_weights = s->n_weights; S.K = K; S.n_count_cols = n_count_cols;
    S.I = I; S.n_inten_cols = n_inten_cols;
    S.CS = CS; S.n_conn_cols = n_conn_cols;
    S.PC = PC; S.n_pat_cols = n_pat_cols;
    S.EC = EC; S.n_env_cols = n_env_cols;
    S.hist_min = B ? s->hist_min : 0.0; S.hist_bin = B ? s->hist_bin : 1.0;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
    const size_t o_n = take(nk * 8), o_under = take(nk * 8), o_over = take(nk * 8), o_shift = take(nk * C * 8),
                 o_s1 = take(nk * C * 8), o_s2 = take(nk * P * 8), o_has = take(nk * C * 8), o_pend = take(nk * L * C * 8),
                 o_b2 = take(nk * L * C * 8), o_nb = take(nk * L * 8), o_hist = take(nk * B * 8);
    S.record_bytes = at;
    const size_t o_col = take((size_t)C * 4), o_w = take((size_t)s->n_weights * 8), o_ucnt = take(nk * (size_t)K * 4);
    HIPCHK(hipMalloc((void **)&S.arena, at));
    unsigned char *d = S.arena;
    S.n = (long long *)(d + o_n); S.under = (long long *)(d + o_under); S.over = (long long *)(d + o_over);
    S.shift = (double *)(d + o_shift); S.s1 = (double *)(d + o_s1); S.s2 = (double *)(d + o_s2); S.has = (uint64_t *)(d + o_has);
    S.pend = (double *)(d + o_pend); S.b2 = (double *)(d + o_b2); S.nb = (long long *)(d + o_nb); S.hist = (long long *)(d + o_hist);
    S.columns = (int32_t *)(d + o_col); S.weights = (double *)(d + o_w); S.u_counts = (int32_t *)(d + o_ucnt);
    hipError_t e = hipMemset(S.arena, 0, at); // (an empty record is all zeros)
    if (e == hipSuccess) e = hipMemcpy(S.columns, s->columns, (size_t)C * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && s->n_weights) e = hipMemcpy(S.weights, s->weights, (size_t)s->n_weights * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        hipFree(S.arena);
        return fail(std::string("statistics upload: ") + hipGetErrorString(e));
    }
    smolmc_stat_free(h);
    h->stats = S;
    return 0;
}

extern "C" int smolmc_statistics_shape(smolmc_handle *h, int *n_keys, int *n_columns, int *n_levels, int *n_bins) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (n_keys) *n_keys = S.n_keys;
    if (n_columns) *n_columns = S.C;
    if (n_levels) *n_levels = S.L;
    if (n_bins) *n_bins = S.n_bins;
    return 0;
}

extern "C" int smolmc_reset_statistics(smolmc_handle *h) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("no statistics record set: call smolmc_set_statistics first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemset(S.arena, 0, S.record_bytes));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int smolmc_get_statistics(smolmc_handle *h, int64_t *n, double *shift, double *s1, double *s2, uint64_t *has, double *pend,
                                     double *b2, int64_t *nb, int64_t *hist, int64_t *under, int64_t *over) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("no statistics record set: call smolmc_set_statistics first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nk = (size_t)S.n_keys, C = (size_t)S.C, L = (size_t)S.L, B = (size_t)S.n_bins, P = C * (C + 1) / 2;
    if (n) HIPCHK(hipMemcpy(n, S.n, nk * 8, hipMemcpyDeviceToHost));
    if (shift) HIPCHK(hipMemcpy(shift, S.shift, nk * C * 8, hipMemcpyDeviceToHost));
    if (s1) HIPCHK(hipMemcpy(s1, S.s1, nk * C * 8, hipMemcpyDeviceToHost));
    if (s2) HIPCHK(hipMemcpy(s2, S.s2, nk * P * 8, hipMemcpyDeviceToHost));
    if (has) HIPCHK(hipMemcpy(has, S.has, nk * C * 8, hipMemcpyDeviceToHost));
    if (pend && L) HIPCHK(hipMemcpy(pend, S.pend, nk * L * C * 8, hipMemcpyDeviceToHost));
    if (b2 && L) HIPCHK(hipMemcpy(b2, S.b2, nk * L * C * 8, hipMemcpyDeviceToHost));
    if (nb && L) HIPCHK(hipMemcpy(nb, S.nb, nk * L * 8, hipMemcpyDeviceToHost));
    if (hist && B) HIPCHK(hipMemcpy(hist, S.hist, nk * B * 8, hipMemcpyDeviceToHost));
    if (under) HIPCHK(hipMemcpy(under, S.under, nk * 8, hipMemcpyDeviceToHost));
    if (over) HIPCHK(hipMemcpy(over, S.over, nk * 8, hipMemcpyDeviceToHost));
    return 0;
}

// elapsed device time of the last reduction in ms (tools/statistics_timing.py); a measuring hook like
// smolmc_debug_minima_kernel_ms, not part of the C-ABI
extern "C" int smolmc_debug_statistics_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcStat &S = h->stats;
    if (!S.ev[0]) return fail("the statistics kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.ev[0], S.ev[1]));
    return 0;
}
