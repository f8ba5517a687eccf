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
//
// Keys by BINS of a column (SMOLMC_STAT_BY_BIN, smolmc_set_statistics_binned) gather several rows of a sample, or none.
// The rows of an offer are taken sample by sample and within a sample in walker order, i.e. in ascending row number of
// the launch; q = floor((x[key_column] - key_min) / key_bin) by floordiv_exact; q < 0 counts in key_under, q >= n_keys or
// a value that is not finite in key_over (one int64 each for the record) and the row is offered to no key; every other
// row is offered to key q by the rule above (no blocking: n_levels = 0).  Two more passes, each a MODE of
// statistics_kernel (StatArgs::mode, uniform over the launch; the library gains no kernel symbol, as with the merge mode
// of wl_exchange_kernel), launched one behind the other:
//   stat_bin_keys      one thread per row: its key (or a negative sentinel) into a scratch array kept with the record,
//                      the rows per key into cnt[n_keys], the two outside totals with one integer atomic per wave.
//                      Integer atomics do not depend on order: nothing here can change a bit.
//   statistics_binned  one workgroup per key; cnt == 0 exits at once.  It scans the row keys in order, 256 rows a pass,
//                      and compacts the matching row numbers in ASCENDING order into an LDS queue (ballot, the lane's
//                      prefix from the mask, per-wave offsets); whenever the queue holds ST_CHUNK rows, or the scan has
//                      ended, their values are staged and consumed with the ownership above.  Its LDS is the kernel's:
//                      the queue lies where the blocking arrays of the other modes do.
//
// The SITE FIELD (smolmc_set_statistics_sites) counts, per key, how often every tracked site held every code: sums of
// integers, so the order of the adds cannot change a bit.  One more mode of statistics_kernel, launched behind the others:
//   statistics_sites   a workgroup is (unit x chunk of ST_SITE_OWN * 256 tracked sites); thread t owns the sites
//                      chunk + t, chunk + 256 + t, ...: neighbouring lanes read neighbouring bytes of a row and add to
//                      neighbouring counters.  The unit is a KEY in the two permutation modes: the thread walks the key's
//                      row of every sample and adds its counters to site_counts once, as their only owner.  Keyed by bin
//                      the unit is a TILE of consecutive rows, read with the keys the key pass left in row_key: the thread
//                      counts while consecutive rows share a key and flushes with 64-bit integer atomics when the key
//                      changes or the tile ends; rows outside the bins are skipped.  The counters of a site are 16 bytes
//                      packed in two 64-bit registers (a flush at the latest after ST_SITE_FLUSH rows); the codes outside
//                      the field go to site_over with one atomic per wave and flush.  No LDS.
//
// The JOINT FIELD (smolmc_set_statistics_joint) counts, per key, the rows in the cells of two columns: joint[n_keys][n_a][n_b]
// and joint_out[n_keys], sums of integers again.  One more mode of statistics_kernel, launched behind the others:
//   statistics_joint   by walker or state point one THREAD per key: it walks the key's row of every sample and adds to the
//                      key's cells as their only owner (neighbouring lanes read neighbouring rows), joint_out once at the
//                      end.  Keyed by bin one thread per row, read with the key the key pass left in row_key; rows outside
//                      the bins are skipped.  Equal targets of a wave are merged before the atomic: in each of
//                      ST_JOINT_ROUNDS rounds the first lane still waiting names its counter, the lanes with the same
//                      counter are counted by ballot and leave, and the first lane sends ONE 64-bit add of that count; what
//                      waits after the rounds goes out as one atomic per lane.  A wave whose rows all meet in one cell sends
//                      one atomic, a wave of 64 different cells pays the rounds and 64 - ST_JOINT_ROUNDS atomics.  No LDS.
//                      Its arguments lie where the record's accumulator pointers do, which it does not read.
#include "smolmc_common.h"
#include <thread>

#define ST_THREADS 256
#define ST_CHUNK 32 // samples staged at a time
#define ST_MAXC SMOLMC_MAX_STAT_COLUMNS
#define ST_MAXL SMOLMC_MAX_STAT_LEVELS
#define ST_OWN 3    // s2 entries a thread owns at most: ceil(528 / 256)
#define ST_WAVES (ST_THREADS / 64)
#define ST_QUEUE 512 // row queue of the binned kernel, a ring: at most ST_CHUNK - 1 rows wait when a pass adds up to 256
#define ST_KEY_UNDER (-1) // row keys of the rows outside the bins
#define ST_KEY_OVER (-2)
#define ST_MODE_KEYS 1   // StatArgs::mode: 0 the reduction by walker or state point, 1 stat_bin_keys, 2 statistics_binned
#define ST_MODE_BINNED 2
#define ST_MODE_SITES 3     // statistics_sites
#define ST_SITE_OWN 2       // tracked sites a thread owns
#define ST_SITE_FLUSH 255   // rows a thread counts between two flushes: its counters are bytes
#define ST_SITE_TILE_MIN 16 // rows of a tile of the binned site pass
#define ST_MODE_JOINT 4     // statistics_joint
#define ST_JOINT_ROUNDS 4   // rounds of merging equal targets within a wave before the lanes that still wait add alone

struct StatArgs {
    // the rows.  The site field (mode 3) reads none of the columns: its arguments lie in their place, and the kernel's
    // arguments stay 304 bytes
    union {
        struct {
            const double *H, *feat;    // [rows], [rows x F]
            const int32_t *counts;     // [rows x K] or null
            const double *inten;       // [rows x I] or null: the intensities of the structure-factor spec in force
            const long long *conn;     // [rows x CS] or null: the stats of the connectivity spec in force, 24 per graph
            const int32_t *pat;        // [rows x PC] or null: the cells of the pattern spec in force
        };
        struct { // mode 3; row_key null: the key is the walker or its state point, else the tile's rows bring theirs
            const uint8_t *occ;            // the rows' occupancy, Npad bytes apart
            const int32_t *site_idx;       // [M] byte of tracked site m in a row, or null: byte m
            long long *site_counts;        // [n_keys x S x M]: code-major within a key (smolmc_get_statistics_sites transposes)
            unsigned long long *site_over; // [n_keys]
            int Npad, M, S, site_tile;     // site_tile: rows per tile
        };
    };
    const int32_t *env;        // [rows x EC] or null: the cells of the environment spec in force
    const int32_t *walker_at;  // key -> walker, or null: the identity
    // the record.  The joint field (mode 4) reads the columns and none of the accumulators: its arguments lie in their place
    union {
        struct {
            long long *n, *nb, *hist, *under, *over;
            double *shift, *s1, *s2, *pend, *b2;
            uint64_t *has;
        };
        struct { // mode 4; row_key null: one thread per key, else one thread per row
            unsigned long long *joint;     // [n_keys x n_a x n_b]
            unsigned long long *joint_out; // [n_keys], in the allocation of `joint`
            double joint_min_a, joint_bin_a, joint_min_b, joint_bin_b;
            int joint_col_a, joint_n_a, joint_col_b, joint_n_b; // the columns are indices into `columns`
        };
    };
    // the spec
    const int32_t *columns;    // [C]
    const double *weights;     // [n_weights]
    double hist_min, hist_bin;
    int C, L, n_bins, hist_column, n_weights;
    int R, F, K, I, CS, PC, EC;
    long long nsamples;
    // a record keyed by bin (modes 1 and 2; walker_at, nb, pend, b2, has are not read: L = 0)
    int mode;
    int key_column, n_keys;
    double key_min, key_bin;
    int32_t *row_key;            // [rows] scratch: the key of every row of the launch, ST_KEY_UNDER / ST_KEY_OVER outside
    int32_t *cnt;                // [n_keys] rows per key in this launch (zeroed before it)
    unsigned long long *outside; // key_under, key_over of the record
    long long rows;              // nsamples x R
};
static_assert(sizeof(StatArgs) == 304, "the site field's arguments lie in the place of the column pointers, the joint field's in "
                                        "the place of the accumulator pointers");

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

// ---- keys by bins of a column ---------------------------------------------------------------------------------------------
// mode 1 of statistics_kernel: one thread per row of the launch
__device__ __forceinline__ void stat_bin_keys(const StatArgs &B) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
    const bool live = row < B.rows;
    bool is_under = false, is_over = false;
    if (live) {
        const double xv = stat_column(B, (size_t)row, B.columns[B.key_column]);
        const double q = floordiv_exact(xv - B.key_min, B.key_bin);
        int key;
        if (!(fabs(xv) <= 1.7976931348623157e308) || !(q == q)) key = ST_KEY_OVER; // (not finite)
        else if (q < 0.0) key = ST_KEY_UNDER;
        else if (q >= (double)B.n_keys) key = ST_KEY_OVER;
        else key = (int)q;
        B.row_key[row] = key;
        is_under = key == ST_KEY_UNDER;
        is_over = key == ST_KEY_OVER;
        if (key >= 0) atomicAdd(&B.cnt[key], 1);
    }
    // the two outside totals: one atomic per wave
    const unsigned long long m_under = __ballot(is_under), m_over = __ballot(is_over);
    if ((threadIdx.x & 63) == 0) {
        if (m_under) atomicAdd(&B.outside[0], (unsigned long long)__popcll(m_under));
        if (m_over) atomicAdd(&B.outside[1], (unsigned long long)__popcll(m_over));
    }
}

// mode 2 of statistics_kernel: one workgroup per key; s_x [ST_CHUNK x ST_MAXC], s_shift [ST_MAXC], s_queue [ST_QUEUE] and
// s_wcnt [ST_WAVES] are the kernel's LDS
__device__ __forceinline__ void statistics_binned(const StatArgs &B, double *s_x, double *s_shift, int *s_queue, int *s_wcnt) {
    // Every product and every sum is rounded on its own, as in the other modes.
#pragma clang fp contract(off)
    const StatArgs &A = B;
    const int key = blockIdx.x, tid = threadIdx.x;
    const int cnt = B.cnt[key];
    if (cnt == 0) return; // (uniform over the workgroup) most keys of a wide grid
    const int C = A.C, P = C * (C + 1) / 2;
    const long long n0 = A.n[key];
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
    if (tid < C) {
        s_shift[tid] = A.shift[(size_t)key * C + tid];
        my_s1 = A.s1[(size_t)key * C + tid];
    }
    const bool hist_owner = tid == ST_THREADS - 1 && A.n_bins > 0;
    long long under = 0, over = 0;
    if (hist_owner) {
        under = A.under[key];
        over = A.over[key];
    }
    const int wave = tid >> 6, lane = tid & 63;
    int head = 0, tail = 0; // (uniform) rows consumed, rows found: the queue holds the rows head .. tail - 1 of the key
    bool first = n0 == 0;
    for (long long base = 0; tail < cnt && base < B.rows; base += ST_THREADS) {
        // one pass of the scan: the matching rows of base .. base + 255 join the queue in ascending order
        const long long row = base + tid;
        const bool match = row < B.rows && B.row_key[row] == key;
        const unsigned long long mask = __ballot(match);
        if (lane == 0) s_wcnt[wave] = __popcll(mask);
        __syncthreads(); // (also: the chunk before is consumed)
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) {
            const int c = s_wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (match) s_queue[(tail + before + __popcll(mask & (((unsigned long long)1 << lane) - 1))) & (ST_QUEUE - 1)] = (int)row;
        tail += total;
        const bool ended = tail >= cnt || base + ST_THREADS >= B.rows;
        while (tail - head >= ST_CHUNK || (ended && tail > head)) {
            const int m = tail - head < ST_CHUNK ? tail - head : ST_CHUNK;
            __syncthreads(); // (the queue is written; the chunk before is consumed)
            for (int e = tid; e < m * C; e += ST_THREADS) {
                const int s = e / C, c = e - s * C;
                s_x[s * ST_MAXC + c] = stat_column(A, (size_t)s_queue[(head + s) & (ST_QUEUE - 1)], A.columns[c]);
            }
            __syncthreads();
            if (first) { // (uniform over the workgroup) the key's first offered value
                if (tid < C) s_shift[tid] = s_x[tid];
                __syncthreads();
                first = false;
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
            head += m;
        }
        __syncthreads(); // (s_wcnt and the queue's consumed entries are free for the next pass)
    }
#pragma unroll
    for (int j = 0; j < ST_OWN; ++j)
        if (ia[j] >= 0) A.s2[(size_t)key * P + tid + j * ST_THREADS] = acc[j];
    if (tid < C) {
        A.shift[(size_t)key * C + tid] = s_shift[tid];
        A.s1[(size_t)key * C + tid] = my_s1;
    }
    if (hist_owner) {
        A.under[key] = under;
        A.over[key] = over;
    }
    if (tid == 0) A.n[key] = n0 + head;
}

// ---- the site field ---------------------------------------------------------------------------------------------------------
// the counters of the thread's sites, one byte per code, and its codes outside the field go to `key`: plain adds for the
// accumulators' only owner, else atomics; one add to site_over per wave (every lane of the wave is here)
__device__ __forceinline__ void stat_sites_flush(const StatArgs &A, int key, int m_first, bool atomic, uint64_t (&lo)[ST_SITE_OWN],
                                                 uint64_t (&hi)[ST_SITE_OWN], unsigned &over) {
#pragma unroll
    for (int j = 0; j < ST_SITE_OWN; ++j) {
        const int m = m_first + j * ST_THREADS;
        if (m < A.M) {
            // (on the device the counters of a key are [S][M]: the lanes' adds of one code are neighbours)
            unsigned long long *dst = (unsigned long long *)A.site_counts + (size_t)key * A.S * A.M + m;
            for (int c = 0; c < A.S; ++c) {
                const unsigned long long v = ((c < 8 ? lo[j] : hi[j]) >> ((c & 7) * 8)) & 255;
                if (v) {
                    if (atomic) atomicAdd(dst + (size_t)c * A.M, v);
                    else dst[(size_t)c * A.M] += v;
                }
            }
        }
        lo[j] = hi[j] = 0;
    }
    unsigned sum = over;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(A.site_over + key, (unsigned long long)sum);
    over = 0;
}

// mode 3 of statistics_kernel
__device__ __forceinline__ void statistics_sites(const StatArgs &A) {
    const int tid = threadIdx.x;
    const int chunks = (A.M + ST_SITE_OWN * ST_THREADS - 1) / (ST_SITE_OWN * ST_THREADS);
    const long long unit = blockIdx.x / chunks;
    const int m_first = (int)(blockIdx.x % chunks) * (ST_SITE_OWN * ST_THREADS) + tid;
    int at[ST_SITE_OWN]; // the byte of the thread's sites in a row (a site past the list: byte 0, read and not counted)
#pragma unroll
    for (int j = 0; j < ST_SITE_OWN; ++j) {
        const int m = m_first + j * ST_THREADS;
        at[j] = m < A.M ? (A.site_idx ? A.site_idx[m] : m) : 0;
    }
    uint64_t lo[ST_SITE_OWN], hi[ST_SITE_OWN];
#pragma unroll
    for (int j = 0; j < ST_SITE_OWN; ++j) lo[j] = hi[j] = 0;
    unsigned over = 0;
    const bool binned = A.row_key != nullptr; // (uniform over the launch)
    long long first, last;                    // the rows of the tile, or the samples
    size_t walker = 0;
    if (binned) {
        first = unit * A.site_tile;
        last = first + A.site_tile < A.rows ? first + A.site_tile : A.rows;
    } else {
        first = 0;
        last = A.nsamples;
        walker = A.walker_at ? (size_t)A.walker_at[unit] : (size_t)unit;
    }
    int cur = -1, pending = 0; // (uniform over the workgroup, like everything the loop branches on)
    for (long long i = first; i < last; ++i) {
        size_t row;
        int key;
        if (binned) {
            row = (size_t)i;
            key = __builtin_amdgcn_readfirstlane(A.row_key[i]);
            if (key < 0) continue; // outside the bins: the row touches nothing
        } else {
            row = (size_t)i * A.R + walker;
            key = (int)unit;
        }
        if (cur >= 0 && (key != cur || pending == ST_SITE_FLUSH)) {
            stat_sites_flush(A, cur, m_first, binned, lo, hi, over);
            pending = 0;
        }
        cur = key;
        ++pending;
        const uint8_t *bytes = A.occ + row * (size_t)A.Npad;
#pragma unroll
        for (int j = 0; j < ST_SITE_OWN; ++j) {
            const unsigned c = bytes[at[j]];
            const bool live = m_first + j * ST_THREADS < A.M, inside = c < (unsigned)A.S;
            const uint64_t one = (uint64_t)1 << ((c & 7) * 8);
            lo[j] += live && inside && c < 8 ? one : 0;
            hi[j] += live && inside && c >= 8 ? one : 0;
            over += live && !inside;
        }
    }
    if (cur >= 0) stat_sites_flush(A, cur, m_first, binned, lo, hi, over);
}

// ---- the joint field --------------------------------------------------------------------------------------------------------
// the cell of a value on an axis of n cells, or -1: below min, at or beyond min + n bin, or not finite (the rule of the
// histogram)
__device__ __forceinline__ int stat_joint_cell(double xv, double vmin, double vbin, int n) {
#pragma clang fp contract(off)
    const double d = xv - vmin;
    const double q = floordiv_exact(d, vbin);
    if (!(fabs(xv) <= 1.7976931348623157e308) || !(q == q)) return -1; // (not finite)
    // d < 0 on its own account: for -ulp(vbin) / 2 <= d < 0 the remainder d + vbin of floordiv_exact rounds to vbin and q
    // comes out 0, where the floor is -1 (the one case in which it is not np.floor_divide: |d| < vbin, d < 0)
    if (d < 0.0 || q < 0.0 || q >= (double)n) return -1;
    return (int)q;
}

// mode 4 of statistics_kernel
__device__ __forceinline__ void statistics_joint(const StatArgs &A) {
    const long long unit = (long long)blockIdx.x * ST_THREADS + threadIdx.x; // a key, or a row
    const int src_a = A.columns[A.joint_col_a], src_b = A.columns[A.joint_col_b];
    const size_t cells = (size_t)A.joint_n_a * (size_t)A.joint_n_b;
    if (A.row_key == nullptr) { // (uniform over the launch) the key's only owner: plain adds
        if (unit >= A.n_keys) return;
        const size_t walker = A.walker_at ? (size_t)A.walker_at[unit] : (size_t)unit;
        unsigned long long *mine = A.joint + (size_t)unit * cells;
        unsigned long long out = 0;
        for (long long s = 0; s < A.nsamples; ++s) {
            const size_t row = (size_t)s * A.R + walker;
            const int qa = stat_joint_cell(stat_column(A, row, src_a), A.joint_min_a, A.joint_bin_a, A.joint_n_a);
            const int qb = stat_joint_cell(stat_column(A, row, src_b), A.joint_min_b, A.joint_bin_b, A.joint_n_b);
            if (qa >= 0 && qb >= 0) mine[(size_t)qa * A.joint_n_b + qb] += 1;
            else ++out;
        }
        if (out) A.joint_out[unit] += out;
        return;
    }
    // keyed by bin: every lane of the wave stays to the end (the rounds below are wave-wide)
    const int key = unit < A.rows ? A.row_key[unit] : -1;
    bool waiting = key >= 0; // rows outside the bins touch nothing
    unsigned long long target = 0; // the row's counter, counted from `joint`
    if (waiting) {
        const int qa = stat_joint_cell(stat_column(A, (size_t)unit, src_a), A.joint_min_a, A.joint_bin_a, A.joint_n_a);
        const int qb = stat_joint_cell(stat_column(A, (size_t)unit, src_b), A.joint_min_b, A.joint_bin_b, A.joint_n_b);
        target = qa >= 0 && qb >= 0 ? (unsigned long long)key * cells + (size_t)qa * A.joint_n_b + qb
                                    : (unsigned long long)(A.joint_out - A.joint) + (unsigned long long)key;
    }
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < ST_JOINT_ROUNDS; ++round) {
        const unsigned long long todo = __ballot(waiting);
        if (!todo) break; // (uniform over the wave)
        const int first = __ffsll((long long)todo) - 1;
        const unsigned long long named = __shfl(target, first);
        const bool same = waiting && target == named;
        const unsigned long long mask = __ballot(same);
        if (lane == first) atomicAdd(A.joint + named, (unsigned long long)__popcll(mask));
        waiting = waiting && !same;
    }
    if (waiting) atomicAdd(A.joint + target, 1ull);
}

__global__ void __launch_bounds__(ST_THREADS) statistics_kernel(const StatArgs A) {
    // Every product and every sum is rounded on its own, as NumPy does it (see weighted_value_rn, smolmc_common.h).
#pragma clang fp contract(off)
    __shared__ double s_x[ST_CHUNK * ST_MAXC];
    __shared__ double s_shift[ST_MAXC];
    __shared__ double s_pend[ST_MAXL * ST_MAXC], s_b2[ST_MAXL * ST_MAXC];
    __shared__ long long s_nb[ST_MAXL];
    static_assert(ST_QUEUE * sizeof(int) <= sizeof(s_pend) && ST_WAVES * sizeof(int) <= sizeof(s_nb), "the queue of the binned mode");
    if (__builtin_expect(A.mode != 0, 0)) { // (uniform over the launch) one test in front of mode 0, the others' code behind it
        if (A.mode == ST_MODE_KEYS) stat_bin_keys(A);
        else if (A.mode == ST_MODE_BINNED)
            statistics_binned(A, s_x, s_shift, reinterpret_cast<int *>(s_pend), reinterpret_cast<int *>(s_nb));
        else if (A.mode == ST_MODE_SITES) statistics_sites(A);
        else if (A.mode == ST_MODE_JOINT) statistics_joint(A);
        return;
    }
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


// the site field's launch, behind the launches of `A` on the handle's stream (a binned record: behind its key pass, whose
// row keys it reads)
static int stat_sites_launch(smolmc_handle *h, StatArgs A, const uint8_t *d_occ8) {
    SmolmcStat &S = h->stats;
    A.mode = ST_MODE_SITES;
    A.occ = d_occ8; A.site_idx = S.site_idx; A.site_counts = S.site_counts; A.site_over = (unsigned long long *)S.site_over;
    A.Npad = h->Npad; A.M = S.site_M; A.S = S.site_S;
    const size_t chunks = ((size_t)S.site_M + ST_SITE_OWN * ST_THREADS - 1) / (ST_SITE_OWN * ST_THREADS);
    size_t units = (size_t)S.n_keys; // a key per unit, or a tile of rows
    if (S.key == SMOLMC_STAT_BY_BIN) {
        // long tiles make few atomics where a key is crowded, short ones fill the device: about 2^19 threads in all
        const size_t fill = ((size_t)A.rows * chunks * ST_THREADS) >> 19;
        A.site_tile = (int)std::min<size_t>(ST_SITE_FLUSH, std::max<size_t>(ST_SITE_TILE_MIN, fill));
        units = ((size_t)A.rows + A.site_tile - 1) / A.site_tile;
    }
    if (units * chunks > 0x7fffffffull) return fail("statistics: the site field's launch has more than 2^31 workgroups");
    if (!S.site_ev[0])
        for (hipEvent_t &e : S.site_ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(S.site_ev[0], h->stream));
    hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)(units * chunks)), dim3(ST_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.site_ev[1], h->stream));
    return 0;
}

// the joint field's launch, behind the launches of `A` on the handle's stream (a binned record: behind its key pass, whose
// row keys it reads)
static int stat_joint_launch(smolmc_handle *h, StatArgs A) {
    SmolmcStat &S = h->stats;
    A.mode = ST_MODE_JOINT;
    A.n_keys = S.n_keys;
    A.joint = (unsigned long long *)S.joint; A.joint_out = (unsigned long long *)S.joint_out;
    A.joint_col_a = S.joint_col[0]; A.joint_n_a = S.joint_n[0]; A.joint_min_a = S.joint_min[0]; A.joint_bin_a = S.joint_bin[0];
    A.joint_col_b = S.joint_col[1]; A.joint_n_b = S.joint_n[1]; A.joint_min_b = S.joint_min[1]; A.joint_bin_b = S.joint_bin[1];
    const size_t units = S.key == SMOLMC_STAT_BY_BIN ? (size_t)A.rows : (size_t)S.n_keys; // a row or a key per thread
    if (!S.joint_ev[0])
        for (hipEvent_t &e : S.joint_ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(S.joint_ev[0], h->stream));
    hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)((units + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.joint_ev[1], h->stream));
    return 0;
}

// the fields of the record, each a launch of its own behind the record's
static int stat_fields_launch(smolmc_handle *h, const StatArgs &A, const uint8_t *d_occ8) {
    if (h->stats.site_S) TRY(stat_sites_launch(h, A, d_occ8));
    if (h->stats.joint_n[0]) TRY(stat_joint_launch(h, A));
    return 0;
}

int smolmc_stat_launch(smolmc_handle *h, const double *d_H, const double *d_feat, const int32_t *d_counts, const double *d_inten,
                       const long long *d_conn, const int32_t *d_pat, const int32_t *d_env, long long nsamples,
                       const uint8_t *d_occ8) {
    SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("no statistics record set (smolmc_set_statistics)");
    if (S.n_count_cols && !d_counts) return fail("statistics: a record with count columns needs the kind counts of the rows");
    if (S.n_inten_cols && !d_inten) return fail("statistics: a record with intensity columns needs the intensities of the rows");
    if (S.n_conn_cols && !d_conn) return fail("statistics: a record with connectivity columns needs the connectivity stats of the rows");
    if (S.n_pat_cols && !d_pat) return fail("statistics: a record with pattern columns needs the pattern cells of the rows");
    if (S.n_env_cols && !d_env) return fail("statistics: a record with environment columns needs the environment cells of the rows");
    if (S.site_S && !d_occ8) return fail("statistics: a record with a site field needs the occupancy of the rows");
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
    if (S.key == SMOLMC_STAT_BY_BIN) {
        const size_t rows = (size_t)nsamples * h->R;
        if (rows > S.row_cap) { // (the scratch grows to the largest launch so far; hipFree waits for the launches that read it)
            if (S.row_key) HIPCHK(hipFree(S.row_key));
            S.row_key = nullptr;
            S.row_cap = 0;
            HIPCHK(hipMalloc((void **)&S.row_key, rows * 4));
            S.row_cap = rows;
        }
        A.row_key = S.row_key; A.cnt = S.bin_cnt; A.outside = (unsigned long long *)S.outside;
        A.key_min = S.key_min; A.key_bin = S.key_bin; A.key_column = S.key_column; A.n_keys = S.n_keys;
        A.rows = (long long)rows;
        HIPCHK(hipMemsetAsync(S.bin_cnt, 0, (size_t)S.n_keys * 4, h->stream));
        HIPCHK(hipEventRecord(S.ev[0], h->stream));
        A.mode = ST_MODE_KEYS;
        hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)((rows + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0,
                           h->stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S.ev[2], h->stream));
        A.mode = ST_MODE_BINNED;
        hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)S.n_keys), dim3(ST_THREADS), 0, h->stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S.ev[1], h->stream));
        return S.site_S || S.joint_n[0] ? stat_fields_launch(h, A, d_occ8) : 0;
    }
    HIPCHK(hipEventRecord(S.ev[0], h->stream));
    hipLaunchKernelGGL(statistics_kernel, dim3((unsigned)S.n_keys), dim3(ST_THREADS), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], h->stream));
    return S.site_S || S.joint_n[0] ? stat_fields_launch(h, A, d_occ8) : 0;
}

// the field of the record goes (smolmc_set_statistics_sites with n_codes = 0, a new spec, the handle's end)
static void stat_sites_free(SmolmcStat &S) {
    if (S.site_arena) hipFree(S.site_arena);
    for (hipEvent_t &e : S.site_ev) {
        if (e) hipEventDestroy(e);
        e = nullptr;
    }
    S.site_arena = nullptr;
    S.site_counts = S.site_over = nullptr;
    S.site_idx = nullptr;
    S.site_M = S.site_S = 0;
    S.site_bytes = 0;
}

// likewise the joint field (smolmc_set_statistics_joint with n_a = 0, a new spec, the handle's end)
static void stat_joint_free(SmolmcStat &S) {
    if (S.joint_arena) hipFree(S.joint_arena);
    for (hipEvent_t &e : S.joint_ev) {
        if (e) hipEventDestroy(e);
        e = nullptr;
    }
    S.joint_arena = nullptr;
    S.joint = S.joint_out = nullptr;
    S.joint_col[0] = S.joint_col[1] = S.joint_n[0] = S.joint_n[1] = 0;
    S.joint_min[0] = S.joint_min[1] = S.joint_bin[0] = S.joint_bin[1] = 0.0;
    S.joint_bytes = 0;
}

void smolmc_stat_free(smolmc_handle *h) {
    SmolmcStat &S = h->stats;
    if (S.arena) hipFree(S.arena);
    if (S.row_key) hipFree(S.row_key);
    stat_sites_free(S);
    stat_joint_free(S);
    for (hipEvent_t e : S.ev)
        if (e) hipEventDestroy(e);
    S = SmolmcStat();
}

// the binned part of a spec (smolmc_set_statistics_binned)
struct StatBins {
    int key_column, n_keys;
    double key_min, key_bin;
};

// smolmc_set_statistics (bins null) and smolmc_set_statistics_binned: every check, then the arena
static int stat_set(smolmc_handle *h, const smolmc_statistics *s, const StatBins *bins) {
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
    if (bins && s->key != SMOLMC_STAT_BY_BIN) {
        snprintf(msg, sizeof msg, "statistics: a binned record has key 2 (by bin), got %d", s->key);
        return fail(msg);
    }
    if (!bins && s->key != SMOLMC_STAT_BY_WALKER && s->key != SMOLMC_STAT_BY_STATE_POINT) {
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
    if (bins) { // (the key is the row's value, not the walker: per-walker Wang-Landau windows do not matter)
        if (s->n_levels != 0) {
            snprintf(msg, sizeof msg, "statistics: a record keyed by bin keeps no blocking sums (successive rows of a key come "
                     "from different walkers): n_levels must be 0, got %d", s->n_levels);
            return fail(msg);
        }
        if (bins->n_keys < 1 || bins->n_keys > SMOLMC_MAX_STAT_KEYS) {
            snprintf(msg, sizeof msg, "statistics: n_keys must be 1..%d, got %d", SMOLMC_MAX_STAT_KEYS, bins->n_keys);
            return fail(msg);
        }
        if (!(bins->key_bin > 0.0) || !std::isfinite(bins->key_bin) || !std::isfinite(bins->key_min))
            return fail("statistics: key_bin must be a positive finite number and key_min finite");
        if (bins->key_column < 0 || bins->key_column >= C) {
            snprintf(msg, sizeof msg, "statistics: key_column = %d is no index into the %d columns", bins->key_column, C);
            return fail(msg);
        }
    }
    const size_t nk = bins ? (size_t)bins->n_keys : (size_t)h->R;
    const size_t L = (size_t)s->n_levels, B = (size_t)s->n_bins, P = (size_t)C * (C + 1) / 2;
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
    if (bins) {
        S.key_column = bins->key_column; S.key_min = bins->key_min; S.key_bin = bins->key_bin;
    }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
    const size_t o_n = take(nk * 8), o_under = take(nk * 8), o_over = take(nk * 8), o_shift = take(nk * C * 8),
                 o_s1 = take(nk * C * 8), o_s2 = take(nk * P * 8), o_has = take(nk * C * 8), o_pend = take(nk * L * C * 8),
                 o_b2 = take(nk * L * C * 8), o_nb = take(nk * L * 8), o_hist = take(nk * B * 8), o_outside = take(16);
    S.record_bytes = at;
    const size_t o_col = take((size_t)C * 4), o_w = take((size_t)s->n_weights * 8), o_ucnt = take((size_t)h->R * (size_t)K * 4),
                 o_bcnt = take(bins ? nk * 4 : 0);
    HIPCHK(hipMalloc((void **)&S.arena, at));
    unsigned char *d = S.arena;
    S.n = (long long *)(d + o_n); S.under = (long long *)(d + o_under); S.over = (long long *)(d + o_over);
    S.shift = (double *)(d + o_shift); S.s1 = (double *)(d + o_s1); S.s2 = (double *)(d + o_s2); S.has = (uint64_t *)(d + o_has);
    S.pend = (double *)(d + o_pend); S.b2 = (double *)(d + o_b2); S.nb = (long long *)(d + o_nb); S.hist = (long long *)(d + o_hist);
    S.columns = (int32_t *)(d + o_col); S.weights = (double *)(d + o_w); S.u_counts = (int32_t *)(d + o_ucnt);
    S.outside = (long long *)(d + o_outside); S.bin_cnt = (int32_t *)(d + o_bcnt);
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

extern "C" int smolmc_set_statistics(smolmc_handle *h, const smolmc_statistics *s) { return stat_set(h, s, nullptr); }

extern "C" int smolmc_set_statistics_binned(smolmc_handle *h, const smolmc_statistics *s, int key_column, int n_keys,
                                            double key_min, double key_bin) {
    if (!s) return fail("statistics: null spec (smolmc_set_statistics removes a record)");
    const StatBins bins = {key_column, n_keys, key_min, key_bin};
    return stat_set(h, s, &bins);
}

extern "C" int smolmc_statistics_bins(smolmc_handle *h, int *key_column, int *n_keys, double *key_min, double *key_bin,
                                      int64_t *key_under, int64_t *key_over) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    const bool binned = S.n_keys && S.key == SMOLMC_STAT_BY_BIN;
    long long outside[2] = {0, 0};
    if (binned && (key_under || key_over)) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(outside, S.outside, 16, hipMemcpyDeviceToHost));
    }
    if (key_column) *key_column = binned ? S.key_column : 0;
    if (n_keys) *n_keys = binned ? S.n_keys : 0;
    if (key_min) *key_min = binned ? S.key_min : 0.0;
    if (key_bin) *key_bin = binned ? S.key_bin : 0.0;
    if (key_under) *key_under = outside[0];
    if (key_over) *key_over = outside[1];
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
    if (S.site_S) HIPCHK(hipMemset(S.site_arena, 0, S.site_bytes));
    if (S.joint_n[0]) HIPCHK(hipMemset(S.joint_arena, 0, S.joint_bytes));
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

// ---- the site field: how often every tracked site held every code, per key ----------------------------------------------
extern "C" int smolmc_set_statistics_sites(smolmc_handle *h, const int32_t *sites, int n_sites, int n_codes) {
    if (!h) return fail("null handle");
    SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("statistics sites: no statistics record set (call smolmc_set_statistics first)");
    char msg[256];
    if (n_codes < 0 || n_codes > SMOLMC_MAX_STAT_SITE_CODES) {
        snprintf(msg, sizeof msg, "statistics sites: n_codes must be 0..%d, got %d", SMOLMC_MAX_STAT_SITE_CODES, n_codes);
        return fail(msg);
    }
    const int N = h->N, M = sites ? n_sites : N;
    if (n_codes && sites) {
        if (n_sites < 1) {
            snprintf(msg, sizeof msg, "statistics sites: a list of %d sites (NULL tracks all %d)", n_sites, N);
            return fail(msg);
        }
        std::vector<int32_t> seen((size_t)N, -1);
        for (int m = 0; m < n_sites; ++m) {
            const int p = sites[m];
            if (p < 0 || p >= N) {
                snprintf(msg, sizeof msg, "statistics sites: entry %d is site %d, outside 0..%d", m, p, N - 1);
                return fail(msg);
            }
            if (seen[p] >= 0) {
                snprintf(msg, sizeof msg, "statistics sites: site %d is listed twice (entries %d and %d)", p, (int)seen[p], m);
                return fail(msg);
            }
            seen[p] = m;
        }
    }
    const size_t nk = (size_t)S.n_keys;
    const size_t o_over = up256(nk * (size_t)M * (size_t)n_codes * 8), o_idx = o_over + up256(nk * 8);
    if (n_codes && S.record_bytes + S.joint_bytes + o_idx > ((size_t)1 << 30)) { // (joint_bytes: the joint field in force)
        snprintf(msg, sizeof msg, "statistics sites: a record of %zu bytes and a field of %zu keys x %d sites x %d codes are larger than "
                 "1 GiB", S.record_bytes, nk, M, n_codes);
        return fail(msg);
    }
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_STATISTICS, "smolmc_set_statistics_sites", "SMOLMC_SAMPLE_STATISTICS"));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream)); // (queued launches still add to the field in force)
    if (!n_codes) {
        stat_sites_free(S);
        return 0;
    }
    // all sites of a handle that is not relabelled: tracked site m is byte m, no list on the device
    std::vector<int32_t> idx;
    if (sites || h->relabelled) {
        idx.resize((size_t)M);
        for (int m = 0; m < M; ++m) {
            const int p = sites ? sites[m] : m;
            idx[(size_t)m] = h->relabelled ? h->new_of[p] : p;
        }
    }
    unsigned char *arena = nullptr;
    HIPCHK(hipMalloc((void **)&arena, o_idx + up256((size_t)M * 4)));
    hipError_t e = hipMemset(arena, 0, o_idx); // (an empty field is all zeros)
    if (e == hipSuccess && !idx.empty()) e = hipMemcpy(arena + o_idx, idx.data(), (size_t)M * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        hipFree(arena);
        return fail(std::string("statistics sites upload: ") + hipGetErrorString(e));
    }
    stat_sites_free(S);
    S.site_arena = arena;
    S.site_bytes = o_idx;
    S.site_counts = (long long *)arena;
    S.site_over = (long long *)(arena + o_over);
    S.site_idx = idx.empty() ? nullptr : (int32_t *)(arena + o_idx);
    S.site_M = M;
    S.site_S = n_codes;
    return 0;
}

extern "C" int smolmc_statistics_sites_shape(smolmc_handle *h, int *n_sites, int *n_codes) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (n_sites) *n_sites = S.site_S ? S.site_M : 0;
    if (n_codes) *n_codes = S.site_S;
    return 0;
}

extern "C" int smolmc_get_statistics_sites(smolmc_handle *h, int64_t *site_counts, int64_t *site_over) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (!S.site_S) return fail("no site field set: call smolmc_set_statistics_sites first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nk = (size_t)S.n_keys, M = (size_t)S.site_M, NC = (size_t)S.site_S;
    if (site_counts) { // the device keeps a key's counters code-major, the caller gets them site-major
        std::vector<int64_t> dev(nk * M * NC);
        HIPCHK(hipMemcpy(dev.data(), S.site_counts, nk * M * NC * 8, hipMemcpyDeviceToHost));
        auto work = [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k)
                for (size_t c = 0; c < NC; ++c) {
                    const int64_t *src = dev.data() + (k * NC + c) * M;
                    int64_t *dst = site_counts + k * M * NC + c;
                    for (size_t m = 0; m < M; ++m) dst[m * NC] = src[m];
                }
        };
        const int nt = 4;
        if (nk * M * NC < ((size_t)1 << 20) || nk < (size_t)nt) work(0, nk);
        else {
            std::thread th[nt];
            for (int t = 0; t < nt; ++t) th[t] = std::thread(work, nk * t / nt, nk * (t + 1) / nt);
            for (int t = 0; t < nt; ++t) th[t].join();
        }
    }
    if (site_over) HIPCHK(hipMemcpy(site_over, S.site_over, nk * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the joint field: the rows of every key in the cells of two columns ---------------------------------------------------
extern "C" int smolmc_set_statistics_joint(smolmc_handle *h, int column_a, int n_a, double min_a, double bin_a, int column_b, int n_b,
                                           double min_b, double bin_b) {
    if (!h) return fail("null handle");
    SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("statistics joint: no statistics record set (call smolmc_set_statistics first)");
    char msg[256];
    if (n_a < 0 || n_a > SMOLMC_MAX_STAT_JOINT_CELLS) {
        snprintf(msg, sizeof msg, "statistics joint: n_a must be 0..%d, got %d", SMOLMC_MAX_STAT_JOINT_CELLS, n_a);
        return fail(msg);
    }
    size_t o_out = 0, bytes = 0;
    if (n_a) {
        if (n_b < 1 || n_b > SMOLMC_MAX_STAT_JOINT_CELLS) {
            snprintf(msg, sizeof msg, "statistics joint: n_b must be 1..%d, got %d", SMOLMC_MAX_STAT_JOINT_CELLS, n_b);
            return fail(msg);
        }
        if (!(bin_a > 0.0) || !std::isfinite(bin_a) || !std::isfinite(min_a))
            return fail("statistics joint: bin_a must be a positive finite number and min_a finite");
        if (!(bin_b > 0.0) || !std::isfinite(bin_b) || !std::isfinite(min_b))
            return fail("statistics joint: bin_b must be a positive finite number and min_b finite");
        if (column_a < 0 || column_a >= S.C) {
            snprintf(msg, sizeof msg, "statistics joint: column_a = %d is no index into the %d columns", column_a, S.C);
            return fail(msg);
        }
        if (column_b < 0 || column_b >= S.C) {
            snprintf(msg, sizeof msg, "statistics joint: column_b = %d is no index into the %d columns", column_b, S.C);
            return fail(msg);
        }
        const size_t nk = (size_t)S.n_keys;
        o_out = up256(nk * (size_t)n_a * (size_t)n_b * 8); // (at most 2^51)
        bytes = o_out + up256(nk * 8);
        if (S.record_bytes + S.site_bytes + bytes > ((size_t)1 << 30)) {
            snprintf(msg, sizeof msg, "statistics joint: a record of %zu bytes, a site field of %zu bytes and a joint field of %zu keys x "
                     "%d x %d cells are larger than 1 GiB", S.record_bytes, S.site_bytes, nk, n_a, n_b);
            return fail(msg);
        }
    }
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_STATISTICS, "smolmc_set_statistics_joint", "SMOLMC_SAMPLE_STATISTICS"));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream)); // (queued launches still add to the field in force)
    if (!n_a) {
        stat_joint_free(S);
        return 0;
    }
    unsigned char *arena = nullptr;
    HIPCHK(hipMalloc((void **)&arena, bytes));
    hipError_t e = hipMemset(arena, 0, bytes); // (an empty field is all zeros)
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        hipFree(arena);
        return fail(std::string("statistics joint: ") + hipGetErrorString(e));
    }
    stat_joint_free(S);
    S.joint_arena = arena;
    S.joint_bytes = bytes;
    S.joint = (long long *)arena;
    S.joint_out = (long long *)(arena + o_out);
    S.joint_col[0] = column_a; S.joint_n[0] = n_a; S.joint_min[0] = min_a; S.joint_bin[0] = bin_a;
    S.joint_col[1] = column_b; S.joint_n[1] = n_b; S.joint_min[1] = min_b; S.joint_bin[1] = bin_b;
    return 0;
}

extern "C" int smolmc_statistics_joint_shape(smolmc_handle *h, int *column_a, int *n_a, double *min_a, double *bin_a, int *column_b,
                                             int *n_b, double *min_b, double *bin_b) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (column_a) *column_a = S.joint_col[0];
    if (n_a) *n_a = S.joint_n[0];
    if (min_a) *min_a = S.joint_min[0];
    if (bin_a) *bin_a = S.joint_bin[0];
    if (column_b) *column_b = S.joint_col[1];
    if (n_b) *n_b = S.joint_n[1];
    if (min_b) *min_b = S.joint_min[1];
    if (bin_b) *bin_b = S.joint_bin[1];
    return 0;
}

extern "C" int smolmc_get_statistics_joint(smolmc_handle *h, int64_t *joint, int64_t *joint_out) {
    if (!h) return fail("null handle");
    const SmolmcStat &S = h->stats;
    if (!S.joint_n[0]) return fail("no joint field set: call smolmc_set_statistics_joint first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nk = (size_t)S.n_keys;
    if (joint) HIPCHK(hipMemcpy(joint, S.joint, nk * (size_t)S.joint_n[0] * (size_t)S.joint_n[1] * 8, hipMemcpyDeviceToHost));
    if (joint_out) HIPCHK(hipMemcpy(joint_out, S.joint_out, nk * 8, hipMemcpyDeviceToHost));
    return 0;
}

// elapsed device time of the joint field's last launch in ms (tools/statistics_joint_timing.py); a measuring hook like the
// ones below, not part of the C-ABI
extern "C" int smolmc_debug_statistics_joint_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcStat &S = h->stats;
    if (!S.joint_ev[0]) return fail("the joint field's kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.joint_ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.joint_ev[0], S.joint_ev[1]));
    return 0;
}

// elapsed device time of the site field's last launch in ms (tools/statistics_sites_timing.py); a measuring hook like the
// two below, not part of the C-ABI
extern "C" int smolmc_debug_statistics_sites_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcStat &S = h->stats;
    if (!S.site_ev[0]) return fail("the site field's kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.site_ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.site_ev[0], S.site_ev[1]));
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

// the same for a binned record, per launch: ms[0] the key pass (mode 1), ms[1] the reduction per key (mode 2)
extern "C" int smolmc_debug_statistics_bins_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcStat &S = h->stats;
    if (!S.ev[0] || S.key != SMOLMC_STAT_BY_BIN) return fail("the binned statistics kernels have not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.ev[0], S.ev[2]));
    HIPCHK(hipEventElapsedTime(ms + 1, S.ev[2], S.ev[1]));
    return 0;
}
