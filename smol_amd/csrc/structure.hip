// Structure factors of recorded states (smolmc_set_structure, smolmc_eval_structure, SMOLMC_SAMPLE_STRUCTURE):
// fixed-point amplitudes per wave vector ("point") and kind, and the intensities made of them, reduced on the device
// where the occupancy rows lie.  A translation unit of its own, like observables.hip.
//
// The kind of (site, code) is kind_base[site] + code, kind_base[site] < 0 leaves the site out; phase[q][site] < M is the
// site's phase class at point q and table[q][m] = (cos, -sin) in fixed point (structure.StructureFactor.evaluate
// is the same in NumPy).  Per row:
//   amp[q][k][c] = sum over counted sites j of kind k of table[q][phase[q][j]][c]                      (int64)
//   inten[i]     = ((double)amp[q][a][0] * (double)amp[q][b][0] + (double)amp[q][a][1] * (double)amp[q][b][1]) * scale[i]
// The sums are integer sums: any order or decomposition gives the same bits.  Both kernels use that: per point they COUNT
// the sites of every (kind, phase class) cell and then form sum_m count[k][m] * table[q][m], K x M products per point
// instead of a table lookup and two 64-bit adds per site.  No global atomics, no scratch.  The intensities are the
// kernels' epilogue, every product and sum rounded on its own.
//
// structure_mask_kernel -- a point has at most SF_MASK_CELLS cells (the Gamma point, the superlattice points of an alloy,
// every commensurate point of a cubic cell with a few kinds).  Counting is popcount: the engine keeps, for every (point,
// class), the class's sites as bits (masks [W x M x Q], W = words of 64 sites); a workgroup turns SF_MROWS occupancy rows
// into bit masks per kind in LDS ([rows][K][W], one ballot per kind and word) and thread (k, q) walks the classes and
// words: count[k][m] = sum_w popcount(mask[w][m][q] & kind[k][w]).  Lanes are consecutive points, so a mask load is one
// contiguous line per wave and the kind word is an LDS broadcast; every mask word loaded serves SF_MROWS rows.  A thread
// owns its amplitudes from the first add to the store: no atomics of any kind, no reduction.
//
// structure_kernel -- more cells.  One workgroup per row.  The row's Npad bytes go to LDS with 16-byte loads and are
// turned into kinds in place (0xff: not counted).  The points are taken in chunks of as many as fit LDS next to the row
// (smolmc_sfac_plan); every wave adds into a counter set of its own (LDS adds) -- one shared set when SF_WAVES of them do
// not fit -- and one thread per amplitude folds the sets.
#include "smolmc_common.h"

#define SF_THREADS 256
#define SF_WAVES (SF_THREADS / 64)
#define SF_MASK_CELLS 128
#define SF_MROWS 4
#define SF_NOKIND 0xffu
#define SF_LDS_BYTES (64 * 1024)

struct SfArgs {
    const uint8_t *occ;        // rows of Npad bytes
    const int32_t *kind_base;  // [N], engine numbering
    const uint16_t *phase;     // [Q x N], engine numbering
    const unsigned long long *masks; // [W x M x Q] (mask kernel)
    const long long *table;    // [Q x M x 2]
    const int32_t *intensity;  // [I x 3]
    const double *scale;       // [I]
    long long *amp;            // [rows x Q x K x 2]
    double *inten;             // [rows x I]
    size_t rows;
    int N, Npad, K, M, Q, I, W;
    int copies, chunk;         // counter kernel: counter sets per point in LDS (SF_WAVES or 1), points per pass
};

// mask kernel, LDS: kind masks u64 [SF_MROWS][K][W]
// counter kernel, LDS: kinds u8 [Npad] | counters i32 [chunk][copies][K x M]
bool smolmc_sfac_plan(int N, int Npad, int K, int M, int Q, int *mask, int *copies, int *chunk, size_t *lds) {
    const size_t cells = (size_t)K * M, W = ((size_t)N + 63) / 64;
    *mask = 0;
    *copies = 1;
    *chunk = 1;
    if (cells <= SF_MASK_CELLS && SF_MROWS * K * W * 8 <= SF_LDS_BYTES) {
        *mask = 1;
        *lds = SF_MROWS * K * W * 8;
        return true;
    }
    if ((size_t)Npad + cells * 4 > SF_LDS_BYTES) return false;
    const int cp = (size_t)Npad + SF_WAVES * cells * 4 <= SF_LDS_BYTES ? SF_WAVES : 1;
    const size_t per_point = (size_t)cp * cells * 4;
    const size_t fit = (SF_LDS_BYTES - (size_t)Npad) / per_point;
    const int ch = (int)std::min<size_t>(fit, (size_t)Q);
    *copies = cp;
    *chunk = ch;
    *lds = (size_t)Npad + (size_t)ch * per_point;
    return true;
}

// the intensities of one row from its amplitudes, threads tid, tid + stride, ... of the caller
__device__ __forceinline__ void sf_intensities(const SfArgs &A, size_t row, int first, int stride) {
    // Every product and every sum is rounded on its own, as NumPy does it (see weighted_value_rn, smolmc_common.h).
#pragma clang fp contract(off)
    const long long *amp = A.amp + row * (size_t)A.Q * A.K * 2;
    for (int i = first; i < A.I; i += stride) {
        const int q = A.intensity[3 * i], a = A.intensity[3 * i + 1], b = A.intensity[3 * i + 2];
        const long long *pa = amp + ((size_t)q * A.K + a) * 2, *pb = amp + ((size_t)q * A.K + b) * 2;
        const double re = (double)pa[0] * (double)pb[0];
        const double im = (double)pa[1] * (double)pb[1];
        const double sum = re + im;
        A.inten[row * (size_t)A.I + i] = sum * A.scale[i];
    }
}

__global__ void __launch_bounds__(SF_THREADS) structure_mask_kernel(const SfArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = A.N, K = A.K, M = A.M, Q = A.Q, W = A.W;
    unsigned long long *km = (unsigned long long *)sf_smem; // [SF_MROWS][K][W]
    const size_t row0 = (size_t)blockIdx.x * SF_MROWS;
    const int nr = A.rows - row0 < SF_MROWS ? (int)(A.rows - row0) : SF_MROWS;

    // the rows as bit masks per kind: a wave per (row, word), one ballot per kind, lane c keeps the mask of kind c
    // (K <= SF_MASK_CELLS; a row beyond the last one gives empty masks)
    for (int item = wave; item < SF_MROWS * W; item += SF_WAVES) { // (wave-uniform: every lane takes part in the ballots)
        const int r = item / W, w = item - r * W, s = w * 64 + lane;
        unsigned k = SF_NOKIND;
        if (r < nr && s < N) {
            const int kb = A.kind_base[s];
            if (kb >= 0) k = (unsigned)kb + A.occ[(row0 + r) * A.Npad + s];
            if (k >= (unsigned)K) k = SF_NOKIND; // (a code the site's block has no kind for: see observables.hip)
        }
        for (int c0 = 0; c0 < K; c0 += 64) {
            unsigned long long keep = 0;
            const int cn = K - c0 < 64 ? K - c0 : 64;
            for (int c = 0; c < cn; ++c) {
                const unsigned long long b = __ballot(k == (unsigned)(c0 + c));
                if (lane == c) keep = b;
            }
            if (lane < cn) km[((size_t)r * K + c0 + lane) * W + w] = keep;
        }
    }
    __syncthreads();
    // thread (k, q): count[k][m] by popcount, amp += count * table, for SF_MROWS rows at once
    const size_t MQ = (size_t)M * Q;
    for (int t = tid; t < Q * K; t += SF_THREADS) {
        const int k = t / Q, q = t - k * Q;
        long long acc[SF_MROWS][2];
#pragma unroll
        for (int r = 0; r < SF_MROWS; ++r) acc[r][0] = acc[r][1] = 0;
        for (int m = 0; m < M; ++m) {
            int cnt[SF_MROWS];
#pragma unroll
            for (int r = 0; r < SF_MROWS; ++r) cnt[r] = 0;
            const unsigned long long *cm = A.masks + (size_t)m * Q + q;
            for (int w = 0; w < W; ++w) {
                const unsigned long long x = cm[(size_t)w * MQ];
#pragma unroll
                for (int r = 0; r < SF_MROWS; ++r) cnt[r] += __popcll(x & km[((size_t)r * K + k) * W + w]);
            }
            const long long t0 = A.table[((size_t)q * M + m) * 2], t1 = A.table[((size_t)q * M + m) * 2 + 1];
#pragma unroll
            for (int r = 0; r < SF_MROWS; ++r) {
                acc[r][0] += (long long)cnt[r] * t0;
                acc[r][1] += (long long)cnt[r] * t1;
            }
        }
#pragma unroll
        for (int r = 0; r < SF_MROWS; ++r)
            if (r < nr) {
                long long *out = A.amp + (((row0 + r) * Q + (size_t)q) * K + k) * 2;
                out[0] = acc[r][0];
                out[1] = acc[r][1];
            }
    }
    if (!A.I) return;
    __syncthreads(); // (the rows' amplitudes, written by other threads of this workgroup, are read back)
    for (int r = 0; r < nr; ++r) sf_intensities(A, row0 + r, tid, SF_THREADS);
}

__global__ void __launch_bounds__(SF_THREADS) structure_kernel(const SfArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_smem[];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int N = A.N, Npad = A.Npad, K = A.K, M = A.M, Q = A.Q;
    const int cells = K * M, per_point = A.copies * cells;
    uint8_t *kinds = sf_smem;
    int32_t *cnt = (int32_t *)(sf_smem + Npad); // (Npad is a multiple of 16)
    const size_t row = blockIdx.x;

    {   // the row, 16 bytes a lane
        const uint4 *src = (const uint4 *)(A.occ + row * Npad);
        uint4 *dst = (uint4 *)kinds;
        for (int i = tid; i < Npad / 16; i += SF_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    // codes -> kinds in place (every byte is read and written by one thread)
    for (int s = tid; s < Npad; s += SF_THREADS) {
        unsigned k = SF_NOKIND;
        if (s < N) {
            const int kb = A.kind_base[s];
            if (kb >= 0) k = (unsigned)kb + kinds[s];
            if (k >= (unsigned)K) k = SF_NOKIND; // (a code the site's block has no kind for: see observables.hip)
        }
        kinds[s] = (uint8_t)k;
    }

    for (int q0 = 0; q0 < Q; q0 += A.chunk) {
        const int nq = Q - q0 < A.chunk ? Q - q0 : A.chunk;
        __syncthreads(); // (the kinds are written; the chunk before is read out)
        for (int i = tid; i < nq * per_point; i += SF_THREADS) cnt[i] = 0;
        __syncthreads();
        for (int qi = 0; qi < nq; ++qi) {
            const uint16_t *ph = A.phase + (size_t)(q0 + qi) * N;
            int32_t *mine = cnt + qi * per_point + (A.copies > 1 ? wave * cells : 0);
            for (int s = tid; s < N; s += SF_THREADS) {
                const unsigned k = kinds[s];
                if (k != SF_NOKIND) atomicAdd(&mine[(int)k * M + (int)ph[s]], 1);
            }
        }
        __syncthreads();
        // amp[q][k][c] = sum_m count[k][m] * table[q][m][c]: one thread per entry, plain stores
        for (int t = tid; t < nq * K * 2; t += SF_THREADS) {
            const int qi = t / (K * 2), k = (t >> 1) % K, c = t & 1;
            const int32_t *hq = cnt + qi * per_point + k * M;
            const long long *tb = A.table + (size_t)(q0 + qi) * M * 2 + c;
            long long a = 0;
            for (int m = 0; m < M; ++m) {
                int n = 0;
                for (int w = 0; w < A.copies; ++w) n += hq[w * cells + m];
                a += (long long)n * tb[2 * m];
            }
            A.amp[((row * Q + (size_t)(q0 + qi)) * K + k) * 2 + c] = a;
        }
    }
    if (!A.I) return;
    __syncthreads(); // (the row's amplitudes, written by other threads of this workgroup, are read back)
    sf_intensities(A, row, tid, SF_THREADS);
}

int smolmc_sfac_launch(smolmc_handle *h, const uint8_t *d_occ8, size_t rows, long long *d_amp, double *d_inten) {
    SmolmcStruct &S = h->sfac;
    if (!S.Q) return fail("no structure-factor spec set (smolmc_set_structure)");
    if (!rows) return 0;
    if (rows > 0x7fffffffull) return fail("structure factors: more than 2^31 rows in one launch");
    if (!d_amp || (S.I && !d_inten)) return fail("structure factors: null output");
    SfArgs A;
    A.occ = d_occ8; A.kind_base = S.d_kind_base; A.phase = S.d_phase; A.masks = S.d_masks; A.table = S.d_table;
    A.rows = rows; A.W = S.W;
    A.intensity = S.d_intensity; A.scale = S.d_scale; A.amp = d_amp; A.inten = d_inten;
    A.N = h->N; A.Npad = h->Npad; A.K = S.K; A.M = S.M; A.Q = S.Q; A.I = S.I;
    A.copies = S.copies; A.chunk = S.chunk;
    if (!S.ev[0])
        for (hipEvent_t &e : S.ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(S.ev[0], h->stream));
    if (S.mask)
        hipLaunchKernelGGL(structure_mask_kernel, dim3((unsigned)((rows + SF_MROWS - 1) / SF_MROWS)), dim3(SF_THREADS), S.lds,
                           h->stream, A);
    else
        hipLaunchKernelGGL(structure_kernel, dim3((unsigned)rows), dim3(SF_THREADS), S.lds, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], h->stream));
    return 0;
}

void smolmc_sfac_free(SmolmcStruct &S) {
    if (S.arena) hipFree(S.arena);
    for (hipEvent_t e : S.ev)
        if (e) hipEventDestroy(e);
    S = SmolmcStruct();
}

// the kernel and layout of the spec in force: the mask kernel or, for the counter kernel, counter sets per point and points
// per pass (tests name the boundaries by it); a test hook like smolmc_debug_block_bytes, not part of the C-ABI
extern "C" int smolmc_debug_structure_plan(smolmc_handle *h, int *mask, int *copies, int *chunk) {
    if (!h || !mask || !copies || !chunk) return fail("null argument");
    if (!h->sfac.Q) return fail("no structure-factor spec set");
    *mask = h->sfac.mask;
    *copies = h->sfac.copies;
    *chunk = h->sfac.chunk;
    return 0;
}

// elapsed device time of the last launch of the structure kernel in ms (tools/structure_timing.py); a measuring hook like
// smolmc_debug_obs_kernel_ms, not part of the C-ABI
extern "C" int smolmc_debug_structure_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcStruct &S = h->sfac;
    if (!S.ev[0]) return fail("the structure kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.ev[0], S.ev[1]));
    return 0;
}

// ---- the C-ABI of the structure-factor spec -------------------------------------------------------------------------------
extern "C" int smolmc_set_structure(smolmc_handle *h, const smolmc_structure *sp) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_STRUCTURE, "smolmc_set_structure", "SMOLMC_SAMPLE_STRUCTURE"));
    if (h->stats.n_keys && h->stats.n_inten_cols)
        return fail("smolmc_set_structure while a statistics record with intensity columns depends on the spec (call "
                    "smolmc_set_statistics(h, NULL) first)");
    SmolmcStruct S;
    if (sp) {
        const int N = h->N, K = sp->n_kinds, Q = sp->n_points, M = sp->n_phases, I = sp->n_intensities;
        char msg[256];
        if (!sp->kind_base || !sp->phase || !sp->table || (I > 0 && (!sp->intensity || !sp->intensity_scale)))
            return fail("structure factors: null argument");
        if (K < 1 || K > 254) return fail("structure factors: n_kinds must be 1..254 (a kind is staged as one byte)");
        if (Q < 1 || Q > SMOLMC_MAX_STRUCT_POINTS) {
            snprintf(msg, sizeof msg, "structure factors: n_points must be 1..%d, got %d", SMOLMC_MAX_STRUCT_POINTS, Q);
            return fail(msg);
        }
        if (M < 1 || M > SMOLMC_MAX_STRUCT_PHASES) {
            snprintf(msg, sizeof msg, "structure factors: n_phases must be 1..%d, got %d", SMOLMC_MAX_STRUCT_PHASES, M);
            return fail(msg);
        }
        if ((size_t)K * M > SMOLMC_MAX_STRUCT_CELLS) {
            snprintf(msg, sizeof msg, "structure factors: %d kinds x %d phase classes = %zu cells, larger than SMOLMC_MAX_STRUCT_CELLS = %d",
                     K, M, (size_t)K * M, SMOLMC_MAX_STRUCT_CELLS);
            return fail(msg);
        }
        if (I < 0 || I > SMOLMC_MAX_STRUCT_INTENSITIES) {
            snprintf(msg, sizeof msg, "structure factors: n_intensities must be 0..%d, got %d", SMOLMC_MAX_STRUCT_INTENSITIES, I);
            return fail(msg);
        }
        std::vector<int32_t> kb;
        size_t n_counted = 0;
        TRY(smolmc_kind_base_in(h, sp->kind_base, K, "structure factors", kb, &n_counted));
        std::vector<uint16_t> ph((size_t)Q * N);
        for (int q = 0; q < Q; ++q)
            for (int p = 0; p < N; ++p) {
                const uint16_t v = sp->phase[(size_t)q * N + p];
                if (v >= M) {
                    snprintf(msg, sizeof msg, "structure factors: phase[%d][%d] = %d, n_phases is %d: phase out of range", q, p, (int)v, M);
                    return fail(msg);
                }
                ph[(size_t)q * N + (h->relabelled ? h->new_of[p] : p)] = v;
            }
        unsigned long long peak = 0;
        for (size_t i = 0; i < (size_t)Q * M * 2; ++i) {
            const int64_t v = sp->table[i];
            const unsigned long long a = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
            peak = std::max(peak, a);
        }
        if (n_counted && peak >= (1ull << 62) / n_counted + ((1ull << 62) % n_counted != 0)) {
            snprintf(msg, sizeof msg, "structure factors: %zu counted sites x max|table| = %llu reaches 2^62: an amplitude could overflow",
                     n_counted, peak);
            return fail(msg);
        }
        for (int i = 0; i < I; ++i) {
            const int32_t q = sp->intensity[3 * i], a = sp->intensity[3 * i + 1], b = sp->intensity[3 * i + 2];
            if (q < 0 || q >= Q) {
                snprintf(msg, sizeof msg, "structure factors: intensity %d names point %d, n_points is %d: point out of range", i, (int)q, Q);
                return fail(msg);
            }
            if (a < 0 || a >= K || b < 0 || b >= K) {
                snprintf(msg, sizeof msg, "structure factors: intensity %d names kinds (%d, %d), n_kinds is %d: kind out of range", i, (int)a,
                         (int)b, K);
                return fail(msg);
            }
            if (!std::isfinite(sp->intensity_scale[i])) {
                snprintf(msg, sizeof msg, "structure factors: intensity_scale[%d] is not finite", i);
                return fail(msg);
            }
        }
        S.K = K; S.Q = Q; S.M = M; S.I = I;
        S.W = (N + 63) / 64;
        if (!smolmc_sfac_plan(N, h->Npad, K, M, Q, &S.mask, &S.copies, &S.chunk, &S.lds)) {
            snprintf(msg, sizeof msg, "structure factors: a row of %d sites is too long to stage in LDS next to the %zu counters of a point "
                     "(%zu bytes, 65536 at most)", N, (size_t)K * M, (size_t)h->Npad + (size_t)K * M * 4);
            return fail(msg);
        }
        S.kind_base = kb;
        // one arena: the spec's arrays, then the scratch of smolmc_update_statistics
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
        const size_t R = (size_t)h->R;
        const size_t o_kb = take((size_t)N * 4), o_ph = take((size_t)Q * N * 2), o_tb = take((size_t)Q * M * 16),
                     o_it = take((size_t)I * 12), o_sc = take((size_t)I * 8), o_ua = take(R * Q * K * 16), o_ui = take(R * I * 8);
        // the mask kernel's table: for every point and class the sites of the class as bits, words of one (word, class)
        // side by side over the points
        std::vector<unsigned long long> masks;
        if (S.mask) {
            masks.assign((size_t)S.W * M * Q, 0ull);
            for (int q = 0; q < Q; ++q)
                for (int s = 0; s < N; ++s)
                    masks[((size_t)(s >> 6) * M + ph[(size_t)q * N + s]) * Q + q] |= 1ull << (s & 63);
        }
        const size_t o_mk = take(masks.size() * 8);
        hipError_t e = hipMalloc((void **)&S.arena, at);
        if (e != hipSuccess) return fail(std::string("structure factors: hipMalloc: ") + hipGetErrorString(e));
        unsigned char *d = S.arena;
        S.d_kind_base = (int32_t *)(d + o_kb); S.d_phase = (uint16_t *)(d + o_ph); S.d_table = (long long *)(d + o_tb);
        S.d_intensity = (int32_t *)(d + o_it); S.d_scale = (double *)(d + o_sc);
        S.u_amp = (long long *)(d + o_ua); S.u_inten = (double *)(d + o_ui);
        S.d_masks = (unsigned long long *)(d + o_mk);
        e = hipMemcpy(S.d_kind_base, kb.data(), (size_t)N * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(S.d_phase, ph.data(), (size_t)Q * N * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(S.d_table, sp->table, (size_t)Q * M * 16, hipMemcpyHostToDevice);
        if (e == hipSuccess && I) e = hipMemcpy(S.d_intensity, sp->intensity, (size_t)I * 12, hipMemcpyHostToDevice);
        if (e == hipSuccess && I) e = hipMemcpy(S.d_scale, sp->intensity_scale, (size_t)I * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && !masks.empty()) e = hipMemcpy(S.d_masks, masks.data(), masks.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            smolmc_sfac_free(S);
            return fail(std::string("structure factors upload: ") + hipGetErrorString(e));
        }
    }
    TRY(smolmc_ring_forget(h, SMOLMC_SAMPLE_STRUCTURE));
    smolmc_sfac_free(h->sfac);
    h->sfac = S;
    return 0;
}

extern "C" int smolmc_structure_shape(smolmc_handle *h, int *n_points, int *n_kinds, int *n_intensities) {
    if (!h) return fail("null handle");
    if (n_points) *n_points = h->sfac.Q;
    if (n_kinds) *n_kinds = h->sfac.Q ? h->sfac.K : 0;
    if (n_intensities) *n_intensities = h->sfac.I;
    return 0;
}

extern "C" int smolmc_eval_structure(smolmc_handle *h, const int32_t *occ, int nocc, int64_t *amp, double *inten) {
    if (!h) return fail("null handle");
    const SmolmcStruct &S = h->sfac;
    if (!S.Q) return fail("no structure-factor spec set: call smolmc_set_structure first");
    HIPCHK(hipSetDevice(h->device));
    const uint8_t *d_occ8;
    size_t rows;
    TRY(smolmc_eval_rows(h, occ, nocc, S.kind_base, S.K, "structure factors", &d_occ8, &rows));
    if (!rows) return 0;
    const size_t na = rows * S.Q * S.K * 2, ni = rows * S.I;
    DevScratch out;
    TRY(out.alloc(std::max<size_t>((na + ni) * 8, 16)));
    unsigned char *d_out = out.as<unsigned char>();
    TRY(smolmc_sfac_launch(h, d_occ8, rows, (long long *)d_out, (double *)(d_out + na * 8)));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (amp) HIPCHK(hipMemcpy(amp, d_out, na * 8, hipMemcpyDeviceToHost));
    if (inten && ni) HIPCHK(hipMemcpy(inten, d_out + na * 8, ni * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_sample_structure(smolmc_handle *h, int64_t *amp, double *inten) {
    const SampleSlot *sl;
    size_t rows;
    TRY(smolmc_sample_block(h, SMOLMC_SAMPLE_STRUCTURE, "the structure factors were not recorded (flags bit 6)", &sl, &rows));
    if (amp) smolmc_host_copy(amp, sl->hst + sl->o_amp, rows * (size_t)h->sfac.Q * h->sfac.K * 16);
    if (inten) smolmc_host_copy(inten, sl->hst + sl->o_inten, rows * (size_t)h->sfac.I * 8);
    return 0;
}
