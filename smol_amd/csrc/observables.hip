// Observables of recorded states (smolmc_set_observables, smolmc_eval_observables, SMOLMC_SAMPLE_OBSERVABLES):
// kind counts and pair counts of occupancy rows, reduced on the device where the rows lie.  A translation unit of its own,
// like pop_anneal.hip: a kernel added to engine.hip would move the descriptors of all of its kernels.
//
// The kind of (site, code) is kind_base[site] + code, kind_base[site] < 0 leaves the site out (DESIGN 4.15;
// observables.Observables.evaluate is the same in NumPy).  Per row:
//   counts[k]          = #{sites of kind k}
//   pairs[s][ka][kb]  += 1 for every bond (i, j) of shell s, as listed, with ka = kind(i), kb = kind(j), both counted
// Everything is int32: the order of summation is no concern, device and host agree entry for entry.
//
// One workgroup per row.  The row's Npad bytes go to LDS with 16-byte loads; one pass turns every byte into the site's
// kind (0xff: not counted) in place and counts the kinds; then the threads stride over the bond table -- one 32-bit word
// per bond, two 16-bit sites: the rows this kernel takes fit LDS, so their sites fit 16 bits -- and look both ends up in
// LDS.  LDS atomics serialise per address and a binary alloy has four cells per shell, so the adds never go to one
// shared histogram: with few cells (kinds, or cells of a shell, <= OBS_BALLOT_CELLS) a wave counts each cell by ballot
// and lane c carries the sum of cell c in a register; with more, every wave adds into a histogram of its own (as long
// as OBS_WAVES copies fit the cell limit).  The wave histograms are folded at the end, one plain store per entry.
//
// Patterns (smolmc_set_patterns, smolmc_eval_patterns, SMOLMC_SAMPLE_PATTERNS; DESIGN 4.21, patterns.Patterns.evaluate is
// the same in NumPy) are counted by the same launch, behind the shells: per set t and tuple (i_0 .. i_{m-1}), as listed,
//   cells[cell_ptr[t] + sum_p class_t[kind(i_p)] C_t^(m-1-p)] += 1, skipped when a site has no kind or its kind no class
// A second row in LDS holds every site's class in the set's map (one table lookup per site; sets with the map of the set
// before share it).  A tuple is one record of 8 (arity <= 4) or 16 bytes of u16 sites, one record a lane.  Its cell is
// counted like a pair cell where the set has more than OBS_BALLOT_CELLS cells; with fewer, in packed counters a lane keeps.
// A launch without sets takes none of these branches.
//
// Environments (smolmc_set_environments, smolmc_eval_environments, SMOLMC_SAMPLE_ENVIRONMENTS; DESIGN 4.23,
// environments.Environments.evaluate is the same in NumPy) are counted behind the patterns: per set e and centre, as listed,
//   cells[cell_ptr[e] + a (z+1)^B + sum_b n_b (z+1)^(B-1-b)] += 1, a the centre's class, n_b its neighbours of class b
// One lane a centre.  The class row in LDS (the one the patterns use, rebuilt by the first set) holds a byte per site: the
// neighbour class in the low nibble, the centre class in the high one, 0xf for none.  The neighbour table is slot-major
// ([z][n] u16 sites, 0xffff an empty slot), so the lanes of a wave read consecutive addresses; n_b sits in 8-bit fields of
// one register (z <= 64).  A launch without sets takes none of these branches.
#include "smolmc_common.h"

#define OBS_THREADS 256
#define OBS_WAVES (OBS_THREADS / 64)
#define OBS_BALLOT_CELLS 16
#define OBS_NOKIND 0xffu

struct ObsArgs {
    const uint8_t *occ;        // rows of Npad bytes
    const int32_t *kind_base;  // [N], engine numbering
    const int64_t *shell_ptr;  // [n_shells + 1]
    const uint32_t *bonds;     // [shell_ptr[n_shells]]: i | j << 16
    int32_t *counts, *pairs;   // [rows x K], [rows x n_shells x K x K]
    int N, Npad, K, n_shells;
    int pair_copies;           // histograms of the pair cells in LDS: OBS_WAVES (one per wave) or 1
    // the pattern sets (n_sets == 0: none, nothing below is read)
    const int32_t *sets;       // [n_sets x 8]: arity, classes, tuples, first cell, first record / 16 bytes, cells, new map, 0
    const uint8_t *class_of;   // [n_sets x 256]: class of a kind, 0xff: skip
    const unsigned char *recs; // records of 4 or 8 u16 sites
    int32_t *cells;            // [rows x n_cells]
    int n_sets, n_cells;
    int pat_copies;            // histograms of the pattern cells in LDS: OBS_WAVES or 1
    // the environment sets (env_hist == 0: none, nothing else below is read); the kernel reads them through obs_kernarg()
    const int32_t *env_sets;   // [n_env_sets x 8]: width, neighbour classes, centres, first cell, first u16 of the sites,
                               // first centre of the codes row, new map, 0
    const uint8_t *env_class;  // [n_env_sets x 256]: neighbour class | centre class << 4 of a kind, a nibble of 0xf: none
    const uint16_t *env_sites; // per set: the centres [n], then the neighbours [z][n], 0xffff: empty
    int32_t *env_cells;        // [rows x n_env_cells] or null
    int32_t *env_codes;        // [rows x n_env_centres] or null
    int n_env_sets, n_env_cells, n_env_centres;
    int env_copies;            // histograms of the environment cells in LDS: OBS_WAVES or 1
    int env_hist;              // env_copies x n_env_cells: the ints of these histograms (0: a launch without environment sets)
};

// The environment arguments as the environment phase reads them: from the kernel argument segment, behind an opaque copy
// of its address, so that the loads stay inside the phase.  Read through `A` they are loaded at the kernel's entry and
// held in SGPRs across the bond and tuple loops: 94 SGPRs instead of 78, and measured 2.12 ms instead of 1.96 ms per block
// for a launch without any set.
typedef const __attribute__((address_space(4))) ObsArgs *ObsKernarg;
__device__ __forceinline__ ObsKernarg obs_kernarg() {
    ObsKernarg p = (ObsKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// LDS: kinds u8 [Npad] | counts i32 [OBS_WAVES][K] | pairs i32 [pair_copies][n_shells K K]
//      | patterns i32 [pat_copies][n_cells] | environments i32 [env_copies][n_env_cells] | classes u8 [Npad]
//      (the patterns in a launch with pattern sets, the environments in one with environment sets, the classes in either)
size_t smolmc_obs_lds_bytes(int Npad, int K, size_t cells, int pair_copies) {
    return (size_t)Npad + ((size_t)OBS_WAVES * K + (size_t)pair_copies * cells) * 4;
}
int smolmc_obs_pair_copies(size_t cells) { return cells * OBS_WAVES <= SMOLMC_MAX_OBS_CELLS ? OBS_WAVES : 1; }
size_t smolmc_pat_lds_bytes(int Npad, size_t n_cells, int copies) { return (size_t)copies * n_cells * 4 + (size_t)Npad; }
static int smolmc_pat_copies(size_t n_cells) { return n_cells * OBS_WAVES <= SMOLMC_MAX_PATTERN_CELLS ? OBS_WAVES : 1; }
static int smolmc_envs_copies(size_t n_cells) { return n_cells * OBS_WAVES <= SMOLMC_MAX_ENV_CELLS ? OBS_WAVES : 1; }
// the dynamic LDS of a launch that counts everything set: the pattern and the environment sets share the class row
static size_t smolmc_obs_launch_lds(const SmolmcObs &O, const SmolmcPat &P, const SmolmcEnvSpec &E, int Npad) {
    return O.lds + (P.n_sets ? P.lds : 0) + (E.n_sets ? E.lds : 0) - (P.n_sets && E.n_sets ? (size_t)Npad : 0);
}

// four sites of a tuple record: the classes of all four are read (a short tuple is filled up with site 0), the first m
// enter the cell, most significant first
__device__ __forceinline__ void pat_unpack4(const uint8_t *cls, uint32_t lo, uint32_t hi, int m, unsigned C, unsigned &cell,
                                            bool &skip) {
    const unsigned c0 = cls[lo & 0xffffu], c1 = cls[lo >> 16], c2 = cls[hi & 0xffffu], c3 = cls[hi >> 16];
    cell = cell * C + c0; skip |= c0 == OBS_NOKIND;
    if (m > 1) { cell = cell * C + c1; skip |= c1 == OBS_NOKIND; }
    if (m > 2) { cell = cell * C + c2; skip |= c2 == OBS_NOKIND; }
    if (m > 3) { cell = cell * C + c3; skip |= c3 == OBS_NOKIND; }
}

// a lane's packed counts of a set of few cells into the histogram (LDS atomics: a wave's copy, or the shared one)
__device__ __forceinline__ void pat_flush(int32_t *hist, int nc, unsigned long long pk0, unsigned long long pk1) {
    for (int c = 0; c < nc; ++c) {
        const int v = (int)(((c < 8 ? pk0 : pk1) >> ((c & 7) * 8)) & 0xffull);
        if (v) atomicAdd(&hist[c], v);
    }
}

__global__ void __launch_bounds__(OBS_THREADS) observables_kernel(const ObsArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char obs_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = A.N, Npad = A.Npad, K = A.K, KK = K * K;
    const int cells = A.n_shells * KK;
    uint8_t *kinds = obs_smem;
    int32_t *cnt = (int32_t *)(obs_smem + Npad); // (Npad is a multiple of 16)
    int32_t *hist = cnt + OBS_WAVES * K;
    const size_t row = blockIdx.x;

    {   // the row, 16 bytes a lane; the histograms start at zero
        const uint4 *src = (const uint4 *)(A.occ + row * Npad);
        uint4 *dst = (uint4 *)kinds;
        for (int i = tid; i < Npad / 16; i += OBS_THREADS) dst[i] = src[i];
        for (int i = tid; i < OBS_WAVES * K + A.pair_copies * cells + A.pat_copies * A.n_cells + A.env_hist;
             i += OBS_THREADS)
            cnt[i] = 0;
    }
    __syncthreads();

    // codes -> kinds in place (every byte is read and written by one thread), and the kind counts
    {
        int acc = 0; // ballot form: lane c holds the count of kind c
        for (int s0 = wave * 64; s0 < Npad; s0 += OBS_THREADS) { // (wave-uniform bounds: every lane takes part in the ballots)
            const int s = s0 + lane;
            unsigned k = OBS_NOKIND;
            if (s < N) {
                const int kb = A.kind_base[s];
                if (kb >= 0) k = (unsigned)kb + kinds[s];
                if (k >= (unsigned)K) k = OBS_NOKIND; // (a code the site's block has no kind for: only on a fixed site whose width the tables do not give)
            }
            if (s < Npad) kinds[s] = (uint8_t)k;
            if (K <= OBS_BALLOT_CELLS) {
                for (int c = 0; c < K; ++c) {
                    const int n = __popcll(__ballot(k == (unsigned)c));
                    if (lane == c) acc += n;
                }
            } else if (k != OBS_NOKIND) {
                atomicAdd(&cnt[wave * K + (int)k], 1);
            }
        }
        if (K <= OBS_BALLOT_CELLS && lane < K) cnt[wave * K + lane] = acc;
    }
    __syncthreads();

    // the bonds, shell by shell
    int32_t *mine = hist + (A.pair_copies > 1 ? wave * cells : 0);
    for (int sh = 0; sh < A.n_shells; ++sh) {
        const int64_t b0 = A.shell_ptr[sh], b1 = A.shell_ptr[sh + 1];
        int acc = 0;
        for (int64_t base = b0 + wave * 64; base < b1; base += OBS_THREADS) {
            const int64_t b = base + lane;
            int cell = -1;
            if (b < b1) {
                const uint32_t w = A.bonds[b];
                const unsigned ka = kinds[w & 0xffffu], kb = kinds[w >> 16];
                if (ka != OBS_NOKIND && kb != OBS_NOKIND) cell = (int)(ka * (unsigned)K + kb);
            }
            if (KK <= OBS_BALLOT_CELLS) {
                for (int c = 0; c < KK; ++c) {
                    const int n = __popcll(__ballot(cell == c));
                    if (lane == c) acc += n;
                }
            } else if (cell >= 0) {
                atomicAdd(&mine[sh * KK + cell], 1);
            }
        }
        // (ballot form: pair_copies == OBS_WAVES whenever a shell has so few cells and the call was accepted with one
        // copy only when cells * OBS_WAVES exceeds the limit -- then every wave adds its sums to the shared copy)
        if (KK <= OBS_BALLOT_CELLS && lane < KK) {
            if (A.pair_copies > 1) mine[sh * KK + lane] = acc;
            else atomicAdd(&mine[sh * KK + lane], acc);
        }
    }

    // the pattern sets: the classes of the sites in the set's map, then the tuples, one record a lane
    int32_t *phist = hist + A.pair_copies * cells;
    int32_t *ehist = phist + A.pat_copies * A.n_cells;
    uint8_t *cls = (uint8_t *)(ehist + A.env_hist);
    for (int t = 0; t < A.n_sets; ++t) {
        const int32_t *S = A.sets + 8 * t; // (uniform: scalar loads)
        const int m = S[0], n = S[2], nc = S[5];
        const unsigned C = (unsigned)S[1];
        if (S[6]) { // another map than the set before had (set 0: always); every thread of the workgroup gets here
            __syncthreads();
            const uint8_t *tab = A.class_of + 256 * t;
            for (int s = tid; s < Npad; s += OBS_THREADS) cls[s] = tab[kinds[s]];
            __syncthreads();
        }
        const unsigned char *recs = A.recs + (size_t)S[4] * 16;
        int32_t *pmine = phist + (A.pat_copies > 1 ? wave * A.n_cells : 0) + S[3];
        // few cells: a lane counts its own tuples in 8-bit fields of two registers (cells 0..7, 8..15) and adds them to
        // the histogram every 255 tuples and at the end -- measured 1.6x the ballot form of the pair cells on the
        // headline shape, whose eight to sixteen ballots a tuple were most of the loop
        const bool few = nc <= OBS_BALLOT_CELLS;
        unsigned long long pk0 = 0, pk1 = 0;
        int held = 0;
        for (int base = wave * 64; base < n; base += OBS_THREADS) {
            const int i = base + lane;
            int cell = -1;
            if (i < n) {
                unsigned v = 0;
                bool skip = false;
                if (m <= 4) {
                    const uint2 w = ((const uint2 *)recs)[i];
                    pat_unpack4(cls, w.x, w.y, m, C, v, skip);
                } else {
                    const uint4 w = ((const uint4 *)recs)[i];
                    pat_unpack4(cls, w.x, w.y, 4, C, v, skip);
                    pat_unpack4(cls, w.z, w.w, m - 4, C, v, skip);
                }
                if (!skip) cell = (int)v;
            }
            if (few) {
                if (cell >= 0) {
                    const unsigned long long one = 1ull << ((cell & 7) * 8);
                    if (cell < 8) pk0 += one;
                    else pk1 += one;
                }
                if (++held == 255) { // (uniform over the wave: a field holds 255 at most)
                    pat_flush(pmine, nc, pk0, pk1);
                    pk0 = pk1 = 0;
                    held = 0;
                }
            } else if (cell >= 0) {
                atomicAdd(&pmine[cell], 1);
            }
        }
        if (few) pat_flush(pmine, nc, pk0, pk1);
    }

    // the environment sets: the two classes of the sites in the set's maps, then the centres, one a lane
    if (A.env_hist) {
        const ObsKernarg E = obs_kernarg();
        const int n_env_cells = E->n_env_cells;
        for (int e = 0; e < E->n_env_sets; ++e) {
            const int32_t *S = E->env_sets + 8 * e; // (uniform: scalar loads)
            const int z = S[0], B = S[1], n = S[2];
            if (S[6]) { // other maps than the set before had (set 0: always); every thread of the workgroup gets here
                __syncthreads();
                const uint8_t *tab = E->env_class + 256 * e;
                for (int s = tid; s < Npad; s += OBS_THREADS) cls[s] = tab[kinds[s]];
                __syncthreads();
            }
            const uint16_t *cen = E->env_sites + S[4], *nb = cen + n;
            int32_t *emine = ehist + (E->env_copies > 1 ? wave * n_env_cells : 0) + S[3];
            int32_t *codes = E->env_codes ? E->env_codes + row * (size_t)E->n_env_centres + S[5] : nullptr;
            for (int i = tid; i < n; i += OBS_THREADS) {
                const unsigned c = cls[cen[i]];
                unsigned pk = 0; // n_b in bits 8 b .. 8 b + 7 (z <= 64)
                for (int q = 0; q < z; ++q) { // (uniform trip count)
                    const unsigned s = nb[(size_t)q * n + i];
                    const unsigned b = cls[s == 0xffffu ? 0u : s] & 0xfu;
                    pk += (s == 0xffffu || b == 0xfu) ? 0u : 1u << ((b & 3u) * 8);
                }
                unsigned code = c >> 4;
                for (int b = 0; b < B; ++b) code = code * (unsigned)(z + 1) + ((pk >> (8 * b)) & 0xffu);
                const bool skip = (c >> 4) == 0xfu;
                if (!skip) atomicAdd(&emine[code], 1);
                if (codes) codes[i] = skip ? -1 : (int)code;
            }
        }
    }
    __syncthreads();

    // fold the waves' copies: plain stores, one per entry (the output pointers are read here, see obs_kernarg)
    const ObsKernarg F = obs_kernarg();
    int32_t *const out_counts = F->counts, *const out_pairs = F->pairs, *const out_cells = F->cells;
    if (out_counts)
        for (int k = tid; k < K; k += OBS_THREADS) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < OBS_WAVES; ++w) v += cnt[w * K + k];
            out_counts[row * K + k] = v;
        }
    if (A.n_sets)
        for (int c = tid; c < A.n_cells; c += OBS_THREADS) {
            int v = 0;
            for (int w = 0; w < A.pat_copies; ++w) v += phist[w * A.n_cells + c];
            out_cells[row * (size_t)A.n_cells + c] = v;
        }
    if (A.env_hist) {
        const ObsKernarg E = obs_kernarg();
        int32_t *out = E->env_cells;
        const int n_env_cells = E->n_env_cells, copies = E->env_copies;
        if (out)
            for (int c = tid; c < n_env_cells; c += OBS_THREADS) {
                int v = 0;
                for (int w = 0; w < copies; ++w) v += ehist[w * n_env_cells + c];
                out[row * (size_t)n_env_cells + c] = v;
            }
    }
    for (int c = tid; c < cells; c += OBS_THREADS) {
        int v = 0;
        for (int w = 0; w < A.pair_copies; ++w) v += hist[w * cells + c];
        out_pairs[row * (size_t)cells + c] = v;
    }
}

int smolmc_obs_launch(smolmc_handle *h, const uint8_t *d_occ8, size_t rows, int32_t *d_counts, int32_t *d_pairs, int32_t *d_cells,
                      int32_t *d_env, int32_t *d_codes) {
    const SmolmcObs &O = h->obs;
    const SmolmcPat &P = O.pat;
    const SmolmcEnvSpec &E = O.env;
    const bool env = d_env || d_codes;
    if (env && !E.n_sets) return fail("no environment spec set (smolmc_set_environments)");
    if (!O.K) return fail("no observables set (smolmc_set_observables)");
    if (d_cells && !P.n_sets) return fail("no pattern spec set (smolmc_set_patterns)");
    if (!rows) return 0;
    if (rows > 0x7fffffffull) return fail("observables: more than 2^31 rows in one launch");
    ObsArgs A;
    A.occ = d_occ8; A.kind_base = O.d_kind_base; A.shell_ptr = O.d_shell_ptr; A.bonds = O.d_bonds;
    A.counts = d_counts; A.pairs = d_pairs;
    A.N = h->N; A.Npad = h->Npad; A.K = O.K; A.pair_copies = O.pair_copies;
    A.n_shells = d_pairs ? O.n_shells : 0; // (no shells: the kernel counts the kinds and never touches the pair arrays)
    A.sets = P.d_sets; A.class_of = P.d_class; A.recs = P.d_recs; A.cells = d_cells;
    A.n_sets = d_cells ? P.n_sets : 0;     // (no sets: the kernel never touches the pattern arrays)
    A.n_cells = d_cells ? (int)P.n_cells : 0; A.pat_copies = P.copies;
    A.env_sets = E.d_sets; A.env_class = E.d_class; A.env_sites = E.d_sites; A.env_cells = d_env; A.env_codes = d_codes;
    A.n_env_sets = env ? E.n_sets : 0;     // (no sets: the kernel never touches the environment arrays)
    A.n_env_cells = env ? (int)E.n_cells : 0; A.n_env_centres = (int)E.n_centres; A.env_copies = E.copies;
    A.env_hist = A.env_copies * A.n_env_cells;
    // (the class row is taken once, by the patterns or the environments)
    const size_t lds = O.lds + (d_cells ? P.lds : 0) + (env ? E.lds : 0) - (d_cells && env ? (size_t)h->Npad : 0);
    if (!h->obs_ev0) {
        HIPCHK(hipEventCreate(&h->obs_ev0));
        HIPCHK(hipEventCreate(&h->obs_ev1));
    }
    HIPCHK(hipEventRecord(h->obs_ev0, h->stream));
    hipLaunchKernelGGL(observables_kernel, dim3((unsigned)rows), dim3(OBS_THREADS), lds, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->obs_ev1, h->stream));
    return 0;
}

// elapsed device time of the last launch of the observables kernel in ms (tools/observables_timing.py); a measuring hook
// like smolmc_debug_relabel, not part of the C-ABI
extern "C" int smolmc_debug_obs_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    if (!h->obs_ev0) return fail("the observables kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->obs_ev1));
    HIPCHK(hipEventElapsedTime(ms, h->obs_ev0, h->obs_ev1));
    return 0;
}

void smolmc_obs_free(SmolmcObs &O) {
    if (O.d_kind_base) hipFree(O.d_kind_base);
    if (O.d_shell_ptr) hipFree(O.d_shell_ptr);
    if (O.d_bonds) hipFree(O.d_bonds);
    smolmc_pat_free(O.pat);
    smolmc_envs_free(O.env);
    O = SmolmcObs();
}
void smolmc_envs_free(SmolmcEnvSpec &E) {
    if (E.arena) hipFree(E.arena);
    E = SmolmcEnvSpec();
}
void smolmc_pat_free(SmolmcPat &P) {
    if (P.arena) hipFree(P.arena);
    P = SmolmcPat();
}

// ---- the C-ABI of the observables --------------------------------------------------------------------------------------
extern "C" int smolmc_set_observables(smolmc_handle *h, const smolmc_observables *obs) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_OBSERVABLES, "smolmc_set_observables", "SMOLMC_SAMPLE_OBSERVABLES"));
    SmolmcObs O;
    if (h->obs.pat.n_sets)
        return fail("smolmc_set_observables while a pattern spec rests on the kinds of the observables (call "
                    "smolmc_set_patterns(h, NULL) first)");
    if (h->obs.env.n_sets)
        return fail("smolmc_set_observables while an environment spec rests on the kinds of the observables (call "
                    "smolmc_set_environments(h, NULL) first)");
    if (h->minima.n_slots && h->minima.n_axes)
        return fail("smolmc_set_observables while a minima record keyed by composition depends on the observables (call "
                    "smolmc_set_minima(h, NULL) first)");
    if (h->stats.n_keys && h->stats.n_count_cols)
        return fail("smolmc_set_observables while a statistics record with count columns depends on the observables (call "
                    "smolmc_set_statistics(h, NULL) first)");
    if (obs) {
        const int N = h->N, K = obs->n_kinds, S = obs->n_shells;
        if (!obs->kind_base || S < 0 || (S > 0 && (!obs->shell_ptr || !obs->bonds))) return fail("observables: null argument");
        if (K < 1 || K > 254) return fail("observables: n_kinds must be 1..254 (a kind is staged as one byte)");
        const size_t cells = (size_t)S * K * K;
        if (cells > SMOLMC_MAX_OBS_CELLS) {
            char msg[160];
            snprintf(msg, sizeof msg, "observables: %d shells x %d x %d kinds = %zu cells, larger than SMOLMC_MAX_OBS_CELLS = %d", S, K, K,
                     cells, SMOLMC_MAX_OBS_CELLS);
            return fail(msg);
        }
        std::vector<int32_t> kb;
        TRY(smolmc_kind_base_in(h, obs->kind_base, K, "observables", kb));
        const int64_t nb = S ? obs->shell_ptr[S] : 0;
        for (int sidx = 0; sidx < S; ++sidx)
            if (obs->shell_ptr[0] != 0 || obs->shell_ptr[sidx] > obs->shell_ptr[sidx + 1])
                return fail("observables: shell_ptr must be ascending from 0");
        O.K = K; O.n_shells = S; O.cells = cells;
        O.kind_base = kb;
        O.pair_copies = smolmc_obs_pair_copies(cells);
        O.lds = smolmc_obs_lds_bytes(h->Npad, K, cells, O.pair_copies);
        if (O.lds > 64 * 1024) {
            char msg[200];
            snprintf(msg, sizeof msg, "observables: a row of %d sites is too long to stage in LDS next to the histograms (%zu bytes, 65536 at most)",
                     N, O.lds);
            return fail(msg);
        }
        // (a row that fits LDS has fewer than 2^16 sites: a bond is one word)
        std::vector<uint32_t> bw((size_t)nb);
        for (int64_t b = 0; b < nb; ++b) {
            const int32_t i = obs->bonds[2 * b], j = obs->bonds[2 * b + 1];
            if (i < 0 || i >= N || j < 0 || j >= N) {
                char msg[160];
                snprintf(msg, sizeof msg, "observables: bond %lld = (%d, %d) out of range (%d sites)", (long long)b, (int)i, (int)j, N);
                return fail(msg);
            }
            const uint32_t ei = (uint32_t)(h->relabelled ? h->new_of[i] : i), ej = (uint32_t)(h->relabelled ? h->new_of[j] : j);
            bw[(size_t)b] = ei | (ej << 16);
        }
        hipError_t e = hipMalloc((void **)&O.d_kind_base, std::max<size_t>((size_t)N * 4, 16));
        if (e == hipSuccess) e = hipMalloc((void **)&O.d_shell_ptr, ((size_t)S + 1) * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&O.d_bonds, std::max<size_t>((size_t)nb * 4, 16));
        if (e == hipSuccess) e = hipMemcpy(O.d_kind_base, kb.data(), (size_t)N * 4, hipMemcpyHostToDevice);
        const int64_t zero = 0;
        if (e == hipSuccess) e = hipMemcpy(O.d_shell_ptr, S ? obs->shell_ptr : &zero, ((size_t)S + 1) * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && nb) e = hipMemcpy(O.d_bonds, bw.data(), (size_t)nb * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            smolmc_obs_free(O);
            return fail(std::string("observables upload: ") + hipGetErrorString(e));
        }
    }
    TRY(smolmc_ring_forget(h, SMOLMC_SAMPLE_OBSERVABLES));
    smolmc_obs_free(h->obs);
    h->obs = O;
    return 0;
}

extern "C" int smolmc_observables_shape(smolmc_handle *h, int *n_kinds, int *n_shells) {
    if (!h) return fail("null handle");
    if (n_kinds) *n_kinds = h->obs.K;
    if (n_shells) *n_shells = h->obs.n_shells;
    return 0;
}

extern "C" int smolmc_eval_observables(smolmc_handle *h, const int32_t *occ, int nocc, int32_t *counts, int32_t *pairs) {
    if (!h) return fail("null handle");
    if (!h->obs.K) return fail("no observables set: call smolmc_set_observables first");
    HIPCHK(hipSetDevice(h->device));
    const uint8_t *d_occ8;
    size_t rows;
    TRY(smolmc_eval_rows(h, occ, nocc, h->obs.kind_base, h->obs.K, "observables", &d_occ8, &rows));
    if (!rows) return 0;
    const size_t nc = rows * h->obs.K, np = rows * h->obs.cells;
    DevScratch out;
    TRY(out.alloc(std::max<size_t>((nc + np) * 4, 16)));
    int32_t *d_out = out.as<int32_t>();
    TRY(smolmc_obs_launch(h, d_occ8, rows, d_out, d_out + nc, nullptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (counts) HIPCHK(hipMemcpy(counts, d_out, nc * 4, hipMemcpyDeviceToHost));
    if (pairs && np) HIPCHK(hipMemcpy(pairs, d_out + nc, np * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_sample_observables(smolmc_handle *h, int32_t *counts, int32_t *pairs) {
    const SampleSlot *sl;
    size_t rows;
    TRY(smolmc_sample_block(h, SMOLMC_SAMPLE_OBSERVABLES, "the observables were not recorded (flags bit 3)", &sl, &rows));
    if (counts) smolmc_host_copy(counts, sl->hst + sl->o_cnt, rows * (size_t)h->obs.K * 4);
    if (pairs) smolmc_host_copy(pairs, sl->hst + sl->o_pair, rows * h->obs.cells * 4);
    return 0;
}

// ---- the C-ABI of the pattern spec ---------------------------------------------------------------------------------------
extern "C" int smolmc_set_patterns(smolmc_handle *h, const smolmc_patterns *sp) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_PATTERNS, "smolmc_set_patterns", "SMOLMC_SAMPLE_PATTERNS"));
    if (h->stats.n_keys && h->stats.n_pat_cols)
        return fail("smolmc_set_patterns while a statistics record with pattern columns depends on the spec (call "
                    "smolmc_set_statistics(h, NULL) first)");
    if (h->stats.n_keys && h->stats.n_env_cols)
        return fail("smolmc_set_patterns while a statistics record with environment columns lies behind the pattern cells (call "
                    "smolmc_set_statistics(h, NULL) first)");
    SmolmcPat P;
    if (sp) {
        const SmolmcObs &O = h->obs;
        const int N = h->N, K = O.K, T = sp->n_sets;
        char msg[256];
        if (!K) return fail("patterns: no observables set: the class maps index their kinds (call smolmc_set_observables first)");
        if (T < 1 || T > SMOLMC_MAX_PATTERN_SETS) {
            snprintf(msg, sizeof msg, "patterns: n_sets must be 1..%d, got %d", SMOLMC_MAX_PATTERN_SETS, T);
            return fail(msg);
        }
        if (!sp->arity || !sp->n_classes || !sp->class_of_kind || !sp->tuple_ptr) return fail("patterns: null argument");
        if (sp->tuple_ptr[0] != 0) return fail("patterns: tuple_ptr[0] must be 0");
        std::vector<int32_t> sets((size_t)T * 8, 0);
        std::vector<uint8_t> tab((size_t)T * 256, (uint8_t)OBS_NOKIND);
        std::vector<uint16_t> recs;
        size_t n_cells = 0, site0 = 0;
        for (int t = 0; t < T; ++t) {
            const int m = sp->arity[t], C = sp->n_classes[t];
            if (m < 1 || m > SMOLMC_MAX_PATTERN_ARITY) {
                snprintf(msg, sizeof msg, "patterns: set %d has arity %d, outside 1..%d", t, m, SMOLMC_MAX_PATTERN_ARITY);
                return fail(msg);
            }
            if (C < 1 || C > SMOLMC_MAX_PATTERN_CLASSES) {
                snprintf(msg, sizeof msg, "patterns: set %d has %d classes, outside 1..%d", t, C, SMOLMC_MAX_PATTERN_CLASSES);
                return fail(msg);
            }
            for (int k = 0; k < K; ++k) {
                const int32_t c = sp->class_of_kind[(size_t)t * K + k];
                if (c < -1 || c >= C) {
                    snprintf(msg, sizeof msg, "patterns: set %d maps kind %d to class %d, outside -1..%d: class out of range", t, k, (int)c, C - 1);
                    return fail(msg);
                }
                tab[(size_t)t * 256 + k] = c < 0 ? (uint8_t)OBS_NOKIND : (uint8_t)c;
            }
            size_t nc = 1;
            for (int p = 0; p < m && nc <= SMOLMC_MAX_PATTERN_CELLS; ++p) nc *= (size_t)C;
            if (n_cells + nc > SMOLMC_MAX_PATTERN_CELLS) {
                snprintf(msg, sizeof msg, "patterns: set %d with %d classes on %d sites brings the spec to more than "
                         "SMOLMC_MAX_PATTERN_CELLS = %d cells", t, C, m, SMOLMC_MAX_PATTERN_CELLS);
                return fail(msg);
            }
            const int64_t n = sp->tuple_ptr[t + 1] - sp->tuple_ptr[t];
            if (n < 0) return fail("patterns: tuple_ptr must not decrease");
            if (n > 0 && !sp->sites) return fail("patterns: null argument");
            const size_t width = m <= 4 ? 4 : 8; // u16 sites of a record
            if ((recs.size() + (size_t)n * width) * 2 > ((size_t)1 << 30)) return fail("patterns: the tuple records take more than 1 GiB");
            int32_t *S = &sets[(size_t)t * 8];
            S[0] = m; S[1] = C; S[2] = (int32_t)n; S[3] = (int32_t)n_cells; S[4] = (int32_t)(recs.size() / 8); S[5] = (int32_t)nc;
            S[6] = t == 0 || memcmp(&tab[(size_t)t * 256], &tab[(size_t)(t - 1) * 256], 256) != 0;
            const size_t r0 = recs.size();
            recs.resize(r0 + (((size_t)n * width + 7) & ~(size_t)7), 0); // (every set starts at a multiple of 16 bytes)
            for (int64_t i = 0; i < n; ++i)
                for (int p = 0; p < m; ++p) {
                    const int32_t s = sp->sites[site0 + (size_t)i * m + p];
                    if (s < 0 || s >= N) {
                        snprintf(msg, sizeof msg, "patterns: set %d tuple %lld names site %d, %d sites: site out of range", t, (long long)i,
                                 (int)s, N);
                        return fail(msg);
                    }
                    recs[r0 + (size_t)i * width + p] = (uint16_t)(h->relabelled ? h->new_of[s] : s);
                }
            site0 += (size_t)n * m;
            n_cells += nc;
        }
        P.n_sets = T; P.n_cells = n_cells;
        P.copies = smolmc_pat_copies(n_cells);
        P.lds = smolmc_pat_lds_bytes(h->Npad, n_cells, P.copies);
        // (a row that fits LDS has fewer than 2^16 sites: a site of a record is 16 bits)
        if (O.lds + P.lds > 64 * 1024) {
            snprintf(msg, sizeof msg, "patterns: a launch takes %zu bytes of LDS for the row and the observables and %zu for the classes "
                     "and %zu cells, 65536 at most", O.lds, P.lds, n_cells);
            return fail(msg);
        }
        if (smolmc_obs_launch_lds(O, P, O.env, h->Npad) > 64 * 1024) {
            snprintf(msg, sizeof msg, "patterns: with the environment spec in force a launch takes %zu bytes of LDS (the row, the "
                     "observables, the classes, %zu pattern and %zu environment cells), 65536 at most",
                     smolmc_obs_launch_lds(O, P, O.env, h->Npad), n_cells, O.env.n_cells);
            return fail(msg);
        }
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
        const size_t o_sets = take(sets.size() * 4), o_tab = take(tab.size()), o_recs = take(recs.size() * 2),
                     o_u = take((size_t)h->R * n_cells * 4);
        hipError_t e = hipMalloc((void **)&P.arena, at);
        if (e != hipSuccess) return fail(std::string("patterns: hipMalloc: ") + hipGetErrorString(e));
        unsigned char *d = P.arena;
        P.d_sets = (int32_t *)(d + o_sets); P.d_class = d + o_tab; P.d_recs = d + o_recs; P.u_cells = (int32_t *)(d + o_u);
        e = hipMemcpy(P.d_sets, sets.data(), sets.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(P.d_class, tab.data(), tab.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !recs.empty()) e = hipMemcpy(P.d_recs, recs.data(), recs.size() * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            smolmc_pat_free(P);
            return fail(std::string("patterns upload: ") + hipGetErrorString(e));
        }
    }
    TRY(smolmc_ring_forget(h, SMOLMC_SAMPLE_PATTERNS));
    smolmc_pat_free(h->obs.pat);
    h->obs.pat = P;
    return 0;
}

extern "C" int smolmc_patterns_shape(smolmc_handle *h, int *n_sets, int *n_cells) {
    if (!h) return fail("null handle");
    if (n_sets) *n_sets = h->obs.pat.n_sets;
    if (n_cells) *n_cells = (int)h->obs.pat.n_cells;
    return 0;
}

extern "C" int smolmc_eval_patterns(smolmc_handle *h, const int32_t *occ, int nocc, int32_t *cells) {
    if (!h) return fail("null handle");
    const SmolmcPat &P = h->obs.pat;
    if (!P.n_sets) return fail("no pattern spec set: call smolmc_set_patterns first");
    HIPCHK(hipSetDevice(h->device));
    const uint8_t *d_occ8;
    size_t rows;
    TRY(smolmc_eval_rows(h, occ, nocc, h->obs.kind_base, h->obs.K, "patterns", &d_occ8, &rows));
    if (!rows) return 0;
    DevScratch out;
    TRY(out.alloc(std::max<size_t>(rows * P.n_cells * 4, 16)));
    TRY(smolmc_obs_launch(h, d_occ8, rows, nullptr, nullptr, out.as<int32_t>()));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (cells) HIPCHK(hipMemcpy(cells, out.p, rows * P.n_cells * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_sample_patterns(smolmc_handle *h, int32_t *cells) {
    const SampleSlot *sl;
    size_t rows;
    TRY(smolmc_sample_block(h, SMOLMC_SAMPLE_PATTERNS, "the patterns were not recorded (flags bit 8)", &sl, &rows));
    if (cells) smolmc_host_copy(cells, sl->hst + sl->o_pat, rows * h->obs.pat.n_cells * 4);
    return 0;
}

// ---- the C-ABI of the environment spec -----------------------------------------------------------------------------------
extern "C" int smolmc_set_environments(smolmc_handle *h, const smolmc_environments *sp) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_ENVIRONMENTS, "smolmc_set_environments", "SMOLMC_SAMPLE_ENVIRONMENTS"));
    if (h->stats.n_keys && h->stats.n_env_cols)
        return fail("smolmc_set_environments while a statistics record with environment columns depends on the spec (call "
                    "smolmc_set_statistics(h, NULL) first)");
    SmolmcEnvSpec E;
    if (sp) {
        const SmolmcObs &O = h->obs;
        const int N = h->N, K = O.K, T = sp->n_sets;
        char msg[256];
        if (!K) return fail("environments: no observables set: the class maps index their kinds (call smolmc_set_observables first)");
        if (T < 1 || T > SMOLMC_MAX_ENV_SETS) {
            snprintf(msg, sizeof msg, "environments: n_sets must be 1..%d, got %d", SMOLMC_MAX_ENV_SETS, T);
            return fail(msg);
        }
        if (!sp->width || !sp->n_centre_classes || !sp->n_neigh_classes || !sp->centre_class_of_kind || !sp->neigh_class_of_kind ||
            !sp->centre_ptr)
            return fail("environments: null argument");
        if (sp->centre_ptr[0] != 0) return fail("environments: centre_ptr[0] must be 0");
        std::vector<int32_t> sets((size_t)T * 8, 0);
        std::vector<uint8_t> tab((size_t)T * 256, (uint8_t)0xff);
        std::vector<uint16_t> sites;
        size_t n_cells = 0, slot0 = 0;
        for (int t = 0; t < T; ++t) {
            const int z = sp->width[t], A = sp->n_centre_classes[t], B = sp->n_neigh_classes[t];
            if (z < 1 || z > SMOLMC_MAX_ENV_WIDTH) {
                snprintf(msg, sizeof msg, "environments: set %d has width %d, outside 1..%d", t, z, SMOLMC_MAX_ENV_WIDTH);
                return fail(msg);
            }
            if (A < 1 || A > SMOLMC_MAX_ENV_CENTRE_CLASSES) {
                snprintf(msg, sizeof msg, "environments: set %d has %d centre classes, outside 1..%d", t, A, SMOLMC_MAX_ENV_CENTRE_CLASSES);
                return fail(msg);
            }
            if (B < 1 || B > SMOLMC_MAX_ENV_NEIGH_CLASSES) {
                snprintf(msg, sizeof msg, "environments: set %d has %d neighbour classes, outside 1..%d", t, B, SMOLMC_MAX_ENV_NEIGH_CLASSES);
                return fail(msg);
            }
            for (int k = 0; k < K; ++k) {
                const int32_t a = sp->centre_class_of_kind[(size_t)t * K + k], b = sp->neigh_class_of_kind[(size_t)t * K + k];
                if (a < -1 || a >= A) {
                    snprintf(msg, sizeof msg, "environments: set %d maps kind %d to centre class %d, outside -1..%d: class out of range", t, k,
                             (int)a, A - 1);
                    return fail(msg);
                }
                if (b < -1 || b >= B) {
                    snprintf(msg, sizeof msg, "environments: set %d maps kind %d to neighbour class %d, outside -1..%d: class out of range", t,
                             k, (int)b, B - 1);
                    return fail(msg);
                }
                tab[(size_t)t * 256 + k] = (uint8_t)((b < 0 ? 0xf : b) | (a < 0 ? 0xf : a) << 4);
            }
            size_t nc = (size_t)A;
            for (int b = 0; b < B && nc <= SMOLMC_MAX_ENV_CELLS; ++b) nc *= (size_t)(z + 1);
            if (n_cells + nc > SMOLMC_MAX_ENV_CELLS) {
                snprintf(msg, sizeof msg, "environments: set %d with %d centre classes, %d neighbour classes and width %d brings the spec "
                         "to more than SMOLMC_MAX_ENV_CELLS = %d cells", t, A, B, z, SMOLMC_MAX_ENV_CELLS);
                return fail(msg);
            }
            const int64_t c0 = sp->centre_ptr[t], n = sp->centre_ptr[t + 1] - c0;
            if (n < 0) return fail("environments: centre_ptr must not decrease");
            if (n > 0 && (!sp->centres || !sp->neighbours)) return fail("environments: null argument");
            if ((sites.size() + (size_t)n * (z + 1)) * 2 > ((size_t)1 << 30) || sp->centre_ptr[t + 1] > 0x7fffffff)
                return fail("environments: the neighbour tables take more than 1 GiB");
            int32_t *S = &sets[(size_t)t * 8];
            S[0] = z; S[1] = B; S[2] = (int32_t)n; S[3] = (int32_t)n_cells; S[4] = (int32_t)sites.size(); S[5] = (int32_t)c0;
            S[6] = t == 0 || memcmp(&tab[(size_t)t * 256], &tab[(size_t)(t - 1) * 256], 256) != 0;
            const size_t r0 = sites.size();
            sites.resize(r0 + (size_t)n * (z + 1), 0xffff);
            for (int64_t i = 0; i < n; ++i) {
                const int32_t c = sp->centres[c0 + i];
                if (c < 0 || c >= N) {
                    snprintf(msg, sizeof msg, "environments: set %d centre %lld is site %d, %d sites: site out of range", t, (long long)i,
                             (int)c, N);
                    return fail(msg);
                }
                sites[r0 + (size_t)i] = (uint16_t)(h->relabelled ? h->new_of[c] : c);
                for (int q = 0; q < z; ++q) {
                    const int32_t s = sp->neighbours[slot0 + (size_t)i * z + q];
                    if (s < -1 || s >= N) {
                        snprintf(msg, sizeof msg, "environments: set %d centre %lld slot %d names site %d, %d sites: site out of range", t,
                                 (long long)i, q, (int)s, N);
                        return fail(msg);
                    }
                    if (s >= 0) sites[r0 + (size_t)(q + 1) * n + i] = (uint16_t)(h->relabelled ? h->new_of[s] : s);
                }
            }
            slot0 += (size_t)n * z;
            n_cells += nc;
        }
        E.n_sets = T; E.n_cells = n_cells; E.n_centres = (size_t)sp->centre_ptr[T];
        E.copies = smolmc_envs_copies(n_cells);
        E.lds = (size_t)E.copies * n_cells * 4 + (size_t)h->Npad;
        // (a row that fits LDS has fewer than 2^16 - 1 sites: a site of the tables is 16 bits and 0xffff is free)
        const size_t lds = smolmc_obs_launch_lds(O, O.pat, E, h->Npad);
        if (lds > 64 * 1024) {
            snprintf(msg, sizeof msg, "environments: a launch takes %zu bytes of LDS (the row, the observables, the classes, %zu "
                     "pattern and %zu environment cells), 65536 at most", lds, O.pat.n_cells, n_cells);
            return fail(msg);
        }
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
        const size_t o_sets = take(sets.size() * 4), o_tab = take(tab.size()), o_sites = take(sites.size() * 2),
                     o_u = take((size_t)h->R * n_cells * 4);
        hipError_t e = hipMalloc((void **)&E.arena, at);
        if (e != hipSuccess) return fail(std::string("environments: hipMalloc: ") + hipGetErrorString(e));
        unsigned char *d = E.arena;
        E.d_sets = (int32_t *)(d + o_sets); E.d_class = d + o_tab; E.d_sites = (uint16_t *)(d + o_sites); E.u_cells = (int32_t *)(d + o_u);
        e = hipMemcpy(E.d_sets, sets.data(), sets.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(E.d_class, tab.data(), tab.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !sites.empty()) e = hipMemcpy(E.d_sites, sites.data(), sites.size() * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            smolmc_envs_free(E);
            return fail(std::string("environments upload: ") + hipGetErrorString(e));
        }
    }
    TRY(smolmc_ring_forget(h, SMOLMC_SAMPLE_ENVIRONMENTS));
    smolmc_envs_free(h->obs.env);
    h->obs.env = E;
    return 0;
}

extern "C" int smolmc_environments_shape(smolmc_handle *h, int *n_sets, int *n_cells, int *n_centres) {
    if (!h) return fail("null handle");
    if (n_sets) *n_sets = h->obs.env.n_sets;
    if (n_cells) *n_cells = (int)h->obs.env.n_cells;
    if (n_centres) *n_centres = (int)h->obs.env.n_centres;
    return 0;
}

extern "C" int smolmc_eval_environments(smolmc_handle *h, const int32_t *occ, int nocc, int32_t *cells, int32_t *codes) {
    if (!h) return fail("null handle");
    const SmolmcEnvSpec &E = h->obs.env;
    if (!E.n_sets) return fail("no environment spec set: call smolmc_set_environments first");
    HIPCHK(hipSetDevice(h->device));
    const uint8_t *d_occ8;
    size_t rows;
    TRY(smolmc_eval_rows(h, occ, nocc, h->obs.kind_base, h->obs.K, "environments", &d_occ8, &rows));
    const size_t nc = cells ? rows * E.n_cells : 0, nk = codes ? rows * E.n_centres : 0;
    if (!nc && !nk) return 0; // (nothing asked for, or the codes of a spec without centres)
    DevScratch out;
    TRY(out.alloc(std::max<size_t>((nc + nk) * 4, 16)));
    int32_t *d_out = out.as<int32_t>();
    TRY(smolmc_obs_launch(h, d_occ8, rows, nullptr, nullptr, nullptr, nc ? d_out : nullptr, nk ? d_out + nc : nullptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (cells) HIPCHK(hipMemcpy(cells, d_out, nc * 4, hipMemcpyDeviceToHost));
    if (codes && nk) HIPCHK(hipMemcpy(codes, d_out + nc, nk * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_sample_environments(smolmc_handle *h, int32_t *cells) {
    const SampleSlot *sl;
    size_t rows;
    TRY(smolmc_sample_block(h, SMOLMC_SAMPLE_ENVIRONMENTS, "the environments were not recorded (flags bit 9)", &sl, &rows));
    if (cells) smolmc_host_copy(cells, sl->hst + sl->o_env, rows * h->obs.env.n_cells * 4);
    return 0;
}
