// Connectivity of recorded states (smolmc_set_connectivity, smolmc_eval_connectivity, SMOLMC_SAMPLE_CONNECTIVITY):
// the connected components of the sites of chosen kinds under a bond list with periodic images, their sizes,
// and whether they wrap the cell -- labelled on the device where the rows lie.  A translation unit of its own, like
// observables.hip.
//
// The definition is connectivity.Connectivity.evaluate.  Everything is integer; the result does not depend on
// the order in which the labels travel, so the device matches the host entry for entry.
//
// One workgroup of 256 threads per row (measured against 1024: a thread that walks more sites in one pass carries a label
// further in it, and fewer passes won over more waves).  The row's Npad bytes go to LDS and are turned into kinds in place, as observables_kernel does.
// Then, per graph, every site gets one 64-bit word in LDS:
//     label << 48 | (off0 + 0x8000) << 32 | (off1 + 0x8000) << 16 | (off2 + 0x8000)
// label is the CALLER's number of the smallest site known to be in the site's component (0xffff: no member), off the
// image sum along a path from that site to this one.  Label and path sum move together in one aligned 64-bit LDS access:
// no thread sees a torn pair.  A pass lets every member look at its neighbours (both directions of every bond, listed per
// site by the host, duplicates removed, four to a 16-byte group and group k of all sites side by side: a wave reads the
// groups of its 64 sites in one coalesced load) and adopt the word of the one with the smallest label below its own, the bond's
// image subtracted.  A word is written by the one thread that owns the site and read by any; the passes work in place,
// so a label crosses many sites in one pass when the sites' order allows.  At every moment a word (L, off) says: there is a
// path from site L to this site with image sum off.  A site adopts a label once, from a site that had adopted it before:
// the path is simple, has at most N - 1 bonds, and |off| <= (N - 1) x SMOLMC_MAX_CONN_IMAGE < 2^15 (checked at set time).
// When a pass changes nothing every member's label is the smallest of its component.  Then every bond with ends of one
// label whose path sums do not match, m = off[i] + w - off[j] != 0, ORs the axes of m into the mask at the label: m is the
// image sum of a closed path, and if no bond has a mismatch on axis a, every closed path sums to zero on a.
//
// Gated graphs (smolmc_set_connectivity_gated): an entry of a site's neighbour list is open in a row when one
// of its channels has at most max_blocked gate sites whose kind is not in the gate mask.  The host gives every entry its
// channel records -- the gate sets of all bond rows that list the entry in either direction, so that s -> t (w) and
// t -> s (-w) have the same ones -- and once per row and gated graph, before the passes, the thread that owns a site tests the
// gate sites' kinds, which are in LDS already, and writes one open bit per entry into LDS (cn_open_bits).  The passes and the mismatch loop
// then read a closed entry as the site itself with image zero, which is what a list that ends early is filled up with: it
// changes nothing.  Whether a graph is gated is read from the launch arguments and is the same for the whole workgroup; an
// ungated graph reads no records and no bits.
//
// No barrier sits under a condition that differs between threads: the "changed" decision is read from LDS by the whole
// workgroup after the barrier, and the pass loop ends after N + 1 passes whatever the data say.
#include "smolmc_common.h"

#define CN_THREADS 256
#define CN_WAVES (CN_THREADS / 64)
#define CN_NOKIND 0xffu
#define CN_NOLABEL 0xffffu
#define CN_BIAS 0x8000

struct ConnArgs {
    const uint8_t *occ;              // rows of Npad bytes
    const int32_t *kind_base;        // [N], engine numbering
    const unsigned long long *mask;  // [G x 4]
    const uint16_t *caller_of;       // [N]
    const uint4 *adj;                // neighbours, four to a group: group k of site s of graph g at adj_off[g] + k N + s
    int adj_off[SMOLMC_MAX_CONN_GRAPHS], adj_groups[SMOLMC_MAX_CONN_GRAPHS];
    const uint2 *chan;               // channel records of the gated graphs: record c of entry e of site s of graph g at
                                     // chan_off[g] + (e << lp | c) N + s, lp = (chan_gate[g] & 0xffff) - 1 (-1: ungated)
    const unsigned long long *gmask; // [G x 4]: the kinds that do not block
    int chan_off[SMOLMC_MAX_CONN_GRAPHS], chan_gate[SMOLMC_MAX_CONN_GRAPHS]; // chan_gate: lp + 1 | max_blocked << 16
    long long *stats;                // [rows x G x 24]
    int32_t *labels;                 // [rows x G x N], caller's numbering, or null
    unsigned long long *passes;      // [2]: max and sum of the passes, or null
    int N, Npad, K, G;
};

// LDS: words u64 [N] | kinds u8 [Npad] | size u16 [N] | axes u8 [N up to 4] | per-wave partial sums i32 [CN_WAVES][24] |
// flags i32 [4] | open bits u8 [open_bytes][N] of a spec with a gated graph: bit 4 (k & 1) + i of byte k / 2 for slot i of group k
__host__ __device__ static inline size_t cn_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static size_t cn_lds_need(int N, int Npad, int open_bytes) {
    return (size_t)N * 8 + (size_t)Npad + cn_up((size_t)N * 2, 4) + cn_up((size_t)N, 4) + (CN_WAVES * SMOLMC_CONN_STATS + 4) * 4 +
           cn_up((size_t)N * open_bytes, 4);
}
size_t smolmc_conn_lds_bytes(int N, int Npad, int open_bytes) {
    const size_t b = cn_lds_need(N, Npad, open_bytes);
    return b <= 65536 ? b : 0;
}

__device__ __forceinline__ unsigned long long cn_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void cn_store(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ bool cn_in_mask(unsigned k, unsigned long long m0, unsigned long long m1, unsigned long long m2,
                                           unsigned long long m3) {
    const unsigned long long mw = k < 64 ? m0 : k < 128 ? m1 : k < 192 ? m2 : m3;
    return k != CN_NOKIND && ((mw >> (k & 63)) & 1ull);
}
__device__ __forceinline__ int cn_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int cn_wave_or(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned cn_wave_max(unsigned v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}

// The open bits of a gated graph, bit 4 (k & 1) + i of open[(k / 2) N + s] for slot i of group k of site s.  Called by the
// whole workgroup (whether a graph is gated does not differ between threads: the two barriers are met by all).  First every
// site gets a byte "my kind lets through" -- in `lets`, the bytes of the axis masks, which the graph does not use before its
// words are set up -- so that a gate site costs one LDS byte and no mask arithmetic.  Then the thread that owns site s looks
// at the site's channel records, record q = e << lp | c for channel c of entry e, and writes the bits; it is the only one to
// read them, in the passes and in the mismatch loop.  Four records are loaded before the first is looked at, so that their
// latencies overlap: the records are the same for all rows and stay in L2, but one load after another is what this phase
// would otherwise be.
__device__ __forceinline__ void cn_open_bits(uint8_t *open, uint8_t *lets, const uint8_t *kinds, const uint2 *chan,
                                             const unsigned long long *gmask, int lp, unsigned most, int groups, int N, int tid) {
    {
        const unsigned long long g0 = gmask[0], g1 = gmask[1], g2 = gmask[2], g3 = gmask[3];
        for (int s = tid; s < N; s += CN_THREADS) lets[s] = cn_in_mask(kinds[s], g0, g1, g2, g3) ? 1 : 0;
    }
    __syncthreads();
    const unsigned T = (4u * (unsigned)groups) << lp; // (T N records: below 2^27, checked at set time)
    for (int s = tid; s < N; s += CN_THREADS) {
        unsigned long long bits = 0; // (at most SMOLMC_MAX_CONN_GATED_NEIGHBOURS = 64 entries)
        for (unsigned q0 = 0; q0 < T; q0 += 4) { // (T is a multiple of four)
            uint2 r[4];
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) r[i] = chan[(q0 + i) * (unsigned)N + (unsigned)s];
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) {
                const unsigned t[4] = {r[i].x & 0xffffu, r[i].x >> 16, r[i].y & 0xffffu, r[i].y >> 16};
                unsigned blocked = 0; // (0xffff: no gate site -- and 0xfffe in the first field: no channel -- read the site's own byte)
#pragma unroll
                for (int j = 0; j < 4; ++j) blocked += (t[j] < (unsigned)N && !lets[t[j] < (unsigned)N ? t[j] : (unsigned)s]) ? 1u : 0u;
                const bool is_open = t[0] != 0xfffeu && blocked <= most;
                bits |= (unsigned long long)(is_open ? 1u : 0u) << ((q0 + i) >> lp);
            }
        }
        for (int b = 0; 2 * b < groups; ++b) open[(size_t)b * N + s] = (uint8_t)(bits >> (8 * b));
    }
    __syncthreads(); // (the bytes of `lets` are the axis masks again)
}

// One pass over the sites this thread owns: true when one of them took a label.  GATED: an entry whose open bit is clear
// reads as the site itself with image zero.
template <bool GATED>
__device__ __forceinline__ bool cn_pass(unsigned long long *word, const uint4 *adj, const uint8_t *open, int groups, int N, int tid) {
    bool changed = false;
    for (int s = tid; s < N; s += CN_THREADS) {
        const unsigned long long me = cn_load(&word[s]);
        const unsigned mine = (unsigned)(me >> 48);
        if (mine == CN_NOLABEL) continue;
        unsigned best = mine;
        unsigned long long take = 0;
        uint32_t via = 0;
        // four neighbours at a time: one 16-byte load that the lanes of a wave make side by side, then the four LDS
        // loads in flight together (a list that ends early is filled up with the site itself, which changes nothing)
        for (int k = 0; k < groups; ++k) {
            const uint4 q = adj[(size_t)k * N + s];
            uint32_t a[4] = {q.x, q.y, q.z, q.w};
            if (GATED) {
                const unsigned ob = (unsigned)open[(size_t)(k >> 1) * N + s] >> (4 * (k & 1));
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (!((ob >> i) & 1u)) a[i] = (uint32_t)s | 8u << 16 | 8u << 20 | 8u << 24;
            }
            unsigned long long o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = cn_load(&word[a[i] & 0xffffu]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((unsigned)(o[i] >> 48) < best) {
                    best = (unsigned)(o[i] >> 48);
                    take = o[i];
                    via = a[i];
                }
        }
        if (best < mine) {
            // the neighbour lies in image w of this site: off[this] = off[neighbour] - w, field by field (no
            // field leaves its 16 bits, see above)
            const unsigned long long w = ((unsigned long long)((via >> 16) & 15u) << 32) |
                                         ((unsigned long long)((via >> 20) & 15u) << 16) | (unsigned long long)((via >> 24) & 15u);
            const unsigned long long eight = (8ull << 32) | (8ull << 16) | 8ull;
            cn_store(&word[s], take + eight - w);
            changed = true;
        }
    }
    return changed;
}

// The bonds whose path sums do not match: the axes of the mismatch go to the label's mask.
template <bool GATED>
__device__ __forceinline__ void cn_mismatch(const unsigned long long *word, const uint4 *adj, const uint8_t *open, uint8_t *axes, int groups,
                                            int N, int tid) {
    for (int s = tid; s < N; s += CN_THREADS) {
        const unsigned long long me = word[s];
        const unsigned mine = (unsigned)(me >> 48);
        if (mine == CN_NOLABEL) continue;
        unsigned bits = 0;
        for (int k = 0; k < groups; ++k) {
            const uint4 q = adj[(size_t)k * N + s];
            uint32_t av[4] = {q.x, q.y, q.z, q.w};
            if (GATED) {
                const unsigned ob = (unsigned)open[(size_t)(k >> 1) * N + s] >> (4 * (k & 1));
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (!((ob >> i) & 1u)) av[i] = (uint32_t)s | 8u << 16 | 8u << 20 | 8u << 24;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t a = av[i];
                const unsigned long long o = word[a & 0xffffu];
                if ((unsigned)(o >> 48) != mine) continue;
                const int d0 = (int)((me >> 32) & 0xffffu) + (int)((a >> 16) & 15u) - 8 - (int)((o >> 32) & 0xffffu);
                const int d1 = (int)((me >> 16) & 0xffffu) + (int)((a >> 20) & 15u) - 8 - (int)((o >> 16) & 0xffffu);
                const int d2 = (int)(me & 0xffffu) + (int)((a >> 24) & 15u) - 8 - (int)(o & 0xffffu);
                bits |= (d0 != 0 ? 1u : 0u) | (d1 != 0 ? 2u : 0u) | (d2 != 0 ? 4u : 0u);
            }
        }
        // (sizes and masks are indexed by the label, a caller's site number: any one-to-one index would do)
        if (bits) atomicOr((unsigned *)(axes + (mine & ~3u)), bits << (8 * (mine & 3u)));
    }
}

__global__ void __launch_bounds__(CN_THREADS) connectivity_kernel(const ConnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cn_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = A.N, Npad = A.Npad, K = A.K;
    unsigned long long *word = (unsigned long long *)cn_smem;
    uint8_t *kinds = cn_smem + (size_t)N * 8;                  // (8 N is a multiple of 8; the row is copied bytewise below)
    uint16_t *size = (uint16_t *)(kinds + Npad);               // (Npad is a multiple of 16)
    uint8_t *axes = (uint8_t *)size + cn_up((size_t)N * 2, 4);
    int32_t *part = (int32_t *)(axes + cn_up((size_t)N, 4));   // [CN_WAVES][24]
    int32_t *flag = part + CN_WAVES * SMOLMC_CONN_STATS;       // [3]: "a site changed" of pass p in flag[p % 3]
    uint8_t *open = (uint8_t *)(flag + 4);                     // open bits of the gated graph at hand
    const size_t row = blockIdx.x;

    {   // the row -> kinds (0xff: not counted), one thread per byte
        const uint8_t *src = A.occ + row * Npad;
        for (int s = tid; s < Npad; s += CN_THREADS) {
            unsigned k = CN_NOKIND;
            if (s < N) {
                const int kb = A.kind_base[s];
                if (kb >= 0) k = (unsigned)kb + src[s];
                if (k >= (unsigned)K) k = CN_NOKIND; // (a code the site's block has no kind for, as in observables_kernel)
            }
            kinds[s] = (uint8_t)k;
        }
    }
    __syncthreads();

    for (int g = 0; g < A.G; ++g) {
        const unsigned long long m0 = A.mask[4 * g], m1 = A.mask[4 * g + 1], m2 = A.mask[4 * g + 2], m3 = A.mask[4 * g + 3];
        const uint4 *adj = A.adj + A.adj_off[g];
        const int groups = A.adj_groups[g];
        const bool gated = (A.chan_gate[g] & 0xffff) != 0; // (from the launch arguments: the same for every thread)
        if (gated)
            cn_open_bits(open, axes, kinds, A.chan + A.chan_off[g], A.gmask + 4 * g, (A.chan_gate[g] & 0xffff) - 1,
                         (unsigned)A.chan_gate[g] >> 16, groups, N, tid);
        // members start as their own component, path sum zero
        for (int s = tid; s < N; s += CN_THREADS) {
            const unsigned k = kinds[s];
            const bool member = cn_in_mask(k, m0, m1, m2, m3);
            const unsigned long long zero = ((unsigned long long)CN_BIAS << 32) | ((unsigned long long)CN_BIAS << 16) | CN_BIAS;
            word[s] = ((unsigned long long)(member ? A.caller_of[s] : CN_NOLABEL) << 48) | zero;
            size[s] = 0;
            axes[s] = 0;
        }
        if (tid < 3) flag[tid] = 0;
        __syncthreads();

        // ---- the passes: at most N + 1 of them -----------------------------------------------------------------------------
        int passes = 0;
        for (int pass = 0; pass <= N; ++pass) {
            const bool changed = gated ? cn_pass<true>(word, adj, open, groups, N, tid) : cn_pass<false>(word, adj, open, groups, N, tid);
            if (changed) flag[pass % 3] = 1;
            __syncthreads();
            const int any = flag[pass % 3];          // (the same LDS word for every thread, written before the barrier)
            if (tid == 0) flag[(pass + 2) % 3] = 0;  // (last read before this barrier, next written after the next one)
            passes = pass + 1;
            if (!any) break;
        }
        // (the break is taken by every thread or none; the writes of the last pass are behind its barrier)

        // ---- the bonds whose path sums do not match: the axes of the mismatch go to the label's mask ----------------------
        if (gated) cn_mismatch<true>(word, adj, open, axes, groups, N, tid);
        else cn_mismatch<false>(word, adj, open, axes, groups, N, tid);
        // ---- the sizes at the labels: the lanes of a wave that share the first lane's label add once ---------------------
        for (int s0 = wave * 64; s0 < N; s0 += CN_THREADS) { // (wave-uniform bounds: every lane takes part in the ballot)
            const int s = s0 + lane;
            const unsigned mine = s < N ? (unsigned)(word[s] >> 48) : CN_NOLABEL;
            const unsigned long long live = __ballot(mine != CN_NOLABEL);
            if (!live) continue;
            const int first = __ffsll((long long)live) - 1;
            const unsigned lead = (unsigned)__shfl((int)mine, first, 64);
            const unsigned long long same = __ballot(mine == lead);
            unsigned add = 0, at = mine;
            if (lane == first) add = (unsigned)__popcll(same);
            else if (mine != CN_NOLABEL && mine != lead) add = 1;
            if (add) atomicAdd((unsigned *)((uint8_t *)size + ((at * 2) & ~3u)), add << (16 * (at & 1u)));
        }
        __syncthreads();

        // ---- the 24 numbers: a component is found at the site that carries its own number ------------------------------------
        int n_members = 0, n_comp = 0, n_wrap = 0, wrap_sites = 0, wrap_axes = 0, hist = 0;
        unsigned sum_sq = 0, top = 0; // top: size << 16 | 0xffff - label -- the largest, among equals the smallest label
        for (int s0 = wave * 64; s0 < N; s0 += CN_THREADS) {
            const int s = s0 + lane;
            int sz = 0, ax = 0;
            unsigned lab = 0;
            if (s < N) {
                lab = A.caller_of[s];
                if ((unsigned)(word[s] >> 48) == lab) { sz = size[lab]; ax = axes[lab]; }
            }
            if (sz) {
                n_members += sz; n_comp += 1; sum_sq += (unsigned)sz * (unsigned)sz;
                if (ax) { n_wrap += 1; wrap_sites += sz; wrap_axes |= ax; }
                top = max(top, ((unsigned)sz << 16) | (0xffffu - lab));
            }
            const int bin = sz ? 31 - __clz(sz) : -1;
            for (int b = 0; b < 16; ++b) { // lane b keeps the count of bin b
                const int n = __popcll(__ballot(bin == b));
                if (lane == b) hist += n;
            }
        }
        n_members = cn_wave_sum(n_members); n_comp = cn_wave_sum(n_comp); n_wrap = cn_wave_sum(n_wrap);
        wrap_sites = cn_wave_sum(wrap_sites); sum_sq = (unsigned)cn_wave_sum((int)sum_sq);
        wrap_axes = cn_wave_or(wrap_axes); top = cn_wave_max(top);
        int32_t *mine_part = part + wave * SMOLMC_CONN_STATS;
        if (lane == 0) {
            mine_part[0] = n_members; mine_part[1] = n_comp; mine_part[2] = (int32_t)top; mine_part[3] = (int32_t)sum_sq;
            mine_part[4] = n_wrap; mine_part[5] = wrap_sites; mine_part[6] = wrap_axes; mine_part[7] = 0;
        }
        if (lane < 16) mine_part[SMOLMC_CONN_HIST + lane] = hist;
        __syncthreads();
        if (tid < SMOLMC_CONN_STATS) {
            long long v = 0;
            unsigned t = 0;
            for (int w = 0; w < CN_WAVES; ++w) t = max(t, (unsigned)part[w * SMOLMC_CONN_STATS + 2]);
            if (tid == SMOLMC_CONN_LARGEST) v = t >> 16;
            else if (tid == SMOLMC_CONN_LARGEST_WRAP_AXES) v = t ? axes[0xffffu - (t & 0xffffu)] : 0;
            else if (tid == SMOLMC_CONN_WRAP_AXES)
                for (int w = 0; w < CN_WAVES; ++w) v |= part[w * SMOLMC_CONN_STATS + tid];
            else if (tid == SMOLMC_CONN_SUM_SQ)
                for (int w = 0; w < CN_WAVES; ++w) v += (unsigned)part[w * SMOLMC_CONN_STATS + tid];
            else
                for (int w = 0; w < CN_WAVES; ++w) v += part[w * SMOLMC_CONN_STATS + tid];
            A.stats[(row * A.G + g) * SMOLMC_CONN_STATS + tid] = v;
        }
        if (A.labels) {
            int32_t *out = A.labels + (row * A.G + g) * (size_t)N;
            for (int s = tid; s < N; s += CN_THREADS) {
                const unsigned lab = (unsigned)(word[s] >> 48);
                out[A.caller_of[s]] = lab == CN_NOLABEL ? -1 : (int32_t)lab;
            }
        }
        if (A.passes && tid == 0) {
            atomicMax(&A.passes[0], (unsigned long long)passes);
            atomicAdd(&A.passes[1], (unsigned long long)passes);
        }
        __syncthreads(); // (the next graph overwrites words, sizes, masks and partial sums)
    }
}

int smolmc_conn_launch(smolmc_handle *h, const uint8_t *d_occ8, size_t rows, long long *d_stats, int32_t *d_labels) {
    SmolmcConn &S = h->conn;
    if (!S.G) return fail("no connectivity spec set (smolmc_set_connectivity)");
    if (!rows) return 0;
    if (rows > 0x7fffffffull) return fail("connectivity: more than 2^31 rows in one launch");
    if (!d_stats) return fail("connectivity: null output");
    ConnArgs A;
    A.occ = d_occ8; A.kind_base = S.d_kind_base; A.mask = S.d_mask; A.caller_of = S.d_caller_of;
    A.adj = (const uint4 *)S.d_adj;
    A.chan = S.d_chan; A.gmask = S.d_gate_mask;
    for (int g = 0; g < SMOLMC_MAX_CONN_GRAPHS; ++g) {
        A.adj_off[g] = S.adj_off[g]; A.adj_groups[g] = S.adj_groups[g];
        A.chan_off[g] = S.chan_off[g];
        A.chan_gate[g] = S.chan_per[g] ? (__builtin_ctz((unsigned)S.chan_per[g]) + 1) | S.max_blocked[g] << 16 : 0;
    }
    A.stats = d_stats; A.labels = d_labels; A.passes = S.d_passes;
    A.N = h->N; A.Npad = h->Npad; A.K = S.K; A.G = S.G;
    if (!S.ev[0])
        for (hipEvent_t &e : S.ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipMemsetAsync(S.d_passes, 0, 16, h->stream));
    HIPCHK(hipEventRecord(S.ev[0], h->stream));
    hipLaunchKernelGGL(connectivity_kernel, dim3((unsigned)rows), dim3(CN_THREADS), S.lds, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], h->stream));
    return 0;
}

void smolmc_conn_free(SmolmcConn &S) {
    if (S.arena) hipFree(S.arena);
    for (hipEvent_t e : S.ev)
        if (e) hipEventDestroy(e);
    S = SmolmcConn();
}

// elapsed device time of the last launch of the connectivity kernel in ms (tools/connectivity_timing.py); a measuring hook
// like smolmc_debug_obs_kernel_ms, not part of the C-ABI
extern "C" int smolmc_debug_connectivity_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    const SmolmcConn &S = h->conn;
    if (!S.ev[0]) return fail("the connectivity kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.ev[1]));
    HIPCHK(hipEventElapsedTime(ms, S.ev[0], S.ev[1]));
    return 0;
}

// the passes of the last launch: the most a (row, graph) took and the sum over all of them; a measuring hook likewise
extern "C" int smolmc_debug_connectivity_passes(smolmc_handle *h, long long *most, long long *sum) {
    if (!h || !most || !sum) return fail("null argument");
    const SmolmcConn &S = h->conn;
    if (!S.ev[0]) return fail("the connectivity kernel has not been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(S.ev[1]));
    unsigned long long v[2];
    HIPCHK(hipMemcpy(v, S.d_passes, 16, hipMemcpyDeviceToHost));
    *most = (long long)v[0];
    *sum = (long long)v[1];
    return 0;
}

// ---- the C-ABI of the connectivity spec ----------------------------------------------------------------------------------
extern "C" int smolmc_set_connectivity(smolmc_handle *h, const smolmc_connectivity *sp) {
    return smolmc_set_connectivity_gated(h, sp, nullptr);
}

namespace {
// one direction of one bond row: the entry of `site`'s neighbour list and the row's gate sites (engine numbering, ascending,
// 0xffff for none: a row without gates is all ones)
struct ConnEnt {
    int32_t site;
    uint32_t ent;
    uint64_t chan;
    bool operator<(const ConnEnt &o) const { return site != o.site ? site < o.site : ent != o.ent ? ent < o.ent : chan < o.chan; }
    bool operator==(const ConnEnt &o) const { return site == o.site && ent == o.ent && chan == o.chan; }
};
const uint64_t CN_NO_GATES = ~0ull;
} // namespace

extern "C" int smolmc_set_connectivity_gated(smolmc_handle *h, const smolmc_connectivity *sp, const smolmc_conn_gates *gt) {
    if (!h) return fail("null handle");
    if (gt && !sp) return fail("connectivity: gates without a spec");
    HIPCHK(hipSetDevice(h->device));
    TRY(smolmc_ring_guard(h, SMOLMC_SAMPLE_CONNECTIVITY, "smolmc_set_connectivity", "SMOLMC_SAMPLE_CONNECTIVITY"));
    if (h->stats.n_keys && h->stats.n_conn_cols)
        return fail("smolmc_set_connectivity while a statistics record with connectivity columns depends on the spec (call "
                    "smolmc_set_statistics(h, NULL) first)");
    SmolmcConn S;
    if (sp) {
        const int N = h->N, K = sp->n_kinds, G = sp->n_graphs;
        char msg[256];
        if (G < 1 || G > SMOLMC_MAX_CONN_GRAPHS) {
            snprintf(msg, sizeof msg, "connectivity: n_graphs must be 1..%d, got %d", SMOLMC_MAX_CONN_GRAPHS, G);
            return fail(msg);
        }
        if (!sp->kind_base || !sp->member_mask || !sp->bond_ptr) return fail("connectivity: null argument");
        if (K < 1 || K > 254) return fail("connectivity: n_kinds must be 1..254 (a kind is staged as one byte)");
        S.lds = smolmc_conn_lds_bytes(N, h->Npad);
        if (!S.lds) {
            snprintf(msg, sizeof msg, "connectivity: a row of %d sites is too long for the LDS plan: a label with its path sum, a size and "
                     "a mask take 11 bytes a site next to the row's %d, 65536 at most", N, h->Npad);
            return fail(msg);
        }
        if ((long long)N * SMOLMC_MAX_CONN_IMAGE > SMOLMC_MAX_CONN_PATH_SUM) {
            snprintf(msg, sizeof msg, "connectivity: %d sites x SMOLMC_MAX_CONN_IMAGE = %d is larger than SMOLMC_MAX_CONN_PATH_SUM = %d: "
                     "the image sum of a path could overflow its 16 bits", N, SMOLMC_MAX_CONN_IMAGE, SMOLMC_MAX_CONN_PATH_SUM);
            return fail(msg);
        }
        std::vector<int32_t> kb;
        TRY(smolmc_kind_base_in(h, sp->kind_base, K, "connectivity", kb));
        for (int g = 0; g < G; ++g)
            for (int k = K; k < 256; ++k)
                if ((sp->member_mask[4 * g + (k >> 6)] >> (k & 63)) & 1ull) {
                    snprintf(msg, sizeof msg, "connectivity: graph %d names member kind %d, n_kinds is %d: kind out of range", g, k, K);
                    return fail(msg);
                }
        if (sp->bond_ptr[0] != 0) return fail("connectivity: bond_ptr[0] must be 0");
        for (int g = 0; g < G; ++g)
            if (sp->bond_ptr[g + 1] < sp->bond_ptr[g]) return fail("connectivity: bond_ptr must not decrease");
        const int64_t nb = sp->bond_ptr[G];
        if (nb > 0 && (!sp->bonds || !sp->images)) return fail("connectivity: null argument");
        // the gates: their masks and limits, and the gate sites of every bond row
        if (gt) {
            if (!gt->gate_mask || !gt->max_blocked || !gt->gate_ptr) return fail("connectivity: null argument (gates)");
            for (int g = 0; g < G; ++g) {
                for (int k = K; k < 256; ++k)
                    if ((gt->gate_mask[4 * g + (k >> 6)] >> (k & 63)) & 1ull) {
                        snprintf(msg, sizeof msg, "connectivity: graph %d names gate kind %d, n_kinds is %d: kind out of range", g, k, K);
                        return fail(msg);
                    }
                if (gt->max_blocked[g] < 0 || gt->max_blocked[g] > SMOLMC_MAX_CONN_GATES) {
                    snprintf(msg, sizeof msg, "connectivity: graph %d has max_blocked = %d, outside 0..SMOLMC_MAX_CONN_GATES = %d: "
                             "max_blocked out of range", g, (int)gt->max_blocked[g], SMOLMC_MAX_CONN_GATES);
                    return fail(msg);
                }
            }
            if (gt->gate_ptr[0] != 0) return fail("connectivity: gate_ptr[0] must be 0");
            for (int64_t b = 0; b < nb; ++b) {
                const int64_t n = gt->gate_ptr[b + 1] - gt->gate_ptr[b];
                if (n < 0) return fail("connectivity: gate_ptr must not decrease");
                if (n > SMOLMC_MAX_CONN_GATES) {
                    snprintf(msg, sizeof msg, "connectivity: bond row %lld has %lld gate sites, SMOLMC_MAX_CONN_GATES = %d: too many gates "
                             "on a row", (long long)b, (long long)n, SMOLMC_MAX_CONN_GATES);
                    return fail(msg);
                }
            }
            if (gt->gate_ptr[nb] > 0 && !gt->gate_sites) return fail("connectivity: null argument (gates)");
            for (int64_t b = 0; b < nb; ++b)
                for (int64_t q = gt->gate_ptr[b]; q < gt->gate_ptr[b + 1]; ++q) {
                    const int32_t t = gt->gate_sites[q];
                    if (t < 0 || t >= N) {
                        snprintf(msg, sizeof msg, "connectivity: bond row %lld has gate site %d, %d sites: gate site out of range", (long long)b,
                                 (int)t, N);
                        return fail(msg);
                    }
                    if (sp->kind_base[t] < 0) {
                        snprintf(msg, sizeof msg, "connectivity: bond row %lld has gate site %d with kind_base %d: a gate site must be a "
                                 "counted site", (long long)b, (int)t, (int)sp->kind_base[t]);
                        return fail(msg);
                    }
                }
        }
        // the neighbours of every site: both directions of every bond, engine numbering, duplicates dropped (a bond listed
        // twice joins what it joined once); in a gated graph every entry with the channels of the rows that list it
        std::vector<uint32_t> adj;
        std::vector<uint2> chan;
        std::vector<ConnEnt> ent;
        int open_bytes = 0;
        for (int g = 0; g < G; ++g) {
            ent.clear();
            bool gated = false;
            for (int64_t b = sp->bond_ptr[g]; b < sp->bond_ptr[g + 1]; ++b) {
                const int32_t i = sp->bonds[2 * b], j = sp->bonds[2 * b + 1];
                if (i < 0 || i >= N || j < 0 || j >= N) {
                    snprintf(msg, sizeof msg, "connectivity: graph %d bond %lld = (%d, %d), %d sites: bond out of range", g,
                             (long long)(b - sp->bond_ptr[g]), (int)i, (int)j, N);
                    return fail(msg);
                }
                const int8_t *w = sp->images + 3 * b;
                for (int a = 0; a < 3; ++a)
                    if (w[a] < -SMOLMC_MAX_CONN_IMAGE || w[a] > SMOLMC_MAX_CONN_IMAGE) {
                        snprintf(msg, sizeof msg, "connectivity: graph %d bond %lld has image (%d, %d, %d), beyond SMOLMC_MAX_CONN_IMAGE = %d: "
                                 "image out of range", g, (long long)(b - sp->bond_ptr[g]), (int)w[0], (int)w[1], (int)w[2],
                                 SMOLMC_MAX_CONN_IMAGE);
                        return fail(msg);
                    }
                const int si = h->relabelled ? h->new_of[i] : i, sj = h->relabelled ? h->new_of[j] : j;
                if (si == sj && !w[0] && !w[1] && !w[2]) continue; // (a site joined to itself in its own cell: no bond)
                uint64_t ch = CN_NO_GATES;
                if (gt && gt->gate_ptr[b + 1] > gt->gate_ptr[b]) {
                    uint16_t t[SMOLMC_MAX_CONN_GATES] = {0xffff, 0xffff, 0xffff, 0xffff};
                    const int n = (int)(gt->gate_ptr[b + 1] - gt->gate_ptr[b]);
                    for (int q = 0; q < n; ++q) {
                        const int32_t c = gt->gate_sites[gt->gate_ptr[b] + q];
                        t[q] = (uint16_t)(h->relabelled ? h->new_of[c] : c);
                    }
                    std::sort(t, t + n); // (a set with multiplicities: two rows with the same gates are one channel)
                    ch = (uint64_t)t[0] | (uint64_t)t[1] << 16 | (uint64_t)t[2] << 32 | (uint64_t)t[3] << 48;
                    gated = true;
                }
                // seen from i the neighbour j lies in image w, seen from j the neighbour i lies in image -w
                ent.push_back({si, (uint32_t)sj | (uint32_t)(w[0] + 8) << 16 | (uint32_t)(w[1] + 8) << 20 | (uint32_t)(w[2] + 8) << 24, ch});
                ent.push_back({sj, (uint32_t)si | (uint32_t)(8 - w[0]) << 16 | (uint32_t)(8 - w[1]) << 20 | (uint32_t)(8 - w[2]) << 24, ch});
            }
            std::sort(ent.begin(), ent.end());
            ent.erase(std::unique(ent.begin(), ent.end()), ent.end());
            // the entries of a site in this order, four to a group, group k of all sites side by side; a list that ends early
            // is filled up with the site itself.  An entry with a row without gates is always open: that row is its one
            // channel (all ones sorts last among the channels of an entry).
            std::vector<int> deg((size_t)N, 0);
            int most = 0, per = 0;
            for (size_t x = 0; x < ent.size();) {
                size_t y = x;
                while (y < ent.size() && ent[y].site == ent[x].site && ent[y].ent == ent[x].ent) ++y;
                most = std::max(most, ++deg[ent[x].site]);
                per = std::max<long long>(per, ent[y - 1].chan == CN_NO_GATES ? 1 : (long long)std::min<size_t>(y - x, 0x10000));
                x = y;
            }
            const int groups = (most + 3) / 4;
            if ((adj.size() + (size_t)groups * N * 4) * 4 > ((size_t)1 << 30)) return fail("connectivity: the neighbour lists take more than 1 GiB");
            S.adj_off[g] = (int)(adj.size() / 4);
            S.adj_groups[g] = groups;
            const size_t base = adj.size();
            adj.resize(base + (size_t)groups * N * 4);
            for (int k = 0; k < groups; ++k)
                for (int s = 0; s < N; ++s)
                    for (int i = 0; i < 4; ++i) adj[base + ((size_t)k * N + s) * 4 + i] = (uint32_t)s | 8u << 16 | 8u << 20 | 8u << 24;
            size_t cbase = 0;
            if (gated) {
                if (most > SMOLMC_MAX_CONN_GATED_NEIGHBOURS) {
                    snprintf(msg, sizeof msg, "connectivity: graph %d is gated and a site has %d neighbour entries, "
                             "SMOLMC_MAX_CONN_GATED_NEIGHBOURS = %d: the open-bit plan keeps 8 bytes of bits a site at most", g, most,
                             SMOLMC_MAX_CONN_GATED_NEIGHBOURS);
                    return fail(msg);
                }
                if (per > 0x4000) {
                    snprintf(msg, sizeof msg, "connectivity: graph %d has a neighbour entry with more than 16384 distinct channels", g);
                    return fail(msg);
                }
                while (per & (per - 1)) ++per; // (a power of two: the kernel finds the entry of a record by a shift)
                if ((chan.size() + (size_t)groups * 4 * per * N) * 8 > ((size_t)1 << 30)) return fail("connectivity: the channel records take more than 1 GiB");
                open_bytes = std::max(open_bytes, (4 * groups + 7) / 8);
                S.gated_mask |= 1 << g;
                S.chan_off[g] = (int)chan.size();
                S.chan_per[g] = per;
                S.max_blocked[g] = gt->max_blocked[g];
                cbase = chan.size();
                chan.resize(cbase + (size_t)groups * 4 * per * N, make_uint2(0xfffefffeu, 0xfffefffeu)); // (no channel)
            }
            std::fill(deg.begin(), deg.end(), 0);
            for (size_t x = 0; x < ent.size();) {
                size_t y = x;
                while (y < ent.size() && ent[y].site == ent[x].site && ent[y].ent == ent[x].ent) ++y;
                const int s = ent[x].site, n = deg[s]++;
                adj[base + ((size_t)(n / 4) * N + s) * 4 + (n & 3)] = ent[x].ent;
                if (gated) {
                    const size_t first = ent[y - 1].chan == CN_NO_GATES ? y - 1 : x;
                    for (size_t c = first; c < y; ++c) {
                        chan[cbase + ((size_t)n * per + (c - first)) * N + s] = make_uint2((uint32_t)ent[c].chan, (uint32_t)(ent[c].chan >> 32));
                        S.n_channels += 1;
                    }
                }
                x = y;
            }
        }
        if (open_bytes) {
            S.lds = smolmc_conn_lds_bytes(N, h->Npad, open_bytes);
            if (!S.lds) {
                snprintf(msg, sizeof msg, "connectivity: a gated row of %d sites is too long for the LDS plan: %d bytes of open bits a site "
                         "next to the rest make %zu bytes, 65536 at most", N, open_bytes, cn_lds_need(N, h->Npad, open_bytes));
                return fail(msg);
            }
        }
        std::vector<uint16_t> caller_of((size_t)N);
        for (int s = 0; s < N; ++s) caller_of[s] = (uint16_t)(h->relabelled ? h->old_of[s] : s);
        S.K = K; S.G = G;
        S.kind_base = kb;
        // one arena: the spec's arrays, then the scratch of smolmc_update_statistics
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up256(std::max<size_t>(bytes, 16)); return o; };
        const size_t o_kb = take((size_t)N * 4), o_mk = take((size_t)G * 32), o_co = take((size_t)N * 2),
                     o_ad = take(adj.size() * 4),
                     o_us = take((size_t)h->R * G * SMOLMC_CONN_STATS * 8), o_ps = take(16),
                     o_gm = take((size_t)G * 32), o_ch = take(chan.size() * 8);
        hipError_t e = hipMalloc((void **)&S.arena, at);
        if (e != hipSuccess) return fail(std::string("connectivity: hipMalloc: ") + hipGetErrorString(e));
        unsigned char *d = S.arena;
        S.d_kind_base = (int32_t *)(d + o_kb); S.d_mask = (unsigned long long *)(d + o_mk); S.d_caller_of = (uint16_t *)(d + o_co);
        S.d_adj = (uint32_t *)(d + o_ad); S.u_stats = (long long *)(d + o_us);
        S.d_passes = (unsigned long long *)(d + o_ps);
        S.d_gate_mask = (unsigned long long *)(d + o_gm); S.d_chan = (uint2 *)(d + o_ch);
        e = hipMemcpy(S.d_kind_base, kb.data(), (size_t)N * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = gt ? hipMemcpy(S.d_gate_mask, gt->gate_mask, (size_t)G * 32, hipMemcpyHostToDevice) : hipMemset(S.d_gate_mask, 0, (size_t)G * 32);
        if (e == hipSuccess && !chan.empty()) e = hipMemcpy(S.d_chan, chan.data(), chan.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(S.d_mask, sp->member_mask, (size_t)G * 32, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(S.d_caller_of, caller_of.data(), (size_t)N * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess && !adj.empty()) e = hipMemcpy(S.d_adj, adj.data(), adj.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(S.d_passes, 0, 16);
        if (e != hipSuccess) {
            smolmc_conn_free(S);
            return fail(std::string("connectivity upload: ") + hipGetErrorString(e));
        }
    }
    TRY(smolmc_ring_forget(h, SMOLMC_SAMPLE_CONNECTIVITY));
    smolmc_conn_free(h->conn);
    h->conn = S;
    return 0;
}

extern "C" int smolmc_connectivity_shape(smolmc_handle *h, int *n_graphs, int *n_kinds) {
    if (!h) return fail("null handle");
    if (n_graphs) *n_graphs = h->conn.G;
    if (n_kinds) *n_kinds = h->conn.G ? h->conn.K : 0;
    return 0;
}

extern "C" int smolmc_connectivity_gates(smolmc_handle *h, int *gated_graph_mask, int64_t *n_channels) {
    if (!h) return fail("null handle");
    if (gated_graph_mask) *gated_graph_mask = h->conn.G ? h->conn.gated_mask : 0;
    if (n_channels) *n_channels = h->conn.G ? h->conn.n_channels : 0;
    return 0;
}

extern "C" int smolmc_eval_connectivity(smolmc_handle *h, const int32_t *occ, int nocc, int64_t *stats, int32_t *labels) {
    if (!h) return fail("null handle");
    const SmolmcConn &S = h->conn;
    if (!S.G) return fail("no connectivity spec set: call smolmc_set_connectivity first");
    HIPCHK(hipSetDevice(h->device));
    const uint8_t *d_occ8;
    size_t rows;
    TRY(smolmc_eval_rows(h, occ, nocc, S.kind_base, S.K, "connectivity", &d_occ8, &rows));
    if (!rows) return 0;
    const size_t ns = rows * S.G * SMOLMC_CONN_STATS, nl = labels ? rows * S.G * h->N : 0;
    DevScratch out;
    TRY(out.alloc(std::max<size_t>(ns * 8 + nl * 4, 16)));
    unsigned char *d_out = out.as<unsigned char>();
    TRY(smolmc_conn_launch(h, d_occ8, rows, (long long *)d_out, labels ? (int32_t *)(d_out + ns * 8) : nullptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (stats) HIPCHK(hipMemcpy(stats, d_out, ns * 8, hipMemcpyDeviceToHost));
    if (labels) HIPCHK(hipMemcpy(labels, d_out + ns * 8, nl * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_sample_connectivity(smolmc_handle *h, int64_t *stats) {
    const SampleSlot *sl;
    size_t rows;
    TRY(smolmc_sample_block(h, SMOLMC_SAMPLE_CONNECTIVITY, "the connectivity stats were not recorded (flags bit 7)", &sl, &rows));
    if (stats) smolmc_host_copy(stats, sl->hst + sl->o_conn, rows * (size_t)h->conn.G * SMOLMC_CONN_STATS * 8);
    return 0;
}
