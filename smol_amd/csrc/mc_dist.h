// mc_dist.h -- distance-objective Metropolis kernel (special quasirandom structures) and its launch template.
//
// The objective of smol's DistanceProcessor (smol/moca/processor/distance.py:20-182):
//     H = -w L + sum_k W_k |f_k - t_k|
// f = the intensive correlation (or cluster-interaction) vector, t the target, W the target weights, L the
// largest diameter up to which every feature matches the target within match_tol (distance.py:307-332).
//
// One wave64 per walker, DIST_WPB walkers per workgroup.  Per walker in LDS: the signed features f (fp64, F),
// the step's feature changes df (fp64, F), the occupancy (u8, Npad) and the best occupancy seen so far
// (u8, Npad).  The target, the weights and the tensors are staged once per workgroup.
//
// A proposal (Flip / Swap from the lean kernels' Philox stream, oracle/smolmc_oracle.c propose_step) is
// priced flip by flip with sequential-flip semantics (expansion.py:217-229): the flip's change of every feature
// it touches comes from the site's local cluster rows (evaluator.pyx:211-317); lane q of the pass takes the
// q-th (local record, function) pair of the site and sums its rows in their order -- one lane per feature and
// pass, no atomics: runs are reproducible.  The flip is then applied in LDS and the next flip of the step sees
// it; a rejected step is reverted.  A cluster that holds the flipped site twice (small, aliased cells) sees the
// new species at both places.
#pragma once
#include "mc_lean.h"

#define SMOLMC_DIST_MAX_F 256 // features of a distance handle (four 64-lane chunks of the exact-match ballot)
#define SMOLMC_DIST_WPB 4     // walkers (waves) per workgroup

// The work of one flip is split into chunks of at most DIST_ROWS consecutive cluster rows of one
// (local record, function) pair of the site: lane c of a pass sums chunk c in row order (one round of loads
// per chunk), the pair's lane then adds its chunks' partial sums in chunk order -- a fixed order, no atomics.
#define DIST_ROWS 4
struct DistChunk {
    int32_t row_off; // first row in DistParams::rows (engine site numbering)
    int32_t t_off;   // offset of the function's tensor in the LDS copy of DistParams::tens
    int16_t n, I;    // rows of the chunk (<= DIST_ROWS), sites per cluster
    int16_t st[6];   // tensor strides of the members
    int32_t pad[2];
};
// a (local record, function) pair of a site: where its chunks are and how its sum is normalised
struct DistPair {
    int32_t feat;    // feature index (bit_id + k, or the orbit id in interaction mode)
    int32_t J;       // cluster rows of the record
    int32_t c0, nc;  // its chunks: c0 .. c0 + nc - 1 of the site
    double ratio;    // cluster_ratio of the record
};

struct DistParams {
    int R, N, Npad, F, nsub, step_type, nchunk, n_groups;
    int lds_per_wave, lds_shared;
    // sublattices (engine numbering, as KParams)
    const int *sub_ptr, *sub_sites, *sub_code_ptr, *sub_codes;
    const double *sub_cum;
    // per-site pairs
    const long long *pair_ptr;  // [N+1]
    const DistPair *pairs;
    const long long *chunk_ptr; // [N+1]
    const DistChunk *chunks;
    int max_chunks;             // most chunks of one site (LDS cells of the partial sums per walker)
    const uint4 *rows;     // cluster rows, eight u16 sites each (members beyond I: site 0, stride 0)
    const double *tens;    // the feature mode's tensors, staged in LDS per workgroup
    long long tens_len;
    // objective
    const double *target;                 // [F]
    const double *wts;                    // [F] natural parameter of feature k >= 1 (wts[0] unused)
    double w_match, tol, size;     // size: prim cells of the supercell (features / size, distance.py:133-135)
    const double *gdiam;                  // [n_groups]
    const unsigned long long *gmask;      // [n_groups][nchunk] features of the groups up to g
    const double *ext;                    // [R][F] extensive features of the occupancies at launch start
    // walker state
    uint8_t *occ;
    double *enthalpy, *features;
    const double *beta;
    const uint64_t *seeds;
    uint64_t *nsteps, *nacc;
    uint8_t *last_acc;
    uint8_t *best_occ;
    double *best_H;
    uint64_t *best_step;
    int init_best; // the launch starts the best record afresh from the current state
    long long steps;
    SampleBufs smp;
    // replay
    const int *rp_steps;   // [R][steps][SMOLMC_STEP_ROW]
    const double *rp_u;    // [R][steps]
    uint8_t *rp_acc;       // [R][steps]
    double *rp_H;          // [R][steps]
};

__device__ __forceinline__ void dist_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// L: diameter of the last group g such that every group up to g is matched (distance.py:307-332)
__device__ __forceinline__ double dist_match_diameter(const DistParams &P, const unsigned long long (&m)[4]) {
    double L = 0.0;
    for (int g = 0; g < P.n_groups; ++g) {
        bool all = true;
        for (int c = 0; c < P.nchunk; ++c) {
            const unsigned long long gm = P.gmask[g * P.nchunk + c];
            all &= (m[c] & gm) == gm;
        }
        if (!all) break;
        L = P.gdiam[g];
    }
    return L;
}

// The change of every feature the flip (site s -> code nw) touches, added to df.  Chunk pass: lane c of round u
// takes chunk 64 (u + NSLOT t) + c of the site and leaves its partial sum in part[]; pair pass: the lane of pair k
// adds its chunks' partials in order and divides by ratio and J as evaluator.pyx:262.
template <int NSLOT>
__device__ __forceinline__ void dist_flip_pass(const DistParams &P, const double *tens, const uint8_t *occ, double *df,
                                               double *part, int lane, int s, int nw) {
    const long long c0s = P.chunk_ptr[s], p0 = P.pair_ptr[s];
    const int nch = (int)(P.chunk_ptr[s + 1] - c0s), np = (int)(P.pair_ptr[s + 1] - p0);
    for (int cb = 0; cb < nch; cb += 64 * NSLOT) {
#pragma unroll
        for (int u = 0; u < NSLOT; ++u) {
            const int c = cb + u * 64 + lane;
            if (c < nch) {
                const DistChunk ck = P.chunks[c0s + c];
                const uint4 *rw = P.rows + ck.row_off;
                const double *T = tens + ck.t_off;
                uint4 rr[DIST_ROWS];
#pragma unroll
                for (int b = 0; b < DIST_ROWS; ++b) rr[b] = rw[b < ck.n ? b : 0];
                double p = 0.0;
#pragma unroll
                for (int b = 0; b < DIST_ROWS; ++b) {
                    const uint32_t w[3] = {rr[b].x, rr[b].y, rr[b].z};
                    int ii = 0, ifl = 0;
#pragma unroll
                    for (int m = 0; m < SMOLMC_MAX_CLUSTER_SITES; ++m) {
                        if (m < ck.I) {
                            const int x = (int)bounded((w[m >> 1] >> ((m & 1) * 16)) & 0xffffu, (uint32_t)P.N);
                            const int o = occ[x];
                            ii += ck.st[m] * o;
                            ifl += ck.st[m] * (x == s ? nw : o);
                        }
                    }
#ifdef SMOLMC_BOUNDS
                    if ((long long)ck.t_off + ii >= P.tens_len || (long long)ck.t_off + ifl >= P.tens_len) __builtin_trap();
#endif
                    if (b < ck.n) p += T[ifl] - T[ii];
                }
                part[c] = p;
            }
        }
    }
    dist_wave_sync();
    for (int k = lane; k < np; k += 64) {
        const DistPair pr = P.pairs[p0 + k];
        double p = 0.0;
        for (int c = pr.c0; c < pr.c0 + pr.nc; ++c) p += part[c];
        df[pr.feat] += p / pr.ratio / pr.J;
    }
}

template <int NSLOT, bool REPLAY>
// (held to 128 VGPRs: four walkers per SIMD, 4096 walkers on the 1024 SIMDs in one round)
__global__ void __launch_bounds__(64 * SMOLMC_DIST_WPB) __attribute__((amdgpu_waves_per_eu(4)))
mc_dist_kernel(const DistParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dist_smem[];
    const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63; // (the walker index lives in SGPRs)
    const int F = P.F;
    double *tgt = (double *)dist_smem, *wt = tgt + F, *tens = wt + F;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        tgt[k] = P.target[k];
        wt[k] = k ? P.wts[k] : 0.0;
    }
    for (int k = threadIdx.x; k < (int)P.tens_len; k += blockDim.x) tens[k] = P.tens[k];
    __syncthreads();
    const int r = blockIdx.x * SMOLMC_DIST_WPB + wave;
    if (r >= P.R) return; // (no barrier below)
    unsigned char *mine = dist_smem + P.lds_shared + (size_t)wave * P.lds_per_wave;
    double *f = (double *)mine, *df = f + F, *part = df + F;
    uint8_t *occ = (uint8_t *)(part + P.max_chunks), *best = occ + P.Npad;
    {
        const uint32_t *go = (const uint32_t *)(P.occ + (size_t)r * P.Npad);
        const uint32_t *gb = (const uint32_t *)(P.best_occ + (size_t)r * P.Npad);
        for (int i = lane; i < P.Npad / 4; i += 64) {
            const uint32_t v = go[i];
            ((uint32_t *)occ)[i] = v;
            ((uint32_t *)best)[i] = P.init_best ? v : gb[i];
        }
    }
    // the features of the occupancy, exactly (no drift carries across launches)
    for (int k = lane; k < F; k += 64) {
        f[k] = P.ext[(size_t)r * F + k] / P.size;
        df[k] = 0.0;
    }
    dist_wave_sync();
    auto objective = [&](double &L, double &sum) {
        unsigned long long m[4] = {0, 0, 0, 0};
        double e = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < P.nchunk) {
                const int k = c * 64 + lane;
                bool ok = false;
                if (k < F && k > 0) {
                    const double d = fabs(f[k] - tgt[k]);
                    e += wt[k] * d;
                    ok = d <= P.tol;
                }
                m[c] = __builtin_amdgcn_ballot_w64(ok);
            }
        }
        sum = wave_sum_all(e);
        L = P.w_match != 0.0 ? dist_match_diameter(P, m) : 0.0;
    };
    double L, sum;
    objective(L, sum);
    double H = -P.w_match * L + sum;
    double bestH = P.init_best ? H : P.best_H[r];
    unsigned long long step = P.nsteps[r];
    unsigned long long bstep = P.init_best ? step : P.best_step[r];
    unsigned long long nacc = P.nacc[r];
    int last = P.last_acc[r];
    const double beta = P.beta[r];
    const uint64_t seed = P.seeds[r];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    // the site word of a step is word 1 of the previous step's block 0 (oracle: orc_mc_run)
    uint32_t w_site = philox4x32_10((uint32_t)(step - 1), (uint32_t)((step - 1) >> 32), 0, 0, k0, k1).w[1];
    for (long long i = 0; i < P.steps; ++i, ++step) {
        constexpr int MF = REPLAY ? SMOLMC_MAX_STEP_FLIPS : 2; // (flips of a step: a native step makes at most two)
        int nf = 0, fs[MF], fc[MF];
        double u;
        if (REPLAY) {
            const int *rec = P.rp_steps + ((size_t)r * P.steps + i) * SMOLMC_STEP_ROW;
            for (; nf < MF && rec[2 * nf] >= 0; ++nf) {
                fs[nf] = uni(rec[2 * nf]);
                fc[nf] = uni(rec[2 * nf + 1]);
            }
            u = P.rp_u[(size_t)r * P.steps + i];
        } else {
            const philox_out w0 = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), 0, 0, k0, k1);
            u = philox_u53(w0.w[2], w0.w[3]);
            int sl = 0;
            if (P.nsub > 1) { // MCUsher.get_random_sublattice (mcusher.py:146-148)
                const double x = (double)w0.w[0] * (1.0 / 4294967296.0);
                sl = P.nsub - 1;
                for (int q = P.nsub - 2; q >= 0; --q)
                    if (x < P.sub_cum[q]) sl = q;
            }
            const int *sites = P.sub_sites + P.sub_ptr[sl];
            const uint32_t nact = (uint32_t)(P.sub_ptr[sl + 1] - P.sub_ptr[sl]);
            const int s1 = uni(sites[__umulhi(w_site, nact)]);
            const int cur = uni(occ[s1]);
            if (P.step_type == SMOLMC_STEP_FLIP) { // Flip.propose_step (mcusher.py:154-170)
                const int *codes = P.sub_codes + P.sub_code_ptr[sl];
                const uint32_t nc = (uint32_t)(P.sub_code_ptr[sl + 1] - P.sub_code_ptr[sl]);
                const uint32_t kk = __umulhi(philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), 1, 0, k0, k1).w[0], nc - 1);
                int code = -1;
                for (uint32_t c = 0, seen = 0; c < nc; ++c) {
                    if (codes[c] == cur) continue;
                    if (seen == kk) { code = codes[c]; break; }
                    seen++;
                }
                fs[0] = s1; fc[0] = uni(code); nf = 1;
            } else { // Swap.propose_step (mcusher.py:176-200): candidate t from W(step, blk(t))[word(t)]
                // The oracle's rule, with one cap: after 4096 candidates without a differing species the step is
                // empty (mcusher.py:197-199) where the oracle would keep drawing.  With at least one site of each
                // species in the sublattice the chance of reaching the cap is (1 - 1/N)^4096 (e^-16 at N = 256).
                for (int t0 = 0; t0 < 64 * 64; t0 += 64) {
                    const int t = t0 + lane;
                    const uint32_t blk = t < 12 ? 1 + t % 3 : 4 + (t - 12) / 4;
                    const int wd = t < 12 ? t / 3 : (t - 12) % 4;
                    const philox_out wc = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), blk, 0, k0, k1);
                    const uint32_t word = wd == 0 ? wc.w[0] : wd == 1 ? wc.w[1] : wd == 2 ? wc.w[2] : wc.w[3];
                    const int s2 = sites[__umulhi(word, nact)];
                    const int sp2 = occ[s2];
                    const unsigned long long hit = __builtin_amdgcn_ballot_w64(sp2 != cur);
                    if (hit) {
                        const int l = __builtin_ctzll(hit);
                        const int s2u = __builtin_amdgcn_readlane(s2, l), sp2u = __builtin_amdgcn_readlane(sp2, l);
                        fs[0] = s1; fc[0] = sp2u; fs[1] = s2u; fc[1] = cur; nf = 2;
                        break;
                    }
                }
                // (a sublattice of one species: no swap exists; the empty step of mcusher.py:197-199)
            }
            w_site = w0.w[1];
        }
        // price the flips one after the other, each applied in LDS for the next
        int old[MF];
#pragma unroll
        for (int q = 0; q < MF; ++q) {
            if (q >= nf) break;
            old[q] = uni(occ[fs[q]]);
            dist_flip_pass<NSLOT>(P, tens, occ, df, part, lane, fs[q], fc[q]);
            dist_wave_sync();
            if (lane == 0) occ[fs[q]] = (uint8_t)fc[q];
            dist_wave_sync();
        }
        // objective change: touched features W_k (|f + df - t| - |f - t|), untouched ones exactly 0
        unsigned long long m[4] = {0, 0, 0, 0};
        double e = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < P.nchunk) {
                const int k = c * 64 + lane;
                bool ok = false;
                if (k < F && k > 0) {
                    const double fo = f[k], fn = fo + df[k];
                    const double dn = fabs(fn - tgt[k]);
                    e += wt[k] * (dn - fabs(fo - tgt[k]));
                    ok = dn <= P.tol;
                }
                m[c] = __builtin_amdgcn_ballot_w64(ok);
            }
        }
        const double Ln = P.w_match != 0.0 ? dist_match_diameter(P, m) : 0.0;
        const double dE = -P.w_match * (Ln - L) + wave_sum_all(e);
        const double expo = -beta * dE; // metropolis.py:31-49
        // (replay: a NaN uniform is a step the reference accepted without drawing, metropolis.py:46-48 -- taken as
        // accepted; the incremental dE of the kernel may differ from the reference's recomputed one by rounding,
        // and an exact 0 there must not become a rejection here)
        const bool acc = (REPLAY && u != u) ? true : (expo >= 0 ? true : (expo > log(u)));
        if (acc) {
            for (int k = lane; k < F; k += 64) f[k] += df[k];
            H += dE;
            L = Ln;
            ++nacc;
            if (H < bestH) { // strictly lower replaces
                for (int b = lane; b < P.Npad / 4; b += 64) ((uint32_t *)best)[b] = ((const uint32_t *)occ)[b];
                bestH = H;
                bstep = step + 1;
            }
        } else {
            if (lane == 0)
#pragma unroll
                for (int q = MF - 1; q >= 0; --q)
                    if (q < nf) occ[fs[q]] = (uint8_t)old[q];
        }
        for (int k = lane; k < F; k += 64) df[k] = 0.0;
        last = acc ? 1 : 0;
        dist_wave_sync();
        if (REPLAY && lane == 0) {
            P.rp_acc[(size_t)r * P.steps + i] = (uint8_t)last;
            P.rp_H[(size_t)r * P.steps + i] = H;
        }
        if (P.smp.every && (i + 1) % P.smp.every == 0) { // Sampler.sample rows (sampler.py:195-210)
            const size_t row = (size_t)((i + 1) / P.smp.every - 1) * P.R + r;
            for (int k = lane; k < F; k += 64) P.smp.feat[row * F + k] = k ? fabs(f[k] - tgt[k]) : L;
            if (lane == 0) {
                P.smp.H[row] = H;
                P.smp.acc[row] = (uint8_t)last;
            }
            if (P.smp.occ)
                for (int b = lane; b < P.Npad / 4; b += 64)
                    ((uint32_t *)(P.smp.occ + row * P.Npad))[b] = ((const uint32_t *)occ)[b];
        }
    }
    // launch end: state, features (the reference's intensive distance vector), counters, best record
    for (int b = lane; b < P.Npad / 4; b += 64) {
        ((uint32_t *)(P.occ + (size_t)r * P.Npad))[b] = ((const uint32_t *)occ)[b];
        ((uint32_t *)(P.best_occ + (size_t)r * P.Npad))[b] = ((const uint32_t *)best)[b];
    }
    for (int k = lane; k < F; k += 64) P.features[(size_t)r * F + k] = k ? fabs(f[k] - tgt[k]) : L;
    if (lane == 0) {
        P.enthalpy[r] = H;
        P.nsteps[r] = step;
        P.nacc[r] = nacc;
        P.last_acc[r] = (uint8_t)last;
        P.best_H[r] = bestH;
        P.best_step[r] = bstep;
    }
}

template <int NSLOT, bool REPLAY> int launch_dist_nslot(smolmc_handle *h, const DistParams &P) {
    const size_t lds = (size_t)P.lds_shared + (size_t)SMOLMC_DIST_WPB * P.lds_per_wave;
    auto kern = mc_dist_kernel<NSLOT, REPLAY>; // (smolmc_create_distance holds lds to 64 KB)
    const unsigned grid = (unsigned)((P.R + SMOLMC_DIST_WPB - 1) / SMOLMC_DIST_WPB);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * SMOLMC_DIST_WPB), lds, h->stream, P);
    HIPCHK(hipGetLastError());
    return 0;
}

// instantiations (dist_n*.hip, dist_replay_n*.hip): NSLOT = 64-lane rounds of a flip's chunk pass (chunks per site / 64)
int smolmc_launch_dist_1(smolmc_handle *h, const DistParams &P);
int smolmc_launch_dist_2(smolmc_handle *h, const DistParams &P);
int smolmc_launch_dist_4(smolmc_handle *h, const DistParams &P);
int smolmc_launch_dist_replay_1(smolmc_handle *h, const DistParams &P);
int smolmc_launch_dist_replay_2(smolmc_handle *h, const DistParams &P);
int smolmc_launch_dist_replay_4(smolmc_handle *h, const DistParams &P);
