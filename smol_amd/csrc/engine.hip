// engine.hip -- C-ABI (include/smolmc.h), host-side table preparation and the evaluation kernels.
#include <array>
#include <map>
#include <string>
#include <thread>

#include "smolmc_common.h"

thread_local std::string smolmc_g_err;

// ----------------------------------------------------------------------------
// reference-layout evaluation kernels (parity API + initial trace)
// ----------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < nw; ++i) s += sh[i];
    return s;
}

// Ensemble.compute_feature_vector for one occupancy per block
// (evaluator.pyx:121-209 x size; processor/ewald.py:128-145; ensemble.py:343-349)
// ce_only: the cluster features alone (lazy cluster features: the scalar features are carried by the kernels)
__global__ void __launch_bounds__(256) eval_full_kernel(const RefTables T, const uint8_t *occ_all,
                                                        double *out_all, const int ce_only, const int nocc, const int M) {
    __shared__ double sh[8];
    extern __shared__ __attribute__((aligned(16))) unsigned char eval_smem[];
    // Round 5 (this kernel is on the sampling path of handles with lazy cluster features): a block evaluates M <= 4
    // occupancies at once -- the index rows of an orbit, 15 MB for config 2, are read once for the M of them -- from
    // copies in LDS (M x Npad bytes of dynamic LDS; M = 0: one occupancy, read through the caches).
    const int m_eff = M > 0 ? M : 1;
    const int first = blockIdx.x * m_eff;
    const uint8_t *gocc = occ_all + (size_t)first * T.Npad;
    if (M > 0) {
        for (int m = 0; m < M; ++m) {
            const int q = first + m < nocc ? m : 0; // (blocks past the end repeat their first occupancy)
            const uint4 *src = (const uint4 *)(gocc + (size_t)q * T.Npad);
            uint4 *dst = (uint4 *)(eval_smem + (size_t)m * T.Npad);
            for (int i = threadIdx.x; i < T.Npad / 16; i += blockDim.x) dst[i] = src[i];
        }
        __syncthreads();
    }
    const uint8_t *occ = M > 0 ? (const uint8_t *)eval_smem : gocc;
    const int ostr = M > 0 ? T.Npad : 0; // occupancy m at occ + m * ostr
    if (threadIdx.x < m_eff && first + (int)threadIdx.x < nocc)
        out_all[(size_t)(first + threadIdx.x) * T.F] = (T.corr_mode ? 1.0 : T.offset) * (double)T.P;
    for (int n = 0; n < T.n_orb; ++n) {
        const int I = T.orb_nsites[n], K = T.corr_mode ? T.orb_nfunc[n] : 1;
        const int Nt = T.orb_tensor_len[n];
        const int *st = T.tensor_indices + T.orb_stride_off[n];
        const int *ind = T.full_idx + T.full_off[n];
        const long long J = (T.full_off[n + 1] - T.full_off[n]) / I;
        const double *t0 = T.corr_mode ? T.corr_tensors + T.orb_ctensor_off[n] : T.interaction_tensors + T.orb_itensor_off[n];
        // the tensor index of a cluster once for up to four functions (the sums of a function are those of the
        // function-by-function loop: same clusters per thread, same order)
        for (int k0 = 0; k0 < K; k0 += 4) {
            double p[4][4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int k = 0; k < 4; ++k) p[m][k] = 0.0;
            const int kn = K - k0 < 4 ? K - k0 : 4;
            for (long long j = threadIdx.x; j < J; j += blockDim.x) {
                int index[4] = {0, 0, 0, 0};
                for (int i = 0; i < I; ++i) {
                    const int x = ind[j * I + i], sti = st[i];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (m < m_eff) index[m] += sti * (int)occ[(size_t)m * ostr + x];
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (m < m_eff)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < kn) p[m][k] += t0[(size_t)(k0 + k) * Nt + index[m]];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < m_eff)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < kn) {
                            const double v = block_sum(p[m][k], sh);
                            if (threadIdx.x == 0 && first + m < nocc) {
                                const int o = T.corr_mode ? T.orb_bit_id[n] + k0 + k : T.orb_id[n];
                                out_all[(size_t)(first + m) * T.F + o] = v / (double)J * (double)T.P;
                            }
                        }
        }
    }
    if (ce_only) return;
    // (the scalar features below: launches with one occupancy per block)
    double *out = out_all + (size_t)first * T.F;
    int f = T.Fce;
    if (T.has_ewald) {
        double s = 0;
        for (int a = 0; a < T.N; ++a) {
            const int ia = T.ew_inds[(size_t)a * T.ew_W + occ[a]];
            if (ia == -1) continue;
            const double *row = T.ew_M_rowmajor + (size_t)ia * T.ew_M;
            for (int b = threadIdx.x; b < T.N; b += blockDim.x) {
                const int ib = T.ew_inds[(size_t)b * T.ew_W + occ[b]];
                if (ib != -1) s += row[ib];
            }
        }
        s = block_sum(s, sh);
        if (threadIdx.x == 0) out[f] = s;
        f++;
    }
    if (T.has_mu) {
        double s = 0;
        for (int a = threadIdx.x; a < T.N; a += blockDim.x) s += T.mu[(size_t)a * T.mu_W + occ[a]];
        s = block_sum(s, sh);
        if (threadIdx.x == 0) out[f] = s;
    }
}

// Ensemble.compute_feature_vector_change for one step (<= SMOLMC_MAX_STEP_FLIPS sequential flips) per
// wave, reference table layout and arithmetic chain p / ratio / J, x size
// (evaluator.pyx:244-262, :302-315; expansion.py:217-231).  Flip f sees the flips before it: a site's
// species is the code of the LAST earlier flip there, else the occupancy's.
__global__ void __launch_bounds__(64) eval_delta_kernel(const RefTables T, const uint8_t *occ,
                                                        const int *flips, double *out_all) {
    const int lane = threadIdx.x;
    const int *fl = flips + (size_t)blockIdx.x * SMOLMC_STEP_ROW;
    double *out = out_all + (size_t)blockIdx.x * T.F;
    for (int i = lane; i < T.F; i += 64) out[i] = 0.0;
    __syncthreads();
    int nfl = 0;
    while (nfl < SMOLMC_MAX_STEP_FLIPS && fl[2 * nfl] >= 0) nfl++;
    auto seen = [&](const int x, const int f) -> int { // species of site x as flip f sees it
        int v = occ[x];
        for (int g = 0; g < f; ++g)
            if (fl[2 * g] == x) v = fl[2 * g + 1];
        return v;
    };
    double dew = 0, dmu = 0;
    for (int f = 0; f < nfl; ++f) {
        const int s = fl[2 * f], newc = fl[2 * f + 1];
        for (long long rr = T.site_ptr[s]; rr < T.site_ptr[s + 1]; ++rr) {
            const int n = T.loc_orbit[rr];
            const int I = T.orb_nsites[n], K = T.corr_mode ? T.orb_nfunc[n] : 1, Nt = T.orb_tensor_len[n];
            const int *st = T.tensor_indices + T.orb_stride_off[n];
            const int *ind = T.loc_idx + T.loc_off[rr];
            const int J = T.loc_nrows[rr];
            for (int k = 0; k < K; ++k) {
                const double *t = T.corr_mode ? T.corr_tensors + T.orb_ctensor_off[n] + (size_t)k * Nt
                                              : T.interaction_tensors + T.orb_itensor_off[n];
                double p = 0;
                for (int j = lane; j < J; j += 64) {
                    int ind_i = 0, ind_f = 0;
                    for (int i = 0; i < I; ++i) {
                        const int x = ind[j * I + i];
                        const int v = seen(x, f);
                        const int vf = (x == s) ? newc : v;
                        ind_i += st[i] * v;
                        ind_f += st[i] * vf;
                    }
                    p += t[ind_f] - t[ind_i];
                }
                p = wave_sum(p);
                if (lane == 0) {
                    const int o = T.corr_mode ? T.orb_bit_id[n] + k : T.orb_id[n];
                    out[o] += p / T.loc_ratio[rr] / (double)J;
                }
            }
        }
        if (T.has_ewald) {
            // ewald.pyx:38-58
            const int oldc = seen(s, f);
            const int W = T.ew_W;
            const int add = T.ew_inds[(size_t)s * W + newc], sub = T.ew_inds[(size_t)s * W + oldc];
            double o = 0;
            for (int k = lane; k < T.N; k += 64) {
                const int v = seen(k, f);
                const int vf = (k == s) ? newc : v;
                const int i = T.ew_inds[(size_t)k * W + vf], j = T.ew_inds[(size_t)k * W + v];
                if (i != -1 && add != -1)
                    o += (i != add ? 2.0 : 1.0) * T.ew_Mt[(size_t)add * T.ew_M + i];
                if (j != -1 && sub != -1)
                    o -= (j != sub ? 2.0 : 1.0) * T.ew_Mt[(size_t)sub * T.ew_M + j];
            }
            dew += wave_sum(o);
        }
        if (T.has_mu) // against the ORIGINAL occupancy (ensemble.py:368-374)
            dmu += T.mu[(size_t)s * T.mu_W + newc] - T.mu[(size_t)s * T.mu_W + occ[s]];
    }
    __syncthreads();
    for (int i = lane; i < T.Fce; i += 64) out[i] *= (double)T.P;
    if (lane == 0) {
        int f = T.Fce;
        if (T.has_ewald) out[f++] = dew;
        if (T.has_mu) out[f++] = dmu;
    }
}

__global__ void pack_occ_kernel(const int *occ32, uint8_t *occ8, int N, int Npad, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t rr = i / Npad;
    const int s = (int)(i % Npad);
    occ8[i] = s < N ? (uint8_t)occ32[rr * N + s] : 0;
}
__global__ void unpack_occ_kernel(const uint8_t *occ8, int *occ32, int N, int Npad, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t rr = i / N;
    const int s = (int)(i % N);
    occ32[i] = (int)occ8[rr * Npad + s];
}
// Ewald potential field of every walker from scratch (set_state): one block per walker, the
// charges q(k, occ_k) of the changeable sites staged in LDS, each wave sums rows
// phi[j] = sum_{k != j} q_k G[site_j][k].
__global__ void __launch_bounds__(256) ewald_field_init_kernel(const LeanParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
    double *q = (double *)fsm;
    const int r = blockIdx.x, na = P.ew_nact, W = P.ew_W;
    const uint8_t *occ = P.occ + (size_t)r * P.Npad;
    for (int k = threadIdx.x; k < na; k += blockDim.x) {
        const int site = P.sbase + k;
        q[k] = P.ew_qs[(size_t)site * W + occ[site]];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = wave; j < na; j += nw) {
        const double *g = P.ew_G + (size_t)(P.sbase + j) * na;
        double acc = 0.0;
        for (int k = lane; k < na; k += 64) acc = fma(k != j ? q[k] : 0.0, g[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) P.ew_phi[(size_t)r * na + j] = acc + P.ew_frozen[P.sbase + j];
    }
}

// Wang-Landau per-bin feature statistics: running means <-> running sums (sum = mean * occurrences)
__global__ void wl_meanf_convert_kernel(double *meanf, const long long *occur, size_t cells, int F, int to_mean) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * (size_t)F) return;
    const long long n = occur[i / F];
    if (n > 0) meanf[i] = to_mean ? meanf[i] / (double)n : meanf[i] * (double)n;
}

__global__ void dot_features_kernel(const double *features, const double *natural, double *enthalpy,
                                    int R, int F) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double s = 0;
    for (int i = 0; i < F; ++i) s += natural[i] * features[(size_t)r * F + i];
    enthalpy[r] = s;
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
static int num_ce_features(const smolmc_tables *t) {
    return t->feature_mode == SMOLMC_FEATURES_CORRELATIONS ? t->num_corr : t->num_orbits;
}

static bool is_wl(const smolmc_handle *h) { return h->cfg.kernel_type == SMOLMC_KERNEL_WANGLANDAU; }
static bool is_table(const smolmc_handle *h) { return h->cfg.step_type == SMOLMC_STEP_TABLE_FLIP; }
// what one cluster of local record r weighs in an extensive feature: size / (cluster ratio * rows of the record)
static double slot_scale(const smolmc_tables *t, int64_t r) { return (double)t->size / t->loc_ratio[r] / (double)t->loc_nrows[r]; }
// Species of member a of orbit o's clusters as the cluster tensors see them: the strides are those of a row-major
// tensor over the members' site spaces (orbit.py:268-275; validate_tables checks that they are)
static int member_species(const smolmc_tables *t, int o, int a) {
    const int32_t *st = t->tensor_indices + t->orb_stride_off[o];
    return (a == 0 ? t->orb_tensor_len[o] : st[a - 1]) / st[a];
}
// site s carries exactly one Ewald species, at code 0 (outside the active sublattices: a charge that never changes)
static bool single_ewald_species(const smolmc_tables *t, int s) {
    const int32_t *inds = t->ewald_inds + (size_t)s * t->ewald_width;
    int nvalid = 0;
    for (int c = 0; c < t->ewald_width; ++c) nvalid += inds[c] >= 0;
    return nvalid == 1 && inds[0] >= 0;
}

// ---- the MC-optimised tables: site classes, mc_kernel's slot tables (h->kp), the lean families' (h->lp) ---------
// build_mc_tables, below, is the list of stages.  Every stage but general_tables and commit_lean_tables is host
// arithmetic on its arguments: no device call, no write to the handle.
// Models mc_kernel / the lean kernels cannot take (more than 1024 clusters per site, more than 255 site
// classes, tensor strides beyond 16 bits, an occupancy that does not fit LDS) are not refused: the
// handle notes why (general_reason) and every launch takes the universal kernel (mc_univ.h).
static int no_general(smolmc_handle *h, const char *why) {
    h->general_ok = false;
    h->general_reason = why;
    return 0;
}

// What has to hold before any table is built, in the order in which it is reported
struct GeneralLimits {
    const char *universal = nullptr; // mc_kernel cannot run the model: why
    const char *error = nullptr;     // no kernel can
    // some local row holds a site twice (a supercell shorter than a cluster); some local row does not hold its own
    // site at all (searched on unaliased cells only)
    bool aliased = false, unnamed = false;
    int maxI = 1;                    // sites of the largest cluster
};
static GeneralLimits general_limits(const smolmc_tables *t, int Npad) {
    GeneralLimits g;
    auto universal = [&](const char *why) { g.universal = why; return g; };
    if ((size_t)Npad + 4096 > 160 * 1024) return universal("occupancy does not fit LDS");
    if (smolmc_env(ENV_FORCE_UNIVERSAL)) return universal("SMOLMC_FORCE_UNIVERSAL");
    for (int s = 0; s < t->num_sites && !g.aliased; ++s)
        for (int64_t r = t->site_ptr[s]; r < t->site_ptr[s + 1] && !g.aliased; ++r) {
            const int I = t->orb_nsites[t->loc_orbit[r]];
            const int32_t *row = t->loc_idx + t->loc_off[r];
            for (int j = 0; j < t->loc_nrows[r] && !g.aliased; ++j, row += I) {
                bool named = false;
                for (int a = 0; a < I; ++a) {
                    named = named || row[a] == s;
                    for (int b = a + 1; b < I; ++b) g.aliased = g.aliased || row[a] == row[b];
                }
                g.unnamed = g.unnamed || !named;
            }
        }
    for (int o = 0; o < t->n_orb; ++o) g.maxI = std::max(g.maxI, (int)t->orb_nsites[o]);
    if (g.maxI > SMOLMC_MAX_CLUSTER_SITES) { g.error = "cluster larger than SMOLMC_MAX_CLUSTER_SITES"; return g; }
    for (int o = 0; o < t->n_orb; ++o)
        for (int i = 0; i < t->orb_nsites[o]; ++i)
            if (t->tensor_indices[t->orb_stride_off[o] + i] > 65535) return universal("tensor stride exceeds 16 bits");
    return g;
}

// One cluster of a site as a kernel evaluates it: a row of one of the site's local records.  The positions of the row
// that count as the site ITSELF (selfmask) are folded into the slot's table; the other members are gathered.
struct Slot {
    int orbit;
    int64_t rec;        // local record
    const int32_t *row; // the member sites (orb_nsites[orbit] of them)
    uint32_t selfmask;
    int pfirst, nother; // first self position (0: none), members gathered
};
// How a table reads a row.  ROWS_OWN: the self positions are where the row holds the site -- the lean families
// everywhere, and mc_kernel too wherever every row holds its site exactly once: there both use ONE list.  mc_kernel
// differs in two cases.  On an ALIASED cell (some row holds a site twice) it keeps generic rows: no self position, all
// I members gathered, rows in the order of the record (ROWS_GENERIC).  And a row that does not hold its site at all --
// validate_tables does not refuse one -- it reads as if member 0 were the site (ROWS_MEMBER0: p = 0, member 0 is not
// gathered), where the lean tables gather all I members and get a delta table of zeros (selfmask 0).
enum RowView { ROWS_OWN, ROWS_MEMBER0, ROWS_GENERIC };
// The slots of site s, in the order both tables use: inside a record by first self position, then by mask -- the
// order of the reference's rows (equivalent cluster major) at equal positions, which is the same on every site of a
// translation class -- and the records' slots with most gathered members first, so that iterations are homogeneous.
static std::vector<Slot> site_slots(const smolmc_tables *t, int s, RowView view) {
    std::vector<Slot> sl;
    for (int64_t r = t->site_ptr[s]; r < t->site_ptr[s + 1]; ++r) {
        const int o = t->loc_orbit[r], I = t->orb_nsites[o];
        const size_t first = sl.size();
        const int32_t *row = t->loc_idx + t->loc_off[r];
        for (int j = 0; j < t->loc_nrows[r]; ++j, row += I) {
            uint32_t mask = 0;
            for (int a = 0; a < I && view != ROWS_GENERIC; ++a)
                if (row[a] == s) mask |= 1u << a;
            if (view == ROWS_MEMBER0 && !mask) mask = 1u;
            sl.push_back(Slot{o, r, row, mask, mask ? __builtin_ctz(mask) : 0, I - __builtin_popcount(mask)});
        }
        std::stable_sort(sl.begin() + first, sl.end(), [](const Slot &a, const Slot &b) {
            return a.pfirst != b.pfirst ? a.pfirst < b.pfirst : a.selfmask < b.selfmask;
        });
    }
    std::stable_sort(sl.begin(), sl.end(), [](const Slot &a, const Slot &b) { return a.nother > b.nother; });
    return sl;
}

// Sites whose records agree (orbit, rows, ratio, rows per self position) form a class: they share slot descriptors.
struct SiteClasses {
    const char *universal = nullptr;           // mc_kernel cannot run the model: why
    // per site: as mc_kernel reads the rows, and as the lean families do where that differs (else empty)
    std::vector<std::vector<Slot>> slots, own_slots;
    std::vector<int> site_class;               // 255: a site without clusters
    std::vector<int> class_rep;                // representative site per class
    int niter_max = 0, lean_need_mm = 1;       // groups of 64 slots of the largest class; most gathered members of a lean slot
    bool lean_alike = true;                    // aliased cells: every site lists its lean slots as its class's representative does
    const std::vector<Slot> &lean_slots(int s) const { return own_slots.empty() ? slots[s] : own_slots[s]; }
};
static SiteClasses site_classes(const smolmc_tables *t, const GeneralLimits &lim) {
    const int N = t->num_sites;
    SiteClasses sc;
    sc.slots.resize(N);
    sc.site_class.assign(N, 255);
    std::map<std::vector<long long>, int> class_of;
    for (int s = 0; s < N; ++s) {
        const int64_t r0 = t->site_ptr[s], nrec = t->site_ptr[s + 1] - r0;
        if (!nrec) continue;
        sc.slots[s] = site_slots(t, s, lim.aliased ? ROWS_GENERIC : lim.unnamed ? ROWS_MEMBER0 : ROWS_OWN);
        // signature: per record its orbit, rows and ratio, then the number of slots at each first self position
        constexpr int W = 3 + SMOLMC_MAX_CLUSTER_SITES;
        std::vector<long long> sig((size_t)nrec * W, 0);
        for (int64_t r = r0; r < r0 + nrec; ++r) {
            long long *g = &sig[(size_t)(r - r0) * W];
            g[0] = t->loc_orbit[r];
            g[1] = t->loc_nrows[r];
            memcpy(&g[2], &t->loc_ratio[r], 8);
        }
        for (const Slot &k : sc.slots[s]) sig[(size_t)(k.rec - r0) * W + 3 + k.pfirst]++;
        auto itc = class_of.find(sig);
        if (itc == class_of.end()) {
            if (sc.class_rep.size() >= 255) { sc.universal = "more than 255 site classes"; return sc; }
            itc = class_of.emplace(std::move(sig), (int)sc.class_rep.size()).first;
            sc.class_rep.push_back(s);
        }
        sc.site_class[s] = itc->second;
    }
    size_t Cmax = 1;
    for (int s : sc.class_rep) Cmax = std::max(Cmax, sc.slots[s].size());
    sc.niter_max = (int)((Cmax + 63) / 64);
    if (sc.niter_max > 16) { sc.universal = "more than 1024 clusters per site"; return sc; }
    if (lim.aliased || lim.unnamed) {
        sc.own_slots.resize(N);
        for (int s = 0; s < N; ++s) sc.own_slots[s] = site_slots(t, s, ROWS_OWN);
    }
    for (int s = 0; s < N; ++s)
        for (const Slot &k : sc.lean_slots(s)) sc.lean_need_mm = std::max(sc.lean_need_mm, k.nother);
    // An aliased cell's classes were made from the generic rows: the lean slots are verified site by site
    for (int s = 0; s < N && lim.aliased && sc.lean_alike; ++s) {
        if (sc.site_class[s] == 255) continue;
        const std::vector<Slot> &a = sc.lean_slots(s), &b = sc.lean_slots(sc.class_rep[sc.site_class[s]]);
        sc.lean_alike = a.size() == b.size();
        for (size_t q = 0; q < a.size() && sc.lean_alike; ++q)
            sc.lean_alike = a[q].orbit == b[q].orbit && a[q].selfmask == b[q].selfmask && a[q].selfmask != 0;
    }
    return sc;
}

// mc_kernel's tables: decision tensors per class (xt), feature tensors (ft), slot descriptors, member index rows
static int general_tables(smolmc_handle *h, const smolmc_tables *t, const GeneralLimits &lim, const SiteClasses &sc) {
    const int N = t->num_sites;
    const bool corr = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS, aliased = lim.aliased;
    const int nclasses = std::max<int>(1, (int)sc.class_rep.size()), niter_max = sc.niter_max;
    const int nslot = niter_max <= 2 ? 2 : (niter_max <= 4 ? 4 : (niter_max <= 8 ? 8 : 16));
    // slot columns per class: the two-group kernels evaluate BOTH groups without a condition
    // (mc_general.h), so the padding goes up to their full width (padded slots add 0.0)
    const int Cpad = 64 * (nslot <= 2 ? nslot : niter_max);
    const int need_mm = aliased ? lim.maxI : std::max(1, lim.maxI - 1);
    const int MM = aliased ? (need_mm <= 3 ? 3 : 6) : (need_mm <= 2 ? 2 : (need_mm <= 3 ? 3 : 5));
    const bool idx16 = (!aliased) && N <= 65535;

    std::vector<double> ft;
    std::vector<int> foff(t->n_orb);
    for (int o = 0; o < t->n_orb; ++o) {
        foff[o] = (int)ft.size();
        const double *src = corr ? t->corr_tensors + t->orb_ctensor_off[o] : t->interaction_tensors + t->orb_itensor_off[o];
        ft.insert(ft.end(), src, src + (size_t)(corr ? t->orb_nfunc[o] : 1) * t->orb_tensor_len[o]);
    }
    std::vector<double> xt;
    std::vector<uint4> descA((size_t)nclasses * Cpad, make_uint4(0, 0, 0, 0));
    std::vector<uint4> descB((size_t)nclasses * Cpad, make_uint4(0, 0, 0, 0));
    std::vector<double> slot_fs((size_t)nclasses * Cpad, 0.0);
    std::vector<int> cls_niter(nclasses, 0);
    xt.push_back(0.0); // padded slots read xt[0] - xt[0]
    for (int c = 0; c < (int)sc.class_rep.size(); ++c) {
        const std::vector<Slot> &sl = sc.slots[sc.class_rep[c]];
        cls_niter[c] = (int)((sl.size() + 63) / 64);
        std::map<int64_t, int> xoff_of_rec;
        for (size_t q = 0; q < sl.size(); ++q) {
            const Slot &k = sl[q];
            const int o = k.orbit, I = t->orb_nsites[o], Nt = t->orb_tensor_len[o];
            const int32_t *st = t->tensor_indices + t->orb_stride_off[o];
            const double scale = slot_scale(t, k.rec);
            if (!xoff_of_rec.count(k.rec)) {
                xoff_of_rec[k.rec] = (int)xt.size();
                for (int i = 0; i < Nt; ++i) {
                    double v = 0;
                    if (corr) { // energy tensor: sum_k coef[bit_id+k] * ct[k][i], times scale
                        const double *ct = t->corr_tensors + t->orb_ctensor_off[o];
                        for (int kk = 0; kk < t->orb_nfunc[o]; ++kk) v += t->ce_coefs[t->orb_bit_id[o] + kk] * ct[(size_t)kk * Nt + i];
                        v *= scale;
                    } else {
                        v = t->ce_coefs[t->orb_id[o]] * scale * t->interaction_tensors[t->orb_itensor_off[o] + i];
                    }
                    xt.push_back(v);
                }
            }
            // strides: the self position first (generic rows have none), then the gathered members
            uint16_t sv[6] = {0, 0, 0, 0, 0, 0};
            int m = 0;
            if (k.selfmask) sv[m++] = (uint16_t)st[k.pfirst];
            for (int a = 0; a < I; ++a)
                if (!((k.selfmask >> a) & 1u)) sv[m++] = (uint16_t)st[a];
            descA[(size_t)c * Cpad + q] = make_uint4((uint32_t)xoff_of_rec[k.rec], sv[0] | ((uint32_t)sv[1] << 16),
                                                     sv[2] | ((uint32_t)sv[3] << 16), sv[4] | ((uint32_t)sv[5] << 16));
            const uint32_t feat = corr ? (uint32_t)t->orb_bit_id[o] : (uint32_t)t->orb_id[o];
            const uint32_t K = corr ? (uint32_t)t->orb_nfunc[o] : 1u;
            descB[(size_t)c * Cpad + q] = make_uint4((uint32_t)foff[o], (uint32_t)Nt, feat | (K << 16), 0);
            slot_fs[(size_t)c * Cpad + q] = scale;
        }
    }
    if (xt.size() > 0xffffffffull) return no_general(h, "decision tensors too large");

    // member index rows [site][m][Cpad]; padded entries point at the site itself
    const size_t idx_n = (size_t)N * MM * Cpad;
    std::vector<int32_t> idx32(idx_n);
    for (int s = 0; s < N; ++s) {
        for (int m = 0; m < MM; ++m)
            for (int c = 0; c < Cpad; ++c) idx32[((size_t)s * MM + m) * Cpad + c] = s;
        const std::vector<Slot> &sl = sc.slots[s];
        for (size_t q = 0; q < sl.size(); ++q) {
            int m = 0;
            for (int a = 0; a < t->orb_nsites[sl[q].orbit]; ++a)
                if (!((sl[q].selfmask >> a) & 1u)) idx32[((size_t)s * MM + m++) * Cpad + q] = sl[q].row[a];
        }
    }
    KParams &kp = h->kp;
    if (idx16) {
        const std::vector<uint16_t> idx16v(idx32.begin(), idx32.end());
        const uint16_t *d;
        TRY(dev_upload(h, idx16v.data(), idx_n, &d));
        kp.idx = d;
    } else {
        const int32_t *d;
        TRY(dev_upload(h, idx32.data(), idx_n, &d));
        kp.idx = d;
    }
    std::vector<uint8_t> sc8(sc.site_class.begin(), sc.site_class.end());
    TRY(dev_upload(h, sc8.data(), (size_t)N, &kp.site_class));
    TRY(dev_upload(h, descA.data(), descA.size(), &kp.descA));
    TRY(dev_upload(h, descB.data(), descB.size(), &kp.descB));
    TRY(dev_upload(h, slot_fs.data(), slot_fs.size(), &kp.slot_fs));
    TRY(dev_upload(h, cls_niter.data(), cls_niter.size(), &kp.cls_niter));
    TRY(dev_upload(h, xt.data(), xt.size(), &kp.xt));
    TRY(dev_upload(h, ft.data(), ft.size(), &kp.ft));
    kp.xt_len = (int)xt.size(); kp.ft_len = (int)ft.size(); kp.nclasses = nclasses; kp.Cpad = Cpad; kp.Mmax = MM;
    h->nslot = nslot; h->mm = MM; h->generic = aliased; h->idx16 = idx16;
    return 0;
}

// ---- lean tables (see mc_lean_kernel) ------------------------------------------
// The lean families' view of a site's clusters: one slot per local row, the flipped site's OWN positions in the row
// folded into the slot's table (selfmask), the other members gathered.  On an ALIASED cell -- a supercell shorter than
// a cluster, so that a row holds a site twice; the reference keeps such rows (clusterspace.py:1353-1359) and its
// evaluator flips every position of the site at once (evaluator.pyx:258-259 read occu_f / occu_i through the whole
// row) -- the delta table of the slot does the same: D[(old, new)][b] = T[base(b) + (sum of the self strides) new] -
// T[... old] (round 6; until then such cells ran on mc_kernel's GENERIC rows).

// Which features the lean kernels carry, and why a model does not get the lean tables at all (reported by
// smolmc_kernel_info: the first condition that fails; empty: the tables are built)
struct LeanMode {
    bool corr_kf = false, corr_lazy = false, wide_lazy = false;
    const char *reason = "";
    bool lazy() const { return corr_lazy || wide_lazy; }
};
static LeanMode lean_mode(const smolmc_handle *h, const smolmc_tables *t, const GeneralLimits &lim, const SiteClasses &sc) {
    const bool corr = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS, wl = is_wl(h);
    const int N = t->num_sites, niter_max = sc.niter_max, nfeat = num_ce_features(t);
    const size_t ncls = sc.class_rep.size();
    LeanMode m;
    // one site class: mc_lean_kernel (NSLOT <= 4); up to four classes or up to 512 clusters per
    // site: mc_lean_multi_kernel (per-class slot records in LDS)
    // Correlation features (ClusterExpansionProcessor, evaluator.pyx:211-265): when every orbit
    // has a single correlation function (K = 1: every binary system) the correlation delta of a
    // cluster is one tensor difference exactly like the interaction delta (:267-317), so the lean
    // kernels serve it with delta tables made from the correlation tensor, the feature index
    // bit_id instead of the orbit id and the weight coefs[bit_id]: same code, other tables.
    bool corr_k1 = corr;
    for (int o = 0; o < t->n_orb; ++o) corr_k1 = corr_k1 && t->orb_nfunc[o] == 1;
    // Several correlation functions per orbit (K <= SMOLMC_LEAN_MAX_KF, one site class): the decision
    // table of a slot is made from the folded tensor E = sum_k coef_k ct_k and the K function
    // tables follow it (mc_lean_kernel KF).
    int kmax = 1;
    for (int o = 0; o < t->n_orb; ++o) kmax = std::max(kmax, (int)t->orb_nfunc[o]);
    // (the KF instantiations are plain Metropolis flip / swap kernels of the single-class layout)
    m.corr_kf = corr && !corr_k1 && kmax <= SMOLMC_LEAN_MAX_KF && ncls == 1 && !wl && !t->bias_type && !is_table(h) &&
                t->n_sublattices == 1 && niter_max <= 4 && nfeat <= 64 && !smolmc_env(ENV_LAZY_FEATURES_ONLY);
    // ... and the Wang-Landau kernel of the multi-class layout (KFW, round 5): any number of classes the layout takes
    if (corr && !corr_k1 && kmax <= SMOLMC_LEAN_MAX_KF && wl && !t->bias_type && !is_table(h) && nfeat <= 61) m.corr_kf = true;
    // LAZY cluster features (round 5): every other Metropolis kernel of the lean families takes a model with several
    // correlation functions per orbit as an interaction-mode model of the folded tensors E = sum_k coef_k ct_k --
    // the decision needs nothing else -- and carries no cluster features at all: they are evaluated from the
    // occupancy where somebody reads them (smolmc_get_state, sample rows; ensure_features / lazy_rows_kernel).
    // Any number of functions per orbit and of cluster features; Wang-Landau needs the features on every step and
    // stays on mc_kernel.
    m.corr_lazy = corr && !corr_k1 && !m.corr_kf && !wl && !smolmc_env(ENV_NO_LAZY_FEATURES);
    // ... and the same for models of more than 64 cluster features (the kernels' feature cells are one per lane)
    m.wide_lazy = !m.corr_lazy && !m.corr_kf && (!corr || corr_k1) && nfeat > 64 && !wl && !smolmc_env(ENV_NO_LAZY_FEATURES);
    const bool aliased_ok = !lim.aliased || (sc.lean_alike && !smolmc_env(ENV_NO_LEAN_ALIASED));
    m.reason = ncls < 1 ? "no site with clusters"
               : ncls > 4 ? "more than 4 site classes"
               : !aliased_ok ? "aliased supercell (a cluster holds a site twice) whose sites do not list their clusters alike"
               : (corr && !corr_k1 && !m.corr_kf && !m.corr_lazy) ? (wl ? "Wang-Landau with more than SMOLMC_LEAN_MAX_KF correlation functions per orbit, more than 61 of them, or TableFlip"
                                                                      : "environment override (SMOLMC_NO_LAZY_FEATURES)")
               : N > 65535 ? "more than 65535 sites"
               : niter_max > 8 ? "more than 512 clusters per site"
               : sc.lean_need_mm > 3 ? "clusters of more than 4 sites"
               : (nfeat > 64 && !m.lazy()) ? "more than 64 cluster features (Wang-Landau or correlation functions on the KF kernels)" : "";
    return m;
}

// lane-packed member rows [site][lane][NSL][MML] of the gathered members; padded entries point at the site itself
static std::vector<uint16_t> lean_index_rows(const smolmc_tables *t, const SiteClasses &sc, int NSL, int MML) {
    const int N = t->num_sites, ROW = NSL * MML;
    std::vector<uint16_t> lidx((size_t)N * 64 * ROW);
    for (int s = 0; s < N; ++s) {
        for (int q = 0; q < 64 * ROW; ++q) lidx[(size_t)s * 64 * ROW + q] = (uint16_t)s;
        const std::vector<Slot> &sl = sc.lean_slots(s);
        for (size_t q = 0; q < sl.size(); ++q) {
            const int it = (int)(q / 64), ln = (int)(q % 64);
            int m = 0;
            for (int a = 0; a < t->orb_nsites[sl[q].orbit]; ++a)
                if (!((sl[q].selfmask >> a) & 1u)) lidx[(((size_t)s * 64 + ln) * NSL + it) * MML + m++] = (uint16_t)sl[q].row[a];
        }
    }
    return lidx;
}

// LDS bank swizzle: the address permutation s ^ (((s >> a) & m) << b) that minimises the modelled
// bank-conflict cycles of the occupancy gathers (each ds_read_u8 is served in two 32-lane groups; a
// group costs the max number of distinct dwords on one of the 32 banks).  tools/lds_conflict_model.py
// restates the model.
struct Swizzle { int a = 0, m = 0, b = 0, Nlds = 0; };
static Swizzle choose_swizzle(const std::vector<uint16_t> &lidx, const SiteClasses &sc, int N, int Npad, int ROW) {
    auto model_cost = [&](int a, int m, int b) {
        double tot = 0;
        const int nsamp = std::min(N, 48);
        for (int k = 0; k < nsamp; ++k) {
            const int s = (int)(((long long)k * 2654435761ll) % N);
            if (sc.lean_slots(s).empty()) continue;
            for (int q = 0; q < ROW; ++q)
                for (int g = 0; g < 2; ++g) {
                    int cnt[32] = {0};
                    int seen[32];
                    int nseen = 0;
                    for (int ln = 32 * g; ln < 32 * g + 32; ++ln) {
                        const int x = lidx[((size_t)s * 64 + ln) * ROW + q];
                        const int dw = (x ^ (((x >> a) & m) << b)) >> 2;
                        bool dup = false;
                        for (int z = 0; z < nseen; ++z) dup |= seen[z] == dw;
                        if (!dup) { seen[nseen++] = dw; cnt[dw & 31]++; }
                    }
                    int mx = 0;
                    for (int z = 0; z < 32; ++z) mx = std::max(mx, cnt[z]);
                    tot += mx;
                }
        }
        return tot;
    };
    Swizzle w;
    w.Nlds = 16;
    while (w.Nlds < Npad) w.Nlds <<= 1;
    double best = model_cost(0, 0, 0);
    for (int a = 3; a <= 12; ++a)
        for (int b = 2; b <= 5; ++b)
            for (int m : {3, 7, 15, 31}) {
                // bijection on [0, Nlds): source bits [a, a+k) above the destination
                // bits [b, b+k) and inside the (power-of-two) array
                const int k = m == 3 ? 2 : (m == 7 ? 3 : (m == 15 ? 4 : 5));
                if (a < b + k || (1 << (a + k)) > w.Nlds) continue;
                const double c = model_cost(a, m, b);
                if (c < best * 0.97) { best = c; w.a = a; w.m = m; w.b = b; }
            }
    if (w.m == 0) w.Nlds = Npad; // identity: no power-of-two padding needed
    return w;
}

// Delta tables, one per (orbit, self positions): D[(old, new)][b] with the COMPACT base
// index b = sum_m S^m * species(member m) over the other members of the cluster (S =
// max species per site), padded to a common [S*S][NTP], NTP = S^MML.  Symmetric
// clusters give bitwise-equal tables for several self positions: those are shared.
struct LeanDeltaTables {
    bool too_large = false;    // more entries than the LDS copy may take: nothing below is complete
    size_t tlen = 0;           // entries of one table
    int NTP = 1;
    // table 0 = zeros, used by padded slots; KF: correlation-function tables (global memory), see LeanParams::dtk
    std::vector<double> dt, dtk;
    std::vector<LeanSlot> ls;  // [class][NSL][64]
    double fast_eps = 0.0;
};
// The tables of one slot: the decision table (LDS) and, in KF mode, K correlation-function tables (global memory,
// read on accepted steps only), tlen entries each
static std::vector<double> slot_delta_tables(const smolmc_tables *t, const Slot &k, const LeanMode &mode, int NTP, size_t tlen) {
    const bool corr = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS, folded = mode.corr_kf || mode.corr_lazy;
    const int o = k.orbit, I = t->orb_nsites[o], Nt = t->orb_tensor_len[o], SMAX = t->max_species;
    const int32_t *st = t->tensor_indices + t->orb_stride_off[o];
    const double *T = corr ? t->corr_tensors + t->orb_ctensor_off[o] // K == 1: the one function
                           : t->interaction_tensors + t->orb_itensor_off[o];
    const int feat = corr ? t->orb_bit_id[o] : t->orb_id[o];
    std::vector<double> Efold; // KF / lazy: folded tensor sum_k coef_k ct_k (decision table source)
    if (folded) {
        Efold.assign((size_t)Nt, 0.0);
        for (int kk = 0; kk < t->orb_nfunc[o]; ++kk)
            for (int i = 0; i < Nt; ++i) Efold[i] += t->ce_coefs[feat + kk] * T[(size_t)kk * Nt + i];
    }
    // the site's own positions: their strides add up (one position on an unaliased cell), its site space is
    // that of the first of them
    int ss = 0;
    for (int a = 0; a < I; ++a)
        if ((k.selfmask >> a) & 1u) ss += st[a];
    const int Sself = member_species(t, o, k.pfirst);
    const int ntab = mode.corr_kf ? 1 + t->orb_nfunc[o] : 1;
    std::vector<double> D((size_t)ntab * tlen, 0.0);
    int nb = 1;
    for (int a = 0; a < k.nother; ++a) nb *= SMAX;
    for (int tb = 0; tb < ntab; ++tb) {
        const double *Tsrc = mode.corr_lazy ? Efold.data() : !mode.corr_kf ? T : (tb == 0 ? Efold.data() : T + (size_t)(tb - 1) * Nt);
        double *Dt = D.data() + (size_t)tb * tlen;
        for (int b = 0; b < nb; ++b) {
            // decode b into the species of the other members -> tensor base index
            long base = 0;
            int rem = b;
            bool valid = true;
            for (int a = 0; a < I; ++a) {
                if ((k.selfmask >> a) & 1u) continue;
                const int v = rem % SMAX;
                rem /= SMAX;
                if (v >= member_species(t, o, a)) valid = false;
                base += (long)st[a] * v;
            }
            if (!valid) continue;
            for (int oldc = 0; oldc < Sself; ++oldc)
                for (int newc = 0; newc < Sself; ++newc)
                    Dt[((size_t)oldc * SMAX + newc) * NTP + b] = Tsrc[base + (long)ss * newc] - Tsrc[base + (long)ss * oldc];
        }
    }
    return D;
}
// where the tables D of a slot start in dt: identical tables are shared (KF: decision AND function tables identical)
static uint32_t place_delta_tables(LeanDeltaTables &L, const std::vector<double> &D, bool kf) {
    const size_t tlen = L.tlen;
    for (size_t off = tlen; off + tlen <= L.dt.size(); off += tlen) {
        if (memcmp(L.dt.data() + off, D.data(), tlen * sizeof(double)) != 0) continue;
        if (kf) {
            std::vector<double> want((size_t)SMOLMC_LEAN_MAX_KF * tlen, 0.0);
            std::copy(D.begin() + tlen, D.end(), want.begin());
            if (memcmp(L.dtk.data() + off * SMOLMC_LEAN_MAX_KF, want.data(), want.size() * sizeof(double)) != 0) continue;
        }
        return (uint32_t)off;
    }
    const uint32_t at = (uint32_t)L.dt.size();
    L.dt.insert(L.dt.end(), D.begin(), D.begin() + tlen);
    if (kf) {
        L.dtk.resize(L.dt.size() * SMOLMC_LEAN_MAX_KF, 0.0);
        std::copy(D.begin() + tlen, D.end(), L.dtk.begin() + (size_t)at * SMOLMC_LEAN_MAX_KF);
    }
    return at;
}
static LeanDeltaTables lean_delta_tables(const smolmc_tables *t, const SiteClasses &sc, const LeanMode &mode, int NSL, int MML) {
    const bool corr = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS, folded = mode.corr_kf || mode.corr_lazy;
    const int SMAX = t->max_species, NCLS = (int)sc.class_rep.size();
    LeanDeltaTables L;
    for (int m = 0; m < MML; ++m) L.NTP *= SMAX;
    // the stride between tables is padded so that it is not a multiple of the 64-dword LDS
    // bank period (lanes of one wave read the same (pair, base) entry of DIFFERENT tables)
    L.tlen = (size_t)SMAX * SMAX * L.NTP;
    if ((L.tlen & 1) == 0) L.tlen += 1;
    L.dt.assign(L.tlen, 0.0);
    // Entries the LDS copy of the tables may take.  8000 (64 KB, two workgroups per CU) until round 6; models between
    // that and what one workgroup's LDS holds beside the walkers' state (the layouts below decide) ran on mc_kernel
    // with the tables in L2: measured on five quaternary triplet / quadruplet models of the fuzz campaign at 2048
    // walkers, 0.39-1.05e9 steps/s there against 0.99-2.43e9 here (tools/time_fuzz_case.py).
    constexpr size_t dt_max = 18000;
    L.ls.resize((size_t)NCLS * NSL * 64);
    memset(L.ls.data(), 0, L.ls.size() * sizeof(LeanSlot));
    std::map<std::pair<int, int>, uint32_t> doff_of;
    double sum_abs_max = 0.0;
    for (int cls = 0; cls < NCLS; ++cls) {
        const std::vector<Slot> &sl = sc.lean_slots(sc.class_rep[cls]);
        double sum_abs = 0.0;
        for (size_t q = 0; q < sl.size(); ++q) {
            const Slot &k = sl[q];
            const int feat = corr ? t->orb_bit_id[k.orbit] : t->orb_id[k.orbit];
            const auto key = std::make_pair(k.orbit, (int)k.selfmask);
            if (!doff_of.count(key)) doff_of[key] = place_delta_tables(L, slot_delta_tables(t, k, mode, L.NTP, L.tlen), mode.corr_kf);
            if (L.dt.size() > dt_max) { L.too_large = true; return L; } // keep the LDS tables within budget
            const double scale = slot_scale(t, k.rec);
            LeanSlot &S = L.ls[((size_t)cls * NSL + q / 64) * 64 + (q % 64)];
            S.doff8 = doff_of[key] * 8u;
            uint32_t cs = 8u;
            for (int m = 0; m < k.nother; ++m, cs *= (uint32_t)SMAX) S.stride8[m] = cs;
            S.feat = mode.lazy() ? 0u : (uint32_t)feat; // (lazy: the kernels' feature cells are never read)
            S.live = mode.corr_kf ? (uint32_t)t->orb_nfunc[k.orbit] : 1u;
            S.w = folded ? scale : t->ce_coefs[feat] * scale; // (KF / lazy: the coefficients are folded into the table)
            S.fs = scale;
            double dmax = 0.0;
            const double *D = L.dt.data() + doff_of[key];
            for (size_t z = 0; z < L.tlen; ++z) dmax = std::max(dmax, std::fabs(D[z]));
            sum_abs += std::fabs(S.w) * dmax;
        }
        sum_abs_max = std::max(sum_abs_max, sum_abs);
    }
    // float32 pre-test of the accept decision: a step sums at most two flips' worth of
    // |w * d| over the slots, a float32 conversion + 6-level tree adds at most
    // 7 * 2^-24 of that; 2^-19 leaves a 4.5x margin.  (That is the derivation.  Measured with the threshold placed
    // a hair from the exact dH on every tested step, tests/fast_band.py: no wrong decision at this band, the first at
    // the band scaled by 2^-7 .. 2^-11 depending on the kernel family, i.e. a margin of 128x or more on every tested
    // case -- profiles/fast_band_margin.jsonl)
    L.fast_eps = 2.0 * sum_abs_max * ldexp(1.0, -19);
    return L;
}

// ---- solo rows (mc_lean.h: ROWS): per-slot gather widths, index rows in LDS-address order
// The clusters of a site, sorted by gathered members (most first, stable), fill the two slots of a solo handle; a slot
// then gathers what its widest lane needs.  Taken when that is two members in slot 0 and one in slot 1 (shape 21:
// triplets that fit one slot beside pairs) or one in both (11: pairs only); anything else keeps the plain solo kernel.
// (site_slots already lists a site's clusters with most gathered members first, so on tables built here the
// permutation is the identity; it is derived from the slot records all the same, so that the rows do not depend on it.)
struct SoloRowsPlan {
    int shape = 0;                // the kernel's MM: 21, 11, or 0 (not taken)
    int row_len = 0;              // entries per lane of a row
    std::vector<int> perm;        // position (slot * 64 + lane) in the new order -> position in the lean row
    std::vector<uint32_t> rows;   // [Nlds][64][row_len]: the row of site s at lean_swz(s); other addresses: self-references
    std::vector<LeanSlot> slots;  // [2][64]: the slot records in the new order
};
// lidx: the lean rows [N][64][NSL][MML], entries swizzled; ls: the slot records [NSL][64] of the one site class
static SoloRowsPlan solo_rows_plan(const std::vector<uint16_t> &lidx, const LeanSlot *ls, int N, int NSL, int MML, const Swizzle &w) {
    SoloRowsPlan p;
    if (NSL != 2 || MML != 2 || w.Nlds < N || lidx.size() != (size_t)N * 64 * NSL * MML) return p;
    const int NQ = 64 * NSL;
    // gathered members of a position: its strides (padded positions and the point cluster have none)
    int nm[128];
    for (int q = 0; q < NQ; ++q) {
        nm[q] = 0;
        for (int m = 0; m < MML; ++m)
            if (ls[q].live && ls[q].stride8[m]) nm[q] = m + 1;
    }
    p.perm.resize(NQ);
    for (int q = 0; q < NQ; ++q) p.perm[q] = q;
    std::stable_sort(p.perm.begin(), p.perm.end(), [&](int a, int b) { return nm[a] > nm[b]; });
    const int mm0 = nm[p.perm[0]], mm1 = nm[p.perm[64]]; // (sorted: a slot's first lane is its widest)
    if (mm0 > 2 || mm1 > 1) return p;
    const int w0 = mm0 == 2 ? 2 : 1;
    p.shape = w0 * 10 + 1;
    p.row_len = w0 + 1;
    const int RL = p.row_len, width[2] = {w0, 1}, off[2] = {0, w0};
    p.slots.resize(NQ);
    for (int q = 0; q < NQ; ++q) p.slots[q] = ls[p.perm[q]];
    p.rows.resize((size_t)w.Nlds * 64 * RL);
    for (int a = 0; a < w.Nlds; ++a)
        for (int k = 0; k < 64 * RL; ++k) p.rows[(size_t)a * 64 * RL + k] = (uint32_t)a;
    for (int s = 0; s < N; ++s) {
        const int a = s ^ (((s >> w.a) & w.m) << w.b);
        for (int q = 0; q < NQ; ++q) {
            const int it = q / 64, ln = q % 64, oit = p.perm[q] / 64, oln = p.perm[q] % 64;
            // (a lane with fewer members than its slot gathers keeps the lean row's padding: the site itself, stride 0)
            for (int m = 0; m < width[it]; ++m)
                p.rows[((size_t)a * 64 + ln) * RL + off[it] + m] = lidx[(((size_t)s * 64 + oln) * NSL + oit) * MML + m];
        }
    }
    return p;
}

// The lean tables are taken: the one place that writes them to the handle and the device
static int commit_lean_tables(smolmc_handle *h, const smolmc_tables *t, const SiteClasses &sc, const LeanMode &mode, int NSL, int MML,
                              const Swizzle &w, std::vector<uint16_t> &lidx, const LeanDeltaTables &L) {
    LeanParams &lp = h->lp;
    memset(&lp, 0, sizeof(LeanParams));
    lp.swz_a = w.a; lp.swz_m = w.m; lp.swz_b = w.b; lp.Nlds = w.Nlds;
    lp.fast_eps = L.fast_eps;
    lp.ktab8 = (uint32_t)L.tlen * 8u;
    lp.nt8 = (uint32_t)L.NTP * 8u;
    lp.snt8 = (uint32_t)L.NTP * 8u * (uint32_t)t->max_species;
    TRY(dev_upload(h, lidx.data(), lidx.size(), &lp.idx));
    h->lean_idx_host = std::move(lidx);
    TRY(dev_upload(h, L.dt.data(), L.dt.size(), &lp.dt));
    if (mode.corr_kf) TRY(dev_upload(h, L.dtk.data(), L.dtk.size(), &lp.dtk));
    TRY(dev_upload(h, L.ls.data(), L.ls.size(), &lp.slots));
    h->lean_slots_host = L.ls;
    lp.dt_len = (int)L.dt.size();
    h->lean_kf = mode.corr_kf ? SMOLMC_LEAN_MAX_KF : 0;
    h->lazy_tables = mode.lazy();
    h->lean_tables = true;
    h->lean_nslot = NSL; h->lean_mm = MML; h->lean_ncls = (int)sc.class_rep.size();
    h->site_class_host = sc.site_class;
    return 0;
}

static int build_mc_tables(smolmc_handle *h, const smolmc_tables *t) {
    const GeneralLimits lim = general_limits(t, h->Npad);
    if (lim.error) return fail(lim.error);
    if (lim.universal) return no_general(h, lim.universal);
    const SiteClasses sc = site_classes(t, lim);
    if (sc.universal) return no_general(h, sc.universal);
    TRY(general_tables(h, t, lim, sc));
    if (!h->general_ok) return 0;
    // the lean tables are built exactly when nothing speaks against them
    const LeanMode mode = lean_mode(h, t, lim, sc);
    const char *why_not = mode.reason;
    const int NSL = sc.niter_max <= 2 ? 2 : (sc.niter_max <= 4 ? 4 : 8), MML = sc.lean_need_mm <= 2 ? 2 : 3;
    std::vector<uint16_t> lidx;
    Swizzle w;
    LeanDeltaTables L;
    if (!*why_not) {
        lidx = lean_index_rows(t, sc, NSL, MML);
        w = choose_swizzle(lidx, sc, t->num_sites, h->Npad, NSL * MML);
        for (uint16_t &x : lidx) x = (uint16_t)(x ^ (((x >> w.a) & w.m) << w.b));
        L = lean_delta_tables(t, sc, mode, NSL, MML);
        if (L.too_large) why_not = "delta tables beyond 18000 entries (species^(cluster size - 1) x species^2 per distinct table)";
    }
    h->lean_reason = why_not;
    return *why_not ? 0 : commit_lean_tables(h, t, sc, mode, NSL, MML, w, lidx, L);
}

// Bounds checks of every gather index the kernels will use, done once at create (the
// reference's compiled core runs with boundscheck=False and reads garbage for a bad index).  The
// kernels themselves never check: every index they form comes from these tables and from occupancy
// codes, which smolmc_set_state checks against the tables.  -DSMOLMC_BOUNDS adds device-side traps
// at the gathers of the lean kernels for debugging the kernels' own address arithmetic.
static int validate_tables(const smolmc_tables *t) {
    const int N = t->num_sites, n = t->n_orb;
    if (N <= 0 || n < 0 || t->size <= 0) return fail("num_sites / size / n_orb must be positive");
    int nstr = 0;
    for (int o = 0; o < n; ++o) {
        if (t->orb_nsites[o] <= 0 || t->orb_nfunc[o] <= 0 || t->orb_tensor_len[o] <= 0)
            return fail("orbit record with a non-positive size");
        if (t->orb_stride_off[o] != nstr) return fail("orb_stride_off does not follow the orbit sizes");
        nstr += t->orb_nsites[o];
        // the largest flat tensor index a cluster of this orbit can form must lie inside the tensor
        // (strides of a row-major tensor over the site spaces of the cluster, orbit.py:268-275: member m
        // has orb_tensor_len / stride_0 species for m = 0 and stride_{m-1} / stride_m after that; the
        // largest flat index sum_m (species_m - 1) stride_m is then orb_tensor_len - 1)
        long long prev = t->orb_tensor_len[o], reach = 0;
        for (int m = 0; m < t->orb_nsites[o]; ++m) {
            const int st = t->tensor_indices[t->orb_stride_off[o] + m];
            if (st <= 0) return fail("tensor stride must be positive");
            if (st > prev || prev % st != 0) return fail("tensor strides do not describe a row-major tensor");
            reach += (long long)(member_species(t, o, m) - 1) * st;
            prev = st;
        }
        if (reach >= t->orb_tensor_len[o]) return fail("tensor strides reach beyond their tensor");
        const int64_t a = t->full_off[o], b = t->full_off[o + 1];
        if (b < a || (b - a) % t->orb_nsites[o] != 0) return fail("full_off does not describe whole cluster rows");
        for (int64_t i = a; i < b; ++i)
            if (t->full_idx[i] < 0 || t->full_idx[i] >= N) return fail("cluster site index out of range (full table)");
    }
    for (int s = 0; s < N; ++s)
        if (t->site_ptr[s + 1] < t->site_ptr[s]) return fail("site_ptr must be non-decreasing");
    const int64_t nloc = t->site_ptr[N];
    for (int64_t r = 0; r < nloc; ++r) {
        const int o = t->loc_orbit[r];
        if (o < 0 || o >= n) return fail("local record refers to an orbit out of range");
        if (t->loc_nrows[r] <= 0 || !(t->loc_ratio[r] > 0)) return fail("local record with a non-positive size / ratio");
        const int64_t cnt = (int64_t)t->loc_nrows[r] * t->orb_nsites[o];
        for (int64_t i = 0; i < cnt; ++i) {
            const int v = t->loc_idx[t->loc_off[r] + i];
            if (v < 0 || v >= N) return fail("cluster site index out of range (local table)");
        }
    }
    if (t->has_ewald) {
        if (t->ewald_width <= 0 || t->ewald_dim <= 0) return fail("Ewald table with a non-positive size");
        for (int64_t i = 0; i < (int64_t)N * t->ewald_width; ++i)
            if (t->ewald_inds[i] < -1 || t->ewald_inds[i] >= t->ewald_dim) return fail("Ewald index out of range");
    }
    if (t->has_mu && t->mu_width <= 0) return fail("chemical-potential table with a non-positive width");
    return 0;
}

static int build_ref_tables(smolmc_handle *h, const smolmc_tables *t) {
    RefTables &rt = h->rt;
    memset(&rt, 0, sizeof(rt));
    const int n = t->n_orb;
    rt.N = t->num_sites;
    rt.Npad = h->Npad;
    rt.P = t->size;
    rt.num_orbits = t->num_orbits;
    rt.num_corr = t->num_corr;
    rt.n_orb = n;
    rt.Fce = h->Fce;
    rt.F = h->F;
    rt.corr_mode = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS;
    rt.offset = t->offset;
    int nstr = 0;
    long long nct = 0, nit = 0;
    for (int o = 0; o < n; ++o) {
        nstr += t->orb_nsites[o];
        nct += (long long)t->orb_nfunc[o] * t->orb_tensor_len[o];
        nit += t->orb_tensor_len[o];
    }
    const int64_t nloc = t->site_ptr[t->num_sites];
    int64_t nlocidx = 0;
    for (int64_t r = 0; r < nloc; ++r)
        nlocidx += (int64_t)t->loc_nrows[r] * t->orb_nsites[t->loc_orbit[r]];
    TRY(dev_upload(h, t->orb_id, n, &rt.orb_id));
    TRY(dev_upload(h, t->orb_bit_id, n, &rt.orb_bit_id));
    TRY(dev_upload(h, t->orb_nsites, n, &rt.orb_nsites));
    TRY(dev_upload(h, t->orb_nfunc, n, &rt.orb_nfunc));
    TRY(dev_upload(h, t->orb_tensor_len, n, &rt.orb_tensor_len));
    TRY(dev_upload(h, t->orb_stride_off, n, &rt.orb_stride_off));
    TRY(dev_upload(h, t->tensor_indices, nstr, &rt.tensor_indices));
    TRY(dev_upload(h, (const long long *)t->orb_ctensor_off, n, &rt.orb_ctensor_off));
    TRY(dev_upload(h, (const long long *)t->orb_itensor_off, n, &rt.orb_itensor_off));
    TRY(dev_upload(h, t->corr_tensors, nct, &rt.corr_tensors));
    TRY(dev_upload(h, t->interaction_tensors, nit, &rt.interaction_tensors));
    TRY(dev_upload(h, (const long long *)t->full_off, n + 1, &rt.full_off));
    TRY(dev_upload(h, t->full_idx, t->full_off[n], &rt.full_idx));
    TRY(dev_upload(h, (const long long *)t->site_ptr, t->num_sites + 1, &rt.site_ptr));
    TRY(dev_upload(h, t->loc_orbit, nloc, &rt.loc_orbit));
    TRY(dev_upload(h, t->loc_ratio, nloc, &rt.loc_ratio));
    TRY(dev_upload(h, t->loc_nrows, nloc, &rt.loc_nrows));
    TRY(dev_upload(h, (const long long *)t->loc_off, nloc, &rt.loc_off));
    TRY(dev_upload(h, t->loc_idx, nlocidx, &rt.loc_idx));
    rt.has_ewald = t->has_ewald;
    rt.has_mu = t->has_mu;
    if (t->has_ewald) {
        const size_t M = t->ewald_dim;
        rt.ew_W = t->ewald_width;
        rt.ew_M = (int)M;
        TRY(dev_upload(h, t->ewald_inds, (size_t)t->num_sites * t->ewald_width, &rt.ew_inds));
        TRY(dev_upload(h, t->ewald_matrix, M * M, &rt.ew_M_rowmajor));
        std::vector<double> mt(M * M);
        const size_t B = 64;
        for (size_t i0 = 0; i0 < M; i0 += B)
            for (size_t j0 = 0; j0 < M; j0 += B)
                for (size_t i = i0; i < std::min(M, i0 + B); ++i)
                    for (size_t j = j0; j < std::min(M, j0 + B); ++j)
                        mt[j * M + i] = t->ewald_matrix[i * M + j];
        TRY(dev_upload(h, mt.data(), M * M, &rt.ew_Mt));
    }
    if (t->has_mu) {
        rt.mu_W = t->mu_width;
        TRY(dev_upload(h, t->mu_table, (size_t)t->num_sites * t->mu_width, &rt.mu));
    }
    return 0;
}

// Check M[a][b] == q_a q_b G[site_a][site_b] (a, b on different sites) and build G.
// Translation-compressed site kernel.  On a supercell of a periodic lattice the site
// kernel G[s][j] of the compact Ewald form depends on the sublattices of s and j and on the lattice
// translation between them only (smol/utils/cluster/ewald.pyx:38-58 reads the same numbers N times
// over).  When the changeable sites come as contiguous blocks of P = `size` sites in the
// lexicographic order of the translation coordinates of a d1 x d2 x d3 supercell -- the order of
// pymatgen's lattice_points_in_supercell (and smol_amd.synth) for diagonal supercell matrices; no
// coordinates travel through the C ABI, the structure is found and then VERIFIED on every entry of
// G -- one table per block pair over the coordinate differences -(d-1) .. d-1 replaces the rows in the
// potential-field updates (field_sweep_gx, smolmc_common.h): entry (s, j) at byte E8[j] + S8[s].
// Anything else (non-diagonal supercells, other site orders) keeps the rows of G.
static int compress_ewald_rows(smolmc_handle *h, const smolmc_tables *t, const std::vector<double> &Gact,
                               const std::vector<int> &act) {
    const size_t na = act.size();
    const int P = t->size;
    if (smolmc_env(ENV_NO_EWALD_GX) || P <= 1 || na == 0 || na % (size_t)P != 0) return 0;
    const int nbk = (int)(na / (size_t)P);
    for (size_t j = 0; j < na; ++j)
        if (act[j] != act[0] + (int)j) return 0; // (the field mode needs contiguous changeable sites anyway)
    auto Gat = [&](size_t js, size_t j) { return Gact[(size_t)act[js] * na + j]; };
    double gmax = 0.0;
    for (size_t js = 0; js < na; ++js)
        for (size_t j = 0; j < na; ++j) gmax = std::max(gmax, std::fabs(Gat(js, j)));
    const double tol = 1e-12 * std::max(gmax, 1e-300);
    // entry (block k, translation t) x (block k2, translation t2) against row "translation 0" of
    // block k at the wrapped coordinate difference
    auto rows_match = [&](const int d[3], int k, int tt) {
        const int x = tt / (d[1] * d[2]), y = (tt / d[2]) % d[1], z = tt % d[2];
        for (int k2 = 0; k2 < nbk; ++k2)
            for (int t2 = 0; t2 < P; ++t2) {
                const int x2 = t2 / (d[1] * d[2]), y2 = (t2 / d[2]) % d[1], z2 = t2 % d[2];
                const int rel = (((x2 - x + d[0]) % d[0]) * d[1] + (y2 - y + d[1]) % d[1]) * d[2] + (z2 - z + d[2]) % d[2];
                if (std::fabs(Gat((size_t)k * P + tt, (size_t)k2 * P + t2) - Gat((size_t)k * P, (size_t)k2 * P + rel)) > tol)
                    return false;
            }
        return true;
    };
    // factorisations d1 d2 d3 = P, the most balanced first; a few rows screen a candidate, then
    // every row confirms it
    std::vector<std::array<int, 3>> cand;
    for (int a = 1; a <= P; ++a)
        if (P % a == 0)
            for (int b = 1; b <= P / a; ++b)
                if ((P / a) % b == 0) cand.push_back({a, b, P / a / b});
    std::sort(cand.begin(), cand.end(), [](const std::array<int, 3> &u, const std::array<int, 3> &v) {
        auto spread = [](const std::array<int, 3> &w) { return std::max({w[0], w[1], w[2]}) - std::min({w[0], w[1], w[2]}); };
        return spread(u) < spread(v);
    });
    int d[3] = {0, 0, 0};
    bool found = false;
    for (const auto &c : cand) {
        const int dd[3] = {c[0], c[1], c[2]};
        bool ok = true;
        for (int probe : {1, P / 2 + 1, P - 1, (int)((2654435761u % (unsigned)P))})
            if (ok && probe > 0 && probe < P) ok = rows_match(dd, nbk - 1, probe);
        for (int k = 0; ok && k < nbk; ++k)
            for (int tt = 0; ok && tt < P; ++tt) ok = rows_match(dd, k, tt);
        if (ok) { d[0] = dd[0]; d[1] = dd[1]; d[2] = dd[2]; found = true; break; }
    }
    if (!found) return 0;
    const int e[3] = {2 * d[0] - 1, 2 * d[1] - 1, 2 * d[2] - 1};
    const size_t EXT = (size_t)e[0] * e[1] * e[2];
    if ((size_t)nbk * nbk * EXT * 8 >= ((size_t)1 << 31)) return 0; // 32-bit byte offsets
    std::vector<double> gx((size_t)nbk * nbk * EXT);
    for (int k = 0; k < nbk; ++k)
        for (int k2 = 0; k2 < nbk; ++k2)
            for (int a = 0; a < e[0]; ++a)
                for (int b = 0; b < e[1]; ++b)
                    for (int c = 0; c < e[2]; ++c) {
                        const int rel = (((a - (d[0] - 1) + d[0]) % d[0]) * d[1] + (b - (d[1] - 1) + d[1]) % d[1]) * d[2] +
                                        (c - (d[2] - 1) + d[2]) % d[2];
                        gx[((size_t)k * nbk + k2) * EXT + ((size_t)a * e[1] + b) * e[2] + c] = Gat((size_t)k * P, (size_t)k2 * P + rel);
                    }
    const size_t center = ((size_t)(d[0] - 1) * e[1] + (d[1] - 1)) * e[2] + (d[2] - 1);
    std::vector<uint32_t> E8(na), S8(na);
    for (int k = 0; k < nbk; ++k)
        for (int tt = 0; tt < P; ++tt) {
            const int x = tt / (d[1] * d[2]), y = (tt / d[2]) % d[1], z = tt % d[2];
            const size_t E = ((size_t)x * e[1] + y) * e[2] + z;
            E8[(size_t)k * P + tt] = (uint32_t)(8 * ((size_t)k * EXT + E));
            S8[(size_t)k * P + tt] = (uint32_t)(8 * ((size_t)k * nbk * EXT + center - E));
        }
    TRY(dev_upload(h, gx.data(), gx.size(), &h->kp.ew_gx));
    TRY(dev_upload(h, E8.data(), E8.size(), &h->kp.ew_E8));
    TRY(dev_upload(h, S8.data(), S8.size(), &h->kp.ew_S8));
    h->ew_gx_dims[0] = d[0]; h->ew_gx_dims[1] = d[1]; h->ew_gx_dims[2] = d[2];
    h->ew_gx_blocks = nbk;
    return 0;
}

static int build_compact_ewald(smolmc_handle *h, const smolmc_tables *t) {
    const int N = t->num_sites, W = t->ewald_width;
    const size_t M = (size_t)t->ewald_dim;
    const double *Mx = t->ewald_matrix, *q = t->ewald_charges;
    std::vector<double> G((size_t)N * N, 0.0), qs((size_t)N * W, 0.0), dg((size_t)N * W, 0.0);
    double mmax = 0;
    for (size_t i = 0; i < M * M; ++i) mmax = std::max(mmax, fabs(Mx[i]));
    const double tol = 1e-12 * std::max(mmax, 1e-300);
    for (int s = 0; s < N; ++s)
        for (int c = 0; c < W; ++c) {
            const int a = t->ewald_inds[(size_t)s * W + c];
            if (a < 0) continue;
            qs[(size_t)s * W + c] = q[a];
            dg[(size_t)s * W + c] = Mx[(size_t)a * M + a];
        }
    bool ok = true;
    for (int s = 0; s < N && ok; ++s)
        for (int u = 0; u < N && ok; ++u) {
            if (s == u) continue;
            double g = 0;
            bool have = false;
            for (int c = 0; c < W && !have; ++c)
                for (int d = 0; d < W && !have; ++d) {
                    const int a = t->ewald_inds[(size_t)s * W + c], b = t->ewald_inds[(size_t)u * W + d];
                    if (a < 0 || b < 0 || q[a] == 0.0 || q[b] == 0.0) continue;
                    g = Mx[(size_t)b * M + a] / (q[a] * q[b]); // the entry ewald.pyx reads: M[i_k, add]
                    have = true;
                }
            for (int c = 0; c < W && ok; ++c)
                for (int d = 0; d < W && ok; ++d) {
                    const int a = t->ewald_inds[(size_t)s * W + c], b = t->ewald_inds[(size_t)u * W + d];
                    if (a < 0 || b < 0) continue;
                    if (fabs(Mx[(size_t)b * M + a] - q[a] * q[b] * g) > tol) ok = false;
                }
            G[(size_t)s * N + u] = g; // row s: kernel between the flipped site s and site u
        }
    if (!ok) return 0; // not of product form: keep the dense rows
    // split sites into changeable ones and single-species ("frozen") ones
    std::vector<int> act;
    std::vector<char> frozen(N, 0);
    std::vector<char> in_active(N, 0);
    for (int64_t i = 0; i < t->sub_site_ptr[t->n_sublattices]; ++i)
        if (t->sub_active_sites[i] >= 0 && t->sub_active_sites[i] < N) in_active[t->sub_active_sites[i]] = 1;
    for (int s = 0; s < N; ++s) {
        // a site is frozen when it is in no active sublattice (its code never changes) and
        // carries exactly one Ewald species (code 0)
        frozen[s] = (!in_active[s] && single_ewald_species(t, s)) ? 1 : 0;
        if (!frozen[s]) act.push_back(s);
    }
    const size_t na = act.size();
    std::vector<double> Gact((size_t)N * std::max<size_t>(na, 1), 0.0), fz(N, 0.0);
    for (int s = 0; s < N; ++s) {
        for (size_t j = 0; j < na; ++j) Gact[(size_t)s * na + j] = G[(size_t)s * N + act[j]];
        double c = 0;
        for (int u = 0; u < N; ++u)
            if (frozen[u] && u != s) c += qs[(size_t)u * W] * G[(size_t)s * N + u];
        fz[s] = c;
    }
    TRY(dev_upload(h, act.data(), act.size(), &h->kp.ew_act));
    TRY(dev_upload(h, fz.data(), fz.size(), &h->kp.ew_frozen));
    h->kp.ew_nact = (int)na;
    h->kp.ew_act_base = na ? act[0] : -1;
    for (size_t j = 0; j < na; ++j)
        if (act[j] != act[0] + (int)j) h->kp.ew_act_base = -1;
    G.swap(Gact);
    TRY(compress_ewald_rows(h, t, G, act));
    TRY(dev_upload(h, G.data(), G.size(), &h->kp.ew_G));
    TRY(dev_upload(h, qs.data(), qs.size(), &h->kp.ew_qs));
    TRY(dev_upload(h, dg.data(), dg.size(), &h->kp.ew_dg));
    h->ew_qs_host = qs;
    h->ew_dg_host = dg;
    h->kp.ew_compact = 1;
    return 0;
}

extern "C" int smolmc_abi_version(void) { return SMOLMC_ABI_VERSION; }
extern "C" const char *smolmc_last_error(void) { return smolmc_g_err.c_str(); }

// ---- site relabelling behind the boundary (ABI 8) -------------------------------------------------------------
// The lean kernel families index an active sublattice as ONE site range (site = base + mulhi(word, n_active)).
// Ensemble.restrict_sites and split_sublattice_by_species (smol/moca/sublattice.py:84-186, ensemble.py:288-321)
// leave the active sites of a sublattice scattered.  smolmc_create then renumbers the sites ITSELF: the active sites
// of every sublattice first, in the order of their lists (so a walker draws the same physical site from the same
// random word), then the other sites whose species can differ between occupancies (restricted sites: the Ewald
// potential field covers one block of changeable sites), then the rest, each group in the caller's order.  The handle
// is built from the renumbered tables; occupancies, step records and sample rows cross every entry point in the
// CALLER's numbering (set_state / get_state / get_samples* / replay / eval_full / eval_delta).  Rounds 4-5 did this in
// the Python binding only (capi.TableSet.permute_sites), so a C client of this header got mc_kernel.
struct RelabelledTables {
    smolmc_tables t;
    std::vector<int32_t> full_idx, loc_idx, sub_active_sites, loc_orbit, loc_nrows, ewald_inds;
    std::vector<int64_t> site_ptr, loc_off;
    std::vector<double> loc_ratio, mu_table, bias_table;
};

// new_of (caller's site -> engine's site) when a relabelling is needed and possible, else empty
static std::vector<int32_t> plan_relabelling(const smolmc_tables *t) {
    std::vector<int32_t> none;
    const int N = t->num_sites, ns = t->n_sublattices;
    if (N <= 0 || ns <= 0 || !t->sub_site_ptr || !t->sub_active_sites || smolmc_env(ENV_NO_SITE_RELABEL)) return none;
    bool needed = false;
    std::vector<char> taken((size_t)N, 0);
    std::vector<int32_t> order;
    order.reserve((size_t)N);
    for (int k = 0; k < ns; ++k) {
        const int64_t a = t->sub_site_ptr[k], b = t->sub_site_ptr[k + 1];
        for (int64_t i = a; i < b; ++i) {
            const int st = t->sub_active_sites[i];
            if (st < 0 || st >= N || taken[st]) return none; // (malformed lists: smolmc_create reports them)
            taken[st] = 1;
            order.push_back(st);
            if (st != t->sub_active_sites[a] + (int)(i - a)) needed = true;
        }
    }
    if (!needed) return none;
    // sites outside the active lists: changeable ones (more than one Ewald species, or a vacancy: what
    // build_compact_ewald does not fold into the frozen-site constants) before the single-species ones
    auto frozen = [&](int s) { return !t->has_ewald || !t->ewald_inds || single_ewald_species(t, s); };
    for (int pass = 0; pass < 2; ++pass)
        for (int s = 0; s < N; ++s)
            if (!taken[s] && frozen(s) == (pass == 1)) order.push_back(s);
    if ((int)order.size() != N) return none;
    std::vector<int32_t> new_of((size_t)N);
    for (int p = 0; p < N; ++p) new_of[order[p]] = p;
    return new_of;
}

// the caller's tables with site p renamed new_of[p] in every site-indexed array (validate_tables has passed)
static void relabel_tables(const smolmc_tables *t, const std::vector<int32_t> &new_of, const std::vector<int32_t> &old_of,
                           RelabelledTables &rt) {
    const int N = t->num_sites;
    rt.t = *t;
    const int64_t nfull = t->full_off[t->n_orb], nrec = t->site_ptr[N];
    rt.full_idx.resize((size_t)nfull);
    for (int64_t i = 0; i < nfull; ++i) rt.full_idx[i] = new_of[t->full_idx[i]];
    int64_t nloc = 0;
    for (int64_t r = 0; r < nrec; ++r)
        nloc = std::max<int64_t>(nloc, t->loc_off[r] + (int64_t)t->loc_nrows[r] * t->orb_nsites[t->loc_orbit[r]]);
    rt.loc_idx.resize((size_t)nloc);
    for (int64_t i = 0; i < nloc; ++i) {
        const int v = t->loc_idx[i];
        rt.loc_idx[i] = (v >= 0 && v < N) ? new_of[v] : v; // (entries between records, if any, are never read)
    }
    // the record range of engine site p is that of the caller's site old_of[p]
    rt.site_ptr.assign((size_t)N + 1, 0);
    rt.loc_orbit.reserve((size_t)nrec); rt.loc_nrows.reserve((size_t)nrec);
    rt.loc_off.reserve((size_t)nrec); rt.loc_ratio.reserve((size_t)nrec);
    for (int p = 0; p < N; ++p) {
        const int q = old_of[p];
        for (int64_t r = t->site_ptr[q]; r < t->site_ptr[q + 1]; ++r) {
            rt.loc_orbit.push_back(t->loc_orbit[r]);
            rt.loc_nrows.push_back(t->loc_nrows[r]);
            rt.loc_off.push_back(t->loc_off[r]);
            rt.loc_ratio.push_back(t->loc_ratio[r]);
        }
        rt.site_ptr[(size_t)p + 1] = (int64_t)rt.loc_orbit.size();
    }
    const int64_t nact = t->sub_site_ptr[t->n_sublattices];
    rt.sub_active_sites.resize((size_t)nact);
    for (int64_t i = 0; i < nact; ++i) rt.sub_active_sites[i] = new_of[t->sub_active_sites[i]];
    auto rows = [&](const auto *src, int width, int blocks, auto &dst) {
        dst.resize((size_t)blocks * N * width);
        for (int b = 0; b < blocks; ++b)
            for (int p = 0; p < N; ++p)
                std::copy(src + ((size_t)b * N + old_of[p]) * width, src + ((size_t)b * N + old_of[p] + 1) * width,
                          dst.begin() + ((size_t)b * N + p) * width);
    };
    rt.t.full_idx = rt.full_idx.data();
    rt.t.loc_idx = rt.loc_idx.data();
    rt.t.site_ptr = rt.site_ptr.data();
    rt.t.loc_orbit = rt.loc_orbit.data();
    rt.t.loc_nrows = rt.loc_nrows.data();
    rt.t.loc_off = rt.loc_off.data();
    rt.t.loc_ratio = rt.loc_ratio.data();
    rt.t.sub_active_sites = rt.sub_active_sites.data();
    if (t->has_ewald && t->ewald_inds) {
        rows(t->ewald_inds, t->ewald_width, 1, rt.ewald_inds);
        rt.t.ewald_inds = rt.ewald_inds.data();
    }
    if (t->has_mu && t->mu_table) {
        rows(t->mu_table, t->mu_width, 1, rt.mu_table);
        rt.t.mu_table = rt.mu_table.data();
    }
    if (t->bias_type && t->bias_table && t->bias_width > 0) {
        const int brows = t->bias_type == SMOLMC_BIAS_SQUARE_HYPERPLANE ? std::max(1, std::min(t->bias_rows, SMOLMC_MAX_BIAS_ROWS)) : 1;
        rows(t->bias_table, t->bias_width, brows, rt.bias_table);
        rt.t.bias_table = rt.bias_table.data();
    }
}

static int create_impl(const smolmc_tables *t, const smolmc_config *cfg, smolmc_handle **out, std::vector<int32_t> *new_of);

// Test hooks, NOT part of the C-ABI (not in include/smolmc.h): the renumbering smolmc_create would apply to these
// tables, as a heap copy whose first member is the renumbered smolmc_tables (NULL: none needed / possible), and the
// map caller's site -> engine's site.  Host code only: tests/test_relabel_host.py runs the CPU oracle on both table
// sets without a GPU.
extern "C" void *smolmc_debug_relabel(const smolmc_tables *t, int32_t *new_of_out) {
    if (!t || validate_tables(t)) return nullptr;
    std::vector<int32_t> new_of = plan_relabelling(t);
    if (new_of.empty()) return nullptr;
    std::vector<int32_t> old_of(new_of.size());
    for (size_t p = 0; p < new_of.size(); ++p) old_of[new_of[p]] = (int32_t)p;
    RelabelledTables *rt = new RelabelledTables();
    relabel_tables(t, new_of, old_of, *rt);
    if (new_of_out) std::copy(new_of.begin(), new_of.end(), new_of_out);
    return rt;
}
extern "C" void smolmc_debug_relabel_free(void *p) { delete (RelabelledTables *)p; }

// ... and the solo rows plan (solo_rows_plan) of a Metropolis handle on these tables, from the lean tables as
// build_mc_tables makes them.  Host code only (tests/test_solo_rows_host.py).  The leading members are plain data a
// ctypes.Structure mirrors; shape 0: the tables get no lean rows, or the clusters fall into neither shape.
struct SoloRowsDebug {
    int shape, row_len, N, Nlds, swz_a, swz_m, swz_b, nslot, mm;
    const int *perm;             // [64 * nslot]
    const uint32_t *rows;        // [Nlds][64][row_len]
    const LeanSlot *slots;       // [nslot][64], new order
    const uint16_t *lean_rows;   // [N][64][nslot][mm], swizzled: what lp.idx holds
    const LeanSlot *lean_slots;  // [nslot][64]: what lp.slots holds
    SoloRowsPlan plan;
    std::vector<uint16_t> lidx;
    std::vector<LeanSlot> ls;
};
// (smolmc_debug_solo_rows) the lean tables of build_mc_tables without a device, and the solo rows plan on them
static void build_mc_tables_host(const smolmc_tables *t, const smolmc_config *cfg, SoloRowsDebug &d) {
    smolmc_handle h; // (never reaches a device: the planners below read its configuration only)
    h.cfg = *cfg;
    h.Npad = (t->num_sites + 15) / 16 * 16;
    d.N = t->num_sites;
    const GeneralLimits lim = general_limits(t, h.Npad);
    if (lim.error || lim.universal) return;
    const SiteClasses sc = site_classes(t, lim);
    if (sc.universal) return;
    const LeanMode mode = lean_mode(&h, t, lim, sc);
    if (*mode.reason || mode.corr_kf) return;
    const int NSL = sc.niter_max <= 2 ? 2 : (sc.niter_max <= 4 ? 4 : 8), MML = sc.lean_need_mm <= 2 ? 2 : 3;
    d.nslot = NSL; d.mm = MML;
    d.lidx = lean_index_rows(t, sc, NSL, MML);
    const Swizzle w = choose_swizzle(d.lidx, sc, t->num_sites, h.Npad, NSL * MML);
    for (uint16_t &x : d.lidx) x = (uint16_t)(x ^ (((x >> w.a) & w.m) << w.b));
    d.Nlds = w.Nlds; d.swz_a = w.a; d.swz_m = w.m; d.swz_b = w.b;
    const LeanDeltaTables L = lean_delta_tables(t, sc, mode, NSL, MML);
    if (L.too_large) return;
    d.ls = L.ls;
    if (sc.class_rep.size() == 1) d.plan = solo_rows_plan(d.lidx, d.ls.data(), t->num_sites, NSL, MML, w);
}
extern "C" void *smolmc_debug_solo_rows(const smolmc_tables *t, const smolmc_config *cfg) {
    if (!t || !cfg || validate_tables(t)) return nullptr;
    SoloRowsDebug *d = new SoloRowsDebug();
    build_mc_tables_host(t, cfg, *d);
    d->shape = d->plan.shape; d->row_len = d->plan.row_len;
    d->perm = d->plan.perm.data(); d->rows = d->plan.rows.data(); d->slots = d->plan.slots.data();
    d->lean_rows = d->lidx.data(); d->lean_slots = d->ls.data();
    return d;
}
extern "C" void smolmc_debug_solo_rows_free(void *p) { delete (SoloRowsDebug *)p; }

extern "C" int smolmc_create(const smolmc_tables *t, const smolmc_config *cfg, smolmc_handle **out) {
    if (!t || !cfg || !out) return fail("null argument");
    if (cfg->n_replicas <= 0) return fail("n_replicas must be positive");
    if (int rc = validate_tables(t)) return rc; // (in the caller's numbering, before anything is renamed)
    std::vector<int32_t> new_of = plan_relabelling(t);
    if (new_of.empty()) return create_impl(t, cfg, out, nullptr);
    std::vector<int32_t> old_of(new_of.size());
    for (size_t p = 0; p < new_of.size(); ++p) old_of[new_of[p]] = (int32_t)p;
    RelabelledTables rt;
    relabel_tables(t, new_of, old_of, rt);
    return create_impl(&rt.t, cfg, out, &new_of); // (the engine copies every table at create: rt may go)
}

// ---- smolmc_create stage by stage.  Every stage returns 0 or the code of its fail(); create_impl lists them in
// order and destroys the handle when one refuses.
// Wang-Landau keeps per-bin feature sums at update_period 1, running means otherwise
static int wl_sum_mode_of(const smolmc_handle *h) { return (h->cfg.wl_update_period == 1 && !smolmc_env(ENV_WL_RUNNING_MEAN)) ? 1 : 0; }
static int cu_count(const smolmc_handle *h) {
    int cus = 0;
    return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess ? cus : 256;
}
// ln(k) for k <= top from the host libm (the oracle's log-factorial sums use the same); cell 0 is 0
static std::vector<double> ln_table(int top) {
    std::vector<double> ln((size_t)top + 1, 0.0);
    for (int k = 1; k <= top; ++k) ln[k] = std::log((double)k);
    return ln;
}

// dimensions, natural parameters and the Wang-Landau window
static int create_dimensions(smolmc_handle *h, const smolmc_tables *t) {
    const smolmc_config *cfg = &h->cfg;
    h->R = cfg->n_replicas;
    h->N = t->num_sites;
    h->Npad = (t->num_sites + 15) / 16 * 16;
    h->Fce = num_ce_features(t);
    h->F = h->Fce + (t->has_ewald ? 1 : 0) + (t->has_mu ? 1 : 0);
    h->natural.assign(t->ce_coefs, t->ce_coefs + h->Fce);
    if (t->has_ewald) h->natural.push_back(t->ewald_coef);
    if (t->has_mu) h->natural.push_back(-1.0);
    if (is_wl(h)) {
        if (cfg->wl_min_enthalpy > cfg->wl_max_enthalpy)
            return fail("min_enthalpy can not be larger than max_enthalpy."); // wanglandau.py:82
        if ((cfg->wl_max_enthalpy - cfg->wl_min_enthalpy) / cfg->wl_bin_size <= 1)
            return fail("The values provided for min and max enthalpy and bin sizer result in a "
                        "single bin!");
        if (cfg->wl_mod_factor <= 0) return fail("mod_factor must be greater than 0.");
        h->L = (int)ceil((cfg->wl_max_enthalpy - cfg->wl_min_enthalpy) / cfg->wl_bin_size);
    }
    memset(&h->kp, 0, sizeof(KParams));
    return 0;
}

// (validate_tables(t) has passed: smolmc_create runs it on the caller's tables before any renaming)
// species codes a site may carry: max_species by default, the largest sublattice code + 1 on
// the sites of an active sublattice
static int create_site_codes(smolmc_handle *h, const smolmc_tables *t) {
    h->site_ncodes.assign((size_t)t->num_sites, (uint8_t)std::min(255, std::max(1, t->max_species)));
    h->site_active.assign((size_t)t->num_sites, 0);
    for (int k = 0; k < t->n_sublattices; ++k) {
        int top = 0;
        for (int64_t c = t->sub_code_ptr[k]; c < t->sub_code_ptr[k + 1]; ++c) top = std::max(top, t->sub_codes[c]);
        for (int64_t i = t->sub_site_ptr[k]; i < t->sub_site_ptr[k + 1]; ++i) {
            const int st = t->sub_active_sites[i];
            if (st >= 0 && st < t->num_sites) {
                h->site_ncodes[st] = (uint8_t)std::min(255, top + 1);
                h->site_active[st] = 1;
            }
        }
    }
    // ... and on every other site the width of its site space as the cluster tensors see it: member m of
    // an orbit's rows has prev_stride / stride species (see validate_tables); a code beyond that would
    // index past the tensors
    std::vector<int> seen((size_t)t->num_sites, 0);
    for (int o = 0; o < t->n_orb; ++o) {
        const int I = t->orb_nsites[o];
        for (int64_t i = t->full_off[o]; i < t->full_off[o + 1]; ++i) {
            const int width = member_species(t, o, (int)((i - t->full_off[o]) % I));
            const int site = t->full_idx[i];
            seen[site] = seen[site] ? std::min(seen[site], width) : width;
        }
    }
    for (int s = 0; s < t->num_sites; ++s)
        if (!h->site_active[s] && seen[s]) h->site_ncodes[s] = (uint8_t)std::min<int>(h->site_ncodes[s], std::min(255, seen[s]));
    h->site_width_known.assign((size_t)t->num_sites, 0);
    for (int s = 0; s < t->num_sites; ++s) h->site_width_known[s] = h->site_active[s] || seen[s];
    return 0;
}

// the model's part of mc_kernel's parameter block (the tables are in h->rt by now)
static int create_model_params(smolmc_handle *h, const smolmc_tables *t) {
    KParams &kp = h->kp;
    kp.N = h->N;
    kp.Npad = h->Npad;
    kp.Fce = h->Fce;
    kp.F = h->F;
    kp.step_type = h->cfg.step_type;
    kp.corr_mode = h->rt.corr_mode;
    kp.has_ewald = t->has_ewald;
    kp.has_mu = t->has_mu;
    kp.ew_W = h->rt.ew_W;
    kp.ew_M = h->rt.ew_M;
    kp.mu_W = h->rt.mu_W;
    kp.ew_inds = h->rt.ew_inds;
    kp.ew_Mt = h->rt.ew_Mt;
    kp.ew_coef = t->ewald_coef;
    kp.mu = h->rt.mu;
    return 0;
}

// MCBias (smol/moca/kernel/bias.py)
static int create_bias(smolmc_handle *h, const smolmc_tables *t) {
    if (!t->bias_type) return 0;
    const smolmc_config *cfg = &h->cfg;
    KParams &kp = h->kp;
    if (t->bias_type != SMOLMC_BIAS_FUGACITY && t->bias_type != SMOLMC_BIAS_SQUARE_CHARGE &&
        t->bias_type != SMOLMC_BIAS_SQUARE_HYPERPLANE)
        return fail("unknown bias_type");
    const int brows = t->bias_type == SMOLMC_BIAS_SQUARE_HYPERPLANE ? t->bias_rows : 1;
    if (brows < 1 || brows > SMOLMC_MAX_BIAS_ROWS)
        return fail("bias_rows must be in [1, SMOLMC_MAX_BIAS_ROWS]");
    if (is_wl(h)) return fail("Cannot apply bias to Wang-Landau simulation!"); // wanglandau.py:127-128
    if (!t->bias_table || t->bias_width < t->max_species)
        return fail("bias_table must be [num_sites x >= max_species]");
    if (t->bias_type != SMOLMC_BIAS_FUGACITY && !(t->bias_penalty > 0.0))
        return fail("Penalty factor should be > 0!"); // bias.py:250-251, :328-329
    h->bias_host.assign(t->bias_table, t->bias_table + (size_t)brows * t->num_sites * t->bias_width);
    h->bias_icpt.assign(SMOLMC_MAX_BIAS_ROWS, 0.0);
    if (t->bias_type == SMOLMC_BIAS_SQUARE_HYPERPLANE && t->bias_intercepts)
        for (int k = 0; k < brows; ++k) h->bias_icpt[k] = t->bias_intercepts[k];
    kp.bias_rows = brows;
    kp.bias_row_stride = (size_t)t->num_sites * t->bias_width;
    if (t->bias_type == SMOLMC_BIAS_FUGACITY)
        for (double v : h->bias_host)
            if (!(v > 0.0)) return fail("fugacity fractions must be positive");
    kp.bias_type = t->bias_type;
    kp.bias_W = t->bias_width;
    kp.bias_pen = t->bias_penalty;
    if (dev_upload(h, h->bias_host.data(), h->bias_host.size(), &kp.bias_tab)) return 1;
    if (dev_alloc(h, (size_t)cfg->n_replicas, &kp.bias) ||
        dev_alloc(h, (size_t)cfg->n_replicas * SMOLMC_MAX_BIAS_ROWS, &kp.charge))
        return 1;
    return 0;
}

// compact Ewald form and the potential field of every walker in HBM: the field needs the compact form
// and contiguous changeable sites; the lean kernels stage the same buffer through LDS
static int create_ewald_field(smolmc_handle *h, const smolmc_tables *t) {
    KParams &kp = h->kp;
    if (t->has_ewald && t->ewald_charges && !smolmc_env(ENV_DENSE_EWALD))
        if (int rc = build_compact_ewald(h, t)) return rc;
    kp.ew_field = 0;
    if (kp.ew_compact && kp.ew_act_base >= 0 && (size_t)kp.ew_nact * 8 <= 150 * 1024 &&
        !smolmc_env(ENV_NO_EWALD_FIELD)) {
        if (dev_alloc(h, (size_t)h->cfg.n_replicas * kp.ew_nact, &kp.ew_phi)) return 1;
        kp.ew_field = 1;
    }
    return 0;
}

// the active sites of sublattice k are one site range
static bool lean_site_range(const smolmc_tables *t, int k) {
    const int64_t a0 = t->sub_site_ptr[k], a1 = t->sub_site_ptr[k + 1];
    for (int64_t i = a0; i < a1; ++i)
        if (t->sub_active_sites[i] != t->sub_active_sites[a0] + (int)(i - a0)) return false;
    return true;
}
static int create_sublattices(smolmc_handle *h, const smolmc_tables *t) {
    KParams &kp = h->kp;
    const int ns = t->n_sublattices;
    if (ns <= 0) return fail("no active sublattice");
    std::vector<int> ptr(ns + 1), cptr(ns + 1), base(ns);
    std::vector<double> cum(ns);
    double c = 0;
    for (int s = 0; s <= ns; ++s) {
        ptr[s] = (int)t->sub_site_ptr[s];
        cptr[s] = (int)t->sub_code_ptr[s];
    }
    for (int s = 0; s < ns; ++s) {
        c += t->sub_probs[s];
        cum[s] = c;
        const int a = ptr[s], b = ptr[s + 1];
        if (b <= a) return fail("empty active sublattice");
        base[s] = lean_site_range(t, s) ? t->sub_active_sites[a] : -1;
        for (int i = a; i < b; ++i)
            if (t->sub_active_sites[i] < 0 || t->sub_active_sites[i] >= t->num_sites)
                return fail("sublattice site index out of range");
    }
    kp.nsub = ns;
    if (dev_upload(h, ptr.data(), ptr.size(), &kp.sub_ptr) ||
        dev_upload(h, t->sub_active_sites, (size_t)ptr[ns], &kp.sub_sites) ||
        dev_upload(h, base.data(), base.size(), &kp.sub_base) ||
        dev_upload(h, cptr.data(), cptr.size(), &kp.sub_code_ptr) ||
        dev_upload(h, t->sub_codes, (size_t)cptr[ns], &kp.sub_codes) ||
        dev_upload(h, cum.data(), cum.size(), &kp.sub_cum))
        return 1;
    return 0;
}

static int create_walker_state(smolmc_handle *h, const smolmc_tables *) {
    KParams &kp = h->kp;
    const size_t R = h->R;
    kp.R = h->R;
    double *dbeta = nullptr;
    uint64_t *dseeds = nullptr;
    if (dev_alloc(h, R * h->Npad, &kp.occ) || dev_alloc(h, R, &kp.enthalpy) ||
        dev_alloc(h, R * h->F, &kp.features) || dev_alloc(h, R, &dbeta) || dev_alloc(h, R, &dseeds) ||
        dev_alloc(h, R, &kp.nsteps) || dev_alloc(h, R, &kp.nacc) || dev_alloc(h, R, &kp.last_acc))
        return 1;
    kp.beta = dbeta;
    h->d_beta = dbeta;
    kp.seeds = dseeds;
    if (dev_upload(h, h->natural.data(), h->natural.size(), (const double **)&h->d_natural))
        return 1;
    return 0;
}

static int create_wl_state(smolmc_handle *h, const smolmc_tables *) {
    if (!is_wl(h)) return 0;
    const smolmc_config *cfg = &h->cfg;
    KParams &kp = h->kp;
    const size_t R = h->R;
    kp.L = h->L;
    kp.wl_min = cfg->wl_min_enthalpy;
    kp.wl_max = cfg->wl_max_enthalpy;
    kp.wl_bin = cfg->wl_bin_size;
    kp.wl_flat = cfg->wl_flatness;
    kp.wl_div = cfg->wl_mod_divisor;
    kp.wl_check = cfg->wl_check_period;
    kp.wl_update = cfg->wl_update_period;
    kp.wl_sum_mode = wl_sum_mode_of(h);
    // (check period 0: the flatness check is the caller's -- a host-side mod_update callable,
    // wanglandau.py:100-105 -- and no kernel runs its own)
    if (kp.wl_check < 0 || kp.wl_update <= 0) return fail("WL periods must be positive");
    // (the lane-indexed feature bookkeeping of mc_kernel / mc_wl_kernel holds 64 features; more -- the
    // reference has no limit, wanglandau.py:117-118 -- take the universal kernel)
    if (h->F > 64 && h->general_ok) no_general(h, "Wang-Landau with more than 64 features");
    if (dev_alloc(h, R * h->L, &kp.wl_entropy) || dev_alloc(h, R * h->L, &kp.wl_hist) ||
        dev_alloc(h, R * h->L, &kp.wl_occur) || dev_alloc(h, R * h->L * h->F + 64, &kp.wl_meanf) || // (+64: the lean kernel's all-lane atomic, see mc_lean.h)
        // (m heads one arena: behind it the walkers' window records and the estimator -> walker map, smolmc_set_wl_windows)
        dev_alloc(h, R + (R * sizeof(WlWindow) + R * 4 + 7) / 8, &kp.wl_m) || dev_alloc(h, R, &kp.wl_counter))
        return 1;
    h->d_wl_win = (WlWindow *)(kp.wl_m + R);
    h->d_wl_walker_at = (int32_t *)(h->d_wl_win + R);
    std::vector<double> m0(R, cfg->wl_mod_factor);
    if (hipMemcpy(kp.wl_m, m0.data(), R * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMemcpy failed");
    return 0;
}

// LDS layout of mc_kernel
static int create_general_layout(smolmc_handle *h, const smolmc_tables *) {
    KParams &kp = h->kp;
    size_t tb = (size_t)kp.nclasses * kp.Cpad * (16 + 16 + 8) + (size_t)(kp.xt_len + kp.ft_len) * 8 +
                (size_t)((kp.nclasses + 3) & ~3) * 4 + (kp.nclasses > 1 ? (size_t)h->N : 0);
    tb = (tb + 15) / 16 * 16;
    size_t pw = (size_t)h->Npad;
    if (is_wl(h))
        pw += (size_t)h->L * 24 + (size_t)h->F * 8;
    else {
        const size_t by_feat = (size_t)h->Fce * 64 * 8;
        const size_t by_slot = ((size_t)kp.nclasses * kp.Cpad + h->Fce) * 8;
        kp.acc_by_slot = (!kp.corr_mode && by_slot < by_feat) ? 1 : 0;
        pw += kp.acc_by_slot ? by_slot : by_feat;
    }
    pw = (pw + 15) / 16 * 16;
    kp.lds_tables = (int)tb;
    kp.lds_per_wave = (int)pw;
    h->waves_per_block = 4;
    while (h->waves_per_block > 1 && tb + pw * h->waves_per_block > 160 * 1024) h->waves_per_block /= 2;
    h->lds_bytes = tb + pw * h->waves_per_block;
    if (h->general_ok && h->lds_bytes > 160 * 1024)
        no_general(h, "tables + one chain exceed the 160 KiB LDS budget of mc_kernel");
    return 0;
}

// ---- the lean planners (everything they leave runs mc_kernel or the universal kernel).  Each first decides --
// host arithmetic on the tables, the config, what the earlier stages left on the handle and the CU count -- and
// only a planner that has said yes fills h->lp and uploads: a handle's LeanParams is written by one planner.

// features the lean kernels carry (lazy cluster features: the scalar ones only -- Ewald energy, chemical work)
static int lean_features(const smolmc_handle *h, const smolmc_tables *t) { return h->lazy_tables ? (t->has_ewald ? 1 : 0) + (t->has_mu ? 1 : 0) : h->F; }
static const char *const lean_why_species = "an active sublattice of fewer than 2 or more than 8 species";
static const char *const lean_why_codes = "a sublattice whose species codes are not 0 .. n-1 (split by species) under a step type that draws codes";
// Species codes of sublattice k: 0 .. n-1, or -- canonical swaps only, which never draw a code: they exchange the
// two sites' own -- any code list (a sublattice split by species, sublattice.py:109-186, keeps the site space's
// codes: {1, 2} of three); the per-code rows (mu, charges, bias pairs) then run up to the largest code.
// -> the number of codes those rows hold, or 0 with the reason in *why
static int lean_code_count(const smolmc_handle *h, const smolmc_tables *t, int k, const char **why) {
    const int32_t *codes = t->sub_codes + t->sub_code_ptr[k];
    const int nc = (int)(t->sub_code_ptr[k + 1] - t->sub_code_ptr[k]);
    bool default_codes = true;
    int top = 0;
    for (int c = 0; c < nc; ++c) {
        default_codes = default_codes && codes[c] == c;
        top = std::max(top, (int)codes[c]);
    }
    *why = (nc < 2 || nc > 8) ? lean_why_species : (!default_codes && !(h->cfg.step_type == SMOLMC_STEP_SWAP && top < 8)) ? lean_why_codes : nullptr;
    return *why ? 0 : (default_codes ? nc : top + 1);
}
// the first ncol columns of a per-site table [site][width] are the same on the n sites from site0 on
static bool row_uniform(const double *tab, int width, int site0, int n, int ncol) {
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < ncol; ++c)
            if (tab[(size_t)(site0 + i) * width + c] != tab[(size_t)site0 * width + c]) return false;
    return true;
}
// Bias pair tables of one sublattice (sites sb .. sb + na - 1, nc codes): pairs[row * row_stride + old * 8 + new].
// false: a bias row differs between its sites (the bias is defined per sublattice)
static bool lean_bias_pairs(const smolmc_handle *h, const smolmc_tables *t, int brows, int sb, int na, int nc, double *pairs, size_t row_stride) {
    const int W = t->bias_width;
    for (int rw = 0; rw < brows; ++rw) {
        const double *tabk = h->bias_host.data() + (size_t)rw * t->num_sites * W;
        if (!row_uniform(tabk, W, sb, na, nc)) return false;
        for (int o = 0; o < nc; ++o)
            for (int n = 0; n < nc; ++n) {
                const double a = tabk[(size_t)sb * W + n], b = tabk[(size_t)sb * W + o];
                pairs[(size_t)rw * row_stride + o * 8 + n] = t->bias_type == SMOLMC_BIAS_FUGACITY ? std::log(a / b) : a - b;
            }
    }
    return true;
}
// Charge / diagonal term per species code of the n sites from sb on (8 cells each): false when they depend on the site
static bool lean_ewald_rows(const smolmc_handle *h, int sb, int n, double *q, double *dg) {
    const int W = h->kp.ew_W;
    if (W > 8 || !row_uniform(h->ew_qs_host.data(), W, sb, n, W) || !row_uniform(h->ew_dg_host.data(), W, sb, n, W)) return false;
    std::copy_n(&h->ew_qs_host[(size_t)sb * W], W, q);
    std::copy_n(&h->ew_dg_host[(size_t)sb * W], W, dg);
    return true;
}
// the mu delta of a step joins the float32 sum (<= 2 flips * 2 |mu|): mmax = the largest |mu| of the rows in use
static void lean_widen_fast_eps(int has_mu, LeanParams &lp, double mmax) {
    if (has_mu) lp.fast_eps += 4.0 * mmax * ldexp(1.0, -19);
    // test hook: widen the undecided band so that both decision paths interleave
    if (const char *sc = smolmc_env(ENV_FAST_EPS_SCALE)) lp.fast_eps *= atof(sc);
}
// The bound of the handle for rows whose largest |mu| is mmax, from the un-widened one kept on the handle: at create
// with the table's rows, at every smolmc_set_walker_mu with the maximum over ALL walkers' rows (a stale bound would
// make about one decision in 1e5 wrong, which no test finds by chance: smolmc_kernel_info prints mu_max)
static void lean_set_fast_eps(smolmc_handle *h, double mmax) {
    h->lp.fast_eps = h->fast_eps_plain;
    for (int i = 0; i < h->fast_eps_widenings; ++i) lean_widen_fast_eps(h->rt.has_mu, h->lp, mmax);
    h->mu_max = mmax;
}
// the walker state, the bias and the Wang-Landau block of LeanParams (pointers and dimensions of mc_kernel's)
static void lean_fill_state(const smolmc_handle *h, const smolmc_tables *t, LeanParams &lp, int bias_row_stride, int wl_sums) {
    const KParams &kp = h->kp;
    lp.occ = kp.occ; lp.enthalpy = kp.enthalpy; lp.features = h->lazy_tables ? h->d_lazy_scal : kp.features; lp.beta = kp.beta;
    lp.seeds = kp.seeds; lp.nsteps = kp.nsteps; lp.nacc = kp.nacc; lp.last_acc = kp.last_acc;
    lp.R = h->R; lp.N = h->N; lp.Npad = h->Npad; lp.F = lean_features(h, t); lp.Fce = h->lazy_tables ? 0 : h->Fce;
    if (t->has_ewald) {
        lp.ew_W = kp.ew_W; lp.ew_nact = kp.ew_nact; lp.ew_act_base = kp.ew_act_base;
        lp.ew_G = kp.ew_G; lp.ew_coef = kp.ew_coef;
        lp.ew_gx = kp.ew_gx; lp.ew_E8 = kp.ew_E8; lp.ew_S8 = kp.ew_S8;
    }
    if (t->bias_type) {
        lp.bias_type = t->bias_type;
        lp.bias_pen = t->bias_penalty;
        lp.bias = kp.bias;
        lp.charge = kp.charge;
        lp.bias_rows = kp.bias_rows;
        lp.bias_row_stride = bias_row_stride;
    }
    if (is_wl(h)) {
        lp.wl.L = h->L;
        lp.wl.vmin = kp.wl_min; lp.wl.vmax = kp.wl_max; lp.wl.bin = kp.wl_bin;
        lp.wl.flat = kp.wl_flat; lp.wl.div = kp.wl_div;
        lp.wl.check = kp.wl_check; lp.wl.update = kp.wl_update;
        lp.wl.entropy = kp.wl_entropy; lp.wl.hist = kp.wl_hist; lp.wl.occur = kp.wl_occur;
        lp.wl.meanf = kp.wl_meanf; lp.wl.m = kp.wl_m; lp.wl.counter = kp.wl_counter;
        lp.wl.sum_mode = wl_sums;
    }
}
// the flip table of a TableFlip handle (dims columns), its weights and ln(k) for k <= ln_top
static int lean_fill_table(smolmc_handle *h, const smolmc_tables *t, LeanParams &lp, int dims, int ln_top, int ln_len) {
    const std::vector<double> ln = ln_table(ln_top);
    if (dev_upload(h, t->flip_table, (size_t)t->n_flip_vectors * dims, &lp.tf_table) ||
        dev_upload(h, t->flip_weights, (size_t)2 * t->n_flip_vectors, &lp.tf_w) ||
        dev_upload(h, ln.data(), ln.size(), &lp.tf_ln))
        return 1;
    lp.tf_n = t->n_flip_vectors;
    lp.tf_sw = t->swap_weight;
    lp.tf_ln_len = ln_len; // cells of tf_ln the kernel keeps in LDS
    return 0;
}

// ---- one site class, one contiguous sublattice: mc_lean_kernel, mc_wl_kernel, mc_table_kernel
struct LeanPlan {
    bool take = false;
    bool late = false;  // refused after the early checks, at the LDS stage (see plan_lean_multi: fast_eps)
    int sbase = -1, nact = 0, nc = 0;
    std::vector<double> mu_row, bias_pair, qrow, dgrow;
    bool field = false; // potential field in LDS
    bool solo = false;
    int occ = 0, wpb = 4, tf_ln_len = 0;
    size_t lds = 0, lds8 = 0;
    SoloRowsPlan rows;  // solo: the rows variant, where the site's clusters fall into one of its shapes
};
static LeanPlan decide_lean(const smolmc_handle *h, const smolmc_tables *t) {
    const smolmc_config *cfg = &h->cfg;
    const KParams &kp = h->kp;
    const LeanParams &lp = h->lp; // (commit_lean_tables has left the table sizes there)
    const bool wl = is_wl(h), table = is_table(h);
    const int wl_sum_mode = wl_sum_mode_of(h), Fk = lean_features(h, t), brows = kp.bias_rows;
    LeanPlan p;
    // (lean Wang-Landau keeps per-bin feature SUMS: update_period 1 only, see WlParams)
    // (... the Wang-Landau TableFlip kernel, mc_table_kernel<..., WLT>, also keeps running means: any update_period)
    const bool table_wl = wl && table;
    const bool lean = h->lean_tables && Fk <= 64 &&
                (!wl || ((wl_sum_mode || (table_wl && cfg->wl_update_period < (1ll << 31))) &&
                         h->F <= 63 && cfg->wl_check_period < (1ll << 31))) && // (cell 63 of the feature scratch is the kernel's zero)
                (!t->has_ewald || kp.ew_compact) && t->n_sublattices == 1 && h->lean_ncls == 1 &&
                h->lean_nslot <= 4 && !smolmc_env(ENV_FORCE_GENERAL);
    if (!lean) return p;
    const int nact = p.nact = (int)(t->sub_site_ptr[1] - t->sub_site_ptr[0]);
    const int sbase = p.sbase = t->sub_active_sites[0];
    const char *why = nullptr;
    const int nc = p.nc = lean_code_count(h, t, 0, &why);
    if (!lean_site_range(t, 0) || !nc) return p;
    if (t->has_mu) {
        if (t->mu_width < nc || !row_uniform(t->mu_table, t->mu_width, sbase, nact, nc)) return p;
        p.mu_row.assign(t->mu_table + (size_t)sbase * t->mu_width, t->mu_table + (size_t)sbase * t->mu_width + nc);
    }
    // the table kernels take at most 8 flip vectors: larger tables run on the universal kernel
    // (Wang-Landau TableFlip: mc_table_kernel<..., WLT>; SMOLMC_NO_TABLE_WL: A/B switch)
    if (table && (t->n_flip_vectors > 8 || (wl && smolmc_env(ENV_NO_TABLE_WL)))) return p;
    // several correlation functions per orbit: plain Metropolis flip / swap variants only
    if (h->lean_kf && (wl || t->bias_type || table)) return p;
    if (t->bias_type) {
        // (pair tables of the bias: [row][old * 8 + new]; the bias row must be the same on every active site)
        p.bias_pair.assign((size_t)64 * SMOLMC_MAX_BIAS_ROWS, 0.0);
        if (!lean_bias_pairs(h, t, brows, sbase, nact, nc, p.bias_pair.data(), 64)) return p;
        // (TableFlip with a bias: mc_table_kernel<..., BIAS>; SMOLMC_NO_TABLE_BIAS: A/B switch)
        if (table && smolmc_env(ENV_NO_TABLE_BIAS)) return p;
    }
    p.late = true;
    // (Wang-Landau: per-bin records and the cached rows of per-bin feature sums, mc_wl.h)
    p.lds = ((size_t)lp.dt_len + 24) * 8 +
            (size_t)4 * (lp.Nlds + 64 * 8 + 64 +
                         (table_wl ? wl_multi_wave_bytes(h->L, h->F, kp.wl_sum_mode) // (mc_table_kernel<..., WLT>: the multi-class kernel's state)
                          : wl     ? wl_lean_bins_bytes(h->L) + (size_t)SMOLMC_WL_ROWS * h->F * 8
                                   : 0));
    if (p.lds > 150 * 1024) return p;
    // Ewald potential field in LDS when the changeable sites are the active
    // sublattice and it fits beside the occupancies
    // (the changeable sites may extend beyond the active ones: restricted sites, which the host
    // API relabels behind the active sites of their sublattice; the field covers them all)
    const int nfield = kp.ew_nact;
    if (t->has_ewald && kp.ew_act_base == sbase && nfield >= nact && !smolmc_env(ENV_NO_EWALD_FIELD)) {
        const size_t with_field = p.lds + (size_t)4 * nfield * 8;
        p.qrow.assign(8, 0.0);
        p.dgrow.assign(8, 0.0);
        if (lean_ewald_rows(h, sbase, nfield, p.qrow.data(), p.dgrow.data()) && kp.ew_field && with_field <= 150 * 1024 && (size_t)nfield * 8 <= 64 * 1024) {
            p.field = true;
            p.lds = with_field;
        }
    }
    // Wang-Landau with the Ewald term: mc_wl_kernel takes it from the field in LDS only
    if (wl && t->has_ewald && !p.field) return p;
    p.take = true;
    // one wave per workgroup (occupancy at LDS address 0, 32-bit index rows, a private
    // copy of the tables): Metropolis flips / swaps without Ewald term or bias, when 16
    // such workgroups still fit a CU
    if (!wl && !t->has_ewald && !t->bias_type && !h->lean_kf && !table && !smolmc_env(ENV_NO_SOLO)) {
        const size_t pw = ((size_t)lp.Nlds + 64 * 8 + 15) & ~(size_t)15;
        const size_t solo_lds = pw + ((size_t)lp.dt_len + 24) * 8;
        if (solo_lds * 16 <= 160 * 1024 - 16 * 256) {
            p.solo = true;
            p.lds = solo_lds;
            // More walkers than the default register allocation (4 waves per SIMD) keeps
            // resident: the 6-waves-per-SIMD instantiation, when 24 workgroups fit a CU.
            // Measured (headline model, 1e4 steps): 6144 walkers 8.74 -> 7.08 ms, 16384
            // walkers 19.7 -> 17.6 ms; at <= 4 waves per SIMD it is 7 % slower.
            if ((long)cfg->n_replicas > 16L * cu_count(h) && solo_lds * 24 <= 160 * 1024 - 24 * 256 &&
                !smolmc_env(ENV_NO_OCC6))
                p.occ = 6;
            // (SMOLMC_NO_SOLO_ROWS: A/B switch, keeps the handle on the plain solo kernel)
            if (!smolmc_env(ENV_NO_SOLO_ROWS))
                p.rows = solo_rows_plan(h->lean_idx_host, h->lean_slots_host.data(), t->num_sites, h->lean_nslot, h->lean_mm,
                                        Swizzle{lp.swz_a, lp.swz_m, lp.swz_b, lp.Nlds});
        }
    }
    if (table) {
        // block-shared flip table / weights (48 doubles) and, when it fits, ln(k) for k <= n_active
        p.lds += 48 * 8;
        // ... unless it would cost the second resident workgroup per CU (160 KiB / 2)
        const size_t half = 80 * 1024, with_ln = p.lds + (size_t)(nact + 1) * 8;
        if (with_ln <= 150 * 1024 && (with_ln <= half || p.lds > half)) {
            p.tf_ln_len = nact + 1;
            p.lds += (size_t)(nact + 1) * 8;
        }
        // Eight walkers per workgroup when two four-walker workgroups would share a CU
        // anyway: waves w and w + 4 of a workgroup sit on the same SIMD, so that the
        // launch order (update_walker_order) can pair a hot walker with a cold one there.
        // (fewer walkers than 8 per CU: four-walker workgroups spread over more CUs)
        const size_t per_wave = (size_t)lp.Nlds + 64 * 8 + 64 + (p.field ? (size_t)kp.ew_nact * 8 : 0);
        const size_t lds8 = p.lds + 4 * per_wave;
        if (!wl && lds8 <= 160 * 1024 && p.lds > 40 * 1024 && cfg->n_replicas % 8 == 0 &&
            (long)cfg->n_replicas >= 8L * cu_count(h)) {
            p.wpb = 8;
            p.lds8 = lds8;
        }
    }
    return p;
}
static int plan_lean(smolmc_handle *h, const smolmc_tables *t, LeanPlan &p) {
    if (h->lazy_tables && dev_alloc(h, (size_t)h->R * 2, &h->d_lazy_scal)) return 1; // (for either planner's kernels)
    p = decide_lean(h, t);
    if (!p.take) return 0;
    const KParams &kp = h->kp;
    LeanParams &lp = h->lp;
    p.mu_row.resize(8, 0.0); // (a whole cell: the re-pricing of per-walker rows reads all eight)
    if (t->has_mu && dev_upload(h, p.mu_row.data(), p.mu_row.size(), &lp.mu_row)) return 1;
    if (t->bias_type && dev_upload(h, p.bias_pair.data(), p.bias_pair.size(), &lp.bias_pair)) return 1;
    double mmax = 0.0;
    for (double v : p.mu_row) mmax = std::max(mmax, std::fabs(v));
    h->fast_eps_plain = lp.fast_eps; h->fast_eps_widenings = 1; h->mu_max_create = mmax; h->d_mu_create = lp.mu_row;
    lean_set_fast_eps(h, mmax);
    lean_fill_state(h, t, lp, 64, is_table(h) ? kp.wl_sum_mode : 1);
    lp.sbase = p.sbase; lp.nact = p.nact; lp.ncodes = p.nc;
    if (t->has_ewald) { lp.ew_act = kp.ew_act; lp.ew_qs = kp.ew_qs; lp.ew_dg = kp.ew_dg; lp.ew_frozen = kp.ew_frozen; }
    lp.ew_field = 0;
    if (p.field) {
        if (dev_upload(h, p.qrow.data(), 8, &lp.ew_qrow) || dev_upload(h, p.dgrow.data(), 8, &lp.ew_dgrow)) return 1;
        lp.ew_phi = kp.ew_phi;
        lp.ew_field = 1;
    }
    if (p.solo) {
        std::vector<uint32_t> wide(h->lean_idx_host.begin(), h->lean_idx_host.end());
        if (dev_upload(h, wide.data(), wide.size(), &lp.idx32)) return 1;
        if (p.rows.shape && (dev_upload(h, p.rows.rows.data(), p.rows.rows.size(), &h->d_rows_idx32) ||
                             dev_upload(h, p.rows.slots.data(), p.rows.slots.size(), &h->d_rows_slots)))
            return 1;
    }
    if (is_table(h) && lean_fill_table(h, t, lp, p.nc, p.nact, p.tf_ln_len)) return 1;
    h->lean_lds = p.lds;
    h->lean_solo = p.solo;
    h->lean_occ = p.occ;
    h->solo_rows = p.solo ? p.rows.shape : 0;
    h->lean_wpb = p.wpb;
    h->lean_lds_wpb8 = p.lds8;
    return 0;
}

// ---- several classes / sublattices (or > 256 clusters per site): mc_lean_multi_kernel, mc_table_multi_kernel
struct LeanMultiPlan {
    bool take = false;
    std::string reason; // why not (the first condition that fails, for smolmc_kernel_info)
    int sbase[4], nact[4], ncodes[4], cls[4];
    double cum[4], mmax = 0.0;
    std::vector<double> mu_rows, q_rows, dg_rows, bias_pairs;
    int ndims = 0, max_nact = 0, wpb = 0;
    bool phi_lds = false;
    size_t lds = 0;
};
static LeanMultiPlan decide_lean_multi(const smolmc_handle *h, const smolmc_tables *t) {
    const smolmc_config *cfg = &h->cfg;
    const KParams &kp = h->kp;
    const LeanParams &lp = h->lp; // (commit_lean_tables has left the table sizes there)
    const bool wl = is_wl(h), table = is_table(h);
    const int wl_sum_mode = wl_sum_mode_of(h), Fk = lean_features(h, t), brows = kp.bias_rows;
    LeanMultiPlan p;
    // (MCBias: every bias type with flips or swaps, and with TableFlip: mc_table_multi_kernel<..., BIAS>;
    // SMOLMC_NO_TABLE_BIAS: A/B switch)
    const bool multi_bias_ok = !t->bias_type || !table || !smolmc_env(ENV_NO_TABLE_BIAS);
    // Wang-Landau on this layout (mc_lean_multi_kernel<..., WLK>): any number of classes the
    // layout takes and any update_period -- what mc_wl_kernel (one class, update_period 1) leaves.  The
    // Wang-Landau TableFlip: mc_table_multi_kernel<..., WLT> with one correlation function per orbit, the
    // universal kernel otherwise.  SMOLMC_NO_WL_MULTI, SMOLMC_NO_TABLE_WL: A/B switches.
    const bool multi_table_wl_ok = !h->lean_kf && !smolmc_env(ENV_NO_TABLE_WL);
    const bool multi_wl_ok = !wl || ((!table || multi_table_wl_ok) && h->F <= 63 && cfg->wl_check_period < (1ll << 31) &&
                                     cfg->wl_update_period < (1ll << 31) && !smolmc_env(ENV_NO_WL_MULTI));
    const bool multi_env_off = smolmc_env(ENV_FORCE_GENERAL) || smolmc_env(ENV_NO_LEAN_MULTI);
    p.reason = (h->lean_kf && !wl) ? "several correlation functions per orbit (KF kernel) on a model outside the single-class lean shape"
               : !multi_wl_ok ? "Wang-Landau with more than 63 features, or with TableFlip and several correlation functions per orbit"
               : !multi_bias_ok ? "environment override (SMOLMC_NO_TABLE_BIAS)"
               : Fk > 64 ? "more than 64 features"
               : t->n_sublattices > 4 ? "more than 4 active sublattices"
               : (t->has_ewald && !kp.ew_field) ? "Ewald matrix that does not factorise into site charges (no potential field)"
               : multi_env_off ? "environment override" : "";
    if (!((!h->lean_kf || wl) && multi_wl_ok && multi_bias_ok && Fk <= 64 && t->n_sublattices <= 4 && (!t->has_ewald || kp.ew_field) &&
          !multi_env_off))
        return p;
    const int ns = t->n_sublattices;
    bool ok = true;
    auto no = [&](const char *why) { if (ok) p.reason = why; ok = false; };
    p.mu_rows.assign(32, 0.0);
    p.q_rows.assign(32, 0.0);
    p.dg_rows.assign(32, 0.0);
    p.bias_pairs.assign((size_t)256 * SMOLMC_MAX_BIAS_ROWS, 0.0);
    double cum = 0.0;
    for (int k = 0; k < ns && ok; ++k) {
        const int na = (int)(t->sub_site_ptr[k + 1] - t->sub_site_ptr[k]);
        const int sb = t->sub_active_sites[t->sub_site_ptr[k]];
        const char *why = nullptr; // (codes other than 0 .. n-1 under canonical swaps only: lean_code_count)
        const int ncod = lean_code_count(h, t, k, &why);
        if (na <= 0 || why == lean_why_species) no(lean_why_species);
        if (ok && !lean_site_range(t, k)) no("the active sites of a sublattice are not one site range (they could not be renumbered into one, or SMOLMC_NO_SITE_RELABEL)");
        if (ok && why) no(why);
        const int cls = ok ? h->site_class_host[sb] : 255;
        if (ok && cls == 255) no("an active sublattice without clusters");
        for (int i = 0; ok && i < na; ++i)
            if (h->site_class_host[sb + i] != cls) no("sites of one sublattice in different site classes (cluster environments)"); // classes == sublattices
        if (!ok) break;
        p.sbase[k] = sb; p.nact[k] = na; p.ncodes[k] = ncod; p.cls[k] = cls;
        cum += t->sub_probs[k];
        p.cum[k] = cum;
        if (t->has_mu) {
            if (t->mu_width < ncod || !row_uniform(t->mu_table, t->mu_width, sb, na, ncod)) ok = false;
            for (int c = 0; ok && c < ncod; ++c) {
                const double v = p.mu_rows[k * 8 + c] = t->mu_table[(size_t)sb * t->mu_width + c];
                p.mmax = std::max(p.mmax, std::fabs(v));
            }
        }
        // one bias row per sublattice (rows of a hyperplane bias: [row][sublattice][old * 8 + new])
        if (t->bias_type && (t->bias_width < ncod || !lean_bias_pairs(h, t, brows, sb, na, ncod, p.bias_pairs.data() + k * 64, 256))) ok = false;
        if (t->has_ewald && (sb < kp.ew_act_base || sb + na > kp.ew_act_base + kp.ew_nact ||
                             !lean_ewald_rows(h, sb, na, &p.q_rows[k * 8], &p.dg_rows[k * 8])))
            ok = false;
    }
    for (int k = 0; k < ns && ok; ++k) { p.ndims += p.ncodes[k]; p.max_nact = std::max(p.max_nact, p.nact[k]); }
    if (table && ok) {
        if (t->n_flip_vectors <= 0 || !t->flip_table || !t->flip_weights) ok = false;
        else if (t->n_flip_vectors > 8 || p.ndims > 16) ok = false;
    }
    // LDS: shared tables + slot records, per wave occupancy + scratch + accumulators (+ field)
    const size_t nrec = (size_t)h->lean_ncls * h->lean_nslot * 64;
    // (Wang-Landau: + feature scale and feature index of every slot record)
    const size_t shared = ((size_t)lp.dt_len + 96 + (table ? 80 : 0)) * 8 + nrec * 24 + (wl ? nrec * 12 : 0);
    // waves per workgroup: the shared tables are paid once per workgroup, so pick the size
    // that keeps the most waves resident per CU (160 KiB of LDS)
    // ... and, at equal residency, the size that spreads the walkers over the most CUs: 1024 walkers in
    // eight-wave workgroups are 128 workgroups -- half the chip idle, two waves per SIMD on the other half
    const int cus = cu_count(h);
    auto layout = [&](size_t per_wave_bytes, int &wpb_out) {
        int best_waves = 0;
        long best_rounds = 0, best_busy = 0;
        wpb_out = 0;
        for (int w : {8, 4, 2, 1}) {
            const size_t need = shared + per_wave_bytes * w;
            if (need > 160 * 1024 - 512) continue;
            const int waves = (int)((160 * 1024) / need) * w;
            const long R_ = cfg->n_replicas, blocks = (R_ + w - 1) / w;
            const long rounds = (R_ + (long)waves * cus - 1) / ((long)waves * cus);
            const long busy = std::min<long>(blocks, cus); // CUs that get a workgroup in the first round
            const bool better = wpb_out == 0 || rounds < best_rounds ||
                                (rounds == best_rounds && (busy > best_busy || (busy == best_busy && waves > best_waves)));
            if (better) { best_waves = waves; best_rounds = rounds; best_busy = busy; wpb_out = w; }
        }
        return best_waves;
    };
    // The potential field goes to LDS while it stays small beside the rest of the wave's
    // state, when all walkers still fit the chip in one round with it there (an accepted
    // flip then reads its G row only, no read-modify-write of phi through L2), or for
    // canonical swaps whenever it fits; else the HBM copy is used in place (ew_field 2).  SMOLMC_MULTI_PHI_HBM / _LDS force either (test hooks).
    // (Wang-Landau: entropies, step counts and cached rows instead of the accumulator cells)
    const size_t base_wave = (size_t)lp.Nlds + 64 + 64 * 8 +
                             (wl ? wl_multi_wave_bytes(h->L, h->F, wl_sum_mode) + (table ? nrec * 8 : 0) // (table: + pending cells)
                                 : nrec * (table ? 16 : 8));
    p.phi_lds = t->has_ewald && (size_t)kp.ew_nact * 8 <= base_wave / 2;
    if (t->has_ewald && !p.phi_lds) {
        int w = 0;
        const int waves = layout(base_wave + (size_t)kp.ew_nact * 8, w);
        // canonical swaps update the field at two sites per accepted step and gain from
        // the LDS copy even when the walkers then need several rounds (LiNiO2 8^3, 4096
        // walkers: 1.13e9 -> 1.58e9 steps/s); flips only while one round holds them all
        // (beyond: 4.1e9 with the HBM field against 3.0e9)
        // -- provided at least 8 waves per CU stay resident: at 3 (config 7, 27 KiB of field
        // per walker) the LDS copy measured 9.6 against 7.4 us per step
        // (Wang-Landau accepts three steps of four: the field update is the step, the LDS copy pays for flips too)
        if ((long)waves * cus >= (long)cfg->n_replicas || ((cfg->step_type == SMOLMC_STEP_SWAP || wl) && waves >= 8) ||
            smolmc_env(ENV_MULTI_PHI_LDS))
            p.phi_lds = waves > 0;
    }
    if (smolmc_env(ENV_MULTI_PHI_HBM)) p.phi_lds = false;
    const size_t per_wave = base_wave + (p.phi_lds ? (size_t)kp.ew_nact * 8 : 0);
    layout(per_wave, p.wpb);
    if (p.wpb == 0 && ok) { ok = false; p.reason = "walker state beyond the workgroup's LDS (multi-class layout)"; }
    if (!ok && p.reason.empty())
        p.reason = "sublattice layout (an active sublattice is not one site range of one class with codes 0..n-1, or per-site "
                   "chemical potentials / bias / charges differ inside a sublattice), or a flip table beyond 8 vectors / 16 dims";
    p.lds = shared + per_wave * p.wpb;
    p.take = ok;
    return p;
}
static int plan_lean_multi(smolmc_handle *h, const smolmc_tables *t, const LeanPlan &one, LeanMultiPlan &p) {
    p = decide_lean_multi(h, t);
    h->lean_reason = p.reason;
    if (!p.take) return 0;
    const KParams &kp = h->kp;
    LeanParams &lp = h->lp;
    const int ns = t->n_sublattices;
    for (int k = 0; k < ns; ++k) {
        lp.m_sbase[k] = p.sbase[k]; lp.m_nact[k] = p.nact[k]; lp.m_ncodes[k] = p.ncodes[k]; lp.m_cls[k] = p.cls[k];
        lp.m_cum[k] = p.cum[k];
    }
    if (t->has_mu && dev_upload(h, p.mu_rows.data(), 32, &lp.m_mu)) return 1;
    if (t->has_ewald &&
        (dev_upload(h, p.q_rows.data(), 32, &lp.m_q) || dev_upload(h, p.dg_rows.data(), 32, &lp.m_dg)))
        return 1;
    if (t->bias_type && dev_upload(h, p.bias_pairs.data(), p.bias_pairs.size(), &lp.bias_pair)) return 1;
    // KEPT FROM EARLIER VERSIONS, bit for bit: a model that the single-class planner refused at its LDS stage had
    // been widened (and scaled) once there before this planner widened it again; NOTES.md lists it for removal
    h->fast_eps_plain = lp.fast_eps; h->fast_eps_widenings = one.late ? 2 : 1; h->mu_max_create = p.mmax; h->d_mu_create = lp.m_mu;
    lean_set_fast_eps(h, p.mmax);
    lp.m_ncls = h->lean_ncls; lp.m_nsub = ns; lp.m_ndims = p.ndims;
    if (is_table(h) && lean_fill_table(h, t, lp, p.ndims, p.max_nact, 0)) return 1;
    lean_fill_state(h, t, lp, 256, wl_sum_mode_of(h));
    lp.ew_field = 0;
    if (t->has_ewald) {
        lp.ew_phi = kp.ew_phi;
        lp.ew_field = p.phi_lds ? 1 : 2;
        lp.sbase = kp.ew_act_base; // field_apply indexes phi relative to it
    }
    h->lean_lds = p.lds;
    h->waves_per_block_lean = p.wpb;
    return 0;
}

// ---- universal kernel (mc_univ.h): parameter block of every handle
// the cluster records (URec) and, packed for the enthalpy pass, the cluster rows of every site (URow / URecE)
static int univ_pack_records(smolmc_handle *h, const smolmc_tables *t) {
    UParams &up = h->up;
    memset(&up, 0, sizeof(up));
    up.T = h->rt;
    up.natural = h->d_natural;
    up.wl = is_wl(h) ? 1 : 0;
    const bool cm = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS;
    const int64_t nloc = t->site_ptr[t->num_sites];
    std::vector<URec> recs((size_t)std::max<int64_t>(nloc, 1));
    memset(recs.data(), 0, recs.size() * sizeof(URec));
    for (int64_t r = 0; r < nloc; ++r) {
        const int o = t->loc_orbit[r];
        URec &u = recs[(size_t)r];
        u.I = t->orb_nsites[o];
        u.K = cm ? t->orb_nfunc[o] : 1;
        u.Nt = t->orb_tensor_len[o];
        u.J = t->loc_nrows[r];
        for (int m = 0; m < u.I; ++m) u.st[m] = t->tensor_indices[t->orb_stride_off[o] + m];
        u.feat = cm ? t->orb_bit_id[o] : t->orb_id[o];
        u.idx_off = t->loc_off[r];
        u.t_off = cm ? t->orb_ctensor_off[o] : t->orb_itensor_off[o];
        u.scale = slot_scale(t, r);
        u.ratio = t->loc_ratio[r];
    }
    if (dev_upload(h, recs.data(), recs.size(), &up.recs)) return 1;
    // the cluster rows of every site, packed for the enthalpy pass (URow / URecE); equal records once
    std::vector<URecE> rec_e;
    std::vector<int32_t> rec_of((size_t)std::max<int64_t>(nloc, 1), 0);
    std::map<std::string, int32_t> rec_index;
    up.max_I = 1;
    up.all_k1 = 1;
    up.tens_len = 0;
    uint64_t nrows = 0;
    for (int64_t r = 0; r < nloc; ++r) {
        const URec &u = recs[(size_t)r];
        URecE e;
        memset(&e, 0, sizeof(e));
        for (int m = 0; m < u.I; ++m) e.st[m] = u.st[m];
        e.K = u.K; e.Nt = u.Nt; e.feat = u.feat; e.scale = u.scale;
        e.nat0 = (u.feat >= 0 && u.feat < h->F) ? h->natural[(size_t)u.feat] : 0.0;
        // (offsets inside one tensor, k * Nt + index, stay below the total checked here)
        if ((uint64_t)u.t_off + (uint64_t)u.K * (uint64_t)u.Nt > 0xffffffffull)
            return fail("cluster tensors of more than 2^32 entries");
        e.t_off = (uint32_t)u.t_off;
        up.tens_len = (int)std::min<uint64_t>(0x7fffffffull, std::max<uint64_t>((uint64_t)up.tens_len, (uint64_t)u.t_off + (uint64_t)u.K * (uint64_t)u.Nt));
        up.max_I = std::max(up.max_I, (int)u.I);
        if (u.K != 1) up.all_k1 = 0;
        nrows += (uint64_t)u.J;
        const std::string key((const char *)&e, sizeof(e));
        auto it = rec_index.find(key);
        if (it == rec_index.end()) {
            it = rec_index.emplace(key, (int32_t)rec_e.size()).first;
            rec_e.push_back(e);
        }
        rec_of[(size_t)r] = it->second;
    }
    if (rec_e.empty()) { URecE e; memset(&e, 0, sizeof(e)); rec_e.push_back(e); }
    up.n_recs_e = (int)rec_e.size();
    up.dict_lds = up.n_recs_e <= SMOLMC_UNIV_DICT_RECS && up.tens_len <= SMOLMC_UNIV_DICT_TENS && h->F <= SMOLMC_UNIV_DICT_NAT;
    if (nloc > 0x7fffffffll || nrows > 0x7fffffffull) return fail("more than 2^31 local cluster rows");
    std::vector<uint32_t> row_ptr((size_t)t->num_sites + 1, 0);
    std::vector<URow> rows((size_t)std::max<uint64_t>(nrows, 1));
    memset(rows.data(), 0, rows.size() * sizeof(URow));
    size_t q = 0;
    for (int s = 0; s < t->num_sites; ++s) {
        for (int64_t r = t->site_ptr[s]; r < t->site_ptr[s + 1]; ++r) {
            const int I = t->orb_nsites[t->loc_orbit[r]];
            for (int j = 0; j < t->loc_nrows[r]; ++j) {
                URow &w = rows[q++];
                const int32_t *m = t->loc_idx + t->loc_off[r] + (int64_t)j * I;
                for (int i = 0; i < SMOLMC_MAX_CLUSTER_SITES; ++i) w.x[i] = i < I ? m[i] : (I ? m[0] : s);
                w.rec = rec_of[(size_t)r];
            }
        }
        row_ptr[(size_t)s + 1] = (uint32_t)q;
    }
    up.rows_uniform = t->num_sites > 0 ? (int)row_ptr[1] : 0;
    for (int s = 0; s < t->num_sites; ++s)
        if (row_ptr[(size_t)s + 1] - row_ptr[(size_t)s] != (uint32_t)up.rows_uniform) up.rows_uniform = 0;
    const URow *d_rows = nullptr;
    if (dev_upload(h, rows.data(), rows.size(), &d_rows) || dev_upload(h, row_ptr.data(), row_ptr.size(), &up.row_ptr) ||
        dev_upload(h, rec_e.data(), rec_e.size(), &up.recs_e))
        return 1;
    up.rows = (const uint4 *)d_rows;
    return 0;
}
// the flip table of a TableFlip handle: checked here for every kernel family
static int univ_flip_table(smolmc_handle *h, const smolmc_tables *t) {
    if (!is_table(h)) return 0;
    UParams &up = h->up;
    if (t->n_flip_vectors <= 0 || !t->flip_table || !t->flip_weights)
        return fail("TableFlip needs a flip table (CompositionSpace.flip_table, "
                    "smol/moca/composition/space.py:404-429)");
    if (!(t->swap_weight >= 0.0 && t->swap_weight < 1.0))
        return fail("swap_weight must be in [0, 1)");
    const int ns = t->n_sublattices, d = (int)t->sub_code_ptr[ns];
    if (t->n_flip_vectors > SMOLMC_MAX_FLIP_VECTORS || d > SMOLMC_MAX_FLIP_DIMS)
        return fail("flip table larger than SMOLMC_MAX_FLIP_VECTORS x SMOLMC_MAX_FLIP_DIMS");
    std::vector<int> dim_sub(d);
    int max_nact = 0;
    for (int k = 0; k < ns; ++k) {
        for (int64_t c = t->sub_code_ptr[k]; c < t->sub_code_ptr[k + 1]; ++c) dim_sub[c] = k;
        max_nact = std::max(max_nact, (int)(t->sub_site_ptr[k + 1] - t->sub_site_ptr[k]));
    }
    h->max_step_flips = 2;
    for (int v = 0; v < t->n_flip_vectors; ++v) {
        // species are exchanged inside a sublattice (mcusher.py:612-634: "Sub-lattices can not
        // cross", assert len(site_ids) == 0), a step flips the sites of the depleted species
        int total = 0;
        for (int k = 0; k < ns; ++k) {
            int sum = 0, picks = 0;
            for (int64_t c = t->sub_code_ptr[k]; c < t->sub_code_ptr[k + 1]; ++c) {
                const int u = t->flip_table[(size_t)v * d + c];
                sum += u;
                picks += u < 0 ? -u : 0;
            }
            if (sum != 0) return fail("flip vector does not conserve the sites of a sublattice");
            total += picks;
        }
        if (total == 0) return fail("flip vector without any flip");
        if (total > SMOLMC_MAX_STEP_FLIPS) return fail("flip vector of more than SMOLMC_MAX_STEP_FLIPS flips");
        h->max_step_flips = std::max(h->max_step_flips, total);
    }
    for (int i = 0; i < 2 * t->n_flip_vectors; ++i)
        if (!(t->flip_weights[i] >= 0.0)) return fail("flip weights must be non-negative");
    const std::vector<double> ln = ln_table(max_nact + 1);
    if (dev_upload(h, t->flip_table, (size_t)t->n_flip_vectors * d, &up.tf_table) ||
        dev_upload(h, t->flip_weights, (size_t)2 * t->n_flip_vectors, &up.tf_w) ||
        dev_upload(h, ln.data(), ln.size(), &up.tf_ln) || dev_upload(h, dim_sub.data(), dim_sub.size(), &up.tf_dim_sub))
        return 1;
    up.tf_n = t->n_flip_vectors;
    up.tf_d = d;
    up.tf_sw = t->swap_weight;
    return 0;
}
// per-wave LDS: step scratch (flips, counts, weights, a-priori factors, running sums: 2464 B) + the occupancy when it fits
// (+ the step's feature deltas, one cell per cluster feature, while that stays small)
static int univ_lds_layout(smolmc_handle *h, const smolmc_tables *) {
    UParams &up = h->up;
    up.dfeat_cells = h->Fce <= 1024 ? (h->Fce + 1) / 2 * 2 : 0;
    up.acc_cells = up.dfeat_cells ? (h->F + 1) / 2 * 2 : 0;
    up.lds_shared = up.dict_lds ? SMOLMC_UNIV_DICT_BYTES : 0;
    auto lay_out = [&]() {
        const size_t scratch = (is_table(h) ? SMOLMC_UNIV_SCRATCH_TABLE : SMOLMC_UNIV_SCRATCH) +
                               (((size_t)up.dfeat_cells << up.dfeat_shift) + (size_t)up.acc_cells) * 8,
                     with_occ = (scratch + (size_t)h->Npad + 15) & ~(size_t)15;
        up.occ_lds = with_occ <= 160 * 1024 - 256 && !smolmc_env(ENV_UNIV_OCC_HBM);
        // the occupancy of one wave fits a CU's LDS alone but not behind the dictionaries: the dictionaries go (never a
        // request above the 160 KiB a CU has), the occupancy stays
        if (up.occ_lds && (size_t)up.lds_shared + with_occ > 160 * 1024) {
            up.dict_lds = 0;
            up.lds_shared = 0;
        }
        up.lds_per_wave = (int)(up.occ_lds ? with_occ : scratch);
        h->univ_wpb = 4;
        while (h->univ_wpb > 1 && (size_t)up.lds_shared + (size_t)up.lds_per_wave * h->univ_wpb > 64 * 1024) h->univ_wpb /= 2;
    };
    // shadow copies of the step's feature cells: as many as keep them within 4 KB -- and, for launches of more than
    // twelve walkers per CU, the workgroup within a quarter of the CU's LDS (a workgroup of 40.1 KB halves the resident
    // walkers of config 2: 1.3e9 -> 8.1e8 flips/s)
    up.dfeat_shift = 0;
    while (up.dfeat_cells && up.dfeat_shift < 3 && ((size_t)up.dfeat_cells << (up.dfeat_shift + 1)) <= 512) up.dfeat_shift++;
    lay_out();
    const bool crowded = (long long)h->cfg.n_replicas > 12ll * 256;
    auto too_big = [&]() { return crowded && h->univ_wpb == 4 && (size_t)up.lds_shared + (size_t)up.lds_per_wave * 4 > 40 * 1024; };
    while (too_big() && up.dfeat_shift > 0) { up.dfeat_shift--; lay_out(); }
    if (too_big() && up.dict_lds) {
        up.dict_lds = 0;
        up.lds_shared = 0;
        lay_out();
    }
    return 0;
}

// The launchers of the lean families: the row of family f is lean_families[f - K_LEAN], a launcher for lean_nslot 2 / 4 /
// 8 each (NULL: no such instantiation).  `replay` serves recorded flips and swaps, `table_replay` recorded TableFlip
// steps; a family without them replays on mc_kernel or the universal kernel (smolmc_replay).
typedef int (*LeanLauncher)(smolmc_handle *, const LeanParams &);
struct LeanFamilyRow {
    const char *name;                 // smolmc_kernel_info: the layout ...
    const char *wl_sums, *wl_means;   // ... and the tag of the Wang-Landau kernel (per-bin feature sums / running means)
    LeanLauncher run[3], replay[3], table_replay[3];
    LeanLauncher walker_mu[3];        // `run` while per-walker chemical potentials are set (smolmc_set_walker_mu)
    LeanLauncher wl_win[3];           // `run` while per-walker Wang-Landau windows are set (smolmc_set_wl_windows)
};
#define L2(f) {smolmc_launch_##f##_2, smolmc_launch_##f##_4, nullptr}
#define L3(f) {smolmc_launch_##f##_2, smolmc_launch_##f##_4, smolmc_launch_##f##_8}
#define NONE {nullptr, nullptr, nullptr}
static const LeanFamilyRow lean_families[] = {
    /* K_LEAN             */ {"lean", nullptr, nullptr, L2(lean), L2(lean_replay), L2(table_replay), L2(lean_wmu)},
    /* K_LEAN_BIAS        */ {"lean", nullptr, nullptr, L2(lean_bias), L2(lean_bias_replay), NONE, L2(lean_bias_wmu)},
    /* K_LEAN_CORR        */ {"lean", nullptr, nullptr, L2(lean_corr), L2(lean_replay), NONE, L2(lean_corr_wmu)}, // (KF: a template flag of the same launchers)
    /* K_WL               */ {"lean", " wl=v3", " wl=v3", L2(wl), L2(wl_replay), NONE, NONE, L2(wl_win)},
    /* K_TABLE_BIAS       */ {"lean", nullptr, nullptr, L2(table_bias), NONE, NONE, L2(table_bias_wmu)},
    /* K_TABLE_WL         */ {"lean", " wl=table", " wl=table-mean", L2(table_wl), NONE, NONE, NONE},
    /* K_MULTI            */ {"lean-multi", nullptr, nullptr, L3(multi), L3(multi_replay), L3(multi_table_replay), L3(multi_wmu)},
    /* K_MULTI_BIAS       */ {"lean-multi", nullptr, nullptr, L3(multi_bias), L3(multi_bias_replay), NONE, L3(multi_bias_wmu)},
    /* K_MULTI_WL         */ {"lean-multi", " wl=multi", " wl=multi-mean", L3(multi_wl), L3(multi_wl_replay), NONE, NONE, L3(multi_wl_win)},
    /* K_MULTI_WL_KF      */ {"lean-multi", " wl=multi", " wl=multi-mean", L3(multi_wl_kf), NONE, NONE, NONE},
    /* K_MULTI_TABLE_BIAS */ {"lean-multi", nullptr, nullptr, L3(multi_table_bias), NONE, NONE, L3(multi_table_bias_wmu)},
    /* K_MULTI_TABLE_WL   */ {"lean-multi", " wl=multi", " wl=multi-mean", L3(multi_table_wl), NONE, NONE, NONE},
};
#undef L2
#undef L3
#undef NONE
static_assert(sizeof(lean_families) / sizeof(lean_families[0]) == K_MULTI_TABLE_WL - K_LEAN + 1, "one row per lean family");
static LeanLauncher lean_launcher(const smolmc_handle *h, bool replay) {
    const LeanFamilyRow &row = lean_families[h->family - K_LEAN];
    const int i = h->lean_nslot == 2 ? 0 : (h->lean_nslot == 4 ? 1 : 2);
    if (!replay && h->lp.mu_stride) return row.walker_mu[i];
    if (!replay && h->lp.wl.win_off) return row.wl_win[i];
    // (the solo rows variants: runs of the plain family's solo handles whose clusters fall into one of their shapes;
    // replays and per-walker chemical potentials stay on the kernels above, which read the site-ordered rows)
    if (!replay && h->family == K_LEAN && h->solo_rows && h->lean_nslot == 2) return smolmc_launch_lean_rows_2;
    return !replay ? row.run[i] : (h->cfg.step_type == SMOLMC_STEP_TABLE_FLIP ? row.table_replay[i] : row.replay[i]);
}

// The kernel family of the handle, decided once: what a planner took, else mc_kernel, else -- TableFlip outside the
// lean families, or a model mc_kernel cannot run -- the universal kernel.
static KernelFamily family_of(const smolmc_handle *h, const LeanPlan &one, const LeanMultiPlan &multi) {
    const bool wl = is_wl(h), table = is_table(h), bias = h->kp.bias_type != 0;
    if (one.take)
        return bias ? (table ? K_TABLE_BIAS : K_LEAN_BIAS) : (wl && table) ? K_TABLE_WL : h->lean_kf ? K_LEAN_CORR : wl ? K_WL : K_LEAN;
    if (multi.take)
        return wl ? (h->lean_kf ? K_MULTI_WL_KF : table ? K_MULTI_TABLE_WL : K_MULTI_WL)
                  : bias ? (table ? K_MULTI_TABLE_BIAS : K_MULTI_BIAS) : K_MULTI;
    return (table || !h->general_ok) ? K_UNIVERSAL : K_GENERAL;
}

static int create_impl(const smolmc_tables *t, const smolmc_config *cfg, smolmc_handle **out, std::vector<int32_t> *new_of) {
    if (t->max_species > 255) return fail("more than 255 species codes per site");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("no HIP device available: the smol_amd engine requires an AMD GPU (there is no "
                    "CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail("invalid device ordinal");
    smolmc_handle *h = new smolmc_handle();
    h->cfg = *cfg;
    h->device = cfg->device;
    for (int e = 0; e < ENV_COUNT; ++e)
        if (smolmc_env_switches[e].dispatch && smolmc_env((SmolmcEnv)e)) h->env_dispatch |= 1u << e;
    if (new_of) {
        h->relabelled = true;
        h->new_of = *new_of;
        h->old_of.resize(new_of->size());
        for (size_t p = 0; p < new_of->size(); ++p) h->old_of[(*new_of)[p]] = (int32_t)p;
    }
    auto bail = [&](int rc) {
        smolmc_destroy(h);
        return rc;
    };
    if (hipSetDevice(h->device) != hipSuccess) return bail(fail("hipSetDevice failed"));
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail("hipStreamCreate failed"));
    h->own_stream = true;
    hipEventCreate(&h->ev0);
    hipEventCreate(&h->ev1);
    for (auto stage : {create_dimensions, create_site_codes, build_mc_tables, build_ref_tables, create_model_params, create_bias,
                       create_ewald_field, create_sublattices, create_walker_state, create_wl_state, create_general_layout})
        if (int rc = stage(h, t)) return bail(rc);
    LeanPlan one;
    LeanMultiPlan multi;
    if (int rc = plan_lean(h, t, one)) return bail(rc);
    if (!one.take && h->lean_tables)
        if (int rc = plan_lean_multi(h, t, one, multi)) return bail(rc);
    if (smolmc_env(ENV_DEBUG))
        fprintf(stderr, "[smolmc] lean=%d tables=%d nslot=%d mm=%d lds=%zu ew=%d compact=%d field=%d nact=%d "
                        "ew_nact=%d ew_act_base=%d sbase=%d general: nslot=%d mm=%d lds=%zu\n",
                (int)one.take, (int)h->lean_tables, h->lean_nslot, h->lean_mm, h->lean_lds, t->has_ewald,
                h->kp.ew_compact, h->lp.ew_field, one.nact, h->kp.ew_nact, h->kp.ew_act_base, one.sbase, h->nslot, h->mm,
                h->lds_bytes);
    for (auto stage : {univ_pack_records, univ_flip_table, univ_lds_layout})
        if (int rc = stage(h, t)) return bail(rc);
    h->family = family_of(h, one, multi);
    *out = h;
    return 0;
}

extern "C" int smolmc_destroy(smolmc_handle *h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    smolmc_dist_free(h);
    for (void *p : h->allocs) hipFree(p);
    if (h->d_eval_occ) hipFree(h->d_eval_occ);
    smolmc_obs_free(h->obs);
    if (h->obs_ev0) hipEventDestroy(h->obs_ev0);
    if (h->obs_ev1) hipEventDestroy(h->obs_ev1);
    smolmc_min_free(h);
    smolmc_stat_free(h);
    smolmc_sfac_free(h->sfac);
    smolmc_conn_free(h->conn);
    free_samples(h);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

extern "C" int smolmc_num_features(const smolmc_handle *h) { return h ? h->F : -1; }
extern "C" int smolmc_wl_num_levels(const smolmc_handle *h) { return h ? h->L : -1; }
extern "C" int smolmc_natural_parameters(const smolmc_handle *h, double *out) {
    if (!h || !out) return fail("null argument");
    memcpy(out, h->natural.data(), h->natural.size() * 8);
    return 0;
}

extern "C" int smolmc_set_stream(smolmc_handle *h, void *stream) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    return 0;
}

static int launch_eval_full(smolmc_handle *h, const uint8_t *d_occ8, int nocc, double *d_out, int ce_only = 0);
int smolmc_eval_extensive(smolmc_handle *h, const uint8_t *d_occ8, int nocc, double *d_out) {
    return launch_eval_full(h, d_occ8, nocc, d_out);
}
static int launch_eval_full(smolmc_handle *h, const uint8_t *d_occ8, int nocc, double *d_out, int ce_only) {
    // occupancies per block (see the kernel): four when the copies fit 60 KB of LDS and only the cluster features are
    // wanted, one with the scalar features (their loops take one occupancy), none staged beyond 60 KB
    int M = h->Npad <= 60 * 1024 ? 1 : 0;
    if (ce_only && M && nocc >= 8) M = std::min(4, (60 * 1024) / h->Npad);
    const int per = M > 0 ? M : 1;
    hipLaunchKernelGGL(eval_full_kernel, dim3((unsigned)((nocc + per - 1) / per)), dim3(256), (size_t)M * h->Npad, h->stream, h->rt, d_occ8,
                       d_out, ce_only, nocc, M);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- lazy cluster features (lean_mode) ---------------------------------------------------------------------
// The lean kernels of such a handle carry the scalar features only (d_lazy_scal, row stride nscal); the cluster
// part of kp.features is evaluated from the occupancies where it is read.
static bool is_lazy(const smolmc_handle *h) { return h->lazy_tables && h->lean(); }
static int lazy_nscal(const smolmc_handle *h) { return (h->rt.has_ewald ? 1 : 0) + (h->rt.has_mu ? 1 : 0); }
// rows of full feature vectors [n][F] <-> rows of scalar features [n][nscal]
__global__ void lazy_scalars_kernel(double *features, double *scal, size_t n, int F, int Fce, int nscal, int to_scal) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (size_t)nscal) return;
    const size_t row = i / nscal;
    const int j = (int)(i % nscal);
    if (to_scal) scal[row * nscal + j] = features[row * F + Fce + j];
    else features[row * F + Fce + j] = scal[row * nscal + j];
}
static int lazy_scalars(smolmc_handle *h, double *features, double *scal, size_t n, int to_scal) {
    const int ns = lazy_nscal(h);
    if (!ns || !n) return 0;
    hipLaunchKernelGGL(lazy_scalars_kernel, dim3((unsigned)((n * ns + 255) / 256)), dim3(256), 0, h->stream, features, scal, n,
                       h->F, h->Fce, ns, to_scal);
    HIPCHK(hipGetLastError());
    return 0;
}
// kp.features current (before anybody reads them, and before a kernel that updates them incrementally -- mc_kernel /
// the universal kernel replaying records the lean kernels do not take -- runs on a lazy handle)
static int ensure_features(smolmc_handle *h) {
    if (!is_lazy(h) || !h->ce_dirty) return 0;
    TRY(launch_eval_full(h, h->kp.occ, h->R, h->kp.features, 1));
    TRY(lazy_scalars(h, h->kp.features, h->d_lazy_scal, (size_t)h->R, 0));
    h->ce_dirty = false;
    return 0;
}
// ... and after such a kernel (or smolmc_set_state): the scalars the lean kernels continue from
static int lazy_scalars_from_features(smolmc_handle *h) {
    if (!is_lazy(h)) return 0;
    TRY(lazy_scalars(h, h->kp.features, h->d_lazy_scal, (size_t)h->R, 1));
    h->ce_dirty = false;
    return 0;
}

// ---- the boundary of a relabelled handle (see plan_relabelling): caller's numbering <-> engine's ----------------
// rows of occupancies in the caller's numbering -> the engine's (a copy; the caller's array on a plain handle)
static const int32_t *occ_in(const smolmc_handle *h, const int32_t *occ, size_t rows, std::vector<int32_t> &tmp) {
    if (!h->relabelled) return occ;
    const size_t N = (size_t)h->N;
    tmp.resize(rows * N);
    const int32_t *old_of = h->old_of.data();
    for (size_t r = 0; r < rows; ++r) {
        const int32_t *src = occ + r * N;
        int32_t *dst = tmp.data() + r * N;
        for (size_t p = 0; p < N; ++p) dst[p] = src[old_of[p]];
    }
    return tmp.data();
}
// ... and back, in place
static void occ_out(const smolmc_handle *h, int32_t *occ, size_t rows) {
    if (!h->relabelled) return;
    const size_t N = (size_t)h->N;
    std::vector<int32_t> row(N);
    const int32_t *new_of = h->new_of.data();
    for (size_t r = 0; r < rows; ++r) {
        int32_t *o = occ + r * N;
        std::copy(o, o + N, row.begin());
        for (size_t p = 0; p < N; ++p) o[p] = row[new_of[p]];
    }
}
// step records (site, code) x SMOLMC_MAX_STEP_FLIPS: the sites renamed; a site outside the cell is left as it is --
// the range checks of the entry point reject it (renaming it would turn it into a step nobody asked for)
static const int32_t *steps_in(const smolmc_handle *h, const int32_t *steps, size_t nrec, std::vector<int32_t> &tmp) {
    if (!h->relabelled) return steps;
    tmp.assign(steps, steps + nrec * SMOLMC_STEP_ROW);
    for (size_t i = 0; i < nrec; ++i)
        for (int f = 0; f < SMOLMC_MAX_STEP_FLIPS; ++f) {
            int32_t &site = tmp[i * SMOLMC_STEP_ROW + 2 * f];
            if (site < 0) break;
            if (site < h->N) site = h->new_of[site];
        }
    return tmp.data();
}

static int upload_occ(smolmc_handle *h, const int32_t *occ, size_t nocc, uint8_t *d_occ8) {
    const size_t n32 = nocc * h->N;
    // every code must exist on its site: a larger one would index past the tensors / tables on the
    // device (the reference reads garbage there, SURVEY 8b "error conventions")
    const uint8_t *lim = h->site_ncodes.data();
    const size_t N = (size_t)h->N;
    for (size_t i = 0, s = 0; i < n32; ++i, s = (s + 1 == N ? 0 : s + 1))
        if (occ[i] < 0 || occ[i] >= (int)lim[s]) {
            char msg[160];
            snprintf(msg, sizeof msg, "occupancy code %d out of range on site %zu (%d species codes there)", occ[i],
                     h->relabelled ? (size_t)h->old_of[s] : s, (int)lim[s]); // (the site in the caller's numbering)
            return fail(msg);
        }
    DevScratch d32;
    TRY(d32.alloc(std::max<size_t>(n32 * 4, 16)));
    HIPCHK(hipMemcpyAsync(d32.p, occ, n32 * 4, hipMemcpyHostToDevice, h->stream));
    const size_t total = nocc * h->Npad;
    hipLaunchKernelGGL(pack_occ_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,
                       d32.as<int>(), d_occ8, h->N, h->Npad, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

static void set_betas(smolmc_handle *h, const double *temperature, std::vector<double> &beta) {
    beta.resize(h->R);
    for (int r = 0; r < h->R; ++r) {
        const double T = temperature ? temperature[r] : 0.0;
        beta[r] = 1.0 / (SMOLMC_KB * T); // ThermalKernelMixin (kernel/base.py:398)
    }
}

// ---- per-walker chemical potentials (smolmc_set_walker_mu) ------------------------------------------------------
// A mu-T grid in one handle: walker r reads its chemical potentials from row r of a device array in the kernels'
// layout (LeanParams::mu_stride) instead of the one row the handle was created with.  The chemical work is the last
// feature, natural parameter -1; a change of rows re-prices it on the device from the current occupancies
// (smolmc_walker_mu_reprice, walker_mu.hip: a kernel of its own translation unit, so that no kernel of this one moves).
// why a handle takes no per-walker rows (null: it does)
static int walker_mu_refused(const smolmc_handle *h, const std::string &what = "per-walker chemical potentials") {
    if (h->dist) return fail(what + ": a distance handle has none (its objective is a distance to a target, no chemical work)");
    if (!h->rt.has_mu) return fail(what + ": the handle was created without has_mu (no chemical-work feature to price)");
    if (is_wl(h)) return fail(what + ": a Wang-Landau handle estimates one density of states, of one Hamiltonian");
    if (!h->lean())
        return fail(what + ": only the lean kernel families take them, this handle runs " +
                    std::string(h->univ() ? "the universal kernel" : "mc_kernel") + " | not lean: " +
                    (h->lean_reason.empty() ? std::string("single-class planner refused the model") : h->lean_reason));
    return 0;
}
// sublattices and species codes per sublattice of the rows' cells in the kernels' layout
static int walker_mu_shape(const smolmc_handle *h, int *ncodes) {
    const int ns = h->lean_multi() ? h->lp.m_nsub : 1;
    for (int k = 0; k < ns; ++k) ncodes[k] = std::min(h->lean_multi() ? h->lp.m_ncodes[k] : h->lp.ncodes, h->rt.mu_W);
    return ns;
}

// ---- exchange across the mu-T grid: the state points (smolmc_exchange_grid, below) ---------------------------------
// walker -> state point after the exchanges so far (the identity when none ran since the points were named)
static int grid_point_of(smolmc_handle *h, std::vector<int32_t> &point_of) {
    point_of.resize(h->R);
    if (!h->grid_permuted) {
        for (int r = 0; r < h->R; ++r) point_of[r] = r;
        return 0;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(point_of.data(), h->d_point_of, (size_t)h->R * 4, hipMemcpyDeviceToHost));
    return 0;
}
// the current assignment becomes the identity map: state point p is what walker p holds now (every call that names
// temperatures or rows starts with this; the device arrays the kernels read already are in walker order)
static int grid_rebase(smolmc_handle *h) {
    if (!h->grid_permuted) return 0;
    std::vector<int32_t> po;
    TRY(grid_point_of(h, po));
    const size_t R = (size_t)h->R;
    if (h->point_T.size() == R) {
        std::vector<double> T(R);
        for (size_t r = 0; r < R; ++r) T[r] = h->point_T[po[r]];
        h->point_T.swap(T);
    }
    if (!h->walker_mu.empty()) {
        const size_t w = h->walker_mu.size() / R;
        std::vector<double> rows(h->walker_mu.size());
        for (size_t r = 0; r < R; ++r) std::copy_n(h->walker_mu.begin() + (size_t)po[r] * w, w, rows.begin() + r * w);
        h->walker_mu.swap(rows);
    }
    for (size_t r = 0; r < R; ++r) po[r] = (int32_t)r;
    HIPCHK(hipMemcpy(h->d_point_of, po.data(), R * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_walker_at, po.data(), R * 4, hipMemcpyHostToDevice));
    h->grid_permuted = false;
    return 0;
}
static void grid_name_temperatures(smolmc_handle *h, const double *temperature) {
    h->point_T.resize(h->R);
    for (int r = 0; r < h->R; ++r) h->point_T[r] = temperature ? temperature[r] : 0.0;
    h->point_T_stale = false;
}

extern "C" int smolmc_set_walker_mu(smolmc_handle *h, const double *mu) {
    if (!h) return fail("null handle");
    TRY(walker_mu_refused(h));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    LeanParams &lp = h->lp;
    const bool multi = h->lean_multi();
    const int stride = multi ? 32 : 8, W = h->rt.mu_W;
    const size_t R = (size_t)h->R;
    int ncodes[4];
    const int ns = walker_mu_shape(h, ncodes);
    const double *rows_old = multi ? lp.m_mu : lp.mu_row;
    const int stride_old = lp.mu_stride;
    const double *rows_new = h->d_mu_create;
    double mmax = h->mu_max_create;
    if (mu) {
        // the per-wave cells go behind the workgroup's LDS: the launch must still fit a CU's 160 KiB
        const int wpb = multi ? h->waves_per_block_lean : is_table(h) ? h->lean_wpb : h->lean_solo ? 1 : 4;
        const size_t lds = ((!multi && is_table(h) && wpb == 8 ? h->lean_lds_wpb8 : h->lean_lds) + 7) & ~(size_t)7;
        if (lds + walker_mu_lds(stride, wpb) > 160 * 1024)
            return fail("per-walker chemical potentials: no LDS left for the walkers' row cells on this handle");
        std::vector<double> rows(R * stride, 0.0);
        mmax = 0.0;
        for (size_t r = 0; r < R; ++r)
            for (int k = 0; k < ns; ++k)
                for (int c = 0; c < ncodes[k]; ++c) {
                    const double v = mu[(r * ns + k) * W + c];
                    if (!std::isfinite(v)) return fail("per-walker chemical potentials must be finite");
                    rows[r * stride + k * 8 + c] = v;
                    mmax = std::max(mmax, std::fabs(v));
                }
        if (!h->d_walker_mu[0])
            for (int i = 0; i < 2; ++i) TRY(dev_alloc(h, R * stride, &h->d_walker_mu[i]));
        // (d_walker_mu[0] is the copy in use: the new rows go to the other one, the two swap after the re-pricing)
        HIPCHK(hipMemcpy(h->d_walker_mu[1], rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
        rows_new = h->d_walker_mu[1];
        lp.mu_cell_off = (uint32_t)lds;
    }
    TRY(grid_rebase(h)); // (past the refusals: the temperatures of the state points follow their walkers)
    // (lazy cluster features: lp.features are the scalar features' rows, the chemical work their last entry too)
    TRY(smolmc_walker_mu_reprice(h, rows_old, stride_old, rows_new, mu ? stride : 0, lp.features, lp.F, h->kp.enthalpy));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (is_lazy(h)) h->ce_dirty = true; // (kp.features takes its scalar entries from the lean kernels' rows when it is read)
    if (mu) {
        std::swap(h->d_walker_mu[0], h->d_walker_mu[1]);
        h->walker_mu.assign(mu, mu + R * ns * W);
    } else {
        h->walker_mu.clear();
    }
    (multi ? lp.m_mu : lp.mu_row) = rows_new;
    lp.mu_stride = mu ? stride : 0;
    lean_set_fast_eps(h, mmax);
    return 0;
}

extern "C" int smolmc_get_walker_mu(smolmc_handle *h, double *mu) {
    if (!h) return fail("null handle");
    TRY(walker_mu_refused(h));
    if (!mu) return fail("null argument");
    int ncodes[4];
    const int ns = walker_mu_shape(h, ncodes), W = h->rt.mu_W;
    const size_t R = (size_t)h->R;
    if (!h->walker_mu.empty()) { // (the rows of the state points, each walker's current one: smolmc_exchange_grid)
        std::vector<int32_t> po;
        TRY(grid_point_of(h, po));
        const size_t w = (size_t)ns * W;
        for (size_t r = 0; r < R; ++r) memcpy(mu + r * w, h->walker_mu.data() + (size_t)po[r] * w, w * 8);
        return 0;
    }
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> row(h->lean_multi() ? 32 : 8, 0.0); // the create-time row: [8], or [4][8], in the kernels' layout
    HIPCHK(hipMemcpy(row.data(), h->d_mu_create, row.size() * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < R; ++r)
        for (int k = 0; k < ns; ++k)
            for (int c = 0; c < W; ++c) mu[(r * ns + k) * W + c] = c < ncodes[k] ? row[k * 8 + c] : 0.0;
    return 0;
}

// ---- per-walker Wang-Landau windows (smolmc_set_wl_windows) and their exchange (smolmc_exchange_wl) ------------------
// Replica-exchange Wang-Landau in one handle: walker r samples the window of the ESTIMATOR it holds and updates that
// estimator's arrays (WlWindow, smolmc_common.h; the window variants of mc_wl_kernel and mc_lean_multi_kernel read the
// record, every other kernel family is refused here).  Estimator e is the window and density-of-states copy walker e
// held at the latest smolmc_set_wl_windows; wl_exchange_kernel (wl_exchange.hip) swaps the records of two walkers.
static int wl_windows_refused(const smolmc_handle *h, const char *what) {
    const std::string w(what);
    if (h->dist || h->cfg.kernel_type != SMOLMC_KERNEL_WANGLANDAU)
        return fail(w + ": the handle is not a Wang-Landau kernel (only those have an energy window)");
    if (!h->lean())
        return fail(w + ": only mc_wl_kernel and the Wang-Landau variant of mc_lean_multi_kernel take per-walker windows, this handle runs " +
                    std::string(h->univ() ? "the universal kernel" : "mc_kernel") + " | not lean: " +
                    (h->lean_reason.empty() ? std::string(smolmc_env(ENV_FORCE_GENERAL) ? "SMOLMC_FORCE_GENERAL" : "single-class planner refused the model") : h->lean_reason));
    if (h->family != K_WL && h->family != K_MULTI_WL)
        return fail(w + ": only mc_wl_kernel and the Wang-Landau variant of mc_lean_multi_kernel take per-walker windows, this handle runs " +
                    (h->family == K_MULTI_WL_KF ? "the KF variant (several correlation functions per orbit)" : "a TableFlip Wang-Landau kernel"));
    return 0;
}
// the walkers' records: estimator r with its window to walker r (the identity map); nothing while no windows are set
static int wl_windows_upload(smolmc_handle *h) {
    if (h->wl_win_min.empty()) return 0;
    const size_t R = (size_t)h->R;
    std::vector<WlWindow> win(R);
    std::vector<int32_t> id(R);
    for (size_t r = 0; r < R; ++r) {
        win[r].vmin = h->wl_win_min[r]; win[r].vmax = h->wl_win_max[r];
        win[r].est = (int32_t)r; win[r].pad = 0;
        id[r] = (int32_t)r;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_wl_win, win.data(), R * sizeof(WlWindow), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_wl_walker_at, id.data(), R * 4, hipMemcpyHostToDevice));
    return 0;
}
// ... as the walkers hold them now (after the exchanges so far); empty while no windows are set
static int wl_windows_download(smolmc_handle *h, std::vector<WlWindow> &win) {
    win.clear();
    if (h->wl_win_min.empty()) return 0;
    win.resize(h->R);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(win.data(), h->d_wl_win, (size_t)h->R * sizeof(WlWindow), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_set_wl_windows(smolmc_handle *h, const double *vmin, const double *vmax) {
    if (!h) return fail("null handle");
    TRY(wl_windows_refused(h, "smolmc_set_wl_windows"));
    if ((vmin == nullptr) != (vmax == nullptr)) return fail("smolmc_set_wl_windows: vmin and vmax are given together, or both NULL");
    HIPCHK(hipSetDevice(h->device));
    const size_t R = (size_t)h->R;
    if (!vmin) { // back to the config's window
        HIPCHK(hipStreamSynchronize(h->stream));
        h->wl_win_min.clear();
        h->wl_win_max.clear();
        h->lp.wl.win_off = 0;
        return 0;
    }
    for (size_t r = 0; r < R; ++r) {
        if (!std::isfinite(vmin[r]) || !std::isfinite(vmax[r]) || !(vmax[r] > vmin[r]))
            return fail("smolmc_set_wl_windows: window of walker " + std::to_string(r) + " is not a finite range vmin < vmax");
        // (the rule of smolmc_create: the LDS layout of the kernels is sized by L)
        const int L = (int)ceil((vmax[r] - vmin[r]) / h->cfg.wl_bin_size);
        if (L != h->L)
            return fail("smolmc_set_wl_windows: window of walker " + std::to_string(r) + " has " + std::to_string(L) +
                        " bins, the handle has L = " + std::to_string(h->L) + " (every window must give ceil((vmax - vmin) / bin_size) == L)");
    }
    h->wl_win_min.assign(vmin, vmin + R);
    h->wl_win_max.assign(vmax, vmax + R);
    TRY(wl_windows_upload(h));
    h->lp.wl.win_off = (uint32_t)((const unsigned char *)h->d_wl_win - (const unsigned char *)h->kp.wl_m);
    return 0;
}

extern "C" int smolmc_get_wl_windows(smolmc_handle *h, double *vmin, double *vmax, int32_t *estimator_of) {
    if (!h) return fail("null handle");
    TRY(wl_windows_refused(h, "smolmc_get_wl_windows"));
    HIPCHK(hipSetDevice(h->device));
    std::vector<WlWindow> win;
    TRY(wl_windows_download(h, win));
    for (int r = 0; r < h->R; ++r) {
        if (vmin) vmin[r] = win.empty() ? h->cfg.wl_min_enthalpy : win[r].vmin;
        if (vmax) vmax[r] = win.empty() ? h->cfg.wl_max_enthalpy : win[r].vmax;
        if (estimator_of) estimator_of[r] = win.empty() ? r : win[r].est;
    }
    return 0;
}

// ---- one exchange attempt between disjoint pairs: what smolmc_exchange_wl (below) and smolmc_exchange_grid share -----
// Either call takes npairs pairs of entries 0 .. R - 1 (`noun` says what an entry names) with one host-made log u per
// pair, decides on the device and reads the accept flags back when `stats` is given.
static int pair_exchange_check(const smolmc_handle *h, const char *fn, const char *noun, int npairs, const int32_t *pairs,
                               const double *log_u) {
    if (npairs < 0 || (npairs > 0 && (!pairs || !log_u))) return fail("null argument");
    const int R = h->R;
    std::vector<uint8_t> seen(R, 0);
    for (int i = 0; i < 2 * npairs; ++i) {
        const int p = pairs[i];
        const auto entry = [&] { return std::string(fn) + ": " + noun + " " + std::to_string(p); };
        if (p < 0 || p >= R) return fail(entry() + " of pair " + std::to_string(i / 2) + " is out of range 0 .. " + std::to_string(R - 1));
        if (seen[p]) return fail(entry() + " appears in two pairs of one call (the pairs of a call are decided at once: they must be disjoint)");
        seen[p] = 1;
    }
    for (int i = 0; i < npairs; ++i)
        if (!std::isfinite(log_u[i]) && !(std::isinf(log_u[i]) && log_u[i] < 0))
            return fail(std::string(fn) + ": log_u must be finite or -inf (pair " + std::to_string(i) + ")");
    return 0;
}
// The staging of a call, h->d_pair_stage, allocated at the first one: log u [half] f64 | pairs [half][2] i32 | accept
// flags [half] i32 with half = R / 2 (disjoint pairs: npairs <= R / 2).  Queues the uploads on the handle's stream.
struct PairStage {
    double *log_u;
    int32_t *pairs, *acc;
};
static int pair_exchange_stage(smolmc_handle *h, int npairs, const int32_t *pairs, const double *log_u, PairStage &st) {
    const size_t half = (size_t)h->R / 2;
    if (!h->d_pair_stage) TRY(dev_alloc(h, 2 * half + half / 2 + 1, &h->d_pair_stage));
    st.log_u = h->d_pair_stage;
    st.pairs = (int32_t *)(h->d_pair_stage + half);
    st.acc = (int32_t *)(h->d_pair_stage + 2 * half);
    // (pageable sources: the runtime has read them -- into its staging memory, or to the device -- when hipMemcpyAsync
    // returns, so the caller may free them at once; the copies wait for the work queued before them on the stream)
    HIPCHK(hipMemcpyAsync(st.log_u, log_u, (size_t)npairs * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st.pairs, pairs, (size_t)npairs * 8, hipMemcpyHostToDevice, h->stream));
    return 0;
}
// stats [npairs][2] gains the attempts and the acceptances of the call (this waits for the kernel)
static int pair_exchange_stats(smolmc_handle *h, int npairs, const int32_t *d_acc, int64_t *stats) {
    std::vector<int32_t> acc(npairs);
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc, (size_t)npairs * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < npairs; ++i) {
        stats[2 * i] += 1;
        stats[2 * i + 1] += acc[i];
    }
    return 0;
}

extern "C" int smolmc_exchange_wl(smolmc_handle *h, int npairs, const int32_t *pairs, const double *log_u, int64_t *stats) {
    if (!h) return fail("null handle");
    TRY(wl_windows_refused(h, "smolmc_exchange_wl"));
    if (h->wl_win_min.empty()) return fail("smolmc_exchange_wl: no per-walker windows are set (smolmc_set_wl_windows first)");
    TRY(pair_exchange_check(h, "smolmc_exchange_wl", "estimator", npairs, pairs, log_u));
    if (npairs == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    PairStage st;
    TRY(pair_exchange_stage(h, npairs, pairs, log_u, st));
    TRY(smolmc_wl_exchange_launch(h, npairs, st.pairs, st.log_u, st.acc));
    return stats ? pair_exchange_stats(h, npairs, st.acc, stats) : 0;
}

// ---- the merge of a window's copies (smolmc_wl_synchronise): the merge mode of wl_exchange_kernel ---------------------
// Valid on every Wang-Landau family: entropy, histogram and factor are the same three arrays for all of them, in
// estimator order; without windows every estimator has the config's window.
static int wl_synchronise_refused(const smolmc_handle *h, int copies) {
    const std::string w("smolmc_wl_synchronise");
    if (h->dist || h->cfg.kernel_type != SMOLMC_KERNEL_WANGLANDAU)
        return fail(w + ": the handle is not a Wang-Landau kernel (only those have entropies to merge)");
    if (copies < 1 || h->R % copies)
        return fail(w + ": copies = " + std::to_string(copies) + " is not a divisor of the handle's " + std::to_string(h->R) +
                    " estimators (group g is the estimators g * copies .. g * copies + copies - 1)");
    if (!h->wl_win_min.empty())
        for (int e = 0; e < h->R; ++e) {
            const int e0 = e - e % copies;
            if (memcmp(&h->wl_win_min[e], &h->wl_win_min[e0], 8) || memcmp(&h->wl_win_max[e], &h->wl_win_max[e0], 8))
                return fail(w + ": group " + std::to_string(e / copies) + " does not have one window: estimator " + std::to_string(e) +
                            " differs from estimator " + std::to_string(e0) + " (only copies of one window [vmin, vmax) are merged)");
        }
    if (h->cfg.wl_check_period != 0)
        return fail(w + ": the handle checks flatness inside the sampling kernels every " + std::to_string(h->cfg.wl_check_period) +
                    " steps, which would reset single copies behind the merge (create the handle with check period 0)");
    return 0;
}

extern "C" int smolmc_wl_synchronise(smolmc_handle *h, int copies, int32_t *status_out, double *mod_factor_out) {
    if (!h) return fail("null handle");
    TRY(wl_synchronise_refused(h, copies));
    HIPCHK(hipSetDevice(h->device));
    const size_t G = (size_t)(h->R / copies);
    if (!status_out && !mod_factor_out) return smolmc_wl_merge_launch(h, copies, nullptr, nullptr);
    DevScratch out; // factors [G] f64 | status words [G] i32 (d_pair_stage holds R / 2 entries: copies = 1 has R groups)
    TRY(out.alloc(G * 12));
    TRY(smolmc_wl_merge_launch(h, copies, (int32_t *)(out.as<double>() + G), out.as<double>()));
    std::vector<unsigned char> host(G * 12);
    HIPCHK(hipMemcpyAsync(host.data(), out.p, G * 12, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (mod_factor_out) memcpy(mod_factor_out, host.data(), G * 8);
    if (status_out) memcpy(status_out, host.data() + G * 8, G * 4);
    return 0;
}

// ---- smolmc_set_state in stages (the first one is shared with smolmc_set_temperature) --------------------------------
// the temperatures of the call in force: the state points named after their walkers, the inverse temperatures uploaded
static int apply_temperatures(smolmc_handle *h, const double *temperature) {
    std::vector<double> beta;
    set_betas(h, temperature, beta);
    TRY(grid_rebase(h));
    grid_name_temperatures(h, temperature);
    HIPCHK(hipMemcpy(h->d_beta, beta.data(), (size_t)h->R * 8, hipMemcpyHostToDevice));
    h->order_dirty = true;
    return 0;
}

// seeds and step counters start over under reset_aux; the accepted flag always does
static int reset_counters(smolmc_handle *h, const uint64_t *seeds, int reset_aux) {
    KParams &kp = h->kp;
    const size_t R = h->R;
    if (reset_aux) {
        std::vector<uint64_t> sd(R);
        for (size_t r = 0; r < R; ++r) sd[r] = seeds ? seeds[r] : (uint64_t)r;
        HIPCHK(hipMemcpy((void *)kp.seeds, sd.data(), R * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(kp.nsteps, 0, R * 8, h->stream));
        HIPCHK(hipMemsetAsync(kp.nacc, 0, R * 8, h->stream));
    }
    HIPCHK(hipMemsetAsync(kp.last_acc, 1, R, h->stream));
    return 0;
}

// MCBias.compute_bias of every initial occupancy (kernel/base.py:362-363), on the host: the occupancies are host
// arrays here and this runs once per set_state.  occ [R][N] in the engine's numbering -> b0 [R], the bias, and
// q0 [R][SMOLMC_MAX_BIAS_ROWS], the running sums of the hyperplane terms
static void initial_bias(const smolmc_handle *h, const int32_t *occ, std::vector<double> &b0, std::vector<double> &q0) {
    const KParams &kp = h->kp;
    const size_t R = h->R;
    const int N = h->N, W = kp.bias_W;
    b0.assign(R, 0.0);
    q0.assign(R * SMOLMC_MAX_BIAS_ROWS, 0.0);
    for (size_t r = 0; r < R; ++r) {
        const int32_t *o = occ + r * (size_t)N;
        if (kp.bias_type == SMOLMC_BIAS_FUGACITY) {
            double acc = 0.0;
            for (int s = 0; s < N; ++s) acc += log(h->bias_host[(size_t)s * W + o[s]]); // bias.py:174-186
            b0[r] = acc;
        } else {
            // SquareChargeBias (bias.py:264-277) = one hyperplane with intercept 0;
            // SquareHyperplaneBias (bias.py:352-366): -penalty * sum_r (A_r . n - b_r)^2
            double sq = 0.0;
            for (int k = 0; k < kp.bias_rows; ++k) {
                double acc = 0.0;
                const double *tab = h->bias_host.data() + (size_t)k * kp.bias_row_stride;
                for (int s = 0; s < N; ++s) acc += tab[(size_t)s * W + o[s]];
                acc -= h->bias_icpt[k];
                q0[r * SMOLMC_MAX_BIAS_ROWS + k] = acc;
                sq += acc * acc;
            }
            b0[r] = -kp.bias_pen * sq;
        }
    }
}

// the potential field of the walkers' occupancies (kp.ew_phi), where the handle keeps one
static int init_ewald_field(smolmc_handle *h) {
    const KParams &kp = h->kp;
    if (!kp.ew_field) return 0;
    LeanParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.occ = kp.occ; fp.Npad = h->Npad; fp.sbase = kp.ew_act_base; fp.ew_nact = kp.ew_nact;
    fp.ew_W = kp.ew_W; fp.ew_qs = kp.ew_qs; fp.ew_G = kp.ew_G; fp.ew_frozen = kp.ew_frozen;
    fp.ew_phi = kp.ew_phi;
    const size_t shm = (size_t)kp.ew_nact * 8;
    if (shm > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)ewald_field_init_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(ewald_field_init_kernel, dim3((unsigned)h->R), dim3(256), shm, h->stream, fp);
    HIPCHK(hipGetLastError());
    return 0;
}

// features and enthalpy of the walkers' occupancies
static int initial_trace(smolmc_handle *h) {
    KParams &kp = h->kp;
    const size_t R = h->R;
    TRY(launch_eval_full(h, kp.occ, (int)R, kp.features));
    // (per-walker chemical potentials: the chemical work of the initial trace at the walker's own row)
    if (!h->walker_mu.empty()) TRY(smolmc_walker_mu_reprice(h, h->d_mu_create, 0, h->d_walker_mu[0], h->lp.mu_stride, kp.features, h->F, nullptr));
    hipLaunchKernelGGL(dot_features_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, h->stream,
                       kp.features, h->d_natural, kp.enthalpy, (int)R, h->F);
    HIPCHK(hipGetLastError());
    return lazy_scalars_from_features(h);
}

// reset_aux: the estimators go back to the walkers they were given to (a continuation keeps the map), and a
// Wang-Landau handle starts its estimate over
static int wl_reset(smolmc_handle *h) {
    TRY(wl_windows_upload(h));
    if (!is_wl(h)) return 0;
    KParams &kp = h->kp;
    const size_t R = h->R, RL = R * h->L;
    HIPCHK(hipMemsetAsync(kp.wl_entropy, 0, RL * 8, h->stream));
    HIPCHK(hipMemsetAsync(kp.wl_hist, 0, RL * 8, h->stream));
    HIPCHK(hipMemsetAsync(kp.wl_occur, 0, RL * 8, h->stream));
    HIPCHK(hipMemsetAsync(kp.wl_meanf, 0, RL * h->F * 8, h->stream));
    h->wl_sums = false; // all zero: either representation
    HIPCHK(hipMemsetAsync(kp.wl_counter, 0, R * 8, h->stream));
    std::vector<double> m0(R, h->cfg.wl_mod_factor);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(kp.wl_m, m0.data(), R * 8, hipMemcpyHostToDevice));
    return 0;
}

// The bin of the CURRENT enthalpy indexes the entropy / histogram arrays unchecked in the
// kernels (only proposed enthalpies are tested against the window, wanglandau.py:190-193).
// The reference raises IndexError above the window and wraps to a wrong bin below it
// (negative Python index, wanglandau.py:175-180); here both are refused up front.
// (the stream is idle: the enthalpies of the initial trace are there)
static int wl_check_window(smolmc_handle *h) {
    if (!is_wl(h)) return 0;
    const size_t R = h->R;
    std::vector<double> H0(R);
    HIPCHK(hipMemcpy(H0.data(), h->kp.enthalpy, R * 8, hipMemcpyDeviceToHost));
    std::vector<WlWindow> win; // (per-walker windows: the window the walker holds)
    TRY(wl_windows_download(h, win));
    for (size_t r = 0; r < R; ++r) {
        const double wmin = win.empty() ? h->cfg.wl_min_enthalpy : win[r].vmin, wmax = win.empty() ? h->cfg.wl_max_enthalpy : win[r].vmax;
        if (!(H0[r] >= wmin && H0[r] < wmax)) {
            char msg[240];
            snprintf(msg, sizeof msg,
                     "initial enthalpy %.6f of walker %zu is outside the Wang-Landau window "
                     "[min_enthalpy, max_enthalpy) = [%.6f, %.6f)%s",
                     H0[r], r, wmin, wmax, win.empty() ? "" : " the walker holds (smolmc_set_wl_windows)");
            return fail(msg);
        }
    }
    return 0;
}

extern "C" int smolmc_set_state(smolmc_handle *h, const int32_t *occ, const uint64_t *seeds,
                                const double *temperature, int reset_aux) {
    if (!h || !occ) return fail("null argument");
    HIPCHK(hipSetDevice(h->device));
    KParams &kp = h->kp;
    const size_t R = h->R;
    std::vector<int32_t> occ_engine;
    occ = occ_in(h, occ, R, occ_engine);
    TRY(upload_occ(h, occ, R, kp.occ));
    TRY(apply_temperatures(h, temperature));
    TRY(reset_counters(h, seeds, reset_aux));
    if (kp.bias_type) {
        std::vector<double> b0, q0;
        initial_bias(h, occ, b0, q0);
        HIPCHK(hipMemcpy(kp.bias, b0.data(), R * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(kp.charge, q0.data(), q0.size() * 8, hipMemcpyHostToDevice));
    }
    TRY(init_ewald_field(h));
    TRY(initial_trace(h));
    if (reset_aux) TRY(wl_reset(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    TRY(wl_check_window(h));
    if (h->dist) return smolmc_dist_after_set_state(h, temperature);
    return 0;
}

extern "C" int smolmc_set_temperature(smolmc_handle *h, const double *temperature) {
    if (!h || !temperature) return fail("null argument");
    if (h->dist) return smolmc_dist_set_temperature(h, temperature);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return apply_temperatures(h, temperature);
}

extern "C" int smolmc_sync(smolmc_handle *h) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int smolmc_kernel_info(const smolmc_handle *h, char *buf, int n) {
    if (!h || !buf || n <= 0) return fail("null argument");
    if (h->dist) return smolmc_dist_kernel_info(h, buf, n);
    const LeanFamilyRow *row = h->lean() ? &lean_families[h->family - K_LEAN] : nullptr;
    if (h->univ()) {
        // the layout (univ_lds_layout) and the instantiation (smolmc_univ_selector) of the handle's launches
        const int sel = smolmc_univ_selector(h, h->up);
        char cells[24];
        if (h->up.dfeat_cells) snprintf(cells, sizeof(cells), "dshift=%d", h->up.dfeat_shift);
        else snprintf(cells, sizeof(cells), "dcells=0");
        snprintf(buf, (size_t)n, "universal occ=%s field=%d lds=%zu wpb=%d %s dict=%d k1=%d table=%d dense=%d (%s)",
                 h->up.occ_lds ? "lds" : "hbm", h->kp.ew_field, (size_t)h->up.lds_shared + (size_t)h->up.lds_per_wave * h->univ_wpb,
                 h->univ_wpb, cells, (sel & UNIV_SEL_DICT) ? 1 : 0, (sel & UNIV_SEL_K1) ? 1 : 0, (sel & UNIV_SEL_TABLE) ? 1 : 0,
                 (sel & UNIV_SEL_DENSE) ? 1 : 0, h->general_ok ? "TableFlip outside the lean families" : h->general_reason.c_str());
    } else if (row) {
        snprintf(buf, (size_t)n, "%s nslot=%d mm=%d field=%d lds=%zu%s", row->name,
                 h->lean_nslot, h->lean_mm, h->lp.ew_field, h->lean_lds,
                 h->lean_solo ? (h->lean_occ ? " solo=1 occ=6" : " solo=1") : (h->lean_kf ? " kf=1" : ""));
        // (the solo rows variants; not while per-walker chemical potentials keep the handle on the plain solo kernel)
        if (h->family == K_LEAN && h->solo_rows && !h->lp.mu_stride && strlen(buf) + 12 < (size_t)n)
            snprintf(buf + strlen(buf), (size_t)n - strlen(buf), " rows=%d", h->solo_rows);
    }
    else
        snprintf(buf, (size_t)n, "general nslot=%d mm=%d field=%d lds=%zu", h->nslot, h->mm, h->kp.ew_field,
                 h->lds_bytes);
    {   // suffixes: the translation-compressed Ewald kernel in use, the Wang-Landau kernel generation
        const size_t used = strlen(buf);
        const bool gx = row && h->lp.ew_field && h->lp.ew_gx && used + 40 < (size_t)n;
        if (gx)
            snprintf(buf + used, (size_t)n - used, " gx=%dx%dx%dx%d", h->ew_gx_blocks, h->ew_gx_dims[0], h->ew_gx_dims[1],
                     h->ew_gx_dims[2]);
        // (mc_wl_kernel's tag gives way to the gx one)
        const char *wl_tag = !row || (gx && h->family == K_WL) ? nullptr : (h->lp.wl.sum_mode ? row->wl_sums : row->wl_means);
        if (wl_tag && strlen(buf) + 24 < (size_t)n) strncat(buf, wl_tag, (size_t)n - strlen(buf) - 1);
        if (is_lazy(h) && strlen(buf) + 16 < (size_t)n) strncat(buf, " lazy-features", (size_t)n - strlen(buf) - 1);
        if (h->relabelled && strlen(buf) + 16 < (size_t)n) strncat(buf, " relabelled=1", (size_t)n - strlen(buf) - 1);
        if (!h->walker_mu.empty() && strlen(buf) + 48 < (size_t)n) // (the largest |mu| over all walkers: what the float32 accept bound was widened by)
            snprintf(buf + strlen(buf), (size_t)n - strlen(buf), " walker_mu=1 mu_max=%.17g", h->mu_max);
        if (h->lp.wl.win_off && strlen(buf) + 16 < (size_t)n) strncat(buf, " wl_windows=1", (size_t)n - strlen(buf) - 1);
        if (h->env_dispatch && strlen(buf) + 8 < (size_t)n) { // the dispatch switches this handle was created under
            strncat(buf, " env=", (size_t)n - strlen(buf) - 1);
            const char *sep = "";
            for (int e = 0; e < ENV_COUNT; ++e)
                if (h->env_dispatch >> e & 1u) {
                    strncat(buf, sep, (size_t)n - strlen(buf) - 1);
                    strncat(buf, smolmc_env_switches[e].name, (size_t)n - strlen(buf) - 1);
                    sep = ",";
                }
        }
        // why the model runs neither lean family (the first condition that failed at smolmc_create)
        if (!h->lean() && !h->lean_reason.empty() && strlen(buf) + h->lean_reason.size() + 16 < (size_t)n) {
            strncat(buf, " | not lean: ", (size_t)n - strlen(buf) - 1);
            strncat(buf, h->lean_reason.c_str(), (size_t)n - strlen(buf) - 1);
        }
    }
    return 0;
}

extern "C" int smolmc_get_bias(smolmc_handle *h, double *bias) {
    if (!h || !bias) return fail("null argument");
    if (!h->kp.bias_type) return fail("the model has no bias term");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(bias, h->kp.bias, (size_t)h->R * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_get_state(smolmc_handle *h, int32_t *occ, double *features, double *enthalpy,
                                uint64_t *n_accepted, uint64_t *n_steps, uint8_t *last_accepted) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t R = h->R;
    KParams &kp = h->kp;
    if (occ) {
        DevScratch d32;
        const size_t total = R * h->N;
        TRY(d32.alloc(total * 4));
        hipLaunchKernelGGL(unpack_occ_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           h->stream, kp.occ, d32.as<int>(), h->N, h->Npad, total);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(occ, d32.p, total * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        occ_out(h, occ, R);
    }
    if (features) {
        TRY(ensure_features(h));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(features, kp.features, R * h->F * 8, hipMemcpyDeviceToHost));
    }
    if (enthalpy) HIPCHK(hipMemcpy(enthalpy, kp.enthalpy, R * 8, hipMemcpyDeviceToHost));
    if (n_accepted) HIPCHK(hipMemcpy(n_accepted, kp.nacc, R * 8, hipMemcpyDeviceToHost));
    if (n_steps) HIPCHK(hipMemcpy(n_steps, kp.nsteps, R * 8, hipMemcpyDeviceToHost));
    if (last_accepted) HIPCHK(hipMemcpy(last_accepted, kp.last_acc, R, hipMemcpyDeviceToHost));
    return 0;
}

// bring kp.wl_meanf into the representation the next consumer expects (see WlParams::sum_mode)
static int wl_set_representation(smolmc_handle *h, bool sums) {
    if (h->cfg.kernel_type != SMOLMC_KERNEL_WANGLANDAU || h->wl_sums == sums) return 0;
    const size_t cells = (size_t)h->R * h->L, n = cells * h->F;
    hipLaunchKernelGGL(wl_meanf_convert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                       h->kp.wl_meanf, h->kp.wl_occur, cells, h->F, sums ? 0 : 1);
    HIPCHK(hipGetLastError());
    h->wl_sums = sums;
    return 0;
}

extern "C" int smolmc_get_wl(smolmc_handle *h, double *entropy, int64_t *histogram,
                             int64_t *occurrences, double *mean_features, double *mod_factor) {
    if (!h) return fail("null handle");
    if (h->cfg.kernel_type != SMOLMC_KERNEL_WANGLANDAU) return fail("handle is not a Wang-Landau kernel");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t RL = (size_t)h->R * h->L;
    KParams &kp = h->kp;
    TRY(wl_set_representation(h, false));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (entropy) HIPCHK(hipMemcpy(entropy, kp.wl_entropy, RL * 8, hipMemcpyDeviceToHost));
    if (histogram) HIPCHK(hipMemcpy(histogram, kp.wl_hist, RL * 8, hipMemcpyDeviceToHost));
    if (occurrences) HIPCHK(hipMemcpy(occurrences, kp.wl_occur, RL * 8, hipMemcpyDeviceToHost));
    if (mean_features)
        HIPCHK(hipMemcpy(mean_features, kp.wl_meanf, RL * h->F * 8, hipMemcpyDeviceToHost));
    if (mod_factor) HIPCHK(hipMemcpy(mod_factor, kp.wl_m, (size_t)h->R * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_set_wl(smolmc_handle *h, const double *entropy, const int64_t *histogram,
                             const int64_t *occurrences, const double *mean_features, const double *mod_factor) {
    if (!h) return fail("null handle");
    if (h->cfg.kernel_type != SMOLMC_KERNEL_WANGLANDAU) return fail("handle is not a Wang-Landau kernel");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t RL = (size_t)h->R * h->L;
    KParams &kp = h->kp;
    // occurrences and mean features belong together: bring the device copy to running MEANS (what
    // the caller holds) before either is replaced
    TRY(wl_set_representation(h, false));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (mod_factor)
        for (int r = 0; r < h->R; ++r)
            if (!(mod_factor[r] > 0)) return fail("mod_factor must be greater than 0.");
    if (entropy) HIPCHK(hipMemcpy(kp.wl_entropy, entropy, RL * 8, hipMemcpyHostToDevice));
    if (histogram) HIPCHK(hipMemcpy(kp.wl_hist, histogram, RL * 8, hipMemcpyHostToDevice));
    if (occurrences) HIPCHK(hipMemcpy(kp.wl_occur, occurrences, RL * 8, hipMemcpyHostToDevice));
    if (mean_features) HIPCHK(hipMemcpy(kp.wl_meanf, mean_features, RL * h->F * 8, hipMemcpyHostToDevice));
    if (mod_factor) HIPCHK(hipMemcpy(kp.wl_m, mod_factor, (size_t)h->R * 8, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int smolmc_set_counters(smolmc_handle *h, const uint64_t *n_steps, const uint64_t *n_accepted) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    KParams &kp = h->kp;
    const size_t R = (size_t)h->R;
    if (n_steps) {
        HIPCHK(hipMemcpy(kp.nsteps, n_steps, R * 8, hipMemcpyHostToDevice));
        if (h->cfg.kernel_type == SMOLMC_KERNEL_WANGLANDAU) // the check period counts the same steps
            HIPCHK(hipMemcpy(kp.wl_counter, n_steps, R * 8, hipMemcpyHostToDevice));
    }
    if (n_accepted) HIPCHK(hipMemcpy(kp.nacc, n_accepted, R * 8, hipMemcpyHostToDevice));
    return 0;
}

// ---- kernel dispatch (instantiations live in general_n*.hip / lean_n*.hip) --------------
static int launch_mc(smolmc_handle *h, const KParams &kp, int replay) {
    switch (h->nslot) {
    case 2: return smolmc_launch_general_2(h, kp, replay);
    case 4: return smolmc_launch_general_4(h, kp, replay);
    case 8: return smolmc_launch_general_8(h, kp, replay);
    default: return smolmc_launch_general_16(h, kp, replay);
    }
}

// Launch-slot -> walker permutation for launches whose walkers differ in cost.  On an exchange ladder
// a hot walker accepts several times as many steps as a cold one and an accepted TableFlip step
// costs several rejected ones (field sweep, stale marking); a launch ends with its slowest SIMD,
// and a SIMD hosts one wave of each of the two workgroups resident on its CU.  Slots are therefore
// dealt so that the hottest walker shares its SIMD with the coldest, the second hottest with the
// second coldest, ...: every SIMD gets about the same work.  mode 1 (SMOLMC_WALKER_ORDER, default):
// the partner of a workgroup is the one half a grid later (workgroups are dealt round-robin over
// the CUs, the second half of the grid lands on the CUs of the first); mode 2: the next workgroup;
// 0: slot q runs walker q.  Ranks by beta ascending (hottest first), ties by walker index; built on
// the host whenever the temperatures changed (one 8 B-per-walker read-back per exchange sweep).
static int update_walker_order(smolmc_handle *h, LeanParams &lp) {
    const char *env = smolmc_env(ENV_WALKER_ORDER); // (read at every launch: tests switch it)
    const int mode = env ? atoi(env) : 1;
    if (mode != h->order_mode) h->order_dirty = true;
    h->order_mode = mode;
    lp.order = nullptr;
    const int R = h->R, wpb = h->lean_wpb;
    if (mode == 0 || h->cfg.step_type != SMOLMC_STEP_TABLE_FLIP || h->lean_multi() || R < 2 * wpb) return 0;
    if (!h->d_order) {
        HIPCHK(hipMalloc((void **)&h->d_order, (size_t)R * sizeof(int)));
        h->allocs.push_back(h->d_order);
        h->order_dirty = true;
    }
    if (h->order_dirty) {
        std::vector<double> beta(R);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(beta.data(), h->d_beta, (size_t)R * 8, hipMemcpyDeviceToHost));
        std::vector<int> by_rank(R), order(R);
        for (int i = 0; i < R; ++i) by_rank[i] = i;
        std::stable_sort(by_rank.begin(), by_rank.end(), [&](int a, int b) { return beta[a] < beta[b]; }); // hottest first
        const int nb = (R + wpb - 1) / wpb;
        for (int q = 0; q < R; ++q) {
            int rho;
            if (wpb == 8) {  // partner of wave w of a workgroup: wave w + 4 of the same workgroup (R % 8 == 0)
                const int k = (q >> 3) * 4 + (q & 3);
                rho = (q & 4) ? R - 1 - k : k;
            } else if (mode == 1) { // partner of workgroup b: workgroup b + nb / 2
                const int half = (nb / 2) * wpb;
                rho = q < half ? q : (q < 2 * half ? R - 1 - (q - half) : q - half);
            } else {         // partner of workgroup 2 p: workgroup 2 p + 1
                const int b = q / wpb, w = q % wpb, k = (b >> 1) * wpb + w;
                const bool paired = (b | 1) < nb;
                rho = !paired ? (nb / 2) * wpb + w : ((b & 1) ? R - 1 - k : k);
            }
            order[q] = by_rank[rho];
        }
        { // (a permutation by construction; a slip here would run a walker twice and another not at all)
            std::vector<char> seen(R, 0);
            for (int q = 0; q < R; ++q) {
                if (order[q] < 0 || order[q] >= R || seen[order[q]]) return fail("internal: walker order is not a permutation");
                seen[order[q]] = 1;
            }
        }
        HIPCHK(hipMemcpy(h->d_order, order.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice));
        h->order_dirty = false;
    }
    lp.order = h->d_order;
    return 0;
}

static int launch_lean(smolmc_handle *h, LeanParams lp, int64_t nsteps) {
    lp.steps = nsteps;
    TRY(update_walker_order(h, lp));
    const LeanLauncher launch = lean_launcher(h, false);
    if (!launch) return fail("internal: no kernel of this family takes per-walker chemical potentials"); // (smolmc_set_walker_mu refuses those)
    return launch(h, lp);
}

static void free_samples(smolmc_handle *h) {
    for (SampleSlot &sl : h->slots) {
        if (sl.copy_done) { hipEventSynchronize(sl.copy_done); hipEventDestroy(sl.copy_done); }
        if (sl.kernel_done) hipEventDestroy(sl.kernel_done);
        if (sl.d) hipFree(sl.d);
        if (sl.hst) hipHostFree(sl.hst);
        sl = SampleSlot();
    }
    if (h->copy_stream) { hipStreamDestroy(h->copy_stream); h->copy_stream = nullptr; }
}

// parameter block of a universal-kernel launch: the handle's current KParams; on a lean handle (a
// replay the lean kernels cannot take) the potential field is used exactly when the lean kernel
// maintains it
static UParams univ_block_of(smolmc_handle *h) {
    UParams up = h->up;
    up.K = h->kp;
    if (h->lean() && !h->lp.ew_field) up.K.ew_field = 0;
    return up;
}

static int run_steps(smolmc_handle *h, int64_t nsteps, const SampleBufs &smp) {
    if (h->dist) return smolmc_dist_run(h, nsteps, smp);
    // (per-bin feature statistics as sums for the lean Wang-Landau kernel and for mc_kernel with
    // update_period 1, as running means for the universal kernel)
    TRY(wl_set_representation(h, h->univ() ? false : (h->lean() ? h->lp.wl.sum_mode != 0 : h->kp.wl_sum_mode != 0)));
    if (h->univ()) {
        UParams up = univ_block_of(h);
        up.K.steps_to_run = nsteps;
        up.K.smp = smp;
        return smolmc_launch_univ(h, up, 0);
    }
    if (h->lean()) {
        // the lean kernels count steps in 32 bits: launches are split at 2^30 steps (on a
        // sample boundary when samples are being recorded)
        int64_t chunk = (int64_t)1 << 30;
        const char *chunk_env = smolmc_env(ENV_LAUNCH_CHUNK); // test hook
        if (chunk_env) chunk = std::max<int64_t>(1, atoll(chunk_env));
        if (smp.every) {
            if (smp.every > chunk) {
                if (chunk_env) chunk = smp.every;
                else return fail("thin_by must be <= 2^30 steps");
            }
            chunk -= chunk % smp.every;
        }
        int64_t done = 0;
        while (done < nsteps) {
            const int64_t n = std::min(chunk, nsteps - done);
            LeanParams lp = h->lp;
            lp.smp = smp;
            if (smp.every) {
                const size_t rows = (size_t)(done / smp.every) * h->R;
                lp.smp.H += rows;
                lp.smp.feat += rows * (size_t)lp.F; // (lazy cluster features: rows of the scalar features)
                lp.smp.acc += rows;
                if (lp.smp.occ) lp.smp.occ += rows * h->Npad;
            }
            if (int rc = launch_lean(h, lp, n)) return rc;
            done += n;
        }
        if (is_lazy(h)) h->ce_dirty = true;
        return 0;
    }
    KParams kp = h->kp;
    kp.steps_to_run = nsteps;
    kp.smp = smp;
    return launch_mc(h, kp, 0);
}

extern "C" int smolmc_run(smolmc_handle *h, int64_t nsteps) {
    if (!h) return fail("null handle");
    if (nsteps < 0) return fail("nsteps must be non-negative");
    if (nsteps == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    SampleBufs none;
    memset(&none, 0, sizeof(none));
    return run_steps(h, nsteps, none);
}

// ---- device-side sampling: a ring of two slots with asynchronous download ---------
// One sample of every walker from the handle's state arrays into row j of a slot -- for the kernels that do
// not record in-kernel (Wang-Landau: the per-walker L and L x F arrays; MCBias: the running bias): the
// block is then a sequence { launch of thin_by steps; this snapshot } queued on the stream, no host round trip.
struct SnapshotArgs {
    const uint8_t *occ; const double *features, *enthalpy; const uint8_t *last_acc; const double *bias;
    const double *wl_S; const long long *wl_hist, *wl_occ; const double *wl_mf, *wl_m;
    uint8_t *o_occ; double *o_feat, *o_H; uint8_t *o_acc; double *o_bias;
    double *o_wlS; long long *o_wlh, *o_wlo; double *o_wlf, *o_wlm;
    int R, F, L, Npad, mf_is_sums;
};
__global__ void __launch_bounds__(256) sample_snapshot_kernel(const SnapshotArgs A, long long j) {
    const int r = blockIdx.x, t = threadIdx.x;
    const size_t row = (size_t)j * A.R + r;
    if (A.o_occ) {
        const uint32_t *src = (const uint32_t *)(A.occ + (size_t)r * A.Npad);
        uint32_t *dst = (uint32_t *)(A.o_occ + row * A.Npad);
        for (int i = t; i < A.Npad / 4; i += 256) dst[i] = src[i];
    }
    for (int i = t; i < A.F; i += 256) A.o_feat[row * A.F + i] = A.features[(size_t)r * A.F + i];
    if (t == 0) {
        A.o_H[row] = A.enthalpy[r];
        A.o_acc[row] = A.last_acc[r];
        if (A.o_bias) A.o_bias[row] = A.bias[r];
        if (A.o_wlm) A.o_wlm[row] = A.wl_m[r];
    }
    if (A.o_wlS) {
        const size_t src = (size_t)r * A.L, dst = row * A.L;
        for (int i = t; i < A.L; i += 256) {
            A.o_wlS[dst + i] = A.wl_S[src + i];
            A.o_wlh[dst + i] = A.wl_hist[src + i];
            A.o_wlo[dst + i] = A.wl_occ[src + i];
        }
        // (mean = sum / occurrences where the kernel keeps per-bin SUMS, see wl_meanf_convert_kernel)
        for (size_t i = t; i < (size_t)A.L * A.F; i += 256) {
            double v = A.wl_mf[src * A.F + i];
            if (A.mf_is_sums) {
                const long long n = A.wl_occ[src + i / A.F];
                if (n > 0) v /= (double)n;
            }
            A.o_wlf[dst * A.F + i] = v;
        }
    }
}

// Which derived columns exist for a set of SMOLMC_SAMPLE_* flags, and which record reads which: the one place that knows.
// A quantity exists when its own flag asks for it or a record reads it; every reader reads the same column (the statistics
// record the counts the observables' flag or the minima record asked for, else its own).
struct ColumnUse {
    bool min_counts, stat_counts, stat_inten, stat_conn, stat_pat, stat_env; // what the records read
    bool stat_sites;                                        // the record's site field reads the occupancy rows
    bool counts, pairs, sfac, conn, pat, env;               // what is derived: kind counts, pair counts (with the observables' flag
                                                         // only), amplitudes with intensities, connectivity stats, pattern cells
};
static ColumnUse column_use(const smolmc_handle *h, int flags) {
    const bool minima = (flags & SMOLMC_SAMPLE_MINIMA) != 0, stats = (flags & SMOLMC_SAMPLE_STATISTICS) != 0;
    ColumnUse u;
    u.min_counts = minima && h->obs.K && h->obs.K == h->minima.K; // (a keyed record: always, see smolmc_set_observables)
    u.stat_counts = stats && h->stats.n_count_cols > 0;           // (then obs.K == stats.K, see smolmc_set_observables)
    u.stat_inten = stats && h->stats.n_inten_cols > 0;            // (then sfac.I == stats.I, see smolmc_set_structure)
    u.stat_conn = stats && h->stats.n_conn_cols > 0;              // (then 24 conn.G == stats.CS, see smolmc_set_connectivity)
    u.pairs = (flags & SMOLMC_SAMPLE_OBSERVABLES) != 0;
    u.counts = u.pairs || u.min_counts || u.stat_counts;
    u.sfac = (flags & SMOLMC_SAMPLE_STRUCTURE) || u.stat_inten;
    u.conn = (flags & SMOLMC_SAMPLE_CONNECTIVITY) || u.stat_conn;
    u.stat_pat = stats && h->stats.n_pat_cols > 0;                // (then obs.pat.n_cells == stats.PC, see smolmc_set_patterns)
    u.pat = (flags & SMOLMC_SAMPLE_PATTERNS) || u.stat_pat;
    u.stat_env = stats && h->stats.n_env_cols > 0;                // (then obs.env.n_cells == stats.EC, see smolmc_set_environments)
    u.env = (flags & SMOLMC_SAMPLE_ENVIRONMENTS) || u.stat_env;
    u.stat_sites = stats && h->stats.site_S > 0;                  // (smolmc_set_statistics_sites)
    return u;
}

// `rows` = nsamples x R rows on the device and where what is derived from them goes: a block of the ring, or the walkers'
// own states with the scratch of smolmc_update_minima / smolmc_update_statistics.  An output column_use does not ask for is
// not read.
struct RowSources {
    size_t rows = 0;
    const double *H = nullptr, *feat = nullptr;
    const uint8_t *occ = nullptr;                     // rows of Npad bytes
    int32_t *counts = nullptr, *pairs = nullptr;
    long long *amp = nullptr;
    double *inten = nullptr;
    long long *conn = nullptr;
    int32_t *pat = nullptr;
    int32_t *env = nullptr;
    uint64_t *min_key = nullptr;                      // scratch of the minima reduction [rows]
    int32_t *min_slot = nullptr;
};
static RowSources walker_rows(const smolmc_handle *h) {
    RowSources s;
    s.rows = (size_t)h->R;
    s.H = h->kp.enthalpy; s.feat = h->kp.features; s.occ = h->kp.occ;
    return s;
}
// the derived columns of the rows, in one fixed order, then the offers to the records `flags` names; all on the handle's stream
static int derive_and_offer(smolmc_handle *h, const RowSources &s, int flags, long long nsamples, long long thin_by) {
    const ColumnUse u = column_use(h, flags);
    if (u.counts || u.pat || u.env) // (one launch stages the rows for kind counts, pair counts, pattern and environment cells)
        TRY(smolmc_obs_launch(h, s.occ, s.rows, u.counts ? s.counts : nullptr, u.pairs ? s.pairs : nullptr, u.pat ? s.pat : nullptr,
                              u.env ? s.env : nullptr, nullptr));
    if (u.sfac) TRY(smolmc_sfac_launch(h, s.occ, s.rows, s.amp, s.inten));
    if (u.conn) TRY(smolmc_conn_launch(h, s.occ, s.rows, s.conn, nullptr));
    if (flags & SMOLMC_SAMPLE_MINIMA)
        TRY(smolmc_min_launch(h, s.H, s.feat, s.occ, u.min_counts ? s.counts : nullptr, s.min_key, s.min_slot, nsamples, thin_by));
    if (flags & SMOLMC_SAMPLE_STATISTICS)
        TRY(smolmc_stat_launch(h, s.H, s.feat, u.stat_counts ? s.counts : nullptr, u.stat_inten ? s.inten : nullptr,
                               u.stat_conn ? s.conn : nullptr, u.stat_pat ? s.pat : nullptr, u.stat_env ? s.env : nullptr, nsamples,
                               u.stat_sites ? s.occ : nullptr));
    return 0;
}

// One block of smolmc_run_sampled: its columns in the slot's arenas and how its rows are recorded.
struct BlockPlan {
    size_t rows = 0;
    SampleColumns col;      // every column the block has, downloaded or not
    bool occ = false;       // occupancy rows are kept (at col.o_occ)
    size_t o_scal = 0, o_min_key = 0, o_min_slot = 0; // never downloaded: the scalar features of lazy rows, the minima scratch
    size_t download = 0, total = 0;                    // bytes in front of the download mark, bytes in all
    // Biased Metropolis handles on the lean families record their rows in-kernel like the unbiased ones (round 6: the
    // running bias is a scalar the kernel carries anyway; LeanParams::smp_bias_off tells it where the column is).  The
    // snapshot path -- one launch + one snapshot kernel per sample -- is left to Wang-Landau (per-walker L and L x F
    // arrays) and to biased handles on mc_kernel / the universal kernel.  SMOLMC_NO_INKERNEL_BIAS: A/B switch.
    // Lazy cluster features, rows recorded in-kernel: the kernels write rows of scalar features and the occupancy of
    // every sample; the cluster features of the rows are evaluated from those when the launch is through.
    bool snapshot = false;  // the snapshot path; else the kernels record the rows themselves ...
    bool bias_rows = false; // ... with the bias column
    bool lazy_rows = false; // ... as rows of scalar features (at o_scal)
};
// Pure host arithmetic: nothing is allocated or launched.  A column lies in front of the download mark exactly when its own
// SMOLMC_SAMPLE_* flag is set; what a derived column or a record needs and the caller did not ask for lies behind it.
static int plan_block(const smolmc_handle *h, int64_t nsamples, int flags, BlockPlan &p) {
    const size_t rows = (size_t)nsamples * h->R, F = (size_t)h->F, L = (size_t)h->L;
    const ColumnUse u = column_use(h, flags);
    p.bias_rows = (flags & SMOLMC_SAMPLE_BIAS) && !(flags & SMOLMC_SAMPLE_WL) && h->lean() && !h->univ() && h->lp.bias_type &&
                  !smolmc_env(ENV_NO_INKERNEL_BIAS);
    p.snapshot = (flags & SMOLMC_SAMPLE_WL) || ((flags & SMOLMC_SAMPLE_BIAS) && !p.bias_rows);
    p.lazy_rows = is_lazy(h) && !p.snapshot;
    const struct { bool applies; const char *noun; } too_many[] = {
        {(flags & SMOLMC_SAMPLE_MINIMA) != 0, "minima"},          {(flags & SMOLMC_SAMPLE_STATISTICS) != 0, "statistics"},
        {(flags & SMOLMC_SAMPLE_CONNECTIVITY) != 0, "connectivity"}, {(flags & SMOLMC_SAMPLE_STRUCTURE) != 0, "structure factors"},
        {p.lazy_rows, "lazy cluster features"},                     {(flags & SMOLMC_SAMPLE_OBSERVABLES) != 0, "observables"},
        {(flags & SMOLMC_SAMPLE_PATTERNS) != 0, "patterns"},      {(flags & SMOLMC_SAMPLE_ENVIRONMENTS) != 0, "environments"}};
    for (const auto &t : too_many)
        if (t.applies && rows > 0x7fffffffull) return fail(std::string(t.noun) + ": more than 2^31 sample rows in one block");
    p.rows = rows;
    p.occ = (flags & SMOLMC_SAMPLE_OCCUPANCY) || p.lazy_rows || u.counts || u.sfac || u.conn || u.pat || u.env ||
            (flags & SMOLMC_SAMPLE_MINIMA) || u.stat_sites;
    const size_t sf_amp = (size_t)h->sfac.Q * h->sfac.K * 2 * 8, sf_inten = (size_t)h->sfac.I * 8; // bytes per row
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
    SampleColumns &c = p.col;
    c.o_H = take(rows * 8);
    c.o_feat = take(rows * F * 8);
    c.o_acc = take(rows);
    if (flags & SMOLMC_SAMPLE_BIAS) c.o_bias = take(rows * 8);
    if (flags & SMOLMC_SAMPLE_WL) {
        c.o_wlm = take(rows * 8);
        c.o_wlS = take(rows * L * 8);
        c.o_wlh = take(rows * L * 8);
        c.o_wlo = take(rows * L * 8);
        c.o_wlf = take(rows * L * F * 8);
    }
    // the columns with a flag of their own: first those whose flag is set, then, behind the download mark, the others
    for (int hidden = 0; hidden < 2; ++hidden) {
        auto here = [&](int flag) { return ((flags & flag) != 0) != (hidden != 0); };
        if (p.occ && here(SMOLMC_SAMPLE_OCCUPANCY)) c.o_occ = take(rows * h->Npad);
        if (u.counts && here(SMOLMC_SAMPLE_OBSERVABLES)) c.o_cnt = take(rows * (size_t)h->obs.K * 4);
        if (u.pairs && !hidden) c.o_pair = take(rows * h->obs.cells * 4);
        if (u.sfac && here(SMOLMC_SAMPLE_STRUCTURE)) {
            c.o_amp = take(rows * sf_amp);
            c.o_inten = take(rows * sf_inten);
        }
        if (u.conn && here(SMOLMC_SAMPLE_CONNECTIVITY)) c.o_conn = take(rows * (size_t)h->conn.G * SMOLMC_CONN_STATS * 8);
        if (u.pat && here(SMOLMC_SAMPLE_PATTERNS)) c.o_pat = take(rows * h->obs.pat.n_cells * 4);
        if (u.env && here(SMOLMC_SAMPLE_ENVIRONMENTS)) c.o_env = take(rows * h->obs.env.n_cells * 4);
        if (!hidden) p.download = at;
    }
    if (p.lazy_rows) p.o_scal = take(rows * (size_t)std::max(1, lazy_nscal(h)) * 8);
    if (flags & SMOLMC_SAMPLE_MINIMA) {
        p.o_min_key = take(rows * 8);
        p.o_min_slot = take(rows * 4);
    }
    p.total = at;
    return 0;
}

// what the flags ask of the handle
static int sampled_check_flags(const smolmc_handle *h, int64_t thin_by, int flags) {
    if ((flags & SMOLMC_SAMPLE_BIAS) && !h->kp.bias_type) return fail("the model has no bias term");
    if ((flags & SMOLMC_SAMPLE_WL) && !is_wl(h)) return fail("handle is not a Wang-Landau kernel");
    if ((flags & SMOLMC_SAMPLE_OBSERVABLES) && !h->obs.K)
        return fail("SMOLMC_SAMPLE_OBSERVABLES without observables: call smolmc_set_observables first");
    if ((flags & SMOLMC_SAMPLE_MINIMA) && !h->minima.n_slots)
        return fail("SMOLMC_SAMPLE_MINIMA without a minima record: call smolmc_set_minima first");
    if ((flags & SMOLMC_SAMPLE_STATISTICS) && !h->stats.n_keys)
        return fail("SMOLMC_SAMPLE_STATISTICS without a statistics record: call smolmc_set_statistics first");
    if ((flags & SMOLMC_SAMPLE_STRUCTURE) && !h->sfac.Q)
        return fail("SMOLMC_SAMPLE_STRUCTURE without a structure-factor spec: call smolmc_set_structure first");
    if ((flags & SMOLMC_SAMPLE_CONNECTIVITY) && !h->conn.G)
        return fail("SMOLMC_SAMPLE_CONNECTIVITY without a connectivity spec: call smolmc_set_connectivity first");
    if ((flags & SMOLMC_SAMPLE_PATTERNS) && !h->obs.pat.n_sets)
        return fail("SMOLMC_SAMPLE_PATTERNS without a pattern spec: call smolmc_set_patterns first");
    if ((flags & SMOLMC_SAMPLE_ENVIRONMENTS) && !h->obs.env.n_sets)
        return fail("SMOLMC_SAMPLE_ENVIRONMENTS without an environment spec: call smolmc_set_environments first");
    if ((flags & SMOLMC_SAMPLE_WL) && !h->wl_win_min.empty())
        return fail("SMOLMC_SAMPLE_WL while per-walker windows are set: the snapshot rows are walker-indexed, the Wang-Landau arrays estimator-indexed (smolmc_get_wl between runs, or smolmc_set_wl_windows(h, NULL, NULL) first)");
    if (thin_by > ((int64_t)1 << 30) && h->lean() && !smolmc_env(ENV_LAUNCH_CHUNK))
        return fail("thin_by must be <= 2^30 steps"); // (before a slot is touched: run_steps would refuse it)
    return 0;
}

// The slot the next block goes to is the older one.  When it still holds a block nobody fetched, so does the other
// (it is younger): the ring is full and the call is refused -- ABI 7 dropped the older block here without a word.
static int sampled_next_slot(smolmc_handle *h, SampleSlot **out) {
    if (!h->copy_stream) HIPCHK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    SampleSlot &sl = h->slots[h->next_slot];
    if (sl.state == 1) {
        fail("sample ring full: both slots hold blocks that were not fetched (call smolmc_get_samples* or "
             "smolmc_discard_samples first)");
        return SMOLMC_ERR_RING_FULL;
    }
    if (!sl.kernel_done) {
        HIPCHK(hipEventCreateWithFlags(&sl.kernel_done, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&sl.copy_done, hipEventDisableTiming));
    }
    *out = &sl;
    return 0;
}

// the slot's arenas free for `bytes` of a new block
static int sampled_reserve(SampleSlot &sl, SampleSlot &w, size_t bytes) {
    // the slot's previous block (delivered, or none) must have left the device before its arenas are reused
    if (sl.state != 0) HIPCHK(hipEventSynchronize(sl.copy_done));
    if (bytes <= sl.cap) return 0;
    // (growing frees the delivered block's mirror: the slot is empty from here on, whatever happens next)
    sl.state = 0;
    if (sl.d) hipFree(sl.d);
    if (sl.hst) hipHostFree(sl.hst);
    sl.d = sl.hst = nullptr;
    sl.cap = 0;
    HIPCHK(hipMalloc((void **)&sl.d, bytes));
    if (hipHostMalloc((void **)&sl.hst, bytes, hipHostMallocDefault) != hipSuccess) {
        hipFree(sl.d);
        sl.d = nullptr;
        return fail("hipHostMalloc failed (pinned mirror of the sample ring)");
    }
    sl.cap = bytes;
    w.d = sl.d; w.hst = sl.hst; w.cap = sl.cap;
    return 0;
}

// the rows of the block into the arena `d`: enthalpy, features, accepted flags, the columns of the bias and Wang-Landau
// flags and, where the plan keeps them, the occupancy rows
static int sampled_record(smolmc_handle *h, unsigned char *d, const BlockPlan &p, int64_t nsamples, int64_t thin_by, int flags) {
    const SampleColumns &c = p.col;
    SampleBufs smp;
    memset(&smp, 0, sizeof(smp));
    smp.every = thin_by;
    smp.H = (double *)(d + c.o_H);
    smp.feat = (double *)(d + (p.lazy_rows ? p.o_scal : c.o_feat));
    smp.acc = d + c.o_acc;
    smp.occ = p.occ ? d + c.o_occ : nullptr;
    if (!p.snapshot) {
        if (p.bias_rows) {
            if ((c.o_bias - c.o_H) / 8 > 0xffffffffull) return fail("sample block too large for the in-kernel bias column");
            h->lp.smp_bias_off = (uint32_t)((c.o_bias - c.o_H) / 8);
        }
        const int rc_run = run_steps(h, nsamples * thin_by, smp); // the kernels record the rows themselves, one launch
        h->lp.smp_bias_off = 0;
        if (rc_run) return rc_run;
        if (p.lazy_rows) {
            TRY(launch_eval_full(h, d + c.o_occ, (int)p.rows, (double *)(d + c.o_feat), 1));
            TRY(lazy_scalars(h, (double *)(d + c.o_feat), (double *)(d + p.o_scal), p.rows, 0));
        }
        return 0;
    }
    SampleBufs none;
    memset(&none, 0, sizeof(none));
    KParams &kp = h->kp;
    SnapshotArgs A;
    memset(&A, 0, sizeof(A));
    A.occ = kp.occ; A.features = kp.features; A.enthalpy = kp.enthalpy; A.last_acc = kp.last_acc; A.bias = kp.bias;
    A.wl_S = kp.wl_entropy; A.wl_hist = kp.wl_hist; A.wl_occ = kp.wl_occur; A.wl_mf = kp.wl_meanf; A.wl_m = kp.wl_m;
    A.o_occ = smp.occ; A.o_feat = smp.feat; A.o_H = smp.H; A.o_acc = smp.acc;
    A.o_bias = (flags & SMOLMC_SAMPLE_BIAS) ? (double *)(d + c.o_bias) : nullptr;
    if (flags & SMOLMC_SAMPLE_WL) {
        A.o_wlm = (double *)(d + c.o_wlm); A.o_wlS = (double *)(d + c.o_wlS);
        A.o_wlh = (long long *)(d + c.o_wlh); A.o_wlo = (long long *)(d + c.o_wlo);
        A.o_wlf = (double *)(d + c.o_wlf);
    }
    A.R = h->R; A.F = h->F; A.L = h->L; A.Npad = h->Npad;
    for (int64_t j = 0; j < nsamples; ++j) {
        TRY(run_steps(h, thin_by, none));
        TRY(ensure_features(h)); // (lazy cluster features: the snapshot reads kp.features)
        A.mf_is_sums = h->wl_sums ? 1 : 0; // (the representation the launch left the per-bin statistics in)
        hipLaunchKernelGGL(sample_snapshot_kernel, dim3((unsigned)h->R), dim3(256), 0, h->stream, A, (long long)j);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// the rows of a recorded block as the consumers read them
static RowSources block_rows(unsigned char *d, const BlockPlan &p) {
    const SampleColumns &c = p.col;
    RowSources s;
    s.rows = p.rows;
    s.H = (const double *)(d + c.o_H); s.feat = (const double *)(d + c.o_feat); s.occ = d + c.o_occ;
    s.counts = (int32_t *)(d + c.o_cnt); s.pairs = (int32_t *)(d + c.o_pair);
    s.amp = (long long *)(d + c.o_amp); s.inten = (double *)(d + c.o_inten); s.conn = (long long *)(d + c.o_conn);
    s.pat = (int32_t *)(d + c.o_pat);
    s.env = (int32_t *)(d + c.o_env);
    s.min_key = (uint64_t *)(d + p.o_min_key); s.min_slot = (int32_t *)(d + p.o_min_slot);
    return s;
}

// download on the copy stream as soon as the block is complete; the next block's launches do not wait for it
static int sampled_publish(smolmc_handle *h, SampleSlot &sl, SampleSlot &w) {
    // (the mirror is about to be overwritten: from here the slot no longer holds its old block)
    sl.state = 0;
    HIPCHK(hipEventRecord(sl.kernel_done, h->stream));
    HIPCHK(hipStreamWaitEvent(h->copy_stream, sl.kernel_done, 0));
    HIPCHK(hipMemcpyAsync(sl.hst, sl.d, w.used, hipMemcpyDeviceToHost, h->copy_stream));
    HIPCHK(hipEventRecord(sl.copy_done, h->copy_stream));
    // (the next writer of this slot's arenas -- the call after next -- waits for copy_done above)
    // every launch is queued: the block takes the slot
    w.state = 1;
    w.seq = ++h->slot_seq;
    sl = w;
    h->next_slot ^= 1;
    return 0;
}

extern "C" int smolmc_run_sampled(smolmc_handle *h, int64_t nsamples, int64_t thin_by, int flags) {
    if (!h) return fail("null handle");
    if (nsamples <= 0 || thin_by <= 0) return fail("nsamples and thin_by must be positive");
    HIPCHK(hipSetDevice(h->device));
    TRY(sampled_check_flags(h, thin_by, flags));
    SampleSlot *sl;
    TRY(sampled_next_slot(h, &sl));
    BlockPlan p;
    TRY(plan_block(h, nsamples, flags, p));
    // the block is laid out on a COPY of the slot record, which replaces the record only when every launch of the block
    // has been queued -- a call that fails on the way (an allocation, a launch) leaves the ring as it was: the slot keeps
    // its delivered block, next_slot does not move
    SampleSlot w = *sl;
    TRY(sampled_reserve(*sl, w, p.total));
    static_cast<SampleColumns &>(w) = p.col;
    w.used = p.download;
    w.n = nsamples;
    w.flags = flags;
    TRY(sampled_record(h, sl->d, p, nsamples, thin_by, flags));
    TRY(derive_and_offer(h, block_rows(sl->d, p), flags, nsamples, thin_by));
    return sampled_publish(h, *sl, w);
}

// The block the next smolmc_get_samples* call delivers (ABI 8): its sample count and flags, so that a caller can size
// its arrays from the ring itself -- get_samples takes no lengths -- and the number of blocks queued and not fetched.
static SampleSlot *next_delivery(smolmc_handle *h) {
    SampleSlot *sl = nullptr;
    for (SampleSlot &c : h->slots)
        if (c.state == 1 && (!sl || c.seq < sl->seq)) sl = &c;
    if (!sl)
        for (SampleSlot &c : h->slots)
            if (c.state == 2 && (!sl || c.seq > sl->seq)) sl = &c;
    return sl;
}
// bytes of the block the next smolmc_get_samples* call delivers that its download moves (-1: none); a test hook like
// smolmc_debug_relabel, not part of the C-ABI
extern "C" long long smolmc_debug_block_bytes(smolmc_handle *h) {
    const SampleSlot *sl = h ? next_delivery(h) : nullptr;
    return sl ? (long long)sl->used : -1;
}
extern "C" int smolmc_pending_samples(smolmc_handle *h, int *n_pending, int64_t *nsamples, int *flags) {
    if (!h) return fail("null handle");
    int np = 0;
    for (SampleSlot &c : h->slots) np += c.state == 1;
    const SampleSlot *sl = next_delivery(h);
    if (n_pending) *n_pending = np;
    if (nsamples) *nsamples = sl ? (int64_t)sl->n : 0;
    if (flags) *flags = sl ? sl->flags : 0;
    return 0;
}
// Forget every block of the ring, fetched or not (a sampling loop that was abandoned half way: the blocks it queued
// must not be delivered to the next one).  The walkers keep the state the queued launches leave them in.
extern "C" int smolmc_discard_samples(smolmc_handle *h) {
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->device));
    for (SampleSlot &c : h->slots) {
        if (c.state != 0 && c.copy_done) HIPCHK(hipEventSynchronize(c.copy_done));
        c.state = 0;
    }
    return 0;
}

// host side of a delivery: pinned mirror -> the caller's arrays, a few threads for the big ones (the copy of a
// block overlaps the kernel of the next one as long as it is shorter)
void smolmc_host_copy(void *dst, const void *src, size_t bytes) {
    const size_t big = (size_t)8 << 20;
    if (bytes < big) { memcpy(dst, src, bytes); return; }
    const int nt = 4;
    std::thread th[nt];
    const size_t part = (bytes / nt + 63) & ~(size_t)63;
    for (int k = 0; k < nt; ++k) {
        const size_t a = std::min(bytes, part * k), b = std::min(bytes, part * (k + 1));
        th[k] = std::thread([=]() { memcpy((char *)dst + a, (const char *)src + a, b - a); });
    }
    for (int k = 0; k < nt; ++k) th[k].join();
}
// occupancy rows: Npad bytes apart in the ring, N bytes (uint8) or N int32 in the caller's array
// (new_of != nullptr: a relabelled handle -- column p of the caller's row is byte new_of[p] of the ring's)
template <typename T> static void host_copy_occ(T *dst, const uint8_t *src, size_t rows, int N, int Npad, const int32_t *new_of) {
    auto work = [=](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; ++r) {
            const uint8_t *s = src + r * Npad;
            T *d = dst + r * (size_t)N;
            if (new_of) for (int i = 0; i < N; ++i) d[i] = (T)s[new_of[i]];
            else if (sizeof(T) == 1) memcpy(d, s, (size_t)N);
            else for (int i = 0; i < N; ++i) d[i] = (T)s[i];
        }
    };
    if (rows * (size_t)N < ((size_t)8 << 20)) { work(0, rows); return; }
    const int nt = 4;
    std::thread th[nt];
    for (int k = 0; k < nt; ++k) th[k] = std::thread(work, rows * k / nt, rows * (k + 1) / nt);
    for (int k = 0; k < nt; ++k) th[k].join();
}

static int get_samples_impl(smolmc_handle *h, double *enthalpy, double *features, uint8_t *accepted,
                            int32_t *occ32, uint8_t *occ8, double *bias, double *wl_S, int64_t *wl_hist,
                            int64_t *wl_occ, double *wl_mf, double *wl_m) {
    if (!h) return fail("null handle");
    // the oldest block not yet delivered; with none pending, the newest delivered one again
    SampleSlot *sl = next_delivery(h);
    if (!sl) return fail("no samples recorded: call smolmc_run_sampled first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(sl->copy_done));
    const size_t rows = (size_t)sl->n * h->R, F = (size_t)h->F, L = (size_t)h->L;
    if ((occ32 || occ8) && !(sl->flags & SMOLMC_SAMPLE_OCCUPANCY)) return fail("occupancies were not recorded (flags bit 0)");
    if (bias && !(sl->flags & SMOLMC_SAMPLE_BIAS)) return fail("the bias was not recorded (flags bit 1)");
    if ((wl_S || wl_hist || wl_occ || wl_mf || wl_m) && !(sl->flags & SMOLMC_SAMPLE_WL))
        return fail("the Wang-Landau trace was not recorded (flags bit 2)");
    if (enthalpy) smolmc_host_copy(enthalpy, sl->hst + sl->o_H, rows * 8);
    if (features) smolmc_host_copy(features, sl->hst + sl->o_feat, rows * F * 8);
    if (accepted) smolmc_host_copy(accepted, sl->hst + sl->o_acc, rows);
    if (bias) smolmc_host_copy(bias, sl->hst + sl->o_bias, rows * 8);
    if (wl_m) smolmc_host_copy(wl_m, sl->hst + sl->o_wlm, rows * 8);
    if (wl_S) smolmc_host_copy(wl_S, sl->hst + sl->o_wlS, rows * L * 8);
    if (wl_hist) smolmc_host_copy(wl_hist, sl->hst + sl->o_wlh, rows * L * 8);
    if (wl_occ) smolmc_host_copy(wl_occ, sl->hst + sl->o_wlo, rows * L * 8);
    if (wl_mf) smolmc_host_copy(wl_mf, sl->hst + sl->o_wlf, rows * L * F * 8);
    const int32_t *new_of = h->relabelled ? h->new_of.data() : nullptr;
    if (occ8) host_copy_occ<uint8_t>(occ8, sl->hst + sl->o_occ, rows, h->N, h->Npad, new_of);
    if (occ32) host_copy_occ<int32_t>(occ32, sl->hst + sl->o_occ, rows, h->N, h->Npad, new_of);
    sl->state = 2;
    return 0;
}
extern "C" int smolmc_get_samples(smolmc_handle *h, double *enthalpy, double *features,
                                  uint8_t *accepted, int32_t *occupancy) {
    return get_samples_impl(h, enthalpy, features, accepted, occupancy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}
extern "C" int smolmc_get_samples_u8(smolmc_handle *h, double *enthalpy, double *features,
                                     uint8_t *accepted, uint8_t *occupancy) {
    return get_samples_impl(h, enthalpy, features, accepted, nullptr, occupancy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}
extern "C" int smolmc_get_samples_ex(smolmc_handle *h, double *enthalpy, double *features, uint8_t *accepted,
                                     uint8_t *occupancy_u8, double *bias, double *wl_entropy, int64_t *wl_histogram,
                                     int64_t *wl_occurrences, double *wl_mean_features, double *wl_mod_factor) {
    return get_samples_impl(h, enthalpy, features, accepted, nullptr, occupancy_u8, bias, wl_entropy, wl_histogram,
                            wl_occurrences, wl_mean_features, wl_mod_factor);
}

// lean replay kernels that exist: the replay entries of lean_families
static bool smolmc_lean_replay_takes(const smolmc_handle *h) { return lean_launcher(h, true) != nullptr; }
static int smolmc_launch_lean_replay(smolmc_handle *h, LeanParams lp) {
    TRY(update_walker_order(h, lp)); // (a permutation for the TableFlip kernels only)
    return lean_launcher(h, true)(h, lp);
}

// ---- smolmc_replay in stages: scan the records, choose the route, stage, launch, read back ------------------------------
struct ReplayFacts {
    int max_flips = 0;          // flips of the longest record
    bool repeated_site = false; // a record that flips one site twice (sequential-flip semantics, expansion.py:217-229)
    bool priori_given = false;  // a factor the Flip / Swap kernels do not model (replay_priori_given)
};
// one pass over the records.  Every flip: a changeable site of an active sublattice (the lean kernels index their
// tables relative to the active range; a code beyond the site's species would index past its tensors)
static int replay_scan(const smolmc_handle *h, const int32_t *steps, size_t n, ReplayFacts &f) {
    for (size_t i = 0; i < n; ++i) {
        const int32_t *st = steps + i * SMOLMC_STEP_ROW;
        int nf = 0;
        for (; nf < SMOLMC_MAX_STEP_FLIPS && st[2 * nf] >= 0; ++nf) {
            const int32_t site = st[2 * nf], code = st[2 * nf + 1];
            if (site >= h->N) return fail("replay step out of range");
            if (!h->site_active[site]) return fail("replay step out of range: the site is not changeable (not on an active sublattice)");
            if (code < 0 || code >= (int)h->site_ncodes[site]) return fail("replay step out of range (species code)");
            for (int g = 0; g < nf; ++g) f.repeated_site |= st[2 * g] == site;
        }
        f.max_flips = std::max(f.max_flips, nf);
    }
    return 0;
}
// ... and over the a-priori factors (behind the distance hand-over: a distance handle has its own refusal): NaN asks
// the kernel to derive the factor, 0 is what the Flip / Swap ushers give
static bool replay_priori_given(const double *log_priori, size_t n) {
    if (log_priori)
        for (size_t i = 0; i < n; ++i)
            if (log_priori[i] == log_priori[i] && log_priori[i] != 0.0) return true;
    return false;
}

// Which kernel replays the records: a function of the handle, the scan's facts, nsteps and the two environment
// switches (SMOLMC_REPLAY_GENERAL, SMOLMC_REPLAY_UNIVERSAL) only.
// Lean handles replay on their own kernels (REPLAY instantiations of mc_lean_kernel,
// mc_lean_multi_kernel, mc_wl_kernel, mc_table_kernel, mc_table_multi_kernel); steps those cannot
// take (more than two flips on a Flip / Swap handle, a given a-priori factor there), universal
// handles and SMOLMC_REPLAY_UNIVERSAL take the universal kernel; SMOLMC_REPLAY_GENERAL: mc_kernel.
enum ReplayRoute { ROUTE_LEAN, ROUTE_LEAN_TABLE, ROUTE_GENERAL, ROUTE_UNIVERSAL };
static const char *const replay_route_names[] = {"lean", "lean-table", "general", "universal"};
static ReplayRoute replay_route(const smolmc_handle *h, const ReplayFacts &f, int64_t nsteps, bool env_general, bool env_universal) {
    // what the two-flip kernels (the Flip / Swap lean kernels, mc_kernel) take
    const bool two_flip_ok = f.max_flips <= 2 && !f.priori_given && !is_table(h);
    // (a biased or Wang-Landau TableFlip handle has no REPLAY instantiation: the universal kernel replays its records)
    if (h->lean() && !env_universal && nsteps < ((int64_t)1 << 30) && smolmc_lean_replay_takes(h)) {
        // (the lean TableFlip replay kernels pick sites without replacement like the usher: a record with a repeated
        // site -- valid for the boundary -- takes the universal kernel, which evaluates it flip by flip;
        // SMOLMC_REPLAY_GENERAL is ignored: mc_kernel takes no table steps)
        if (is_table(h)) {
            if (!f.repeated_site) return ROUTE_LEAN_TABLE;
        }
        // (a Flip handle's own kernel takes single flips: records of two flips go to mc_kernel / the universal kernel)
        else if (two_flip_ok && !(env_general && h->general_ok) && (h->cfg.step_type != SMOLMC_STEP_FLIP || f.max_flips <= 1))
            return ROUTE_LEAN;
    }
    if (!h->univ() && two_flip_ok && h->general_ok && !env_universal) return ROUTE_GENERAL;
    return ROUTE_UNIVERSAL;
}

int ReplayStage::upload(size_t n, const int32_t *steps_host, const double *uniforms, bool narrow, bool priori, const double *log_priori) {
    // the two-flip kernels read records of four ints
    std::vector<int32_t> packed;
    if (narrow) {
        packed.resize(n * 4);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 4; ++k) packed[i * 4 + k] = steps_host[i * SMOLMC_STEP_ROW + k];
    }
    const size_t row_bytes = narrow ? 16 : SMOLMC_STEP_ROW * 4;
    TRY(steps.alloc(n * row_bytes));
    if (priori) TRY(err.alloc(16, true));
    TRY(u.alloc(n * 8));
    TRY(H.alloc(n * 8));
    TRY(acc.alloc(n));
    if (priori) TRY(lp_out.alloc(n * 8, true));
    if (priori && log_priori) {
        TRY(lp_in.alloc(n * 8));
        HIPCHK(hipMemcpy(lp_in.p, log_priori, n * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(steps.p, narrow ? packed.data() : steps_host, n * row_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(u.p, uniforms, n * 8, hipMemcpyHostToDevice));
    return 0;
}

// the handle's own REPLAY kernel (ROUTE_LEAN, ROUTE_LEAN_TABLE)
static int replay_on_lean(smolmc_handle *h, int64_t nsteps, const ReplayStage &st) {
    TRY(wl_set_representation(h, is_wl(h) && h->lp.wl.sum_mode));
    LeanParams lp = h->lp;
    memset(&lp.smp, 0, sizeof(lp.smp));
    lp.steps = nsteps;
    lp.rp_steps = st.steps.as<int>(); lp.rp_u = st.u.as<double>(); lp.rp_acc = st.acc.as<uint8_t>(); lp.rp_H = st.H.as<double>();
    lp.rp_err = st.err.as<int>(); lp.rp_lp = st.lp_in.as<double>(); lp.rp_lp_out = st.lp_out.as<double>();
    if (is_lazy(h)) h->ce_dirty = true;
    return smolmc_launch_lean_replay(h, lp);
}
// mc_kernel (ROUTE_GENERAL)
static int replay_on_general(smolmc_handle *h, int64_t nsteps, const ReplayStage &st) {
    TRY(wl_set_representation(h, h->kp.wl_sum_mode != 0));
    TRY(ensure_features(h)); // (mc_kernel updates the features incrementally)
    KParams kp = h->kp;
    kp.steps_to_run = nsteps;
    kp.rp_steps = st.steps.as<int>(); kp.rp_u = st.u.as<double>(); kp.rp_acc = st.acc.as<uint8_t>(); kp.rp_H = st.H.as<double>();
    TRY(launch_mc(h, kp, 1));
    return lazy_scalars_from_features(h);
}
// the universal kernel (ROUTE_UNIVERSAL)
static int replay_on_universal(smolmc_handle *h, int64_t nsteps, const ReplayStage &st) {
    TRY(wl_set_representation(h, false));
    TRY(ensure_features(h)); // (the universal kernel updates the features incrementally)
    UParams up = univ_block_of(h);
    up.K.steps_to_run = nsteps;
    memset(&up.K.smp, 0, sizeof(up.K.smp));
    up.K.rp_steps = st.steps.as<int>(); up.K.rp_u = st.u.as<double>(); up.K.rp_acc = st.acc.as<uint8_t>(); up.K.rp_H = st.H.as<double>();
    up.rp_lp = st.lp_in.as<double>(); up.rp_lp_out = st.lp_out.as<double>(); up.rp_err = st.err.as<int>();
    TRY(smolmc_launch_univ(h, up, 1));
    return lazy_scalars_from_features(h);
}

static const char *const replay_not_in_table =
    "replay: Step is not in flip table (neither a canonical swap nor +-(a row of flip_table)); "
    "the walkers have been advanced -- set the state again";
static const char *const replay_wrong_shape =
    "replay step does not fit the handle's step type (a swap handle takes proper swaps: "
    "code1 == species at site2, code2 == species at site1; a flip handle single flips); "
    "the walkers have been advanced -- set the state again";
// the kernel has finished: its error word (mc_kernel writes none) as a refusal, else the outputs
static int replay_finish(ReplayRoute route, const ReplayStage &st, size_t n, uint8_t *accepted_out, double *enthalpy_out,
                         double *log_priori_out) {
    if (route != ROUTE_GENERAL) {
        int bad = 0;
        HIPCHK(hipMemcpy(&bad, st.err.p, 4, hipMemcpyDeviceToHost));
        if (bad) return fail(route == ROUTE_LEAN ? replay_wrong_shape : replay_not_in_table);
    }
    if (accepted_out) HIPCHK(hipMemcpy(accepted_out, st.acc.p, n, hipMemcpyDeviceToHost));
    if (enthalpy_out) HIPCHK(hipMemcpy(enthalpy_out, st.H.p, n * 8, hipMemcpyDeviceToHost));
    if (log_priori_out) HIPCHK(hipMemcpy(log_priori_out, st.lp_out.p, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_replay(smolmc_handle *h, int64_t nsteps, const int32_t *steps, const double *uniforms,
                             const double *log_priori, uint8_t *accepted_out, double *enthalpy_out,
                             double *log_priori_out) {
    if (!h || !steps || !uniforms) return fail("null argument");
    if (!h->walker_mu.empty()) return fail("smolmc_replay while per-walker chemical potentials are set: the replay kernels price every walker with the handle's own table (smolmc_set_walker_mu(h, NULL) first)");
    if (!h->wl_win_min.empty()) return fail("smolmc_replay while per-walker windows are set: the replay kernels give every walker the config's window (smolmc_set_wl_windows(h, NULL, NULL) first)");
    if (nsteps <= 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->R * nsteps;
    std::vector<int32_t> steps_engine;
    steps = steps_in(h, steps, n, steps_engine);
    ReplayFacts facts;
    TRY(replay_scan(h, steps, n, facts));
    if (h->dist) return smolmc_dist_replay(h, nsteps, steps, uniforms, log_priori, accepted_out, enthalpy_out, log_priori_out);
    facts.priori_given = replay_priori_given(log_priori, n);
    const ReplayRoute route = replay_route(h, facts, nsteps, smolmc_env(ENV_REPLAY_GENERAL) != nullptr,
                                           smolmc_env(ENV_REPLAY_UNIVERSAL) != nullptr);
    if (smolmc_env(ENV_DEBUG))
        fprintf(stderr, "[smolmc] replay path=%s max_flips=%d priori_given=%d\n", replay_route_names[route], facts.max_flips,
                (int)facts.priori_given);
    ReplayStage st; // (freed on every way out; hipFree waits for the kernel)
    TRY(st.upload(n, steps, uniforms, route == ROUTE_LEAN || route == ROUTE_GENERAL, true, log_priori));
    switch (route) {
    case ROUTE_LEAN:
    case ROUTE_LEAN_TABLE: TRY(replay_on_lean(h, nsteps, st)); break;
    case ROUTE_GENERAL: TRY(replay_on_general(h, nsteps, st)); break;
    case ROUTE_UNIVERSAL: TRY(replay_on_universal(h, nsteps, st)); break;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return replay_finish(route, st, n, accepted_out, enthalpy_out, log_priori_out);
}

extern "C" int smolmc_last_kernel_ms(smolmc_handle *h, float *ms) {
    if (!h || !ms) return fail("null argument");
    if (!h->timed) return fail("no kernel has been launched yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return 0;
}

static int ensure_eval_occ(smolmc_handle *h, size_t nocc) {
    const size_t need = nocc * h->Npad;
    if (need > h->eval_occ_cap) {
        if (h->d_eval_occ) hipFree(h->d_eval_occ);
        h->d_eval_occ = nullptr;
        h->eval_occ_cap = 0;
        HIPCHK(hipMalloc((void **)&h->d_eval_occ, need));
        h->eval_occ_cap = need;
    }
    return 0;
}

extern "C" int smolmc_eval_full(smolmc_handle *h, const int32_t *occ, int nocc, double *features) {
    if (!h || !occ || !features) return fail("null argument");
    if (nocc <= 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    TRY(ensure_eval_occ(h, nocc));
    std::vector<int32_t> occ_engine;
    occ = occ_in(h, occ, (size_t)nocc, occ_engine);
    TRY(upload_occ(h, occ, nocc, h->d_eval_occ));
    DevScratch d_out;
    TRY(d_out.alloc((size_t)nocc * h->F * 8));
    TRY(launch_eval_full(h, h->d_eval_occ, nocc, d_out.as<double>()));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(features, d_out.p, (size_t)nocc * h->F * 8, hipMemcpyDeviceToHost));
    if (h->dist) return smolmc_dist_from_extensive(h, features, (size_t)nocc);
    return 0;
}

// ---- shared by the host code of the specs that read occupancy rows (observables.hip, structure.hip, connectivity.hip) ----
int smolmc_ring_guard(const smolmc_handle *h, int flag, const char *fn, const char *flag_name) {
    for (const SampleSlot &c : h->slots)
        if (c.state == 1 && (c.flags & flag))
            return fail(std::string(fn) + " while a block recorded with " + flag_name +
                        " waits in the ring (call smolmc_get_samples* or smolmc_discard_samples first)");
    return 0;
}

int smolmc_ring_forget(smolmc_handle *h, int flag) {
    HIPCHK(hipStreamSynchronize(h->stream));
    for (SampleSlot &c : h->slots)
        if (c.state == 2 && (c.flags & flag)) c.state = 0;
    return 0;
}

int smolmc_kind_base_in(const smolmc_handle *h, const int32_t *kind_base, int K, const char *noun, std::vector<int32_t> &kb,
                        size_t *n_counted) {
    kb.assign((size_t)h->N, 0);
    size_t counted = 0;
    for (int p = 0; p < h->N; ++p) {
        const int s = h->relabelled ? h->new_of[p] : p;
        const int32_t b = kind_base[p];
        // (a fixed site outside every cluster: the tables do not say how many codes it has, site_ncodes is the
        // model's widest site there -- its block must hold one kind at least; the kernels leave out a kind >= K)
        const int width = h->site_width_known[s] ? (int)h->site_ncodes[s] : 1;
        if (b >= 0 && b + width > K) {
            char msg[256];
            snprintf(msg, sizeof msg, "%s: kind_base[%d] + site_ncodes = %d + %d is larger than n_kinds = %d: kind out of range", noun, p,
                     (int)b, width, K);
            return fail(msg);
        }
        kb[s] = b < 0 ? -1 : b;
        counted += b >= 0;
    }
    if (n_counted) *n_counted = counted;
    return 0;
}

int smolmc_eval_rows(smolmc_handle *h, const int32_t *occ, int nocc, const std::vector<int32_t> &kind_base, int K, const char *noun,
                     const uint8_t **d_occ8, size_t *rows) {
    *d_occ8 = h->kp.occ;
    *rows = (size_t)h->R;
    if (!occ) return 0;
    *rows = 0;
    if (nocc <= 0) return 0;
    TRY(ensure_eval_occ(h, nocc));
    std::vector<int32_t> occ_engine;
    occ = occ_in(h, occ, (size_t)nocc, occ_engine);
    for (size_t r = 0; r < (size_t)nocc; ++r)
        for (int s = 0; s < h->N; ++s) {
            const int32_t b = kind_base[s], c = occ[r * h->N + s];
            if (b >= 0 && c >= 0 && b + c >= K) {
                char msg[256];
                snprintf(msg, sizeof msg, "%s: occupancy code %d on site %d gives kind %d, n_kinds = %d: kind out of range", noun, (int)c,
                         h->relabelled ? (int)h->old_of[s] : s, (int)(b + c), K);
                return fail(msg);
            }
        }
    TRY(upload_occ(h, occ, nocc, h->d_eval_occ));
    *d_occ8 = h->d_eval_occ;
    *rows = (size_t)nocc;
    return 0;
}

int smolmc_sample_block(smolmc_handle *h, int flag, const char *not_recorded, const SampleSlot **sl, size_t *rows) {
    if (!h) return fail("null handle");
    *sl = next_delivery(h);
    if (!*sl) return fail("no samples recorded: call smolmc_run_sampled first");
    if (!((*sl)->flags & flag)) return fail(not_recorded);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize((*sl)->copy_done));
    *rows = (size_t)(*sl)->n * h->R;
    return 0;
}

// one offer of the walkers' current states to the minima record (minima.hip): what a caller of smolmc_run does where
// smolmc_run_sampled offers the rows of its block
extern "C" int smolmc_update_minima(smolmc_handle *h) {
    if (!h) return fail("null handle");
    SmolmcMin &M = h->minima;
    if (!M.n_slots) return fail("no minima record set: call smolmc_set_minima first");
    HIPCHK(hipSetDevice(h->device));
    TRY(ensure_features(h));
    RowSources s = walker_rows(h);
    s.counts = M.u_counts; s.min_key = M.u_key; s.min_slot = M.u_slot;
    return derive_and_offer(h, s, SMOLMC_SAMPLE_MINIMA, 1, 1);
}

// one offer of the walkers' current states to the statistics record (statistics.hip), as smolmc_update_minima
extern "C" int smolmc_update_statistics(smolmc_handle *h) {
    if (!h) return fail("null handle");
    SmolmcStat &S = h->stats;
    if (!S.n_keys) return fail("no statistics record set: call smolmc_set_statistics first");
    HIPCHK(hipSetDevice(h->device));
    TRY(ensure_features(h));
    RowSources s = walker_rows(h);
    s.counts = S.u_counts; s.amp = h->sfac.u_amp; s.inten = h->sfac.u_inten; s.conn = h->conn.u_stats;
    s.pat = h->obs.pat.u_cells;
    s.env = h->obs.env.u_cells;
    return derive_and_offer(h, s, SMOLMC_SAMPLE_STATISTICS, 1, 1);
}

extern "C" int smolmc_eval_delta(smolmc_handle *h, const int32_t *occ, const int32_t *flips, int nstep,
                                 double *dfeatures) {
    if (!h || !occ || !flips || !dfeatures) return fail("null argument");
    if (nstep <= 0) return 0;
    if (h->dist) return smolmc_dist_eval_delta(h, occ, flips, nstep, dfeatures);
    HIPCHK(hipSetDevice(h->device));
    std::vector<int32_t> occ_engine, flips_engine;
    occ = occ_in(h, occ, 1, occ_engine);
    flips = steps_in(h, flips, (size_t)nstep, flips_engine);
    for (int i = 0; i < nstep; ++i)
        for (int f = 0; f < SMOLMC_MAX_STEP_FLIPS; ++f) {
            const int s = flips[(size_t)i * SMOLMC_STEP_ROW + 2 * f], c = flips[(size_t)i * SMOLMC_STEP_ROW + 2 * f + 1];
            if (s < 0) break;
            if (s >= h->N || c < 0 || c >= (int)h->site_ncodes[s]) return fail("flip out of range");
        }
    TRY(ensure_eval_occ(h, 1));
    TRY(upload_occ(h, occ, 1, h->d_eval_occ));
    DevScratch d_fl, d_out;
    TRY(d_fl.alloc((size_t)nstep * SMOLMC_STEP_ROW * 4));
    TRY(d_out.alloc((size_t)nstep * h->F * 8));
    HIPCHK(hipMemcpy(d_fl.p, flips, (size_t)nstep * SMOLMC_STEP_ROW * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_delta_kernel, dim3(nstep), dim3(64), 0, h->stream, h->rt, h->d_eval_occ,
                       d_fl.as<int>(), d_out.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(dfeatures, d_out.p, (size_t)nstep * h->F * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int smolmc_export_enthalpy_dev(smolmc_handle *h, double *dst_dev) {
    if (!h || !dst_dev) return fail("null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(dst_dev, h->kp.enthalpy, (size_t)h->R * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

__global__ void beta_from_T_kernel(const double *T, double *beta, int R, double kB) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) beta[r] = 1.0 / (kB * T[r]);
}

// One exchange attempt of a temperature ladder decided on the device: the serial section of the N-rank config-5 loop
// (host NumPy over the all-gathered enthalpies until round 5: parallel.ReplicaExchange.decide).  One workgroup; the
// rung -> walker map lives in LDS.  Every operation is the NumPy path's own (beta = 1 / (kB T), the product of the two
// differences, the comparison with the host-made log u): the same decisions bit for bit.
__global__ void __launch_bounds__(1024) rex_decide_kernel(const int n, const int first, const int parity, const double *H,
                                                          const double *ladder, const double *log_u, int *rung_of,
                                                          long long *stats, double *beta_out, const int R, const double kB) {
    extern __shared__ int walker_at[]; // [n] rung -> walker
    for (int g = threadIdx.x; g < n; g += blockDim.x) walker_at[rung_of[g]] = g;
    __syncthreads();
    const int npairs = (n - 1 - parity + 1) / 2; // pairs (k, k + 1), k = parity, parity + 2, ... < n - 1
    for (int p = threadIdx.x; p < npairs; p += blockDim.x) {
        const int k = parity + 2 * p;
        const int a = walker_at[k], b = walker_at[k + 1];
        const double bk = 1.0 / (kB * ladder[k]), bk1 = 1.0 / (kB * ladder[k + 1]);
        const double expo = (bk - bk1) * (H[a] - H[b]);
        const bool acc = expo >= 0.0 || log_u[p] < expo;
        if (stats) {
            stats[k] += 1;                          // attempted
            if (acc) stats[(n - 1) + k] += 1;       // accepted
        }
        if (acc) { rung_of[a] = k + 1; rung_of[b] = k; } // (the pairs of one parity are disjoint)
    }
    __threadfence_block();
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += blockDim.x) beta_out[r] = 1.0 / (kB * ladder[rung_of[first + r]]);
}

extern "C" int smolmc_exchange_dev(smolmc_handle *h, int n_total, int first, int parity, const double *enthalpy_all_dev,
                                   const double *ladder_dev, const double *log_u_dev, int32_t *rung_of_dev,
                                   int64_t *stats_dev) {
    if (!h || !enthalpy_all_dev || !ladder_dev || !log_u_dev || !rung_of_dev) return fail("null argument");
    if (h->dist) return fail("a distance handle takes no replica exchange (its temperatures use the handle's kB)");
    if (!h->walker_mu.empty()) return fail("smolmc_exchange_dev while per-walker chemical potentials are set: an exchange of temperatures alone is no valid move between walkers of different Hamiltonians");
    if (n_total < 2 || n_total > 16384) return fail("exchange ladder must hold 2 .. 16384 walkers (the rung map lives in LDS)");
    if (first < 0 || first + h->R > n_total) return fail("this handle's walkers are out of range of the ladder");
    if (parity != 0 && parity != 1) return fail("parity must be 0 or 1");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(rex_decide_kernel, dim3(1), dim3(1024), (size_t)n_total * sizeof(int), h->stream, n_total, first, parity,
                       enthalpy_all_dev, ladder_dev, log_u_dev, (int *)rung_of_dev, (long long *)stats_dev, h->d_beta, h->R,
                       SMOLMC_KB);
    HIPCHK(hipGetLastError());
    h->order_dirty = true; // (the launch order of the TableFlip kernels follows the temperatures)
    h->point_T_stale = true;
    return 0;
}

extern "C" int smolmc_import_temperature_dev(smolmc_handle *h, const double *src_dev) {
    if (!h || !src_dev) return fail("null argument");
    if (h->dist) return fail("a distance handle takes no replica exchange (its temperatures use the handle's kB)");
    if (!h->walker_mu.empty()) return fail("smolmc_import_temperature_dev while per-walker chemical potentials are set: an exchange of temperatures alone is no valid move between walkers of different Hamiltonians");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(beta_from_T_kernel, dim3((h->R + 63) / 64), dim3(64), 0, h->stream, src_dev,
                       h->d_beta, h->R, SMOLMC_KB);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->order_dirty = true;
    h->point_T_stale = true;
    return 0;
}

// ---- exchange across the mu-T grid (hyper-parallel tempering) ------------------------------------------------------
// The walkers at the state points pairs[p][0] and pairs[p][1] attempt to swap their points -- temperature and row of
// chemical potentials together, the valid move between walkers of different Hamiltonians -- decided and applied by
// grid_exchange_kernel (grid_exchange.hip; the formula is spelled out there).  A permutation leaves the largest |mu|
// over all rows alone: fast_eps and mu_max stay.  A handle without rows exchanges temperatures only.
static int grid_exchange_refused(const smolmc_handle *h, const char *what) {
    TRY(walker_mu_refused(h, what));
    if (h->point_T_stale || h->point_T.size() != (size_t)h->R)
        return fail(std::string(what) + ": the state points have no temperatures (smolmc_set_state or smolmc_set_temperature names them; "
                    "smolmc_exchange_dev and smolmc_import_temperature_dev move temperatures without naming points)");
    return 0;
}

extern "C" int smolmc_exchange_grid(smolmc_handle *h, int npairs, const int32_t *pairs, const double *log_u, int64_t *stats) {
    if (!h) return fail("null handle");
    TRY(grid_exchange_refused(h, "smolmc_exchange_grid"));
    TRY(pair_exchange_check(h, "smolmc_exchange_grid", "state point", npairs, pairs, log_u));
    if (npairs == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    if (!h->d_point_of) {
        const int R = h->R;
        std::vector<int32_t> id(R);
        for (int r = 0; r < R; ++r) id[r] = r;
        TRY(dev_alloc(h, (size_t)R, &h->d_point_of));
        TRY(dev_alloc(h, (size_t)R, &h->d_walker_at));
        HIPCHK(hipMemcpy(h->d_point_of, id.data(), (size_t)R * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_walker_at, id.data(), (size_t)R * 4, hipMemcpyHostToDevice));
    }
    PairStage st;
    TRY(pair_exchange_stage(h, npairs, pairs, log_u, st));
    TRY(smolmc_grid_exchange_launch(h, npairs, st.pairs, st.log_u, st.acc, h->d_point_of, h->d_walker_at));
    h->grid_permuted = true;
    h->order_dirty = true;              // (as smolmc_set_temperature: the launch order of the TableFlip kernels follows the temperatures)
    if (is_lazy(h)) h->ce_dirty = true; // (as smolmc_set_walker_mu: kp.features takes its scalar entries from the lean kernels' rows)
    return stats ? pair_exchange_stats(h, npairs, st.acc, stats) : 0;
}

extern "C" int smolmc_get_state_points(smolmc_handle *h, int32_t *point_of, double *temperature) {
    if (!h) return fail("null handle");
    TRY(grid_exchange_refused(h, "smolmc_get_state_points"));
    std::vector<int32_t> po;
    TRY(grid_point_of(h, po));
    for (int r = 0; r < h->R; ++r) {
        if (point_of) point_of[r] = po[r];
        if (temperature) temperature[r] = h->point_T[po[r]];
    }
    return 0;
}

// ---- population annealing: resample and clone walkers on the device (pop_anneal.hip) --------------------------------
// The move is spelled out in pop_anneal.hip and DESIGN 4.14; parallel.PopulationAnnealing is its definition in NumPy.
// It touches nothing but HBM state between launches, so every Metropolis kernel family is served.  (A lazy handle: the
// scalar rows and kp.features move together, and cluster features that were stale before a clone are stale for source and
// copy alike: ce_dirty stays what it was.)
static int resample_refused(const smolmc_handle *h, const char *what) {
    if (h->dist) return fail(std::string(what) + ": a distance handle keeps best records per walker, its walkers are not resampled");
    if (is_wl(h)) return fail(std::string(what) + ": a Wang-Landau handle samples no Boltzmann weight (its walkers build one density of states, no population at a temperature)");
    if (!h->walker_mu.empty()) return fail(std::string(what) + " while per-walker chemical potentials are set: walkers of different Hamiltonians are no population");
    return 0; // (Wang-Landau windows exist on Wang-Landau handles only)
}
static int pop_scratch(smolmc_handle *h) {
    if (h->pop.parent) return 0;
    const size_t R = (size_t)h->R;
    uint64_t *arena = nullptr; // six arrays of 8 bytes, four of 4 bytes per walker; the two words of an adaptive step
    TRY(dev_alloc(h, 8 * R + 2, &arena));
    SmolmcPopScratch &S = h->pop;
    S.q = arena; S.qsum = arena + R; S.word = arena + 2 * R; S.C = arena + 3 * R;
    S.href = (double *)(arena + 4 * R); S.beta_new = (double *)(arena + 5 * R);
    S.cnt = (uint32_t *)(arena + 6 * R); S.sur = S.cnt + R; S.drank = S.cnt + 2 * R;
    S.T_new = (double *)(arena + 8 * R); S.flags = (int32_t *)(arena + 8 * R + 1);
    S.parent = (int32_t *)(S.cnt + 3 * R);
    return 0;
}

extern "C" int smolmc_resample(smolmc_handle *h, const int32_t *parent) {
    if (!h || !parent) return fail("null argument");
    TRY(resample_refused(h, "smolmc_resample"));
    const int R = h->R;
    for (int m = 0; m < R; ++m)
        if (parent[m] < 0 || parent[m] >= R)
            return fail("smolmc_resample: parent " + std::to_string(parent[m]) + " of slot " + std::to_string(m) + " is out of range 0 .. " + std::to_string(R - 1));
    for (int m = 0; m < R; ++m)
        if (parent[parent[m]] != parent[m])
            return fail("smolmc_resample: slot " + std::to_string(parent[m]) + " is a source (of slot " + std::to_string(m) + ") and a destination (of slot " +
                        std::to_string(parent[parent[m]]) + "): every source must map to itself, the copy is in place");
    HIPCHK(hipSetDevice(h->device));
    TRY(pop_scratch(h));
    // (a pageable source: read when hipMemcpyAsync returns, as in smolmc_exchange_grid)
    HIPCHK(hipMemcpyAsync(h->pop.parent, parent, (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
    return smolmc_pop_clone_launch(h, h->pop.parent, 1, nullptr);
}

// what both annealing entries refuse, and the temperatures in force (T_old, R): as named by the latest call that set
// them, or read back where exchanges moved them
static int anneal_refused(smolmc_handle *h, const std::string &what, int npop, std::vector<double> &T_old) {
    TRY(resample_refused(h, what.c_str()));
    const int R = h->R;
    if (npop < 1 || R % npop != 0)
        return fail(what + ": " + std::to_string(npop) + " populations do not divide the " + std::to_string(R) + " walkers (populations are equal blocks of slots: R % npop must be 0)");
    const int n = R / npop;
    if (n > (1 << 22)) return fail(what + ": a population must be no larger than 2^22 walkers (the sum of the weights stays below 2^62)");
    HIPCHK(hipSetDevice(h->device));
    T_old.resize(R);
    if (!h->point_T_stale && !h->grid_permuted && h->point_T.size() == (size_t)R) T_old = h->point_T;
    else {
        std::vector<double> beta(R);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(beta.data(), h->d_beta, (size_t)R * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < R; ++r) T_old[r] = 1.0 / (SMOLMC_KB * beta[r]);
    }
    for (int r = 0; r < R; ++r)
        if (T_old[r] != T_old[(r / n) * n])
            return fail(what + ": the walkers of population " + std::to_string(r / n) + " are at different temperatures (walker " +
                        std::to_string((r / n) * n) + ": " + std::to_string(T_old[(r / n) * n]) + ", walker " + std::to_string(r) + ": " + std::to_string(T_old[r]) +
                        "); a population is reweighted from one temperature");
    return 0;
}
static int anneal_outputs(smolmc_handle *h, int npop, int32_t *parent_out, uint64_t *q_out, uint64_t *qsum_out, double *href_out) {
    const SmolmcPopScratch &S = h->pop;
    if (parent_out) HIPCHK(hipMemcpyAsync(parent_out, S.parent, (size_t)h->R * 4, hipMemcpyDeviceToHost, h->stream));
    if (q_out) HIPCHK(hipMemcpyAsync(q_out, S.q, (size_t)h->R * 8, hipMemcpyDeviceToHost, h->stream));
    if (qsum_out) HIPCHK(hipMemcpyAsync(qsum_out, S.qsum, (size_t)npop * 8, hipMemcpyDeviceToHost, h->stream));
    if (href_out) HIPCHK(hipMemcpyAsync(href_out, S.href, (size_t)npop * 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

extern "C" int smolmc_anneal_resample(smolmc_handle *h, int npop, const double *temperature_new, const uint64_t *offset_word,
                                      int32_t *parent_out, uint64_t *q_out, uint64_t *qsum_out, double *href_out) {
    if (!h || !temperature_new || !offset_word) return fail("null argument");
    std::vector<double> T_old;
    TRY(anneal_refused(h, "smolmc_anneal_resample", npop, T_old));
    const int R = h->R, n = R / npop;
    for (int p = 0; p < npop; ++p)
        if (!(temperature_new[p] > 0.0) || !std::isfinite(temperature_new[p]))
            return fail("smolmc_anneal_resample: the temperature of population " + std::to_string(p) + " must be positive and finite");
    TRY(pop_scratch(h));
    TRY(grid_rebase(h));
    std::vector<double> T_new(R), beta_new(npop);
    for (int r = 0; r < R; ++r) T_new[r] = temperature_new[r / n];
    for (int p = 0; p < npop; ++p) beta_new[p] = 1.0 / (SMOLMC_KB * temperature_new[p]); // (as set_betas)
    const SmolmcPopScratch &S = h->pop;
    HIPCHK(hipMemcpyAsync(S.beta_new, beta_new.data(), (size_t)npop * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(S.word, offset_word, (size_t)npop * 8, hipMemcpyHostToDevice, h->stream));
    TRY(smolmc_pop_parent_launch(h, npop, S, nullptr));
    TRY(smolmc_pop_clone_launch(h, S.parent, npop, S.beta_new));
    grid_name_temperatures(h, T_new.data());
    h->order_dirty = true; // (as smolmc_set_temperature: the launch order of the TableFlip kernels follows the temperatures)
    if (parent_out || q_out || qsum_out || href_out) {
        TRY(anneal_outputs(h, npop, parent_out, q_out, qsum_out, href_out));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// The adaptive step: pop_parent_kernel chooses beta' itself (the largest step towards the limit that keeps the target
// overlap), then resamples; the clone kernel writes beta'.  The call waits: the points are named with the
// temperature that comes back, and the driver stops at `reached`.
extern "C" int smolmc_anneal_adaptive(smolmc_handle *h, int npop, double temperature_limit, uint32_t overlap_target, int n_iter,
                                      const uint64_t *offset_word, double *temperature_out, int32_t *flags_out,
                                      int32_t *parent_out, uint64_t *q_out, uint64_t *qsum_out, double *href_out) {
    if (!h || !offset_word || !temperature_out || !flags_out) return fail("null argument");
    std::vector<double> T_old;
    TRY(anneal_refused(h, "smolmc_anneal_adaptive", npop, T_old));
    if (overlap_target == 0) return fail("smolmc_anneal_adaptive: the overlap target must be positive (the target overlap is overlap_target / 2^32)");
    if (n_iter < 1 || n_iter > 60) return fail("smolmc_anneal_adaptive: n_iter must lie in 1 .. 60 (the bisections of one step: a double has no more bits to halve)");
    if (!(temperature_limit > 0.0) || !std::isfinite(temperature_limit))
        return fail("smolmc_anneal_adaptive: the temperature limit must be positive and finite");
    const int R = h->R;
    for (int r = 1; r < R; ++r)
        if (T_old[r] != T_old[0])
            return fail("smolmc_anneal_adaptive: the populations are at different temperatures (walker 0: " + std::to_string(T_old[0]) + ", walker " +
                        std::to_string(r) + ": " + std::to_string(T_old[r]) + "); the search of the step has one beta, the populations share one schedule");
    TRY(pop_scratch(h));
    TRY(grid_rebase(h));
    const SmolmcPopScratch &S = h->pop;
    SmolmcPopSearch search;
    search.T_limit = temperature_limit;
    search.beta_limit = 1.0 / (SMOLMC_KB * temperature_limit); // (as set_betas)
    search.target = overlap_target;
    search.n_iter = n_iter;
    HIPCHK(hipMemcpyAsync(S.word, offset_word, (size_t)npop * 8, hipMemcpyHostToDevice, h->stream));
    TRY(smolmc_pop_parent_launch(h, npop, S, &search));
    TRY(smolmc_pop_clone_launch(h, S.parent, npop, S.beta_new));
    h->order_dirty = true;
    h->point_T_stale = true; // (until the temperature is back: a failure below leaves the handle reading d_beta)
    HIPCHK(hipMemcpyAsync(temperature_out, S.T_new, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(flags_out, S.flags, 4, hipMemcpyDeviceToHost, h->stream));
    TRY(anneal_outputs(h, npop, parent_out, q_out, qsum_out, href_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    const std::vector<double> T_new((size_t)R, *temperature_out);
    grid_name_temperatures(h, T_new.data());
    return 0;
}
