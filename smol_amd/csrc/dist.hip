// dist.hip -- distance-objective handles (smolmc_create_distance): creation, validation, dispatch to
// mc_dist_kernel (mc_dist.h), the intensive distance vector of the evaluation entry points and the per-walker
// best records.  The model tables, site relabelling, sublattices and walker state come from smolmc_create;
// engine.hip hands a handle with `dist` set over to the functions below.
#include "mc_dist.h"

struct DistState {
    DistParams P; // tables and objective; the walker pointers and launch fields are filled per launch
    int nslot = 1;
    int mode = 0;
    double kB = SMOLMC_KB, w = 0.0, tol = 0.0, size = 1.0;
    std::vector<double> target;
    std::vector<std::vector<int>> group_feats; // features of every diameter group
    std::vector<double> gdiam;
    double *d_ext = nullptr;
    uint8_t *best_occ = nullptr;
    double *best_H = nullptr;
    uint64_t *best_step = nullptr;
    size_t lds = 0;
};

int smolmc_dist_free(smolmc_handle *h) {
    delete h->dist;
    h->dist = nullptr;
    return 0;
}

// L of a distance vector on the host: exact_match_max_diameter (distance.py:307-332, :454-472)
static double host_match_diameter(const DistState &D, const double *d) {
    double L = 0.0;
    for (size_t g = 0; g < D.gdiam.size(); ++g) {
        bool all = true;
        for (int k : D.group_feats[g]) all &= d[k] <= D.tol;
        if (!all) break;
        L = D.gdiam[g];
    }
    return L;
}

int smolmc_dist_from_extensive(const smolmc_handle *h, double *features, size_t nocc) {
    const DistState &D = *h->dist;
    const int F = h->F;
    for (size_t i = 0; i < nocc; ++i) {
        double *row = features + i * F;
        for (int k = 0; k < F; ++k) row[k] = fabs(row[k] / D.size - D.target[k]); // distance.py:133-136
        row[0] = D.w != 0.0 ? host_match_diameter(D, row) : 0.0;
    }
    return 0;
}

static int dist_set_betas(smolmc_handle *h, const double *temperature) {
    std::vector<double> beta(h->R);
    for (int r = 0; r < h->R; ++r) beta[r] = 1.0 / (h->dist->kB * temperature[r]); // metropolis.py:31-49
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_beta, beta.data(), (size_t)h->R * 8, hipMemcpyHostToDevice));
    return 0;
}

static int dist_launch(smolmc_handle *h, int64_t nsteps, const SampleBufs &smp, int init_best, const int *d_steps,
                       const double *d_u, uint8_t *d_acc, double *d_H) {
    DistState &D = *h->dist;
    KParams &kp = h->kp;
    DistParams P = D.P;
    P.occ = kp.occ;
    P.enthalpy = kp.enthalpy;
    P.features = kp.features;
    P.beta = h->d_beta;
    P.seeds = kp.seeds;
    P.nsteps = kp.nsteps;
    P.nacc = kp.nacc;
    P.last_acc = kp.last_acc;
    P.best_occ = D.best_occ;
    P.best_H = D.best_H;
    P.best_step = D.best_step;
    P.ext = D.d_ext;
    P.init_best = init_best;
    P.steps = nsteps;
    P.smp = smp;
    P.rp_steps = d_steps;
    P.rp_u = d_u;
    P.rp_acc = d_acc;
    P.rp_H = d_H;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // the features of every walker's occupancy at launch start (eval_full_kernel, extensive)
    TRY(smolmc_eval_extensive(h, kp.occ, h->R, D.d_ext));
    const bool replay = d_steps != nullptr;
    int rc;
    switch (D.nslot) {
    case 1: rc = replay ? smolmc_launch_dist_replay_1(h, P) : smolmc_launch_dist_1(h, P); break;
    case 2: rc = replay ? smolmc_launch_dist_replay_2(h, P) : smolmc_launch_dist_2(h, P); break;
    default: rc = replay ? smolmc_launch_dist_replay_4(h, P) : smolmc_launch_dist_4(h, P); break;
    }
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

int smolmc_dist_after_set_state(smolmc_handle *h, const double *temperature) {
    std::vector<double> T(h->R, 0.0);
    if (temperature) T.assign(temperature, temperature + h->R);
    TRY(dist_set_betas(h, T.data()));
    SampleBufs none;
    memset(&none, 0, sizeof(none));
    TRY(dist_launch(h, 0, none, 1, nullptr, nullptr, nullptr, nullptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int smolmc_dist_set_temperature(smolmc_handle *h, const double *temperature) {
    HIPCHK(hipSetDevice(h->device));
    TRY(dist_set_betas(h, temperature));
    return 0;
}

int smolmc_dist_run(smolmc_handle *h, int64_t nsteps, const SampleBufs &smp) {
    return dist_launch(h, nsteps, smp, 0, nullptr, nullptr, nullptr, nullptr);
}

int smolmc_dist_replay(smolmc_handle *h, int64_t nsteps, const int32_t *steps, const double *uniforms,
                       const double *log_priori, uint8_t *accepted_out, double *enthalpy_out, double *log_priori_out) {
    const size_t n = (size_t)h->R * nsteps;
    if (log_priori)
        for (size_t i = 0; i < n; ++i)
            if (!std::isnan(log_priori[i]) && log_priori[i] != 0.0)
                return fail("a distance handle takes no a-priori factor (Flip / Swap: 0, mcusher.py:118-134)");
    ReplayStage st; // (wide rows; no a-priori factors, no error word)
    TRY(st.upload(n, steps, uniforms, false, false, nullptr));
    SampleBufs none;
    memset(&none, 0, sizeof(none));
    TRY(dist_launch(h, nsteps, none, 0, st.steps.as<int>(), st.u.as<double>(), st.acc.as<uint8_t>(), st.H.as<double>()));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (accepted_out) HIPCHK(hipMemcpy(accepted_out, st.acc.p, n, hipMemcpyDeviceToHost));
    if (enthalpy_out) HIPCHK(hipMemcpy(enthalpy_out, st.H.p, n * 8, hipMemcpyDeviceToHost));
    if (log_priori_out) std::fill(log_priori_out, log_priori_out + n, 0.0);
    return 0;
}

// compute_feature_vector_change (distance.py:156-182): distance vector after the step minus before
int smolmc_dist_eval_delta(smolmc_handle *h, const int32_t *occ, const int32_t *flips, int nstep, double *dfeatures) {
    const size_t N = (size_t)h->N, F = (size_t)h->F;
    std::vector<int32_t> rows(((size_t)nstep + 1) * N);
    std::copy(occ, occ + N, rows.begin());
    for (int i = 0; i < nstep; ++i) {
        int32_t *o = rows.data() + ((size_t)i + 1) * N;
        std::copy(occ, occ + N, o);
        for (int f = 0; f < SMOLMC_MAX_STEP_FLIPS; ++f) {
            const int s = flips[(size_t)i * SMOLMC_STEP_ROW + 2 * f], c = flips[(size_t)i * SMOLMC_STEP_ROW + 2 * f + 1];
            if (s < 0) break;
            const int se = s < h->N && h->relabelled ? h->new_of[s] : s;
            if (s >= h->N || c < 0 || c >= (int)h->site_ncodes[se]) return fail("flip out of range");
            o[s] = c; // sequential flips (expansion.py:217-229)
        }
    }
    std::vector<double> d(((size_t)nstep + 1) * F);
    TRY(smolmc_eval_full(h, rows.data(), nstep + 1, d.data()));
    for (int i = 0; i < nstep; ++i)
        for (size_t k = 0; k < F; ++k) dfeatures[(size_t)i * F + k] = d[((size_t)i + 1) * F + k] - d[k];
    return 0;
}

int smolmc_dist_kernel_info(const smolmc_handle *h, char *buf, int n) {
    const DistState &D = *h->dist;
    snprintf(buf, (size_t)n, "dist nslot=%d mode=%s F=%d wpb=%d lds=%zu%s", D.nslot, D.mode ? "interactions" : "corr", h->F,
             SMOLMC_DIST_WPB, D.lds, h->relabelled ? " relabelled=1" : "");
    return 0;
}

extern "C" int smolmc_get_best(smolmc_handle *h, double *score, double *features, int32_t *occ, uint64_t *step) {
    if (!h) return fail("null handle");
    if (!h->dist) return fail("not a distance handle (smolmc_create_distance)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const DistState &D = *h->dist;
    const size_t R = h->R, N = h->N, Npad = h->Npad;
    if (score) HIPCHK(hipMemcpy(score, D.best_H, R * 8, hipMemcpyDeviceToHost));
    if (step) HIPCHK(hipMemcpy(step, D.best_step, R * 8, hipMemcpyDeviceToHost));
    if (occ || features) {
        std::vector<uint8_t> b(R * Npad);
        HIPCHK(hipMemcpy(b.data(), D.best_occ, b.size(), hipMemcpyDeviceToHost));
        std::vector<int32_t> tmp;
        int32_t *o = occ;
        if (!o) {
            tmp.resize(R * N);
            o = tmp.data();
        }
        for (size_t r = 0; r < R; ++r) // back to the caller's site order
            for (size_t s = 0; s < N; ++s) o[r * N + s] = b[r * Npad + (h->relabelled ? (size_t)h->new_of[s] : s)];
        if (features) TRY(smolmc_eval_full(h, o, (int)R, features));
    }
    return 0;
}

extern "C" int smolmc_reset_best(smolmc_handle *h) {
    if (!h) return fail("null handle");
    if (!h->dist) return fail("not a distance handle (smolmc_create_distance)");
    HIPCHK(hipSetDevice(h->device));
    SampleBufs none;
    memset(&none, 0, sizeof(none));
    TRY(dist_launch(h, 0, none, 1, nullptr, nullptr, nullptr, nullptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

static int validate_distance(const smolmc_tables *t, const smolmc_distance *d, const smolmc_config *c) {
    if (t->has_ewald) return fail("The given cluster subspace cannot have external terms."); // distance.py:76-77
    if (t->has_mu) return fail("a distance handle takes no chemical potentials");
    if (t->bias_type) return fail("a distance handle takes no bias term");
    if (c->kernel_type != SMOLMC_KERNEL_METROPOLIS) return fail("a distance handle runs Metropolis only (no Wang-Landau)");
    if (c->step_type != SMOLMC_STEP_FLIP && c->step_type != SMOLMC_STEP_SWAP)
        return fail("a distance handle takes Flip or Swap steps (no TableFlip)");
    if (!(d->match_weight >= 0)) return fail("The match weight must be a positive number."); // distance.py:79-80
    const int F = t->feature_mode == SMOLMC_FEATURES_CORRELATIONS ? t->num_corr : t->num_orbits;
    if (t->feature_mode != SMOLMC_FEATURES_CORRELATIONS && t->feature_mode != SMOLMC_FEATURES_INTERACTIONS)
        return fail("unknown feature_mode");
    if (t->feature_mode == SMOLMC_FEATURES_INTERACTIONS && !t->interaction_tensors)
        return fail("interaction mode needs interaction_tensors");
    if (d->n_features != F) return fail("n_features must equal num_corr (correlations) or num_orbits (interactions)");
    if (F > SMOLMC_DIST_MAX_FEATURES) {
        char m[160];
        snprintf(m, sizeof m, "%d features: a distance handle takes at most %d", F, SMOLMC_DIST_MAX_FEATURES);
        return fail(m);
    }
    if (!d->target || !d->weights || (d->n_groups > 0 && (!d->group_diameter || !d->feature_group)))
        return fail("null argument in smolmc_distance");
    if (d->n_groups < 0 || (d->n_groups == 0 && F > 1)) return fail("n_groups must cover every feature");
    for (int g = 1; g < d->n_groups; ++g)
        if (!(d->group_diameter[g] > d->group_diameter[g - 1])) return fail("group_diameter must be ascending");
    for (int k = 1; k < F; ++k)
        if (d->feature_group[k] < 0 || d->feature_group[k] >= d->n_groups) return fail("feature_group out of range");
    if (!(d->kB > 0)) return fail("kB must be positive");
    if (!(d->match_tol >= 0)) return fail("match_tol must be non-negative");
    return 0;
}

extern "C" int smolmc_create_distance(const smolmc_tables *t, const smolmc_distance *d, const smolmc_config *c,
                                      smolmc_handle **out) {
    if (!t || !d || !c || !out) return fail("null argument");
    TRY(validate_distance(t, d, c));
    const int F = d->n_features, mode = t->feature_mode;
    // the model tables, relabelling, sublattices and walker state of an ordinary handle (ce_coefs ignored)
    smolmc_tables t0 = *t;
    std::vector<double> zeros((size_t)F, 0.0);
    t0.ce_coefs = zeros.data();
    smolmc_handle *h = nullptr;
    TRY(smolmc_create(&t0, c, &h));
    auto bail = [&](int rc) {
        smolmc_destroy(h);
        return rc;
    };
    h->family = K_GENERAL; // (no other family runs on this handle)
    DistState *Dp = new DistState();
    h->dist = Dp;
    DistState &D = *Dp;
    D.mode = mode;
    D.kB = d->kB;
    D.w = d->match_weight;
    D.tol = d->match_tol;
    D.size = (double)t->size;
    D.target.assign(d->target, d->target + F);
    D.gdiam.assign(d->group_diameter, d->group_diameter + d->n_groups);
    D.group_feats.assign((size_t)d->n_groups, {});
    for (int k = 1; k < F; ++k) D.group_feats[d->feature_group[k]].push_back(k);
    h->natural.assign(1, -d->match_weight); // distance.py:95
    h->natural.insert(h->natural.end(), d->weights, d->weights + F - 1);
    // per-site (local record, function) pairs in the engine's site numbering
    const int N = t->num_sites;
    std::vector<long long> pptr(N + 1, 0), cptr(N + 1, 0);
    std::vector<DistPair> pairs;
    std::vector<DistChunk> chunks;
    std::vector<uint16_t> rows; // eight u16 per row
    int max_chunks = 0;
    std::vector<int> seen((size_t)F, -1);
    for (int e = 0; e < N; ++e) {
        const int cs = h->relabelled ? h->old_of[e] : e;
        for (int64_t rec = t->site_ptr[cs]; rec < t->site_ptr[cs + 1]; ++rec) {
            const int o = t->loc_orbit[rec], I = t->orb_nsites[o], J = t->loc_nrows[rec];
            if (I > SMOLMC_MAX_CLUSTER_SITES) return bail(fail("cluster larger than SMOLMC_MAX_CLUSTER_SITES"));
            const long long row_off = (long long)rows.size() / 8;
            const int32_t *src = t->loc_idx + t->loc_off[rec];
            for (int j = 0; j < J; ++j)
                for (int m = 0; m < 8; ++m) {
                    const int x = m < I ? src[(size_t)j * I + m] : 0;
                    if (x < 0 || x >= N) return bail(fail("local cluster row out of range"));
                    rows.push_back((uint16_t)(h->relabelled ? h->new_of[x] : x));
                }
            const int K = mode == SMOLMC_FEATURES_CORRELATIONS ? t->orb_nfunc[o] : 1;
            for (int k = 0; k < K; ++k) {
                DistPair p;
                memset(&p, 0, sizeof(p));
                p.feat = mode == SMOLMC_FEATURES_CORRELATIONS ? t->orb_bit_id[o] + k : t->orb_id[o];
                if (p.feat <= 0 || p.feat >= F) return bail(fail("feature index of a local record out of range"));
                if (seen[p.feat] == e) return bail(fail("a site holds two local records of one feature"));
                seen[p.feat] = e;
                p.J = J;
                p.ratio = t->loc_ratio[rec];
                p.c0 = (int32_t)((long long)chunks.size() - cptr[e]);
                const int64_t t_off = mode == SMOLMC_FEATURES_CORRELATIONS
                                          ? (int64_t)t->orb_ctensor_off[o] + (int64_t)k * t->orb_tensor_len[o]
                                          : (int64_t)t->orb_itensor_off[o];
                for (int j0 = 0; j0 < J; j0 += DIST_ROWS) { // chunks of DIST_ROWS rows, in row order
                    DistChunk c;
                    memset(&c, 0, sizeof(c));
                    c.row_off = (int32_t)(row_off + j0);
                    c.t_off = (int32_t)t_off;
                    c.n = (int16_t)std::min(DIST_ROWS, J - j0);
                    c.I = (int16_t)I;
                    for (int m = 0; m < I; ++m) {
                        const int st = t->tensor_indices[t->orb_stride_off[o] + m];
                        if (st > 32767) return bail(fail("tensor stride too large for the distance kernel"));
                        c.st[m] = (int16_t)st;
                    }
                    chunks.push_back(c);
                }
                p.nc = (int32_t)((long long)chunks.size() - cptr[e]) - p.c0;
                pairs.push_back(p);
            }
        }
        pptr[e + 1] = (long long)pairs.size();
        cptr[e + 1] = (long long)chunks.size();
        max_chunks = std::max(max_chunks, (int)(cptr[e + 1] - cptr[e]));
    }
    if (rows.size() / 8 > 0x7fffffffull) return bail(fail("too many cluster rows for the distance kernel"));
    // rounds of 64 chunks per pass: one, two or four unrolled (larger sites loop over such rounds)
    D.nslot = max_chunks <= 64 ? 1 : max_chunks <= 128 ? 2 : 4;
    // the tensors of the feature mode, as far as the records reach
    size_t tens_len = 0;
    for (int o = 0; o < t->n_orb; ++o) {
        const size_t len = (size_t)t->orb_tensor_len[o];
        tens_len = std::max(tens_len, mode == SMOLMC_FEATURES_CORRELATIONS
                                          ? (size_t)t->orb_ctensor_off[o] + (size_t)t->orb_nfunc[o] * len
                                          : (size_t)t->orb_itensor_off[o] + len);
    }
    const double *tens = mode == SMOLMC_FEATURES_CORRELATIONS ? t->corr_tensors : t->interaction_tensors;
    // exact-match masks: bit k of chunk c set in the row of group g when feature 64 c + k belongs to a group <= g
    const int nchunk = (F + 63) / 64;
    std::vector<unsigned long long> gmask((size_t)std::max(1, d->n_groups) * nchunk, 0ull);
    for (int k = 1; k < F; ++k)
        for (int g = d->feature_group[k]; g < d->n_groups; ++g) gmask[(size_t)g * nchunk + k / 64] |= 1ull << (k % 64);
    std::vector<double> wts((size_t)F, 0.0);
    for (int k = 1; k < F; ++k) wts[k] = d->weights[k - 1];
    DistParams &P = D.P;
    memset(&P, 0, sizeof(P));
    P.R = h->R;
    P.N = h->N;
    P.Npad = h->Npad;
    P.F = F;
    P.nsub = h->kp.nsub;
    P.step_type = c->step_type;
    P.nchunk = nchunk;
    P.n_groups = d->n_groups;
    P.sub_ptr = h->kp.sub_ptr;
    P.sub_sites = h->kp.sub_sites;
    P.sub_code_ptr = h->kp.sub_code_ptr;
    P.sub_codes = h->kp.sub_codes;
    P.sub_cum = h->kp.sub_cum;
    P.tens_len = (long long)tens_len;
    P.w_match = d->match_weight;
    P.tol = d->match_tol;
    P.size = (double)t->size;
    if (P.nsub < 1) return bail(fail("no active sublattice"));
    if (N > 65535) return bail(fail("a distance handle takes at most 65535 sites"));
    const uint16_t *d_rows = nullptr;
    P.max_chunks = max_chunks;
    if (dev_upload(h, pptr.data(), pptr.size(), &P.pair_ptr) || dev_upload(h, pairs.data(), pairs.size(), &P.pairs) ||
        dev_upload(h, cptr.data(), cptr.size(), &P.chunk_ptr) || dev_upload(h, chunks.data(), chunks.size(), &P.chunks) ||
        dev_upload(h, rows.data(), rows.size() + 8, &d_rows) || dev_upload(h, tens, tens_len, &P.tens) ||
        dev_upload(h, D.target.data(), D.target.size(), &P.target) || dev_upload(h, wts.data(), wts.size(), &P.wts) ||
        dev_upload(h, D.gdiam.data(), D.gdiam.size(), &P.gdiam) || dev_upload(h, gmask.data(), gmask.size(), &P.gmask))
        return bail(1);
    P.rows = (const uint4 *)d_rows; // (one spare row behind the last: batches read at most the record's own rows)
    P.lds_shared = (int)(((size_t)F * 16 + tens_len * 8 + 15) / 16 * 16);
    P.lds_per_wave = (int)(((size_t)F * 16 + (size_t)max_chunks * 8 + 2 * (size_t)h->Npad + 15) / 16 * 16);
    D.lds = (size_t)P.lds_shared + (size_t)SMOLMC_DIST_WPB * P.lds_per_wave;
    if (D.lds > 64 * 1024) {
        char m[320];
        snprintf(m, sizeof m,
                 "model too large for the distance kernel: %zu bytes of LDS per workgroup (limit 65536) -- the feature "
                 "mode's tensors (%zu doubles) and, per walker, 16 F + 8 x (row chunks of a site, %d) + 2 x sites bytes",
                 D.lds, tens_len, max_chunks);
        return bail(fail(m));
    }
    const size_t R = h->R;
    if (dev_alloc(h, R * F, &D.d_ext) || dev_alloc(h, R * h->Npad, &D.best_occ) || dev_alloc(h, R, &D.best_H) ||
        dev_alloc(h, R, &D.best_step))
        return bail(1);
    *out = h;
    return 0;
}
