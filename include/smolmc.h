/*
 * smolmc.h -- C-ABI of the MI355X-native ensemble Monte-Carlo engine.
 *
 * Drop-in boundary for ONE hot path of CederGroupHub/smol: the
 * per-flip local correlation / cluster-interaction delta, the Ewald single-flip
 * delta and the Metropolis / Wang-Landau accept step, batched over independent
 * replica walkers.  The reference has no C ABI of its own for this path: its
 * native entry points are the Cython cpdef methods listed below, called from
 * Python objects.  Each entry point here names the reference interface it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions (same as the reference):
 *   - occupancies are int32, C-contiguous, values = species codes per site
 *     (smol/moca/processor/base.py:228-237);
 *   - index tables are int32 C-contiguous, tensors / outputs are float64;
 *   - feature vectors handed back are EXTENSIVE (x size) like
 *     Processor.compute_feature_vector[_change] (processor/expansion.py:184,231);
 *   - the engine copies every table at smolmc_create(); the caller keeps
 *     ownership of all buffers it passes; outputs are caller-allocated;
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from smolmc_last_error() (the Python shim raises
 *     ValueError / RuntimeError like the reference, expansion.py:186-188).
 *   - a handle is not thread-safe; one host thread drives one device.
 *
 * All pointers in this header are HOST pointers unless the name says _dev.
 */
#ifndef SMOLMC_H
#define SMOLMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMOLMC_ABI_VERSION 8

/* Status codes: 0 = ok; SMOLMC_ERR (1) = any failure, message in smolmc_last_error(); the codes below name failures a
 * caller may want to handle without parsing the message (the message is set for them too). */
#define SMOLMC_ERR 1
#define SMOLMC_ERR_RING_FULL 2 /* smolmc_run_sampled: both ring slots hold blocks that were not fetched */

#define SMOLMC_BIAS_NONE 0
#define SMOLMC_BIAS_FUGACITY 1
#define SMOLMC_BIAS_SQUARE_CHARGE 2
#define SMOLMC_BIAS_SQUARE_HYPERPLANE 3
#define SMOLMC_MAX_BIAS_ROWS 4 /* hyperplanes of a SquareHyperplaneBias */
#define SMOLMC_MAX_CLUSTER_SITES 6 /* largest cluster (sites per cluster) supported */

/* feature_mode */
#define SMOLMC_FEATURES_CORRELATIONS 0 /* ClusterExpansionProcessor  (expansion.py:39)  */
#define SMOLMC_FEATURES_INTERACTIONS 1 /* ClusterDecompositionProcessor (expansion.py:243) */
/* kernel_type (smol/moca/kernel/__init__.py:35-56 mckernel_factory names) */
#define SMOLMC_KERNEL_METROPOLIS 0 /* kernel/metropolis.py:52 */
#define SMOLMC_KERNEL_WANGLANDAU 1 /* kernel/wanglandau.py:17 */
/* step_type (smol/moca/kernel/mcusher.py) */
#define SMOLMC_STEP_FLIP 0 /* Flip  mcusher.py:151 */
#define SMOLMC_STEP_SWAP 1 /* Swap  mcusher.py:173 */
#define SMOLMC_STEP_TABLE_FLIP 2 /* TableFlip mcusher.py:397 (charge-neutral semigrand) */
#define SMOLMC_MAX_STEP_FLIPS 8  /* most single-site flips in one TableFlip step */
/* One MC step as the ushers return it (a list of (site, code) tuples, mcusher.py:104-116), as a fixed
 * record of SMOLMC_STEP_ROW int32: (site_0, code_0, ..., site_7, code_7), flips in the order the
 * reference applies them (sequential-flip semantics, expansion.py:217-229); the record ends at the
 * first site < 0 (-1 = no flip; an all -1 record is the empty step of mcusher.py:197-199). */
#define SMOLMC_STEP_ROW (2 * SMOLMC_MAX_STEP_FLIPS)
#define SMOLMC_MAX_FLIP_VECTORS 32 /* rows of flip_table (2 x that many directions) */
#define SMOLMC_MAX_FLIP_DIMS 64    /* columns of flip_table: species over the active sublattices */

/*
 * Read-only model tables.  Flattened, caller-owned equivalents of the
 * containers in smol/utils/cluster/container.pyx (OrbitContainer :21,
 * IntArray2DContainer :287, FloatArray1DContainer :173) and struct.pxd:12-38.
 */
typedef struct smolmc_tables {
    int32_t num_sites;   /* N, length of an occupancy (Processor.num_sites) */
    int32_t size;        /* P, number of prim cells in the supercell (Processor.size) */
    int32_t num_orbits;  /* incl. empty cluster (ClusterSubspace.num_orbits) */
    int32_t num_corr;    /* incl. empty cluster (num_corr_functions) */
    int32_t max_species; /* largest number of species codes on any site */
    int32_t n_orb;       /* number of OrbitC records = num_orbits - 1 */

    /* OrbitC records, order of ClusterSubspace.orbits
     * (struct.pxd:33-38, get_orbit_data smol/utils/cluster/__init__.py:4-15) */
    const int32_t *orb_id;          /* [n_orb] orbit.id        (>= 1) */
    const int32_t *orb_bit_id;      /* [n_orb] orbit.bit_id    (>= 1) */
    const int32_t *orb_nsites;      /* [n_orb] I = tensor_indices.size */
    const int32_t *orb_nfunc;       /* [n_orb] K = correlation_tensors.size_r */
    const int32_t *orb_tensor_len;  /* [n_orb] correlation_tensors.size_c */
    const int32_t *orb_stride_off;  /* [n_orb] offset into tensor_indices[] */
    const int32_t *tensor_indices;  /* concatenated flat_tensor_indices (orbit.py:268-275) */
    const int64_t *orb_ctensor_off; /* [n_orb] offset into corr_tensors[] */
    const double *corr_tensors;     /* concatenated [K x len] row-major (orbit.py:251-266) */
    const int64_t *orb_itensor_off; /* [n_orb] offset into interaction_tensors[] */
    const double *interaction_tensors; /* concatenated [len] (expansion.py:186-201) */
    double offset;                  /* interaction of the empty cluster (evaluator.pxd:20) */

    /* full cluster-site tables: OrbitIndices (clusterspace.py:1329-1366) */
    const int64_t *full_off; /* [n_orb+1] offsets (int32 entries) into full_idx */
    const int32_t *full_idx; /* per orbit rows [J_full x I] */

    /* per-site reduced tables: LocalEvalData (processor/expansion.py:24-36,120-156) */
    const int64_t *site_ptr;  /* [N+1] local-record range of each site (empty if inactive) */
    const int32_t *loc_orbit; /* [n_loc] index into orb_* records */
    const double *loc_ratio;  /* [n_loc] cluster_ratio */
    const int32_t *loc_nrows; /* [n_loc] J_local */
    const int64_t *loc_off;   /* [n_loc] offset (int32 entries) into loc_idx */
    const int32_t *loc_idx;   /* rows [J_local x I] */

    /* natural parameters of the cluster-expansion part (Processor.coefs) */
    int32_t feature_mode;   /* SMOLMC_FEATURES_* */
    const double *ce_coefs; /* [num_corr] (mode 0) or [num_orbits] (mode 1) */

    /* EwaldProcessor tables (smol/moca/processor/ewald.py:76-101), optional */
    int32_t has_ewald;
    int32_t ewald_dim;         /* M */
    int32_t ewald_width;       /* columns of ewald_inds */
    const int32_t *ewald_inds; /* [N x ewald_width], -1 = vacancy / absent */
    const double *ewald_matrix; /* [M x M] */
    double ewald_coef;          /* coefficient of the Ewald feature (ensemble.py:191-199) */

    /* chemical-potential table (smol/moca/ensemble.py:90-99), optional */
    int32_t has_mu;
    int32_t mu_width;
    const double *mu_table; /* [N x mu_width]; natural parameter -1 appended last */

    /* active sublattices (smol/moca/sublattice.py:23; mcusher.py:55-57) */
    int32_t n_sublattices;
    const int64_t *sub_site_ptr;   /* [n_sub+1] ranges into sub_active_sites */
    const int32_t *sub_active_sites;
    const int64_t *sub_code_ptr;   /* [n_sub+1] ranges into sub_codes */
    const int32_t *sub_codes;      /* Sublattice.encoding */
    const double *sub_probs;       /* [n_sub] sublattice_probabilities (sum to 1) */

    /* Optional: charge of every Ewald index, [ewald_dim] (the oxidation states of
     * EwaldProcessor._ewald_structure, processor/ewald.py:76-78).  When given, the engine
     * checks that ewald_matrix[a][b] == q_a q_b G[site_a][site_b] off the diagonal (what
     * pymatgen's EwaldSummation builds) and, if it holds to 1e-12, evaluates single-flip
     * deltas from the N x N site kernel G (4x less memory traffic than two matrix rows);
     * otherwise it silently uses the dense rows.  NULL = dense. */
    const double *ewald_charges;

    /* TableFlip (smol/moca/kernel/mcusher.py:397-711), used with SMOLMC_STEP_TABLE_FLIP.
     * flip_table rows are flip vectors in "counts" format over the ACTIVE sublattices'
     * species, concatenated in sub_* order (the reference's dims of inactive sublattices
     * are always zero and are dropped); directions 2i / 2i+1 are +row i / -row i. */
    int32_t n_flip_vectors;      /* <= SMOLMC_MAX_FLIP_VECTORS */
    const int32_t *flip_table;   /* [n_flip_vectors x sum(codes of active sublattices)], <= SMOLMC_MAX_FLIP_DIMS columns */
    const double *flip_weights;  /* [2 x n_flip_vectors] (mcusher.py:519-538) */
    double swap_weight;          /* probability of a canonical Swap instead (mcusher.py:540) */

    /* MCBias (smol/moca/kernel/bias.py): an extra term delta_bias added to the Metropolis
     * exponent (metropolis.py:43-44) and traced as `bias` (kernel/base.py:307-311,362-363).
     * bias_table is [num_sites x bias_width], indexed [site][species code]:
     *   SMOLMC_BIAS_FUGACITY       FugacityBias._fu_table (bias.py:208-226): fugacity fractions,
     *                              1 where unused; bias = sum_sites log(table[site][occ])
     *   SMOLMC_BIAS_SQUARE_CHARGE  SquareChargeBias._c_table (bias.py:256-262): oxidation states,
     *                              0 where unused; bias = -bias_penalty * (sum_sites table)^2
     *   SMOLMC_BIAS_SQUARE_HYPERPLANE  SquareHyperplaneBias (bias.py:290-366): bias_rows tables
     *                              [bias_rows x num_sites x bias_width], table r holding
     *                              A[r][dim_id(site, code)] (the hyperplane normal's entry of the
     *                              species, get_dim_ids_table occu_utils.py:8-23; 0 where unused)
     *                              and bias_intercepts[r] = b[r];
     *                              bias = -bias_penalty * sum_r (sum_sites table_r - b_r)^2
     * Not allowed with Wang-Landau (wanglandau.py:127-128). */
    int32_t bias_type;           /* SMOLMC_BIAS_* */
    int32_t bias_width;
    const double *bias_table;
    double bias_penalty;         /* SquareChargeBias / SquareHyperplaneBias .penalty (> 0) */
    int32_t bias_rows;           /* hyperplanes (<= SMOLMC_MAX_BIAS_ROWS); 0 or 1 for the other types */
    const double *bias_intercepts; /* [bias_rows] (NULL = zeros) */
} smolmc_tables;

typedef struct smolmc_config {
    int32_t n_replicas;  /* walkers owned by this handle (Sampler nwalkers) */
    int32_t kernel_type; /* SMOLMC_KERNEL_* */
    int32_t step_type;   /* SMOLMC_STEP_* */
    int32_t device;      /* HIP device ordinal (ignored by the CPU oracle) */
    /* Wang-Landau parameters (kernel/wanglandau.py:26-39) */
    double wl_min_enthalpy, wl_max_enthalpy, wl_bin_size;
    double wl_flatness, wl_mod_factor, wl_mod_divisor; /* mod_update = m / divisor */
    int64_t wl_check_period, wl_update_period; /* check period 0: no device-side flatness check (the
                                                * caller checks and applies its own mod_update callable) */
} smolmc_config;

typedef struct smolmc_handle smolmc_handle;

/* ---- lifetime ----------------------------------------------------------- */
/* Replaces construction of Processor + Ensemble + one MCKernel per walker
 * (processor/expansion.py:61-163, ensemble.py:102-217, kernel/base.py:192-239). */
int smolmc_create(const smolmc_tables *tables, const smolmc_config *config,
                  smolmc_handle **out);
int smolmc_destroy(smolmc_handle *h);
const char *smolmc_last_error(void);
int smolmc_abi_version(void);

/* Which kernel family this handle dispatches to, as a short text ("lean nslot=2 mm=2 field=1" /
 * "general nslot=8 mm=2 field=1"): lets callers and tests assert that the intended path runs
 * (no reference counterpart). Writes at most n bytes including the terminator (give it 512).
 * A handle on mc_kernel / the universal kernel appends " | not lean: <the first condition of
 * smolmc_create that kept the model off the specialised kernels>".  "lazy-features" marks a handle
 * whose kernels carry the scalar features only (Ewald energy, chemical work) and whose cluster
 * features -- several correlation functions per orbit, evaluator.pyx:211-265, or more than 64 of
 * them -- are evaluated from the occupancies wherever this interface returns them
 * (smolmc_get_state, smolmc_get_samples*): same values, to rounding, as the step-by-step trace
 * of sampler/sampler.py:204-207. */
int smolmc_kernel_info(const smolmc_handle *h, char *buf, int n);

/* ---- sizes -------------------------------------------------------------- */
int smolmc_num_features(const smolmc_handle *h); /* len(ensemble.natural_parameters) */
int smolmc_wl_num_levels(const smolmc_handle *h); /* len(np.arange(min,max,bin)) wanglandau.py:107 */
/* natural parameters vector (Ensemble.natural_parameters, ensemble.py:25,61-65) */
int smolmc_natural_parameters(const smolmc_handle *h, double *out /*F*/);

/* ---- state: Sampler.setup_sample + MCKernel.compute_initial_trace ------- */
/* (sampler/sampler.py:386-434, kernel/base.py:345-365, wanglandau.py:290-300).
 * occ [R x N] int32, seeds [R], temperature [R] (Kelvin; ignored by WL).
 * Computes the initial features / enthalpy of every walker on the device.
 * reset_aux != 0: fresh kernels -- per-walker RNG counters (= step counters), accept
 * counters and Wang-Landau aux arrays are reset.  reset_aux == 0: continuation --
 * counters and WL arrays are kept (a kernel's Generator and aux state persist
 * across Sampler.run calls in the reference, sampler.py:254-262), seeds are ignored. */
int smolmc_set_state(smolmc_handle *h, const int32_t *occ, const uint64_t *seeds,
                     const double *temperature, int reset_aux);
/* ThermalKernelMixin.temperature setter (kernel/base.py:418-422), per walker */
int smolmc_set_temperature(smolmc_handle *h, const double *temperature /*R*/);
/* Per-walker chemical potentials: a mu-T grid in one semigrand handle (the reference assigns
 * ensemble.chemical_potentials and runs again, ensemble.py:35-73; here walker r has its own row, as it has its own
 * temperature).  mu [R x n_sublattices x mu_width] in the caller's numbering: the active sublattices in the order of
 * smolmc_tables, the columns the species codes exactly as in mu_table at smolmc_create.  NULL returns the handle to
 * the table it was created with.  The chemical-work feature (the last of F, natural parameter -1) and the enthalpy
 * of every walker are re-priced on the device from its current occupancy at its new row, so a call between two
 * smolmc_run is a mu sweep that carries the configurations along; smolmc_set_state prices the initial trace with the
 * walker's own row, and the rows survive it.  smolmc_eval_full and smolmc_eval_delta keep the create-time table.
 * Valid on a handle created with has_mu that runs a lean kernel family; refused, each with its reason, on handles
 * without has_mu, distance handles, Wang-Landau handles (one density of states per Hamiltonian) and handles on
 * mc_kernel / the universal kernel; while rows are set smolmc_replay, smolmc_exchange_dev and
 * smolmc_import_temperature_dev are refused (an exchange of temperatures alone is no valid move between different
 * Hamiltonians) and smolmc_kernel_info appends " walker_mu=1 mu_max=<largest |mu| over all walkers>".  The valid
 * exchange move between such walkers is smolmc_exchange_grid, which swaps temperature and row together. */
int smolmc_set_walker_mu(smolmc_handle *h, const double *mu /* R x n_sublattices x mu_width, or NULL */);
/* ... the rows in the same shape: each walker's current row (those of the last call, moved by the exchanges of
 * smolmc_exchange_grid since), the create-time rows when none are set */
int smolmc_get_walker_mu(smolmc_handle *h, double *mu /* R x n_sublattices x mu_width */);
/* Replica exchange across the mu-T grid (hyper-parallel tempering), decided and applied on the device.  State point p
 * is the (temperature, row of chemical potentials) walker p held at the latest smolmc_set_state,
 * smolmc_set_temperature or smolmc_set_walker_mu: each of those calls makes the current assignment the new identity
 * map.  For every pair (s, t) of state points, with walker a at s, walker b at t, beta = 1 / (kB T), H the current
 * enthalpies, n the species counts per (active sublattice, code) and d = row_t - row_s:
 *     Delta = (beta_s - beta_t) (Hb - Ha) + beta_s (n_b . d) - beta_t (n_a . d),  accept iff -Delta >= 0 or log_u < -Delta
 * (from H_s(x) = E0(x) - n(x) . row_s; with d = 0 the temperature exchange of smolmc_exchange_dev).  On acceptance the
 * two walkers swap their state points: temperatures and rows change places, the chemical work and the enthalpy of
 * both are re-priced, occupancies do not move.  The pairs of one call must be disjoint; log_u is finite or -inf
 * (-inf accepts every pair).  Queued on the handle's stream; stats, when given, gains 1 per attempted pair in
 * stats[2 p] and 1 per accepted pair in stats[2 p + 1] (this waits for the kernel; with NULL nothing is copied back).
 * A handle created with has_mu on a lean kernel family whose rows are not set exchanges temperatures only.  Refused,
 * each with its reason: handles without has_mu, distance handles, Wang-Landau handles, handles on mc_kernel / the
 * universal kernel, and handles whose state points have no temperatures: before the first smolmc_set_state /
 * smolmc_set_temperature, and after smolmc_exchange_dev / smolmc_import_temperature_dev moved the temperatures last
 * (they name no points; a handle that exchanged temperatures that way calls smolmc_set_temperature with its current
 * temperatures once, then exchanges with this call). */
int smolmc_exchange_grid(smolmc_handle *h, int npairs, const int32_t *pairs /* npairs x 2 state points, host */,
                         const double *log_u /* npairs, host */, int64_t *stats /* npairs x 2 in/out, host, or NULL */);
/* ... the state point every walker is at, and its temperature: the value the point was named with, not 1 / (kB beta)
 * recomputed.  Either pointer may be NULL. */
int smolmc_get_state_points(smolmc_handle *h, int32_t *point_of /* R */, double *temperature /* R */);
/* Per-walker Wang-Landau windows: replica-exchange Wang-Landau (Vogel, Li, Wuest, Landau, PRL 110, 210603) in one
 * handle.  Walker r samples the window [vmin[r], vmax[r]) with the handle's bin size instead of the one window of
 * smolmc_config.  Every window must give the handle's number of levels by the rule of smolmc_create,
 * ceil((vmax - vmin) / wl_bin_size) == smolmc_wl_num_levels(h); otherwise the call is refused and names the first
 * offending walker (create the handle with any one of the windows as wl_min_enthalpy / wl_max_enthalpy).
 * ESTIMATORS: the Wang-Landau arrays (entropy, histogram, occurrences, mean features, modification factor) belong to
 * an estimator; estimator e is the window and density-of-states copy walker e held at the latest
 * smolmc_set_wl_windows.  smolmc_exchange_wl moves estimators between walkers; a walker always updates the arrays of
 * the estimator it holds, while its step counter, random stream and configuration stay its own.  smolmc_get_wl and
 * smolmc_set_wl are in ESTIMATOR order (walker order while no exchange was accepted, and always without windows).
 * This call and smolmc_set_state(reset_aux != 0) reset the walker -> estimator map to the identity; a continuation
 * (reset_aux == 0) keeps it; the windows survive smolmc_set_state, which checks every start enthalpy against the
 * window its walker holds.  The call itself leaves the Wang-Landau arrays alone.  NULL, NULL: back to the config's
 * window.  Valid on Wang-Landau handles that run mc_wl_kernel or the Wang-Landau variant of mc_lean_multi_kernel;
 * refused, each naming its kernel family, on the KF and TableFlip Wang-Landau kernels, on mc_kernel and the universal
 * kernel, and on handles that are not Wang-Landau.  While windows are set smolmc_replay and the SMOLMC_SAMPLE_WL
 * column of smolmc_run_sampled are refused, and smolmc_kernel_info appends " wl_windows=1". */
int smolmc_set_wl_windows(smolmc_handle *h, const double *vmin /* R, or NULL */, const double *vmax /* R, or NULL */);
/* ... the window every walker holds now and the estimator it belongs to (the config's window and the identity while
 * none are set).  Any pointer may be NULL. */
int smolmc_get_wl_windows(smolmc_handle *h, double *vmin /* R */, double *vmax /* R */, int32_t *estimator_of /* R */);
/* Replica exchange between energy windows, decided and applied on the device.  For every pair (s, t) of estimators,
 * with walker a holding s, walker b holding t, Ea / Eb the enthalpies smolmc_get_state returns, S the entropies:
 * the pair is rejected, whatever log_u, unless Ea lies in [vmin_t, vmax_t) and Eb in [vmin_s, vmax_s); else, with
 * ia(E) = floor((E - vmin_s) / bin), ib(E) = floor((E - vmin_t) / bin) (the exact floor division of the sampling step),
 *     ex = ((S_s[ia(Ea)] - S_s[ia(Eb)]) + S_t[ib(Eb)]) - S_t[ib(Ea)],  accept iff ex >= 0 or log_u < ex.
 * On acceptance the two walkers swap estimators (window and row of every Wang-Landau array); occupancies, features,
 * enthalpies, Ewald fields, counters and the arrays themselves do not move, and nothing is recorded: the next sampling
 * step's post-step records each walker in its new estimator.  The pairs of one call must be disjoint; log_u is finite
 * or -inf (-inf accepts every in-window pair).  Queued on the handle's stream; stats as in smolmc_exchange_grid.
 * Refused like smolmc_set_wl_windows, and while no windows are set. */
int smolmc_exchange_wl(smolmc_handle *h, int npairs, const int32_t *pairs /* npairs x 2 estimators, host */,
                       const double *log_u /* npairs, host */, int64_t *stats /* npairs x 2 in/out, host, or NULL */);
/* The second half of the method: the copies of a window go through the Wang-Landau stages together.  Entropy S,
 * histogram and modification factor m are in ESTIMATOR order (smolmc_get_wl); group g is the estimators g * copies ..
 * g * copies + copies - 1, G = R / copies groups.  Per group, in this order:
 *   status 2  the copies' factors are not all bitwise equal: the group is left alone;
 *   flat(e):  V = {i : S_e[i] > 0}, n = |V|; not flat if n < 2; mean = (double) (sum over V of hist_e[i], in integers) /
 *             (double) n; thr = wl_flatness * mean (one rounding each); flat iff (double) hist_e[i] > thr for every i in V
 *             (the criterion of the sampling kernels' own check);
 *   status 0  some copy of the group is not flat: the group is left alone;
 *   status 1  otherwise, for every bin i, also one no copy visited: a = S_e0[i], then a = a + S_e0+c[i] for c = 1 ..
 *             copies - 1 in that order, and S_e[i] = a / (double) copies for every copy; the histogram of every copy
 *             becomes 0 and the factor of every copy m / wl_mod_divisor.
 * A bin that some copies never visited takes the plain mean with their zeros: every copy then sees it as visited.
 * Occurrences, mean features, step counters and the walker -> estimator map are not touched.  Queued on the handle's
 * stream: with both outputs NULL the call only queues work, with either it waits for the kernel.  Valid on EVERY
 * Wang-Landau handle, with or without per-walker windows (without: every estimator has the config's window; copies = R
 * is plain multi-walker Wang-Landau with one shared ln g).  Refused, naming the reason: on handles that are not
 * Wang-Landau and on distance handles; for copies < 1 or copies that does not divide R; while windows are set and the
 * estimators of a group do not have bitwise one [vmin, vmax) (names the group and the first offending estimator); and on
 * a handle with wl_check_period != 0, whose kernels would reset single copies behind the merge (create it with 0). */
int smolmc_wl_synchronise(smolmc_handle *h, int copies, int32_t *status_out /* R / copies, host, or NULL */,
                          double *mod_factor_out /* R / copies, host, or NULL: the groups' factors after the call (copy 0's) */);
/* Population annealing (Hukushima & Iba 2003; Machta, PRE 82, 026704): resample and clone walkers on the device.
 * smolmc_resample clones by an explicit map (host, R entries): slot m takes the state of slot parent[m] -- occupancy,
 * features, enthalpy, accepted flag, bias and Ewald field; every source must map to itself (parent[parent[m]] ==
 * parent[m]: the copy is in place); step counters, seeds and temperatures stay with the slot, so clones diverge from
 * the next step on without reseeding.  Queued on the handle's stream.
 * Both calls are refused, naming the reason, on Wang-Landau and distance handles, while per-walker chemical potentials
 * are set, for a parent out of range or a source that is a destination, for npop that does not divide R and for a
 * population whose walkers are not at one temperature. */
int smolmc_resample(smolmc_handle *h, const int32_t *parent /* R, host */);
/* ... one population-annealing step: npop populations of n = R / npop walkers (contiguous slots), population p goes
 * from its inverse temperature beta to beta' = 1 / (kB temperature_new[p]), db = beta' - beta of either sign:
 *     H_ref = min H (db > 0) or max H;  w_j = exp(-(db * (H_j - H_ref)));  q_j = (uint64) floor(w_j * 2^40);  Q = sum q_j
 *     off = (offset_word[p] * Q) >> 64;  C_j = q_0 + ... + q_j
 *     child m (0 <= m < n) descends from the smallest j with n * C_j > m * Q + off   (systematic resampling)
 *     survivors keep their slot; the k-th slot without a child takes the k-th surplus copy, parents ascending
 * then the walkers are cloned as by smolmc_resample and the new temperatures are in force.  n <= 2^22.
 * ln(Q / (n 2^40)) - db * H_ref estimates ln Z(beta') - ln Z(beta).  Outputs (host) may be NULL: without them the call
 * only queues work on the handle's stream; with any it waits for the kernels.  parent_out holds slot numbers of the
 * handle. */
int smolmc_anneal_resample(smolmc_handle *h, int npop, const double *temperature_new /* npop */,
                           const uint64_t *offset_word /* npop */, int32_t *parent_out /* R */, uint64_t *q_out /* R */,
                           uint64_t *qsum_out /* npop */, double *href_out /* npop */);
/* ... the same step with the temperature chosen on the device: the largest step from the populations' common beta
 * towards 1 / (kB temperature_limit), cooling or heating, at which the energy histograms at beta and beta' still overlap
 * by overlap_target / 2^32 (Barash, Weigel, Borovsky, Janke, Shchur 2017).  For one population and a step db, with q_j and
 * Q as above:
 *     s = sum_j min(Q, n q_j) = c Q + n U  (c walkers with n q_j >= Q, U the sum of the other q_j);  ok iff s 2^32 >= t n Q
 * (s / (n Q) is the expected share of distinct survivors of the resampling).  Per population: D = 1 / (kB
 * temperature_limit) - beta if ok(D) (the limit is reached); else lo = 0, hi = D, at most n_iter times mid = 0.5 * (lo +
 * hi), stop if mid equals lo or hi, lo = mid if ok(mid) else hi = mid; the step is lo, or hi while lo is still 0 (forced:
 * the target is not met at this resolution, the schedule moves all the same).  All populations take the step of smallest
 * magnitude (the first of equals): T' = temperature_limit if every population reached it, else 1 / (kB (beta + db)), and
 * beta' = 1 / (kB T'), every operation rounded on its own.  temperature_out receives T', flags_out bit 0 `reached` and
 * bit 1 `forced` (of the population whose step was taken).  The call always waits for its kernels.  Refused like
 * smolmc_anneal_resample, and for overlap_target == 0, n_iter outside 1 .. 60, a limit that is not positive and finite,
 * and populations that are not all at one temperature.  The other outputs as above (may be NULL). */
int smolmc_anneal_adaptive(smolmc_handle *h, int npop, double temperature_limit, uint32_t overlap_target, int n_iter,
                           const uint64_t *offset_word /* npop */, double *temperature_out /* 1 */,
                           int32_t *flags_out /* 1: bit 0 reached, bit 1 forced */, int32_t *parent_out /* R */,
                           uint64_t *q_out /* R */, uint64_t *qsum_out /* npop */, double *href_out /* npop */);
/* any output pointer may be NULL */
int smolmc_get_state(smolmc_handle *h, int32_t *occ /*RxN*/, double *features /*RxF*/,
                     double *enthalpy /*R*/, uint64_t *n_accepted /*R*/,
                     uint64_t *n_steps /*R*/, uint8_t *last_accepted /*R*/);
/* WangLandau trace extras (wanglandau.py:247-251,268-288); NULLs allowed */
/* trace.bias of every walker (kernel/base.py:362-363 + accumulated delta_trace.bias);
 * error when the model has no bias term */
int smolmc_get_bias(smolmc_handle *h, double *bias /*R*/);
int smolmc_get_wl(smolmc_handle *h, double *entropy /*RxL*/, int64_t *histogram /*RxL*/,
                  int64_t *occurrences /*RxL*/, double *mean_features /*RxLxF*/,
                  double *mod_factor /*R*/);

/* Restore of a kernel's auxiliary state in a fresh handle / process: the inverse of smolmc_get_wl
 * (WangLandau._entropy, _histogram, _occurrences, _mean_features, _m, wanglandau.py:107-122, which
 * set_aux_state resets, :290-300; the reference's SampleContainer carries an `aux_checkpoint`
 * placeholder it never fills, sampler/container.py:89,539-541).  Arrays as smolmc_get_wl returns
 * them; NULL = leave as it is.  Also what a host-side `mod_update` callable needs
 * (wanglandau.py:100-105): download, apply, upload. */
int smolmc_set_wl(smolmc_handle *h, const double *entropy /*RxL*/, const int64_t *histogram /*RxL*/,
                  const int64_t *occurrences /*RxL*/, const double *mean_features /*RxLxF*/,
                  const double *mod_factor /*R*/);
/* Step / accept counters of every walker.  n_steps is the walker's position in its random stream
 * (Philox counter) and, for Wang-Landau, the step counter the check period refers to
 * (WangLandau._steps_counter).  Resume in a fresh handle / process, bit for bit:
 * smolmc_set_state(occ, seeds, T, reset_aux = 1) -- the seeds are only taken with reset_aux != 0 --
 * then smolmc_set_counters and, for Wang-Landau, smolmc_set_wl.  NULL = leave as it is. */
int smolmc_set_counters(smolmc_handle *h, const uint64_t *n_steps /*R*/, const uint64_t *n_accepted /*R*/);

/* ---- the hot path -------------------------------------------------------- */
/* Advance every walker nsteps MC steps: the body of Sampler.sample
 * (sampler/sampler.py:195-208) = MCUsher.propose_step + compute_feature_vector_change
 * + accept + in-place update + trace accumulation, engine RNG (Philox4x32-10
 * keyed by the walker seed, counter = step index).
 * Asynchronous on the handle's stream; smolmc_sync() or any get_* waits. */
int smolmc_run(smolmc_handle *h, int64_t nsteps);
int smolmc_sync(smolmc_handle *h);
/* Device-side thinning: advance nsamples x thin_by steps and record, after every thin_by
 * steps, one row per walker -- what Sampler.sample yields and
 * SampleContainer.save_sampled_trace stores (sampler/sampler.py:195-210,
 * container.py:384-397): enthalpy, features, the accept flag of the last step of the
 * block and, as `flags` asks (SMOLMC_SAMPLE_*): the occupancy; trace.bias (kernel/base.py:307-311,
 * 362-363); the Wang-Landau trace (wanglandau.py:247-251: entropy, histogram, occurrences,
 * cumulative mean features, mod_factor of every walker AT that sample).
 *
 * A sample ring of two slots (ABI 7): the call returns as soon as the launches are queued; when they
 * finish the block is copied to a pinned host mirror on a stream of its own, so that the download of
 * block k overlaps the kernel of block k + 1 (the reference streams samples while it runs,
 * sampler/sampler.py:286-291, container.py:420-437).  The intended sequence is
 *     run_sampled(0); run_sampled(1); get_samples -> block 0; run_sampled(2); get_samples -> block 1; ...
 * smolmc_get_samples* deliver the OLDEST block not yet delivered (waiting for its copy only, not for
 * younger launches); with none pending they deliver the newest block again.  A third
 * smolmc_run_sampled while two blocks are pending is REFUSED with SMOLMC_ERR_RING_FULL and changes nothing
 * (ABI 8; ABI 7 silently dropped the older block) -- fetch or smolmc_discard_samples first.  A call that fails
 * for any other reason (arguments, an allocation, a launch) leaves the ring as it was: the slot is taken only
 * when every launch of the block has been queued.  Nothing is allocated per call once the slots have grown
 * to the block size. */
#define SMOLMC_SAMPLE_OCCUPANCY 1 /* flags bit 0 */
#define SMOLMC_SAMPLE_BIAS 2      /* flags bit 1: trace.bias (error without an MCBias term) */
#define SMOLMC_SAMPLE_WL 4        /* flags bit 2: the Wang-Landau trace (error on a Metropolis handle) */
#define SMOLMC_SAMPLE_OBSERVABLES 8 /* flags bit 3: kind and pair counts of every row (see smolmc_set_observables) */
#define SMOLMC_SAMPLE_MINIMA 16     /* flags bit 4: offer every row to the minima record (see smolmc_set_minima) */
#define SMOLMC_SAMPLE_STATISTICS 32 /* flags bit 5: offer every row to the statistics record (see smolmc_set_statistics) */
#define SMOLMC_SAMPLE_STRUCTURE 64  /* flags bit 6: structure-factor amplitudes and intensities of every row (see smolmc_set_structure) */
int smolmc_run_sampled(smolmc_handle *h, int64_t nsamples, int64_t thin_by, int flags);
/* The ring as the next smolmc_get_samples* call sees it (ABI 8): *n_pending = blocks queued and not fetched
 * (0..2), *nsamples / *flags = sample count and SMOLMC_SAMPLE_* flags of the block that call would deliver
 * (0 / 0 when the ring is empty) -- get_samples takes no array lengths, a caller that did not queue the
 * block itself sizes its arrays from here (container.py:409-413 allocates from nsamples the same way).
 * Any pointer may be NULL. */
int smolmc_pending_samples(smolmc_handle *h, int *n_pending, int64_t *nsamples, int *flags);
/* Forget every block of the ring, fetched or not: what a sampling loop that is abandoned half way
 * (an exception between two blocks, sampler/sampler.py:195-210 left early) calls so that the next loop
 * does not receive its blocks.  The walkers keep the state the queued launches leave them in. */
int smolmc_discard_samples(smolmc_handle *h);
/* [nsamples x R (x F | x N)], NULLs allowed */
int smolmc_get_samples(smolmc_handle *h, double *enthalpy, double *features,
                       uint8_t *accepted, int32_t *occupancy);
/* smolmc_get_samples with the occupancies as bytes, [nsamples x R x N] uint8 -- the device
 * ring's own format: a quarter of the PCIe traffic and host memory of the int32 form the
 * reference's trace uses (trace.occupancy is int32, sampler/sampler.py:411-415; codes are
 * < 256 by construction, smolmc_tables.n_codes). */
int smolmc_get_samples_u8(smolmc_handle *h, double *enthalpy, double *features,
                          uint8_t *accepted, uint8_t *occupancy);
/* ... and the columns ABI 7 added (each may be NULL; asking for one that was not recorded is an error):
 * bias [nsamples x R]; wl_entropy / wl_histogram / wl_occurrences [nsamples x R x L], wl_mean_features
 * [nsamples x R x L x F], wl_mod_factor [nsamples x R] (as smolmc_get_wl returns them, at every sample). */
int smolmc_get_samples_ex(smolmc_handle *h, double *enthalpy, double *features, uint8_t *accepted,
                          uint8_t *occupancy_u8, double *bias, double *wl_entropy, int64_t *wl_histogram,
                          int64_t *wl_occurrences, double *wl_mean_features, double *wl_mod_factor);
/* ---- observables: species and pair counts of sampled states, reduced on the device ---------------------------
 * (no reference counterpart: the reference's container scans the stored occupancies on the host,
 * sampler/container.py:226-262).  Two int32 vectors per occupancy row:
 *   counts[K]                 how many counted sites hold each KIND; the kind of (site, code) is kind_base[site] + code,
 *                             kind_base[site] = -1 leaves the site out
 *   pairs[n_shells][K][K]     for every bond (i, j) of a shell, as listed, cell (kind(i), kind(j)) gains 1; a bond with
 *                             an end that is not counted is skipped; duplicate rows and i == j rows count as they stand
 * Site numbers are the caller's.  The engine copies and uploads everything.  smolmc_eval_observables refuses a code that
 * gives a kind >= K; in the walkers' own states that can only happen on a fixed site outside every cluster (the tables
 * do not say how many codes such a site has), and such a site is then left out. */
#define SMOLMC_MAX_OBS_CELLS 4096 /* most pair cells n_shells x K x K (16 KB of int32: with the row and the kind counts
                                   * they share 64 KB of LDS of one workgroup) */
typedef struct {
    int n_kinds;              /* K, 1..254 */
    const int32_t *kind_base; /* [N] */
    int n_shells;
    const int64_t *shell_ptr; /* [n_shells + 1], ascending from 0 */
    const int32_t *bonds;     /* [shell_ptr[n_shells] x 2] */
} smolmc_observables;
/* Sets (NULL: removes) the observables of the handle.  Refused, each naming its reason: a bond out of range; a site with
 * kind_base[s] + (species codes on s) > n_kinds; more than SMOLMC_MAX_OBS_CELLS cells; a row too long to stage in LDS
 * next to the histograms; and while a block recorded with SMOLMC_SAMPLE_OBSERVABLES waits in the ring.  A refused call
 * leaves the handle's observables as they were. */
int smolmc_set_observables(smolmc_handle *h, const smolmc_observables *obs);
/* K and n_shells in force (0, 0: none set) */
int smolmc_observables_shape(smolmc_handle *h, int *n_kinds, int *n_shells);
/* counts [nocc x K] and pairs [nocc x n_shells x K x K] of nocc occupancies (host, int32 like smolmc_eval_full), or, with
 * occ == NULL, of the walkers' current states (nocc = R then).  Either output may be NULL. */
int smolmc_eval_observables(smolmc_handle *h, const int32_t *occ /* nocc x N, or NULL */, int nocc, int32_t *counts,
                            int32_t *pairs);
/* With SMOLMC_SAMPLE_OBSERVABLES smolmc_run_sampled adds the two columns [rows x K] and [rows x n_shells x K x K] to the
 * block, filled on the device from the block's occupancy rows when its launches are through; without
 * SMOLMC_SAMPLE_OCCUPANCY those rows never leave the device.  The flag is refused while no observables are set.  This
 * call reads the columns of the block the next smolmc_get_samples* call delivers ([nsamples x R x ...], either may be
 * NULL) and does not mark it delivered, like smolmc_pending_samples; an error when that block was recorded without
 * the flag. */
int smolmc_get_sample_observables(smolmc_handle *h, int32_t *counts, int32_t *pairs);
/* ---- minima: the lowest recorded states, kept on the device ------------------------------------------------------
 * (the reference's container takes an argmin over stored occupancies, sampler/container.py:306-334; here the rows of a
 * block are reduced where they lie and only the record is ever downloaded).  A minima record is a table of n_slots
 * entries that lives as long as the handle.  Every recorded sample is OFFERED to the entry its key selects:
 *   n_axes == 0   one slot per walker, the key is the walker index (n_slots = R)
 *   n_axes 1..4   the key comes from the sample's kind counts (the observables' counts[K]): on axis a
 *                 d_a = sum_k axis_weights[a][k] * counts[k] (int64), c_a = floor(d_a / axis_bin[a]); the row is skipped
 *                 unless 0 <= c_a < axis_extent[a] on every axis; the key is the mixed-radix number of the c_a, axis 0
 *                 slowest (n_slots = product of the extents)
 * The value that is minimised: the enthalpy (n_weights == 0), or sum_{i < n_weights} weights[i] * features[i] taken left
 * to right, every product and every sum rounded on its own (no fused multiply-add).  Values are compared as v + 0.0
 * (-0.0 and +0.0 are one value); a NaN never wins.  Offers are numbered from 0 since the last reset in launch order:
 * each sample of a block recorded with SMOLMC_SAMPLE_MINIMA is one offer, each smolmc_update_minima call is one.  A
 * strictly lower value replaces the entry; among equal values the earliest offer wins, within one offer the lowest
 * walker.  An entry holds value, enthalpy, features [F], occupancy [N] (the caller's site numbering), counts [K] (zeros
 * without observables), walker, sample (the offer number) and step (the walker's n_steps at that sample).  An empty
 * entry reads value = +inf, walker = -1, sample = -1 and zeros elsewhere.
 * smolmc_set_state and smolmc_discard_samples leave the record alone: it belongs to the handle, not to a block. */
#define SMOLMC_MAX_MINIMA_AXES 4
typedef struct {
    int n_weights;               /* 0: the enthalpy column */
    const double *weights;       /* [n_weights], n_weights <= F */
    int n_axes;                  /* 0: one slot per walker */
    const int32_t *axis_weights; /* [n_axes x K], K of the observables in force */
    const int32_t *axis_bin;     /* [n_axes], each >= 1 */
    const int32_t *axis_extent;  /* [n_axes], each >= 1 */
} smolmc_minima;
/* Sets the record (NULL: removes it); a new spec starts an empty record.  Refused, each naming its reason and leaving
 * the handle as it was: n_axes > 0 without observables; n_weights > F; a bin or an extent below 1; more than 2^20 slots
 * or a record of more than 1 GiB (n_slots x (Npad + 8 F + 4 K + 40) bytes).  While a keyed record is set,
 * smolmc_set_observables is refused.  Waits for the handle's stream (queued blocks still write the record), like
 * smolmc_reset_minima and smolmc_get_minima. */
int smolmc_set_minima(smolmc_handle *h, const smolmc_minima *m);
/* n_slots and n_axes in force (0, 0: none set) */
int smolmc_minima_shape(smolmc_handle *h, int *n_slots, int *n_axes);
/* Offers the walkers' CURRENT states, one offer (for callers of smolmc_run); a keyed record counts the kinds of the
 * current states on the device first. */
int smolmc_update_minima(smolmc_handle *h);
/* Empties the record; the offer numbering restarts at 0. */
int smolmc_reset_minima(smolmc_handle *h);
/* The record: value, enthalpy, walker, sample, step [n_slots]; features [n_slots x F]; occ [n_slots x N]; counts
 * [n_slots x K].  Any pointer may be NULL. */
int smolmc_get_minima(smolmc_handle *h, double *value, double *enthalpy, double *features, int32_t *occ,
                      int32_t *counts, int32_t *walker, int64_t *sample, uint64_t *step);
/* A per-walker record also keeps the COMPANIONS of walker 0's entry: the occupancy of every walker at the offer that
 * entry was taken from, occ [R x N] in the caller's numbering (zeros while the entry is empty).  It is what the
 * reference's get_minimum_*_occupancy(flat=False) returns (sampler/container.py:316-318: every walker's occupancy at the
 * sample where walker 0 was lowest).  Refused on a record keyed by composition.  Waits for the handle's stream. */
int smolmc_get_minima_companions(smolmc_handle *h, int32_t *occ);
/* ---- statistics: running moments, blocking sums and a histogram of the samples, kept on the device -----------------
 * A statistics record is a set of accumulators per KEY that lives as long as the handle.  Every recorded sample is
 * OFFERED to it: each sample of a block recorded with SMOLMC_SAMPLE_STATISTICS is one offer, each
 * smolmc_update_statistics call is one.  One offer gives every key exactly one row of C column values x[C] (both key
 * modes are permutations of the walkers), and the key's accumulators take it in launch order:
 *   if n == 0: shift[c] = x[c]                       (the key's first offered value)
 *   d[c] = x[c] - shift[c];  s1[c] += d[c];  s2[a,b] += d[a] * d[b] for a <= b   (upper triangle, row-major)
 *   blocking (Flyvbjerg & Petersen 1989), per column c:  carry = d[c]; for l = 0 .. n_levels - 1:
 *       b2[l,c] += carry * carry; nb[l] += 1 (once per level);
 *       bit l of has[c] clear: pend[l,c] = carry, set the bit, stop;   else carry = pend[l,c] + carry, clear the bit
 *   histogram of column hist_column: q = floor((x - hist_min) / hist_bin), the exact floor division of the Wang-Landau
 *       step; q < 0 counts in under, q >= n_bins or x not finite in over, else hist[q] += 1
 *   n += 1
 * Every product and every sum is rounded on its own (no fused multiply-add): smol_amd/statistics.py is the same in NumPy
 * and the device matches it entry for entry.  smolmc_set_state and smolmc_discard_samples leave the record alone. */
#define SMOLMC_STAT_BY_WALKER 0      /* n_keys = R, the key is the walker */
#define SMOLMC_STAT_BY_STATE_POINT 1 /* n_keys = R, the key is the state point the walker holds when the reduction runs
                                      * on the handle's stream (the identity while smolmc_exchange_grid has never run) */
#define SMOLMC_STAT_BY_BIN 2         /* n_keys bins of one of the columns (smolmc_set_statistics_binned, below) */
#define SMOLMC_MAX_STAT_KEYS 65536   /* bins of a record keyed by bin */
#define SMOLMC_MAX_STAT_COLUMNS 32
#define SMOLMC_MAX_STAT_LEVELS 32
#define SMOLMC_MAX_STAT_BINS 65536
typedef struct smolmc_statistics {
    int key;                /* SMOLMC_STAT_BY_WALKER or SMOLMC_STAT_BY_STATE_POINT; SMOLMC_STAT_BY_BIN only through
                             * smolmc_set_statistics_binned */
    int n_columns;          /* C, 1..32 */
    const int32_t *columns; /* [C] sources, no duplicates: 0 the enthalpy, 1 + i feature i (i < F), 1 + F + k kind count k
                             * of the observables in force (k < K, as a double), 1 + F + K the weighted sum below,
                             * 2 + F + K + i intensity i of the structure-factor spec in force (i < I, see
                             * smolmc_set_structure; with no spec set the range ends at the weighted sum); behind them
                             * the connectivity numbers, the pattern cells and the environment cells
                             * (smolmc_get_sample_connectivity, smolmc_get_sample_patterns,
                             * smolmc_get_sample_environments) */
    int n_weights;          /* the weighted sum: sum_{i < n_weights} weights[i] * features[i] left to right, the value of */
    const double *weights;  /* a minima record (n_weights <= F) */
    int n_levels;           /* blocking levels, 0..32 */
    int hist_column;        /* an index into columns */
    int n_bins;             /* 0: no histogram, else 1..65536 */
    double hist_min, hist_bin; /* hist_bin > 0 */
} smolmc_statistics;
/* Sets the record (NULL: removes it); a new spec starts an empty record.  Refused, each naming its reason and leaving
 * the handle as it was: a key other than the two; SMOLMC_STAT_BY_STATE_POINT on a Wang-Landau handle with per-walker
 * windows; C outside 1..32, a source out of range or named twice; a count column without observables; n_weights > F;
 * n_levels outside 0..32; n_bins outside 0..65536, hist_bin not a positive finite number, hist_column outside the
 * columns; a record of more than 1 GiB.  While a record with count columns is set, smolmc_set_observables is refused,
 * and smolmc_set_structure while a record with intensity columns is set.
 * Waits for the handle's stream, like smolmc_reset_statistics and smolmc_get_statistics. */
int smolmc_set_statistics(smolmc_handle *h, const smolmc_statistics *s);
/* ---- statistics keyed by BINS of a column (SMOLMC_STAT_BY_BIN): microcanonical averages, averages per composition ----
 * A key of this mode gathers several rows of a sample, or none.  The rows of an offer are taken SAMPLE BY SAMPLE, AND
 * WITHIN A SAMPLE IN WALKER ORDER 0 .. R - 1.  For each row:
 *   q = floor((x[key_column] - key_min) / key_bin), the exact floor division of the Wang-Landau step and of the record's
 *       histogram
 *   q < 0 counts in key_under, ONE int64 for the whole record; q >= n_keys, or a value that is not finite, counts in
 *       key_over; neither row is offered to any key
 *   every other row is offered to key q by the rule above: the key's first row is the shift, then s1, the s2 triangle,
 *       the per-key histogram of hist_column with the key's under and over, and n += 1
 * Blocking means nothing when successive rows of a key come from different walkers: n_levels must be 0, and the record's
 * arrays keep their shapes with n_levels = 0.  Every product and every sum is rounded on its own, as above.  The
 * walker-to-state-point map is not read.
 * s->key must be SMOLMC_STAT_BY_BIN; key_column is an index into s->columns, like hist_column.  Makes every check
 * smolmc_set_statistics makes and refuses further, each naming its reason and leaving the record in force untouched:
 * n_levels != 0; n_keys outside 1..65536; key_bin not a positive finite number or key_min not finite; key_column outside
 * the columns; a record of more than 1 GiB.  Allowed on a Wang-Landau handle with per-walker windows: the key is the
 * row's value, not the walker.  smolmc_set_statistics itself keeps refusing key 2.  Everything else is the one record:
 * smolmc_statistics_shape and smolmc_get_statistics report n_keys bins, SMOLMC_SAMPLE_STATISTICS blocks offer their rows,
 * smolmc_update_statistics offers one sample of R rows, smolmc_reset_statistics also clears the two outside counters, and
 * the refusals of smolmc_set_observables, smolmc_set_structure and the rest count the key column like any other. */
int smolmc_set_statistics_binned(smolmc_handle *h, const smolmc_statistics *s, int key_column, int n_keys, double key_min,
                                 double key_bin);
/* The binned spec in force and its two outside counters; all zeros when the record in force is not binned (or none is
 * set).  Any pointer may be NULL.  Waits for the handle's stream when a counter is asked for. */
int smolmc_statistics_bins(smolmc_handle *h, int *key_column, int *n_keys, double *key_min, double *key_bin,
                           int64_t *key_under, int64_t *key_over);
/* the shape in force (all 0: none set) */
int smolmc_statistics_shape(smolmc_handle *h, int *n_keys, int *n_columns, int *n_levels, int *n_bins);
/* Offers the walkers' CURRENT states, one offer (for callers of smolmc_run); with count columns the kinds of the current
 * states are counted on the device first, with intensity columns their intensities are evaluated first. */
int smolmc_update_statistics(smolmc_handle *h);
/* Empties the record. */
int smolmc_reset_statistics(smolmc_handle *h);
/* The record: n, under, over [n_keys]; shift, s1 [n_keys x C]; s2 [n_keys x C (C + 1) / 2]; has [n_keys x C] (bit l:
 * pend[l, c] holds a pending block); pend, b2 [n_keys x n_levels x C]; nb [n_keys x n_levels]; hist [n_keys x n_bins].
 * Any pointer may be NULL. */
int smolmc_get_statistics(smolmc_handle *h, int64_t *n, double *shift, double *s1, double *s2, uint64_t *has, double *pend,
                          double *b2, int64_t *nb, int64_t *hist, int64_t *under, int64_t *over);
/* ---- the site field of a statistics record: how often every tracked site held every species code, per key -------------
 * A record may carry a SITE FIELD: site_counts[n_keys][M][S] and site_over[n_keys], int64.  The M tracked sites are a list
 * of distinct site numbers in the caller's numbering (NULL: all N sites, in order); S = n_codes, 1..16.  For every row that
 * the record's rule offers to key k, and for every tracked site m with code c in that row's occupancy:
 *   c < S:      site_counts[k][m][c] += 1
 *   otherwise:  site_over[k] += 1
 * The rows offered are the rows that increment n[k]: one per key and sample in the two permutation modes, the rows inside
 * the bins in SMOLMC_STAT_BY_BIN; rows counted in key_under / key_over touch nothing.  Hence
 *   sum over m, c of site_counts[k][m][c] + site_over[k] == M * n[k]
 * as long as field and record were reset together.  site_counts[k][m][c] / n[k] is the site-resolved average
 * <delta(sigma_m, c)> of key k.  Sums of integers: the field does not depend on the order of the adds, and the device
 * equals smol_amd/statistics.py (StatisticsRecord.offer with occupancy rows) entry for entry.
 *
 * Attaches a field to the record IN FORCE, in any key mode, and zeroes the field (the record's other accumulators stay);
 * n_codes = 0 detaches it (sites and n_sites are not read).  Refused, each naming its reason and leaving record and field
 * untouched: no record set; n_codes outside 0..16; an empty list, a site outside 0..N-1 or listed twice; record plus
 * field larger than 1 GiB; while a block recorded with SMOLMC_SAMPLE_STATISTICS waits in the ring.  Setting a record
 * (smolmc_set_statistics, smolmc_set_statistics_binned) drops the field: a new spec starts an empty record.
 * smolmc_reset_statistics also clears the field, smolmc_update_statistics offers the walkers' current states to it as well.
 * A SMOLMC_SAMPLE_STATISTICS block on a record with a field keeps the block's occupancy rows on the device, whether or
 * not SMOLMC_SAMPLE_OCCUPANCY is set (without it they never leave the device); the field's launch is ordered on the
 * handle's stream behind the block's launches and in front of the slot's reuse.  Chains are not affected.
 * Waits for the handle's stream. */
#define SMOLMC_MAX_STAT_SITE_CODES 16
int smolmc_set_statistics_sites(smolmc_handle *h, const int32_t *sites /* [n_sites] or NULL */, int n_sites, int n_codes);
/* the field in force (both 0: none set) */
int smolmc_statistics_sites_shape(smolmc_handle *h, int *n_sites, int *n_codes);
/* The field: site_counts [n_keys x M x S], site_over [n_keys]; either pointer may be NULL.  Columns are in the caller's
 * order: tracked site m is the m-th entry of the list given (on a relabelled handle the engine reads byte new_of[p] of a
 * ring row for the caller's site p, as smolmc_get_minima does).  Waits for the handle's stream. */
int smolmc_get_statistics_sites(smolmc_handle *h, int64_t *site_counts, int64_t *site_over);
/* ---- the joint field of a statistics record: a histogram of TWO columns, per key ----------------------------------------
 * A record may carry a JOINT FIELD: joint[n_keys][n_a][n_b] and joint_out[n_keys], int64.  column_a and column_b are
 * indices into the record's columns, like hist_column; they may be equal.  For every row that the record's rule offers to
 * key k -- the rows that increment n[k] in any of the three key modes: one per key and sample by walker and by state
 * point, the rows inside the bins in SMOLMC_STAT_BY_BIN, never a row counted in key_under / key_over --
 *   qa = floor((x[column_a] - min_a) / bin_a),  qb = floor((x[column_b] - min_b) / bin_b)
 * as numpy.floor_divide gives them, and
 *   both values finite, 0 <= qa < n_a and 0 <= qb < n_b:   joint[k][qa][qb] += 1
 *   otherwise:                                             joint_out[k] += 1
 * This is the floor division of the histogram and of the Wang-Landau step with one difference: a value below min is
 * ALWAYS outside.  The histogram's division puts x with -ulp(bin) / 2 <= x - min < 0 in bin 0 (its remainder x - min + bin
 * rounds to bin), so for one column with one min and bin the sum of joint over the other axis and hist can differ by the
 * rows that lie that close below min; everywhere else the two agree.
 * Hence
 *   sum over qa, qb of joint[k][qa][qb] + joint_out[k] == n[k]
 * as long as field and record were reset together.  joint[k] is H_k(a, b), the joint histogram of key k: with the key a
 * state point of a semigrand handle, column_a the energy (the weighted sum of the features with weight 0 on the
 * chemical-work feature; NOT the enthalpy column, which already contains -mu N) and column_b a kind count it is what
 * reweighting in T and mu, the multiple-histogram method and the equal-weight rule read.  Sums of integers: the field does
 * not depend on the order of the adds, and the device equals smol_amd/statistics.py (StatisticsRecord.offer) entry for
 * entry.
 *
 * Attaches a field to the record IN FORCE, in any key mode, and zeroes the field (the record's other accumulators and a
 * site field stay); n_a = 0 detaches it (nothing else is read).  Refused, each naming its reason and leaving record and
 * fields untouched: no record set; n_a outside 0..65536 or n_b outside 1..65536; a bin width that is not a positive finite
 * number or a minimum that is not finite; a column outside the record's columns; record plus both fields larger than
 * 1 GiB (smolmc_set_statistics_sites counts a joint field in force likewise); while a block recorded with
 * SMOLMC_SAMPLE_STATISTICS waits in the ring.  Setting a record (smolmc_set_statistics, smolmc_set_statistics_binned)
 * drops the field, smolmc_reset_statistics also clears it, smolmc_update_statistics offers the walkers' current states to
 * it as well.  A joint field and a site field may be attached together.  The field's launch is one more mode of the
 * record's kernel, ordered on the handle's stream behind the record's launches; a record without a joint field launches
 * what it launched.  Waits for the handle's stream. */
#define SMOLMC_MAX_STAT_JOINT_CELLS 65536
int smolmc_set_statistics_joint(smolmc_handle *h, int column_a, int n_a, double min_a, double bin_a, int column_b, int n_b,
                                double min_b, double bin_b);
/* the field in force (all 0: none set); any pointer may be NULL */
int smolmc_statistics_joint_shape(smolmc_handle *h, int *column_a, int *n_a, double *min_a, double *bin_a, int *column_b, int *n_b,
                                  double *min_b, double *bin_b);
/* The field: joint [n_keys x n_a x n_b], joint_out [n_keys]; either pointer may be NULL.  Waits for the handle's stream. */
int smolmc_get_statistics_joint(smolmc_handle *h, int64_t *joint, int64_t *joint_out);

/* ---- structure factors: fixed-point amplitudes and intensities of sampled states, reduced on the device ---------------
 * (no reference counterpart).  Kinds as in smolmc_observables: the kind of (site, code) is kind_base[site] + code,
 * kind_base[site] = -1 leaves the site out.  For every wave vector ("point") q every site j has a phase class
 * phase[q][j] < n_phases, and every class the fixed-point pair table[q][m] = (cos, -sin) of its angle.  Per occupancy row
 *   amp[q][k][c] = sum over counted sites j with kind(j) == k of table[q][phase[q][j]][c]            (int64, c = 0, 1)
 *   inten[i]     = ((double)amp[q][a][0] * (double)amp[q][b][0] + (double)amp[q][a][1] * (double)amp[q][b][1]) * scale[i]
 *                  for intensity[i] = (q, a, b)
 * The sums are integer sums, so their order is of no concern; every floating product and sum of inten is rounded on its
 * own (no fused multiply-add).  smol_amd/structure.py is the same in NumPy and the device matches it entry for entry.
 * The engine knows no geometry: the caller supplies phase and table (structure.StructureFactor.from_supercell makes
 * them).  Site numbers are the caller's.  The engine copies and uploads everything. */
#define SMOLMC_MAX_STRUCT_POINTS 4096  /* Q: an amplitude column of a row is Q x K x 16 bytes and the phase table Q x N x 2
                                        * bytes; with rows of at most 65535 sites the table stays below 512 MiB */
#define SMOLMC_MAX_STRUCT_PHASES 65535 /* M: a phase class is a uint16 */
#define SMOLMC_MAX_STRUCT_CELLS 12288  /* K x M, the (kind, phase class) counters of one point: 48 KB of int32, which
                                        * share the 64 KB of LDS of one workgroup with the row */
#define SMOLMC_MAX_STRUCT_INTENSITIES 4096 /* I: one thread pass of the epilogue per 256; keeps a row's column at 32 KB */
typedef struct smolmc_structure {
    int n_kinds;                   /* K, 1..254 */
    const int32_t *kind_base;      /* [N] */
    int n_points;                  /* Q, 1..SMOLMC_MAX_STRUCT_POINTS */
    int n_phases;                  /* M, 1..SMOLMC_MAX_STRUCT_PHASES, K x M <= SMOLMC_MAX_STRUCT_CELLS */
    const uint16_t *phase;         /* [Q x N], every entry < M */
    const int64_t *table;          /* [Q x M x 2] */
    int n_intensities;             /* I, 0..SMOLMC_MAX_STRUCT_INTENSITIES */
    const int32_t *intensity;      /* [I x 3]: point q, kind a, kind b */
    const double *intensity_scale; /* [I] */
} smolmc_structure;
/* Sets (NULL: removes) the structure-factor spec of the handle.  Refused, each naming its reason: a phase >= n_phases; a
 * site with kind_base[s] + (species codes on s) > n_kinds (a fixed site outside every cluster needs one kind, as for the
 * observables); Q, M, K, K x M or I beyond the limits above; a row too long to stage in LDS next to the counters;
 * N_counted x max|table| >= 2^62 (a sum could overflow); an intensity naming a point or kind out of range; a scale that
 * is not finite; while a block recorded with SMOLMC_SAMPLE_STRUCTURE waits in the ring; while a statistics record with
 * intensity columns is set.  A refused call leaves the handle's spec as it was. */
int smolmc_set_structure(smolmc_handle *h, const smolmc_structure *s);
/* Q, K and I in force (all 0: none set) */
int smolmc_structure_shape(smolmc_handle *h, int *n_points, int *n_kinds, int *n_intensities);
/* amp [nocc x Q x K x 2] and inten [nocc x I] of nocc occupancies (host, int32 like smolmc_eval_full), or, with
 * occ == NULL, of the walkers' current states (nocc = R then).  Either output may be NULL. */
int smolmc_eval_structure(smolmc_handle *h, const int32_t *occ /* nocc x N, or NULL */, int nocc, int64_t *amp, double *inten);
/* With SMOLMC_SAMPLE_STRUCTURE smolmc_run_sampled adds the two columns [rows x Q x K x 2] (int64) and [rows x I] (double)
 * to the block, filled on the device from the block's occupancy rows when its launches are through; without
 * SMOLMC_SAMPLE_OCCUPANCY those rows never leave the device.  The flag is refused while no spec is set.  This call reads
 * the columns of the block the next smolmc_get_samples* call delivers ([nsamples x R x ...], either may be NULL) and does
 * not mark it delivered, like smolmc_get_sample_observables; an error when that block was recorded without the flag. */
int smolmc_get_sample_structure(smolmc_handle *h, int64_t *amp, double *inten);

/* ---- connectivity: connected components of sampled states and whether they span the cell, on the device ---------------
 * (no reference counterpart).  Kinds as in smolmc_observables.  A spec holds G graphs.  Graph g has member kinds (bit k
 * of the 256-bit row member_mask[g]) and the bonds bond_ptr[g] .. bond_ptr[g + 1]: bond (i, j, w) joins site i of the home
 * cell to site j of the periodic image displaced by w[0] S_0 + w[1] S_1 + w[2] S_2, S_a the supercell vectors.  A site is
 * a member when its kind is one; a bond is active when both ends are members.  Duplicate rows, rows i == j with w != 0 and
 * rows that join the same sites by different images are legal.  Components are the connected components of the members
 * under the active bonds; a component wraps axis a when the image sum over one of its closed paths has a nonzero entry a.
 * Per occupancy row and graph: the SMOLMC_CONN_STATS numbers below, and per site the smallest site number of its
 * component (-1: no member).  Everything is integer; smol_amd/connectivity.py is the same in NumPy and the device matches
 * it entry for entry.  Site numbers are the caller's.  The engine copies and uploads everything. */
#define SMOLMC_MAX_CONN_GRAPHS 8
#define SMOLMC_MAX_CONN_IMAGE 7       /* |w[a]| of a bond */
#define SMOLMC_MAX_CONN_PATH_SUM 32767 /* the kernel keeps the image sum of a path in 16 bits an axis: N x
                                        * SMOLMC_MAX_CONN_IMAGE must not exceed it (N <= 4681) */
#define SMOLMC_CONN_STATS 24          /* numbers per row and graph: */
#define SMOLMC_CONN_N_MEMBERS 0
#define SMOLMC_CONN_N_COMPONENTS 1
#define SMOLMC_CONN_LARGEST 2         /* size of the largest component, 0 if none */
#define SMOLMC_CONN_SUM_SQ 3          /* sum of size^2 */
#define SMOLMC_CONN_N_WRAPPING 4      /* components that wrap any axis */
#define SMOLMC_CONN_WRAPPING_SITES 5  /* members in wrapping components */
#define SMOLMC_CONN_WRAP_AXES 6       /* OR over the components of their 3-bit axis mask */
#define SMOLMC_CONN_LARGEST_WRAP_AXES 7 /* axis mask of the largest component; among equals the one with the smallest label */
#define SMOLMC_CONN_HIST 8            /* 8 + b, b = 0..15: components with floor(log2 size) == b */
typedef struct smolmc_connectivity {
    int n_kinds;
    const int32_t *kind_base;      /* [N] */
    int n_graphs;
    const uint64_t *member_mask;   /* [G x 4], bit k: kind k is a member */
    const int64_t *bond_ptr;       /* [G + 1] */
    const int32_t *bonds;          /* [nb x 2] */
    const int8_t *images;          /* [nb x 3] */
} smolmc_connectivity;
/* Sets (NULL: removes) the connectivity spec of the handle.  Refused, each naming its reason: a bond out of range; a site
 * with kind_base[s] + (species codes on s) > n_kinds, or a member kind >= n_kinds; n_kinds outside 1..254; G outside
 * 1..SMOLMC_MAX_CONN_GRAPHS; an image beyond SMOLMC_MAX_CONN_IMAGE; N x SMOLMC_MAX_CONN_IMAGE > SMOLMC_MAX_CONN_PATH_SUM
 * or a row whose labels, path sums and sizes do not fit the LDS of one workgroup (rows of 4096 sites fit); while a block
 * recorded with SMOLMC_SAMPLE_CONNECTIVITY waits in the ring; while a statistics record with connectivity columns is set.
 * A refused call leaves the handle's spec as it was. */
int smolmc_set_connectivity(smolmc_handle *h, const smolmc_connectivity *s);
/* Gated bonds.  Bond row b (counted over all graphs, b < nb = bond_ptr[G]) may carry 0..SMOLMC_MAX_CONN_GATES gate sites
 * gate_sites[gate_ptr[b] .. gate_ptr[b + 1]], caller's site numbers; an occupancy is periodic, so a gate site has no image.
 * A gate site is blocked when its kind is not in the 256-bit row gate_mask[g] of the row's graph; a site listed twice in a
 * row counts twice.  A row is open when both ends are members and at most max_blocked[g] of its gate sites are blocked; a
 * row without gate sites is open whenever both ends are members.  The adjacency (i, j, w) with its reverse (j, i, -w) is
 * active when at least one row that lists it, in either direction, is open: components, winding sets, the 24 numbers and
 * the labels are those of the active adjacencies.  (The 0-TM channels of a disordered rocksalt: the rows of a Li-Li bond
 * are its two tetrahedra, the gate sites the two other corners, gate_mask the kinds that are no transition metal,
 * max_blocked = 0.)  A graph none of whose rows has a gate site is ungated: its results and its path through the kernel
 * are those of smolmc_set_connectivity.  smolmc_set_connectivity(h, s) is smolmc_set_connectivity_gated(h, s, NULL).
 * Refused besides what smolmc_set_connectivity refuses, each naming its reason and leaving the spec as it was: a gate site
 * out of range or with kind_base < 0; more than SMOLMC_MAX_CONN_GATES gates on a row; gate_ptr not starting at 0 or
 * decreasing; a gate kind >= n_kinds; max_blocked outside 0..SMOLMC_MAX_CONN_GATES; a gated graph in which a site has more
 * than SMOLMC_MAX_CONN_GATED_NEIGHBOURS distinct (neighbour, image) entries; a row whose open bits (one per entry, four
 * entries to a group) do not fit the LDS of one workgroup next to the rest (rows of 4096 sites with the 12 neighbours and
 * two tetrahedra a bond of fcc fit). */
#define SMOLMC_MAX_CONN_GATES 4
#define SMOLMC_MAX_CONN_GATED_NEIGHBOURS 64
typedef struct smolmc_conn_gates {
    const uint64_t *gate_mask;    /* [G x 4], bit k: a gate site of kind k does not block */
    const int32_t *max_blocked;   /* [G], 0..SMOLMC_MAX_CONN_GATES */
    const int64_t *gate_ptr;      /* [nb + 1], nb = bond_ptr[G]: the gate sites of bond row b */
    const int32_t *gate_sites;    /* [gate_ptr[nb]], caller's site numbers */
} smolmc_conn_gates;
int smolmc_set_connectivity_gated(smolmc_handle *h, const smolmc_connectivity *s, const smolmc_conn_gates *g);
/* G and K in force (both 0: none set) */
int smolmc_connectivity_shape(smolmc_handle *h, int *n_graphs, int *n_kinds);
/* bit g of gated_graph_mask: graph g of the spec in force has a gate site; n_channels: the channel records the kernel
 * walks, summed over the neighbour-list entries of the gated graphs (both 0: an ungated spec, or none).  Either may be NULL. */
int smolmc_connectivity_gates(smolmc_handle *h, int *gated_graph_mask, int64_t *n_channels);
/* stats [nocc x G x 24] and labels [nocc x G x N] of nocc occupancies (host, int32 like smolmc_eval_full), or, with
 * occ == NULL, of the walkers' current states (nocc = R then).  Either output may be NULL. */
int smolmc_eval_connectivity(smolmc_handle *h, const int32_t *occ /* nocc x N, or NULL */, int nocc, int64_t *stats, int32_t *labels);
/* With SMOLMC_SAMPLE_CONNECTIVITY (128, flags bit 7) smolmc_run_sampled adds the column [rows x G x 24] (int64) to the
 * block, filled on the device from the block's occupancy rows when its launches are through; without
 * SMOLMC_SAMPLE_OCCUPANCY those rows never leave the device.  The ring carries no labels: smolmc_eval_connectivity gives
 * them.  The flag is refused while no spec is set.  This call reads the column of the block the next smolmc_get_samples*
 * call delivers ([nsamples x R x G x 24]) and does not mark it delivered, like smolmc_get_sample_structure; an error when
 * that block was recorded without the flag.  In a statistics record the column sources 2 + F + K + I + 24 g + c read
 * stats[g][c] as a double (with no spec set the range ends where it ends without). */
#define SMOLMC_SAMPLE_CONNECTIVITY 128
int smolmc_get_sample_connectivity(smolmc_handle *h, int64_t *stats);

/* ---- patterns: species patterns on site tuples of sampled states, counted on the device -----------------------------
 * (no reference counterpart).  A pattern spec rests on the observables in force: the kind of (site, code) is
 * kind_base[site] + code and there are K kinds.  The spec holds T sets.  Set t has an arity m_t, a class map
 * class_of_kind[t][K] with values in 0 .. C_t - 1 or -1, and the site tuples tuple_ptr[t] .. tuple_ptr[t + 1] of m_t sites
 * each.  Per occupancy row and set, for every tuple (i_0 .. i_{m-1}) as listed, with c_p = class_of_kind[t][kind(i_p)]:
 *   cells[cell_ptr[t] + sum_p c_p * C_t^(m - 1 - p)] += 1        (row-major, the first position most significant)
 * A tuple is skipped when one of its sites is not counted (kind_base < 0) or holds a kind whose class is -1.  Duplicate
 * tuples and tuples that name a site twice count as they stand.  cell_ptr[t] = sum_{u < t} C_u^m_u, n_cells = cell_ptr[T].
 * Everything is int32; smol_amd/patterns.py is the same in NumPy and the device matches it entry for entry.  The count
 * runs in the observables' kernel: a block that asks for counts, pairs and patterns stages its rows once.  Site numbers
 * are the caller's.  The engine copies and uploads everything. */
#define SMOLMC_MAX_PATTERN_SETS 8
#define SMOLMC_MAX_PATTERN_ARITY 8
#define SMOLMC_MAX_PATTERN_CLASSES 255 /* C_t: a class is staged as one byte, 0xff marks a site that is skipped */
#define SMOLMC_MAX_PATTERN_CELLS 4096  /* n_cells: 16 KB of int32 in LDS next to the row, its classes and the pair cells */
typedef struct smolmc_patterns {
    int n_sets;                   /* T, 1..SMOLMC_MAX_PATTERN_SETS */
    const int32_t *arity;         /* [T], each 1..SMOLMC_MAX_PATTERN_ARITY */
    const int32_t *n_classes;     /* [T], each 1..SMOLMC_MAX_PATTERN_CLASSES */
    const int32_t *class_of_kind; /* [T x K], K of the observables in force; -1 .. n_classes[t] - 1 */
    const int64_t *tuple_ptr;     /* [T + 1] tuples, ascending from 0 */
    const int32_t *sites;         /* the tuples of set 0, then of set 1 ...: sum_t n_t x arity[t] sites */
} smolmc_patterns;
/* Sets (NULL: removes) the pattern spec of the handle.  Refused, each naming its reason: no observables set; T, an arity
 * or a number of classes outside its range; a class outside -1 .. C_t - 1; a site out of range; more than
 * SMOLMC_MAX_PATTERN_CELLS cells; a launch that does not fit the LDS of one workgroup; while a block recorded with
 * SMOLMC_SAMPLE_PATTERNS waits in the ring; while a statistics record with pattern columns is set.  A refused call leaves
 * the handle's spec as it was.  While a spec is set smolmc_set_observables is refused: K and the kinds are what the class
 * maps index. */
int smolmc_set_patterns(smolmc_handle *h, const smolmc_patterns *spec);
/* T and n_cells in force (both 0: none set) */
int smolmc_patterns_shape(smolmc_handle *h, int *n_sets, int *n_cells);
/* cells [nocc x n_cells] of nocc occupancies (host, int32 like smolmc_eval_full), or, with occ == NULL, of the walkers'
 * current states (nocc = R then). */
int smolmc_eval_patterns(smolmc_handle *h, const int32_t *occ /* nocc x N, or NULL */, int nocc, int32_t *cells);
/* With SMOLMC_SAMPLE_PATTERNS (256, flags bit 8) smolmc_run_sampled adds the column [rows x n_cells] (int32) to the block,
 * filled on the device from the block's occupancy rows when its launches are through, by the launch that counts kinds and
 * pairs; without SMOLMC_SAMPLE_OCCUPANCY those rows never leave the device.  The flag is refused while no spec is set.
 * This call reads the column of the block the next smolmc_get_samples* call delivers ([nsamples x R x n_cells]) and does
 * not mark it delivered, like smolmc_get_sample_observables; an error when that block was recorded without the flag.  In
 * a statistics record the column sources 2 + F + K + I + 24 G + c read cell c as a double (with no spec set the range
 * ends where it ends without); smolmc_update_statistics counts the patterns of the current states first. */
#define SMOLMC_SAMPLE_PATTERNS 256
int smolmc_get_sample_patterns(smolmc_handle *h, int32_t *cells);

/* ---- environments: coordination environments of sampled states, counted on the device ---------------------------------
 * (no reference counterpart).  An environment spec rests on the observables in force: the kind of (site, code) is
 * kind_base[site] + code and there are K kinds.  The spec holds E sets.  Set e has a width z_e, A_e centre classes and B_e
 * neighbour classes, the maps centre_class_of_kind[e][K] (values -1 .. A_e - 1) and neigh_class_of_kind[e][K] (values
 * -1 .. B_e - 1), and the centres centre_ptr[e] .. centre_ptr[e + 1], each a site with a row of z_e neighbour sites; a slot
 * that holds -1 is empty.  Per occupancy row and set, for every centre as listed, with a = centre_class[kind(centre)]:
 *   n_b = #{slots of its row that are not empty, whose site is counted and whose neighbour class is b}
 *   code = a (z + 1)^B + sum_b n_b (z + 1)^(B - 1 - b)          (row-major, class 0 most significant)
 *   cells[cell_ptr[e] + code] += 1
 * A centre is skipped when it is not counted (kind_base < 0) or a == -1.  A slot whose site is not counted or has class -1
 * adds to no n_b; it does not skip the centre.  Duplicate centres, slots that repeat a site and slots that name the centre
 * count as they stand.  cell_ptr[e] = sum_{u < e} A_u (z_u + 1)^B_u, n_cells = cell_ptr[E]: the plain product, not the
 * simplex.  Everything is int32; smol_amd/environments.py is the same in NumPy and the device matches it entry for entry.
 * The count runs in the observables' kernel, behind the patterns.  Site numbers are the caller's.  The engine copies and
 * uploads everything. */
#define SMOLMC_MAX_ENV_SETS 8
#define SMOLMC_MAX_ENV_WIDTH 64          /* z: a count of neighbours is an 8-bit field of one register */
#define SMOLMC_MAX_ENV_CENTRE_CLASSES 15 /* A: the classes of a site are staged as two nibbles of one byte, 0xf: none */
#define SMOLMC_MAX_ENV_NEIGH_CLASSES 4   /* B */
#define SMOLMC_MAX_ENV_CELLS 4096        /* n_cells: 16 KB of int32 in LDS */
typedef struct smolmc_environments {
    int n_sets;                          /* E, 1..SMOLMC_MAX_ENV_SETS */
    const int32_t *width;                /* [E], each 1..SMOLMC_MAX_ENV_WIDTH */
    const int32_t *n_centre_classes;     /* [E], each 1..SMOLMC_MAX_ENV_CENTRE_CLASSES */
    const int32_t *n_neigh_classes;      /* [E], each 1..SMOLMC_MAX_ENV_NEIGH_CLASSES */
    const int32_t *centre_class_of_kind; /* [E x K], K of the observables in force; -1 .. n_centre_classes[e] - 1 */
    const int32_t *neigh_class_of_kind;  /* [E x K]; -1 .. n_neigh_classes[e] - 1 */
    const int64_t *centre_ptr;           /* [E + 1] centres, ascending from 0 */
    const int32_t *centres;              /* [centre_ptr[E]] sites */
    const int32_t *neighbours;           /* the rows of set 0, then of set 1 ...: sum_e n_e x width[e] sites, -1: empty */
} smolmc_environments;
/* Sets (NULL: removes) the environment spec of the handle.  Refused, each naming its reason: no observables set; E, a
 * width or a number of classes outside its range; a class outside its range; a centre or a non-empty slot out of range;
 * more than SMOLMC_MAX_ENV_CELLS cells; a launch (row, observables, patterns and environments together) that does not fit
 * the 64 KB of LDS a workgroup takes; while a block recorded with SMOLMC_SAMPLE_ENVIRONMENTS waits in the ring; while a
 * statistics record with environment columns is set.  A refused call leaves the handle's spec as it was.  While a spec is
 * set smolmc_set_observables is refused, and smolmc_set_patterns checks the LDS of the launch with both. */
int smolmc_set_environments(smolmc_handle *h, const smolmc_environments *spec);
/* E, n_cells and the centres of all sets in force (all 0: none set) */
int smolmc_environments_shape(smolmc_handle *h, int *n_sets, int *n_cells, int *n_centres);
/* cells [nocc x n_cells] and codes [nocc x n_centres] (the set-local code of every centre, set after set, or -1 for a
 * skipped centre) of nocc occupancies (host, int32 like smolmc_eval_full), or, with occ == NULL, of the walkers' current
 * states (nocc = R then).  Either output may be NULL. */
int smolmc_eval_environments(smolmc_handle *h, const int32_t *occ /* nocc x N, or NULL */, int nocc, int32_t *cells,
                             int32_t *codes);
/* With SMOLMC_SAMPLE_ENVIRONMENTS (512, flags bit 9) smolmc_run_sampled adds the column [rows x n_cells] (int32) to the
 * block, filled on the device by the launch that counts kinds, pairs and patterns; without SMOLMC_SAMPLE_OCCUPANCY the rows
 * never leave the device.  The flag is refused while no spec is set.  This call reads the column of the block the next
 * smolmc_get_samples* call delivers ([nsamples x R x n_cells]) and does not mark it delivered, like
 * smolmc_get_sample_patterns; an error when that block was recorded without the flag.  In a statistics record the column
 * sources 2 + F + K + I + 24 G + P + c (P the pattern cells in force) read cell c as a double (with no spec set the range
 * ends where it ends without); smolmc_update_statistics counts the environments of the current states first. */
#define SMOLMC_SAMPLE_ENVIRONMENTS 512
int smolmc_get_sample_environments(smolmc_handle *h, int32_t *cells);

/* Same loop driven by host-provided proposals ("replay mode"): what
 * StandardSingleStepMixin.single_step (kernel/base.py:145-166) does after mcusher.propose_step
 * returned, with the numbers the reference's Generator produced.
 *   steps       [R x nsteps x SMOLMC_STEP_ROW] step records (see SMOLMC_STEP_ROW); every site must be
 *               a changeable site of an active sublattice and every code one of its species.
 *   uniforms    [R x nsteps] the number rng.random() returned in _accept_step (NaN if not drawn:
 *               the reference accepted without drawing, metropolis.py:46-48).
 *   log_priori  [R x nsteps] or NULL: mcusher.compute_log_priori_factor(occupancy, step) added to the
 *               exponent (metropolis.py:41-42, wanglandau.py:197-198).  NULL or a NaN entry: the
 *               engine's own value -- 0 for Flip / Swap handles (mcusher.py:118-134); for TableFlip
 *               handles TableFlip.compute_log_priori_factor (mcusher.py:656-711) evaluated on the
 *               device from the step and the walker's species counts; a step that is neither a
 *               canonical swap nor +-(a row of flip_table) fails like the reference's
 *               ValueError("Step ... is not in flip table.", :673-674).
 * Outputs (each may be NULL): accepted_out [R x nsteps]; enthalpy_out [R x nsteps] the walker's
 * enthalpy AFTER the step; log_priori_out [R x nsteps] the a-priori factor that entered the
 * exponent.  Bias terms (MCBias) and Wang-Landau state take part exactly as in smolmc_run. */
int smolmc_replay(smolmc_handle *h, int64_t nsteps, const int32_t *steps, const double *uniforms,
                  const double *log_priori, uint8_t *accepted_out, double *enthalpy_out,
                  double *log_priori_out);
/* elapsed device time of the last smolmc_run / smolmc_replay launch in ms
 * (HIP events recorded on the launch stream) */
int smolmc_last_kernel_ms(smolmc_handle *h, float *ms);

/* ---- evaluator-level entry points (parity + Processor shim) ------------- */
/* Ensemble.compute_feature_vector (ensemble.py:323-351) for nocc occupancies:
 * correlations_from_occupancy / interactions_from_occupancy x size
 * (evaluator.pyx:121-209; expansion.py:165-189,391-414), Ewald feature
 * (processor/ewald.py:128-145), chemical work.  features [nocc x F]. */
int smolmc_eval_full(smolmc_handle *h, const int32_t *occ /*nocc x N*/, int nocc,
                     double *features);
/* Ensemble.compute_feature_vector_change (ensemble.py:353-376) for nstep steps of
 * up to SMOLMC_MAX_STEP_FLIPS sequential flips each on ONE occupancy:
 * delta_correlations_from_occupancies / delta_interactions_from_occupancies
 * (evaluator.pyx:211-317) x size with sequential-flip semantics
 * (expansion.py:217-229), delta_ewald_single_flip (ewald.pyx:9-59), mu table.
 * flips [nstep x SMOLMC_STEP_ROW] step records like smolmc_replay; dfeatures [nstep x F]. */
int smolmc_eval_delta(smolmc_handle *h, const int32_t *occ /*N*/, const int32_t *flips,
                      int nstep, double *dfeatures);

/* ---- device plumbing (multi-GPU / RCCL glue, optional) ------------------- */
/* Use an externally created hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int smolmc_set_stream(smolmc_handle *h, void *hip_stream);
/* Copy per-walker enthalpies (float64[R]) into a DEVICE buffer (for all_gather) */
int smolmc_export_enthalpy_dev(smolmc_handle *h, double *dst_dev);
/* Permute per-walker temperatures from a DEVICE or host array after an exchange */
int smolmc_import_temperature_dev(smolmc_handle *h, const double *src_dev);
/* One exchange attempt of a replica-exchange temperature ladder decided on the device (ABI 8; no reference
 * counterpart: SURVEY 8e, BASELINE configs[4]).  n_total walkers over all ranks, this handle holds walkers
 * first .. first + R - 1 of them.  All arrays are DEVICE arrays of this handle's GPU:
 *   enthalpy_all_dev [n_total]   the all-gathered enthalpies, global walker order
 *   ladder_dev       [n_total]   temperature of every rung
 *   log_u_dev        [>= n_total / 2]  log of the acceptance uniform of the p-th pair of this attempt (the caller's
 *                                counter-based stream: identical on every rank)
 *   rung_of_dev      [n_total]   in / out: walker -> rung
 *   stats_dev        [2 (n_total - 1)] in / out, may be NULL: attempts | acceptances per neighbouring pair of rungs
 * parity 0 / 1: pairs (0,1),(2,3),... / (1,2),(3,4),...  Accepts with min(1, exp((beta_k - beta_k+1)(H_a - H_b))),
 * moves the rung assignment and sets THIS handle's temperatures to ladder[rung_of[first + r]]; asynchronous on the
 * handle's stream (the inputs must be complete when it is called).  Every rank that calls it with the same inputs
 * takes the same decisions; only temperatures move, occupancies never leave their GPU. */
int smolmc_exchange_dev(smolmc_handle *h, int n_total, int first, int parity, const double *enthalpy_all_dev,
                        const double *ladder_dev, const double *log_u_dev, int32_t *rung_of_dev, int64_t *stats_dev);

/* ---- distance objective: special quasirandom structures ------------------ */
/* The objective of smol's DistanceProcessor (smol/moca/processor/distance.py:20-182),
 *     H = -w L + sum_k W_k |f_k - t_k|,
 * f the INTENSIVE correlation vector (feature_mode SMOLMC_FEATURES_CORRELATIONS, CorrelationDistanceProcessor)
 * or cluster-interaction vector (SMOLMC_FEATURES_INTERACTIONS with tables->interaction_tensors,
 * ClusterInteractionDistanceProcessor, distance.py:392-412), t the target, L the largest diameter up to which
 * every feature matches the target within match_tol (distance.py:307-332).
 *
 * A distance handle works with smolmc_set_state, get_state, set_temperature, set_counters, run, replay,
 * run_sampled (SMOLMC_SAMPLE_OCCUPANCY), eval_full, eval_delta, natural_parameters and kernel_info.  Unlike the
 * extensive convention above, the features it hands back are the reference's intensive DISTANCE vector
 * [L or 0, |f_1 - t_1|, ..., |f_{F-1} - t_{F-1}|] (distance.py:133-182); eval_delta returns the difference of
 * two such vectors (distance.py:156-182), and the enthalpy is H.  tables->ce_coefs is ignored. */
#define SMOLMC_DIST_MAX_FEATURES 256 /* largest F of a distance handle */
typedef struct smolmc_distance {
    int32_t n_features;            /* F = num_corr (correlations) or num_orbits (interactions), incl. entry 0 */
    const double *target;          /* [F] target_vector; entry 0 unused (distance.py:133-154) */
    const double *weights;         /* [F-1] target_weights */
    double match_weight;           /* w >= 0; natural parameters are [-w, weights...] (distance.py:95) */
    double match_tol;              /* exact-match tolerance, `<=` (distance.py:307-332) */
    int32_t n_groups;              /* distinct diameters rounded to 6 decimals, ascending */
    const double *group_diameter;  /* [n_groups] (clusterspace.py:368-381 orbits_by_diameter) */
    const int32_t *feature_group;  /* [F] group of every feature, -1 for entry 0 */
    double kB;                     /* Boltzmann constant of this handle's temperatures (sqs.py:522-524 uses 1.0) */
} smolmc_distance;

/* Refused: Ewald tables (distance.py:76-77), mu_table, bias terms, Wang-Landau, TableFlip, match_weight < 0,
 * F above SMOLMC_DIST_MAX_FEATURES, and models whose kernel state does not fit 64 KB of LDS per workgroup of four
 * walkers: the feature mode's tensors (8 bytes per entry, shared) plus, per walker, 16 F + 8 x (row chunks of the
 * busiest site: ceil(J / 4) per local record and function) + 2 x num_sites bytes.  smolmc_import_temperature_dev
 * and smolmc_exchange_dev refuse a distance handle.  Metropolis with beta = 1 / (kB T) (metropolis.py:31-49). */
int smolmc_create_distance(const smolmc_tables *t, const smolmc_distance *d,
                           const smolmc_config *c, smolmc_handle **out);
/* per walker: lowest running enthalpy seen (strictly lower replaces), its distance features,
 * its occupancy, the step at which it was reached (the walker's n_steps then); any pointer may be NULL.
 * smolmc_set_state starts the record at the initial state. */
int smolmc_get_best(smolmc_handle *h, double *score /*R*/, double *features /*RxF*/,
                    int32_t *occ /*RxN*/, uint64_t *step /*R*/);
/* forget the record: it restarts at every walker's current state */
int smolmc_reset_best(smolmc_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* SMOLMC_H */
