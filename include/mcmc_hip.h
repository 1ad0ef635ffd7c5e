/*
 * mcmc_hip.h -- C ABI of libmcmc_hip.so, the MI355X (gfx950) walker-ensemble Metropolis
 * engine behind Cobaya's sampler plugin surface.
 *
 * The reference (CobayaSampler/cobaya v3.6.2) is pure Python and has no FFI on this path;
 * each entry point below names the reference interface it stands in for (paths relative to
 * the reference checkout).  The Python class cobaya_amd.sampler.MCMCHip (registered as
 * sampler `mcmc_hip`) is the only caller: initialize() -> create/set_*, run() -> loop of
 * step/accumulate_moments/read_moments/gelman_rubin/set_proposal_cov/drain_samples,
 * products() -> get_state/drain_samples.  See INTEGRATION.md for the ctypes binding.
 *
 * Conventions: opaque handle; all buffers are caller-owned C-contiguous host arrays
 * (the library copies in/out and never retains a pointer); every function returns 0 on
 * success and a negative code on error, with a message available from
 * mcmc_hip_last_error(); nothing throws across the boundary; a handle is not thread-safe;
 * all calls may be made with the GIL released.  There is NO CPU fallback: create() fails
 * if no gfx950 device is usable.
 */
#ifndef MCMC_HIP_H
#define MCMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcmc_hip_ctx mcmc_hip_ctx;

/* The library is built with -fvisibility=hidden: exactly the functions declared in this header
 * are exported (tests/test_host_logic.py compares `nm -D` with it). */
#define MCMC_HIP_API __attribute__((visibility("default")))

enum {
    MCMC_HIP_OK = 0,
    MCMC_HIP_ERR_ARG = -1,       /* invalid argument / unsupported configuration */
    MCMC_HIP_ERR_DEVICE = -2,    /* HIP runtime error or no usable gfx950 device */
    MCMC_HIP_ERR_NOT_PD = -3,    /* matrix not symmetric positive definite */
    MCMC_HIP_ERR_STATE = -4,     /* call order violated (e.g. step before set_state) */
    MCMC_HIP_ERR_STUCK = -5,     /* a walker exceeded max_tries (mcmc.py:717-743) */
    MCMC_HIP_ERR_TARGET = -6,    /* a function target returned NaN or +inf inside the prior support */
    MCMC_HIP_ERR_CALLBACK = -7   /* the callback of a function target returned non-zero */
};

/* Options fixed at creation.  Mirrors the attributes cobaya/samplers/mcmc/mcmc.py:111-271
 * (MCMC.initialize) reads from mcmc.yaml, plus the ensemble geometry. */
typedef struct mcmc_hip_config {
    int32_t d;               /* number of sampled parameters, 1..256 (mcmc_hip_max_dim) */
    int32_t n_walkers;       /* walkers on this device; multiple of group_size */
    int32_t group_size;      /* walkers sharing one Haar basis: 64, 128 or 256 */
    int32_t device;          /* HIP device ordinal */
    uint64_t seed;           /* mcmc.yaml:75 `seed` (Philox key; sampler.py:369-384) */
    uint32_t walker_offset;  /* global id of this device's first walker (multi-GPU shard) */
    int32_t burn_in;         /* accepted steps discarded per walker (mcmc.py:265, 691-707) */
    double temperature;      /* mcmc.yaml:24 (mcmc.py:127-130, 438-440, 682) */
    double proposal_scale;   /* mcmc.yaml:17 (proposal.py:223) */
    double max_tries;        /* mcmc.yaml:9, already multiplied by d (mcmc.py:717-743) */
    int32_t emit_capacity;   /* accepted rows kept per walker between drains; 0 = none */
    int32_t flags;           /* MCMC_HIP_FLAG_* (0: the default ensemble) */
} mcmc_hip_config;

/* every walker draws its OWN Haar basis per cycle (proposal.py:59-69 to the letter) instead
 * of sharing the group's: the reference-faithful control, much slower */
#define MCMC_HIP_FLAG_OWN_BASIS 1
/* incremental evaluation (Gaussian mixtures of up to 64 modes with uniform / normal priors and
 * any number of periodic parameters, parameter blocks of any size and oversampling, Metropolis
 * steps -- mcmc_hip_incremental_supported says whether a shape fits; dragging for one mode with
 * non-periodic priors; 2 <= d <= 128; emitted rows, emit_capacity > 0, with Metropolis steps):
 * every walker carries y_k = L_k^-1 (x - mu_k) and a trial moves it along the whitened shared
 * direction, y_k' = y_k + r L_k^-1 v -- the same log-posterior (gaussian_mixture.py:158-163) in
 * O(d) per step and mode; y is recomputed from x every 40 cycle lengths (40 d steps for one
 * block).  With ONE mode and no periodic parameter the log-likelihood is carried as well:
 * loglike' = loglike - r/2 (2 y.u + r |u|^2), u = L^-1 v, re-anchored on y wherever y is
 * recomputed.  What the mode does not serve is refused by mcmc_hip_step with MCMC_HIP_ERR_ARG.
 * Specified in oracle/mcmc_oracle.c. */
#define MCMC_HIP_FLAG_INCREMENTAL 2
/* incremental mode: the walkers that share one Haar basis = group_size << ((flags >> 8) & 15)
 * (the R-1 groups of the moments stay group_size wide): fewer bases and whitened columns per
 * launch */
#define MCMC_HIP_FLAG_BASIS_GROUP_MASK 0x0F00

MCMC_HIP_API const char* mcmc_hip_version(void);
/* message of the last error on this handle (or of the last failed create if h == NULL) */
MCMC_HIP_API const char* mcmc_hip_last_error(const mcmc_hip_ctx* h);
/* 1 if the lane-per-walker kernels for dimension d were compiled into this library */
MCMC_HIP_API int mcmc_hip_dim_supported(int d);
/* the largest number of sampled parameters any configuration serves (256): d <= 128 on every path,
 * 128 < d <= 256 with incremental evaluation of one parameter block (Metropolis steps, the `one` likelihood or 1..4
 * Gaussian modes, no periodic parameter, no emitted rows; huge_kernels.hip) */
MCMC_HIP_API int32_t mcmc_hip_max_dim(void);
/* 1 if MCMC_HIP_FLAG_INCREMENTAL serves a Gaussian mixture of n_modes (>= 1) modes in d dimensions
 * of which n_periodic are periodic (prior.py:658-676), with n_drag interpolation steps per dragging
 * step (0: Metropolis steps), for n_walkers walkers of which basis_group_size share a proposal
 * direction: the tuned kernels (one mode; up to four at d <= 64, five and six at d <= 32 / 28; up to 16 periodic parameters
 * of one mode; dragging of one non-periodic mode) or the general one (anything else without
 * dragging whose per-walker state -- n_modes * d doubles -- fits the LDS of a CU).  0: such a model
 * is sampled from scratch (no flag).  A pure function: no device is touched. */
MCMC_HIP_API int mcmc_hip_incremental_supported(int32_t d, int32_t n_modes, int32_t n_periodic, int32_t n_drag,
                                   int32_t n_walkers, int32_t basis_group_size);

/* The rule behind mcmc_hip_incremental_supported in full: which incremental step kernel serves a
 * shape and what that kernel carries.  A pure function as well (no device), so the rule is tested
 * where there is no GPU.  Flags are 0 / 1. */
typedef struct mcmc_hip_inc_shape {
    int32_t d, n_modes, n_periodic;
    int32_t n_drag;             /* interpolation steps per dragging step; 0: Metropolis steps */
    int32_t n_walkers, basis_group_size;
    int32_t any_normal;         /* some prior is normal */
    int32_t one_box;            /* every parameter uniform on the same interval */
    int32_t box_lo_is_zero;     /* ... which begins at 0 */
    int32_t has_1d_block;       /* a parameter block of one parameter */
    int32_t emit;               /* emit_capacity > 0 */
    int32_t duo;                /* two lanes per walker: -1 where it pays, 0 never, 1 wherever it serves */
} mcmc_hip_inc_shape;
#define MCMC_HIP_INC_NOT_SERVED 0
#define MCMC_HIP_INC_STEP 1       /* one mode, four lanes per walker */
#define MCMC_HIP_INC_STEP_EMIT 2  /* ... with emitted rows */
#define MCMC_HIP_INC_MIX 3        /* mixture with carried mode log-densities, four lanes */
#define MCMC_HIP_INC_ANY 4        /* the general kernels */
#define MCMC_HIP_INC_DRAG 5       /* dragging */
#define MCMC_HIP_INC_DUO_MIX 6    /* mixture, two lanes per walker */
#define MCMC_HIP_INC_DUO_ONE 7    /* one mode, two lanes per walker */
typedef struct mcmc_hip_inc_choice {
    int32_t family;             /* MCMC_HIP_INC_* */
    int32_t reason;             /* not served: 1 shape out of range, 2 dragging with a mixture / a periodic
                                 * parameter / too many columns, 3 the general kernel's state does not fit,
                                 * 4 emitted rows with dragging; served: 0 */
    int32_t dq_lo;              /* first dq = ceil(d / 4) of the launcher's translation unit; 0: one launcher */
    int32_t carry, carry_modes, carry_prior, carry_periodic, fold;
    int32_t chunk_steps;        /* dragging steps per LDS chunk */
    int32_t colb;               /* doubles per direction column */
    int32_t thins_on_device;    /* mcmc_hip_set_emit_thin is served */
    int32_t box;                /* the step kernel takes the one-interval path of the prior */
} mcmc_hip_inc_choice;
MCMC_HIP_API int mcmc_hip_incremental_choice(const mcmc_hip_inc_shape* shape, mcmc_hip_inc_choice* out);

/* The same for the kernels that evaluate every trial from scratch (no MCMC_HIP_FLAG_INCREMENTAL): which
 * kernel mcmc_hip_step launches for a shape and with what geometry (csrc/scratch_choice.h).  A pure
 * function (no context, no device); what this library was built with is read from its own tables. */
typedef struct mcmc_hip_scratch_shape {
    int32_t d, n_modes;         /* n_modes 0: the `one` likelihood */
    int32_t n_walkers, group_size;
    int32_t any_normal, any_periodic;
    int32_t emit;               /* emit_capacity > 0 */
    int32_t emit_thin;          /* mcmc_hip_set_emit_thin > 1 */
    int32_t unit_t;             /* temperature == 1 */
    int32_t own_basis;          /* MCMC_HIP_FLAG_OWN_BASIS */
    int32_t blocked;            /* parameter blocks */
    int32_t n_drag;             /* interpolation steps per dragging step; 0: Metropolis steps */
    int32_t cps, cps_f;         /* direction columns per cycle (0: d); of the fast blocks (dragging) */
    int32_t has_1d_column;      /* the launch's columns include one of a one-parameter block */
} mcmc_hip_scratch_shape;
#define MCMC_HIP_SCRATCH_NOT_SERVED 0
#define MCMC_HIP_SCRATCH_STEP 1          /* step_kernel<MULTI, GENERAL> */
#define MCMC_HIP_SCRATCH_STEP_OWN 2      /* step_kernel<MULTI, true, own basis> */
#define MCMC_HIP_SCRATCH_PAIR 3          /* step_pair_kernel<UNIT_T, NORMP> */
#define MCMC_HIP_SCRATCH_MFMA 4          /* step_mfma_kernel<NORMP> */
#define MCMC_HIP_SCRATCH_BIG_REG 5       /* step_big_reg_kernel */
#define MCMC_HIP_SCRATCH_GENERAL 6       /* step_general_kernel */
#define MCMC_HIP_SCRATCH_DRAG 7          /* drag_kernel<MULTI> */
#define MCMC_HIP_SCRATCH_GENERAL_DRAG 8  /* drag_general_kernel */
typedef struct mcmc_hip_scratch_answer {
    int32_t family;             /* MCMC_HIP_SCRATCH_* */
    int32_t reason;             /* not served: 1 a shape mcmc_hip_create refuses, 2 emit_thin, 3 own bases with blocks
                                 * or dragging, 4 the general d > 32 kernels' LDS, 5 a cycle's directions against
                                 * the LDS, 6 / 7 no column sweep at this size / with normal priors; served: 0 */
    int32_t multi, general, unit_t, normp;   /* the template arguments of the instantiation */
    int32_t unit;               /* the compiled MCMC_D or MCMC_DP of its translation unit; 0: one symbol */
    int32_t walkers_per_wg, threads, grid;
    int32_t lds_bytes;          /* dynamic LDS of the launch, placement request included */
    int32_t lds_attr;           /* hipFuncAttributeMaxDynamicSharedMemorySize set before it; 0: not set */
    int32_t v_ld;               /* doubles between two direction columns */
    int32_t slab, slab_f;       /* doubles per (group, cycle) slab of directions; of the fast blocks' */
} mcmc_hip_scratch_answer;
MCMC_HIP_API int mcmc_hip_scratch_choice(const mcmc_hip_scratch_shape* shape, mcmc_hip_scratch_answer* out);

/* Sampler.__init__ + MCMC.initialize (cobaya/sampler.py:257-322, mcmc.py:111-271) */
MCMC_HIP_API int mcmc_hip_create(const mcmc_hip_config* cfg, mcmc_hip_ctx** out);
MCMC_HIP_API void mcmc_hip_destroy(mcmc_hip_ctx* h);

/* Prior.__init__ constants (cobaya/prior.py:464-533): kind[i] 0 = uniform on [a,b],
 * 1 = normal(loc=a, scale=b); periodic[i] != 0 wraps into [a,b) (prior.py:658-676). */
MCMC_HIP_API int mcmc_hip_set_prior(mcmc_hip_ctx* h, const int32_t* kind, const double* a, const double* b,
                       const int32_t* periodic);

/* GaussianMixture.initialize_with_params (gaussian_mixture.py:45-136): means[K*d],
 * covs[K*d*d] row-major, weights[K] (NULL = equal; renormalised if they do not sum to 1). */
MCMC_HIP_API int mcmc_hip_set_target_gaussian_mixture(mcmc_hip_ctx* h, int32_t n_modes, const double* means,
                                         const double* covs, const double* weights);
/* Gaussian.initialize_with_params (gaussian/gaussian.py:30-94) */
MCMC_HIP_API int mcmc_hip_set_target_gaussian(mcmc_hip_ctx* h, const double* mean, const double* cov,
                                 int32_t normalized);
/* likelihoods/one/one.py:27-29: loglike = 0 (prior-only sampling) */
MCMC_HIP_API int mcmc_hip_set_target_one(mcmc_hip_ctx* h);

/* Target kind `function` (the batched counterpart of LikelihoodExternalFunction,
 * cobaya/likelihood.py:150-255): the log-likelihood of a point is whatever `fn` computes for it.
 *   points   device memory, [n][d] row-major (point-major, as mcmc_hip_evaluate's x)
 *   loglike  device memory, [n]: fn leaves the log-likelihood of point k in loglike[k]
 *   stream   the engine's hipStream_t (mcmc_hip_stream_handle)
 * fn must only QUEUE work -- kernels, copies -- on `stream`, or on streams it orders against
 * `stream` with events on both sides; it must not synchronise the device and returns 0 on success.
 * It is called once per Metropolis step with the trial points of ALL n_walkers walkers, the rows
 * outside the prior support included: what it returns for those is ignored (NaN is allowed there;
 * the reference skips the likelihood outside the support, model.py:650-653 -- a batched call
 * cannot).  Inside the support -inf is an ordinary rejection; NaN or +inf is an error of the
 * target: the id of the first such walker is kept and the next mcmc_hip_sync or
 * mcmc_hip_fetch_moments returns MCMC_HIP_ERR_TARGET (mcmc_hip_evaluate returns it at once).
 * If fn returns non-zero, mcmc_hip_step / mcmc_hip_evaluate return MCMC_HIP_ERR_CALLBACK: the
 * pending trial is dropped, state and step counter stay as of the last completed step, and the
 * context stays usable.
 * Per step ("Function targets"): variates of the un-paired stream, trial
 * t = fma(r, v, x) along the group's shared direction, support test and log-prior as under
 * mcmc_hip_set_target_one, loglike = fn(t), the Metropolis rule and bookkeeping of every other
 * target; one launch accepts step s and proposes step s + 1 (function_kernels.hip).
 * Served: 1 <= d <= 128, evaluation from scratch, the shared basis, one parameter block, Metropolis
 * steps, non-periodic priors, emit_capacity 0.  Refused with MCMC_HIP_ERR_ARG here or by
 * mcmc_hip_step: MCMC_HIP_FLAG_INCREMENTAL, MCMC_HIP_FLAG_OWN_BASIS, parameter blocks /
 * oversampling / dragging (mcmc_hip_set_blocking), periodic parameters, emit_capacity > 0, d > 128.
 * Moments, checkpoints, the bounds ring, get / set_full_state, walker_offset, temperature, burn-in
 * and timing work as for every target. */
typedef int (*mcmc_hip_loglike_fn)(void* user, int32_t n, int32_t d, const double* points,
                                   double* loglike, void* stream);
MCMC_HIP_API int mcmc_hip_set_target_function(mcmc_hip_ctx* h, mcmc_hip_loglike_fn fn, void* user);
/* Target kind `function` with SEVERAL functions over parameter blocks ("Function
 * targets with parameter blocks"): the log-likelihood is the sum of n = 1..8 batched device functions.
 * Function c reads n_inputs[c] of the sampled parameters -- their sampler indices are the next
 * n_inputs[c] entries of `inputs`, function after function; the subsets may overlap, every sampled
 * parameter must feed at least one -- as a point-major (n_points, n_inputs[c]) tensor in that order:
 * the `d` argument of its callback is n_inputs[c].  Unlike mcmc_hip_set_target_function this target
 * accepts parameter blocks and oversampling (mcmc_hip_set_blocking, before or after; no dragging).
 * The slot schedule of a cycle is then shared by the whole ensemble (the shuffle of global group 0),
 * and at a slot of sorted block b only the functions with an input in a block >= b are called, once,
 * with the trials of all walkers; the others keep the value carried per walker.  mcmc_hip_set_state
 * and mcmc_hip_evaluate call every function.  Otherwise the limits of mcmc_hip_set_target_function. */
MCMC_HIP_API int mcmc_hip_set_target_functions(mcmc_hip_ctx* h, int32_t n, const mcmc_hip_loglike_fn* fns,
                                               void* const* users, const int32_t* n_inputs,
                                               const int32_t* inputs);
/* The carried per-function log-likelihoods of the state, ll[n * n_walkers] (function c of walker w at
 * c * n_walkers + w): part of the full state of such a target.  mcmc_hip_set_full_state without a
 * following mcmc_hip_set_component_loglikes has every function called on the state at the next
 * mcmc_hip_step.  MCMC_HIP_ERR_STATE unless mcmc_hip_set_target_functions is in force. */
MCMC_HIP_API int mcmc_hip_get_component_loglikes(mcmc_hip_ctx* h, double* ll);
MCMC_HIP_API int mcmc_hip_set_component_loglikes(mcmc_hip_ctx* h, const double* ll);

/* PlanckPlikLite.init_params (cobaya/likelihoods/base_classes/planck_pliklite.py:32-141) for the
 * used bins, + the Cl provider of `logp` (planck_pliklite.py:170-178) as a LINEAR emulator:
 *   bins[n_bins*3] = (spectrum 0 tt / 1 te / 2 ee, first l, last l) of every used bin in
 *   data-vector order (`used_indices`); weights[lmax+1] in D_l space (planck_pliklite.py:52-56);
 *   X[n_bins] = X_data; cov[n_bins*n_bins] row-major (the reference inverts it, :141; here
 *   chi2 = |L^-1 delta|^2 with cov = L L^T, the same quadratic form);
 *   D_l(theta) = D0[tp*(lmax+1)+l] + sum_p J[(tp*(lmax+1)+l)*n_lin+p] (theta_p - theta0_p), theta =
 *   the sampled parameters without the calibration parameter (`calibration_param`, A_planck) at
 *   position calib_index, in order; n_lin = d - 1.
 * loglike = -chi2/2, chi2 = get_chi_squared(0, D_tt, D_te, D_ee, A) (planck_pliklite.py:143-155).
 * Binning commutes with the linear emulator: the library bins D0 and J once and evaluates
 * cl_b(theta) from that binned response (specification: oracle/mcmc_oracle.c, orc_binned).
 * n_bins <= 640, 2 <= d <= 32, evaluation from scratch (no MCMC_HIP_FLAG_INCREMENTAL: the
 * posterior is not Gaussian in the calibration parameter), shared basis, emit_capacity 0. */
MCMC_HIP_API int mcmc_hip_set_target_binned_gaussian(mcmc_hip_ctx* h, int32_t n_bins, const int32_t* bins,
                                        int32_t lmax, const double* weights, const double* X,
                                        const double* cov, int32_t n_lin, const double* theta0,
                                        const double* D0, const double* J, int32_t calib_index);
/* PlanckPlikLite.get_chi_squared(L0, ctt, cte, cee, A_planck) (planck_pliklite.py:143-155) for
 * n_pts sets of EXPLICIT spectra: cl[n_pts*3*n_ell], element l - L0 of row (pt, spectrum) is
 * D_l; A[n_pts]; chi2[n_pts] out.  Binning on the device as the banded product it is, then the
 * same matrix-core kernel as the sampler's steps. */
MCMC_HIP_API int mcmc_hip_evaluate_binned(mcmc_hip_ctx* h, int32_t n_pts, int32_t L0, int32_t n_ell,
                             const double* cl, const double* A, double* chi2);
/* Constants derived by set_target_binned_gaussian: Linv[n_bins*n_bins] (functions.py:81-89 of
 * cov), the binned response Bc0[n_bins], BJ[n_bins*n_lin]; any pointer may be NULL.  Lets tests
 * hand the CPU oracle exactly the problem the kernels evaluate. */
MCMC_HIP_API int mcmc_hip_get_binned_constants(const mcmc_hip_ctx* h, double* Linv, double* Bc0, double* BJ);

/* BlockedProposer.__init__ (proposal.py:96-196) + MCMC.set_proposer_blocking (mcmc.py:320-410):
 * n_blocks parameter blocks sorted slow -> fast, block b holding block_size[b] consecutive
 * entries of i_of_j[d] (sampler indices in sorted order) and visited oversampling[b] *
 * block_size[b] times per cycle.  drag_last_slow >= 0 switches mcmc_hip_step to the dragging
 * step (mcmc.py:564-668) with blocks 0..drag_last_slow slow and drag_steps interpolation
 * steps; -1 keeps Metropolis steps.  From scratch: the tuned kernels for d <= 32, the general
 * ones (step_general_kernel, drag_general_kernel) for 32 < d <= 128; with emit_capacity > 0 a
 * dragging step emits the point it leaves (mcmc.py:656-668) from the from-scratch kernels.  Must
 * precede set_proposal_cov (a previous covariance is forgotten).  One block with factor 1 and the identity order is the default. */
MCMC_HIP_API int mcmc_hip_set_blocking(mcmc_hip_ctx* h, int32_t n_blocks, const int32_t* block_size,
                          const int32_t* oversampling, const int32_t* i_of_j,
                          int32_t drag_last_slow, int32_t drag_steps);
/* steps per cycle: d for one block, sum_b oversampling_b n_b with blocks, the number of slow
 * parameters when dragging (mcmc.py:400-407) */
MCMC_HIP_API int mcmc_hip_cycle_length(const mcmc_hip_ctx* h);

/* BlockedProposer.set_covariance (proposal.py:226-260); with blocks the covariance is
 * reordered by i_of_j first and get_proposal_transform returns T in that sorted order:
 * checks symmetric positive definite, builds T = scale * diag(std) * chol(corr).  `cov`
 * must already carry the temperature factor (mcmc.py:438-440), as in the reference. */
MCMC_HIP_API int mcmc_hip_set_proposal_cov(mcmc_hip_ctx* h, const double* cov);
MCMC_HIP_API int mcmc_hip_get_proposal_cov(const mcmc_hip_ctx* h, double* cov);          /* proposal.py:262 */
MCMC_HIP_API int mcmc_hip_get_proposal_transform(const mcmc_hip_ctx* h, double* T);      /* transform[0] * scale */

/* Model.logposterior for a batch (cobaya/model.py:579-678): x[n*d] point-major ->
 * logprior[n], loglike[n] (-inf outside the prior support), derived[n*K*d] or NULL =
 * L_k^-1 (x - mu_k) (gaussian_mixture.py:146-156). */
MCMC_HIP_API int mcmc_hip_evaluate(mcmc_hip_ctx* h, int32_t n, const double* x, double* logprior,
                      double* loglike, double* derived);

/* OneSamplePoint.add of the initial points (mcmc.py:219-222): x[n_walkers*d] walker-major.
 * Evaluates their log-posterior on the device; n_bad (may be NULL) receives the number of
 * walkers with a non-finite posterior (an error, as in model.py:707-754). */
MCMC_HIP_API int mcmc_hip_set_state(mcmc_hip_ctx* h, const double* x, int32_t* n_bad);
/* current point of every walker: x[W*d], logpost[W], logprior[W], loglike[W], weight[W];
 * any pointer may be NULL */
MCMC_HIP_API int mcmc_hip_get_state(mcmc_hip_ctx* h, double* x, double* logpost, double* logprior,
                       double* loglike, int32_t* weight);

/* Complete per-walker state for checkpoint/resume (mcmc.py:189-214, 1045-1078 -- the reference
 * restarts from the last stored row and cannot save its RNG state, sampler.py:373; here the
 * Philox counter is just `step`, so a resumed run continues bit-identically): x[W*d]
 * walker-major, logpost/logprior/loglike[W], weight/prior_rej/burn_left[W] (int32),
 * n_accept[W] (int64), *step = Metropolis steps taken per walker.  set_ restores all of it
 * without re-evaluating anything (set_prior, a set_target call and set_proposal_cov must precede). */
MCMC_HIP_API int mcmc_hip_get_full_state(mcmc_hip_ctx* h, double* x, double* logpost, double* logprior,
                            double* loglike, int32_t* weight, int32_t* prior_rej,
                            int32_t* burn_left, int64_t* n_accept, uint64_t* step);
MCMC_HIP_API int mcmc_hip_set_full_state(mcmc_hip_ctx* h, const double* x, const double* logpost,
                            const double* logprior, const double* loglike, const int32_t* weight,
                            const int32_t* prior_rej, const int32_t* burn_left,
                            const int64_t* n_accept, uint64_t step);

/* n_steps iterations of MCMC.get_new_sample_metropolis (mcmc.py:545-562) for every walker,
 * asynchronously on the engine's stream; generates the Haar bases the steps need. */
MCMC_HIP_API int mcmc_hip_step(mcmc_hip_ctx* h, int32_t n_steps);
/* The move mcmc_hip_step makes.  MCMC_HIP_MOVE_METROPOLIS (the default): the Gaussian proposal along
 * Haar directions of everything above; `a` is ignored.  MCMC_HIP_MOVE_STRETCH: the affine-invariant
 * stretch move (Goodman & Weare 2010; DESIGN.md section 2, "Stretch move"; stretch_kernels.hip) with
 * scale a (finite, > 1; 2 is the usual choice) on the target of mcmc_hip_set_target_function.  A
 * group of group_size walkers is two halves; one step is two half-updates, in each of which the
 * walkers of one half move to t = p + z (x - p), p the current state of a partner drawn from the
 * OTHER half of the same group, z in [1 / a, a] with density ~ 1 / sqrt(z), accepted with probability
 * min(1, z^(d - 1) (post(t) / post(x))^(1 / temperature)).  The function is called once per half-update
 * with the n_walkers / 2 trial rows of the active half, in ascending walker order.  mcmc_hip_step(n)
 * is 2 n half-updates and ends with the state complete; step counter, weights, max_tries, burn-in and
 * the accept counters mean what they mean for Metropolis steps (one trial per walker and step).
 * No proposal covariance is needed (mcmc_hip_set_proposal_cov is accepted and unused), no basis is
 * formed.  If the callback fails (MCMC_HIP_ERR_CALLBACK) the step counter is that of the last
 * completed step, but half 0 of the interrupted step may already be committed: mcmc_hip_step then
 * answers MCMC_HIP_ERR_STATE until a state is set again (mcmc_hip_set_state / _set_full_state).
 * Refused by mcmc_hip_step with MCMC_HIP_ERR_ARG, each by name: any target but one function (analytic
 * targets, mcmc_hip_set_target_functions), parameter blocks / oversampling / dragging, periodic
 * parameters, emit_capacity > 0, MCMC_HIP_FLAG_INCREMENTAL, group_size < 4 d, and a state in which some
 * parameter has one value in every walker of a half-group (the move never leaves that hyperplane).
 * mcmc_hip_set_move itself refuses an unknown kind and an `a` that is not finite or <= 1. */
enum { MCMC_HIP_MOVE_METROPOLIS = 0, MCMC_HIP_MOVE_STRETCH = 1 };
MCMC_HIP_API int mcmc_hip_set_move(mcmc_hip_ctx* h, int32_t kind, double a);
/* A weighted mixture of ensemble moves in place of the one move above ("Ensemble
 * move mixtures"; ensemble_move_kernels.hip): n = 1 .. 8 members, member j of kind kinds[j] with weight
 * weights[j] (positive and finite; normalised here) and parameters p0[j], p1[j]:
 *   MCMC_HIP_ENSEMBLE_STRETCH   p0 = a > 1: the stretch move above
 *   MCMC_HIP_ENSEMBLE_DE        differential evolution, t = x + gamma (p1 - p2) with two distinct partners
 *                               and gamma = p0 (1 + p1 n), n standard normal: p0 = gamma0 > 0 (the usual
 *                               2.38 / sqrt(2 d) is the caller's to form; 1 hops between modes),
 *                               p1 = sigma >= 0
 *   MCMC_HIP_ENSEMBLE_SNOOKER   the snooker update, t = x + c (x - z) with c = p0 s / |x - z|^2, s the
 *                               projection of the difference of two further partners on x - z:
 *                               p0 = gamma_s > 0 (1.7 is usual); accepted with (|t - z| / |x - z|)^(d - 1)
 * Halves, partners (the other half of the walker's own group, pairwise distinct), the one call of the
 * function per half-update, the callback rule and every limit are those of MCMC_HIP_MOVE_STRETCH; the
 * kind of a step is drawn once per step for the whole ensemble -- every rank and every walker offset
 * draws the same -- from the seed and the step alone.  n = 0 switches the mixture off (the pointers may
 * be NULL).  A mixture needs mcmc_hip_set_move at MCMC_HIP_MOVE_METROPOLIS (mcmc_hip_step refuses both).
 * Refused here with MCMC_HIP_ERR_ARG, the offender named: n outside 0 .. 8, an unknown kind, a weight
 * that is not positive and finite, a <= 1, a gamma that is not finite or <= 0, sigma < 0. */
enum { MCMC_HIP_ENSEMBLE_STRETCH = 0, MCMC_HIP_ENSEMBLE_DE = 1, MCMC_HIP_ENSEMBLE_SNOOKER = 2 };
MCMC_HIP_API int mcmc_hip_set_moves(mcmc_hip_ctx* h, int32_t n, const int32_t* kinds, const double* weights,
                                    const double* p0, const double* p1);
/* wait for queued work; returns MCMC_HIP_ERR_STUCK if a walker tripped max_tries, and
 * MCMC_HIP_ERR_TARGET if a function target returned NaN or +inf inside the prior support */
MCMC_HIP_API int mcmc_hip_sync(mcmc_hip_ctx* h);

/* counters[0] steps per walker so far, [1] accepted steps summed over walkers (n_steps_raw /
 * acceptance of mcmc.py:311-318, 472), [2] id+1 of a stuck walker or 0, [3] rows dropped
 * because emit_capacity was exceeded */
MCMC_HIP_API int mcmc_hip_get_counters(mcmc_hip_ctx* h, int64_t counters[4]);

/* SampleCollection.add rows accumulated since the last drain (mcmc.py:691-707,
 * collection.py:402-427): rows[n][d+5] = (walker id, weight, logpost, logprior, loglike,
 * x[0..d)), walker-major then in chain order.  cap_rows = capacity of `rows` in rows. */
MCMC_HIP_API int mcmc_hip_drain_samples(mcmc_hip_ctx* h, double* rows, int64_t cap_rows, int64_t* n_rows);

/* The same drain at PCIe speed and without a host-side copy: the packed rows are copied into a
 * pinned host slot owned by the library and `*rows` points at them ([*n_rows][d+5], as
 * drain_samples); the slot is reused after `n_slots - 1` further calls (ring of 4 slots unless
 * mcmc_hip_set_drain_slots changed it; 2..64), so the caller may keep reading the rows of the
 * last n_slots - 1 drains in place.  (The exception to "the library never hands out memory":
 * stated here.) */
MCMC_HIP_API int mcmc_hip_drain_samples_pinned(mcmc_hip_ctx* h, const double** rows, int64_t* n_rows);
MCMC_HIP_API int mcmc_hip_set_drain_slots(mcmc_hip_ctx* h, int32_t n_slots);
/* Thinned emission ON THE DEVICE (round 5): OneSamplePoint.add_to_collection with output_thin > 1
 * (collection.py:1373-1383) -- the weights of a walker's accepted rows add up, a row is emitted when
 * the sum reaches `thin`, with weight sum / thin, the remainder carried to its next rows.  `emit:
 * chains` is bound by PCIe (54 GB/s of rows): thinned by T it moves T times fewer.  Served by every
 * incremental Metropolis kernel (round 6: mixtures, periodic parameters and blocks of one parameter
 * too, on the general incremental kernels); the from-scratch and dragging kernels refuse at their
 * first step (thin on the host as before).  thin = 1: off.
 * get / set_thin_carry: the per-walker remainders [W] (part of the state of a resumed run). */
MCMC_HIP_API int mcmc_hip_set_emit_thin(mcmc_hip_ctx* h, int32_t thin);
MCMC_HIP_API int mcmc_hip_get_thin_carry(mcmc_hip_ctx* h, int32_t* carry);
MCMC_HIP_API int mcmc_hip_set_thin_carry(mcmc_hip_ctx* h, const int32_t* carry);

/* Constants the engine derived from set_prior / set_target_* (uniform_logp of prior.py:528-533,
 * mls[d] of tools.py:723, Linv[K*d*d] row-major of functions.py:81-89, cnorm[K] =
 * d log 2pi + log|S_k|, weight[K]); any pointer may be NULL.  Lets tests hand the CPU oracle
 * exactly the problem the kernels evaluate. */
MCMC_HIP_API int mcmc_hip_get_derived_constants(const mcmc_hip_ctx* h, double* uniform_logp, double* mls,
                                   double* Linv, double* cnorm, double* weight);

/* Vector subtracted from every walker before its moments are accumulated (numerical
 * conditioning only; R-1 and covariances are shift invariant).  Only right after a reset. */
MCMC_HIP_API int mcmc_hip_set_moment_shift(mcmc_hip_ctx* h, const double* shift);

/* Streaming replacement of SampleCollection.mean/cov (collection.py:893-981): adds the
 * current state of every walker to the interval accumulators (one "snapshot"). */
MCMC_HIP_API int mcmc_hip_accumulate_moments(mcmc_hip_ctx* h);
/* n_snapshots since the last reset; group_sum[G*d] = sum over snapshots and the group's
 * walkers of x; pooled_S[d*d] = sum over everything of x x^T.  reset != 0 clears them. */
MCMC_HIP_API int mcmc_hip_read_moments(mcmc_hip_ctx* h, int64_t* n_snapshots, double* group_sum,
                          double* pooled_S, int32_t reset);
/* restores accumulators read with reset == 0 (resume: the snapshots taken since the last
 * read-out are part of the state) */
MCMC_HIP_API int mcmc_hip_set_moments(mcmc_hip_ctx* h, int64_t n_snapshots, const double* group_sum,
                         const double* pooled_S);
/* The same read-out without stalling the host (the learn/convergence checkpoint off the
 * critical path): `request` queues the device->host copies of the accumulators and of the
 * accept counter behind the work already in the stream, resets the accumulators in stream
 * order and returns at once; `fetch` waits for those copies only -- launches queued AFTER the
 * request keep running meanwhile.  counters[2] = (steps per walker, accepted steps of all
 * walkers) at the time of the request.  One request may be pending at a time.  The stuck flag
 * travels with the read-out: `fetch` returns MCMC_HIP_ERR_STUCK (after filling its outputs) if
 * a walker had tripped max_tries when the request was served (mcmc.py:717-743) -- the run loop
 * never calls mcmc_hip_sync, so this is where it learns of it. */
MCMC_HIP_API int mcmc_hip_request_moments(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_fetch_moments(mcmc_hip_ctx* h, int64_t* n_snapshots, double* group_sum,
                           double* pooled_S, int64_t counters[2]);

/* Streaming marginal histograms of the ensemble (marginal_kernels.hip): the 1-D densities and 2-D
 * contours GetDist draws from the stored rows (MCSamples.get1DDensity / get2DDensity behind
 * SampleCollection.to_getdist, collection.py), counted here from EVERY walker of every
 * accumulation instead of from the rows that `max_rows` retains.  Same life cycle as the moments.
 * The rule ("Marginals"): on an axis of B bins over [lo, hi] a value is in
 * range iff x >= lo && x <= hi and falls in bin k = min((int)floor((x - lo) * s), B - 1),
 * s = B / (hi - lo) formed in double on the host; x == hi falls in the last bin, a value on an
 * interior edge in the upper one.  Counters are uint64:
 *   1-D entry k (0 <= k < n1) at k (bins1 + 2):            [under, over, c_0 .. c_{bins1-1}]
 *   pair p (0 <= p < n2) at offset_pairs + p (bins2^2 + 1): [outside, c_{0,0} .. ], row-major with the
 *   pair's FIRST parameter as the row; `outside` counts a walker either coordinate of which is out.
 * configure: dims1[n1] sampler indices, 1 <= bins1 <= 1024; pairs[n2][2] ordered (i, j), i != j,
 * 1 <= bins2 <= 64; lo[d], hi[d] indexed by sampler index (read for the parameters in use only:
 * finite, lo < hi).  With m derived rows configured (mcmc_hip_derived_configure, which must come
 * first) an index d + r names row r of z and lo / hi hold d + m entries; a NaN there is counted
 * nowhere by a 1-D entry and `outside` by a pair.  Allocates and zeroes the slab and its pinned read-out; n1 = n2 = 0 frees them
 * (the feature is off).  A bad call returns MCMC_HIP_ERR_ARG and names the argument.
 * accumulate: ONE launch on the engine's stream adds every walker of this process once to every
 * entry (the population a moment snapshot sums); no host synchronisation, no allocation.
 * MCMC_HIP_ERR_STATE without a state or a slab.
 * request / fetch: the contract of mcmc_hip_request_moments / mcmc_hip_fetch_moments -- `request`
 * queues the copy of the slab to pinned host memory and the zeroing of the slab in stream order,
 * `fetch` waits for that copy only; counts[n] with n = n_counters of `layout`,
 * *n_accumulations = accumulations the read-out holds.  One request may be pending.
 * set: restores the counts of an unfinished interval (resume); synchronous.
 * layout: n_counters (0: off), n1, bins1, n2, bins2, offset_pairs; any pointer may be NULL. */
MCMC_HIP_API int mcmc_hip_marginals_configure(mcmc_hip_ctx* h, int32_t n1, const int32_t* dims1, int32_t bins1,
                                 int32_t n2, const int32_t* pairs, int32_t bins2, const double* lo,
                                 const double* hi);
MCMC_HIP_API int mcmc_hip_marginals_accumulate(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_marginals_request(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_marginals_fetch(mcmc_hip_ctx* h, uint64_t* counts, int64_t n, int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_marginals_set(mcmc_hip_ctx* h, const uint64_t* counts, int64_t n, int64_t n_accumulations);
MCMC_HIP_API int mcmc_hip_marginals_layout(const mcmc_hip_ctx* h, int64_t* n_counters, int32_t* n1, int32_t* bins1,
                              int32_t* n2, int32_t* bins2, int64_t* offset_pairs);

/* Lagged cross-products of the ensemble for the integrated autocorrelation time
 * (autocorr_kernels.hip).  Same life cycle as the marginals.  The engine keeps a ring of the last
 * lags + 1 accumulated snapshots of the configured parameters and, per slot, the slot's group sums.
 * The rule ("Autocorrelation"), all in float64 with separate roundings: with
 * a[l,i] = x_t[i][l] - shift_i (the moment shift) and b[l,i] = x_{t-k}[i][l] - shift_i, per group g and
 * configured dimension i, S_t[g,i] = sum_l a and P[g,k,i] = sum_l a*b are chains over the group's
 * walkers in ascending order from +0.0; for every lag k = 0 .. min(lags, held - 1) the accumulators
 * add the groups in ascending order from their current value: accP[k,i] += P[g,k,i],
 * accA[k,i] += S_t[g,i], accB[k,i] += S_{t-k}[g,i], and n_pairs[k] += 1 once per accumulation.
 * Lags not yet held are left untouched.
 * configure: dims[n_dims] distinct sampler indices, 1 <= lags <= 64; allocates the ring
 * ((lags + 1) n_dims W doubles) and zeroes the accumulators; n_dims = 0 frees them (the feature is
 * off).  A bad call returns MCMC_HIP_ERR_ARG and names the argument; a ring that does not fit the
 * free device memory names `lags` and the bytes needed.
 * accumulate: two launches on the engine's stream (the group chains, the pooling), right after
 * mcmc_hip_accumulate_moments on the same population; no host synchronisation, no allocation.
 * MCMC_HIP_ERR_STATE without a state or before configure.
 * request / fetch: `request` queues the copy of the accumulators to pinned host memory and their
 * zeroing in stream order and keeps the ring, `fetch` waits for that copy only; sums[n] with
 * n = n_doubles of `layout`, laid out [3][lags + 1][n_dims] (P, A, B), n_pairs[lags + 1].  One request
 * may be pending.
 * set: restores open accumulators (resume); synchronous.  The ring is not restored: it refills.
 * reset: empties the ring (the accumulators stay).  The ring is otherwise emptied only by
 * configure and by a change of the moment shift, which also zeroes the accumulators;
 * mcmc_hip_set_state / set_full_state keep it.
 * layout: n_dims, lags, n_doubles, snapshots held -- all zero: off; any pointer may be NULL. */
MCMC_HIP_API int mcmc_hip_autocorr_configure(mcmc_hip_ctx* h, int32_t n_dims, const int32_t* dims, int32_t lags);
MCMC_HIP_API int mcmc_hip_autocorr_accumulate(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_autocorr_request(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_autocorr_fetch(mcmc_hip_ctx* h, double* sums, int64_t n, int64_t* n_pairs);
MCMC_HIP_API int mcmc_hip_autocorr_set(mcmc_hip_ctx* h, const double* sums, int64_t n, const int64_t* n_pairs);
MCMC_HIP_API int mcmc_hip_autocorr_reset(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_autocorr_layout(const mcmc_hip_ctx* h, int32_t* n_dims, int32_t* lags, int64_t* n_doubles,
                             int32_t* held);

/* Best fit, MAP and profile likelihoods of the ensemble (bestfit_kernels.hip).  Same life cycle as
 * the marginals.  The rule ("Best fit and profiles"): the ordering key of a
 * double v is b ^ ((b >> 63) ? ~0 : 1 << 63) with b = bits(v), an unsigned 64-bit integer whose order
 * is the order of the doubles (-0.0 < +0.0; -inf is the smallest non-empty key; NaN is skipped;
 * 0 = empty).  An accumulation reads x, logpost, logprior and loglike as the state holds them
 * between two launches.
 * records[2][6 + d] as 64-bit words -- 0: map (maximum of logpost), 1: bestfit (maximum of loglike):
 * key, global walker id (walker_offset + w), step counter at the accumulation, bits of logpost,
 * logprior, loglike, bits of x[d].  Within an accumulation ties on the key go to the lowest walker
 * id; a later accumulation replaces a record only with a strictly greater key.
 * slab[n][bins]: bin k of configured parameter dims[e] holds the largest key of the profiled
 * `quantity` among the walkers whose x[dims[e]] is in range (lo <= x <= hi) and falls in that bin --
 * the marginals' rule, k = min((int)floor((x - lo) * s), bins - 1), s = bins / (hi - lo).
 * configure: n >= 0 parameters (n = 0: the records only; dims, lo, hi may then be NULL), bins in
 * 1..1024, lo / hi [d] the fixed range of every parameter in use; empties everything.
 * request / fetch / set: as for the marginals, for slab and records together; the read-out leaves
 * slab and records empty in stream order.  One request may be pending.  Before configure,
 * accumulate / request / set answer MCMC_HIP_ERR_STATE and nothing is allocated or launched.
 * layout: on (0 before configure), n, bins, quantity, n_slab = n * bins, n_records = 2 (6 + d); any
 * pointer may be NULL. */
#define MCMC_HIP_BESTFIT_LOGLIKE 0
#define MCMC_HIP_BESTFIT_LOGPOST 1
MCMC_HIP_API int mcmc_hip_bestfit_configure(mcmc_hip_ctx* h, int32_t n, const int32_t* dims, int32_t bins,
                               const double* lo, const double* hi, int32_t quantity);
MCMC_HIP_API int mcmc_hip_bestfit_accumulate(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_bestfit_request(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_bestfit_fetch(mcmc_hip_ctx* h, uint64_t* slab, int64_t n_slab, uint64_t* records,
                           int64_t n_records, int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_bestfit_set(mcmc_hip_ctx* h, const uint64_t* slab, int64_t n_slab, const uint64_t* records,
                         int64_t n_records, int64_t n_accumulations);
MCMC_HIP_API int mcmc_hip_bestfit_layout(const mcmc_hip_ctx* h, int32_t* on, int32_t* n, int32_t* bins,
                            int32_t* quantity, int64_t* n_slab, int64_t* n_records);

/* Evidence of the run: the sums of the ellipsoid-truncated harmonic mean (evidence_kernels.hip).
 * The rule ("Evidence").  An ellipsoid is m[d] | Linv[d][d] (row-major, lower
 * triangular, the inverse of chol(C) formed on the host) | c, n_ell = d + d d + 1 doubles; c is
 * taken ON THE DEVICE when the ellipsoid becomes active: the exact maximum of logpost over this
 * process's walkers (0 if none is a number).  An accumulation reads x and logpost as the state
 * holds them between two launches; per walker s = |Linv (x - m)|^2 (every sum one ascending chain
 * from +0.0, products and additions rounded separately) and e = dexp(min(c - logpost, 700)); per
 * group g of group_size walkers and radius r, S = the sum of e over the walkers with s <= r2[r] in
 * ascending order from +0.0, then acc[g][r] = acc[g][r] + S and cnt[g][r] += the walkers inside;
 * `clamped` counts the arguments above 700.
 * configure: n_radii in 1..8 ascending finite positive r2 (n_radii = 0 frees everything: off),
 * d <= 256; empties everything, no ellipsoid is active.
 * set_ellipsoid: the FIRST one after configure becomes active at once (a state is needed); a later
 * one is only staged (replacing an earlier staged one) and becomes active, with a fresh c, in
 * stream order inside the next closing request.  MCMC_HIP_ERR_NOT_PD if cov has no Cholesky factor.
 * request(close): queue the read-out of sums, counts, clamped and c behind the work already in
 * the stream, with the ellipsoids as they are now; close != 0 also zeroes sums, counts and clamped
 * and activates a staged ellipsoid, all in stream order (close = 0 disturbs nothing).  One request
 * may be pending.
 * fetch: waits for that copy only.  sums / counts [n = G n_radii]; active / staged [n_ell] each (c of
 * the staged one is 0), *has_active / *has_staged say which exist.
 * set: an unfinished interval goes back (resume): active with its c (NULL: none), staged (NULL:
 * none); no maximum is taken.
 * Before configure, accumulate / request / set / set_ellipsoid answer MCMC_HIP_ERR_STATE and
 * nothing is allocated or launched.  layout: any pointer may be NULL; all zero: off. */
MCMC_HIP_API int mcmc_hip_evidence_configure(mcmc_hip_ctx* h, int32_t n_radii, const double* r2);
MCMC_HIP_API int mcmc_hip_evidence_set_ellipsoid(mcmc_hip_ctx* h, const double* m, const double* cov);
MCMC_HIP_API int mcmc_hip_evidence_accumulate(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_evidence_request(mcmc_hip_ctx* h, int32_t close);
MCMC_HIP_API int mcmc_hip_evidence_fetch(mcmc_hip_ctx* h, double* sums, uint64_t* counts, int64_t n,
                            uint64_t* clamped, int64_t* n_accumulations, double* active, double* staged,
                            int64_t n_ell, int32_t* has_active, int32_t* has_staged);
MCMC_HIP_API int mcmc_hip_evidence_set(mcmc_hip_ctx* h, const double* sums, const uint64_t* counts, int64_t n,
                          uint64_t clamped, int64_t n_accumulations, const double* active,
                          const double* staged, int64_t n_ell);
MCMC_HIP_API int mcmc_hip_evidence_layout(const mcmc_hip_ctx* h, int32_t* on, int32_t* n_radii, int32_t* n_groups,
                             int64_t* n_ell, int32_t* has_active, int32_t* has_staged,
                             int64_t* n_accumulations);

/* Derived parameters: m <= 32 rows z[m][W], dimension-major like x, that the CALLER fills on the
 * engine's stream (mcmc_hip_stream_handle) from the state as it lies in HBM, and their moments
 * (derived_kernels.hip).  Same life cycle as the marginals.  The rule ("Derived"):
 * with a_j = z_j - shift_j and b_c = x_{cross_dims[c]} - (moment shift)_{cross_dims[c]}, a walker is used
 * iff all m of its derived values are finite; per group g of group_size walkers, over the used
 * walkers in ascending order from +0.0 (one chain each, product and addition rounded separately):
 * N[g], A[g][j] = sum a_j, B[g][j][k] = sum a_j a_k (k <= j), C[g][j][c] = sum a_j b_c and, beside
 * them, X[g][c] = sum b_c and V[g][c] = sum b_c b_c (the sampled parameters over the same walkers); the pooled
 * accumulators then add the groups in ascending order from their current value.  Exact and
 * order-independent per name: bad[j] counts the non-finite values, min[j] / max[j] are those of the
 * finite ones (NaN: none yet).
 * configure: m in 1..32 (m = 0 frees everything: off), n_cross in 0..d distinct sampler indices,
 * shift[m] finite; allocates and zeroes z and the accumulators.  It must precede
 * mcmc_hip_marginals_configure, whose indices d .. d + m - 1 name the rows of z (lo / hi then hold
 * d + m entries), and is refused while marginals are configured.
 * buffers: the device pointers of x[d][W] and z[m][W].  x is read-only for the caller.
 * set_values / get_values: host copies of z, point-major [W][m]; synchronous.
 * set_group_size: the groups of the sums, by default the engine's group_size; any divisor of
 * n_walkers (a group may be far larger than LDS).  Synchronous; call it between read-outs.
 * accumulate: two launches on the engine's stream (the group chains, the pooling) over z as it is;
 * no host synchronisation, no allocation.  MCMC_HIP_ERR_STATE without a state or before configure.
 * request / fetch: `request` queues the copy of the accumulators to pinned host memory and their
 * zeroing in stream order, `fetch` waits for that copy only.  A[m], B[m (m + 1) / 2] with (j, k <= j)
 * at j (j + 1) / 2 + k, C[m][n_cross], X[n_cross] and V[n_cross] (may be NULL when n_cross = 0), bad[m], min[m],
 * max[m].  One
 * request may be pending.
 * set: restores open accumulators (resume); synchronous.
 * layout: m (0: off), n_cross, group_size, accumulations since the last request; any pointer may be NULL. */
MCMC_HIP_API int mcmc_hip_derived_configure(mcmc_hip_ctx* h, int32_t m, int32_t n_cross, const int32_t* cross_dims,
                               const double* shift);
MCMC_HIP_API int mcmc_hip_derived_set_group_size(mcmc_hip_ctx* h, int32_t group_size);
MCMC_HIP_API int mcmc_hip_derived_layout(const mcmc_hip_ctx* h, int32_t* m, int32_t* n_cross, int32_t* group_size,
                            int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_derived_buffers(mcmc_hip_ctx* h, uint64_t* x_device_ptr, uint64_t* z_device_ptr);
MCMC_HIP_API int mcmc_hip_derived_set_values(mcmc_hip_ctx* h, const double* values);
MCMC_HIP_API int mcmc_hip_derived_get_values(mcmc_hip_ctx* h, double* values);
MCMC_HIP_API int mcmc_hip_derived_accumulate(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_derived_request(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_derived_fetch(mcmc_hip_ctx* h, uint64_t* n_used, double* A, double* B, double* C,
                           double* X, double* V, uint64_t* bad, double* min, double* max,
                           int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_derived_set(mcmc_hip_ctx* h, uint64_t n_used, const double* A, const double* B,
                         const double* C, const double* X, const double* V, const uint64_t* bad,
                         const double* min, const double* max, int64_t n_accumulations);

/* Importance reweighting: the weighted sums of the sampled parameters under w = exp(delta)
 * (importance_kernels.hip).  The rule ("Importance").  The CALLER owns the
 * log-weights delta[n_alt][W] (row k: alternative k) and fills them on the engine's stream from the state
 * x[d][W], whose device pointer `layout` hands out.
 * configure: n_alt alternatives (0: off, everything is freed; at most 8), cov[k] != 0: alternative k
 *   keeps the full weighted covariance (d <= 128).  Per (alternative, group) the chains are
 *   S1 | S2 | M[d] | V[d] | Q[d (d - 1) / 2] with (i, j < i) at i (i - 1) / 2 + j, Q with cov[k] alone;
 *   `sums` holds alternative k's [n_groups][n_chains] doubles at offsets[k], n_sums doubles in all.
 * accumulate: queues one accumulation of every walker of this process on the engine's stream.  The first
 *   accumulation after configure, a closing request or a set with n_accumulations = 0 OPENS an interval:
 *   c[k] = the exact maximum of the finite delta[k] (0.0: none) is taken on the device first.
 * request: queues the read-out behind the work already in the stream; close != 0: also zeroes the sums.
 * fetch: waits for the copy only.  n[n_alt][n_groups] the used walkers, counters[n_alt][3] = zero,
 *   nonfinite, clamped, c[n_alt].
 * set: restores an unfinished interval (resume).
 * set_group_size: the groups of the sums (default: the engine's group_size), any divisor of n_walkers;
 *   the sums are dropped.
 * Before configure, accumulate / request / set answer MCMC_HIP_ERR_STATE and nothing is allocated or
 * launched.  layout: any pointer may be NULL (offsets, cov: 8 entries each); n_alt == 0: off. */
MCMC_HIP_API int mcmc_hip_importance_configure(mcmc_hip_ctx* h, int32_t n_alt, const int32_t* cov);
MCMC_HIP_API int mcmc_hip_importance_set_group_size(mcmc_hip_ctx* h, int32_t group_size);
MCMC_HIP_API int mcmc_hip_importance_layout(const mcmc_hip_ctx* h, int32_t* n_alt, int32_t* n_groups,
                               int64_t* n_sums, int64_t* offsets, int32_t* cov, int64_t* n_accumulations,
                               uint64_t* x_device_ptr);
MCMC_HIP_API int mcmc_hip_importance_accumulate(mcmc_hip_ctx* h, uint64_t delta_device_ptr);
MCMC_HIP_API int mcmc_hip_importance_request(mcmc_hip_ctx* h, int32_t close);
MCMC_HIP_API int mcmc_hip_importance_fetch(mcmc_hip_ctx* h, double* sums, int64_t n_sums, uint64_t* n,
                              int64_t n_groups, uint64_t* counters, double* c, int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_importance_set(mcmc_hip_ctx* h, const double* sums, int64_t n_sums, const uint64_t* n,
                            int64_t n_groups, const uint64_t* counters, const double* c,
                            int64_t n_accumulations);

/* Reweighted marginal histograms of the importance alternatives (importance_hist_kernels.hip).  The rule
 * ("Importance marginals"): the entries, ranges and bins are those of
 * mcmc_hip_marginals_configure; a used walker of alternative k adds the fixed-point weight
 * q = floor(min(e, 2^16) * 2^32), e being the weight the sums use, where marginals_accumulate adds 1;
 * saturated[k] counts e > 2^16.  Every counter is a 128-bit unsigned integer kept as two words (lo, hi):
 * its value is (hi * 2^64 + lo) * 2^-32 at the scale exp(c[k]) of its interval.
 * hist_configure: on[n_alt], != 0: alternative k keeps histograms.  After BOTH importance_configure and
 *   marginals_configure (MCMC_HIP_ERR_STATE otherwise); all zeros releases everything, and so do
 *   marginals_configure and importance_configure.  The slab: per alternative with on[k], ascending,
 *   lo[n_counters] | hi[n_counters] in the layout of the marginals slab, then saturated[n_hist].
 * The intervals are the sums': importance_accumulate adds to both (and launches nothing new when the
 *   histograms are off), importance_request copies out both and with close != 0 zeroes both; a request is
 *   refused while a histogram read-out of the last one has not been fetched; importance_set_group_size
 *   empties both.
 * hist_fetch: the read-out of the last importance_request (before or after importance_fetch); lo and hi
 *   hold n = n_hist * n_counters words each, saturated n_hist.
 * hist_set: restores an unfinished interval (resume), behind importance_set, which carries c and
 *   n_accumulations.
 * hist_layout: any pointer may be NULL (on: 8 entries); n_words == 0: off. */
MCMC_HIP_API int mcmc_hip_importance_hist_configure(mcmc_hip_ctx* h, const int32_t* on);
MCMC_HIP_API int mcmc_hip_importance_hist_layout(const mcmc_hip_ctx* h, int32_t* n_hist, int32_t* on,
                                    int64_t* n_counters, int64_t* n_words);
MCMC_HIP_API int mcmc_hip_importance_hist_fetch(mcmc_hip_ctx* h, uint64_t* lo, uint64_t* hi, int64_t n,
                                   uint64_t* saturated, int64_t* n_accumulations);
MCMC_HIP_API int mcmc_hip_importance_hist_set(mcmc_hip_ctx* h, const uint64_t* lo, const uint64_t* hi, int64_t n,
                                 const uint64_t* saturated);

/* The learn / convergence checkpoint ON THE DEVICE (MCMC.check_convergence_and_learn_proposal,
 * mcmc.py:773-1032; checkpoint_kernels.hip): the intervals between checkpoints are kept in a
 * device ring, the statistics of the window (the later half of the run, mcmc.py:787-790) are
 * summed there, R-1 of the means is formed (mcmc.py:856-889, functions.py:81-89) and -- when
 * learn_lo <= R-1 x group_size <= learn_hi (mcmc.py:1009-1023) -- the proposal transform is
 * refreshed IN PLACE (proposal.py:226-260) with the operations of mcmc_hip_set_proposal_cov, all
 * in stream order: launches queued after checkpoint_solve use the new proposal, no host round
 * trip.  Call order per checkpoint: request_moments (the host's copy of the interval) ->
 * checkpoint_begin (window sums + the buffer an all-reduce carries: *payload_device_ptr is a
 * device pointer to *payload_len doubles = [chains, sum N, accepted since the last checkpoint,
 * steps x walkers since, accepted | sum N cov (d*d) | sum of chain means (d) | sum of m m^T (d*d)];
 * with several processes it is all-reduced on the engine's stream before the solve -- by the
 * library itself when a communicator is attached (mcmc_hip_set_comm: ncclAllReduce in place,
 * queued by checkpoint_begin), else by the caller, see mcmc_hip_stream_handle) -> checkpoint_solve -> [more launches] -> checkpoint_fetch:
 * stats = {R-1 of the chain (= group) means, status (0 ok; 1, 2, 3: the LinAlgError cases of
 * mcmc.py:870-887), 1 if the proposal was refreshed, chains, sum N, accepted since the last
 * checkpoint, steps x walkers since, accepted}, mean_of_covs[d*d].
 * checkpoint_set_ring (re)loads the ring with the intervals the caller still holds (start: none;
 * resume; growth of the window beyond the capacity): group_sum[n][G*d], pooled_S[n][d*d]. */
MCMC_HIP_API int mcmc_hip_checkpoint_set_ring(mcmc_hip_ctx* h, int32_t n_intervals, const double* group_sum,
                                 const double* pooled_S, int32_t min_capacity);
MCMC_HIP_API int mcmc_hip_checkpoint_set_accepted(mcmc_hip_ctx* h, int64_t accepted_at_last_checkpoint);
MCMC_HIP_API int mcmc_hip_checkpoint_begin(mcmc_hip_ctx* h, int32_t n_window_intervals, int64_t n_window_snapshots,
                              double steps_since, uint64_t* payload_device_ptr, int32_t* payload_len);
MCMC_HIP_API int mcmc_hip_checkpoint_solve(mcmc_hip_ctx* h, double learn_lo, double learn_hi);
MCMC_HIP_API int mcmc_hip_checkpoint_fetch(mcmc_hip_ctx* h, double stats[8], double* mean_of_covs);
/* Instead of checkpoint_solve: only the (all-reduced) payload is read out behind the launch --
 * checkpoint_begin -> checkpoint_request_payload -> [the next launch] -> checkpoint_fetch_payload
 * (waits for the copy; n = the payload_len of checkpoint_begin) -- and the caller solves it on the
 * host (mcmc_hip_gelman_rubin, mcmc_hip_set_proposal_cov) while that launch runs.  The window sums
 * and the collective stay on the device in stream order; the single-workgroup d^3 solve leaves
 * the stream (replaces the gather + host arithmetic of mcmc.py:791-793, 856-889). */
MCMC_HIP_API int mcmc_hip_checkpoint_request_payload(mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_checkpoint_fetch_payload(mcmc_hip_ctx* h, double* payload, int32_t n);
/* R-1 of the confidence-interval bounds ON THE DEVICE (mcmc.py:918-1002), in every emit mode: a ring
 * of n_slots ensemble snapshots [slot][d][n_walkers] (bounds_configure; 0 frees it);
 * bounds_snapshot(slot) copies the current points into a slot in stream order (the caller decides
 * which: a thinned record of the later half of the run, sampler.py `_bounds_take`);
 * bounds_statistics forms, per chain (= walker group) and parameter, the lower and the upper
 * bound as GetDist's `MCSamples.confidence(i, limfrac, upper)` does (mcmc.py:927-929: the sample
 * at which the cumulative weight first reaches limfrac * norm, resp. (1 - limfrac) * norm) from
 * the chain's samples in the n_window listed slots (unit weights: exact order statistics,
 * selected in LDS) and returns stats[1 + 4 d] = {chains, sum_c lo_i, sum_c hi_i, sum_c lo_i^2,
 * sum_c hi_i^2} with the moment shift (mcmc_hip_set_moment_shift) subtracted from the bounds --
 * summed over the chains of ALL ranks when a communicator is attached (mcmc.py:957
 * `mpi.gather(bound)`); np.std(bounds, axis=0) of mcmc.py:977 follows from them.  `bounds`
 * (may be NULL) receives this rank's [G][d][2].  Synchronous.  n_window * group_size <= 16384.
 * get_slot / set_slot: a slot as x[n_walkers][d] (checkpoint / resume). */
MCMC_HIP_API int mcmc_hip_bounds_configure(mcmc_hip_ctx* h, int32_t n_slots);
MCMC_HIP_API int mcmc_hip_bounds_snapshot(mcmc_hip_ctx* h, int32_t slot);
MCMC_HIP_API int mcmc_hip_bounds_statistics(mcmc_hip_ctx* h, int32_t n_window, const int32_t* slots, double limfrac,
                               double* stats, double* bounds);
MCMC_HIP_API int mcmc_hip_bounds_get_slot(mcmc_hip_ctx* h, int32_t slot, double* x);
MCMC_HIP_API int mcmc_hip_bounds_set_slot(mcmc_hip_ctx* h, int32_t slot, const double* x);
/* the engine's HIP stream (a hipStream_t as an integer), for callers that queue their own work
 * -- the all-reduce of a multi-process checkpoint -- in order with the engine's */
MCMC_HIP_API uint64_t mcmc_hip_stream_handle(const mcmc_hip_ctx* h);

/* Multi-GPU: the communicator of the walker shards -- RCCL over xGMI, one process per GPU
 * (SURVEY 8e).  Stands in for the mpi4py calls of the reference's checkpoint: the gather of
 * (N, mean, cov, acceptance rate) to the root and the broadcasts back (mcmc.py:791-793
 * `mpi.array_gather`, :1005-1007 and :1021 `mpi.share`; mpi.py:178-191) become ONE all-reduce(sum)
 * of pooled sufficient statistics.  A communicator is a process-level object (created before
 * the first engine: the job's seed is agreed through it, sampler.py:369-384):
 *   rank 0: mcmc_hip_comm_unique_id(id) -> the host hands `id` to every rank out of band (any
 *   launcher's store; cobaya_amd/dist.py uses MASTER_ADDR/MASTER_PORT) -> every rank:
 *   mcmc_hip_comm_create(id, rank, n_ranks, device) [collective: ncclCommInitRank] ->
 *   mcmc_hip_set_comm(engine, comm).
 * With a communicator attached, mcmc_hip_checkpoint_begin queues `ncclAllReduce` of its payload
 * IN PLACE on the engine's stream, between the payload and the solve kernel: every rank solves
 * the same reduced statistics and refreshes its own proposal, no host bounce and no host
 * synchronisation.  mcmc_hip_comm_allreduce reduces a HOST buffer (staged through pinned memory,
 * synchronous; op 0 = sum, 1 = max): counters, the host-path checkpoint's payload, the bench
 * clock.  mcmc_hip_comm_allreduce_device reduces n doubles at a device pointer in order on a
 * caller's stream (0: the communicator's own).  RCCL is bound at run time (dlopen of
 * librccl.so.1, or $MCMC_HIP_RCCL_LIB): single-GPU runs never load it.
 * mcmc_hip_comm_last_error(NULL): the last failure before a communicator existed. */
typedef struct mcmc_hip_comm mcmc_hip_comm;
#define MCMC_HIP_COMM_ID_BYTES 128
MCMC_HIP_API const char* mcmc_hip_comm_version(void);      /* "RCCL 2.x.y", "" if it cannot be loaded */
MCMC_HIP_API const char* mcmc_hip_comm_last_error(const mcmc_hip_comm* c);
MCMC_HIP_API int mcmc_hip_comm_unique_id(uint8_t id[MCMC_HIP_COMM_ID_BYTES]);
MCMC_HIP_API int mcmc_hip_comm_create(const uint8_t id[MCMC_HIP_COMM_ID_BYTES], int32_t rank, int32_t n_ranks,
                         int32_t device, mcmc_hip_comm** out);
MCMC_HIP_API void mcmc_hip_comm_destroy(mcmc_hip_comm* c);
MCMC_HIP_API int mcmc_hip_comm_rank(const mcmc_hip_comm* c);
MCMC_HIP_API int mcmc_hip_comm_size(const mcmc_hip_comm* c);
MCMC_HIP_API int mcmc_hip_comm_allreduce(mcmc_hip_comm* c, double* buf, int64_t n, int32_t op);
MCMC_HIP_API int mcmc_hip_comm_allreduce_device(mcmc_hip_comm* c, uint64_t device_ptr, int64_t n, int32_t op,
                                   uint64_t stream);
/* HIP-event time (microseconds per call) of `reps` back-to-back in-stream all-reduces of n doubles
 * on the communicator's own stream and scratch buffer -- what one device checkpoint's collective
 * costs the stream (bench.py reports it).  Collective: every rank must call it alike. */
MCMC_HIP_API int mcmc_hip_comm_time_allreduce(mcmc_hip_comm* c, int64_t n, int32_t reps, double* us_per_call);
/* attach (or, with NULL, detach) the communicator the device checkpoint reduces over; the
 * communicator must live on the engine's device and outlive the engine */
MCMC_HIP_API int mcmc_hip_set_comm(mcmc_hip_ctx* h, mcmc_hip_comm* c);

/* The R-1 arithmetic of MCMC.check_convergence_and_learn_proposal (mcmc.py:856-889) on
 * reduced sufficient statistics (what the RCCL all-reduce of SURVEY 8e carries):
 * n_chains, sum_N = sum_c N_c, sum_Ncov[d*d] = sum_c N_c cov_c, sum_mean[d] = sum_c m_c,
 * sum_mm[d*d] = sum_c m_c m_c^T.  Outputs Rminus1 and mean_of_covs[d*d].
 * Returns MCMC_HIP_ERR_NOT_PD where the reference catches LinAlgError (mcmc.py:870-887). */
MCMC_HIP_API int mcmc_hip_gelman_rubin(int32_t d, double n_chains, double sum_N, const double* sum_Ncov,
                          const double* sum_mean, const double* sum_mm, double* Rminus1,
                          double* mean_of_covs);

/* HIP-event time (ms) spent in step kernels / basis kernels / moment kernels since the last
 * call with reset != 0, and the number of step-kernel launches: the live measurement
 * bench.py's roofline block uses.  Timing is enabled by mcmc_hip_enable_timing(h, 1).  Every
 * step kernel is timed; of the direction and moment regions one in eight, scaled to all of
 * them (an event record costs the stream about 6 us between two dependent kernels). */
MCMC_HIP_API int mcmc_hip_enable_timing(mcmc_hip_ctx* h, int32_t on);
/* incremental mode: the carried y[n_walkers][n_modes * d] -- part of the state a bit-identical resume
 * needs (call mcmc_hip_set_whitened after mcmc_hip_set_full_state) */
MCMC_HIP_API int mcmc_hip_get_whitened(mcmc_hip_ctx* h, double* y);
MCMC_HIP_API int mcmc_hip_set_whitened(mcmc_hip_ctx* h, const double* y);
/* incremental mode, Gaussian mixtures (gaussian_mixture.py:138-163): 1 if the step kernel this
 * engine's configuration selects CARRIES the log-density a_k = -(c_k + chi2_k) / 2 of every mode
 * with the walker (round 5: step_inc_mix_kernel -- 2..4 modes at d <= 64, 5 at d <= 32, 6 at d <= 28, no periodic parameter,
 * Metropolis steps, emit_capacity 0), moved along the whitened direction like the carried
 * log-likelihood of a single mode; 0 if every chi2_k is summed from the trial's residual (the
 * general kernels: more modes, periodic parameters, emitted rows).  The
 * specification (oracle/mcmc_oracle.c: carries_modes) takes the rule from here.  The carried
 * a[n_walkers][n_modes] are part of the state a bit-identical resume needs (call
 * mcmc_hip_set_mode_logdensities after mcmc_hip_set_whitened; without it they are re-anchored on y
 * at the next step). */
MCMC_HIP_API int mcmc_hip_incremental_carries_modes(const mcmc_hip_ctx* h);
/* incremental mode, ONE mode with periodic parameters (prior.py:658-676): 1 if this configuration
 * runs on step_inc_kernel<.., periodic> (1..16 periodic parameters, Metropolis steps, emit_capacity 0),
 * whose rule since round 5 is: a periodic coordinate is wrapped only where the trial leaves
 * [lo, hi), and the log-likelihood is carried along the whitened direction, re-summed from the
 * moved residual at a step that wraps; 0: the coordinate passes through the wrap at every step
 * (the general kernels).  The specification (oracle: carry_periodic) takes the rule from here. */
MCMC_HIP_API int mcmc_hip_incremental_carries_periodic(const mcmc_hip_ctx* h);
/* test entry: the two-lane incremental kernels decide `Ea > delta` from a single-precision estimate
 * ea_f of the accept variate Ea = -log((2 ka + 1) 2^-29) wherever the two are further apart than
 * 2^-14, which is right as long as |ea_f - Ea| <= 2^-16 for every 28-bit ka.  Runs a small kernel
 * over ka = 1 .. 2^28 - 1 on the current device (milliseconds): the largest |ea_f - Ea| and the ka
 * that attains it. */
MCMC_HIP_API int mcmc_hip_accept_estimate_error(double* max_err, uint32_t* ka_at_max);
/* test entry: one function of the device math (det_math.h) applied to n <= 2^24 elements on the
 * current device, raw 64-bit words in and out, for the bit-for-bit comparison with the oracle on whole
 * argument domains (tests/test_gpu_math_domains.py).  Words per element, in -> out (a double is its
 * bit pattern, a 32-bit integer sits in the low half of its word):
 *   PHILOX   k0 k1 c0 c1 c2 c3 -> w0 w1 w2 w3        U52        k -> u
 *   DLOG, DEXP, DLOG_TAB, DEXP_TAB, SQRT_MIDRANGE, SQRT   x -> f(x)
 *   SINCOS2PI  k -> sin cos                          NEG_LOG_SHORT_25 / _29   n -> -log(n 2^-b)
 *   DIV_BY   a w R -> div_by(a, w, R)                 DIV        a w -> a / w
 * args[n * words in] on the host, or NULL for a function of one word: element i then has the argument
 * first + i * stride (the integer domains need no upload).  out[n * words out] on the host.
 * MCMC_HIP_ERR_ARG for an unknown function, a null `out`, NULL args where a function takes more than
 * one word, or n outside [0, 2^24]. */
enum {
    MCMC_HIP_PROBE_PHILOX = 0, MCMC_HIP_PROBE_U52 = 1, MCMC_HIP_PROBE_DLOG = 2, MCMC_HIP_PROBE_DEXP = 3,
    MCMC_HIP_PROBE_SINCOS2PI = 4, MCMC_HIP_PROBE_NEG_LOG_SHORT_25 = 5, MCMC_HIP_PROBE_NEG_LOG_SHORT_29 = 6,
    MCMC_HIP_PROBE_DLOG_TAB = 7, MCMC_HIP_PROBE_DEXP_TAB = 8, MCMC_HIP_PROBE_SQRT_MIDRANGE = 9,
    MCMC_HIP_PROBE_SQRT = 10, MCMC_HIP_PROBE_DIV_BY = 11, MCMC_HIP_PROBE_DIV = 12
};
#define MCMC_HIP_PROBE_MAX_ELEMENTS (1 << 24)
MCMC_HIP_API int mcmc_hip_math_probe(int32_t fn, const uint64_t* args, uint64_t first, uint64_t stride,
                                     int64_t n, uint64_t* out);
MCMC_HIP_API int mcmc_hip_get_mode_logdensities(mcmc_hip_ctx* h, double* a);
MCMC_HIP_API int mcmc_hip_set_mode_logdensities(mcmc_hip_ctx* h, const double* a);

/* name of the step kernel the last mcmc_hip_step launched, e.g.
 * "mcmc::step_pair_kernel<true, false> (d=30)" -- reported by the launcher itself, so that
 * profiles and bench lines quote the kernel that ran ("" before the first step) */
MCMC_HIP_API const char* mcmc_hip_last_step_kernel(const mcmc_hip_ctx* h);
MCMC_HIP_API int mcmc_hip_kernel_times(mcmc_hip_ctx* h, double ms[3], int64_t* n_step_launches, int32_t reset);
/* binned Gaussian target: HIP-event time (ms) and number of launches of the three kernels of a
 * step -- pl_walker_kernel, pl_residual_kernel, pl_chi2_kernel -- since the last reset */
MCMC_HIP_API int mcmc_hip_binned_kernel_times(mcmc_hip_ctx* h, double ms[3], int64_t n_launches[3], int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* MCMC_HIP_H */
