// libmcmc_hip.so: the binned Gaussian target (pliklite_kernels.hip) and function targets
// (function_kernels.hip) -- their setters, evaluation and steppers.
#include "ctx.h"
#include "host_linalg.h"

namespace {

// ------------------------------------------------------------------ the trial pipeline
// mcmc_hip_step on a target that is evaluated outside the walker kernel: per step one launch
// [accept of the previous trial +] proposal, then the target on the trial points; a call ends with
// the accept of its last trial, so the state is complete between calls.  The steps are cut into
// spans of at most max_cyc cycles of L (step_span.h), whose directions go to h->V, and every step
// is placed in w, the walker kernel's arguments (w.s: its StepArgs).  The stepper's own parts:
// directions(span) forms the span's directions; launch(accept, propose) launches the walker kernel
// on w; evaluate() evaluates the trial.  All three return a code of mcmc_hip.h.  The launch has
// settled the previous trial, so an evaluation that fails drops THIS trial only -- state and step
// counter stay as of the last completed step -- and ends the call with its code.
template <class WalkerArgs, class Directions, class Launch, class Evaluate>
int trial_pipeline(mcmc_hip_ctx* h, int n_steps, int L, int max_cyc, WalkerArgs& w, Directions directions,
                   Launch launch, Evaluate evaluate)
{
    const unsigned long long Lu = (unsigned long long)L;
    bool pending = false;   // a trial has been proposed and evaluated, not yet accepted / rejected
    int rc = MCMC_HIP_OK;
    for (int left = n_steps; left > 0 && rc == MCMC_HIP_OK;) {
        const StepSpan sp = step_span(h->step, left, L, max_cyc);
        {
            Timed t(h, 1);
            const int drc = directions(sp);
            if (drc) return drc;
        }
        w.s.V = h->V.p; w.s.ncyc = sp.ncyc;
        for (int s = 0; s < sp.n && rc == MCMC_HIP_OK; ++s) {
            w.s.step0 = h->step;
            w.cyc = (int)(h->step / Lu - sp.c0);
            w.col = (int)(h->step % Lu);
            const int lrc = launch(pending ? 1 : 0, 1);
            if (lrc) return lrc;
            h->n_step_launches += 1;
            pending = false;
            rc = evaluate();
            if (rc == MCMC_HIP_OK) {
                pending = true;
                h->step += 1;
            }
        }
        left -= sp.n;
    }
    if (pending) {
        const int lrc = launch(1, 0);
        if (lrc) return lrc;
    }
    return rc;
}

// ------------------------------------------------------------------ binned Gaussian target
// chain of the chi2 sum that row tile R of NT joins (oracle: binned_class): its position in its
// group of eight tiles, the groups counted down from the last tile.  pl_fused_kernel gives the
// tile at a position to one wave per pair of walker tiles; pl_chi2_kernel (explicit points) gives
// wave q the tiles of class q.
inline int binned_shift(int NT) { return (8 - NT % 8) % 8; }
inline int binned_class(int R, int NT) { return (R + binned_shift(NT)) & 7; }

// the 32 partial sums of chi2 per walker of the residuals held in `delta` (n walkers, a multiple
// of 64) -> psum[32][n]; chi2 (may be null): their combination, one value per walker
int binned_chi2(mcmc_hip_ctx* h, const double* delta, double* psum, double* chi2, int n)
{
    auto& B = h->bg;
    mcmc::PlChi2Args c{};
    c.delta = delta; c.Astream = B.Astream.p; c.psum = psum;
    std::memcpy(c.tile_off, B.tile_off, sizeof c.tile_off);
    std::memcpy(c.nk, B.nk, sizeof c.nk);
    c.KT = B.KT; c.ntw = B.ntw; c.n_walkers = n; c.n_sets = n / 64;
    HIP_TRY(h, mcmc_hip_launch_pl_chi2(&c, h->stream));
    if (chi2) HIP_TRY(h, mcmc_hip_launch_pl_combine(psum, chi2, n, h->stream));
    return MCMC_HIP_OK;
}

int binned_residual(mcmc_hip_ctx* h, const double* trial, double* delta, int n)
{
    auto& B = h->bg;
    // MCMC_HIP_PL_SCALAR_RESIDUAL (developer switch): the lane-per-walker kernel of round 3
    static const bool scalar = getenv("MCMC_HIP_PL_SCALAR_RESIDUAL") != nullptr;
    if (!scalar) {
        mcmc::PlResidualMfmaArgs m{};
        m.trial = trial; m.theta0 = B.theta0.p; m.bjs = B.bjs.p; m.es = B.es.p; m.delta = delta;
        m.W = n; m.KT = B.KT; m.n_lin = B.n_lin; m.np = (B.n_lin + 7) / 8; m.calib = B.calib;
        m.n_tiles = (B.KT + 3) / 4;
        HIP_TRY(h, mcmc_hip_launch_pl_residual_mfma(&m, h->stream));
        return MCMC_HIP_OK;
    }
    mcmc::PlResidualArgs r{};
    r.trial = trial; r.theta0 = B.theta0.p; r.resp = B.resp.p; r.delta = delta;
    r.W = n; r.n_bins = B.n_bins; r.KT = B.KT; r.n_lin = B.n_lin; r.nlp = B.nlp; r.calib = B.calib;
    HIP_TRY(h, mcmc_hip_launch_pl_residual(&r, h->stream));
    return MCMC_HIP_OK;
}

}  // namespace

// Model.logposterior for n points on the binned target (mcmc_hip_evaluate)
int evaluate_binned_points(mcmc_hip_ctx* h, int n, const double* x, double* logprior, double* loglike)
{
    auto& B = h->bg;
    const size_t d = h->d, np = ((size_t)n + 63) & ~(size_t)63;
    std::vector<double> t(d * np);
    for (size_t w = 0; w < np; ++w)
        for (size_t i = 0; i < d; ++i) t[i * np + w] = x[(w < (size_t)n ? w : 0) * d + i];
    HIP_TRY(h, B.etrial.resize(d * np));
    HIP_TRY(h, B.elp.resize(np));
    HIP_TRY(h, B.echi2.resize(np));
    HIP_TRY(h, B.edelta.resize((np / 64) * (size_t)B.KT * 256 + (size_t)mcmc::kPlPad * 256));
    HIP_TRY(h, hipMemcpyAsync(B.etrial.p, t.data(), sizeof(double) * d * np, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, mcmc_hip_launch_pl_prior(B.etrial.p, (int)np, (int)d, h->cblock.p, h->norm_mask,
                                        h->uniform_logp, B.elp.p, h->stream));
    int rc = binned_residual(h, B.etrial.p, B.edelta.p, (int)np);
    if (rc) return rc;
    HIP_TRY(h, B.epsum.resize(32 * np));
    rc = binned_chi2(h, B.edelta.p, B.epsum.p, B.echi2.p, (int)np);
    if (rc) return rc;
    std::vector<double> c2(np), lp(np);
    HIP_TRY(h, hipMemcpyAsync(lp.data(), B.elp.p, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(c2.data(), B.echi2.p, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int w = 0; w < n; ++w) {
        logprior[w] = lp[w];
        // (the likelihood is skipped outside the prior support, model.py:650-653)
        loglike[w] = std::isinf(lp[w]) ? -INFINITY : -0.5 * c2[w];
    }
    return MCMC_HIP_OK;
}

// mcmc_hip_step on the binned target: per step  [accept of the previous trial +] proposal ->
// residuals -> chi2 on the matrix cores; a call ends with the accept of its last trial, so the
// state is complete between calls.
int step_binned(mcmc_hip_ctx* h, int n_steps)
{
    auto& B = h->bg;
    const int d = h->d, W = h->W;
    if (h->blocked || h->drag_last_slow >= 0 || h->own_basis || h->cfg.emit_capacity > 0 || h->any_periodic)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the binned Gaussian target serves one parameter block, the shared basis, "
                    "non-periodic priors and emit_capacity 0");
    HIP_TRY(h, B.trial.resize((size_t)d * W));
    HIP_TRY(h, B.lp_t.resize(W));
    HIP_TRY(h, B.Ea.resize(W));
    HIP_TRY(h, B.psum.resize((size_t)32 * W));
    // MCMC_HIP_PL_UNFUSED (developer switch): residuals and chi2 as two launches (round 3)
    static const bool unfused = getenv("MCMC_HIP_PL_UNFUSED") != nullptr;
    if (unfused)    // (fused: delta lives in LDS, 323 MB of HBM less at 65 536 walkers)
        HIP_TRY(h, B.delta.resize(((size_t)W / 64) * (size_t)B.KT * 256 + (size_t)mcmc::kPlPad * 256));
    const size_t dd = (size_t)mcmc::v_slab(d);
    mcmc::PlWalkerArgs a{};
    a.s = step_args(h);
    a.s.cps = d; a.s.slab = (int)dd;
    a.d = d; a.trial = B.trial.p; a.lp_t = B.lp_t.p; a.Ea = B.Ea.p; a.psum_t = B.psum.p;
    const int rc = trial_pipeline(
        h, n_steps, d, max_span_cycles(h, 64u << 20, dd, h->G), a,
        [&](const StepSpan& sp) {
            return shared_basis(h, h->V, h->G, h->cfg.walker_offset / (uint32_t)h->gs, sp.c0, sp.ncyc, dd, h->stream);
        },
        [&](int accept, int propose) -> int {
            Timed t(h, 3);
            HIP_TRY(h, mcmc_hip_launch_pl_walker(&a, accept, propose, h->stream));
            return MCMC_HIP_OK;
        },
        [&]() -> int {   // (no callback here: only a launch can fail, and the call returns at once)
            if (unfused) {
                {
                    Timed t(h, 4);
                    const int rrc = binned_residual(h, B.trial.p, B.delta.p, W);
                    if (rrc) return rrc;
                }
                Timed t(h, 5);
                return binned_chi2(h, B.delta.p, B.psum.p, nullptr, W);
            }
            Timed t(h, 5);
            mcmc::PlFusedArgs f{};
            f.trial = B.trial.p; f.theta0 = B.theta0.p; f.bjs = B.bjs.p; f.es = B.es.p;
            f.Astream = B.Afused.p; f.psum = B.psum.p;
            std::memcpy(f.a_off, B.f_off, sizeof f.a_off);
            std::memcpy(f.a_pairs, B.f_pairs, sizeof f.a_pairs);
            f.W = W; f.KT = B.KT; f.n_lin = B.n_lin; f.np = (B.n_lin + 7) / 8; f.calib = B.calib;
            f.n_tiles = (B.KT + 3) / 4; f.shift = B.f_shift; f.ng = B.f_ng; f.n_sets = W / 64;
            HIP_TRY(h, mcmc_hip_launch_pl_fused(&f, h->stream));
            return MCMC_HIP_OK;
        });
    if (rc) return rc;
    take_noted_kernel(h, "n_bins", B.n_bins);
    return MCMC_HIP_OK;
}

namespace {

// ------------------------------------------------------------------ function target
// what the engine was created with: checked by mcmc_hip_set_target_function and _functions
int function_target_refusals(mcmc_hip_ctx* h)
{
    if (h->d > kMaxDimBig)
        return fail(h, MCMC_HIP_ERR_ARG, "a function target serves d <= %d, got d=%d", kMaxDimBig, h->d);
    if (h->cfg.flags & MCMC_HIP_FLAG_INCREMENTAL)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "a function target is evaluated from scratch (incremental evaluation, "
                    "MCMC_HIP_FLAG_INCREMENTAL, is not served)");
    if (h->cfg.flags & MCMC_HIP_FLAG_OWN_BASIS)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "a function target needs the shared basis (own basis, MCMC_HIP_FLAG_OWN_BASIS / "
                    "shared_basis: False, is not served)");
    if (h->cfg.emit_capacity > 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "a function target emits no rows on the device (emit_capacity > 0 / emit: chains is "
                    "not served; use emit: snapshots)");
    return MCMC_HIP_OK;
}

// what may be set before or after the target: checked by mcmc_hip_set_target_function and again by
// every mcmc_hip_step
int function_refusals(mcmc_hip_ctx* h)
{
    if (h->blocked || h->drag_last_slow >= 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "a function target serves one parameter block with Metropolis steps (parameter "
                    "blocks, oversampling and dragging are not served)");
    if (h->any_periodic)
        return fail(h, MCMC_HIP_ERR_ARG, "a function target does not serve periodic parameters");
    return MCMC_HIP_OK;
}

}  // namespace

int function_call(mcmc_hip_ctx* h, int n, const double* points, double* loglike)
{
    const int rc = h->fnt.fn(h->fnt.user, n, h->d, points, loglike, (void*)h->stream);
    if (rc)
        return fail(h, MCMC_HIP_ERR_CALLBACK, "the callback of the function target returned %d", rc);
    return MCMC_HIP_OK;
}

// mcmc_hip_step on a function target: per step  [accept of the previous trial +] proposal ->
// the user's function on the trial points; a call ends with the accept of its last trial, so the
// state is complete between calls.  Nothing here waits for the device.
int step_function(mcmc_hip_ctx* h, int n_steps)
{
    auto& F = h->fnt;
    const int d = h->d, W = h->W;
    int rc = function_refusals(h);
    if (rc) return rc;
    HIP_TRY(h, F.points.resize((size_t)d * W));
    HIP_TRY(h, F.lp_t.resize(W));
    HIP_TRY(h, F.Ea.resize(W));
    HIP_TRY(h, F.ll_t.resize(W));
    const size_t dd = h->kb ? (size_t)mcmc::v_slab_big(d) : (size_t)mcmc::v_slab(d);
    mcmc::FnWalkerArgs a{};
    a.s = step_args(h);
    a.s.cps = d; a.s.slab = (int)dd;
    a.d = d; a.ld = h->kb ? mcmc::v_ld(d) : d;
    put_norm_mask4(h, a.norm_mask4);
    a.points = F.points.p; a.lp_t = F.lp_t.p; a.Ea = F.Ea.p; a.ll_t = F.ll_t.p; a.bad = F.bad.p;
    rc = trial_pipeline(
        h, n_steps, d, max_span_cycles(h, 64u << 20, dd, h->G), a,
        [&](const StepSpan& sp) {
            return shared_basis(h, h->V, h->G, h->cfg.walker_offset / (uint32_t)h->gs, sp.c0, sp.ncyc, dd, h->stream);
        },
        [&](int accept, int propose) -> int {
            Timed t(h, 0);
            HIP_TRY(h, mcmc_hip_launch_fn_walker(&a, accept, propose, h->stream));
            return MCMC_HIP_OK;
        },
        [&] { return function_call(h, W, F.points.p, F.ll_t.p); });
    take_noted_kernel(h);
    return rc;
}

namespace {

// ------------------------------------------------------------------ several functions over blocks
int functions_refusals(mcmc_hip_ctx* h)
{
    if (h->drag_last_slow >= 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "function targets are sampled with Metropolis steps (dragging is not served)");
    if (h->any_periodic)
        return fail(h, MCMC_HIP_ERR_ARG, "a function target does not serve periodic parameters");
    return MCMC_HIP_OK;
}

// the block of every slot of `cycle` in the schedule all groups share: the Fisher-Yates shuffle of
// basis_blocked_kernel (sequence 0) with GLOBAL group 0 in its counter
void shared_schedule(mcmc_hip_ctx* h, unsigned long long cycle, int L)
{
    auto& F = h->fnt;
    if (F.sched_cycle == cycle && F.sched_epoch == h->dir_epoch && (int)F.sched.size() == L) return;
    F.sched.clear();
    for (size_t b = 0; b < h->blk_size.size(); ++b)
        F.sched.insert(F.sched.end(), (size_t)h->blk_over[b] * h->blk_size[b], (short)b);
    const uint32_t k0 = (uint32_t)h->cfg.seed, k1 = (uint32_t)(h->cfg.seed >> 32);
    if (L > 2)
        for (int i = L - 1; i >= 1; --i) {
            const uint32_t w0 = philox_w0(k0, k1, 0u, 2u, (uint32_t)cycle, (uint32_t)i);
            const int j = (int)(((unsigned long long)w0 * (unsigned long long)(i + 1)) >> 32);
            std::swap(F.sched[i], F.sched[j]);
        }
    F.sched_cycle = cycle;
    F.sched_epoch = h->dir_epoch;
}

int functions_call_one(mcmc_hip_ctx* h, int c, int n, const double* points, double* loglike)
{
    auto& F = h->fnt;
    const int rc = F.fns[c](F.users[c], n, (int)F.inputs[c].size(), points, loglike, (void*)h->stream);
    if (rc)
        return fail(h, MCMC_HIP_ERR_CALLBACK, "the callback of function %d of the function target returned %d", c, rc);
    return MCMC_HIP_OK;
}

}  // namespace

int functions_evaluate(mcmc_hip_ctx* h, int n, const double* x, double* comps)
{
    auto& F = h->fnt;
    const size_t d = h->d;
    HIP_TRY(h, F.ell.resize(n));
    std::vector<double> in;
    for (int c = 0; c < F.n_fn; ++c) {
        const size_t dc = F.inputs[c].size();
        in.resize((size_t)n * dc);
        for (size_t w = 0; w < (size_t)n; ++w)
            for (size_t k = 0; k < dc; ++k) in[w * dc + k] = x[w * d + F.inputs[c][k]];
        HIP_TRY(h, F.epts.resize((size_t)n * dc));
        HIP_TRY(h, hipMemcpyAsync(F.epts.p, in.data(), sizeof(double) * n * dc, hipMemcpyHostToDevice, h->stream));
        const int rc = functions_call_one(h, c, n, F.epts.p, F.ell.p);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpyAsync(comps + (size_t)c * n, F.ell.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (`in` and the scratch are reused)
    }
    return MCMC_HIP_OK;
}

// mcmc_hip_step with several functions: per step  [accept of the previous trial +] proposal of the
// slot -> the DUE functions on their inputs; a call ends with the accept of its last trial.  Which
// functions are due is the host's knowledge (the shared schedule); nothing waits for the device.
int step_functions(mcmc_hip_ctx* h, int n_steps)
{
    auto& F = h->fnt;
    const int d = h->d, W = h->W, nf = F.n_fn;
    int rc = functions_refusals(h);
    if (rc) return rc;
    const bool blocked = h->blocked;
    const int L = block_slots(h, 0);
    // the fastest block each function reads: it is due at the slots of that block and of slower ones
    int last_block[mcmc::kFnMaxFunctions] = {};
    if (blocked) {
        std::vector<int> block_of(d, 0);
        int j = 0;
        for (size_t b = 0; b < h->blk_size.size(); ++b)
            for (int k = 0; k < h->blk_size[b]; ++k, ++j) block_of[h->i_of_j[j]] = (int)b;
        for (int c = 0; c < nf; ++c)
            for (int i : F.inputs[c]) last_block[c] = std::max(last_block[c], block_of[i]);
    }
    if (!F.llc_valid) {   // a state that came without its components: every function, on the state
        std::vector<double> x((size_t)W * d), comps((size_t)nf * W);
        rc = mcmc_hip_get_state(h, x.data(), nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
        rc = functions_evaluate(h, W, x.data(), comps.data());
        if (rc) return rc;
        HIP_TRY(h, F.ll_c.resize((size_t)nf * W));
        HIP_TRY(h, hipMemcpy(F.ll_c.p, comps.data(), sizeof(double) * nf * W, hipMemcpyHostToDevice));
        F.llc_valid = true;
    }
    HIP_TRY(h, F.points.resize((size_t)d * W));
    HIP_TRY(h, F.lp_t.resize(W));
    HIP_TRY(h, F.Ea.resize(W));
    HIP_TRY(h, F.ll_new.resize((size_t)nf * W));
    const size_t dd = blocked ? (size_t)mcmc::v_slab_cols(L, d)
                              : (h->kb ? (size_t)mcmc::v_slab_big(d) : (size_t)mcmc::v_slab(d));
    mcmc::FnBlockedArgs a{};
    a.w.s = step_args(h);
    a.w.s.cps = L; a.w.s.slab = (int)dd;
    a.w.d = d; a.w.ld = blocked ? d : (h->kb ? mcmc::v_ld(d) : d);
    put_norm_mask4(h, a.w.norm_mask4);
    a.w.points = F.points.p; a.w.lp_t = F.lp_t.p; a.w.Ea = F.Ea.p; a.w.ll_t = nullptr; a.w.bad = F.bad.p;
    a.n_fn = nf; a.inputs = F.dinputs.p; a.ll_c = F.ll_c.p;
    for (int c = 0, off = 0; c < nf; ++c) {
        const int dc = (int)F.inputs[c].size();
        HIP_TRY(h, F.pts[c].resize((size_t)dc * W));
        a.in_off[c] = off; a.n_in[c] = dc; a.pts[c] = F.pts[c].p;
        a.ll_new[c] = F.ll_new.p + (size_t)c * W;
        off += dc;
    }
    rc = trial_pipeline(
        h, n_steps, L, max_span_cycles(h, 64u << 20, dd, h->G), a.w,
        [&](const StepSpan& sp) {
            bool any_1d = false;
            return blocked ? blocked_basis(h, 0, sp.c0, sp.ncyc, L, dd, h->V, h->vflag, any_1d, nullptr, true)
                           : shared_basis(h, h->V, h->G, h->cfg.walker_offset / (uint32_t)h->gs, sp.c0, sp.ncyc,
                                          dd, h->stream);
        },
        [&](int accept, int propose) -> int {
            if (propose) {   // the functions due at the slot of this step
                a.due = (1u << nf) - 1u;
                a.oned = d == 1;
                if (blocked) {
                    // (the cycle index is kept modulo 2^32, as the direction kernels keep it)
                    shared_schedule(h, (h->step / (unsigned long long)L) & 0xFFFFFFFFull, L);
                    const int b = F.sched[a.w.col];
                    a.due = 0;
                    for (int c = 0; c < nf; ++c)
                        if (last_block[c] >= b) a.due |= 1u << c;
                    a.oned = h->blk_size[b] == 1;
                }
            }
            Timed t(h, 0);
            HIP_TRY(h, mcmc_hip_launch_fn_blocked_walker(&a, accept, propose, h->stream));
            return MCMC_HIP_OK;
        },
        [&] {
            int erc = MCMC_HIP_OK;
            for (int c = 0; c < nf && erc == MCMC_HIP_OK; ++c)
                if ((a.due >> c) & 1u) erc = functions_call_one(h, c, W, F.pts[c].p, F.ll_new.p + (size_t)c * W);
            if (erc == MCMC_HIP_OK) a.due_prev = a.due;
            return erc;
        });
    take_noted_kernel(h);
    return rc;
}

// the flag of a function target that returned NaN or +inf inside the support (1 + walker, 0: none)
int function_target_error(mcmc_hip_ctx* h, int bad)
{
    return fail(h, MCMC_HIP_ERR_TARGET,
                "the function target returned NaN or +inf inside the prior support (walker %d): a "
                "log-likelihood there must be finite or -inf", bad - 1);
}

extern "C" {

int mcmc_hip_set_target_function(mcmc_hip_ctx* h, mcmc_hip_loglike_fn fn, void* user)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!fn) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    int rc = function_target_refusals(h);
    if (rc == MCMC_HIP_OK) rc = function_refusals(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, h->fnt.bad.resize(1));
    HIP_TRY(h, hipMemsetAsync(h->fnt.bad.p, 0, sizeof(int), h->stream));
    h->fnt.fn = fn;
    h->fnt.user = user;
    h->fnt.on = true;
    h->fnt.n_fn = 0;
    h->K = 0;
    h->bg.on = false;
    h->mean.clear(); h->Linv.clear(); h->cnorm.clear(); h->weight.clear();
    h->have_target = true;
    ++h->dir_epoch;
    h->have_state = false;
    return upload_constants(h);
}

int mcmc_hip_set_target_functions(mcmc_hip_ctx* h, int32_t n, const mcmc_hip_loglike_fn* fns,
                                  void* const* users, const int32_t* n_inputs, const int32_t* inputs)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!fns || !n_inputs || !inputs) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    if (n < 1 || n > mcmc::kFnMaxFunctions)
        return fail(h, MCMC_HIP_ERR_ARG, "a function target takes 1..%d functions, got %d",
                    mcmc::kFnMaxFunctions, n);
    int rc = function_target_refusals(h);
    if (rc == MCMC_HIP_OK) rc = functions_refusals(h);
    if (rc) return rc;
    std::vector<char> fed(h->d, 0);
    std::vector<int> flat;
    for (int c = 0, off = 0; c < n; off += n_inputs[c], ++c) {
        if (!fns[c]) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
        if (n_inputs[c] < 1 || n_inputs[c] > h->d)
            return fail(h, MCMC_HIP_ERR_ARG, "function %d takes %d inputs: it must take 1..d = %d of the "
                        "sampled parameters", c, n_inputs[c], h->d);
        std::vector<char> mine(h->d, 0);
        for (int k = 0; k < n_inputs[c]; ++k) {
            const int i = inputs[off + k];
            if (i < 0 || i >= h->d || mine[i])
                return fail(h, MCMC_HIP_ERR_ARG, "input %d of function %d is %d: not a sampled parameter "
                            "(0..%d), or listed twice", k, c, i, h->d - 1);
            mine[i] = fed[i] = 1;
            flat.push_back(i);
        }
    }
    for (int i = 0; i < h->d; ++i)
        if (!fed[i])
            return fail(h, MCMC_HIP_ERR_ARG, "sampled parameter %d feeds no function: every sampled "
                        "parameter must be an input of at least one", i);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& F = h->fnt;
    HIP_TRY(h, F.bad.resize(1));
    HIP_TRY(h, hipMemsetAsync(F.bad.p, 0, sizeof(int), h->stream));
    HIP_TRY(h, F.dinputs.resize(flat.size()));
    HIP_TRY(h, hipMemcpy(F.dinputs.p, flat.data(), sizeof(int) * flat.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, F.ll_c.resize((size_t)n * h->W));
    for (int c = 0, off = 0; c < n; off += n_inputs[c], ++c) {
        F.fns[c] = fns[c];
        F.users[c] = users ? users[c] : nullptr;
        F.inputs[c].assign(inputs + off, inputs + off + n_inputs[c]);
    }
    F.n_fn = n;
    F.fn = nullptr; F.user = nullptr;
    F.llc_valid = false;
    F.last_eval_n = 0;
    F.on = true;
    h->K = 0;
    h->bg.on = false;
    h->mean.clear(); h->Linv.clear(); h->cnorm.clear(); h->weight.clear();
    h->have_target = true;
    ++h->dir_epoch;
    h->have_state = false;
    return upload_constants(h);
}

int mcmc_hip_get_component_loglikes(mcmc_hip_ctx* h, double* ll)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!ll) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    auto& F = h->fnt;
    if (!F.on || F.n_fn < 1 || !h->have_state)
        return fail(h, MCMC_HIP_ERR_STATE, "no component log-likelihoods: set_target_functions and a state first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!F.llc_valid) {   // a full state set without them: what the next launch would form
        std::vector<double> x((size_t)h->W * h->d);
        int rc = mcmc_hip_get_state(h, x.data(), nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
        rc = functions_evaluate(h, h->W, x.data(), ll);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpy(F.ll_c.p, ll, sizeof(double) * F.n_fn * h->W, hipMemcpyHostToDevice));
        F.llc_valid = true;
        return MCMC_HIP_OK;
    }
    HIP_TRY(h, hipMemcpy(ll, F.ll_c.p, sizeof(double) * F.n_fn * h->W, hipMemcpyDeviceToHost));
    return MCMC_HIP_OK;
}

int mcmc_hip_set_component_loglikes(mcmc_hip_ctx* h, const double* ll)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!ll) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    auto& F = h->fnt;
    if (!F.on || F.n_fn < 1 || !h->have_state)
        return fail(h, MCMC_HIP_ERR_STATE, "set_target_functions and a state must precede set_component_loglikes");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(F.ll_c.p, ll, sizeof(double) * F.n_fn * h->W, hipMemcpyHostToDevice));
    F.llc_valid = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_set_target_binned_gaussian(mcmc_hip_ctx* h, int32_t n_bins, const int32_t* bins,
                                        int32_t lmax, const double* weights, const double* X,
                                        const double* cov, int32_t n_lin, const double* theta0,
                                        const double* D0, const double* J, int32_t calib_index)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (h->huge)
        return fail(h, MCMC_HIP_ERR_ARG, "d=%d > %d: the binned Gaussian target is not served", h->d, kMaxDimBig);
    if (!bins || !weights || !X || !cov || !theta0 || !D0 || !J)
        return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    const int d = h->d;
    if (!h->k || n_lin != d - 1 || n_lin < 1 || calib_index < 0 || calib_index >= d)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the binned Gaussian target takes d - 1 = %d emulator parameters and one "
                    "calibration parameter among 2 <= d <= 32 sampled ones (n_lin=%d, calib=%d)",
                    d - 1, n_lin, calib_index);
    if (n_bins < 1 || n_bins > 640 || lmax < 1)
        return fail(h, MCMC_HIP_ERR_ARG, "n_bins must be in 1..640 (got %d) and lmax >= 1", n_bins);
    if (h->incremental || h->own_basis || h->cfg.emit_capacity > 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the binned Gaussian target is evaluated from scratch with the shared basis "
                    "and emit_capacity 0 (it is not Gaussian in the calibration parameter)");
    for (int b = 0; b < n_bins; ++b) {
        const int tp = bins[3 * b], l0 = bins[3 * b + 1], l1 = bins[3 * b + 2];
        if (tp < 0 || tp > 2 || l0 < 0 || l1 < l0 || l1 > lmax)
            return fail(h, MCMC_HIP_ERR_ARG, "bin %d = (%d, %d, %d) is not inside 0..%d", b, tp, l0, l1, lmax);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& B = h->bg;
    const size_t n = n_bins, L1 = (size_t)lmax + 1;
    // cov = L L^T; chi2 = |L^-1 delta|^2 (the quadratic form of functions.py:64-78)
    std::vector<double> L(n * n);
    B.Linv.assign(n * n, 0.0);
    if (!is_symmetric(n_bins, cov) || !cholesky_lower(n_bins, cov, L.data()))
        return fail(h, MCMC_HIP_ERR_NOT_PD,
                    "the covariance of the binned data is not a symmetric positive-definite matrix");
    tri_inverse_lower(n_bins, L.data(), B.Linv.data());
    // binned response of the linear emulator (oracle: orc_binned_collapse)
    B.Bc0.assign(n, 0.0);
    B.BJ.assign(n * (size_t)n_lin, 0.0);
    for (size_t b = 0; b < n; ++b) {
        const size_t tp = bins[3 * b], l0 = bins[3 * b + 1], l1 = bins[3 * b + 2];
        double acc = 0.0;
        for (size_t l = l0; l <= l1; ++l) acc = std::fma(D0[tp * L1 + l], weights[l], acc);
        B.Bc0[b] = acc;
        for (int p = 0; p < n_lin; ++p) {
            double a = 0.0;
            for (size_t l = l0; l <= l1; ++l) a = std::fma(J[(tp * L1 + l) * n_lin + p], weights[l], a);
            B.BJ[b * n_lin + p] = a;
        }
    }
    B.n_bins = n_bins; B.lmax = lmax; B.n_lin = n_lin; B.calib = calib_index;
    B.nlp = (n_lin + 3) & ~3;
    // k-steps of four bins, an EVEN number of them: pl_chi2_kernel fetches the operands of two
    // k-steps with one 16-byte load (a padding k-step is zeros: exact no-ops at the end of a chain)
    B.KT = (((n_bins + 3) / 4) + 1) & ~1;
    B.bins.assign(bins, bins + 3 * n);
    const int NT = (n_bins + 15) / 16;
    B.ntw = (NT + 7) / 8;
    // records (Bc0_b, BJ_b0 .. BJ_b,nlp-1, X_b) and the padded fiducial point
    std::vector<double> resp(n * (size_t)(B.nlp + 2), 0.0), th((size_t)B.nlp, 0.0);
    for (size_t b = 0; b < n; ++b) {
        double* r = resp.data() + b * (size_t)(B.nlp + 2);
        r[0] = B.Bc0[b];
        for (int p = 0; p < n_lin; ++p) r[1 + p] = B.BJ[b * n_lin + p];
        r[1 + B.nlp] = X[b];
    }
    th.resize(32, 0.0);    // (pl_residual_mfma_kernel reads 8 np <= 32 entries)
    std::copy(theta0, theta0 + n_lin, th.begin());
    // the same response as matrix-core operands (PlResidualMfmaArgs)
    const int n_tiles = (B.KT + 3) / 4, npairs = (n_lin + 7) / 8;
    std::vector<double> bjs((size_t)n_tiles * npairs * 128, 0.0), es((size_t)n_tiles * 4 * 128, 0.0);
    for (int T = 0; T < n_tiles; ++T) {
        for (int jp = 0; jp < npairs; ++jp)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 2; ++e) {
                    const size_t b = 16 * (size_t)T + (l & 15);
                    const int p = 4 * (2 * jp + e) + (l >> 4);
                    if (b < n && p < n_lin)
                        bjs[(((size_t)T * npairs + jp) * 64 + l) * 2 + e] = B.BJ[b * n_lin + p];
                }
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
                const size_t b = 16 * (size_t)T + 4 * r + (l >> 4);
                if (b >= n) continue;
                es[(((size_t)T * 4 + r / 2) * 64 + l) * 2 + (r & 1)] = B.Bc0[b];
                es[(((size_t)T * 4 + 2 + r / 2) * 64 + l) * 2 + (r & 1)] = X[b];
            }
    }
    HIP_TRY(h, B.bjs.resize(bjs.size()));
    HIP_TRY(h, B.es.resize(es.size()));
    HIP_TRY(h, hipMemcpy(B.bjs.p, bjs.data(), sizeof(double) * bjs.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.es.p, es.data(), sizeof(double) * es.size(), hipMemcpyHostToDevice));
    // tiles of L^-1 per wave of pl_chi2_kernel: wave q owns the 16-row tiles of class q in
    // ascending order, absent tiles first; tile R has min(4 R + 4, KT) k-steps
    std::vector<double> As;
    for (int q = 0; q < 8; ++q) {
        std::vector<int> mine;
        for (int R = 0; R < NT; ++R)
            if (binned_class(R, NT) == q) mine.push_back(R);
        const int absent = B.ntw - (int)mine.size();
        for (int t = 0; t < 5; ++t) { B.nk[q][t] = 0; B.tile_off[q][t] = 0; }
        for (int t = 0; t < (int)mine.size(); ++t) {
            const int R = mine[t], nk = std::min(4 * R + 4, B.KT);   // (even)
            B.nk[q][absent + t] = nk;
            B.tile_off[q][absent + t] = As.size();
            // (A-operand lane order, the k-steps 2 m and 2 m + 1 of a lane side by side)
            for (int kk2 = 0; kk2 < nk / 2; ++kk2)
                for (int l = 0; l < 64; ++l)
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const size_t j = 16 * (size_t)R + (l & 15), i = 4 * (size_t)(2 * kk2 + h2) + (l >> 4);
                        As.push_back((j < n && i <= j) ? B.Linv[j * n + i] : 0.0);
                    }
        }
    }
    As.resize(As.size() + (size_t)mcmc::kPlPad * 64, 0.0);   // (operands are fetched ahead)
    // pl_fused_kernel: per wave q and group G of eight virtual tiles (virtual = real + shift) the
    // tile at position s = min(q, 7 - q) (half 0) and at 7 - s (half 1), each as a stream of its
    // k-step pairs from pair 0, in A-operand lane order; absent tiles point at a block of zeros
    {
        const int sh = binned_shift(NT), NG = (NT + sh) / 8;
        B.f_shift = sh; B.f_ng = NG;
        std::vector<double> Af(128, 0.0);       // [0, 128): the zero block
        for (int q = 0; q < 8; ++q) {
            const int s_pos = q < 4 ? q : 7 - q;
            for (int G = 0; G < 5; ++G)
                for (int hf = 0; hf < 2; ++hf) {
                    B.f_off[q][G][hf] = 0; B.f_pairs[q][G][hf] = 0;
                    const int R = 8 * G + (hf ? 7 - s_pos : s_pos) - sh;
                    if (G >= NG || R < 0 || R >= NT) continue;
                    const int np2 = std::min(2 * R + 2, B.KT / 2);
                    B.f_off[q][G][hf] = Af.size();
                    B.f_pairs[q][G][hf] = np2 + 2 * sh;
                    for (int P = 0; P < np2; ++P)
                        for (int l = 0; l < 64; ++l)
                            for (int e = 0; e < 2; ++e) {
                                const size_t j = 16 * (size_t)R + (l & 15), i = 4 * (size_t)(2 * P + e) + (l >> 4);
                                Af.push_back((j < n && i <= j) ? B.Linv[j * n + i] : 0.0);
                            }
                }
        }
        Af.resize(Af.size() + 256, 0.0);
        HIP_TRY(h, B.Afused.resize(Af.size()));
        HIP_TRY(h, hipMemcpy(B.Afused.p, Af.data(), sizeof(double) * Af.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(h, B.resp.resize(resp.size()));
    HIP_TRY(h, B.theta0.resize(th.size()));
    HIP_TRY(h, B.Astream.resize(As.size()));
    HIP_TRY(h, B.weights.resize(L1));
    HIP_TRY(h, B.X.resize(n));
    HIP_TRY(h, B.dbins.resize(3 * n));
    HIP_TRY(h, hipMemcpy(B.resp.p, resp.data(), sizeof(double) * resp.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.theta0.p, th.data(), sizeof(double) * th.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.Astream.p, As.data(), sizeof(double) * As.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.weights.p, weights, sizeof(double) * L1, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.X.p, X, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(B.dbins.p, bins, sizeof(int32_t) * 3 * n, hipMemcpyHostToDevice));
    B.on = true;
    h->fnt.on = false;
    h->K = 0;
    h->mean.clear(); h->Linv.clear(); h->cnorm.clear(); h->weight.clear();
    h->have_target = true;
    ++h->dir_epoch;
    h->have_state = false;
    return upload_constants(h);
}

int mcmc_hip_get_binned_constants(const mcmc_hip_ctx* h, double* Linv, double* Bc0, double* BJ)
{
    if (!h || !h->bg.on) return MCMC_HIP_ERR_STATE;
    const auto& B = h->bg;
    if (Linv) std::copy(B.Linv.begin(), B.Linv.end(), Linv);
    if (Bc0) std::copy(B.Bc0.begin(), B.Bc0.end(), Bc0);
    if (BJ) std::copy(B.BJ.begin(), B.BJ.end(), BJ);
    return MCMC_HIP_OK;
}

int mcmc_hip_evaluate_binned(mcmc_hip_ctx* h, int32_t n_pts, int32_t L0, int32_t n_ell,
                             const double* cl, const double* A, double* chi2)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->bg.on) return fail(h, MCMC_HIP_ERR_STATE, "set_target_binned_gaussian must precede evaluate_binned");
    auto& B = h->bg;
    if (n_pts <= 0 || !cl || !A || !chi2 || L0 < 0 || n_ell <= 0)
        return fail(h, MCMC_HIP_ERR_ARG, "bad argument");
    for (int b = 0; b < B.n_bins; ++b)
        if (B.bins[3 * b + 1] < L0 || B.bins[3 * b + 2] - L0 >= n_ell)
            return fail(h, MCMC_HIP_ERR_ARG, "bin %d (l = %d..%d) is outside the spectra given (l = %d..%d)",
                        b, B.bins[3 * b + 1], B.bins[3 * b + 2], L0, L0 + n_ell - 1);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t np = ((size_t)n_pts + 63) & ~(size_t)63;
    HIP_TRY(h, B.ecl.resize((size_t)n_pts * 3 * n_ell));
    HIP_TRY(h, B.eA.resize(n_pts));
    HIP_TRY(h, B.echi2.resize(np));
    HIP_TRY(h, B.edelta.resize((np / 64) * (size_t)B.KT * 256 + (size_t)mcmc::kPlPad * 256));
    HIP_TRY(h, hipMemcpyAsync(B.ecl.p, cl, sizeof(double) * (size_t)n_pts * 3 * n_ell,
                              hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(B.eA.p, A, sizeof(double) * n_pts, hipMemcpyHostToDevice, h->stream));
    mcmc::PlBinArgs b{};
    b.cl = B.ecl.p; b.A = B.eA.p; b.bins = B.dbins.p; b.weights = B.weights.p; b.X = B.X.p;
    b.delta = B.edelta.p; b.n_pts = n_pts; b.n_bins = B.n_bins; b.KT = B.KT; b.L0 = L0; b.stride = n_ell;
    HIP_TRY(h, mcmc_hip_launch_pl_bin(&b, h->stream));
    HIP_TRY(h, B.epsum.resize(32 * np));
    const int rc = binned_chi2(h, B.edelta.p, B.epsum.p, B.echi2.p, (int)np);
    if (rc) return rc;
    std::vector<double> c2(np);
    HIP_TRY(h, hipMemcpyAsync(c2.data(), B.echi2.p, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::copy(c2.begin(), c2.begin() + n_pts, chi2);
    take_noted_kernel(nullptr);
    return MCMC_HIP_OK;
}

}  // extern "C"
