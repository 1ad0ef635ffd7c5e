// libmcmc_hip.so: the stretch move on the single-function target (stretch_kernels.hip; DESIGN.md
// section 2, "Stretch move") -- its option, its refusals and its stepper.
#include "ctx.h"

namespace {

// what the stretch move does not serve, each by name; checked by every mcmc_hip_step, since target,
// blocking and state may be set in any order (the scale a is checked where it arrives: mcmc_hip_set_move)
int stretch_refusals(mcmc_hip_ctx* h)
{
    const int d = h->d;
    if (h->cfg.flags & MCMC_HIP_FLAG_INCREMENTAL)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the stretch move evaluates from scratch (incremental evaluation, "
                    "MCMC_HIP_FLAG_INCREMENTAL, is not served)");
    if (h->cfg.emit_capacity > 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the stretch move emits no rows on the device (emit_capacity > 0 / emit: chains is "
                    "not served; use emit: snapshots)");
    if (!h->fnt.on || h->fnt.n_fn > 0 || !h->fnt.fn)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the stretch move serves one device_function target (mcmc_hip_set_target_function); "
                    "analytic targets and the several-functions target are not served");
    if (h->blocked || h->drag_last_slow >= 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the stretch move moves all parameters at once (parameter blocks, oversampling and "
                    "dragging are not served)");
    if (h->any_periodic)
        return fail(h, MCMC_HIP_ERR_ARG, "the stretch move does not serve periodic parameters");
    if (d > kMaxDimBig) return fail(h, MCMC_HIP_ERR_ARG, "the stretch move serves d <= %d, got d=%d", kMaxDimBig, d);
    if (h->gs < 4 * d)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the stretch move needs group_size >= 4 d (a half-group of %d walkers spans too little "
                    "of d=%d dimensions): use a larger group_size (256 serves d <= 64)", h->gs / 2, d);
    return MCMC_HIP_OK;
}

// a parameter with the same value in every walker of a half-group: the trials of the other half
// stay on lines through those points, and the move never leaves the hyperplane
int stretch_check_state(mcmc_hip_ctx* h)
{
    const size_t W = h->W, d = h->d, hg = (size_t)h->gs / 2;
    std::vector<double> x(W * d);
    HIP_TRY(h, hipMemcpyAsync(x.data(), h->x.p, sizeof(double) * W * d, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < d; ++i)
        for (size_t w0 = 0; w0 < W; w0 += hg) {
            const double* xi = x.data() + i * W + w0;
            bool flat = true;
            for (size_t m = 1; m < hg && flat; ++m) flat = xi[m] == xi[0];
            if (flat)
                return fail(h, MCMC_HIP_ERR_ARG,
                            "the stretch move cannot start here: parameter %zu has the same value (%g) in every "
                            "walker of the half-group at walker %zu, and the move never leaves that hyperplane "
                            "(a fixed `ref` point does this: give `ref` as a pdf)",
                            i, xi[0], (size_t)h->cfg.walker_offset + w0);
        }
    h->mv.checked = true;
    return MCMC_HIP_OK;
}

}  // namespace

// mcmc_hip_step with the stretch move: per step two half-updates, each  [accept of the previous
// half's trial +] proposal of this half -> the user's function on the W / 2 trial rows; a call
// ends with the accept of its last trial, so the state is complete between calls.  Nothing here
// waits for the device.
int step_stretch(mcmc_hip_ctx* h, int n_steps)
{
    auto& F = h->fnt;
    int rc = stretch_refusals(h);
    if (rc) return rc;
    if (h->mv.broken)
        return fail(h, MCMC_HIP_ERR_STATE,
                    "a callback failed between the two half-updates of a stretch step: set a state again "
                    "(mcmc_hip_set_state / mcmc_hip_set_full_state) before the next step");
    if (!h->mv.checked && (rc = stretch_check_state(h)) != MCMC_HIP_OK) return rc;
    const int d = h->d, W = h->W, n_act = W / 2;
    HIP_TRY(h, F.points.resize((size_t)d * n_act));
    HIP_TRY(h, F.lp_t.resize(n_act));
    HIP_TRY(h, F.Ea.resize(n_act));
    HIP_TRY(h, F.ll_t.resize(n_act));
    HIP_TRY(h, h->mv.q.resize(n_act));
    mcmc::StretchArgs a{};
    a.s.x = h->x.p; a.s.logpost = h->logpost.p; a.s.logprior = h->logprior.p;
    a.s.loglike = h->loglike.p; a.s.weight = h->weight_i.p; a.s.prior_rej = h->prej.p;
    a.s.burn_left = h->burn.p; a.s.n_accept = h->nacc.p; a.s.stuck = h->stuck.p;
    a.s.accept_total = h->acc_total.p;
    a.s.cblock = h->cblock.p; a.s.W = W; a.s.group_size = h->gs; a.s.n_modes = 0;
    a.s.norm_mask = h->norm_mask; a.s.walker0 = h->cfg.walker_offset;
    a.s.key0 = (uint32_t)h->cfg.seed; a.s.key1 = (uint32_t)(h->cfg.seed >> 32);
    a.s.uniform_logp = h->uniform_logp; a.s.temperature = h->cfg.temperature;
    a.s.max_tries = h->cfg.max_tries;
    a.d = d; a.a = h->mv.a; a.dm1 = (double)(d - 1);
    a.log2_half = h->gs == 64 ? 5 : (h->gs == 128 ? 6 : 7);
    for (int q = 0; q < 4; ++q) a.norm_mask4[q] = h->norm_mask4[q];
    a.points = F.points.p; a.lp_t = F.lp_t.p; a.Ea = F.Ea.p; a.q = h->mv.q.p; a.ll_t = F.ll_t.p;
    a.bad = F.bad.p;
    int pending = -1;   // the half whose trial has been proposed and evaluated, not yet accepted / rejected
    for (int s = 0; s < n_steps && rc == MCMC_HIP_OK; ++s)
        for (int half = 0; half < 2; ++half) {
            a.s.step0 = h->step;
            a.half_accept = pending < 0 ? 0 : pending;
            a.half_propose = half;
            {
                Timed t(h, 0);
                HIP_TRY(h, mcmc_hip_launch_stretch(&a, pending >= 0 ? 1 : 0, 1, h->stream));
            }
            h->n_step_launches += 1;
            // (the launch has settled the previous trial; a callback that fails drops THIS one: the
            // step counter stays that of the last completed step, half 0 of this one may be committed)
            pending = -1;
            rc = function_call(h, n_act, F.points.p, F.ll_t.p);
            if (rc) {
                h->mv.broken = true;
                break;
            }
            pending = half;
            if (half == 1) h->step += 1;
        }
    if (pending >= 0) {
        a.half_accept = pending;
        Timed t(h, 0);
        HIP_TRY(h, mcmc_hip_launch_stretch(&a, 1, 0, h->stream));
    }
    take_noted_kernel(h);
    return rc;
}

extern "C" {

int mcmc_hip_set_move(mcmc_hip_ctx* h, int32_t kind, double a)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (kind != MCMC_HIP_MOVE_METROPOLIS && kind != MCMC_HIP_MOVE_STRETCH)
        return fail(h, MCMC_HIP_ERR_ARG, "move must be MCMC_HIP_MOVE_METROPOLIS (0) or MCMC_HIP_MOVE_STRETCH (1), got %d", kind);
    if (kind == MCMC_HIP_MOVE_STRETCH && !(std::isfinite(a) && a > 1.0))
        return fail(h, MCMC_HIP_ERR_ARG, "the stretch move needs a finite stretch_a > 1, got %g", a);
    h->mv.kind = kind;
    if (kind == MCMC_HIP_MOVE_STRETCH) h->mv.a = a;
    h->mv.checked = false;
    return MCMC_HIP_OK;
}

}  // extern "C"
