// libmcmc_hip.so: the half-ensemble moves on the single-function target -- the stretch move
// (stretch_kernels.hip; DESIGN.md section 2, "Stretch move") and the weighted mixtures of stretch,
// differential-evolution and snooker moves (ensemble_move_kernels.hip; "Ensemble move mixtures") --:
// their options, their refusals and their stepper.
#include "ctx.h"

namespace {

// the subject of a refusal: the move in force
const char* who(const mcmc_hip_ctx* h) { return h->mx.n > 0 ? "a mixture of ensemble moves" : "the stretch move"; }

// what the stretch move -- and a mixture, whose limits are the same -- does not serve, each by name;
// checked by every mcmc_hip_step, since target, blocking and state may be set in any order (the
// parameters are checked where they arrive: mcmc_hip_set_move, mcmc_hip_set_moves)
int stretch_refusals(mcmc_hip_ctx* h)
{
    const int d = h->d;
    const char* const me = who(h);
    if (h->cfg.flags & MCMC_HIP_FLAG_INCREMENTAL)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "%s evaluates from scratch (incremental evaluation, "
                    "MCMC_HIP_FLAG_INCREMENTAL, is not served)", me);
    if (h->cfg.emit_capacity > 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "%s emits no rows on the device (emit_capacity > 0 / emit: chains is "
                    "not served; use emit: snapshots)", me);
    if (!h->fnt.on || h->fnt.n_fn > 0 || !h->fnt.fn)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "%s serves one device_function target (mcmc_hip_set_target_function); "
                    "analytic targets and the several-functions target are not served", me);
    if (h->blocked || h->drag_last_slow >= 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "%s moves all parameters at once (parameter blocks, oversampling and "
                    "dragging are not served)", me);
    if (h->any_periodic)
        return fail(h, MCMC_HIP_ERR_ARG, "%s does not serve periodic parameters", me);
    if (d > kMaxDimBig) return fail(h, MCMC_HIP_ERR_ARG, "%s serves d <= %d, got d=%d", me, kMaxDimBig, d);
    if (h->gs < 4 * d)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "%s needs group_size >= 4 d (a half-group of %d walkers spans too little "
                    "of d=%d dimensions): use a larger group_size (256 serves d <= 64)", me, h->gs / 2, d);
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
                            "%s cannot start here: parameter %zu has the same value (%g) in every "
                            "walker of the half-group at walker %zu, and the move never leaves that hyperplane "
                            "(a fixed `ref` point does this: give `ref` as a pdf)",
                            who(h), i, xi[0], (size_t)h->cfg.walker_offset + w0);
        }
    h->mv.checked = true;
    return MCMC_HIP_OK;
}

static_assert(MCMC_HIP_ENSEMBLE_STRETCH == mcmc::kEnsembleStretch && MCMC_HIP_ENSEMBLE_DE == mcmc::kEnsembleDE &&
                  MCMC_HIP_ENSEMBLE_SNOOKER == mcmc::kEnsembleSnooker, "the kinds of mcmc_hip.h are the kernel's");

// the member of the mixture that step `step` makes: one Philox block whose counter holds no walker
// or group -- (0, kStreamMoveKind, S_lo, S_hi) --, word 0 by inverse CDF over the normalised weights.
// Every rank, shard and walker forms the same; a one-member mixture draws nothing
int mixture_member(const mcmc_hip_ctx* h, unsigned long long step)
{
    const auto& M = h->mx;
    if (M.n == 1) return 0;
    const uint32_t w0 = philox_w0((uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), 0u, mcmc::kStreamMoveKind,
                                  (uint32_t)step, (uint32_t)(step >> 32));
    int j = 0;
    while (j < M.n - 1 && (unsigned long long)w0 >= M.below[j]) ++j;
    return j;
}

}  // namespace

// mcmc_hip_step with the stretch move, or with a mixture of ensemble moves (h->mx.n > 0: the kind of
// a step is mixture_member's, the kernel ensemble_move_kernel): per step two half-updates, each
// [accept of the previous half's trial +] proposal of this half -> the user's function on the W / 2
// trial rows; a call ends with the accept of its last trial, so the state is complete between
// calls.  Nothing here waits for the device.
int step_stretch(mcmc_hip_ctx* h, int n_steps)
{
    auto& F = h->fnt;
    int rc = stretch_refusals(h);
    if (rc) return rc;
    if (h->mv.broken)
        return fail(h, MCMC_HIP_ERR_STATE,
                    "a callback failed between the two half-updates of %s: set a state again "
                    "(mcmc_hip_set_state / mcmc_hip_set_full_state) before the next step",
                    h->mx.n > 0 ? "an ensemble-move step" : "a stretch step");
    if (!h->mv.checked && (rc = stretch_check_state(h)) != MCMC_HIP_OK) return rc;
    const int d = h->d, W = h->W, n_act = W / 2;
    const auto& M = h->mx;
    const bool mixture = M.n > 0;
    // (the snooker update draws three distinct members of a half-group; group_size >= 64 gives it 32)
    if (mixture && h->gs / 2 < 3)
        return fail(h, MCMC_HIP_ERR_ARG, "a mixture of ensemble moves needs a half-group of at least 3 walkers, got %d", h->gs / 2);
    HIP_TRY(h, F.points.resize((size_t)d * n_act));
    HIP_TRY(h, F.lp_t.resize(n_act));
    HIP_TRY(h, F.Ea.resize(n_act));
    HIP_TRY(h, F.ll_t.resize(n_act));
    HIP_TRY(h, h->mv.q.resize(n_act));
    mcmc::EnsembleMoveArgs ma{};
    mcmc::StretchArgs& a = ma.st;
    a.s = step_args(h);
    a.d = d; a.a = h->mv.a; a.dm1 = (double)(d - 1);
    a.log2_half = h->gs == 64 ? 5 : (h->gs == 128 ? 6 : 7);
    put_norm_mask4(h, a.norm_mask4);
    a.points = F.points.p; a.lp_t = F.lp_t.p; a.Ea = F.Ea.p; a.q = h->mv.q.p; a.ll_t = F.ll_t.p;
    a.bad = F.bad.p;
    // one launch: [accept of the pending half +] the proposal (propose: 0 for the last accept of a call)
    auto launch = [&](int accept, int propose) {
        return mixture ? mcmc_hip_launch_ensemble_move(&ma, accept, propose ? ma.kind : -1, h->stream)
                       : mcmc_hip_launch_stretch(&a, accept, propose, h->stream);
    };
    int pending = -1;   // the half whose trial has been proposed and evaluated, not yet accepted / rejected
    for (int s = 0; s < n_steps && rc == MCMC_HIP_OK; ++s) {
        if (mixture) {   // both halves of a step make the same kind of move
            const int j = mixture_member(h, h->step);
            ma.kind = M.kind[j]; ma.p0 = M.p0[j]; ma.p1 = M.p1[j];
        }
        for (int half = 0; half < 2; ++half) {
            a.s.step0 = h->step;
            a.half_accept = pending < 0 ? 0 : pending;
            a.half_propose = half;
            {
                Timed t(h, 0);
                HIP_TRY(h, launch(pending >= 0 ? 1 : 0, 1));
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
    }
    if (pending >= 0) {
        a.half_accept = pending;
        Timed t(h, 0);
        HIP_TRY(h, launch(1, 0));
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

int mcmc_hip_set_moves(mcmc_hip_ctx* h, int32_t n, const int32_t* kinds, const double* weights,
                       const double* p0, const double* p1)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n < 0 || n > mcmc::kMaxEnsembleMoves)
        return fail(h, MCMC_HIP_ERR_ARG, "a mixture of ensemble moves has 1 .. %d members (0: off), got n=%d",
                    mcmc::kMaxEnsembleMoves, n);
    if (n > 0 && (!kinds || !weights || !p0 || !p1))
        return fail(h, MCMC_HIP_ERR_ARG, "mcmc_hip_set_moves: kinds, weights, p0 and p1 must be given for n > 0");
    double total = 0.0;
    for (int j = 0; j < n; ++j) {
        if (!(std::isfinite(weights[j]) && weights[j] > 0.0))
            return fail(h, MCMC_HIP_ERR_ARG, "member %d of the mixture: the weight must be positive and finite, got %g",
                        j, weights[j]);
        switch (kinds[j]) {
        case MCMC_HIP_ENSEMBLE_STRETCH:
            if (!(std::isfinite(p0[j]) && p0[j] > 1.0))
                return fail(h, MCMC_HIP_ERR_ARG, "member %d of the mixture (stretch): needs a finite a > 1, got %g", j, p0[j]);
            break;
        case MCMC_HIP_ENSEMBLE_DE:
            if (!(std::isfinite(p0[j]) && p0[j] > 0.0))
                return fail(h, MCMC_HIP_ERR_ARG, "member %d of the mixture (de): needs a finite gamma > 0, got %g", j, p0[j]);
            if (!(std::isfinite(p1[j]) && p1[j] >= 0.0))
                return fail(h, MCMC_HIP_ERR_ARG, "member %d of the mixture (de): needs a finite sigma >= 0, got %g", j, p1[j]);
            break;
        case MCMC_HIP_ENSEMBLE_SNOOKER:
            if (!(std::isfinite(p0[j]) && p0[j] > 0.0))
                return fail(h, MCMC_HIP_ERR_ARG, "member %d of the mixture (snooker): needs a finite gamma > 0, got %g", j, p0[j]);
            break;
        default:
            return fail(h, MCMC_HIP_ERR_ARG,
                        "member %d of the mixture: the kind must be MCMC_HIP_ENSEMBLE_STRETCH (0), _DE (1) or "
                        "_SNOOKER (2), got %d", j, kinds[j]);
        }
        total += weights[j];
    }
    if (n > 0 && !std::isfinite(total))
        return fail(h, MCMC_HIP_ERR_ARG, "the weights of the mixture must have a finite sum, got %g", total);
    auto& M = h->mx;
    M.n = n;
    double cum = 0.0;
    for (int j = 0; j < n; ++j) {
        M.kind[j] = kinds[j];
        M.weight[j] = weights[j] / total;
        M.p0[j] = p0[j];
        M.p1[j] = kinds[j] == MCMC_HIP_ENSEMBLE_DE ? p1[j] : 0.0;
        cum += M.weight[j];
        // (cum 2^32 is exact; the last member takes what is left of the 2^32 words)
        M.below[j] = j == n - 1 ? 1ull << 32 : (unsigned long long)std::fmin(cum * 4294967296.0, 4294967296.0);
    }
    h->mv.checked = false;
    return MCMC_HIP_OK;
}

}  // extern "C"
