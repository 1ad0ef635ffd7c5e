// libmcmc_hip.so: incremental evaluation (MCMC_HIP_FLAG_INCREMENTAL) -- the directions of a
// launch, the scheduler of the step kernels (step_incremental), the d > 128 stepper (step_huge),
// and the carried state's getters and setters.
#include "ctx.h"

// fills `V` (and `flag` when the sequence has one-parameter blocks) with the directions of
// cycles [c0, c0 + ncyc) of sequence `which` of the blocked proposer; shared_schedule: every group
// takes its slots in the order of global group 0
int blocked_basis(mcmc_hip_ctx* h, int which, unsigned long long c0, int ncyc, int L, size_t slab,
                  DevBuf<double>& V, DevBuf<int>& flag, bool& any_1d, hipStream_t st, bool shared_schedule)
{
    if (!st) st = h->stream;
    const int nb = (int)h->blk_size.size();
    any_1d = false;
    for (int b = 0; b < nb; ++b) {
        const bool in_seq = which == 0 || (which == 1) == (b <= h->drag_last_slow);
        any_1d = any_1d || (in_seq && h->blk_size[b] == 1);
    }
    HIP_TRY(h, V.resize((size_t)h->BG * ncyc * slab));
    if (any_1d) HIP_TRY(h, flag.resize((size_t)h->BG * ncyc * L));
    mcmc::BlockedBasisArgs b{};
    b.T = h->dT.p; b.V = V.p; b.vflag = any_1d ? flag.p : nullptr;
    b.block_size = h->dblk.p; b.oversample = h->dblk.p + nb; b.i_of_j = h->dblk.p + 2 * nb;
    b.n_blocks = nb; b.d = h->d; b.which = which; b.drag_last_slow = h->drag_last_slow;
    b.L = L; b.slab = (int)slab;
    b.ld = h->d;
    b.nmax = *std::max_element(h->blk_size.begin(), h->blk_size.end());
    b.group0 = h->cfg.walker_offset / (uint32_t)h->bgs;   // (bgs == gs outside incremental mode)
    b.cycle0 = (uint32_t)c0;
    b.key0 = (uint32_t)h->cfg.seed; b.key1 = (uint32_t)(h->cfg.seed >> 32);
    b.ncyc = ncyc;
    // one slot schedule for the whole ensemble: the shuffle of GLOBAL group 0 (function targets)
    b.shuffle_group1 = shared_schedule ? 1u : 0u;
    HIP_TRY(h, mcmc_hip_launch_blocked_basis(&b, h->BG, st));
    return MCMC_HIP_OK;
}

namespace {

using mcmc::IncChoice;
using mcmc::IncShape;

// ---- which kernel (inc_choice.h), asked with this engine's shape ----

// the general kernels' answer for a shape (mcmc_hip_inc_any_fits); to launch one, its launcher
// must be linked in as well
bool inc_any_fits(const IncShape& s, bool to_launch)
{
    if (!mcmc::inc_shape_valid(s) || !mcmc_hip_inc_any_fits) return false;
    if (to_launch && !mcmc_hip_launch_inc_any) return false;
    return mcmc_hip_inc_any_fits(s.d, s.K, s.n_periodic, s.W, s.bgs) != 0;
}

// the shape of this engine's model and ensemble: the context is read HERE and nowhere else
IncShape inc_shape_of(const mcmc_hip_ctx* h)
{
    IncShape s;
    s.d = h->d; s.K = h->K; s.W = h->W; s.bgs = h->bgs;
    for (int32_t p : h->periodic) s.n_periodic += p ? 1 : 0;
    s.n_drag = h->drag_last_slow >= 0 ? h->drag_steps : 0;
    s.any_normal = (h->norm_mask4[0] | h->norm_mask4[1] | h->norm_mask4[2] | h->norm_mask4[3]) != 0u;
    s.one_box = h->have_prior && !s.any_normal;
    for (int i = 1; i < h->d && s.one_box; ++i) s.one_box = h->lo[i] == h->lo[0] && h->hi[i] == h->hi[0];
    s.box_lo_is_zero = s.one_box && h->lo[0] == 0.0;
    for (size_t b = 0; h->blocked && b < h->blk_size.size(); ++b)
        s.has_1d_block = s.has_1d_block || h->blk_size[b] == 1;
    s.emit = h->cfg.emit_capacity > 0;
    s.duo = h->duo;
    return s;
}

typedef hipError_t (*IncLauncher)(const mcmc::IncStepArgs*, hipStream_t);

// the launcher of a choice; null: not linked in (a build of a few dimensions)
IncLauncher inc_launcher(const IncChoice& C)
{
    if (C.any()) return mcmc_hip_launch_inc_any;
    const int dq = C.dq;
    const IncLauncher four =
        C.family == mcmc::kIncStepEmit
            ? (dq <= 8 ? mcmc_hip_launch_inc_emit_1 : dq <= 16 ? mcmc_hip_launch_inc_emit_9
               : dq <= 24 ? mcmc_hip_launch_inc_emit_17 : mcmc_hip_launch_inc_emit_25)
            : (dq <= 8 ? mcmc_hip_launch_inc_step_1 : dq <= 16 ? mcmc_hip_launch_inc_step_9
               : dq <= 24 ? mcmc_hip_launch_inc_step_17 : mcmc_hip_launch_inc_step_25);
    const IncLauncher two = C.family == mcmc::kIncDuoOne ? mcmc_hip_launch_inc_duo1
                            : C.family == mcmc::kIncDuoMix
                                ? (C.dq_lo == 1 ? mcmc_hip_launch_inc_duo_1 : mcmc_hip_launch_inc_duo_9)
                                : nullptr;
    return two ? two : four;   // (a build without incremental_duo.hip keeps the four-lane kernels)
}

// ---- the launches of a call ----
// mcmc_hip_step in incremental mode (MCMC_HIP_FLAG_INCREMENTAL; incremental_kernels.hip).
// Launches are cut at the multiples of refresh_every = 40 cycle lengths, where y = L^-1 (x - mu)
// is recomputed from x (the specification: oracle/mcmc_oracle.c, orc_run).
struct IncPlan {   // what the cutting of launches depends on besides the step counter and the choice
    int d, K, nd, Lc, Lf, ld, max_cyc, max_cyc_f, max_steps_vu;
    size_t dd, ddf;
    unsigned long long R;
    IncLauncher launch;
};
struct IncSeg {    // one launch: steps [step0, step0 + n)
    unsigned long long step0, c0, cyc0_f;
    int n, ncyc, ncyc_f;
};

IncSeg plan_segment(const IncPlan& P, unsigned long long step, int left)
{
    IncSeg s{};
    const unsigned long long Lc = (unsigned long long)P.Lc;
    s.step0 = step;
    s.c0 = step / Lc;
    unsigned long long room = P.R - step % P.R;
    room = std::min<unsigned long long>(room, (s.c0 + (unsigned long long)P.max_cyc) * Lc - step);
    room = std::min<unsigned long long>(room, (unsigned long long)P.max_steps_vu);
    int n = (int)std::min<unsigned long long>((unsigned long long)left, room);
    if (P.nd > 0) {   // at most max_cyc_f cycles of fast directions per launch
        const unsigned long long und = (unsigned long long)P.nd, uLf = (unsigned long long)P.Lf;
        s.cyc0_f = step * und / uLf;
        const unsigned long long fend = (s.cyc0_f + (unsigned long long)P.max_cyc_f) * uLf;
        const unsigned long long room_f = (fend - step * und) / und;   // whole steps
        n = (int)std::min<unsigned long long>((unsigned long long)n, std::max<unsigned long long>(1, room_f));
        const unsigned long long f1 = (step + (unsigned long long)n) * und - 1;
        s.ncyc_f = (int)(f1 / uLf - s.cyc0_f + 1);
    }
    s.n = n;
    s.ncyc = (int)((step + (unsigned long long)n - 1) / Lc - s.c0 + 1);
    return s;
}

// step_inc_kernel (C.fold): the steps whose directions are formed TOGETHER -- a call's steps as
// far as the direction buffers hold them, NOT cut at the refresh of y: the launches inside (cut
// there by plan_segment) read their columns out of one set and follow each other directly
IncSeg plan_span(const IncChoice& C, const IncPlan& P, unsigned long long step, int left)
{
    if (!C.fold) return plan_segment(P, step, left);
    IncSeg s{};
    const unsigned long long Lc = (unsigned long long)P.Lc;
    s.step0 = step;
    s.c0 = step / Lc;
    unsigned long long room = (s.c0 + (unsigned long long)P.max_cyc) * Lc - step;
    room = std::min<unsigned long long>(room, (unsigned long long)P.max_steps_vu);
    s.n = (int)std::min<unsigned long long>((unsigned long long)left, room);
    s.ncyc = (int)((step + (unsigned long long)s.n - 1) / Lc - s.c0 + 1);
    return s;
}

// fills the set D with the directions of launch `s`, on stream `st`
int make_directions(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, const IncSeg& s,
                    mcmc_hip_ctx::DirSet& D, hipStream_t st)
{
    Timed t(h, 1, st);
    const int nd = P.nd;
    bool any_1d = false, any_1d_f = false;
    if (h->blocked) {
        int rc = blocked_basis(h, C.drag() ? 1 : 0, s.c0, s.ncyc, P.Lc, P.dd, D.V, D.vflag, any_1d, st);
        if (rc != MCMC_HIP_OK) return rc;
        if (C.drag()) {
            rc = blocked_basis(h, 2, s.cyc0_f, s.ncyc_f, P.Lf, P.ddf, D.Vf, D.vflag_f, any_1d_f, st);
            if (rc != MCMC_HIP_OK) return rc;
        }
    } else {
        const int rc = shared_basis(h, D.V, h->BG, h->cfg.walker_offset / (uint32_t)h->bgs, s.c0, s.ncyc, P.dd, st);
        if (rc != MCMC_HIP_OK) return rc;
    }
    HIP_TRY(h, D.VU.resize((size_t)h->BG * s.n * (1 + nd) * (size_t)C.colb));
    // one-parameter blocks: the columns that draw the RandProposer1D variates, in VU order
    D.has_flags = any_1d || any_1d_f;
    if (D.has_flags) HIP_TRY(h, D.colflag.resize((size_t)h->BG * s.n * (1 + nd)));
    mcmc::IncDirArgs w{};
    w.V = D.V.p; w.Lrow = h->inc_Lrow.p; w.VU = D.VU.p;
    w.step0 = s.step0; w.cycle0 = s.c0; w.n_steps = s.n; w.ncyc = s.ncyc;
    w.slab = (int)P.dd; w.ld = P.ld; w.d = P.d; w.dq = C.dq; w.n_modes = P.K; w.cps = P.Lc;
    w.out_total = s.n * (1 + nd);
    w.colflag = D.has_flags ? D.colflag.p : nullptr;
    w.vflag = any_1d ? D.vflag.p : nullptr;
    if (C.carry || C.carry_modes) {
        HIP_TRY(h, D.UU.resize((size_t)h->BG * s.n * (C.carry_modes ? (size_t)P.K : 1)));
        w.UU = D.UU.p;
    }
    if (C.carry_prior) {
        HIP_TRY(h, D.VW.resize((size_t)h->BG * s.n * 4 * (size_t)C.dq));
        HIP_TRY(h, D.NL.resize((size_t)h->BG * s.n * 2));
        w.prior = h->inc_prior.p; w.VW = D.VW.p; w.NL = D.NL.p;
    }

    if (C.drag()) { w.out_div = 1; w.out_cols = 1 + nd; w.out_slot0 = 0; }
    if (C.any()) HIP_TRY(h, mcmc_hip_launch_whiten_directions_planes(&w, h->BG, st));
    else HIP_TRY(h, mcmc_hip_launch_whiten_directions(&w, h->BG, st));
    if (C.drag()) {   // the fast directions of the n * n_drag interpolation steps
        w.V = D.Vf.p;
        w.step0 = s.step0 * (unsigned long long)nd; w.cycle0 = s.cyc0_f;
        w.n_steps = s.n * nd; w.ncyc = s.ncyc_f; w.slab = (int)P.ddf; w.cps = P.Lf;
        w.out_div = nd; w.out_cols = 1 + nd; w.out_slot0 = 1;
        w.vflag = any_1d_f ? D.vflag_f.p : nullptr;
        HIP_TRY(h, mcmc_hip_launch_whiten_directions(&w, h->BG, st));
    }
    D.step0 = s.step0; D.n = s.n; D.epoch = h->dir_epoch;
    HIP_TRY(h, hipEventRecord(D.ready, st));
    return MCMC_HIP_OK;
}

}  // namespace

// mcmc_hip_step at 128 < d <= 256 (huge_kernels.hip): one parameter block, Metropolis steps, 1..4
// Gaussian modes, no periodic parameter, no emitted rows.  A launch stays inside one cycle of the
// basis: the Haar columns of that cycle are formed for every basis group (kept while the cycle and
// the transform stay), then the directions of the launch's steps, then the step kernel -- which
// refreshes y from x itself at the multiples of refresh_every = 40 d (oracle: orc_run).
int step_huge(mcmc_hip_ctx* h, int n_steps)
{
    const int d = h->d, K = h->K;
    if (K < 0 || K > mcmc::kHugeMaxModes || h->bg.on)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "d=%d > %d steps the `one` likelihood and Gaussian targets of 1..%d modes (K=%d is not served)",
                    d, kMaxDimBig, mcmc::kHugeMaxModes, K);
    if (h->any_periodic || h->blocked || h->drag_last_slow >= 0 || h->cfg.emit_capacity > 0 || h->emit_thin > 1)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "d=%d > %d serves one parameter block without periodic parameters or emitted rows",
                    d, kMaxDimBig);
    bool any_normal = false;
    for (int i = 0; i < d; ++i) any_normal = any_normal || h->kind[i] == 1;
    const int dpad = 4 * ((d + 3) / 4);
    const int stride = mcmc::huge_col_stride(d, K);
    const size_t BG = (size_t)h->BG;
    const unsigned long long ud = (unsigned long long)d, R = 40ull * ud;
    // steps per launch: at most what is left of the cycle, and a direction set of <= 256 MiB
    const int max_n = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)32 << 20) / (BG * stride)));
    int left = n_steps;
    while (left > 0) {
        const unsigned long long cyc = h->step / ud;
        const int n = (int)std::min<unsigned long long>(
            (unsigned long long)std::min(left, max_n), ud - h->step % ud);
        if (h->hV_cycle != cyc || h->hV_epoch != h->dir_epoch) {
            Timed t(h, 1);
            const long long per = mcmc::huge_basis_scratch(d);
            const int slabs = (int)std::max<long long>(1, std::min<long long>((long long)BG, (32ll << 20) / per));
            HIP_TRY(h, h->hV.resize(BG * (size_t)d * d));
            HIP_TRY(h, h->hScratch.resize((size_t)slabs * (size_t)per));
            mcmc::HugeBasisArgs b{};
            b.T = h->dT.p; b.V = h->hV.p; b.scratch = h->hScratch.p; b.d = d; b.ncyc = 1;
            b.group0 = h->cfg.walker_offset / (uint32_t)h->bgs; b.cycle0 = (uint32_t)cyc;
            b.key0 = (uint32_t)h->cfg.seed; b.key1 = (uint32_t)(h->cfg.seed >> 32);
            HIP_TRY(h, mcmc_hip_launch_huge_basis(&b, (int)BG, slabs, h->stream));
            h->hV_cycle = cyc; h->hV_epoch = h->dir_epoch;
        }
        {
            Timed t(h, 1);
            HIP_TRY(h, h->hCols.resize(BG * (size_t)n * stride));
            mcmc::HugeDirArgs w{};
            w.V = h->hV.p; w.Lrow = h->inc_Lrow.p; w.prior = h->inc_prior.p; w.out = h->hCols.p;
            w.step0 = h->step; w.cycle0 = cyc; w.n_steps = n; w.ncyc = 1; w.d = d; w.dpad = dpad; w.K = K;
            w.carry_prior = (K == 1 && any_normal) ? 1 : 0;
            HIP_TRY(h, mcmc_hip_launch_huge_dirs(&w, (int)BG, h->stream));
        }
        {
            Timed t(h, 0);
            const ConstLayout cl{d, K};
            mcmc::HugeStepArgs a{};
            a.x = h->x.p; a.y = h->y.p; a.logpost = h->logpost.p; a.logprior = h->logprior.p;
            a.loglike = h->loglike.p; a.weight = h->weight_i.p; a.prior_rej = h->prej.p;
            a.burn_left = h->burn.p; a.n_accept = h->nacc.p; a.accept_total = h->acc_total.p;
            a.stuck = h->stuck.p; a.cols = h->hCols.p; a.prior = h->inc_prior.p;
            a.Lrow = h->inc_Lrow.p; a.mean = h->inc_mean.p; a.scale = h->cblock.p + cl.scale();
            a.cnorm = h->cblock.p + cl.cnorm(); a.mweight = h->cblock.p + cl.weight();
            a.d = d; a.dpad = dpad; a.K = K; a.W = h->W; a.bgs = h->bgs;
            a.walker0 = h->cfg.walker_offset;
            a.key0 = (uint32_t)h->cfg.seed; a.key1 = (uint32_t)(h->cfg.seed >> 32);
            a.step0 = h->step; a.refresh = R; a.n_steps = n;
            a.anchor = h->y_valid ? 0 : 1;
            a.carry_prior = (K == 1 && any_normal) ? 1 : 0;
            a.uniform_logp = h->uniform_logp; a.temperature = h->cfg.temperature;
            a.max_tries = h->cfg.max_tries;
            HIP_TRY(h, mcmc_hip_launch_huge_step(&a, h->stream));
            h->y_valid = true;
            h->n_step_launches += 1;
            take_noted_kernel(h);
        }
        h->step += (unsigned long long)n;
        left -= n;
    }
    return MCMC_HIP_OK;
}

namespace {

// the arguments of one step kernel: n steps from h->step on, their columns in the set D
mcmc::IncStepArgs fill_inc_args(const mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P,
                                const mcmc_hip_ctx::DirSet& D, int n, int anchor)
{
    const int d = P.d, K = P.K;
    mcmc::IncStepArgs a{};
    a.s = step_args(h);
    a.s.group_size = h->bgs;   // the walkers that share a column of VU
    a.s.norm_mask = 0;         // (these kernels take the priors from `prior` and has_norm)
    a.s.rows = h->rows.p; a.s.n_rows = h->nrows.p; a.s.row_cap = h->cfg.emit_capacity;
    a.s.thin = h->emit_thin; a.s.thin_acc = h->thin_acc.p;
    a.s.n_modes = K;
    {
        const ConstLayout cl{d, K};
        a.n_modes = K; a.cnorm_off = cl.cnorm(); a.weight_off = cl.weight();
    }
    a.s.step0 = h->step; a.s.n_steps = n;
    a.s.cnorm0 = h->cnorm[0];
    a.y = h->y.p; a.VU = D.VU.p; a.prior = h->inc_prior.p;
    a.d = d; a.dq = C.dq;
    a.has_norm = (h->norm_mask4[0] | h->norm_mask4[1] | h->norm_mask4[2] | h->norm_mask4[3]) != 0u;
    a.box = C.box;
    a.box_lo = h->lo[0]; a.box_hi = h->hi[0];
    a.n_drag = P.nd; a.chunk_steps = C.chunk_steps;
    a.colflag = D.has_flags ? D.colflag.p : nullptr;
    a.Lrow = h->inc_Lrow.p;
    a.UU = (C.carry || C.carry_modes) ? D.UU.p : nullptr;
    a.anchor = anchor;
    a.amode = C.carry_modes ? h->amode.p : nullptr;
    // (the launch's columns inside the set; 0 / 0: the set is this launch's own)
    a.vu_cols = C.fold ? D.n : 0;
    a.col0 = C.fold ? (int)(h->step - D.step0) : 0;
    a.mean = h->inc_mean.p;
    a.VW = C.carry_prior ? D.VW.p : nullptr;
    a.NL = C.carry_prior ? D.NL.p : nullptr;
    a.accept_slack = h->accept_slack;
    periodic_mask4(h, a.periodic_mask4);
    return a;
}

// Makes the current set, h->dirs[h->dir_cur], hold the directions of `span`: `covers` (the set
// still holds columns of this call: span becomes the set's own), a hit on a set prepared ahead,
// or formed now.  wait_ready: the set is being formed on the second stream, and the main stream
// still has to wait for D.ready in front of the step kernel.
int acquire_direction_set(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, IncSeg& span,
                          bool covers, bool& wait_ready)
{
    auto& D = h->dirs[h->dir_cur];
    if (covers) { span.step0 = D.step0; span.n = D.n; }
    const bool hit = covers ||
        (D.ahead && D.step0 == span.step0 && D.n == span.n && D.epoch == h->dir_epoch);
    // (a set filled ahead on stream2 -- hit or not -- must have been written before it is
    // read or overwritten here)
    if (D.ahead) HIP_TRY(h, hipStreamWaitEvent(h->stream, D.ready, 0));
    D.ahead = false;
    wait_ready = false;
    if (hit) return MCMC_HIP_OK;
    // Not prepared (the first launch of a call, see prepare_next_set): formed on the SECOND stream
    // behind the previous step kernel (`mark`) -- beside the moment snapshot and the y
    // refresh the main stream still holds, like a set prepared ahead -- and behind the
    // last write of the transform: a proposal refreshed since the previous call is in
    // them at once, nothing stale is computed and thrown away.
    if (h->prefetch && h->lazy_dirs && h->mark_valid && h->stream2) {
        HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->mark, 0));
        if (h->T_fresh) HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->T_event, 0));
        const int rc = make_directions(h, C, P, span, D, h->stream2);
        if (rc != MCMC_HIP_OK) return rc;
        // (the main stream waits for the set where it needs it: in front of the step
        // kernel, BEHIND the refresh of y -- which does not read the directions and ran
        // 24 us late behind this wait: timeline of round 5, 101 -> 77 us between the
        // step kernels of a call that forms its set)
        wait_ready = true;
    } else {
        const int rc = make_directions(h, C, P, span, D, h->stream);
        if (rc != MCMC_HIP_OK) return rc;
    }
    h->T_fresh = false;
    return MCMC_HIP_OK;
}

// One step kernel over the next steps of the set D: at most `room` of them, cut at the refresh of
// y (plan_segment); n: how many it took.  `inside`: a launch of this call went before it.
int launch_segment(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, mcmc_hip_ctx::DirSet& D,
                   bool inside, int room, bool& wait_ready, int& n)
{
    bool anchor = false;   // y is refreshed from x before (or, step_inc_kernel: in) this launch
    bool refresh_in_kernel = false;
    if (!h->y_valid || h->step % P.R == 0) {
        if (C.fold && inside) {
            // (round 5) a launch INSIDE a call refreshes y itself: nothing stands between it
            // and the launch before.  The first launch of a call keeps the separate kernel:
            // the refresh inside the step kernel -- two barriers and a memory round trip per
            // eight dimensions before the first chunk can be staged -- costs that launch 22 us
            // (timeline: 912 against 890 us), whiten_state_kernel 14 beside the moment
            // snapshot's host gap
            refresh_in_kernel = true;
        } else {
            HIP_TRY(h, mcmc_hip_launch_whiten_state(h->x.p, h->y.p, h->inc_mean.p, h->inc_Lrow.p,
                                                    P.d, h->W, P.K, h->stream));
        }
        h->y_valid = true;
        anchor = true;
    }
    // (carried mode log-densities that no launch has written since y was set are re-anchored
    // on y: after set_state always; after a resume only if the state file did not hold them)
    if (C.carry_modes && !h->amode_valid) anchor = true;
    n = plan_segment(P, h->step, room).n;
    if (wait_ready) {
        HIP_TRY(h, hipStreamWaitEvent(h->stream, D.ready, 0));
        wait_ready = false;
    }
    {
        Timed t(h, 0);
        const mcmc::IncStepArgs a =
            fill_inc_args(h, C, P, D, n, (anchor ? 1 : 0) | (refresh_in_kernel ? 2 : 0));
        if (C.carry_modes) h->amode_valid = true;
        HIP_TRY(h, P.launch(&a, h->stream));
        h->n_step_launches += 1;
        take_noted_kernel(h);
    }
    h->step += (unsigned long long)n;
    return MCMC_HIP_OK;
}

// Behind the last step kernel of a set: records `mark` there and, by the regime's rule, forms the
// set expected next on the second stream behind it; then the other set becomes the current one.
// left: the steps of this call still to come; n_steps: the call's length (a later call is
// expected to be like this one).
int prepare_next_set(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, int left, int n_steps)
{
    auto& N = h->dirs[h->dir_cur ^ 1];
    if (C.fold) {
        // the set is kept while it has columns left; the next one is formed by the call that
        // needs it (acquire_direction_set: lazy_dirs), behind this step kernel
        HIP_TRY(h, hipEventRecord(h->mark, h->stream));
        h->mark_valid = true;
        const auto& D = h->dirs[h->dir_cur];
        if (h->step < D.step0 + (unsigned long long)D.n) return MCMC_HIP_OK;
        if (h->prefetch && h->stream2 && (left > 0 || !h->lazy_dirs)) {
            const IncSeg nxt = plan_span(
                C, P, h->step, std::max(left, std::min(h->lookahead, 16) * n_steps));
            HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->mark, 0));
            const int rc = make_directions(h, C, P, nxt, N, h->stream2);
            if (rc != MCMC_HIP_OK) return rc;
            N.ahead = true;
        }
    } else if (h->prefetch) {
        // the launch expected next: the rest of this call, or a call like this one.  Its
        // directions are computed on the second stream BEHIND this step kernel (the event
        // is recorded after it), beside the moment snapshot and the refresh of y that the
        // main stream runs between two step kernels.  Never beside the step kernel: its
        // 1024 workgroups are exactly what the chip holds at once, and a direction kernel
        // that takes a few of those places first -- it happened once in a hundred launches
        // when both became runnable together -- costs the displaced workgroups a second
        // round (1.78 ms instead of 1.04; with the event recorded BEFORE the step kernel
        // d = 64 ran 6.13 ms per launch instead of 4.24, d = 48 and d = 100 unchanged).
        const IncSeg nxt = plan_span(C, P, h->step, left > 0 ? left : n_steps);
        HIP_TRY(h, hipEventRecord(h->mark, h->stream));
        h->mark_valid = true;
        // (round 4) the launch a LATER call begins with is left to that call
        // (acquire_direction_set): the host is a launch ahead of the device, so its
        // directions still run in the same place -- behind this step kernel, beside the main
        // stream's work -- but see a transform that set_proposal_cov / the device checkpoint
        // writes in between.  Before, a refreshed proposal made the set prepared here stale
        // and the next call recomputed it on the MAIN stream: 141 us instead of 72 between
        // two step kernels after every learn checkpoint (tools/gpu.sh timeline, round 4).
        if (left > 0 || !h->lazy_dirs) {
            HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->mark, 0));
            const int rc = make_directions(h, C, P, nxt, N, h->stream2);
            if (rc != MCMC_HIP_OK) return rc;
            N.ahead = true;
        }
    }
    h->dir_cur ^= 1;
    return MCMC_HIP_OK;
}

// step_inc_kernel (C.fold), round 5 late: a set of directions reaches over SEVERAL calls --
// `lookahead` calls like this one -- and the calls that find their columns in it start
// with nothing but the moment snapshot between them and the previous step kernel (the
// direction kernels are latency-bound: 80 us for one launch's columns at config 2, hardly
// more for four).  Directions are pure functions of (group, cycle, transform): a set
// formed under another transform (dir_epoch) is dropped, never used.  The launches inside a
// set are cut at the refresh of y and follow each other directly: from the second of a call on,
// the kernel refreshes y itself.
int run_sets_over_calls(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, int n_steps)
{
    int left = n_steps;
    while (left > 0) {
        const auto& C0 = h->dirs[h->dir_cur];
        const bool covers = C0.n > 0 && C0.epoch == h->dir_epoch && C0.step0 <= h->step &&
                            h->step < C0.step0 + (unsigned long long)C0.n;
        // the steps whose directions form one set: the calls ahead as far as the buffers hold them
        IncSeg span = plan_span(C, P, h->step, std::max(left, std::min(h->lookahead, 16) * n_steps));
        bool wait_ready = false;
        int rc = acquire_direction_set(h, C, P, span, covers, wait_ready);
        if (rc != MCMC_HIP_OK) return rc;
        auto& D = h->dirs[h->dir_cur];
        // the steps of THIS call the set holds
        const int take = (int)std::min<unsigned long long>(
            (unsigned long long)left, D.step0 + (unsigned long long)D.n - h->step);
        for (int done = 0, n = 0; done < take; done += n) {
            rc = launch_segment(h, C, P, D, done > 0, take - done, wait_ready, n);
            if (rc != MCMC_HIP_OK) return rc;
        }
        left -= take;
        rc = prepare_next_set(h, C, P, left, n_steps);
        if (rc != MCMC_HIP_OK) return rc;
    }
    return MCMC_HIP_OK;
}

// Every other kernel: each launch (cut at the refresh of y, which a separate kernel does in
// front of it) has a set of its own, and the set of the next launch is formed behind it.
int run_set_per_launch(mcmc_hip_ctx* h, const IncChoice& C, const IncPlan& P, int n_steps)
{
    int left = n_steps;
    while (left > 0) {
        IncSeg span = plan_span(C, P, h->step, left);
        bool wait_ready = false;
        int rc = acquire_direction_set(h, C, P, span, false, wait_ready);
        if (rc != MCMC_HIP_OK) return rc;
        int n = 0;
        rc = launch_segment(h, C, P, h->dirs[h->dir_cur], false, span.n, wait_ready, n);
        if (rc != MCMC_HIP_OK) return rc;
        left -= n;
        rc = prepare_next_set(h, C, P, left, n_steps);
        if (rc != MCMC_HIP_OK) return rc;
    }
    return MCMC_HIP_OK;
}

}  // namespace

mcmc::IncChoice inc_choice_of(const mcmc_hip_ctx* h)
{
    if (!h->incremental) return IncChoice{};
    const IncShape s = inc_shape_of(h);
    return mcmc::inc_choose(s, inc_any_fits(s, true));
}

int step_incremental(mcmc_hip_ctx* h, int n_steps)
{
    const int d = h->d, K = h->K;
    const IncShape S = inc_shape_of(h);
    const IncChoice C = mcmc::inc_choose(S, inc_any_fits(S, true));
    if (C.reason == mcmc::kIncBadShape || C.reason == mcmc::kIncDragShape)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "incremental evaluation with dragging serves one Gaussian mode with "
                    "non-periodic priors; use evaluation: full for this model");
    if (C.reason == mcmc::kIncAnyLds)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "incremental evaluation: %d modes at d=%d with %d periodic parameters do not "
                    "fit the LDS of a CU; use evaluation: full for this model", K, d, S.n_periodic);
    // (round 6: the general incremental kernels thin too -- mixtures, periodic parameters, blocks of
    // one parameter; dragging emits on the from-scratch kernels, which do not)
    if (C.reason == mcmc::kIncEmitDrag && h->emit_thin > 1)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "emit_thin: rows are thinned on the device by the incremental Metropolis kernels; "
                    "thin on the host");
    if (C.reason == mcmc::kIncEmitDrag)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "incremental evaluation emits rows (emit_capacity > 0) with Metropolis "
                    "steps; use evaluation: full for dragging with emitted rows");
    IncPlan P{};
    P.d = d; P.K = K; P.nd = S.n_drag;
    P.launch = inc_launcher(C);
    if (!P.launch || !mcmc_hip_launch_whiten_directions)
        return fail(h, MCMC_HIP_ERR_DEVICE, "the incremental kernels for d=%d are not linked in", d);
    // columns (= steps) per cycle: d for one block, sum_b oversample_b n_b with blocks, the slow
    // blocks' parameters when dragging (+ the fast sequence of the interpolation steps)
    P.Lc = block_slots(h, C.drag() ? 1 : 0);
    P.Lf = C.drag() ? block_slots(h, 2) : 0;
    P.R = 40ull * (unsigned long long)P.Lc;
    P.max_steps_vu = (int)std::max<size_t>(
        4, ((size_t)512 << 20) / (sizeof(double) * (size_t)C.colb * (size_t)(1 + P.nd) * (size_t)h->BG));
    // (blocked directions are written with column stride d at every d)
    P.dd = (h->kb && !h->blocked) ? (size_t)mcmc::v_slab_big(d) : (size_t)mcmc::v_slab_cols(P.Lc, d);
    P.ddf = C.drag() ? (size_t)mcmc::v_slab_cols(P.Lf, d) : 0;
    P.ld = (h->kb && !h->blocked) ? mcmc::v_ld(d) : d;
    P.max_cyc = (int)std::max<size_t>(1, (256u << 20) / (sizeof(double) * P.dd * (size_t)h->BG));
    P.max_cyc_f =
        C.drag() ? (int)std::max<size_t>(2, (256u << 20) / (sizeof(double) * P.ddf * (size_t)h->BG)) : 0;
    return C.fold ? run_sets_over_calls(h, C, P, n_steps) : run_set_per_launch(h, C, P, n_steps);
}

extern "C" {

// An ASYMMETRY, kept on purpose: this answers for the shape WITHOUT emitted rows or blocks of one
// parameter (its arguments do not say), although with either a shape the tuned kernels serve
// goes to the general one, which may not fit.  mcmc_hip_incremental_choice takes the whole shape.
int mcmc_hip_incremental_supported(int32_t d, int32_t n_modes, int32_t n_periodic, int32_t n_drag,
                                   int32_t n_walkers, int32_t basis_group_size)
{
    if (!mcmc_hip_launch_whiten_state) return 0;
    IncShape s;
    s.d = d; s.K = n_modes; s.n_periodic = n_periodic; s.n_drag = n_drag;
    s.W = n_walkers; s.bgs = basis_group_size;
    return mcmc::inc_choose(s, inc_any_fits(s, false)).family != mcmc::kIncNotServed ? 1 : 0;
}

int mcmc_hip_incremental_choice(const mcmc_hip_inc_shape* shape, mcmc_hip_inc_choice* out)
{
    if (!shape || !out) return MCMC_HIP_ERR_ARG;
    IncShape s;
    s.d = shape->d; s.K = shape->n_modes; s.n_periodic = shape->n_periodic; s.n_drag = shape->n_drag;
    s.W = shape->n_walkers; s.bgs = shape->basis_group_size;
    s.any_normal = shape->any_normal != 0; s.one_box = shape->one_box != 0;
    s.box_lo_is_zero = shape->box_lo_is_zero != 0; s.has_1d_block = shape->has_1d_block != 0;
    s.emit = shape->emit != 0; s.duo = shape->duo;
    const IncChoice c = mcmc::inc_choose(s, inc_any_fits(s, false));
    static_assert(mcmc::kIncStep == MCMC_HIP_INC_STEP && mcmc::kIncStepEmit == MCMC_HIP_INC_STEP_EMIT &&
                  mcmc::kIncMix == MCMC_HIP_INC_MIX && mcmc::kIncAny == MCMC_HIP_INC_ANY &&
                  mcmc::kIncDrag == MCMC_HIP_INC_DRAG && mcmc::kIncDuoMix == MCMC_HIP_INC_DUO_MIX &&
                  mcmc::kIncDuoOne == MCMC_HIP_INC_DUO_ONE, "mcmc_hip.h names the families of inc_choice.h");
    out->family = c.family; out->reason = c.reason; out->dq_lo = c.dq_lo;
    out->carry = c.carry; out->carry_modes = c.carry_modes; out->carry_prior = c.carry_prior;
    out->carry_periodic = c.carry_periodic; out->fold = c.fold;
    out->chunk_steps = c.chunk_steps; out->colb = c.colb;
    out->thins_on_device = c.thins_on_device; out->box = c.box;
    return MCMC_HIP_OK;
}

int mcmc_hip_get_whitened(mcmc_hip_ctx* h, double* y)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->incremental || !y) return fail(h, MCMC_HIP_ERR_ARG, "not in incremental mode, or null");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->y_valid) {
        HIP_TRY(h, mcmc_hip_launch_whiten_state(h->x.p, h->y.p, h->inc_mean.p, h->inc_Lrow.p, h->d,
                                                h->W, h->K, h->stream));
        h->y_valid = true;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, d = (size_t)h->d * (size_t)h->K;   // device: [K d][W]
    std::vector<double> yt(W * d);
    HIP_TRY(h, hipMemcpy(yt.data(), h->y.p, sizeof(double) * W * d, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < d; ++i) y[w * d + i] = yt[i * W + w];
    return MCMC_HIP_OK;
}

int mcmc_hip_set_whitened(mcmc_hip_ctx* h, const double* y)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->incremental || !y) return fail(h, MCMC_HIP_ERR_ARG, "not in incremental mode, or null");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "set_full_state must precede set_whitened");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, d = (size_t)h->d * (size_t)h->K;
    std::vector<double> yt(W * d);
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < d; ++i) yt[i * W + w] = y[w * d + i];
    HIP_TRY(h, hipMemcpy(h->y.p, yt.data(), sizeof(double) * W * d, hipMemcpyHostToDevice));
    h->y_valid = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_incremental_carries_periodic(const mcmc_hip_ctx* h)
{
    return h && inc_choice_of(h).carry_periodic ? 1 : 0;
}

int mcmc_hip_accept_estimate_error(double* max_err, uint32_t* ka_at_max)
{
    if (!max_err || !ka_at_max) return MCMC_HIP_ERR_ARG;
    if (!mcmc_hip_launch_accept_estimate_error) return MCMC_HIP_ERR_ARG;   // (a build without incremental_duo.hip)
    constexpr int nb = 4096;
    double* derr = nullptr;
    uint32_t* dka = nullptr;
    std::vector<double> err(nb);
    std::vector<uint32_t> ka(nb);
    hipError_t r = hipMalloc(&derr, sizeof(double) * nb);
    if (r == hipSuccess) r = hipMalloc(&dka, sizeof(uint32_t) * nb);
    if (r == hipSuccess) r = mcmc_hip_launch_accept_estimate_error(derr, dka, nb, nullptr);
    if (r == hipSuccess) r = hipMemcpy(err.data(), derr, sizeof(double) * nb, hipMemcpyDeviceToHost);
    if (r == hipSuccess) r = hipMemcpy(ka.data(), dka, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost);
    if (derr) (void)hipFree(derr);
    if (dka) (void)hipFree(dka);
    if (r != hipSuccess) return MCMC_HIP_ERR_DEVICE;
    int at = 0;
    for (int b = 1; b < nb; ++b)
        if (err[b] > err[at] || err[b] != err[b]) at = b;   // (a NaN wins)
    *max_err = err[at];
    *ka_at_max = ka[at];
    return MCMC_HIP_OK;
}

int mcmc_hip_incremental_carries_modes(const mcmc_hip_ctx* h)
{
    return h && inc_choice_of(h).carry_modes ? 1 : 0;
}

int mcmc_hip_get_mode_logdensities(mcmc_hip_ctx* h, double* a)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!a || !inc_choice_of(h).carry_modes)
        return fail(h, MCMC_HIP_ERR_ARG, "this engine does not carry mode log-densities, or null");
    if (!h->have_state || !h->amode_valid)
        return fail(h, MCMC_HIP_ERR_STATE, "no carried mode log-densities yet (a step forms them)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, K = (size_t)h->K;
    std::vector<double> t(W * K);
    HIP_TRY(h, hipMemcpy(t.data(), h->amode.p, sizeof(double) * W * K, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
        for (size_t k = 0; k < K; ++k) a[w * K + k] = t[k * W + w];
    return MCMC_HIP_OK;
}

int mcmc_hip_set_mode_logdensities(mcmc_hip_ctx* h, const double* a)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!a || !inc_choice_of(h).carry_modes)
        return fail(h, MCMC_HIP_ERR_ARG, "this engine does not carry mode log-densities, or null");
    if (!h->have_state || !h->y_valid)
        return fail(h, MCMC_HIP_ERR_STATE, "set_full_state and set_whitened must precede set_mode_logdensities");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, K = (size_t)h->K;
    std::vector<double> t(W * K);
    for (size_t w = 0; w < W; ++w)
        for (size_t k = 0; k < K; ++k) t[k * W + w] = a[w * K + k];
    HIP_TRY(h, hipMemcpy(h->amode.p, t.data(), sizeof(double) * W * K, hipMemcpyHostToDevice));
    h->amode_valid = true;
    return MCMC_HIP_OK;
}

}  // extern "C"
