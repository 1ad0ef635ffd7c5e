// libmcmc_hip.so: the learn / convergence checkpoint on the device and R-1 of the confidence
// bounds (checkpoint_kernels.hip), and the communicator they reduce over.
#include "ctx.h"

extern "C" {

// ---- the checkpoint on the device -------------------------------------------------------------
int mcmc_hip_checkpoint_set_ring(mcmc_hip_ctx* h, int32_t n_intervals, const double* group_sum,
                                 const double* pooled_S, int32_t min_capacity)
{
    if (!h || n_intervals < 0 || (n_intervals > 0 && (!group_sum || !pooled_S))) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& K = h->ck;
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2, ne = G * d + np;
    int cap = 16;
    while (cap < std::max(n_intervals + 2, (int)min_capacity)) cap *= 2;
    K.ring.release();
    HIP_TRY(h, K.ring.resize((size_t)cap * ne));
    K.cap = cap;
    K.n_done = n_intervals;      // (slot of interval k of the list = k)
    std::vector<double> buf((size_t)std::max(n_intervals, 1) * ne, 0.0);
    for (int k = 0; k < n_intervals; ++k) {
        double* dst = buf.data() + (size_t)k * ne;
        std::copy(group_sum + (size_t)k * G * d, group_sum + (size_t)(k + 1) * G * d, dst);
        const double* S = pooled_S + (size_t)k * d * d;
        for (size_t i = 0; i < d; ++i)
            for (size_t j = 0; j <= i; ++j) dst[G * d + i * (i + 1) / 2 + j] = S[i * d + j];
    }
    if (n_intervals > 0)
        HIP_TRY(h, hipMemcpy(K.ring.p, buf.data(), sizeof(double) * (size_t)n_intervals * ne,
                             hipMemcpyHostToDevice));
    HIP_TRY(h, K.wsum.resize(ne + G * d));   // window sums | chain means
    HIP_TRY(h, K.payload.resize(5 + 2 * d * d + d));
    HIP_TRY(h, K.ws.resize(7 * d * d + 5 * d + 16));
    HIP_TRY(h, K.out.resize(8 + 2 * d * d));
    if (!K.acc_prev.p) {   // (a reload of the ring keeps the counter of the last checkpoint)
        HIP_TRY(h, K.acc_prev.resize(1));
        HIP_TRY(h, hipMemset(K.acc_prev.p, 0, sizeof(unsigned long long)));
    }
    if (!K.pin_out)
        HIP_TRY(h, hipHostMalloc((void**)&K.pin_out, sizeof(double) * (8 + 2 * d * d + d), hipHostMallocDefault));
    if (!K.ev) HIP_TRY(h, hipEventCreateWithFlags(&K.ev, hipEventDisableTiming));
    return MCMC_HIP_OK;
}

int mcmc_hip_checkpoint_set_accepted(mcmc_hip_ctx* h, int64_t accepted_at_last_checkpoint)
{
    if (!h || !h->ck.acc_prev.p) return MCMC_HIP_ERR_STATE;
    const unsigned long long v = (unsigned long long)accepted_at_last_checkpoint;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpy(h->ck.acc_prev.p, &v, sizeof v, hipMemcpyHostToDevice));
    return MCMC_HIP_OK;
}

int mcmc_hip_checkpoint_begin(mcmc_hip_ctx* h, int32_t n_window_intervals, int64_t n_window_snapshots,
                              double steps_since, uint64_t* payload_device_ptr, int32_t* payload_len)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& K = h->ck;
    if (!K.ring.p) return fail(h, MCMC_HIP_ERR_STATE, "checkpoint_set_ring must precede checkpoint_begin");
    if (K.begun || K.pending) return fail(h, MCMC_HIP_ERR_STATE, "a device checkpoint is already in flight");
    if (!h->mom_pending)
        return fail(h, MCMC_HIP_ERR_STATE, "request_moments (the read-out of this interval) must precede checkpoint_begin");
    if (n_window_intervals < 1 || n_window_intervals > K.cap || n_window_snapshots < 1)
        return fail(h, MCMC_HIP_ERR_ARG, "the window holds %d intervals (ring capacity %d)", n_window_intervals, K.cap);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2, ne = G * d + np;
    // (mcmc_hip_request_moments copied the interval out for the host's books and, with a ring,
    // left the accumulators alone: ckpt_window_kernel files them in the ring and resets them)
    mcmc::CkptWindowArgs w{};
    w.acc = h->gsum.p; w.ring = K.ring.p; w.wsum = K.wsum.p; w.n_elem = ne;
    w.means = K.wsum.p + ne; w.n_mean = G * d;
    w.n_per_chain = (double)n_window_snapshots * (double)h->gs;
    w.cap = K.cap; w.slot = (int)(K.n_done % K.cap);
    w.n_slots = n_window_intervals;
    w.first = (int)(((K.n_done - (n_window_intervals - 1)) % K.cap + K.cap) % K.cap);
    HIP_TRY(h, mcmc_hip_launch_ckpt_window(&w, h->stream));
    K.n_done += 1;
    mcmc::CkptPayloadArgs p{};
    p.wsum = K.wsum.p; p.means = K.wsum.p + ne; p.payload = K.payload.p; p.accept_total = h->acc_total.p;
    p.accept_prev = K.acc_prev.p; p.d = (int)d; p.G = (int)G; p.W = h->W;
    p.n_per_chain = (double)n_window_snapshots * (double)h->gs;
    p.steps_since = steps_since;
    HIP_TRY(h, mcmc_hip_launch_ckpt_payload(&p, h->stream));
    if (h->comm) {   // (also a communicator of ONE rank: the same RCCL launch an 8-GPU job queues)
        // ONE all-reduce per checkpoint, in place, in stream order: RCCL over xGMI
        if (int rc = mcmc_comm_allreduce_on_stream(h->comm, K.payload.p, 5 + 2 * d * d + d, 0, h->stream))
            return fail(h, rc, "%s", mcmc_comm_error(h->comm));
    }
    K.begun = true;
    if (payload_device_ptr) *payload_device_ptr = (uint64_t)(uintptr_t)K.payload.p;
    if (payload_len) *payload_len = (int32_t)(5 + 2 * d * d + d);
    return MCMC_HIP_OK;
}

int mcmc_hip_checkpoint_solve(mcmc_hip_ctx* h, double learn_lo, double learn_hi)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& K = h->ck;
    if (!K.begun) return fail(h, MCMC_HIP_ERR_STATE, "checkpoint_begin must precede checkpoint_solve");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t d = h->d;
    // a direction set being filled ahead still reads the transform (as in set_proposal_cov)
    for (auto& D : h->dirs)
        if (D.ahead && D.ready) HIP_TRY(h, hipStreamWaitEvent(h->stream, D.ready, 0));
    mcmc::CkptSolveArgs s{};
    s.payload = K.payload.p; s.ws = K.ws.p; s.out = K.out.p; s.T = h->dT.p;
    s.i_of_j = h->blocked ? h->dblk.p + 2 * (int)h->blk_size.size() : nullptr;
    s.d = (int)d; s.group_size = (double)h->gs; s.learn_lo = learn_lo; s.learn_hi = learn_hi;
    s.proposal_scale = h->cfg.proposal_scale;
    HIP_TRY(h, mcmc_hip_launch_ckpt_solve(&s, h->stream));
    if (h->T_event) {   // (the kernel may have refreshed dT)
        HIP_TRY(h, hipEventRecord(h->T_event, h->stream));
        h->T_fresh = true;
    }
    HIP_TRY(h, hipMemcpyAsync(K.pin_out, K.out.p, sizeof(double) * (8 + 2 * d * d),
                              hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipEventRecord(K.ev, h->stream));
    ++h->dir_epoch;     // the transform may have changed: directions computed ahead are stale
    K.begun = false;
    K.pending = true;
    K.payload_only = false;
    return MCMC_HIP_OK;
}

// The other way to finish a checkpoint begun on the device: only the (all-reduced) payload comes
// back -- 15 KB behind the launch, one event -- and the host solves it (mcmc_hip_gelman_rubin,
// mcmc_hip_set_proposal_cov) while the next launch runs: the window sums and the collective stay
// in stream order on the device, the d^3 work of ONE workgroup leaves the stream.
int mcmc_hip_checkpoint_request_payload(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& K = h->ck;
    if (!K.begun) return fail(h, MCMC_HIP_ERR_STATE, "checkpoint_begin must precede checkpoint_request_payload");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t d = h->d;
    HIP_TRY(h, hipMemcpyAsync(K.pin_out, K.payload.p, sizeof(double) * (5 + 2 * d * d + d),
                              hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipEventRecord(K.ev, h->stream));
    K.begun = false;
    K.pending = true;
    K.payload_only = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_checkpoint_fetch_payload(mcmc_hip_ctx* h, double* payload, int32_t n)
{
    if (!h || !payload) return MCMC_HIP_ERR_ARG;
    auto& K = h->ck;
    if (!K.pending || !K.payload_only)
        return fail(h, MCMC_HIP_ERR_STATE, "no payload read-out is pending (checkpoint_request_payload)");
    const size_t d = h->d;
    if ((size_t)n != 5 + 2 * d * d + d)
        return fail(h, MCMC_HIP_ERR_ARG, "the payload holds %zu doubles, not %d", 5 + 2 * d * d + d, n);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(K.ev));
    K.pending = false;
    K.payload_only = false;
    std::copy(K.pin_out, K.pin_out + n, payload);
    return MCMC_HIP_OK;
}

int mcmc_hip_checkpoint_fetch(mcmc_hip_ctx* h, double stats[8], double* mean_of_covs)
{
    if (!h || !stats) return MCMC_HIP_ERR_ARG;
    auto& K = h->ck;
    if (!K.pending || K.payload_only) return fail(h, MCMC_HIP_ERR_STATE, "no device checkpoint is pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(K.ev));
    K.pending = false;
    const size_t d = h->d, nn = d * d;
    std::copy(K.pin_out, K.pin_out + 8, stats);
    if (mean_of_covs) std::copy(K.pin_out + 8, K.pin_out + 8 + nn, mean_of_covs);
    if (K.pin_out[2] != 0.0) {    // the proposal was refreshed on the device: mirror it on the host
        h->cov.assign(K.pin_out + 8, K.pin_out + 8 + nn);
        h->T.assign(K.pin_out + 8 + nn, K.pin_out + 8 + 2 * nn);
        h->have_cov = true;
    }
    return MCMC_HIP_OK;
}

// ---- R-1 of the confidence-interval bounds on the device ----------------------------------------
int mcmc_hip_bounds_configure(mcmc_hip_ctx* h, int32_t n_slots)
{
    if (!h || n_slots < 0) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& B = h->bd;
    const size_t d = h->d, W = h->W, G = h->G;
    B.ring.release();
    B.n_slots = 0;
    if (n_slots == 0) return MCMC_HIP_OK;
    HIP_TRY(h, B.ring.resize((size_t)n_slots * d * W));
    HIP_TRY(h, B.bounds.resize(G * d * 2));
    HIP_TRY(h, B.payload.resize(1 + 4 * d));
    if (!B.pin) HIP_TRY(h, hipHostMalloc((void**)&B.pin, sizeof(double) * (1 + 4 * d + G * d * 2), hipHostMallocDefault));
    B.n_slots = n_slots;
    return MCMC_HIP_OK;
}

int mcmc_hip_bounds_snapshot(mcmc_hip_ctx* h, int32_t slot)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& B = h->bd;
    if (slot < 0 || slot >= B.n_slots) return fail(h, MCMC_HIP_ERR_ARG, "bounds slot %d of %d", slot, B.n_slots);
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)h->d * h->W;
    HIP_TRY(h, hipMemcpyAsync(B.ring.p + (size_t)slot * n, h->x.p, sizeof(double) * n,
                              hipMemcpyDeviceToDevice, h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_bounds_get_slot(mcmc_hip_ctx* h, int32_t slot, double* x)
{
    if (!h || !x) return MCMC_HIP_ERR_ARG;
    auto& B = h->bd;
    if (slot < 0 || slot >= B.n_slots) return fail(h, MCMC_HIP_ERR_ARG, "bounds slot %d of %d", slot, B.n_slots);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t d = h->d, W = h->W;
    std::vector<double> t(d * W);
    HIP_TRY(h, hipMemcpy(t.data(), B.ring.p + (size_t)slot * d * W, sizeof(double) * d * W, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < d; ++i) x[w * d + i] = t[i * W + w];
    return MCMC_HIP_OK;
}

int mcmc_hip_bounds_set_slot(mcmc_hip_ctx* h, int32_t slot, const double* x)
{
    if (!h || !x) return MCMC_HIP_ERR_ARG;
    auto& B = h->bd;
    if (slot < 0 || slot >= B.n_slots) return fail(h, MCMC_HIP_ERR_ARG, "bounds slot %d of %d", slot, B.n_slots);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t d = h->d, W = h->W;
    std::vector<double> t(d * W);
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < d; ++i) t[i * W + w] = x[w * d + i];
    HIP_TRY(h, hipMemcpy(B.ring.p + (size_t)slot * d * W, t.data(), sizeof(double) * d * W, hipMemcpyHostToDevice));
    return MCMC_HIP_OK;
}

int mcmc_hip_bounds_statistics(mcmc_hip_ctx* h, int32_t n_window, const int32_t* slots, double limfrac,
                               double* stats, double* bounds)
{
    if (!h || !slots || !stats) return MCMC_HIP_ERR_ARG;
    auto& B = h->bd;
    if (B.n_slots == 0) return fail(h, MCMC_HIP_ERR_STATE, "bounds_configure must precede bounds_statistics");
    if (n_window < 1 || n_window > mcmc::kBoundsMaxSlots || n_window > B.n_slots)
        return fail(h, MCMC_HIP_ERR_ARG, "the window holds %d snapshots (at most %d)", n_window,
                    std::min(mcmc::kBoundsMaxSlots, B.n_slots));
    if (!(limfrac > 0.0 && limfrac < 1.0)) return fail(h, MCMC_HIP_ERR_ARG, "limfrac must lie in (0, 1)");
    const long long n = (long long)n_window * h->gs;
    if ((size_t)n * sizeof(double) > (size_t)mcmc::kBoundsLdsBytes)
        return fail(h, MCMC_HIP_ERR_ARG, "%d snapshots of %d walkers do not fit the LDS of a compute unit", n_window, h->gs);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    mcmc::CkptBoundsArgs a{};
    a.ring = B.ring.p; a.bounds = B.bounds.p; a.n_slots = n_window; a.d = h->d; a.W = h->W; a.gs = h->gs;
    for (int s = 0; s < n_window; ++s) {
        if (slots[s] < 0 || slots[s] >= B.n_slots) return fail(h, MCMC_HIP_ERR_ARG, "bounds slot %d of %d", slots[s], B.n_slots);
        a.slots[s] = slots[s];
    }
    // GetDist's `confidence` (chains.py): index = searchsorted(cumsum(weights), target), capped at
    // n - 1, target = norm * limfrac (lower) | norm * (1 - limfrac) (upper); unit weights:
    // cumsum = 1, 2, ..., n, so the index is ceil(target) - 1
    auto order = [n](double target) {
        long long k = (long long)std::ceil(target) - 1;
        return (int)std::min(std::max(k, 0ll), n - 1);
    };
    a.k_lo = order((double)n * limfrac);
    a.k_hi = order((double)n * (1.0 - limfrac));
    HIP_TRY(h, mcmc_hip_launch_ckpt_bounds(&a, h->G, h->stream));
    mcmc::CkptBoundsReduceArgs r{};
    r.bounds = B.bounds.p; r.shift = h->dshift.p; r.payload = B.payload.p; r.d = h->d; r.G = h->G;
    HIP_TRY(h, mcmc_hip_launch_ckpt_bounds_reduce(&r, h->stream));
    const size_t np_ = 1 + 4 * (size_t)h->d, nb = (size_t)h->G * h->d * 2;
    if (h->comm)     // std over the chains of ALL ranks (mcmc.py:957 `mpi.gather(bound)`): one all-reduce
        if (int rc = mcmc_comm_allreduce_on_stream(h->comm, B.payload.p, np_, 0, h->stream))
            return fail(h, rc, "%s", mcmc_comm_error(h->comm));
    HIP_TRY(h, hipMemcpyAsync(B.pin, B.payload.p, sizeof(double) * np_, hipMemcpyDeviceToHost, h->stream));
    if (bounds)
        HIP_TRY(h, hipMemcpyAsync(B.pin + np_, B.bounds.p, sizeof(double) * nb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::copy(B.pin, B.pin + np_, stats);
    if (bounds) std::copy(B.pin + np_, B.pin + np_ + nb, bounds);
    return MCMC_HIP_OK;
}

int mcmc_hip_set_comm(mcmc_hip_ctx* h, mcmc_hip_comm* c)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (c && mcmc_comm_device(c) != h->cfg.device)
        return fail(h, MCMC_HIP_ERR_ARG, "the communicator lives on device %d, the engine on device %d",
                    mcmc_comm_device(c), h->cfg.device);
    if (h->ck.begun) return fail(h, MCMC_HIP_ERR_STATE, "a device checkpoint is in flight");
    h->comm = c;
    return MCMC_HIP_OK;
}

}  // extern "C"
