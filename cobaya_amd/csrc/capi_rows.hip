// libmcmc_hip.so: the rows the step kernels emit (emit_capacity > 0) -- draining them to the
// host and thinning them on the device.
#include "ctx.h"

extern "C" {

int mcmc_hip_drain_samples(mcmc_hip_ctx* h, double* rows, int64_t cap_rows, int64_t* n_rows)
{
    if (!h || !n_rows) return MCMC_HIP_ERR_ARG;
    *n_rows = 0;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    if (h->cfg.emit_capacity <= 0) return MCMC_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, d = h->d, cap = h->cfg.emit_capacity;
    std::vector<int> nr(W);
    HIP_TRY(h, hipMemcpy(nr.data(), h->nrows.p, sizeof(int) * W, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (size_t w = 0; w < W; ++w) total += std::min<int>(nr[w], (int)cap);
    *n_rows = total;
    if (!rows) return MCMC_HIP_OK;  // size query
    if (cap_rows < total)
        return fail(h, MCMC_HIP_ERR_ARG, "drain buffer holds %lld rows, %lld are pending",
                    (long long)cap_rows, (long long)total);
    // pack on the device, then move only the rows that exist (they are ~ acceptance x steps
    // of the buffer) straight into the caller's array
    std::vector<long long> off(W);
    long long run = 0;
    for (size_t w = 0; w < W; ++w) { off[w] = run; run += std::min<int>(nr[w], (int)cap); }
    if (total > 0) {
        HIP_TRY(h, h->pack_off.resize(W));
        HIP_TRY(h, h->pack_out.resize(std::min<size_t>(W * cap, (size_t)total + (size_t)total / 4 + 1024) * (d + 5)));
        HIP_TRY(h, hipMemcpyAsync(h->pack_off.p, off.data(), sizeof(long long) * W,
                                  hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, mcmc_hip_launch_pack_rows(h->rows.p, h->nrows.p, h->pack_off.p, h->pack_out.p,
                                             (int)W, (int)cap, (int)d, h->cfg.walker_offset,
                                             h->stream));
        HIP_TRY(h, hipMemcpyAsync(rows, h->pack_out.p, sizeof(double) * (size_t)total * (d + 5),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    HIP_TRY(h, hipMemset(h->nrows.p, 0, sizeof(int) * W));
    return MCMC_HIP_OK;
}

// Thinned emission on the device (round 5; collection.py:1373-1383, OneSamplePoint.add_to_collection
// with output_thin > 1): every incremental Metropolis kernel that emits rows (round 6) -- the
// from-scratch and dragging kernels refuse at their first step, and the caller thins on the host.
int mcmc_hip_set_emit_thin(mcmc_hip_ctx* h, int32_t thin)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (thin < 1) return fail(h, MCMC_HIP_ERR_ARG, "thin must be >= 1");
    if (thin > 1 && h->cfg.emit_capacity <= 0)
        return fail(h, MCMC_HIP_ERR_ARG, "emit_thin needs emitted rows (emit_capacity > 0)");
    if (thin > 1) {   // (the configuration as it stands now; mcmc_hip_step checks again)
        const bool ok = inc_choice_of(h).thins_on_device;
        if (!ok)
            return fail(h, MCMC_HIP_ERR_ARG,
                        "emit_thin: rows are thinned on the device by the incremental kernels (Gaussian "
                        "mixtures with Metropolis steps: step_inc_kernel<.., emit> for one mode, the "
                        "general incremental kernels for mixtures, periodic parameters and blocks of "
                        "one parameter); thin on the host");
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (thin > 1 && !h->thin_acc.p) HIP_TRY(h, h->thin_acc.resize((size_t)h->W));
    // remainders are in units of the factor they were added up under: a new factor starts from zero
    if (thin > 1 && thin != h->emit_thin)
        HIP_TRY(h, hipMemsetAsync(h->thin_acc.p, 0, sizeof(int) * (size_t)h->W, h->stream));
    h->emit_thin = thin;
    return MCMC_HIP_OK;
}

int mcmc_hip_get_thin_carry(mcmc_hip_ctx* h, int32_t* carry)
{
    if (!h || !carry) return MCMC_HIP_ERR_ARG;
    if (!h->thin_acc.p) return fail(h, MCMC_HIP_ERR_STATE, "emit_thin is not set");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(carry, h->thin_acc.p, sizeof(int) * (size_t)h->W, hipMemcpyDeviceToHost));
    return MCMC_HIP_OK;
}

int mcmc_hip_set_thin_carry(mcmc_hip_ctx* h, const int32_t* carry)
{
    if (!h || !carry) return MCMC_HIP_ERR_ARG;
    if (!h->thin_acc.p) return fail(h, MCMC_HIP_ERR_STATE, "emit_thin is not set");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->thin_acc.p, carry, sizeof(int) * (size_t)h->W, hipMemcpyHostToDevice));
    return MCMC_HIP_OK;
}

int mcmc_hip_set_drain_slots(mcmc_hip_ctx* h, int32_t n_slots)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n_slots < 2 || n_slots > 64) return fail(h, MCMC_HIP_ERR_ARG, "n_slots must be in 2..64");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (auto& sl : h->slots)
        if (sl.p) (void)hipHostFree(sl.p);
    h->slots.assign((size_t)n_slots, mcmc_hip_ctx::HostSlot{});
    h->slot_next = 0;
    return MCMC_HIP_OK;
}

int mcmc_hip_drain_samples_pinned(mcmc_hip_ctx* h, const double** rows, int64_t* n_rows)
{
    if (!h || !rows || !n_rows) return MCMC_HIP_ERR_ARG;
    *rows = nullptr;
    *n_rows = 0;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    if (h->cfg.emit_capacity <= 0) return MCMC_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t W = h->W, d = h->d, cap = h->cfg.emit_capacity;
    std::vector<int> nr(W);
    HIP_TRY(h, hipMemcpy(nr.data(), h->nrows.p, sizeof(int) * W, hipMemcpyDeviceToHost));
    std::vector<long long> off(W);
    long long total = 0;
    for (size_t w = 0; w < W; ++w) { off[w] = total; total += std::min<int>(nr[w], (int)cap); }
    auto& sl = h->slots[(size_t)h->slot_next];
    h->slot_next = (h->slot_next + 1) % (int)h->slots.size();
    if (total > 0) {
        if ((size_t)total > sl.cap_rows) {   // (grown with headroom: pinning memory is slow)
            if (sl.p) (void)hipHostFree(sl.p);
            sl.p = nullptr;
            sl.cap_rows = 0;
            const size_t want = std::min<size_t>(W * cap, (size_t)total + (size_t)total / 4 + 1024);
            HIP_TRY(h, hipHostMalloc((void**)&sl.p, sizeof(double) * want * (d + 5), hipHostMallocDefault));
            sl.cap_rows = want;
        }
        HIP_TRY(h, h->pack_off.resize(W));
        // (the packed rows that exist: ~ acceptance x steps of the device buffer; sized to what
        // is there, with headroom, since the device buffer itself may be many GiB)
        HIP_TRY(h, h->pack_out.resize(std::min<size_t>(W * cap, (size_t)total + (size_t)total / 4 + 1024) * (d + 5)));
        HIP_TRY(h, hipMemcpyAsync(h->pack_off.p, off.data(), sizeof(long long) * W,
                                  hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, mcmc_hip_launch_pack_rows(h->rows.p, h->nrows.p, h->pack_off.p, h->pack_out.p,
                                             (int)W, (int)cap, (int)d, h->cfg.walker_offset,
                                             h->stream));
        HIP_TRY(h, hipMemcpyAsync(sl.p, h->pack_out.p, sizeof(double) * (size_t)total * (d + 5),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->nrows.p, 0, sizeof(int) * W, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        *rows = sl.p;
    } else {
        HIP_TRY(h, hipMemset(h->nrows.p, 0, sizeof(int) * W));
    }
    *n_rows = total;
    return MCMC_HIP_OK;
}

}  // extern "C"
