// libmcmc_hip.so: best fit, MAP and profile likelihoods of the ensemble (bestfit_kernels.hip).
// The life cycle is the Readout's (readout.h); its slab holds the keys and, behind them, the records.
#include "ctx.h"

namespace {

// walkers one workgroup reads: 4096 (16 per thread) amortise the flush of the LDS bins; with few
// entries the slices shrink (to 1024) so that the launch still spreads over the chip.  A maximum
// does not depend on it.
int bf_slice(const mcmc_hip_ctx* h)
{
    int slice = 4096;
    while (slice > 1024 && (long long)(h->bf.n + 1) * ((h->W + slice - 1) / slice) < 512) slice /= 2;
    return slice;
}

int bf_sizes_ok(mcmc_hip_ctx* h, const char* what, const void* slab, int64_t n_slab, const void* records,
                int64_t n_records)
{
    const auto& F = h->bf;
    if ((F.n_slab && !slab) || (size_t)n_slab != F.n_slab)
        return fail(h, MCMC_HIP_ERR_ARG, "%s: the slab holds %zu keys, not %lld", what, F.n_slab, (long long)n_slab);
    if (!records || (size_t)n_records != F.n_rec)
        return fail(h, MCMC_HIP_ERR_ARG, "%s: the records hold %zu words, not %lld", what, F.n_rec,
                    (long long)n_records);
    return MCMC_HIP_OK;
}

}  // namespace

extern "C" {

int mcmc_hip_bestfit_configure(mcmc_hip_ctx* h, int32_t n, const int32_t* dims, int32_t bins, const double* lo,
                               const double* hi, int32_t quantity)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n < 0) return fail(h, MCMC_HIP_ERR_ARG, "n = %d must be >= 0", n);
    if (quantity != MCMC_HIP_BESTFIT_LOGLIKE && quantity != MCMC_HIP_BESTFIT_LOGPOST)
        return fail(h, MCMC_HIP_ERR_ARG, "quantity = %d must be 0 (loglike) or 1 (logpost)", quantity);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n > 0 && !dims) return fail(h, MCMC_HIP_ERR_ARG, "dims is null");
    if (n > 0 && (!lo || !hi)) return fail(h, MCMC_HIP_ERR_ARG, "%s is null", !lo ? "lo" : "hi");
    if (n > 0 && (bins < 1 || bins > mcmc::kBfMaxBins))
        return fail(h, MCMC_HIP_ERR_ARG, "bins = %d must lie in 1..%d", bins, mcmc::kBfMaxBins);
    const int d = h->d;
    for (int k = 0; k < n; ++k) {
        const int i = dims[k];
        if (i < 0 || i >= d)
            return fail(h, MCMC_HIP_ERR_ARG, "dims[%d] = %d is not a parameter index (d = %d)", k, i, d);
        if (!(std::isfinite(lo[i]) && std::isfinite(hi[i]) && lo[i] < hi[i]))
            return fail(h, MCMC_HIP_ERR_ARG, "lo / hi of parameter %d (dims[%d]): [%g, %g] is not a finite range with lo < hi",
                        i, k, lo[i], hi[i]);
        if (!std::isfinite((double)bins / (hi[i] - lo[i])))
            return fail(h, MCMC_HIP_ERR_ARG, "lo / hi of parameter %d (dims[%d]): the range [%g, %g] is too narrow for %d bins",
                        i, k, lo[i], hi[i], bins);
    }
    auto& F = h->bf;
    F.release();
    std::vector<mcmc::BfEntry> E((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int i = dims[k];
        E[k] = mcmc::BfEntry{};
        E[k].i = i;
        E[k].lo = lo[i]; E[k].hi = hi[i]; E[k].s = (double)bins / (hi[i] - lo[i]);
    }
    const size_t n_slab = (size_t)n * (n ? bins : 0);
    const size_t n_rec = (size_t)mcmc::kBfRecords * (mcmc::kBfRecordHead + d);
    const size_t n_cand = (size_t)((h->W + 1023) / 1024) * mcmc::kBfRecords * 2;   // the most slices there can be
    HIP_TRY_BUILD(h, F, F.ro.alloc(n_slab + n_rec, h->stream));
    if (n) HIP_TRY_BUILD(h, F, F.entries.resize(E.size()));
    HIP_TRY_BUILD(h, F, F.cand.resize(n_cand));
    if (n) HIP_TRY_BUILD(h, F, hipMemcpy(F.entries.p, E.data(), sizeof(mcmc::BfEntry) * E.size(), hipMemcpyHostToDevice));
    HIP_TRY_BUILD(h, F, hipMemsetAsync(F.cand.p, 0, sizeof(unsigned long long) * n_cand, h->stream));
    F.n_slab = n_slab; F.n_rec = n_rec;
    F.n = n; F.bins = n ? bins : 0; F.quantity = quantity;
    return MCMC_HIP_OK;
}

int mcmc_hip_bestfit_layout(const mcmc_hip_ctx* h, int32_t* on, int32_t* n, int32_t* bins, int32_t* quantity,
                            int64_t* n_slab, int64_t* n_records)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& F = h->bf;
    if (on) *on = F.ro.on() ? 1 : 0;
    if (n) *n = F.n;
    if (bins) *bins = F.bins;
    if (quantity) *quantity = F.quantity;
    if (n_slab) *n_slab = (int64_t)F.n_slab;
    if (n_records) *n_records = (int64_t)F.n_rec;
    return MCMC_HIP_OK;
}

int mcmc_hip_bestfit_accumulate(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->bf;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "bestfit_configure must precede bestfit_accumulate");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    mcmc::BfArgs a{};
    a.x = h->x.p; a.logpost = h->logpost.p; a.logprior = h->logprior.p; a.loglike = h->loglike.p;
    a.value = F.quantity == MCMC_HIP_BESTFIT_LOGPOST ? h->logpost.p : h->loglike.p;
    a.entries = F.entries.p; a.slab = F.ro.dev(); a.cand = F.cand.p; a.records = F.ro.dev() + F.n_slab;
    a.step = h->step; a.walker0 = h->cfg.walker_offset;
    a.W = h->W; a.d = h->d; a.n_entries = F.n; a.B = F.bins;
    a.slice = bf_slice(h);
    a.n_slices = (h->W + a.slice - 1) / a.slice;
    HIP_TRY(h, mcmc_hip_launch_bestfit(&a, h->stream));
    HIP_TRY(h, mcmc_hip_launch_bestfit_commit(&a, h->stream));
    F.ro.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_bestfit_request(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->bf;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "bestfit_configure must precede bestfit_request");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a bestfit request is already pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, F.ro.copy_out(h->stream, F.ro.n_words));
    HIP_TRY(h, F.ro.mark(h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_bestfit_fetch(mcmc_hip_ctx* h, uint64_t* slab, int64_t n_slab, uint64_t* records, int64_t n_records,
                           int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->bf;
    if (!F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no bestfit request is pending");
    if (int rc = bf_sizes_ok(h, "bestfit_fetch", slab, n_slab, records, n_records)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, F.ro.wait());
    if (F.n_slab) std::copy(F.ro.host(), F.ro.host() + F.n_slab, slab);
    std::copy(F.ro.host() + F.n_slab, F.ro.host() + F.ro.n_words, records);
    if (n_accumulations) *n_accumulations = F.ro.pend_n;
    return MCMC_HIP_OK;
}

int mcmc_hip_bestfit_set(mcmc_hip_ctx* h, const uint64_t* slab, int64_t n_slab, const uint64_t* records,
                         int64_t n_records, int64_t n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->bf;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "bestfit_configure must precede bestfit_set");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a bestfit request is pending (fetch it first)");
    if (int rc = bf_sizes_ok(h, "bestfit_set", slab, n_slab, records, n_records)) return rc;
    if (n_accumulations < 0) return fail(h, MCMC_HIP_ERR_ARG, "n_accumulations = %lld must be >= 0", (long long)n_accumulations);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, F.ro.upload(slab, 0, F.n_slab));
    HIP_TRY(h, F.ro.upload(records, F.n_slab, F.n_rec));
    F.ro.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

}  // extern "C"
