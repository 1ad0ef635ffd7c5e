// libmcmc_hip.so: streaming 1-D and 2-D marginal histograms of the ensemble (marginal_kernels.hip).
// The life cycle is the Readout's (readout.h).
#include "ctx.h"

namespace {

size_t marg_counters_1d(int bins1) { return (size_t)bins1 + 2; }
size_t marg_counters_2d(int bins2) { return (size_t)bins2 * bins2 + 1; }

}  // namespace

extern "C" {

int mcmc_hip_marginals_configure(mcmc_hip_ctx* h, int32_t n1, const int32_t* dims1, int32_t bins1,
                                 int32_t n2, const int32_t* pairs, int32_t bins2, const double* lo,
                                 const double* hi)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n1 < 0) return fail(h, MCMC_HIP_ERR_ARG, "n1 = %d must be >= 0", n1);
    if (n2 < 0) return fail(h, MCMC_HIP_ERR_ARG, "n2 = %d must be >= 0", n2);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n1 == 0 && n2 == 0) {
        h->mg.release();
        h->imp.release_hist();
        return MCMC_HIP_OK;
    }
    if (n1 > 0 && !dims1) return fail(h, MCMC_HIP_ERR_ARG, "dims1 is null");
    if (n2 > 0 && !pairs) return fail(h, MCMC_HIP_ERR_ARG, "pairs is null");
    if (!lo || !hi) return fail(h, MCMC_HIP_ERR_ARG, "%s is null", !lo ? "lo" : "hi");
    if (n1 > 0 && (bins1 < 1 || bins1 > mcmc::kMargMaxBins1))
        return fail(h, MCMC_HIP_ERR_ARG, "bins1 = %d must lie in 1..%d", bins1, mcmc::kMargMaxBins1);
    if (n2 > 0 && (bins2 < 1 || bins2 > mcmc::kMargMaxBins2))
        return fail(h, MCMC_HIP_ERR_ARG, "bins2 = %d must lie in 1..%d", bins2, mcmc::kMargMaxBins2);
    const int d = h->d + h->dv.m;   // (the derived rows follow the sampled parameters)
    auto range_ok = [&](int i, int B, const char* what, int k) {
        if (!(std::isfinite(lo[i]) && std::isfinite(hi[i]) && lo[i] < hi[i]))
            return fail(h, MCMC_HIP_ERR_ARG, "lo / hi of parameter %d (%s[%d]): [%g, %g] is not a finite range with lo < hi",
                        i, what, k, lo[i], hi[i]);
        if (!std::isfinite((double)B / (hi[i] - lo[i])))
            return fail(h, MCMC_HIP_ERR_ARG, "lo / hi of parameter %d (%s[%d]): the range [%g, %g] is too narrow for %d bins",
                        i, what, k, lo[i], hi[i], B);
        return (int)MCMC_HIP_OK;
    };
    for (int k = 0; k < n1; ++k) {
        if (dims1[k] < 0 || dims1[k] >= d)
            return fail(h, MCMC_HIP_ERR_ARG, "dims1[%d] = %d is not a parameter index (d = %d)", k, dims1[k], d);
        if (int rc = range_ok(dims1[k], bins1, "dims1", k)) return rc;
    }
    for (int k = 0; k < n2; ++k) {
        const int i = pairs[2 * k], j = pairs[2 * k + 1];
        if (i < 0 || i >= d || j < 0 || j >= d)
            return fail(h, MCMC_HIP_ERR_ARG, "pairs[%d] = (%d, %d) holds no parameter index (d = %d)", k, i, j, d);
        if (i == j) return fail(h, MCMC_HIP_ERR_ARG, "pairs[%d] = (%d, %d): a pair needs two different parameters", k, i, j);
        if (int rc = range_ok(i, bins2, "pairs", k)) return rc;
        if (int rc = range_ok(j, bins2, "pairs", k)) return rc;
    }
    auto& M = h->mg;
    M.release();
    h->imp.release_hist();   // (the reweighted histograms of the importance follow this layout)
    const size_t c1 = n1 ? marg_counters_1d(bins1) : 0, c2 = n2 ? marg_counters_2d(bins2) : 0;
    std::vector<mcmc::MargEntry> E((size_t)n1 + n2);
    for (int k = 0; k < n1; ++k) {
        const int i = dims1[k];
        mcmc::MargEntry& e = E[k];
        e = mcmc::MargEntry{};
        e.i = i; e.j = -1; e.B = bins1;
        e.lo_i = lo[i]; e.hi_i = hi[i]; e.s_i = (double)bins1 / (hi[i] - lo[i]);
        e.offset = (long long)(c1 * k);
    }
    for (int k = 0; k < n2; ++k) {
        const int i = pairs[2 * k], j = pairs[2 * k + 1];
        mcmc::MargEntry& e = E[(size_t)n1 + k];
        e = mcmc::MargEntry{};
        e.i = i; e.j = j; e.B = bins2;
        e.lo_i = lo[i]; e.hi_i = hi[i]; e.s_i = (double)bins2 / (hi[i] - lo[i]);
        e.lo_j = lo[j]; e.hi_j = hi[j]; e.s_j = (double)bins2 / (hi[j] - lo[j]);
        e.offset = (long long)(c1 * n1 + c2 * k);
    }
    const size_t n = c1 * n1 + c2 * n2;
    HIP_TRY_BUILD(h, M, M.ro.alloc(n, h->stream));
    HIP_TRY_BUILD(h, M, M.entries.resize(E.size()));
    HIP_TRY_BUILD(h, M, hipMemcpy(M.entries.p, E.data(), sizeof(mcmc::MargEntry) * E.size(), hipMemcpyHostToDevice));
    M.off_pairs = c1 * n1;
    M.n1 = n1; M.n2 = n2; M.bins1 = n1 ? bins1 : 0; M.bins2 = n2 ? bins2 : 0;
    M.n_entries = n1 + n2;
    M.lds_words = (int)std::max(c1, c2);
    return MCMC_HIP_OK;
}

int mcmc_hip_marginals_layout(const mcmc_hip_ctx* h, int64_t* n_counters, int32_t* n1, int32_t* bins1,
                              int32_t* n2, int32_t* bins2, int64_t* offset_pairs)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& M = h->mg;
    if (n_counters) *n_counters = (int64_t)M.ro.n_words;
    if (n1) *n1 = M.n1;
    if (bins1) *bins1 = M.bins1;
    if (n2) *n2 = M.n2;
    if (bins2) *bins2 = M.bins2;
    if (offset_pairs) *offset_pairs = (int64_t)M.off_pairs;
    return MCMC_HIP_OK;
}

int mcmc_hip_marginals_accumulate(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& M = h->mg;
    if (!M.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "marginals_configure must precede marginals_accumulate");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    mcmc::MargArgs a{};
    a.x = h->x.p; a.z = h->dv.z.p; a.d = h->d; a.entries = M.entries.p; a.slab = M.ro.dev(); a.W = h->W; a.n_entries = M.n_entries;
    // a slice of 4096 walkers (16 per thread) amortises the flush of the LDS histogram; with few
    // entries the slices shrink (to 1024) so that the launch still spreads over the chip.  The
    // counts do not depend on it.
    int slice = 4096;
    while (slice > 1024 && (long long)M.n_entries * ((h->W + slice - 1) / slice) < 512) slice /= 2;
    a.slice = slice;
    a.n_slices = (h->W + slice - 1) / slice;
    HIP_TRY(h, mcmc_hip_launch_marginals(&a, M.lds_words, h->stream));
    M.ro.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_marginals_request(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& M = h->mg;
    if (!M.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "marginals_configure must precede marginals_request");
    if (M.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a marginals request is already pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, M.ro.copy_out(h->stream, M.ro.n_words));
    HIP_TRY(h, M.ro.mark(h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_marginals_fetch(mcmc_hip_ctx* h, uint64_t* counts, int64_t n, int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& M = h->mg;
    if (!M.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no marginals request is pending");
    if (!counts || (size_t)n != M.ro.n_words)
        return fail(h, MCMC_HIP_ERR_ARG, "counts: the slab holds %zu counters, not %lld", M.ro.n_words, (long long)n);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, M.ro.wait());
    std::copy(M.ro.host(), M.ro.host() + M.ro.n_words, counts);
    if (n_accumulations) *n_accumulations = M.ro.pend_n;
    return MCMC_HIP_OK;
}

int mcmc_hip_marginals_set(mcmc_hip_ctx* h, const uint64_t* counts, int64_t n, int64_t n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& M = h->mg;
    if (!M.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "marginals_configure must precede marginals_set");
    if (M.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a marginals request is pending (fetch it first)");
    if (!counts || (size_t)n != M.ro.n_words)
        return fail(h, MCMC_HIP_ERR_ARG, "counts: the slab holds %zu counters, not %lld", M.ro.n_words, (long long)n);
    if (n_accumulations < 0) return fail(h, MCMC_HIP_ERR_ARG, "n_accumulations = %lld must be >= 0", (long long)n_accumulations);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, M.ro.upload(counts));
    M.ro.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

}  // extern "C"
