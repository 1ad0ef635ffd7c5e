// libmcmc_hip.so: the weighted sums of importance reweighting (importance_kernels.hip).  The CALLER
// owns the log-weights delta[n_alt][W]: it fills them on the engine's stream from the state as it lies
// in HBM (mcmc_hip_importance_layout hands out the pointer of x) and passes their device pointer to
// accumulate.  The life cycle is the Readout's (readout.h); a request may leave the interval open
// (close = 0).  The centring constants c are taken ON THE DEVICE by the first accumulation of an interval.
// The reweighted marginal histograms (importance_hist_kernels.hip; mcmc_hip_importance_hist_*) are a
// second slab with the same intervals: one request copies out (and closes) both.
#include "ctx.h"

namespace {

size_t im_n_groups(const mcmc_hip_ctx* h) { return (size_t)h->imp.n_alt * h->imp.G; }

mcmc::ImArgs im_args(mcmc_hip_ctx* h, const double* delta)
{
    auto& F = h->imp;
    mcmc::ImArgs a{};
    a.x = h->x.p; a.shift = h->dshift.p; a.delta = delta;
    a.sums = F.ro.dev<double>();
    a.n = F.ro.dev() + F.n_sums;
    a.counters = a.n + im_n_groups(h);
    a.ckey = a.counters + 3 * (size_t)F.n_alt;
    for (int k = 0; k < mcmc::kImMaxAlt; ++k) { a.off[k] = F.off[k]; a.cov[k] = F.cov[k]; }
    a.W = h->W; a.d = h->d; a.gs = F.gs; a.G = F.G; a.n_alt = F.n_alt;
    return a;
}

// the slab of n_alt alternatives over groups of gs walkers, zeroed
int im_resize_groups(mcmc_hip_ctx* h, int gs)
{
    auto& F = h->imp;
    F.gs = gs;
    F.G = h->W / gs;
    size_t at = 0;
    for (int k = 0; k < mcmc::kImMaxAlt; ++k) {
        F.off[k] = at;
        if (k < F.n_alt) at += (size_t)F.G * mcmc::im_n_chains(h->d, F.cov[k]);
    }
    F.n_sums = at;
    HIP_TRY_BUILD(h, F, F.ro.alloc(F.n_sums + im_n_groups(h) + 4 * (size_t)F.n_alt, h->stream));
    return MCMC_HIP_OK;
}

// the words of the histogram slab: lo | hi per histogram set, then saturated[n_hist]
size_t imh_n_words(const mcmc_hip_ctx* h) { return (size_t)h->imp.n_hist * (2 * h->imp.n_counters + 1); }

mcmc::ImHistArgs imh_args(mcmc_hip_ctx* h, const mcmc::ImArgs& im)
{
    auto& F = h->imp;
    mcmc::ImHistArgs a{};
    a.x = h->x.p; a.z = h->dv.z.p; a.entries = h->mg.entries.p;
    a.delta = im.delta; a.ckey = im.ckey;
    a.q = F.q.p;
    a.slab = F.hist.dev();
    a.saturated = a.slab + (size_t)F.n_hist * 2 * F.n_counters;
    a.n_counters = F.n_counters;
    for (int k = 0; k < mcmc::kImMaxAlt; ++k) a.alt[k] = F.hist_alt[k];
    a.W = h->W; a.d = h->d; a.n_entries = h->mg.n_entries; a.n_hist = F.n_hist;
    // the slices of marginals_accumulate, with the histogram sets counted in: the sums do not depend on it
    int slice = mcmc::kImHistMaxSlice;
    while (slice > 1024 && (long long)F.n_hist * a.n_entries * ((h->W + slice - 1) / slice) < 512) slice /= 2;
    a.slice = slice;
    a.n_slices = (h->W + slice - 1) / slice;
    return a;
}

int imh_sizes_ok(mcmc_hip_ctx* h, const char* what, const void* lo, const void* hi, const void* saturated, int64_t n)
{
    const auto& F = h->imp;
    const char* name = !lo ? "lo" : !hi ? "hi" : !saturated ? "saturated" : nullptr;
    if (name) return fail(h, MCMC_HIP_ERR_ARG, "%s: %s is null", what, name);
    if ((size_t)n != (size_t)F.n_hist * F.n_counters)
        return fail(h, MCMC_HIP_ERR_ARG, "%s: %d histogram sets of %zu counters hold %zu words each way, not %lld", what,
                    F.n_hist, F.n_counters, (size_t)F.n_hist * F.n_counters, (long long)n);
    return MCMC_HIP_OK;
}

int im_sizes_ok(mcmc_hip_ctx* h, const char* what, const void* sums, const void* n, const void* counters,
                const void* c, int64_t n_sums, int64_t n_groups)
{
    const auto& F = h->imp;
    const char* name = !sums ? "sums" : !n ? "n" : !counters ? "counters" : !c ? "c" : nullptr;
    if (name) return fail(h, MCMC_HIP_ERR_ARG, "%s: %s is null", what, name);
    if ((size_t)n_sums != F.n_sums || (size_t)n_groups != im_n_groups(h))
        return fail(h, MCMC_HIP_ERR_ARG, "%s: sums holds %zu values and n %zu, not %lld and %lld", what, F.n_sums,
                    im_n_groups(h), (long long)n_sums, (long long)n_groups);
    return MCMC_HIP_OK;
}

}  // namespace

extern "C" {

int mcmc_hip_importance_configure(mcmc_hip_ctx* h, int32_t n_alt, const int32_t* cov)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n_alt < 0 || n_alt > mcmc::kImMaxAlt)
        return fail(h, MCMC_HIP_ERR_ARG, "n_alt = %d must lie in 0..%d", n_alt, mcmc::kImMaxAlt);
    if (n_alt > 0 && !cov) return fail(h, MCMC_HIP_ERR_ARG, "cov is null");
    if (n_alt > 0 && h->d > mcmc::kImMaxDim)
        return fail(h, MCMC_HIP_ERR_ARG, "d = %d: the importance kernel serves d <= %d", h->d, mcmc::kImMaxDim);
    for (int k = 0; k < n_alt; ++k)
        if (cov[k] && h->d > mcmc::kImMaxCovDim)
            return fail(h, MCMC_HIP_ERR_ARG, "cov[%d] at d = %d: the covariance is kept for d <= %d", k, h->d,
                        mcmc::kImMaxCovDim);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& F = h->imp;
    F.release();
    if (n_alt == 0) return MCMC_HIP_OK;
    F.n_alt = n_alt;
    for (int k = 0; k < mcmc::kImMaxAlt; ++k) F.cov[k] = k < n_alt && cov[k] ? 1 : 0;
    return im_resize_groups(h, h->gs);
}

int mcmc_hip_importance_set_group_size(mcmc_hip_ctx* h, int32_t group_size)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_configure must precede importance_set_group_size");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an importance request is pending (fetch it first)");
    if (group_size < 1 || h->W % group_size)
        return fail(h, MCMC_HIP_ERR_ARG, "group_size = %d must divide n_walkers = %d", group_size, h->W);
    if (F.hist.pending)
        return fail(h, MCMC_HIP_ERR_STATE, "an importance histogram read-out is pending (fetch it first)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // (what empties the sums empties the histograms: they share the interval)
    if (F.hist.on()) HIP_TRY(h, hipMemsetAsync(F.hist.slab, 0, F.hist.bytes(), h->stream));
    return im_resize_groups(h, group_size);
}

int mcmc_hip_importance_layout(const mcmc_hip_ctx* h, int32_t* n_alt, int32_t* n_groups, int64_t* n_sums,
                               int64_t* offsets, int32_t* cov, int64_t* n_accumulations, uint64_t* x_device_ptr)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& F = h->imp;
    if (n_alt) *n_alt = F.n_alt;
    if (n_groups) *n_groups = F.ro.on() ? F.G : 0;
    if (n_sums) *n_sums = (int64_t)F.n_sums;
    for (int k = 0; k < mcmc::kImMaxAlt; ++k) {
        if (offsets) offsets[k] = k < F.n_alt ? (int64_t)F.off[k] : 0;
        if (cov) cov[k] = k < F.n_alt ? F.cov[k] : 0;
    }
    if (n_accumulations) *n_accumulations = F.ro.n_acc;
    if (x_device_ptr) *x_device_ptr = (uint64_t)(uintptr_t)h->x.p;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_accumulate(mcmc_hip_ctx* h, uint64_t delta_device_ptr)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_configure must precede importance_accumulate");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    if (!delta_device_ptr || delta_device_ptr % sizeof(double))
        return fail(h, MCMC_HIP_ERR_ARG, "delta_device_ptr = %llu is not the device pointer of doubles",
                    (unsigned long long)delta_device_ptr);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const mcmc::ImArgs a = im_args(h, (const double*)(uintptr_t)delta_device_ptr);
    if (F.ro.n_acc == 0) HIP_TRY(h, mcmc_hip_launch_importance_max(&a, h->stream));   // the interval opens
    if (F.hist.on()) {   // the reweighted histograms: behind the maximum, whose key of c they read
        if (!h->mg.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "the marginals the importance histograms follow are gone");
        const mcmc::ImHistArgs ha = imh_args(h, a);
        HIP_TRY(h, mcmc_hip_launch_importance_hist_weights(&ha, h->stream));
        HIP_TRY(h, mcmc_hip_launch_importance_hist(&ha, h->mg.lds_words, h->stream));
    }
    HIP_TRY(h, mcmc_hip_launch_importance(&a, h->stream));
    F.ro.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_request(mcmc_hip_ctx* h, int32_t close)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_configure must precede importance_request");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an importance request is already pending");
    if (F.hist.pending)
        return fail(h, MCMC_HIP_ERR_STATE, "an importance histogram read-out is pending (fetch it first)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (F.hist.on()) {   // both slabs leave, and close, in the same call: neither closes without the other
        F.hist.n_acc = F.ro.n_acc;
        HIP_TRY(h, F.hist.copy_out(h->stream, close ? F.hist.n_words : 0));
    }
    HIP_TRY(h, F.ro.copy_out(h->stream, close ? F.ro.n_words : 0));
    HIP_TRY(h, F.ro.mark(h->stream));
    F.hist.pending = F.hist.on();   // (behind the same event)
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_fetch(mcmc_hip_ctx* h, double* sums, int64_t n_sums, uint64_t* n, int64_t n_groups,
                              uint64_t* counters, double* c, int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no importance request is pending");
    if (int rc = im_sizes_ok(h, "importance_fetch", sums, n, counters, c, n_sums, n_groups)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, F.ro.wait());
    const size_t ng = im_n_groups(h);
    const unsigned long long* words = F.ro.host();
    std::memcpy(sums, words, sizeof(double) * F.n_sums);
    std::memcpy(n, words + F.n_sums, sizeof(uint64_t) * ng);
    std::memcpy(counters, words + F.n_sums + ng, sizeof(uint64_t) * 3 * F.n_alt);
    for (int k = 0; k < F.n_alt; ++k) c[k] = mcmc::im_value(words[F.n_sums + ng + 3 * (size_t)F.n_alt + k]);
    if (n_accumulations) *n_accumulations = F.ro.pend_n;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_set(mcmc_hip_ctx* h, const double* sums, int64_t n_sums, const uint64_t* n,
                            int64_t n_groups, const uint64_t* counters, const double* c, int64_t n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_configure must precede importance_set");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an importance request is pending (fetch it first)");
    if (int rc = im_sizes_ok(h, "importance_set", sums, n, counters, c, n_sums, n_groups)) return rc;
    if (n_accumulations < 0)
        return fail(h, MCMC_HIP_ERR_ARG, "n_accumulations = %lld must be >= 0", (long long)n_accumulations);
    for (int k = 0; k < F.n_alt; ++k)
        if (!std::isfinite(c[k])) return fail(h, MCMC_HIP_ERR_ARG, "c[%d] = %g is not finite", k, c[k]);
    const size_t ng = im_n_groups(h);
    std::vector<unsigned long long> words(F.ro.n_words, 0ull);
    std::memcpy(words.data(), sums, sizeof(double) * F.n_sums);
    std::memcpy(words.data() + F.n_sums, n, sizeof(uint64_t) * ng);
    std::memcpy(words.data() + F.n_sums + ng, counters, sizeof(uint64_t) * 3 * F.n_alt);
    // (c = 0.0 of an interval without a finite log-weight goes back as the key of 0.0: the same value)
    for (int k = 0; k < F.n_alt; ++k) words[F.n_sums + ng + 3 * (size_t)F.n_alt + k] = mcmc::im_key(c[k]);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, F.ro.upload(words.data()));
    F.ro.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_hist_configure(mcmc_hip_ctx* h, const int32_t* on)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_configure must precede importance_hist_configure");
    if (!h->mg.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "marginals_configure must precede importance_hist_configure");
    if (F.ro.pending || F.hist.pending)
        return fail(h, MCMC_HIP_ERR_STATE, "an importance request is pending (fetch it first)");
    if (!on) return fail(h, MCMC_HIP_ERR_ARG, "on is null");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    F.release_hist();
    int n_hist = 0;
    for (int k = 0; k < F.n_alt; ++k)
        if (on[k]) {
            F.hist_on[k] = 1;
            F.hist_alt[n_hist++] = k;
        }
    if (n_hist == 0) return MCMC_HIP_OK;
    F.n_hist = n_hist;
    F.n_counters = h->mg.ro.n_words;
    auto undo = [&] { F.release_hist(); };
    HIP_TRY_ELSE(h, F.hist.alloc(imh_n_words(h), h->stream), undo());
    HIP_TRY_ELSE(h, F.q.resize((size_t)n_hist * h->W), undo());
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_hist_layout(const mcmc_hip_ctx* h, int32_t* n_hist, int32_t* on, int64_t* n_counters,
                                    int64_t* n_words)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& F = h->imp;
    if (n_hist) *n_hist = F.n_hist;
    if (on)
        for (int k = 0; k < mcmc::kImMaxAlt; ++k) on[k] = F.hist_on[k];
    if (n_counters) *n_counters = (int64_t)F.n_counters;
    if (n_words) *n_words = (int64_t)F.hist.n_words;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_hist_fetch(mcmc_hip_ctx* h, uint64_t* lo, uint64_t* hi, int64_t n, uint64_t* saturated,
                                   int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.hist.pending) return fail(h, MCMC_HIP_ERR_STATE, "no importance histogram read-out is pending");
    if (int rc = imh_sizes_ok(h, "importance_hist_fetch", lo, hi, saturated, n)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(F.ro.ev));   // (the request's one event, behind both copies)
    F.hist.pending = false;
    const unsigned long long* words = F.hist.host();
    const size_t nc = F.n_counters;
    for (int q = 0; q < F.n_hist; ++q) {
        std::memcpy(lo + q * nc, words + 2 * q * nc, sizeof(uint64_t) * nc);
        std::memcpy(hi + q * nc, words + (2 * q + 1) * nc, sizeof(uint64_t) * nc);
    }
    std::memcpy(saturated, words + 2 * (size_t)F.n_hist * nc, sizeof(uint64_t) * F.n_hist);
    if (n_accumulations) *n_accumulations = F.hist.pend_n;
    return MCMC_HIP_OK;
}

int mcmc_hip_importance_hist_set(mcmc_hip_ctx* h, const uint64_t* lo, const uint64_t* hi, int64_t n,
                                 const uint64_t* saturated)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->imp;
    if (!F.hist.on()) return fail(h, MCMC_HIP_ERR_STATE, "importance_hist_configure must precede importance_hist_set");
    if (F.ro.pending || F.hist.pending)
        return fail(h, MCMC_HIP_ERR_STATE, "an importance request is pending (fetch it first)");
    if (int rc = imh_sizes_ok(h, "importance_hist_set", lo, hi, saturated, n)) return rc;
    const size_t nc = F.n_counters;
    std::vector<unsigned long long> words(F.hist.n_words, 0ull);
    for (int q = 0; q < F.n_hist; ++q) {
        std::memcpy(words.data() + 2 * q * nc, lo + q * nc, sizeof(uint64_t) * nc);
        std::memcpy(words.data() + (2 * q + 1) * nc, hi + q * nc, sizeof(uint64_t) * nc);
    }
    std::memcpy(words.data() + 2 * (size_t)F.n_hist * nc, saturated, sizeof(uint64_t) * F.n_hist);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, F.hist.upload(words.data()));
    return MCMC_HIP_OK;
}

}  // extern "C"
