// libmcmc_hip.so: the sums of the ellipsoid-truncated harmonic mean (evidence_kernels.hip).  The
// life cycle is the Readout's (readout.h); a request may leave the interval open (close = 0), and a
// closing one keeps the slab's last word, c.  What is new here is the
// ellipsoid: handed in as (m, cov), factorised on the host, and -- after the first -- only STAGED
// until a closing request activates it in stream order, so that no interval mixes two ellipsoids.
#include "ctx.h"
#include "host_linalg.h"

namespace {

size_t ev_n(const mcmc_hip_ctx* h) { return (size_t)h->G * h->evd.n_r; }
size_t ev_n_ell(const mcmc_hip_ctx* h) { return (size_t)h->d * (h->d + 1) + 1; }

mcmc::EvArgs ev_args(mcmc_hip_ctx* h)
{
    auto& F = h->evd;
    const size_t n = ev_n(h), d = h->d;
    mcmc::EvArgs a{};
    a.x = h->x.p; a.logpost = h->logpost.p;
    a.m = F.ell.p; a.Linv = F.ell.p + d;
    a.s = F.s.p;
    a.acc = F.ro.dev<double>();
    a.cnt = F.ro.dev() + n;
    a.clamped = F.ro.dev() + 2 * n;
    a.ckey = F.ro.dev() + 2 * n + 1;
    for (int r = 0; r < mcmc::kEvMaxRadii; ++r) a.r2[r] = F.r2[r];
    a.W = h->W; a.d = h->d; a.gs = h->gs; a.G = h->G; a.n_r = F.n_r;
    return a;
}

// `ell` (m | Linv) -> the device, then c = the maximum of logpost, all in stream order.  The pinned
// slot is free: whoever used it last was waited for (the event of a closing request, or a
// synchronised stream)
int ev_activate(mcmc_hip_ctx* h, const std::vector<double>& ell)
{
    auto& F = h->evd;
    const size_t n = (size_t)h->d * (h->d + 1);
    std::copy(ell.begin(), ell.begin() + n, F.pin_ell);
    HIP_TRY(h, hipMemcpyAsync(F.ell.p, F.pin_ell, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    const mcmc::EvArgs a = ev_args(h);
    HIP_TRY(h, mcmc_hip_launch_evidence_max(&a, h->stream));
    return MCMC_HIP_OK;
}

int ev_sizes_ok(mcmc_hip_ctx* h, const char* what, const void* sums, const void* counts, int64_t n, int64_t n_ell)
{
    if (!sums || !counts || (size_t)n != ev_n(h))
        return fail(h, MCMC_HIP_ERR_ARG, "%s: sums and counts hold %zu values each, not %lld", what, ev_n(h),
                    (long long)n);
    if ((size_t)n_ell != ev_n_ell(h))
        return fail(h, MCMC_HIP_ERR_ARG, "%s: an ellipsoid holds n_ell = %zu doubles, not %lld", what, ev_n_ell(h),
                    (long long)n_ell);
    return MCMC_HIP_OK;
}

}  // namespace

extern "C" {

int mcmc_hip_evidence_configure(mcmc_hip_ctx* h, int32_t n_radii, const double* r2)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n_radii < 0 || n_radii > mcmc::kEvMaxRadii)
        return fail(h, MCMC_HIP_ERR_ARG, "n_radii = %d must lie in 0..%d", n_radii, mcmc::kEvMaxRadii);
    if (n_radii > 0 && !r2) return fail(h, MCMC_HIP_ERR_ARG, "r2 is null");
    for (int r = 0; r < n_radii; ++r)
        if (!(std::isfinite(r2[r]) && r2[r] > 0.0 && (r == 0 || r2[r] > r2[r - 1])))
            return fail(h, MCMC_HIP_ERR_ARG, "r2[%d] = %g: the radii must be finite, positive and ascending", r, r2[r]);
    if (n_radii > 0 && h->d > mcmc::kEvMaxDim)
        return fail(h, MCMC_HIP_ERR_ARG, "d = %d: the evidence kernel serves d <= %d", h->d, mcmc::kEvMaxDim);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto& F = h->evd;
    F.release();
    if (n_radii == 0) return MCMC_HIP_OK;
    F.n_r = n_radii;
    for (int r = 0; r < mcmc::kEvMaxRadii; ++r) F.r2[r] = r < n_radii ? r2[r] : 0.0;
    const size_t n = ev_n(h), d = h->d;
    HIP_TRY_BUILD(h, F, F.ro.alloc(2 * n + 2, h->stream));
    HIP_TRY_BUILD(h, F, F.ell.resize(d * (d + 1)));
    HIP_TRY_BUILD(h, F, F.s.resize((size_t)h->W));
    HIP_TRY_BUILD(h, F, hipHostMalloc((void**)&F.pin_ell, sizeof(double) * d * (d + 1), hipHostMallocDefault));
    HIP_TRY_BUILD(h, F, hipMemsetAsync(F.ell.p, 0, sizeof(double) * d * (d + 1), h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_layout(const mcmc_hip_ctx* h, int32_t* on, int32_t* n_radii, int32_t* n_groups,
                             int64_t* n_ell, int32_t* has_active, int32_t* has_staged, int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& F = h->evd;
    if (on) *on = F.ro.on() ? 1 : 0;
    if (n_radii) *n_radii = F.n_r;
    if (n_groups) *n_groups = F.ro.on() ? h->G : 0;
    if (n_ell) *n_ell = F.ro.on() ? (int64_t)ev_n_ell(h) : 0;
    if (has_active) *has_active = F.active.empty() ? 0 : 1;
    if (has_staged) *has_staged = F.staged.empty() ? 0 : 1;
    if (n_accumulations) *n_accumulations = F.ro.n_acc;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_set_ellipsoid(mcmc_hip_ctx* h, const double* m, const double* cov)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_set_ellipsoid");
    if (!m || !cov) return fail(h, MCMC_HIP_ERR_ARG, "%s is null", !m ? "m" : "cov");
    const int d = h->d;
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(m[i])) return fail(h, MCMC_HIP_ERR_ARG, "m[%d] = %g is not finite", i, m[i]);
    std::vector<double> L((size_t)d * d), ell((size_t)d * (d + 1));
    if (!is_symmetric(d, cov) || !cholesky_lower(d, cov, L.data()))
        return fail(h, MCMC_HIP_ERR_NOT_PD, "cov is not a symmetric positive-definite matrix");
    std::copy(m, m + d, ell.begin());
    tri_inverse_lower(d, L.data(), ell.data() + d);
    for (size_t k = 0; k < ell.size(); ++k)
        if (!std::isfinite(ell[k])) return fail(h, MCMC_HIP_ERR_NOT_PD, "the inverse of chol(cov) is not finite");
    if (!F.active.empty()) {   // staged: the next closing request activates it
        F.staged = std::move(ell);
        return MCMC_HIP_OK;
    }
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state: the first ellipsoid takes c from logpost");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = ev_activate(h, ell)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    F.active = std::move(ell);
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_accumulate(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_accumulate");
    if (F.active.empty()) return fail(h, MCMC_HIP_ERR_STATE, "no ellipsoid is active: call evidence_set_ellipsoid first");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const mcmc::EvArgs a = ev_args(h);
    HIP_TRY(h, mcmc_hip_launch_evidence(&a, h->stream));
    F.ro.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_request(mcmc_hip_ctx* h, int32_t close)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_request");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an evidence request is already pending");
    if (close && !F.staged.empty() && !h->have_state)
        return fail(h, MCMC_HIP_ERR_STATE, "no state: the staged ellipsoid takes c from logpost");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, F.ro.copy_out(h->stream, close ? F.ro.n_words - 1 : 0));   // (c stays)
    F.pend_active = F.active;
    F.pend_staged = F.staged;
    if (close && !F.staged.empty()) {
        if (int rc = ev_activate(h, F.staged)) return rc;
        F.active = std::move(F.staged);
        F.staged.clear();
    }
    HIP_TRY(h, F.ro.mark(h->stream));   // (last: a fetch also vouches for the pinned ellipsoid)
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_fetch(mcmc_hip_ctx* h, double* sums, uint64_t* counts, int64_t n, uint64_t* clamped,
                            int64_t* n_accumulations, double* active, double* staged, int64_t n_ell,
                            int32_t* has_active, int32_t* has_staged)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no evidence request is pending");
    if (int rc = ev_sizes_ok(h, "evidence_fetch", sums, counts, n, n_ell)) return rc;
    if (!active || !staged) return fail(h, MCMC_HIP_ERR_ARG, "%s is null", !active ? "active" : "staged");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, F.ro.wait());
    const size_t k = ev_n(h);
    const unsigned long long* words = F.ro.host();
    std::copy(F.ro.host<double>(), F.ro.host<double>() + k, sums);
    std::copy(words + k, words + 2 * k, counts);
    if (clamped) *clamped = words[2 * k];
    if (n_accumulations) *n_accumulations = F.ro.pend_n;
    std::fill(active, active + n_ell, 0.0);
    std::fill(staged, staged + n_ell, 0.0);
    if (!F.pend_active.empty()) {
        std::copy(F.pend_active.begin(), F.pend_active.end(), active);
        active[n_ell - 1] = mcmc::ev_value(words[2 * k + 1]);
    }
    if (!F.pend_staged.empty()) std::copy(F.pend_staged.begin(), F.pend_staged.end(), staged);
    if (has_active) *has_active = F.pend_active.empty() ? 0 : 1;
    if (has_staged) *has_staged = F.pend_staged.empty() ? 0 : 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_set(mcmc_hip_ctx* h, const double* sums, const uint64_t* counts, int64_t n, uint64_t clamped,
                          int64_t n_accumulations, const double* active, const double* staged, int64_t n_ell)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_set");
    if (F.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an evidence request is pending (fetch it first)");
    if (int rc = ev_sizes_ok(h, "evidence_set", sums, counts, n, n_ell)) return rc;
    if (n_accumulations < 0)
        return fail(h, MCMC_HIP_ERR_ARG, "n_accumulations = %lld must be >= 0", (long long)n_accumulations);
    if (!active && (staged || n_accumulations > 0))
        return fail(h, MCMC_HIP_ERR_ARG, "active is null: sums and a staged ellipsoid need an active one");
    for (const double* e : {active, staged})
        for (int64_t k = 0; e && k < n_ell; ++k)
            if (!std::isfinite(e[k]))
                return fail(h, MCMC_HIP_ERR_ARG, "%s[%lld] is not finite", e == active ? "active" : "staged", (long long)k);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t k = ev_n(h), ne = (size_t)n_ell - 1;
    std::vector<unsigned long long> words(F.ro.n_words, 0ull);
    std::memcpy(words.data(), sums, sizeof(double) * k);
    std::copy(counts, counts + k, words.begin() + k);
    words[2 * k] = clamped;
    words[2 * k + 1] = active ? mcmc::ev_key(active[ne]) : 0ull;
    HIP_TRY(h, F.ro.upload(words.data()));
    F.active.clear();
    F.staged.clear();
    if (active) {
        F.active.assign(active, active + ne);
        HIP_TRY(h, hipMemcpy(F.ell.p, active, sizeof(double) * ne, hipMemcpyHostToDevice));
    }
    if (staged) F.staged.assign(staged, staged + ne);
    F.ro.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

}  // extern "C"
