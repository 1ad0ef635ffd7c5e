// libmcmc_hip.so: the sums of the ellipsoid-truncated harmonic mean (evidence_kernels.hip).  Life
// cycle of the other device products: configure once, accumulate beside a moment snapshot, request /
// fetch at a checkpoint (the hot loop is never stalled), set on resume.  What is new here is the
// ellipsoid: handed in as (m, cov), factorised on the host, and -- after the first -- only STAGED
// until a closing request activates it in stream order, so that no interval mixes two ellipsoids.
#include "ctx.h"
#include "host_linalg.h"

namespace {

void ev_release(mcmc_hip_ctx* h)
{
    auto& F = h->evd;
    F.slab.release();
    F.ell.release();
    F.s.release();
    if (F.pin) (void)hipHostFree(F.pin);
    if (F.pin_ell) (void)hipHostFree(F.pin_ell);
    F.pin = F.pin_ell = nullptr;
    F.active.clear(); F.staged.clear(); F.pend_active.clear(); F.pend_staged.clear();
    F.n_words = 0;
    F.n_r = 0;
    F.n_acc = F.pend_n = 0;
    F.on = F.pending = false;
}

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
    a.acc = F.slab.p;
    a.cnt = (unsigned long long*)(F.slab.p + n);
    a.clamped = (unsigned long long*)(F.slab.p + 2 * n);
    a.ckey = (unsigned long long*)(F.slab.p + 2 * n + 1);
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
    ev_release(h);
    if (n_radii == 0) return MCMC_HIP_OK;
    auto& F = h->evd;
    F.n_r = n_radii;
    for (int r = 0; r < mcmc::kEvMaxRadii; ++r) F.r2[r] = r < n_radii ? r2[r] : 0.0;
    const size_t n = ev_n(h), d = h->d;
    F.n_words = 2 * n + 2;
    HIP_TRY(h, F.slab.resize(F.n_words));
    HIP_TRY(h, F.ell.resize(d * (d + 1)));
    HIP_TRY(h, F.s.resize((size_t)h->W));
    HIP_TRY(h, hipHostMalloc((void**)&F.pin, sizeof(double) * F.n_words, hipHostMallocDefault));
    HIP_TRY(h, hipHostMalloc((void**)&F.pin_ell, sizeof(double) * d * (d + 1), hipHostMallocDefault));
    if (!F.ev) HIP_TRY(h, hipEventCreateWithFlags(&F.ev, hipEventDisableTiming));
    HIP_TRY(h, hipMemset(F.slab.p, 0, sizeof(double) * F.n_words));
    HIP_TRY(h, hipMemset(F.ell.p, 0, sizeof(double) * d * (d + 1)));
    F.on = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_layout(const mcmc_hip_ctx* h, int32_t* on, int32_t* n_radii, int32_t* n_groups,
                             int64_t* n_ell, int32_t* has_active, int32_t* has_staged, int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& F = h->evd;
    if (on) *on = F.on ? 1 : 0;
    if (n_radii) *n_radii = F.n_r;
    if (n_groups) *n_groups = F.on ? h->G : 0;
    if (n_ell) *n_ell = F.on ? (int64_t)ev_n_ell(h) : 0;
    if (has_active) *has_active = F.active.empty() ? 0 : 1;
    if (has_staged) *has_staged = F.staged.empty() ? 0 : 1;
    if (n_accumulations) *n_accumulations = F.n_acc;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_set_ellipsoid(mcmc_hip_ctx* h, const double* m, const double* cov)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.on) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_set_ellipsoid");
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
    if (!F.on) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_accumulate");
    if (F.active.empty()) return fail(h, MCMC_HIP_ERR_STATE, "no ellipsoid is active: call evidence_set_ellipsoid first");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const mcmc::EvArgs a = ev_args(h);
    HIP_TRY(h, mcmc_hip_launch_evidence(&a, h->stream));
    F.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_request(mcmc_hip_ctx* h, int32_t close)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.on) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_request");
    if (F.pending) return fail(h, MCMC_HIP_ERR_STATE, "an evidence request is already pending");
    if (close && !F.staged.empty() && !h->have_state)
        return fail(h, MCMC_HIP_ERR_STATE, "no state: the staged ellipsoid takes c from logpost");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(F.pin, F.slab.p, sizeof(double) * F.n_words, hipMemcpyDeviceToHost, h->stream));
    F.pend_active = F.active;
    F.pend_staged = F.staged;
    F.pend_n = F.n_acc;
    if (close) {
        HIP_TRY(h, hipMemsetAsync(F.slab.p, 0, sizeof(double) * (F.n_words - 1), h->stream));   // (c stays)
        F.n_acc = 0;
        if (!F.staged.empty()) {
            if (int rc = ev_activate(h, F.staged)) return rc;
            F.active = std::move(F.staged);
            F.staged.clear();
        }
    }
    HIP_TRY(h, hipEventRecord(F.ev, h->stream));   // (last: a fetch also vouches for the pinned ellipsoid)
    F.pending = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_evidence_fetch(mcmc_hip_ctx* h, double* sums, uint64_t* counts, int64_t n, uint64_t* clamped,
                            int64_t* n_accumulations, double* active, double* staged, int64_t n_ell,
                            int32_t* has_active, int32_t* has_staged)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& F = h->evd;
    if (!F.pending) return fail(h, MCMC_HIP_ERR_STATE, "no evidence request is pending");
    if (int rc = ev_sizes_ok(h, "evidence_fetch", sums, counts, n, n_ell)) return rc;
    if (!active || !staged) return fail(h, MCMC_HIP_ERR_ARG, "%s is null", !active ? "active" : "staged");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(F.ev));
    F.pending = false;
    const size_t k = ev_n(h);
    std::copy(F.pin, F.pin + k, sums);
    std::memcpy(counts, F.pin + k, sizeof(uint64_t) * k);
    if (clamped) std::memcpy(clamped, F.pin + 2 * k, sizeof(uint64_t));
    if (n_accumulations) *n_accumulations = F.pend_n;
    std::fill(active, active + n_ell, 0.0);
    std::fill(staged, staged + n_ell, 0.0);
    if (!F.pend_active.empty()) {
        std::copy(F.pend_active.begin(), F.pend_active.end(), active);
        unsigned long long key;
        std::memcpy(&key, F.pin + 2 * k + 1, sizeof key);
        active[n_ell - 1] = mcmc::ev_value(key);
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
    if (!F.on) return fail(h, MCMC_HIP_ERR_STATE, "evidence_configure must precede evidence_set");
    if (F.pending) return fail(h, MCMC_HIP_ERR_STATE, "an evidence request is pending (fetch it first)");
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
    std::vector<double> words(F.n_words, 0.0);
    std::copy(sums, sums + k, words.begin());
    std::memcpy(words.data() + k, counts, sizeof(uint64_t) * k);
    std::memcpy(words.data() + 2 * k, &clamped, sizeof(uint64_t));
    const unsigned long long key = active ? mcmc::ev_key(active[ne]) : 0ull;
    std::memcpy(words.data() + 2 * k + 1, &key, sizeof key);
    HIP_TRY(h, hipMemcpy(F.slab.p, words.data(), sizeof(double) * F.n_words, hipMemcpyHostToDevice));
    F.active.clear();
    F.staged.clear();
    if (active) {
        F.active.assign(active, active + ne);
        HIP_TRY(h, hipMemcpy(F.ell.p, active, sizeof(double) * ne, hipMemcpyHostToDevice));
    }
    if (staged) F.staged.assign(staged, staged + ne);
    F.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

}  // extern "C"
