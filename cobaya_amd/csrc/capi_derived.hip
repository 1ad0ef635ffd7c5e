// libmcmc_hip.so: derived parameters (derived_kernels.hip).  The library owns the rows z[m][W] and
// their moments; the CALLER fills z on the engine's stream from the state as it lies in HBM
// (mcmc_hip_derived_buffers hands out both pointers).  The life cycle of the moments is the Readout's
// (readout.h).
#include "ctx.h"

namespace {

size_t dv_n_pairs(int m) { return (size_t)m * (m + 1) / 2; }

mcmc::DvArgs dv_args(mcmc_hip_ctx* h)
{
    auto& D = h->dv;
    const size_t n_S = (size_t)(D.m + 2) * D.n_col;
    mcmc::DvArgs a{};
    a.x = h->x.p; a.z = D.z.p; a.shift = D.shift.p; a.xshift = h->dshift.p; a.cross = D.cross.p;
    a.Sg = D.Sg.p; a.Ng = D.Ng.p;
    a.N = D.ro.dev();
    a.S = D.ro.dev<double>() + 1;
    a.bad = D.ro.dev() + 1 + n_S;
    a.kmax = a.bad + D.m;
    a.kmin = a.kmax + D.m;
    a.W = h->W; a.gs = D.gs; a.G = D.G; a.m = D.m; a.n_cross = D.n_cross; a.n_col = D.n_col;
    return a;
}

// the slab's words <-> (N, A[m], B[m (m + 1) / 2] with (j, k <= j) at j (j + 1) / 2 + k, C[m][n_cross],
// X[n_cross], V[n_cross], bad[m], min[m], max[m]); a name without a finite value has min = max = NaN
void dv_unpack(const mcmc_hip_ctx* h, const unsigned long long* words, uint64_t* n_used, double* A, double* B,
               double* C, double* X, double* V, uint64_t* bad, double* mn, double* mx)
{
    const auto& D = h->dv;
    const int m = D.m, nc = D.n_col;
    const double* S = (const double*)(words + 1);
    const unsigned long long* wb = words + 1 + (size_t)(m + 2) * nc;
    for (int c = 0; c < D.n_cross; ++c) {
        X[c] = S[(size_t)m * nc + 1 + m + c];
        V[c] = S[(size_t)(m + 1) * nc + 1 + m + c];
    }
    *n_used = words[0];
    for (int j = 0; j < m; ++j) {
        A[j] = S[(size_t)j * nc];
        for (int k = 0; k <= j; ++k) B[dv_n_pairs(j) + k] = S[(size_t)j * nc + 1 + k];
        for (int c = 0; c < D.n_cross; ++c) C[(size_t)j * D.n_cross + c] = S[(size_t)j * nc + 1 + m + c];
        bad[j] = wb[j];
        const unsigned long long kx = wb[m + j], kn = wb[2 * m + j];
        mx[j] = kx ? mcmc::dv_value(kx) : std::numeric_limits<double>::quiet_NaN();
        mn[j] = kn ? mcmc::dv_value(~kn) : std::numeric_limits<double>::quiet_NaN();
    }
}

int dv_null(mcmc_hip_ctx* h, const char* what, const void* A, const void* B, const void* C, const void* X,
            const void* V, const void* bad, const void* mn, const void* mx)
{
    const bool cross = h->dv.n_cross > 0;
    const char* name = !A ? "A" : !B ? "B" : (!C && cross) ? "C" : (!X && cross) ? "X" : (!V && cross) ? "V" : !bad ? "bad" : !mn ? "min" : !mx ? "max" : nullptr;
    return name ? fail(h, MCMC_HIP_ERR_ARG, "%s: %s is null", what, name) : (int)MCMC_HIP_OK;
}

int dv_resize_groups(mcmc_hip_ctx* h, int gs)
{
    auto& D = h->dv;
    D.gs = gs;
    D.G = h->W / gs;
    HIP_TRY(h, D.Sg.resize((size_t)D.G * (D.m + 2) * D.n_col));
    HIP_TRY(h, D.Ng.resize((size_t)D.G));
    return MCMC_HIP_OK;
}

}  // namespace

extern "C" {

int mcmc_hip_derived_configure(mcmc_hip_ctx* h, int32_t m, int32_t n_cross, const int32_t* cross_dims,
                               const double* shift)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (m < 0 || m > mcmc::kDvMaxNames)
        return fail(h, MCMC_HIP_ERR_ARG, "m = %d must lie in 0..%d", m, mcmc::kDvMaxNames);
    if (h->mg.ro.on())
        return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede marginals_configure (release the "
                    "marginals first: their entries may read the derived rows)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (m == 0) {
        h->dv.release();
        return MCMC_HIP_OK;
    }
    const int d = h->d;
    if (n_cross < 0 || n_cross > d || n_cross > mcmc::kDvMaxCross)
        return fail(h, MCMC_HIP_ERR_ARG, "n_cross = %d must lie in 0..%d", n_cross, std::min(d, mcmc::kDvMaxCross));
    if (n_cross > 0 && !cross_dims) return fail(h, MCMC_HIP_ERR_ARG, "cross_dims is null");
    if (!shift) return fail(h, MCMC_HIP_ERR_ARG, "shift is null");
    std::vector<char> seen(d, 0);
    for (int c = 0; c < n_cross; ++c) {
        if (cross_dims[c] < 0 || cross_dims[c] >= d)
            return fail(h, MCMC_HIP_ERR_ARG, "cross_dims[%d] = %d is not a parameter index (d = %d)", c, cross_dims[c], d);
        if (seen[cross_dims[c]])
            return fail(h, MCMC_HIP_ERR_ARG, "cross_dims[%d] = %d is a duplicate: a parameter is listed once", c, cross_dims[c]);
        seen[cross_dims[c]] = 1;
    }
    for (int j = 0; j < m; ++j)
        if (!std::isfinite(shift[j])) return fail(h, MCMC_HIP_ERR_ARG, "shift[%d] = %g is not finite", j, shift[j]);
    auto& D = h->dv;
    D.release();
    D.m = m; D.n_cross = n_cross; D.n_col = 1 + m + n_cross;
    HIP_TRY_BUILD(h, D, D.z.resize((size_t)m * h->W));
    HIP_TRY_BUILD(h, D, D.shift.resize((size_t)m));
    HIP_TRY_BUILD(h, D, D.cross.resize((size_t)std::max(n_cross, 1)));
    HIP_TRY_BUILD(h, D, D.ro.alloc(1 + (size_t)(m + 2) * D.n_col + 3 * (size_t)m, h->stream));
    if (int rc = dv_resize_groups(h, h->gs)) {
        D.release();
        return rc;
    }
    HIP_TRY_BUILD(h, D, hipMemsetAsync(D.z.p, 0, sizeof(double) * (size_t)m * h->W, h->stream));
    HIP_TRY_BUILD(h, D, hipMemcpy(D.shift.p, shift, sizeof(double) * m, hipMemcpyHostToDevice));
    if (n_cross > 0) HIP_TRY_BUILD(h, D, hipMemcpy(D.cross.p, cross_dims, sizeof(int) * n_cross, hipMemcpyHostToDevice));
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_set_group_size(mcmc_hip_ctx* h, int32_t group_size)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_set_group_size");
    if (group_size < 1 || h->W % group_size)
        return fail(h, MCMC_HIP_ERR_ARG, "group_size = %d must divide n_walkers = %d", group_size, h->W);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return dv_resize_groups(h, group_size);
}

int mcmc_hip_derived_layout(const mcmc_hip_ctx* h, int32_t* m, int32_t* n_cross, int32_t* group_size,
                            int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& D = h->dv;
    if (m) *m = D.m;
    if (n_cross) *n_cross = D.n_cross;
    if (group_size) *group_size = D.gs;
    if (n_accumulations) *n_accumulations = D.ro.n_acc;
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_buffers(mcmc_hip_ctx* h, uint64_t* x_device_ptr, uint64_t* z_device_ptr)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->dv.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_buffers");
    if (x_device_ptr) *x_device_ptr = (uint64_t)(uintptr_t)h->x.p;
    if (z_device_ptr) *z_device_ptr = (uint64_t)(uintptr_t)h->dv.z.p;
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_set_values(mcmc_hip_ctx* h, const double* values)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_set_values");
    if (!values) return fail(h, MCMC_HIP_ERR_ARG, "values is null");
    const size_t W = h->W, m = D.m;
    std::vector<double> t(m * W);
    for (size_t w = 0; w < W; ++w)
        for (size_t j = 0; j < m; ++j) t[j * W + w] = values[w * m + j];
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(D.z.p, t.data(), sizeof(double) * m * W, hipMemcpyHostToDevice));
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_get_values(mcmc_hip_ctx* h, double* values)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_get_values");
    if (!values) return fail(h, MCMC_HIP_ERR_ARG, "values is null");
    const size_t W = h->W, m = D.m;
    std::vector<double> t(m * W);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(t.data(), D.z.p, sizeof(double) * m * W, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
        for (size_t j = 0; j < m; ++j) values[w * m + j] = t[j * W + w];
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_accumulate(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_accumulate");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const mcmc::DvArgs a = dv_args(h);
    HIP_TRY(h, mcmc_hip_launch_derived(&a, h->stream));
    D.ro.n_acc += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_request(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_request");
    if (D.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a derived request is already pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, D.ro.copy_out(h->stream, D.ro.n_words));
    HIP_TRY(h, D.ro.mark(h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_fetch(mcmc_hip_ctx* h, uint64_t* n_used, double* A, double* B, double* C, double* X,
                           double* V, uint64_t* bad, double* min, double* max, int64_t* n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no derived request is pending");
    if (!n_used) return fail(h, MCMC_HIP_ERR_ARG, "derived_fetch: n_used is null");
    if (int rc = dv_null(h, "derived_fetch", A, B, C, X, V, bad, min, max)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, D.ro.wait());
    dv_unpack(h, D.ro.host(), n_used, A, B, C, X, V, bad, min, max);
    if (n_accumulations) *n_accumulations = D.ro.pend_n;
    return MCMC_HIP_OK;
}

int mcmc_hip_derived_set(mcmc_hip_ctx* h, uint64_t n_used, const double* A, const double* B, const double* C,
                         const double* X, const double* V, const uint64_t* bad, const double* min,
                         const double* max, int64_t n_accumulations)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& D = h->dv;
    if (!D.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "derived_configure must precede derived_set");
    if (D.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "a derived request is pending (fetch it first)");
    if (int rc = dv_null(h, "derived_set", A, B, C, X, V, bad, min, max)) return rc;
    if (n_accumulations < 0)
        return fail(h, MCMC_HIP_ERR_ARG, "n_accumulations = %lld must be >= 0", (long long)n_accumulations);
    const int m = D.m, nc = D.n_col;
    std::vector<unsigned long long> words(D.ro.n_words, 0ull);
    double* S = (double*)(words.data() + 1);
    unsigned long long* wb = words.data() + 1 + (size_t)(m + 2) * nc;
    words[0] = n_used;
    for (int c = 0; c < D.n_cross; ++c) {
        S[(size_t)m * nc + 1 + m + c] = X[c];
        S[(size_t)(m + 1) * nc + 1 + m + c] = V[c];
    }
    for (int j = 0; j < m; ++j) {
        S[(size_t)j * nc] = A[j];
        for (int k = 0; k <= j; ++k) S[(size_t)j * nc + 1 + k] = B[dv_n_pairs(j) + k];
        for (int c = 0; c < D.n_cross; ++c) S[(size_t)j * nc + 1 + m + c] = C[(size_t)j * D.n_cross + c];
        wb[j] = bad[j];
        if (std::isinf(min[j]) || std::isinf(max[j]))
            return fail(h, MCMC_HIP_ERR_ARG, "min / max[%d] = %g / %g: a finite value, or NaN for none", j, min[j], max[j]);
        wb[m + j] = std::isnan(max[j]) ? 0ull : mcmc::dv_key(max[j]);
        wb[2 * m + j] = std::isnan(min[j]) ? 0ull : ~mcmc::dv_key(min[j]);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, D.ro.upload(words.data()));
    D.ro.n_acc = n_accumulations;
    return MCMC_HIP_OK;
}

}  // extern "C"
