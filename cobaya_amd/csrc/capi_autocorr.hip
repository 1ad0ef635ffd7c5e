// libmcmc_hip.so: lagged cross-products of the ensemble for the integrated autocorrelation time
// (autocorr_kernels.hip).  The life cycle is the Readout's (readout.h), but what is counted is pairs
// per lag, not accumulations.
#include "ctx.h"

extern "C" {

int mcmc_hip_autocorr_configure(mcmc_hip_ctx* h, int32_t n_dims, const int32_t* dims, int32_t lags)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (n_dims < 0) return fail(h, MCMC_HIP_ERR_ARG, "n_dims = %d must be >= 0", n_dims);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n_dims == 0) {
        h->ac.release();
        return MCMC_HIP_OK;
    }
    if (!dims) return fail(h, MCMC_HIP_ERR_ARG, "dims is null");
    if (lags < 1 || lags > mcmc::kAcMaxLags)
        return fail(h, MCMC_HIP_ERR_ARG, "lags = %d must lie in 1..%d", lags, mcmc::kAcMaxLags);
    const int d = h->d;
    std::vector<char> seen(d, 0);
    for (int k = 0; k < n_dims; ++k) {
        if (dims[k] < 0 || dims[k] >= d)
            return fail(h, MCMC_HIP_ERR_ARG, "dims[%d] = %d is not a parameter index (d = %d)", k, dims[k], d);
        if (seen[dims[k]])
            return fail(h, MCMC_HIP_ERR_ARG, "dims[%d] = %d is a duplicate: a parameter is listed once", k, dims[k]);
        seen[dims[k]] = 1;
    }
    const int rows = mcmc_hip_autocorr_rows_per_pass(h->gs, lags);
    if (rows < 1)
        return fail(h, MCMC_HIP_ERR_ARG, "lags = %d: a group of %d walkers does not fit the kernel's tile", lags, h->gs);
    auto& A = h->ac;
    A.release();
    const size_t slots = (size_t)lags + 1, n = (size_t)n_dims;
    const size_t n_ring = slots * n * (size_t)h->W, n_S = slots * (size_t)h->G * n, n_acc = 3 * slots * n;
    const size_t need = sizeof(double) * (n_ring + 2 * n_S + n_acc) + sizeof(int) * n;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        return fail(h, MCMC_HIP_ERR_ARG, "lags = %d: the ring of %d snapshots of %d parameters x %d walkers needs "
                    "%zu bytes of device memory, %zu are free", lags, lags + 1, n_dims, h->W, need, free_b);
    HIP_TRY_BUILD(h, A, A.ring.resize(n_ring));
    HIP_TRY_BUILD(h, A, A.ringS.resize(n_S));
    HIP_TRY_BUILD(h, A, A.Pg.resize(n_S));
    HIP_TRY_BUILD(h, A, A.ro.alloc(n_acc, h->stream));
    HIP_TRY_BUILD(h, A, A.dims.resize(n));
    HIP_TRY_BUILD(h, A, hipMemcpy(A.dims.p, dims, sizeof(int) * n, hipMemcpyHostToDevice));
    A.n = n_dims; A.lags = lags; A.rows_per_pass = rows;
    A.n_pairs.assign(slots, 0);
    A.pend_pairs.assign(slots, 0);
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_layout(const mcmc_hip_ctx* h, int32_t* n_dims, int32_t* lags, int64_t* n_doubles,
                             int32_t* held)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    const auto& A = h->ac;
    if (n_dims) *n_dims = A.n;
    if (lags) *lags = A.lags;
    if (n_doubles) *n_doubles = (int64_t)A.ro.n_words;
    if (held) *held = A.held;
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_accumulate(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& A = h->ac;
    if (!A.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "autocorr_configure must precede autocorr_accumulate");
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int held = std::min(A.held + 1, A.lags + 1);
    mcmc::AcArgs a{};
    a.x = h->x.p; a.shift = h->dshift.p; a.dims = A.dims.p;
    a.ring = A.ring.p; a.ringS = A.ringS.p; a.Pg = A.Pg.p; a.acc = A.ro.dev<double>();
    a.W = h->W; a.G = h->G; a.gs = h->gs; a.n = A.n; a.lags = A.lags;
    a.held = held; a.head = A.head; a.rows_per_pass = A.rows_per_pass;
    HIP_TRY(h, mcmc_hip_launch_autocorr(&a, h->stream));
    A.held = held;
    A.head = (A.head + 1) % (A.lags + 1);
    for (int k = 0; k < held; ++k) A.n_pairs[k] += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_request(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& A = h->ac;
    if (!A.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "autocorr_configure must precede autocorr_request");
    if (A.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an autocorr request is already pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, A.ro.copy_out(h->stream, A.ro.n_words));
    HIP_TRY(h, A.ro.mark(h->stream));
    A.pend_pairs = A.n_pairs;
    std::fill(A.n_pairs.begin(), A.n_pairs.end(), (int64_t)0);
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_fetch(mcmc_hip_ctx* h, double* sums, int64_t n, int64_t* n_pairs)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& A = h->ac;
    if (!A.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "no autocorr request is pending");
    if (!sums || (size_t)n != A.ro.n_words)
        return fail(h, MCMC_HIP_ERR_ARG, "sums: the accumulators hold %zu doubles, not %lld", A.ro.n_words, (long long)n);
    if (!n_pairs) return fail(h, MCMC_HIP_ERR_ARG, "n_pairs is null");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, A.ro.wait());
    std::copy(A.ro.host<double>(), A.ro.host<double>() + A.ro.n_words, sums);
    std::copy(A.pend_pairs.begin(), A.pend_pairs.end(), n_pairs);
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_set(mcmc_hip_ctx* h, const double* sums, int64_t n, const int64_t* n_pairs)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& A = h->ac;
    if (!A.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "autocorr_configure must precede autocorr_set");
    if (A.ro.pending) return fail(h, MCMC_HIP_ERR_STATE, "an autocorr request is pending (fetch it first)");
    if (!sums || (size_t)n != A.ro.n_words)
        return fail(h, MCMC_HIP_ERR_ARG, "sums: the accumulators hold %zu doubles, not %lld", A.ro.n_words, (long long)n);
    if (!n_pairs) return fail(h, MCMC_HIP_ERR_ARG, "n_pairs is null");
    for (int k = 0; k <= A.lags; ++k)
        if (n_pairs[k] < 0) return fail(h, MCMC_HIP_ERR_ARG, "n_pairs[%d] = %lld must be >= 0", k, (long long)n_pairs[k]);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, A.ro.upload(sums));
    A.n_pairs.assign(n_pairs, n_pairs + A.lags + 1);
    return MCMC_HIP_OK;
}

int mcmc_hip_autocorr_reset(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    auto& A = h->ac;
    if (!A.ro.on()) return fail(h, MCMC_HIP_ERR_STATE, "autocorr_configure must precede autocorr_reset");
    A.held = A.head = 0;   // (the slots are overwritten before they are read again)
    return MCMC_HIP_OK;
}

}  // extern "C"
