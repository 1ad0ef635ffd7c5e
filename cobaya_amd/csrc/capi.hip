// libmcmc_hip.so: the C ABI declared in include/mcmc_hip.h -- create / destroy, prior, Gaussian
// targets, blocking, proposal, evaluate, state, the mcmc_hip_step dispatch with the from-scratch
// stepper, row draining, moments and timing.  The other targets: capi_targets.hip; incremental
// evaluation: capi_incremental.hip; the device checkpoint: capi_checkpoint.hip.
#include "ctx.h"
#include "host_linalg.h"

int block_slots(const mcmc_hip_ctx* h, int which)
{
    if (!h->blocked) return h->d;
    int L = 0;
    for (size_t b = 0; b < h->blk_size.size(); ++b) {
        if (which == 0) L += h->blk_over[b] * h->blk_size[b];
        else if (which == 1) L += ((int)b <= h->drag_last_slow) ? h->blk_size[b] : 0;
        else L += ((int)b > h->drag_last_slow) ? h->blk_size[b] : 0;
    }
    return L;
}

int upload_constants(mcmc_hip_ctx* h)
{
    if (!h->have_prior || !h->have_target) return MCMC_HIP_OK;
    const int d = h->d, K = h->K;
    const ConstLayout cl{d, K};
    std::vector<double> c((size_t)cl.size() + 16, 0.0);
    for (int i = 0; i < d; ++i) {
        c[cl.lo() + i] = h->lo[i];
        c[cl.hi() + i] = h->hi[i];
        c[cl.loc() + i] = h->loc[i];
        c[cl.scale() + i] = h->scale[i];
        c[cl.mls() + i] = h->mls[i];
        c[cl.elem() + 3 * i + 0] = h->lo[i];
        c[cl.elem() + 3 * i + 1] = h->hi[i];
        c[cl.elem() + 3 * i + 2] = K > 0 ? h->mean[i] : 0.0;
    }
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < d; ++i) c[cl.mean(k) + i] = h->mean[(size_t)k * d + i];
        c[cl.cnorm() + k] = h->cnorm[k];
        c[cl.weight() + k] = h->weight[k];
        const double* Lk = h->Linv.data() + (size_t)k * d * d;
        double* dst = c.data() + cl.linv(k);
        mcmc::tri_stream_for_each(d, [&](int idx, int j, int i) { dst[idx] = Lk[(size_t)j * d + i]; });
    }
    HIP_TRY(h, h->cblock.resize(c.size()));
    HIP_TRY(h, hipMemcpyAsync(h->cblock.p, c.data(), sizeof(double) * c.size(),
                              hipMemcpyHostToDevice, h->stream));
    std::vector<double> lcol;
    if (h->kb && K > 0) {
        // row-major L^-1 per mode (evaluator) and the column-major, zero-padded [dp][dp]
        // copy of mode 0 that the column-sweep step kernel stages in LDS
        const int dp = h->kb->dp;
        HIP_TRY(h, h->dLrow.resize(h->Linv.size()));
        HIP_TRY(h, hipMemcpyAsync(h->dLrow.p, h->Linv.data(), sizeof(double) * h->Linv.size(),
                                  hipMemcpyHostToDevice, h->stream));
        // 4x4 tiles [column block][row block][col][row], zero above the diagonal and in the pad
        const int nb = dp / 4;
        lcol.assign((size_t)dp * dp, 0.0);
        for (int j = 0; j < d; ++j)
            for (int i = 0; i <= j; ++i)
                lcol[(((size_t)(i / 4) * nb + (j / 4)) * 4 + (i % 4)) * 4 + (j % 4)] =
                    h->Linv[(size_t)j * d + i];
        // then the 16 x 4 tiles (R, kk), kk <= 4R + 3 - shift/4, of the matrix-core kernel,
        // R-major, each in A-operand lane order: lane l holds
        // L^-1[16R - shift + (l & 15)][4kk + (l >> 4)]
        {
            const int sh = h->kb->row_shift;   // the partial row tile comes first
            const int RT = (dp + sh + 15) / 16, KT = (dp + 3) / 4;
            for (int R = 0; R < RT; ++R)
                for (int kk = 0; kk < std::min(4 * R + 4 - sh / 4, KT); ++kk)
                    for (int l = 0; l < 64; ++l) {
                        const int j = 16 * R - sh + (l & 15), i = 4 * kk + (l >> 4);
                        lcol.push_back((j >= 0 && j < d && i <= j) ? h->Linv[(size_t)j * d + i] : 0.0);
                    }
            if ((int)(lcol.size() - (size_t)dp * dp) != 64 * h->kb->n_tiles)
                return fail(h, MCMC_HIP_ERR_ARG, "internal: tile count mismatch");
        }
        HIP_TRY(h, h->dLcol.resize(lcol.size()));
        HIP_TRY(h, hipMemcpyAsync(h->dLcol.p, lcol.data(), sizeof(double) * lcol.size(),
                                  hipMemcpyHostToDevice, h->stream));
    }
    if (h->incremental && (K >= 1 || h->huge) && K <= mcmc::kMaxModes) {
        const int dq = (d + 3) / 4, dpad = 4 * dq;
        if (K > 0) HIP_TRY(h, h->y.resize((size_t)K * d * h->W));
        if (K > 1) HIP_TRY(h, h->amode.resize((size_t)K * h->W));
        h->amode_valid = false;
        std::vector<double> pr((size_t)5 * dpad, 0.0);
        for (int i = 0; i < dpad; ++i) {
            pr[i] = i < d ? h->lo[i] : -INFINITY;
            pr[dpad + i] = i < d ? h->hi[i] : INFINITY;
            pr[2 * dpad + i] = i < d ? h->loc[i] : 0.0;
            // 1/scale = 0 and mls = 0: "no normal prior here" (kind 0 and the padding)
            const bool nrm = i < d && h->kind[i] == 1;
            pr[3 * dpad + i] = nrm ? 1.0 / h->scale[i] : 0.0;
            pr[4 * dpad + i] = nrm ? h->mls[i] : 0.0;
        }
        HIP_TRY(h, h->inc_prior.resize(pr.size()));
        HIP_TRY(h, hipMemcpyAsync(h->inc_prior.p, pr.data(), sizeof(double) * pr.size(),
                                  hipMemcpyHostToDevice, h->stream));
        if (K > 0) {
            HIP_TRY(h, h->inc_Lrow.resize((size_t)K * d * d));
            HIP_TRY(h, hipMemcpyAsync(h->inc_Lrow.p, h->Linv.data(), sizeof(double) * K * d * d,
                                      hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, h->inc_mean.resize((size_t)K * d));
            HIP_TRY(h, hipMemcpyAsync(h->inc_mean.p, h->mean.data(), sizeof(double) * K * d,
                                      hipMemcpyHostToDevice, h->stream));
        }
        h->y_valid = false; h->amode_valid = false;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MCMC_HIP_OK;
}

namespace {

// (at set-target time: step_kernel's LDS at the widest workgroup, one parameter block)
int lds_check(mcmc_hip_ctx* h)
{
    if (h->kb || h->huge) return MCMC_HIP_OK;  // the big / huge step kernels' LDS does not depend on K
    const size_t lds = mcmc::step_lds_bytes(h->K, 256, h->gs, mcmc::v_slab(h->d));
    if (lds > mcmc::kLdsMax)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "the step kernel needs %zu bytes of LDS per workgroup (> 160 KiB): fewer "
                    "mixture modes or a smaller group_size are required", lds);
    return MCMC_HIP_OK;
}

int set_target_common(mcmc_hip_ctx* h, int K, const double* means, const double* covs,
                      const double* weights, bool normalized)
{
    const int d = h->d;
    if (K < 1 || K > mcmc::kMaxModes)
        return fail(h, MCMC_HIP_ERR_ARG, "n_modes must be in 1..%d, got %d", mcmc::kMaxModes, K);
    if (h->huge && K > mcmc::kHugeMaxModes)
        return fail(h, MCMC_HIP_ERR_ARG, "d=%d > %d serves at most %d mixture modes, got %d", d, kMaxDimBig,
                    mcmc::kHugeMaxModes, K);
    std::vector<double> L((size_t)d * d), Li((size_t)d * d);
    h->mean.assign(means, means + (size_t)K * d);
    h->Linv.assign((size_t)K * d * d, 0.0);
    h->cnorm.assign(K, 0.0);
    h->weight.assign(K, 1.0 / K);
    for (int k = 0; k < K; ++k) {
        const double* C = covs + (size_t)k * d * d;
        if (!is_symmetric(d, C) || !cholesky_lower(d, C, L.data()))
            return fail(h, MCMC_HIP_ERR_NOT_PD,
                        "covariance of mode %d is not a symmetric positive-definite matrix", k);
        tri_inverse_lower(d, L.data(), Li.data());
        std::copy(Li.begin(), Li.end(), h->Linv.begin() + (size_t)k * d * d);
        double logdet = 0.0;
        for (int i = 0; i < d; ++i) logdet += std::log(L[i * d + i]);
        logdet *= 2.0;
        h->cnorm[k] = normalized ? d * std::log(2.0 * M_PI) + logdet : 0.0;
    }
    if (weights) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            if (!(weights[k] >= 0.0)) return fail(h, MCMC_HIP_ERR_ARG, "negative mixture weight");
            s += weights[k];
        }
        if (!(s > 0.0)) return fail(h, MCMC_HIP_ERR_ARG, "mixture weights sum to zero");
        const bool renorm = !(std::fabs(s - 1.0) <= 1e-8 + 1e-5);  // np.isclose(sum, 1)
        for (int k = 0; k < K; ++k) h->weight[k] = renorm ? weights[k] / s : weights[k];
    }
    h->K = K;
    h->bg.on = false;
    h->fnt.on = false;
    h->have_target = true;
    ++h->dir_epoch;
    h->have_state = false;
    int rc = lds_check(h);
    if (rc) return rc;
    return upload_constants(h);
}

}  // namespace

// (outside the extern "C" block: a kernel declared inside it would be exported under its bare name)
namespace mcmc {
namespace {
// The checkpoint read-out: word i of the block gsum | pooled (n_acc accumulators) | accept counter
// goes to word i of the pinned host block, the stuck flag and a function target's error flag to
// the two halves of the word behind them; the accumulators -- not the counter -- are zeroed in
// the same pass when `zero` is set.  Words travel as bit patterns (the counter is an integer).
__global__ void __launch_bounds__(256) readout_moments_kernel(unsigned long long* __restrict__ acc,
                                                              size_t n_acc, const int* __restrict__ stuck,
                                                              const int* __restrict__ fn_bad,
                                                              unsigned long long* __restrict__ pin, int zero)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_acc) {
        pin[i] = acc[i];
        if (zero) acc[i] = 0ull;
    } else if (i == n_acc) {
        pin[i] = acc[i];
        const unsigned lo = (unsigned)*stuck, hi = fn_bad ? (unsigned)*fn_bad : 0u;
        pin[i + 1] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    }
}
}  // namespace
}  // namespace mcmc

extern "C" {

const char* mcmc_hip_version(void) { return "mcmc_hip 0.1 (gfx950)"; }

const char* mcmc_hip_last_error(const mcmc_hip_ctx* h)
{
    return h ? h->err.c_str() : g_create_error.c_str();
}

int mcmc_hip_dim_supported(int d)
{
    return kernels_for_dim(d) != nullptr || big_for_dim(d) != nullptr;
}

int32_t mcmc_hip_max_dim(void) { return mcmc::kMaxDimHuge; }

int mcmc_hip_create(const mcmc_hip_config* cfg, mcmc_hip_ctx** out)
{
    if (!cfg || !out) return fail(nullptr, MCMC_HIP_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->d < 1) return fail(nullptr, MCMC_HIP_ERR_ARG, "d must be >= 1, got %d", cfg->d);
    const DimKernels* k = kernels_for_dim(cfg->d);
    const BigKernels* kb = k ? nullptr : big_for_dim(cfg->d);
    const bool huge = cfg->d > kMaxDimBig;
    if (huge) {   // 128 < d <= 256: huge_kernels.hip serves incremental evaluation with the shared basis
        if (cfg->d > mcmc::kMaxDimHuge)
            return fail(nullptr, MCMC_HIP_ERR_ARG, "d=%d is above the largest dimension served (%d)",
                        cfg->d, mcmc::kMaxDimHuge);
        if (!(cfg->flags & MCMC_HIP_FLAG_INCREMENTAL))
            return fail(nullptr, MCMC_HIP_ERR_ARG,
                        "d=%d > %d is served with incremental evaluation only (evaluation: full is not)",
                        cfg->d, kMaxDimBig);
        if (cfg->flags & MCMC_HIP_FLAG_OWN_BASIS)
            return fail(nullptr, MCMC_HIP_ERR_ARG, "d=%d > %d needs the shared basis (shared_basis: False is not served)",
                        cfg->d, kMaxDimBig);
        if (cfg->emit_capacity > 0)
            return fail(nullptr, MCMC_HIP_ERR_ARG,
                        "d=%d > %d emits no rows on the device (emit: chains is not served; use emit: snapshots)",
                        cfg->d, kMaxDimBig);
    }
    if (!k && !kb && !huge)
        return fail(nullptr, MCMC_HIP_ERR_ARG,
                    "no kernels compiled for d=%d (this build covers d = 1..32 lane-per-walker "
                    "and 33..%d column-sweep, as selected at build time)", cfg->d, kMaxDimBig);
    if (cfg->group_size != 64 && cfg->group_size != 128 && cfg->group_size != 256)
        return fail(nullptr, MCMC_HIP_ERR_ARG, "group_size must be 64, 128 or 256, got %d",
                    cfg->group_size);
    if (cfg->n_walkers < cfg->group_size || cfg->n_walkers % cfg->group_size)
        return fail(nullptr, MCMC_HIP_ERR_ARG,
                    "n_walkers (%d) must be a positive multiple of group_size (%d)",
                    cfg->n_walkers, cfg->group_size);
    if (cfg->walker_offset % (uint32_t)cfg->group_size)
        return fail(nullptr, MCMC_HIP_ERR_ARG, "walker_offset must be a multiple of group_size");
    if (!(cfg->temperature > 0) || !(cfg->proposal_scale > 0))
        return fail(nullptr, MCMC_HIP_ERR_ARG, "temperature and proposal_scale must be > 0");
    if (cfg->flags & ~(MCMC_HIP_FLAG_INCREMENTAL | MCMC_HIP_FLAG_OWN_BASIS | MCMC_HIP_FLAG_BASIS_GROUP_MASK))
        return fail(nullptr, MCMC_HIP_ERR_ARG, "unknown flags 0x%x", (unsigned)cfg->flags);
    {
        const int m = (cfg->flags & MCMC_HIP_FLAG_BASIS_GROUP_MASK) >> 8;
        const long long bgs = (long long)cfg->group_size << m;
        if (m && (!(cfg->flags & MCMC_HIP_FLAG_INCREMENTAL) || m > 6 || cfg->n_walkers % bgs ||
                  cfg->walker_offset % bgs))
            return fail(nullptr, MCMC_HIP_ERR_ARG,
                        "a basis group wider than group_size needs incremental evaluation, and "
                        "n_walkers and walker_offset must be multiples of it (%lld)", bgs);
    }
    if ((cfg->flags & MCMC_HIP_FLAG_INCREMENTAL) && (cfg->flags & MCMC_HIP_FLAG_OWN_BASIS))
        return fail(nullptr, MCMC_HIP_ERR_ARG,
                    "incremental evaluation needs the shared basis (the whitened direction is "
                    "shared with it)");
    if ((cfg->flags & MCMC_HIP_FLAG_INCREMENTAL) &&
        (cfg->d < 2 || cfg->group_size % 64 != 0 || !mcmc_hip_launch_whiten_state))
        return fail(nullptr, MCMC_HIP_ERR_ARG,
                    "incremental evaluation needs d >= 2 and a group_size that is a multiple of 64");
    if (cfg->emit_capacity < 0 || cfg->burn_in < 0)
        return fail(nullptr, MCMC_HIP_ERR_ARG, "emit_capacity and burn_in must be >= 0");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, MCMC_HIP_ERR_DEVICE, "no HIP device available (%s)",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, MCMC_HIP_ERR_ARG, "device %d out of range (0..%d)", cfg->device,
                    ndev - 1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, MCMC_HIP_ERR_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MCMC_HIP_ERR_DEVICE,
                    "device %d is %s; this library is built for gfx950 only", cfg->device,
                    prop.gcnArchName);
    if (hipSetDevice(cfg->device) != hipSuccess)
        return fail(nullptr, MCMC_HIP_ERR_DEVICE, "hipSetDevice(%d) failed", cfg->device);
    mcmc_hip_ctx* h = new mcmc_hip_ctx();
    h->cfg = *cfg;
    h->k = k;
    h->kb = kb;
    h->huge = huge;
    // MCMC_HIP_NO_PAIR_BIG (developer switch): keep 32 < d <= 56 on the matrix-core kernel
    h->kp = (kb && !getenv("MCMC_HIP_NO_PAIR_BIG")) ? pair_for_dim(cfg->d) : nullptr;
    h->d = cfg->d;
    h->W = cfg->n_walkers;
    h->gs = cfg->group_size;
    h->G = h->W / h->gs;
    h->bgs = h->gs << ((cfg->flags & MCMC_HIP_FLAG_BASIS_GROUP_MASK) >> 8);
    h->BG = h->W / h->bgs;
    h->shift.assign(h->d, 0.0);
    h->incremental = (cfg->flags & MCMC_HIP_FLAG_INCREMENTAL) != 0;
    h->own_basis = (cfg->flags & MCMC_HIP_FLAG_OWN_BASIS) != 0 && cfg->d > 1;
    // MCMC_HIP_DIR_BUDGET_KIB (test switch): KiB of directions per span of mcmc_hip_step instead of the
    // steppers' 256 and 64 MiB (step_span.h; 1: every span is one cycle)
    if (const char* e = getenv("MCMC_HIP_DIR_BUDGET_KIB"))
        if (atol(e) > 0) h->dir_budget = (size_t)atol(e) << 10;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, MCMC_HIP_ERR_DEVICE, "hipStreamCreate failed");
    }
    const size_t W = h->W, d = h->d, G = h->G, np = d * (d + 1) / 2;
    hipError_t r = hipSuccess;
    auto acc = [&](hipError_t x) { if (r == hipSuccess) r = x; };
    acc(h->x.resize(W * d)); acc(h->logpost.resize(W)); acc(h->logprior.resize(W));
    acc(h->loglike.resize(W)); acc(h->weight_i.resize(W)); acc(h->prej.resize(W));
    acc(h->burn.resize(W)); acc(h->nacc.resize(W)); acc(h->stuck.resize(1));
    acc(h->dT.resize(d * d + 16)); /* +16: wide scalar loads at the end of T */ acc(h->Sg.resize(G * np));
    // the checkpoint's read-out in ONE block (one copy and one fill per checkpoint instead of
    // three and two): [group sums | pooled second moments | accept counter]; `pooled` and
    // `acc_total` are views into it (n = 0: not owned)
    acc(h->gsum.resize(G * d + np + 1));
    if (r == hipSuccess) {
        h->pooled.p = h->gsum.p + G * d;
        h->acc_total.p = reinterpret_cast<unsigned long long*>(h->gsum.p + G * d + np);
    }
    acc(h->dshift.resize(d));
    if (cfg->emit_capacity > 0) {
        acc(h->rows.resize(W * (size_t)cfg->emit_capacity * (d + 4)));
        acc(h->nrows.resize(W));
    }
    // (y is sized when the target is known: [K][d][W])
    // (coherent and mapped: readout_moments_kernel stores into it, mcmc_hip_fetch_moments reads it behind mom_event)
    acc(hipHostMalloc((void**)&h->pin_mom, sizeof(double) * (G * d + np + 2),
                      hipHostMallocCoherent | hipHostMallocMapped));
    if (h->pin_mom) acc(hipHostGetDevicePointer((void**)&h->pin_mom_dev, h->pin_mom, 0));
    acc(hipHostMalloc((void**)&h->pin_T, sizeof(double) * 4 * d * d, hipHostMallocDefault));
    for (auto& e : h->pin_T_done) acc(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    acc(hipEventCreateWithFlags(&h->mom_event, hipEventDisableTiming));
    if (h->incremental) {
        // (LOWEST priority: the step kernel's 1024 workgroups are exactly what the chip holds
        // at once, four per compute unit; a direction kernel that took some of those places
        // first would push the displaced step workgroups into a second round -- 1.74 ms
        // instead of 1.22, measured with the order of the two reversed.  The direction kernels
        // run behind the step kernel, beside the moment snapshot: step_incremental.)
        int prio_least = 0, prio_greatest = 0;
        acc(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        acc(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, prio_least));
        acc(hipEventCreateWithFlags(&h->mark, hipEventDisableTiming));
        acc(hipEventCreateWithFlags(&h->T_event, hipEventDisableTiming));
        if (const char* e = getenv("MCMC_HIP_EAGER_DIRECTIONS")) h->lazy_dirs = !(e[0] && e[0] != '0');
        // MCMC_HIP_LOOKAHEAD (developer switch): calls per direction set of step_inc_kernel; 1: a set per call
        if (const char* e = getenv("MCMC_HIP_LOOKAHEAD")) h->lookahead = std::max(1, atoi(e));
        // MCMC_HIP_DUO (developer switch): 0 = the four-lane kernels always, 1 = the two-lane ones wherever they serve
        if (const char* e = getenv("MCMC_HIP_DUO")) h->duo = (e[0] && e[0] != '0') ? 1 : 0;
        // MCMC_HIP_ACCEPT_SLACK (test switch): how far the accept variate's estimate must be from delta to
        // decide a step of the two-lane kernels; inf = every step takes the exact branch
        // (never below kAcceptSlack, what the proof at accept_lanes needs: a smaller or unparsable value is
        // the default; a NaN makes every step exact like inf)
        if (const char* e = getenv("MCMC_HIP_ACCEPT_SLACK")) {
            const double v = strtod(e, nullptr);
            h->accept_slack = v < mcmc::kAcceptSlack ? mcmc::kAcceptSlack : v;
        }
        for (auto& D : h->dirs) acc(hipEventCreateWithFlags(&D.ready, hipEventDisableTiming));
        // MCMC_HIP_NO_PREFETCH (developer switch): directions on the main stream, in line
        h->prefetch = !getenv("MCMC_HIP_NO_PREFETCH");
    }
    if (r == hipSuccess) r = hipMemsetAsync(h->gsum.p, 0, sizeof(double) * G * d, h->stream);
    if (r == hipSuccess) r = hipMemsetAsync(h->pooled.p, 0, sizeof(double) * np, h->stream);
    if (r == hipSuccess) r = hipMemsetAsync(h->dshift.p, 0, sizeof(double) * d, h->stream);
    if (r == hipSuccess) r = hipMemsetAsync(h->stuck.p, 0, sizeof(int), h->stream);
    if (r == hipSuccess) r = hipMemsetAsync(h->acc_total.p, 0, sizeof(unsigned long long), h->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(h->stream);
    if (r != hipSuccess) {
        fail(nullptr, MCMC_HIP_ERR_DEVICE, "device allocation failed: %s", hipGetErrorString(r));
        mcmc_hip_destroy(h);
        return MCMC_HIP_ERR_DEVICE;
    }
    *out = h;
    return MCMC_HIP_OK;
}

void mcmc_hip_destroy(mcmc_hip_ctx* h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    resolve_timing(h);
    for (auto e : h->pool) (void)hipEventDestroy(e);
    for (auto& D : h->dirs) {
        D.V.release(); D.Vf.release(); D.VU.release(); D.vflag.release(); D.vflag_f.release(); D.UU.release();
        D.colflag.release(); D.VW.release(); D.NL.release();
        if (D.ready) (void)hipEventDestroy(D.ready);
    }
    if (h->mark) (void)hipEventDestroy(h->mark);
    if (h->T_event) (void)hipEventDestroy(h->T_event);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    h->x.release(); h->logpost.release(); h->logprior.release(); h->loglike.release();
    h->hV.release(); h->hScratch.release(); h->hCols.release();
    h->cblock.release(); h->dT.release(); h->V.release(); h->rows.release(); h->gsum.release();
    h->Sg.release(); h->pooled.p = nullptr; /* (a view into gsum) */ h->dshift.release(); h->ex.release(); h->elp.release();
    h->ell.release(); h->eder.release(); h->escratch.release(); h->dLrow.release();
    h->dLcol.release(); h->weight_i.release(); h->prej.release();
    h->burn.release(); h->stuck.release(); h->nrows.release(); h->nacc.release();
    h->acc_total.p = nullptr;   // (a view into gsum)
    h->dblk.release(); h->vflag.release(); h->vflag_f.release(); h->Vf.release(); h->drag_cs.release();
    for (auto& sl : h->slots)
        if (sl.p) (void)hipHostFree(sl.p);
    h->ck.ring.release(); h->ck.wsum.release(); h->ck.payload.release(); h->ck.ws.release();
    h->ck.out.release(); h->ck.acc_prev.release();
    h->bd.ring.release(); h->bd.bounds.release(); h->bd.payload.release();
    if (h->bd.pin) (void)hipHostFree(h->bd.pin);
    if (h->ck.pin_out) (void)hipHostFree(h->ck.pin_out);
    destroy_product(h->mg); destroy_product(h->ac); destroy_product(h->bf);
    destroy_product(h->evd); destroy_product(h->dv); destroy_product(h->imp);
    h->imp.hist.destroy();   // (the second read-out of the importance: its reweighted histograms)
    if (h->ck.ev) (void)hipEventDestroy(h->ck.ev);
    if (h->pin_mom) (void)hipHostFree(h->pin_mom);
    if (h->pin_T) (void)hipHostFree(h->pin_T);
    for (auto& e : h->pin_T_done) if (e) (void)hipEventDestroy(e);
    if (h->mom_event) (void)hipEventDestroy(h->mom_event);
    h->pack_out.release(); h->pack_off.release();
    h->y.release(); h->amode.release(); h->inc_prior.release(); h->inc_Lrow.release();
    h->inc_mean.release();
    {
        auto& B = h->bg;
        B.bjs.release(); B.es.release(); B.Afused.release();
        B.resp.release(); B.theta0.release(); B.Astream.release(); B.weights.release();
        B.X.release(); B.dbins.release(); B.delta.release(); B.trial.release(); B.lp_t.release();
        B.Ea.release(); B.psum.release(); B.epsum.release(); B.edelta.release(); B.etrial.release(); B.elp.release();
        B.echi2.release(); B.ecl.release(); B.eA.release();
    }
    h->fnt.points.release(); h->fnt.lp_t.release(); h->fnt.Ea.release(); h->fnt.ll_t.release();
    h->fnt.bad.release();
    h->mv.q.release();
    h->fnt.dinputs.release(); h->fnt.ll_new.release(); h->fnt.ll_c.release();
    h->fnt.epts.release(); h->fnt.ell.release();
    for (auto& b : h->fnt.pts) b.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int mcmc_hip_set_prior(mcmc_hip_ctx* h, const int32_t* kind, const double* a, const double* b,
                       const int32_t* periodic)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!kind || !a || !b) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    const int d = h->d;
    const double inf = std::numeric_limits<double>::infinity();
    h->kind.assign(kind, kind + d);
    h->periodic.assign(d, 0);
    h->lo.assign(d, -inf); h->hi.assign(d, inf);
    h->loc.assign(d, 0.0); h->scale.assign(d, 1.0); h->mls.assign(d, 0.0);
    h->norm_mask = h->periodic_mask = 0;
    h->norm_mask4[0] = h->norm_mask4[1] = h->norm_mask4[2] = h->norm_mask4[3] = 0;
    h->any_periodic = false;
    double ulp = 0.0;
    for (int i = 0; i < d; ++i) {
        if (kind[i] == 0) {
            if (!(b[i] > a[i]) || !std::isfinite(a[i]) || !std::isfinite(b[i]))
                return fail(h, MCMC_HIP_ERR_ARG, "uniform prior %d needs finite min < max", i);
            h->lo[i] = a[i]; h->hi[i] = b[i];
            ulp += std::log(b[i] - a[i]);
            if (periodic && periodic[i]) {
                if (h->huge)
                    return fail(h, MCMC_HIP_ERR_ARG, "d=%d > %d: periodic parameters are not served (prior %d)",
                                d, kMaxDimBig, i);
                h->periodic[i] = 1;
                h->any_periodic = true;
                if (i < 32) h->periodic_mask |= 1u << i;
            }
        } else if (kind[i] == 1) {
            if (!(b[i] > 0) || !std::isfinite(a[i]) || !std::isfinite(b[i]))
                return fail(h, MCMC_HIP_ERR_ARG, "normal prior %d needs finite loc, scale > 0", i);
            if (periodic && periodic[i])
                return fail(h, MCMC_HIP_ERR_ARG,
                            "parameter %d cannot be periodic if it is not bounded", i);
            h->loc[i] = a[i]; h->scale[i] = b[i];
            h->mls[i] = -std::log(b[i]) - std::log(2.0 * M_PI) / 2.0;  // tools.py:723
            if (i < 128) h->norm_mask4[i >> 5] |= 1u << (i & 31);   // (d > 128: h->kind)
            if (i < 32) h->norm_mask |= 1u << i;
        } else {
            return fail(h, MCMC_HIP_ERR_ARG,
                        "prior kind %d of parameter %d is not supported (0 uniform, 1 norm)",
                        kind[i], i);
        }
    }
    h->uniform_logp = -ulp;  // prior.py:528-533
    h->have_prior = true;
    ++h->dir_epoch;
    h->have_state = false;
    return upload_constants(h);
}

int mcmc_hip_set_target_gaussian_mixture(mcmc_hip_ctx* h, int32_t n_modes, const double* means,
                                         const double* covs, const double* weights)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!means || !covs) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    return set_target_common(h, n_modes, means, covs, weights, true);
}

int mcmc_hip_set_target_gaussian(mcmc_hip_ctx* h, const double* mean, const double* cov,
                                 int32_t normalized)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!mean || !cov) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    return set_target_common(h, 1, mean, cov, nullptr, normalized != 0);
}

int mcmc_hip_set_target_one(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    h->K = 0;
    h->bg.on = false;
    h->fnt.on = false;
    h->mean.clear(); h->Linv.clear(); h->cnorm.clear(); h->weight.clear();
    h->have_target = true;
    ++h->dir_epoch;
    h->have_state = false;
    return upload_constants(h);
}

int mcmc_hip_get_derived_constants(const mcmc_hip_ctx* h, double* uniform_logp, double* mls,
                                   double* Linv, double* cnorm, double* weight)
{
    if (!h || !h->have_prior || !h->have_target) return MCMC_HIP_ERR_STATE;
    if (uniform_logp) *uniform_logp = h->uniform_logp;
    if (mls) std::copy(h->mls.begin(), h->mls.end(), mls);
    if (Linv) std::copy(h->Linv.begin(), h->Linv.end(), Linv);
    if (cnorm) std::copy(h->cnorm.begin(), h->cnorm.end(), cnorm);
    if (weight) std::copy(h->weight.begin(), h->weight.end(), weight);
    return MCMC_HIP_OK;
}

int mcmc_hip_set_blocking(mcmc_hip_ctx* h, int32_t n_blocks, const int32_t* block_size,
                          const int32_t* oversampling, const int32_t* i_of_j,
                          int32_t drag_last_slow, int32_t drag_steps)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!block_size || !oversampling || !i_of_j) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    if (h->huge && (n_blocks != 1 || drag_last_slow >= 0))
        return fail(h, MCMC_HIP_ERR_ARG,
                    "d=%d > %d samples one parameter block (blocking / oversampling / drag are not served)",
                    h->d, kMaxDimBig);
    const int d = h->d;
    // (d > 32 from scratch: the general kernels -- step_general_kernel, drag_general_kernel)
    if (n_blocks < 1 || n_blocks > 32)
        return fail(h, MCMC_HIP_ERR_ARG, "n_blocks must be in 1..32, got %d", n_blocks);
    int total = 0;
    bool trivial = n_blocks == 1;
    for (int b = 0; b < n_blocks; ++b) {
        if (block_size[b] < 1) return fail(h, MCMC_HIP_ERR_ARG, "empty parameter block %d", b);
        if (oversampling[b] < 1)   // proposal.py:131-137
            return fail(h, MCMC_HIP_ERR_ARG, "Oversampling factors must be integer! Got %d.",
                        oversampling[b]);
        total += block_size[b];
        trivial = trivial && oversampling[b] == 1;
    }
    std::vector<char> seen(d, 0);
    if (total == d)
        for (int j = 0; j < d; ++j) {
            if (i_of_j[j] < 0 || i_of_j[j] >= d || seen[i_of_j[j]]) { total = -1; break; }
            seen[i_of_j[j]] = 1;
            trivial = trivial && i_of_j[j] == j;
        }
    if (total != d)   // proposal.py:153-156
        return fail(h, MCMC_HIP_ERR_ARG, "The blocks do not contain all the parameter indices.");
    if (drag_last_slow >= 0) {
        if (drag_last_slow > n_blocks - 2)   // proposal.py:143-150: a fast block must remain
            return fail(h, MCMC_HIP_ERR_ARG,
                        "The index given for the last slow block, %d, is not valid: there are "
                        "only %d blocks.", drag_last_slow, n_blocks);
        if (drag_steps < 1 || drag_steps > 256)
            return fail(h, MCMC_HIP_ERR_ARG, "drag_steps must be in 1..256, got %d", drag_steps);
        // (emitted rows, emit_capacity > 0: the from-scratch drag_kernel -- d <= 32 --; the
        // incremental dragging kernel does not emit and refuses at mcmc_hip_step)
        trivial = false;
    } else {
        drag_last_slow = -1;
        drag_steps = 0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->blocked = !trivial;
    ++h->dir_epoch;
    h->blk_size.assign(block_size, block_size + n_blocks);
    h->blk_over.assign(oversampling, oversampling + n_blocks);
    h->i_of_j.assign(i_of_j, i_of_j + d);
    h->drag_last_slow = drag_last_slow;
    h->drag_steps = drag_steps;
    for (int w = 0; w < 3; ++w)
        if (block_slots(h, w) > 2048)
            return fail(h, MCMC_HIP_ERR_ARG, "a cycle of %d steps exceeds the supported 2048",
                        block_slots(h, w));
    std::vector<int> pack;
    pack.insert(pack.end(), h->blk_size.begin(), h->blk_size.end());
    pack.insert(pack.end(), h->blk_over.begin(), h->blk_over.end());
    pack.insert(pack.end(), h->i_of_j.begin(), h->i_of_j.end());
    HIP_TRY(h, h->dblk.resize(pack.size()));
    HIP_TRY(h, hipMemcpy(h->dblk.p, pack.data(), sizeof(int) * pack.size(), hipMemcpyHostToDevice));
    h->have_cov = false;  // the transform depends on the parameter order
    return MCMC_HIP_OK;
}

int mcmc_hip_cycle_length(const mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    return block_slots(h, h->drag_last_slow >= 0 ? 1 : 0);
}

int mcmc_hip_set_proposal_cov(mcmc_hip_ctx* h, const double* cov)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!cov) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    const int d = h->d;
    std::vector<double> corr((size_t)d * d), L((size_t)d * d), sd(d);
    if (!is_symmetric(d, cov))
        return fail(h, MCMC_HIP_ERR_NOT_PD,
                    "The given covmat is not a positive-definite, symmetric square matrix.");
    const std::vector<double> cov_in(cov, cov + (size_t)d * d);
    std::vector<double> sorted_cov;
    if (h->blocked) {  // proposal.py:250-252: reorder by i_of_j before std / corr / Cholesky
        sorted_cov.resize((size_t)d * d);
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j)
                sorted_cov[i * d + j] = cov_in[h->i_of_j[i] * d + h->i_of_j[j]];
        cov = sorted_cov.data();
    }
    for (int i = 0; i < d; ++i) {
        if (!(cov[i * d + i] > 0.0) || !std::isfinite(cov[i * d + i]))
            return fail(h, MCMC_HIP_ERR_NOT_PD,
                        "The given covmat is not a positive-definite, symmetric square matrix.");
        sd[i] = std::sqrt(cov[i * d + i]);
    }
    // tools.py:779-788: corr = cov / std / std^T with unit diagonal
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j)
            corr[i * d + j] = (i == j) ? 1.0 : (1.0 / sd[i]) * cov[i * d + j] * (1.0 / sd[j]);
    if (!cholesky_lower(d, corr.data(), L.data()))
        return fail(h, MCMC_HIP_ERR_NOT_PD,
                    "The given covmat is not a positive-definite, symmetric square matrix.");
    h->cov = cov_in;
    h->T.assign((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) h->T[i * d + j] = h->cfg.proposal_scale * (sd[i] * L[i * d + j]);
    // Stream-ordered, no host synchronisation: launches already queued keep the old transform
    // (their basis kernels precede this copy in the stream), later ones see the new one.  The
    // source is a pinned ring slot that stays untouched for the next three refreshes: before it
    // is written again the host waits for the copy that last read it -- an event recorded four
    // refreshes ago, long complete.  (Rounds 1-5 synchronised the whole stream whenever the ring
    // wrapped: every fourth refresh the host lost its lead of several launches, and the device
    // then idled through the host's pass over the checkpoint -- 275 instead of 96 us between
    // two step kernels, tools/gpu.sh timeline, round 6.)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int k_slot = h->pin_T_slot;
    double* slot = h->pin_T + (size_t)k_slot * d * d;
    h->pin_T_slot = (h->pin_T_slot + 1) & 3;
    HIP_TRY(h, hipEventSynchronize(h->pin_T_done[k_slot]));   // (never recorded: returns at once)
    std::copy(h->T.begin(), h->T.end(), slot);
    // a direction set being filled ahead on the second stream still reads dT: the copy waits for
    // it (that set is stale after ++dir_epoch and is recomputed, but it must not read a torn T)
    for (auto& D : h->dirs)
        if (D.ahead && D.ready) HIP_TRY(h, hipStreamWaitEvent(h->stream, D.ready, 0));
    HIP_TRY(h, hipMemcpyAsync(h->dT.p, slot, sizeof(double) * d * d, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipEventRecord(h->pin_T_done[k_slot], h->stream));
    if (h->T_event) {
        HIP_TRY(h, hipEventRecord(h->T_event, h->stream));
        h->T_fresh = true;
    }
    h->have_cov = true;
    ++h->dir_epoch;
    return MCMC_HIP_OK;
}

int mcmc_hip_get_proposal_cov(const mcmc_hip_ctx* h, double* cov)
{
    if (!h || !cov || !h->have_cov) return MCMC_HIP_ERR_STATE;
    std::copy(h->cov.begin(), h->cov.end(), cov);
    return MCMC_HIP_OK;
}

int mcmc_hip_get_proposal_transform(const mcmc_hip_ctx* h, double* T)
{
    if (!h || !T || !h->have_cov) return MCMC_HIP_ERR_STATE;
    std::copy(h->T.begin(), h->T.end(), T);
    return MCMC_HIP_OK;
}

int mcmc_hip_evaluate(mcmc_hip_ctx* h, int32_t n, const double* x, double* logprior,
                      double* loglike, double* derived)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_prior || !h->have_target)
        return fail(h, MCMC_HIP_ERR_STATE, "set_prior and set_target_* must precede evaluate");
    if (n <= 0 || !x || !logprior || !loglike) return fail(h, MCMC_HIP_ERR_ARG, "bad argument");
    const size_t d = h->d, Kd = (size_t)std::max(h->K, 1) * d;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->bg.on) {
        if (derived) return fail(h, MCMC_HIP_ERR_ARG, "the binned Gaussian target has no derived parameters");
        return evaluate_binned_points(h, n, x, logprior, loglike);
    }
    HIP_TRY(h, h->ex.resize((size_t)n * d));
    HIP_TRY(h, h->elp.resize(n));
    HIP_TRY(h, h->ell.resize(n));
    if (derived) HIP_TRY(h, h->eder.resize((size_t)n * Kd));
    HIP_TRY(h, hipMemcpyAsync(h->ex.p, x, sizeof(double) * n * d, hipMemcpyHostToDevice, h->stream));
    mcmc::EvalArgs a{};
    a.x = h->ex.p; a.logprior = h->elp.p; a.loglike = h->ell.p;
    a.derived = (derived && h->K > 0) ? h->eder.p : nullptr;
    a.cblock = h->cblock.p; a.n = n; a.n_modes = h->K;
    a.norm_mask = h->norm_mask; a.periodic_mask = h->periodic_mask;
    a.uniform_logp = h->uniform_logp;
    for (int q = 0; q < 4; ++q) a.norm_mask4[q] = h->norm_mask4[q];
    if (h->huge) {
        const ConstLayout cl{h->d, std::max(h->K, 0)};
        mcmc::HugeEvalArgs e{};
        e.x = h->ex.p; e.logprior = h->elp.p; e.loglike = h->ell.p; e.derived = a.derived;
        e.prior = h->inc_prior.p; e.scale = h->cblock.p + cl.scale();
        e.Lrow = h->inc_Lrow.p; e.mean = h->inc_mean.p;
        e.cnorm = h->cblock.p + cl.cnorm(); e.mweight = h->cblock.p + cl.weight();
        e.n = n; e.d = h->d; e.dpad = 4 * ((h->d + 3) / 4); e.K = std::max(h->K, 0);
        e.uniform_logp = h->uniform_logp;
        HIP_TRY(h, mcmc_hip_launch_huge_evaluate(&e, h->stream));
    } else if (h->kb) {
        HIP_TRY(h, h->escratch.resize((size_t)n * std::max(h->K, 1)));
        HIP_TRY(h, h->kb->evaluate(a, h->dLrow.p, h->d, h->escratch.p, h->stream));
    } else {
        HIP_TRY(h, h->k->evaluate(a, h->stream));
    }
    if (h->fnt.on && h->fnt.n_fn == 0) {   // the log-prior is the `one` target's; the log-likelihood is the function's
        const int rc = function_call(h, n, h->ex.p, h->ell.p);
        if (rc) return rc;
    }
    HIP_TRY(h, hipMemcpyAsync(logprior, h->elp.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(loglike, h->ell.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (a.derived)
        HIP_TRY(h, hipMemcpyAsync(derived, h->eder.p, sizeof(double) * n * Kd, hipMemcpyDeviceToHost,
                                  h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->fnt.on && h->fnt.n_fn > 0) {   // several functions: every one is called, summed left to right
        auto& F = h->fnt;
        F.last_eval_n = 0;
        F.last_eval.resize((size_t)F.n_fn * n);
        const int rc = functions_evaluate(h, n, x, F.last_eval.data());
        if (rc) return rc;
        for (int w = 0; w < n; ++w) {
            double ll = F.last_eval[w];
            for (int c = 1; c < F.n_fn; ++c) ll = ll + F.last_eval[(size_t)c * n + w];
            loglike[w] = ll;
        }
        F.last_eval_n = n;
    }
    if (h->fnt.on)
        for (int w = 0; w < n; ++w) {
            // (the likelihood is skipped outside the prior support, model.py:650-653: what the
            // batched function returned there is ignored)
            if (std::isinf(logprior[w])) loglike[w] = -INFINITY;
            else if (std::isnan(loglike[w]) || loglike[w] == INFINITY)
                return fail(h, MCMC_HIP_ERR_TARGET,
                            "the function target returned NaN or +inf inside the prior support (point "
                            "%d): a log-likelihood there must be finite or -inf", w);
        }
    return MCMC_HIP_OK;
}

int mcmc_hip_set_state(mcmc_hip_ctx* h, const double* x, int32_t* n_bad)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_prior || !h->have_target)
        return fail(h, MCMC_HIP_ERR_STATE, "set_prior and set_target_* must precede set_state");
    if (!x) return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    const size_t W = h->W, d = h->d;
    std::vector<double> lp(W), ll(W), lpost(W), xt(W * d);
    int rc = mcmc_hip_evaluate(h, (int)W, x, lp.data(), ll.data(), nullptr);
    if (rc) return rc;
    int bad = 0;
    for (size_t w = 0; w < W; ++w) {
        lpost[w] = lp[w] + ll[w];
        if (!std::isfinite(lpost[w])) ++bad;
        for (size_t i = 0; i < d; ++i) xt[i * W + w] = x[w * d + i];
    }
    if (n_bad) *n_bad = bad;
    if (bad)
        return fail(h, MCMC_HIP_ERR_ARG, "%d initial points have a non-finite log-posterior", bad);
    std::vector<int> ones(W, 1), zeros(W, 0), burn(W, h->cfg.burn_in + 1);  // mcmc.py:265
    std::vector<long long> z64(W, 0);
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->x.p, xt.data(), sizeof(double) * W * d, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->logpost.p, lpost.data(), sizeof(double) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->logprior.p, lp.data(), sizeof(double) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->loglike.p, ll.data(), sizeof(double) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->weight_i.p, ones.data(), sizeof(int) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->prej.p, zeros.data(), sizeof(int) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->burn.p, burn.data(), sizeof(int) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->nacc.p, z64.data(), sizeof(long long) * W, hipMemcpyHostToDevice, s));
    if (h->nrows.p)
        HIP_TRY(h, hipMemcpyAsync(h->nrows.p, zeros.data(), sizeof(int) * W, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(h->stuck.p, 0, sizeof(int), s));
    if (h->fnt.bad.p) HIP_TRY(h, hipMemsetAsync(h->fnt.bad.p, 0, sizeof(int), s));
    if (h->fnt.on && h->fnt.n_fn > 0) {   // the components of the evaluation above are the state's
        auto& F = h->fnt;
        if (F.last_eval_n != (int)W) return fail(h, MCMC_HIP_ERR_STATE, "no component log-likelihoods of the state");
        HIP_TRY(h, hipMemcpyAsync(F.ll_c.p, F.last_eval.data(), sizeof(double) * F.n_fn * W, hipMemcpyHostToDevice, s));
        F.llc_valid = true;
    }
    HIP_TRY(h, hipMemsetAsync(h->acc_total.p, 0, sizeof(unsigned long long), s));
    // a fresh start: no thinning remainders from an earlier run (the oracle's State starts at zero;
    // mcmc_hip_set_full_state leaves them alone -- mcmc_hip_set_thin_carry follows it)
    if (h->thin_acc.p) HIP_TRY(h, hipMemsetAsync(h->thin_acc.p, 0, sizeof(int) * W, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->step = 0;
    h->have_state = true;
    h->mv.checked = false; h->mv.broken = false;
    h->y_valid = false; h->amode_valid = false;   // incremental mode: y = L^-1 (x - mu) is formed before the next step
    return MCMC_HIP_OK;
}

int mcmc_hip_get_state(mcmc_hip_ctx* h, double* x, double* logpost, double* logprior,
                       double* loglike, int32_t* weight)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state: call set_state first");
    const size_t W = h->W, d = h->d;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::vector<double> xt;
    if (x) {
        xt.resize(W * d);
        HIP_TRY(h, hipMemcpyAsync(xt.data(), h->x.p, sizeof(double) * W * d, hipMemcpyDeviceToHost, s));
    }
    if (logpost) HIP_TRY(h, hipMemcpyAsync(logpost, h->logpost.p, sizeof(double) * W, hipMemcpyDeviceToHost, s));
    if (logprior) HIP_TRY(h, hipMemcpyAsync(logprior, h->logprior.p, sizeof(double) * W, hipMemcpyDeviceToHost, s));
    if (loglike) HIP_TRY(h, hipMemcpyAsync(loglike, h->loglike.p, sizeof(double) * W, hipMemcpyDeviceToHost, s));
    if (weight) HIP_TRY(h, hipMemcpyAsync(weight, h->weight_i.p, sizeof(int) * W, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (x)
        for (size_t w = 0; w < W; ++w)
            for (size_t i = 0; i < d; ++i) x[w * d + i] = xt[i * W + w];
    return MCMC_HIP_OK;
}

int mcmc_hip_get_full_state(mcmc_hip_ctx* h, double* x, double* logpost, double* logprior,
                            double* loglike, int32_t* weight, int32_t* prior_rej,
                            int32_t* burn_left, int64_t* n_accept, uint64_t* step)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    int rc = mcmc_hip_get_state(h, x, logpost, logprior, loglike, weight);
    if (rc) return rc;
    const size_t W = h->W;
    if (prior_rej) HIP_TRY(h, hipMemcpy(prior_rej, h->prej.p, sizeof(int) * W, hipMemcpyDeviceToHost));
    if (burn_left) HIP_TRY(h, hipMemcpy(burn_left, h->burn.p, sizeof(int) * W, hipMemcpyDeviceToHost));
    if (n_accept) {
        static_assert(sizeof(long long) == sizeof(int64_t), "n_accept layout");
        HIP_TRY(h, hipMemcpy(n_accept, h->nacc.p, sizeof(int64_t) * W, hipMemcpyDeviceToHost));
    }
    if (step) *step = h->step;
    return MCMC_HIP_OK;
}

int mcmc_hip_set_full_state(mcmc_hip_ctx* h, const double* x, const double* logpost,
                            const double* logprior, const double* loglike, const int32_t* weight,
                            const int32_t* prior_rej, const int32_t* burn_left,
                            const int64_t* n_accept, uint64_t step)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_prior || !h->have_target)
        return fail(h, MCMC_HIP_ERR_STATE, "set_prior and set_target_* must precede set_full_state");
    if (!x || !logpost || !logprior || !loglike || !weight || !prior_rej || !burn_left || !n_accept)
        return fail(h, MCMC_HIP_ERR_ARG, "null argument");
    const size_t W = h->W, d = h->d;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<double> xt(W * d);
    for (size_t w = 0; w < W; ++w) {
        if (!std::isfinite(logpost[w]))
            return fail(h, MCMC_HIP_ERR_ARG, "walker %zu has a non-finite log-posterior", w);
        for (size_t i = 0; i < d; ++i) xt[i * W + w] = x[w * d + i];
    }
    HIP_TRY(h, hipMemcpy(h->x.p, xt.data(), sizeof(double) * W * d, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->logpost.p, logpost, sizeof(double) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->logprior.p, logprior, sizeof(double) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->loglike.p, loglike, sizeof(double) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->weight_i.p, weight, sizeof(int) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->prej.p, prior_rej, sizeof(int) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->burn.p, burn_left, sizeof(int) * W, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->nacc.p, n_accept, sizeof(int64_t) * W, hipMemcpyHostToDevice));
    if (h->nrows.p) HIP_TRY(h, hipMemset(h->nrows.p, 0, sizeof(int) * W));
    HIP_TRY(h, hipMemset(h->stuck.p, 0, sizeof(int)));
    if (h->fnt.bad.p) HIP_TRY(h, hipMemset(h->fnt.bad.p, 0, sizeof(int)));
    h->fnt.llc_valid = false;   // several functions: mcmc_hip_set_component_loglikes follows, or they are formed again
    {
        unsigned long long tot = 0;
        for (size_t w = 0; w < W; ++w) tot += (unsigned long long)n_accept[w];
        HIP_TRY(h, hipMemcpy(h->acc_total.p, &tot, sizeof tot, hipMemcpyHostToDevice));
    }
    h->step = step;
    h->have_state = true;
    h->mv.checked = false; h->mv.broken = false;
    h->y_valid = false; h->amode_valid = false;   // incremental mode: mcmc_hip_set_whitened must follow (bit-exact resume)
    return MCMC_HIP_OK;
}

namespace {
// the model, ensemble and build of an engine, as scratch_choose is asked about them (no launch's
// one-parameter column yet)
mcmc::ScratchShape scratch_shape_of(mcmc_hip_ctx* h)
{
    mcmc::ScratchShape s;
    const bool drag = h->drag_last_slow >= 0;
    s.d = h->d; s.K = h->K; s.W = h->W; s.group_size = h->gs;
    s.any_normal = h->norm_mask4[0] || h->norm_mask4[1] || h->norm_mask4[2] || h->norm_mask4[3];
    s.any_periodic = h->any_periodic;
    s.emit = h->cfg.emit_capacity > 0; s.emit_thin = h->emit_thin > 1;
    s.unit_t = h->cfg.temperature == 1.0;
    s.own_basis = h->own_basis; s.blocked = h->blocked;
    s.n_drag = drag ? h->drag_steps : 0;
    // steps (= direction columns) per cycle
    s.cps = block_slots(h, drag ? 1 : 0);
    s.cps_f = drag ? block_slots(h, 2) : 0;
    s.lane_compiled = h->k != nullptr; s.big_dp = h->kb ? h->kb->dp : 0; s.pair_compiled = h->kp != nullptr;
    return s;
}
}  // namespace

int mcmc_hip_scratch_choice(const mcmc_hip_scratch_shape* shape, mcmc_hip_scratch_answer* out)
{
    if (!shape || !out) return MCMC_HIP_ERR_ARG;
    mcmc::ScratchShape s;
    s.d = shape->d; s.K = shape->n_modes; s.W = shape->n_walkers; s.group_size = shape->group_size;
    s.any_normal = shape->any_normal != 0; s.any_periodic = shape->any_periodic != 0;
    s.emit = shape->emit != 0; s.emit_thin = shape->emit_thin != 0; s.unit_t = shape->unit_t != 0;
    s.own_basis = shape->own_basis != 0; s.blocked = shape->blocked != 0; s.n_drag = shape->n_drag;
    s.cps = shape->cps > 0 ? shape->cps : shape->d; s.cps_f = shape->cps_f;
    s.has_1d_column = shape->has_1d_column != 0;
    // what this library was built with, as mcmc_hip_create finds it
    s.lane_compiled = kernels_for_dim(s.d) != nullptr;
    const BigKernels* kb = s.lane_compiled ? nullptr : big_for_dim(s.d);
    s.big_dp = kb ? kb->dp : 0;
    s.pair_compiled = kb && !getenv("MCMC_HIP_NO_PAIR_BIG") && pair_for_dim(s.d) != nullptr;
    const mcmc::ScratchChoice c = mcmc::scratch_choose(s);
    static_assert(mcmc::kScratchStep == MCMC_HIP_SCRATCH_STEP && mcmc::kScratchStepOwn == MCMC_HIP_SCRATCH_STEP_OWN &&
                  mcmc::kScratchPair == MCMC_HIP_SCRATCH_PAIR && mcmc::kScratchMfma == MCMC_HIP_SCRATCH_MFMA &&
                  mcmc::kScratchBigReg == MCMC_HIP_SCRATCH_BIG_REG && mcmc::kScratchGeneral == MCMC_HIP_SCRATCH_GENERAL &&
                  mcmc::kScratchDrag == MCMC_HIP_SCRATCH_DRAG && mcmc::kScratchGeneralDrag == MCMC_HIP_SCRATCH_GENERAL_DRAG,
                  "mcmc_hip.h names the families of scratch_choice.h");
    out->family = c.family; out->reason = c.reason;
    out->multi = c.multi; out->general = c.general; out->unit_t = c.unit_t; out->normp = c.normp;
    out->unit = c.unit; out->walkers_per_wg = c.walkers_per_wg; out->threads = c.threads; out->grid = c.grid;
    out->lds_bytes = (int32_t)c.lds_bytes; out->lds_attr = (int32_t)c.lds_attr;
    out->v_ld = c.v_ld; out->slab = c.slab; out->slab_f = c.slab_f;
    return MCMC_HIP_OK;
}

int mcmc_hip_step(mcmc_hip_ctx* h, int32_t n_steps)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    // (the stretch move and the mixtures of ensemble moves need no proposal covariance)
    const bool stretch = h->mv.kind == MCMC_HIP_MOVE_STRETCH || h->mx.n > 0;
    if (h->mv.kind == MCMC_HIP_MOVE_STRETCH && h->mx.n > 0)
        return fail(h, MCMC_HIP_ERR_ARG,
                    "mcmc_hip_set_moves and mcmc_hip_set_move(MCMC_HIP_MOVE_STRETCH) are both in force: a mixture "
                    "replaces the one move (give the stretch move as a member, or switch one of them off)");
    if (!h->have_state || (!h->have_cov && !stretch))
        return fail(h, MCMC_HIP_ERR_STATE, "set_state and set_proposal_cov must precede step");
    if (n_steps <= 0) return fail(h, MCMC_HIP_ERR_ARG, "n_steps must be > 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (stretch) return step_stretch(h, n_steps);
    if (h->bg.on) return step_binned(h, n_steps);
    if (h->fnt.on) return h->fnt.n_fn > 0 ? step_functions(h, n_steps) : step_function(h, n_steps);
    if (h->incremental && h->huge) return step_huge(h, n_steps);
    if (h->incremental) return step_incremental(h, n_steps);
    // every trial from scratch: which kernel serves the shape and how it is launched is
    // scratch_choose's (scratch_choice.h); only a one-parameter column can differ from span to span
    mcmc::ScratchShape shape = scratch_shape_of(h);
    const mcmc::ScratchChoice whole = mcmc::scratch_choose(shape);
    switch (whole.reason) {
    case mcmc::kScratchServed: break;
    case mcmc::kScratchEmitThin:
        return fail(h, MCMC_HIP_ERR_ARG, "emit_thin needs incremental evaluation; thin on the host");
    case mcmc::kScratchOwnBlocks:
        return fail(h, MCMC_HIP_ERR_ARG,
                    "shared_basis: False serves a single parameter block without dragging");
    case mcmc::kScratchGeneralLds:
        return fail(h, MCMC_HIP_ERR_ARG,
                    "d=%d with %d modes does not fit the general d > 32 kernel (LDS)", h->d, h->K);
    case mcmc::kScratchCycleLds:
        return fail(h, MCMC_HIP_ERR_ARG,
                    "a cycle of %d steps needs %zu KiB of LDS per group: use group_size 256 or "
                    "smaller oversampling factors", shape.cps, (size_t)whole.slab * sizeof(double) / 1024);
    default:   // (kScratchBadShape, kScratchSweepSize, kScratchSweepNormal: what the launchers answered)
        HIP_TRY(h, hipErrorInvalidValue);
    }
    const bool drag = shape.n_drag > 0;
    const int Lc = shape.cps, Lf = shape.cps_f;
    const size_t dd = (size_t)whole.slab, ddf = (size_t)whole.slab_f;
    // basis "groups": the walker groups, or every walker on its own
    const int n_basis = h->own_basis ? h->W : h->G;
    const uint32_t basis0 = h->own_basis ? h->cfg.walker_offset
                                         : h->cfg.walker_offset / (uint32_t)h->gs;
    // directions buffer: at most ~256 MiB of cycles per launch
    const int max_cyc = max_span_cycles(h, 256u << 20, dd, n_basis);
    // dragging: the fast blocks' directions, n_drag columns per step
    const unsigned long long nd = (unsigned long long)h->drag_steps;
    const int max_cyc_f = drag ? max_span_cycles(h, 256u << 20, ddf, h->G, 2) : 0;
    // the arguments of the general d > 32 kernels around those of a launch
    auto general_args = [h, &whole](const mcmc::StepArgs& a) {
        mcmc::GeneralStepArgs g{};
        g.s = a;
        g.Lrow = h->dLrow.p; g.d = h->d; g.ld = whole.v_ld; g.own_basis = h->own_basis ? 1 : 0;
        put_norm_mask4(h, g.norm_mask4);
        periodic_mask4(h, g.periodic_mask4);
        return g;
    };
    int left = n_steps;
    while (left > 0) {
        // (dragging: at most max_cyc_f cycles of fast directions per launch as well)
        const StepSpan sp = drag ? drag_span(h->step, left, Lc, max_cyc, h->drag_steps, Lf, max_cyc_f)
                                 : step_span(h->step, left, Lc, max_cyc);
        const unsigned long long c0 = sp.c0;
        const int n = sp.n, ncyc = sp.ncyc;
        bool any_1d = false;
        {
            Timed t(h, 1);
            const int rc = h->blocked ? blocked_basis(h, drag ? 1 : 0, c0, ncyc, Lc, dd, h->V, h->vflag, any_1d)
                                      : shared_basis(h, h->V, n_basis, basis0, c0, ncyc, dd, h->stream);
            if (rc != MCMC_HIP_OK) return rc;
        }
        {
            Timed t(h, 0);
            mcmc::StepArgs a = step_args(h);
            a.rows = h->rows.p; a.n_rows = h->nrows.p; a.row_cap = h->cfg.emit_capacity;
            a.V = h->V.p; a.n_modes = h->K;
            a.periodic_mask = h->periodic_mask;
            a.step0 = h->step; a.n_steps = n; a.ncyc = ncyc;
            a.cnorm0 = h->K > 0 ? h->cnorm[0] : 0.0;
            a.cps = Lc; a.slab = (int)dd;
            a.vflag = any_1d ? h->vflag.p : nullptr;
            a.own_basis = (h->own_basis && !h->kb) ? 1 : 0;
            shape.has_1d_column = any_1d;
            const mcmc::ScratchChoice c = mcmc::scratch_choose(shape);
            if (c.family == mcmc::kScratchDrag || c.family == mcmc::kScratchGeneralDrag) {
                mcmc::DragArgs g{};
                g.s = a;
                const unsigned long long f0 = h->step * nd;
                const unsigned long long f1 = (h->step + (unsigned long long)n) * nd - 1;
                g.cyc0 = c0;
                g.cyc0_f = f0 / (unsigned long long)Lf;
                g.ncyc_f = (int)(f1 / (unsigned long long)Lf - g.cyc0_f + 1);
                g.cps_f = Lf; g.slab_f = (int)ddf; g.n_drag = h->drag_steps;
                bool any_1d_f = false;
                const int rc = blocked_basis(h, 2, g.cyc0_f, g.ncyc_f, Lf, ddf, h->Vf, h->vflag_f,
                                             any_1d_f);
                if (rc != MCMC_HIP_OK) return rc;
                g.Vf = h->Vf.p;
                g.vflag_f = any_1d_f ? h->vflag_f.p : nullptr;
                if (c.family == mcmc::kScratchGeneralDrag) {   // 32 < d <= 128
                    mcmc::GeneralDragArgs q{};
                    q.g = general_args(a);
                    HIP_TRY(h, h->drag_cs.resize((size_t)h->d * h->W));
                    q.Vf = g.Vf; q.vflag_f = g.vflag_f; q.cs = h->drag_cs.p;
                    q.cyc0 = g.cyc0; q.cyc0_f = g.cyc0_f; q.cps_f = g.cps_f; q.slab_f = g.slab_f;
                    q.ncyc_f = g.ncyc_f; q.n_drag = g.n_drag;
                    HIP_TRY(h, mcmc_hip_launch_general_drag(&q, &c, h->stream));
                } else {
                    HIP_TRY(h, h->k->drag(g, c, h->stream));
                }
            } else if (c.family == mcmc::kScratchGeneral) {
                const mcmc::GeneralStepArgs g = general_args(a);
                HIP_TRY(h, mcmc_hip_launch_general_step(&g, &c, h->stream));
            } else if (h->kb) {
                a.norm_mask = h->norm_mask4[0];
                a.norm_mask_hi = h->norm_mask4[1];
                if (c.family == mcmc::kScratchPair) HIP_TRY(h, h->kp(&a, &c, h->stream));
                else HIP_TRY(h, h->kb->step(a, h->dLcol.p, h->d, h->norm_mask4, c, h->stream));
            }
            else HIP_TRY(h, h->k->step(a, c, h->stream));
            h->n_step_launches += 1;
            take_noted_kernel(h);
        }
        h->step += (unsigned long long)n;
        left -= n;
    }
    return MCMC_HIP_OK;
}

int mcmc_hip_sync(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));   // directions computed ahead
    resolve_timing(h);
    if (h->fnt.on) {
        int bad = 0;
        HIP_TRY(h, hipMemcpy(&bad, h->fnt.bad.p, sizeof(int), hipMemcpyDeviceToHost));
        if (bad) return function_target_error(h, bad);
    }
    int stuck = 0;
    HIP_TRY(h, hipMemcpy(&stuck, h->stuck.p, sizeof(int), hipMemcpyDeviceToHost));
    if (stuck)
        return fail(h, MCMC_HIP_ERR_STUCK,
                    "The chain has been stuck for %g attempts (walker %d), stopping sampling.",
                    h->cfg.max_tries, stuck - 1);
    return MCMC_HIP_OK;
}

int mcmc_hip_get_counters(mcmc_hip_ctx* h, int64_t counters[4])
{
    if (!h || !counters) return MCMC_HIP_ERR_ARG;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    unsigned long long tot = 0;
    HIP_TRY(h, hipMemcpy(&tot, h->acc_total.p, sizeof tot, hipMemcpyDeviceToHost));
    int stuck = 0;
    HIP_TRY(h, hipMemcpy(&stuck, h->stuck.p, sizeof(int), hipMemcpyDeviceToHost));
    int64_t dropped = 0;
    if (h->nrows.p) {
        std::vector<int> nr(h->W);
        HIP_TRY(h, hipMemcpy(nr.data(), h->nrows.p, sizeof(int) * h->W, hipMemcpyDeviceToHost));
        for (auto v : nr) dropped += std::max(0, v - h->cfg.emit_capacity);
    }
    counters[0] = (int64_t)h->step;
    counters[1] = (int64_t)tot;
    counters[2] = stuck;
    counters[3] = dropped;
    return MCMC_HIP_OK;
}

int mcmc_hip_set_moment_shift(mcmc_hip_ctx* h, const double* shift)
{
    if (!h || !shift) return MCMC_HIP_ERR_ARG;
    if (h->n_snapshots != 0)
        return fail(h, MCMC_HIP_ERR_STATE, "the moment shift can only change right after a reset");
    const bool changed = !std::equal(h->shift.begin(), h->shift.end(), shift);
    h->shift.assign(shift, shift + h->d);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(h->dshift.p, h->shift.data(), sizeof(double) * h->d,
                              hipMemcpyHostToDevice, h->stream));
    if (changed && h->ac.ro.on()) {
        // the autocorrelation ring's group sums and the open accumulators refer to the old shift
        h->ac.held = h->ac.head = 0;
        std::fill(h->ac.n_pairs.begin(), h->ac.n_pairs.end(), (int64_t)0);
        HIP_TRY(h, hipMemsetAsync(h->ac.ro.slab, 0, h->ac.ro.bytes(), h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MCMC_HIP_OK;
}

int mcmc_hip_accumulate_moments(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    Timed t(h, 2);
    mcmc::MomentArgs a{};
    a.x = h->x.p; a.shift = h->dshift.p; a.group_sum = h->gsum.p; a.Sg = h->Sg.p;
    a.pooled = h->pooled.p; a.W = h->W; a.G = h->G;
    if (h->huge) HIP_TRY(h, mcmc_hip_launch_huge_moments(&a, h->gs, h->d, h->stream));
    else if (h->kb) HIP_TRY(h, h->kb->moments(a, h->gs, h->d, h->stream));
    else HIP_TRY(h, h->k->moments(a, h->gs, h->stream));
    h->n_snapshots += 1;
    return MCMC_HIP_OK;
}

int mcmc_hip_read_moments(mcmc_hip_ctx* h, int64_t* n_snapshots, double* group_sum,
                          double* pooled_S, int32_t reset)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));   // (events of the direction kernels)
    resolve_timing(h);
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2;
    if (n_snapshots) *n_snapshots = h->n_snapshots;
    if (group_sum)
        HIP_TRY(h, hipMemcpy(group_sum, h->gsum.p, sizeof(double) * G * d, hipMemcpyDeviceToHost));
    if (pooled_S) {
        std::vector<double> p(np);
        HIP_TRY(h, hipMemcpy(p.data(), h->pooled.p, sizeof(double) * np, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < d; ++i)
            for (size_t j = 0; j <= i; ++j)
                pooled_S[i * d + j] = pooled_S[j * d + i] = p[i * (i + 1) / 2 + j];
    }
    if (reset) {
        HIP_TRY(h, hipMemset(h->gsum.p, 0, sizeof(double) * G * d));
        HIP_TRY(h, hipMemset(h->pooled.p, 0, sizeof(double) * np));
        h->n_snapshots = 0;
    }
    return MCMC_HIP_OK;
}

int mcmc_hip_set_moments(mcmc_hip_ctx* h, int64_t n_snapshots, const double* group_sum,
                         const double* pooled_S)
{
    if (!h || !group_sum || !pooled_S || n_snapshots < 0) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2;
    std::vector<double> p(np);
    for (size_t i = 0; i < d; ++i)
        for (size_t j = 0; j <= i; ++j) p[i * (i + 1) / 2 + j] = pooled_S[i * d + j];
    HIP_TRY(h, hipMemcpy(h->gsum.p, group_sum, sizeof(double) * G * d, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->pooled.p, p.data(), sizeof(double) * np, hipMemcpyHostToDevice));
    h->n_snapshots = n_snapshots;
    return MCMC_HIP_OK;
}

int mcmc_hip_request_moments(mcmc_hip_ctx* h)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->have_state) return fail(h, MCMC_HIP_ERR_STATE, "no state");
    if (h->mom_pending) return fail(h, MCMC_HIP_ERR_STATE, "a moment request is already pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2;
    hipStream_t s = h->stream;
    // gsum, pooled and the accept counter are one block; the stuck flag travels with the read-out
    // (the spare word behind the accept counter): the run loop never synchronises, so this is
    // where a walker that tripped max_tries is seen (mcmc.py:717-743 stops at once); a function
    // target's error flag is the other half of that word.  ONE kernel stores all of it to its
    // places in the pinned block and zeroes the accumulators in the same pass (two or three
    // device-to-host copies and a fill before: four dependent blits, all latency).
    // (with the device-side checkpoint the accumulators are reset by ckpt_window_kernel, which
    // first files them in the ring: mcmc_hip_checkpoint_begin must follow)
    {
        const size_t n_acc = G * d + np;
        hipLaunchKernelGGL(mcmc::readout_moments_kernel, dim3((unsigned)((n_acc + 1 + 255) / 256)),
                           dim3(256), 0, s, reinterpret_cast<unsigned long long*>(h->gsum.p), n_acc,
                           (const int*)h->stuck.p, h->fnt.on ? (const int*)h->fnt.bad.p : nullptr,
                           h->pin_mom_dev, h->ck.ring.p ? 0 : 1);
        HIP_TRY(h, hipGetLastError());
    }
    h->mom_fn = h->fnt.on;
    HIP_TRY(h, hipEventRecord(h->mom_event, s));
    h->mom_n = h->n_snapshots;
    h->mom_step = h->step;
    h->n_snapshots = 0;
    h->mom_pending = true;
    return MCMC_HIP_OK;
}

int mcmc_hip_fetch_moments(mcmc_hip_ctx* h, int64_t* n_snapshots, double* group_sum,
                           double* pooled_S, int64_t counters[2])
{
    if (!h) return MCMC_HIP_ERR_ARG;
    if (!h->mom_pending) return fail(h, MCMC_HIP_ERR_STATE, "no moment request is pending");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(h->mom_event));
    h->mom_pending = false;
    const size_t d = h->d, G = h->G, np = d * (d + 1) / 2;
    if (n_snapshots) *n_snapshots = h->mom_n;
    if (group_sum) std::copy(h->pin_mom, h->pin_mom + G * d, group_sum);
    if (pooled_S) {
        const double* p = h->pin_mom + G * d;
        for (size_t i = 0; i < d; ++i)
            for (size_t j = 0; j <= i; ++j)
                pooled_S[i * d + j] = pooled_S[j * d + i] = p[i * (i + 1) / 2 + j];
    }
    if (counters) {
        unsigned long long tot;
        std::memcpy(&tot, h->pin_mom + G * d + np, sizeof tot);
        counters[0] = (int64_t)h->mom_step;
        counters[1] = (int64_t)tot;
    }
    if (h->mom_fn) {
        int bad = 0;
        std::memcpy(&bad, reinterpret_cast<const int*>(h->pin_mom + G * d + np + 1) + 1, sizeof bad);
        if (bad) return function_target_error(h, bad);
    }
    int stuck = 0;
    std::memcpy(&stuck, h->pin_mom + G * d + np + 1, sizeof stuck);
    if (stuck)
        return fail(h, MCMC_HIP_ERR_STUCK,
                    "The chain has been stuck for %g attempts (walker %d), stopping sampling.",
                    h->cfg.max_tries, stuck - 1);
    return MCMC_HIP_OK;
}

void mcmc_hip_note_step_kernel(const char* name) { g_noted_kernel = name; }

const char* mcmc_hip_last_step_kernel(const mcmc_hip_ctx* h)
{
    return h ? h->last_step_kernel.c_str() : "";
}

int mcmc_hip_enable_timing(mcmc_hip_ctx* h, int32_t on)
{
    if (!h) return MCMC_HIP_ERR_ARG;
    h->timing = on != 0;
    return MCMC_HIP_OK;
}

uint64_t mcmc_hip_stream_handle(const mcmc_hip_ctx* h) { return h ? (uint64_t)(uintptr_t)h->stream : 0; }

int mcmc_hip_kernel_times(mcmc_hip_ctx* h, double ms[3], int64_t* n_step_launches, int32_t reset)
{
    if (!h || !ms) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));   // (events of the direction kernels)
    resolve_timing(h);
    for (int i = 0; i < 3; ++i)   // (kinds 1 and 2 are sampled: scaled to all their regions)
        ms[i] = h->n_timed[i] > 0 ? h->ms[i] * ((double)h->n_seen[i] / (double)h->n_timed[i]) : 0.0;
    if (h->bg.on) ms[0] = h->ms[3] + h->ms[4] + h->ms[5];   // the three kernels of a step
    if (n_step_launches) *n_step_launches = h->n_step_launches;
    if (reset) {
        for (int i = 0; i < 6; ++i) { h->ms[i] = 0.0; h->n_seen[i] = h->n_timed[i] = 0; }
        h->n_step_launches = 0;
    }
    return MCMC_HIP_OK;
}

int mcmc_hip_binned_kernel_times(mcmc_hip_ctx* h, double ms[3], int64_t n_launches[3], int32_t reset)
{
    if (!h || !ms || !n_launches) return MCMC_HIP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    resolve_timing(h);
    for (int i = 0; i < 3; ++i) {
        ms[i] = h->ms[3 + i];
        n_launches[i] = h->n_timed[3 + i];
        if (reset) { h->ms[3 + i] = 0.0; h->n_seen[3 + i] = h->n_timed[3 + i] = 0; }
    }
    return MCMC_HIP_OK;
}

}  // extern "C"
