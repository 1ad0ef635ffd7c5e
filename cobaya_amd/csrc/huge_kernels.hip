// Kernels of the dimensions 128 < d <= 256 (run-time d; one parameter block, incremental
// evaluation of up to four Gaussian modes).  Every sum follows the d > 32 order of the
// specification (four interleaved chains over i mod 4, combined (s0 + s1) + (s2 + s3)), so the
// results equal the oracle's bit for bit (docs/KERNELS.md "The d > 128 kernels").
//   huge_reflect_kernel   the (d+2)(d-1)/2 normals of a (group, cycle), then the norm, sign, pivot
//                         and denominator of every reflection (one thread each) and the reflectors
//                         normalised in place -- in a device scratch slab, not LDS (H alone is
//                         d^2 doubles: 512 KiB at d = 256)
//   huge_rows_kernel      the d - 1 reflections of 64 rows of H, four lanes per row (lane class c
//                         owns the columns j = c mod 4), the rows in LDS; no barrier -- a row needs
//                         its own four lanes and the read-only reflectors; R = D H to the slab
//   huge_product_kernel   V = T R, one thread per (row, column), the ascending chain over k
//   huge_dirs_kernel      per (basis group, step): v, u_k = L_k^-1 v, w = v / s^2, |u|^2, v.w, loc.w
//   huge_step_kernel      the incremental Metropolis step, one lane per walker: x [d][W] and y
//                         [K][d][W] streamed from HBM, the carried log-densities in registers;
//                         K = 0 (the `one` likelihood) takes the from-scratch step of orc_run:
//                         the un-paired variates, the prior's division by the scale, ll = 0
//   huge_evaluate_kernel  log-prior / log-likelihood of points from scratch (eval_point)
//   huge_group_moments_kernel, huge_pool_moments_kernel   sufficient statistics of the ensemble
#include <algorithm>
#include "det_math.h"
#include "huge_args.h"
#include "kernels.h"

namespace mcmc {
namespace {

__host__ __device__ constexpr int huge_refl_offset(int n, int d) { return n * d - n * (n - 1) / 2; }
__host__ __device__ constexpr long long huge_sign_offset(int d) { return (long long)(d + 2) * (d - 1) / 2 + 2; }
__host__ __device__ constexpr long long huge_r_offset(int d)
{
    return (((long long)(d + 2) * (d - 1) / 2 + 2 + d + 1) & ~1ll);
}

// ---------------------------------------------------------------- Haar basis
__global__ void __launch_bounds__(256) huge_reflect_kernel(const HugeBasisArgs a)
{
    const int d = a.d, tid = threadIdx.x;
    const int s = a.slab0 + (int)blockIdx.x;
    const uint32_t group = a.group0 + (uint32_t)(s / a.ncyc);
    const uint32_t cycle = a.cycle0 + (uint32_t)(s % a.ncyc);
    double* __restrict__ Z = a.scratch + (size_t)blockIdx.x * (size_t)huge_basis_scratch(d);
    double* __restrict__ sgn = Z + huge_sign_offset(d);
    const int nz = (d + 2) * (d - 1) / 2;
    for (int j = tid; 2 * j < nz; j += blockDim.x) {
        const u32x4 w4 = philox4x32_10(a.key0, a.key1, group, kStreamBasis, cycle, (uint32_t)j);
        const uint64_t ka = ((uint64_t)w4.w0 << 20) | (w4.w1 >> 12);
        const uint64_t kb = ((uint64_t)w4.w2 << 20) | (w4.w3 >> 12);
        const double rad = sqrt(-2.0 * dlog(u52(ka)));
        double sn, cs;
        sincos2pi(kb, sn, cs);
        Z[2 * j] = rad * cs;
        Z[2 * j + 1] = rad * sn;   // (2 j + 1 <= nz: inside the two doubles of padding)
    }
    __syncthreads();
    for (int n = tid; n < d - 1; n += blockDim.x) {   // reflection n: its own segment of Z only
        const int m = d - n, ix = huge_refl_offset(n, d);
        double norm2 = 0.0;
        for (int k = 0; k < m; ++k) norm2 = fma(Z[ix + k], Z[ix + k], norm2);
        const double x0 = Z[ix];
        const double Dn = (x0 < 0.0) ? -1.0 : 1.0;
        const double x0n = x0 + Dn * sqrt(norm2);
        double tt = norm2 - x0 * x0;
        tt = tt + x0n * x0n;
        const double den = sqrt(0.5 * tt);
        Z[ix] = x0n / den;
        for (int k = 1; k < m; ++k) Z[ix + k] = Z[ix + k] / den;
        sgn[n] = Dn;
    }
    __syncthreads();
    if (tid == 0) {   // the last sign closes det = +1 (product of the signs in order: exact)
        double dprod = 1.0;
        for (int n = 0; n < d - 1; ++n) dprod *= sgn[n];
        sgn[d - 1] = (((d - 1) & 1) ? -1.0 : 1.0) * dprod;
    }
}

__global__ void __launch_bounds__(256) huge_rows_kernel(const HugeBasisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int d = a.d, ld = d + 1;
    const int tl = threadIdx.x >> 2, c = threadIdx.x & 3;
    const int t = (int)blockIdx.x * kHugeRows + tl;
    const double* __restrict__ Z = a.scratch + (size_t)blockIdx.y * (size_t)huge_basis_scratch(d);
    double* __restrict__ h = smem + tl * ld;
    for (int j = c; j < d; j += 4) h[j] = (j == t) ? 1.0 : 0.0;
    const int lane = __lane_id();
    for (int n = 0; n < d - 1; ++n) {
        const double* __restrict__ xr = Z + (huge_refl_offset(n, d) - n);   // xr[j], j >= n
        const int j0 = n + ((c - n) & 3);
        double tmp = 0.0;
        for (int j = j0; j < d; j += 4) tmp = fma(h[j], xr[j], tmp);
        const double t0 = __shfl(tmp, (lane & ~3) | 0), t1 = __shfl(tmp, (lane & ~3) | 1),
                     t2 = __shfl(tmp, (lane & ~3) | 2), t3 = __shfl(tmp, (lane & ~3) | 3);
        const double tot = (t0 + t1) + (t2 + t3);
        for (int j = j0; j < d; j += 4) h[j] = fma(-tot, xr[j], h[j]);
    }
    if (t < d) {
        const double Dt = Z[huge_sign_offset(d) + t];
        double* __restrict__ R = a.scratch + (size_t)blockIdx.y * (size_t)huge_basis_scratch(d) + huge_r_offset(d);
        for (int j = c; j < d; j += 4) R[(size_t)t * d + j] = Dt * h[j];
    }
}

__global__ void __launch_bounds__(256) huge_product_kernel(const HugeBasisArgs a)
{
    const int d = a.d;
    const int idx = (int)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= d * d) return;
    const int i = idx / d, c = idx - i * d;
    const double* __restrict__ R = a.scratch + (size_t)blockIdx.y * (size_t)huge_basis_scratch(d) + huge_r_offset(d);
    const double* __restrict__ Ti = a.T + (size_t)i * d;
    double s = 0.0;
    for (int k = 0; k <= i; ++k) s = fma(Ti[k], R[(size_t)k * d + c], s);
    a.V[((size_t)(a.slab0 + blockIdx.y) * d + c) * d + i] = s;
}

// ---------------------------------------------------------------- directions of a launch
__global__ void __launch_bounds__(256) huge_dirs_kernel(const HugeDirArgs a)
{
    const int d = a.d, K = a.K, j = threadIdx.x;
    const int s = blockIdx.x, g = blockIdx.y;
    const unsigned long long step = a.step0 + (unsigned long long)s;
    const int cyc = (int)(step / (unsigned long long)d - a.cycle0), col = (int)(step % (unsigned long long)d);
    const double* __restrict__ v = a.V + (((size_t)g * a.ncyc + cyc) * d + col) * d;
    const int stride = huge_col_stride(d, K);
    double* __restrict__ o = a.out + ((size_t)g * a.n_steps + s) * stride;
    const double* __restrict__ inv = a.prior + 3 * a.dpad;
    if (j < d) {
        const double vj = v[j];
        o[j] = vj;
        for (int k = 0; k < K; ++k) {
            const double* __restrict__ Lj = a.Lrow + ((size_t)k * d + j) * d;
            double u = 0.0;
            for (int i = 0; i <= j; ++i) u = fma(Lj[i], v[i], u);
            o[(size_t)(1 + k) * d + j] = u;
        }
        o[(size_t)(1 + K) * d + j] = (vj * inv[j]) * inv[j];
    }
    __syncthreads();
    if (j == 0) {
        double q[4] = {0.0, 0.0, 0.0, 0.0}, nn[4] = {0.0, 0.0, 0.0, 0.0}, lw[4] = {0.0, 0.0, 0.0, 0.0};
        const double* __restrict__ loc = a.prior + 2 * a.dpad;
        for (int i = 0; i < d; ++i) {
            const double u = o[d + i], w = o[(size_t)(1 + K) * d + i];
            q[i & 3] = fma(u, u, q[i & 3]);
            nn[i & 3] = fma(o[i], w, nn[i & 3]);
            if (inv[i] != 0.0) lw[i & 3] = fma(loc[i], w, lw[i & 3]);
        }
        double* tail = o + (size_t)(2 + K) * d;
        tail[0] = (q[0] + q[1]) + (q[2] + q[3]);
        tail[1] = (nn[0] + nn[1]) + (nn[2] + nn[3]);
        tail[2] = (lw[0] + lw[1]) + (lw[2] + lw[3]);
        tail[3] = 0.0;
    }
}

// ---------------------------------------------------------------- the step
// the normal terms of the log-prior at x (incremental mode: the reciprocal of the scale)
__device__ __forceinline__ double huge_inc_logprior(const double* __restrict__ x, int W, int d,
                                                    const double* __restrict__ pr, int dpad, double uniform_logp)
{
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < d; ++i) {
        const double inv = pr[3 * dpad + i];
        if (inv != 0.0) {
            const double q = (x[(size_t)i * W] - pr[2 * dpad + i]) * inv;
            sc[i & 3] = sc[i & 3] + fma(-0.5 * q, q, pr[4 * dpad + i]);
        }
    }
    return uniform_logp + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
}

__global__ void __launch_bounds__(64) huge_step_kernel(const HugeStepArgs a)
{
    __shared__ dpair_t s_log[SHORT_LOG_TABLE_SIZE];
    __shared__ double s_exp[64];
    const short_log_tab ltab = short_log_load(s_log);
    const exp_tab etab = exp_tab_load(s_exp);
    __syncthreads();
    const int d = a.d, K = a.K, W = a.W, dpad = a.dpad;
    const int w = (int)blockIdx.x * 64 + threadIdx.x;   // (W is a multiple of 64)
    const uint32_t gid = a.walker0 + (uint32_t)w;
    const int g = w / a.bgs;
    const int stride = huge_col_stride(d, K);
    double* __restrict__ xw = a.x + w;
    double* __restrict__ yw = a.y + w;
    const double* __restrict__ lo = a.prior;
    const double* __restrict__ hi = a.prior + dpad;
    const double* __restrict__ loc = a.prior + 2 * dpad;
    const double* __restrict__ inv = a.prior + 3 * dpad;
    const double* __restrict__ mls = a.prior + 4 * dpad;
    double logpost = a.logpost[w], logprior = a.logprior[w], loglike = a.loglike[w];
    int weight = a.weight[w], prej = a.prior_rej[w], burn = a.burn_left[w];
    long long nacc = a.n_accept[w];
    long long accepted = 0;
    PairRng rng;
    for (int s = 0; s < a.n_steps; ++s) {
        const unsigned long long step = a.step0 + (unsigned long long)s;
        if ((s == 0 && a.anchor) || step % a.refresh == 0) {
            // y = L^-1 (x - mu) from scratch; one mode: the carried log-densities re-anchored
            double q[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < K; ++k) {
                const double* __restrict__ mu = a.mean + (size_t)k * d;
                for (int j = 0; j < d; ++j) {
                    const double* __restrict__ Lj = a.Lrow + ((size_t)k * d + j) * d;
                    double acc = 0.0;
                    for (int i = 0; i <= j; ++i) acc = fma(Lj[i], xw[(size_t)i * W] - mu[i], acc);
                    yw[((size_t)k * d + j) * W] = acc;
                    if (k == 0) q[j & 3] = fma(acc, acc, q[j & 3]);
                }
            }
            if (K == 1) {
                loglike = -0.5 * (a.cnorm[0] + ((q[0] + q[1]) + (q[2] + q[3])));
                if (a.carry_prior) logprior = huge_inc_logprior(xw, W, d, a.prior, dpad, a.uniform_logp);
                logpost = logprior + loglike;
            }
        }
        double r, Ea;
        if (K == 0) {   // the `one` likelihood: the from-scratch step (orc_run, full evaluation)
            step_variates(a.key0, a.key1, gid, step, 0u, false, r, Ea);
        } else {
            if (s == 0 || (step & 1ull) == 0ull) rng.run(a.key0, a.key1, gid, step >> 1, ltab);
            r = rng.r[step & 1ull];
            Ea = rng.Ea[step & 1ull];
        }
        const double* __restrict__ col = a.cols + ((size_t)g * a.n_steps + s) * stride;
        const double* __restrict__ wd = col + (size_t)(1 + K) * d;
        const double* __restrict__ tail = col + (size_t)(2 + K) * d;
        bool inb = true;
        double sc[4] = {0.0, 0.0, 0.0, 0.0};
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        double pc[kHugeMaxModes][4] = {};
        for (int i = 0; i < d; ++i) {
            const int c = i & 3;
            const double xi = xw[(size_t)i * W];
            const double t = fma(r, col[i], xi);
            inb = inb & (t <= hi[i]) & (t >= lo[i]);
            if (a.carry_prior) {
                sc[c] = fma(xi, wd[i], sc[c]);
            } else if (K == 0 && inv[i] != 0.0) {   // (eval_point: the division by the scale)
                const double qq = (t - loc[i]) / a.scale[i];
                sc[c] = sc[c] + fma(-0.5 * qq, qq, mls[i]);
            } else if (inv[i] != 0.0) {
                const double qq = (t - loc[i]) * inv[i];
                sc[c] = sc[c] + fma(-0.5 * qq, qq, mls[i]);
            }
            if (K == 1) {
                q[c] = fma(yw[(size_t)i * W], col[d + i], q[c]);
            } else if (K > 1) {
#pragma unroll
                for (int k = 0; k < kHugeMaxModes; ++k)
                    if (k < K) {
                        const double yt = fma(r, col[(size_t)(1 + k) * d + i], yw[((size_t)k * d + i) * W]);
                        pc[k][c] = fma(yt, yt, pc[k][c]);
                    }
            }
        }
        double lp = -INFINITY, ll = -INFINITY, lt = -INFINITY;
        if (inb) {
            const double ssum = (sc[0] + sc[1]) + (sc[2] + sc[3]);
            if (a.carry_prior) {
                const double xwv = ssum - tail[2];
                lp = fma(-0.5 * r, fma(r, tail[1], xwv + xwv), logprior);
            } else {
                lp = a.uniform_logp + ssum;
            }
            if (K == 0) {
                ll = 0.0;
            } else if (K == 1) {
                const double yu = (q[0] + q[1]) + (q[2] + q[3]);
                ll = fma(-0.5 * r, fma(r, tail[0], yu + yu), loglike);
            } else {
                double am[kHugeMaxModes], amax = -INFINITY;
#pragma unroll
                for (int k = 0; k < kHugeMaxModes; ++k)
                    if (k < K) {
                        am[k] = -0.5 * (a.cnorm[k] + ((pc[k][0] + pc[k][1]) + (pc[k][2] + pc[k][3])));
                        if (am[k] > amax) amax = am[k];
                    }
                double S = 0.0;
#pragma unroll
                for (int k = 0; k < kHugeMaxModes; ++k)
                    if (k < K) S = fma(a.mweight[k], dexp_tab(am[k] - amax, etab), S);
                ll = dlog_tab(S, ltab) + amax;
            }
            lt = lp + ll;
        }
        bool accept;
        if (!inb || lt == -INFINITY) accept = false;
        else if (lt > logpost) accept = true;
        else accept = Ea > (logpost - lt) / a.temperature;
        if (accept) {
            if (burn > 0) burn -= 1;
            for (int i = 0; i < d; ++i) {
                const double xi = xw[(size_t)i * W];
                xw[(size_t)i * W] = fma(r, col[i], xi);
                for (int k = 0; k < K; ++k) {
                    double* yk = yw + ((size_t)k * d + i) * W;
                    *yk = fma(r, col[(size_t)(1 + k) * d + i], *yk);
                }
            }
            logprior = lp; loglike = ll; logpost = lt;
            weight = 1; prej = 0; nacc += 1; accepted += 1;
        } else {
            weight += 1;
            if (!inb) prej += 1;
            const double max_now = a.max_tries * (burn > 0 ? 10.0 : 1.0);
            if ((double)(weight - prej) > max_now) atomicCAS(a.stuck, 0, 1 + (int)gid);
        }
    }
    a.logpost[w] = logpost; a.logprior[w] = logprior; a.loglike[w] = loglike;
    a.weight[w] = weight; a.prior_rej[w] = prej; a.burn_left[w] = burn;
    a.n_accept[w] = nacc;
    wave_add_accepts(a.accept_total, accepted);
}

// ---------------------------------------------------------------- evaluation from scratch
__global__ void __launch_bounds__(64) huge_evaluate_kernel(const HugeEvalArgs a)
{
    const int p = (int)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.n) return;
    const int d = a.d, K = a.K, dpad = a.dpad;
    const double* __restrict__ t = a.x + (size_t)p * d;
    const double* __restrict__ lo = a.prior;
    const double* __restrict__ hi = a.prior + dpad;
    const double* __restrict__ loc = a.prior + 2 * dpad;
    const double* __restrict__ inv = a.prior + 3 * dpad;
    const double* __restrict__ mls = a.prior + 4 * dpad;
    bool inb = true;
    for (int i = 0; i < d; ++i) inb = inb & (t[i] <= hi[i]) & (t[i] >= lo[i]);
    if (!inb) {
        a.logprior[p] = -INFINITY;
        a.loglike[p] = -INFINITY;
        return;
    }
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < d; ++i)
        if (inv[i] != 0.0) {
            const double q = (t[i] - loc[i]) / a.scale[i];
            sc[i & 3] = sc[i & 3] + fma(-0.5 * q, q, mls[i]);
        }
    a.logprior[p] = a.uniform_logp + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
    if (K == 0) {
        a.loglike[p] = 0.0;
        return;
    }
    double am[kHugeMaxModes], amax = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const double* __restrict__ mu = a.mean + (size_t)k * d;
        double pc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < d; ++j) {
            const double* __restrict__ Lj = a.Lrow + ((size_t)k * d + j) * d;
            double y = 0.0;
            for (int i = 0; i <= j; ++i) y = fma(Lj[i], t[i] - mu[i], y);
            if (a.derived) a.derived[(size_t)p * K * d + (size_t)k * d + j] = y;
            pc[j & 3] = fma(y, y, pc[j & 3]);
        }
        am[k] = -0.5 * (a.cnorm[k] + ((pc[0] + pc[1]) + (pc[2] + pc[3])));
        if (am[k] > amax) amax = am[k];
    }
    if (K == 1) {
        a.loglike[p] = am[0];
        return;
    }
    double S = 0.0;
    for (int k = 0; k < K; ++k) S = fma(a.mweight[k], dexp(am[k] - amax), S);
    a.loglike[p] = dlog(S) + amax;
}

// ---------------------------------------------------------------- moments
constexpr int kHugeMomentSlice = 32;   // walkers of a group staged in LDS at a time

__global__ void __launch_bounds__(256) huge_group_moments_kernel(const MomentArgs a, int gs, int d)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];   // [slice][d]
    const int g = blockIdx.y, tid = threadIdx.x;
    const int npair = d * (d + 1) / 2;
    const int p = (int)blockIdx.x * 256 + tid;
    int i = 0, j = 0;
    if (p < npair) {   // p = i (i + 1) / 2 + j, j <= i
        i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        while (i * (i + 1) / 2 > p) --i;
        j = p - i * (i + 1) / 2;
    }
    const bool sums = blockIdx.x == 0 && tid < d;
    double s = 0.0, gsum = 0.0;
    for (int l0 = 0; l0 < gs; l0 += kHugeMomentSlice) {
        __syncthreads();
        for (int e = tid; e < kHugeMomentSlice * d; e += 256) {
            const int l = e / d, ii = e - l * d;
            smem[e] = a.x[(size_t)ii * a.W + (size_t)g * gs + l0 + l] - a.shift[ii];
        }
        __syncthreads();
        if (p < npair)
            for (int l = 0; l < kHugeMomentSlice; ++l) s = fma(smem[l * d + i], smem[l * d + j], s);
        if (sums)
            for (int l = 0; l < kHugeMomentSlice; ++l) gsum = gsum + smem[l * d + tid];
    }
    if (p < npair) a.Sg[(size_t)g * npair + p] = s;
    if (sums) a.group_sum[(size_t)g * d + tid] += gsum;
}

__global__ void __launch_bounds__(256) huge_pool_moments_kernel(const MomentArgs a, int npair)
{
    const int p = (int)blockIdx.x * 256 + threadIdx.x;
    if (p >= npair) return;
    double acc = a.pooled[p];
    for (int g = 0; g < a.G; ++g) acc += a.Sg[(size_t)g * npair + p];
    a.pooled[p] = acc;
}

}  // namespace
}  // namespace mcmc

using namespace mcmc;

// V of cycles [cycle0, cycle0 + ncyc) of n_groups basis groups, in batches of (group, cycle)
// slabs as the scratch holds them (scratch_slabs of huge_basis_scratch(d) doubles)
extern "C" hipError_t mcmc_hip_launch_huge_basis(const HugeBasisArgs* in, int n_groups, int scratch_slabs,
                                                 hipStream_t st)
{
    HugeBasisArgs a = *in;
    const int d = a.d, total = n_groups * a.ncyc;
    if (d <= kMaxDimLane || d > kMaxDimHuge || scratch_slabs <= 0) return hipErrorInvalidValue;
    const size_t rows_lds = sizeof(double) * (size_t)kHugeRows * (d + 1);
    if (rows_lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)huge_rows_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_lds);
        if (e != hipSuccess) return e;
    }
    for (int s0 = 0; s0 < total; s0 += scratch_slabs) {
        a.slab0 = s0;
        a.n_slabs = std::min(scratch_slabs, total - s0);
        hipLaunchKernelGGL(huge_reflect_kernel, dim3(a.n_slabs), dim3(256), 0, st, a);
        hipLaunchKernelGGL(huge_rows_kernel, dim3((d + kHugeRows - 1) / kHugeRows, a.n_slabs), dim3(256),
                           rows_lds, st, a);
        hipLaunchKernelGGL(huge_product_kernel, dim3((d * d + 255) / 256, a.n_slabs), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_huge_dirs(const HugeDirArgs* a, int n_groups, hipStream_t st)
{
    if (a->d > kMaxDimHuge || a->K < 0 || a->K > kHugeMaxModes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(huge_dirs_kernel, dim3(a->n_steps, n_groups), dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_huge_step(const HugeStepArgs* a, hipStream_t st)
{
    if (a->d > kMaxDimHuge || a->K < 0 || a->K > kHugeMaxModes || a->W % 64 || a->bgs % 64)
        return hipErrorInvalidValue;
    mcmc_hip_note_step_kernel("mcmc::huge_step_kernel");
    hipLaunchKernelGGL(huge_step_kernel, dim3(a->W / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_huge_evaluate(const HugeEvalArgs* a, hipStream_t st)
{
    if (a->d > kMaxDimHuge || a->K < 0 || a->K > kHugeMaxModes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(huge_evaluate_kernel, dim3((a->n + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_huge_moments(const MomentArgs* a, int group_size, int d, hipStream_t st)
{
    if (d > kMaxDimHuge || group_size % kHugeMomentSlice) return hipErrorInvalidValue;
    const int npair = d * (d + 1) / 2;
    const size_t lds = sizeof(double) * kHugeMomentSlice * d;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)huge_group_moments_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(huge_group_moments_kernel, dim3((npair + 255) / 256, a->G), dim3(256), lds, st, *a,
                       group_size, d);
    hipLaunchKernelGGL(huge_pool_moments_kernel, dim3((npair + 255) / 256), dim3(256), 0, st, *a, npair);
    return hipGetLastError();
}
