// Lagged cross-products of the ensemble with its previous snapshots (gfx950): what a moment snapshot
// keeps of the state x[d][W] for the integrated autocorrelation time.  The rule (DESIGN.md section 2,
// "Autocorrelation"): with a = x_t - shift and b = x_{t-k} - shift, per group g of group_size walkers
// and configured dimension i
//     S_t[g, i]  = sum_l a          P[g, k, i] = sum_l a * b        (k = 0 .. held - 1)
// each ONE chain over the group's walkers in ascending order from +0.0; the product and the addition
// are separate roundings (-ffp-contract=off).  The pooled accumulators then add the groups in
// ascending order, starting from their current value, the way pool_moments_kernel does.
//
//   autocorr_group_kernel  one workgroup per (group, dimension): the group's tile of the current
//                          snapshot is read once, written to its ring slot and staged (shifted) in
//                          LDS; the lagged slices are streamed coalesced along w, multiplied by the
//                          tile lane by lane (the products are independent roundings) and laid down
//                          in LDS as one row per lag; one thread per lag then adds its row in
//                          ascending order, a further thread the tile itself (S_t).
//   autocorr_pool_kernel   one thread per (P | A | B, lag, dimension): adds the G group values to the
//                          accumulator in ascending order.  A launch boundary separates the two.
//
// The kernels are d-agnostic: they read x[d][W] like marginals_kernel, whatever step kernel wrote it.
#include "autocorr_args.h"
#include <algorithm>

namespace mcmc {
namespace {

// ONE ascending chain over n (a multiple of 8) doubles in LDS, read eight at a time so that the
// reads of a batch travel together; the additions stay in order
__device__ __forceinline__ double ac_chain(const double* __restrict__ row, int n)
{
    double s = 0.0;
    for (int l = 0; l < n; l += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = row[l + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) s = s + v[q];
    }
    return s;
}

__global__ void __launch_bounds__(kAcThreads) autocorr_group_kernel(const AcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_ac[];   // tile [gs] | rows [rp][gs + 1]
    const int tid = threadIdx.x, gs = a.gs, g = blockIdx.x, i = blockIdx.y;
    if (g >= a.G || i >= a.n) return;
    const int slots = a.lags + 1, ldr = gs + 1;
    double* sa = s_ac;
    double* sp = s_ac + gs;
    const int di = a.dims[i];
    const double sh = a.shift[di];
    const size_t col = (size_t)g * gs;
    if (tid < gs) {
        const double xa = a.x[(size_t)di * a.W + col + tid];
        a.ring[((size_t)a.head * a.n + i) * a.W + col + tid] = xa;
        sa[tid] = xa - sh;
    }
    __syncthreads();
    // 256 / gs rows are filled side by side (group_size is 64, 128 or 256)
    const int rpb = kAcThreads / gs;
    const int r_off = tid / gs, l = tid - r_off * gs;
    const double av = sa[l];
    for (int c0 = 0; c0 < a.held; c0 += a.rows_per_pass) {
        const int c1 = min(c0 + a.rows_per_pass, a.held);
        for (int r = c0 + r_off; r < c1; r += 4 * rpb) {
            double b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // the loads of four lags are in flight together
                const int rq = r + q * rpb;
                b[q] = av;                  // lag 0: b = a
                if (rq < c1 && rq > 0) {
                    int slot = a.head - rq;
                    if (slot < 0) slot += slots;
                    b[q] = a.ring[((size_t)slot * a.n + i) * a.W + col + l] - sh;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rq = r + q * rpb;
                if (rq < c1) sp[(rq - c0) * ldr + l] = av * b[q];
            }
        }
        __syncthreads();
        const int nr = c1 - c0;
        if (tid < nr) {
            a.Pg[((size_t)g * slots + c0 + tid) * a.n + i] = ac_chain(sp + tid * ldr, gs);
        } else if (c0 == 0 && tid == kAcThreads - 1) {   // (another wave than the chains of P)
            a.ringS[((size_t)a.head * a.G + g) * a.n + i] = ac_chain(sa, gs);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) autocorr_pool_kernel(const AcArgs a)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int per = a.held * a.n;
    if (q >= 3 * per) return;
    const int slots = a.lags + 1;
    const int kind = q / per, rem = q - kind * per;
    const int k = rem / a.n, i = rem - k * a.n;
    const double* __restrict__ src;
    size_t stride;
    if (kind == 0) {            // accP[k, i] += P[g, k, i]
        src = a.Pg + (size_t)k * a.n + i;
        stride = (size_t)slots * a.n;
    } else {                    // accA[k, i] += S_t[g, i]; accB[k, i] += S_{t-k}[g, i]
        int slot = a.head - (kind == 1 ? 0 : k);
        if (slot < 0) slot += slots;
        src = a.ringS + (size_t)slot * a.G * a.n + i;
        stride = (size_t)a.n;
    }
    double* dst = a.acc + ((size_t)kind * slots + k) * a.n + i;
    double acc = *dst;
    int g = 0;
    for (; g + 16 <= a.G; g += 16) {   // loads batched, additions strictly in ascending group order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = src[(size_t)(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; g < a.G; ++g) acc += src[(size_t)g * stride];
    *dst = acc;
}

}  // namespace
}  // namespace mcmc

extern "C" int mcmc_hip_autocorr_rows_per_pass(int group_size, int lags)
{
    const size_t row = sizeof(double) * ((size_t)group_size + 1);
    const size_t tile = sizeof(double) * (size_t)group_size;
    if (group_size < 8 || group_size % 8 || group_size > mcmc::kAcThreads || tile + row > mcmc::kAcLdsMax)
        return 0;
    const size_t fit = (mcmc::kAcLdsMax - tile) / row;
    // (the last thread of the workgroup carries S_t: the rows' threads stay below it)
    return (int)std::min<size_t>({fit, (size_t)lags + 1, (size_t)mcmc::kAcThreads - 2});
}

extern "C" hipError_t mcmc_hip_launch_autocorr(const mcmc::AcArgs* a, hipStream_t st)
{
    if (a->n <= 0 || a->G <= 0) return hipSuccess;
    if (a->held < 1 || a->held > a->lags + 1 || a->head < 0 || a->head > a->lags ||
        a->rows_per_pass < 1 || a->rows_per_pass != mcmc_hip_autocorr_rows_per_pass(a->gs, a->lags))
        return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * ((size_t)a->gs + (size_t)a->rows_per_pass * (a->gs + 1));
    hipLaunchKernelGGL(mcmc::autocorr_group_kernel, dim3((unsigned)a->G, (unsigned)a->n),
                       dim3(mcmc::kAcThreads), lds, st, *a);
    const int n_chain = 3 * a->held * a->n;
    hipLaunchKernelGGL(mcmc::autocorr_pool_kernel, dim3((unsigned)((n_chain + 63) / 64)), dim3(64), 0, st, *a);
    return hipGetLastError();
}
