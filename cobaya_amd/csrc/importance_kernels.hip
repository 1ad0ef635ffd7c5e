// Importance reweighting of the ensemble (gfx950): what a moment snapshot adds to the weighted moments
// of the sampled parameters under w = exp(delta), delta[k][W] being the log-weights of alternative k
// the caller has filled from the state x[d][W].  The rule ("Importance"): with c the
// centring constant of the interval and s the moment shift, per walker
//     NaN or +inf: left out (nonfinite);   -inf: used, e = 0 (zero);
//     otherwise e = dexp(min(delta - c, 700)), clamped counts delta - c > 700;
//     b_i = x_i - s_i,   u_i = e * b_i   (one rounding each)
// and per group g of group_size walkers, over the used walkers in ascending order, ONE chain each from
// +0.0 with the product and the addition as separate roundings (-ffp-contract=off; no fma):
//     n   S1 = sum e   S2 = sum e * e   M_i = sum u_i   V_i = sum u_i * b_i   Q_ij = sum u_i * b_j (j < i)
// The chain of an accumulation is then added to the slab's value: sums = sums + chain.  A walker that is
// left out adds +0.0 in every chain, which no chain that began at +0.0 can tell from skipping it.
//
//   importance_group_kernel  one workgroup per (group, alternative, block of 32 columns j).  The block
//                            carries the rows i >= 32 cb with the covariance, its own 32 rows without.
//                            The group is walked in chunks of 64 walkers: every wave forms e of the
//                            chunk's walkers itself (a lane per walker: dexp is cheaper than a barrier),
//                            u goes to the row tile [rows][65], b of the block's columns to [32][65].
//                            A lane owns a column, a thread the rows tid / 32 + 8 q: independent chains
//                            in registers that share one read of the column; u_i is a broadcast.  The
//                            last wave carries one more chain per lane beside them: M of the block's
//                            rows, S1 and S2.  Where two sets of tiles fit they alternate and a chunk
//                            costs ONE barrier; else a second one guards the tiles.
//   importance_max_kernel    2 048 walkers per workgroup and alternative: the maximum of the
//                            order-preserving 64-bit keys of the finite delta, one 64-bit atomic max per
//                            workgroup into the zeroed key of c.
//
// Nothing depends on the launch geometry.  Vector stores only; the stream orders the launches.
#include "importance_args.h"
#include "det_math.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace mcmc {
namespace {

__device__ __forceinline__ bool im_finite(double v)
{
    return (((unsigned long long)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull;
}

// the chains of a thread over n8 (a multiple of 8, <= kImChunk) staged walkers: NQ rows against one
// column, reads batched B walkers at a time, the additions in ascending order
template <int NQ, bool EXTRA>
__device__ __forceinline__ void im_chains(const double* __restrict__ rows, const double* __restrict__ col,
                                          const double* __restrict__ ex, bool ex_sq, int n8,
                                          double (&acc)[kImMaxPasses], double& acc_ex)
{
    constexpr int B = NQ <= 4 ? 8 : (NQ <= 8 ? 4 : 2);
    for (int l0 = 0; l0 < n8; l0 += B) {
        double cv[B], av[NQ][B], xv[B];
#pragma unroll
        for (int u = 0; u < B; ++u) cv[u] = col[l0 + u];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int u = 0; u < B; ++u) av[q][u] = rows[q * kImRowsPerPass * kImLd + l0 + u];
        if (EXTRA) {
#pragma unroll
            for (int u = 0; u < B; ++u) xv[u] = ex[l0 + u];
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const double p = av[q][u] * cv[u];
                acc[q] = acc[q] + p;
            }
            if (EXTRA) {
                const double p = ex_sq ? xv[u] * xv[u] : xv[u];
                acc_ex = acc_ex + p;
            }
        }
    }
}

template <int NQ>
__device__ __forceinline__ void im_chains_of(bool extra, const double* rows, const double* col, const double* ex,
                                             bool ex_sq, int n8, double (&acc)[kImMaxPasses], double& acc_ex)
{
    if (extra) im_chains<NQ, true>(rows, col, ex, ex_sq, n8, acc, acc_ex);
    else im_chains<NQ, false>(rows, col, ex, ex_sq, n8, acc, acc_ex);
}

// passes of eight rows a block of n_rows rows is served with (an instantiation exists for each)
__host__ __device__ inline int im_passes(int n_rows)
{
    const int nq = (n_rows + kImRowsPerPass - 1) / kImRowsPerPass;
    return nq <= 4 ? nq : (nq <= 6 ? 6 : (nq <= 8 ? 8 : (nq <= 12 ? 12 : 16)));
}
// doubles of one set of tiles: u[8 nq][65] | b[32][65] | e[64]
__host__ __device__ inline size_t im_tile_doubles(int nq)
{
    return (size_t)(kImRowsPerPass * nq + kImCols) * kImLd + kImChunk;
}

__global__ void __launch_bounds__(kImThreads) importance_group_kernel(const ImArgs a, const int dbl)
{
    extern __shared__ __attribute__((aligned(16))) double s_im[];
    const int tid = threadIdx.x, g = blockIdx.x, k = blockIdx.y, cb = blockIdx.z;
    const int d = a.d, cov = a.cov[k];
    const int R0 = cb * kImCols;
    const int n_rows = cov ? d - R0 : min(kImCols, d - R0);
    const int nq = im_passes(n_rows), t_rows = kImRowsPerPass * nq;
    const size_t set = im_tile_doubles(nq);
    const int l = tid & (kImChunk - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = tid & (kImCols - 1), jr = tid >> 5;
    const bool extra = wave == kImThreads / 64 - 1;
    const bool stats = cb == 0 && wave == 0;
    const double cc = im_value(a.ckey[k]);
    const double* __restrict__ dk = a.delta + (size_t)k * a.W;
    double acc[kImMaxPasses];
#pragma unroll
    for (int q = 0; q < kImMaxPasses; ++q) acc[q] = 0.0;
    double acc_ex = 0.0;
    unsigned long long n_used = 0ull, n_zero = 0ull, n_bad = 0ull, n_clamp = 0ull;
    int p = 0;
    for (int t0 = 0; t0 < a.gs; t0 += kImChunk) {
        const int n_l = min(kImChunk, a.gs - t0);
        const bool on = l < n_l;
        const size_t w = (size_t)g * a.gs + t0 + (on ? l : 0);
        double* su = s_im + (size_t)p * set;
        double* sc = su + (size_t)t_rows * kImLd;
        double* se = sc + kImCols * kImLd;
        // e of the walker: every wave forms it for itself
        const double dl = dk[w];
        const bool fin = im_finite(dl);
        const bool zero = on && !fin && dl < 0.0;                 // -inf
        const bool used = on && (fin || zero);
        const double arg = dl - cc;
        const bool cl = on && fin && arg > kImClamp;
        const double er = dexp(cl ? kImClamp : arg);
        const double e = (on && fin) ? er : 0.0;
        if (stats) {
            n_used += (unsigned long long)__popcll(lanes(used));
            n_zero += (unsigned long long)__popcll(lanes(zero));
            n_bad += (unsigned long long)__popcll(lanes(on && !used));
            n_clamp += (unsigned long long)__popcll(lanes(cl));
        }
        if (wave == 0) se[l] = e;
        for (int r = wave; r < t_rows; r += kImThreads / 64) {
            const int i = R0 + r;
            double b = 0.0;
            if (used && r < n_rows) b = a.x[(size_t)i * a.W + w] - a.shift[i];
            su[r * kImLd + l] = e * b;
            if (r < kImCols) sc[r * kImLd + l] = b;
        }
        __syncthreads();
        const int n8 = (n_l + 7) & ~7;                            // (the tiles are zero past n_l)
        const double* rows = su + jr * kImLd;
        const double* col = sc + c * kImLd;
        const double* ex = l < kImCols ? su + l * kImLd : se;    // (the last wave: M of a row, S1, S2)
        const bool ex_sq = l == kImCols + 1;
        switch (nq) {
        case 1: im_chains_of<1>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 2: im_chains_of<2>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 3: im_chains_of<3>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 4: im_chains_of<4>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 6: im_chains_of<6>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 8: im_chains_of<8>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        case 12: im_chains_of<12>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        default: im_chains_of<16>(extra, rows, col, ex, ex_sq, n8, acc, acc_ex); break;
        }
        if (dbl) p ^= 1;                                          // (the next chunk fills the other set)
        else __syncthreads();                                     // (the next chunk overwrites the tiles)
    }
    double* __restrict__ S = a.sums + a.off[k] + (size_t)g * im_n_chains(d, cov);
    const int j = R0 + c;
#pragma unroll
    for (int q = 0; q < kImMaxPasses; ++q) {
        const int i = R0 + jr + kImRowsPerPass * q;
        if (q < nq && i < d && j <= i && (i == j || cov)) {
            const size_t at = i == j ? 2 + (size_t)d + i : 2 + 2 * (size_t)d + (size_t)i * (i - 1) / 2 + j;
            S[at] = S[at] + acc[q];
        }
    }
    if (extra) {
        if (l < kImCols) {
            if (R0 + l < d) S[2 + R0 + l] = S[2 + R0 + l] + acc_ex;
        } else if (cb == 0 && l <= kImCols + 1) {
            S[l - kImCols] = S[l - kImCols] + acc_ex;
        }
    }
    if (stats && l == 0) {
        a.n[(size_t)k * a.G + g] += n_used;
        if (n_zero != 0ull) atomicAdd(&a.counters[3 * k], n_zero);
        if (n_bad != 0ull) atomicAdd(&a.counters[3 * k + 1], n_bad);
        if (n_clamp != 0ull) atomicAdd(&a.counters[3 * k + 2], n_clamp);
    }
}

__global__ void __launch_bounds__(kImThreads) importance_max_kernel(const ImArgs a)
{
    __shared__ unsigned long long sk[kImThreads / 64];
    const int k = blockIdx.y;
    const double* __restrict__ dk = a.delta + (size_t)k * a.W;
    unsigned long long key = 0ull;
    const int w0 = (int)blockIdx.x * (kImThreads * kImMaxPerThread) + (int)threadIdx.x;
    double v[kImMaxPerThread];
#pragma unroll
    for (int q = 0; q < kImMaxPerThread; ++q) {          // the loads travel together
        const int w = w0 + q * kImThreads;
        v[q] = w < a.W ? dk[w] : __longlong_as_double(-1ll);   // (a NaN: skipped)
    }
#pragma unroll
    for (int q = 0; q < kImMaxPerThread; ++q)
        if (im_finite(v[q])) {
            const unsigned long long kq = im_key(v[q]);
            key = kq > key ? kq : key;
        }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        const unsigned long long o = __shfl_xor(key, mk, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < kImThreads / 64; ++q) key = sk[q] > key ? sk[q] : key;
        if (key != 0ull) atomicMax(&a.ckey[k], key);      // (no finite delta: the key stays 0, c = 0)
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_importance(const mcmc::ImArgs* a, hipStream_t st)
{
    if (a->W <= 0 || a->G <= 0 || a->n_alt <= 0) return hipSuccess;
    if (a->d < 1 || a->d > mcmc::kImMaxDim || a->n_alt > mcmc::kImMaxAlt || a->gs < 1 ||
        (long long)a->G * a->gs != a->W)
        return hipErrorInvalidValue;
    bool any_cov = false;
    for (int k = 0; k < a->n_alt; ++k) {
        if (a->cov[k] && a->d > mcmc::kImMaxCovDim) return hipErrorInvalidValue;
        any_cov = any_cov || a->cov[k];
    }
    // the largest set of tiles is that of the first block of columns
    const int nq = mcmc::im_passes(any_cov ? a->d : std::min(mcmc::kImCols, a->d));
    const size_t one = sizeof(double) * mcmc::im_tile_doubles(nq);
    const int dbl = 2 * one <= 80 * 1024 ? 1 : 0;
    const size_t lds = dbl ? 2 * one : one;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)mcmc::importance_group_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned blocks = (unsigned)((a->d + mcmc::kImCols - 1) / mcmc::kImCols);
    hipLaunchKernelGGL(mcmc::importance_group_kernel, dim3((unsigned)a->G, (unsigned)a->n_alt, blocks),
                       dim3(mcmc::kImThreads), lds, st, *a, dbl);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_importance_max(const mcmc::ImArgs* a, hipStream_t st)
{
    if (a->W <= 0 || a->n_alt <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a->ckey, 0, sizeof(unsigned long long) * a->n_alt, st);
    if (e != hipSuccess) return e;
    const int per = mcmc::kImThreads * mcmc::kImMaxPerThread;
    hipLaunchKernelGGL(mcmc::importance_max_kernel, dim3((unsigned)((a->W + per - 1) / per), (unsigned)a->n_alt),
                       dim3(mcmc::kImThreads), 0, st, *a);
    return hipGetLastError();
}
