// Evidence of the run (gfx950): what a moment snapshot adds to the ellipsoid-truncated harmonic
// mean.  The rule ("Evidence"): with the active ellipsoid (m, Linv, c), per
// walker
//     delta_i = x_i - m_i,   z_j = sum_{i <= j} Linv[j][i] * delta_i,   s = sum_j z_j * z_j,
// every sum ONE ascending chain from +0.0 with the product and the addition as separate roundings
// (-ffp-contract=off), and e = dexp(min(c - logpost, 700)).  Per group g of group_size walkers and
// radius r the walkers with s <= R2_r add their e in ascending order from +0.0 (S_t), then
// acc[g][r] = acc[g][r] + S_t, cnt[g][r] += the walkers inside; one counter takes the clamped
// arguments.  Nothing depends on the launch geometry or on how the walkers are sharded.
//
//   evidence_kernel        one workgroup per 64 walkers, one LANE per walker, four waves.  delta
//                          goes to LDS as [d][64] (a lane reads its own column: no bank conflict).
//                          Rows of Linv are taken four at a time (four chains side by side share one
//                          LDS read of delta_i); the blocks of four rows are dealt to the waves from
//                          the LAST row down, so that z_j can replace delta_j in place -- no later
//                          block reads it -- behind one barrier per round.  m and Linv are
//                          wave-uniform: the wave index goes through readfirstlane and they arrive
//                          by the scalar operand path.  Wave 0 then adds z_j * z_j in ascending j.
//                          LDS: 512 d bytes -- 15 KiB at d = 30 (ten workgroups a CU), all 128 KiB at
//                          d = 256, where the four waves are what keeps the CU's SIMDs busy.
//                          With group_size 64 a workgroup IS a group: wave 0 forms e (dexp) beside
//                          s, both go to rows 0 and 1 of the tile, and one thread per radius adds
//                          its ordered chain -- no second launch.
//   evidence_group_kernel  group_size 128 and 256, one workgroup per group: e of every walker (dexp,
//                          in parallel) and s are staged through LDS 256 walkers at a time; one
//                          thread per radius carries the ordered chain across the tiles.
//   evidence_max_kernel    2 048 walkers per workgroup: the maximum of the order-preserving 64-bit
//                          keys of logpost (bestfit_kernels.hip's key; NaN skipped), one 64-bit
//                          atomic max per workgroup into the zeroed key of c.
//
// Vector stores only; the stream orders the launches.
#include "evidence_args.h"
#include "det_math.h"
#include <algorithm>

namespace mcmc {
namespace {

// m and Linv do not change while an accumulation runs: read through the constant address space, a
// wave-uniform index is a scalar load whatever barrier lies between
typedef const double __attribute__((address_space(4))) * cdbl;

// R^2 of the radius a chain thread carries (thread r < n_r; compile-time indices into the arguments)
__device__ __forceinline__ double ev_r2_of(const EvArgs& a, int tid)
{
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < kEvMaxRadii; ++q)
        if (tid == q) r2 = a.r2[q];
    return r2;
}

// one radius' ordered chain over n_l (a multiple of 8) walkers staged in LDS: reads batched, the
// additions strictly in ascending order
__device__ __forceinline__ void ev_chain(const double* ss, const double* se, int n_l, double r2, double& S,
                                         unsigned long long& n_in)
{
    for (int l0 = 0; l0 < n_l; l0 += 8) {
        double vs[8], ve[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { vs[q] = ss[l0 + q]; ve[q] = se[l0 + q]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool in = vs[q] <= r2;
            S = S + (in ? ve[q] : 0.0);
            n_in += in ? 1ull : 0ull;
        }
    }
}

__global__ void __launch_bounds__(kEvThreads) evidence_kernel(const EvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_ev[];   // [d][64]: delta, then z
    const int lane = threadIdx.x & (kEvLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = a.d;
    const int w = (int)blockIdx.x * kEvLanes + lane;
    const bool on = w < a.W;
    const cdbl m = (cdbl)(unsigned long long)a.m;
    const cdbl Linv = (cdbl)(unsigned long long)a.Linv;
    for (int i = wave; i < d; i += kEvThreads / kEvLanes) {
        const double xv = on ? a.x[(size_t)i * a.W + w] : 0.0;
        s_ev[i * kEvLanes + lane] = xv - m[i];
    }
    __syncthreads();
    const int nb = (d + kEvRows - 1) / kEvRows;
    for (int top = nb - 1; top >= 0; top -= kEvThreads / kEvLanes) {   // (uniform: every wave meets the barrier)
        const int b = top - wave;
        const int j0 = kEvRows * b;
        double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
        if (b >= 0) {
            // rows past d - 1 (the last block of a d that is no multiple of four) repeat row d - 1:
            // they are computed and dropped
            const cdbl L0 = Linv + (size_t)j0 * d;
            const cdbl L1 = Linv + (size_t)min(j0 + 1, d - 1) * d;
            const cdbl L2 = Linv + (size_t)min(j0 + 2, d - 1) * d;
            const cdbl L3 = Linv + (size_t)min(j0 + 3, d - 1) * d;
#pragma unroll 4
            for (int i = 0; i <= j0; ++i) {           // the part all four rows share
                const double dl = s_ev[i * kEvLanes + lane];
                z0 = z0 + L0[i] * dl;
                z1 = z1 + L1[i] * dl;
                z2 = z2 + L2[i] * dl;
                z3 = z3 + L3[i] * dl;
            }
            if (j0 + 1 < d) {                         // the triangle: row j0 + q ends at i = j0 + q
                const double dl = s_ev[(j0 + 1) * kEvLanes + lane];
                z1 = z1 + L1[j0 + 1] * dl;
                z2 = z2 + L2[j0 + 1] * dl;
                z3 = z3 + L3[j0 + 1] * dl;
            }
            if (j0 + 2 < d) {
                const double dl = s_ev[(j0 + 2) * kEvLanes + lane];
                z2 = z2 + L2[j0 + 2] * dl;
                z3 = z3 + L3[j0 + 2] * dl;
            }
            if (j0 + 3 < d) {
                const double dl = s_ev[(j0 + 3) * kEvLanes + lane];
                z3 = z3 + L3[j0 + 3] * dl;
            }
        }
        __syncthreads();      // every wave has read the rows this round replaces
        if (b >= 0) {
            s_ev[j0 * kEvLanes + lane] = z0;
            if (j0 + 1 < d) s_ev[(j0 + 1) * kEvLanes + lane] = z1;
            if (j0 + 2 < d) s_ev[(j0 + 2) * kEvLanes + lane] = z2;
            if (j0 + 3 < d) s_ev[(j0 + 3) * kEvLanes + lane] = z3;
        }
    }
    __syncthreads();
    double s = 0.0, e = 0.0;
    bool cl = false;
    if (wave == 0) {
#pragma unroll 8
        for (int j = 0; j < d; ++j) {
            const double z = s_ev[j * kEvLanes + lane];
            s = s + z * z;
        }
        if (!a.fused) {
            if (on) a.s[w] = s;
        } else {              // (group_size 64 divides W: every lane holds a walker)
            const double arg = ev_value(*a.ckey) - a.logpost[w];
            cl = arg > kEvClamp;
            e = dexp(cl ? kEvClamp : arg);
        }
    }
    if (!a.fused) return;     // (uniform)
    // the workgroup's 64 walkers are group blockIdx.x: rows 0 and 1 of the tile take s and e
    __syncthreads();
    if (wave == 0) {
        s_ev[lane] = s;
        s_ev[kEvLanes + lane] = e;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.n_r) {
        double S = 0.0;
        unsigned long long n_in = 0ull;
        ev_chain(s_ev, s_ev + kEvLanes, kEvLanes, ev_r2_of(a, threadIdx.x), S, n_in);
        const size_t k = (size_t)blockIdx.x * a.n_r + threadIdx.x;
        a.acc[k] = a.acc[k] + S;
        a.cnt[k] += n_in;
    }
    if (wave == 0) {
        const unsigned long long n_clamp = (unsigned long long)__popcll(lanes(cl));
        if (lane == 0 && n_clamp != 0ull) atomicAdd(a.clamped, n_clamp);
    }
}

__global__ void __launch_bounds__(kEvThreads) evidence_group_kernel(const EvArgs a)
{
    __shared__ double ss[kEvThreads], se[kEvThreads];
    const int g = blockIdx.x, tid = threadIdx.x;
    const double c = ev_value(*a.ckey);
    const double r2 = ev_r2_of(a, tid);
    double S = 0.0;
    unsigned long long n_in = 0ull, n_clamp = 0ull;
    for (int t0 = 0; t0 < a.gs; t0 += kEvThreads) {
        const int l = t0 + tid;
        double sv = 0.0, ev = 0.0;
        if (l < a.gs) {
            const size_t w = (size_t)g * a.gs + l;
            const double arg = c - a.logpost[w];
            const bool cl = arg > kEvClamp;
            ev = dexp(cl ? kEvClamp : arg);
            sv = a.s[w];
            n_clamp += cl ? 1ull : 0ull;
        }
        __syncthreads();      // (the chains of the tile before have read it)
        ss[tid] = sv;
        se[tid] = ev;
        __syncthreads();
        if (tid < a.n_r) ev_chain(ss, se, min(kEvThreads, a.gs - t0), r2, S, n_in);   // (a multiple of 8)
    }
    if (tid < a.n_r) {
        const size_t k = (size_t)g * a.n_r + tid;
        a.acc[k] = a.acc[k] + S;
        a.cnt[k] += n_in;
    }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) n_clamp += __shfl_xor(n_clamp, mk, 64);
    if ((tid & 63) == 0 && n_clamp != 0ull) atomicAdd(a.clamped, n_clamp);
}

__global__ void __launch_bounds__(kEvThreads) evidence_max_kernel(const EvArgs a)
{
    __shared__ unsigned long long sk[kEvThreads / 64];
    unsigned long long k = 0ull;
    const int w0 = (int)blockIdx.x * (kEvThreads * kEvMaxPerThread) + (int)threadIdx.x;
    double p[kEvMaxPerThread];
#pragma unroll
    for (int q = 0; q < kEvMaxPerThread; ++q) {          // the loads travel together
        const int w = w0 + q * kEvThreads;
        p[q] = w < a.W ? a.logpost[w] : __longlong_as_double(-1ll);   // (a NaN: skipped)
    }
#pragma unroll
    for (int q = 0; q < kEvMaxPerThread; ++q)
        if (p[q] == p[q]) {
            const unsigned long long key = ev_key(p[q]);
            k = key > k ? key : k;
        }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        const unsigned long long o = __shfl_xor(k, mk, 64);
        k = o > k ? o : k;
    }
    if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < kEvThreads / 64; ++v) k = sk[v] > k ? sk[v] : k;
        if (k != 0ull) atomicMax(a.ckey, k);              // (no logpost is a number: the key stays 0, c = 0)
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_evidence(const mcmc::EvArgs* a, hipStream_t st)
{
    if (a->W <= 0 || a->G <= 0 || a->n_r <= 0) return hipSuccess;
    if (a->d < 1 || a->d > mcmc::kEvMaxDim || a->n_r > mcmc::kEvMaxRadii || a->gs < 8 || a->gs % 8 ||
        (long long)a->G * a->gs != a->W)
        return hipErrorInvalidValue;
    mcmc::EvArgs b = *a;
    b.fused = a->gs == mcmc::kEvLanes ? 1 : 0;
    const size_t lds = sizeof(double) * (size_t)mcmc::kEvLanes * std::max(a->d, 2);   // (two rows for s and e)
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)mcmc::evidence_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mcmc::evidence_kernel, dim3((unsigned)((a->W + mcmc::kEvLanes - 1) / mcmc::kEvLanes)),
                       dim3(mcmc::kEvThreads), lds, st, b);
    if (!b.fused)
        hipLaunchKernelGGL(mcmc::evidence_group_kernel, dim3((unsigned)a->G), dim3(mcmc::kEvThreads), 0, st, b);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_evidence_max(const mcmc::EvArgs* a, hipStream_t st)
{
    if (a->W <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a->ckey, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const int per = mcmc::kEvThreads * mcmc::kEvMaxPerThread;
    hipLaunchKernelGGL(mcmc::evidence_max_kernel, dim3((unsigned)((a->W + per - 1) / per)), dim3(mcmc::kEvThreads), 0,
                       st, *a);
    return hipGetLastError();
}
