// Best fit, MAP and profile likelihoods of the ensemble (gfx950): what a moment snapshot keeps of
// where the posterior and the likelihood peak.  The rule ("Best fit and
// profiles"): the ordering key of a double v is key(v) = b ^ ((b >> 63) ? ~0 : 1 << 63) with
// b = bits(v) -- an unsigned 64-bit integer whose order is the order of the doubles; NaN is skipped
// and 0 means "empty".  Every statistic here is a MAXIMUM of keys, so it depends neither on the
// order of the atomics nor on the launch geometry.
//
//   bestfit_kernel          one workgroup per (profile entry, slice of walkers): the entry's row of
//                           x and the value row are read coalesced, the walker's bin is the
//                           marginals' rule (in range iff lo <= x <= hi,
//                           k = min((int)floor((x - lo) * s), B - 1), separate roundings), and
//                           uint64 best[B] in LDS takes the keys with 64-bit LDS atomicMax; the
//                           non-empty bins go to the slab with 64-bit global atomicMax.  The same
//                           launch carries one more workgroup per slice, which reduces its slice
//                           to the candidates (key, lowest walker id) of logpost and loglike and
//                           stores them with plain stores.
//   bestfit_commit_kernel   one workgroup, queued behind it: reduces the candidates, compares
//                           with the two device records and copies the winner's scalars and x[d]
//                           where the key is STRICTLY greater.
//
// No tickets, spin-waits or cross-workgroup flags: the stream orders the two launches.
#include "bestfit_args.h"

namespace mcmc {
namespace {

constexpr int kUnroll = 4;
constexpr int kWaves = kBfThreads / 64;
constexpr unsigned long long kNoWalker = ~0ull;

__device__ __forceinline__ unsigned long long bf_bits(double v)
{
    return (unsigned long long)__double_as_longlong(v);
}

__device__ __forceinline__ unsigned long long bf_key(double v)
{
    const unsigned long long b = bf_bits(v);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}

// bin of an in-range value (the marginals' rule); max(.., 0) never acts on a finite in-range
// value -- it keeps the LDS index in bounds whatever the host handed down
__device__ __forceinline__ int bf_bin(double x, double lo, double s, int B)
{
    const double t = (x - lo) * s;
    const int k = (int)floor(t);
    return max(min(k, B - 1), 0);
}

// (key, walker) a beats b: the greater key, on a tie the lower walker id
__device__ __forceinline__ bool bf_beats(unsigned long long ka, unsigned long long wa,
                                         unsigned long long kb, unsigned long long wb)
{
    return ka > kb || (ka == kb && wa < wb);
}

// the best (key, walker) of the workgroup, returned to every thread; `sk`, `sw`: [kWaves] of LDS
__device__ __forceinline__ void bf_block_best(unsigned long long& k, unsigned long long& w,
                                              unsigned long long* sk, unsigned long long* sw)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long ok = __shfl_xor(k, m, 64), ow = __shfl_xor(w, m, 64);
        if (bf_beats(ok, ow, k, w)) { k = ok; w = ow; }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // (the arrays may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) { sk[wave] = k; sw[wave] = w; }
    __syncthreads();
    k = sk[0]; w = sw[0];
#pragma unroll
    for (int v = 1; v < kWaves; ++v)
        if (bf_beats(sk[v], sw[v], k, w)) { k = sk[v]; w = sw[v]; }
}

__global__ void __launch_bounds__(kBfThreads) bestfit_kernel(const BfArgs a)
{
    extern __shared__ unsigned long long best[];
    __shared__ unsigned long long sk[kWaves], sw[kWaves];
    const int n_prof = a.n_entries * a.n_slices;
    if ((int)blockIdx.x < n_prof) {
        // ---- a profile entry over one slice
        const int e = blockIdx.x / a.n_slices;
        const int sl = blockIdx.x - e * a.n_slices;
        const BfEntry E = a.entries[e];
        const int B = a.B;
        for (int k = threadIdx.x; k < B; k += kBfThreads) best[k] = 0ull;
        __syncthreads();
        const int w0 = sl * a.slice;
        const int w1 = min(w0 + a.slice, a.W);
        const double* __restrict__ xi = a.x + (size_t)E.i * a.W;
        const double* __restrict__ val = a.value;
        for (int wb = w0 + (int)threadIdx.x; wb < w1; wb += kBfThreads * kUnroll) {
            double vx[kUnroll], vv[kUnroll];
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                const int w = wb + r * kBfThreads;
                const bool on = w < w1;
                vx[r] = on ? xi[w] : 0.0;
                vv[r] = on ? val[w] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                if (wb + r * kBfThreads >= w1) continue;
                const double x = vx[r], v = vv[r];
                if (!(x >= E.lo && x <= E.hi) || v != v) continue;
                const int k = bf_bin(x, E.lo, E.s, B);
                const unsigned long long key = bf_key(v);
                // the bins only grow: a plain read that is stale is lower, and the atomic follows
                if (key > best[k]) atomicMax(&best[k], key);
            }
        }
        __syncthreads();
        unsigned long long* __restrict__ out = a.slab + (size_t)e * B;
        for (int k = threadIdx.x; k < B; k += kBfThreads) {
            const unsigned long long c = best[k];
            if (c != 0ull) atomicMax(&out[k], c);
        }
        return;
    }
    // ---- the candidates of one slice for the two records
    const int sl = (int)blockIdx.x - n_prof;
    if (sl >= a.n_slices) return;
    const int w0 = sl * a.slice;
    const int w1 = min(w0 + a.slice, a.W);
    unsigned long long kp = 0ull, wp = kNoWalker, kl = 0ull, wl = kNoWalker;
    for (int w = w0 + (int)threadIdx.x; w < w1; w += kBfThreads) {   // ascending: the lowest id stays
        const double p = a.logpost[w], l = a.loglike[w];
        if (p == p) {
            const unsigned long long key = bf_key(p);
            if (key > kp) { kp = key; wp = (unsigned long long)w; }
        }
        if (l == l) {
            const unsigned long long key = bf_key(l);
            if (key > kl) { kl = key; wl = (unsigned long long)w; }
        }
    }
    bf_block_best(kp, wp, sk, sw);
    bf_block_best(kl, wl, sk, sw);
    if (threadIdx.x == 0) {
        unsigned long long* c = a.cand + (size_t)sl * (kBfRecords * 2);
        c[0] = kp; c[1] = wp; c[2] = kl; c[3] = wl;
    }
}

__global__ void __launch_bounds__(kBfThreads) bestfit_commit_kernel(const BfArgs a)
{
    __shared__ unsigned long long sk[kWaves], sw[kWaves];
    const int words = kBfRecordHead + a.d;
    for (int r = 0; r < kBfRecords; ++r) {
        unsigned long long k = 0ull, w = kNoWalker;
        for (int s = threadIdx.x; s < a.n_slices; s += kBfThreads) {
            const unsigned long long* c = a.cand + (size_t)s * (kBfRecords * 2) + 2 * r;
            if (bf_beats(c[0], c[1], k, w)) { k = c[0]; w = c[1]; }
        }
        bf_block_best(k, w, sk, sw);
        unsigned long long* rec = a.records + (size_t)r * words;
        const unsigned long long old = rec[0];
        __syncthreads();      // every thread has read the record's key before it is replaced
        if (k == 0ull || k <= old || w >= (unsigned long long)a.W) continue;   // (uniform)
        if (threadIdx.x == 0) {
            rec[0] = k;
            rec[1] = (unsigned long long)a.walker0 + w;
            rec[2] = a.step;
            rec[3] = bf_bits(a.logpost[w]);
            rec[4] = bf_bits(a.logprior[w]);
            rec[5] = bf_bits(a.loglike[w]);
        }
        for (int i = threadIdx.x; i < a.d; i += kBfThreads)
            rec[kBfRecordHead + i] = bf_bits(a.x[(size_t)i * a.W + w]);
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_bestfit(const mcmc::BfArgs* a, hipStream_t st)
{
    if (a->n_slices <= 0) return hipSuccess;
    const size_t lds = sizeof(unsigned long long) * (size_t)(a->n_entries > 0 ? a->B : 0);
    hipLaunchKernelGGL(mcmc::bestfit_kernel, dim3((unsigned)((a->n_entries + 1) * a->n_slices)),
                       dim3(mcmc::kBfThreads), lds, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_bestfit_commit(const mcmc::BfArgs* a, hipStream_t st)
{
    if (a->n_slices <= 0) return hipSuccess;
    hipLaunchKernelGGL(mcmc::bestfit_commit_kernel, dim3(1), dim3(mcmc::kBfThreads), 0, st, *a);
    return hipGetLastError();
}
