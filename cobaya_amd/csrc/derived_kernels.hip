// Moments of the derived parameters (gfx950): what a moment snapshot keeps of the derived rows
// z[m][W] the caller has filled from the state x[d][W].  The rule ("Derived"):
// with a_j = z_j - shift_j and b_c = x_{cross[c]} - (moment shift)_{cross[c]}, a walker is USED iff
// all m of its derived values are finite; per group g of group_size walkers, over the used walkers,
//     N[g] (an integer)   A[g][j] = sum a_j   B[g][j][k] = sum a_j * a_k (k <= j)   C[g][j][c] = sum a_j * b_c
// and, beside them, X[g][c] = sum b_c and V[g][c] = sum b_c * b_c (what a cross-covariance and a
// correlation need of the sampled parameters over the SAME walkers: a further row a_m = 1 of a used
// walker, whose products are exact, and a row that is the column itself),
// each ONE chain over the group's walkers in ascending order from +0.0, the product and the addition
// as separate roundings (-ffp-contract=off).  The pooled accumulators then add the groups in ascending
// order, starting from their current value, the way pool_moments_kernel does.  Per name, exact and
// whatever the order: bad[j] counts the non-finite values, min[j] / max[j] of the finite ones are
// kept as order-preserving 64-bit keys under an integer atomic max (bestfit_kernels.hip's key).
//
//   derived_group_kernel  one workgroup per (group, block of 32 columns).  A COLUMN is what a_j is
//                         multiplied with: the constant 1 of a used walker (the chain is A[j]: a * 1.0
//                         is exact), a_k, or b_c -- n_col = 1 + m + n_cross of them.  The group is
//                         walked in chunks of 64 walkers, so a group may be far larger than LDS: per
//                         chunk z is read coalesced along w into the tile a[32][65], wave 0 marks the
//                         used walkers, the tile is shifted in place (row m becomes the 1 of X; an
//                         unused walker becomes 0.0 in every row and column: it adds +0.0, which no
//                         chain that began at +0.0 can tell from skipping it), and the block's
//                         columns go to c[32][65].  A lane
//                         owns a column, a thread up to five rows j = tid / 32 + 8 q: independent
//                         chains, carried in registers across the chunks, that share one read of the
//                         column; a_j is a broadcast, the column read has an odd row stride (65: the
//                         32 lanes of a half-wave hit 32 different bank pairs).  Reads are batched eight
//                         walkers at a time, the additions stay in order.
//   derived_pool_kernel   one thread per (j, column): adds the G group values to the accumulator in
//                         ascending order; one more thread adds N.  A launch boundary separates the two.
//
// Nothing depends on the launch geometry.  Vector stores only; the stream orders the launches.
#include "derived_args.h"

namespace mcmc {
namespace {

__device__ __forceinline__ bool dv_finite(double v)
{
    return (((unsigned long long)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull;
}

// column cg of row j is kept: A, the lower triangle of B, all of C; of rows m (the ones) and m + 1
// (the column itself) X and V alone
__device__ __forceinline__ bool dv_kept(int j, int cg, int m, int n_col)
{
    if (j > m + 1 || cg >= n_col) return false;
    return j >= m ? cg > m : !(cg >= 1 && cg <= m && cg - 1 > j);
}

// the chains of a thread over n8 (a multiple of 8, <= kDvChunk) staged walkers
template <int NQ>
__device__ __forceinline__ void dv_chains(const double* __restrict__ sa, const double* __restrict__ col, int n8,
                                          int jr, int m, double (&acc)[kDvMaxPasses])
{
    const double* row[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j = jr + kDvRowsPerPass * q;
        row[q] = j == m + 1 ? col : sa + j * kDvLd;        // (row m + 1: the column itself, V)
    }
    for (int l0 = 0; l0 < n8; l0 += 8) {
        double cv[8], av[NQ][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cv[u] = col[l0 + u];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int u = 0; u < 8; ++u) av[q][u] = row[q][l0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = acc[q] + av[q][u] * cv[u];
    }
}

__global__ void __launch_bounds__(kDvThreads) derived_group_kernel(const DvArgs a)
{
    __shared__ double sa[kDvMaxPasses * kDvRowsPerPass * kDvLd];   // a[j][l]: raw z, then shifted; row m: the ones
    __shared__ double sc[kDvCols * kDvLd];         // the block's columns
    __shared__ int s_used[kDvChunk];
    __shared__ unsigned long long s_bad[kDvMaxNames], s_kmax[kDvMaxNames], s_kmin[kDvMaxNames];
    const int tid = threadIdx.x, g = blockIdx.x, cb = blockIdx.y;
    const int c = tid & (kDvCols - 1), jr = tid >> 5;      // chains: a lane per column
    const int l = tid & (kDvChunk - 1), r0 = tid >> 6;     // staging: a lane per walker, four rows side by side
    const int m = a.m, nq = (m + 1 + kDvRowsPerPass) / kDvRowsPerPass, rows = kDvRowsPerPass * nq;   // (m + 2 rows)
    const bool stats = cb == 0;                            // (one block of columns keeps N, bad, min, max)
    if (tid < kDvMaxNames) s_bad[tid] = s_kmax[tid] = s_kmin[tid] = 0ull;
    double acc[kDvMaxPasses] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned long long n_used = 0ull;
    for (int t0 = 0; t0 < a.gs; t0 += kDvChunk) {
        const int n_l = min(kDvChunk, a.gs - t0);
        const bool on = l < n_l;
        const size_t w = (size_t)g * a.gs + t0 + l;
        for (int j = r0; j < rows; j += kDvThreads / kDvChunk)
            sa[j * kDvLd + l] = (on && j < m) ? a.z[(size_t)j * a.W + w] : 0.0;
        __syncthreads();
        if (tid < kDvChunk) {                              // wave 0: which walkers are used
            bool u = on;
            for (int j = 0; j < m; ++j) u = u && dv_finite(sa[j * kDvLd + l]);
            s_used[l] = u ? 1 : 0;
            n_used += (unsigned long long)__popcll(__ballot(u));
        }
        if (stats) {                                       // row j belongs to wave j % 4, chunk after chunk
            for (int j = r0; j < m; j += kDvThreads / kDvChunk) {
                const double v = sa[j * kDvLd + l];
                const bool fin = on && dv_finite(v);
                const unsigned long long key = dv_key(v);
                unsigned long long kx = fin ? key : 0ull, kn = fin ? ~key : 0ull;
                const unsigned long long nb = (unsigned long long)__popcll(__ballot(on && !fin));
#pragma unroll
                for (int mk = 32; mk >= 1; mk >>= 1) {
                    const unsigned long long ox = __shfl_xor(kx, mk, 64), on_ = __shfl_xor(kn, mk, 64);
                    kx = ox > kx ? ox : kx;
                    kn = on_ > kn ? on_ : kn;
                }
                if (l == 0) {
                    s_bad[j] += nb;
                    s_kmax[j] = kx > s_kmax[j] ? kx : s_kmax[j];
                    s_kmin[j] = kn > s_kmin[j] ? kn : s_kmin[j];
                }
            }
        }
        __syncthreads();
        const bool u = s_used[l] != 0;
        for (int j = r0; j < m; j += kDvThreads / kDvChunk)          // (a thread rewrites what it staged)
            sa[j * kDvLd + l] = u ? sa[j * kDvLd + l] - a.shift[j] : 0.0;
        if (tid < kDvChunk) sa[m * kDvLd + l] = u ? 1.0 : 0.0;
        for (int r = r0; r < kDvCols; r += kDvThreads / kDvChunk) {
            const int cg = cb * kDvCols + r;
            double v = 0.0;
            if (u && cg < a.n_col) {
                if (cg == 0) {
                    v = 1.0;
                } else if (cg <= m) {
                    v = a.z[(size_t)(cg - 1) * a.W + w] - a.shift[cg - 1];
                } else {
                    const int i = a.cross[cg - m - 1];
                    v = a.x[(size_t)i * a.W + w] - a.xshift[i];
                }
            }
            sc[r * kDvLd + l] = v;
        }
        __syncthreads();
        const int n8 = (n_l + 7) & ~7;                     // (the tiles are zero past n_l)
        const double* col = sc + c * kDvLd;
        switch (nq) {
        case 1: dv_chains<1>(sa, col, n8, jr, m, acc); break;
        case 2: dv_chains<2>(sa, col, n8, jr, m, acc); break;
        case 3: dv_chains<3>(sa, col, n8, jr, m, acc); break;
        case 4: dv_chains<4>(sa, col, n8, jr, m, acc); break;
        default: dv_chains<5>(sa, col, n8, jr, m, acc); break;
        }
        __syncthreads();                                   // (the next chunk overwrites the tiles)
    }
    const int cg = cb * kDvCols + c;
#pragma unroll
    for (int q = 0; q < kDvMaxPasses; ++q) {
        const int j = jr + kDvRowsPerPass * q;
        if (q < nq && dv_kept(j, cg, m, a.n_col)) a.Sg[((size_t)g * (m + 2) + j) * a.n_col + cg] = acc[q];
    }
    if (stats) {
        if (tid == 0) a.Ng[g] = n_used;
        if (tid < m) {
            if (s_bad[tid] != 0ull) atomicAdd(&a.bad[tid], s_bad[tid]);
            if (s_kmax[tid] != 0ull) atomicMax(&a.kmax[tid], s_kmax[tid]);
            if (s_kmin[tid] != 0ull) atomicMax(&a.kmin[tid], s_kmin[tid]);
        }
    }
}

__global__ void __launch_bounds__(64) derived_pool_kernel(const DvArgs a)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int n_chain = (a.m + 2) * a.n_col;
    if (q == n_chain) {                                    // N: an integer, any order
        unsigned long long n = *a.N;
        int g = 0;
        for (; g + 64 <= a.G; g += 64) {
            unsigned long long v[64];
#pragma unroll
            for (int u = 0; u < 64; ++u) v[u] = a.Ng[g + u];
#pragma unroll
            for (int u = 0; u < 64; ++u) n += v[u];
        }
        for (; g < a.G; ++g) n += a.Ng[g];
        *a.N = n;
        return;
    }
    if (q > n_chain) return;
    const int j = q / a.n_col, cg = q - j * a.n_col;
    if (!dv_kept(j, cg, a.m, a.n_col)) return;
    const double* __restrict__ src = a.Sg + q;
    const size_t stride = (size_t)n_chain;
    double acc = a.S[q];
    int g = 0;
    // loads batched 64 deep (a batch is one L2 round trip; pool_moments_kernel's lesson: 16 deep, the 256
    // groups of config 2 took 22 us here), additions strictly in ascending group order
    for (; g + 64 <= a.G; g += 64) {
        double v[64];
#pragma unroll
        for (int u = 0; u < 64; ++u) v[u] = src[(size_t)(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 64; ++u) acc += v[u];
    }
    for (; g + 16 <= a.G; g += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = src[(size_t)(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; g < a.G; ++g) acc += src[(size_t)g * stride];
    a.S[q] = acc;
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_derived(const mcmc::DvArgs* a, hipStream_t st)
{
    if (a->W <= 0 || a->G <= 0 || a->m <= 0) return hipSuccess;
    if (a->m > mcmc::kDvMaxNames || a->n_cross < 0 || a->n_cross > mcmc::kDvMaxCross ||
        a->n_col != 1 + a->m + a->n_cross || a->gs < 1 || (long long)a->G * a->gs != a->W)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a->n_col + mcmc::kDvCols - 1) / mcmc::kDvCols);
    hipLaunchKernelGGL(mcmc::derived_group_kernel, dim3((unsigned)a->G, blocks), dim3(mcmc::kDvThreads), 0, st, *a);
    const int n_thread = (a->m + 2) * a->n_col + 1;
    hipLaunchKernelGGL(mcmc::derived_pool_kernel, dim3((unsigned)((n_thread + 63) / 64)), dim3(64), 0, st, *a);
    return hipGetLastError();
}
