// The affine-invariant stretch move (Goodman & Weare 2010, in the parallel half-ensemble form of
// Foreman-Mackey et al. 2013) around a function target (gfx950).  DESIGN.md section 2, "Stretch
// move", is the normative text; the shape is fn_walker_kernel's (function_kernels.hip):
//
//     stretch_kernel<ACCEPT, PROPOSE>
//         ACCEPT   the test of the trial the previous launch proposed for half `half_accept` and the
//                  function evaluated -- E_a > (logpost - lt) / temperature - (d - 1) log z --, the
//                  bookkeeping of every other target, commit of x
//         PROPOSE  for half `half_propose`: one Philox block per walker -> partner in the OTHER half
//                  of its own group, stretch factor z, E_a; trial t = fma(z, x - p, p) with p the
//                  partner's CURRENT state; prior support and normal priors in eval_point's order
//
// A step is two half-updates, so the launches of a call run  P(0) | f | A(0)+P(1) | f | A(1)+P(0) |
// ... | A(1): the half a launch accepts is the half its proposals take their partners from.
//
// Packing.  A half-update moves W / 2 walkers, and threads are mapped to ACTIVE walkers: thread
// k = g (gs / 2) + m serves walker g gs + h gs / 2 + m, so no half-wave idles.  Everything a trial
// carries between its two halves (row of `points`, lp_t, Ea, q, ll_t) is indexed by k.
//
// Ordering.  The accepts of half h must be complete and visible before the proposals of half 1 - h
// read their partners.  A workgroup owns WHOLE groups -- max(64, gs / 2) threads: two groups of 64,
// or one group of 128 or 256 -- so the walkers whose accept a proposal depends on are committed by
// threads of the same workgroup, and one workgroup barrier (with its workgroup-scope release /
// acquire: the waves of a workgroup share the CU's vector L1) between the two roles orders them.
// No other workgroup touches those lines: a half-group's part of a dimension is >= 256 bytes and
// 256-byte aligned.  The alternative -- accept and propose as separate launches -- costs one more
// launch per half-update on the critical path between two calls of the function.
//
// Partner gather.  x[i][partner] per dimension is a scattered read inside the 256 B .. 1 KiB the
// other half-group takes in that dimension: at most 2 .. 8 lines per wave-instruction, all of them
// just written (or read) by this workgroup.  Trial rows leave through the padded LDS tile in whole
// rows, exactly as fn_walker_kernel's do; a wave of a workgroup of two has a tile of its own.
#include "det_math.h"
#include "stretch_args.h"

namespace mcmc {
namespace {

typedef const double __attribute__((address_space(4))) * cdbl;

// tile[c][row] <-> points[k0 + row][i0 + c], c < tw, row < nrows: fn_tile_copy with a bound on the
// rows (the last workgroup of an odd number of 64-walker groups holds 32 active walkers)
template <bool TO_GLOBAL>
__device__ __forceinline__ void st_tile_copy(double* __restrict__ tile, double* __restrict__ rows,
                                             const int d, const int tw, const int lane, const int nrows)
{
    const int q = 64 / tw, rm = 64 % tw;   // (wave-uniform)
    int row = lane / tw, c = lane % tw;
    for (int f = 0; f < 64 * tw; f += 64) {
        if (row < nrows) {
            double* g = rows + (size_t)row * d + c;
            double* l = tile + c * kFnTileStride + row;
            if (TO_GLOBAL) *g = *l;
            else *l = *g;
        }
        row += q; c += rm;
        if (c >= tw) { c -= tw; ++row; }
    }
}

template <bool ACCEPT, bool PROPOSE>
__global__ void __launch_bounds__(128) stretch_kernel(const StretchArgs a)
{
    __shared__ double tiles[2][kFnTileDims * kFnTileStride];
    const StepArgs& s = a.s;
    const int d = a.d, W = s.W;
    const int hg = 1 << a.log2_half, n_act = W >> 1;
    const int lane = threadIdx.x & 63;
    double* const tile = tiles[threadIdx.x >> 6];
    const int k0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63);   // first active index of the wave
    const int nrows = (n_act - k0) < 64 ? (n_act - k0) : 64;       // (wave-uniform; 32 or 64)
    const bool act = lane < nrows;
    const int k = act ? k0 + lane : n_act - 1;                      // (idle lanes: clamped, no stores)
    const int g = k >> a.log2_half, m = k & (hg - 1);
    const int base = g * s.group_size + m;
    const ConstLayout cl{d, 0};
    const cdbl C = (cdbl)(unsigned long long)s.cblock;
    double* const rows = a.points + (size_t)k0 * d;
    if (ACCEPT) {
        const int w = base + a.half_accept * hg;
        const uint32_t gid = s.walker0 + (uint32_t)w;
        const double lpost = s.logpost[w];
        int wt = s.weight[w], prej = s.prior_rej[w], burn = s.burn_left[w];
        const double lp = a.lp_t[k], Ea = a.Ea[k], q = a.q[k];
        const double ll = a.ll_t[k];
        const bool inb = lp != -INFINITY;
        // a value inside the support that is NaN or +inf is an error of the target, not a rejection
        const bool bad = inb && (ll != ll || ll == INFINITY);
        if (bad && act) atomicCAS(a.bad, 0, 1 + (int)gid);
        const double lt = inb ? lp + ll : -INFINITY;
        // (the Jacobian factor z^(d - 1) is not tempered)
        const bool accept = act && inb && !bad && lt != -INFINITY && Ea > (lpost - lt) / s.temperature - q;
        if (accept) {
            if (burn > 0) --burn;
            s.logprior[w] = lp; s.loglike[w] = ll; s.logpost[w] = lt;
            s.n_accept[w] += 1;
        }
        prej = accept ? 0 : (prej + (inb ? 0 : 1));
        wt = accept ? 1 : wt + 1;
        if (!accept && act) {
            const double max_now = s.max_tries * (burn > 0 ? 10.0 : 1.0);
            if ((double)(wt - prej) > max_now) atomicCAS(s.stuck, 0, 1 + (int)gid);
        }
        if (act) { s.weight[w] = wt; s.prior_rej[w] = prej; s.burn_left[w] = burn; }
        wave_add_accepts(s.accept_total, accept ? 1 : 0);
        for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
            const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
            st_tile_copy<false>(tile, rows + i0, d, tw, lane, nrows);
            __syncthreads();
            if (accept)
                for (int c = 0; c < tw; ++c) s.x[(size_t)(i0 + c) * W + w] = tile[c * kFnTileStride + lane];
            __syncthreads();   // the tile is reused (by the next tile, or by PROPOSE)
        }
    }
    if (ACCEPT && PROPOSE) {
        // every commit of this workgroup's groups is visible to its proposals
        __threadfence_block();
        __syncthreads();
    }
    if (PROPOSE) {
        const int w = base + a.half_propose * hg;
        const uint32_t gid = s.walker0 + (uint32_t)w;
        const u32x4 r4 = philox4x32_10(s.key0, s.key1, gid, kStreamStretch, (uint32_t)s.step0,
                                       (uint32_t)(s.step0 >> 32));
        const int pm = (int)(r4.w0 >> (32 - a.log2_half));
        const int wp = g * s.group_size + (1 - a.half_propose) * hg + pm;   // the partner
        const uint64_t kz = ((uint64_t)r4.w1 << 20) | (r4.w2 >> 12);
        const uint64_t ka = ((uint64_t)r4.w3 << 20) | ((uint64_t)(r4.w2 & 0xFFFu) << 8) | (r4.w0 & 0xFFu);
        const double sz = fma(a.a - 1.0, u52(kz), 1.0);
        const double z = (sz * sz) / a.a;
        const double Ea = -dlog(u52(ka));
        bool inb = true;
        const int cm = d > 32 ? 3 : 0;   // chain of dimension i: i & cm
        double sc0 = 0.0, sc1 = 0.0, sc2 = 0.0, sc3 = 0.0;
        for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
            const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
            // the tile's part of x and of the partner first, every load in flight at once
            double xs[kFnTileDims], ps[kFnTileDims];
#pragma unroll
            for (int c = 0; c < kFnTileDims; ++c)
                if (c < tw) {
                    xs[c] = s.x[(size_t)(i0 + c) * W + w];
                    ps[c] = s.x[(size_t)(i0 + c) * W + wp];
                }
#pragma unroll
            for (int c = 0; c < kFnTileDims; ++c) {
                if (c >= tw) continue;   // (wave-uniform)
                const int i = i0 + c;
                const double t = fma(z, xs[c] - ps[c], ps[c]);
                tile[c * kFnTileStride + lane] = t;
                inb = inb && t <= C[cl.hi() + i] && t >= C[cl.lo() + i];
                if ((a.norm_mask4[i >> 5] >> (i & 31)) & 1u) {   // (wave-uniform)
                    const double u = (t - C[cl.loc() + i]) / C[cl.scale() + i];
                    const double term = fma(-0.5 * u, u, C[cl.mls() + i]);
                    const int ch = i & cm;
                    sc0 = ch == 0 ? sc0 + term : sc0;
                    sc1 = ch == 1 ? sc1 + term : sc1;
                    sc2 = ch == 2 ? sc2 + term : sc2;
                    sc3 = ch == 3 ? sc3 + term : sc3;
                }
            }
            __syncthreads();
            st_tile_copy<true>(tile, rows + i0, d, tw, lane, nrows);
            if (i0 + kFnTileDims < d) __syncthreads();   // the tile is reused
        }
        if (act) {
            const double sc = d > 32 ? (sc0 + sc1) + (sc2 + sc3) : sc0;
            a.lp_t[k] = inb ? s.uniform_logp + sc : -INFINITY;
            a.Ea[k] = Ea;
            a.q[k] = a.dm1 * dlog(z);
        }
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_stretch(const mcmc::StretchArgs* a, int accept, int propose,
                                              hipStream_t st)
{
    using namespace mcmc;
    const int gs = a->s.group_size, hg = gs / 2;
    if (a->d < 1 || a->d > 128 || (gs != 64 && gs != 128 && gs != 256) || a->s.W <= 0 || a->s.W % gs != 0 ||
        (1 << a->log2_half) != hg || (accept && (a->half_accept | 1) != 1) ||
        (propose && (a->half_propose | 1) != 1) || (accept && propose && a->half_accept == a->half_propose))
        return hipErrorInvalidValue;
    // a workgroup owns whole groups: two of 64 walkers, or one of 128 or 256
    const int block = hg < 64 ? 64 : hg;
    const int n_act = a->s.W / 2;
    const dim3 g((n_act + block - 1) / block), b(block);
    mcmc_hip_note_step_kernel("mcmc::stretch_kernel");
    if (accept && propose) hipLaunchKernelGGL((stretch_kernel<true, true>), g, b, 0, st, *a);
    else if (accept) hipLaunchKernelGGL((stretch_kernel<true, false>), g, b, 0, st, *a);
    else if (propose) hipLaunchKernelGGL((stretch_kernel<false, true>), g, b, 0, st, *a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
