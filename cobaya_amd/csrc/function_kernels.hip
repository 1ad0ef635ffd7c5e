// Target kind `function` (gfx950): the Metropolis step around a log-likelihood that is NOT ours --
// a batched device function the user registered (mcmc_hip_set_target_function), which maps the
// (n, d) tensor of trial points to n log-likelihoods and queues its work on the engine's stream.
// The step is split where pl_walker_kernel splits it (pliklite_kernels.hip), for any d <= 128:
//
//     fn_walker_kernel<ACCEPT, PROPOSE>
//         ACCEPT   the Metropolis test of the trial a previous launch proposed and the function
//                  evaluated (mcmc.py:670-683), the bookkeeping of mcmc.py:685-748, commit of x
//         PROPOSE  variates of step a.s.step0 (un-paired stream, RandProposer1D at d = 1), trial
//                  t = fma(r, v, x) along the group's direction (proposal.py:69, 224), prior support
//                  and normal priors in eval_point's order (prior.py:733-763; one ascending chain
//                  for d <= 32, four interleaved chains for d > 32)
//
// (the accept of step s and the proposal of step s + 1 share a launch).  The state is dimension-
// major, x[d][W]: lane w reads x[i W + w], coalesced.  The function's input is POINT-major,
// points[W][d] -- what a (n, d) tensor is -- and a lane per walker writing its own row would be a
// scatter with a stride of 8 d bytes.  So a wave (64 walkers) stages a tile of 64 walkers x <= 32
// dimensions through LDS: the lanes write their trial into tile[dimension][walker] (65 doubles
// per dimension: the padding keeps both directions free of bank conflicts) and the wave then
// copies the tile out in the order of the rows, 64 consecutive doubles of the tile per
// instruction: whole rows of contiguous bytes (all 64 d doubles of the wave are ONE contiguous
// run for d <= 32; 256-byte row segments above).  The accept half reads the previous trial back
// through the same tile.  Per step 4 x 8 d W bytes cross HBM (x in, trial out; trial in, x out
// where accepted).  Measured (profiles/r08_device_function.txt): 38 us per step of 65 536 walkers
// at d = 30 -- what pl_walker_kernel takes at d = 27, 3.8 x the byte floor: one wave per SIMD,
// bound by the latency of its own chain, not by HBM.  The evaluation is the user's.
#include "det_math.h"
#include "function_args.h"

namespace mcmc {
namespace {

typedef const double __attribute__((address_space(4))) * cdbl;

// tile[c][walker] <-> points[w0 + row][i0 + c], c < tw: the flat index f = row tw + c walks the
// rows of the tile in memory order, 64 consecutive f per wave-instruction
template <bool TO_GLOBAL>
__device__ __forceinline__ void fn_tile_copy(double* __restrict__ tile, double* __restrict__ rows,
                                             const int d, const int tw, const int lane)
{
    const int q = 64 / tw, rm = 64 % tw;   // (wave-uniform)
    int row = lane / tw, c = lane % tw;
    for (int f = 0; f < 64 * tw; f += 64) {
        double* g = rows + (size_t)row * d + c;
        double* l = tile + c * kFnTileStride + row;
        if (TO_GLOBAL) *g = *l;
        else *l = *g;
        row += q; c += rm;
        if (c >= tw) { c -= tw; ++row; }
    }
}

template <bool ACCEPT, bool PROPOSE>
__global__ void __launch_bounds__(64) fn_walker_kernel(const FnWalkerArgs a)
{
    __shared__ double tile[kFnTileDims * kFnTileStride];
    const StepArgs& s = a.s;
    const int d = a.d, W = s.W;
    const int lane = threadIdx.x;
    const int w0 = blockIdx.x * 64, w = w0 + lane;
    const ConstLayout cl{d, 0};
    const cdbl C = (cdbl)(unsigned long long)s.cblock;
    const uint32_t gid = s.walker0 + (uint32_t)w;
    bool accept = false;
    if (ACCEPT) {
        const double lpost = s.logpost[w];
        int wt = s.weight[w], prej = s.prior_rej[w], burn = s.burn_left[w];
        const double lp = a.lp_t[w], Ea = a.Ea[w];
        const double ll = a.ll_t[w];
        const bool inb = lp != -INFINITY;
        // a value inside the support that is NaN or +inf is an error of the target, not a rejection
        const bool bad = inb && (ll != ll || ll == INFINITY);
        if (bad) atomicCAS(a.bad, 0, 1 + (int)gid);
        const double lt = inb ? lp + ll : -INFINITY;
        accept = inb && !bad && lt != -INFINITY && (lt > lpost || Ea > (lpost - lt) / s.temperature);
        if (accept) {
            if (burn > 0) --burn;
            s.logprior[w] = lp; s.loglike[w] = ll; s.logpost[w] = lt;
            s.n_accept[w] += 1;
        }
        prej = accept ? 0 : (prej + (inb ? 0 : 1));
        wt = accept ? 1 : wt + 1;
        if (!accept) {
            const double max_now = s.max_tries * (burn > 0 ? 10.0 : 1.0);
            if ((double)(wt - prej) > max_now) atomicCAS(s.stuck, 0, 1 + (int)gid);
        }
        s.weight[w] = wt; s.prior_rej[w] = prej; s.burn_left[w] = burn;
        wave_add_accepts(s.accept_total, accept ? 1 : 0);
    }
    double r = 0.0, Ea = 0.0;
    cdbl v = nullptr;
    if (PROPOSE) {
        step_variates(s.key0, s.key1, gid, s.step0, 0, d == 1, r, Ea);
        const int group = __builtin_amdgcn_readfirstlane(w / s.group_size);
        v = (cdbl)(unsigned long long)(s.V + ((size_t)group * s.ncyc + a.cyc) * (size_t)s.slab +
                                       (size_t)a.col * a.ld);
    }
    bool inb = true;
    const int cm = d > 32 ? 3 : 0;   // chain of dimension i: i & cm
    double sc0 = 0.0, sc1 = 0.0, sc2 = 0.0, sc3 = 0.0;
    double* const rows = a.points + (size_t)w0 * d;
    for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
        const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
        // the tile's part of x first, every load in flight at once (the dimensions of a tile are
        // unrolled: xs stays in registers)
        double xs[kFnTileDims];
        if (PROPOSE) {
#pragma unroll
            for (int c = 0; c < kFnTileDims; ++c)
                if (c < tw) xs[c] = s.x[(size_t)(i0 + c) * W + w];
        }
        if (ACCEPT) {
            fn_tile_copy<false>(tile, rows + i0, d, tw, lane);
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < kFnTileDims; ++c) {
            if (c >= tw) continue;   // (wave-uniform)
            const int i = i0 + c;
            double xi = PROPOSE ? xs[c] : 0.0;
            if (ACCEPT && accept) {
                xi = tile[c * kFnTileStride + lane];
                s.x[(size_t)i * W + w] = xi;
            }
            if (PROPOSE) {
                const double t = fma(r, v[i], xi);
                tile[c * kFnTileStride + lane] = t;
                inb = inb && t <= C[cl.hi() + i] && t >= C[cl.lo() + i];
                if ((a.norm_mask4[i >> 5] >> (i & 31)) & 1u) {   // (wave-uniform)
                    const double q = (t - C[cl.loc() + i]) / C[cl.scale() + i];
                    const double term = fma(-0.5 * q, q, C[cl.mls() + i]);
                    const int ch = i & cm;
                    sc0 = ch == 0 ? sc0 + term : sc0;
                    sc1 = ch == 1 ? sc1 + term : sc1;
                    sc2 = ch == 2 ? sc2 + term : sc2;
                    sc3 = ch == 3 ? sc3 + term : sc3;
                }
            }
        }
        if (PROPOSE) {
            __syncthreads();
            fn_tile_copy<true>(tile, rows + i0, d, tw, lane);
        }
        if (i0 + kFnTileDims < d) __syncthreads();   // the tile is reused
    }
    if (PROPOSE) {
        const double sc = d > 32 ? (sc0 + sc1) + (sc2 + sc3) : sc0;
        a.lp_t[w] = inb ? s.uniform_logp + sc : -INFINITY;
        a.Ea[w] = Ea;
    }
}

// ---- several functions over parameter blocks ("Function targets with
// parameter blocks").  The sibling of fn_walker_kernel for ONE slot of the blocked cycle:
//
//     ACCEPT   the log-likelihood of the trial is the sum over the functions c ascending of what
//              function c returned for it where it was DUE (a.due_prev) and of the carried
//              ll_c[c][w] where not; the NaN / +inf error looks at due values only; an accept
//              commits x from the full trial (w.points) and the due ll_c
//     PROPOSE  direction = column `w.col` (the slot) of the group's blocked directions, the
//              RandProposer1D variates when the slot's flag says so (a.oned); full trial through
//              the tile to w.points, support and log-prior as in fn_walker_kernel; then, per DUE
//              function (a.due), its inputs t[inputs[.]] through the same tile to pts[c], whole
//              contiguous rows.  The inputs are formed again as fma(r, v_i, x_i) from x in memory
//              -- the lane's own commit above, or the untouched state: the same bits -- so that no
//              trial of up to 128 dimensions has to stay in registers or LDS.
//
// Per step 8 W (sum of the due d_c) bytes are written on top of fn_walker_kernel's traffic and as
// many read again from L2.  Measured (profiles/r18_function_blocks.txt): 61 us per step of 65 536
// walkers at d = 30 with two functions of 10 and 30 inputs both due, 1.47 x fn_walker_kernel in
// the same session, where those bytes explain 1.67 x.  One wave per workgroup: a barrier waits
// for nobody else.
template <bool ACCEPT, bool PROPOSE>
__global__ void __launch_bounds__(64) fn_blocked_walker_kernel(const FnBlockedArgs a)
{
    __shared__ double tile[kFnTileDims * kFnTileStride];
    const StepArgs& s = a.w.s;
    const int d = a.w.d, W = s.W;
    const int lane = threadIdx.x;
    const int w0 = blockIdx.x * 64, w = w0 + lane;
    const ConstLayout cl{d, 0};
    const cdbl C = (cdbl)(unsigned long long)s.cblock;
    const uint32_t gid = s.walker0 + (uint32_t)w;
    bool accept = false;
    if (ACCEPT) {
        const double lpost = s.logpost[w];
        int wt = s.weight[w], prej = s.prior_rej[w], burn = s.burn_left[w];
        const double lp = a.w.lp_t[w], Ea = a.w.Ea[w];
        const bool inb = lp != -INFINITY;
        // new-or-carried values, summed left to right; NaN or +inf of a DUE function inside the
        // support is an error of the target, not a rejection
        double llc[kFnMaxFunctions];
        double ll = 0.0;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < kFnMaxFunctions; ++c) {
            if (c >= a.n_fn) continue;   // (wave-uniform)
            const bool due = (a.due_prev >> c) & 1u;
            const double v = due ? a.ll_new[c][w] : a.ll_c[(size_t)c * W + w];
            bad = bad || (due && (v != v || v == INFINITY));
            llc[c] = v;
            ll = c == 0 ? v : ll + v;
        }
        bad = bad && inb;
        if (bad) atomicCAS(a.w.bad, 0, 1 + (int)gid);
        const double lt = inb ? lp + ll : -INFINITY;
        accept = inb && !bad && lt != -INFINITY && (lt > lpost || Ea > (lpost - lt) / s.temperature);
        if (accept) {
            if (burn > 0) --burn;
            s.logprior[w] = lp; s.loglike[w] = ll; s.logpost[w] = lt;
            s.n_accept[w] += 1;
#pragma unroll
            for (int c = 0; c < kFnMaxFunctions; ++c)
                if (c < a.n_fn && ((a.due_prev >> c) & 1u)) a.ll_c[(size_t)c * W + w] = llc[c];
        }
        prej = accept ? 0 : (prej + (inb ? 0 : 1));
        wt = accept ? 1 : wt + 1;
        if (!accept) {
            const double max_now = s.max_tries * (burn > 0 ? 10.0 : 1.0);
            if ((double)(wt - prej) > max_now) atomicCAS(s.stuck, 0, 1 + (int)gid);
        }
        s.weight[w] = wt; s.prior_rej[w] = prej; s.burn_left[w] = burn;
        wave_add_accepts(s.accept_total, accept ? 1 : 0);
    }
    double r = 0.0, Ea = 0.0;
    cdbl v = nullptr;
    if (PROPOSE) {
        step_variates(s.key0, s.key1, gid, s.step0, 0, a.oned != 0, r, Ea);
        const int group = __builtin_amdgcn_readfirstlane(w / s.group_size);
        v = (cdbl)(unsigned long long)(s.V + ((size_t)group * s.ncyc + a.w.cyc) * (size_t)s.slab +
                                       (size_t)a.w.col * a.w.ld);
    }
    bool inb = true;
    const int cm = d > 32 ? 3 : 0;   // chain of dimension i: i & cm
    double sc0 = 0.0, sc1 = 0.0, sc2 = 0.0, sc3 = 0.0;
    double* const rows = a.w.points + (size_t)w0 * d;
    for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
        const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
        double xs[kFnTileDims];
        if (PROPOSE) {
#pragma unroll
            for (int c = 0; c < kFnTileDims; ++c)
                if (c < tw) xs[c] = s.x[(size_t)(i0 + c) * W + w];
        }
        if (ACCEPT) {
            fn_tile_copy<false>(tile, rows + i0, d, tw, lane);
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < kFnTileDims; ++c) {
            if (c >= tw) continue;   // (wave-uniform)
            const int i = i0 + c;
            double xi = PROPOSE ? xs[c] : 0.0;
            if (ACCEPT && accept) {
                xi = tile[c * kFnTileStride + lane];
                s.x[(size_t)i * W + w] = xi;
            }
            if (PROPOSE) {
                const double t = fma(r, v[i], xi);
                tile[c * kFnTileStride + lane] = t;
                inb = inb && t <= C[cl.hi() + i] && t >= C[cl.lo() + i];
                if ((a.w.norm_mask4[i >> 5] >> (i & 31)) & 1u) {   // (wave-uniform)
                    const double q = (t - C[cl.loc() + i]) / C[cl.scale() + i];
                    const double term = fma(-0.5 * q, q, C[cl.mls() + i]);
                    const int ch = i & cm;
                    sc0 = ch == 0 ? sc0 + term : sc0;
                    sc1 = ch == 1 ? sc1 + term : sc1;
                    sc2 = ch == 2 ? sc2 + term : sc2;
                    sc3 = ch == 3 ? sc3 + term : sc3;
                }
            }
        }
        if (PROPOSE) {
            __syncthreads();
            fn_tile_copy<true>(tile, rows + i0, d, tw, lane);
        }
        if (i0 + kFnTileDims < d) __syncthreads();   // the tile is reused
    }
    if (PROPOSE) {
        const double sc = d > 32 ? (sc0 + sc1) + (sc2 + sc3) : sc0;
        a.w.lp_t[w] = inb ? s.uniform_logp + sc : -INFINITY;
        a.w.Ea[w] = Ea;
        // the inputs of every due function, in the order it lists them
        for (int c = 0; c < a.n_fn; ++c) {
            if (!((a.due >> c) & 1u)) continue;   // (wave-uniform)
            const int dc = a.n_in[c];
            const int* __restrict__ idx = a.inputs + a.in_off[c];
            double* const rows_c = a.pts[c] + (size_t)w0 * dc;
            for (int j0 = 0; j0 < dc; j0 += kFnTileDims) {
                const int tw = (dc - j0) < kFnTileDims ? (dc - j0) : kFnTileDims;
                __syncthreads();   // the tile is reused
                for (int k = 0; k < tw; ++k) {
                    const int i = idx[j0 + k];   // (wave-uniform)
                    tile[k * kFnTileStride + lane] = fma(r, v[i], s.x[(size_t)i * W + w]);
                }
                __syncthreads();
                fn_tile_copy<true>(tile, rows_c + j0, dc, tw, lane);
            }
        }
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_fn_blocked_walker(const mcmc::FnBlockedArgs* a, int accept,
                                                        int propose, hipStream_t st)
{
    using namespace mcmc;
    if (a->w.d < 1 || a->w.d > 128 || a->w.s.W <= 0 || a->w.s.W % 64 != 0 || a->w.s.group_size % 64 != 0 ||
        a->n_fn < 1 || a->n_fn > kFnMaxFunctions)
        return hipErrorInvalidValue;
    for (int c = 0; c < a->n_fn; ++c)
        if (a->n_in[c] < 1 || a->n_in[c] > 128 || a->in_off[c] < 0) return hipErrorInvalidValue;
    const dim3 g(a->w.s.W / 64), b(64);
    mcmc_hip_note_step_kernel("mcmc::fn_blocked_walker_kernel");
    if (accept && propose) hipLaunchKernelGGL((fn_blocked_walker_kernel<true, true>), g, b, 0, st, *a);
    else if (accept) hipLaunchKernelGGL((fn_blocked_walker_kernel<true, false>), g, b, 0, st, *a);
    else if (propose) hipLaunchKernelGGL((fn_blocked_walker_kernel<false, true>), g, b, 0, st, *a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_fn_walker(const mcmc::FnWalkerArgs* a, int accept, int propose,
                                                hipStream_t st)
{
    using namespace mcmc;
    if (a->d < 1 || a->d > 128 || a->s.W <= 0 || a->s.W % 64 != 0 || a->s.group_size % 64 != 0)
        return hipErrorInvalidValue;
    const dim3 g(a->s.W / 64), b(64);
    mcmc_hip_note_step_kernel("mcmc::fn_walker_kernel");
    if (accept && propose) hipLaunchKernelGGL((fn_walker_kernel<true, true>), g, b, 0, st, *a);
    else if (accept) hipLaunchKernelGGL((fn_walker_kernel<true, false>), g, b, 0, st, *a);
    else if (propose) hipLaunchKernelGGL((fn_walker_kernel<false, true>), g, b, 0, st, *a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
