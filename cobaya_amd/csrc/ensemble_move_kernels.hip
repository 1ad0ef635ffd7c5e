// Mixtures of ensemble moves around a function target (gfx950): the stretch move, the
// differential-evolution move (ter Braak 2006; Nelson et al. 2013) and the snooker update (ter Braak &
// Vrugt 2008) in the half-ensemble form of stretch_kernels.hip.  DESIGN.md section 2, "Ensemble move
// mixtures", is the normative text.
//
//     ensemble_move_kernel<ACCEPT, KIND>
//         ACCEPT   half_accept: the test E_a > (logpost - lt) / temperature - q of
//                  the trial the previous launch proposed, whatever its kind -- the accept of half 1
//                  of step S shares a launch with a proposal of ANOTHER kind for step S + 1
//         KIND     the proposal for half `half_propose` (-1: none), with partners from the other half
//                  of the walker's own group, their CURRENT state:
//                  stretch   t = fma(z, x - p, p),                    q = (d - 1) log z    (stretch_kernel's bits)
//                  de        t = fma(gamma, p1 - p2, x),              q = 0
//                  snooker   t = fma(c, x - z, x), c = gamma_s s / n2, q = (d - 1) log(|t - z| / |x - z|)
//
// The kind is wave-uniform by construction: the host draws it once per step for the whole ensemble
// and it is a template argument here.  Halves, packing (threads on ACTIVE walkers), workgroups that
// own whole groups, the barrier and fence between the roles and the padded LDS tile the rows leave
// through are stretch_kernel's; see its header.  stretch_kernels.hip itself is untouched -- `move:
// stretch` keeps its kernel to the instruction --, so the accept role and the tile copy are restated
// here.
//
// Partner gather.  DE reads two partner rows and the walker's own, snooker three and its own:
// scattered reads inside the 256 B .. 1 KiB the other half-group takes per dimension, lines this
// workgroup has just written or read.  Snooker makes two passes over the dimensions -- the sums n2
// and s, then the trial --; at d <= 32 (one tile) x and z stay in registers between them, above
// they are read again from the cache (formed again, the same bits).
#include "det_math.h"
#include "ensemble_move_args.h"

namespace mcmc {
namespace {

typedef const double __attribute__((address_space(4))) * cdbl;

// tile[c][row] <-> points[k0 + row][i0 + c], c < tw, row < nrows: stretch_kernels.hip's bounded tile
// copy (the last workgroup of an odd number of 64-walker groups holds 32 active walkers)
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

// The ACCEPT role of a half-update, stretch_kernel's with one addition: the test of the trial of
// active walker k (walker w of the state), the bookkeeping of every other target, commit of x from
// the rows through the wave's tile.  Every thread of the workgroup calls it (barriers inside).  A
// trial whose q is -inf is VOID -- the proposal had no trial to make (the snooker walker that sits
// on its partner) --: it is rejected like a trial outside the support, lp_t = -inf, but is no
// prior rejection
__device__ __forceinline__ void half_accept(const StretchArgs& a, double* const tile, double* const rows,
                                            const int k, const int w, const bool act, const int lane,
                                            const int nrows)
{
    const StepArgs& s = a.s;
    const int d = a.d, W = s.W;
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
    // (the Jacobian factor in q is not tempered)
    const bool accept = act && inb && !bad && lt != -INFINITY && Ea > (lpost - lt) / s.temperature - q;
    if (accept) {
        if (burn > 0) --burn;
        s.logprior[w] = lp; s.loglike[w] = ll; s.logpost[w] = lt;
        s.n_accept[w] += 1;
    }
    const bool outside = !inb && q != -INFINITY;
    prej = accept ? 0 : (prej + (outside ? 1 : 0));
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

// Support and normal priors of a trial in eval_point's order: `add` per dimension, ascending; the
// log-prior is one chain for d <= 32, four interleaved ones above (stretch_kernel's operations)
struct TrialPrior {
    bool inb = true;
    double sc0 = 0.0, sc1 = 0.0, sc2 = 0.0, sc3 = 0.0;
    __device__ __forceinline__ void add(const StretchArgs& a, const cdbl C, const ConstLayout cl, const int i,
                                        const double t)
    {
        const int cm = a.d > 32 ? 3 : 0;   // chain of dimension i: i & cm
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
    __device__ __forceinline__ double logprior(const StretchArgs& a) const
    {
        const double sc = a.d > 32 ? (sc0 + sc1) + (sc2 + sc3) : sc0;
        return inb ? a.s.uniform_logp + sc : -INFINITY;
    }
};

// sum of products u_i v_i in the chain shape of the log-prior: one ascending fma chain for d <= 32,
// four chains over i mod 4 combined (s0 + s1) + (s2 + s3) above
struct DotChains {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    __device__ __forceinline__ void add(const int d, const int i, const double u, const double v)
    {
        const int ch = d > 32 ? (i & 3) : 0;   // (wave-uniform)
        s0 = ch == 0 ? fma(u, v, s0) : s0;
        s1 = ch == 1 ? fma(u, v, s1) : s1;
        s2 = ch == 2 ? fma(u, v, s2) : s2;
        s3 = ch == 3 ? fma(u, v, s3) : s3;
    }
    __device__ __forceinline__ double total(const int d) const { return d > 32 ? (s0 + s1) + (s2 + s3) : s0; }
};

template <bool ACCEPT, int KIND>
__global__ void __launch_bounds__(128) ensemble_move_kernel(const EnsembleMoveArgs e)
{
    __shared__ double tiles[2][kFnTileDims * kFnTileStride];
    const StretchArgs& a = e.st;
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
    constexpr bool PROPOSE = KIND >= 0;
    if (ACCEPT) {
        half_accept(a, tile, rows, k, base + a.half_accept * hg, act, lane, nrows);
    }
    if (ACCEPT && PROPOSE) {
        // every commit of this workgroup's groups is visible to its proposals
        __threadfence_block();
        __syncthreads();
    }
    if (PROPOSE) {
        const int w = base + a.half_propose * hg;
        const uint32_t gid = s.walker0 + (uint32_t)w;
        const uint32_t stream = KIND == kEnsembleStretch ? kStreamStretch
                                                         : (KIND == kEnsembleDE ? kStreamDE : kStreamSnooker);
        const uint32_t s_lo = (uint32_t)s.step0, s_hi = (uint32_t)(s.step0 >> 32);
        const u32x4 r4 = philox4x32_10(s.key0, s.key1, gid, stream, s_lo, s_hi);
        const int other = g * s.group_size + (1 - a.half_propose) * hg;   // member 0 of the other half
        const int m0 = (int)(r4.w0 >> (32 - a.log2_half));
        const uint64_t ka = ((uint64_t)r4.w3 << 20) | ((uint64_t)(r4.w2 & 0xFFFu) << 8) | (r4.w0 & 0xFFu);
        const double Ea = -dlog(u52(ka));
        // a second member, distinct from m0 (DE, snooker; the multiply-shift draw of hg - 1 values)
        const int m1 = (m0 + 1 + (int)(((uint64_t)r4.w1 * (uint64_t)(hg - 1)) >> 32)) & (hg - 1);
        const int w0p = other + m0, w1p = other + m1;
        TrialPrior prior;
        double q = 0.0;
        bool whole = true;   // (snooker: false where the walker sits on its partner)
        if (KIND == kEnsembleStretch || KIND == kEnsembleDE) {
            double f;   // stretch: z;  de: gamma
            if (KIND == kEnsembleStretch) {
                const uint64_t kz = ((uint64_t)r4.w1 << 20) | (r4.w2 >> 12);
                const double sz = fma(e.p0 - 1.0, u52(kz), 1.0);
                f = (sz * sz) / e.p0;
                q = a.dm1 * dlog(f);
            } else {
                const u32x4 rb = philox4x32_10(s.key0, s.key1, gid, stream | kStreamSecond, s_lo, s_hi);
                const uint64_t k1 = ((uint64_t)rb.w1 << 20) | (rb.w2 >> 12);
                const uint64_t k2 = ((uint64_t)rb.w3 << 20) | ((uint64_t)(rb.w2 & 0xFFFu) << 8) | (rb.w0 & 0xFFu);
                double sn, cs;
                sincos2pi(k2, sn, cs);
                const double n = sqrt(-2.0 * dlog(u52(k1))) * cs;
                f = e.p0 * fma(e.p1, n, 1.0);
            }
            for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
                const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
                // the tile's part of x and of the partners first, every load in flight at once
                double xs[kFnTileDims], ps[kFnTileDims], p2[kFnTileDims];
#pragma unroll
                for (int c = 0; c < kFnTileDims; ++c)
                    if (c < tw) {
                        xs[c] = s.x[(size_t)(i0 + c) * W + w];
                        ps[c] = s.x[(size_t)(i0 + c) * W + w0p];
                        if (KIND == kEnsembleDE) p2[c] = s.x[(size_t)(i0 + c) * W + w1p];
                    }
#pragma unroll
                for (int c = 0; c < kFnTileDims; ++c) {
                    if (c >= tw) continue;   // (wave-uniform)
                    const double t = KIND == kEnsembleStretch ? fma(f, xs[c] - ps[c], ps[c])
                                                              : fma(f, ps[c] - p2[c], xs[c]);
                    tile[c * kFnTileStride + lane] = t;
                    prior.add(a, C, cl, i0 + c, t);
                }
                __syncthreads();
                st_tile_copy<true>(tile, rows + i0, d, tw, lane, nrows);
                if (i0 + kFnTileDims < d) __syncthreads();   // the tile is reused
            }
        } else {
            // the third member, distinct from both: hg - 2 values, stepped past the smaller and then the larger
            const u32x4 rb = philox4x32_10(s.key0, s.key1, gid, stream | kStreamSecond, s_lo, s_hi);
            int m2 = (int)(((uint64_t)rb.w0 * (uint64_t)(hg - 2)) >> 32);
            const int mlo = m0 < m1 ? m0 : m1, mhi = m0 < m1 ? m1 : m0;
            if (m2 >= mlo) ++m2;
            if (m2 >= mhi) ++m2;
            const int w2p = other + m2;
            double xs[kFnTileDims], zs[kFnTileDims];   // (d <= 32: kept from pass 1 to pass 2)
            DotChains n2c, sc, ntc;
            for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
                const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
                // x and z of the tile first (kept), then the two further partners a quarter tile at a
                // time: all four rows of a whole tile in flight would take every register there is
#pragma unroll
                for (int c = 0; c < kFnTileDims; ++c)
                    if (c < tw) {
                        xs[c] = s.x[(size_t)(i0 + c) * W + w];
                        zs[c] = s.x[(size_t)(i0 + c) * W + w0p];
                    }
#pragma unroll
                for (int c0 = 0; c0 < kFnTileDims; c0 += kFnTileDims / 4) {
                    double dz[kFnTileDims / 4];
#pragma unroll
                    for (int c = 0; c < kFnTileDims / 4; ++c)
                        if (c0 + c < tw)
                            dz[c] = s.x[(size_t)(i0 + c0 + c) * W + w1p] - s.x[(size_t)(i0 + c0 + c) * W + w2p];
#pragma unroll
                    for (int c = 0; c < kFnTileDims / 4; ++c) {
                        if (c0 + c >= tw) continue;   // (wave-uniform)
                        const double dl = xs[c0 + c] - zs[c0 + c];
                        n2c.add(d, i0 + c0 + c, dl, dl);
                        sc.add(d, i0 + c0 + c, dl, dz[c]);
                    }
                }
            }
            const double n2 = n2c.total(d);
            whole = n2 > 0.0;
            const double cf = whole ? (e.p0 * sc.total(d)) / n2 : 0.0;
            for (int i0 = 0; i0 < d; i0 += kFnTileDims) {
                const int tw = (d - i0) < kFnTileDims ? (d - i0) : kFnTileDims;
                if (d > kFnTileDims) {   // (wave-uniform: the registers hold the LAST tile)
#pragma unroll
                    for (int c = 0; c < kFnTileDims; ++c)
                        if (c < tw) {
                            xs[c] = s.x[(size_t)(i0 + c) * W + w];
                            zs[c] = s.x[(size_t)(i0 + c) * W + w0p];
                        }
                }
#pragma unroll
                for (int c = 0; c < kFnTileDims; ++c) {
                    if (c >= tw) continue;   // (wave-uniform)
                    const double t = fma(cf, xs[c] - zs[c], xs[c]);
                    tile[c * kFnTileStride + lane] = t;
                    prior.add(a, C, cl, i0 + c, t);
                    const double tz = t - zs[c];
                    ntc.add(d, i0 + c, tz, tz);
                }
                __syncthreads();
                st_tile_copy<true>(tile, rows + i0, d, tw, lane, nrows);
                if (i0 + kFnTileDims < d) __syncthreads();   // the tile is reused
            }
            const double nt2 = ntc.total(d);
            whole = whole && nt2 > 0.0;
            // a void trial (q = -inf, lp_t = -inf): rejected, and no prior rejection (half_accept)
            q = whole ? a.dm1 * (0.5 * dlog(nt2) - 0.5 * dlog(n2)) : -INFINITY;
        }
        if (act) {
            a.lp_t[k] = whole ? prior.logprior(a) : -INFINITY;
            a.Ea[k] = Ea;
            a.q[k] = q;
        }
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_ensemble_move(const mcmc::EnsembleMoveArgs* e, int accept,
                                                    int propose_kind, hipStream_t st)
{
    using namespace mcmc;
    const StretchArgs* a = &e->st;
    const int gs = a->s.group_size, hg = gs / 2;
    const bool propose = propose_kind >= 0;
    if (a->d < 1 || a->d > 128 || (gs != 64 && gs != 128 && gs != 256) || a->s.W <= 0 || a->s.W % gs != 0 ||
        (1 << a->log2_half) != hg || (accept && (a->half_accept | 1) != 1) ||
        (propose && (a->half_propose | 1) != 1) || (accept && propose && a->half_accept == a->half_propose) ||
        propose_kind > kEnsembleSnooker || (propose && propose_kind != e->kind) || (!accept && !propose))
        return hipErrorInvalidValue;
    // a workgroup owns whole groups: two of 64 walkers, or one of 128 or 256
    const int block = hg < 64 ? 64 : hg;
    const int n_act = a->s.W / 2;
    const dim3 g((n_act + block - 1) / block), b(block);
    mcmc_hip_note_step_kernel("mcmc::ensemble_move_kernel");
#define LAUNCH(ACC, KIND) hipLaunchKernelGGL((ensemble_move_kernel<ACC, KIND>), g, b, 0, st, *e)
    switch (propose_kind) {
    case kEnsembleStretch: if (accept) LAUNCH(true, kEnsembleStretch); else LAUNCH(false, kEnsembleStretch); break;
    case kEnsembleDE: if (accept) LAUNCH(true, kEnsembleDE); else LAUNCH(false, kEnsembleDE); break;
    case kEnsembleSnooker: if (accept) LAUNCH(true, kEnsembleSnooker); else LAUNCH(false, kEnsembleSnooker); break;
    default: LAUNCH(true, -1); break;
    }
#undef LAUNCH
    return hipGetLastError();
}
