// mcmc_hip -- INCREMENTAL EVALUATION of mixtures, TWO lanes per walker (round 6; gfx950 only).
//
// The same step as step_inc_mix_kernel (incremental_kernels.hip) -- the same arithmetic bit for bit,
// specification: oracle/mcmc_oracle.c step_core_inc with `carries_modes` -- in another layout.
// step_inc_mix_kernel gives a walker FOUR lanes (lane class c holds the dimensions i = 4 kk + c): 16
// walkers per wave, and everything that is not a sum over the dimensions -- the log-sum-exp
// (gaussian_mixture.py:158-163) with its exponential and logarithm, the accept test, the selects of
// the carried values, the bookkeeping of weight / rejections / burn-in, the fetch of the variates --
// is executed once per LANE, four times per walker: ~120 of the ~175 vector instructions of a
// wave-step at d = 30, K = 2.  Its state (dq (K + 1) doubles per lane beside a ~100-register body)
// holds it to three waves per SIMD -- 65 536 walkers are four: a second round of a quarter of the
// workgroups at one wave per SIMD --, and the SIMDs wait 38 % of their cycles
// (profiles/r05_variant_counters.txt).
// Here a walker has TWO lanes: lane half h = lane & 1 holds the dimensions i = 4 kk + 2 h + j,
// j = 0, 1 -- two of the specification's four interleaved chains --, a wave serves 32 walkers, and the
// per-lane work is done twice per walker.  The sums over the dimensions stay the specification's
// (p0 + p1) + (p2 + p3): a lane adds its own two chains, one DPP swap adds the neighbour's.  The
// planes (v, u_1 .. u_K) of a column give a lane the operands of both its chains in ONE ds_read_b128.
// 65 536 walkers are 2 048 waves of this layout: two per SIMD in one round, 256 registers each --
// which hold x and y_1, y_2 of a two-mode walker at d <= 32; with three modes above d = 24 and four above d = 20 x
// moves to LDS (XLDS below) and the registers hold y_1 .. y_K: two modes up to d = 48, three up to d = 32,
// four up to d = 24 (kernels.h: duo_serves, duo_x_in_lds).
//
// Measured (same box, 65 536 walkers, tools/mix_bench.py; step kernel ms per 40 d steps, four lanes ->
// two; profiles/r06_duo.txt): d = 30: K = 2 2.907 -> 1.855 (2.71 -> 4.24e10 evals/s), K = 3 3.568 -> 2.815;
// d = 24: K = 2 1.978 -> 1.250, K = 3 2.605 -> 1.527, K = 4 2.882 -> 2.222; d = 16: K = 3 1.359 -> 1.054,
// K = 4 1.563 -> 1.019; two modes above d = 32 (x in LDS): d = 36 3.66 -> 3.04, d = 40 4.38 -> 3.47, d = 48 5.66 -> 4.99.
// Four modes at d = 30 do not fit (y_1 .. y_4 alone are 128 registers: with x in
// registers as well the step loop spilled, 4.07 -> 19.9 ms) and stay on step_inc_mix_kernel.
//
// ONE mode (round 7, step_inc_duo_kernel below, reported as step_inc_kernel<dq, 0, .., two lanes>):
// the four-lane kernel is issue-bound, and about a third of its vector instructions are per walker and
// run in all four lanes; on two lanes they run twice, and with the chains {h, h + 2} in lane h a
// d = 30 walker has 15 dimensions per lane and no padded row.  The step's (v, u) pairs stay in registers
// from the trial to the commit (256 registers at two waves per SIMD).  Measured at d = 30, 65 536
// walkers, same box (profiles/r07_one_mode_two_lanes.txt): step kernel 1.11 -> 0.99 ms per 1 200
// steps (bench.py: 0.902 -> 0.856), 20 % fewer vector instructions; chains {2 h, 2 h + 1} (16 rows,
// two padded) 4 % slower than {h, h + 2}; the next step's pairs requested a step ahead 22 % slower.
// Below 65 536 walkers the four-lane kernel is as fast or faster (inc_choice.h: kDuo1MinWalkers).
// The accept variate of the one-mode kernel is lazily exact (round 12; det_math.h: PairRng::run_lazy, accept_lanes):
// the burst stages a single-precision estimate of Ea and its 28-bit integer, the step takes the exact logarithm only
// for a wave with a lane within 2^-14 of delta.  Measured (profiles/r12_lazy_accept.txt, same box, parent / new
// alternated four times): step kernel 0.8579 -> 0.8387 ms (-2.2 %), bench.py 8.483e10 -> 8.664e10 (+2.1 %; the
// parent's spread was 0.59 %); 3.2 % fewer vector instructions per launch.  With the certain path laid over two
// taken branches the same instructions gained 0.4 %.  step_duo_mix_kernel keeps the exact staging: at K = 2 the
// lazy form measured 1.881 -> 1.850 ms per 1 200 steps, inside three times the parent's spread (1.2 %).
// The commit of the one-mode kernel runs under the accept mask (round 20): an accepting lane takes the step's trial as its
// x (15 v_mov_b64 at d = 30, not 15 FMAs with a selected r) and moves y on with r, a rejecting lane is not touched; the
// test of the limit of tries leaves the step of a wave whose chains cannot pass it within the chunk.  v_mov_b64 issues in
// one pass at the rate of v_add_f64 (4.6 clocks at two waves per SIMD, v_fma_f64 5.6; tools/probes/valu_op_cost.hip).  Measured
// (profiles/r20_masked_commit.txt, same box, parent / new alternated four times): step kernel 0.7416 -> 0.7033 ms (-5.2 %;
// the masked commit alone -1.8 %, the stuck test a further -3.5 %), bench.py 9.845e10 -> 1.0337e11 (+5.0 %; the parent's
// spread was 0.73 %); 6.9 fewer vector instructions per wave-step.
//
// Served: Metropolis steps, no periodic parameter, no emitted rows, no block of one parameter, whole
// workgroups of 128 walkers inside one basis group -- for ensembles that fill the chip with it
// (inc_choice.h: kDuoMinWalkers); smaller ensembles keep the four-lane kernel, whose twice as many
// waves cover their latencies better.
#include <string>

#include "incremental_common.h"

#ifndef MCMC_DUO_DEPK
#define MCMC_DUO_DEPK(tuned) (tuned)   // (experiment hooks: _exp/inc_experiment.h)
#endif
#ifndef MCMC_DUO_KEEPV
#define MCMC_DUO_KEEPV(tuned) (tuned)
#endif
// the staging DMA of step_inc_duo_kernel where the compiler does not count it (incremental_common.h: stage16_dma;
// measured: profiles/r14_lds_wait_ladder.txt; step_duo_mix_kernel was measured with it at K = 2 and keeps the builtin)
#ifndef MCMC_DUO1_DMA_HIDDEN
#define MCMC_DUO1_DMA_HIDDEN 1
#endif
// |u|^2 of a chunk's columns staged into LDS with the chunk (1) or read by a scalar load inside the step (0)
// (measured: profiles/r17_step_path.txt)
#ifndef MCMC_DUO1_UU_LDS
#define MCMC_DUO1_UU_LDS 1
#endif
#ifndef MCMC_DUO1_LADDER
#define MCMC_DUO1_LADDER 4   // (pairs per counted LDS wait of the one-mode step, >= 1: see its step loop)
#endif
// the variate burst of step_inc_duo_kernel: one straight-line burst of interleaved chains per octet (1: det_math.h
// OctetRng) or a rolled loop over the lane half's two Philox blocks (0: PairRng, what step_duo_mix_kernel keeps)
// (measured: profiles/r25_burst_chains.txt)
#ifndef MCMC_DUO1_BURST_CHAINS
#define MCMC_DUO1_BURST_CHAINS 1
#endif
// measurement hook: every octet's variates are drawn this many times into the same LDS slots (the outputs do not
// change); the difference between 2 and 1 is what one burst costs.  The shipped build draws once
#ifndef MCMC_DUO1_BURST_REPEAT
#define MCMC_DUO1_BURST_REPEAT 1
#endif

namespace mcmc {
namespace {

// the neighbour lane's value (lane ^ 1)
__device__ __forceinline__ double pair_swap(double v) { return quad_perm<0xB1>(v); }
// (p0 + p1) + (p2 + p3): s = this lane's two chains added, the neighbour holds the other two
__device__ __forceinline__ double duo_sum(double p_even, double p_odd)
{
    const double s = p_even + p_odd;
    return s + pair_swap(s);
}
__device__ __forceinline__ unsigned pair_max_u32(unsigned v)
{
    const unsigned o = (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);
    return v > o ? v : o;
}
// lane mask -> the mask of the lanes whose PAIR is held completely
__device__ __forceinline__ unsigned long long pair_all_mask(unsigned long long m)
{
    m &= m >> 1;
    m &= 0x5555555555555555ull;
    return m * 3ull;
}

// The (r, Ea) variates of an octet of steps (StagedVariates of incremental_common.h for 32 walkers
// per wave): lane half h draws the Philox blocks of the step pairs 4 * octet + 2 h and + 2 h + 1
// and leaves their four pairs in sRE[wave][step of the octet][walker of the wave].  Row stride 33
// pairs = 528 bytes: the eight lanes a ds_write_b128 serves together (four walkers x two halves)
// then cover the 128-byte bank window once (the halves' rows are 4 x 528 = 64 bytes apart mod 128).
constexpr int kDuoRow = 33;
constexpr int kDuoStagedPairs = 4 * 8 * kDuoRow;   // 16.5 KB per workgroup of four waves
struct DuoVariates {
    unsigned base, off;
    __device__ __forceinline__ void init(const pair_t* sRE, int wave, int lane)
    {
        base = lds_offset(sRE + (wave * 8 * kDuoRow + (lane >> 1)));
        off = base;
    }
    // the two pairs of the step pair 4 * octet + 2 h + q (q = 0, 1), as soon as they are drawn
    // (step_inc_duo_kernel draws with PairRng::run_lazy: the second half of a pair is then accept_pack(ka), what
    // accept_lanes takes; step_duo_mix_kernel keeps the exact Ea of PairRng::run)
    __device__ __forceinline__ void put(pair_t* sRE, int wave, int lane, int h, int q, const PairRng& p)
    {
        pair_t* const mine = sRE + ((wave * 8 + 4 * h + 2 * q) * kDuoRow + (lane >> 1));
        mine[0] = pair_t{p.r[0], p.Ea[0]};
        mine[kDuoRow] = pair_t{p.r[1], p.Ea[1]};
    }
    // ... and the four of an octet's lane half at once (the same slots)
    __device__ __forceinline__ void put(pair_t* sRE, int wave, int lane, int h, const OctetRng& p)
    {
        pair_t* const mine = sRE + ((wave * 8 + 4 * h) * kDuoRow + (lane >> 1));
#pragma unroll
        for (int v = 0; v < 4; ++v) mine[v * kDuoRow] = pair_t{p.r[v], p.Ea[v]};
    }
    __device__ __forceinline__ void seek(unsigned long long S) { off = base + (unsigned)(S & 7ull) * (16u * kDuoRow); }
    __device__ __forceinline__ void fetch(double& r, double& Ea) const
    {
        const pair_t re = *(lds_pairs)(unsigned long long)off;
        r = re.x;
        Ea = re.y;
    }
    __device__ __forceinline__ void next() { off += 16u * kDuoRow; }
};

// ---------------------------------------------------------------- mixtures
// The log-sum-exp (gaussian_mixture.py:158-163; mixture_lse of the oracle): lane half h takes the
// exponential of mode h and of mode h + 2, pair broadcasts hand them to the neighbour, the weighted sum runs in
// the order of the specification.
// columns of one LDS chunk (a multiple of 4): two workgroups per CU have 80 KB each -- what the staged
// variates (16.5 KB), the tables (2.5 KB), the bounds (2 KB) and, where x lives in LDS (duo_x_in_lds,
// kernels.h), its 128 dq bytes per walker leave, for two buffers of planes
__host__ __device__ constexpr int duo_chunk_mix(int dq, int km)
{
    const int avail = 80 * 1024 - 16896 - 2560 - 2048 - (duo_x_in_lds(km, dq) ? dq * 4096 : 0);
    int c = ((avail / 16) / ((1 + km) * 4 * dq)) & ~3;
    return c < 4 ? 4 : (c > 64 ? 64 : c);
}
// the v plane of a step kept in registers from the trial to the commit where the registers hold it
// beside the state: up to 64 doubles of state + plane per lane (measured at d = 30, K = 2: 1.93 -> 1.83 ms
// per 1200 steps)
__host__ __device__ constexpr bool duo_keep_v(int dq, int km)
{
    return 2 * dq * (km + (duo_x_in_lds(km, dq) ? 0 : 1)) + 2 * dq <= 64;
}

template <int DQ, int KM, bool UNIT_T, bool BOX0>
__global__ void __launch_bounds__(256, 2) step_duo_mix_kernel(const IncStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int dpad = 4 * DQ;
    constexpr int NE = 2 * DQ;                    // dimensions per lane: e = 2 kk + j <-> i = 4 kk + 2 h + j
    constexpr int COL = (1 + KM) * dpad;          // doubles per column
    constexpr int C = duo_chunk_mix(DQ, KM);
    constexpr int CHUNK = C * COL;
    // the element of a plane whose result the next plane's reads wait for (measured at d = 30, K = 2:
    // first, middle and last element within 1 %)
    constexpr int DEPK = MCMC_DUO_DEPK(DQ / 2);
    // XLDS (two modes from d = 33 on, three from d = 25 on, four from d = 21 on): x lives in LDS, [kk][lane] pairs
    // (x_even, x_odd) -- 16 reads and 8 writes of 16 bytes per lane and step --, so that the registers
    // hold y_1 .. y_KM as they hold x, y_1, y_2 of a two-mode walker (with x in registers too three
    // modes spilled ~45 doubles inside the step loop: 7.6 ms per 1200 steps at d = 30 against
    // step_inc_mix_kernel's 3.5; with x in LDS 2.8)
    constexpr bool XLDS = duo_x_in_lds(KM, DQ);
    constexpr bool KEEPV = MCMC_DUO_KEEPV(duo_keep_v(DQ, KM));
    const StepArgs& s = a.s;
    const int tid = threadIdx.x, h = tid & 1, wave = tid >> 6, lane = tid & 63;
    const int W = s.W, d = a.d;
    const int w = blockIdx.x * 128 + (tid >> 1);
    const int g = __builtin_amdgcn_readfirstlane(w / s.group_size);
    const int ncols = s.n_steps;
    const double* __restrict__ gVU = a.VU + (size_t)g * ncols * COL;
    auto stage = [&](int k) {   // (written out in every kernel: incremental_common.h, "around the step loop")
        const int first = k * C;
        if (first >= ncols) return;
        const int cols = ncols - first < C ? ncols - first : C;
        const int bytes = cols * COL * 8;
        const char* src = (const char*)(gVU + (size_t)first * COL);
        char* dst = (char*)(smem + (k & 1) * CHUNK);
        for (int kb = wave; kb * 1024 < bytes; kb += 4) {
            if (kb * 1024 + lane * 16 < bytes)
                stage16_dma<false>(dst + kb * 1024, src + kb * 1024 + lane * 16);
        }
    };
    stage(0);
    // BOX0: every prior uniform on the same [0, hi]; else per-parameter bounds and normal priors
    __shared__ double2 sLH[BOX0 ? 1 : 4 * DQ];     // the bounds as (lo, hi) pairs
    __shared__ double2 sNA[BOX0 ? 1 : 4 * DQ];     // normal priors: (loc, 1/scale) and -log(scale sqrt(2 pi))
    __shared__ double sNM[BOX0 ? 1 : 4 * DQ];
    if (!BOX0)
        for (int i = tid; i < dpad; i += 256) {
            sLH[i] = make_double2(a.prior[i], a.prior[dpad + i]);
            sNA[i] = make_double2(a.prior[2 * dpad + i], a.prior[3 * dpad + i]);
            sNM[i] = a.prior[4 * dpad + i];
        }
    double x[XLDS ? 1 : NE], y[KM][NE];
    typedef pair_t __attribute__((address_space(3))) * lds_pairs_rw;
    __shared__ pair_t sX[XLDS ? DQ * 256 : 1];
    const unsigned xoff0 = lds_offset(sX + tid);
#pragma unroll
    for (int kk = 0; kk < DQ; ++kk) {
        double xe[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = 2 * kk + j, i = 4 * kk + 2 * h + j;
            const bool in = i < d;
            // (one box for all dimensions: a padded dimension rests at its middle, inside for every step)
            xe[j] = in ? s.x[(size_t)i * W + w] : (BOX0 ? 0.5 * a.box_hi : 0.0);
            if (!XLDS) x[XLDS ? 0 : e] = xe[j];
#pragma unroll
            for (int k = 0; k < KM; ++k) y[k][e] = in ? a.y[((size_t)k * d + i) * W + w] : 0.0;
        }
        if (XLDS) sX[kk * 256 + tid] = pair_t{xe[0], xe[1]};
    }
    double cn[KM], wk[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) { cn[k] = s.cblock[a.cnorm_off + k]; wk[k] = s.cblock[a.weight_off + k]; }
    double lpost = s.logpost[w], lpri = s.logprior[w], llik = s.loglike[w];
    int wt = s.weight[w], prej = s.prior_rej[w], burn = s.burn_left[w];
    const long long nacc0 = s.n_accept[w];
    int nacc = 0;
    const uint32_t gid = s.walker0 + (uint32_t)w;
    const TryLimits tl = try_limits(s.max_tries);
    __shared__ dpair_t short_log_lds[SHORT_LOG_TABLE_SIZE];
    const short_log_tab slog = short_log_load(short_log_lds);
    __shared__ double exp64_lds[64];   // 2^(j / 64): the log-sum-exp's table-driven exponential
    const exp_tab etab = exp_tab_load(exp64_lds);
    dma_wait();   // chunk 0 has landed
    __syncthreads();
    const unsigned long long half1 = 0xAAAAAAAAAAAAAAAAull;   // the lanes with h = 1
    auto lse = [&](const double (&ak)[KM]) {
        double amax = ak[0];
#pragma unroll
        for (int k = 1; k < KM; ++k) amax = fmax(ak[k], amax);
        const double mine = sel(half1, ak[1], ak[0]);
        const double e_mine = dexp_tab(mine - amax, etab);
        double Ssum = fma(wk[0], quad_perm<0xA0>(e_mine), 0.0);    // [0,0,2,2]: the pair's h = 0 lane
        Ssum = fma(wk[1], quad_perm<0xF5>(e_mine), Ssum);          // [1,1,3,3]: its h = 1 lane
        if (KM > 2) {   // modes 2, 3: a second exponential per lane
            const double mine2 = KM > 3 ? sel(half1, ak[3 < KM ? 3 : 0], ak[2 < KM ? 2 : 0]) : ak[2 < KM ? 2 : 0];
            const double e2 = dexp_tab(mine2 - amax, etab);
            Ssum = fma(wk[2 < KM ? 2 : 0], quad_perm<0xA0>(e2), Ssum);
            if (KM > 3) Ssum = fma(wk[3 < KM ? 3 : 0], quad_perm<0xF5>(e2), Ssum);
        }
        return dlog_tab(Ssum, slog) + amax;
    };
    // the carried log-density of every mode (the same value in both lanes of a walker)
    double am[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) am[k] = a.amode[(size_t)k * W + w];
    if (a.anchor) {   // (wave-uniform) y has just been refreshed from x: orc_anchor_modes
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            double pa0 = 0.0, pa1 = 0.0;
#pragma unroll
            for (int kk = 0; kk < DQ; ++kk) {
                pa0 = fma(y[k][2 * kk], y[k][2 * kk], pa0);
                pa1 = fma(y[k][2 * kk + 1], y[k][2 * kk + 1], pa1);
            }
            am[k] = anchored_logpdf(cn[k], duo_sum(pa0, pa1));
        }
        llik = lse(am);
        lpost = lpri + llik;
    }
    const cdoubles gUU = (cdoubles)(unsigned long long)(a.UU + (size_t)g * ncols * KM);
    // (the box [0, hi]: the support test on the high words of the trial coordinates, as in
    // step_inc_mix_kernel)
    const unsigned bhi_word = (unsigned)__double2hiint(a.box_hi);
    const int hw_slot = hw_wave_slot();
    bool burning = lanes(burn > 0) != 0ull;   // wave-uniform
    unsigned long long cur_oct = ~0ull;
    __shared__ pair_t sRE[kDuoStagedPairs];
    DuoVariates sv;
    sv.init(sRE, wave, lane);

    for (int base = 0, kc = 0; base < ncols; base += C, ++kc) {
        const double* __restrict__ cur = smem + (kc & 1) * CHUNK;
        stage(kc + 1);
        const int cols = __builtin_amdgcn_readfirstlane(ncols - base < C ? ncols - base : C);
        unsigned coff = lds_offset(cur + 2 * h);
#pragma unroll 1
        for (int sl = 0; sl < cols; ++sl, coff += COL * 8) {
            const unsigned long long S = s.step0 + (unsigned long long)(base + sl);
            if ((S >> 3) != cur_oct) {   // wave-uniform: every eighth step
                cur_oct = S >> 3;
                rotate_priority<2>(hw_slot);
#pragma unroll 1
                for (int q = 0; q < 2; ++q) {   // (rolled: one Philox block's registers at a time)
                    PairRng pr;
                    pr.run(s.key0, s.key1, gid, (cur_oct << 2) + (unsigned long long)(2 * h + q), slog);
                    sv.put(sRE, wave, lane, h, q, pr);
                }
                sv.seek(S);
            }
            double r, Ea;
            sv.fetch(r, Ea);
            sv.next();
            const lds_pairs col = (lds_pairs)(unsigned long long)coff;   // plane v: [2 kk] = (v_even, v_odd)
            unsigned long long inb = ~0ull;
            double sc0 = 0.0, sc1 = 0.0;
            double dep;   // what the next plane's reads are ordered behind
            pair_t vk[KEEPV ? DQ : 1];
            // (XLDS: the offset of the walker's x passes through an empty asm at every use -- an
            // address the compiler takes as new: nothing is promoted back to registers, and the
            // reads stay behind the writes of the step before)
            unsigned xo = xoff0;
            if (XLDS) asm volatile("" : "+v"(xo));
            const lds_pairs xs = (lds_pairs)(unsigned long long)xo;
            auto xpair = [&](int kk) {
                if constexpr (XLDS) return xs[kk * 256];
                else return pair_t{x[2 * kk], x[2 * kk + 1]};
            };
            if constexpr (BOX0) {
                unsigned hmx = 0u;
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    const pair_t v = col[2 * kk];
                    const pair_t xp = xpair(kk);
                    if (KEEPV) vk[kk] = v;
                    if (kk == DEPK) dep = fma(r, v.x, xp.x);
                    const unsigned h0 = (unsigned)__double2hiint(fma(r, v.x, xp.x));
                    const unsigned h1 = (unsigned)__double2hiint(fma(r, v.y, xp.y));
                    hmx = hmx > h0 ? hmx : h0;
                    hmx = hmx > h1 ? hmx : h1;
                }
                inb = lanes(pair_max_u32(hmx) < bhi_word);
                if (inb != lanes(true)) {   // (wave-uniform, rare) the exact comparisons
                    unsigned xoff = coff;
                    asm volatile("" : "+v"(xoff));
                    const lds_pairs colx = (lds_pairs)(unsigned long long)xoff;
                    inb = ~0ull;
#pragma unroll
                    for (int kk = 0; kk < DQ; ++kk) {
                        const pair_t v = colx[2 * kk];
                        const pair_t xp = xpair(kk);
                        const double t0 = fma(r, v.x, xp.x), t1 = fma(r, v.y, xp.y);
                        inb &= lanes(t0 <= a.box_hi) & lanes(t0 >= 0.0);
                        inb &= lanes(t1 <= a.box_hi) & lanes(t1 >= 0.0);
                    }
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    const pair_t v = col[2 * kk];
                    const pair_t xp = xpair(kk);
                    if (KEEPV) vk[kk] = v;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int i = 4 * kk + 2 * h + j;
                        const double t = fma(r, j ? v.y : v.x, j ? xp.y : xp.x);
                        if (kk == DEPK && j == 0) dep = t;
                        const double2 lh = sLH[i];
                        inb &= lanes(t <= lh.y) & lanes(t >= lh.x);
                        if (a.has_norm) {   // wave-uniform; branch-free inside (1/scale = 0: no term)
                            const double2 li = sNA[i];
                            const double qq = (t - li.x) * li.y;
                            if (j) sc1 = sc1 + fma(-0.5 * qq, qq, sNM[i]);
                            else sc0 = sc0 + fma(-0.5 * qq, qq, sNM[i]);
                        }
                    }
                }
            }
            // (the reads of a plane are ordered behind the MIDDLE result of the plane before -- half
            // of its arithmetic covers these reads' latency --: issued all up
            // front, the (1 + KM) NE operands of a step do not fit beside the (1 + KM) NE of state)
            double ak[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                unsigned uoff = coff + (unsigned)((1 + k) * dpad * 8);
                asm volatile("" : "+v"(uoff) : "v"(dep));
                const lds_pairs uk = (lds_pairs)(unsigned long long)uoff;
                double pc0 = 0.0, pc1 = 0.0;
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {   // y_k . u_k
                    const pair_t u = uk[2 * kk];
                    pc0 = fma(y[k][2 * kk], u.x, pc0);
                    pc1 = fma(y[k][2 * kk + 1], u.y, pc1);
                    if (kk == DEPK) dep = pc0;
                }
                const double yu = duo_sum(pc0, pc1);
                const double uu = gUU[(size_t)(base + sl) * KM + k];   // (a scalar load)
                ak[k] = fma(-0.5 * r, fma(r, uu, yu + yu), am[k]);
            }
            const unsigned long long inside_m = pair_all_mask(inb);
            const double lp = s.uniform_logp + ((!BOX0 && a.has_norm) ? duo_sum(sc0, sc1) : 0.0);
            const double ll = lse(ak);
            const double lt = lp + ll;   // (finite: the sum of the weights' terms is >= w_max)
            const double delta = UNIT_T ? (lpost - lt) : (lpost - lt) / s.temperature;
            const unsigned long long acc_m = inside_m & (lanes(lt > lpost) | lanes(Ea > delta));
            const bool accept = __builtin_amdgcn_inverse_ballot_w64(acc_m);
            int lim = tl.lim1;
            if (burning) {   // wave-uniform (see step_inc_kernel)
                lim = tl.of(burn);
                burn -= (accept & (burn > 0)) ? 1 : 0;
                burning = lanes(burn > 0) != 0ull;
            }
            const double ra = sel(acc_m, r, 0.0);
            // the commit reads the planes AGAIN (x, then y_1 .. y_KM): the pointer passes through
            // an empty asm behind the accept decision, nothing is kept from the trial
            if constexpr (XLDS) {
                unsigned xw = xoff0, poff = coff;
                asm volatile("" : "+v"(xw), "+v"(poff) : "v"(ra));
                const lds_pairs_rw px = (lds_pairs_rw)(unsigned long long)xw;
                const lds_pairs pv = (lds_pairs)(unsigned long long)poff;
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    pair_t xp = px[kk * 256];
                    pair_t v;
                    if constexpr (KEEPV) v = vk[kk];
                    else v = pv[2 * kk];
                    xp.x = fma(ra, v.x, xp.x);
                    xp.y = fma(ra, v.y, xp.y);
                    px[kk * 256] = xp;
                }
            } else if constexpr (KEEPV) {
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    x[2 * kk] = fma(ra, vk[kk].x, x[2 * kk]);
                    x[2 * kk + 1] = fma(ra, vk[kk].y, x[2 * kk + 1]);
                }
            } else {
                unsigned poff = coff;
                asm volatile("" : "+v"(poff) : "v"(ra));
                const lds_pairs pv = (lds_pairs)(unsigned long long)poff;
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    const pair_t v = pv[2 * kk];
                    x[2 * kk] = fma(ra, v.x, x[2 * kk]);
                    x[2 * kk + 1] = fma(ra, v.y, x[2 * kk + 1]);
                }
            }
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                unsigned poff = coff + (unsigned)((1 + k) * dpad * 8);
                // (behind the middle result of the plane before, as in the trial)
                asm volatile("" : "+v"(poff) : "v"(k == 0 ? ((KEEPV || XLDS) ? ra : x[XLDS ? 0 : 2 * DEPK]) : y[k > 0 ? k - 1 : 0][2 * DEPK]));
                const lds_pairs pu = (lds_pairs)(unsigned long long)poff;
#pragma unroll
                for (int kk = 0; kk < DQ; ++kk) {
                    const pair_t u = pu[2 * kk];
                    y[k][2 * kk] = fma(ra, u.x, y[k][2 * kk]);
                    y[k][2 * kk + 1] = fma(ra, u.y, y[k][2 * kk + 1]);
                }
            }
#pragma unroll
            for (int k = 0; k < KM; ++k) am[k] = sel(acc_m, ak[k], am[k]);
            lpri = sel(acc_m, lp, lpri);
            llik = sel(acc_m, ll, llik);
            lpost = sel(acc_m, lt, lpost);
            prej = sel(acc_m, 0, prej + sel(inside_m, 0, 1));
            wt = sel(acc_m, 1, wt + 1);
            nacc += sel(acc_m, 1, 0);
            if (wt - prej > lim && h == 0) report_stuck(s.stuck, gid);
        }
        dma_wait();   // the next chunk has landed
        __syncthreads();
    }
    // (the walker index passes through an empty asm: the addresses of the stores below are then
    // formed HERE -- else the compiler keeps the addresses of the prologue's (1 + KM) NE loads alive
    // through the whole step loop to reuse them, two registers each)
    int we = w, he = h;
    unsigned xe_off = xoff0;
    asm volatile("" : "+v"(we), "+v"(he), "+v"(xe_off));
    const lds_pairs xend = (lds_pairs)(unsigned long long)xe_off;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = 4 * (e >> 1) + 2 * he + (e & 1);
        if (i < d) {
            double xv;
            if constexpr (XLDS) { const pair_t xp = xend[(e >> 1) * 256]; xv = (e & 1) ? xp.y : xp.x; }
            else xv = x[XLDS ? 0 : e];
            s.x[(size_t)i * W + we] = xv;
#pragma unroll
            for (int k = 0; k < KM; ++k) a.y[((size_t)k * d + i) * W + we] = y[k][e];
        }
    }
    if (h == 0) {
#pragma unroll
        for (int k = 0; k < KM; ++k) a.amode[(size_t)k * W + we] = am[k];
        s.logpost[we] = lpost; s.logprior[we] = lpri; s.loglike[we] = llik;
        s.weight[we] = wt; s.prior_rej[we] = prej; s.burn_left[we] = burn;
        s.n_accept[we] = nacc0 + nacc;
    }
    wave_add_accepts(s.accept_total, (h == 0) ? nacc : 0);
}

template <int DQ, int KM>
hipError_t launch_duo_mix(const IncStepArgs& a, hipStream_t st)
{
    constexpr int C = duo_chunk_mix(DQ, KM);
    const size_t lds = sizeof(double) * 2 * C * (1 + KM) * 4 * DQ;
    const bool unit_t = a.s.temperature == 1.0;
    typedef void (*kern_t)(const IncStepArgs);
    const bool box0 = a.box && a.box_lo == 0.0 && a.box_hi > 0.0 && a.box_hi < INFINITY;
    static const kern_t kerns[4] = {
        step_duo_mix_kernel<DQ, KM, false, false>, step_duo_mix_kernel<DQ, KM, true, false>,
        step_duo_mix_kernel<DQ, KM, false, true>, step_duo_mix_kernel<DQ, KM, true, true>};
    const std::string stem = "mcmc::step_duo_mix_kernel<" + std::to_string(DQ) + ", " + std::to_string(KM);
    static const std::string names[4] = {stem + ", false>", stem + ", true>", stem + ", false, box>",
                                         stem + ", true, box>"};
    const int v = (unit_t ? 1 : 0) + (box0 ? 2 : 0);
    if (lds > 40 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kerns[v],
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    mcmc_hip_note_step_kernel(names[v].c_str());
    hipLaunchKernelGGL(kerns[v], dim3(a.s.W / 128), dim3(256), lds, st, a);
    return hipGetLastError();
}

template <int DQ>
hipError_t dispatch_duo_mix(const IncStepArgs& a, hipStream_t st)
{
    if constexpr (DQ > MCMC_DUO_DQ_HI) {
        return hipErrorInvalidValue;
    } else {
        if (a.dq == DQ) {
            if (!duo_serves(a.n_modes, DQ)) return hipErrorInvalidValue;
            if constexpr (duo_serves(4, DQ)) {
                if (a.n_modes == 4) return launch_duo_mix<DQ, 4>(a, st);
            }
            if constexpr (duo_serves(3, DQ)) {
                if (a.n_modes == 3) return launch_duo_mix<DQ, 3>(a, st);
            }
            return a.n_modes == 2 ? launch_duo_mix<DQ, 2>(a, st) : hipErrorInvalidValue;
        }
        return dispatch_duo_mix<DQ + 1>(a, st);
    }
}

#if MCMC_DUO_DQ_LO == 1
// ---------------------------------------------------------------- one mode
// step_inc_kernel's MODE 0 step (one Gaussian mode, the box [0, hi] for every dimension; specification:
// oracle/mcmc_oracle.c step_core_inc with `carry`) with TWO lanes per walker.  The columns are
// step_inc_kernel's: (v_i, u_i) pairs, pair i at 16 i bytes.  Lane half h holds the NE dimensions
// i = duo1_dim(e, h) of two of the four interleaved chains -- element e belongs to the lane's chain e & 1:
//   SPLIT = false: chains {2 h, 2 h + 1}, i = 4 (e / 2) + 2 h + (e & 1), NE = 2 dq (d = 30: two padded rows in lane 1)
//   SPLIT = true:  chains {h, h + 2},     i = 2 e + h,                   NE = ceil(d / 2) (d = 30: no padded row)
// The sums over the dimensions stay (p0 + p1) + (p2 + p3): with SPLIT = false a lane adds its own two chains
// and one pair swap adds the neighbour's; with SPLIT = true two swaps give p0 + p1 and p2 + p3 in both lanes.
#ifndef MCMC_DUO1_SPLIT
#define MCMC_DUO1_SPLIT 1   // (experiment hook: the chain assignment; measured, profiles/r07_one_mode_two_lanes.txt)
#endif
template <bool SPLIT>
__host__ __device__ constexpr int duo1_off(int e) { return SPLIT ? 2 * e : 4 * (e >> 1) + (e & 1); }
template <bool SPLIT>
__device__ __forceinline__ int duo1_dim(int e, int h) { return duo1_off<SPLIT>(e) + (SPLIT ? h : 2 * h); }
// (p0 + p1) + (p2 + p3) in both lanes of the walker from this lane's chains (q0, q1)
template <bool SPLIT>
__device__ __forceinline__ double duo1_sum(double q0, double q1)
{
    if constexpr (SPLIT) {   // q0 = p_h, q1 = p_(h + 2)
        const double lo = q0 + pair_swap(q0), hi = q1 + pair_swap(q1);
        return lo + hi;
    } else {
        return duo_sum(q0, q1);
    }
}
// columns of one LDS chunk: two workgroups per CU have 80 KB each -- what the staged variates (16.5 KB)
// and the logarithm table (2 KB) leave for two buffers of 64 dq bytes per column
__host__ __device__ constexpr int duo1_chunk(int dq)
{
    int c = ((80 * 1024 - 16896 - 2048) / (2 * 64 * dq)) & ~3;
    return c > 64 ? 64 : c;
}
// the dynamic LDS of step_inc_duo_kernel: two buffers of pairs and, behind them, two of the columns' |u|^2
__host__ __device__ constexpr size_t duo1_lds(int dq)
{
    return (size_t)2 * duo1_chunk(dq) * (64 * dq + (MCMC_DUO1_UU_LDS != 0 ? 8 : 0));
}

template <int DQ, int NE, bool SPLIT, bool UNIT_T>
__global__ void __launch_bounds__(256, 2) step_inc_duo_kernel(const IncStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 smem2[];
    constexpr int COLB = 4 * DQ, dpad = 4 * DQ;  // (v, u) pairs per column
    constexpr int C = duo1_chunk(DQ);
    constexpr int CHUNK = C * COLB;              // pairs per chunk
    constexpr bool UU_LDS = MCMC_DUO1_UU_LDS != 0;
    static_assert(duo1_lds(DQ) + sizeof(pair_t) * kDuoStagedPairs + sizeof(dpair_t) * SHORT_LOG_TABLE_SIZE <= 80 * 1024,
                  "two workgroups per CU");
    static_assert(2 * C <= 256, "a chunk's |u|^2: at most one dword per lane of the workgroup");
    static_assert(SPLIT ? (NE == 2 * DQ || NE == 2 * DQ - 1) : NE == 2 * DQ, "dimensions per lane");
    const StepArgs& s = a.s;
    const int tid = threadIdx.x, h = tid & 1, wave = tid >> 6, lane = tid & 63;
    const int W = s.W, d = a.d;
    const int w = blockIdx.x * 128 + (tid >> 1);
    const int g = __builtin_amdgcn_readfirstlane(w / s.group_size);
    const int ncols = s.n_steps;
    // (the launch's columns inside its direction set: see IncStepArgs::vu_cols)
    const int set_cols = a.vu_cols > 0 ? a.vu_cols : ncols;
    const double2* __restrict__ gVU = (const double2*)a.VU + ((size_t)g * set_cols + (size_t)a.col0) * COLB;
    const double* __restrict__ gUUc = a.UU + ((size_t)g * set_cols + (size_t)a.col0);   // |u|^2 of the launch's columns
    double* const sUU = (double*)(smem2 + 2 * CHUNK);                                    // [2][C], behind the pairs
    // chunk k -> buffer k & 1, by DMA (as in step_inc_kernel)
    auto stage = [&](int k) {   // (written out in every kernel: incremental_common.h, "around the step loop")
        const int first = k * C;
        if (first >= ncols) return;
        const int cols = ncols - first < C ? ncols - first : C;
        const int bytes = cols * COLB * 16;
        const char* src = (const char*)(gVU + (size_t)first * COLB);
        char* dst = (char*)(smem2 + (k & 1) * CHUNK);
        for (int kb = wave; kb * 1024 < bytes; kb += 4) {
            if (kb * 1024 + lane * 16 < bytes)
                stage16_dma<MCMC_DUO1_DMA_HIDDEN != 0>(dst + kb * 1024, src + kb * 1024 + lane * 16);
        }
        // the chunk's |u|^2, a dword per lane (8-byte aligned only: a launch starts at any column of its set); wave
        // j moves the dwords 64 j .. 64 j + 63 of the 2 cols
        if constexpr (UU_LDS) {
            if (wave * 64 + lane < 2 * cols)
                stage4_dma((char*)(sUU + (k & 1) * C) + wave * 256, (const char*)(gUUc + first) + (wave * 64 + lane) * 4);
        }
    };
    const bool refresh_y = (a.anchor & 2) != 0;   // wave-uniform
    if (!refresh_y) stage(0);
    const double blo = a.box_lo, bhi = a.box_hi;
    const unsigned bhi_word = (unsigned)__double2hiint(bhi);   // (blo == +0, 0 < bhi < inf)
    double x[NE], y[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = duo1_dim<SPLIT>(e, h);
        const bool in = i < d;
        // (a padded dimension rests at the middle of the box, inside for every step)
        x[e] = in ? s.x[(size_t)i * W + w] : 0.5 * (blo + bhi);
        y[e] = in ? a.y[(size_t)i * W + w] : 0.0;
    }
    double lpost = s.logpost[w], lpri = s.logprior[w], llik = s.loglike[w];
    __shared__ pair_t sRE[kDuoStagedPairs];
    if (refresh_y) {
        // y = L^-1 (x - mu) from the walker's x, as step_inc_kernel does it: the deviations of the
        // workgroup's 128 walkers in the chunk buffers ([walker][SD doubles], zero beyond d), L^-1 eight
        // columns at a time through a [dpad][8] tile in sRE, one ascending fma chain per row from +0.0
        constexpr int TW = 8, SD = (dpad + TW - 1) / TW * TW;
        static_assert(128 * SD <= 4 * CHUNK, "the chunk buffers hold the deviations of the workgroup's walkers");
        static_assert(sizeof(pair_t) * kDuoStagedPairs >= sizeof(double) * dpad * TW, "the tile fits sRE");
        double* const sdev = (double*)smem2 + (size_t)(tid >> 1) * SD;
        double* const tile = (double*)sRE;
        for (int i = h; i < SD; i += 2) sdev[i] = 0.0;   // (a wave's LDS writes land in order)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = duo1_dim<SPLIT>(e, h);
            if (i < d) sdev[i] = x[e] - a.mean[i];
            y[e] = 0.0;
        }
        for (int i0 = 0; i0 < d; i0 += TW) {
            __syncthreads();   // (the previous tile has been used; the first: sdev is written)
            for (int e = tid; e < dpad * TW; e += 256) {
                const int j = e / TW, i = i0 + e % TW;
                tile[e] = (j < d && i < d) ? a.Lrow[(size_t)j * d + i] : 0.0;
            }
            __syncthreads();
            const lds_doubles pt = relaunder(tile + (SPLIT ? h : 2 * h) * TW), pd = relaunder(sdev + i0);
#pragma unroll
            for (int ii = 0; ii < TW; ++ii) {
                const double dv = pd[ii];   // (beyond d: 0, and the tile's column is 0)
#pragma unroll
                for (int e = 0; e < NE; ++e) y[e] = fma(pt[duo1_off<SPLIT>(e) * TW + ii], dv, y[e]);
            }
        }
        __syncthreads();   // every wave is done with its scratch: the first chunk may land
        stage(0);
    }
    if (a.anchor) {   // (wave-uniform) y has just been refreshed from x: orc_anchor_loglike
        double pa0 = 0.0, pa1 = 0.0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e & 1) pa1 = fma(y[e], y[e], pa1);
            else pa0 = fma(y[e], y[e], pa0);
        }
        llik = anchored_logpdf(s.cnorm0, duo1_sum<SPLIT>(pa0, pa1));
        lpost = lpri + llik;
    }
    int wt = s.weight[w], prej = s.prior_rej[w], burn = s.burn_left[w];
    long long nacc0 = s.n_accept[w];
    int nacc = 0;
    const cdoubles gUU = (cdoubles)(unsigned long long)(a.UU + (size_t)g * set_cols + (size_t)a.col0);
    const uint32_t gid = s.walker0 + (uint32_t)w;
    const TryLimits tl = try_limits(s.max_tries);
    __shared__ dpair_t short_log_lds[SHORT_LOG_TABLE_SIZE];
    const short_log_tab slog = short_log_load(short_log_lds);
    dma_wait();   // chunk 0 has landed
    __syncthreads();
    // (the walker's own loads have landed with it, and the compiler is told so: it does not see the wait above, and
    // with one of them pending by its books it drains vmcnt in front of every chunk's steps -- the DMA just issued)
    if constexpr (MCMC_DUO1_DMA_HIDDEN != 0) {
        asm volatile("" : "+v"(lpost), "+v"(lpri), "+v"(llik), "+v"(wt), "+v"(prej), "+v"(burn), "+v"(nacc0));
#pragma unroll
        for (int e = 0; e < NE; ++e) asm volatile("" : "+v"(x[e]), "+v"(y[e]));
    }
    bool burning = lanes(burn > 0) != 0ull;   // wave-uniform
    unsigned long long cur_oct = ~0ull;
    DuoVariates sv;
    sv.init(sRE, wave, lane);
    const int hw_slot = hw_wave_slot();
    // the lanes that were over the limit of tries at some step: gathered by every step, looked at once per chunk
    unsigned long long stuck_m = 0ull;

    // A chunk's steps run OCTET by octet of the global step index (round 17): the burst of variates, then the up to
    // eight steps the octet has inside the chunk -- a chunk is a multiple of four columns and a launch starts
    // anywhere, so an octet may begin in one chunk and end in the next.  The common path of a step is straight-line
    // code whose one taken branch is the back-edge (tools/check_step_path.py): the octet test and the 64-bit step
    // index stand in front of the octet, the exact support test, the exact accept, the burn-in bookkeeping, the test
    // of the limit of tries and the report of a stuck chain behind the loop.  The commit's block, under the accept
    // mask, lies in front of the latch: its guard (s_cbranch_execz) is taken by a wave without an accepting lane only.
    for (int base = 0, k = 0; base < ncols; base += C, ++k) {
        const double2* __restrict__ cur = smem2 + (k & 1) * CHUNK;
        stage(k + 1);
        const int cols = __builtin_amdgcn_readfirstlane(ncols - base < C ? ncols - base : C);
        unsigned coff = lds_offset(cur + (SPLIT ? h : 2 * h));
        unsigned uoff = lds_offset(sUU + (k & 1) * C);   // (the same address in every lane: a broadcast read)
        // wt - prej grows by at most one per step: where no chain of the wave can pass lim1 within the chunk's columns,
        // its steps do not look (the burning wave keeps its bookkeeping, and its higher limit, at every step)
        bool watch = burning || lanes(wt - prej > tl.lim1 - cols) != 0ull;   // wave-uniform
#pragma unroll 1
        for (int sl0 = 0; sl0 < cols;) {
            const unsigned long long S0 = s.step0 + (unsigned long long)(base + sl0);
            if ((S0 >> 3) != cur_oct) {   // (not the octet the chunk before ended in)
                cur_oct = S0 >> 3;
                // (the turn from the shader clock: taken from the octet index instead -- a turn every 16 octets, no
                // s_memtime and no wait for it -- the kernel ran 5.5 % slower, profiles/r25_burst_chains.txt)
                rotate_priority<2>(hw_slot);
                // the lane half's two Philox blocks one after the other (rolled: one block's registers at a time)
                auto rolled = [&](uint32_t id) {
#pragma unroll 1
                    for (int q = 0; q < 2; ++q) {
                        PairRng pr;
                        pr.run_lazy(s.key0, s.key1, id, (cur_oct << 2) + (unsigned long long)(2 * h + q), slog);
                        sv.put(sRE, wave, lane, h, q, pr);
                    }
                };
#pragma unroll
                for (int rep = 0; rep < MCMC_DUO1_BURST_REPEAT; ++rep) {
                    uint32_t id = gid;
                    if constexpr (MCMC_DUO1_BURST_REPEAT > 1) asm volatile("; burst again" : "+v"(id));
                    if constexpr (MCMC_DUO1_BURST_CHAINS != 0) {
                        // one straight-line burst (det_math.h: OctetRng) in the registers of the step's (v, u) pairs,
                        // which are dead here.  A radial uniform in its lowest bin: the rolled loop, behind the
                        // stores, draws the lane half's four variates again with the redrawn tail, over the same slots
                        OctetRng o;
                        o.draw_lazy(s.key0, s.key1, id, (cur_oct << 2) + (unsigned long long)(2 * h), slog);
                        sv.put(sRE, wave, lane, h, o);
                        if (__builtin_expect(o.low != 0ull, 0)) rolled(id);   // (wave-uniform, rare)
                    } else {
                        rolled(id);
                    }
                }
            }
            sv.seek(S0);
            const int left = cols - sl0, in_oct = 8 - (int)(S0 & 7ull);
            const int n_oct = left < in_oct ? left : in_oct;   // >= 1
            [[maybe_unused]] const cdoubles uu_oct = gUU + (base + sl0);
#pragma unroll 1
            for (int so = 0; so < n_oct; ++so, coff += COLB * 16) {
                // (the step's place in the octet as the compiler cannot follow it: the 64-bit step index, which only
                // the exact accept needs, is then formed there and not carried by every step)
                int so_here = so;
                asm volatile("" : "+s"(so_here));
                // |u|^2 of the column from the chunk's LDS, requested in FRONT of the step's other reads (LDS answers in
                // order: the first rung's count covers it) -- no scalar load between the reads and the commit
                double uu;
                if constexpr (UU_LDS) {
                    uu = *(lds_doubles)(unsigned long long)uoff;
                    uoff += 8u;
                }
                double r, Ea;
                sv.fetch(r, Ea);
                sv.next();
                // the step's pairs stay in registers from the trial to the commit (requesting the next
                // step's behind the commit, over the bookkeeping, was measured slower: 1.24 against 1.02 ms)
                pair_t pk[NE];
                double tx[NE];   // the trial coordinates: the support test reads them, an accepting lane commits them
                const lds_pairs col = (lds_pairs)(unsigned long long)coff;
#pragma unroll
                for (int e = 0; e < NE; ++e) pk[e] = col[duo1_off<SPLIT>(e)];
                // the support test on the high words of the trial coordinates (step_inc_kernel MODE 0)
                unsigned hmx = 0u;
                double pc0 = 0.0, pc1 = 0.0;
                // The reads land in order and each is waited for by its count (stage16_dma), so the arithmetic runs
                // underneath their return: groups of G = MCMC_DUO1_LADDER pairs (1 <= G <= NE; measured at dq = 8 only:
                // G = 4 against G = 1 and the compiler's own order, profiles/r14_lds_wait_ladder.txt; the smaller dq
                // take the same G unmeasured) pinned in this order: the trial of the group's LAST pair first -- one rung
                // retires the group's reads --, then the others, then the group's y . u in ascending order (the sums'
                // order is the specification's).
                {
                    constexpr int G = MCMC_DUO1_LADDER;
                    static_assert(G >= 1, "pairs per rung");
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int e0 = 0; e0 < NE; e0 += G) {
                        const int e1 = e0 + G < NE ? e0 + G : NE;
#pragma unroll
                        for (int q = 0; q < e1 - e0; ++q) {
                            const int e = q == 0 ? e1 - 1 : e0 + q - 1;
                            tx[e] = fma(r, pk[e].x, x[e]);
                            const unsigned hw = (unsigned)__double2hiint(tx[e]);
                            hmx = hmx > hw ? hmx : hw;
                        }
#pragma unroll
                        for (int e = e0; e < e1; ++e) {
                            if (e & 1) pc1 = fma(y[e], pk[e].y, pc1);   // (y . u: the log-likelihood is carried)
                            else pc0 = fma(y[e], pk[e].y, pc0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    asm volatile("" : "+v"(pc0), "+v"(pc1));   // (here, not sunk behind the support test's branch)
                }
                // (behind the last rung: a scalar load in flight across the reads puts LGKM truly out of order)
                if constexpr (!UU_LDS) uu = uu_oct[so_here];   // (wave-uniform address: a scalar load)
                // The support test, decided on the high words where they decide it (round 17).  hmx is the unsigned maximum
                // of the high words of the walker's trial coordinates t (both lanes: pair_max_u32), W = bhi_word the high
                // word of hi; blo == +0 and 0 < hi < inf, so W < 0x7ff00000.  The exact test is 0 <= t && t <= hi for every t.
                //   hmx < W: INSIDE.  Every high word is below W, so every sign bit is clear (t >= +0) and, the doubles of one
                //     sign being ordered as their bit patterns, every t < the least double with high word W <= hi.
                //   hmx > W and hmx != 0x80000000: OUTSIDE.  Let t be a coordinate whose high word is hmx.  Sign bit clear:
                //     t's bit pattern is above that of every double with high word W, hi among them -- t > hi, +inf, or a
                //     NaN, for which both exact compares are false.  Sign bit set and hmx > 0x80000000: a negative normal
                //     number, -inf or a NaN with the sign set -- t >= 0 is false.
                //   hmx == 0x80000000: IN DOUBT.  The coordinate is -0.0 (inside: -0.0 >= +0 and <= hi) or a negative
                //     denormal (outside), which the low word tells apart; every other high word is at most 0x80000000, so
                //     the other coordinates may lie on either side of hi.
                //   hmx == W: IN DOUBT.  Every coordinate is >= +0 and those with a high word below W are inside; those
                //     with W lie in the slice [trunc(hi), trunc(hi) + 2^-20 ulp_hi), hi itself among them, on either side of hi.
                // (A padded dimension rests at hi / 2 with v = 0: its high word is below W for a normal hi; for a denormal
                // hi W is 0, nothing is below it and every step is in doubt.)  Only a wave with a lane in doubt takes the
                // exact comparisons, for all its lanes; they agree with the two certain classes by the above.  A wave with a
                // lane outside and none in doubt (estimated at 13 % of the wave-steps on bench.py's target) took them before.
                const unsigned pmx = pair_max_u32(hmx);
                unsigned long long inside_m = lanes(pmx < bhi_word);
                if (__builtin_expect(inside_m != lanes(true), 0)) {   // (wave-uniform) a lane outside or in doubt
                    if (__builtin_expect((lanes(pmx == bhi_word) | lanes(pmx == 0x80000000u)) != 0ull, 0)) {   // (rare) in doubt
                        unsigned long long inb = ~0ull;
#pragma unroll
                        for (int e = 0; e < NE; ++e) inb &= lanes(tx[e] <= bhi) & lanes(tx[e] >= blo);
                        inside_m = pair_all_mask(inb);
                    }
                }
                // chi2(y + r u) - chi2(y) = r (2 y.u + r |u|^2) (step_core_inc, `carry`)
                const double yu = duo1_sum<SPLIT>(pc0, pc1);
                const double mhr = -0.5 * r;
                const double lp = s.uniform_logp;
                const double ll = fma(mhr, fma(r, uu, yu + yu), llik);
                const double lt = lp + ll;
                const double delta = UNIT_T ? (lpost - lt) : (lpost - lt) / s.temperature;
                // (Ea > delta from the staged estimate, exact where in doubt: det_math.h accept_lanes.  At T = 1
                // lt > lpost is delta = lpost - lt < 0 < Ea, already in it; at other temperatures the compare stays)
                const unsigned long long up_m = UNIT_T ? 0ull : lanes(lt > lpost);
                const unsigned long long acc_m =
                    inside_m & (up_m | accept_lanes(Ea, delta, a.accept_slack, s.key0, s.key1, gid,
                                                    S0 + (unsigned long long)so_here, slog));   // (the index: formed where it is used)
                const bool accept = __builtin_amdgcn_inverse_ballot_w64(acc_m);
                // The commit runs on the accepting lanes alone (round 20; step_core_inc -> commit assigns x = t, y = yt
                // on an accept and touches nothing on a reject): x takes the trial -- on such a lane fma(r, v, x) IS the
                // new coordinate, nothing is formed again --, y moves on with r itself, the carried values and the
                // bookkeeping are written under the same mask.  A wave of 32 walkers has an accepting lane at nearly
                // every step: the block lies on the common path and falls through into the loop's latch.
                wt += 1;
                prej += __builtin_amdgcn_inverse_ballot_w64(inside_m) ? 0 : 1;
                if (accept) {
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        x[e] = tx[e];
                        y[e] = fma(r, pk[e].y, y[e]);
                    }
                    llik = ll;
                    lpost = lt;
                    wt = 1;
                    prej = 0;
                    nacc += 1;
                }
                // (the test of the limit of tries and the burning wave's bookkeeping lie behind the loop: a wave past its
                // burn-in whose chains cannot pass the limit inside this chunk -- `watch`, at the head of the chunk -- skips both)
                if (__builtin_expect(watch, 0)) {   // wave-uniform
                    unsigned long long over_m = lanes(wt - prej > tl.lim1);
                    if (burning) {   // wave-uniform (see step_inc_kernel); goes from true to false once per run
                        // (wt and prej are the committed ones, the limit is that of the burn-in left BEFORE this step)
                        const int lim = tl.of(burn);
                        burn -= (accept & (burn > 0)) ? 1 : 0;
                        burning = lanes(burn > 0) != 0ull;
                        over_m = lanes(wt - prej > lim);
                    }
                    stuck_m |= over_m;
                }
            }
            sl0 += n_oct;
        }
        // a chain over its limit of tries is reported by a lane that was over it at some step of the chunk (it may
        // have accepted since): the flag says that, and names such a walker
        if (__builtin_expect(stuck_m != 0ull, 0)) {
            if (__builtin_amdgcn_inverse_ballot_w64(stuck_m) && h == 0) report_stuck(s.stuck, gid);
            stuck_m = 0ull;
        }
        dma_wait();   // the next chunk has landed
        __syncthreads();
    }
    // (the walker index passes through an empty asm: the store addresses are formed here, not kept
    // alive from the prologue's loads)
    int we = w, he = h;
    asm volatile("" : "+v"(we), "+v"(he));
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = duo1_dim<SPLIT>(e, he);
        if (i < d) {
            s.x[(size_t)i * W + we] = x[e];
            a.y[(size_t)i * W + we] = y[e];
        }
    }
    if (h == 0) {
        s.logpost[we] = lpost; s.logprior[we] = lpri; s.loglike[we] = llik;
        s.weight[we] = wt; s.prior_rej[we] = prej; s.burn_left[we] = burn;
        s.n_accept[we] = nacc0 + nacc;
    }
    wave_add_accepts(s.accept_total, (h == 0) ? nacc : 0);
}

// max |ea_f - Ea| over this block's share of ka = 1 .. 2^28 - 1 (Ea = neg_log_short(2 ka + 1, 29), the
// value the estimate stands for): the condition on the hardware's log2 that accept_lanes rests on
__global__ void __launch_bounds__(256) accept_estimate_error_kernel(double* err, uint32_t* at)
{
    __shared__ dpair_t short_log_lds[SHORT_LOG_TABLE_SIZE];
    const short_log_tab slog = short_log_load(short_log_lds);
    __shared__ double serr[256];
    __shared__ uint32_t sat[256];
    __syncthreads();
    const unsigned long long n = 1ull << 28, stride = (unsigned long long)gridDim.x * 256ull;
    double worst = -1.0;
    uint32_t where = 0u;
    for (unsigned long long k = 1ull + blockIdx.x * 256ull + threadIdx.x; k < n; k += stride) {
        const uint32_t ka = (uint32_t)k;
        const double e = fabs((double)accept_estimate(ka) - neg_log_short(2u * ka + 1u, 29, slog));
        if (e > worst || e != e) { worst = e; where = ka; }   // (a NaN stays and fails the check)
    }
    serr[threadIdx.x] = worst;
    sat[threadIdx.x] = where;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i)
            if (serr[i] > worst || serr[i] != serr[i]) { worst = serr[i]; where = sat[i]; }
        err[blockIdx.x] = worst;
        at[blockIdx.x] = where;
    }
}

template <int DQ, int NE, bool SPLIT>
hipError_t launch_duo1(const IncStepArgs& a, hipStream_t st)
{
    constexpr int C = duo1_chunk(DQ);
    const size_t lds = duo1_lds(DQ);
    static_assert(duo1_lds(DQ) >= sizeof(double2) * 2 * C * 4 * DQ, "the pairs' buffers");
    const bool unit_t = a.s.temperature == 1.0;
    typedef void (*kern_t)(const IncStepArgs);
    static const kern_t kerns[2] = {step_inc_duo_kernel<DQ, NE, SPLIT, false>,
                                    step_inc_duo_kernel<DQ, NE, SPLIT, true>};
    static const std::string names[2] = {"mcmc::step_inc_kernel<" + std::to_string(DQ) + ", 0, false, two lanes>",
                                         "mcmc::step_inc_kernel<" + std::to_string(DQ) + ", 0, true, two lanes>"};
    const int v = unit_t ? 1 : 0;
    if (lds > 40 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kerns[v],
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    mcmc_hip_note_step_kernel(names[v].c_str());
    hipLaunchKernelGGL(kerns[v], dim3(a.s.W / 128), dim3(256), lds, st, a);
    return hipGetLastError();
}

template <int DQ>
hipError_t dispatch_duo1(const IncStepArgs& a, hipStream_t st)
{
    if constexpr (DQ > kDuo1MaxDq) {
        return hipErrorInvalidValue;
    } else {
        if (a.dq != DQ) return dispatch_duo1<DQ + 1>(a, st);
        constexpr bool SPLIT = MCMC_DUO1_SPLIT != 0;
        if constexpr (SPLIT) {
            if ((a.d + 1) / 2 == 2 * DQ - 1) return launch_duo1<DQ, 2 * DQ - 1, true>(a, st);
            return launch_duo1<DQ, 2 * DQ, true>(a, st);
        } else {
            return launch_duo1<DQ, 2 * DQ, false>(a, st);
        }
    }
}
#endif  // MCMC_DUO_DQ_LO == 1

}  // namespace
}  // namespace mcmc

#define MCMC_CAT2(a, b) a##b
#define MCMC_CAT(a, b) MCMC_CAT2(a, b)
// one translation unit per range of DQ (build.py: -DMCMC_DUO_DQ_LO=.. -DMCMC_DUO_DQ_HI=..)
extern "C" hipError_t MCMC_CAT(mcmc_hip_launch_inc_duo_, MCMC_DUO_DQ_LO)(const mcmc::IncStepArgs* a,
                                                                       hipStream_t st)
{
    if (a->dq < MCMC_DUO_DQ_LO || a->dq > MCMC_DUO_DQ_HI || a->n_drag > 0 || a->colflag || a->s.rows ||
        a->s.W % 128 != 0 || a->s.group_size % 128 != 0)
        return hipErrorInvalidValue;
    for (int q = 0; q < 4; ++q)
        if (a->periodic_mask4[q]) return hipErrorInvalidValue;
    if (a->n_modes < 2 || !a->amode || a->vu_cols > 0) return hipErrorInvalidValue;
    return mcmc::dispatch_duo_mix<MCMC_DUO_DQ_LO>(*a, st);
}

#if MCMC_DUO_DQ_LO == 1
// one mode (step_inc_duo_kernel): MODE 0 (one box [0, hi]), Metropolis steps, no periodic parameter, no
// emitted rows, no block of one parameter, whole workgroups of 128 walkers inside one basis group
extern "C" hipError_t mcmc_hip_launch_inc_duo1(const mcmc::IncStepArgs* a, hipStream_t st)
{
    if (a->dq < 1 || a->dq > mcmc::kDuo1MaxDq || a->n_modes != 1 || a->n_drag > 0 || a->colflag || a->s.rows ||
        a->s.W % 128 != 0 || a->s.group_size % 128 != 0 || a->has_norm || !a->box || a->box_lo != 0.0 || !a->UU)
        return hipErrorInvalidValue;
    for (int q = 0; q < 4; ++q)
        if (a->periodic_mask4[q]) return hipErrorInvalidValue;
    return mcmc::dispatch_duo1<1>(*a, st);
}

extern "C" hipError_t mcmc_hip_launch_accept_estimate_error(double* err, uint32_t* ka, int n_blocks, hipStream_t st)
{
    if (n_blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcmc::accept_estimate_error_kernel, dim3(n_blocks), dim3(256), 0, st, err, ka);
    return hipGetLastError();
}
#endif
