// Which incremental step kernel serves a model shape, and what that kernel carries: the ONE
// statement of the rule.  mcmc_hip_incremental_supported, mcmc_hip_incremental_choice, the
// scheduler (capi_incremental.hip: step_incremental), the carries_* predicates and
// mcmc_hip_set_emit_thin all ask inc_choose().  No HIP in here: plain C++17, so the rule is
// compiled and tested where there is no GPU (tests/test_host_logic.py).
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define MCMC_CHOICE_HD __host__ __device__
#else
#define MCMC_CHOICE_HD
#endif

namespace mcmc {

constexpr int kMaxModes = 64;   // (16 until round 5; the tuned incremental kernels: 16, incremental_any.hip)

// step_inc_mix_kernel (carried mode log-densities): 2..4 modes up to d = 64, 5 and 6 as far as
// the state -- dq (K + 1) doubles per lane -- leaves the body its registers at two waves per SIMD
// (K = 5: d <= 32, K = 6: d <= 28; measured at d = 30, ms per 1200 steps of 65 536 walkers:
// K = 5 7.71 on the register-plane kernel -> 5.84 here; K = 6 at dq = 8 spills: 13.3 against ~8.6);
// everything else: the general incremental kernels
constexpr int kIncMixWideDq = 8;
MCMC_CHOICE_HD constexpr bool inc_mix_serves(int K, int dq)
{
    return K >= 2 && ((K <= 4 && dq <= 16) || (K <= 6 && dq <= kIncMixWideDq && dq * (K + 1) <= 50));
}

// step_duo_mix_kernel (incremental_duo.hip, round 6): the same step with TWO lanes per walker, each
// holding 2 dq dimensions -- 2..4 modes while the residuals y_1 .. y_K of a lane (2 dq K doubles) leave
// the body its registers at two waves per SIMD; x moves to LDS where it does not fit beside them
// (duo_x_in_lds: two modes from d = 33 on, three from d = 25 on, four from d = 21 on).  K = 2: d <= 48;
// K = 3: d <= 32; K = 4: d <= 24.
constexpr int kDuoStateDoubles = 48;
#ifndef MCMC_DUO_MAX_DQ
#define MCMC_DUO_MAX_DQ 12
#endif
constexpr int kDuoMaxDq = MCMC_DUO_MAX_DQ;   // two modes up to d = 48 (round 6, late)
MCMC_CHOICE_HD constexpr bool duo_serves(int K, int dq)
{
    return K >= 2 && K <= 4 && dq <= kDuoMaxDq && 2 * dq * K <= kDuoStateDoubles;
}

// step_inc_duo_kernel (incremental_duo.hip, round 7): one mode, MODE 0, two lanes per walker up to d = 32
constexpr int kDuo1MaxDq = 8;

// periodic parameters step_inc_kernel<.., PER> serves (one mode, Metropolis steps, no emitted rows);
// more: the general incremental kernels (incremental_any.hip)
constexpr int kIncMaxPeriodic = 16;

// incremental_duo.hip (two lanes per walker) from this ensemble size on.  Measured (same box, d = 30,
// K = 2, step kernel ms per 1200 steps, four lanes / two; profiles/r06_duo.txt): 16 384 walkers 1.17 / 1.41,
// 32 768: 1.57 / 1.49 (K = 3, x in LDS: 1.85 / 2.13), 49 152: 2.06 / 1.77 (K = 3: 3.33 / 2.71; K = 4 at d = 24:
// 2.55 / 2.11), 65 536: 2.91 / 1.85, 98 304: 3.94 / 3.35, 131 072: 5.14 / 3.68 -- two lanes win once the
// four-lane kernel needs a second round of waves (49 152 walkers are its three waves per SIMD)
constexpr int kDuoMinWalkers = 49152;
// ... and for one mode (step_inc_duo_kernel, MODE 0, d <= 32) from this size on.  Measured (same box, d = 30,
// step kernel ms per 1200 steps, four lanes / two; profiles/r07_one_mode_two_lanes.txt): 32 768 walkers
// 0.751 / 0.762, 49 152: 0.926 / 0.935, 65 536: 1.096 / 0.990, 98 304: 1.863 / 1.821, 131 072: 2.156 / 1.952
#ifndef MCMC_DUO1_MIN_WALKERS
#define MCMC_DUO1_MIN_WALKERS 65536
#endif
constexpr int kDuo1MinWalkers = MCMC_DUO1_MIN_WALKERS;

// dragging (drag_inc_kernel): a step's 1 + n_drag columns must fit the LDS twice over
constexpr size_t kIncDragLdsBytes = 128u << 10;
// step_inc_kernel with a carried log-prior: from d = 113 on (dq >= 29) its chunks leave no room
// for the refresh of y inside the kernel
constexpr int kIncFoldPriorMaxDq = 28;

// the model and ensemble, as far as the choice depends on them
struct IncShape {
    int d = 0, K = 0, n_periodic = 0;
    int n_drag = 0;              // interpolation steps per dragging step; 0: Metropolis steps
    int W = 0, bgs = 0;          // walkers; walkers that share one Haar basis
    bool any_normal = false;     // some prior is normal
    bool one_box = false;        // every dimension uniform on the same interval
    bool box_lo_is_zero = false; // ... which begins at 0
    bool has_1d_block = false;   // a parameter block of one parameter (its columns draw other variates)
    bool emit = false;           // accepted rows are stored on the device (emit_capacity > 0)
    int duo = -1;                // two lanes per walker: -1 where it pays, 0 never, 1 wherever it serves
};

enum IncFamily {
    kIncNotServed = 0,
    kIncStep,        // step_inc_kernel / step_inc_periodic_kernel: one mode, four lanes per walker
    kIncStepEmit,    // step_inc_kernel<.., EMIT>: ... with emitted rows
    kIncMix,         // step_inc_mix_kernel: 2..6 modes, four lanes
    kIncAny,         // incremental_any.hip: the general kernels
    kIncDrag,        // drag_inc_kernel
    kIncDuoMix,      // step_duo_mix_kernel: 2..4 modes, two lanes per walker
    kIncDuoOne       // step_inc_duo_kernel: one mode, two lanes
};

enum IncReason {     // why a shape is not served
    kIncServed = 0,
    kIncBadShape,    // outside 2 <= d <= 128, 1 <= K <= kMaxModes, or an ensemble no basis group divides
    kIncDragShape,   // dragging with a mixture, a periodic parameter, or columns beyond the LDS
    kIncAnyLds,      // the general kernel's residuals fit neither registers nor LDS
    kIncEmitDrag     // emitted rows with dragging
};

struct IncChoice {
    IncFamily family = kIncNotServed;
    IncReason reason = kIncBadShape;
    int dq = 0;
    int dq_lo = 0;             // the translation unit of the launcher: 1 / 9 / 17 / 25 (two lanes: 1 / 9); 0: one symbol
    bool carry = false;        // one mode on step_inc_kernel: the log-likelihood is carried, |u|^2 of every column
    bool carry_modes = false;  // step_inc_mix_kernel / step_duo_mix_kernel: the log-density of every mode is carried
    bool carry_prior = false;  // step_inc_kernel with normal priors: the log-prior is carried
    bool carry_periodic = false;   // step_inc_kernel<.., periodic>: 1..16 periodic parameters
    bool fold = false;         // step_inc_kernel: the refresh of y is the kernel's, a direction set spans calls
    bool box = false;          // IncStepArgs::box
    int chunk_steps = 0;       // dragging steps per LDS chunk
    int colb = 0;              // doubles per column of VU: (v, u) pairs, or the planes v, u_1 .. u_K
    bool thins_on_device = false;   // mcmc_hip_set_emit_thin: the kernels of this shape thin emitted rows
    bool any() const { return family == kIncAny; }
    bool drag() const { return family == kIncDrag; }
    bool two_lanes() const { return family == kIncDuoMix || family == kIncDuoOne; }
};

// a shape incremental evaluation can be asked about at all (IncReason: kIncBadShape otherwise)
inline bool inc_shape_valid(const IncShape& s)
{
    return s.d >= 2 && s.d <= 128 && s.K >= 1 && s.K <= kMaxModes && s.n_periodic >= 0 &&
           s.n_periodic <= s.d && s.n_drag >= 0 && s.W > 0 && s.bgs > 0 && s.bgs % 64 == 0 &&
           s.W % s.bgs == 0;
}

// any_fits: the answer of mcmc_hip_inc_any_fits for this shape (asked by the caller: the general
// kernels' LDS budget lives with them)
inline IncChoice inc_choose(const IncShape& s, bool any_fits)
{
    IncChoice c;
    const int d = s.d, K = s.K, np = s.n_periodic, nd = s.n_drag;
    const int dq = c.dq = (d + 3) / 4;
    const bool drag = nd > 0;
    c.thins_on_device = K >= 1 && !drag;
    if (!inc_shape_valid(s)) return c;
    c.chunk_steps = (1024 / (4 * dq)) / (1 + nd) > 1 ? (1024 / (4 * dq)) / (1 + nd) : 1;
    const size_t drag_lds = sizeof(double) * 2 * 2 * (size_t)c.chunk_steps * (size_t)(1 + nd) * 4 * (size_t)dq;
    if (drag && (K > 1 || np > 0 || drag_lds > kIncDragLdsBytes)) {
        c.reason = kIncDragShape;
        return c;
    }
    // what the tuned kernels leave out runs on the general one (incremental_any.hip): more than
    // four modes, mixtures above d = 64, periodic parameters with a mixture, more than 16 of
    // them -- Metropolis steps only
    bool any = !drag && ((K > 1 && !inc_mix_serves(K, dq)) || (np > 0 && (K > 1 || np > kIncMaxPeriodic)));
    if (any && !any_fits) {
        c.reason = kIncAnyLds;
        return c;
    }
    if (s.emit) {
        if (drag) {
            c.reason = kIncEmitDrag;
            return c;
        }
        // step_inc_kernel<.., EMIT> emits for one mode with non-periodic priors and blocks of at
        // least two parameters; every other shape on the general kernels, which emit at run time
        if (K != 1 || np > 0 || s.has_1d_block) any = true;
        if (any && !any_fits) {
            c.reason = kIncAnyLds;
            return c;
        }
    }
    c.reason = kIncServed;
    // one mode, Metropolis steps: step_inc_kernel / step_inc_periodic_kernel, which carry the
    // log-likelihood along the whitened direction and need |u|^2 of every column
    c.carry = !any && !drag && K == 1;   // (round 5: with up to 16 periodic parameters too)
    c.carry_periodic = c.carry && np > 0;
    c.fold = c.carry && np == 0;         // step_inc_kernel: y refreshed in the kernel, sets of several launches
    // ... with normal priors: the log-prior is carried as well (the oracle's rule is the same --
    // carries_prior: where the log-likelihood is carried)
    c.carry_prior = c.carry && s.any_normal;
    if (c.carry_prior && dq > kIncFoldPriorMaxDq) c.fold = false;
    // mixtures on step_inc_mix_kernel (no periodic parameter, no emitted rows): the log-density of
    // every mode is carried; |u_k|^2 of every column and mode.  Everything else goes to the general
    // kernels, which sum every chi2_k from the trial's residual: the carried form was built for the
    // register-plane kernel as well and measured SLOWER there (K = 5 / 8 / 16 at d = 30:
    // 9.66 -> 8.26, 7.37 -> 6.46, 2.09 -> 1.85e9 evals/s, profiles/r05_carried_modes.txt) -- those
    // kernels wait on latency at one or two waves per SIMD, and the extra K registers cost more
    // than the d / 4 fewer FMAs per mode bought
    c.carry_modes = !any && !drag && K > 1;
    c.box = s.one_box;
    // doubles per column: (v, u) pairs, or the planes v, u_1 .. u_K of a mixture
    c.colb = ((K == 1 && !any) ? 8 : 4 * (1 + K)) * dq;
    c.dq_lo = any ? 0 : dq <= 8 ? 1 : dq <= 16 ? 9 : dq <= 24 ? 17 : 25;
    c.family = any ? kIncAny : drag ? kIncDrag : K > 1 ? kIncMix : s.emit ? kIncStepEmit : kIncStep;
    // Two lanes per walker (incremental_duo.hip): mixtures with carried mode log-densities, two modes
    // up to d = 48, three up to d = 32, four up to d = 24 (duo_serves), from kDuoMinWalkers
    // = 49 152 walkers on; one mode (round 7: step_inc_duo_kernel) with one box [0, hi] for every
    // dimension up to d = 32, from kDuo1MinWalkers on.  Metropolis steps without periodic parameters,
    // emitted rows or a block of one parameter, whole workgroups of 128 walkers inside a basis group.
    // Smaller ensembles keep the four-lane kernels, whose twice as many waves cover their latencies.
    const bool duo = s.duo != 0 && !any && !s.emit && !drag && np == 0 && s.W % 128 == 0 &&
                     s.bgs % 128 == 0 && !s.has_1d_block;
    if (duo && c.carry_modes && duo_serves(K, dq) && (s.duo == 1 || s.W >= kDuoMinWalkers)) {
        c.family = kIncDuoMix;
        c.dq_lo = dq <= 8 ? 1 : 9;
    }
    // (MODE 0 of step_inc_kernel: the same [0, hi] for every dimension)
    if (duo && c.carry && c.fold && s.one_box && s.box_lo_is_zero && dq <= kDuo1MaxDq &&
        (s.duo == 1 || s.W >= kDuo1MinWalkers)) {
        c.family = kIncDuoOne;
        c.dq_lo = 0;
    }
    return c;
}

}  // namespace mcmc
