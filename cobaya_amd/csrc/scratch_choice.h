// Which from-scratch step kernel (`evaluation: full`: every trial evaluated from scratch) serves a
// model shape, and with what launch geometry: the ONE statement of the rule.  mcmc_hip_step,
// mcmc_hip_set_target_*'s LDS check and mcmc_hip_scratch_choice all ask scratch_choose(); the
// launchers (walker_kernels.hip, walker_kernels_big.hip, general_kernels.hip) take its answer and
// only launch.  The constants and constexpr helpers the rule shares with the kernels live here too.
// No HIP in here: plain C++17, so the rule is compiled and tested where there is no GPU
// (tests/test_host_logic.py).
#pragma once
#include <stddef.h>

#include "inc_choice.h"   // MCMC_CHOICE_HD

namespace mcmc {

constexpr int kMaxDimLane = 32;   // lane-per-walker kernels: d <= 32 (state in VGPRs)
constexpr int kMaxDimPair = 56;   // ... and the two-wave step kernel alone up to here
// padded sizes MCMC_DP of the d > 32 kernels, one translation unit of walker_kernels_big.hip each
// (the other copy: BIG_DPS in cobaya_amd/build.py)
constexpr int kBigDps[] = {48, 56, 64, 72, 80, 88, 96, 100, 112, 120, 128};
constexpr int kSweepMaxDim = 112; // step_big_reg_kernel (column sweep) is compiled for MCMC_DP <= 112

constexpr size_t kLdsMax = 160 * 1024;   // LDS of a compute unit
constexpr int kPlacementCUs = 256;       // compute units the placement requests below reckon with
constexpr size_t kLdsNoAttr = 64 * 1024; // dynamic LDS up to here needs no hipFuncSetAttribute

// rows per block of the packed whitening factor (kernels.h: tri_stream_for_each)
constexpr int kRowBlock = 4;

// Doubles per (group, cycle) slab of proposal directions V[col][i]: d*d rounded up to whole
// KiB so that the step kernel can move a slab into LDS with 1 KiB global->LDS DMA pieces.
// With parameter blocks a cycle has `ncols` = sum_b oversample_b * n_b columns instead of d.
MCMC_CHOICE_HD constexpr int v_slab_cols(int ncols, int d)
{
    return ((ncols * d * 8 + 1023) / 1024) * 128;
}
MCMC_CHOICE_HD constexpr int v_slab(int d) { return v_slab_cols(d, d); }

// d > 32 ("big" kernels): columns of V are padded to an even number of doubles (16-byte aligned
// for the per-step 1 KiB global->LDS DMA), and a slab keeps >= 1 KiB behind its last column.
MCMC_CHOICE_HD constexpr int v_ld(int d) { return (d + 1) & ~1; }
MCMC_CHOICE_HD constexpr int v_slab_big(int d)
{
    return ((d * v_ld(d) * 8 + 1024 + 1023) / 1024) * 128;
}

// ---- the two-wave step kernel (walker_kernels.hip: step_pair_kernel)
// The split pays from d ~ 14: per 40d steps of 65 536 walkers, two waves vs one wave per walker
// set run 0.387 / 0.385 ms at d = 8, 0.698 / 0.655 at 12, 1.09 / 1.25 at 16, 1.61 / 1.93 at 20,
// 2.22 / 2.84 at 24.
#ifndef MCMC_PAIR_MIN
#define MCMC_PAIR_MIN 14
#endif
// (with normal priors the matrix-core kernel is ahead again from d = 55: 7.3 against 7.0)
constexpr int kMaxDimPairNormal = 54;
// Rows [0, split) of the whitening go to role 0, the rest to role 1.
// Measured at d = 30 (W = 65 536): splits 16 / 20 / 24 run 3.47 / 3.32 / 3.46 ms per 1200 steps,
// 12 runs 4.1 ms -- role 0 (which also generates the variates) takes about two thirds of the rows.
// With normal priors role 1 also forms the prior terms (a division each), and one more row
// block moves to role 0: at the config-5 shape (d = 27, 21 normal priors) splits 16 / 20 / 24
// run 4.42 / 4.25 / 4.03 ms per 1080 steps.
MCMC_CHOICE_HD constexpr int pair_split(int d, bool normp)
{
    if (d < MCMC_PAIR_MIN) return d;
    int h = kRowBlock * ((2 * d + 6) / 12);  // multiple of the row block nearest 2D/3
    // 32 < d <= 48, measured (10^10 evals/s at W = 65 536; the matrix-core kernel runs 1.15 at
    // every one of these d): d = 33: split 24 / 28 give 2.01 / 1.85; d = 36: 24 / 28 / 32 give
    // 1.85 / 1.76 / 1.78; d = 40: 24 / 28 / 32 / 36 give 1.60 / 1.63 / 1.68 / 1.51; d = 44:
    // 28 / 32 / 36 give 1.46 / 1.52 / 1.48; d = 48: 28 / 32 / 36 / 40 give 1.31 / 1.31 / 1.38 / 1.26
    // (d = 38 with split 24 dips to 1.56)
    // d = 50: 32 / 36 / 40 give 1.16 / 1.18 / 1.20; d = 52: 32 / 36 / 40 give 0.89 / 1.00 / 1.15;
    // d = 54: 40 / 44 give 1.02 / 1.07; d = 56: 40 / 44 / 48 give 0.85 / 0.97 / 0.84 (matrix
    // cores, padded to 56: 0.93) -- past d = 48 role 1 runs out of registers first
    if (d > kMaxDimLane) h = d < 37 ? 24 : (d < 47 ? 32 : (d < 49 ? 36 : (d < 53 ? 40 : 44)));
    if (normp) h += kRowBlock;
    const int hmax = d - 1 - (d - 1) % kRowBlock;   // largest whole number of row blocks below d
    return h < kRowBlock ? kRowBlock : (h > hmax ? hmax : h);
}
// exchanged doubles per walker and step: chi2 of role 0, r, Ea, the y_j of role 1; with
// normal priors also role 1's prior sum
// (d > 32: the three other chi2 chains of role 0 at the end)
MCMC_CHOICE_HD constexpr int pair_xf(int d, bool normp)
{
    return d - pair_split(d, normp) + (normp ? 4 : 3) + (d > kMaxDimLane ? 3 : 0);
}
constexpr int kPairWalkers = 256;   // two waves per 64 walkers: 512-thread workgroups of 256 walkers

// ---- the matrix-core step kernel (walker_kernels_big.hip: step_mfma_kernel)
// kMfmaWaves waves of 16 walkers per workgroup.  16 (256 walkers, one workgroup per CU, 128
// registers per lane, two passes with 73 spilled registers) measured 4.04 ms per 200 steps at
// d = 100; 8 (128 walkers, two workgroups per CU, 256 registers: one pass, no spills, no second
// evaluation of the trial) 4.33 ms -- four waves per SIMD hide more than the spills cost.
#ifndef MCMC_MFMA_WAVES
#define MCMC_MFMA_WAVES 16
#endif
constexpr int kMfmaWaves = MCMC_MFMA_WAVES;
constexpr int kMfmaWalkers = 16 * kMfmaWaves;
constexpr int kMfmaThreads = 64 * kMfmaWaves;
// Its 16 x 4 tiles of L^-1.  Row tile R holds the rows 16 R - shift .. + 15: when DP is not a
// multiple of 16 the PARTIAL row tile is the FIRST one (rows < 0 are zero padding), where it costs
// 4 - shift/4 tiles, instead of the last one, where it would cost KT (DP = 100: 91 tiles instead
// of 109).  The shift is a multiple of 4, so lane class c still holds the rows j = c (mod 4).
MCMC_CHOICE_HD constexpr int mfma_row_shift(int dp) { return (16 - (dp + 3) / 4 * 4 % 16) % 16; }
MCMC_CHOICE_HD constexpr int mfma_row_tiles(int dp) { return (dp + mfma_row_shift(dp) + 15) / 16; }
MCMC_CHOICE_HD constexpr int mfma_k_steps(int dp) { return (dp + 3) / 4; }
// tile (R, kk) exists for kk <= 4 R + 3 - shift / 4 (its last row is 16 R - shift + 15)
MCMC_CHOICE_HD constexpr int mfma_tiles(int dp)
{
    int n = 0;
    for (int R = 0; R < mfma_row_tiles(dp); ++R) {
        const int row = 4 * R + 4 - mfma_row_shift(dp) / 4;
        n += row < mfma_k_steps(dp) ? row : mfma_k_steps(dp);
    }
    return n;
}

// bytes of dynamic LDS step_kernel needs: two slabs of directions per group of a workgroup of `wg`
// walkers, the mode log-densities of a mixture
constexpr size_t step_lds_bytes(int K, int wg, int group_size, int slab)
{
    return sizeof(double) * ((size_t)2 * (size_t)(wg / group_size > 1 ? wg / group_size : 1) * (size_t)slab +
                             (K > 1 ? (size_t)K * (size_t)wg : 0));
}

// the model, the ensemble and the build, as far as the choice depends on them
struct ScratchShape {
    int d = 0;
    int K = 1;                   // Gaussian modes; 0: the `one` likelihood
    int W = 0, group_size = 0;   // walkers; walkers that share one Haar basis
    bool any_normal = false;     // some prior is normal
    bool any_periodic = false;   // some parameter is periodic
    bool emit = false;           // accepted rows are stored on the device (emit_capacity > 0)
    bool emit_thin = false;      // ... thinned on the device (mcmc_hip_set_emit_thin > 1)
    bool unit_t = true;          // temperature == 1
    bool own_basis = false;      // `shared_basis: False`: every walker has its own Haar basis
    bool blocked = false;        // parameter blocks
    int n_drag = 0;              // interpolation steps per dragging step; 0: Metropolis steps
    int cps = 0, cps_f = 0;      // direction columns per cycle: d, or sum_b oversample_b n_b with blocks
                                 // (dragging: of the slow blocks); of the fast blocks
    bool has_1d_column = false;  // this launch's columns include one of a one-parameter block
    // what the build provides
    bool lane_compiled = false;  // walker_kernels.hip for MCMC_D = d <= 32
    int big_dp = 0;              // the MCMC_DP of walker_kernels_big.hip that serves 32 < d <= 128; 0: none
    bool pair_compiled = false;  // walker_kernels.hip for 32 < MCMC_D = d <= 56 (the two-wave kernel alone)
};

enum ScratchFamily {
    kScratchNotServed = 0,
    kScratchStep,         // step_kernel<MULTI, GENERAL>: one lane per walker, d <= 32
    kScratchStepOwn,      // step_kernel<MULTI, true, own basis>
    kScratchPair,         // step_pair_kernel<UNIT_T, NORMP>: two waves per 64 walkers, 14 <= d <= 56
    kScratchMfma,         // step_mfma_kernel<NORMP>: matrix cores, 32 < d <= 128
    kScratchBigReg,       // step_big_reg_kernel: the column sweep, 32 < d <= 112
    kScratchGeneral,      // step_general_kernel: everything else at 32 < d <= 128
    kScratchDrag,         // drag_kernel<MULTI>: dragging at d <= 32
    kScratchGeneralDrag   // drag_general_kernel: dragging at 32 < d <= 128
};

enum ScratchReason {      // why a shape is not served
    kScratchServed = 0,
    kScratchBadShape,     // what mcmc_hip_create refuses: no kernels compiled for d, an ensemble that is
                          // no whole number of groups of a multiple of 64 walkers
    kScratchEmitThin,     // emit_thin without incremental evaluation
    kScratchOwnBlocks,    // own bases with parameter blocks or dragging
    kScratchGeneralLds,   // the general d > 32 kernels' LDS (x, the trial and the mode log-densities of 64 walkers)
    kScratchCycleLds,     // a cycle's directions, twice per group of a workgroup, against the LDS
    kScratchSweepSize,    // walker_kernels_big.hip's launcher: no column sweep above MCMC_DP = 112
    kScratchSweepNormal   // ... and none with normal priors
};

struct ScratchChoice {
    ScratchFamily family = kScratchNotServed;
    ScratchReason reason = kScratchBadShape;
    // the template arguments the launcher selects the instantiation by
    bool multi = false, general = false, unit_t = false, normp = false;
    int unit = 0;            // the compiled MCMC_D or MCMC_DP of the translation unit; 0: one symbol
    int walkers_per_wg = 0, threads = 0, grid = 0;
    size_t lds_bytes = 0;    // dynamic LDS of the launch, placement request included
    size_t lds_attr = 0;     // hipFuncAttributeMaxDynamicSharedMemorySize to set first; 0: not set
    int v_ld = 0;            // doubles between two columns of the directions
    int slab = 0, slab_f = 0;   // doubles per (group, cycle) slab of directions; of the fast blocks' (dragging)
};

namespace scratch_detail {
inline void geometry(ScratchChoice& c, int W, int walkers_per_wg, int threads, size_t lds, bool always_attr)
{
    c.walkers_per_wg = walkers_per_wg;
    c.threads = threads;
    c.grid = W / walkers_per_wg;
    c.lds_bytes = lds;
    c.lds_attr = (always_attr || lds > kLdsNoAttr) ? lds : 0;
}
// Placement: the waves of a step kernel run for the whole launch, and at W = 65 536 there are
// exactly as many waves as SIMDs.  Requesting (otherwise unused) LDS so that only
// ceil(#workgroups / kPlacementCUs) workgroups fit on a CU makes the dispatcher spread them
// evenly instead of doubling up waves on some SIMDs while others idle.
constexpr size_t placement_share(int grid)
{
    return (kLdsMax / (size_t)((grid + kPlacementCUs - 1) / kPlacementCUs) / 1024) * 1024;
}
}  // namespace scratch_detail

// The tests stand in the order mcmc_hip_step and the launchers applied them before they moved here.
inline ScratchChoice scratch_choose(const ScratchShape& s)
{
    using scratch_detail::geometry;
    using scratch_detail::placement_share;
    ScratchChoice c;
    const int d = s.d, K = s.K, W = s.W, gs = s.group_size;
    const bool big = !s.lane_compiled && s.big_dp > 0;
    if (d < 1 || (!s.lane_compiled && !big) || (s.lane_compiled && d > kMaxDimLane) || (big && s.big_dp < d) ||
        K < 0 || W <= 0 || gs <= 0 || gs % 64 != 0 || W % gs != 0)
        return c;
    const auto refuse = [&c](ScratchReason r) { c.reason = r; return c; };
    if (s.emit_thin) return refuse(kScratchEmitThin);
    const bool drag = s.n_drag > 0, multi = K > 1;
    const bool own = s.own_basis && d > 1;   // (mcmc_hip_create: a basis per walker needs d > 1)
    // parameter blocks and dragging at d > 32: blocked directions in the d <= 32 layout -- column
    // stride d -- read by the general kernels
    const bool big_blocked = big && (s.blocked || drag);
    c.slab = (big && !big_blocked) ? v_slab_big(d) : v_slab_cols(s.cps, d);
    c.slab_f = drag ? v_slab_cols(s.cps_f, d) : 0;
    c.v_ld = (big && !big_blocked) ? v_ld(d) : d;
    if (own && (s.blocked || drag)) return refuse(kScratchOwnBlocks);
    // d > 32: what the matrix-core / two-wave / column-sweep kernels leave out (own bases, blocks,
    // mixtures, `one`, periodic parameters, emitted rows; ensembles of no whole 256 walkers with
    // normal priors or d > kSweepMaxDim, which the column sweep does not serve) runs on the general kernels
    const bool to_general = big && (own || big_blocked || K != 1 || s.any_periodic || s.emit ||
                                    (W % kMfmaWalkers != 0 && (s.any_normal || d > kSweepMaxDim)));
    const size_t general_lds = sizeof(double) * 64 * (size_t)(2 * d + (K > 1 ? K : 1));
    if (to_general && general_lds > kLdsMax) return refuse(kScratchGeneralLds);
    // workgroups are 256, 128 or 64 walkers wide
    const int wg = (W % 256 == 0) ? 256 : (W % 128 == 0) ? 128 : 64;
    if (!big && !drag && !own && step_lds_bytes(K, wg, gs, c.slab) > kLdsMax) return refuse(kScratchCycleLds);

    c.reason = kScratchServed;
    c.multi = multi; c.unit_t = s.unit_t; c.normp = s.any_normal;
    if (drag && big) {
        c.family = kScratchGeneralDrag;
        geometry(c, W, 64, 64, general_lds, false);
        return c;
    }
    if (drag) {   // (its own workgroup rule: 256 or 64, not 128)
        c.family = kScratchDrag;
        c.unit = d;
        const int bs = (W % 256 == 0) ? 256 : 64;
        geometry(c, W, bs, bs, sizeof(double) * (size_t)bs * (size_t)(2 * d + (multi ? K : 0)), false);
        return c;
    }
    if (to_general) {   // (the launcher's own test of general_lds against kLdsMax: kScratchGeneralLds above)
        c.family = kScratchGeneral;
        geometry(c, W, 64, 64, general_lds, false);
        return c;
    }
    // the two-wave kernel serves: one mode, non-periodic priors (normal ones have their own
    // instantiation), no emitted rows, no one-parameter blocks, whole 256-walker workgroups
    const size_t pair_lds = sizeof(double) * ((size_t)2 * (size_t)(kPairWalkers / gs) * (size_t)c.slab +
                                              (size_t)2 * (size_t)pair_xf(d, s.any_normal) * kPairWalkers);
    const bool pair = (big ? s.pair_compiled : true) && d >= MCMC_PAIR_MIN && d <= kMaxDimPair &&
                      !(s.any_normal && d > kMaxDimPairNormal) && !s.any_periodic && K == 1 && !s.emit &&
                      !s.has_1d_column && W % kPairWalkers == 0 && kPairWalkers % gs == 0 && pair_lds <= kLdsMax;
    if (pair && !own) {   // (own bases at d <= 32 come first: step_kernel<.., own basis> below)
        c.family = kScratchPair;
        c.unit = d;
        const int grid = W / kPairWalkers;
        size_t want = placement_share(grid);
        if (grid <= kPlacementCUs) want = 96 * 1024;   // > half of the LDS: one workgroup per CU
        geometry(c, W, kPairWalkers, 2 * kPairWalkers, want > pair_lds ? want : pair_lds, true);
        return c;
    }
    if (big) {
        c.unit = s.big_dp;
        if (W % kMfmaWalkers == 0 && (kMfmaWalkers % gs == 0 || gs % kMfmaWalkers == 0)) {
            c.family = kScratchMfma;
            const int gpb = (kMfmaWalkers + gs - 1) / gs;   // groups touching a workgroup
            const size_t lds = sizeof(double) * (size_t)(mfma_tiles(s.big_dp) * 64 + 24 * mfma_k_steps(s.big_dp) +
                                                         2 * gpb * 128);
            // placement: 256 walkers per CU at W = 65 536 -- ask for just under 1/n of the LDS so
            // that exactly n = 256 / walkers-per-workgroup workgroups share a CU
            const size_t share = kLdsMax / (size_t)(256 / kMfmaWalkers) - 2048;
            geometry(c, W, kMfmaWalkers, kMfmaThreads, lds > share ? lds : share, true);
            return c;
        }
        // Unreachable from an engine: mcmc_hip_create admits group_size 64, 128 and 256 only, so the
        // matrix-core kernel takes every W % 256 == 0, and `to_general` above has taken normal priors
        // and d > kSweepMaxDim at every other W.
        if (s.big_dp > kSweepMaxDim) return refuse(kScratchSweepSize);
        if (s.any_normal) return refuse(kScratchSweepNormal);
        c.family = kScratchBigReg;
        geometry(c, W, wg, wg, sizeof(double) * (size_t)(s.big_dp * s.big_dp + 4 * s.big_dp + 2 * (wg / gs) * 128),
                 true);
        return c;
    }
    c.unit = d;
    const int grid = W / wg;
    size_t want = placement_share(grid);
    if (want > kLdsNoAttr) want = kLdsNoAttr;
    if (own) {
        // no directions in LDS (the mode log-densities of a mixture and the placement request only):
        // the GENERAL step with every walker's own columns from HBM.  (The launcher's own test
        // against kLdsMax: at most kMaxModes * 256 doubles, never above it.)
        c.family = kScratchStepOwn;
        c.general = true;
        const size_t lds = sizeof(double) * (size_t)(multi ? K * wg : 0);
        geometry(c, W, wg, wg, want > lds ? want : lds, false);
        return c;
    }
    // (the launcher's own test of the cycle's directions against kLdsMax: kScratchCycleLds above)
    c.family = kScratchStep;
    c.general = s.any_normal || s.any_periodic || K == 0 || s.emit || d == 1 || s.has_1d_column;
    const size_t lds = step_lds_bytes(K, wg, gs, c.slab);
    geometry(c, W, wg, wg, want > lds ? want : lds, false);
    return c;
}

}  // namespace mcmc
