// Kernel arguments of function_kernels.hip (shared with capi_targets.hip).
#pragma once
#include "kernels.h"

namespace mcmc {

// ---- target kind `function` (function_kernels.hip; DESIGN.md section 2, "Function targets"):
// the Metropolis step split at the evaluation.  The trial points leave the propose half
// POINT-MAJOR, [W][d] contiguous -- the (n, d) tensor the user's batched function reads -- and
// come back through the accept half, which reads the [W] log-likelihoods the function left.
constexpr int kFnTileDims = 32;      // dimensions per LDS tile (64 walkers x <= 32 dimensions)
constexpr int kFnTileStride = 65;    // doubles between the dimensions of a tile: 64 walkers + 1 of padding
struct FnWalkerArgs {
    StepArgs s;            // state, prior constants (cblock, ConstLayout{d, 0}), V, keys;
                           // s.step0 = the step PROPOSED by this launch, s.ncyc cycles in V
    int d;
    int ld;                // column stride of V: d (the d <= 32 layout) or v_ld(d)
    int cyc, col;          // cycle (relative to the first one held in V) and column of that step
    uint32_t norm_mask4[4];   // one bit per dimension with a normal prior
    double* points;        // [W][d] trial points, point-major (the function's input)
    double* lp_t;          // [W] log-prior of the trial, -inf outside the support
    double* Ea;            // [W] Exp(1) variate of the accept test
    const double* ll_t;    // [W] what the function returned for the trial
    int* bad;              // [1] 1 + global id of the first walker whose value INSIDE the support
                           // was NaN or +inf (0: none)
};

// ---- several functions over parameter blocks (fn_blocked_walker_kernel; DESIGN.md section 2,
// "Function targets with parameter blocks"): the step of ONE slot of the blocked cycle.  The slot
// schedule is the same for every group, so whether function c is called at a slot ("due": it has an
// input in the slot's block or a faster one) is one bit per launch; a function that is not due
// keeps its carried value ll_c[c][w].  The full trial goes to w.points as in fn_walker_kernel (the
// accept half commits it from there); each DUE function's inputs go to its own point-major buffer.
constexpr int kFnMaxFunctions = 8;
struct FnBlockedArgs {
    FnWalkerArgs w;        // w.col = the slot, w.ld = column stride of the directions of a cycle,
                           // w.points = the FULL trial [W][d]; w.ll_t is not read
    int oned;              // the slot moves a one-parameter block: RandProposer1D variates (the slot's flag)
    int n_fn;
    unsigned due;          // bit c: function c is called for the trial this launch PROPOSES
    unsigned due_prev;     // ... was called for the trial this launch ACCEPTS or rejects
    const int* inputs;     // sampler indices of the inputs, function after function
    int in_off[kFnMaxFunctions], n_in[kFnMaxFunctions];   // function c reads inputs[in_off[c] .. + n_in[c])
    double* pts[kFnMaxFunctions];            // [W][n_in[c]] the inputs of function c, point-major
    const double* ll_new[kFnMaxFunctions];   // [W] what function c returned for the trial to accept
    double* ll_c;          // [n_fn][W] the carried per-function log-likelihoods of the state
};

}  // namespace mcmc

// the launchers of function_kernels.hip: declared here alone, for the kernels' translation unit
// and the host side
extern "C" hipError_t mcmc_hip_launch_fn_walker(const mcmc::FnWalkerArgs* a, int accept, int propose,
                                                hipStream_t st);
extern "C" hipError_t mcmc_hip_launch_fn_blocked_walker(const mcmc::FnBlockedArgs* a, int accept,
                                                        int propose, hipStream_t st);
