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

}  // namespace mcmc

// the launcher of function_kernels.hip: declared here alone, for the kernels' translation unit
// and the host side
extern "C" hipError_t mcmc_hip_launch_fn_walker(const mcmc::FnWalkerArgs* a, int accept, int propose,
                                                hipStream_t st);
