// Kernel arguments of stretch_kernels.hip (shared with capi_stretch.hip).
#pragma once
#include "function_args.h"

namespace mcmc {

// ---- the affine-invariant stretch move on a function target (stretch_kernels.hip; DESIGN.md
// section 2, "Stretch move"): one step is two HALF-UPDATES, h = 0 then h = 1.  A group of
// `group_size` walkers is two halves (l < group_size / 2: half 0); in half-update h the walkers of
// half h move, each towards or away from a partner drawn from the OTHER half of its own group.
// The W / 2 active walkers of a half-update are counted k = 0 .. W / 2 - 1 in ascending walker
// order: k = g (group_size / 2) + m  <->  walker g group_size + h group_size / 2 + m.  Everything a
// trial carries from its propose half to its accept half is indexed by k.
constexpr uint32_t kStreamStretch = 0x2000u;   // word 1 of the Philox counter (det_math.h: the streams)
struct StretchArgs {
    StepArgs s;            // state, prior constants (cblock, ConstLayout{d, 0}), keys;
                           // s.step0 = the step of the half-update PROPOSED by this launch
    int d;
    int half_accept;       // the half whose trial this launch accepts or rejects (ACCEPT)
    int half_propose;      // the half this launch proposes for (PROPOSE); its partners are the other half
    int log2_half;         // log2(group_size / 2): 5, 6 or 7
    double a;              // the stretch scale, z in [1 / a, a]
    double dm1;            // (double)(d - 1): the power of z in the accept rule
    uint32_t norm_mask4[4];   // one bit per dimension with a normal prior
    double* points;        // [W / 2][d] trial points, point-major (the function's input)
    double* lp_t;          // [W / 2] log-prior of the trial, -inf outside the support
    double* Ea;            // [W / 2] Exp(1) variate of the accept test
    double* q;             // [W / 2] (d - 1) log z, the untempered Jacobian term of the accept test
    const double* ll_t;    // [W / 2] what the function returned for the trial
    int* bad;              // [1] 1 + global id of the first walker whose value INSIDE the support
                           // was NaN or +inf (0: none)
};

}  // namespace mcmc

// the launcher of stretch_kernels.hip: declared here alone, for the kernel's translation unit and
// the host side
extern "C" hipError_t mcmc_hip_launch_stretch(const mcmc::StretchArgs* a, int accept, int propose,
                                              hipStream_t st);
