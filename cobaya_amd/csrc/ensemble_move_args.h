// Kernel arguments of ensemble_move_kernels.hip (shared with capi_stretch.hip).
#pragma once
#include "stretch_args.h"

namespace mcmc {

// ---- mixtures of ensemble moves on a function target (ensemble_move_kernels.hip; DESIGN.md
// section 2, "Ensemble move mixtures"): the half-updates, packing and trial buffers of StretchArgs;
// the KIND of a step -- stretch, differential evolution or snooker -- is chosen on the host, once
// per step for the whole ensemble, and arrives as a launch argument.
enum EnsembleKind : int { kEnsembleStretch = 0, kEnsembleDE = 1, kEnsembleSnooker = 2 };
constexpr int kMaxEnsembleMoves = 8;          // members of a mixture
// word 1 of the Philox counter (det_math.h: the streams; stretch_args.h: 0x2000)
constexpr uint32_t kStreamMoveKind = 0x2001u; // the kind of step S: counter (0, 0x2001, S_lo, S_hi)
constexpr uint32_t kStreamDE = 0x2002u;       // partners and E_a of a DE trial; | 0x10: its normal variate
constexpr uint32_t kStreamSnooker = 0x2003u;  // partners z, z1 and E_a of a snooker trial; | 0x10: partner z2
constexpr uint32_t kStreamSecond = 0x10u;
struct EnsembleMoveArgs {
    StretchArgs st;        // st.a is not read; st.s.step0 = the step of the half-update PROPOSED
    int kind;              // EnsembleKind of the half-update this launch proposes
    double p0;             // stretch: a;  de: gamma0;  snooker: gamma_s
    double p1;             // de: sigma
};

}  // namespace mcmc

// the launcher of ensemble_move_kernels.hip; propose_kind < 0: no proposal (the last accept of a call)
extern "C" hipError_t mcmc_hip_launch_ensemble_move(const mcmc::EnsembleMoveArgs* a, int accept,
                                                    int propose_kind, hipStream_t st);
