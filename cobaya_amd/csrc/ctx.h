// The engine context and what every host translation unit of libmcmc_hip.so shares: error
// reporting, the timing regions, the per-dimension kernel lookups and the noted step kernel.
// Private to the library (the C ABI is include/mcmc_hip.h).  gfx950 only; no CPU fallback.
#pragma once
#include "../../include/mcmc_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

// the host side may find a launcher missing (a developer build of a few dimensions): there, and
// only there, the optional launchers are weak references (kernels.h: MCMC_HIP_OPTIONAL)
#define MCMC_HIP_HOST_SIDE 1
#include "kernels.h"
#include "huge_args.h"
#include "pliklite_args.h"
#include "function_args.h"
#include "stretch_args.h"
#include "ensemble_move_args.h"
#include "checkpoint_args.h"
#include "marginal_args.h"
#include "autocorr_args.h"
#include "bestfit_args.h"
#include "evidence_args.h"
#include "derived_args.h"
#include "importance_args.h"
#include "importance_hist_args.h"
#include "comm.h"
#include "inc_choice.h"
#include "readout.h"
#include "step_span.h"

MCMC_DECLARE_DIM(1) MCMC_DECLARE_DIM(2) MCMC_DECLARE_DIM(3) MCMC_DECLARE_DIM(4)
MCMC_DECLARE_DIM(5) MCMC_DECLARE_DIM(6) MCMC_DECLARE_DIM(7) MCMC_DECLARE_DIM(8)
MCMC_DECLARE_DIM(9) MCMC_DECLARE_DIM(10) MCMC_DECLARE_DIM(11) MCMC_DECLARE_DIM(12)
MCMC_DECLARE_DIM(13) MCMC_DECLARE_DIM(14) MCMC_DECLARE_DIM(15) MCMC_DECLARE_DIM(16)
MCMC_DECLARE_DIM(17) MCMC_DECLARE_DIM(18) MCMC_DECLARE_DIM(19) MCMC_DECLARE_DIM(20)
MCMC_DECLARE_DIM(21) MCMC_DECLARE_DIM(22) MCMC_DECLARE_DIM(23) MCMC_DECLARE_DIM(24)
MCMC_DECLARE_DIM(25) MCMC_DECLARE_DIM(26) MCMC_DECLARE_DIM(27) MCMC_DECLARE_DIM(28)
MCMC_DECLARE_DIM(29) MCMC_DECLARE_DIM(30) MCMC_DECLARE_DIM(31) MCMC_DECLARE_DIM(32)

MCMC_DECLARE_BIG(48) MCMC_DECLARE_BIG(56) MCMC_DECLARE_BIG(64) MCMC_DECLARE_BIG(72)
MCMC_DECLARE_BIG(80) MCMC_DECLARE_BIG(88) MCMC_DECLARE_BIG(96) MCMC_DECLARE_BIG(100)
MCMC_DECLARE_BIG(112) MCMC_DECLARE_BIG(120) MCMC_DECLARE_BIG(128)

MCMC_DECLARE_PAIR(33) MCMC_DECLARE_PAIR(34) MCMC_DECLARE_PAIR(35) MCMC_DECLARE_PAIR(36)
MCMC_DECLARE_PAIR(37) MCMC_DECLARE_PAIR(38) MCMC_DECLARE_PAIR(39) MCMC_DECLARE_PAIR(40)
MCMC_DECLARE_PAIR(41) MCMC_DECLARE_PAIR(42) MCMC_DECLARE_PAIR(43) MCMC_DECLARE_PAIR(44)
MCMC_DECLARE_PAIR(45) MCMC_DECLARE_PAIR(46) MCMC_DECLARE_PAIR(47) MCMC_DECLARE_PAIR(48)
MCMC_DECLARE_PAIR(49) MCMC_DECLARE_PAIR(50) MCMC_DECLARE_PAIR(51) MCMC_DECLARE_PAIR(52)
MCMC_DECLARE_PAIR(53) MCMC_DECLARE_PAIR(54) MCMC_DECLARE_PAIR(55) MCMC_DECLARE_PAIR(56)

using mcmc::BigKernels;
using mcmc::ConstLayout;
using mcmc::DimKernels;

constexpr int kMaxDimBig = 128;  // basis_big_kernel keeps H (d*d doubles) in 160 KiB of LDS

// smallest compiled padded size that serves dimension d (32 < d <= 128)
inline const BigKernels* big_for_dim(int d)
{
    typedef const BigKernels* (*getter)();
    static const getter table[] = {mcmc_hip_big_48,  mcmc_hip_big_56,  mcmc_hip_big_64,
                                   mcmc_hip_big_72,  mcmc_hip_big_80,  mcmc_hip_big_88,
                                   mcmc_hip_big_96,  mcmc_hip_big_100, mcmc_hip_big_112,
                                   mcmc_hip_big_120, mcmc_hip_big_128};
    static_assert(sizeof(table) / sizeof(table[0]) == sizeof(mcmc::kBigDps) / sizeof(mcmc::kBigDps[0]), "");
    if (d <= mcmc::kMaxDimLane || d > kMaxDimBig) return nullptr;
    for (getter g : table)
        if (g != nullptr && g()->dp >= d) return g();
    return nullptr;
}

// the launcher of the two-wave step kernel of a dimension 32 < d <= kMaxDimPair, if compiled
inline mcmc::PairStep pair_for_dim(int d)
{
    static const mcmc::PairStep table[] = {mcmc_hip_pair_33, mcmc_hip_pair_34, mcmc_hip_pair_35,
                                   mcmc_hip_pair_36, mcmc_hip_pair_37, mcmc_hip_pair_38,
                                   mcmc_hip_pair_39, mcmc_hip_pair_40, mcmc_hip_pair_41,
                                   mcmc_hip_pair_42, mcmc_hip_pair_43, mcmc_hip_pair_44,
                                   mcmc_hip_pair_45, mcmc_hip_pair_46, mcmc_hip_pair_47,
                                   mcmc_hip_pair_48, mcmc_hip_pair_49, mcmc_hip_pair_50,
                                   mcmc_hip_pair_51, mcmc_hip_pair_52, mcmc_hip_pair_53,
                                   mcmc_hip_pair_54, mcmc_hip_pair_55, mcmc_hip_pair_56};
    static_assert(sizeof(table) / sizeof(table[0]) == mcmc::kMaxDimPair - mcmc::kMaxDimLane, "");
    if (d <= mcmc::kMaxDimLane || d > mcmc::kMaxDimPair) return nullptr;
    return table[d - mcmc::kMaxDimLane - 1];
}

inline const DimKernels* kernels_for_dim(int d)
{
    typedef const DimKernels* (*getter)();
    static const getter table[33] = {
        nullptr,          mcmc_hip_dim_1,  mcmc_hip_dim_2,  mcmc_hip_dim_3,  mcmc_hip_dim_4,
        mcmc_hip_dim_5,   mcmc_hip_dim_6,  mcmc_hip_dim_7,  mcmc_hip_dim_8,  mcmc_hip_dim_9,
        mcmc_hip_dim_10,  mcmc_hip_dim_11, mcmc_hip_dim_12, mcmc_hip_dim_13, mcmc_hip_dim_14,
        mcmc_hip_dim_15,  mcmc_hip_dim_16, mcmc_hip_dim_17, mcmc_hip_dim_18, mcmc_hip_dim_19,
        mcmc_hip_dim_20,  mcmc_hip_dim_21, mcmc_hip_dim_22, mcmc_hip_dim_23, mcmc_hip_dim_24,
        mcmc_hip_dim_25,  mcmc_hip_dim_26, mcmc_hip_dim_27, mcmc_hip_dim_28, mcmc_hip_dim_29,
        mcmc_hip_dim_30,  mcmc_hip_dim_31, mcmc_hip_dim_32};
    if (d < 1 || d > 32 || table[d] == nullptr) return nullptr;
    return table[d]();
}

inline std::string g_create_error;

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t resize(size_t count)
    {
        if (count <= n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void**)&p, sizeof(T) * count);
        if (e == hipSuccess) n = count;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

struct mcmc_hip_ctx {
    mcmc_hip_config cfg{};
    const DimKernels* k = nullptr;    // d <= 32: lane-per-walker kernels of that dimension
    const BigKernels* kb = nullptr;   // 32 < d <= 128: column-sweep / matrix-core kernels
    mcmc::PairStep kp = nullptr;   // 32 < d <= 56: the two-wave step kernel, if compiled
    bool huge = false;                // 128 < d <= 256: huge_kernels.hip (incremental, one block, K <= 4)
    // huge: the Haar columns of one cycle of every basis group ([BG][d][d]), the basis scratch, and
    // the per-step direction columns of a launch ([BG][n][huge_col_stride])
    DevBuf<double> hV, hScratch, hCols;
    unsigned long long hV_cycle = ~0ull, hV_epoch = ~0ull;
    hipStream_t stream = nullptr;
    std::string err;
    int d = 0, W = 0, G = 0, gs = 0, K = -1;
    bool have_prior = false, have_target = false, have_cov = false, have_state = false;
    // host copies of the problem
    std::vector<int32_t> kind, periodic;
    std::vector<double> lo, hi, loc, scale, mls;
    double uniform_logp = 0.0;
    uint32_t norm_mask = 0, periodic_mask = 0;
    uint32_t norm_mask4[4] = {0, 0, 0, 0};
    bool any_periodic = false;
    std::vector<double> mean, Linv, cnorm, weight;  // Linv: [K][d*d] row-major
    std::vector<double> cov, T;                     // proposal
    // parameter blocks (proposal.py:96-196); blocked == false: one block, identity order
    bool blocked = false;
    std::vector<int32_t> blk_size, blk_over, i_of_j;
    int drag_last_slow = -1, drag_steps = 0;
    DevBuf<int> dblk, vflag, vflag_f;               // dblk: size | oversample | i_of_j
    DevBuf<double> Vf;                              // dragging: directions of the fast blocks
    DevBuf<double> drag_cs;                         // drag_general_kernel: start points [d][W]
    std::vector<double> shift;                      // moment shift
    // device
    DevBuf<double> x, logpost, logprior, loglike, cblock, dT, V, rows, gsum, Sg, pooled, dshift;
    DevBuf<double> ex, elp, ell, eder, escratch, dLrow, dLcol;
    // incremental evaluation (MCMC_HIP_FLAG_INCREMENTAL): carried y, per-step (v, u) pairs,
    // padded prior constants, row-major L^-1 and the mean of the one mode
    bool incremental = false;
    bool y_valid = false;
    bool own_basis = false;     // MCMC_HIP_FLAG_OWN_BASIS (d > 1): a Haar basis per walker
    // incremental mode: walkers sharing one Haar basis (a multiple of group_size, flags bits
    // 8..11 = log2 of the multiple); the R-1 groups (moments) stay group_size wide
    int bgs = 0, BG = 0;
    DevBuf<double> y, inc_prior, inc_Lrow, inc_mean;
    // mixtures on the kernels that carry the log-density of every mode (inc_choice.h: IncChoice::carry_modes):
    // amode[K][W]; valid = written by a launch (or set) since y was; else re-anchored on y
    DevBuf<double> amode;
    bool amode_valid = false;
    // The directions of a launch -- Haar columns V (Vf: the fast blocks' when dragging) and their
    // whitened pairs VU -- do not depend on the walkers' state, so the set of the NEXT launch is
    // computed on a second stream while the step kernel of this one runs (two sets, used in
    // turn).  A set computed ahead is used only if the launch that comes is the one predicted
    // (same first step, same length) and nothing the directions depend on has been set since
    // (dir_epoch); otherwise it is recomputed on the main stream.
    struct DirSet {
        DevBuf<double> V, Vf, VU;
        DevBuf<int> vflag, vflag_f, colflag;   // colflag: 1-D columns of the launch, in VU order
        bool has_flags = false;
        DevBuf<double> UU;                   // |u|^2 of the columns (step_inc_kernel: one mode, no periodic parameter)
        DevBuf<double> VW, NL;               // the carried log-prior's stream and (v.w, loc.w) of the columns
        hipEvent_t ready = nullptr;          // recorded on the stream that filled the set
        bool ahead = false;                  // filled ahead of its launch (on stream2)
        unsigned long long step0 = ~0ull, epoch = 0;
        int n = 0;
    } dirs[2];
    int dir_cur = 0;
    unsigned long long dir_epoch = 0;
    hipStream_t stream2 = nullptr;
    hipEvent_t mark = nullptr;               // main stream: behind the last step kernel
    bool mark_valid = false;
    bool prefetch = true;
    // the directions of the launch a call BEGINS with are formed at that call, not at the end of
    // the previous one (capi_incremental.hip: acquire_direction_set): a proposal refreshed in between is then in them at once
    bool lazy_dirs = true;
    // step_inc_kernel: calls whose directions are formed together (MCMC_HIP_LOOKAHEAD, default 4)
    int lookahead = 4;
    // bytes of directions a span of mcmc_hip_step may hold (MCMC_HIP_DIR_BUDGET_KIB; 0: the stepper's default)
    size_t dir_budget = 0;
    // incremental_duo.hip (two lanes per walker): -1 = where the ensemble fills the chip with it
    // (kDuoMinWalkers), 0 = never, 1 = wherever the kernel serves the model (MCMC_HIP_DUO)
    int duo = -1;
    // IncStepArgs::accept_slack of the one-mode two-lane kernel (MCMC_HIP_ACCEPT_SLACK; inf: every step exact)
    double accept_slack = mcmc::kAcceptSlack;
    hipEvent_t T_event = nullptr;            // main stream: behind the last write of dT
    bool T_fresh = false;                    // ... which no direction set has been ordered behind yet
    // asynchronous checkpoint (mcmc_hip_request_moments / mcmc_hip_fetch_moments) and
    // stream-ordered proposal refresh: pinned host staging
    double* pin_mom = nullptr;                      // [G*d + d(d+1)/2 + 2]
    unsigned long long* pin_mom_dev = nullptr;      // the device's alias of pin_mom (readout_moments_kernel stores there)
    double* pin_T = nullptr;                        // ring of 4 transforms [4][d*d]
    int pin_T_slot = 0;
    hipEvent_t pin_T_done[4] = {nullptr, nullptr, nullptr, nullptr};   // the copy out of slot k has run
    hipEvent_t mom_event = nullptr;
    bool mom_pending = false;
    bool mom_fn = false;                            // the pending read-out carries a function target's error flag
    int64_t mom_n = 0;
    unsigned long long mom_step = 0;
    // drain_samples_pinned: ring of pinned host slots the packed rows are copied into (PCIe at
    // full rate, and the caller reads them in place)
    struct HostSlot { double* p = nullptr; size_t cap_rows = 0; };
    std::vector<HostSlot> slots = std::vector<HostSlot>(4);
    int slot_next = 0;
    DevBuf<double> pack_out;                        // drain_samples: packed rows
    DevBuf<long long> pack_off;
    DevBuf<int> weight_i, prej, burn, stuck, nrows;
    DevBuf<int> thin_acc;   // thinned emission (mcmc_hip_set_emit_thin): the weight a walker has added up
    int emit_thin = 1;
    DevBuf<long long> nacc;
    DevBuf<unsigned long long> acc_total;
    unsigned long long step = 0;
    int64_t n_snapshots = 0;
    // timing
    bool timing = false;
    struct Ev {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    // kinds 0..2: step kernels / directions / moment snapshots; 3..5: the three kernels of a
    // step on the binned target (pl_walker, pl_residual, pl_chi2), each launch timed
    double ms[6] = {0, 0, 0, 0, 0, 0};
    int64_t n_seen[6] = {0, 0, 0, 0, 0, 0}, n_timed[6] = {0, 0, 0, 0, 0, 0};   // timed regions per kind (Timed)
    int64_t n_step_launches = 0;
    std::string last_step_kernel;     // what the last step launcher said it launched
    // device-side learn / convergence checkpoint (checkpoint_kernels.hip)
    struct Ckpt {
        DevBuf<double> ring, wsum, payload, ws, out;
        DevBuf<unsigned long long> acc_prev;
        int cap = 0;               // ring slots
        long long n_done = 0;      // checkpoints taken so far (the next one goes to slot n_done % cap)
        double* pin_out = nullptr; // [8 + 2 d^2 + d]: the solve's outcome, or the reduced payload
        hipEvent_t ev = nullptr;
        bool begun = false, pending = false;
        bool payload_only = false; // the pending read-out is the payload (checkpoint_request_payload)
    } ck;
    // R-1 of the confidence bounds (mcmc.py:918-1002): ring of ensemble snapshots [slot][d][W]
    struct Bounds {
        DevBuf<double> ring, bounds, payload;
        int n_slots = 0;
        double* pin = nullptr;     // [1 + 4 d + G d 2]
    } bd;
    // The six device products.  Each keeps its slab of 64-bit words, the pinned read-out and the
    // request / fetch / set state in `ro` (readout.h: the life cycle, once) and here only what is its
    // own; release(): back to "not configured" (ro.slab == nullptr), the event stays for the next
    // configure; mcmc_hip_destroy ends each with release() and ro.destroy().
    //
    // streaming marginal histograms (mcmc_hip_marginals_*; marginal_kernels.hip): the slab
    // [1-D entries: under, over, bins1 | pairs: outside, bins2 x bins2]
    struct Marginals {
        Readout ro;
        DevBuf<mcmc::MargEntry> entries;
        size_t off_pairs = 0;
        int n1 = 0, n2 = 0, bins1 = 0, bins2 = 0, n_entries = 0, lds_words = 0;
        void release()
        {
            ro.release();
            entries.release();
            off_pairs = 0;
            n1 = n2 = bins1 = bins2 = n_entries = lds_words = 0;
        }
    } mg;
    // lagged cross-products for the autocorrelation time (mcmc_hip_autocorr_*; autocorr_kernels.hip):
    // the ring of the last lags + 1 snapshots with their group sums and the slab of doubles
    // [3][lags + 1][n] (P, A, B).  It counts pairs per lag, on the host, not accumulations
    struct AutoCorr {
        Readout ro;
        DevBuf<double> ring, ringS, Pg;
        DevBuf<int> dims;
        int n = 0, lags = 0, rows_per_pass = 0;
        int held = 0;                          // snapshots the ring holds (<= lags + 1)
        int head = 0;                          // slot of the NEXT snapshot
        std::vector<int64_t> n_pairs, pend_pairs;   // [lags + 1]: open, of the pending read-out
        void release()
        {
            ro.release();
            ring.release(); ringS.release(); Pg.release(); dims.release();
            n = lags = rows_per_pass = held = head = 0;
            n_pairs.clear(); pend_pairs.clear();
        }
    } ac;
    // best fit, MAP and profile likelihoods (mcmc_hip_bestfit_*; bestfit_kernels.hip): the slab of
    // keys [n][bins] | the two records [2][6 + d] (key, walker, step, logpost, logprior, loglike,
    // x[d] as 64-bit words) at word n_slab, and the slices' candidates
    struct BestFit {
        Readout ro;
        DevBuf<unsigned long long> cand;
        DevBuf<mcmc::BfEntry> entries;
        size_t n_slab = 0, n_rec = 0;
        int n = 0, bins = 0, quantity = 0;
        void release()
        {
            ro.release();
            cand.release(); entries.release();
            n_slab = n_rec = 0;
            n = bins = quantity = 0;
        }
    } bf;
    // evidence of the run (mcmc_hip_evidence_*; evidence_kernels.hip): the slab
    // acc[G][n_r] doubles | cnt[G][n_r] uint64 | clamped uint64 | the key of c, the active ellipsoid
    // m[d] | Linv[d][d] on the device, the staged one in pinned memory until a closing request
    // uploads it in stream order; host copies of both travel with every read-out
    struct Evidence {
        Readout ro;                            // [2 G n_r + 2]
        DevBuf<double> ell, s;                 // [d + d d], [W]
        double* pin_ell = nullptr;             // [d + d d] the ellipsoid on its way to the device
        std::vector<double> active, staged;    // [d + d d] each (empty: none)
        std::vector<double> pend_active, pend_staged;   // ... as they were at the pending request
        double r2[mcmc::kEvMaxRadii] = {};
        int n_r = 0;
        void release()
        {
            ro.release();
            ell.release(); s.release();
            if (pin_ell) (void)hipHostFree(pin_ell);
            pin_ell = nullptr;
            active.clear(); staged.clear(); pend_active.clear(); pend_staged.clear();
            n_r = 0;
        }
    } evd;
    // derived parameters (mcmc_hip_derived_*; derived_kernels.hip): the rows z[m][W] the caller fills
    // on the engine's stream, this accumulation's group chains, and the slab
    // N | S[m][n_col] doubles | bad[m] | kmax[m] | kmin[m] (derived_args.h)
    struct Derived {
        Readout ro;
        DevBuf<double> z, Sg, shift;           // [m][W], [G][m][n_col], [m]
        DevBuf<unsigned long long> Ng;         // [G]
        DevBuf<int> cross;                     // [n_cross]
        int m = 0, n_cross = 0, n_col = 0;
        int gs = 0, G = 0;                     // the groups of the sums (default: the engine's)
        void release()
        {
            ro.release();
            z.release(); Sg.release(); shift.release(); Ng.release(); cross.release();
            m = n_cross = n_col = gs = G = 0;
        }
    } dv;
    // importance reweighting (mcmc_hip_importance_*; importance_kernels.hip): the slab
    // sums (alternative k at off[k]: [G][n_chains_k] doubles) | n[n_alt][G] | counters[n_alt][3] | the
    // keys of c [n_alt].  The log-weights live with the caller.
    // The reweighted marginal histograms (mcmc_hip_importance_hist_*; importance_hist_kernels.hip) are a
    // second slab, `hist`: per alternative with histograms, ascending, lo[n_counters] | hi[n_counters]
    // (the words of 128-bit counters in the layout of the marginals slab), behind them saturated[n_hist].
    // Its intervals are the sums': it is copied out and zeroed by the same request, behind the same event
    // (`ro.ev`); of `hist` only the slab, the mirror, `pending` and `pend_n` are in use
    struct Importance {
        Readout ro, hist;
        DevBuf<unsigned long long> q;          // [n_hist][W] the quantised weights of an accumulation
        size_t n_sums = 0, n_counters = 0;
        unsigned long long off[mcmc::kImMaxAlt] = {};
        int cov[mcmc::kImMaxAlt] = {};
        int hist_on[mcmc::kImMaxAlt] = {};     // per alternative
        int hist_alt[mcmc::kImMaxAlt] = {};    // the alternative of histogram set h
        int n_alt = 0, n_hist = 0;
        int gs = 0, G = 0;                     // the groups of the sums (default: the engine's)
        void release_hist()
        {
            hist.release();
            q.release();
            n_counters = 0;
            n_hist = 0;
            for (int k = 0; k < mcmc::kImMaxAlt; ++k) hist_on[k] = hist_alt[k] = 0;
        }
        void release()
        {
            ro.release();
            release_hist();
            n_sums = 0;
            n_alt = gs = G = 0;
        }
    } imp;
    // the walker shards' communicator (comm.hip; not owned): the device checkpoint all-reduces
    // its payload over it in stream order
    mcmc_hip_comm* comm = nullptr;
    // binned-bandpower Gaussian target (planck_pliklite.py:143-155; pliklite_kernels.hip)
    struct Binned {
        bool on = false;
        int n_bins = 0, KT = 0, ntw = 0, n_lin = 0, nlp = 0, calib = 0, lmax = 0;
        std::vector<int32_t> bins;                       // [n_bins][3]
        std::vector<double> Linv, Bc0, BJ;               // host copies (tests hand them to the oracle)
        DevBuf<double> resp, theta0, Astream, weights, X, bjs, es;   // bjs, es: pl_residual_mfma_kernel
        DevBuf<double> Afused;                           // pl_fused_kernel: half-tile streams of L^-1
        unsigned long long f_off[8][5][2];
        int f_pairs[8][5][2];
        int f_shift = 0, f_ng = 0;
        DevBuf<int> dbins;
        DevBuf<double> delta, trial, lp_t, Ea, psum;     // step scratch, W walkers
        DevBuf<double> edelta, etrial, elp, echi2, epsum, ecl, eA;   // evaluate scratch
        unsigned long long tile_off[8][5];
        int nk[8][5];
    } bg;
    // function target (mcmc_hip_set_target_function; function_kernels.hip): the user's batched
    // device function stands where the likelihood kernels of the other targets do
    struct Function {
        bool on = false;
        mcmc_hip_loglike_fn fn = nullptr;
        void* user = nullptr;
        DevBuf<double> points, lp_t, Ea, ll_t;   // step scratch: trial [W][d], its log-prior, E_a, the function's values
        DevBuf<int> bad;                         // [1] 1 + global id of the first walker with NaN / +inf inside the support
        // several functions over parameter blocks (mcmc_hip_set_target_functions; n_fn == 0: the one
        // function above): function c reads the sampled parameters inputs[c], in that order
        int n_fn = 0;
        mcmc_hip_loglike_fn fns[mcmc::kFnMaxFunctions] = {};
        void* users[mcmc::kFnMaxFunctions] = {};
        std::vector<int32_t> inputs[mcmc::kFnMaxFunctions];
        DevBuf<int> dinputs;                     // the inputs, function after function
        DevBuf<double> pts[mcmc::kFnMaxFunctions];   // step scratch: [W][d_c] the inputs of function c
        DevBuf<double> ll_new, ll_c;             // [n_fn][W]: what the functions returned; the carried values
        DevBuf<double> epts, ell;                // evaluate scratch: [n][d_c], [n]
        bool llc_valid = false;                  // ll_c belongs to the state (else: re-evaluated at the next launch)
        std::vector<double> last_eval;           // [n_fn][n] of the last mcmc_hip_evaluate (set_state keeps them)
        int last_eval_n = 0;
        unsigned long long sched_cycle = ~0ull, sched_epoch = ~0ull;
        std::vector<short> sched;                // block of every slot of cycle sched_cycle
    } fnt;
    // the move of mcmc_hip_step (mcmc_hip_set_move): Metropolis along Haar directions, or the stretch
    // move of stretch_kernels.hip on the single-function target.  With the default nothing below is
    // allocated or read
    struct Stretch {
        int kind = MCMC_HIP_MOVE_METROPOLIS;
        double a = 2.0;
        DevBuf<double> q;          // [W / 2] (d - 1) log z of the pending trials
        bool checked = false;      // the state in force has no half-group flat in a parameter
        bool broken = false;       // a callback failed between the half-updates: a state must be set again
    } mv;
    // the mixture of ensemble moves (mcmc_hip_set_moves; DESIGN.md section 2, "Ensemble move
    // mixtures"); n = 0: off.  It shares mv.q, mv.checked and mv.broken with the stretch move
    struct Mixture {
        int n = 0;
        int kind[mcmc::kMaxEnsembleMoves];
        double weight[mcmc::kMaxEnsembleMoves];        // normalised
        double p0[mcmc::kMaxEnsembleMoves], p1[mcmc::kMaxEnsembleMoves];
        unsigned long long below[mcmc::kMaxEnsembleMoves];   // member j is chosen by a word w0 < below[j] (and >= below[j - 1])
    } mx;
};

// the end of a device product (mcmc_hip_destroy): what it holds, then the event of its read-out
template <class P>
inline void destroy_product(P& p)
{
    p.release();
    p.ro.destroy();
}

// what the last step launcher said it was about to launch (mcmc_hip_note_step_kernel)
inline thread_local const char* g_noted_kernel = nullptr;

// keeps the noted kernel as the context's last step kernel, "<name> (<what>=<value>)"; value < 0:
// the dimension.  h == nullptr: the note is dropped (a launcher ran outside a step).
inline void take_noted_kernel(mcmc_hip_ctx* h, const char* what = "d", int value = -1)
{
    if (!g_noted_kernel) return;
    if (h)
        h->last_step_kernel = std::string(g_noted_kernel) + " (" + what + "=" +
                              std::to_string(value < 0 ? h->d : value) + ")";
    g_noted_kernel = nullptr;
}

inline int fail(mcmc_hip_ctx* h, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIP_TRY_ELSE(h, call, undo)                                                           \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            undo;                                                                             \
            return fail(h, MCMC_HIP_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                     \
    } while (0)
#define HIP_TRY(h, call) HIP_TRY_ELSE(h, call, (void)0)
// inside the configure of a device product P: a failure leaves it released, not half-built
#define HIP_TRY_BUILD(h, P, call) HIP_TRY_ELSE(h, call, (P).release())

inline hipEvent_t get_event(mcmc_hip_ctx* h)
{
    if (!h->pool.empty()) {
        hipEvent_t e = h->pool.back();
        h->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct Timed {
    mcmc_hip_ctx* h;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    bool on = false;
    // Every step kernel is timed; of the regions around it (kind 1: directions, kind 2: moment
    // snapshot) one in eight, scaled up in mcmc_hip_kernel_times: an event record is a packet
    // of its own between two dependent kernels (about 6 us each on the critical path).
    Timed(mcmc_hip_ctx* h_, int kind_, hipStream_t st_ = nullptr)
        : h(h_), kind(kind_), st(st_ ? st_ : h_->stream)
    {
        if (h->timing) {
            on = kind == 0 || kind >= 3 || (h->n_seen[kind] % 8) == 0;
            h->n_seen[kind] += 1;
        }
        if (on) {
            h->n_timed[kind] += 1;
            a = get_event(h);
            b = get_event(h);
            (void)hipEventRecord(a, st);
        }
    }
    ~Timed()
    {
        if (on) {
            (void)hipEventRecord(b, st);
            h->pending.push_back({a, b, kind});
        }
    }
};

inline void resolve_timing(mcmc_hip_ctx* h)
{
    for (auto& e : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) h->ms[e.kind] += ms;
        h->pool.push_back(e.a);
        h->pool.push_back(e.b);
    }
    h->pending.clear();
}

// ---- what every host stepper fills the same way ----
// The ensemble's part of a step kernel's arguments.  The directions (V, vflag, own_basis), the cycle
// geometry (cps, slab, ncyc), the steps (step0, n_steps), the emitted rows and their thinning, the
// modes (n_modes, cnorm0) and periodic_mask are the stepper's own: kernels test several of them
// against null or zero.
inline mcmc::StepArgs step_args(const mcmc_hip_ctx* h)
{
    mcmc::StepArgs a{};
    a.x = h->x.p; a.logpost = h->logpost.p; a.logprior = h->logprior.p;
    a.loglike = h->loglike.p; a.weight = h->weight_i.p; a.prior_rej = h->prej.p;
    a.burn_left = h->burn.p; a.n_accept = h->nacc.p; a.stuck = h->stuck.p;
    a.accept_total = h->acc_total.p;
    a.cblock = h->cblock.p; a.W = h->W; a.group_size = h->gs;
    a.norm_mask = h->norm_mask; a.walker0 = h->cfg.walker_offset;
    a.key0 = (uint32_t)h->cfg.seed; a.key1 = (uint32_t)(h->cfg.seed >> 32);
    a.uniform_logp = h->uniform_logp; a.temperature = h->cfg.temperature;
    a.max_tries = h->cfg.max_tries;
    return a;
}

// one bit per dimension d <= 128 with a normal prior / that is periodic, into a kernel's arguments
// (out: still zero)
inline void put_norm_mask4(const mcmc_hip_ctx* h, uint32_t out[4])
{
    std::copy(h->norm_mask4, h->norm_mask4 + 4, out);
}
inline void periodic_mask4(const mcmc_hip_ctx* h, uint32_t out[4])
{
    for (int i = 0; i < h->d; ++i)
        if (h->periodic[i]) out[i >> 5] |= 1u << (i & 31);
}

// cycles of directions per span (step_span.h): what the byte budget -- MCMC_HIP_DIR_BUDGET_KIB, or
// the stepper's default -- holds of slabs of `slab` doubles for n_groups bases, at least `least`
inline int max_span_cycles(const mcmc_hip_ctx* h, size_t default_bytes, size_t slab, int n_groups,
                           size_t least = 1)
{
    const size_t bytes = h->dir_budget ? h->dir_budget : default_bytes;
    return (int)std::max<size_t>(least, bytes / (sizeof(double) * slab * (size_t)n_groups));
}

// The Haar bases of cycles [c0, c0 + ncyc) of n_groups basis groups from global group group0 on,
// into V ([n_groups][ncyc][slab]), on stream st (blocked directions: blocked_basis)
inline int shared_basis(mcmc_hip_ctx* h, DevBuf<double>& V, int n_groups, uint32_t group0,
                        unsigned long long c0, int ncyc, size_t slab, hipStream_t st)
{
    HIP_TRY(h, V.resize((size_t)n_groups * ncyc * slab));
    mcmc::BasisArgs b{};
    b.T = h->dT.p; b.V = V.p;
    b.group0 = group0;
    b.cycle0 = (uint32_t)c0;
    b.key0 = (uint32_t)h->cfg.seed; b.key1 = (uint32_t)(h->cfg.seed >> 32);
    b.ncyc = ncyc;
    if (h->kb) HIP_TRY(h, h->kb->basis(b, n_groups, h->d, st));
    else HIP_TRY(h, h->k->basis(b, n_groups, st));
    return MCMC_HIP_OK;
}

// ---- what one host translation unit defines for the others ----
// capi.hip
// slots per cycle of the blocked proposer's three sequences (oracle: orc_block_slots)
int block_slots(const mcmc_hip_ctx* h, int which);
int upload_constants(mcmc_hip_ctx* h);
// capi_targets.hip: the binned Gaussian target and function targets
int step_binned(mcmc_hip_ctx* h, int n_steps);
int step_function(mcmc_hip_ctx* h, int n_steps);
int step_functions(mcmc_hip_ctx* h, int n_steps);
// several functions: component values [n_fn][n] of the host points x[n][d] (every function called)
int functions_evaluate(mcmc_hip_ctx* h, int n, const double* x, double* comps);
int evaluate_binned_points(mcmc_hip_ctx* h, int n, const double* x, double* logprior, double* loglike);
int function_call(mcmc_hip_ctx* h, int n, const double* points, double* loglike);
int function_target_error(mcmc_hip_ctx* h, int bad);
// word 0 of Philox4x32-10 (det_math.h: philox4x32_10), on the host: the slot shuffle decides which
// functions a step calls and the mixture of ensemble moves the kind of a step, so the host forms it too
inline uint32_t philox_w0(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// capi_stretch.hip: the stretch move, or a mixture of ensemble moves, on the single-function target
int step_stretch(mcmc_hip_ctx* h, int n_steps);
// capi_incremental.hip: incremental evaluation (d <= 128: step_incremental; above: step_huge)
int blocked_basis(mcmc_hip_ctx* h, int which, unsigned long long c0, int ncyc, int L, size_t slab,
                  DevBuf<double>& V, DevBuf<int>& flag, bool& any_1d, hipStream_t st = nullptr,
                  bool shared_schedule = false);
int step_huge(mcmc_hip_ctx* h, int n_steps);
int step_incremental(mcmc_hip_ctx* h, int n_steps);
// the kernel that serves this engine's incremental steps and what it carries (inc_choice.h);
// not served when the engine is not in incremental mode
mcmc::IncChoice inc_choice_of(const mcmc_hip_ctx* h);
