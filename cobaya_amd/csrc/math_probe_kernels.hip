// The probe of det_math.h: every function there that claims to be "a pure function of the input bits",
// applied to an array of arguments in a translation unit of its own, words in and words out, so that
// tests/test_gpu_math_domains.py can compare the device with the oracle (oracle/mcmc_oracle.c: the
// orc_*_bulk forms) bit for bit on whole argument domains.  det_math.h is included as the step kernels
// include it and nothing in it is edited; the two LDS tables are filled with short_log_load /
// exp_tab_load as the step kernels fill them.  (The copies the compiler inlines into the step kernels
// stay covered by the bit-exact step tests: this file tests the source-level function.)
#include "det_math.h"
#include "math_probe.h"
#include "../../include/mcmc_hip.h"

namespace mcmc {
namespace {

__device__ __forceinline__ double as_d(uint64_t w) { return __longlong_as_double((long long)w); }
__device__ __forceinline__ uint64_t as_w(double x) { return (uint64_t)__double_as_longlong(x); }

// One struct per probed function: words per element in and out, and the call itself.
struct ProbePhilox {
    static constexpr int kIn = 6, kOut = 4;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        const u32x4 q = philox4x32_10((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3],
                                      (uint32_t)a[4], (uint32_t)a[5]);
        r[0] = q.w0; r[1] = q.w1; r[2] = q.w2; r[3] = q.w3;
    }
};
struct ProbeU52 {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(u52(a[0]));
    }
};
struct ProbeDlog {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(dlog(as_d(a[0])));
    }
};
struct ProbeDexp {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(dexp(as_d(a[0])));
    }
};
struct ProbeSincos2pi {
    static constexpr int kIn = 1, kOut = 2;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        double sn, cs;
        sincos2pi(a[0], sn, cs);
        r[0] = as_w(sn); r[1] = as_w(cs);
    }
};
template <int B>
struct ProbeNegLogShort {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab lt, exp_tab)
    {
        r[0] = as_w(neg_log_short((uint32_t)a[0], B, lt));
    }
};
struct ProbeDlogTab {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab lt, exp_tab)
    {
        r[0] = as_w(dlog_tab(as_d(a[0]), lt));
    }
};
struct ProbeDexpTab {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab et)
    {
        r[0] = as_w(dexp_tab(as_d(a[0]), et));
    }
};
struct ProbeSqrtMidrange {
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(sqrt_midrange(as_d(a[0])));
    }
};
struct ProbeSqrt {   // what StepRng stage 15 and the Box-Muller radii use
    static constexpr int kIn = 1, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(sqrt(as_d(a[0])));
    }
};
struct ProbeDivBy {   // (a, w, R): R is the caller's RN(1 / w)
    static constexpr int kIn = 3, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(div_by(as_d(a[0]), as_d(a[1]), as_d(a[2])));
    }
};
struct ProbeDiv {
    static constexpr int kIn = 2, kOut = 1;
    static __device__ __forceinline__ void apply(const uint64_t* a, uint64_t* r, short_log_tab, exp_tab)
    {
        r[0] = as_w(as_d(a[0]) / as_d(a[1]));
    }
};

template <class F>
__global__ void __launch_bounds__(256) math_probe_kernel(const uint64_t* __restrict__ in, uint64_t first,
                                                         uint64_t stride, long long n, uint64_t* __restrict__ out)
{
    __shared__ dpair_t short_log_lds[SHORT_LOG_TABLE_SIZE];
    __shared__ double exp_lds[64];
    const short_log_tab lt = short_log_load(short_log_lds);
    const exp_tab et = exp_tab_load(exp_lds);
    __syncthreads();
    const long long step = (long long)gridDim.x * 256ll;
    for (long long i = (long long)blockIdx.x * 256ll + threadIdx.x; i < n; i += step) {
        uint64_t a[F::kIn], r[F::kOut];
        if (in) {
#pragma unroll
            for (int j = 0; j < F::kIn; ++j) a[j] = in[i * F::kIn + j];
        } else {
#pragma unroll
            for (int j = 0; j < F::kIn; ++j) a[j] = first + (uint64_t)i * stride;
        }
        F::apply(a, r, lt, et);
#pragma unroll
        for (int j = 0; j < F::kOut; ++j) out[i * F::kOut + j] = r[j];
    }
}

template <class F>
hipError_t launch(const uint64_t* in, uint64_t first, uint64_t stride, long long n, uint64_t* out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const long long want = (n + 255) / 256;
    const int blocks = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(math_probe_kernel<F>, dim3(blocks), dim3(256), 0, st, in, first, stride, n, out);
    return hipGetLastError();
}

// calls f.template operator()<F>() for the struct of `fn`; false for an unknown function
template <class Fn>
bool dispatch(int fn, Fn&& f)
{
    switch (fn) {
    case MCMC_HIP_PROBE_PHILOX: f.template operator()<ProbePhilox>(); return true;
    case MCMC_HIP_PROBE_U52: f.template operator()<ProbeU52>(); return true;
    case MCMC_HIP_PROBE_DLOG: f.template operator()<ProbeDlog>(); return true;
    case MCMC_HIP_PROBE_DEXP: f.template operator()<ProbeDexp>(); return true;
    case MCMC_HIP_PROBE_SINCOS2PI: f.template operator()<ProbeSincos2pi>(); return true;
    case MCMC_HIP_PROBE_NEG_LOG_SHORT_25: f.template operator()<ProbeNegLogShort<25>>(); return true;
    case MCMC_HIP_PROBE_NEG_LOG_SHORT_29: f.template operator()<ProbeNegLogShort<29>>(); return true;
    case MCMC_HIP_PROBE_DLOG_TAB: f.template operator()<ProbeDlogTab>(); return true;
    case MCMC_HIP_PROBE_DEXP_TAB: f.template operator()<ProbeDexpTab>(); return true;
    case MCMC_HIP_PROBE_SQRT_MIDRANGE: f.template operator()<ProbeSqrtMidrange>(); return true;
    case MCMC_HIP_PROBE_SQRT: f.template operator()<ProbeSqrt>(); return true;
    case MCMC_HIP_PROBE_DIV_BY: f.template operator()<ProbeDivBy>(); return true;
    case MCMC_HIP_PROBE_DIV: f.template operator()<ProbeDiv>(); return true;
    default: return false;
    }
}

struct Words {
    int n_in = 0, n_out = 0;
    template <class F> void operator()() { n_in = F::kIn; n_out = F::kOut; }
};
struct Launch {
    const uint64_t* in; uint64_t first, stride; long long n; uint64_t* out; hipStream_t st;
    hipError_t r = hipSuccess;
    template <class F> void operator()() { r = launch<F>(in, first, stride, n, out, st); }
};

}  // namespace
}  // namespace mcmc

extern "C" int mcmc_hip_math_probe_words(int fn, int* n_in, int* n_out)
{
    mcmc::Words w;
    if (!mcmc::dispatch(fn, w)) return 0;
    if (n_in) *n_in = w.n_in;
    if (n_out) *n_out = w.n_out;
    return 1;
}

extern "C" hipError_t mcmc_hip_launch_math_probe(int fn, const uint64_t* in, uint64_t first, uint64_t stride,
                                                 long long n, uint64_t* out, hipStream_t st)
{
    mcmc::Words w;
    if (!mcmc::dispatch(fn, w) || !out || (!in && w.n_in != 1)) return hipErrorInvalidValue;
    mcmc::Launch l{in, first, stride, n, out, st};
    mcmc::dispatch(fn, l);
    return l.r;
}
