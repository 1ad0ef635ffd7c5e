// libmcmc_hip.so: the test entry of the device-math probe (math_probe_kernels.hip).  Needs no
// context: host pointers in and out, its own allocation, copies and one launch per call, on the
// current device -- like mcmc_hip_accept_estimate_error.
#include "../../include/mcmc_hip.h"
#include "math_probe.h"

int mcmc_hip_math_probe(int32_t fn, const uint64_t* args, uint64_t first, uint64_t stride, int64_t n,
                        uint64_t* out)
{
    int n_in = 0, n_out = 0;
    if (!mcmc_hip_math_probe_words(fn, &n_in, &n_out)) return MCMC_HIP_ERR_ARG;
    if (!out || n < 0 || n > MCMC_HIP_PROBE_MAX_ELEMENTS) return MCMC_HIP_ERR_ARG;
    if (!args && n_in != 1) return MCMC_HIP_ERR_ARG;   // only a one-word argument can be generated
    if (n == 0) return MCMC_HIP_OK;
    const size_t in_bytes = sizeof(uint64_t) * (size_t)n * (size_t)n_in;
    const size_t out_bytes = sizeof(uint64_t) * (size_t)n * (size_t)n_out;
    uint64_t* din = nullptr;
    uint64_t* dout = nullptr;
    hipError_t r = hipMalloc(&dout, out_bytes);
    if (r == hipSuccess && args) r = hipMalloc(&din, in_bytes);
    if (r == hipSuccess && args) r = hipMemcpy(din, args, in_bytes, hipMemcpyHostToDevice);
    if (r == hipSuccess) r = mcmc_hip_launch_math_probe(fn, din, first, stride, n, dout, nullptr);
    if (r == hipSuccess) r = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return r == hipSuccess ? MCMC_HIP_OK : MCMC_HIP_ERR_DEVICE;
}
