// The probe of det_math.h (math_probe_kernels.hip): one function of the device math applied to an
// array of arguments, words in and words out, so that a test can compare it with the oracle bit for
// bit on a whole domain.  Declared here and not in kernels.h: nothing else depends on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// `fn` is one of MCMC_HIP_PROBE_* (include/mcmc_hip.h).  Words per element of function `fn`
// (0 for an unknown one):
extern "C" int mcmc_hip_math_probe_words(int fn, int* n_in, int* n_out);
// out[i * n_out + ..] = fn(in[i * n_in + ..]) for i < n; in == nullptr (n_in == 1 only): the
// argument of element i is first + i * stride.  hipErrorInvalidValue for an unknown fn.
extern "C" hipError_t mcmc_hip_launch_math_probe(int fn, const uint64_t* in, uint64_t first, uint64_t stride,
                                                 long long n, uint64_t* out, hipStream_t st);
