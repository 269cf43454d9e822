// prior_sample.h -- the per-element arithmetic of the prior sample z = (m + n * exp(logs)) * mask (vits/models.py:51-52), shared by the
// two kernels that draw it (vits_elem.hip: sample_prior_kernel; sweep.hip: sweep_sample_prior_kernel): one definition of the expf call and
// of the multiply-add the compiler contracts, so a singer's rows carry the bits of the solo path.
#pragma once

// exp(logs): the one transcendental of the sample.  The singer sweep takes it once per element and reuses it for every row.
__device__ __forceinline__ float prior_scale(float logs) { return expf(logs); }

// *z = m + n * e inside the length, 0 past it
__device__ __forceinline__ void prior_sample_store(float* z, float m, float n, float e, bool valid) {
    const float v = m + n * e;
    *z = valid ? v : 0.f;
}
