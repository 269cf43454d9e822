// pitch_coarse.h -- f0_to_coarse on the device, shared by the pitch-embedding kernels (vits_elem.hip: embed_pitch_kernel; sweep.hip:
// sweep_embed_kernel): one definition, so a key of the sweep lands in the bin the solo path gives the same fp32 pitch.
#pragma once

// vits/utils.py:20-33 in fp32, same operation order as the torch path.
__device__ __forceinline__ int f0_to_coarse_dev(float f0) {
    // f0_mel_min and (f0_mel_max - f0_mel_min) are float64 Python scalars in the reference
    // (utils.py:16-17), rounded to fp32 when they meet the fp32 tensor: 77.75496616579426, 986.6532669978451.
    const float mel_min = 77.75496616579426f;
    const float mel_span = 986.6532669978451f;
    float mel = 1127.0f * logf(1.0f + f0 / 700.0f);
    if (mel > 0.f) mel = (mel - mel_min) * 254.0f / mel_span + 1.0f;
    // the clamp, written so that it also holds for what the reference's comparisons let through: f0 < -700 or NaN gives mel = NaN, every
    // compare with NaN is false and (int)NaN is undefined -- `!(mel > 1)` sends it to bin 1 (unvoiced) instead of an arbitrary table row
    if (!(mel > 1.f)) mel = 1.f;
    if (mel > 255.f) mel = 255.f;
    return (int)(mel + 0.5f);
}
