// resample.hip -- any-rate wav input: PCM decode, channel downmix and rational resampling to the model rate in ONE launch
// (whisper/audio.py:24-26, librosa.load(file, sr=16000), as svcmi.whisper.audio.load_audio does it on the host: scipy's
// polyphase filter).  In: the interleaved PCM frames exactly as the file holds them (half the upload of a float32 copy for int16);
// out: mono float32 at the new rate.  The filter is evaluated directly in its polyphase form
//     c = m * down + half,  p = c mod up,  j = c div up,     y[m] = sum_{k < K} x[j - k] * taps[p * K + k],   x = 0 outside [0, frames)
// with fmaf in ascending k, so an output's bits depend on nothing but its index: not on the tile, not on the grid, not on where the
// taps are read from.
// A 256-thread block owns `tile` consecutive outputs.  Their inputs are the contiguous span x[j(m0) - (K - 1) .. j(m_last)]: the block
// decodes and downmixes it into LDS once (a sample is decoded once, not K times), together with the whole tap image when that fits
// (44.1 kHz -> 16 kHz: 160 phases x 56 taps = 35 KB; every block of a clip needs every phase).  The LDS phase stride is K | 1: with the even
// K = 56 the 32 lanes of an LDS access group, which sit on 32 different phases, would hit only 4 banks.  An image that does not fit
// (47999 Hz -> 16 kHz: 16000 phases) is read from global memory, where L2 holds the few rows a tile touches.
// The arithmetic is ~9 MFLOP for a 10 s clip: the kernel is launch- and latency-bound, what it buys is the host's resampling
// milliseconds and the single upload.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int RS_TILE = 1024;       // outputs per block (fewer where the input span of 1024 would not fit)
constexpr int RS_SPAN = 4096;       // decoded input samples per block in LDS: 16 KB
constexpr int RS_TAPS = 14336;      // tap image in LDS, padded phase stride included: 56 KB (11.025 kHz -> 16 kHz: 640 x 21 = 13440)

// frame g of the file as load_audio computes it: every channel to float32, summed in channel order, divided by the channel count
// (numpy's float32 mean(axis=1): a true division, not a reciprocal multiply)
__device__ __forceinline__ float pcm_sample(const void* pcm, int fmt, long long i) {
    switch (fmt) {
    case 1: return (float)static_cast<const short*>(pcm)[i] / 32768.0f;
    case 2: return (float)static_cast<const int*>(pcm)[i] / 2147483648.0f;
    case 3: return ((float)static_cast<const unsigned char*>(pcm)[i] - 128.0f) / 128.0f;
    default: return static_cast<const float*>(pcm)[i];
    }
}

__device__ __forceinline__ float pcm_frame(const void* pcm, int fmt, int channels, long long g) {
    const long long b = g * channels;
    float s = pcm_sample(pcm, fmt, b);
    if (channels > 1) {
        for (int c = 1; c < channels; ++c) s += pcm_sample(pcm, fmt, b + c);
        s = s / (float)channels;
    }
    return s;
}

__global__ __launch_bounds__(TPB) void pcm_resample_kernel(const void* pcm, int fmt, int channels, long long frames, const float* taps,
                                                           int up, int down, int K, int half, float* out, long long n_out, int tile,
                                                           int taps_in_lds) {
    __shared__ float xs[RS_SPAN];
    __shared__ float ts[RS_TAPS];
    const int tid = threadIdx.x;
    if (!taps) {                       // same rate: decode + downmix only
        for (long long i = (long long)blockIdx.x * TPB + tid; i < n_out; i += (long long)gridDim.x * TPB) out[i] = pcm_frame(pcm, fmt, channels, i);
        return;
    }
    const long long m0 = (long long)blockIdx.x * tile;
    const int cnt = n_out - m0 < tile ? (int)(n_out - m0) : tile;
    const long long c0 = m0 * down + half;          // 64-bit: one hour of 44.1 kHz audio is past 2^31 here
    const long long jb = c0 / up;
    const int r0 = (int)(c0 - jb * up);
    const long long j_lo = jb - (K - 1);              // xs[i] = x[j_lo + i]
    int span = (int)(((long long)(cnt - 1) * down + r0) / up) + K;      // <= RS_SPAN by the host's choice of `tile`
    if (span > RS_SPAN) span = RS_SPAN;
    for (int i = tid; i < span; i += TPB) {
        const long long g = j_lo + i;
        xs[i] = (g >= 0 && g < frames) ? pcm_frame(pcm, fmt, channels, g) : 0.f;
    }
    const int kp = K | 1;
    if (taps_in_lds) {
        const int total = up * K;
        for (int i = tid; i < total; i += TPB) {
            const int p = i / K;
            ts[p * kp + (i - p * K)] = taps[i];
        }
    }
    __syncthreads();
    for (int o = tid; o < cnt; o += TPB) {
        const long long d = (long long)o * down + r0;
        const int jr = (int)(d / up);
        const int p = (int)(d - (long long)jr * up);
        const float* xr = xs + jr + (K - 1);          // x[j - k] = xr[-k]
        float acc = 0.f;
        if (taps_in_lds) {
            const float* tp = ts + p * kp;
            for (int k = 0; k < K; ++k) acc = fmaf(xr[-k], tp[k], acc);
        } else {
            const float* tp = taps + (long long)p * K;
            for (int k = 0; k < K; ++k) acc = fmaf(xr[-k], tp[k], acc);
        }
        out[m0 + o] = acc;
    }
}

}  // namespace

extern "C" int svcmi_pcm_resample_f32(const void* pcm, int32_t fmt, int32_t channels, int64_t frames, const float* taps, int32_t up,
                                      int32_t down, int32_t taps_per_phase, int32_t half, float* out, int64_t n_out, void* stream) {
    if (!pcm || !out || frames <= 0 || fmt < 0 || fmt > 3 || channels < 1 || channels > 8 || up < 1 || down < 1) return SVCMI_EINVAL;
    if (frames > (INT64_MAX - down) / up) return SVCMI_EINVAL;           // frames * up must not wrap
    if (n_out != (frames * up + down - 1) / down) return SVCMI_EINVAL;
    if (((uintptr_t)pcm & (fmt == 3 ? 0 : fmt == 1 ? 1 : 3)) || ((uintptr_t)out & 3) || ((uintptr_t)taps & 3)) return SVCMI_EALIGN;
    if (!taps) {
        if (up != 1 || down != 1) return SVCMI_EINVAL;
        long long nb = (n_out + TPB - 1) / TPB;
        if (nb > 4096) nb = 4096;
        SVCMI_LAUNCH(pcm_resample_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, pcm, fmt, channels, (long long)frames, taps, 1, 1, 0, 0, out,
                     (long long)n_out, 0, 0);
        return SVCMI_LAST_ERROR();
    }
    if (half < 0 || (long long)taps_per_phase != (2LL * half + up) / up) return SVCMI_EINVAL;      // ceil((2 * half + 1) / up)
    const int K = taps_per_phase;
    if (K > RS_SPAN) return SVCMI_EUNSUPPORTED;
    // the input span of a tile, ceil((tile - 1) * down / up) + K samples, has to fit the LDS buffer
    long long tile = RS_TILE;
    if (((tile - 1) * down + up - 1) / up + K > RS_SPAN) tile = (long long)(RS_SPAN - K) * up / down + 1;
    const long long nb = (n_out + tile - 1) / tile;
    if (nb > 0x7fffffffLL) return SVCMI_EUNSUPPORTED;
    const int in_lds = (long long)up * (K | 1) <= RS_TAPS;
    SVCMI_LAUNCH(pcm_resample_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, pcm, fmt, channels, (long long)frames, taps, up, down, K, half, out,
                 (long long)n_out, (int)tile, in_lds);
    return SVCMI_LAST_ERROR();
}
