// spectrogram.hip -- linear (STFT magnitude) spectrogram in ONE launch: the posterior-encoder input of every training item
// (prepare/preprocess_spec.py -> vits/spectrogram.py:41-76, spectrogram_torch with center=False):
//     xp[p]       = x[reflect(p - pad)],  p < n + 2 pad                            (F.pad(..., mode="reflect"), index arithmetic on the load)
//     re/im[k, t] = sum_{i < n_fft} xp[t hop + i] * basis[i, 2k / 2k + 1]          (window folded into the table: win_length < n_fft is free)
//     out[b, k, t] = sqrt(re^2 + im^2 + eps)                                       ([batch, bins, frames] contiguous, the layout the reference saves)
// The real DFT is a matrix product on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): K = n_fft, N = 2 bins, M = frames.
// A wave owns 32 frames x 16 bins.  The 32 frames are the instruction's COLUMNS (lane & 31), so the epilogue's stores run along
// `frames`: 128 contiguous bytes per half-wave.  The 32 ROWS are the 16 bins' (re, im) columns of the table in the order
//     row i -> bin 8 (i >> 4) + (i & 7),  part (i >> 3) & 1        (0 = cos, 1 = sin)
// because a lane holds rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of its column: rows i and i + 8 sit in the same lane, so re and im of
// a bin are acc[8 g + q] and acc[8 g + 4 + q] and the magnitude needs no exchange.  The lanes' table addresses are still 32 consecutive
// floats per half-wave (a permutation of one 128-byte run).
// A 256-thread block = 4 waves = 32 frames x 64 bins.  The block stages the padded sample span of its 32 frames, 31 hop + n_fft
// samples, into LDS once (at 1024 / 320 consecutive frames overlap 3.2x); all four waves read their frame operand from it.  Lane j
// reads sample j hop + c: with an even hop the 32 lanes of a ds_read_b32 group would share few banks (hop = 320: ONE), so sample s
// is stored at s + s / hop then (row stride hop + 1, odd: 32 different banks); an odd hop needs nothing.  A span that does not fit
// (31 hop + n_fft > ~12 K samples, e.g. 2048 / 512) is read from global memory with the same index arithmetic.  The table operand
// goes from L2 straight to registers, one float per lane and K-step, prefetched 8 K-steps ahead: the four waves of a block own
// different bins, so an LDS copy would have no second reader.  Blocks of one bin column are neighbours in the grid (blockIdx.x =
// frame tile), so the columns in flight are few and stay in L2.
// Determinism contract: out[b, k, t] is ONE accumulator chain over the K-steps (i = 0, 1), (2, 3), ... in ascending order, started
// from zero, then sqrtf(fmaf(re, re, fmaf(im, im, eps))).  No split-K, nothing data-dependent: the bits depend on the
// frame's n_fft padded samples and the table alone -- not on the tile the frame falls in (the tile decides the lane, not the
// arithmetic), the number of frames, the batch index, the stream, or whether the span came from LDS or global memory.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int SP_FRAMES = 32;                    // frames per block (the MFMA's columns)
constexpr int SP_BINS = 16;                      // bins per wave (x 2 table columns = the MFMA's rows)
constexpr int SP_WAVES = TPB / SVCMI_WAVE;
constexpr int SP_SPAN = 12288;                   // staged samples, skew included: 48 KB (1024 / 320: 10944 + 34)
constexpr int SP_U = 8;                          // K-steps of table prefetch (16 table rows)

// sample p of the reflect-padded signal; zero past its end (the unused tail of a block's span).  pad < n: one reflection is enough.
__device__ __forceinline__ float padded_sample(const float* x, long long n, int pad, long long p, long long total) {
    if (p >= total) return 0.f;
    long long s = p - pad;
    if (s < 0) s = -s;
    if (s >= n) s = 2 * (n - 1) - s;
    return x[s];
}

template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void linear_spectrogram_kernel(const float* x, long long x_bstride, long long n, const float* basis, int n_fft,
                                                                 int hop, int pad, float eps, float* out, long long frames, int skew) {
    __shared__ float xs[IN_LDS ? SP_SPAN : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const int bins = n_fft / 2 + 1;
    const long long t0 = (long long)blockIdx.x * SP_FRAMES;
    const float* xb = x + (long long)blockIdx.z * x_bstride;
    const long long total = n + 2LL * pad;
    if constexpr (IN_LDS) {
        const long long p0 = t0 * hop;
        const int span = (SP_FRAMES - 1) * hop + n_fft;               // + skew <= SP_SPAN: the host checked
        for (int s = tid; s < span; s += TPB) xs[s + skew * (s / hop)] = padded_sample(xb, n, pad, p0 + s, total);
        __syncthreads();
    }
    const int bin0 = ((int)blockIdx.y * SP_WAVES + wave) * SP_BINS;   // wave-uniform
    if (bin0 >= bins) return;                                         // after the only barrier

    // table operand: row i = idx of the instruction, K index khalf
    const int bin_a = bin0 + 8 * (idx >> 4) + (idx & 7), part = (idx >> 3) & 1;
    const long long ldb = 2LL * bins;
    const float* bp = basis + khalf * ldb + (bin_a < bins ? 2 * bin_a + part : 0);      // rows past the last bin: any valid column, never stored
    const long long kstride = 2 * ldb;
    const int nsteps = n_fft / 2;

    // frame operand: column j = idx, sample t hop + c with c = 2 ks + khalf
    int off = idx * hop + khalf + skew * (idx + khalf / hop), r = khalf % hop;           // LDS: position of sample (idx hop + c), c mod hop
    long long frame = t0 + idx;
    if (frame > frames - 1) frame = frames - 1;                                           // columns past the last frame: a valid one, never stored
    long long pg = frame * hop + khalf;                                                   // global: padded index

    auto next_sample = [&]() -> float {
        float b;
        if constexpr (IN_LDS) {
            b = xs[off];
            off += 2;
            if (skew) {                   // even hop (>= 2): at most one row boundary per step
                r += 2;
                if (r >= hop) { r -= hop; off += 1; }
            }
        } else {
            b = padded_sample(xb, n, pad, pg, total);
            pg += 2;
        }
        return b;
    };

    svcmi_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float a_cur[SP_U], a_nxt[SP_U];
#pragma unroll
    for (int u = 0; u < SP_U; ++u) a_cur[u] = bp[(long long)(u < nsteps ? u : nsteps - 1) * kstride];
    int ks = 0;
    for (; ks + SP_U <= nsteps; ks += SP_U) {
#pragma unroll
        for (int u = 0; u < SP_U; ++u) {
            int s = ks + SP_U + u;
            if (s > nsteps - 1) s = nsteps - 1;                       // clamped: always a valid row, no branch around the loads
            a_nxt[u] = bp[(long long)s * kstride];
        }
#pragma unroll
        for (int u = 0; u < SP_U; ++u) acc = svcmi_mfma_32x32x2(a_cur[u], next_sample(), acc);
#pragma unroll
        for (int u = 0; u < SP_U; ++u) a_cur[u] = a_nxt[u];
    }
    for (; ks < nsteps; ++ks) acc = svcmi_mfma_32x32x2(bp[(long long)ks * kstride], next_sample(), acc);

    // lane: frame t0 + idx, bins bin0 + 8 g + q + 4 khalf; re = acc[8 g + q], im = acc[8 g + 4 + q]
    const long long t = t0 + idx;
    if (t >= frames) return;
    float* ob = out + (long long)blockIdx.z * bins * frames + t;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bin = bin0 + 8 * g + q + 4 * khalf;
            const float re = acc[8 * g + q], im = acc[8 * g + 4 + q];
            if (bin < bins) ob[(long long)bin * frames] = sqrtf(fmaf(re, re, fmaf(im, im, eps)));
        }
    }
}

}  // namespace

extern "C" int svcmi_linear_spectrogram_f32(const float* x, int64_t x_bstride, int32_t batch, int64_t n, const float* basis, int32_t n_fft,
                                            int32_t hop, int32_t pad, float eps, float* out, int64_t frames, void* stream) {
    if (!x || !basis || !out || batch < 1 || hop < 1 || pad < 0 || n_fft < 2 || (n_fft & 1)) return SVCMI_EINVAL;
    if (n <= pad) return SVCMI_EINVAL;                                 // the reference's reflect pad raises too
    if (n + 2LL * pad < n_fft) return SVCMI_EINVAL;                    // frames < 1
    if (frames != 1 + (n + 2LL * pad - n_fft) / hop) return SVCMI_EINVAL;
    if (batch > 1 && x_bstride < n) return SVCMI_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)basis & 3) || ((uintptr_t)out & 3)) return SVCMI_EALIGN;
    const int bins = n_fft / 2 + 1;
    const long long tiles = (frames + SP_FRAMES - 1) / SP_FRAMES;
    const long long cols = (bins + SP_BINS * SP_WAVES - 1) / (SP_BINS * SP_WAVES);
    if (tiles > 0x7fffffffLL || cols > 65535 || batch > 65535) return SVCMI_EUNSUPPORTED;
    const int skew = (hop & 1) ? 0 : 1;
    const long long span = (long long)(SP_FRAMES - 1) * hop + n_fft;
    const dim3 grid((unsigned)tiles, (unsigned)cols, (unsigned)batch);
    if (span + skew * ((span - 1) / hop) <= SP_SPAN)
        SVCMI_LAUNCH(linear_spectrogram_kernel<true>, grid, dim3(TPB), 0, stream, x, (long long)x_bstride, (long long)n, basis, n_fft, hop, pad, eps,
                     out, (long long)frames, skew);
    else
        SVCMI_LAUNCH(linear_spectrogram_kernel<false>, grid, dim3(TPB), 0, stream, x, (long long)x_bstride, (long long)n, basis, n_fft, hop, pad, eps,
                     out, (long long)frames, skew);
    return SVCMI_LAST_ERROR();
}
