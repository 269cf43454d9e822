// spectral_loss.hip -- the reconstruction figures by which a checkpoint is picked (vits_extend/validation.py, stft.py, stft_loss.py),
// without ever materialising a spectrogram that exists only to be summed:
//   svcmi_stft_distance_f32  one STFT resolution of a (predicted, recorded) pair -> three sums per item
//       mx[k, t] = sqrt(max(re_x^2 + im_x^2, floor)),  my likewise                    (stft_loss.py:28: clamp, then sqrt)
//       out[b]   = ( sum (my - mx)^2,  sum my^2,  sum |log my - log mx| )   over k < bins, t < frames, as doubles
//   svcmi_log_mel_f32        out[b, m, t] = log(max(sum_k mel[m, k] spec[b, k, t], clip))   (stft.py:94-104 after the magnitude; a clamped
//                            element is the host's logf(clip), the same bits whatever the device's logf rounds to)
//   svcmi_abs_diff_sum_f32   out[b] = sum |a[b, i] - b[b, i]| as a double                    (the mel L1 before its division)
// stft_distance is csrc/spectrogram.hip's decomposition -- a wave owns 32 frames (the MFMA's columns) x 16 bins (re, im = its 32 rows), a
// 256-thread block 32 frames x 64 bins, reflect padding as index arithmetic on the load, the table from L2 straight to registers 8
// K-steps ahead -- with two changes.  (1) Every table fragment feeds TWO matrix instructions, one per signal, into two accumulator sets:
// the table, the dominant traffic, is read once per pair.  The block stages both signals' spans (2 x 6144 floats = the same 48 KB; a longer
// span, e.g. 2048 / 240, is read from global memory with the same index arithmetic).  (2) The epilogue stores nothing but one triple per
// block: lanes whose bin >= bins or frame >= frames contribute nothing, a lane sums its (at most 8) elements in fp32 in ascending (g, q)
// order, the wave reduces by shuffles (lane l += lane l + 32, 16, 8, 4, 2, 1), the block through LDS (waves 0, 1, 2, 3 in that order), and
// the block's triple goes to ITS OWN slot of the workspace: slot = bin column * frame tiles + frame tile.  No atomics anywhere; a second
// small kernel adds an item's slots in ascending slot order in fp64.
// Determinism contract: re and im of either signal are ONE accumulator chain over the K-steps (i = 0, 1), (2, 3), ... in ascending order,
// started from zero; p = fmaf(re, re, im * im); m = sqrtf(fmaxf(p, floor)); l = logf(m) (the accurate one) -- the SAME chain for x and for
// y, so distance(x, x) is exactly (0, sum, 0).  The order of every addition after that is fixed by (bin, frame) alone.  An item's three
// doubles therefore depend on that item's samples and the table alone: not on the batch index, the batch size, the stream, the thread
// order, or whether the span was in LDS.  (They do depend on n_fft, hop and pad, which fix the tiling.)
// log_mel: matrix cores again, frames = the instruction's columns (stores and spectrogram loads run along `frames`), 32 mel rows = its
// rows, K = bins in ascending order, one accumulator chain per output; the filterbank comes TRANSPOSED, melT[k][m] with row stride ldm, so
// the 32 lanes of a half-wave read 32 consecutive floats.  A block's 4 waves own 4 mel row tiles of the same 32 frames (n_mel = 100: one
// block column).  Padding rows (m >= n_mel), padding columns (t >= frames) and the odd K tail (k >= bins: both operands zero) are
// computed on valid addresses and never stored.
// abs_diff_sum: a block owns 4096 consecutive elements, thread `tid` elements tid + 256 i in ascending i; the same fixed-order wave /
// block / slot reduction.
#include <math.h>
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int SD_FRAMES = 32;                    // frames per block (the MFMA's columns)
constexpr int SD_BINS = 16;                      // bins per wave (x 2 table columns = the MFMA's rows)
constexpr int SD_WAVES = TPB / SVCMI_WAVE;
constexpr int SD_SPAN = 6144;                    // staged samples PER SIGNAL, skew included: 2 x 24 KB (1024 / 120: 4744 + 39)
constexpr int SD_U = 8;                          // K-steps of table prefetch (16 table rows)
constexpr int AD_PER_THREAD = 16;
constexpr int AD_CHUNK = TPB * AD_PER_THREAD;    // elements per block of abs_diff_sum
constexpr int LM_ROWS = 32, LM_FRAMES = 32;      // log_mel: mel rows x frames per wave

// sample p of the reflect-padded signal; zero past its end (the unused tail of a block's span).  pad < n: one reflection is enough.
__device__ __forceinline__ float padded_sample(const float* x, long long n, int pad, long long p, long long total) {
    if (p >= total) return 0.f;
    long long s = p - pad;
    if (s < 0) s = -s;
    if (s >= n) s = 2 * (n - 1) - s;
    return x[s];
}

// lane 0 receives v[0] + v[32] ... in the fixed tree order l += l + 32, 16, 8, 4, 2, 1 (every lane takes part in every shuffle)
__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// NC sums of a thread -> wave (shuffles) -> block (LDS, waves in ascending order) -> slot[0 .. NC).  Every thread of the block calls it.
template <int NC>
__device__ __forceinline__ void block_sums_to_slot(const float (&v)[NC], float* slot) {
    __shared__ float red[SD_WAVES][NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float s = wave_sum_fixed(v[c]);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SD_WAVES; ++w) s += red[w][threadIdx.x];
        slot[threadIdx.x] = s;
    }
}

template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void stft_distance_kernel(const float* x, long long x_bstride, const float* y, long long y_bstride, long long n,
                                                            const float* basis, int n_fft, int hop, int pad, float floor_, long long frames, int skew,
                                                            float* partials) {
    __shared__ float xs[IN_LDS ? SD_SPAN : 1], ys[IN_LDS ? SD_SPAN : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const int bins = n_fft / 2 + 1;
    const long long t0 = (long long)blockIdx.x * SD_FRAMES;
    const float* xb = x + (long long)blockIdx.z * x_bstride;
    const float* yb = y + (long long)blockIdx.z * y_bstride;
    const long long total = n + 2LL * pad;
    if constexpr (IN_LDS) {
        const long long p0 = t0 * hop;
        const int span = (SD_FRAMES - 1) * hop + n_fft;               // + skew <= SD_SPAN: the host checked
        for (int s = tid; s < span; s += TPB) {
            const int at = s + skew * (s / hop);
            xs[at] = padded_sample(xb, n, pad, p0 + s, total);
            ys[at] = padded_sample(yb, n, pad, p0 + s, total);
        }
        __syncthreads();
    }
    const int bin0 = ((int)blockIdx.y * SD_WAVES + wave) * SD_BINS;   // wave-uniform
    float sums[3] = {0.f, 0.f, 0.f};                                  // (my - mx)^2, my^2, |log my - log mx|
    if (bin0 < bins) {                                                // a wave past the last bin adds zeros: it still joins the block's reduction
        // table operand: row i = idx of the instruction, K index khalf
        const int bin_a = bin0 + 8 * (idx >> 4) + (idx & 7), part = (idx >> 3) & 1;
        const long long ldb = 2LL * bins;
        const float* bp = basis + khalf * ldb + (bin_a < bins ? 2 * bin_a + part : 0);  // rows past the last bin: any valid column, never summed
        const long long kstride = 2 * ldb;
        const int nsteps = n_fft / 2;

        // frame operand: column j = idx, sample t hop + c with c = 2 ks + khalf
        int off = idx * hop + khalf + skew * (idx + khalf / hop), r = khalf % hop;       // LDS: position of sample (idx hop + c), c mod hop
        long long frame = t0 + idx;
        if (frame > frames - 1) frame = frames - 1;                                       // columns past the last frame: a valid one, never summed
        long long pg = frame * hop + khalf;                                               // global: padded index

        auto next_pair = [&](float& bx, float& by) {
            if constexpr (IN_LDS) {
                bx = xs[off];
                by = ys[off];
                off += 2;
                if (skew) {               // even hop (>= 2): at most one row boundary per step
                    r += 2;
                    if (r >= hop) { r -= hop; off += 1; }
                }
            } else {
                bx = padded_sample(xb, n, pad, pg, total);
                by = padded_sample(yb, n, pad, pg, total);
                pg += 2;
            }
        };

        svcmi_f32x16 accx, accy;
#pragma unroll
        for (int i = 0; i < 16; ++i) accx[i] = accy[i] = 0.f;
        float a_cur[SD_U], a_nxt[SD_U];
#pragma unroll
        for (int u = 0; u < SD_U; ++u) a_cur[u] = bp[(long long)(u < nsteps ? u : nsteps - 1) * kstride];
        int ks = 0;
        for (; ks + SD_U <= nsteps; ks += SD_U) {
#pragma unroll
            for (int u = 0; u < SD_U; ++u) {
                int s = ks + SD_U + u;
                if (s > nsteps - 1) s = nsteps - 1;                   // clamped: always a valid row, no branch around the loads
                a_nxt[u] = bp[(long long)s * kstride];
            }
#pragma unroll
            for (int u = 0; u < SD_U; ++u) {
                float bx, by;
                next_pair(bx, by);
                accx = svcmi_mfma_32x32x2(a_cur[u], bx, accx);        // one table fragment, both signals
                accy = svcmi_mfma_32x32x2(a_cur[u], by, accy);
            }
#pragma unroll
            for (int u = 0; u < SD_U; ++u) a_cur[u] = a_nxt[u];
        }
        for (; ks < nsteps; ++ks) {
            const float a = bp[(long long)ks * kstride];
            float bx, by;
            next_pair(bx, by);
            accx = svcmi_mfma_32x32x2(a, bx, accx);
            accy = svcmi_mfma_32x32x2(a, by, accy);
        }

        // lane: frame t0 + idx, bins bin0 + 8 g + q + 4 khalf; re = acc[8 g + q], im = acc[8 g + 4 + q]
        const bool frame_ok = t0 + idx < frames;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int bin = bin0 + 8 * g + q + 4 * khalf;
                const float rx = accx[8 * g + q], ix = accx[8 * g + 4 + q], ry = accy[8 * g + q], iy = accy[8 * g + 4 + q];
                const float mx = sqrtf(fmaxf(fmaf(rx, rx, ix * ix), floor_)), my = sqrtf(fmaxf(fmaf(ry, ry, iy * iy), floor_));
                const float d = my - mx, l = fabsf(logf(my) - logf(mx));
                if (frame_ok && bin < bins) {
                    sums[0] = fmaf(d, d, sums[0]);
                    sums[1] = fmaf(my, my, sums[1]);
                    sums[2] += l;
                }
            }
        }
    }
    const long long slot = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_sums_to_slot<3>(sums, partials + 3 * slot);
}

// out[b][c] = partials[b][0][c] + partials[b][1][c] + ... in ascending slot order, in fp64: thread c of block b
__global__ __launch_bounds__(SVCMI_WAVE) void slots_to_double_kernel(const float* partials, long long nslots, int nc, double* out) {
    const int c = threadIdx.x;
    if (c >= nc) return;
    const float* p = partials + (long long)blockIdx.x * nslots * nc + c;
    double s = 0.0;
    for (long long i = 0; i < nslots; ++i) s += (double)p[i * nc];
    out[(long long)blockIdx.x * nc + c] = s;
}

__global__ __launch_bounds__(TPB) void abs_diff_sum_kernel(const float* a, long long a_bstride, const float* b, long long b_bstride, long long count,
                                                           float* partials) {
    const float* ab = a + (long long)blockIdx.y * a_bstride;
    const float* bb = b + (long long)blockIdx.y * b_bstride;
    const long long base = (long long)blockIdx.x * AD_CHUNK + threadIdx.x;
    float s[1] = {0.f};
#pragma unroll
    for (int i = 0; i < AD_PER_THREAD; ++i) {
        const long long e = base + (long long)i * TPB;
        if (e < count) s[0] += fabsf(ab[e] - bb[e]);
    }
    block_sums_to_slot<1>(s, partials + (long long)blockIdx.y * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(TPB) void log_mel_kernel(const float* spec, const float* melT, int ldm, int n_mel, int bins, long long frames, float clip,
                                                      float log_clip, float* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const int m0 = ((int)blockIdx.y * SD_WAVES + wave) * LM_ROWS;     // wave-uniform
    if (m0 >= n_mel) return;                                          // no barrier in this kernel
    const long long t0 = (long long)blockIdx.x * LM_FRAMES;
    long long tc = t0 + idx;
    if (tc > frames - 1) tc = frames - 1;                             // columns past the last frame: a valid one, never stored
    const float* sp = spec + (long long)blockIdx.z * bins * frames + tc;
    const float* mp = melT + m0 + idx;                                // m0 + idx < ldm: rows past n_mel are the host's padding, never stored
    svcmi_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nsteps = (bins + 1) / 2;
#pragma unroll 4
    for (int ks = 0; ks < nsteps; ++ks) {
        const int k = 2 * ks + khalf, kc = k < bins ? k : bins - 1;   // the odd tail: a valid address, both operands zero
        const float a = mp[(long long)kc * ldm], b = sp[(long long)kc * frames];
        acc = svcmi_mfma_32x32x2(k < bins ? a : 0.f, k < bins ? b : 0.f, acc);
    }
    // lane: frame t0 + idx, mel rows m0 + (r & 3) + 8 (r >> 2) + 4 khalf
    const long long t = t0 + idx;
    if (t >= frames) return;
    float* ob = out + (long long)blockIdx.z * n_mel * frames + t;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (m < n_mel) ob[(long long)m * frames] = acc[r] <= clip ? log_clip : logf(acc[r]);      // NaN stays NaN, as torch.clamp keeps it
    }
}

struct DistanceGrid { long long tiles, cols; };
// frames > 0 and the rest of the geometry already checked
inline DistanceGrid distance_grid(int n_fft, long long frames) {
    const int bins = n_fft / 2 + 1;
    return DistanceGrid{(frames + SD_FRAMES - 1) / SD_FRAMES, (bins + SD_BINS * SD_WAVES - 1) / (SD_BINS * SD_WAVES)};
}
inline bool distance_geometry_ok(int batch, long long n, int n_fft, int hop, int pad) {
    return batch >= 1 && hop >= 1 && pad >= 0 && n_fft >= 2 && !(n_fft & 1) && n > pad && n + 2LL * pad >= n_fft;
}

}  // namespace

extern "C" int64_t svcmi_stft_distance_workspace_bytes(int32_t batch, int64_t n, int32_t n_fft, int32_t hop, int32_t pad) {
    if (!distance_geometry_ok(batch, n, n_fft, hop, pad)) return SVCMI_EINVAL;
    const DistanceGrid g = distance_grid(n_fft, 1 + (n + 2LL * pad - n_fft) / hop);
    return (int64_t)batch * g.tiles * g.cols * 3 * (int64_t)sizeof(float);
}

extern "C" int svcmi_stft_distance_f32(const float* x, int64_t x_bstride, const float* y, int64_t y_bstride, int32_t batch, int64_t n,
                                       const float* basis, int32_t n_fft, int32_t hop, int32_t pad, float floor_, int64_t frames, float* partials,
                                       int64_t partials_bytes, double* out, void* stream) {
    if (!x || !y || !basis || !partials || !out || !distance_geometry_ok(batch, n, n_fft, hop, pad)) return SVCMI_EINVAL;
    if (frames != 1 + (n + 2LL * pad - n_fft) / hop) return SVCMI_EINVAL;
    if (batch > 1 && (x_bstride < n || y_bstride < n)) return SVCMI_EINVAL;
    if (!(floor_ > 0.f)) return SVCMI_EINVAL;                          // log of the clamped magnitude must be finite
    const DistanceGrid g = distance_grid(n_fft, frames);
    if (partials_bytes < (int64_t)batch * g.tiles * g.cols * 3 * (int64_t)sizeof(float)) return SVCMI_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)basis & 3) || ((uintptr_t)partials & 3) || ((uintptr_t)out & 7)) return SVCMI_EALIGN;
    if (g.tiles > 0x7fffffffLL || g.cols > 65535 || batch > 65535) return SVCMI_EUNSUPPORTED;
    const int skew = (hop & 1) ? 0 : 1;
    const long long span = (long long)(SD_FRAMES - 1) * hop + n_fft;
    const dim3 grid((unsigned)g.tiles, (unsigned)g.cols, (unsigned)batch);
    if (span + skew * ((span - 1) / hop) <= SD_SPAN)
        SVCMI_LAUNCH(stft_distance_kernel<true>, grid, dim3(TPB), 0, stream, x, (long long)x_bstride, y, (long long)y_bstride, (long long)n, basis, n_fft,
                     hop, pad, floor_, (long long)frames, skew, partials);
    else
        SVCMI_LAUNCH(stft_distance_kernel<false>, grid, dim3(TPB), 0, stream, x, (long long)x_bstride, y, (long long)y_bstride, (long long)n, basis, n_fft,
                     hop, pad, floor_, (long long)frames, skew, partials);
    SVCMI_LAUNCH(slots_to_double_kernel, dim3((unsigned)batch), dim3(SVCMI_WAVE), 0, stream, (const float*)partials, g.tiles * g.cols, 3, out);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_log_mel_f32(const float* spec, int32_t batch, int32_t bins, int64_t frames, const float* melT, int32_t ldm, int32_t n_mel,
                                 float clip, float* out, void* stream) {
    if (!spec || !melT || !out || batch < 1 || bins < 1 || frames < 1 || n_mel < 1) return SVCMI_EINVAL;
    if (ldm < (n_mel + LM_ROWS - 1) / LM_ROWS * LM_ROWS) return SVCMI_EINVAL;      // the lanes of the last row tile read its padding
    if (!(clip > 0.f)) return SVCMI_EINVAL;
    if (((uintptr_t)spec & 3) || ((uintptr_t)melT & 3) || ((uintptr_t)out & 3)) return SVCMI_EALIGN;
    const long long tiles = (frames + LM_FRAMES - 1) / LM_FRAMES;
    const int rows = (n_mel + LM_ROWS * SD_WAVES - 1) / (LM_ROWS * SD_WAVES);
    if (tiles > 0x7fffffffLL || rows > 65535 || batch > 65535) return SVCMI_EUNSUPPORTED;
    SVCMI_LAUNCH(log_mel_kernel, dim3((unsigned)tiles, (unsigned)rows, (unsigned)batch), dim3(TPB), 0, stream, spec, melT, ldm, n_mel, bins,
                 (long long)frames, clip, logf(clip), out);      // the clamped value's log from the host's libm: the same bits from every build
    return SVCMI_LAST_ERROR();
}

extern "C" int64_t svcmi_abs_diff_sum_workspace_bytes(int32_t batch, int64_t count) {
    if (batch < 1 || count < 1) return SVCMI_EINVAL;
    return (int64_t)batch * ((count + AD_CHUNK - 1) / AD_CHUNK) * (int64_t)sizeof(float);
}

extern "C" int svcmi_abs_diff_sum_f32(const float* a, int64_t a_bstride, const float* b, int64_t b_bstride, int32_t batch, int64_t count,
                                      float* partials, int64_t partials_bytes, double* out, void* stream) {
    if (!a || !b || !partials || !out || batch < 1 || count < 1) return SVCMI_EINVAL;
    if (batch > 1 && (a_bstride < count || b_bstride < count)) return SVCMI_EINVAL;
    const long long chunks = (count + AD_CHUNK - 1) / AD_CHUNK;
    if (partials_bytes < (int64_t)batch * chunks * (int64_t)sizeof(float)) return SVCMI_EINVAL;
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)partials & 3) || ((uintptr_t)out & 7)) return SVCMI_EALIGN;
    if (chunks > 0x7fffffffLL || batch > 65535) return SVCMI_EUNSUPPORTED;
    SVCMI_LAUNCH(abs_diff_sum_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(TPB), 0, stream, a, (long long)a_bstride, b, (long long)b_bstride,
                 (long long)count, partials);
    SVCMI_LAUNCH(slots_to_double_kernel, dim3((unsigned)batch), dim3(SVCMI_WAVE), 0, stream, (const float*)partials, chunks, 1, out);
    return SVCMI_LAST_ERROR();
}
