// salience.hip -- the salience F0 extractor of pitch/inference.py:31-44 (compute_f0_salience -> pitch/core/salience.py, a Melodia-style
// salience map followed by ONE dynamic programme over the clip).  The host makes a plan (svcmi_salience_plan: tables, bin range,
// constants); the device runs
//
//   salience_stft_kernel   X[t, k] = sum_{i < n_fft} xp[t hop + i] * basis[i, 2j / 2j + 1], k = k_lo + j, xp = x zero-padded by n_fft / 2
//                          (librosa.stft: center=True, pad_mode='constant'; the padding is index arithmetic on the load).  The tile of
//                          csrc/spectrogram.hip: a real DFT as a product on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), a wave owns
//                          32 frames x 16 bins, a block 32 frames x 64 bins, the frames' sample span staged once in LDS (skewed rows for
//                          an even hop), the table operand prefetched from L2 into registers.  Re and im are kept ([frames][n_bins]
//                          complex64), and only the n_bins bins whose instantaneous frequency can reach [f_min, f_max) are computed
//                          (about 230 of 1025 for the reference's parameters).  One ascending accumulator chain per output.
//   salience_map_kernel    one block per frame, the column in LDS: phase increment against the previous frame, wrapped to one turn,
//                          -> instantaneous frequency -> log-frequency bin per STFT bin; thread b then adds the powers of the STFT bins
//                          that fell into bin b in ASCENDING k (no atomics: the sum has one order), the column is smoothed along
//                          frequency and written out, its maximum goes into an integer atomic max on the bit pattern.
//   salience_harm_kernel   one block per frame: the first threshold against the global maximum (which zeroes exactly the maximal cell
//                          for gamma = 0, and everything when the maximum is 0: a NaN quotient compares false), the harmonic
//                          summation as a sparse correlation in ascending tap order, the second global maximum.
//   salience_finish_kernel the second threshold, elementwise.
//   salience_dp_kernel     one block per clip, thread b owns pitch bin b: D in fp64 in LDS, every one of the B predecessors evaluated
//                          per state in ascending order with a strict compare -- numpy's argmax, also where two sums only become equal
//                          through the rounding of `+ log_lo` (a banded form that takes the out-of-band argmax from D itself gets those
//                          wrong).  Back pointers int16 [frames][B] in global memory; the walk back stages them through LDS.
//
// Phase arithmetic runs in TURNS: omega_k H / (2 pi) = k H / n_fft, whose fractional part ((k H) mod n_fft) / n_fft is exact, so the
// wrapped increment loses nothing to a 200-radian intermediate; the instantaneous frequency and the bin position are float64 (230
// values per frame): an fp32 log2 alone would move a position by 6e-5 bins, far more than the fp32 phases do (3e-6 at 100 Hz).
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int SP_FRAMES = 32;                    // frames per block (the MFMA's columns)
constexpr int SP_BINS = 16;                      // bins per wave (x 2 table columns = the MFMA's rows)
constexpr int SP_WAVES = TPB / SVCMI_WAVE;
constexpr int SP_SPAN = 12288;                   // staged samples, skew included: 48 KB (2048 / 320: 11968 + 37)
constexpr int SP_U = 8;                          // K-steps of table prefetch (16 table rows)
constexpr int SAL_MAX = SVCMI_SALIENCE_MAX_BINS;
constexpr int SAL_SMOOTH_MAX = 65;
constexpr int SAL_HALO = SAL_SMOOTH_MAX / 2;
constexpr int DP_CHUNK = 16;                     // frames of back pointers staged per step of the walk back (16 x 1024 x 2 bytes)
constexpr double EPS32 = 1.1920928955078125e-7;  // np.finfo(np.float32).eps

// max on the bit patterns of non-negative floats: the result does not depend on the order of arrival
#ifdef SVCMI_EMU
static inline void sal_atomic_max(unsigned* p, unsigned v) {
    unsigned o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
#else
__device__ __forceinline__ void sal_atomic_max(unsigned* p, unsigned v) { atomicMax(p, v); }
#endif

SVCMI_DEV float sal_bits_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
SVCMI_DEV unsigned sal_float_bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

// the reference's mask `20 log10(v / max + eps) < gamma` as `v / max + eps < 10^(gamma / 20)`, in float64 like the reference
SVCMI_DEV bool sal_keep(float v, float mx, double thresh) { return (double)v / (double)mx + EPS32 < thresh; }

// block maximum of non-negative values -> one atomic per block (red: SVCMI_WAVE floats of LDS at most)
SVCMI_DEV void sal_block_max(float m, float* red, unsigned* gmax) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float v = red[0];
        for (int w = 1; w < (int)blockDim.x / SVCMI_WAVE; ++w) v = fmaxf(v, red[w]);
        sal_atomic_max(gmax, sal_float_bits(v));
    }
}

// sample p of the zero-padded signal
__device__ __forceinline__ float centred_sample(const float* x, long long n, int pad, long long p) {
    const long long s = p - pad;
    return (s >= 0 && s < n) ? x[s] : 0.f;
}

template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void salience_stft_kernel(const float* x, long long n, const float* basis, int n_fft, int hop, int bins,
                                                            float* out, long long frames, int skew) {
    __shared__ float xs[IN_LDS ? SP_SPAN : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const int pad = n_fft / 2;
    const long long t0 = (long long)blockIdx.x * SP_FRAMES;
    if constexpr (IN_LDS) {
        const long long p0 = t0 * hop;
        const int span = (SP_FRAMES - 1) * hop + n_fft;               // + skew <= SP_SPAN: the host checked
        for (int s = tid; s < span; s += TPB) xs[s + skew * (s / hop)] = centred_sample(x, n, pad, p0 + s);
        __syncthreads();
    }
    const int bin0 = ((int)blockIdx.y * SP_WAVES + wave) * SP_BINS;   // wave-uniform
    if (bin0 >= bins) return;                                         // after the only barrier

    // table operand: row i = idx of the instruction, K index khalf (the row order of csrc/spectrogram.hip: re and im of a bin in one lane)
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
            b = centred_sample(x, n, pad, pg);
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
    float* ob = out + t * ldb;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bin = bin0 + 8 * g + q + 4 * khalf;
            if (bin < bins) *reinterpret_cast<float2*>(ob + 2 * bin) = make_float2(acc[8 * g + q], acc[8 * g + 4 + q]);
        }
    }
}

__global__ __launch_bounds__(64) void salience_zero_kernel(unsigned* gmax) {
    if (threadIdx.x < 2) gmax[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(TPB) void salience_map_kernel(svcmi_salience_plan p, const float* X, int frames, float* lf, unsigned* gmax) {
    __shared__ int kbin[SAL_MAX];
    __shared__ float kpow[SAL_MAX];
    __shared__ float y[SAL_MAX + 2 * SAL_HALO];
    __shared__ float taps[SAL_SMOOTH_MAX];
    __shared__ float red[TPB / SVCMI_WAVE];
    const int tid = threadIdx.x, t = blockIdx.x;
    const int nb = p.n_bins, B = p.n_pitch, half = p.smooth_len / 2;
    const int tc = t > 0 ? t : 1;                                       // frame 0 repeats frame 1's instantaneous frequencies
    const float2* cur = reinterpret_cast<const float2*>(X) + (long long)tc * nb;
    const float2* prv = cur - nb;
    const float2* own = reinterpret_cast<const float2*>(X) + (long long)t * nb;
    const double hz_per_bin = (double)p.fs / (double)p.n_fft, turn_bins = (double)p.n_fft / (double)p.hop;
    for (int j = tid; j < nb; j += TPB) {
        const int k = p.k_lo + j;
        const float2 a = cur[j], b = prv[j], o = own[j];
        // heterodyned phase increment in turns: (angle(a) - angle(b)) / 2 pi - frac(k hop / n_fft), then the reference's wrap
        const float dphi = atan2f(a.y, a.x) - atan2f(b.y, b.x);
        const float frac = (float)(int)(((long long)k * p.hop) % p.n_fft) / (float)p.n_fft;
        float w = fmaf(dphi, 0.15915494309189535f, -frac);
        w = w - (rintf(w + 1.0f) - 1.0f);
        const double f = ((double)k + (double)w * turn_bins) * hz_per_bin;
        int bin = -1;
        if (f >= (double)p.f_min && f < (double)p.f_max) {
            bin = (int)floor((double)p.bins_per_octave * log2(f / (double)p.f_min) + 0.5);
            if (bin < 0 || bin >= B) bin = -1;
        }
        kbin[j] = bin;
        kpow[j] = fmaf(o.x, o.x, o.y * o.y);
    }
    for (int i = tid; i < B + 2 * SAL_HALO; i += TPB) y[i] = 0.f;
    if (tid < p.smooth_len) taps[tid] = p.smooth[tid];
    __syncthreads();
    for (int b = tid; b < B; b += TPB) {
        float s = 0.f;
        for (int j = 0; j < nb; ++j)                                     // ascending k: the one order of this sum
            if (kbin[j] == b) s += kpow[j];
        y[SAL_HALO + b] = s;
    }
    __syncthreads();
    float m = 0.f;
    for (int b = tid; b < B; b += TPB) {
        float s = 0.f;
        for (int d = 0; d < p.smooth_len; ++d) s = fmaf(taps[d], y[SAL_HALO + b + half - d], s);     // convolution, zero extension
        lf[(long long)t * B + b] = s;
        m = fmaxf(m, s);
    }
    sal_block_max(m, red, gmax);
}

__global__ __launch_bounds__(TPB) void salience_harm_kernel(svcmi_salience_plan p, float* lf, float* z, unsigned* gmax) {
    __shared__ float row[SAL_MAX];
    __shared__ int hoff[SAL_MAX];
    __shared__ float hw[SAL_MAX];
    __shared__ float red[TPB / SVCMI_WAVE];
    const int tid = threadIdx.x, t = blockIdx.x, B = p.n_pitch, nh = p.n_harm;
    const float mx = sal_bits_float(gmax[0]);
    float* lr = lf + (long long)t * B;
    for (int b = tid; b < B; b += TPB) {
        const float v = lr[b];
        const float kept = sal_keep(v, mx, p.thresh) ? v : 0.f;
        row[b] = kept;
        lr[b] = kept;
    }
    for (int m = tid; m < nh; m += TPB) {
        hoff[m] = p.harm_off[m];
        hw[m] = p.harm_w[m];
    }
    __syncthreads();
    float mz = 0.f;
    for (int b = tid; b < B; b += TPB) {
        float s = 0.f;
        for (int m = 0; m < nh; ++m) {                                   // ascending taps: the order of scipy's correlate1d
            const int j = b + hoff[m];
            if (j >= 0 && j < B) s = fmaf(hw[m], row[j], s);
        }
        z[(long long)t * B + b] = s;
        mz = fmaxf(mz, s);
    }
    sal_block_max(mz, red, gmax + 1);
}

__global__ __launch_bounds__(TPB) void salience_finish_kernel(float* z, long long count, const unsigned* gmax, double thresh) {
    const float mx = sal_bits_float(gmax[1]);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < count; i += (long long)gridDim.x * TPB) {
        const float v = z[i];
        if (!sal_keep(v, mx, thresh)) z[i] = 0.f;
    }
}

__global__ __launch_bounds__(SAL_MAX) void salience_dp_kernel(const float* z, int frames, int B, int tol, double c_hi, double c_lo, short* ptr,
                                                              int* path) {
    __shared__ double val[2][SAL_MAX];
    __shared__ short pbuf[DP_CHUNK * SAL_MAX];
    __shared__ int cur_s;
    const int k = threadIdx.x;
    if (k < B) val[0][k] = log((double)z[k] + EPS32);
    float z_next = k < B ? z[B + k] : 0.f;                                // frames >= 2: the host checked
    const int lo = k - tol > 0 ? k - tol : 0, hi = k + tol < B - 1 ? k + tol : B - 1;
    __syncthreads();
    for (int t = 1; t < frames; ++t) {
        const double* prev = val[(t - 1) & 1];
        const float zt = z_next;
        if (k < B && t + 1 < frames) z_next = z[(long long)(t + 1) * B + k];
        if (k < B) {
            // every predecessor in ascending order, strict '>': the lowest index attaining the maximum of the ROUNDED sums
            double bv = -HUGE_VAL;
            int bj = 0;
            for (int j = 0; j < lo; ++j) {
                const double c = c_lo + prev[j];
                if (c > bv) { bv = c; bj = j; }
            }
            for (int j = lo; j <= hi; ++j) {
                const double c = c_hi + prev[j];
                if (c > bv) { bv = c; bj = j; }
            }
            for (int j = hi + 1; j < B; ++j) {
                const double c = c_lo + prev[j];
                if (c > bv) { bv = c; bj = j; }
            }
            val[t & 1][k] = bv + log((double)zt + EPS32);
            ptr[(long long)t * B + k] = (short)bj;
        }
        __syncthreads();
    }
    if (k == 0) {
        const double* last = val[(frames - 1) & 1];
        int bj = 0;
        for (int j = 1; j < B; ++j)
            if (last[j] > last[bj]) bj = j;
        cur_s = bj;
        path[frames - 1] = bj;
    }
    __syncthreads();
    // the walk back follows frames - 1 dependent back pointers: rows staged through LDS DP_CHUNK frames at a time by the whole block
    for (int t_hi = frames - 1; t_hi >= 1; t_hi -= DP_CHUNK) {
        const int t_lo = t_hi - DP_CHUNK + 1 > 1 ? t_hi - DP_CHUNK + 1 : 1;                // rows t_lo .. t_hi
        const int count = (t_hi - t_lo + 1) * B;
        const short* src = ptr + (long long)t_lo * B;
        for (int i = k; i < count; i += (int)blockDim.x) pbuf[i] = src[i];
        __syncthreads();
        if (k == 0) {
            int cur = cur_s;
            for (int t = t_hi; t >= t_lo; --t) {
                cur = pbuf[(t - t_lo) * B + cur];
                path[t - 1] = cur;
            }
            cur_s = cur;
        }
        __syncthreads();
    }
}

int plan_check(const svcmi_salience_plan* p) {
    if (!p || !p->basis || !p->smooth || !p->harm_off || !p->harm_w) return SVCMI_EINVAL;
    if (p->hop < 1 || p->n_fft < 2 || (p->n_fft & 1) || p->n_bins < 1 || p->k_lo < 0 || (long long)p->k_lo + p->n_bins > p->n_fft / 2 + 1) return SVCMI_EINVAL;
    if (p->n_pitch < 1 || p->n_harm < 1 || p->smooth_len < 1 || !(p->smooth_len & 1) || p->tol < 0) return SVCMI_EINVAL;
    if (!(p->fs > 0.f) || !(p->f_min > 0.f) || !(p->f_max > p->f_min) || !(p->bins_per_octave > 0.f)) return SVCMI_EINVAL;
    if (p->n_bins > SAL_MAX || p->n_pitch > SAL_MAX || p->tol > SAL_MAX || p->n_harm > SAL_MAX || p->smooth_len > SAL_SMOOTH_MAX) return SVCMI_EUNSUPPORTED;
    if (((uintptr_t)p->basis & 3) || ((uintptr_t)p->smooth & 3) || ((uintptr_t)p->harm_off & 3) || ((uintptr_t)p->harm_w & 3)) return SVCMI_EALIGN;
    return 0;
}

int frames_check(int64_t frames, int32_t n_pitch) {
    if (frames < 2) return SVCMI_EINVAL;
    if (frames >= 0x7fffffffLL / n_pitch) return SVCMI_EUNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int64_t svcmi_salience_plan_bytes(void) { return (int64_t)sizeof(svcmi_salience_plan); }

extern "C" int svcmi_salience_stft_f32(const svcmi_salience_plan* p, const float* x, int64_t n, float* X, int64_t frames, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!x || !X || n < 1 || frames != 1 + n / p->hop) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, p->n_bins > p->n_pitch ? p->n_bins : p->n_pitch)) return rc;
    if (((uintptr_t)x & 3) || ((uintptr_t)X & 7)) return SVCMI_EALIGN;
    const int hop = p->hop, n_fft = p->n_fft, bins = p->n_bins;
    const long long tiles = (frames + SP_FRAMES - 1) / SP_FRAMES;
    const int cols = (bins + SP_BINS * SP_WAVES - 1) / (SP_BINS * SP_WAVES);
    const int skew = (hop & 1) ? 0 : 1;
    const long long span = (long long)(SP_FRAMES - 1) * hop + n_fft;
    const dim3 grid((unsigned)tiles, (unsigned)cols);
    if (span + skew * ((span - 1) / hop) <= SP_SPAN)
        SVCMI_LAUNCH(salience_stft_kernel<true>, grid, dim3(TPB), 0, stream, x, (long long)n, p->basis, n_fft, hop, bins, X, (long long)frames, skew);
    else
        SVCMI_LAUNCH(salience_stft_kernel<false>, grid, dim3(TPB), 0, stream, x, (long long)n, p->basis, n_fft, hop, bins, X, (long long)frames, skew);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_salience_map_f32(const svcmi_salience_plan* p, const float* X, int64_t frames, float* lf, float* z, uint32_t* gmax, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!X || !lf || !z || !gmax) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, p->n_bins > p->n_pitch ? p->n_bins : p->n_pitch)) return rc;
    if (((uintptr_t)X & 7) || ((uintptr_t)lf & 3) || ((uintptr_t)z & 3) || ((uintptr_t)gmax & 3)) return SVCMI_EALIGN;
    unsigned* gm = reinterpret_cast<unsigned*>(gmax);
    SVCMI_LAUNCH(salience_zero_kernel, dim3(1), dim3(64), 0, stream, gm);
    SVCMI_LAUNCH(salience_map_kernel, dim3((unsigned)frames), dim3(TPB), 0, stream, *p, X, (int)frames, lf, gm);
    SVCMI_LAUNCH(salience_harm_kernel, dim3((unsigned)frames), dim3(TPB), 0, stream, *p, lf, z, gm);
    const long long count = (long long)frames * p->n_pitch;
    long long nblk = (count + TPB - 1) / TPB;
    if (nblk > 2048) nblk = 2048;
    SVCMI_LAUNCH(salience_finish_kernel, dim3((unsigned)nblk), dim3(TPB), 0, stream, z, count, (const unsigned*)gm, p->thresh);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_salience_dp_f64(const float* z, int64_t frames, int32_t n_pitch, int32_t tol, double log_hi, double log_lo, int16_t* ptr,
                                     int32_t* path, void* stream) {
    if (!z || !ptr || !path || n_pitch < 1 || tol < 0) return SVCMI_EINVAL;
    if (n_pitch > SAL_MAX || tol > SAL_MAX) return SVCMI_EUNSUPPORTED;
    if (int rc = frames_check(frames, n_pitch)) return rc;
    if (((uintptr_t)z & 3) || ((uintptr_t)ptr & 1) || ((uintptr_t)path & 3)) return SVCMI_EALIGN;
    const int threads = (n_pitch + SVCMI_WAVE - 1) / SVCMI_WAVE * SVCMI_WAVE;
    SVCMI_LAUNCH(salience_dp_kernel, dim3(1), dim3((unsigned)threads), 0, stream, z, (int)frames, n_pitch, tol, log_hi, log_lo, (short*)ptr, path);
    return SVCMI_LAST_ERROR();
}
