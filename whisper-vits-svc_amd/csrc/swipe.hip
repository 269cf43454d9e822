// swipe.hip -- the SWIPE' F0 extractor of pitch/core/swipe_slim.py (libf0's `swipe_slim`): per window size N (a power of two, hop N / 2)
// the magnitudes of a centred Hann STFT are resampled onto a log-frequency axis by a cubic spline, every column is normalised and
// correlated with one prime-harmonic sawtooth kernel per pitch candidate; the windows' pitch strengths are interpolated linearly in time
// onto the output frames and summed with a weight per (window, candidate); the arg-max per frame is refined by a parabola.  There is no
// sequential part: the spline on a uniform grid is a FIXED LINEAR MAP, tabulated by the host as W_N [n_log][N / 2 + 1], so per window
//
//   S_N = K_N (W_N Y) / (|| W_N Y || + eps)          Y: the magnitudes, K_N: the kernel rows of that window's candidates
//
// is an STFT and two dense products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).  Everything is time-major ([frames][...]); the
// tables' and intermediates' rows are zero-padded to a multiple of 8 floats, so the products have no ragged K edge and take 16-byte
// operand loads.  The host makes the plan (svcmi_swipe_plan); the device runs, per window in ascending N,
//
//   swipe_mag_kernel       Y[t, k] = | sum_{i < N} xp[t N / 2 + i] basis[i, 2k / 2k + 1] |, xp = x with N / 2 zeros in front and
//                          N + N / 2 behind (librosa.stft(np.pad(x, (0, N)), center=True, pad_mode='constant'): index arithmetic on the
//                          load).  The tile of csrc/salience.hip, restated: a real DFT as a product on the matrix cores, a wave owns
//                          32 frames x 16 bins, a block 32 frames x 64 bins, the frames' sample span staged once in LDS (skewed rows)
//                          where it fits (N <= 512), the table operand prefetched into registers.  One ascending accumulator chain per
//                          output.  The pad columns of a row are written as zeros.
//   swipe_product_kernel   out[t, i] = sum_k A[i, k] B[t, k]: a wave owns 32 rows x 32 frames, both operands straight from global
//                          memory (L2-resident tables) as one float4 per lane and 8 K, prefetched one step ahead.  Lane half h takes
//                          k = 8 s + 4 h .. + 3, so the chain of an output runs 8s, 8s+4, 8s+1, 8s+5, ...: one FIXED order that depends on
//                          nothing but K.  <false>: the resampling W_N Y (pad columns zero).  <true>: the kernel product; the column
//                          norm is taken from the very operand values the lane loads (the two lane halves of a column hold all of
//                          it; each sums its part in ascending s, then half 0 + half 1), so it costs no pass and every wave gets the
//                          same bits, and the quotient acc / (sqrt(norm2) + eps) is the epilogue.
//
// and then once per clip
//
//   swipe_accum_kernel     one block per output frame j: per window in ascending N the two source frames around j H / (N / 2)
//                          (integer arithmetic; the weight r / hop is exact), v = s0 + w (s1 - s0), S[j, cand[c]] += mu[c] v in LDS.
//                          The sum of a cell has one order: windows ascending.
//   swipe_finish_kernel    one block per frame, float64 on the fp32 S like the reference's host code: arg-max with numpy's tie rule
//                          (lowest index), the neighbours S[i - 1] -- index -1 WRAPS to n_cand - 1 like numpy's -- and S[i + 1], the
//                          parabolic shift with its eps, f0 = f_min 2^(step (i + shift)), conf = S[i], f0 = 0 below the threshold.
//                          An arg-max at n_cand - 1 (the reference raises IndexError there) takes shift 0 and counts in `flags`.
#include <algorithm>
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

#if defined(__clang__)
#pragma clang fp contract(off)          // the finish kernel restates numpy's float64 operations one rounding each
#endif

namespace {

constexpr int TPB = 256;
constexpr int SP_FRAMES = 32;                    // frames per block (the MFMA's columns)
constexpr int SP_BINS = 16;                      // bins per wave (x 2 table columns = the MFMA's rows)
constexpr int SP_WAVES = TPB / SVCMI_WAVE;
constexpr int SP_SPAN = 12288;                   // staged samples, skew included: 48 KB (N = 512: 31 * 256 + 512 + 32)
constexpr int SP_U = 8;                          // K-steps of table prefetch (16 table rows)
constexpr int PR_ROWS = 32;                      // output rows per wave of the products
constexpr int SW_MAX_B = SVCMI_SWIPE_MAX_CANDIDATES;
constexpr double SW_EPS = 2.220446049250313e-16; // np.finfo(np.float64).eps

__host__ __device__ inline int pad8(int v) { return (v + 7) & ~7; }

// sample p of the padded signal: n_fft / 2 zeros in front, zeros behind
__device__ __forceinline__ float padded_sample(const float* x, long long n, int pad, long long p) {
    const long long s = p - pad;
    return (s >= 0 && s < n) ? x[s] : 0.f;
}

template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void swipe_mag_kernel(const float* x, long long n, const float* basis, int n_fft, float* out, long long frames) {
    __shared__ float xs[IN_LDS ? SP_SPAN : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const int hop = n_fft / 2, pad = n_fft / 2, bins = n_fft / 2 + 1, ldy = pad8(bins);
    const int skew = (hop & 1) ? 0 : 1;
    const long long t0 = (long long)blockIdx.x * SP_FRAMES;
    if constexpr (IN_LDS) {
        const long long p0 = t0 * hop;
        const int span = (SP_FRAMES - 1) * hop + n_fft;               // + skew <= SP_SPAN: the host checked
        for (int s = tid; s < span; s += TPB) xs[s + skew * (s / hop)] = padded_sample(x, n, pad, p0 + s);
        __syncthreads();
    }
    const int bin0 = ((int)blockIdx.y * SP_WAVES + wave) * SP_BINS;   // wave-uniform
    if (bin0 >= ldy) return;                                          // after the only barrier

    // table operand: row i = idx of the instruction, K index khalf (re and im of a bin in one lane)
    const int bin_a = bin0 + 8 * (idx >> 4) + (idx & 7), part = (idx >> 3) & 1;
    const long long ldb = 2LL * bins;
    const float* bp = basis + khalf * ldb + (bin_a < bins ? 2 * bin_a + part : 0);      // rows past the last bin: any valid column, stored as zero
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
            b = padded_sample(x, n, pad, pg);
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
    float* ob = out + t * ldy;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bin = bin0 + 8 * g + q + 4 * khalf;
            const float re = acc[8 * g + q], im = acc[8 * g + 4 + q];
            if (bin < ldy) ob[bin] = bin < bins ? sqrtf(re * re + im * im) : 0.f;
        }
    }
}

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// out[t, i] = sum_k A[i, k] B[t, k], K a multiple of 8.  rows_out >= M rows are written per frame (the rows M .. rows_out - 1 as zeros).
template <bool STRENGTH>
__global__ __launch_bounds__(TPB) void swipe_product_kernel(const float* A, int lda, int M, const float* Bm, int ldb, long long T, int K, float* out,
                                                            int ldo, int rows_out, float eps) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, khalf = lane >> 5;
    const long long t0 = (long long)blockIdx.x * 32;
    const int i0 = ((int)blockIdx.y * SP_WAVES + wave) * PR_ROWS;     // wave-uniform
    if (i0 >= rows_out) return;
    int arow = i0 + idx;
    if (arow > M - 1) arow = M - 1;                                   // rows past the last: a valid one, stored as zero or not at all
    long long brow = t0 + idx;
    if (brow > T - 1) brow = T - 1;
    const float* ap = A + (long long)arow * lda + 4 * khalf;
    const float* bp = Bm + brow * ldb + 4 * khalf;
    const int steps = K / 8;

    svcmi_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float ss = 0.f;
    float4 a = load4(ap), b = load4(bp);
    for (int s = 0; s < steps; ++s) {
        const int sn = s + 1 < steps ? s + 1 : s;                     // clamped: the last step loads itself again
        const float4 an = load4(ap + 8 * sn), bn = load4(bp + 8 * sn);
        acc = svcmi_mfma_32x32x2(a.x, b.x, acc);
        acc = svcmi_mfma_32x32x2(a.y, b.y, acc);
        acc = svcmi_mfma_32x32x2(a.z, b.z, acc);
        acc = svcmi_mfma_32x32x2(a.w, b.w, acc);
        if constexpr (STRENGTH) {
            ss = fmaf(b.x, b.x, ss);
            ss = fmaf(b.y, b.y, ss);
            ss = fmaf(b.z, b.z, ss);
            ss = fmaf(b.w, b.w, ss);
        }
        a = an;
        b = bn;
    }
    float den = 1.f;
    if constexpr (STRENGTH) {
        const float tot = ss + __shfl_xor(ss, 32);                    // the two halves of the column; a commutative sum: both lanes get the same bits
        den = sqrtf(tot) + eps;
    }
    // lane: frame t0 + idx, rows i0 + (r & 3) + 8 (r >> 2) + 4 khalf
    const long long t = t0 + idx;
    if (t >= T) return;
    float* ob = out + t * ldo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (i < rows_out) {
            const float v = STRENGTH ? acc[r] / den : acc[r];
            ob[i] = i < M ? v : 0.f;
        }
    }
}

struct accum_args {
    const float* sn[SVCMI_SWIPE_MAX_WINDOWS];        // S_N [frames_N][n_cand] of every window
};

__global__ __launch_bounds__(TPB) void swipe_accum_kernel(svcmi_swipe_plan p, accum_args a, float* S) {
    __shared__ float acc[SW_MAX_B];
    const int tid = threadIdx.x, B = p.n_pitch;
    const long long j = blockIdx.x, pos = j * p.hop;
    for (int b = tid; b < B; b += TPB) acc[b] = 0.f;
    __syncthreads();
    for (int o = 0; o < p.n_win; ++o) {
        const svcmi_swipe_window w = p.win[o];
        const int hop = w.n_fft / 2, nc = w.n_cand;
        const long long lo = pos / hop;
        const float frac = (float)(int)(pos - lo * hop) / (float)hop;  // exact: hop is a power of two in every plan the host makes
        const float* s0 = a.sn[o] + lo * nc;
        const float* s1 = s0 + nc;                                     // frame lo + 1 exists: frames_N = 1 + (n + N) / hop >= lo + 3
        for (int c = tid; c < nc; c += TPB) {
            const float v0 = s0[c], v1 = s1[c];
            const float v = v0 + frac * (v1 - v0);
            acc[w.cand[c]] += w.mu[c] * v;                             // cand ascends strictly: one writer per cell
        }
        __syncthreads();
    }
    for (int b = tid; b < B; b += TPB) S[j * B + b] = acc[b];
}

__global__ __launch_bounds__(64) void swipe_zero_kernel(unsigned* flags) {
    if (threadIdx.x == 0) flags[0] = 0u;
}

// greater value wins, an equal value takes the lower index (np.argmax)
SVCMI_DEV void sw_better(float c, int j, float& bv, int& bj) {
    const bool take = (c > bv) | ((c == bv) & (j < bj));
    bv = take ? c : bv;
    bj = take ? j : bj;
}

#ifdef SVCMI_EMU
static inline void sw_count(unsigned* p) { __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void sw_count(unsigned* p) { atomicAdd(p, 1u); }
#endif

__global__ __launch_bounds__(TPB) void swipe_finish_kernel(const float* S, int B, int n_log, double f_min, double step, double threshold, double* f0,
                                                           double* conf, int* amax, unsigned* flags) {
    __shared__ float redv[TPB / SVCMI_WAVE];
    __shared__ int redi[TPB / SVCMI_WAVE];
    const int tid = threadIdx.x;
    const long long t = blockIdx.x;
    const float* row = S + t * B;
    float bv = row[0];
    int bj = 0;
    for (int b = tid; b < B; b += TPB) sw_better(row[b], b, bv, bj);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(bv, s);
        const int oi = __shfl_xor(bj, s);
        sw_better(ov, oi, bv, bj);
    }
    if ((tid & 63) == 0) { redv[tid >> 6] = bv; redi[tid >> 6] = bj; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < TPB / SVCMI_WAVE; ++w) sw_better(redv[w], redi[w], bv, bj);
    const int i = bj;
    const double y2 = (double)row[i], y1 = (double)row[i > 0 ? i - 1 : B - 1];       // index -1 wraps, like numpy's
    double shift = 0.0;
    if (i == B - 1) {
        sw_count(flags);                                                              // the reference raises IndexError for the clip
    } else {
        const double y3 = (double)row[i + 1];
        const double a = SW_EPS + (y1 + y3 - 2 * y2) / 2;                             // yin.parabolic_interpolation
        const double b = (y3 - y1) / 2;
        shift = -b / (2 * a);
    }
    // interp1d(arange(n_log), arange(n_log) * step, 'linear')(i + shift): the segment below the first axis point >= x
    const double xq = (double)i + shift;
    int hi = (int)ceil(xq);
    if (!(hi >= 1)) hi = 1;
    if (hi > n_log - 1) hi = n_log - 1;
    const double x_lo = (double)(hi - 1), y_lo = (double)(hi - 1) * step, y_hi = (double)hi * step;
    const double slope = (y_hi - y_lo) / ((double)hi - x_lo);
    const double e = slope * (xq - x_lo) + y_lo;
    double f = f_min * exp2(e);
    if (y2 < threshold) f = 0.0;
    f0[t] = f;
    conf[t] = y2;
    if (amax) amax[t] = i;
}

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int plan_check(const svcmi_swipe_plan* p) {
    if (!p) return SVCMI_EINVAL;
    if (p->n_win < 1 || p->n_win > SVCMI_SWIPE_MAX_WINDOWS || p->hop < 1) return SVCMI_EINVAL;
    if (p->n_log < 2 || p->n_log > SVCMI_SWIPE_MAX_LOGBINS || p->n_pitch < 1 || p->n_pitch > SVCMI_SWIPE_MAX_CANDIDATES) return SVCMI_EINVAL;
    if (!(p->f_min > 0.0) || !(p->step > 0.0) || p->threshold != p->threshold) return SVCMI_EINVAL;
    for (int o = 0; o < p->n_win; ++o) {
        const svcmi_swipe_window& w = p->win[o];
        if (!w.basis || !w.resample || !w.kernels || !w.cand || !w.mu) return SVCMI_EINVAL;
        if (w.n_fft < 8 || w.n_fft > SVCMI_SWIPE_MAX_NFFT || !is_pow2(w.n_fft) || w.n_cand < 1 || w.n_cand > p->n_pitch) return SVCMI_EINVAL;
        if (((uintptr_t)w.basis & 3) || ((uintptr_t)w.resample & 15) || ((uintptr_t)w.kernels & 15) || ((uintptr_t)w.cand & 3) || ((uintptr_t)w.mu & 3))
            return SVCMI_EALIGN;
    }
    return 0;
}

int clip_check(int64_t n) {
    if (n < 1) return SVCMI_EINVAL;
    if (n >= (1LL << 31) - 4 * SVCMI_SWIPE_MAX_NFFT) return SVCMI_EUNSUPPORTED;       // frame counts and grids stay below 2^31; offsets are 64-bit
    return 0;
}

int64_t win_frames(int64_t n, int n_fft) { return 1 + (n + n_fft) / (n_fft / 2); }
int64_t out_frames(int64_t n, int hop) { return (n + hop - 1) / hop; }

int launch_product(bool strength, const float* A, int lda, int M, const float* Bm, int ldb, int64_t T, int K, float* out, int ldo, int rows_out,
                   void* stream) {
    const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((rows_out + PR_ROWS * SP_WAVES - 1) / (PR_ROWS * SP_WAVES)));
    if (strength)
        SVCMI_LAUNCH(swipe_product_kernel<true>, grid, dim3(TPB), 0, stream, A, lda, M, Bm, ldb, (long long)T, K, out, ldo, rows_out, (float)SW_EPS);
    else
        SVCMI_LAUNCH(swipe_product_kernel<false>, grid, dim3(TPB), 0, stream, A, lda, M, Bm, ldb, (long long)T, K, out, ldo, rows_out, 0.f);
    return SVCMI_LAST_ERROR();
}

}  // namespace

extern "C" int64_t svcmi_swipe_plan_bytes(void) { return (int64_t)sizeof(svcmi_swipe_plan); }

extern "C" int64_t svcmi_swipe_frames(const svcmi_swipe_plan* p, int32_t window, int64_t n) {
    if (int rc = plan_check(p)) return rc;
    if (int rc = clip_check(n)) return rc;
    if (window < 0) return out_frames(n, p->hop);
    if (window >= p->n_win) return SVCMI_EINVAL;
    return win_frames(n, p->win[window].n_fft);
}

extern "C" int svcmi_swipe_mag_f32(const svcmi_swipe_plan* p, int32_t window, const float* x, int64_t n, float* Y, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (int rc = clip_check(n)) return rc;
    if (!x || !Y || window < 0 || window >= p->n_win) return SVCMI_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)Y & 15)) return SVCMI_EALIGN;
    const svcmi_swipe_window& w = p->win[window];
    const int n_fft = w.n_fft, hop = n_fft / 2, ldy = pad8(n_fft / 2 + 1);
    const int64_t frames = win_frames(n, n_fft);
    const dim3 grid((unsigned)((frames + SP_FRAMES - 1) / SP_FRAMES), (unsigned)((ldy + SP_BINS * SP_WAVES - 1) / (SP_BINS * SP_WAVES)));
    const long long span = (long long)(SP_FRAMES - 1) * hop + n_fft;
    if (span + (span - 1) / hop <= SP_SPAN)                                            // hop is even: the skew is one float per row
        SVCMI_LAUNCH(swipe_mag_kernel<true>, grid, dim3(TPB), 0, stream, x, (long long)n, w.basis, n_fft, Y, (long long)frames);
    else
        SVCMI_LAUNCH(swipe_mag_kernel<false>, grid, dim3(TPB), 0, stream, x, (long long)n, w.basis, n_fft, Y, (long long)frames);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_swipe_resample_f32(const svcmi_swipe_plan* p, int32_t window, const float* Y, int64_t frames, float* L, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!Y || !L || window < 0 || window >= p->n_win || frames < 1 || frames >= (1LL << 31)) return SVCMI_EINVAL;
    if (((uintptr_t)Y & 15) || ((uintptr_t)L & 15)) return SVCMI_EALIGN;
    const svcmi_swipe_window& w = p->win[window];
    const int ldy = pad8(w.n_fft / 2 + 1), ldl = pad8(p->n_log);
    return launch_product(false, w.resample, ldy, p->n_log, Y, ldy, frames, ldy, L, ldl, ldl, stream);
}

extern "C" int svcmi_swipe_strength_f32(const svcmi_swipe_plan* p, int32_t window, const float* L, int64_t frames, float* SN, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!L || !SN || window < 0 || window >= p->n_win || frames < 1 || frames >= (1LL << 31)) return SVCMI_EINVAL;
    if (((uintptr_t)L & 15) || ((uintptr_t)SN & 3)) return SVCMI_EALIGN;
    const svcmi_swipe_window& w = p->win[window];
    const int ldl = pad8(p->n_log);
    return launch_product(true, w.kernels, ldl, w.n_cand, L, ldl, frames, ldl, SN, w.n_cand, w.n_cand, stream);
}

extern "C" int svcmi_swipe_accum_f32(const svcmi_swipe_plan* p, const float* SN, int64_t n, float* S, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (int rc = clip_check(n)) return rc;
    if (!SN || !S) return SVCMI_EINVAL;
    if (((uintptr_t)SN & 3) || ((uintptr_t)S & 3)) return SVCMI_EALIGN;
    accum_args a;
    int64_t off = 0;
    for (int o = 0; o < SVCMI_SWIPE_MAX_WINDOWS; ++o) {
        a.sn[o] = SN + off;
        if (o < p->n_win) off += win_frames(n, p->win[o].n_fft) * p->win[o].n_cand;
    }
    SVCMI_LAUNCH(swipe_accum_kernel, dim3((unsigned)out_frames(n, p->hop)), dim3(TPB), 0, stream, *p, a, S);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_swipe_finish_f64(const float* S, int64_t frames, int32_t n_pitch, int32_t n_log, double f_min, double step, double threshold,
                                      double* f0, double* conf, int32_t* amax, uint32_t* flags, void* stream) {
    if (!S || !f0 || !conf || !flags || frames < 1 || frames >= (1LL << 31)) return SVCMI_EINVAL;
    if (n_pitch < 1 || n_pitch > SVCMI_SWIPE_MAX_CANDIDATES || n_log < 2 || n_log > SVCMI_SWIPE_MAX_LOGBINS) return SVCMI_EINVAL;
    if (!(f_min > 0.0) || !(step > 0.0) || threshold != threshold) return SVCMI_EINVAL;
    if (((uintptr_t)S & 3) || ((uintptr_t)f0 & 7) || ((uintptr_t)conf & 7) || ((uintptr_t)amax & 3) || ((uintptr_t)flags & 3)) return SVCMI_EALIGN;
    unsigned* fl = reinterpret_cast<unsigned*>(flags);
    SVCMI_LAUNCH(swipe_zero_kernel, dim3(1), dim3(64), 0, stream, fl);
    SVCMI_LAUNCH(swipe_finish_kernel, dim3((unsigned)frames), dim3(TPB), 0, stream, S, n_pitch, n_log, f_min, step, threshold, f0, conf, amax, fl);
    return SVCMI_LAST_ERROR();
}

// ------------------------------------------------------------------------------------------------ the stage
// Workspace layout (256-byte aligned pieces): Y and L of the largest window (reused by every window: the launches of a stream run in
// order), the windows' S_N back to back, S when the caller does not ask for it.
namespace {
int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
struct layout { int64_t y, l, sn, s, total; };
layout stage_layout(const svcmi_swipe_plan& p, int64_t n) {
    int64_t ymax = 0, lmax = 0, sn = 0;
    for (int o = 0; o < p.n_win; ++o) {
        const int64_t T = win_frames(n, p.win[o].n_fft);
        ymax = std::max(ymax, T * pad8(p.win[o].n_fft / 2 + 1));
        lmax = std::max(lmax, T * pad8(p.n_log));
        sn += T * p.win[o].n_cand;
    }
    layout a;
    a.y = 0;
    a.l = a.y + up256(ymax * 4);
    a.sn = a.l + up256(lmax * 4);
    a.s = a.sn + up256(sn * 4);
    a.total = a.s + up256(out_frames(n, p.hop) * p.n_pitch * 4);
    return a;
}
}  // namespace

extern "C" int64_t svcmi_swipe_workspace_bytes(const svcmi_swipe_plan* p, int64_t n) {
    if (int rc = plan_check(p)) return rc;
    if (int rc = clip_check(n)) return rc;
    return stage_layout(*p, n).total + 256;
}

extern "C" int svcmi_swipe_f0_fwd(const svcmi_swipe_plan* p, const float* x, int64_t n, double* f0, double* conf, float* S, uint32_t* flags,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!p || !x || !f0 || !conf || !flags || !workspace) return SVCMI_EINVAL;
    const int64_t need = svcmi_swipe_workspace_bytes(p, n);
    if (need < 0) return (int)need;
    if (((uintptr_t)workspace & 255) || workspace_bytes < need) return SVCMI_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)S & 3) || ((uintptr_t)flags & 3) || (((uintptr_t)f0 | (uintptr_t)conf) & 7)) return SVCMI_EALIGN;
    const layout a = stage_layout(*p, n);
    char* ws = static_cast<char*>(workspace);
    float* Y = reinterpret_cast<float*>(ws + a.y);
    float* L = reinterpret_cast<float*>(ws + a.l);
    float* SN = reinterpret_cast<float*>(ws + a.sn);
    float* Sout = S ? S : reinterpret_cast<float*>(ws + a.s);
    int64_t off = 0;
    for (int o = 0; o < p->n_win; ++o) {
        const int64_t T = win_frames(n, p->win[o].n_fft);
        if (int rc = svcmi_swipe_mag_f32(p, o, x, n, Y, stream)) return rc;
        if (int rc = svcmi_swipe_resample_f32(p, o, Y, T, L, stream)) return rc;
        if (int rc = svcmi_swipe_strength_f32(p, o, L, T, SN + off, stream)) return rc;
        off += T * p->win[o].n_cand;
    }
    if (int rc = svcmi_swipe_accum_f32(p, SN, n, Sout, stream)) return rc;
    return svcmi_swipe_finish_f64(Sout, out_frames(n, p->hop), p->n_pitch, p->n_log, p->f_min, p->step, p->threshold, f0, conf, nullptr, flags, stream);
}
