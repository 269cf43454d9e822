// yin.hip -- the YIN F0 extractor of pitch/core/yin.py (libf0): per frame the cumulative mean normalised difference function (CMNDF),
// absolute thresholding with a parabolic refinement, a second thresholding inside +/- 25 cents of the first estimate, f0 = Fs / lag, and
// the aperiodicity of the frame at that lag.  The device reproduces the reference AS IT EXECUTES under numpy; everything
// is float64.  The host makes a plan of plain numbers (svcmi_yin_plan: geometry, lag range, threshold, the two ratio constants of the
// refinement window); the device runs
//
//   pyin_cmndf_kernel        of csrc/pyin.hip, through its launcher svcmi_pyin_cmndf_launch_: the difference function exists once, so a
//                            YIN row and a pYIN row of the same frame and lag range hold the same bits.
//   yin_pick_kernel          one block per frame, the CMNDF row copied to LDS (the first thresholding writes into it).  A thresholding
//                            over [lo, hi) is: lo == hi -> lo at once; else the FIRST index i in [lo, hi) that is a strict local minimum
//                            (c[i] < c[i - 1] and c[i] < c[i + 1]) with c[i] < threshold (strict) -- thread t scans i = lo + t, lo + t + 256,
//                            ... and the block takes the lowest hit, an integer minimum, so the order of the reduction cannot matter --, moved
//                            by the parabola's offset -b / (2 a), a = eps + (y1 + y3 - 2 y2) / 2, b = (y3 - y1) / 2, and c[i] REPLACED by
//                            the parabola's value y2 - b^2 / (4 a); without a hit np.argmin of c[lo:hi] (the lowest index among equal
//                            values), a bare integer.  The first thresholding runs over [lag_min, lag_max) with the plan's threshold, the
//                            second with threshold = inf over [rint(Fs / ((Fs / lag) r_up)), rint(Fs / ((Fs / lag) r_down))) clipped to
//                            lag_min .. lag_max, on the row the first one modified: rint rounds half to even like np.round, the products
//                            keep the reference's order, r_up = 2^(25 / 1200) and r_down = 2^(-25 / 1200) come from the host.
//   yin_aperiodicity_kernel  one block per frame, the frame staged in LDS (centre padding = index arithmetic on the fp32 clip).  The
//                            mirror-padded frame shifted by the lag -- an integer shift when the lag has no fractional part (the reference
//                            does not multiply there), else (1 - frac) s[k] + frac s[k + 1] --, then sum f^2, sum s^2, sum (f - s)^2 in one
//                            fixed order (thread t takes j = t, t + 256, ... ascending; the wave butterfly; the four waves in order), the
//                            means, pwr = (m1 + m2) / 2, res = m3 / 2, ap = res / (pwr + eps).  Silence gives exactly 0.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

#if defined(__clang__)
#pragma clang fp contract(off)          // every product and sum below rounds once, like numpy's
#endif

// csrc/pyin.hip: pyin_cmndf_kernel's launcher without a pYIN plan and without pYIN's two-frame minimum (not part of the ABI)
extern "C" int svcmi_pyin_cmndf_launch_(const float* x, int64_t n, int32_t n_fft, int32_t hop, int32_t p_max, double* cmndf, double* rms,
                                        int64_t frames, void* stream);

namespace {

constexpr int YN_TPB = 256;
constexpr int YN_MAX_N = SVCMI_YIN_MAX_NFFT;
static_assert(SVCMI_YIN_MAX_NFFT <= SVCMI_PYIN_MAX_NFFT, "pyin_cmndf_kernel stages the frame in its own LDS array");
constexpr int YN_NONE = 0x7fffffff;
constexpr double YN_EPS = 2.220446049250313e-16;         // np.finfo(np.float64).eps

// np.argmin's rule: a smaller value wins, an equal value takes the lower index
SVCMI_DEV void yn_lower(double c, int j, double& bv, int& bj) {
    const bool take = (c < bv) | ((c == bv) & (j < bj));       // no short circuit: selects, not branches
    bv = take ? c : bv;
    bj = take ? j : bj;
}

// One thresholding over [lo, hi), lo < hi, block-wide: `hit` = the first strict local minimum below thr (YN_NONE without one), `am` = np.argmin
// of c[lo:hi] + lo.  Every thread returns both.  The caller keeps a barrier between two calls.
SVCMI_DEV void yn_search(const double* c, int lo, int hi, double thr, int& hit, int& am, int* redh, double* redv, int* redi) {
    const int tid = threadIdx.x;
    int h = YN_NONE, bi = YN_NONE;
    double bv = HUGE_VAL;
    for (int i = lo + tid; i < hi; i += YN_TPB) {          // 1 <= lo, hi <= lag_max: c[i - 1] and c[i + 1] are inside the row
        const double v = c[i];
        if (h == YN_NONE && v < c[i - 1] && v < c[i + 1] && v < thr) h = i;
        yn_lower(v, i, bv, bi);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int oh = __shfl_xor(h, s);
        const double ov = __shfl_xor(bv, s);
        const int oi = __shfl_xor(bi, s);
        h = oh < h ? oh : h;
        yn_lower(ov, oi, bv, bi);
    }
    if ((tid & 63) == 0) { redh[tid >> 6] = h; redv[tid >> 6] = bv; redi[tid >> 6] = bi; }
    __syncthreads();
    h = redh[0];
    bv = redv[0];
    bi = redi[0];
    for (int w = 1; w < YN_TPB / SVCMI_WAVE; ++w) {
        h = redh[w] < h ? redh[w] : h;
        yn_lower(redv[w], redi[w], bv, bi);
    }
    hit = h;
    am = bi < hi ? bi : lo;                                // (bi stays out of range only for a row of NaN; never index outside the row)
}

// the window limit rint(v) as an index inside lag_min .. lag_max (a NaN takes the lower end)
SVCMI_DEV int yn_clip(double v, int lag_min, int lag_max) {
    if (!(v >= (double)lag_min)) return lag_min;
    if (!(v <= (double)lag_max)) return lag_max;
    return (int)v;
}

// ------------------------------------------------------------------------------------------------ the two thresholdings
__global__ __launch_bounds__(YN_TPB) void yin_pick_kernel(svcmi_yin_plan p, const double* cm, double* lag_out, double* f0_out, double* first_out,
                                                          int* kind_out) {
    __shared__ double cs[YN_MAX_N + 1];
    __shared__ int redh[YN_TPB / SVCMI_WAVE], redi[YN_TPB / SVCMI_WAVE];
    __shared__ double redv[YN_TPB / SVCMI_WAVE];
    __shared__ double sh_lag;
    const int tid = threadIdx.x, lag_min = p.lag_min, lag_max = p.lag_max;
    const long long m = blockIdx.x;
    const double* row = cm + m * (long long)(lag_max + 1);
    for (int i = tid; i <= lag_max; i += YN_TPB) cs[i] = row[i];
    __syncthreads();
    int kind = 0;
    double lag1 = (double)lag_min;
    if (lag_min < lag_max) {                               // block-uniform
        int hit, am;
        yn_search(cs, lag_min, lag_max, p.threshold, hit, am, redh, redv, redi);
        if (hit != YN_NONE) {
            if (tid == 0) {
                const double y1 = cs[hit - 1], y2 = cs[hit], y3 = cs[hit + 1];
                const double a = YN_EPS + (y1 + y3 - 2.0 * y2) / 2.0, b = (y3 - y1) / 2.0;
                cs[hit] = y2 - (b * b) / (4.0 * a);        // the write-back: the second thresholding interpolates from this value
                sh_lag = (double)hit + -b / (2.0 * a);
            }
            __syncthreads();
            lag1 = sh_lag;
        } else {
            lag1 = (double)am;
            kind |= 1;
        }
    }
    const int lo = yn_clip(rint(p.fs / ((p.fs / lag1) * p.ratio_up)), lag_min, lag_max);
    const int hi = yn_clip(rint(p.fs / ((p.fs / lag1) * p.ratio_down)), lag_min, lag_max);
    double lag2 = (double)lo;
    if (lo >= hi) {                                        // the window collapsed (lo > hi cannot happen for a finite row; it takes the same way out)
        kind |= 2;
    } else {
        __syncthreads();                                   // the reduction slots are reused
        int hit, am;
        yn_search(cs, lo, hi, HUGE_VAL, hit, am, redh, redv, redi);
        if (hit != YN_NONE) {
            const double y1 = cs[hit - 1], y2 = cs[hit], y3 = cs[hit + 1];
            const double a = YN_EPS + (y1 + y3 - 2.0 * y2) / 2.0, b = (y3 - y1) / 2.0;
            lag2 = (double)hit + -b / (2.0 * a);
        } else {
            lag2 = (double)am;
            kind |= 4;
        }
    }
    if (tid == 0) {
        lag_out[m] = lag2;
        if (f0_out) f0_out[m] = p.fs / lag2;
        if (first_out) first_out[m] = lag1;
        if (kind_out) kind_out[m] = kind;
    }
}

// ------------------------------------------------------------------------------------------------ aperiodicity
// the mirror-padded frame np.concatenate((frame, np.flip(frame))) at index k; past its end (only a lag outside the documented range gets there) 0
SVCMI_DEV double yn_mirror(const float* fr, int n_fft, int k) {
    if (k < n_fft) return (double)fr[k];
    if (k < 2 * n_fft) return (double)fr[2 * n_fft - 1 - k];
    return 0.0;
}

__global__ __launch_bounds__(YN_TPB) void yin_aperiodicity_kernel(const float* x, long long n, int n_fft, int hop, const double* lag, double* ap) {
    __shared__ float fr[YN_MAX_N];                        // fp32 samples widen to fp64 exactly
    __shared__ double red[3][YN_TPB / SVCMI_WAVE];
    const int tid = threadIdx.x;
    const long long m = blockIdx.x, p0 = m * hop - n_fft / 2;
    for (int j = tid; j < n_fft; j += YN_TPB) {
        const long long s = p0 + j;
        fr[j] = (s >= 0 && s < n) ? x[s] : 0.f;
    }
    __syncthreads();
    const double lg = lag[m];
    double fl = floor(lg);
    if (!(fl >= 0.0)) fl = 0.0;                            // a lag is device data: never index outside the frame (a NaN lands here too)
    if (fl > (double)n_fft) fl = (double)n_fft;
    const int li = (int)fl;
    const double frac = lg - fl;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (frac == 0.0) {                                     // block-uniform
        for (int j = tid; j < n_fft; j += YN_TPB) {
            const double f = (double)fr[j], s = yn_mirror(fr, n_fft, li + j);
            const double d = f - s;
            s1 += f * f;
            s2 += s * s;
            s3 += d * d;
        }
    } else {
        const double w0 = 1.0 - frac;
        for (int j = tid; j < n_fft; j += YN_TPB) {
            const double f = (double)fr[j];
            const double s = w0 * yn_mirror(fr, n_fft, li + j) + frac * yn_mirror(fr, n_fft, li + 1 + j);
            const double d = f - s;
            s1 += f * f;
            s2 += s * s;
            s3 += d * d;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        s1 += __shfl_xor(s1, s);
        s2 += __shfl_xor(s2, s);
        s3 += __shfl_xor(s3, s);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; red[2][tid >> 6] = s3; }
    __syncthreads();
    if (tid == 0) {
        double t1 = red[0][0], t2 = red[1][0], t3 = red[2][0];
        for (int w = 1; w < YN_TPB / SVCMI_WAVE; ++w) { t1 += red[0][w]; t2 += red[1][w]; t3 += red[2][w]; }
        const double nn = (double)n_fft;
        const double pwr = (t1 / nn + t2 / nn) / 2.0, res = (t3 / nn) / 2.0;
        ap[m] = res / (pwr + YN_EPS);
    }
}

int plan_check(const svcmi_yin_plan* p) {
    if (!p) return SVCMI_EINVAL;
    if (p->hop < 1 || p->n_fft < 2 || (p->n_fft & 1) || p->lag_min < 1 || p->lag_max < p->lag_min) return SVCMI_EINVAL;
    if (!(p->fs > 0.0) || p->threshold != p->threshold || !(p->ratio_up > 0.0) || !(p->ratio_down > 0.0)) return SVCMI_EINVAL;
    if (p->n_fft > YN_MAX_N || p->lag_max > p->n_fft) return SVCMI_EUNSUPPORTED;
    return 0;
}

int frames_check(int64_t frames, int64_t widest) {
    if (frames < 1) return SVCMI_EINVAL;
    if (frames >= 0x7fffffffLL / widest) return SVCMI_EUNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int64_t svcmi_yin_plan_bytes(void) { return (int64_t)sizeof(svcmi_yin_plan); }

// for the stage's planning pass (csrc/host_stages.hip): not part of the ABI
extern "C" int svcmi_yin_plan_check_(const svcmi_yin_plan* p) { return plan_check(p); }

extern "C" int svcmi_yin_cmndf_f64(const svcmi_yin_plan* p, const float* x, int64_t n, double* cmndf, double* rms, int64_t frames, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!x || !cmndf || !rms || n < 1 || frames != 1 + n / p->hop) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, (int64_t)p->lag_max + 1)) return rc;
    if (((uintptr_t)x & 3) || ((uintptr_t)cmndf & 7) || ((uintptr_t)rms & 7)) return SVCMI_EALIGN;
    return svcmi_pyin_cmndf_launch_(x, n, p->n_fft, p->hop, p->lag_max, cmndf, rms, frames, stream);
}

extern "C" int svcmi_yin_pick_f64(const svcmi_yin_plan* p, const double* cmndf, int64_t frames, double* lag, double* f0, double* lag_first,
                                  int32_t* kind, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!cmndf || !lag) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, (int64_t)p->lag_max + 1)) return rc;
    if (((uintptr_t)cmndf & 7) || ((uintptr_t)lag & 7) || ((uintptr_t)f0 & 7) || ((uintptr_t)lag_first & 7) || ((uintptr_t)kind & 3)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(yin_pick_kernel, dim3((unsigned)frames), dim3(YN_TPB), 0, stream, *p, cmndf, lag, f0, lag_first, (int*)kind);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_yin_aperiodicity_f64(const svcmi_yin_plan* p, const float* x, int64_t n, const double* lag, int64_t frames, double* ap,
                                          void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!x || !lag || !ap || n < 1 || frames != 1 + n / p->hop) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, (int64_t)p->lag_max + 1)) return rc;
    if (((uintptr_t)x & 3) || ((uintptr_t)lag & 7) || ((uintptr_t)ap & 7)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(yin_aperiodicity_kernel, dim3((unsigned)frames), dim3(YN_TPB), 0, stream, x, (long long)n, p->n_fft, p->hop, lag, ap);
    return SVCMI_LAST_ERROR();
}
