// pyin.hip -- the pYIN F0 extractor of pitch/core/pyin.py (libf0): YIN's cumulative mean normalised difference function (CMNDF) per frame,
// 99 thresholds weighted by a beta distribution into an observation column, a 2B-state voiced / unvoiced HMM decoded with Viterbi, and
// the refinement of the decoded bin by the closest per-threshold YIN estimate.  The device reproduces the reference AS IT EXECUTES under
// numpy (DESIGN.md 4.10 lists where that differs from the paper); everything is float64.  The host makes a plan (svcmi_pyin_plan:
// thresholds, beta weights, frequency axis, the transition band, constants); the device runs
//
//   pyin_cmndf_kernel    one block per frame.  The frame's n_fft samples (centre padding = index arithmetic on the fp32 clip) are staged in
//                        LDS once; thread i owns the lags i + 1, i + 1 + 256, ...: d(tau) = sum_j (x[j] - x[j + tau])^2 in its DIRECT form
//                        (every term is non-negative, so the error is relative and the minima near zero that the thresholds test do not
//                        suffer the cancellation of an autocorrelation form), four interleaved accumulator chains combined as
//                        (a0 + a1) + (a2 + a3): one fixed order per (frame, tau).  Then one thread runs the mean recursion
//                        m = m (tau - 1) / tau + d / tau, c = d / (m + eps) with the reference's operation order, and the RMS is a
//                        fixed-order block sum.
//   pyin_observe_kernel  one block per frame, the CMNDF row in LDS: the strict local minima M, the reference's border "deletion" (a no-op
//                        but for one case that drops the FIRST minimum from the interpolation set), the parabolic interpolation from the
//                        pre-update values (a border minimum has an infinite neighbour: NaN), then per threshold the first minimum below
//                        it or np.argmin / np.min of the row with numpy's NaN rules written out, the lag clamp, the bin
//                        argmin_b |1200 log2(F[b] / (Fs / lag))| as a block reduction (lowest index on ties; evaluated only when the lag
//                        changes from one threshold to the next), the weights added in threshold order, and the normalisation of the column
//                        (voiced half times voicing_prob, the unvoiced half one constant per frame) with its logarithm.
//   pyin_viterbi_kernel  one block per clip; thread k owns voiced state k and unvoiced state k + B.  Per time step s[j] = log_tiny + D[j] is
//                        the cost of reaching ANY state from j over an "impossible" transition (np.log(0 + tiny), about -708.4, not -inf:
//                        such transitions do win).  One block-wide arg-max of s (greater value wins, equal values take the lower index)
//                        serves every successor; each state then combines it under the same rule with its <= 2 max_step + 1 band entries
//                        band[i][d] + D[j] and its cross link.  The band entries and the cross link ALSO appear in s with the weaker
//                        constant; that is harmless: log A >= log_tiny and rounding is monotonic, so at the same index the true candidate
//                        dominates the duplicate, and a dominated duplicate can never change an arg-max under this rule.  Each candidate is
//                        one rounded sum, as in numpy's `A_log[:, i] + D_log[:, n - 1]`, so the result is numpy's argmax index for index.
//                        Back pointers int16 [frames][2B]; the walk back stages them through LDS.
//   pyin_finish_kernel   one block per frame: f0 from the decoded state, frame 0 and frames with rms < 0.01 set to 0, conf = O[state] / max
//                        of the column, and refine_estimates_yin (np.argmin of val_thr among the thresholds within R cents: the first NaN wins).
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

#if defined(__clang__)
#pragma clang fp contract(off)          // every product and sum below rounds once, like numpy's
#endif

namespace {

constexpr int PY_TPB = 256;
constexpr int PY_MAX_N = SVCMI_PYIN_MAX_NFFT;
constexpr int PY_MAX_B = SVCMI_PYIN_MAX_BINS;
constexpr int PY_MAX_THR = SVCMI_PYIN_MAX_THRESHOLDS;
constexpr int PY_MAX_W = SVCMI_PYIN_MAX_BAND;
constexpr int PY_FIN_TPB = 128;
constexpr int PY_CHUNK = 8;                              // frames of back pointers per step of the walk back (8 x 2048 x 2 bytes = D's LDS)
constexpr double PY_EPS = 2.220446049250313e-16;         // np.finfo(np.float64).eps
constexpr double PY_RMS_FLOOR = 0.01;

SVCMI_DEV unsigned long long py_bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }

// the arg-max rule of the trajectory: a greater value wins, an equal value takes the lower index
SVCMI_DEV void py_better(double c, int j, double& bv, int& bj) {
    const bool take = (c > bv) | ((c == bv) & (j < bj));      // no short circuit: selects, not branches
    bv = take ? c : bv;
    bj = take ? j : bj;
}

// block-wide arg-max under py_better; every thread returns the result.  redv / redi: one slot per wave.  The caller keeps a barrier
// between two calls.
SVCMI_DEV void py_block_argmax(double& v, int& idx, double* redv, int* redi) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s);
        const int oi = __shfl_xor(idx, s);
        py_better(ov, oi, v, idx);
    }
    const int tid = threadIdx.x, nw = ((int)blockDim.x + SVCMI_WAVE - 1) / SVCMI_WAVE;
    if ((tid & 63) == 0) { redv[tid >> 6] = v; redi[tid >> 6] = idx; }
    __syncthreads();
    v = redv[0];
    idx = redi[0];
    for (int w = 1; w < nw; ++w) py_better(redv[w], redi[w], v, idx);
}

// ------------------------------------------------------------------------------------------------ CMNDF and RMS
__global__ __launch_bounds__(PY_TPB) void pyin_cmndf_kernel(const float* x, long long n, int n_fft, int hop, int p_max, double* cm, double* rms) {
    __shared__ float fr[PY_MAX_N];                       // fp32 samples widen to fp64 exactly
    __shared__ double df[PY_MAX_N + 1];
    __shared__ double red[PY_TPB / SVCMI_WAVE];
    const int tid = threadIdx.x;
    const long long m = blockIdx.x, p0 = m * hop - n_fft / 2;
    double sq = 0.0;
    for (int j = tid; j < n_fft; j += PY_TPB) {
        const long long s = p0 + j;
        const float v = (s >= 0 && s < n) ? x[s] : 0.f;
        fr[j] = v;
        sq += (double)v * (double)v;
    }
    __syncthreads();
    for (int tau = 1 + tid; tau <= p_max; tau += PY_TPB) {
        const int cnt = n_fft - tau;                     // >= 0: p_max <= n_fft
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            const double d0 = (double)fr[j] - (double)fr[j + tau], d1 = (double)fr[j + 1] - (double)fr[j + 1 + tau];
            const double d2 = (double)fr[j + 2] - (double)fr[j + 2 + tau], d3 = (double)fr[j + 3] - (double)fr[j + 3 + tau];
            a0 += d0 * d0;
            a1 += d1 * d1;
            a2 += d2 * d2;
            a3 += d3 * d3;
        }
        for (; j < cnt; ++j) {
            const double d = (double)fr[j] - (double)fr[j + tau];
            a0 += d * d;
        }
        df[tau] = (a0 + a1) + (a2 + a3);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sq += __shfl_xor(sq, s);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        double mean = 0.0;
        df[0] = 1.0;
        for (int tau = 1; tau <= p_max; ++tau) {
            const double d = df[tau], t = (double)tau;
            mean = mean * (double)(tau - 1) / t + d / t;
            df[tau] = d / (mean + PY_EPS);
        }
        double s = red[0];
        for (int w = 1; w < PY_TPB / SVCMI_WAVE; ++w) s += red[w];
        rms[m] = sqrt(s / (double)n_fft);
    }
    __syncthreads();
    double* row = cm + m * (long long)(p_max + 1);
    for (int i = tid; i <= p_max; i += PY_TPB) row[i] = df[i];
}

// ------------------------------------------------------------------------------------------------ observation column
__global__ __launch_bounds__(PY_TPB) void pyin_observe_kernel(svcmi_pyin_plan p, const double* cm, double* O, double* logO, double* lag_thr,
                                                              double* val_thr) {
    __shared__ double cs[PY_MAX_N + 1];
    __shared__ int mlist[PY_MAX_N / 2 + 1];              // strict minima are never adjacent
    __shared__ double om[PY_MAX_B];
    __shared__ double lagv[PY_MAX_THR], valv[PY_MAX_THR];
    __shared__ int idxv[PY_MAX_THR], hit[PY_MAX_THR];
    __shared__ double redv[PY_TPB / SVCMI_WAVE];
    __shared__ int redi[PY_TPB / SVCMI_WAVE];
    __shared__ int sh_L, sh_start;
    __shared__ double sh_corr0, sh_unv;
    const int tid = threadIdx.x, B = p.n_pitch, nt = p.n_thr, p_min = p.p_min, p_max = p.p_max;
    const long long m = blockIdx.x;
    const double* row = cm + m * (long long)(p_max + 1);
    const double inf = HUGE_VAL;
    for (int i = tid; i <= p_max; i += PY_TPB) cs[i] = (i < p_min || i == p_max) ? inf : row[i];
    for (int b = tid; b < B; b += PY_TPB) om[b] = 0.0;
    __syncthreads();
    if (tid == 0) {
        int L = 0;
        for (int i = p_min; i <= p_max - 1; ++i)
            if (cs[i] < cs[i - 1] && cs[i] < cs[i + 1]) mlist[L++] = i;
        // the reference deletes "the value at the position of p_max - 1" from the list: position L - 1, and a minimum AT lag L - 1 makes
        // its mask drop element 0
        int start = 0;
        if (L > 0 && mlist[L - 1] == p_max - 1)
            for (int k = 0; k < L && mlist[k] <= L - 1; ++k)
                if (mlist[k] == L - 1) start = 1;
        sh_L = L;
        sh_start = start;
        sh_corr0 = 0.0;
    }
    __syncthreads();
    const int L = sh_L, start = sh_start;
    if (L > 0) {                                          // block-uniform
        for (int k = start + tid; k < L; k += PY_TPB) {   // neighbours of a strict minimum are not minima: in place is race-free
            const int i = mlist[k];
            const double y1 = cs[i - 1], y2 = cs[i], y3 = cs[i + 1];
            const double a = PY_EPS + (y1 + y3 - 2.0 * y2) / 2.0, b = (y3 - y1) / 2.0;
            cs[i] = y2 - (b * b) / (4.0 * a);
            if (k == start && mlist[0] != p_min) sh_corr0 = -b / (2.0 * a);
        }
        __syncthreads();
        if (tid == 0) {
            // np.argmin / np.min of the whole row: the first NaN if there is one, else the first minimum
            int gi = 0;
            double gv = cs[0];
            bool nan_seen = gv != gv;
            for (int i = 1; i <= p_max && !nan_seen; ++i) {
                const double v = cs[i];
                if (v != v) { gi = i; gv = v; nan_seen = true; }
                else if (v < gv) { gi = i; gv = v; }
            }
            double lowest = inf;                           // the smallest comparable value among the minima: no threshold at or below it selects anything
            for (int k = 0; k < L; ++k) {
                const double v = cs[mlist[k]];
                if (v < lowest) lowest = v;
            }
            const double corr0 = sh_corr0;
            for (int i = 0; i < nt; ++i) {
                const double thr = p.thresholds[i];
                int pos = -1;
                if (lowest < thr)
                    for (int k = 0; k < L; ++k)
                        if (cs[mlist[k]] < thr) { pos = k; break; }
                double lag, val;
                if (pos >= 0) {
                    lag = (double)mlist[pos] + corr0;      // p_corr[np.argmin(ascending list)] = p_corr[0], whichever minimum was chosen
                    val = cs[mlist[pos]];
                } else {
                    lag = (double)gi;
                    val = gv;
                }
                if (lag < (double)p_min) lag = (double)p_min;
                else if (lag >= (double)p_max) lag = (double)(p_max - 1);     // a NaN lag fails both and stays NaN
                lagv[i] = lag;
                valv[i] = val;
                hit[i] = pos >= 0;
            }
        }
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const double lag = lagv[i];
            if (i > 0 && py_bits(lag) == py_bits(lagv[i - 1])) {
                if (tid == 0) idxv[i] = idxv[i - 1];
                continue;                                  // block-uniform
            }
            // argmin_b |1200 log2(F[b] / (Fs / lag))|, lowest index on ties; all-NaN (a NaN lag) gives 0
            double bv = -inf;
            int bi = 0x7fffffff;
            if (lag == lag) {
                const double q = p.fs / lag;
                for (int b = tid; b < B; b += PY_TPB) py_better(-fabs(1200.0 * log2(p.f_axis[b] / q)), b, bv, bi);
            }
            py_block_argmax(bv, bi, redv, redi);
            if (tid == 0) idxv[i] = (lag == lag && bi < B) ? bi : 0;     // (bi stays out of range only for a plan whose axis is not positive)
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < nt; ++i) om[idxv[i]] += hit[i] ? p.beta[i] : p.absolute_min_prob * p.beta[i];
        __syncthreads();
    }
    for (int b = tid; b < B; b += PY_TPB) om[b] *= p.voicing_prob;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += om[b];            // np.sum(axis=0) of a [B, frames] array: row after row
        sh_unv = (1.0 - p.voicing_prob) * (1.0 - s) / (double)B;
    }
    __syncthreads();
    const double unv = sh_unv, log_unv = log(unv + p.tiny);
    double* orow = O + m * 2LL * B;
    for (int b = tid; b < B; b += PY_TPB) {
        orow[b] = om[b];
        orow[B + b] = unv;
    }
    if (logO) {
        double* lrow = logO + m * 2LL * B;
        for (int b = tid; b < B; b += PY_TPB) {
            lrow[b] = log(om[b] + p.tiny);
            lrow[B + b] = log_unv;
        }
    }
    for (int i = tid; i < nt; i += PY_TPB) {
        lag_thr[m * nt + i] = L > 0 ? lagv[i] : (double)p_min;
        val_thr[m * nt + i] = L > 0 ? valv[i] : 1.0;
    }
}

// ------------------------------------------------------------------------------------------------ Viterbi
// MAXT: the largest block this instantiation is launched with; WMAX: the widest band it takes.  The band sits in registers (66 of them
// at WMAX = 33): a block of up to 768 threads leaves 168 registers per thread and holds it without spilling, the full 1024 leaves 128 and
// spills a part of the widest.  WMAX = 11 (the reference's max_step = 5) keeps the unrolled candidate loop a third as long.
template <int MAXT, int WMAX>
__global__ __launch_bounds__(MAXT) void pyin_viterbi_kernel(const double* logO, int frames, int B, int ms, const double* band, double log_tiny,
                                                                 double log_cross, double log_c, short* ptr, int* path) {
    __shared__ double D[2][2 * PY_MAX_B];                // 32 KB; the walk back reuses it for the staged back pointers
    __shared__ double redv[PY_MAX_B / SVCMI_WAVE];
    __shared__ int redi[PY_MAX_B / SVCMI_WAVE];
    __shared__ int cur_s;
    const int k = threadIdx.x, W = 2 * ms + 1, S = 2 * B;
    const bool own = k < B;
    const double ninf = -HUGE_VAL;
    double bw[WMAX];
#pragma unroll
    for (int d = 0; d < WMAX; ++d) bw[d] = (own && d < W) ? band[(long long)k * W + d] : 0.0;
    double ov = 0.0, ou = 0.0;
    if (own) {
        D[0][k] = log_c + logO[k];
        D[0][k + B] = log_c + logO[k + B];
        ov = logO[S + k];                                  // frames >= 2: the host checked
        ou = logO[S + k + B];
    }
    __syncthreads();
    for (int t = 1; t < frames; ++t) {
        const double* prev = D[(t - 1) & 1];
        double* next = D[t & 1];
        const double o_v = ov, o_u = ou;
        if (own && t + 1 < frames) {
            ov = logO[(long long)(t + 1) * S + k];
            ou = logO[(long long)(t + 1) * S + k + B];
        }
        double gv = ninf;
        int gi = 0x7fffffff;
        if (own) {
            py_better(log_tiny + prev[k], k, gv, gi);
            py_better(log_tiny + prev[k + B], k + B, gv, gi);
        }
        py_block_argmax(gv, gi, redv, redi);
        if (own) {
            double vv = gv, uv = gv;
            int vi = gi, ui = gi;
#pragma unroll
            for (int d = 0; d < WMAX; ++d) {
                if (d < W) {                               // block-uniform
                    const int j = k - ms + d;
                    const bool in = j >= 0 && j < B;       // edge states: a predecessor outside the matrix never wins (-inf at a valid index)
                    const int jj = in ? j : k;
                    py_better(in ? bw[d] + prev[jj] : ninf, jj, vv, vi);
                    py_better(in ? bw[d] + prev[B + jj] : ninf, B + jj, uv, ui);
                }
            }
            py_better(log_cross + prev[k + B], k + B, vv, vi);
            py_better(log_cross + prev[k], k, uv, ui);
            next[k] = vv + o_v;
            next[k + B] = uv + o_u;
            short* pr = ptr + (long long)t * S;
            pr[k] = (short)vi;
            pr[k + B] = (short)ui;
        }
        __syncthreads();
    }
    {
        const double* last = D[(frames - 1) & 1];
        double gv = ninf;
        int gi = 0x7fffffff;
        if (own) {
            py_better(last[k], k, gv, gi);
            py_better(last[k + B], k + B, gv, gi);
        }
        py_block_argmax(gv, gi, redv, redi);
        if (k == 0) {
            if (gi >= S) gi = 0;                           // only a NaN column leaves no winner; never index outside the row
            cur_s = gi;
            path[frames - 1] = gi;
        }
    }
    __syncthreads();                                       // D is dead from here on
    short* pbuf = reinterpret_cast<short*>(&D[0][0]);
    for (int t_hi = frames - 1; t_hi >= 1; t_hi -= PY_CHUNK) {
        const int t_lo = t_hi - PY_CHUNK + 1 > 1 ? t_hi - PY_CHUNK + 1 : 1;                // rows t_lo .. t_hi
        const int count = (t_hi - t_lo + 1) * S;
        const short* src = ptr + (long long)t_lo * S;
        for (int i = k; i < count; i += (int)blockDim.x) pbuf[i] = src[i];
        __syncthreads();
        if (k == 0) {
            int cur = cur_s;
            for (int t = t_hi; t >= t_lo; --t) {
                cur = pbuf[(t - t_lo) * S + cur];
                if (cur < 0 || cur >= S) cur = 0;          // (see above)
                path[t - 1] = cur;
            }
            cur_s = cur;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ f0, confidence, refinement
__global__ __launch_bounds__(PY_FIN_TPB) void pyin_finish_kernel(svcmi_pyin_plan p, const int* path, const double* O, const double* rms,
                                                                 const double* lag_thr, const double* val_thr, double* f0_out, double* conf_out) {
    __shared__ double red[PY_FIN_TPB / SVCMI_WAVE];
    __shared__ double vals[PY_MAX_THR], fo[PY_MAX_THR];
    __shared__ int cand[PY_MAX_THR];
    const int tid = threadIdx.x, B = p.n_pitch, nt = p.n_thr;
    const long long m = blockIdx.x;
    const double* orow = O + m * 2LL * B;
    int st = path[m];
    st = st < 0 ? 0 : (st > 2 * B - 1 ? 2 * B - 1 : st);             // a caller's path is device data: never index outside the column
    double mx = -HUGE_VAL;
    for (int b = tid; b < 2 * B; b += PY_FIN_TPB) mx = fmax(mx, orow[b]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    double f0 = st < B ? p.f_axis[st] : 0.0;
    if (m == 0 || rms[m] < PY_RMS_FLOOR) f0 = 0.0;
    if (tid < nt) {
        const double f = p.fs / lag_thr[m * nt + tid];
        fo[tid] = f;
        vals[tid] = val_thr[m * nt + tid];
        cand[tid] = f0 > 0.0 && fabs(1200.0 * log2(f / f0)) < p.tol_cents;      // a NaN lag is no candidate
    }
    __syncthreads();
    if (tid == 0) {
        double best = red[0];
        for (int w = 1; w < PY_FIN_TPB / SVCMI_WAVE; ++w) best = fmax(best, red[w]);
        conf_out[m] = orow[st] / best;
        if (f0 > 0.0) {
            // np.argmin over the candidates' val_thr: the first NaN wins, else the first minimum
            int pick = -1;
            double pv = 0.0;
            for (int i = 0; i < nt; ++i) {
                if (!cand[i]) continue;
                const double v = vals[i];
                if (pick < 0) { pick = i; pv = v; if (v != v) break; }
                else if (v != v) { pick = i; break; }
                else if (v < pv) { pick = i; pv = v; }
            }
            if (pick >= 0) f0 = fo[pick];
        }
        f0_out[m] = f0;
    }
}

int plan_check(const svcmi_pyin_plan* p) {
    if (!p || !p->thresholds || !p->beta || !p->f_axis || !p->band) return SVCMI_EINVAL;
    if (p->hop < 1 || p->n_fft < 2 || (p->n_fft & 1) || p->p_min < 1 || p->p_max < p->p_min || p->n_pitch < 1 || p->n_thr < 1 || p->max_step < 1)
        return SVCMI_EINVAL;
    if (!(p->fs > 0.0) || !(p->tol_cents > 0.0) || !(p->voicing_prob >= 0.0) || !(p->voicing_prob <= 1.0) || !(p->tiny > 0.0)) return SVCMI_EINVAL;
    if (p->n_pitch < 2 * p->max_step + 1) return SVCMI_EINVAL;       // the reference's edge rows would not fit its matrix
    if (p->n_fft > PY_MAX_N || p->p_max > p->n_fft || p->n_pitch > PY_MAX_B || p->n_thr > PY_MAX_THR || 2 * p->max_step + 1 > PY_MAX_W)
        return SVCMI_EUNSUPPORTED;
    if (((uintptr_t)p->thresholds & 7) || ((uintptr_t)p->beta & 7) || ((uintptr_t)p->f_axis & 7) || ((uintptr_t)p->band & 7)) return SVCMI_EALIGN;
    return 0;
}

int frames_check(int64_t frames, int64_t min_frames, int64_t widest) {
    if (frames < min_frames) return SVCMI_EINVAL;
    if (frames >= 0x7fffffffLL / widest) return SVCMI_EUNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int64_t svcmi_pyin_plan_bytes(void) { return (int64_t)sizeof(svcmi_pyin_plan); }

// for the stage's planning pass (csrc/host_stages.hip): not part of the ABI
extern "C" int svcmi_pyin_plan_check_(const svcmi_pyin_plan* p) { return plan_check(p); }

// pyin_cmndf_kernel for csrc/yin.hip, whose rows must hold the same bits: the launch alone, for arguments the caller has checked (n_fft even,
// 2 .. SVCMI_PYIN_MAX_NFFT; 1 <= p_max <= n_fft; frames = 1 + n / hop >= 1, any number: the kernel knows no frame but its own).  Not part
// of the ABI
extern "C" int svcmi_pyin_cmndf_launch_(const float* x, int64_t n, int32_t n_fft, int32_t hop, int32_t p_max, double* cmndf, double* rms,
                                        int64_t frames, void* stream) {
    SVCMI_LAUNCH(pyin_cmndf_kernel, dim3((unsigned)frames), dim3(PY_TPB), 0, stream, x, (long long)n, n_fft, hop, p_max, cmndf, rms);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_pyin_cmndf_f64(const svcmi_pyin_plan* p, const float* x, int64_t n, double* cmndf, double* rms, int64_t frames, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!x || !cmndf || !rms || n < 1 || frames != 1 + n / p->hop) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, 2, p->p_max + 1)) return rc;
    if (((uintptr_t)x & 3) || ((uintptr_t)cmndf & 7) || ((uintptr_t)rms & 7)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(pyin_cmndf_kernel, dim3((unsigned)frames), dim3(PY_TPB), 0, stream, x, (long long)n, p->n_fft, p->hop, p->p_max, cmndf, rms);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_pyin_observe_f64(const svcmi_pyin_plan* p, const double* cmndf, int64_t frames, double* O, double* logO, double* lag_thr,
                                      double* val_thr, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!cmndf || !O || !lag_thr || !val_thr) return SVCMI_EINVAL;
    const int64_t widest = 2 * p->n_pitch > p->p_max + 1 ? 2 * p->n_pitch : p->p_max + 1;
    if (int rc = frames_check(frames, 1, widest)) return rc;
    if (((uintptr_t)cmndf & 7) || ((uintptr_t)O & 7) || ((uintptr_t)logO & 7) || ((uintptr_t)lag_thr & 7) || ((uintptr_t)val_thr & 7)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(pyin_observe_kernel, dim3((unsigned)frames), dim3(PY_TPB), 0, stream, *p, cmndf, O, logO, lag_thr, val_thr);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_pyin_viterbi_f64(const double* logO, int64_t frames, int32_t n_pitch, int32_t max_step, const double* band, double log_tiny,
                                      double log_cross, double log_c, int16_t* ptr, int32_t* path, void* stream) {
    if (!logO || !band || !ptr || !path || n_pitch < 1 || max_step < 1) return SVCMI_EINVAL;
    if (n_pitch > PY_MAX_B || 2 * max_step + 1 > PY_MAX_W) return SVCMI_EUNSUPPORTED;
    if (int rc = frames_check(frames, 2, 2 * (int64_t)n_pitch)) return rc;
    if (((uintptr_t)logO & 7) || ((uintptr_t)band & 7) || ((uintptr_t)ptr & 1) || ((uintptr_t)path & 3)) return SVCMI_EALIGN;
    const int threads = (n_pitch + SVCMI_WAVE - 1) / SVCMI_WAVE * SVCMI_WAVE;
#define PY_VITERBI(MAXT, WMAX)                                                                                                          \
    SVCMI_LAUNCH((pyin_viterbi_kernel<MAXT, WMAX>), dim3(1), dim3((unsigned)threads), 0, stream, logO, (int)frames, n_pitch, max_step, band, \
                 log_tiny, log_cross, log_c, (short*)ptr, path)
    const bool narrow = 2 * max_step + 1 <= 11;
    if (threads <= 768 && narrow) PY_VITERBI(768, 11);
    else if (threads <= 768) PY_VITERBI(768, PY_MAX_W);
    else if (narrow) PY_VITERBI(PY_MAX_B, 11);
    else PY_VITERBI(PY_MAX_B, PY_MAX_W);
#undef PY_VITERBI
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_pyin_finish_f64(const svcmi_pyin_plan* p, const int32_t* path, const double* O, const double* rms, const double* lag_thr,
                                     const double* val_thr, int64_t frames, double* f0, double* conf, void* stream) {
    if (int rc = plan_check(p)) return rc;
    if (!path || !O || !rms || !lag_thr || !val_thr || !f0 || !conf) return SVCMI_EINVAL;
    if (int rc = frames_check(frames, 1, 2 * (int64_t)p->n_pitch)) return rc;
    if (((uintptr_t)path & 3) || ((uintptr_t)O & 7) || ((uintptr_t)rms & 7) || ((uintptr_t)lag_thr & 7) || ((uintptr_t)val_thr & 7) ||
        ((uintptr_t)f0 & 7) || ((uintptr_t)conf & 7))
        return SVCMI_EALIGN;
    SVCMI_LAUNCH(pyin_finish_kernel, dim3((unsigned)frames), dim3(PY_FIN_TPB), 0, stream, *p, path, O, rms, lag_thr, val_thr, f0, conf);
    return SVCMI_LAST_ERROR();
}
