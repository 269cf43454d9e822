// lstm.hip -- the speaker encoder's kernels (speaker/models/lstm.py: three nn.LSTM(.., 768) + Linear(768, 256, bias=False) layers over
// 250-frame mel windows; speaker/utils/audio.py: the mel front-end that feeds them).
//
// The recurrence.  One launch of lstm_step_kernel is ONE time step of one layer for all batch rows (PyTorch's rules: gate order
// i, f, g, o; zero initial state; the bias sum b_ih + b_hh arrives inside Gx):
//     G = Gx[:, t, :] + h_{t-1} * W_hh^T,     c = sigmoid(f) * c + sigmoid(i) * tanh(g),     h_t = sigmoid(o) * tanh(c)
// The input projections Gx = X * W_ih^T + b of all T steps and the output projection are launches of the implicit GEMM; what is left
// per step is [B, H] x [H, 4H] with B <= 64: 0.05 GFLOP against 9.4 MB of W_hh at H = 768 -- bound by latency and by reading the
// weights, not by the matrix pipe.
//   * A block owns LU = 4 hidden units and all four of their gate rows: 16 weight rows = one N tile of v_mfma_f32_16x16x4_f32, and
//     c and h of those units are finished inside the block (192 blocks at H = 768).  W_hh is packed once at load in tile order
//     [unit tile][gate][unit][K], so the block's rows are one contiguous 16-byte aligned span; W_ih's rows and the bias are permuted
//     the same way, so the big GEMM writes Gx in that column order already.
//   * The batch is the 16-row M tile (A operand: h_{t-1}); MT = ceil(B / 16) <= 4 tiles share every weight fragment.
//   * K = H is split over the block's four waves in blocks of 16 (lane l reads the float4 at k = 16 * blk + 4 * (l >> 4) of its row:
//     four matrix instructions per block, the K index a lane's element stands for is the same on both operands, which is all a dot
//     product needs).  The four partial tiles meet in LDS and are added in wave order: run-to-run identical bits, and a row's bits
//     do not depend on the batch it is launched in.
//   * State: h_t goes straight into row t of the layer's output sequence [B][T][H], h_{t-1} is row t - 1 (t = 0 reads nothing),
//     c lives in a [B][H] buffer updated in place by the block that owns the units.  No block waits on another block: the T steps
//     of a layer are T launches on the caller's stream.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int LU = 4;                  // hidden units per block
constexpr int LROWS = 4 * LU;          // their gate rows: one 16-wide N tile
constexpr int LWAVES = TPB / 64;
constexpr int LMT_MAX = 4;             // M tiles per launch: batch <= 64

// 1 / (1 + e^-v): e^-v overflows to +inf for v < -88.7 (-> exactly 0) and is below half an ulp of 1 for v > 17.4 (-> exactly 1);
// never NaN for a finite v.  tanhf is the library's (exactly +-1 from |v| ~ 9.1 on).
__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int MT>
__global__ __launch_bounds__(TPB) void lstm_step_kernel(const float* gx, long long gx_bs, const float* whh, float* hseq, long long h_bs, int ldh,
                                                        float* cst, int ldc, int B, int H, int t) {
    __shared__ float red[LWAVES][MT * 16][LROWS + 4];       // row stride 20: the 32 lanes of an LDS access group, writing or reading, hit 32 banks
    const int tid = threadIdx.x, lane = tid & 63, wave = SVCMI_UNIFORM(tid >> 6);
    const int tile = blockIdx.x;
    if (t > 0) {
        const int r16 = lane & 15, kq = (lane >> 4) * 4;
        const float* wrow = whh + ((long long)tile * LROWS + r16) * H;
        const float* hrow[MT];
        bool hok[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int b = m * 16 + r16;
            hok[m] = b < B;
            hrow[m] = hseq + (long long)(hok[m] ? b : 0) * h_bs + (long long)(t - 1) * ldh;
        }
        svcmi_f32x4 acc[MT][2];                           // two independent chains per tile: the instruction's dependent latency exceeds its issue time
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = svcmi_f32x4{0.f, 0.f, 0.f, 0.f};
        const int nblk = (H + 15) / 16, per = (nblk + LWAVES - 1) / LWAVES;
        const int blk0 = wave * per, blk1 = blk0 + per < nblk ? blk0 + per : nblk;
        // The K loop runs KU blocks at a time: their loads are all issued before the first matrix instruction waits (a step is a chain
        // of memory latencies, not of FLOPs; the compiler does not unroll a runtime-trip loop around the convergent matrix
        // instruction itself).  Every load is unconditional -- a lane or a block out of range reads a valid address and selects
        // zero -- and a zero block adds exactly nothing, so the bits do not depend on KU.
        constexpr int KU = MT <= 2 ? 4 : 2;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int blk = blk0; blk < blk1; blk += KU) {
            float4 w4[KU], h4[KU][MT];
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const int k = (blk + u) * 16 + kq;
                const bool kok = blk + u < blk1 && k < H;       // H % 4 == 0: a float4 is inside the row or outside it
                const int ks = kok ? k : 0;
                w4[u] = *reinterpret_cast<const float4*>(wrow + ks);
                if (!kok) w4[u] = zero4;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    h4[u][m] = *reinterpret_cast<const float4*>(hrow[m] + ks);      // (a row >= B points at row 0)
                    if (!(kok && hok[m])) h4[u][m] = zero4;
                }
            }
#pragma unroll
            for (int u = 0; u < KU; ++u)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    acc[m][0] = svcmi_mfma_16x16x4(h4[u][m].x, w4[u].x, acc[m][0]);
                    acc[m][1] = svcmi_mfma_16x16x4(h4[u][m].y, w4[u].y, acc[m][1]);
                    acc[m][0] = svcmi_mfma_16x16x4(h4[u][m].z, w4[u].z, acc[m][0]);
                    acc[m][1] = svcmi_mfma_16x16x4(h4[u][m].w, w4[u].w, acc[m][1]);
                }
        }
        // D: column (gate row of the tile) = lane & 15, batch row = 4 * (lane >> 4) + r
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][m * 16 + 4 * (lane >> 4) + r][r16] = acc[m][0][r] + acc[m][1][r];
    }
    __syncthreads();
    if (tid < MT * 16 * LU) {
        const int b = tid >> 2, u = tid & 3;
        if (b < B) {
            const float* g = gx + (long long)b * gx_bs + (long long)tile * LROWS + u;
            float pre[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float s = 0.f;
                if (t > 0) s = (red[0][b][q * LU + u] + red[1][b][q * LU + u]) + (red[2][b][q * LU + u] + red[3][b][q * LU + u]);
                pre[q] = g[q * LU] + s;
            }
            const int col = tile * LU + u;
            float* cp = cst + (long long)b * ldc + col;
            const float c_old = t > 0 ? *cp : 0.f;
            const float c_new = fmaf(lstm_sigmoid(pre[1]), c_old, lstm_sigmoid(pre[0]) * tanhf(pre[2]));
            *cp = c_new;
            hseq[(long long)b * h_bs + (long long)t * ldh + col] = lstm_sigmoid(pre[3]) * tanhf(c_new);
        }
    }
}

// ------------------------------------------------------------------------------------ speaker mel front-end glue
// y[n] = x[n] - coef * x[n - 1], y[0] = x[0] (scipy.signal.lfilter([1, -coef], [1], x): speaker/utils/audio.py apply_preemphasis), then
// the reflect padding of librosa.stft(center=True), in one pass: out[i] = y[reflect(i - pad)].
__global__ __launch_bounds__(TPB) void preemph_pad_kernel(const float* x, float* y, long long n, int pad, float coef) {
    const int b = blockIdx.y;
    const long long m = n + 2LL * pad;
    const float* xb = x + (long long)b * n;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < m; i += (long long)gridDim.x * TPB) {
        long long j = i - pad;
        if (j < 0) j = -j;
        if (j >= n) j = 2 * (n - 1) - j;
        y[(long long)b * m + i] = j > 0 ? fmaf(-coef, xb[j - 1], xb[j]) : xb[0];
    }
}

// p[r][f] = sqrt(re^2 + im^2) with (re | im) = ri[r][f], ri[r][half + f]; columns nbins..ldp-1 of p are written as zero
__global__ __launch_bounds__(TPB) void magnitude_kernel(const float* ri, float* p, long long rows, int nbins, int half, int ldri, int ldp) {
    const long long total = rows * ldp;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long r = i / ldp;
        const int f = (int)(i - r * ldp);
        float v = 0.f;
        if (f < nbins) {
            const float re = ri[r * ldri + f], im = ri[r * ldri + half + f];
            v = sqrtf(fmaf(re, re, im * im));
        }
        p[i] = v;
    }
}

// AudioProcessor.melspectrogram's tail with speaker_pretrain/config.json, in place on the mel projection m:
//   S = 20 log10(max(1e-5, m)) - ref_level_db;  S = (S - min_level_db) / -min_level_db;  S = 2 max_norm S - max_norm;  clip to +-max_norm
__global__ __launch_bounds__(TPB) void speaker_mel_finish_kernel(float* x, long long total, float ref_db, float min_db, float max_norm) {
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        float s = 20.0f * log10f(fmaxf(1e-5f, x[i])) - ref_db;
        s = (s - min_db) / (-min_db);
        s = (2.0f * max_norm) * s - max_norm;
        x[i] = fminf(fmaxf(s, -max_norm), max_norm);
    }
}

// y[r] = x[r] / max(|x[r]|_2, 1e-12) (torch.nn.functional.normalize): one wave per row, the squares summed in a fixed order
__global__ __launch_bounds__(64) void l2norm_rows_kernel(const float* x, long long ldx, int d, float* y, long long ldy) {
    const float* xr = x + (long long)blockIdx.x * ldx;
    float s = 0.f;
    for (int i = threadIdx.x; i < d; i += 64) s = fmaf(xr[i], xr[i], s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
    float* yr = y + (long long)blockIdx.x * ldy;
    for (int i = threadIdx.x; i < d; i += 64) yr[i] = xr[i] / nrm;
}

// y[g][c] = (sum over the group's rows, in row order) / rows_per_group
__global__ __launch_bounds__(TPB) void group_mean_kernel(const float* x, int rows_per_group, int groups, int d, float* y) {
    const long long total = (long long)groups * d;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long g = i / d;
        const int c = (int)(i - g * d);
        const float* xg = x + g * rows_per_group * d + c;
        float s = xg[0];
        for (int r = 1; r < rows_per_group; ++r) s += xg[(long long)r * d];
        y[i] = s / (float)rows_per_group;
    }
}

}  // namespace

extern "C" int svcmi_lstm_step_f32(const float* gx, int64_t gx_bstride, const float* whh, float* hseq, int64_t h_bstride, int32_t ldh,
                                   float* c, int32_t ldc, int32_t batch, int32_t hidden, int32_t t, int32_t t_total, void* stream) {
    if (!gx || !whh || !hseq || !c || batch < 1 || t_total < 1 || hidden < 1 || t < 0 || t >= t_total) return SVCMI_EINVAL;
    if (ldh < hidden || ldc < hidden || h_bstride < (int64_t)t_total * ldh || gx_bstride < 4LL * hidden) return SVCMI_EINVAL;
    if (batch > 16 * LMT_MAX) return SVCMI_EUNSUPPORTED;
    if (hidden % LU || ldh % 4 || h_bstride % 4 || ((uintptr_t)whh & 15) || ((uintptr_t)hseq & 15) || ((uintptr_t)gx & 3) || ((uintptr_t)c & 3))
        return SVCMI_EALIGN;
    const dim3 grid((unsigned)(hidden / LU));
    const float* g = gx + (int64_t)t * 4 * hidden;
    switch ((batch + 15) / 16) {
    case 1: SVCMI_LAUNCH(lstm_step_kernel<1>, grid, dim3(TPB), 0, stream, g, (long long)gx_bstride, whh, hseq, (long long)h_bstride, ldh, c, ldc, batch, hidden, t); break;
    case 2: SVCMI_LAUNCH(lstm_step_kernel<2>, grid, dim3(TPB), 0, stream, g, (long long)gx_bstride, whh, hseq, (long long)h_bstride, ldh, c, ldc, batch, hidden, t); break;
    case 3: SVCMI_LAUNCH(lstm_step_kernel<3>, grid, dim3(TPB), 0, stream, g, (long long)gx_bstride, whh, hseq, (long long)h_bstride, ldh, c, ldc, batch, hidden, t); break;
    default: SVCMI_LAUNCH(lstm_step_kernel<4>, grid, dim3(TPB), 0, stream, g, (long long)gx_bstride, whh, hseq, (long long)h_bstride, ldh, c, ldc, batch, hidden, t); break;
    }
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_preemph_pad_f32(const float* x, float* y, int32_t batch, int64_t n, int32_t pad, float coef, void* stream) {
    if (!x || !y || batch <= 0 || n <= 0 || pad < 0 || pad >= n) return SVCMI_EINVAL;
    if (batch > 65535) return SVCMI_EUNSUPPORTED;
    long long nb = (n + 2LL * pad + TPB - 1) / TPB;
    if (nb > 4096) nb = 4096;
    SVCMI_LAUNCH(preemph_pad_kernel, dim3((unsigned)nb, batch), dim3(TPB), 0, stream, x, y, (long long)n, pad, coef);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_magnitude_spectrum_f32(const float* ri, float* p, int64_t rows, int32_t nbins, int32_t half, int32_t ldri, int32_t ldp, void* stream) {
    if (!ri || !p || rows <= 0 || nbins <= 0 || half < nbins || ldri < half + nbins || ldp < nbins) return SVCMI_EINVAL;
    long long nb = (rows * ldp + TPB - 1) / TPB;
    if (nb > 4096) nb = 4096;
    SVCMI_LAUNCH(magnitude_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, ri, p, (long long)rows, nbins, half, ldri, ldp);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_speaker_mel_finish_f32(float* mel, int64_t total, float ref_level_db, float min_level_db, float max_norm, void* stream) {
    if (!mel || total <= 0 || !(min_level_db < 0.f) || !(max_norm > 0.f)) return SVCMI_EINVAL;
    long long nb = (total + TPB - 1) / TPB;
    if (nb > 4096) nb = 4096;
    SVCMI_LAUNCH(speaker_mel_finish_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, mel, (long long)total, ref_level_db, min_level_db, max_norm);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_l2norm_rows_f32(const float* x, int64_t ldx, int32_t rows, int32_t d, float* y, int64_t ldy, void* stream) {
    if (!x || !y || rows <= 0 || d <= 0 || ldx < d || ldy < d) return SVCMI_EINVAL;
    SVCMI_LAUNCH(l2norm_rows_kernel, dim3((unsigned)rows), dim3(64), 0, stream, x, (long long)ldx, d, y, (long long)ldy);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_group_mean_f32(const float* x, int32_t rows_per_group, int32_t groups, int32_t d, float* y, void* stream) {
    if (!x || !y || rows_per_group <= 0 || groups <= 0 || d <= 0) return SVCMI_EINVAL;
    long long nb = ((long long)groups * d + TPB - 1) / TPB;
    if (nb > 4096) nb = 4096;
    SVCMI_LAUNCH(group_mean_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, x, rows_per_group, groups, d, y);
    return SVCMI_LAST_ERROR();
}
