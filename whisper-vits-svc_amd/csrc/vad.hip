// vad.hip -- the Silero voice-activity detector behind svc_inference_post.py (vad/utils.py get_speech_timestamps; the 16 kHz model of
// vad/assets/silero_vad.jit) and the masking of the converted waveform.
//
// Per window of 512 samples the network is: reflect pad by 96 inside the window -> 8 STFT frames (258 rows of 256 taps, hop 64) ->
// magnitude, log1p(2^20 mag) minus a smoothed mean -> four ConvBlocks (depthwise k = 5, pointwise, residual) with three stride-2 and one
// stride-1 pointwise + BatchNorm + ReLU in between -> ONE 64-vector -> one step of a 2-layer LSTM(64, 64) whose state runs from window to
// window -> sigmoid(w . relu(h) + b).  Everything in front of the LSTM is independent per window; only the LSTM is serial.
//
//   vad_frontend_kernel   one block per (window, recording): all of the convolutional part in LDS, the 64-vector and the layer-0 gate
//                         pre-activations W_ih0 x + b_ih0 + b_hh0 written out.  The STFT basis (264 KB) is read from global memory,
//                         transposed at load ([tap][row]) so that a wave reads 64 consecutive floats; every block reads the same
//                         table, which stays in L2.  Every sum is one chain in ascending index order: the bits of a window depend on
//                         its 512 samples and the weights alone -- not on the run, the number of windows or the batch.
//   vad_lstm_scan_kernel  one block per recording, thread j owns gate row j of both layers: its rows of W_hh0, W_ih1, W_hh1 (192 floats)
//                         live in registers for the whole scan (4 waves = 1 per SIMD: the 512-register budget), h and the gate values
//                         go through LDS (every thread reads the same h[k]: broadcast reads), threads 0..63 do the cell updates and the
//                         decoder.  The loop bound is the recording's own window count; no block waits for another.
//   mask_spans_kernel     out[i] = in[i] inside a span (scaled by the integer rate ratio), 0 outside: binary search per sample.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"

namespace {

constexpr int TPB = 256;
constexpr int WIN = 512;               // samples per window
constexpr int PADW = 96;               // reflect padding inside the window
constexpr int XP = WIN + 2 * PADW;     // 704
constexpr int NTAP = 256, HOP = 64, NF = 8, NBIN = 129, NROW = 2 * NBIN;      // 258 basis rows: 0..128 real, 129..257 imaginary
constexpr int LDB = 260;               // row stride of the transposed basis [NTAP][LDB]
constexpr int LDT = 8;                 // time stride of every activation buffer [C][8]
constexpr int HID = 64, G4 = 4 * HID;

// log(1 + y) for y >= 0 as log(u) * y / (u - 1) with u = fl(1 + y) (y itself where u == 1): the rounding of 1 + y cancels in the
// quotient, a few ulp over the whole range.  The library's log1pf expands into double-float arithmetic that the compiler packs into
// v_pk_add_f32 with the src1 half-select -- the operand form isa_audit.py keeps out of this library.
__device__ __forceinline__ float vad_log1p(float y) {
    const float u = 1.0f + y;
    return u == 1.0f ? y : logf(u) * (y / (u - 1.0f));
}

// the same formulas as csrc/lstm.hip: exactly 0 / 1 for saturated inputs, never NaN for a finite v
__device__ __forceinline__ float vad_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// y[c][t] = relu(b[c] + sum_{j < 5} w[c][j] x[c][t + j - 2]), zeros outside 0..T-1
__device__ __forceinline__ void vad_dw5_relu(const float* x, float* y, const float* w, const float* b, int C, int T) {
    for (int idx = threadIdx.x; idx < C * T; idx += TPB) {
        const int c = idx / T, t = idx - c * T;
        float s = b[c];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int u = t + j - 2;
            if (u >= 0 && u < T) s = fmaf(w[c * 5 + j], x[c * LDT + u], s);
        }
        y[c * LDT + t] = fmaxf(s, 0.f);
    }
}

// b[o] + sum_{c < cin} w[o][c] x[c][t * stride], c ascending
__device__ __forceinline__ float vad_pw(const float* x, const float* w, const float* b, int cin, int o, int col) {
    float s = b[o];
    const float* wr = w + o * cin;
    for (int c = 0; c < cin; ++c) s = fmaf(wr[c], x[c * LDT + col], s);
    return s;
}

// ConvBlock: y = relu(pw(relu(dw(x))) + res(x)); res = the 1x1 `proj` or the identity.  The two sums of an output run on two threads.
__device__ __forceinline__ void vad_conv_block(const svcmi_vad_conv_block& k, const float* x, float* d, float* y, float* ta, float* tb, int T) {
    vad_dw5_relu(x, d, k.dw_w, k.dw_b, k.c_in, T);
    __syncthreads();
    const int n = k.c_out * T;
    for (int idx = threadIdx.x; idx < 2 * n; idx += TPB) {
        const int half = idx >= n, rem = half ? idx - n : idx;
        const int o = rem / T, t = rem - o * T;
        if (!half) ta[rem] = vad_pw(d, k.pw_w, k.pw_b, k.c_in, o, t);
        else tb[rem] = k.proj_w ? vad_pw(x, k.proj_w, k.proj_b, k.c_in, o, t) : x[o * LDT + t];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n; idx += TPB) {
        const int o = idx / T, t = idx - o * T;
        y[o * LDT + t] = fmaxf(ta[idx] + tb[idx], 0.f);
    }
    __syncthreads();
}

// 1x1 convolution with a stride, BatchNorm (eval) as scale / shift, ReLU: y[o][t] = relu(scale[o] (b[o] + sum_c w[o][c] x[c][t stride]) + shift[o])
__device__ __forceinline__ void vad_down(const svcmi_vad_down& k, const float* x, float* y, int T_out) {
    for (int idx = threadIdx.x; idx < k.c * T_out; idx += TPB) {
        const int o = idx / T_out, t = idx - o * T_out;
        y[o * LDT + t] = fmaxf(fmaf(vad_pw(x, k.w, k.b, k.c, o, t * k.stride), k.scale[o], k.shift[o]), 0.f);
    }
    __syncthreads();
}

__global__ __launch_bounds__(TPB) void vad_frontend_kernel(svcmi_vad_model m, const float* audio, const long long* offsets, const long long* lengths,
                                                           int wmax, float* feat, float* gates) {
    __shared__ __attribute__((aligned(16))) float xp[XP];
    __shared__ float st[NROW * LDT];      // STFT sums, later the depthwise output
    __shared__ float xin[NROW * LDT];     // cat(mag, norm): the first ConvBlock's input
    __shared__ float sl[NBIN * LDT];      // log1p(2^20 mag)
    __shared__ float ta[16 * LDT], tb[16 * LDT];      // (c_out * T <= 128 in every block)
    __shared__ float a0[64 * LDT], a1[64 * LDT];
    __shared__ float mean8[NF + 1];
    const int tid = threadIdx.x, b = blockIdx.y, w = blockIdx.x;
    const long long len = lengths[b];
    if ((long long)w * WIN >= len) return;                                  // the recording has fewer windows (block-uniform: before any barrier)
    const float* x = audio + offsets[b] + (long long)w * WIN;
    const long long left = len - (long long)w * WIN;                        // samples of this window inside the recording; the rest are zeros
    for (int i = tid; i < XP; i += TPB) {
        int j = i - PADW;
        if (j < 0) j = -j;
        if (j >= WIN) j = 2 * (WIN - 1) - j;
        xp[i] = j < left ? x[j] : 0.f;
    }
    __syncthreads();
    // ---- STFT: thread r < 256 owns basis row r for all 8 frames; rows 256, 257 x 8 frames are 16 more sums on threads 0..15
    {
        float acc[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = 0.f;
        const float* bt = m.basis_t + tid;
        for (int i = 0; i < NTAP; i += 4) {
            const float b0 = bt[(i + 0) * LDB], b1 = bt[(i + 1) * LDB], b2 = bt[(i + 2) * LDB], b3 = bt[(i + 3) * LDB];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float4 v = *reinterpret_cast<const float4*>(&xp[f * HOP + i]);
                acc[f] = fmaf(b3, v.w, fmaf(b2, v.z, fmaf(b1, v.y, fmaf(b0, v.x, acc[f]))));
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) st[tid * LDT + f] = acc[f];
        if (tid < 2 * NF) {
            const int r = NTAP + (tid >> 3), f = tid & 7;
            const float* br = m.basis_t + r;
            float s = 0.f;
            for (int i = 0; i < NTAP; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(&xp[f * HOP + i]);
                s = fmaf(br[(i + 3) * LDB], v.w, fmaf(br[(i + 2) * LDB], v.z, fmaf(br[(i + 1) * LDB], v.y, fmaf(br[i * LDB], v.x, s))));
            }
            st[r * LDT + f] = s;
        }
    }
    __syncthreads();
    // ---- magnitude and its compressed copy
    for (int idx = tid; idx < NBIN * NF; idx += TPB) {
        const float re = st[idx], im = st[NBIN * LDT + idx];
        const float mag = sqrtf(fmaf(re, re, im * im));
        xin[idx] = mag;
        sl[idx] = vad_log1p(mag * 1048576.0f);
    }
    __syncthreads();
    // ---- the normaliser: per-frame mean over the bins, reflect-extended by 3, smoothed by the 7 taps, averaged to one scalar
    if (tid < NF) {
        float s = 0.f;
        for (int k = 0; k < NBIN; ++k) s += sl[k * LDT + tid];
        mean8[tid] = s / (float)NBIN;
    }
    __syncthreads();
    if (tid == 0) {
        float e[NF + 6];
        for (int i = 0; i < NF + 6; ++i) {
            int j = i - 3;
            if (j < 0) j = -j;
            if (j >= NF) j = 2 * (NF - 1) - j;
            e[i] = mean8[j];
        }
        float mu = 0.f;
        for (int t = 0; t < NF; ++t) {
            float s = 0.f;
            for (int j = 0; j < 7; ++j) s = fmaf(m.filt[j], e[t + j], s);
            mu += s;
        }
        mean8[NF] = mu / (float)NF;
    }
    __syncthreads();
    {
        const float mu = mean8[NF];
        for (int idx = tid; idx < NBIN * NF; idx += TPB) xin[NBIN * LDT + idx] = sl[idx] - mu;
    }
    __syncthreads();
    // ---- encoder: T = 8 -> 4 -> 2 -> 1
    vad_conv_block(m.block[0], xin, st, a0, ta, tb, 8);      // 258 -> 16
    vad_down(m.down[0], a0, a1, 4);
    vad_conv_block(m.block[1], a1, st, a0, ta, tb, 4);       // 16 -> 32
    vad_down(m.down[1], a0, a1, 2);
    vad_conv_block(m.block[2], a1, st, a0, ta, tb, 2);       // 32 -> 32
    vad_down(m.down[2], a0, a1, 1);
    vad_conv_block(m.block[3], a1, st, a0, ta, tb, 1);       // 32 -> 64
    vad_down(m.down[3], a0, a1, 1);
    const long long row = (long long)b * wmax + w;
    if (tid < HID) feat[row * HID + tid] = a1[tid * LDT];
    {
        float s = m.gate0_b[tid];
        const float* wr = m.gate0_w + tid * HID;
        for (int k = 0; k < HID; ++k) s = fmaf(wr[k], a1[k * LDT], s);
        gates[row * G4 + tid] = s;
    }
}

// h and c of both layers: state[b][0..3][64] = h0, c0, h1, c1 (NULL: start from zero, nothing is written back)
__global__ __launch_bounds__(TPB) void vad_lstm_scan_kernel(svcmi_vad_model m, const float* gates, const long long* lengths, int wmax, float* state,
                                                            float* probs) {
    __shared__ __attribute__((aligned(16))) float h0[HID];
    __shared__ __attribute__((aligned(16))) float h1[HID];
    __shared__ float pre[G4];
    const int j = threadIdx.x, b = blockIdx.x;
    const long long len = lengths[b];
    long long nw = (len + WIN - 1) / WIN;
    if (nw > wmax) nw = wmax;
    float a[HID], u[HID], v[HID];                 // rows j of W_hh0, W_ih1, W_hh1 (stored [k][j]: a wave reads 64 consecutive floats)
#pragma unroll
    for (int k = 0; k < HID; ++k) {
        a[k] = m.whh0_t[k * G4 + j];
        u[k] = m.wih1_t[k * G4 + j];
        v[k] = m.whh1_t[k * G4 + j];
    }
    const float bias1 = m.gate1_b[j];
    float c0 = 0.f, c1 = 0.f, dw = 0.f;
    if (j < HID) {
        dw = m.dec_w[j];
        float* s = state ? state + (long long)b * 4 * HID : nullptr;
        h0[j] = s ? s[j] : 0.f;
        c0 = s ? s[HID + j] : 0.f;
        h1[j] = s ? s[2 * HID + j] : 0.f;
        c1 = s ? s[3 * HID + j] : 0.f;
    }
    __syncthreads();
    const float* g = gates + (long long)b * wmax * G4 + j;
    for (long long w = 0; w < nw; ++w) {
        float p = g[w * G4];
#pragma unroll
        for (int k = 0; k < HID; k += 4) {
            const float4 h = *reinterpret_cast<const float4*>(&h0[k]);
            p = fmaf(a[k + 3], h.w, fmaf(a[k + 2], h.z, fmaf(a[k + 1], h.y, fmaf(a[k], h.x, p))));
        }
        pre[j] = p;
        __syncthreads();
        if (j < HID) {
            c0 = fmaf(vad_sigmoid(pre[HID + j]), c0, vad_sigmoid(pre[j]) * tanhf(pre[2 * HID + j]));
            h0[j] = vad_sigmoid(pre[3 * HID + j]) * tanhf(c0);
        }
        __syncthreads();
        float q = bias1;
#pragma unroll
        for (int k = 0; k < HID; k += 4) {
            const float4 h = *reinterpret_cast<const float4*>(&h0[k]);
            q = fmaf(u[k + 3], h.w, fmaf(u[k + 2], h.z, fmaf(u[k + 1], h.y, fmaf(u[k], h.x, q))));
        }
#pragma unroll
        for (int k = 0; k < HID; k += 4) {
            const float4 h = *reinterpret_cast<const float4*>(&h1[k]);
            q = fmaf(v[k + 3], h.w, fmaf(v[k + 2], h.z, fmaf(v[k + 1], h.y, fmaf(v[k], h.x, q))));
        }
        pre[j] = q;                               // (layer 0's cell update read pre before the barrier above)
        __syncthreads();                          // ... and every thread has read h1 before layer 1's cell update writes it
        if (j < HID) {                            // one wave: the cell update of layer 1, then the decoder as a fixed butterfly
            c1 = fmaf(vad_sigmoid(pre[HID + j]), c1, vad_sigmoid(pre[j]) * tanhf(pre[2 * HID + j]));
            const float h = vad_sigmoid(pre[3 * HID + j]) * tanhf(c1);
            h1[j] = h;
            float d = dw * fmaxf(h, 0.f);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) d += __shfl_xor(d, s);
            if (j == 0) probs[(long long)b * wmax + w] = vad_sigmoid(d + m.dec_b);
        }
        __syncthreads();
    }
    if (state && j < HID) {
        float* s = state + (long long)b * 4 * HID;
        s[j] = h0[j];
        s[HID + j] = c0;
        s[2 * HID + j] = h1[j];
        s[3 * HID + j] = c1;
    }
}

__global__ __launch_bounds__(TPB) void mask_spans_kernel(const float* in, float* out, long long n, const int* spans, int n_spans, int ratio) {
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        int lo = 0, hi = n_spans;                 // the first span whose scaled start lies beyond i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long)spans[2 * mid] * ratio <= i) lo = mid + 1; else hi = mid;
        }
        out[i] = (lo > 0 && i < (long long)spans[2 * lo - 1] * ratio) ? in[i] : 0.f;
    }
}

int vad_model_check(const svcmi_vad_model* m) {
    if (!m || !m->basis_t || !m->filt || !m->gate0_w || !m->gate0_b || !m->whh0_t || !m->wih1_t || !m->whh1_t || !m->gate1_b || !m->dec_w) return SVCMI_EINVAL;
    static const int cin[4] = {NROW, 16, 32, 32}, cout[4] = {16, 32, 32, 64}, stride[4] = {2, 2, 2, 1};
    for (int i = 0; i < 4; ++i) {
        const svcmi_vad_conv_block& k = m->block[i];
        const svcmi_vad_down& d = m->down[i];
        if (!k.dw_w || !k.dw_b || !k.pw_w || !k.pw_b || !d.w || !d.b || !d.scale || !d.shift) return SVCMI_EINVAL;
        if ((k.proj_w == nullptr) != (k.proj_b == nullptr)) return SVCMI_EINVAL;
        if (k.c_in != cin[i] || k.c_out != cout[i] || d.c != cout[i] || d.stride != stride[i]) return SVCMI_EUNSUPPORTED;     // the LDS plan is this architecture's
        if (!k.proj_w && k.c_in != k.c_out) return SVCMI_EINVAL;
    }
    return 0;
}

}  // namespace

extern "C" int64_t svcmi_vad_model_bytes(void) { return (int64_t)sizeof(svcmi_vad_model); }

extern "C" int svcmi_vad_frontend_f32(const svcmi_vad_model* m, const float* audio, const int64_t* offsets, const int64_t* lengths, int32_t batch,
                                      int32_t wmax, float* feat, float* gates, void* stream) {
    if (int rc = vad_model_check(m)) return rc;
    if (!audio || !offsets || !lengths || !feat || !gates || batch < 1 || wmax < 1) return SVCMI_EINVAL;
    if (batch > 65535) return SVCMI_EUNSUPPORTED;
    if (((uintptr_t)audio & 3) || ((uintptr_t)feat & 3) || ((uintptr_t)gates & 3) || ((uintptr_t)offsets & 7) || ((uintptr_t)lengths & 7)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(vad_frontend_kernel, dim3((unsigned)wmax, (unsigned)batch), dim3(TPB), 0, stream, *m, audio, (const long long*)offsets,
                 (const long long*)lengths, wmax, feat, gates);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_vad_lstm_scan_f32(const svcmi_vad_model* m, const float* gates, const int64_t* lengths, int32_t batch, int32_t wmax, float* state,
                                       float* probs, void* stream) {
    if (int rc = vad_model_check(m)) return rc;
    if (!gates || !lengths || !probs || batch < 1 || wmax < 1) return SVCMI_EINVAL;
    if (((uintptr_t)gates & 3) || ((uintptr_t)probs & 3) || ((uintptr_t)state & 3) || ((uintptr_t)lengths & 7)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(vad_lstm_scan_kernel, dim3((unsigned)batch), dim3(TPB), 0, stream, *m, gates, (const long long*)lengths, wmax, state, probs);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_mask_spans_f32(const float* in, int64_t n_in, const int32_t* spans, int32_t n_spans, int64_t n_ref, int32_t ratio, float* out,
                                    int64_t n_out, void* stream) {
    if (!in || !out || n_in < 1 || n_ref < 1 || ratio < 1 || n_spans < 0 || (n_spans > 0 && !spans)) return SVCMI_EINVAL;
    const int64_t n = n_in < n_ref * ratio ? n_in : n_ref * ratio;
    if (n_out != n) return SVCMI_EINVAL;
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)spans & 3)) return SVCMI_EALIGN;
    long long nb = (n + TPB - 1) / TPB;
    if (nb > 4096) nb = 4096;
    SVCMI_LAUNCH(mask_spans_kernel, dim3((unsigned)nb), dim3(TPB), 0, stream, in, out, (long long)n, (const int*)spans, n_spans, ratio);
    return SVCMI_LAST_ERROR();
}
