// sweep.hip -- the two kernels of the key sweep (svc_inference_shift.py: one clip rendered at every transposition of a range).
// Across keys only the pitch changes, so the prior encoder's two front convolutions run once at batch 1 and these kernels fan their
// masked sum out to one row block per key:
//   sweep_pitch_kernel   pit_k[k][t] = (float)((double)pit[t] * factors[k])     -- the reference's float64 product, then FloatTensor
//   sweep_embed_kernel   x[k][t][:] = (xs[t][:] + emb[f0_to_coarse(pit_k[k][t])][:]) * mask
// Both are one-pass streaming kernels like the rest of the prior encoder's glue (vits_elem.hip): float4 lanes, channel index fastest,
// the key on blockIdx.y so that everything a block needs of its key (the factor, the row bases) is wave-uniform.  xs is read once per
// key (T x H floats: resident in L2 after the first key), x is written once.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"
#include "pitch_coarse.h"

namespace {

constexpr int TPB = 256;

// the factors travel in the kernel arguments: plain data, no device table to manage
struct SweepFactors { double f[SVCMI_SWEEP_MAX_KEYS]; };

__global__ __launch_bounds__(TPB) void sweep_pitch_kernel(const float* pit, SweepFactors fac, float* pit_k, int t) {
    const int k = blockIdx.y;
    const double f = fac.f[k];
    float* out = pit_k + (long long)k * t;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < t; i += gridDim.x * TPB) out[i] = (float)((double)pit[i] * f);
}

// the operation order of embed_pitch_kernel (vits_elem.hip): (v + e) * m per lane, so a key's rows carry the bits of the solo path
__global__ __launch_bounds__(TPB) void sweep_embed_kernel(const float* xs, int ldxs, const float* pit_k, const float* emb,
                                                          const int32_t* length, float* x, int ldx, int t, int c) {
    const int k = blockIdx.y;
    const int c4 = c >> 2;
    const long long total = (long long)t * c4;
    const int len = length ? length[0] : t;
    const float* pk = pit_k + (long long)k * t;
    float* xk = x + (long long)k * t * ldx;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int tt = (int)(i / c4);
        const int cc = (int)(i - (long long)tt * c4) * 4;
        const float m = tt < len ? 1.f : 0.f;
        const int bin = f0_to_coarse_dev(pk[tt]);
        const float4 e = *reinterpret_cast<const float4*>(emb + (long long)bin * c + cc);
        float4 v = *reinterpret_cast<const float4*>(xs + (long long)tt * ldxs + cc);
        v.x = (v.x + e.x) * m; v.y = (v.y + e.y) * m; v.z = (v.z + e.z) * m; v.w = (v.w + e.w) * m;
        *reinterpret_cast<float4*>(xk + (long long)tt * ldx + cc) = v;
    }
}

inline unsigned blocks_for(long long total) {
    const long long nb = (total + TPB - 1) / TPB;
    const long long cap = 256 * 8;   // CUs x blocks/CU over all keys' rows at most, grid-stride beyond that
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

inline bool mis(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int svcmi_sweep_pitch_f32(const float* pit, const double* factors, float* pit_k, int32_t n_keys, int32_t t, void* stream) {
    if (!pit || !factors || !pit_k || n_keys <= 0 || t <= 0) return SVCMI_EINVAL;
    if (n_keys > SVCMI_SWEEP_MAX_KEYS) return SVCMI_EUNSUPPORTED;
    if (mis(pit, 4) || mis(pit_k, 4) || mis(factors, 8)) return SVCMI_EALIGN;
    SweepFactors fac;
    for (int k = 0; k < SVCMI_SWEEP_MAX_KEYS; ++k) fac.f[k] = k < n_keys ? factors[k] : 0.0;
    SVCMI_LAUNCH(sweep_pitch_kernel, dim3(blocks_for(t), n_keys), dim3(TPB), 0, stream, pit, fac, pit_k, t);
    return SVCMI_LAST_ERROR();
}

extern "C" int svcmi_sweep_embed_f32(const float* xs, int32_t ldxs, const float* pit_k, const float* emb, const int32_t* length, float* x,
                                     int32_t ldx, int32_t n_keys, int32_t t, int32_t c, void* stream) {
    if (!xs || !pit_k || !emb || !x || n_keys <= 0 || t <= 0 || c <= 0 || ldxs < c || ldx < c) return SVCMI_EINVAL;
    if (n_keys > SVCMI_SWEEP_MAX_KEYS) return SVCMI_EUNSUPPORTED;
    if (c % 4 || ldxs % 4 || ldx % 4 || mis(xs, 16) || mis(x, 16) || mis(emb, 16) || mis(pit_k, 4) || mis(length, 4)) return SVCMI_EALIGN;
    SVCMI_LAUNCH(sweep_embed_kernel, dim3(blocks_for((long long)t * (c / 4)), n_keys), dim3(TPB), 0, stream, xs, ldxs, pit_k, emb, length, x,
                 ldx, t, c);
    return SVCMI_LAST_ERROR();
}
