// sweep.hip -- the two kernels of the key sweep (svc_inference_shift.py: one clip rendered at every transposition of a range).
// Across keys only the pitch changes, so the prior encoder's two front convolutions run once at batch 1 and these kernels fan their
// masked sum out to one row block per key:
//   sweep_pitch_kernel   pit_k[k][t] = (float)((double)pit[t] * factors[k])     -- the reference's float64 product, then FloatTensor
//   sweep_embed_kernel   x[k][t][:] = (xs[t][:] + emb[f0_to_coarse(pit_k[k][t])][:]) * mask
// Both are one-pass streaming kernels like the rest of the prior encoder's glue (vits_elem.hip): float4 lanes, channel index fastest,
// the key on blockIdx.y so that everything a block needs of its key (the factor, the row bases) is wave-uniform.  xs is read once per
// key (T x H floats: resident in L2 after the first key), x is written once.
//
// The singer sweep (svcmi.svc_inference_singers: one clip in many timbres) shares more: nothing up to the prior statistics sees the
// speaker, so the whole prior encoder runs once at batch 1 and ONE kernel fans its m | logs out to a noise draw per singer:
//   sweep_sample_prior_kernel   z[r][t][:] = (m[t][:] + noise[r][:][t] * exp(logs[t][:])) * mask
// the 32 x 32 LDS-transposed tile of sample_prior_kernel (vits_elem.hip) with the arithmetic of prior_sample.h.  A block keeps m and
// exp(logs) of its tile in registers (4 + 4 per thread, one expf per element whatever the number of rows) and walks a contiguous group
// of rows, each row's noise tile through a double-buffered [32][33] LDS transpose (one barrier per row).  Rows per block: the rows are
// split over blockIdx.z into the fewest groups that bring the grid to 512 blocks (two per CU) or to one row per block, whichever comes
// first -- at base widths one chunk is about 31 x 6 tiles, so 16 singers go as 3 groups of 6, 6 and 4 rows.  Glue: memory-bound,
// microseconds; what the sweep saves is the S - 1 prior encoders that do not run.
#include "svcmi_rt.h"
#include "../../include/svcmi.h"
#include "pitch_coarse.h"
#include "prior_sample.h"

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

__global__ __launch_bounds__(TPB) void sweep_sample_prior_kernel(const float* stats, int lds_, const float* noise, const int32_t* length,
                                                                 float* z, int ldz, int n_rows, int rows_per_block, int t, int ic) {
    __shared__ float tile[2][32][33];
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int r0 = blockIdx.z * rows_per_block, r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int len = length ? length[0] : t;
    const int c = c0 + tx;
    float m[4], e[4];                                           // the thread's four elements of the tile: stats[t0+ty+8j][c], once for all rows
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tt = t0 + ty + 8 * j;
        const bool in = tt < t && c < ic;
        const float* sp = stats + (long long)tt * lds_;
        m[j] = in ? sp[c] : 0.f;
        e[j] = in ? prior_scale(sp[ic + c]) : 0.f;
    }
    for (int r = r0; r < r1; ++r) {
        float(*tl)[33] = tile[(r - r0) & 1];                    // two buffers: the barrier of row r + 1 separates row r's reads from row r + 2's writes
        const float* nb = noise + (long long)r * ic * t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                           // noise[r][c0+k][t0+tx]
            const int k = ty + 8 * j, cn = c0 + k, tn = t0 + tx;
            tl[k][tx] = (cn < ic && tn < t) ? nb[(long long)cn * t + tn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {                           // z[r][t0+k][c0+tx]
            const int k = ty + 8 * j, tt = t0 + k;
            if (tt < t && c < ic) prior_sample_store(z + ((long long)r * t + tt) * ldz + c, m[j], tl[tx][k], e[j], tt < len);
        }
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

extern "C" int svcmi_sweep_sample_prior_f32(const float* stats, int32_t lds, const float* noise_ncl, const int32_t* length, float* z,
                                            int32_t ldz, int32_t n_rows, int32_t t, int32_t i, void* stream) {
    if (!stats || !noise_ncl || !z || n_rows <= 0 || t <= 0 || i <= 0 || lds < 2 * i || ldz < i) return SVCMI_EINVAL;
    if (n_rows > SVCMI_SINGERS_MAX) return SVCMI_EUNSUPPORTED;
    if (mis(stats, 4) || mis(noise_ncl, 4) || mis(z, 4) || mis(length, 4)) return SVCMI_EALIGN;
    const int gx = (t - 1) / 32 + 1, gy = (i - 1) / 32 + 1;
    if (gy > 65535) return SVCMI_EUNSUPPORTED;
    // the fewest row groups that bring the grid to 512 blocks, at most one group per row
    const long long tiles = (long long)gx * gy;
    long long groups = (512 + tiles - 1) / tiles;
    if (groups > n_rows) groups = n_rows;
    const int rows_per_block = (int)((n_rows + groups - 1) / groups);
    const int gz = (n_rows + rows_per_block - 1) / rows_per_block;
    SVCMI_LAUNCH(sweep_sample_prior_kernel, dim3(gx, gy, gz), dim3(TPB), 0, stream, stats, lds, noise_ncl, length, z, ldz, n_rows,
                 rows_per_block, t, i);
    return SVCMI_LAST_ERROR();
}
