// Attention-transfer distillation (the feature term of compute_lost_KD4, reference utils/utils.py:553-563) on the engines' own buffers:
//   yh_kd_attention      A[n, p] = sum_c |y[n, p, c]| of every feature, straight from the NHWC activations, ONE launch over a row table
//   yh_kd_attention_kl   KLDivLoss(sum)(log_softmax(A_s / T), softmax(A_t / T)) * T * T / batch and G = p_s - p_t, one workgroup per row
//   yh_kd_inject         grad(y)[n, p, c] += fl32(g * (T / batch) * G[n, p]) * sign(y[n, p, c]) into the NHWC gradient buffers
// The reference hands out ~70 NCHW fp32 copies per model and step for this; here nothing but the maps (one float per pixel) is written.
// No float atomics: every sum has a fixed order, the bits repeat from run to run.
#include "common.h"

namespace yh {

constexpr int KD_THREADS = 256;
constexpr int KD_GRID_CAP = 4096;       // 256 CUs x 16 workgroups: beyond that the workgroups stride over the chunks
constexpr int KD_LANES = 8;             // lanes that share a pixel of >= 64 channels
constexpr int KL_THREADS = YH_KD_KL_THREADS;
constexpr int KL_WAVES = KL_THREADS / 64;
constexpr int FIN_THREADS = 256;
static_assert(YH_KD_CHUNK % (KD_THREADS / KD_LANES) == 0, "a full chunk is a whole number of shared-pixel passes");

// chunk -> row: the last row whose chunk0 <= c (workgroup-uniform binary search, as csrc/ema.hip)
__device__ __forceinline__ int kd_find_row(const yh_kd_row* __restrict__ rows, const int n_rows, const int64_t c) {
    int lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// eight consecutive channels as floats (16 bytes of f16, 32 bytes of f32; the address is 16-byte aligned by the table's contract)
template <typename T> struct Vec8;
template <> struct Vec8<f16> {
    float v[8];
    __device__ __forceinline__ void load(const f16* p) {
        const f16x8 t = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (float)t[k];
    }
    __device__ __forceinline__ void store(f16* p) const {
        f16x8 t;
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = (f16)v[k];
        *reinterpret_cast<f16x8*>(p) = t;
    }
};
template <> struct Vec8<float> {
    float v[8];
    __device__ __forceinline__ void load(const float* p) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
    }
    __device__ __forceinline__ void store(float* p) const {
        f32x4 a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = v[k]; b[k] = v[4 + k]; }
        reinterpret_cast<f32x4*>(p)[0] = a;
        reinterpret_cast<f32x4*>(p)[1] = b;
    }
};

template <typename T>
__device__ __forceinline__ void attention_chunk(const yh_kd_row& row, const int64_t pix0, const int cnt, float* __restrict__ out) {
#pragma clang fp contract(off)
    const T* __restrict__ const y = reinterpret_cast<const T*>(row.y) + row.c_off;
    const int vpp = row.c >> 3;
    float* __restrict__ const o = out + row.out_off;
    if (vpp < KD_LANES) {                          // few channels: one lane per pixel, channel 0 upwards
        for (int i = threadIdx.x; i < cnt; i += KD_THREADS) {
            const int64_t q = pix0 + i;
            float s = 0.f;
            for (int g = 0; g < vpp; ++g) {
                Vec8<T> t;
                t.load(y + q * row.ld + g * 8);
#pragma unroll
                for (int k = 0; k < 8; ++k) s += fabsf(t.v[k]);
            }
            o[q] = s;
        }
        return;
    }
    const int j = threadIdx.x & (KD_LANES - 1);
    // the 8 lanes of a pixel enter and leave the loop together (i does not depend on j), so the butterfly only meets live lanes
    for (int i = threadIdx.x / KD_LANES; i < cnt; i += KD_THREADS / KD_LANES) {
        const int64_t q = pix0 + i;
        float s = 0.f;
        for (int g = j; g < vpp; g += KD_LANES) {
            Vec8<T> t;
            t.load(y + q * row.ld + g * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) s += fabsf(t.v[k]);
        }
#pragma unroll
        for (int m = KD_LANES / 2; m; m >>= 1) s += __shfl_xor(s, m, KD_LANES);
        if (j == 0) o[q] = s;
    }
}

__global__ __launch_bounds__(KD_THREADS) void kd_attention_kernel(const yh_kd_row* __restrict__ rows, const int n_rows, const int64_t n_chunks,
                                                                  float* __restrict__ out) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const yh_kd_row row = rows[kd_find_row(rows, n_rows, c)];
        const int64_t total = (int64_t)row.n * row.hw;
        const int64_t pix0 = (c - row.chunk0) * YH_KD_CHUNK;
        if (pix0 < 0 || pix0 >= total) continue;       // a chunk index the table does not cover: touch nothing
        const int cnt = (int)(total - pix0 < YH_KD_CHUNK ? total - pix0 : YH_KD_CHUNK);
        if (row.dtype == YH_F16) attention_chunk<f16>(row, pix0, cnt, out);
        else attention_chunk<float>(row, pix0, cnt, out);
    }
}

// torch.sign: (0 < x) - (x < 0); +0, -0 and NaN give 0
__device__ __forceinline__ float kd_sign(float x) { return (float)((0.f < x) - (x < 0.f)); }

template <typename T>
__device__ __forceinline__ void inject_chunk(const yh_kd_row& row, const int64_t pix0, const int cnt, const float* __restrict__ G, const float gc) {
#pragma clang fp contract(off)
    const T* __restrict__ const y = reinterpret_cast<const T*>(row.y) + row.c_off;
    T* __restrict__ const dy = reinterpret_cast<T*>(row.dy) + row.c_off;
    const int vpp = row.c >> 3;
    const int items = cnt * vpp;                   // <= 256 pixels x (2^31 / 8 / 256) groups: the table's c keeps this inside int
    for (int idx = threadIdx.x; idx < items; idx += KD_THREADS) {
        const int i = idx / vpp, g = idx - i * vpp;
        const int64_t q = pix0 + i;
        const float t = __fmul_rn(gc, G[row.out_off + q]);
        const int64_t e = q * row.ld + g * 8;
        Vec8<T> a, d;
        a.load(y + e);
        d.load(dy + e);
#pragma unroll
        for (int k = 0; k < 8; ++k) d.v[k] = __fadd_rn(d.v[k], __fmul_rn(t, kd_sign(a.v[k])));
        d.store(dy + e);
    }
}

__global__ __launch_bounds__(KD_THREADS) void kd_inject_kernel(const yh_kd_row* __restrict__ rows, const int n_rows, const int64_t n_chunks,
                                                               const float* __restrict__ G, const float* __restrict__ g, const float coef) {
    const float gc = __fmul_rn(g[0], coef);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const yh_kd_row row = rows[kd_find_row(rows, n_rows, c)];
        const int64_t total = (int64_t)row.n * row.hw;
        const int64_t pix0 = (c - row.chunk0) * YH_KD_CHUNK;
        if (pix0 < 0 || pix0 >= total) continue;
        const int cnt = (int)(total - pix0 < YH_KD_CHUNK ? total - pix0 : YH_KD_CHUNK);
        if (row.dtype == YH_F16) inject_chunk<f16>(row, pix0, cnt, G, gc);
        else inject_chunk<float>(row, pix0, cnt, G, gc);
    }
}

// Workgroup reductions of the KL kernel: a butterfly inside each wave, the 16 wave results through LDS, every thread then adds
// (or compares) them in wave order - one fixed order, the same value in every thread.
template <bool MAX> __device__ __forceinline__ float kl_block_reduce(float v, float* red) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        const float o = __shfl_xor(v, m, 64);
        v = MAX ? fmaxf(v, o) : v + o;
    }
    __syncthreads();                               // the previous reduction's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < KL_WAVES; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

__global__ __launch_bounds__(KL_THREADS) void kd_attention_kl_kernel(const float* __restrict__ a_s, const float* __restrict__ a_t,
                                                                     float* __restrict__ G, const yh_kd_kl_row* __restrict__ rows,
                                                                     float* __restrict__ partials, const float inv_T) {
#pragma clang fp contract(off)
    __shared__ float red[KL_WAVES];
    const yh_kd_kl_row row = rows[blockIdx.x];
    const float* __restrict__ const s = a_s + row.off;
    const float* __restrict__ const t = a_t + row.off;
    float* __restrict__ const gout = G + row.off;
    const int len = row.len;
    float ms = -INFINITY, mt = -INFINITY;
    for (int i = threadIdx.x; i < len; i += KL_THREADS) {
        ms = fmaxf(ms, s[i]);
        mt = fmaxf(mt, t[i]);
    }
    ms = kl_block_reduce<true>(ms, red);
    mt = kl_block_reduce<true>(mt, red);
    float ss = 0.f, st = 0.f;
    for (int i = threadIdx.x; i < len; i += KL_THREADS) {
        ss += expf((s[i] - ms) * inv_T);
        st += expf((t[i] - mt) * inv_T);
    }
    ss = kl_block_reduce<false>(ss, red);
    st = kl_block_reduce<false>(st, red);
    const float ls = logf(ss), lt = logf(st);
    float kl = 0.f;
    for (int i = threadIdx.x; i < len; i += KL_THREADS) {
        const float xs = (s[i] - ms) * inv_T - ls, xt = (t[i] - mt) * inv_T - lt;      // log p_s, log p_t
        const float ps = expf(xs), pt = expf(xt);
        gout[i] = ps - pt;
        kl += pt > 0.f ? pt * (xt - xs) : 0.f;
    }
    kl = kl_block_reduce<false>(kl, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = kl;
}

// loss = (sum of the row partials) * T * T / batch: thread k adds rows k, k + 256, ... in order, then a fixed tree over the 256 sums
__global__ __launch_bounds__(FIN_THREADS) void kd_kl_finish_kernel(const float* __restrict__ partials, const int n_rows, float* __restrict__ loss,
                                                                   const float tt, const float batch) {
#pragma clang fp contract(off)
    __shared__ float red[FIN_THREADS];
    float v = 0.f;
    for (int r = threadIdx.x; r < n_rows; r += FIN_THREADS) v += partials[r];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int m = FIN_THREADS / 2; m; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = __fdiv_rn(__fmul_rn(red[0], tt), batch);
}

}  // namespace yh

static int kd_table_check(const void* rows, int n_rows, int64_t n_chunks) {
    if (n_rows < 0 || n_chunks < 0) return YH_EINVAL;
    if (n_rows == 0) return YH_OK;
    if (!rows || n_chunks < n_rows) return YH_EINVAL;
    if (((uintptr_t)rows) & 7u) return YH_EALIGN;
    return 1;
}

extern "C" int yh_kd_attention(const yh_kd_row* rows, int n_rows, int64_t n_chunks, float* out, void* stream) {
    const int rc = kd_table_check(rows, n_rows, n_chunks);
    if (rc != 1) return rc;
    if (!out) return YH_EINVAL;
    if (((uintptr_t)out) & 3u) return YH_EALIGN;
    const int64_t grid = n_chunks < yh::KD_GRID_CAP ? n_chunks : yh::KD_GRID_CAP;
    hipLaunchKernelGGL(yh::kd_attention_kernel, dim3((unsigned)grid), dim3(yh::KD_THREADS), 0, (hipStream_t)stream, rows, n_rows, n_chunks, out);
    return yh::check_launch();
}

extern "C" int yh_kd_attention_kl(const float* a_s, const float* a_t, float* G, const yh_kd_kl_row* rows, int n_rows, float* partials,
                                  float* loss, float T, int batch, void* stream) {
    if (n_rows < 0 || !(T > 0.f) || batch <= 0) return YH_EINVAL;
    if (!loss) return YH_EINVAL;
    if (n_rows > 0) {
        if (!a_s || !a_t || !G || !rows || !partials) return YH_EINVAL;
        if ((((uintptr_t)rows) & 7u) || ((((uintptr_t)a_s) | ((uintptr_t)a_t) | ((uintptr_t)G) | ((uintptr_t)partials)) & 3u)) return YH_EALIGN;
        hipLaunchKernelGGL(yh::kd_attention_kl_kernel, dim3((unsigned)n_rows), dim3(yh::KL_THREADS), 0, (hipStream_t)stream, a_s, a_t, G, rows,
                           partials, 1.f / T);
        const int rc = yh::check_launch();
        if (rc != YH_OK) return rc;
    }
    // no rows: the sum is empty and the loss 0, written by the same finishing launch
    hipLaunchKernelGGL(yh::kd_kl_finish_kernel, dim3(1), dim3(yh::FIN_THREADS), 0, (hipStream_t)stream, partials, n_rows, loss, T * T, (float)batch);
    return yh::check_launch();
}

extern "C" int yh_kd_inject(const yh_kd_row* rows, int n_rows, int64_t n_chunks, const float* G, const float* g, float coef, void* stream) {
    const int rc = kd_table_check(rows, n_rows, n_chunks);
    if (rc != 1) return rc;
    if (!G || !g) return YH_EINVAL;
    if ((((uintptr_t)G) | ((uintptr_t)g)) & 3u) return YH_EALIGN;
    const int64_t grid = n_chunks < yh::KD_GRID_CAP ? n_chunks : yh::KD_GRID_CAP;
    hipLaunchKernelGGL(yh::kd_inject_kernel, dim3((unsigned)grid), dim3(yh::KD_THREADS), 0, (hipStream_t)stream, rows, n_rows, n_chunks, G, g, coef);
    return yh::check_launch();
}
