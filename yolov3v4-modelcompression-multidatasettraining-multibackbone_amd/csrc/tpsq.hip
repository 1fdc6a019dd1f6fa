// TPSQ, learnable power-of-two scales (utils/quantized/quantized_TPSQ.py of this package), on the device.  One quantiser call of the
// reference (utils/quantized/quantized_TPSQ.py:29-63 Search_Pow2, :79-118 clamp / quantize / round / dequantize, :262-282 the warm-up)
// costs four Search_Pow2 applications (about ten one-element launches and a host read each), about ten full-tensor passes forward,
// about a dozen backward plus four full-tensor reductions into the scale's gradient, and on its first call a 99-candidate search of
// about 1500 passes.  Here:
//     tpsq_fake_quant_fwd_kernel                      snap the scale to its power of two p (in the parameter, in place), snapshot {s0, p},
//                                                     y = (round(((0.5 (|x + p| - |x - p|)) qmul) / p) p) / qdiv: one pass
//     tpsq_fake_quant_bwd_kernel + tpsq_grad_final    dx and the four sums of the scale gradient: one pass over x and dy, per-workgroup
//                                                     partials, one finishing wave, no atomics: the same bits on every run
//     tpsq_warmup_partial_kernel + tpsq_warmup_final  the 99 candidates snap to at most nine powers of two: one pass takes sum x^2 and per
//                                                     power sum x y and sum y^2; a finishing wave forms the cosines and applies the
//                                                     reference's choice rule
// Every float operation of the forward and of dx is the one torch performs, in its order, with IEEE division and no contraction (this
// object is built with -ffp-contract=off).
#include "common.h"

#include <math.h>

namespace yh {

constexpr int TPSQ_THREADS = 256;
constexpr int TPSQ_MAX_BLOCKS = 1024;
constexpr int TPSQ_POWERS = 9;                       // 99 step / (1 step) < 2^8 after snapping both ends: exponents k = 0 .. 8 cover it
constexpr int TPSQ_WARM_SUMS = 1 + 2 * TPSQ_POWERS;  // sum x^2, then {sum x y_k, sum y_k^2}

static int tpsq_blocks(long count) {
    long b = (count + (long)TPSQ_THREADS * 16 - 1) / ((long)TPSQ_THREADS * 16);
    if (b < 1) b = 1;
    if (b > TPSQ_MAX_BLOCKS) b = TPSQ_MAX_BLOCKS;
    return (int)b;
}

// The rule of qat.hip's nearest_pow2 (x = m 2^e, m in [0.5, 1): 2^e if m > 0.75 else 2^(e-1); the tie 1.5 2^e goes down), with
// Search_Pow2's results for the values a scale parameter can take (:37-42): +-0 -> +0 (2 ** -inf), +inf -> +inf, negative and NaN -> NaN.
__device__ __forceinline__ float tpsq_pow2(float x) {
    if (x != x || x < 0.f) return NAN;
    if (x == 0.f) return 0.f;
    if (x == INFINITY) return x;
    int e;
    const float m = frexpf(x, &e);
    return ldexpf(1.f, m > 0.75f ? e : e - 1);
}

// torch.sign: (0 < v) - (v < 0), 0 for a NaN
__device__ __forceinline__ float tpsq_sign(float v) { return (float)((0.f < v) - (v < 0.f)); }

struct TpsqChain {
    float a, b, c, m, q, r;
};

// clamp (:84-85), quantize (:90-91) and Round (:19-20) with the snapped scale p
__device__ __forceinline__ TpsqChain tpsq_chain(float x, float p, float qmul) {
    TpsqChain t;
    t.a = x + p;
    t.b = x - p;
    t.c = 0.5f * (fabsf(t.a) - fabsf(t.b));
    t.m = t.c * qmul;
    t.q = __fdiv_rn(t.m, p);
    t.r = tpsq_sign(t.q) * floorf(fabsf(t.q) + 0.5f);
    return t;
}

// dequantize (:101-102)
__device__ __forceinline__ float tpsq_fake_quant(float x, float p, float qmul, float qdiv) { return __fdiv_rn(tpsq_chain(x, p, qmul).r * p, qdiv); }

// The scale is read with one relaxed load per thread and written by one thread.  Whether a thread sees the raw value s0 or the snapped
// p that thread 0 has already stored, it computes the same p: snapping a power of two gives itself (0, inf and NaN too).  Thread 0 is
// the only writer and reads before it writes, so the snapshot's s0 is the raw value.
__global__ __launch_bounds__(TPSQ_THREADS) void tpsq_fake_quant_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long count, float* scale,
                                                                           float qmul, float qdiv, float* __restrict__ snapshot) {
    const float seen = __hip_atomic_load(scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float p = tpsq_pow2(seen);
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 == 0) {
        snapshot[0] = seen;
        snapshot[1] = p;
        __hip_atomic_store(scale, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // Search_Pow2 leaves p in the parameter (:39-42)
    }
    if (((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        f32x4* y4 = reinterpret_cast<f32x4*>(y);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = x4[i];
            f32x4 o;
            o[0] = tpsq_fake_quant(v[0], p, qmul, qdiv); o[1] = tpsq_fake_quant(v[1], p, qmul, qdiv);
            o[2] = tpsq_fake_quant(v[2], p, qmul, qdiv); o[3] = tpsq_fake_quant(v[3], p, qmul, qdiv);
            y4[i] = o;
        }
        for (long i = (n4 << 2) + i0; i < count; i += stride) y[i] = tpsq_fake_quant(x[i], p, qmul, qdiv);
    } else {
        for (long i = i0; i < count; i += stride) y[i] = tpsq_fake_quant(x[i], p, qmul, qdiv);
    }
}

// The four sums of one thread / wave / workgroup: g[k] belongs to the (k+1)-th Search_Pow2 application of the call
struct TpsqSums {
    float g[4];
};

__device__ __forceinline__ TpsqSums tpsq_add(TpsqSums s, const TpsqSums& t) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s.g[k] += t.g[k];
    return s;
}

// Autograd's chain through dequantize, Round, quantize and clamp, operation for operation:
//   g_n = dy / qdiv            g4 term = g_n r        g_r = g_n p        g_q = g_r
//   g_m = g_q / p              g3 term = -g_q ((m / p) / p)
//   g_c = g_m qmul             g_d = g_c 0.5
//   g_a = g_d sign(a)          g_b = (-g_d) sign(b)   dx = g_a + g_b     g1 term = g_a    g2 term = -g_b
__device__ __forceinline__ float tpsq_bwd_element(float x, float dy, float p, float qmul, float qdiv, TpsqSums& t) {
    const TpsqChain f = tpsq_chain(x, p, qmul);
    const float g_n = __fdiv_rn(dy, qdiv);
    const float g_q = g_n * p;
    const float g_m = __fdiv_rn(g_q, p);
    const float g_d = (g_m * qmul) * 0.5f;
    const float g_a = g_d * tpsq_sign(f.a);
    const float g_b = (-g_d) * tpsq_sign(f.b);
    t.g[0] = g_a;
    t.g[1] = -g_b;
    t.g[2] = (-g_q) * __fdiv_rn(__fdiv_rn(f.m, p), p);
    t.g[3] = g_n * f.r;
    return g_a + g_b;
}

// partial[4 * block + k]: every thread adds its elements' terms in a fixed order (the four of a 16-byte load as a two-level tree), the
// wave and the workgroup as trees: the result depends on count and on the alignment alone
__global__ __launch_bounds__(TPSQ_THREADS) void tpsq_fake_quant_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                                           long count, const float* __restrict__ snapshot, float qmul, float qdiv,
                                                                           float* __restrict__ partial) {
    const float p = snapshot[1];
    TpsqSums acc = {{0.f, 0.f, 0.f, 0.f}};
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // one element per step, four steps' terms as a two-level tree like the four of a 16-byte load
    auto scalar_span = [&](long i) {
        for (; i + 3 * stride < count; i += 4 * stride) {
            TpsqSums t0, t1, t2, t3;
            dx[i] = tpsq_bwd_element(x[i], dy[i], p, qmul, qdiv, t0);
            dx[i + stride] = tpsq_bwd_element(x[i + stride], dy[i + stride], p, qmul, qdiv, t1);
            dx[i + 2 * stride] = tpsq_bwd_element(x[i + 2 * stride], dy[i + 2 * stride], p, qmul, qdiv, t2);
            dx[i + 3 * stride] = tpsq_bwd_element(x[i + 3 * stride], dy[i + 3 * stride], p, qmul, qdiv, t3);
            acc = tpsq_add(acc, tpsq_add(tpsq_add(t0, t1), tpsq_add(t2, t3)));
        }
        for (; i < count; i += stride) {
            TpsqSums t;
            dx[i] = tpsq_bwd_element(x[i], dy[i], p, qmul, qdiv, t);
            acc = tpsq_add(acc, t);
        }
    };
    if (((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)dx)) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(dy);
        f32x4* o4 = reinterpret_cast<f32x4*>(dx);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = x4[i], g = g4[i];
            f32x4 o;
            TpsqSums t0, t1, t2, t3;
            o[0] = tpsq_bwd_element(v[0], g[0], p, qmul, qdiv, t0); o[1] = tpsq_bwd_element(v[1], g[1], p, qmul, qdiv, t1);
            o[2] = tpsq_bwd_element(v[2], g[2], p, qmul, qdiv, t2); o[3] = tpsq_bwd_element(v[3], g[3], p, qmul, qdiv, t3);
            o4[i] = o;
            acc = tpsq_add(acc, tpsq_add(tpsq_add(t0, t1), tpsq_add(t2, t3)));
        }
        scalar_span((n4 << 2) + i0);
    } else {
        scalar_span(i0);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.g[k] += __shfl_xor(acc.g[k], d);
    __shared__ float red[TPSQ_THREADS / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[wave][k] = acc.g[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        partial[4 * (long)blockIdx.x + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// One wave: the four sums over the workgroups, then Search_Pow2's backward (:48-51) per application - the first saw s0 and scales its
// sum by p / s0, the others saw p (p / p) - added in the order autograd's engine hands them to the parameter: fourth application first.
__global__ __launch_bounds__(64) void tpsq_grad_final_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ snapshot,
                                                             float* __restrict__ scale_grad) {
    TpsqSums acc = {{0.f, 0.f, 0.f, 0.f}};
    for (int b = threadIdx.x; b < nblocks; b += 64)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.g[k] += partial[4 * b + k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.g[k] += __shfl_xor(acc.g[k], d);
    if (threadIdx.x == 0) {
        const float s0 = snapshot[0], p = snapshot[1];
        const float first = __fdiv_rn(p, s0), later = __fdiv_rn(p, p);
        *scale_grad = ((later * acc.g[3] + later * acc.g[2]) + later * acc.g[1]) + first * acc.g[0];
    }
}

__device__ __forceinline__ double tpsq_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// partial[TPSQ_WARM_SUMS * block + ..]: sum x^2, and for the powers pow2(step) 2^k, k < TPSQ_POWERS, sum x y_k and sum y_k^2 with
// y_k the fake-quantised x.  fp32 element arithmetic as the forward's, products and sums in double.
__global__ __launch_bounds__(TPSQ_THREADS) void tpsq_warmup_partial_kernel(const float* __restrict__ x, long count, const float* __restrict__ step,
                                                                           float qmul, float qdiv, double* __restrict__ partial) {
    const float p0 = tpsq_pow2(*step);      // pow2(step * 1): the lowest candidate
    double acc[TPSQ_WARM_SUMS];
#pragma unroll
    for (int k = 0; k < TPSQ_WARM_SUMS; ++k) acc[k] = 0.0;
    auto take = [&](float v) {
        acc[0] += (double)v * (double)v;
#pragma unroll
        for (int k = 0; k < TPSQ_POWERS; ++k) {
            const float y = tpsq_fake_quant(v, ldexpf(p0, k), qmul, qdiv);
            acc[1 + 2 * k] += (double)v * (double)y;
            acc[2 + 2 * k] += (double)y * (double)y;
        }
    };
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((((uintptr_t)x) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = x4[i];
            take(v[0]); take(v[1]); take(v[2]); take(v[3]);
        }
        for (long i = (n4 << 2) + i0; i < count; i += stride) take(x[i]);
    } else {
        for (long i = i0; i < count; i += stride) take(x[i]);
    }
    __shared__ double red[TPSQ_THREADS / 64][TPSQ_WARM_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < TPSQ_WARM_SUMS; ++k) {
        const double v = tpsq_wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < TPSQ_WARM_SUMS) {
        const int k = threadIdx.x;
        partial[(long)TPSQ_WARM_SUMS * blockIdx.x + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// One wave: the cosines of the distinct powers (torch.cosine_similarity clamps each norm at 1e-8), then the reference's loop (:264-282):
// max_metrics = -1, max_step = -5; candidate i = 1 .. 99 has the scale step * i, which the chain snaps; a strict > keeps the first
// maximum and never takes a NaN.  scale = step * max_step (not snapped: the next forward does that), warmup += -1.
__global__ __launch_bounds__(64) void tpsq_warmup_final_kernel(const double* __restrict__ partial, int nblocks, const float* __restrict__ step,
                                                               float* __restrict__ scale, float* __restrict__ warmup) {
    __shared__ double total[TPSQ_WARM_SUMS];
    for (int k = 0; k < TPSQ_WARM_SUMS; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += 64) v += partial[(long)TPSQ_WARM_SUMS * b + k];
        v = tpsq_wave_sum(v);
        if (threadIdx.x == 0) total[k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float st = *step;
    const float p0 = tpsq_pow2(st);
    const double nx = fmax(sqrt(total[0]), 1e-8);
    double best = -1.0;
    int max_step = -5;
    for (int i = 1; i < 100; ++i) {
        const float p = tpsq_pow2(st * (float)i);
        double cosine = NAN;
        for (int k = 0; k < TPSQ_POWERS; ++k)
            if (p == ldexpf(p0, k)) {
                cosine = (double)(float)(total[1 + 2 * k] / (nx * fmax(sqrt(total[2 + 2 * k]), 1e-8)));
                break;
            }
        if (cosine > best) {
            best = cosine;
            max_step = i;
        }
    }
    *scale = st * (float)max_step;
    *warmup = *warmup + (-1.f);
}

static bool tpsq_misaligned4(const void* p) { return (((uintptr_t)p) & 3u) != 0; }
static bool tpsq_bits_ok(int bits) { return bits >= 2 && bits <= 24; }

}  // namespace yh

using namespace yh;

extern "C" int yh_tpsq_fake_quant_fwd(const float* x, float* y, int64_t count, float* scale, int bits, float* snapshot, void* stream) {
    if (!x || !y || !scale || !snapshot || count <= 0 || !tpsq_bits_ok(bits)) return YH_EINVAL;
    if (tpsq_misaligned4(x) || tpsq_misaligned4(y) || tpsq_misaligned4(scale) || tpsq_misaligned4(snapshot)) return YH_EALIGN;
    hipLaunchKernelGGL(tpsq_fake_quant_fwd_kernel, dim3(tpsq_blocks(count)), dim3(TPSQ_THREADS), 0, (hipStream_t)stream, x, y, (long)count, scale,
                       (float)((1 << (bits - 1)) - 1), (float)(1 << (bits - 1)), snapshot);
    return check_launch();
}

extern "C" int64_t yh_tpsq_grad_workspace(int64_t count) {
    if (count <= 0) return 0;
    return (int64_t)tpsq_blocks(count) * 4 * (int64_t)sizeof(float);
}

extern "C" int yh_tpsq_fake_quant_bwd(const float* x, const float* dy, float* dx, int64_t count, const float* snapshot, int bits, void* ws,
                                      int64_t ws_bytes, float* scale_grad, void* stream) {
    if (!x || !dy || !dx || !snapshot || !ws || !scale_grad || count <= 0 || !tpsq_bits_ok(bits)) return YH_EINVAL;
    if (tpsq_misaligned4(x) || tpsq_misaligned4(dy) || tpsq_misaligned4(dx) || tpsq_misaligned4(snapshot) || tpsq_misaligned4(ws) ||
        tpsq_misaligned4(scale_grad))
        return YH_EALIGN;
    const int blocks = tpsq_blocks(count);
    if (ws_bytes < (int64_t)blocks * 4 * (int64_t)sizeof(float)) return YH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tpsq_fake_quant_bwd_kernel, dim3(blocks), dim3(TPSQ_THREADS), 0, s, x, dy, dx, (long)count, snapshot,
                       (float)((1 << (bits - 1)) - 1), (float)(1 << (bits - 1)), (float*)ws);
    hipLaunchKernelGGL(tpsq_grad_final_kernel, dim3(1), dim3(64), 0, s, (const float*)ws, blocks, snapshot, scale_grad);
    return check_launch();
}

extern "C" int64_t yh_tpsq_warmup_workspace(int64_t count) {
    if (count <= 0) return 0;
    return (int64_t)tpsq_blocks(count) * TPSQ_WARM_SUMS * (int64_t)sizeof(double);
}

extern "C" int yh_tpsq_warmup_search(const float* x, int64_t count, const float* step, int bits, void* ws, int64_t ws_bytes, float* scale,
                                     float* warmup, void* stream) {
    if (!x || !step || !ws || !scale || !warmup || count <= 0 || !tpsq_bits_ok(bits)) return YH_EINVAL;
    if (tpsq_misaligned4(x) || tpsq_misaligned4(step) || (((uintptr_t)ws) & 7u) != 0 || tpsq_misaligned4(scale) || tpsq_misaligned4(warmup))
        return YH_EALIGN;
    const int blocks = tpsq_blocks(count);
    if (ws_bytes < (int64_t)blocks * TPSQ_WARM_SUMS * (int64_t)sizeof(double)) return YH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tpsq_warmup_partial_kernel, dim3(blocks), dim3(TPSQ_THREADS), 0, s, x, (long)count, step, (float)((1 << (bits - 1)) - 1),
                       (float)(1 << (bits - 1)), (double*)ws);
    hipLaunchKernelGGL(tpsq_warmup_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, blocks, step, scale, warmup);
    return check_launch();
}
