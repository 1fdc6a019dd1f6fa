// Quantization-aware training (utils/quantized/quantized_google.py of this package) on the device: what one quantiser call of the
// reference spends about a dozen full-tensor elementwise launches, two reductions and three host reads on
// (reference utils/quantized/quantized_google.py:24-32 RangeTracker.forward, :46-55 / :70-77 update_range, :178-219 update_params,
// :114-153 quantize / round / clamp / dequantize and the step counter) as
//     qat_observe_partial_kernel + qat_observe_final_kernel   min and max in one pass, NaN-propagating like torch.min / torch.max
//     qat_range_update_kernel                                 tracker rule + first-call flag + power-of-two scale + zero point, one wave
//     qat_fake_quant_fwd_kernel                               u = x / s + zp; r = sign(u) floor(|u| + .5); clamp; y = (r - zp) s
//     qat_fake_quant_bwd_kernel                               straight-through estimator with the clamp's mask recomputed from x
// Every float operation is the one torch performs, in its order, with IEEE division and no contraction (this object is built with
// -ffp-contract=off), so the results are the torch formulas' bit for bit.  HBM-bound byte work: the observe pass reads the tensor
// once, the forward reads and writes it once, the backward reads x and dy and writes dx.
#include "common.h"

#include <math.h>

namespace yh {

constexpr int QAT_THREADS = 256;
constexpr int QAT_MAX_BLOCKS = 1024;

static int qat_blocks(long count) {
    long b = (count + (long)QAT_THREADS * 16 - 1) / ((long)QAT_THREADS * 16);
    if (b < 1) b = 1;
    if (b > QAT_MAX_BLOCKS) b = QAT_MAX_BLOCKS;
    return (int)b;
}

// v_min_f32 / v_max_f32 return the other operand when one is a NaN, so a NaN is carried as a flag next to the extremes
struct MinMax {
    float lo, hi;
    int nan;
};

__device__ __forceinline__ void mm_take(MinMax& m, float v) {
    m.lo = fminf(m.lo, v);
    m.hi = fmaxf(m.hi, v);
    m.nan |= (v != v) ? 1 : 0;
}

__device__ __forceinline__ MinMax mm_wave(MinMax m) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m.lo = fminf(m.lo, __shfl_xor(m.lo, d));
        m.hi = fmaxf(m.hi, __shfl_xor(m.hi, d));
        m.nan |= __shfl_xor(m.nan, d);
    }
    return m;
}

// partial[3 * block + {0, 1, 2}] = min, max, NaN flag of the elements this workgroup visited.  Min and max are exact and do not depend
// on the order, so neither do the results.
__global__ __launch_bounds__(QAT_THREADS) void qat_observe_partial_kernel(const float* __restrict__ t, long count, float* __restrict__ partial) {
    MinMax m = {INFINITY, -INFINITY, 0};
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((((uintptr_t)t) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* t4 = reinterpret_cast<const f32x4*>(t);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = t4[i];
            mm_take(m, v[0]); mm_take(m, v[1]); mm_take(m, v[2]); mm_take(m, v[3]);
        }
        for (long i = (n4 << 2) + i0; i < count; i += stride) mm_take(m, t[i]);
    } else {
        for (long i = i0; i < count; i += stride) mm_take(m, t[i]);
    }
    m = mm_wave(m);
    __shared__ float red[QAT_THREADS / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = m.lo; red[wave][1] = m.hi; red[wave][2] = m.nan ? 1.f : 0.f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float lo = red[0][0], hi = red[0][1], nan = red[0][2];
#pragma unroll
        for (int w = 1; w < QAT_THREADS / 64; ++w) { lo = fminf(lo, red[w][0]); hi = fmaxf(hi, red[w][1]); nan = fmaxf(nan, red[w][2]); }
        partial[3 * (long)blockIdx.x + 0] = lo;
        partial[3 * (long)blockIdx.x + 1] = hi;
        partial[3 * (long)blockIdx.x + 2] = nan;
    }
}

// one wave: minmax[0] = min, minmax[1] = max, both NaN when any element was
__global__ __launch_bounds__(64) void qat_observe_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ minmax) {
    MinMax m = {INFINITY, -INFINITY, 0};
    for (int b = threadIdx.x; b < nblocks; b += 64) {
        m.lo = fminf(m.lo, partial[3 * b + 0]);
        m.hi = fmaxf(m.hi, partial[3 * b + 1]);
        m.nan |= partial[3 * b + 2] != 0.f ? 1 : 0;
    }
    m = mm_wave(m);
    if (threadIdx.x == 0) {
        minmax[0] = m.nan ? NAN : m.lo;
        minmax[1] = m.nan ? NAN : m.hi;
    }
}

// torch.min / torch.max of two values: a NaN on either side wins
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

// The power of two nearest to x in absolute distance, the lower one on a tie - reference :189-194 `2 ** log2(x).floor()` against
// `2 ** log2(x).ceil()` - chosen from the bits of x: with x = m 2^e, m in [0.5, 1), the candidates are 2^(e-1) and 2^e and the upper one
// is nearer iff m > 0.75.  0 -> 0, +inf -> +inf, NaN and negative values -> NaN, as the log2 form gives.
__device__ __forceinline__ float nearest_pow2(float x) {
    if (x != x || x < 0.f) return NAN;
    if (x == 0.f || x == INFINITY) return x;
    int e;
    const float m = frexpf(x, &e);
    return ldexpf(1.f, m > 0.75f ? e : e - 1);
}

// One tracker update followed (scale != nullptr) by one scale update; lane 0 of one wave does the two dozen flops.
__global__ __launch_bounds__(64) void qat_range_update_kernel(const float* __restrict__ minmax, float* __restrict__ min_val, float* __restrict__ max_val,
                                                              float* __restrict__ first, float* __restrict__ scale, float* __restrict__ zero_point,
                                                              int averaged, float mom, float one_minus_mom, int asymmetric, float q_lo, float q_hi) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float mn = minmax[0], mx = minmax[1];
    float lo = *min_val, hi = *max_val;
    if (*first == 0.f) {                                  // :49-52, :71-74
        *first = *first + 1.f;
        lo = lo + mn;
        hi = hi + mx;
    } else if (averaged) {                                // :76-77
        lo = lo * one_minus_mom + mn * mom;
        hi = hi * one_minus_mom + mx * mom;
    } else {
        // :47-55: `temp_minval` is the buffer itself, so `add_(-temp)` leaves zero behind and the minimum is taken against that zero
        const float zl = lo + (-lo), zh = hi + (-hi);
        lo = zl + nan_min(zl, mn);
        hi = zh + nan_max(zh, mx);
    }
    *min_val = lo;
    *max_val = hi;
    if (!scale) return;
    if (!asymmetric) {                                    // :179-196
        const float q_range = fmaxf(fabsf(q_lo), fabsf(q_hi));
        *scale = __fdiv_rn(nearest_pow2(nan_max(fabsf(lo), fabsf(hi))), q_range);
        if (zero_point) *zero_point = 0.f;
    } else {                                              // :203-219
        const float s = __fdiv_rn(nearest_pow2(hi - lo), q_hi - q_lo);
        *scale = s;
        if (zero_point) *zero_point = rintf(q_hi - __fdiv_rn(hi, s));
    }
}

__device__ __forceinline__ float qat_round(float x, float s, float zp) {
    const float u = __fdiv_rn(x, s) + zp;
    return copysignf(floorf(fabsf(u) + 0.5f), u);        // NaN stays NaN; the sign of a zero is not part of the contract
}
// torch.clamp: a NaN passes through
__device__ __forceinline__ float qat_clamp(float r, float lo, float hi) { return r != r ? r : fminf(fmaxf(r, lo), hi); }

__global__ __launch_bounds__(QAT_THREADS) void qat_fake_quant_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long count,
                                                                         const float* __restrict__ scale, const float* __restrict__ zero_point,
                                                                         float lo, float hi, int do_clamp, float* __restrict__ snapshot,
                                                                         float* __restrict__ step) {
    const float s = *scale, zp = zero_point ? *zero_point : 0.f;
    auto element = [&](float v) {
        float r = qat_round(v, s, zp);
        if (do_clamp) r = qat_clamp(r, lo, hi);
        return (r - zp) * s;
    };
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 == 0) {
        if (snapshot) { snapshot[0] = s; snapshot[1] = zp; }      // what the backward recomputes the mask with, should the buffers move on
        if (step) *step = *step + 1.f;                             // :152
    }
    if (((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        f32x4* y4 = reinterpret_cast<f32x4*>(y);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = x4[i];
            f32x4 o;
            o[0] = element(v[0]); o[1] = element(v[1]); o[2] = element(v[2]); o[3] = element(v[3]);
            y4[i] = o;
        }
        for (long i = (n4 << 2) + i0; i < count; i += stride) y[i] = element(x[i]);
    } else {
        for (long i = i0; i < count; i += stride) y[i] = element(x[i]);
    }
}

// dx = ((dy s) mask) / s: the chain torch's autograd walks (dequantize, clamp, round, quantize: :114-136) - for a power-of-two s that is
// dy under the mask.  mask = lo <= r <= hi, false for a NaN.
__global__ __launch_bounds__(QAT_THREADS) void qat_fake_quant_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                                         long count, const float* __restrict__ snapshot, float lo, float hi) {
    const float s = snapshot[0], zp = snapshot[1];
    auto element = [&](float v, float g) {
        const float r = qat_round(v, s, zp);
        return __fdiv_rn((r >= lo && r <= hi) ? g * s : 0.f, s);
    };
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)dx)) & 15u) == 0) {
        const long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(dy);
        f32x4* o4 = reinterpret_cast<f32x4*>(dx);
        for (long i = i0; i < n4; i += stride) {
            const f32x4 v = x4[i], g = g4[i];
            f32x4 o;
            o[0] = element(v[0], g[0]); o[1] = element(v[1], g[1]); o[2] = element(v[2], g[2]); o[3] = element(v[3], g[3]);
            o4[i] = o;
        }
        for (long i = (n4 << 2) + i0; i < count; i += stride) dx[i] = element(x[i], dy[i]);
    } else {
        for (long i = i0; i < count; i += stride) dx[i] = element(x[i], dy[i]);
    }
}

static bool misaligned4(const void* p) { return (((uintptr_t)p) & 3u) != 0; }

}  // namespace yh

using namespace yh;

extern "C" int64_t yh_qat_observe_workspace(int64_t count) {
    if (count <= 0) return 0;
    return (int64_t)qat_blocks(count) * 3 * (int64_t)sizeof(float);
}

extern "C" int yh_qat_observe(const float* t, int64_t count, void* ws, int64_t ws_bytes, float* minmax, void* stream) {
    if (!t || !ws || !minmax || count <= 0) return YH_EINVAL;
    if (misaligned4(t) || misaligned4(ws) || misaligned4(minmax)) return YH_EALIGN;
    const int blocks = qat_blocks(count);
    if (ws_bytes < (int64_t)blocks * 3 * (int64_t)sizeof(float)) return YH_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(qat_observe_partial_kernel, dim3(blocks), dim3(QAT_THREADS), 0, s, t, (long)count, (float*)ws);
    hipLaunchKernelGGL(qat_observe_final_kernel, dim3(1), dim3(64), 0, s, (const float*)ws, blocks, minmax);
    return check_launch();
}

extern "C" int yh_qat_range_update(const float* minmax, float* min_val, float* max_val, float* first, float* scale, float* zero_point,
                                   int tracker, double momentum, int asymmetric, int is_signed, int bits, void* stream) {
    if (!minmax || !min_val || !max_val || !first || bits < 2 || bits > 24) return YH_EINVAL;
    if (tracker != YH_QAT_TRACK_GLOBAL && tracker != YH_QAT_TRACK_AVERAGED) return YH_EINVAL;
    if (misaligned4(minmax) || misaligned4(min_val) || misaligned4(max_val) || misaligned4(first) || misaligned4(scale) ||
        misaligned4(zero_point))
        return YH_EALIGN;
    const float q_lo = is_signed ? -(float)(1 << (bits - 1)) : 0.f;
    const float q_hi = is_signed ? (float)((1 << (bits - 1)) - 1) : (float)((1 << bits) - 1);
    // the tracker multiplies by the Python floats `1 - momentum` and `momentum`, each rounded to fp32 where it meets the tensor
    hipLaunchKernelGGL(qat_range_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, minmax, min_val, max_val, first, scale, zero_point,
                       tracker == YH_QAT_TRACK_AVERAGED ? 1 : 0, (float)momentum, (float)(1.0 - momentum), asymmetric ? 1 : 0, q_lo, q_hi);
    return check_launch();
}

extern "C" int yh_qat_fake_quant_fwd(const float* x, float* y, int64_t count, const float* scale, const float* zero_point, float lo, float hi,
                                     int do_clamp, float* snapshot, float* step, void* stream) {
    if (!x || !y || !scale || count <= 0 || (do_clamp && !(lo < hi))) return YH_EINVAL;
    if (misaligned4(x) || misaligned4(y) || misaligned4(scale) || misaligned4(zero_point) || misaligned4(snapshot) || misaligned4(step))
        return YH_EALIGN;
    hipLaunchKernelGGL(qat_fake_quant_fwd_kernel, dim3(qat_blocks(count)), dim3(QAT_THREADS), 0, (hipStream_t)stream, x, y, (long)count, scale,
                       zero_point, lo, hi, do_clamp ? 1 : 0, snapshot, step);
    return check_launch();
}

extern "C" int yh_qat_fake_quant_bwd(const float* x, const float* dy, float* dx, int64_t count, const float* snapshot, float lo, float hi,
                                     void* stream) {
    if (!x || !dy || !dx || !snapshot || count <= 0 || !(lo < hi)) return YH_EINVAL;
    if (misaligned4(x) || misaligned4(dy) || misaligned4(dx) || misaligned4(snapshot)) return YH_EALIGN;
    hipLaunchKernelGGL(qat_fake_quant_bwd_kernel, dim3(qat_blocks(count)), dim3(QAT_THREADS), 0, (hipStream_t)stream, x, dy, dx, (long)count,
                       snapshot, lo, hi);
    return check_launch();
}
