// Network-slimming sparsity term of a training step: grad += s * sign(gamma) for the BatchNorm gammas under the L1 penalty - the
// per-layer Python loop of the reference (train.py:443-448 -> BNOptimizer.updateBN, utils/prune_utils.py:130-138: sign, mul and add_
// per layer, ~200 launches on YOLOv3) as ONE multi-tensor launch over a device table of rows.
#include "common.h"

namespace yh {

// torch.sign on floats: (0 < x) - (x < 0), so +0, -0 and NaN give 0
__device__ __forceinline__ float sign_f32(float x) { return (float)((0.f < x) - (x < 0.f)); }

// One workgroup per row (rows are BatchNorm widths: 1 .. 1024 floats, far below what a second grid dimension would pay for).  The
// start of a row is 16-byte aligned, its length is arbitrary: whole float4 groups first, then the last n % 4 elements one by one, so
// nothing past element n is read or written (a row that is NOT aligned - parameters living in somebody's flat buffer - takes the
// element loop from its start).  The product s * sign is formed on its own and then added (no contraction; with a
// factor of -1 / 0 / +1 it is exact either way), which makes the result the bits of grad.add_(s * torch.sign(gamma)).
__global__ __launch_bounds__(256) void bn_l1_subgrad_kernel(const yh_bn_l1_row* __restrict__ rows, const int first, const float s) {
#pragma clang fp contract(off)
    const yh_bn_l1_row row = rows[first + blockIdx.x];
    const float* __restrict__ const gamma = row.gamma;
    float* __restrict__ const grad = row.grad;
    const int n = row.n;
    const int n4 = ((((uintptr_t)gamma | (uintptr_t)grad) & 15u) == 0) ? n >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[i];
        f32x4 d = reinterpret_cast<f32x4*>(grad)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = s * sign_f32(g[e]);
            d[e] = d[e] + t;
        }
        reinterpret_cast<f32x4*>(grad)[i] = d;
    }
    for (int i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
        const float t = s * sign_f32(gamma[i]);
        grad[i] = grad[i] + t;
    }
}

}  // namespace yh

extern "C" int yh_bn_l1_subgrad(const yh_bn_l1_row* rows, int first, int last, float s, void* stream) {
    if (first < 0 || last < first) return YH_EINVAL;
    if (last == first) return YH_OK;          // empty range: nothing to launch
    if (!rows) return YH_EINVAL;
    if (((uintptr_t)rows) & 7u) return YH_EALIGN;      // the rows themselves are device memory: their pointers are the caller's promise
    hipLaunchKernelGGL(yh::bn_l1_subgrad_kernel, dim3(last - first), dim3(256), 0, (hipStream_t)stream, rows, first, s);
    return yh::check_launch();
}
