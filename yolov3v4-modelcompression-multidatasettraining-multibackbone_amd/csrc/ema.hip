// Model EMA of a training step: ema = ema * d + (1 - d) * src over every floating-point tensor of the state_dict - the per-tensor
// Python loop of ModelEMA.update (utils/torch_utils.py: mul_ and add_ per tensor, 732 launches on YOLOv3, ema read twice) as ONE
// multi-tensor launch over a device table of rows.
#include "common.h"

namespace yh {

constexpr int EMA_THREADS = 256;
constexpr int EMA_GRID_CAP = 2048;      // 256 CUs x 8 workgroups: beyond that the workgroups stride over the chunks
constexpr int EMA_VEC_PASSES = YH_EMA_CHUNK / (4 * EMA_THREADS);      // float4 groups a thread moves in a full aligned chunk
static_assert(YH_EMA_CHUNK % (4 * EMA_THREADS) == 0, "a full chunk is a whole number of float4 passes");

// Table pointers come out of memory as generic addresses; the tensors are device memory, and saying so gives global_* instead of flat_*
// loads and stores (a flat access also counts against the LDS queue).
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// The bits of `v.mul_(d).add_(src, alpha=a)`: the product with d rounded to fp32 on its own, then ONE fused multiply-add.
__device__ __forceinline__ float ema_elem(float e, float s, float d, float a) { return __fmaf_rn(a, s, __fmul_rn(e, d)); }

// A workgroup serves chunks blockIdx.x, blockIdx.x + gridDim.x, ...; chunk c belongs to the last row whose chunk0 <= c (binary search,
// workgroup-uniform: the probes are scalar loads that hit the L2).  A chunk starts a multiple of 16 KiB into its row, so it is 16-byte
// aligned exactly when the row is: then whole float4 groups (a full chunk: four per thread, all loads issued before the first store),
// and the last cnt % 4 elements one by one; a row that is not aligned on both sides takes the element loop for the whole chunk.
// Neither side is touched past element n.
__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const yh_ema_row* __restrict__ rows, const int n_rows,
                                                                 const int64_t n_chunks, const float d, const float a) {
#pragma clang fp contract(off)
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        int lo = 0, hi = n_rows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rows[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
        }
        const yh_ema_row row = rows[lo];
        const int64_t off = (c - row.chunk0) * YH_EMA_CHUNK;
        if (off < 0 || off >= row.n) continue;          // a chunk index the table does not cover: touch nothing
        const int cnt = (int)(row.n - off < YH_EMA_CHUNK ? row.n - off : YH_EMA_CHUNK);
        gf32* __restrict__ const ema = (gf32*)(row.ema + off);
        const gf32* __restrict__ const src = (const gf32*)(row.src + off);
        const bool aligned = ((((uintptr_t)ema) | ((uintptr_t)src)) & 15u) == 0;
        const int n4 = aligned ? cnt >> 2 : 0;
        if (n4 == YH_EMA_CHUNK / 4) {
            f32x4 e[EMA_VEC_PASSES], s[EMA_VEC_PASSES];
#pragma unroll
            for (int k = 0; k < EMA_VEC_PASSES; ++k) {
                e[k] = reinterpret_cast<const gf32x4*>(ema)[threadIdx.x + k * EMA_THREADS];
                s[k] = reinterpret_cast<const gf32x4*>(src)[threadIdx.x + k * EMA_THREADS];
            }
#pragma unroll
            for (int k = 0; k < EMA_VEC_PASSES; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[k][j] = ema_elem(e[k][j], s[k][j], d, a);
                reinterpret_cast<gf32x4*>(ema)[threadIdx.x + k * EMA_THREADS] = e[k];
            }
            continue;
        }
        for (int i = threadIdx.x; i < n4; i += EMA_THREADS) {
            f32x4 e = reinterpret_cast<const gf32x4*>(ema)[i];
            const f32x4 s = reinterpret_cast<const gf32x4*>(src)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ema_elem(e[j], s[j], d, a);
            reinterpret_cast<gf32x4*>(ema)[i] = e;
        }
        for (int i = 4 * n4 + threadIdx.x; i < cnt; i += EMA_THREADS) ema[i] = ema_elem(ema[i], src[i], d, a);
    }
}

}  // namespace yh

extern "C" int yh_ema_update(const yh_ema_row* rows, int n_rows, int64_t n_chunks, float d, float one_minus_d, void* stream) {
    if (n_rows < 0 || n_chunks < 0) return YH_EINVAL;
    if (n_rows == 0) return YH_OK;            // an empty table: nothing to launch
    if (!rows || n_chunks < n_rows) return YH_EINVAL;
    if (((uintptr_t)rows) & 7u) return YH_EALIGN;      // the rows themselves are device memory: their pointers are the caller's promise
    const int64_t grid = n_chunks < yh::EMA_GRID_CAP ? n_chunks : yh::EMA_GRID_CAP;
    hipLaunchKernelGGL(yh::ema_update_kernel, dim3((unsigned)grid), dim3(yh::EMA_THREADS), 0, (hipStream_t)stream, rows, n_rows, n_chunks,
                       d, one_minus_d);
    return yh::check_launch();
}
