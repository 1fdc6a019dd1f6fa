// Bilinear resize of an fp32 NCHW batch on the device: the per-step rescale of multi-scale training (reference train.py:368-374,
// F.interpolate(mode='bilinear', align_corners=False) with a given output size).  Formula and rounding: include/yolo_hip.h
// yh_resize_bilinear.  One wave per 64-pixel segment of one output row: the row taps are wave-uniform, the two source rows are
// read through the cache (neighbouring lanes share taps, neighbouring output rows share source rows), stores are coalesced.
// Compiled with -ffp-contract=off (csrc/Makefile): every product and sum below is rounded to fp32 once.
#include "common.h"

namespace yh {

__device__ __forceinline__ void resize_taps(int d, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    s = s > 2.0e9f ? 2.0e9f : s;     // only a scale no (in, out) pair gives gets here: keeps the conversion below defined
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int segs,
                                                              int ih, int iw, int oh, int ow, float scale_h, float scale_w) {
#pragma clang fp contract(off)
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);     // (plane * oh + y) * segs + segment
    if (wave >= rows * segs) return;
    const long row = wave / segs;
    const int seg = (int)(wave - row * segs);
    const long plane = row / oh;
    const int y = (int)(row - plane * oh);
    const int x = seg * 64 + (threadIdx.x & 63);
    if (x >= ow) return;
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    resize_taps(y, scale_h, ih, y0, y1, hy0, hy1);
    resize_taps(x, scale_w, iw, x0, x1, wx0, wx1);
    const float* p0 = src + (plane * ih + y0) * (long)iw;
    const float* p1 = src + (plane * ih + y1) * (long)iw;
    const float a = p0[x0], b = p0[x1], c = p1[x0], e = p1[x1];
    const float top = wx0 * a + wx1 * b;
    const float bot = wx0 * c + wx1 * e;
    dst[row * ow + x] = hy0 * top + hy1 * bot;
}

}  // namespace yh

extern "C" int yh_resize_bilinear(const yh_resize_desc* d, void* stream) {
    using namespace yh;
    if (!d || !d->src || !d->dst) return YH_EINVAL;
    if (d->n <= 0 || d->c <= 0 || d->ih <= 0 || d->iw <= 0 || d->oh <= 0 || d->ow <= 0) return YH_EINVAL;
    if (!(d->scale_h > 0.f) || !(d->scale_w > 0.f) || !(d->scale_h <= 16777216.f) || !(d->scale_w <= 16777216.f)) return YH_EINVAL;
    const long rows = (long)d->n * d->c * d->oh;
    const int segs = (d->ow + 63) / 64;
    const long blocks = (rows * segs + 3) / 4;
    if (blocks > 0x7fffffffL) return YH_EUNSUPPORTED;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d->src, d->dst, rows, segs, d->ih,
                       d->iw, d->oh, d->ow, d->scale_h, d->scale_w);
    return check_launch();
}
