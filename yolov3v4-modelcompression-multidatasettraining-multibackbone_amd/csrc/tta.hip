// Test-time augmentation (reference models.py:477-506, `--augment`): the frame, a flipped 0.83x copy and a 0.67x copy go through the
// network, the two copies' boxes are mapped back (models.py:493-495) and all rows are concatenated in front of the NMS.
//   yh_tta_view       one view in one launch: flip + bilinear resize + pad to the /64 grid (torch_utils.scale_img, same_shape=False)
//   yh_tta_deaugment  the mapping back, in place on a slice of rows of a decoded (n, rows, no) tensor (the two-pass path)
// The fused path's mapping back sits inside the decode + candidate kernel (csrc/nms.hip, yh_yolo_decode_candidates_tta); both divide
// in correctly rounded fp32, so the two paths share one arithmetic.  Formulas and rounding: include/yolo_hip.h.
// Compiled with -ffp-contract=off (csrc/Makefile): every product and sum below is rounded to fp32 once.
#include "common.h"

namespace yh {

// the taps of csrc/resize.hip (yh_resize_bilinear), operation for operation
__device__ __forceinline__ void tta_taps(int d, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
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

// one wave per 64-pixel segment of one output row (the launch shape of resize_bilinear_kernel): rows below rh and columns right of rw
// are the pad value, inside them the two source rows are read through the cache, mirrored in x when `flip`
__global__ void __launch_bounds__(256) tta_view_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int segs, int ih,
                                                       int iw, int oh, int ow, int rh, int rw, int flip, float scale_h, float scale_w,
                                                       float pad_value) {
#pragma clang fp contract(off)
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);     // (plane * oh + y) * segs + segment
    if (wave >= rows * segs) return;
    const long row = wave / segs;
    const int seg = (int)(wave - row * segs);
    const long plane = row / oh;
    const int y = (int)(row - plane * oh);
    const int x = seg * 64 + (threadIdx.x & 63);
    if (x >= ow) return;
    float v = pad_value;
    if (y < rh && x < rw) {
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        tta_taps(y, scale_h, ih, y0, y1, hy0, hy1);
        tta_taps(x, scale_w, iw, x0, x1, wx0, wx1);
        if (flip) {
            x0 = iw - 1 - x0;
            x1 = iw - 1 - x1;
        }
        const float* p0 = src + (plane * ih + y0) * (long)iw;
        const float* p1 = src + (plane * ih + y1) * (long)iw;
        const float a = p0[x0], b = p0[x1], c = p1[x0], e = p1[x1];
        const float top = wx0 * a + wx1 * b;
        const float bot = wx0 * c + wx1 * e;
        v = hy0 * top + hy1 * bot;
    }
    dst[row * ow + x] = v;
}

// one thread per (image, row) of the slice: cx, cy, w, h /= scale (IEEE division), then cx = flip_w - cx when flip_w >= 0
__global__ void __launch_bounds__(256) tta_deaugment_kernel(float* __restrict__ io, long total, int rows_total, int no, int row0, int nrows,
                                                            float scale, float flip_w) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long img = i / nrows;
    const int r = (int)(i - img * nrows);
    float* p = io + (img * rows_total + row0 + r) * (long)no;
    float cx = p[0] / scale;
    const float cy = p[1] / scale, w = p[2] / scale, h = p[3] / scale;
    if (flip_w >= 0.f) cx = flip_w - cx;
    p[0] = cx; p[1] = cy; p[2] = w; p[3] = h;
}

}  // namespace yh

extern "C" int yh_tta_view(const yh_tta_view_desc* d, void* stream) {
    using namespace yh;
    if (!d || !d->src || !d->dst) return YH_EINVAL;
    if (d->n <= 0 || d->c <= 0 || d->ih <= 0 || d->iw <= 0 || d->oh <= 0 || d->ow <= 0) return YH_EINVAL;
    if (d->rh <= 0 || d->rw <= 0 || d->rh > d->oh || d->rw > d->ow || (d->flip != 0 && d->flip != 1)) return YH_EINVAL;
    if (!(d->scale_h > 0.f) || !(d->scale_w > 0.f) || !(d->scale_h <= 16777216.f) || !(d->scale_w <= 16777216.f)) return YH_EINVAL;
    const long rows = (long)d->n * d->c * d->oh;
    const int segs = (d->ow + 63) / 64;
    const long blocks = (rows * segs + 3) / 4;
    if (blocks > 0x7fffffffL) return YH_EUNSUPPORTED;
    hipLaunchKernelGGL(tta_view_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d->src, d->dst, rows, segs, d->ih, d->iw,
                       d->oh, d->ow, d->rh, d->rw, d->flip, d->scale_h, d->scale_w, d->pad_value);
    return check_launch();
}

extern "C" int yh_tta_deaugment(float* io, int n, int rows_total, int no, int row0, int nrows, float scale, float flip_w, void* stream) {
    using namespace yh;
    if (!io || n <= 0 || rows_total <= 0 || no < 4 || row0 < 0 || nrows <= 0 || (long)row0 + nrows > rows_total) return YH_EINVAL;
    if (!(scale > 0.f)) return YH_EINVAL;
    const long total = (long)n * nrows;
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return YH_EUNSUPPORTED;
    hipLaunchKernelGGL(tta_deaugment_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, io, total, rows_total, no, row0,
                       nrows, scale, flip_w);
    return check_launch();
}
