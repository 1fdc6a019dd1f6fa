// compute_loss of the reference (utils/utils.py:368-432) and its hand-derived gradient, fused: a handful of launches per
// head instead of ~200 small torch kernels and several full-size zero-filled temporaries in autograd.
#include <cmath>

#include "common.h"

namespace yh {

struct Dual4 {  // value + partial derivatives w.r.t. the four raw box logits
    float v, d[4];
};
__device__ __forceinline__ Dual4 mk(float v) { return Dual4{v, {0.f, 0.f, 0.f, 0.f}}; }
__device__ __forceinline__ Dual4 operator+(const Dual4& a, const Dual4& b) {
    return Dual4{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2], a.d[3] + b.d[3]}};
}
__device__ __forceinline__ Dual4 operator-(const Dual4& a, const Dual4& b) {
    return Dual4{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2], a.d[3] - b.d[3]}};
}
__device__ __forceinline__ Dual4 operator*(const Dual4& a, const Dual4& b) {
    Dual4 r;
    r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
__device__ __forceinline__ Dual4 operator/(const Dual4& a, const Dual4& b) {
    Dual4 r;
    const float inv = 1.f / b.v;
    r.v = a.v * inv;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
    return r;
}
__device__ __forceinline__ Dual4 dmin(const Dual4& a, const Dual4& b) { return a.v <= b.v ? a : b; }
__device__ __forceinline__ Dual4 dmax(const Dual4& a, const Dual4& b) { return a.v >= b.v ? a : b; }
__device__ __forceinline__ Dual4 clamp0(const Dual4& a) { return a.v > 0.f ? a : mk(0.f); }

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
// BCEWithLogits with pos_weight: -(pw t log s + (1 - t) log(1 - s)), stable form
__device__ __forceinline__ float bce(float x, float t, float pw) {
    const float sp = fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));   // softplus(-x) = -log sigmoid(x)
    return (1.f - t) * x + (1.f + (pw - 1.f) * t) * sp;
}
__device__ __forceinline__ float bce_grad(float x, float t, float pw) {
    const float s = sigmoidf(x);
    return s * (1.f - t + pw * t) - pw * t;
}

// One BCE element of the class / objectness terms, optionally under FocalLoss (utils/utils.py FocalLoss, the alpha-balanced TF-addons
// form the reference wraps around both BCEs when hyp['fl_gamma'] > 0):  L = B * a * q^gamma,  q = 1 - p_t = t + s * (1 - 2 t),
// a = t * alpha + (1 - t) * (1 - alpha).  FOCAL == false is the plain BCE, the code of the default loss.  Where q <= 0 (s rounded to
// t in fp32) value and derivative are 0, the limit: B vanishes like q.  A NaN logit fails `q <= 0` and propagates, as in the BCE.
template <bool FOCAL>
__device__ __forceinline__ float loss_elem(float x, float t, float pw, float gamma, float alpha) {
    const float B = bce(x, t, pw);
    if constexpr (!FOCAL) return B;
    const float q = t + sigmoidf(x) * (1.f - 2.f * t);
    const float a = t * alpha + (1.f - t) * (1.f - alpha);
    return q <= 0.f ? 0.f : B * a * powf(q, gamma);
}
// dL/dx = a * (bce_grad * M + B * gamma * q^(gamma - 1) * (1 - 2 t) * s * (1 - s)),  M = q^gamma.  One pow: q^(gamma - 1) = M / q, taken
// as (B / q) * M - B / q stays O(1) (B ~ q where q is small), M / q alone overflows for gamma < 1 at the smallest q.
template <bool FOCAL>
__device__ __forceinline__ float loss_elem_grad(float x, float t, float pw, float gamma, float alpha) {
    if constexpr (!FOCAL) return bce_grad(x, t, pw);
    const float s = sigmoidf(x), u = 1.f - 2.f * t;
    const float q = t + s * u;
    if (q <= 0.f) return 0.f;
    const float a = t * alpha + (1.f - t) * (1.f - alpha);
    const float M = powf(q, gamma);
    return a * (bce_grad(x, t, pw) * M + (bce(x, t, pw) / q) * M * gamma * u * s * (1.f - s));
}

// d atan(u) = du / (1 + u^2)
__device__ __forceinline__ Dual4 datan(const Dual4& a) {
    Dual4 r;
    const float inv = 1.f / (1.f + a.v * a.v);
    r.v = atanf(a.v);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] * inv;
    return r;
}

// The box measure of the predicted box (from 4 raw logits, xywh) against the target (xywh): bbox_iou(x1y1x2y2=False, ...) with
// GIoU=True (BOX == YH_BOX_GIOU, the default loss), DIoU=True or CIoU=True, in the statement's operation order:
//   c2 = cw^2 + ch^2 + 1e-16,  rho2 = ((bx1 + bx2) - (ax1 + ax2))^2 / 4 + (the same in y),  DIoU = iou - rho2 / c2
//   v = (4 / pi^2) (atan(w2 / h2) - atan(w1 / h1))^2,  alpha = v / (1 - iou + v),  CIoU = iou - (rho2 / c2 + v * alpha)
// alpha is a constant for the derivative (the statement's torch.no_grad()).  Where 1 - iou + v <= 0 - the prediction equals its label
// exactly: iou == 1 and v == 0 in fp32 - alpha is 0, the limit of v * alpha; the statement divides 0 by 0 there and returns NaN for
// value and gradient.  A NaN logit fails `<= 0` and propagates.
// SXY (darknet's scale_x_y, the yh_yolo_loss_head_* entries): pxy = sigmoid * s - c, c = 0.5 (s - 1), d pxy / dt = s * (sg * (1 - sg));
// everything downstream is the same chain.  SXY = false is the code above without s and c: the instantiations behind the older entries.
template <int BOX, bool SXY>
__device__ __forceinline__ Dual4 box_measure_of(const float* ps4, const float* an, const float* tb, float s, float c) {
    Dual4 px = mk(sigmoidf(ps4[0])), py = mk(sigmoidf(ps4[1]));
    px.d[0] = px.v * (1.f - px.v);
    py.d[1] = py.v * (1.f - py.v);
    if constexpr (SXY) {
        px.v = px.v * s - c; px.d[0] = s * px.d[0];
        py.v = py.v * s - c; py.d[1] = s * py.d[1];
    }
    const float ew = expf(ps4[2]), eh = expf(ps4[3]);
    Dual4 pw = mk(fminf(ew, 1e3f) * an[0]), ph = mk(fminf(eh, 1e3f) * an[1]);
    pw.d[2] = ew < 1e3f ? pw.v : 0.f;                    // clamp(max=1e3) cuts the gradient
    ph.d[3] = eh < 1e3f ? ph.v : 0.f;
    const Dual4 half = mk(0.5f);
    const Dual4 ax1 = px - pw * half, ax2 = px + pw * half, ay1 = py - ph * half, ay2 = py + ph * half;
    const Dual4 bx1 = mk(tb[0] - tb[2] / 2), bx2 = mk(tb[0] + tb[2] / 2), by1 = mk(tb[1] - tb[3] / 2), by2 = mk(tb[1] + tb[3] / 2);
    const Dual4 inter = clamp0(dmin(ax2, bx2) - dmax(ax1, bx1)) * clamp0(dmin(ay2, by2) - dmax(ay1, by1));
    const Dual4 w1 = ax2 - ax1, h1 = ay2 - ay1, w2 = bx2 - bx1, h2 = by2 - by1;
    const Dual4 uni = (w1 * h1 + mk(1e-16f)) + w2 * h2 - inter;
    const Dual4 iou = inter / uni;
    const Dual4 cw = dmax(ax2, bx2) - dmin(ax1, bx1), ch = dmax(ay2, by2) - dmin(ay1, by1);
    if constexpr (BOX == YH_BOX_GIOU) {
        const Dual4 hull = cw * ch + mk(1e-16f);
        return iou - (hull - uni) / hull;
    } else {
        const Dual4 c2 = (cw * cw + ch * ch) + mk(1e-16f);
        const Dual4 dx = (bx1 + bx2) - (ax1 + ax2), dy = (by1 + by2) - (ay1 + ay2);
        const Dual4 rho2 = (dx * dx) * mk(0.25f) + (dy * dy) * mk(0.25f);
        if constexpr (BOX == YH_BOX_DIOU) {
            return iou - rho2 / c2;
        } else {
            const Dual4 da = mk(atanf(w2.v / h2.v)) - datan(w1 / h1);
            const Dual4 v = mk(0.40528473456935116f) * (da * da);                   // 4 / pi^2
            const float den = (1.f - iou.v) + v.v;
            const Dual4 alpha = mk(den <= 0.f ? 0.f : v.v / den);
            return iou - (rho2 / c2 + v * alpha);
        }
    }
}

__device__ __forceinline__ void block_sum_atomic(float v, float* dst) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dst, red[0] + red[1] + red[2] + red[3]);
    __syncthreads();
}

// build_targets (utils/utils.py:725-779) for one candidate k = a * nt + t, in the reference's fp32 arithmetic
struct Match {
    int b, a, gy, gx, cls;
    long cell;
    float tb[4], an[2];
};
// 0: matched, -1: wh_iou <= iou_t, > 0: label error mask (class / image / cell out of range)
__device__ __forceinline__ int assign(const yh_loss_desc& d, int k, Match& m) {
    m.a = k / d.nt;
    const float* tg = d.targets + 6L * (k - m.a * d.nt);
    const float gx = tg[2] * (float)d.nx, gy = tg[3] * (float)d.ny, gw = tg[4] * (float)d.nx, gh = tg[5] * (float)d.ny;
    m.an[0] = d.anchors[2 * m.a];
    m.an[1] = d.anchors[2 * m.a + 1];
    const float inter = fminf(m.an[0], gw) * fminf(m.an[1], gh);      // wh_iou (utils.py:325-331)
    if (!(inter / (m.an[0] * m.an[1] + gw * gh - inter) > d.iou_t)) return -1;
    m.b = (int)tg[0];
    m.cls = (int)tg[1];
    m.gx = (int)gx;
    m.gy = (int)gy;
    int err = 0;
    if (m.cls < 0 || m.cls >= d.nc) err |= 1;
    if (m.b < 0 || m.b >= d.bs || m.gx < 0 || m.gx >= d.nx || m.gy < 0 || m.gy >= d.ny) err |= 2;
    if (err) return err;
    m.tb[0] = gx - floorf(gx);
    m.tb[1] = gy - floorf(gy);
    m.tb[2] = gw;
    m.tb[3] = gh;
    m.cell = (((long)m.b * d.na + m.a) * d.ny + m.gy) * d.nx + m.gx;
    return 0;
}

// count the matched candidates; several may share a cell: remember the last one per cell
__global__ __launch_bounds__(256) void loss_assign_kernel(const yh_loss_desc d) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    Match m;
    const int r = k < d.na * d.nt ? assign(d, k, m) : -1;
    if (r == 0) atomicMax(d.winner + m.cell, k);
    if (r > 0) atomicOr(d.count + 1, r);
    const unsigned long long hit = __ballot(r == 0);
    if ((threadIdx.x & 63) == 0 && hit) atomicAdd(d.count, __popcll(hit));
}

// matched candidates, forward: box and class sums, objectness targets.  One thread per (candidate, class) - the class loop of a
// candidate used to run inside one thread (80 dependent global loads + BCEs: 33 - 83 us for 1536 threads, latency bound); the thread
// of class 0 also takes the box term.  nc == 1: one thread per candidate, no class term (as the reference, utils.py:412).
// BOX selects the box measure (box_measure_of); it is the statement's one variable, so the objectness target takes it too.
template <bool FOCAL, int BOX, bool SXY>
__global__ __launch_bounds__(256) void loss_matched_fwd_kernel(const yh_loss_desc d, const float gamma, const float alpha, const float sxy,
                                                               const float sxy_c) {
    const int ncl = d.nc > 1 ? d.nc : 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx / ncl, c = idx - k * ncl;
    float lbox = 0.f, lcls = 0.f;
    Match m;
    if (k < d.na * d.nt && assign(d, k, m) == 0) {
        const float* ps = d.p + m.b * d.sb + m.a * d.sa + m.gy * d.sy + m.gx * d.sx;
        if (c == 0) {
            const float box[4] = {ps[0], ps[1], ps[2], ps[3]};
            const Dual4 g = box_measure_of<BOX, SXY>(box, m.an, m.tb, sxy, sxy_c);
            lbox = 1.f - g.v;
            if (d.winner[m.cell] == k) d.tobj[m.cell] = (1.f - d.gr) + d.gr * fmaxf(g.v, 0.f);
        }
        if (d.nc > 1) lcls = loss_elem<FOCAL>(ps[5 + c], c == m.cls ? d.cp : d.cn, d.cls_pw, gamma, alpha);
    }
    block_sum_atomic(lbox, d.sums + 0);
    if (d.nc > 1) block_sum_atomic(lcls, d.sums + 2);
}

// every cell, forward: objectness BCE against tobj (32-bit cell decode: the launcher keeps the cell count below 2^31)
template <bool FOCAL>
__global__ __launch_bounds__(256) void loss_obj_fwd_kernel(const yh_loss_desc d, const float gamma, const float alpha) {
    const unsigned cells = (unsigned)d.bs * d.na * d.ny * d.nx;
    float acc = 0.f;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x) {
        const unsigned x = i % (unsigned)d.nx;
        unsigned r = i / (unsigned)d.nx;
        const unsigned y = r % (unsigned)d.ny;
        r /= (unsigned)d.ny;
        const unsigned a = r % (unsigned)d.na, b = r / (unsigned)d.na;
        acc += loss_elem<FOCAL>(d.p[(long)b * d.sb + (long)a * d.sa + (long)y * d.sy + (long)x * d.sx + 4], d.tobj[i], d.obj_pw, gamma, alpha);
    }
    block_sum_atomic(acc, d.sums + 1);
}

// every cell, backward: the whole gradient row of the cell (zeros, objectness term in slot 4).  One workgroup row = the na * no
// values of one grid position (contiguous in the NHWC head tensors: consecutive threads store consecutive floats), the position
// decoded once per row with 32-bit arithmetic.  (The first form decoded every ELEMENT with five 64-bit divisions: 0.41 ms for the
// 76 x 76 head of YOLOv3-608 batch 64 - 1 TB/s - against 0.1 ms of bytes.)
template <bool FOCAL>
__global__ __launch_bounds__(256) void loss_dense_bwd_kernel(const yh_loss_desc d, const float gamma, const float alpha) {
    const int row = d.na * d.no;                              // any width: a thread takes elements j, j + 256, .. of the row
    const int pixels = d.bs * d.ny * d.nx, hw = d.ny * d.nx;
    const float sc = *d.scale * d.g_obj / (float)((long)d.bs * d.na * d.ny * d.nx);
    if constexpr (FOCAL) {
        // The focal derivative is a few hundred instructions (exp, log1p, pow, divisions) and only the na objectness slots of a row
        // need it: inside the row loop below a whole wave executes them for ONE live lane, and the kernel is bound by that issue
        // (0.87 ms against the plain kernel's 0.35 ms on the three heads of YOLOv3-608 batch 64).  So the workgroup first evaluates
        // the slots of up to 256 / na of its pixels with one lane each and parks them in LDS; the row loop then only stores.
        const int per = 256 / d.na;                           // pixels per pass; na > 256: 0, the loop below serves such a head
        if (per > 0) {
            __shared__ float gobj[256];
            const int kk = threadIdx.x / d.na, ka = threadIdx.x - kk * d.na;
            for (long p0 = blockIdx.x; p0 < pixels; p0 += (long)per * gridDim.x) {      // workgroup-uniform trip count
                const long ps = p0 + (long)kk * gridDim.x;                 // the pixel whose slot ka this lane stages
                if (kk < per && ps < pixels) {
                    const int b = (int)ps / hw, r = (int)ps - b * hw;     // ps < pixels < 2^31: 32-bit decode
                    const int y = r / d.nx, x = r - y * d.nx;
                    const long cell = (((long)b * d.na + ka) * d.ny + y) * d.nx + x;
                    gobj[threadIdx.x] = sc * loss_elem_grad<true>(d.p[(long)b * d.sb + (long)ka * d.sa + (long)y * d.sy + (long)x * d.sx + 4],
                                                                  d.tobj[cell], d.obj_pw, gamma, alpha);
                }
                __syncthreads();
                for (int j = threadIdx.x; j < row; j += 256) {
                    const int a = j / d.no, o = j - a * d.no;
                    for (int k = 0; k < per; ++k) {
                        const long p = p0 + (long)k * gridDim.x;
                        if (p >= pixels) break;
                        const int b = (int)p / hw, r = (int)p - b * hw;
                        const int y = r / d.nx, x = r - y * d.nx;
                        d.grad[(long)b * d.gb + (long)a * d.ga + (long)y * d.gy + (long)x * d.gx + o] = o == 4 ? gobj[k * d.na + a] : 0.f;
                    }
                }
                __syncthreads();
            }
            return;
        }
    }
    for (int j = threadIdx.x; j < row; j += 256) {            // one trip for na * no <= 256 (COCO: 255), more for nc > 80
        const int a = j / d.no, o = j - a * d.no;
        for (int p = blockIdx.x; p < pixels; p += gridDim.x) {
            const int b = p / hw, r = p - b * hw;
            const int y = r / d.nx, x = r - y * d.nx;
            float g = 0.f;
            if (o == 4) {
                const long cell = (((long)b * d.na + a) * d.ny + y) * d.nx + x;
                g = sc * loss_elem_grad<FOCAL>(d.p[(long)b * d.sb + (long)a * d.sa + (long)y * d.sy + (long)x * d.sx + 4], d.tobj[cell], d.obj_pw, gamma,
                                               alpha);
            }
            d.grad[(long)b * d.gb + (long)a * d.ga + (long)y * d.gy + (long)x * d.gx + o] = g;
        }
    }
}

// matched candidates, backward: box and class terms added on top of the dense pass (duplicates of a cell accumulate); one thread per
// (candidate, class) as in the forward
template <bool FOCAL, int BOX, bool SXY>
__global__ __launch_bounds__(256) void loss_matched_bwd_kernel(const yh_loss_desc d, const float gamma, const float alpha, const float sxy,
                                                               const float sxy_c) {
    const int ncl = d.nc > 1 ? d.nc : 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx / ncl, c = idx - k * ncl;
    Match m;
    if (k >= d.na * d.nt || assign(d, k, m) != 0) return;
    const float* ps = d.p + m.b * d.sb + m.a * d.sa + m.gy * d.sy + m.gx * d.sx;
    float* gp = d.grad + m.b * d.gb + m.a * d.ga + m.gy * d.gy + m.gx * d.gx;
    const int nb = d.count[0] > 1 ? d.count[0] : 1;
    if (c == 0) {
        const float w_box = *d.scale * d.g_box / (float)nb;
        const float box[4] = {ps[0], ps[1], ps[2], ps[3]};
        const Dual4 g = box_measure_of<BOX, SXY>(box, m.an, m.tb, sxy, sxy_c);
#pragma unroll
        for (int i = 0; i < 4; ++i) atomicAdd(gp + i, -w_box * g.d[i]);
    }
    if (d.nc > 1) {
        const float w_cls = *d.scale * d.g_cls / (float)((long)nb * d.nc);
        atomicAdd(gp + 5 + c, w_cls * loss_elem_grad<FOCAL>(ps[5 + c], c == m.cls ? d.cp : d.cn, d.cls_pw, gamma, alpha));
    }
}

static int check_loss(const yh_loss_desc* d, bool bwd) {
    if (!d || !d->p || !d->tobj || d->bs <= 0 || d->na <= 0 || d->ny <= 0 || d->nx <= 0 || d->no < 5 || d->nc != d->no - 5) return YH_EINVAL;
    if (d->nt < 0 || !d->count || (d->nt > 0 && (!d->targets || !d->anchors || (!bwd && !d->winner)))) return YH_EINVAL;
    if (bwd ? (!d->grad || !d->scale) : !d->sums) return YH_EINVAL;
    return YH_OK;
}

static inline unsigned grid_n(long total) {
    long g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// FocalLoss parameters of the yh_yolo_loss_focal_* entries: gamma finite and > 0, alpha finite and in [0, 1]
static int check_focal(float gamma, float alpha) {
    if (!std::isfinite(gamma) || !(gamma > 0.f) || !std::isfinite(alpha) || alpha < 0.f || alpha > 1.f) return YH_EINVAL;
    return YH_OK;
}

template <bool FOCAL, int BOX, bool SXY = false>
static int loss_fwd(const yh_loss_desc* d, float gamma, float alpha, hipStream_t s, float sxy = 1.f) {
    if (d->nt > 0) {
        const unsigned blocks = (unsigned)(((long)d->na * d->nt + 255) / 256);
        const unsigned cblocks = (unsigned)(((long)d->na * d->nt * (d->nc > 1 ? d->nc : 1) + 255) / 256);
        hipLaunchKernelGGL(loss_assign_kernel, dim3(blocks), dim3(256), 0, s, *d);
        hipLaunchKernelGGL((loss_matched_fwd_kernel<FOCAL, BOX, SXY>), dim3(cblocks), dim3(256), 0, s, *d, gamma, alpha, sxy, 0.5f * (sxy - 1.f));
    }
    if ((long)d->bs * d->na * d->ny * d->nx >= 0x7fffffffL) return YH_EUNSUPPORTED;
    hipLaunchKernelGGL((loss_obj_fwd_kernel<FOCAL>), dim3(grid_n((long)d->bs * d->na * d->ny * d->nx)), dim3(256), 0, s, *d, gamma, alpha);
    return check_launch();
}

template <bool FOCAL, int BOX, bool SXY = false>
static int loss_bwd(const yh_loss_desc* d, float gamma, float alpha, hipStream_t s, float sxy = 1.f) {
    if ((long)d->bs * d->ny * d->nx >= 0x7fffffffL) return YH_EUNSUPPORTED;
    const long pixels = (long)d->bs * d->ny * d->nx;
    hipLaunchKernelGGL((loss_dense_bwd_kernel<FOCAL>), dim3((unsigned)(pixels < 16384 ? pixels : 16384)), dim3(256), 0, s, *d, gamma, alpha);
    if (d->nt > 0)
        hipLaunchKernelGGL((loss_matched_bwd_kernel<FOCAL, BOX, SXY>), dim3((unsigned)(((long)d->na * d->nt * (d->nc > 1 ? d->nc : 1) + 255) / 256)),
                           dim3(256), 0, s, *d, gamma, alpha, sxy, 0.5f * (sxy - 1.f));
    return check_launch();
}

// the yh_yolo_loss_box_* entries: box kind 0..2; gamma finite and >= 0 (0: plain BCE, alpha ignored), gamma > 0 under check_focal
static int check_box(int box, float gamma, float alpha) {
    if (box < YH_BOX_GIOU || box > YH_BOX_CIOU || !std::isfinite(gamma) || gamma < 0.f) return YH_EINVAL;
    return gamma > 0.f ? check_focal(gamma, alpha) : YH_OK;
}

template <int BOX, bool SXY>
static int loss_box(const yh_loss_desc* d, bool bwd, float gamma, float alpha, hipStream_t s, float sxy) {
    if (gamma > 0.f) return bwd ? loss_bwd<true, BOX, SXY>(d, gamma, alpha, s, sxy) : loss_fwd<true, BOX, SXY>(d, gamma, alpha, s, sxy);
    return bwd ? loss_bwd<false, BOX, SXY>(d, 0.f, 0.f, s, sxy) : loss_fwd<false, BOX, SXY>(d, 0.f, 0.f, s, sxy);
}

// the yh_yolo_loss_head_* entries add scale_x_y, finite and in [1, 2]; 1 takes the instantiations of the yh_yolo_loss_box_* entries
template <bool SXY>
static int loss_box_kind(const yh_loss_desc* d, bool bwd, int box, float gamma, float alpha, hipStream_t s, float sxy) {
    if (box == YH_BOX_DIOU) return loss_box<YH_BOX_DIOU, SXY>(d, bwd, gamma, alpha, s, sxy);
    if (box == YH_BOX_CIOU) return loss_box<YH_BOX_CIOU, SXY>(d, bwd, gamma, alpha, s, sxy);
    return loss_box<YH_BOX_GIOU, SXY>(d, bwd, gamma, alpha, s, sxy);
}

static int loss_box_entry(const yh_loss_desc* d, bool bwd, int box, float gamma, float alpha, float sxy, void* stream) {
    int rc = check_loss(d, bwd);
    if (!rc) rc = check_box(box, gamma, alpha);
    if (!rc && !yh_scale_xy_ok(sxy)) rc = YH_EINVAL;
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (sxy == 1.f) return loss_box_kind<false>(d, bwd, box, gamma, alpha, s, 1.f);
    return loss_box_kind<true>(d, bwd, box, gamma, alpha, s, sxy);
}

}  // namespace yh

using namespace yh;

extern "C" int yh_yolo_loss_fwd(const yh_loss_desc* d, void* stream) {
    int rc = check_loss(d, false);
    if (rc) return rc;
    return loss_fwd<false, YH_BOX_GIOU>(d, 0.f, 0.f, (hipStream_t)stream);
}

extern "C" int yh_yolo_loss_bwd(const yh_loss_desc* d, void* stream) {
    int rc = check_loss(d, true);
    if (rc) return rc;
    return loss_bwd<false, YH_BOX_GIOU>(d, 0.f, 0.f, (hipStream_t)stream);
}

extern "C" int yh_yolo_loss_focal_fwd(const yh_loss_desc* d, float gamma, float alpha, void* stream) {
    int rc = check_loss(d, false);
    if (!rc) rc = check_focal(gamma, alpha);
    if (rc) return rc;
    return loss_fwd<true, YH_BOX_GIOU>(d, gamma, alpha, (hipStream_t)stream);
}

extern "C" int yh_yolo_loss_focal_bwd(const yh_loss_desc* d, float gamma, float alpha, void* stream) {
    int rc = check_loss(d, true);
    if (!rc) rc = check_focal(gamma, alpha);
    if (rc) return rc;
    return loss_bwd<true, YH_BOX_GIOU>(d, gamma, alpha, (hipStream_t)stream);
}

extern "C" int yh_yolo_loss_box_fwd(const yh_loss_desc* d, int box, float gamma, float alpha, void* stream) {
    return loss_box_entry(d, false, box, gamma, alpha, 1.f, stream);
}

extern "C" int yh_yolo_loss_box_bwd(const yh_loss_desc* d, int box, float gamma, float alpha, void* stream) {
    return loss_box_entry(d, true, box, gamma, alpha, 1.f, stream);
}

extern "C" int yh_yolo_loss_head_fwd(const yh_loss_desc* d, int box, float gamma, float alpha, float scale_x_y, void* stream) {
    return loss_box_entry(d, false, box, gamma, alpha, scale_x_y, stream);
}

extern "C" int yh_yolo_loss_head_bwd(const yh_loss_desc* d, int box, float gamma, float alpha, float scale_x_y, void* stream) {
    return loss_box_entry(d, true, box, gamma, alpha, scale_x_y, stream);
}
