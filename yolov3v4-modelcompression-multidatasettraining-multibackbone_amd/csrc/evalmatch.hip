// Evaluation statistics of a batch: which detections are true positives (yh_eval_match, include/yolo_hip.h) - the per-image loop of the
// mAP protocol (reference test.py:139-185: clip_coords, per label class two nonzero calls and a box_iou, one host read per over-threshold
// detection) as ONE launch.  One workgroup per image; the detections are walked strided over its 256 threads.
//
// Capacity: up to YH_EVAL_MATCH_LDS_LABELS labels of an image are staged in LDS (pixel box, area, class) together with their claim slots.
// An image with more labels takes the chunked form of the same code: the labels pass through the staging area chunk by chunk, every
// detection carries its running best (label, IoU) from chunk to chunk in the workspace, and the claim slots live in the workspace
// too.  Slower (the detections are re-read per chunk, the claims are global atomics), same result; no batch goes back to the host loop.
//
// Arithmetic: every value is a single fp32 operation in the order of utils/utils.py (xywh2xyxy, clip_coords, box_iou) - built without
// contraction, IEEE divide - so the flags are the host loop's bit for bit.  The only atomic is an integer minimum.
#include "common.h"

namespace yh {

constexpr int EM_THREADS = 256;
constexpr int EM_CAP = YH_EVAL_MATCH_LDS_LABELS;
constexpr int EM_FREE = 0x7fffffff;       // a claim slot nobody has claimed

// torch.clamp_(lo, hi) on one value: a NaN stays a NaN (fminf / fmaxf would drop it), +-inf goes to the bound
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(EM_THREADS) void eval_match_kernel(const yh_eval_match_desc d) {
#pragma clang fp contract(off)
    __shared__ float lab[EM_CAP][6];      // x1, y1, x2, y2, area, class
    __shared__ int claim_lds[EM_CAP];
    __shared__ float thr[10];

    const yh_eval_match_row row = d.rows[blockIdx.x];
    const int n = row.n, nl = row.nl;
    float* const pred = row.pred;
    if (!pred || n <= 0) return;          // uniform: the whole workgroup leaves
    const int tid = threadIdx.x;
    const long out0 = row.out_off;
    int* const best_t = reinterpret_cast<int*>(d.ws) + out0;                 // [total] label of the largest IoU (-1: none of its class)
    float* const best_iou = reinterpret_cast<float*>(d.ws) + d.total + out0;  // [total]
    const bool chunked = nl > EM_CAP;
    int* const claim_ws = reinterpret_cast<int*>(d.ws) + 2L * d.total + row.lab_first;   // [nt] claim slots of the chunked form
    const float W = d.width, H = d.height;
    const int niou = d.niou;

    if (tid < niou) thr[tid] = d.iouv[tid];
    if (chunked)
        for (int j = tid; j < nl; j += EM_THREADS) __hip_atomic_store(&claim_ws[j], EM_FREE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int nchunks = nl > 0 ? (nl + EM_CAP - 1) / EM_CAP : 1;

    for (int c = 0; c < nchunks; ++c) {
        const int l0 = c * EM_CAP;
        const int cnt = min(nl - l0, EM_CAP);
        if (c) __syncthreads();           // the previous chunk's scans are done with the staging area
        for (int j = tid; j < cnt; j += EM_THREADS) {
            const float* const t = d.targets + 6L * d.label_index[row.lab_first + l0 + j];
            const float x = t[2], y = t[3], hw = t[4] / 2.f, hh = t[5] / 2.f;
            const float x1 = (x - hw) * W, y1 = (y - hh) * H, x2 = (x + hw) * W, y2 = (y + hh) * H;
            lab[j][0] = x1;
            lab[j][1] = y1;
            lab[j][2] = x2;
            lab[j][3] = y2;
            lab[j][4] = (x2 - x1) * (y2 - y1);
            lab[j][5] = t[1];
            if (!chunked) claim_lds[j] = EM_FREE;
        }
        __syncthreads();                  // staging (and thr, and the chunked form's claim slots in global memory) visible
        const bool last = c == nchunks - 1;
        const float thr0 = thr[0];
        for (int p = tid; p < n; p += EM_THREADS) {
            float* const r = pred + 6L * p;
            float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            const float cls = r[5];
            int bt = -1;
            float bi = 0.f;
            bool nan = false;
            if (c == 0) {
                x1 = clamp_keep_nan(x1, 0.f, W);
                y1 = clamp_keep_nan(y1, 0.f, H);
                x2 = clamp_keep_nan(x2, 0.f, W);
                y2 = clamp_keep_nan(y2, 0.f, H);
                r[0] = x1;
                r[1] = y1;
                r[2] = x2;
                r[3] = y2;
                d.conf_cls[2 * (out0 + p)] = r[4];
                d.conf_cls[2 * (out0 + p) + 1] = cls;
            } else {                      // this thread's own values of the previous chunk (the box was clipped then)
                bt = best_t[p];
                bi = best_iou[p];
                nan = bi != bi;
            }
            const float a1 = (x2 - x1) * (y2 - y1);
            for (int j = 0; j < cnt; ++j) {
                if (lab[j][5] != cls) continue;
                float iw = fminf(x2, lab[j][2]) - fmaxf(x1, lab[j][0]);
                float ih = fminf(y2, lab[j][3]) - fmaxf(y1, lab[j][1]);
                iw = iw < 0.f ? 0.f : iw;
                ih = ih < 0.f ? 0.f : ih;
                const float inter = iw * ih;
                const float iou = inter / ((a1 + lab[j][4]) - inter);
                nan = nan || iou != iou;
                if (bt < 0 || iou > bi) {   // strict: the first maximum stays
                    bt = l0 + j;
                    bi = iou;
                }
            }
            if (nan) bi = __builtin_nanf("");   // torch.max over a row with a NaN is NaN: it claims nothing
            best_t[p] = bt;
            best_iou[p] = bi;
            if (last && bt >= 0 && bi > thr0) {
                if (chunked)
                    atomicMin(&claim_ws[bt], p);
                else
                    atomicMin(&claim_lds[bt], p);     // ds_min_i32
            }
        }
    }
    __syncthreads();                      // every claim is in (LDS, or device-scope atomics of this workgroup)
    for (int p = tid; p < n; p += EM_THREADS) {
        const int bt = best_t[p];
        const float bi = best_iou[p];
        bool win = false;
        if (bt >= 0 && bi > thr[0])
            win = (chunked ? __hip_atomic_load(&claim_ws[bt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : claim_lds[bt]) == p;
        uint8_t* const o = d.correct + (out0 + p) * niou;
        for (int k = 0; k < niou; ++k) o[k] = (win && bi > thr[k]) ? 1 : 0;
    }
}

}  // namespace yh

extern "C" int yh_eval_match(const yh_eval_match_desc* d, void* stream) {
    if (!d) return YH_EINVAL;
    if (d->images < 0 || d->nt < 0 || d->total < 0 || d->niou < 1 || d->niou > 10) return YH_EINVAL;
    if (d->images == 0 || d->total == 0) return YH_OK;      // nothing to match: nothing is launched
    if (!d->rows || !d->iouv || !d->correct || !d->conf_cls || !d->ws) return YH_EINVAL;
    if (d->nt > 0 && (!d->targets || !d->label_index)) return YH_EINVAL;
    if (!(d->width > 0.f) || !(d->height > 0.f)) return YH_EINVAL;
    if (d->ws_bytes < 8LL * d->total + 4LL * d->nt) return YH_EINVAL;
    if (((uintptr_t)d->rows) & 7u) return YH_EALIGN;
    if ((((uintptr_t)d->targets) | ((uintptr_t)d->label_index) | ((uintptr_t)d->iouv) | ((uintptr_t)d->conf_cls) | ((uintptr_t)d->ws)) & 3u)
        return YH_EALIGN;
    hipLaunchKernelGGL(yh::eval_match_kernel, dim3(d->images), dim3(yh::EM_THREADS), 0, (hipStream_t)stream, *d);
    return yh::check_launch();
}
