// COCO bbox scoring (yh_coco_match, yh_coco_accumulate; include/yolo_hip.h): the per-image, per-category, per-area-range loops of the
// protocol stated in utils/cocoeval.py as two launches.
//
// yh_coco_match: one workgroup per (image, category) pair, its four waves are the four area ranges.  The serial part is the walk over
// the pair's (at most 100) detections; inside a step the ground truths lie across the 64 lanes, in passes of 64 when there are more.
// The IoU of the detection with a lane's ground truth is computed once and tested against the ten thresholds; per threshold a lane
// keeps its best candidate as (key, index) with key = the bits of the IoU (positive doubles order like their bits) with bit 62 set
// for a ground truth that is not ignored (an IoU is <= 1 < 2, so bit 62 of its own bits is clear): one unsigned maximum then states
// "not ignored first, then the largest IoU", and a second one over the index picks the latest ground truth among equals - the
// serial loop's `later equal IoU replaces the earlier one`.  The ten matched bits of a ground truth live in the workspace, read and
// written only by the lane that owns it.
//
// yh_coco_accumulate: one workgroup per (category, area range, maxDets, threshold); see the header for the two passes.  tp and fp are
// integers, so the order of the prefix sums does not matter; pr is never stored.
//
// Arithmetic: fp64, every value a single operation in the order of utils/cocoeval.py, built without contraction, IEEE divide.
#include "common.h"

namespace yh {

constexpr int CM_THREADS = 256;       // four waves: the four area ranges of one pair
constexpr int CA_THREADS = 256;       // = the chunk of the accumulation's scans
constexpr int CE_T = 10, CE_R = 101;
constexpr unsigned long long CE_NOT_IGNORED = 1ull << 62;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int m = 32; m; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
    for (int m = 32; m; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(CM_THREADS) void coco_match_kernel(const yh_coco_match_desc d) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, a = threadIdx.x >> 6;
    const int* const pr = d.pairs + 4L * blockIdx.x;
    const int d0 = pr[0], D = pr[1], g0 = pr[2], G = pr[3];
    if (d0 < 0 || D < 0 || g0 < 0 || G < 0 || (long)d0 + D > d.n_dets || (long)g0 + G > d.n_gts) return;     // uniform
    const double lo = d.area_rng[2 * a], hi = d.area_rng[2 * a + 1];
    uint16_t* const matched = reinterpret_cast<uint16_t*>(d.ws) + (long)a * d.n_gts + g0;
    uint8_t* const gig = d.gt_ignore + (long)a * d.n_gts + g0;
    const double* const gts = d.gts + 6L * g0;
    for (int g = lane; g < G; g += 64) {
        const double area = gts[6L * g + 4];
        gig[g] = (gts[6L * g + 5] != 0.0 || area < lo || area > hi) ? 1 : 0;
        matched[g] = 0;
    }
    double thr[CE_T];
#pragma unroll
    for (int t = 0; t < CE_T; ++t) {
        const double v = d.iou_thrs[t];
        thr[t] = v < 1 - 1e-10 ? v : 1 - 1e-10;
    }
    uint16_t* const dtm = d.dt_matched + (long)a * d.n_dets + d0;
    uint16_t* const dti = d.dt_ignore + (long)a * d.n_dets + d0;

    for (int di = 0; di < D; ++di) {
        const double* const r = d.dets + 4L * (d0 + di);
        const double dx = r[0], dy = r[1], dw = r[2], dh = r[3];
        const double dx2 = dx + dw, dy2 = dy + dh, da = dw * dh;
        unsigned long long key[CE_T];
        int idx[CE_T];
#pragma unroll
        for (int t = 0; t < CE_T; ++t) {
            key[t] = 0;
            idx[t] = -1;
        }
        for (int g = lane; g < G; g += 64) {
            const double* const q = gts + 6L * g;
            const double gx = q[0], gy = q[1], gw = q[2], gh = q[3], area = q[4];
            const bool crowd = q[5] != 0.0;
            const bool ig = crowd || area < lo || area > hi;
            const double w = fmin(dx2, gx + gw) - fmax(dx, gx);
            const double h = fmin(dy2, gy + gh) - fmax(dy, gy);
            double iou = 0.0;
            if (w > 0.0 && h > 0.0) {
                const double i = w * h;
                const double u = crowd ? da : (da + gw * gh) - i;
                iou = i / u;
            }
            const unsigned m = matched[g];
            const unsigned long long k = (unsigned long long)__double_as_longlong(iou) | (ig ? 0ull : CE_NOT_IGNORED);
#pragma unroll
            for (int t = 0; t < CE_T; ++t) {
                const bool eligible = crowd || !((m >> t) & 1u);
                if (eligible && iou >= thr[t] && k >= key[t]) {      // >=: a later ground truth replaces an equal earlier one
                    key[t] = k;
                    idx[t] = g;
                }
            }
        }
        unsigned dm = 0, dg = 0;
#pragma unroll
        for (int t = 0; t < CE_T; ++t) {
            if (__ballot(idx[t] >= 0) == 0ull) continue;              // uniform: nobody has a candidate at this threshold
            const unsigned long long best = wave_max_u64(idx[t] >= 0 ? key[t] : 0ull);
            const int win = wave_max_i32((idx[t] >= 0 && key[t] == best) ? idx[t] : -1);
            dm |= 1u << t;
            if (!(best & CE_NOT_IGNORED)) dg |= 1u << t;
            if ((win & 63) == lane) matched[win] = (uint16_t)(matched[win] | (1u << t));     // lane owns g = lane + 64 j
        }
        if (da < lo || da > hi) dg |= ~dm & 0x3ffu;
        if (lane == 0) {
            dtm[di] = (uint16_t)dm;
            dti[di] = (uint16_t)dg;
        }
    }
}

// first index j in [0, CE_R) with rec[j] > v (CE_R when there is none)
__device__ __forceinline__ int upper_bound_rec(const double* rec, double v) {
    int lo = 0, hi = CE_R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(CA_THREADS) void coco_accum_kernel(const yh_coco_accum_desc d) {
#pragma clang fp contract(off)
    __shared__ double rec[CE_R];
    __shared__ int s_sum[4];
    __shared__ int s_scan[4];
    __shared__ double s_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x, a = blockIdx.y, mi = blockIdx.z / CE_T, t = blockIdx.z % CE_T;
    const int maxdet = mi == 0 ? 1 : (mi == 1 ? 10 : 100);
    const int K = d.K;
    const long stride = (long)K * 12;                                            // precision: between two recall thresholds
    double* const P = d.precision + ((long)t * CE_R * K + k) * 12 + a * 3 + mi;
    double* const Rc = d.recall + ((long)t * K + k) * 12 + a * 3 + mi;
    if (tid < CE_R) rec[tid] = d.rec_thrs[tid];

    // packed (tp, fp) counts: a thread or a chunk holds at most 2^15 of either between two unpackings
    auto block_sum = [&](int v) -> int {
        for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m, 64);
        __syncthreads();                       // the previous use of s_sum has been read
        if (lane == 0) s_sum[wave] = v;
        __syncthreads();
        return s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    };

    // npig: the category's ground truths that are not ignored in this range
    const int gb = d.gt_first[k], ge = d.gt_first[k + 1];
    int cnt = 0;
    if (gb >= 0 && ge <= d.n_gts)
        for (int j = gb + tid; j < ge; j += CA_THREADS) {
            const int g = d.cat_gts[j];
            if (g >= 0 && g < d.n_gts) cnt += d.gt_ignore[(long)a * d.n_gts + g] == 0;
        }
    const int npig = block_sum(cnt);
    if (npig == 0) {                            // uniform
        if (tid < CE_R) P[tid * stride] = -1.0;
        if (tid == 0) *Rc = -1.0;
        return;
    }
    const int b = d.cat_first[k];
    int n = d.cat_first[k + 1] - b;
    if (b < 0 || n < 0 || (long)b + n > d.n_dets) n = 0;
    const uint16_t* const dtm = d.dt_matched + (long)a * d.n_dets;
    const uint16_t* const dti = d.dt_ignore + (long)a * d.n_dets;
    // 1 = true positive, 0x10000 = false positive, 0 = ignored, or past maxDets in its pair
    auto flags = [&](int i) -> int {
        const int s = d.cat_dets[b + i];
        if (s < 0 || s >= d.n_dets || d.det_rank[s] >= maxdet) return 0;
        if ((dti[s] >> t) & 1) return 0;
        return ((dtm[s] >> t) & 1) ? 1 : 0x10000;
    };

    // pass 1: the totals.  A thread visits n / 256 elements: unpack every 2^15 of them
    long ttp = 0, tfp = 0;
    {
        int acc = 0, since = 0;
        long ltp = 0, lfp = 0;
        for (int i = tid; i < n; i += CA_THREADS) {
            acc += flags(i);
            if (++since == 32767) {
                ltp += acc & 0xffff;
                lfp += acc >> 16;
                acc = since = 0;
            }
        }
        ltp += acc & 0xffff;
        lfp += acc >> 16;
        // n < 2^31 detections: the two block sums run on plain ints
        ttp = block_sum((int)ltp);
        tfp = block_sum((int)lfp);
    }
    const double dn = (double)npig;
    const double eps = 2.220446049250313e-16;   // 2^-52

    // pass 2: backwards in chunks of the workgroup
    long after_tp = 0, after_fp = 0;
    double carry = 0.0;                          // the running maximum of pr over everything behind the chunk (pr >= 0)
    for (int c = (n + CA_THREADS - 1) / CA_THREADS - 1; c >= 0; --c) {
        const int i = c * CA_THREADS + tid;
        const bool in = i < n;
        const int f = in ? flags(i) : 0;
        int inc = f;                             // inclusive prefix sum of the packed flags over the chunk
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_scan[wave] = inc;
        __syncthreads();
        int chunk = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) inc += s_scan[w];
            chunk += s_scan[w];
        }
        const long ctp = chunk & 0xffff, cfp = chunk >> 16;
        const long tp = ttp - after_tp - ctp + (inc & 0xffff);
        const long fp = tfp - after_fp - cfp + (inc >> 16);
        const double dtp = (double)tp;
        const double prv = in ? dtp / (((double)fp + dtp) + eps) : 0.0;
        double sm = prv;                         // the maximum from here to the end of the chunk
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_down(sm, o, 64);
            if (lane + o < 64) sm = fmax(sm, u);
        }
        if (lane == 0) s_max[wave] = sm;
        __syncthreads();
        double all = carry;
        for (int w = 0; w < 4; ++w) {
            if (w > wave) sm = fmax(sm, s_max[w]);
            all = fmax(all, s_max[w]);
        }
        sm = fmax(sm, carry);
        if (in && (i == 0 || (f & 1))) {         // the first element that reaches the recall thresholds in (rc of i - 1, rc of i]
            const int jlo = i == 0 ? 0 : upper_bound_rec(rec, (double)(tp - 1) / dn);
            const int jhi = upper_bound_rec(rec, dtp / dn);
            for (int j = jlo; j < jhi; ++j) P[j * stride] = sm;
        }
        carry = all;
        after_tp += ctp;
        after_fp += cfp;
    }
    const double last = (double)ttp / dn;
    if (tid < CE_R && (n == 0 || rec[tid] > last)) P[tid * stride] = 0.0;
    if (tid == 0) *Rc = last;
}

}  // namespace yh

extern "C" int64_t yh_coco_workspace(int64_t n_dets, int64_t n_gts) {
    if (n_dets < 0 || n_gts < 0) return YH_EINVAL;
    return 8 * n_gts;                            // four area ranges x one uint16 of matched bits per ground truth
}

extern "C" int yh_coco_match(const yh_coco_match_desc* d, void* stream) {
    if (!d) return YH_EINVAL;
    if (d->n_pairs < 0 || d->n_dets < 0 || d->n_gts < 0) return YH_EINVAL;
    if (d->n_pairs == 0) return YH_OK;           // nothing to match: nothing is launched
    if (!d->pairs || !d->iou_thrs || !d->area_rng) return YH_EINVAL;
    if (d->n_dets > 0 && (!d->dets || !d->dt_matched || !d->dt_ignore)) return YH_EINVAL;
    if (d->n_gts > 0 && (!d->gts || !d->gt_ignore || !d->ws)) return YH_EINVAL;
    if (d->ws_bytes < 8LL * d->n_gts) return YH_EINVAL;
    if ((((uintptr_t)d->dets) | ((uintptr_t)d->gts) | ((uintptr_t)d->iou_thrs) | ((uintptr_t)d->area_rng)) & 7u) return YH_EALIGN;
    if (((uintptr_t)d->pairs) & 3u) return YH_EALIGN;
    if ((((uintptr_t)d->dt_matched) | ((uintptr_t)d->dt_ignore) | ((uintptr_t)d->ws)) & 1u) return YH_EALIGN;
    hipLaunchKernelGGL(yh::coco_match_kernel, dim3(d->n_pairs), dim3(yh::CM_THREADS), 0, (hipStream_t)stream, *d);
    return yh::check_launch();
}

extern "C" int yh_coco_accumulate(const yh_coco_accum_desc* d, void* stream) {
    if (!d) return YH_EINVAL;
    if (d->n_dets < 0 || d->n_gts < 0 || d->K < 1 || d->K > 65535) return YH_EINVAL;
    if (!d->cat_first || !d->gt_first || !d->rec_thrs || !d->precision || !d->recall) return YH_EINVAL;
    if (d->n_dets > 0 && (!d->cat_dets || !d->det_rank || !d->dt_matched || !d->dt_ignore)) return YH_EINVAL;
    if (d->n_gts > 0 && (!d->cat_gts || !d->gt_ignore)) return YH_EINVAL;
    if ((((uintptr_t)d->rec_thrs) | ((uintptr_t)d->precision) | ((uintptr_t)d->recall)) & 7u) return YH_EALIGN;
    if ((((uintptr_t)d->cat_dets) | ((uintptr_t)d->cat_first) | ((uintptr_t)d->cat_gts) | ((uintptr_t)d->gt_first)) & 3u) return YH_EALIGN;
    if ((((uintptr_t)d->dt_matched) | ((uintptr_t)d->dt_ignore)) & 1u) return YH_EALIGN;
    hipLaunchKernelGGL(yh::coco_accum_kernel, dim3(d->K, 4, 3 * yh::CE_T), dim3(yh::CA_THREADS), 0, (hipStream_t)stream, *d);
    return yh::check_launch();
}
