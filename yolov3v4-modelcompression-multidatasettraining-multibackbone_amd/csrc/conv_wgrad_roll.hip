// 3x3 / stride 1 / pad 1 weight gradient, "rolling halo" form (fp16; cout % 128 == 0, cin % 64 == 0, 16 <= W <= 190).
//
//   dw[co][ci][r][s] = sum over output pixels p of dz[p][co] * x[p shifted by tap (r, s)][ci]        (autograd of models.py:92-98)
//
// The im2col kernels (conv_wgrad.hip) fetch a shifted copy of the x rows for every (tap, ci) column tile, nine times per layer.  A first
// halo form (round 3, since deleted: profiles/r03_wgrad_halo.txt) owned a 256 (co) x [9 taps x 32 ci] tile per workgroup and moved 16 KB
// of dz plus 1/8 of a 256-pixel halo image of x per 32-pixel K step: 18 - 19 KB for 4.7 MFLOP, and its compute side alone ran at 1550
// TFLOP/s where the full kernel reached 830 - 970 - the global -> LDS stream, not the matrix pipe, set its step time (DESIGN.md 3, round 3
// item 2).  This kernel has the same accumulator budget (73 728 outputs = 295 KB of registers, one workgroup per CU, 12 waves in three
// rotating groups) and is shaped by what the stream has to deliver:
//   * tile 128 (co) x [9 taps x 64 ci]: the squarest split of 73 728 outputs.  Per 32-pixel step 8 KB of dz + 4 KB of x = 12 KB;
//   * x is not staged per chunk but ROLLS: the virtual pixel space of conv_halo_pp.hip (one shared pad row / column per image:
//     v = n (H+1)(W+1) + (y+1)(W+1) + (x+1), tap (r, s) = row offset (r-1)(W+1) + (s-1)) is walked in order, row v of x lives in
//     slot v mod 512 of a 64 KB ring of 128-byte rows, and every step fetches exactly the 32 rows that enter the window
//     [v - (W+2), v + 31 + (W+2)] - no halo overlap is fetched twice inside a split, no second buffer, no per-split pixel table;
//   * every DMA lane decodes its own row: (image, y, x) advance by 32 positions per step with two compare-selects (32 = q (W+1) + r),
//     a pad position (or one beyond the batch) reads the zero page.  One LDS-DMA instruction per wave per step: waves 0 .. 7 the 4-row
//     pieces of dz (256-byte rows), waves 8 .. 11 the 8-row pieces of x - a uniform stream, every wave's in-order counter sees only
//     its own pieces;
//   * the LDS beside the x ring (no second halo image, no table) goes into the dz ring: up to S = min(10, 16 - JL) stages (JL = x steps
//     the window leads by), S - 1 steps = up to 108 KB in flight per CU.
// Fragment reads are ds_read_b64_tr_b16 on both operands (rows = pixels, transposed on the read side).  dz rows: the unit permutation
// of conv_wgrad_dma_kernel<4, .> (16 units, XOR ((r & 3) | ((r >> 3) & 1) << 2) << 1).  x rows (128 B = half of the 64 banks, any tap
// offset): 32-byte column k of row r is stored at k ^ (((r >> 1) & 1) | ((r >> 3) & 1) << 1) - the 8 row pieces that share an LDS cycle
// (rows e + {0,1,2,3,8,9,10,11}) split into two parities of four rows {e, e+2, e+8, e+10} whose XOR values are always distinct (bit 3
// flips between r and r + 8, bit 1 between r and r + 2, a carry out of bits 1-2 flips both of one pair): conflict-free for every e.
// Partial tiles per pixel split go to the workspace in MFMA-native order, summed by wgrad_roll_reduce_kernel in split order.
// The forms that lost and are no longer built: the K loops with a LOAD segment of their own (one, two or no barrier-enforced read
// intervals per step: profiles/r05_wgrad_roll_segments.txt, r05_wgrad_roll_ab.txt, r05_wgrad_roll_order3_ab.txt), the 32x32x16 MFMA form
// (9 - 13 % slower, profiles/r05_wgrad_roll_mfma32_ab.txt), s_setprio around the MFMAs (1 - 3 % slower) and the scattering reduce
// (r05_wgrad_roll_ab.txt).
#include "common.h"
#include <stdlib.h>

namespace yh {

__device__ __attribute__((aligned(16))) const uint32_t g_zero16r[4] = {0u, 0u, 0u, 0u};  // source of every pad-position 16-byte load

struct RollArgs {
    yh_wgrad_desc d;
    int tiles_m, tiles_n;     // cout / 128, cin / 64
    int steps_total, sps;     // 32-position steps of the virtual pixel space, steps per split
    int S, JL;                // dz ring stages; x stream lead in steps: ceil((2 (W+1) + 2) / 32)
    int q32, r32;             // 32 = q32 (W+1) + r32
    int cin_w;
};

typedef int wr_v2i __attribute__((ext_vector_type(2)));
template <int OFF> __device__ __forceinline__ wr_v2i wr_read_tr16(unsigned lds_byte_addr) {
    wr_v2i r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(OFF));
    return r;
}

__device__ __forceinline__ int wr_swz_dz(int r) { return ((r & 3) | (((r >> 3) & 1) << 2)) << 1; }   // 16-byte units of a 256-byte dz row
__device__ __forceinline__ int wr_swz_x(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 1); }    // 32-byte columns of a 128-byte x row

__device__ __forceinline__ void wr_wait_keep(int keep) {      // counted wait with a wave-uniform run-time count: literal operands only
    switch (keep) {
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

constexpr int WR_XRING = 65536;     // 512 rows x 128 B
constexpr int WR_ABYTES = 8192;     // one dz step: 32 rows x 256 B

__global__ __launch_bounds__(768, 3) void conv_wgrad_roll_kernel(const RollArgs a) {
    constexpr int NT = 768;
    const yh_wgrad_desc& d = a.d;
    extern __shared__ __attribute__((aligned(128))) unsigned char rsm[];   // [x ring 64 KB][S dz stages of 8 KB]: the only LDS object
    typedef const void __attribute__((address_space(1))) * gptr_t;
    typedef void __attribute__((address_space(3))) * lptr_t;

    const int tiles = a.tiles_m * a.tiles_n;
    int tile_id, split_id;
    {   // consecutive (split, tile) ids share an XCD: all tiles of a split read the same dz / x rows through one L2
        const int nb = gridDim.x, bid = blockIdx.x;
        const int q = nb >> 3, rr = nb & 7, xcd = bid & 7;
        const int logical = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
        split_id = logical / tiles;
        tile_id = logical - split_id * tiles;
    }
    const int tm = tile_id % a.tiles_m, tn = tile_id / a.tiles_m;
    const int co0 = tm * 128, ci0 = tn * 64;
    const int s0 = split_id * a.sps;
    const int nsteps = min(a.sps, a.steps_total - s0);
    if (nsteps <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / 6, wn = wave - wm * 6;      // wave tile: channels 64 wm .. +63 x the three taps of filter row wn >> 1 x 32 ci (half wn & 1)
    const int trow = wn >> 1, hh = wn & 1;
    const int S = a.S, D = S - 1, JL = a.JL;
    constexpr int KW = 3;                      // the counted wait of a step covers the piece of KW steps on
    const int Wp = d.w_in + 1, Hp = d.h + 1, IMG = Hp * Wp;
    const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)rsm;

    // the zero page's address as two SCALARS: a pointer select against it costs no vector registers (168-register cap; a spilled
    // pointer would be reloaded by a scratch load, which sits on the LDS-DMA queue's counter)
    const unsigned zlo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)g_zero16r);
    const unsigned zhi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)g_zero16r >> 32));

    // ---- this lane's row of the stream.  dz waves (0 .. 7): instruction = 4 rows x 16 units, row 4 wave + lane / 16 of the step;
    // x waves (8 .. 11): 8 rows x 8 units, row 8 (wave - 8) + lane / 8 of the x step, which starts W + 2 positions before the dz step
    const bool dz_wave = wave < 8;                                      // wave-uniform
    int n, yy, xx, cofs;
    {
        int rowl, p;
        if (dz_wave) {
            rowl = 4 * wave + (lane >> 4);
            cofs = co0 + (((lane & 15) ^ wr_swz_dz(rowl)) << 3);
            p = 32 * s0 + rowl;
        } else {
            rowl = 8 * (wave - 8) + (lane >> 3);
            cofs = ci0 + (((lane & 7) ^ (wr_swz_x(rowl) << 1)) << 3);
            p = 32 * s0 - Wp - 1 + rowl;
        }
        const int pp = p + IMG;                      // p >= -(W + 2) > -IMG
        const int q = pp / IMG;
        const int rem = pp - q * IMG;
        n = q - 1;
        yy = rem / Wp;
        xx = rem - yy * Wp;
    }
    const f16* const srcbase = reinterpret_cast<const f16*>(dz_wave ? d.dz : d.x);
    const unsigned ld = (unsigned)(dz_wave ? d.lddz : d.ldx);
    unsigned slot;                                   // LDS byte offset (from rsm) of this wave's next piece
    int stage_i = 0;                                 // dz: ring stage of the next piece; x: x step of the next piece (mod 16)
    slot = dz_wave ? WR_XRING + wave * 1024 : (wave - 8) * 1024;
    auto issue = [&]() {
        const bool ok = (unsigned)n < (unsigned)d.n && yy >= 1 && xx >= 1;
        const unsigned pix = (unsigned)((n * d.h + yy - 1) * d.w_in + xx - 1);
        const unsigned long long u = (unsigned long long)(uintptr_t)(srcbase + (pix * ld + (unsigned)cofs));
        const unsigned lo = ok ? (unsigned)u : zlo, hi = ok ? (unsigned)(u >> 32) : zhi;
        __builtin_amdgcn_global_load_lds((gptr_t)(uintptr_t)(((unsigned long long)hi << 32) | lo), (lptr_t)(rsm + slot), 16, 0, 0);
        // the next step's row: 32 positions on
        xx += a.r32;
        yy += a.q32;
        const bool cx = xx >= Wp;
        xx = cx ? xx - Wp : xx;
        yy = cx ? yy + 1 : yy;
        const bool cy = yy >= Hp;
        yy = cy ? yy - Hp : yy;
        n = cy ? n + 1 : n;
        ++stage_i;
        if (dz_wave) {
            const bool w = stage_i == S;
            stage_i = w ? 0 : stage_i;
            slot = w ? WR_XRING + wave * 1024 : slot + WR_ABYTES;
        } else {
            slot = (slot + 4096) & (WR_XRING - 1);
        }
    };

    f32x4 acc[4][6];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- fragment addressing (ds_read_b64_tr_b16: lane (q, g) supplies 4 consecutive channels of pixel row 8g + 4h + q/4 and
    // receives 4 consecutive pixels of channel q of the 16-channel block)
    const int q = lane & 15, g = lane >> 4;
    unsigned a_addr0;                  // dz fragment 0, half 0, inside a stage; fragment i: ^ (i << 5); half 1: + 4 rows = offset 1024
    unsigned b_abs[3][2];              // x: tap column s, half h; channel block 0 (block 1 = ^ 32); absolute LDS address, rolls 4 KB per step
    {
        const int row = 8 * g + (q >> 2);
        const int cha = wm * 64 + 4 * (q & 3);
        a_addr0 = row * 256 + ((((cha >> 3) ^ wr_swz_dz(row)) << 4) | ((cha & 7) * 2));
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int xr = row + 4 * h + trow * Wp + s;      // slot row at step 0 (slot 0 = position 32 s0 - (W + 2))
                b_abs[s][h] = lds0 + (unsigned)((xr & 511) * 128 + (((2 * hh) ^ wr_swz_x(xr)) << 5) + (q & 3) * 8);
            }
    }
    const unsigned roll_add = 4096u - lds0;       // b = lds0 + ((b - lds0 + 4096) & 0xffff)

    // ---- K loop.  A segment of 8-byte LDS reads is issue-bound per wave (one per ~24 cycles) and its latency is dead time for that wave;
    // spread between the MFMAs it is not (tools/probe/run_lds_probe.py: twelve waves that each do 20 fragment reads THEN 24 MFMAs per
    // trip need 1530 cycles per trip, the same waves with every fragment re-read right after its last MFMA of the trip 1382).  So a wave
    // holds ONE set of fragments and refreshes it in place: x fragment pair j (tap column j) is dead after the four MFMAs of column j and
    // is re-read for step s + 1 at once, dz fragment i after MFMA (i, last column).  A step is C_0 .. C_5 (4 MFMAs + refresh reads each)
    // and ST (this wave's LDS-DMA piece, the counted wait).  One barrier per step, at a group-dependent point of the stream (after C_1 /
    // C_3 / C_5 for the wave groups 0-3 / 4-7 / 8-11, one wave per SIMD each) so that the three waves of a SIMD stay a third of a step apart.
    // Hazards (b_s = barrier of step s; interval I_s ends with it): step s + 1's data is read in C(s), i.e. in I_s or I_(s+1), and
    // every such read has RETURNED at the lgkmcnt(0) that opens step s + 1, before b_(s+1); the wait in ST(s') (in I_(s'+1)) covers the
    // piece of step s' + 3, published by b_(s'+1), first read in C_0(s' + 2) in I_(s'+2); the piece of step s' + D (D = S - 1) issued in
    // ST(s') overwrites the stage of step s' - 1, whose reads returned before b_(s'-1).
#define YH_WR_BARRIER()                      \
    do {                                     \
        __builtin_amdgcn_sched_barrier(0);   \
        __builtin_amdgcn_s_barrier();        \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)
    const int n_pro = dz_wave ? min(D, nsteps) : min(JL + D, nsteps + JL);
    for (int k = 0; k < n_pro; ++k) issue();
    wr_wait_keep(max(0, n_pro - (dz_wave ? KW : JL + KW)));       // steps 0 .. KW - 1 (x steps 0 .. JL + KW - 1) have landed
    YH_WR_BARRIER();
    wr_v2i ra[4][2], rb[6][2];
    const int g3 = wave >> 2;
    // fragments of step 0 (landed and published by the prologue), addresses rolled to step 1
    {
        const unsigned stage = lds0 + WR_XRING;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i][0] = wr_read_tr16<0>(stage + (a_addr0 ^ (i << 5)));
            ra[i][1] = wr_read_tr16<1024>(stage + (a_addr0 ^ (i << 5)));
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int sx = 0; sx < 3; ++sx) {
                rb[2 * sx][h] = wr_read_tr16<0>(b_abs[sx][h]);
                rb[2 * sx + 1][h] = wr_read_tr16<0>(b_abs[sx][h] ^ 32);
            }
    }
    int st_read = 1 == S ? 0 : 1;
    for (int s = 0; s < nsteps; ++s) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[1][0]), "+v"(ra[1][1]), "+v"(ra[2][0]), "+v"(ra[2][1]),
                       "+v"(ra[3][0]), "+v"(ra[3][1]), "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[1][0]), "+v"(rb[1][1]),
                       "+v"(rb[2][0]), "+v"(rb[2][1]), "+v"(rb[3][0]), "+v"(rb[3][1]), "+v"(rb[4][0]), "+v"(rb[4][1]),
                       "+v"(rb[5][0]), "+v"(rb[5][1])
                     :
                     : "memory");
        const unsigned stage = lds0 + WR_XRING + st_read * WR_ABYTES;      // dz of step s + 1
        typedef int v4i __attribute__((ext_vector_type(4)));
        f16x8 fa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v4i t = {ra[i][0][0], ra[i][0][1], ra[i][1][0], ra[i][1][1]};
            fa[i] = __builtin_bit_cast(f16x8, t);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sx = 0; sx < 3; ++sx) {
#pragma unroll
            for (int bq = 0; bq < 2; ++bq) {
                const int j = 2 * sx + bq;
                const v4i tb = {rb[j][0][0], rb[j][0][1], rb[j][1][0], rb[j][1][1]};
                const f16x8 fb = __builtin_bit_cast(f16x8, tb);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb, acc[i][j], 0, 0, 0);
                    if (j == 5) {           // dz fragment i is dead: refresh it from the stage of step s + 1
                        __builtin_amdgcn_sched_barrier(0);
                        ra[i][0] = wr_read_tr16<0>(stage + (a_addr0 ^ (i << 5)));
                        ra[i][1] = wr_read_tr16<1024>(stage + (a_addr0 ^ (i << 5)));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                // x fragment j is dead: refresh it (step s + 1's rows; block bq of tap column sx; the pair's addresses roll
                // here, between the MFMAs, not in a block of their own)
                if (bq == 0) {
                    b_abs[sx][0] = lds0 + ((b_abs[sx][0] + roll_add) & (WR_XRING - 1));
                    b_abs[sx][1] = lds0 + ((b_abs[sx][1] + roll_add) & (WR_XRING - 1));
                }
                rb[j][0] = wr_read_tr16<0>(b_abs[sx][0] ^ (32 * bq));
                rb[j][1] = wr_read_tr16<0>(b_abs[sx][1] ^ (32 * bq));
                __builtin_amdgcn_sched_barrier(0);
                if (bq == 1 && g3 == sx) YH_WR_BARRIER();       // this group's one barrier of the step: after C_1 / C_3 / C_5
                // this wave's LDS-DMA piece of step s + D, behind column 2 (after group 0's barrier point, so that every
                // group issues it after ITS barrier of the step ... no: groups 1, 2 issue it before theirs - the stage it
                // overwrites was last read two steps ago either way, see the hazard note above)
                if (j == 2 && s + D < nsteps) issue();
            }
        }
        st_read = st_read + 1 == S ? 0 : st_read + 1;
        // ---- this wave's piece of step s + 3 must have landed (its piece of step s + D was issued behind column 2)
        wr_wait_keep(min(D - 3, max(0, nsteps - 4 - s)));
    }
#undef YH_WR_BARRIER

    f32x4* part = reinterpret_cast<f32x4*>(d.ws) + ((long)split_id * tiles + tile_id) * (24 * NT);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) part[(i * 6 + j) * NT + tid] = acc[i][j];
}

// Partial tiles -> dw.  Writing them out lane by lane scatters: a lane's four values are four output channels of one (ci, tap), 36 bytes
// from its neighbour's - 1.2 M four-byte read-modify-writes (or atomics) per 76 x 76 layer; a first reduce of that form measured 41 us per
// launch for 75 MB (1.9 TB/s), a sixth of the whole weight gradient.  Here one workgroup owns a [16 co][16 ci][9 taps] block of dw:
// wave t (of 9) sums the fragment that holds tap t of the block over the splits (eight independent 16-byte loads in flight per lane,
// fixed order), the block is transposed through LDS and leaves as 16 rows of 576 contiguous bytes.  Workgroups = tiles x 32 x G; G > 1
// (few tiles: the 76 x 76 and 152 x 152 layers) splits the pixel splits over G workgroups that meet in row-contiguous atomics.
template <bool VEC>
__global__ __launch_bounds__(576) void wgrad_roll_reduce_kernel(const RollArgs a, int splits, int per_group, int sstep, int native) {
    constexpr int NT = 768;
    const yh_wgrad_desc& d = a.d;
    __shared__ __attribute__((aligned(16))) float blk[16][148];
    const int tiles = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    const int b = bid & 1, hh = (bid >> 1) & 1, i = (bid >> 2) & 3, wm = (bid >> 4) & 1, tile = bid >> 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int tap = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int trow = tap / 3, tcol = tap - trow * 3;
    const int w_src = wm * 6 + trow * 2 + hh;
    const int ij = i * 6 + tcol * 2 + b;      // partial tiles: fragment (i, 2 tcol + b), lane = (co quad, ci)
    f32x4* part = reinterpret_cast<f32x4*>(d.ws) + ((long)tile * 24 + ij) * NT + w_src * 64 + lane;
    const long stride = (long)tiles * 24 * NT * sstep;      // sstep > 1: the second pass, over the groups' in-place sums
    const int sA = blockIdx.y * per_group, sB = min(sA + per_group, splits);
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    int sp = sA;
    for (; sp + 7 < sB; sp += 8) {
        f32x4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = part[(sp + k) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += t[k];
    }
    for (int k = 0; sp < sB; ++sp, ++k) v[k & 7] += part[sp * stride];
    const f32x4 sum = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    if (native) {      // deterministic form (common.h), first pass: the group's sum replaces its first partial tile - every thread reads and
        part[sA * stride] = sum;      // writes its own element only - and a second launch with ONE group adds the groups in order
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) blk[4 * (lane >> 4) + r][(lane & 15) * 9 + tap] = sum[r];
    __syncthreads();
    const int row = tid / 36, c4 = tid - row * 36;
    const int tm = tile % a.tiles_m, tn = tile / a.tiles_m;
    const int co = tm * 128 + wm * 64 + i * 16 + row, ci0 = tn * 64 + hh * 32 + b * 16;
    float* dst = d.dw + ((long)co * a.cin_w + ci0) * 9 + c4 * 4;
    const f32x4 o = *reinterpret_cast<const f32x4*>(&blk[row][c4 * 4]);
    if (gridDim.y == 1) {       // this workgroup owns the rows: plain accumulate (dw is accumulated into; the caller zeroes it)
        if constexpr (VEC) {
            f32x4 cur = *reinterpret_cast<f32x4*>(dst);
            cur += o;
            *reinterpret_cast<f32x4*>(dst) = cur;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] += o[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dst + e, o[e]);
    }
}

// geometry of the rolling form; false when the layer does not qualify (host code, no launch)
bool wgrad_roll_geometry(const yh_wgrad_desc* d, RollArgs* pa, int* psplits, size_t* plds) {
    RollArgs& a = *pa;
    if (d->dtype != YH_F16 || d->splits == -1) return false;
    if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1 || d->ho != d->h || d->wo != d->w_in) return false;
    if (d->cout % 128 || d->cin % 64 || d->w_in < 16 || d->h < 2) return false;
    if (d->cin_w > 0 && d->cin_w != d->cin) return false;
    const int Wp = d->w_in + 1;
    const int JL = (2 * Wp + 2 + 31) / 32;
    // dz ring stages.  The x ring bounds them at 16 - JL, the LDS at 10; measured (profiles/r05_wgrad_roll_ab.txt): 6 stages = four
    // steps (48 KB) in flight are the fastest on every layer of YOLOv3-608 - 8 and 10 lose 1 - 5 %: a CU is served ~11 B / clk of LDS-DMA
    // however deep its queue is (tools/probe/run_probe.py), more pieces in flight only lengthen the in-order queue each wave waits on
    const int s_max = 16 - JL < 10 ? 16 - JL : 10;
    const int S = s_max < 8 ? s_max : 8;
    if (S < 4) return false;
    const long Q = (long)d->n * (d->h + 1) * Wp;
    if (Q + 4096 >= 0x7fffffffL) return false;
    a.d = *d;
    a.cin_w = d->cin;
    a.tiles_m = d->cout / 128;
    a.tiles_n = d->cin / 64;
    a.steps_total = (int)((Q + 31) / 32);
    a.S = S;
    a.JL = JL;
    a.q32 = 32 / Wp;
    a.r32 = 32 - a.q32 * Wp;
    const int tiles = a.tiles_m * a.tiles_n;
    // Every layer that qualifies takes this form: it beat the round-3 halo kernel on all four stage shapes of YOLOv3-608 batch 64 - 76^2
    // 0.201 / 0.241 ms, 38^2 0.198 / 0.216, 19^2 0.211 / 0.241, 152^2 0.221 / 0.316 (profiles/r05_wgrad_roll_order3_ab.txt).
    // Split groups of the reduce launch: summed in place and added by a one-group launch (deterministic, common.h), or - YH_DETERMINISTIC=0 -
    // meeting in fp32 atomics on the few-tile layers.
    int splits = d->splits > 0 ? d->splits : 256 / tiles;          // one workgroup per CU
    {
        const char* e = getenv("YH_WGRAD_HALO_WGS");       // A/B and test knob: total workgroups aimed for
        if (e && d->splits <= 0) splits = atoi(e) / tiles;
        else if (d->splits <= 0 && splits > a.steps_total / 8) splits = a.steps_total / 8;      // library's choice: >= 8 steps per workgroup
    }
    if (splits < 1) splits = 1;
    if (splits > a.steps_total) splits = a.steps_total;
    a.sps = (a.steps_total + splits - 1) / splits;
    *psplits = (a.steps_total + a.sps - 1) / a.sps;
    *plds = (size_t)WR_XRING + (size_t)S * WR_ABYTES;
    return true;
}

int64_t wgrad_roll_workspace(const yh_wgrad_desc* d) {
    RollArgs a;
    int splits;
    size_t lds;
    if (!wgrad_roll_geometry(d, &a, &splits, &lds)) return 0;
    return (int64_t)splits * a.tiles_m * a.tiles_n * 128 * 576;
}

// YH_EUNSUPPORTED: the layer does not qualify or the workspace is too small (the caller falls back to the other forms)
int launch_wgrad_roll(const yh_wgrad_desc* d, hipStream_t st) {
    RollArgs a;
    int splits;
    size_t lds;
    if (!wgrad_roll_geometry(d, &a, &splits, &lds)) return YH_EUNSUPPORTED;
    const int tiles = a.tiles_m * a.tiles_n;
    if (!d->ws || d->ws_floats < (int64_t)splits * tiles * 128 * 576) return YH_EUNSUPPORTED;
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_wgrad_roll_kernel), lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(conv_wgrad_roll_kernel, dim3((unsigned)(tiles * splits)), dim3(768), lds, st, a);
    int groups = (256 + tiles * 32 - 1) / (tiles * 32);       // >= one workgroup per CU where the splits allow it
    if (groups > splits / 4) groups = splits / 4;
    if (groups < 1) groups = 1;
    const int per_group = (splits + groups - 1) / groups;
    groups = (splits + per_group - 1) / per_group;
    auto reduce = [&](int ngroups, int nsplits, int per, int sstep, int native) {
        const dim3 rg(tiles * 32, ngroups);
        if (aligned16(d->dw)) hipLaunchKernelGGL(wgrad_roll_reduce_kernel<true>, rg, dim3(576), 0, st, a, nsplits, per, sstep, native);
        else hipLaunchKernelGGL(wgrad_roll_reduce_kernel<false>, rg, dim3(576), 0, st, a, nsplits, per, sstep, native);
    };
    if (deterministic() && groups > 1) {      // few-tile layers (76 x 76, 152 x 152): the split groups no longer meet in fp32 atomics
        reduce(groups, splits, per_group, 1, 1);
        reduce(1, groups, groups, per_group, 0);
    } else {
        reduce(groups, splits, per_group, 1, 0);
    }
    return check_launch();
}

}  // namespace yh
