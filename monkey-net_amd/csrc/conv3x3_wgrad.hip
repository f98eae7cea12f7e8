// Weight gradients of the K x K / stride 1 convolutions on folded NHWC frames (3x3 / pad 1 of the hot path, 4x4 / pad 0 of the
// discriminator) on the gfx950 matrix cores; forward and data gradient: conv3x3.hip.
//
//   weight-gradient GEMM:  dW[co][ci*9+tap] = sum_p dY[p][co] * X[p+off(tap)][ci]   (K = pixels, split over blocks)
//
// Five kernel families (tap-major and its sub-pixel form for up-sampled layers, nine-tap 16x16, LDS-halo, gather), each with
// the launch plan its measurements gave it (TPlan / NPlan / HPlan / WPlan); wgrad_select is the ONE place that says which of
// them a layer runs, single or in a grouped launch.  Splits along the pixels leave deterministic partials (no atomics) that
// a second pass sums in a fixed order: per layer here, or for all layers of a backward pass in one launch
// (mnk_wgrad_reduce_multi).
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "conv_common.h"
#include "pack_tile.h"

using namespace mnk;

namespace {

// ---- weight gradient ----------------------------------------------------------------------------------------
// GEMM  dW[co][n] = sum_p dY[p][co] * X[p + off(tap)][ci]  with n = ci*9 + tap, i.e. exactly the memory order of
// the (Cout, Cin, 1, 3, 3) parameter: a block's result tile is written straight into the gradient (or into a
// split-K partial of the same shape), coalesced along n.  K = pixels, split over blockIdx.z.
struct WgradArgs {
    const float* x;
    int ld_x, C, ups;
    const float* dy;
    int ld_dy, Cout;
    int N, H, W;         // output (dy) geometry
    int Hi, Wi, ntaps, kw, pad;
    long M;              // pixels
    long pix_per_split;  // multiple of 16
    int NT;              // ntaps * C
    float* out;          // unsplit: dw + c_start*9 (row stride ld_out); else partials [splits][Cout][NT]
    long ld_out;
    int splits;
};

template <int BM>
__global__ void __launch_bounds__(256) conv3x3_wgrad_kernel(WgradArgs a) {
    constexpr int BN = 128;
    constexpr int TMW = BM >= 64 ? 2 : 1;          // 32-row MFMA tiles per wave along co
    constexpr int WM = BM / (32 * TMW), WN = 4 / WM;   // waves along co / along n
    constexpr int TN = BN / WN / 32;               // 32-wide MFMA tiles per wave along n
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A4 = BM / 4;                     // float4 columns of the dy tile
    constexpr int APASS = 256 / A4;                // dy rows covered by one pass of the block
    constexpr int RA = (BK + APASS - 1) / APASS;   // dy rows per thread per step
    __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];   // dy tile   [pixel][co]
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];   // x-shifted [pixel][n]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int co0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int split = blockIdx.z;
    const long p_begin = (long)split * a.pix_per_split;
    long p_end = p_begin + a.pix_per_split;
    if (p_end > a.M) p_end = a.M;
    const int Hs = a.ups ? a.Hi >> 1 : a.Hi, Ws = a.ups ? a.Wi >> 1 : a.Wi;

    // dy loader: float4 along co
    const int akr = t / A4, ac4 = t % A4;
    const int coa = co0 + ac4 * 4;
    // x loader: one fixed column n (-> ci, tap) per thread, 8 pixel rows (bk2, bk2+2, ...)
    const int bn = t & 127, bk2 = t >> 7;
    const int ncol = n0 + bn;
    const bool n_ok = ncol < a.NT;
    const int ci = n_ok ? ncol / a.ntaps : 0;
    const int tap = ncol - ci * a.ntaps;
    const int dyb = tap / a.kw - a.pad, dxb = tap % a.kw - a.pad;

    float4 ra[RA];
    float rb[8];
    auto load_step = [&](long p0) {
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const long p = p0 + akr + APASS * j;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
            if (akr + APASS * j < BK && p < p_end && coa < a.Cout) {
                va = *reinterpret_cast<const float4*>(a.dy + p * a.ld_dy + coa);
                const int rem = a.Cout - coa;
                if (rem < 4) {
                    if (rem < 2) va.y = 0.f;
                    if (rem < 3) va.z = 0.f;
                    va.w = 0.f;
                }
            }
            ra[j] = va;
        }
        // (n_img, h, w) of the first row, then incremental updates (rows advance by 2 pixels)
        long p = p0 + bk2;
        int w = (int)(p % a.W);
        long tt = p / a.W;
        int h = (int)(tt % a.H);
        long nimg = tt / a.H;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (n_ok && p < p_end) {
                const int hh = h + dyb, ww = w + dxb;
                if (hh >= 0 && hh < a.Hi && ww >= 0 && ww < a.Wi) {
                    const int hs = a.ups ? hh >> 1 : hh, wsrc = a.ups ? ww >> 1 : ww;
                    v = a.x[((nimg * Hs + hs) * Ws + wsrc) * a.ld_x + ci];
                }
            }
            rb[j] = v;
            p += 2;
            w += 2;
            while (w >= a.W) {
                w -= a.W;
                if (++h >= a.H) {
                    h = 0;
                    ++nimg;
                }
            }
        }
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int j = 0; j < RA; ++j)
            if (akr + APASS * j < BK) *reinterpret_cast<float4*>(&As[buf][akr + APASS * j][ac4 * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[buf][bk2 + 2 * j][bn] = rb[j];
    };

    f32x16 acc[TMW][TN];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int fi = lane & 31, fk = lane >> 5;
    if (p_begin < p_end) {
        load_step(p_begin);
        store_step(0);
    }
    __syncthreads();
    int it = 0;
    for (long p0 = p_begin; p0 < p_end; p0 += BK, ++it) {
        const int buf = it & 1;
        if (p0 + BK < p_end) load_step(p0 + BK);
#pragma unroll
        for (int e = 0; e < BK / 2; ++e) {
            float fa[TMW], fb[TN];
#pragma unroll
            for (int i = 0; i < TMW; ++i) fa[i] = As[buf][2 * e + fk][wm * (32 * TMW) + 32 * i + fi];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = Bs[buf][2 * e + fk][wn * (32 * TN) + 32 * j + fi];
#pragma unroll
            for (int i = 0; i < TMW; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (p0 + BK < p_end) store_step(buf ^ 1);
        __syncthreads();
    }
    // rows = co, cols = n (contiguous in the parameter layout): 32 lanes write 128 consecutive bytes
    const bool partial = a.splits > 1;       // split partials are summed in a fixed order by the reduction (no fp32 atomics)
    float* outp = partial ? a.out + (long)split * a.Cout * a.NT : a.out;
    const long ldo = partial ? (long)a.NT : a.ld_out;
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * (32 * TN) + 32 * j + fi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * (32 * TMW) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fk;
                if (co < a.Cout && n < a.NT) outp[(long)co * ldo + n] = acc[i][j][r];
            }
        }
}

// ---- weight gradient, LDS-halo form (layers with W >= 16) -------------------------------------------------------
// One block owns a 64 (co) x 64 (ci) x 3 (one tap ROW: ky fixed, kx = 0..2) slab of dW and walks a range of 64-pixel
// tiles (TR rows x TC columns of one frame, TC = min(W,64)).  Per tile it stages in LDS (a) the dy tile [64 px][64 co]
// and (b) the x rows shifted by ky-1 with one ZERO-bordered column on each side [(TR) x (TC+2) px][64 ci]; the three
// kx taps are then served from LDS: B(k = pixel, n = ci) for kx is the staged row shifted by kx-1 -- no per-tap global
// gathers, no masks.  Each wave owns one 32x32 (co, ci) quadrant = 3 accumulators; per pixel pair it issues 1 + 3
// ds_read_b32 and 3 MFMAs.  Splitting the taps over blockIdx.y triples the block count at the same split-K partial
// volume (different tap rows write different dW elements), which is what keeps the partial traffic small.
struct WgradHaloArgs {
    const float* x;
    int ld_x, C, ups;
    const float* dy;
    int ld_dy, Cout;
    int N, H, W;
    int TR, TC, tiles_w, tiles_per_img, gn;
    long total_tiles, tiles_per_split;
    int NT;
    float* out;
    long ld_out;
    int splits;
};

constexpr int WH_HP = 72;   // max staged x pixels: TR x (TC+2) = 1x66, 2x34, 4x18

__global__ void __launch_bounds__(256) conv3x3_wgrad_halo_kernel(WgradHaloArgs a) {
    __shared__ __attribute__((aligned(16))) float As[64][68];        // dy tile  [pixel][co]
    __shared__ __attribute__((aligned(16))) float Xs[WH_HP][64];     // x rows   [staged pixel][ci]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cot = wave >> 1, cit = wave & 1;
    const int fi = lane & 31, fk = lane >> 5;
    const int co0 = blockIdx.x * 64;
    const int ci0 = (blockIdx.y % a.gn) * 64;
    const int ky = blockIdx.y / a.gn;            // tap row 0..2  (dy = ky - 1)
    const int split = blockIdx.z;
    const long tile_begin = (long)split * a.tiles_per_split;
    long tile_end = tile_begin + a.tiles_per_split;
    if (tile_end > a.total_tiles) tile_end = a.total_tiles;
    const int TC = a.TC, TR = a.TR, HW2 = TC + 2, HP = TR * HW2;
    const int Hs = a.ups ? a.H >> 1 : a.H, Ws = a.ups ? a.W >> 1 : a.W;

    f32x16 acc[3];
#pragma unroll
    for (int tp = 0; tp < 3; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;

    for (long tile = tile_begin; tile < tile_end; ++tile) {
        const int n = (int)(tile / a.tiles_per_img);
        const int ti = (int)(tile - (long)n * a.tiles_per_img);
        const int r0 = (ti / a.tiles_w) * TR, c0 = (ti % a.tiles_w) * TC;
        __syncthreads();   // previous tile's LDS reads are done
        // ---- dy tile: pixel q = (q / TC, q % TC), 16 float4 of co per pixel
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = (t >> 4) + 16 * j, c4 = t & 15;
            const int r = q / TC, c = q - r * TC;
            const int h = r0 + r, w = c0 + c, co = co0 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (h < a.H && w < a.W && co < a.Cout) {
                v = *reinterpret_cast<const float4*>(a.dy + (((long)n * a.H + h) * a.W + w) * a.ld_dy + co);
                const int rem = a.Cout - co;
                if (rem < 4) {
                    if (rem < 2) v.y = 0.f;
                    if (rem < 3) v.z = 0.f;
                    v.w = 0.f;
                }
            }
            *reinterpret_cast<float4*>(&As[q][c4 * 4]) = v;
        }
        // ---- x rows (shifted by ky-1) with zero border columns / rows outside the frame
        for (int idx = t; idx < HP * 16; idx += 256) {
            const int hp = idx >> 4, c4 = idx & 15;
            const int hr = hp / HW2, hc = hp - hr * HW2;
            const int h = r0 + hr + ky - 1, w = c0 + hc - 1, ci = ci0 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (h >= 0 && h < a.H && w >= 0 && w < a.W && ci < a.C) {
                const int hs = a.ups ? h >> 1 : h, wsrc = a.ups ? w >> 1 : w;
                const float* px = a.x + (((long)n * Hs + hs) * Ws + wsrc) * a.ld_x + ci;
                const int rem = a.C - ci;
                if (rem >= 4) {
                    v = *reinterpret_cast<const float4*>(px);
                } else {   // ld_x is only guaranteed >= C: read the tail element-wise
                    v.x = px[0];
                    if (rem > 1) v.y = px[1];
                    if (rem > 2) v.z = px[2];
                }
            }
            *reinterpret_cast<float4*>(&Xs[hp][c4 * 4]) = v;
        }
        __syncthreads();
        // ---- 32 pixel pairs x 3 taps
        int r = 0, c = fk;               // pixel q = 2e + fk  ->  (r, c); TC is even
        while (c >= TC) {
            c -= TC;
            ++r;
        }
#pragma unroll 4
        for (int e = 0; e < 32; ++e) {
            const float av = As[2 * e + fk][cot * 32 + fi];
            const float* xb = &Xs[r * HW2 + c][cit * 32 + fi];      // kx = 0 reads column c-1 (+1 border) = index c
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[64], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[128], acc[2], 0, 0, 0);
            c += 2;
            if (c >= TC) {
                c -= TC;
                ++r;
            }
        }
    }
    const bool partial = a.splits > 1;
    float* outp = partial ? a.out + (long)split * a.Cout * a.NT : a.out;
    const long ldo = partial ? (long)a.NT : a.ld_out;
    const int ci = ci0 + cit * 32 + fi;
#pragma unroll
    for (int tp = 0; tp < 3; ++tp)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int co = co0 + cot * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * fk;
            if (co < a.Cout && ci < a.C) outp[(long)co * ldo + ci * 9 + ky * 3 + tp] = acc[tp][rr];
        }
}

// ---- weight gradient, narrow layers (C, Cout <= 64 at high resolution: the 45-channel refinement stack) ------------
// 16x16x4 MFMA tiles on a 48 (co) x 48 (ci) channel tile (45 channels fill 94 % of it; a 64-wide tile only 49 %) with
// ALL nine taps in one block: per 8x8-pixel tile the dy tile [64 px][48 co] and the x tile with a one-pixel halo
// [10 x 10 px][48 ci] are staged in LDS once, and every tap is a shifted LDS read.
// Work split over the 4 wavefronts (81 = 9 taps x 3 co tiles x 3 ci tiles accumulators of 4 registers): wavefront w
// owns taps 2w and 2w+1 completely (18 tiles, sharing the three dy fragments) plus co tile w of tap 8 (3 tiles;
// wavefront 3 repeats one as a dummy) -- 21 MFMAs per 13 ds_read_b32 and K group, 96 % balanced.
// The next pixel tile is prefetched into registers while the MFMAs of the current one run.
// LDS rows are 48 floats (= 16 mod 32 banks): the four 16-lane groups of a fragment read hit disjoint banks.
struct WgradN16Args {
    const float* x;
    int ld_x, C, ups;
    const float* dy;
    int ld_dy, Cout;
    int H, W;
    int tiles_w, tiles_per_img;
    long total_tiles, tiles_per_split;
    int NT;
    float* out;
    long ld_out;
    int splits;
};

template <int NCT, int NCI>     // 16-wide co / ci tiles in use (1..3): narrower layers skip the padded tiles at compile time
__device__ __forceinline__ void wgrad_n16_body(const WgradN16Args& a, int bxi, int byi, int split) {
    constexpr int LD = 48, HW2 = 10, HP = 100;
    constexpr int XP = (HP * 12 + 255) / 256;                       // x loader passes (5)
    __shared__ __attribute__((aligned(16))) float As[64][LD];       // dy tile [pixel][co]
    __shared__ __attribute__((aligned(16))) float Xs[HP][LD];       // x tile with halo [staged pixel][ci]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int co0 = bxi * 48, ci0 = byi * 48;
    const long tile_begin = (long)split * a.tiles_per_split;
    long tile_end = tile_begin + a.tiles_per_split;
    if (tile_end > a.total_tiles) tile_end = a.total_tiles;
    const int Hs = a.ups ? a.H >> 1 : a.H, Ws = a.ups ? a.W >> 1 : a.W;

    f32x4 acc[2][NCT][NCI];       // taps 2*wave + {0, 1}: [tap][co tile][ci tile]
    f32x4 accx[NCI];              // tap 8, co tile xc: [ci tile]
#pragma unroll
    for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int i = 0; i < NCT; ++i)
#pragma unroll
            for (int j = 0; j < NCI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[tp][i][j][r] = 0.f;
#pragma unroll
    for (int j = 0; j < NCI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) accx[j][r] = 0.f;
    // staged-pixel offsets of this wavefront's taps (kernel row * 10 + kernel column) and its co tile of tap 8
    const int tap0 = 2 * wave, tap1 = 2 * wave + 1;
    const int toff0 = (tap0 / 3) * HW2 + tap0 % 3, toff1 = (tap1 / 3) * HW2 + tap1 % 3, toffx = 2 * HW2 + 2;
    const int xc = wave < NCT ? wave : 0;

    // loader assignment: dy 64 px x 12 float4 = 3 per thread; x 100 px x 12 float4 = 1200 -> 5 passes of 256
    float4 rd[3], rx[XP];
    const int tail_b0 = a.C - ci0;                // valid channels from the tile start

    auto zero_tail = [&](float4 v, int tl) __attribute__((always_inline)) {
        v.x = tl < 1 ? 0.f : v.x;
        v.y = tl < 2 ? 0.f : v.y;
        v.z = tl < 3 ? 0.f : v.z;
        v.w = tl < 4 ? 0.f : v.w;
        return v;
    };
    auto load_tile = [&](long tile) __attribute__((always_inline)) {
        const unsigned ut = (unsigned)tile;                        // total_tiles < 2^31 (host check)
        const int n = (int)(ut / (unsigned)a.tiles_per_img);
        const unsigned ti = ut - (unsigned)n * (unsigned)a.tiles_per_img, tr = ti / (unsigned)a.tiles_w;
        const int r0 = (int)tr * 8, c0 = (int)(ti - tr * (unsigned)a.tiles_w) * 8;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int idx = t + 256 * j;
            const int q = idx / 12, c4 = idx % 12;       // 256 * 3 = 64 px * 12 float4 exactly
            const int h = r0 + (q >> 3), w = c0 + (q & 7);
            const int tl = a.Cout - (co0 + c4 * 4);
            const int ce = tl > 0 ? co0 + c4 * 4 : 0;
            const float4 v = *reinterpret_cast<const float4*>(a.dy + (((long)n * a.H + h) * a.W + w) * a.ld_dy + ce);
            rd[j] = zero_tail(v, tl);
        }
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            const int idx = t + 256 * j;
            const int hp = idx / 12 < HP ? idx / 12 : HP - 1, c4 = idx % 12;
            const int hr = hp / HW2, hc = hp - hr * HW2;
            int h = r0 + hr - 1, w = c0 + hc - 1;
            const bool ok = h >= 0 && h < a.H && w >= 0 && w < a.W;
            h = h < 0 ? 0 : (h >= a.H ? a.H - 1 : h);
            w = w < 0 ? 0 : (w >= a.W ? a.W - 1 : w);
            const int tl = ok ? tail_b0 - c4 * 4 : 0;
            const int ce = tl > 0 ? ci0 + c4 * 4 : 0;
            const float4 v = *reinterpret_cast<const float4*>(
                a.x + (((long)n * Hs + (h >> a.ups)) * Ws + (w >> a.ups)) * a.ld_x + ce);
            rx[j] = zero_tail(v, tl);
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {             // 256 * 3 = 768 = 64 px * 12 exactly; the float4 column is idx % 12
            const int idx = t + 256 * j;
            *reinterpret_cast<float4*>(&As[idx / 12][(idx % 12) * 4]) = rd[j];
        }
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            const int idx = t + 256 * j;
            if (idx < HP * 12) *reinterpret_cast<float4*>(&Xs[idx / 12][(idx % 12) * 4]) = rx[j];
        }
    };

    const int fi = lane & 15, fk = lane >> 4;     // row/col inside a 16-tile, pixel 0..3 of the K group
    if (tile_begin < tile_end) load_tile(tile_begin);
    for (long tile = tile_begin; tile < tile_end; ++tile) {
        __syncthreads();                          // the previous tile's LDS reads are done
        store_tile();
        __syncthreads();
        if (tile + 1 < tile_end) load_tile(tile + 1);     // in flight during the MFMAs below
#pragma unroll 2
        for (int g = 0; g < 16; ++g) {            // K group = pixels 4g..4g+3 = row g>>1, columns 4*(g&1)..+3
            const int q = 4 * g + fk;
            const int xr = (g >> 1) * HW2 + (g & 1) * 4 + fk;        // staged pixel of tap (0, 0)
            float fa[NCT], fb0[NCI], fb1[NCI], fbx[NCI];
#pragma unroll
            for (int i = 0; i < NCT; ++i) fa[i] = As[q][16 * i + fi];
            const float fax = As[q][16 * xc + fi];
#pragma unroll
            for (int j = 0; j < NCI; ++j) {
                fb0[j] = Xs[xr + toff0][16 * j + fi];
                fb1[j] = Xs[xr + toff1][16 * j + fi];
                fbx[j] = Xs[xr + toffx][16 * j + fi];
            }
#pragma unroll
            for (int i = 0; i < NCT; ++i)
#pragma unroll
                for (int j = 0; j < NCI; ++j) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb0[j], acc[0][i][j], 0, 0, 0);
                    acc[1][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb1[j], acc[1][i][j], 0, 0, 0);
                }
#pragma unroll
            for (int j = 0; j < NCI; ++j) accx[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fax, fbx[j], accx[j], 0, 0, 0);
        }
    }
    // D: col = lane & 15 (-> ci), row = 4 * (lane >> 4) + r (-> co).  A single split writes the parameter layout
    // (n = ci * 9 + tap) directly; split partials are tap-major [split][tap][co][ci] -- 64-byte runs along ci instead
    // of 36-byte-strided words (measured: 82 MB of HBM writes per launch for 37 MB of partials) -- and are summed and
    // transposed by conv3x3_wgrad_tap_reduce_kernel.
    const bool partial = a.splits > 1;
    float* outp = partial ? a.out + (long)split * a.Cout * a.NT : a.out;
    const long ldo = partial ? (long)a.C : a.ld_out;                 // row stride (co)
    const long tstride = partial ? (long)a.Cout * a.C : 1;             // tap stride
    const int cstride = partial ? 1 : 9;                               // ci stride
    if (wave < 4) {
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
            const int tap = 2 * wave + tp;
            if (tap < 8)
#pragma unroll
                for (int i = 0; i < NCT; ++i)
#pragma unroll
                    for (int j = 0; j < NCI; ++j) {
                        const int ci = ci0 + 16 * j + fi;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int co = co0 + 16 * i + 4 * fk + r;
                            if (co < a.Cout && ci < a.C)
                                outp[tap * tstride + (long)co * ldo + ci * cstride] = acc[tp][i][j][r];
                        }
                    }
        }
        if (wave < NCT)
#pragma unroll
            for (int j = 0; j < NCI; ++j) {
                const int ci = ci0 + 16 * j + fi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + 16 * xc + 4 * fk + r;
                    if (co < a.Cout && ci < a.C) outp[8 * tstride + (long)co * ldo + ci * cstride] = accx[j][r];
                }
            }
    }
}

template <int NCT, int NCI>
__global__ void __launch_bounds__(256, 2) conv3x3_wgrad_n16_kernel(WgradN16Args a) {
    wgrad_n16_body<NCT, NCI>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// index of the last record whose block_begin (an int column with `stride_ints` between rows) is <= b
__device__ __forceinline__ int find_desc(const int* begins_stride_bytes_base, int stride_ints, int n, int b, int* sh) {
    // sh: one LDS int; every thread of the block returns the index of the last descriptor with block_begin <= b
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        if (i < n && begins_stride_bytes_base[(long)i * stride_ints] <= b) atomicAdd(sh, 1);    // LDS atomic, <= n per block
    }
    __syncthreads();
    return *sh - 1;
}

// ---- weight gradient, tap-major form (the default for C >= 16) ---------------------------------------------------
// The same pipeline as the forward kernel with K = pixels: one block owns a BM (co) x BN (ci) tile of ONE tap and a
// range of pixels.  Per 16-pixel K step both operands are plain coalesced float4 reads along channels -- dy rows
// [pixel][co] and x rows of the tap-shifted pixels [pixel + off(tap)][ci] (clamped into the image, zeroed on the way
// to LDS when the tap falls outside) -- so there are no scalar gathers and no branches in the steady-state loop;
// registers hold step s+1, loads of step s+2 are issued before the MFMAs of step s.  The tile is written to a
// tap-major partial [split][tap][co][ci] (coalesced along ci); conv3x3_wgrad_tap_reduce_kernel sums the splits and
// transposes (tap, ci) -> the parameter order ci*ntaps + tap through LDS.
struct WgradTapArgs {
    const float* x;
    int ld_x, C, ups;
    const float* dy;
    int ld_dy, Cout;
    int H, W;            // dy geometry
    int Hi, Wi, ntaps, kw, pad;
    long M, pix_per_split;
    int gn;              // ci tiles per tap
    float* part;         // [splits][ntaps][Cout][C]
    unsigned mulW, shW, mulH, shH;   // division by W / H of a pixel index < 2^31 (mul == 0: shift only)
    int xcd;             // re-chunk the launch order per XCD (xcd_tile)
    int clean;           // pad channels of x and dy hold zeros: the buffer-load fast path may be used
    int sw, sh, sn;      // fast path: one 16-pixel K step = sw columns + sh rows + sn frames
    // small maps (H * W <= wtap_compact, MODE 0 / 3): K runs over the pixels whose tap lies INSIDE the source only -- on a 2 x 2 map
    // a corner tap sees one pixel of four, an edge tap two (56 % of the (pixel, tap) pairs of a 3x3 pad-1 convolution are zeros
    // there, 31 % on 4 x 4, 16 % on 8 x 8; three quarters of the sub-pixel form's pseudo taps on a 1 x 1 source).  The range of a
    // tap is cut into `nsplits` equal pieces.  compact == 2 (MODE 3 on a 1 x 1 source, up1x1_skips): the launch has tiles for the
    // four LIVE pseudo taps only (pack_tile.h: up1x1_live_tap) -- the tile index along the taps counts phases, and the slices
    // of the twelve dead pseudo taps of `part` are not written.
    int compact, nsplits;
    // MODE 3 -- sub-pixel form of an up-sampled 3x3 convolution: H, W, M are the LOW resolution; the 16 "taps" are
    // t = 4 * (2a + b) + (2u + v): dWeff[t] = sum_{n,i,j} dy[n, 2i+a, 2j+b] (x) x[n, i+a-1+u, j+b-1+v]  (4/9 of the multiply-adds of
    // the nine-tap form; the reduction folds the 16 pseudo taps into the nine kernel taps)
};

// MODE 0: generic loader (any K x K, masks, clamps, magic-number division per row and step).  MODE 1 / 2: 3x3 pad 1 with
// clean pad channels, W >= 16 (plain / x2 up-sampled source): raw buffer loads whose out-of-range lanes read zero --
// dy rows beyond the split's pixel range fall off the end of the buffer, taps outside the image and float4s beyond
// the channel count get bit 30 added to their offset -- and the (h, w) of a row is advanced incrementally (16 pixels
// per step wrap at most once), so a row costs ~10 vector instructions per step instead of ~35.
template <int BM, int BN, int WM, int WN, int MODE>
__device__ __forceinline__ void wgrad_tap_body(const WgradTapArgs& a, const int bx, const int by, const int split) {
    static_assert(WM * WN == 4, "4 waves per block");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A4 = BM / 4, B4 = BN / 4;              // float4 columns of a tile row
    constexpr int APASS = 256 / A4, BPASS = 256 / B4;     // pixel rows covered by one pass of the block
    constexpr int RA = (BK + APASS - 1) / APASS, RB = (BK + BPASS - 1) / BPASS;
    static_assert(RA <= 2 && RB <= 2, "at most two rows per thread and operand");
    __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];   // dy tile   [pixel][co]
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];   // x-shifted [pixel][ci]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    constexpr bool SUBPIX = MODE == 3, FAST = MODE == 1 || MODE == 2;
    const int co0 = bx * BM;
    const int tapi = by / a.gn;
    const int ci0 = (by - tapi * a.gn) * BN;
    const int tap = SUBPIX && a.compact == 2 ? up1x1_live_tap(tapi) : tapi;     // 1 x 1 source: tiles of the live pseudo taps only
    long p_begin = (long)split * a.pix_per_split;
    long p_end = p_begin + a.pix_per_split;
    if (p_end > a.M) p_end = a.M;
    const int Hs = a.ups ? a.Hi >> 1 : a.Hi, Ws = a.ups ? a.Wi >> 1 : a.Wi;
    const int ph_a = (tap >> 3) & 1, ph_b = (tap >> 2) & 1;                      // SUBPIX: output phase of this pseudo tap
    const int dyt = SUBPIX ? ph_a - 1 + ((tap >> 1) & 1) : tap / a.kw - a.pad;   // SUBPIX: low-resolution row / column offset
    const int dxt = SUBPIX ? ph_b - 1 + (tap & 1) : tap % a.kw - a.pad;
    const int hmax = a.Hi - 1, wmax = a.Wi - 1;
    // compact K (small maps): the rectangle [ch0, ch0 + chh) x [cw0, cw0 + cww) of output pixels whose tap lies inside the source;
    // K index k -> (frame, row, column) of that rectangle, Kt = frames * chh * cww entries
    const bool compact = !FAST && a.compact;
    int ch0 = 0, cw0 = 0, chh = a.H, cww = a.W;
    float inv_chh = 0.f, inv_cww = 0.f;
    long Klast = a.M - 1;
    if (compact) {
        ch0 = dyt < 0 ? -dyt : 0;
        cw0 = dxt < 0 ? -dxt : 0;
        int h1 = a.Hi - dyt, w1 = a.Wi - dxt;
        h1 = h1 > a.H ? a.H : h1;
        w1 = w1 > a.W ? a.W : w1;
        chh = h1 > ch0 ? h1 - ch0 : 0;
        cww = w1 > cw0 ? w1 - cw0 : 0;
        const long frames = a.M / ((long)a.H * a.W);
        const long Kt = frames * chh * cww;
        const long per = ((Kt + a.nsplits - 1) / a.nsplits + BK - 1) / BK * BK;
        p_begin = (long)split * per;
        p_end = p_begin + per;
        if (p_end > Kt) p_end = Kt;
        if (p_begin > p_end) p_begin = p_end;
        Klast = Kt > 0 ? Kt - 1 : 0;
        inv_chh = chh > 0 ? 1.f / (float)chh : 0.f;
        inv_cww = cww > 0 ? 1.f / (float)cww : 0.f;
    }
    const unsigned plast = (unsigned)Klast, pend = (unsigned)p_end;
    // k -> (n, i, j) inside the rectangle; k < 2^20: (k + 0.5) / d is at least 0.5 / d away from an integer, far beyond the rounding
    auto unpack = [&](unsigned k, unsigned& n, unsigned& i, unsigned& j) __attribute__((always_inline)) {
        const unsigned q = (unsigned)(((float)k + 0.5f) * inv_cww);
        j = k - q * (unsigned)cww + (unsigned)cw0;
        n = (unsigned)(((float)q + 0.5f) * inv_chh);
        i = q - n * (unsigned)chh + (unsigned)ch0;
    };

    const int ar = t / A4, ac4 = t % A4, br = t / B4, bc4 = t % B4;
    const int coa = co0 + ac4 * 4, cib = ci0 + bc4 * 4;
    const int tail_a = a.Cout - coa, tail_b = a.C - cib;
    const unsigned coa_e = tail_a > 0 ? coa : 0, cib_e = tail_b > 0 ? cib : 0;

    float4 ra0, ra1, rb0, rb1;
    int ta0 = 0, ta1 = 0, tb0 = 0, tb1 = 0;       // valid channels of the float4s (<= 0: zero the whole vector)

    auto load_a = [&](unsigned p, float4& v, int& tl) __attribute__((always_inline)) {
        tl = p < pend ? tail_a : 0;
        const unsigned pe = p < plast ? p : plast;
        unsigned long row = pe;
        if (compact) {
            unsigned n, i, j;
            unpack(pe, n, i, j);
            row = SUBPIX ? ((unsigned long)(n * (unsigned)a.H + i) * 2u + (unsigned)ph_a) * (2u * (unsigned)a.W) + 2u * j + (unsigned)ph_b
                         : (unsigned long)(n * (unsigned)a.H + i) * (unsigned)a.W + j;
        } else if constexpr (SUBPIX) {   // low-resolution pixel (n, i, j) -> pixel (2i + a, 2j + b) of the up-sampled dy
            const unsigned q = fast_div(pe, a.mulW, a.shW), n = fast_div(q, a.mulH, a.shH);
            const unsigned j = pe - q * (unsigned)a.W, i = q - n * (unsigned)a.H;
            row = ((unsigned long)(n * (unsigned)a.H + i) * 2u + (unsigned)ph_a) * (2u * (unsigned)a.W) + 2u * j + (unsigned)ph_b;
        }
        v = *reinterpret_cast<const float4*>(a.dy + row * (unsigned)a.ld_dy + coa_e);
    };
    auto load_b = [&](unsigned p, float4& v, int& tl) __attribute__((always_inline)) {
        const unsigned pe = p < plast ? p : plast;
        if (compact) {                   // every entry of the range lies inside the source: no clamps, no masks but the range's end
            unsigned n, i, j;
            unpack(pe, n, i, j);
            tl = p < pend ? tail_b : 0;
            const unsigned pix = (n * (unsigned)Hs + (unsigned)((int)i + dyt)) * (unsigned)Ws + (unsigned)((int)j + dxt);
            v = *reinterpret_cast<const float4*>(a.x + (unsigned long)pix * (unsigned)a.ld_x + cib_e);
            return;
        }
        const unsigned q = fast_div(pe, a.mulW, a.shW);
        const int w = (int)(pe - q * (unsigned)a.W);
        const unsigned n = fast_div(q, a.mulH, a.shH);
        const int h = (int)(q - n * (unsigned)a.H);
        int hh = h + dyt, ww = w + dxt;
        const bool ok = hh >= 0 && hh <= hmax && ww >= 0 && ww <= wmax;
        hh = hh < 0 ? 0 : (hh > hmax ? hmax : hh);
        ww = ww < 0 ? 0 : (ww > wmax ? wmax : ww);
        tl = ok ? tail_b : 0;
        const unsigned pix = (n * (unsigned)Hs + (unsigned)(hh >> a.ups)) * (unsigned)Ws + (unsigned)(ww >> a.ups);
        v = *reinterpret_cast<const float4*>(a.x + (unsigned long)pix * (unsigned)a.ld_x + cib_e);
    };
    // ---- fast loader state (MODE 1 / 2) ---------------------------------------------------------------------
    constexpr bool FUPS = MODE == 2;
    __amdgpu_buffer_rsrc_t rsa, rsb;
    unsigned aoff0 = 0, aoff1 = 0, boff0 = 0, boff1 = 0;     // running byte offsets (non-ups B: linear in the pixel)
    int bw0 = 0, bh0 = 0, bn0 = 0, bw1 = 0, bh1 = 0, bn1 = 0;  // (w, h, frame relative to the first) of the B rows
    const int ldy4 = a.ld_dy * 4, ldx4 = a.ld_x * 4;
    const int hbad = dyt < 0 ? 0 : (dyt > 0 ? a.H - 1 : -1), wbad = dxt < 0 ? 0 : (dxt > 0 ? a.W - 1 : -1);
    if constexpr (FAST) {
        rsa = uniform_rsrc(a.dy + p_begin * a.ld_dy, (unsigned)((p_end - p_begin) * ldy4));
        const unsigned tail_flag_a = tail_a > 0 ? 0u : 0x40000000u, tail_flag_b = tail_b > 0 ? 0u : 0x40000000u;
        aoff0 = (unsigned)(ar * ldy4 + (int)coa_e * 4) + tail_flag_a;
        aoff1 = aoff0 + (unsigned)(APASS * ldy4);
        const long frame_px = (long)a.H * a.W;
        const long nb = p_begin / frame_px;                       // first frame of the split
        long pb0 = FUPS ? nb * Hs * Ws : p_begin + dyt * a.W + dxt;   // pixel the B resource starts at
        if (pb0 < 0) pb0 = 0;
        const long total_src = FUPS ? (a.M / frame_px) * Hs * Ws : a.M;
        long nrec = (total_src - pb0) * ldx4;
        if (nrec > 0x40000000L) nrec = 0x40000000L;
        // a split that starts in the last image row has pb0 > total_src for the taps of the row below (every row of it is
        // "bad"): an empty buffer -- a negative length would wrap to ~4 GB of "valid" range and the bit-30 offsets of the
        // bad rows would be dereferenced (seen as a memory fault at 256x256: three image rows per split)
        if (nrec < 0) nrec = 0;
        rsb = uniform_rsrc(a.x + pb0 * a.ld_x, (unsigned)nrec);
        auto init_b = [&](long p, int& w, int& h, int& n, unsigned& off) __attribute__((always_inline)) {
            const unsigned up = (unsigned)p, q = fast_div(up, a.mulW, a.shW), fr = fast_div(q, a.mulH, a.shH);
            w = (int)(up - q * (unsigned)a.W);
            h = (int)(q - fr * (unsigned)a.H);
            n = (int)((long)fr - nb);
            off = (FUPS ? (unsigned)((int)cib_e * 4) : (unsigned)((int)(p + dyt * a.W + dxt - pb0) * ldx4 + (int)cib_e * 4)) +
                  tail_flag_b;
        };
        init_b(p_begin + br, bw0, bh0, bn0, boff0);
        init_b(p_begin + br + BPASS, bw1, bh1, bn1, boff1);
    }
    auto fast_b = [&](int& w, int& h, int& n, unsigned& off, float4& v) __attribute__((always_inline)) {
        const bool bad = (h == hbad) | (w == wbad);
        unsigned o = off;
        if constexpr (FUPS)
            o += (unsigned)(((n * Hs + ((h + dyt) >> 1)) * Ws + ((w + dxt) >> 1)) * ldx4);
        o |= bad ? 0x40000000u : 0u;
        v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsb, o, 0, 0));
        if constexpr (!FUPS) off += (unsigned)(BK * ldx4);
        // 16 pixels ahead as (sw, sh, sn) columns / rows / frames (host: W >= 16 -> (16,0,0); W | 16 -> rows or whole
        // frames), each with at most one wrap
        w += a.sw;
        const bool ww = w >= a.W;
        w -= ww ? a.W : 0;
        h += a.sh + (ww ? 1 : 0);
        const bool hw = h >= a.H;
        h -= hw ? a.H : 0;
        if constexpr (FUPS) n += a.sn + (hw ? 1 : 0);
    };
    auto load_step = [&](long p0) __attribute__((always_inline)) {
        if constexpr (FAST) {
            ra0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsa, aoff0, 0, 0));
            aoff0 += (unsigned)(BK * ldy4);
            if constexpr (RA > 1) {
                ra1 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsa, aoff1, 0, 0));
                aoff1 += (unsigned)(BK * ldy4);
            }
            fast_b(bw0, bh0, bn0, boff0, rb0);
            if constexpr (RB > 1) fast_b(bw1, bh1, bn1, boff1, rb1);
        } else {
            const unsigned pa = (unsigned)p0 + ar, pb = (unsigned)p0 + br;
            load_a(pa, ra0, ta0);
            if constexpr (RA > 1) load_a(pa + APASS, ra1, ta1);
            load_b(pb, rb0, tb0);
            if constexpr (RB > 1) load_b(pb + BPASS, rb1, tb1);
        }
    };
    auto masked = [&](float4 v, int tl) __attribute__((always_inline)) {
        if constexpr (FAST) return v;
        v.x = tl < 1 ? 0.f : v.x;
        v.y = tl < 2 ? 0.f : v.y;
        v.z = tl < 3 ? 0.f : v.z;
        v.w = tl < 4 ? 0.f : v.w;
        return v;
    };
    auto store_step = [&](int buf) __attribute__((always_inline)) {
        if (APASS >= BK ? ar < BK : true) *reinterpret_cast<float4*>(&As[buf][ar][ac4 * 4]) = masked(ra0, ta0);
        if constexpr (RA > 1) *reinterpret_cast<float4*>(&As[buf][ar + APASS][ac4 * 4]) = masked(ra1, ta1);
        if (BPASS >= BK ? br < BK : true) *reinterpret_cast<float4*>(&Bs[buf][br][bc4 * 4]) = masked(rb0, tb0);
        if constexpr (RB > 1) *reinterpret_cast<float4*>(&Bs[buf][br + BPASS][bc4 * 4]) = masked(rb1, tb1);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int fi = lane & 31, fk = lane >> 5;
    auto mfma_step = [&](int buf) __attribute__((always_inline)) {
        // fragments are read two pixel pairs ahead of the MFMAs that use them (sched_group_barrier pins the order the
        // source states: without it the scheduler reads each pair right before its MFMAs and waits for the LDS every time)
        float fa[BK / 2][TM], fb[BK / 2][TN];
        auto rd = [&](int e) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[e][i] = As[buf][2 * e + fk][wm * (32 * TM) + 32 * i + fi];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[e][j] = Bs[buf][2 * e + fk][wn * (32 * TN) + 32 * j + fi];
        };
        rd(0);
        rd(1);
#pragma unroll
        for (int e = 0; e < BK / 2; ++e) {
            if (e + 2 < BK / 2) rd(e + 2);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e][i], fb[e][j], acc[i][j], 0, 0, 0);
            MNK_SCHED_GROUP(0x100, TM + TN);      // DS reads of pair e + 2
            MNK_SCHED_GROUP(0x008, TM * TN);      // MFMAs of pair e
        }
    };

    if (p_begin < p_end) {
        load_step(p_begin);
        store_step(0);
        if (p_begin + BK < p_end) load_step(p_begin + BK);
    }
    __syncthreads();
    long p0 = p_begin;
    int it = 0;
    for (; p0 + 2 * BK < p_end; p0 += BK, ++it) {
        const int buf = it & 1;
        store_step(buf ^ 1);
        load_step(p0 + 2 * BK);
        mfma_step(buf);
        __syncthreads();
    }
    if (p0 + BK < p_end) {
        const int buf = it & 1;
        store_step(buf ^ 1);
        mfma_step(buf);
        __syncthreads();
        p0 += BK;
        ++it;
    }
    if (p0 < p_end) mfma_step(it & 1);

    // rows = co, cols = ci: 32 lanes write 128 consecutive bytes of the tap-major partial (32-bit offsets inside the
    // tap plane, no per-row guards when the whole co tile exists)
    float* outp = a.part + ((long)split * a.ntaps + tap) * a.Cout * a.C;
    const unsigned Cu = (unsigned)a.C, corow0 = (unsigned)co0 + wm * (32 * TM) + 4 * fk;
    auto emit = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const unsigned ci = (unsigned)ci0 + wn * (32 * TN) + 32 * j + fi;
                const unsigned cb = corow0 + 32 * i, off0 = cb * Cu + ci;
                if (ci < Cu) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned ro = (r & 3) + 8 * (r >> 2);
                        if (FULL || cb + ro < (unsigned)a.Cout) outp[off0 + ro * Cu] = acc[i][j][r];
                    }
                }
            }
    };
    if (co0 + BM <= a.Cout)
        emit(TrueTag{});
    else
        emit(FalseTag{});
}

// ---- the tap-major weight gradient on the bf16 matrix cores (round 6; GM = 1 of the forward kernel, mnk_common.h) -------------
// K = pixels here, and both operands are K-STRIDED in memory (dy [pixel][co], x [pixel][ci]) while a lane of
// v_mfma_f32_32x32x16_bf16 wants eight consecutive k of ONE channel.  The loader therefore transposes on its way to LDS: a
// loader thread owns four consecutive pixels x four consecutive channels (four float4 loads, lanes along the channels: coalesced
// rows), regroups them per channel, splits each float4-of-pixels into three bf16 planes and writes four halves (8 bytes) per
// plane and channel.  LDS image per plane: 16-byte chunks [k group of 8][channel], chunk(kg, m) = kg * BMP + m + (m >> 4) (one pad
// chunk per 16 channels: conflict-free b128 fragment reads, 2-way on the writes).  Threads [0, BM) load dy, [BM, BM + BN) load x.
// Generic addressing only (magic-number divisions, clamps, masks, the compact K of small maps): the split dominates the loader.
// NPL = 3: the exact three-way split ("wgrad_bf16x3", six MFMAs per tile pair).  NPL = 1: the one-plane form of MNK_WGRAD_BF16 --
// the loader rounds each operand to nearest-even bf16 (mnk_round_bf16x4, the first plane of the split), one MFMA per tile pair;
// the same chunk layout, per plane.
template <int BM, int BN, int WM, int WN, bool SUBPIX, int NPL>
__device__ __forceinline__ void wgrad_tap_body_h(const WgradTapArgs& a, const int bx, const int by, const int split) {
    static_assert(NPL == 1 || NPL == 3, "one rounded plane or the three-way split");
    static_assert(WM * WN == 4, "4 waves per block");
    static_assert(BM + BN <= 256, "one loader thread per (pixel group, channel quad) of both operands");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int BMP = BM + BM / 16, BNP = BN + BN / 16;
    __shared__ __attribute__((aligned(16))) uint4 Ah[2][NPL][2 * BMP];
    __shared__ __attribute__((aligned(16))) uint4 Bh[2][NPL][2 * BNP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int co0 = bx * BM;
    const int tapi = by / a.gn;
    const int ci0 = (by - tapi * a.gn) * BN;
    const int tap = SUBPIX && a.compact == 2 ? up1x1_live_tap(tapi) : tapi;     // (see wgrad_tap_body)
    long p_begin = (long)split * a.pix_per_split;
    long p_end = p_begin + a.pix_per_split;
    if (p_end > a.M) p_end = a.M;
    const int Hs = a.ups ? a.Hi >> 1 : a.Hi, Ws = a.ups ? a.Wi >> 1 : a.Wi;
    const int ph_a = (tap >> 3) & 1, ph_b = (tap >> 2) & 1;
    const int dyt = SUBPIX ? ph_a - 1 + ((tap >> 1) & 1) : tap / a.kw - a.pad;
    const int dxt = SUBPIX ? ph_b - 1 + (tap & 1) : tap % a.kw - a.pad;
    const int hmax = a.Hi - 1, wmax = a.Wi - 1;
    const bool compact = a.compact;
    int ch0 = 0, cw0 = 0, chh = a.H, cww = a.W;
    float inv_chh = 0.f, inv_cww = 0.f;
    long Klast = a.M - 1;
    if (compact) {          // (see wgrad_tap_body)
        ch0 = dyt < 0 ? -dyt : 0;
        cw0 = dxt < 0 ? -dxt : 0;
        int h1 = a.Hi - dyt, w1 = a.Wi - dxt;
        h1 = h1 > a.H ? a.H : h1;
        w1 = w1 > a.W ? a.W : w1;
        chh = h1 > ch0 ? h1 - ch0 : 0;
        cww = w1 > cw0 ? w1 - cw0 : 0;
        const long frames = a.M / ((long)a.H * a.W);
        const long Kt = frames * chh * cww;
        const long per = ((Kt + a.nsplits - 1) / a.nsplits + BK - 1) / BK * BK;
        p_begin = (long)split * per;
        p_end = p_begin + per;
        if (p_end > Kt) p_end = Kt;
        if (p_begin > p_end) p_begin = p_end;
        Klast = Kt > 0 ? Kt - 1 : 0;
        inv_chh = chh > 0 ? 1.f / (float)chh : 0.f;
        inv_cww = cww > 0 ? 1.f / (float)cww : 0.f;
    }
    const unsigned plast = (unsigned)Klast, pend = (unsigned)p_end;
    auto unpack = [&](unsigned k, unsigned& n, unsigned& i, unsigned& j) __attribute__((always_inline)) {
        const unsigned q = (unsigned)(((float)k + 0.5f) * inv_cww);
        j = k - q * (unsigned)cww + (unsigned)cw0;
        n = (unsigned)(((float)q + 0.5f) * inv_chh);
        i = q - n * (unsigned)chh + (unsigned)ch0;
    };
    // loader role: A (dy) threads [0, BM), B (x) threads [BM, BM + BN)
    const bool is_a = t < BM, is_b = !is_a && t < BM + BN;
    const int u = is_a ? t : t - BM;
    const int quads = is_a ? BM / 4 : BN / 4;
    const int cq = u % quads, pg = u / quads;                 // channel quad, pixel group (4 pixels) of the 16-pixel K step
    const int ch = (is_a ? co0 : ci0) + cq * 4;
    const int tail = (is_a ? a.Cout : a.C) - ch;               // real channels of the quad (<= 0: none)
    const unsigned ch_e = tail > 0 ? (unsigned)ch : 0u;

    float4 rv[4];
    int rt[4];
    auto load_one = [&](unsigned p, float4& v, int& tl) __attribute__((always_inline)) {
        const unsigned pe = p < plast ? p : plast;
        tl = p < pend ? tail : 0;
        unsigned n, i, j;
        if (compact) {
            unpack(pe, n, i, j);
        } else {
            const unsigned q = fast_div(pe, a.mulW, a.shW);
            j = pe - q * (unsigned)a.W;
            n = fast_div(q, a.mulH, a.shH);
            i = q - n * (unsigned)a.H;
        }
        if (is_a) {
            const unsigned long row = SUBPIX ? ((unsigned long)(n * (unsigned)a.H + i) * 2u + (unsigned)ph_a) * (2u * (unsigned)a.W) + 2u * j + (unsigned)ph_b
                                             : (unsigned long)(n * (unsigned)a.H + i) * (unsigned)a.W + j;
            v = *reinterpret_cast<const float4*>(a.dy + row * (unsigned)a.ld_dy + ch_e);
        } else {
            int hh = (int)i + dyt, ww = (int)j + dxt;
            const bool ok = hh >= 0 && hh <= hmax && ww >= 0 && ww <= wmax;
            hh = hh < 0 ? 0 : (hh > hmax ? hmax : hh);
            ww = ww < 0 ? 0 : (ww > wmax ? wmax : ww);
            if (!ok) tl = 0;
            const unsigned pix = (n * (unsigned)Hs + (unsigned)(hh >> a.ups)) * (unsigned)Ws + (unsigned)(ww >> a.ups);
            v = *reinterpret_cast<const float4*>(a.x + (unsigned long)pix * (unsigned)a.ld_x + ch_e);
        }
    };
    auto load_step = [&](long p0) __attribute__((always_inline)) {
        if (is_a || is_b) {
#pragma unroll
            for (int i = 0; i < 4; ++i) load_one((unsigned)p0 + 4 * pg + i, rv[i], rt[i]);
        }
    };
    auto store_step = [&](int buf) __attribute__((always_inline)) {
        if (!(is_a || is_b)) return;
        float m[4][4];          // [pixel][channel of the quad], masked
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m[i][0] = rt[i] < 1 ? 0.f : rv[i].x;
            m[i][1] = rt[i] < 2 ? 0.f : rv[i].y;
            m[i][2] = rt[i] < 3 ? 0.f : rv[i].z;
            m[i][3] = rt[i] < 4 ? 0.f : rv[i].w;
        }
        const int rowbase = cq * 4, kg = pg >> 1, half = pg & 1;
        uint4* const planes = is_a ? &Ah[buf][0][0] : &Bh[buf][0][0];
        const int pstride = is_a ? 2 * BMP : 2 * BNP, kstride = is_a ? BMP : BNP;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rowbase + e;
            const int chunk = kg * kstride + row + (row >> 4);
            const float4 k4 = make_float4(m[0][e], m[1][e], m[2][e], m[3][e]);
            if constexpr (NPL == 1) {
                reinterpret_cast<uint2*>(planes + chunk)[half] = mnk_round_bf16x4(k4);
            } else {
                uint2 p0, p1, p2;
                mnk_split3(k4, p0, p1, p2);
                reinterpret_cast<uint2*>(planes + chunk)[half] = p0;
                reinterpret_cast<uint2*>(planes + pstride + chunk)[half] = p1;
                reinterpret_cast<uint2*>(planes + 2 * pstride + chunk)[half] = p2;
            }
        }
    };

    constexpr int NACC = (TM * TN == 1) ? 2 : 1;
    f32x16 acc[NACC][TM][TN];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][i][j][r] = 0.f;
    const int fi = lane & 31, fk = lane >> 5;
    auto mfma_step = [&](int buf) __attribute__((always_inline)) {
        mnk_bf16x8 ha[NPL][TM], hb[NPL][TN];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * (32 * TM) + 32 * i + fi;
                ha[pl][i] = mnk_as_bf16x8(Ah[buf][pl][fk * BMP + row + (row >> 4)]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * (32 * TN) + 32 * j + fi;
                hb[pl][j] = mnk_as_bf16x8(Bh[buf][pl][fk * BNP + row + (row >> 4)]);
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                constexpr int Q = NACC - 1;
                if constexpr (NPL == 1) {
                    // one MFMA per tile pair; a lone tile alternates two accumulators so that consecutive K steps do not chain
                    if (Q && (buf & 1)) acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                    else acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[0][j], acc[0][i][j], 0, 0, 0);
                } else {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[1][i], hb[1][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[2][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[2][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[1][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[1][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                }
            }
    };

    if (p_begin < p_end) {
        load_step(p_begin);
        store_step(0);
        if (p_begin + BK < p_end) load_step(p_begin + BK);
    }
    __syncthreads();
    long p0 = p_begin;
    int it = 0;
    for (; p0 + 2 * BK < p_end; p0 += BK, ++it) {
        const int buf = it & 1;
        store_step(buf ^ 1);
        load_step(p0 + 2 * BK);
        mfma_step(buf);
        __syncthreads();
    }
    if (p0 + BK < p_end) {
        const int buf = it & 1;
        store_step(buf ^ 1);
        mfma_step(buf);
        __syncthreads();
        p0 += BK;
        ++it;
    }
    if (p0 < p_end) mfma_step(it & 1);
    if constexpr (NACC == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][0][r] += acc[1][0][0][r];
    }

    float* outp = a.part + ((long)split * a.ntaps + tap) * a.Cout * a.C;
    const unsigned Cu = (unsigned)a.C, corow0 = (unsigned)co0 + wm * (32 * TM) + 4 * fk;
    auto emit = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const unsigned ci = (unsigned)ci0 + wn * (32 * TN) + 32 * j + fi;
                const unsigned cb = corow0 + 32 * i, off0 = cb * Cu + ci;
                if (ci < Cu) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned ro = (r & 3) + 8 * (r >> 2);
                        if (FULL || cb + ro < (unsigned)a.Cout) outp[off0 + ro * Cu] = acc[0][i][j][r];
                    }
                }
            }
    };
    if (co0 + BM <= a.Cout)
        emit(TrueTag{});
    else
        emit(FalseTag{});
}

template <int BM, int BN, int WM, int WN, bool SUBPIX, int NPL = 3>
__global__ void __launch_bounds__(256, 2) conv3x3_wgrad_tap_h_kernel(WgradTapArgs a) {
    int bx, by;
    xcd_tile(a.xcd, bx, by);
    wgrad_tap_body_h<BM, BN, WM, WN, SUBPIX, NPL>(a, bx, by, (int)blockIdx.z);
}

template <int BM, int BN, int WM, int WN, int MODE>
__global__ void __launch_bounds__(256, 3) conv3x3_wgrad_tap_kernel(WgradTapArgs a) {
    int bx, by;
    xcd_tile(a.xcd, bx, by);
    wgrad_tap_body<BM, BN, WM, WN, MODE>(a, bx, by, (int)blockIdx.z);
}

// ---- the same GEMM for MANY layers in one launch ("grouped"): a block looks up its job (layer, source), its tile and
// its pixel chunk.  A backward pass has ~50 tap-major weight-gradient GEMMs of 27..650 tiles each; launched one by one,
// every layer has to be cut into 2..86 pixel splits to fill 256 CUs, and the split partials (1.3 GB per iteration on
// BASELINE configs[1]) are written by the GEMMs and read again by the reductions.  Launched together the tiles of all
// layers fill the chip, so a layer is only split where its pixel range is long (chunks of ~1024 pixels): 0.2 GB.
struct TapJobRec {
    WgradTapArgs a;
    int gm, gnt, splits, block_begin;     // tile grid (gnt = ci tiles x taps), pixel splits; blocks = gm * gnt * splits
};

template <int BM, int BN, int WM, int WN, int MODE>
__global__ void __launch_bounds__(256, 3) conv3x3_wgrad_tap_grouped_kernel(const TapJobRec* __restrict__ recs, int n) {
    __shared__ int sh_idx;
    // XCD-aware order (see xcd_tile): workgroup L runs on XCD L % 8; XCD class c takes the contiguous range
    // [c * per, (c + 1) * per) of the logical block order, in which the blocks that share a pixel chunk of a layer
    // (all its co / ci tiles and taps) are neighbours -- so a chunk's activations are fetched into one L2, not eight
    int b = blockIdx.x;
    {
        const unsigned total = gridDim.x, L = blockIdx.x, c = L & 7u, base = total >> 3, rem = total & 7u;
        if (total >= 64) b = (int)(c * base + (c < rem ? c : rem) + (L >> 3));
    }
    const int di = find_desc(&recs[0].block_begin, (int)(sizeof(TapJobRec) / sizeof(int)), n, b, &sh_idx);
    // the record is wave-uniform: keep it in scalar registers (copied field by field through readfirstlane by the compiler
    // when it can prove uniformity; `di` comes from LDS, so say it explicitly)
    const TapJobRec* __restrict__ rp = recs + __builtin_amdgcn_readfirstlane(di);
    const WgradTapArgs a = rp->a;
    const int local = b - rp->block_begin;
    const int gm = rp->gm, gnt = rp->gnt;
    const int bx = local % gm, rest = local / gm;
    const int by = rest % gnt, split = rest / gnt;
    wgrad_tap_body<BM, BN, WM, WN, MODE>(a, bx, by, split);
}

template <int BM, int BN, int WM, int WN, bool SUBPIX, int NPL = 3>
__global__ void __launch_bounds__(256, 2) conv3x3_wgrad_tap_grouped_h_kernel(const TapJobRec* __restrict__ recs, int n) {
    __shared__ int sh_idx;
    int b = blockIdx.x;
    {
        const unsigned total = gridDim.x, L = blockIdx.x, c = L & 7u, base = total >> 3, rem = total & 7u;
        if (total >= 64) b = (int)(c * base + (c < rem ? c : rem) + (L >> 3));
    }
    const int di = find_desc(&recs[0].block_begin, (int)(sizeof(TapJobRec) / sizeof(int)), n, b, &sh_idx);
    const TapJobRec* __restrict__ rp = recs + __builtin_amdgcn_readfirstlane(di);
    const WgradTapArgs a = rp->a;
    const int local = b - rp->block_begin;
    const int gm = rp->gm, gnt = rp->gnt;
    const int bx = local % gm, rest = local / gm;
    const int by = rest % gnt, split = rest / gnt;
    wgrad_tap_body_h<BM, BN, WM, WN, SUBPIX, NPL>(a, bx, by, split);
}

// the nine-tap 16x16 kernel for MANY narrow layers in one launch (the eight 45 -> 45 convolutions of the refinement stack:
// launched one by one each needs 512 pixel splits to fill the chip -- 37 MB of partials per layer; together 128 do)
struct N16JobRec {      // same size and block_begin offset as TapJobRec (one table, one lookup)
    WgradN16Args a;
    char pad[sizeof(WgradTapArgs) - sizeof(WgradN16Args)];
    int gm, gn, splits, block_begin;
};
static_assert(sizeof(N16JobRec) == sizeof(TapJobRec), "grouped job records share one table");

template <int NCT, int NCI>
__global__ void __launch_bounds__(256, 2) conv3x3_wgrad_n16_grouped_kernel(const N16JobRec* __restrict__ recs, int n) {
    __shared__ int sh_idx;
    const int b = blockIdx.x;
    const int di = find_desc(&recs[0].block_begin, (int)(sizeof(N16JobRec) / sizeof(int)), n, b, &sh_idx);
    const N16JobRec* __restrict__ rp = recs + __builtin_amdgcn_readfirstlane(di);
    const WgradN16Args a = rp->a;
    const int local = b - rp->block_begin;
    const int gm = rp->gm, gn = rp->gn;
    const int bx = local % gm, rest = local / gm;
    wgrad_n16_body<NCT, NCI>(a, bx, rest % gn, rest / gn);
}

// dw[co][(c_start + ci) * ntaps + tap] = sum_s part[s][tap][co][ci]: one block per (64-channel ci tile, co row);
// reads are coalesced along ci with four independent split-sum chains per element (loads in flight), the
// (tap, ci) -> (ci, tap) transposition goes through LDS, writes are contiguous runs of 64 * ntaps floats.
// Fixed summation order (deterministic).
// (up_fold / up_fold_pairs: pack_tile.h -- the optimiser kernel folds tap-major partials too)
__global__ void __launch_bounds__(256) conv3x3_wgrad_tap_reduce_kernel(const float* __restrict__ part, int splits,
                                                                       int ntaps, int Cout, int C,
                                                                       float* __restrict__ dw, long ld_out, int up) {
    // up: `ntaps` = 16 pseudo taps of the sub-pixel form in `part`, folded into the 9 kernel taps of dw; up == 2: of a 1 x 1 source
    // (WgradSel::dead1x1) -- the slices of the dead pseudo taps were never written: +0.f without a load, the same fold
    __shared__ float tile[16][65];
    const int t = threadIdx.x;
    const int ci0 = blockIdx.x * 64, co = blockIdx.y;
    const long plane = (long)Cout * C, sstride = (long)ntaps * plane;
    const int c = t & 63;
    const bool c_ok = ci0 + c < C;
    for (int tp = t >> 6; tp < ntaps; tp += 4) {
        if (up == 2 && !up1x1_live(tp)) {
            tile[tp][c] = 0.f;
            continue;
        }
        const float* src = c_ok ? part + (long)tp * plane + (long)co * C + ci0 + c : part;   // always loadable
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        int sp = 0;
        for (; sp + 3 < splits; sp += 4) {
            const float x0 = src[(long)sp * sstride], x1 = src[(long)(sp + 1) * sstride];
            const float x2 = src[(long)(sp + 2) * sstride], x3 = src[(long)(sp + 3) * sstride];
            v0 += x0;
            v1 += x1;
            v2 += x2;
            v3 += x3;
        }
        for (; sp < splits; ++sp) v0 += src[(long)sp * sstride];
        tile[tp][c] = c_ok ? (v0 + v1) + (v2 + v3) : 0.f;
    }
    __syncthreads();
    const int nout = up ? 9 : ntaps;
    float* dst = dw + (long)co * ld_out + (long)ci0 * nout;
    const int lim = (C - ci0 < 64 ? C - ci0 : 64) * nout;
    for (int idx = t; idx < lim; idx += 256) {
        const int cc = idx / nout, tp = idx - cc * nout;
        dst[idx] = up ? up_fold(&tile[0][cc], tp / 3, tp % 3, 65) : tile[tp][cc];
    }
}

// first stage for many-split layers (large pixel counts, small dW): out[z][i] = sum of the splits of group z, so the
// summation runs over (elements x groups) threads instead of elements only; the transposing kernel above then sums
// the groups.  Fixed order inside a group and over the groups (deterministic).
__global__ void __launch_bounds__(256) conv3x3_wgrad_group_sum_kernel(const float* __restrict__ part, long n, int splits,
                                                                      int per_group, float* __restrict__ out,
                                                                      long dead_plane) {
    // dead_plane != 0: [16 pseudo taps][dead_plane] partials of a 1 x 1 source (WgradSel::dead1x1) -- the dead taps' slices hold
    // nothing: neither read nor summed here (the reduction behind this stage does not read their group sums either)
    const int z = blockIdx.y;
    const int s0 = z * per_group;
    int s1 = s0 + per_group;
    if (s1 > splits) s1 = splits;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (dead_plane && !up1x1_live((int)(i / dead_plane))) continue;
        const float* src = part + i;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        int sp = s0;
        for (; sp + 3 < s1; sp += 4) {
            const float x0 = src[(long)sp * n], x1 = src[(long)(sp + 1) * n];
            const float x2 = src[(long)(sp + 2) * n], x3 = src[(long)(sp + 3) * n];
            v0 += x0;
            v1 += x1;
            v2 += x2;
            v3 += x3;
        }
        for (; sp < s1; ++sp) v0 += src[(long)sp * n];
        out[(long)z * n + i] = (v0 + v1) + (v2 + v3);
    }
}

// dw[co][c_start*9 + n] = sum_splits partial[s][co][n]
__global__ void __launch_bounds__(256) conv3x3_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int Cout,
                                                                   int NT, float* __restrict__ dw, long ld_out) {
    __shared__ float sm[4][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long total = (long)Cout * NT;
    for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {
        const long i = base + o;
        float v = 0.f;
        if (i < total)
            for (int s = g; s < splits; s += 4) v += ws[(long)s * total + i];
        sm[g][o] = v;
        __syncthreads();
        if (g == 0 && i < total) {
            const int n = (int)(i % NT);
            const int co = (int)(i / NT);
            dw[(long)co * ld_out + n] = (sm[0][o] + sm[1][o]) + (sm[2][o] + sm[3][o]);
        }
        __syncthreads();
    }
}

// ---- split reductions of MANY layers in one launch (deferred weight-gradient reductions of a whole backward pass) ----
// Block b belongs to the layer whose [block_begin, block_begin + blocks) range contains it -- found with ONE coalesced
// read of the table's block_begin column and an LDS count (a binary search over device memory costs ~6 dependent loads per
// block, several microseconds on blocks that move 5 KB) -- and owns a tw-channel ci tile of one output row (or of four
// rows): thread group g sums the splits g, g + groups, ... with 2 * ntaps independent loads in flight, the groups are
// combined through LDS in a fixed order (deterministic), and the (tap, ci) -> (ci, tap) transposition of the tap-major
// partials happens on the way into LDS.  blocks = ceil(Cout / rows) * ceil(C / tw) with (tw, rows) = reduce_map(splits).
// That is the TILE map: a lane loads one float per (split, tap).  It fixes the sum of a gradient element; with
// "wgrad_reduce_vec" = 1 (the default) the layers whose partials are cut into 16-byte quads take a vector map with the same
// sums and float4 loads (reduce_map_id, reduce_vec_tap, reduce_param_major_vec below), which never needs more blocks than
// the tile map -- surplus blocks return at once, and a table built under either value of the tuning value is valid under both.
// thread map of one layer: channel-tile width tw and thread groups = 256 / tw
//   splits <  4 : tw = 64, the 4 groups own 4 different output rows (each sums all its splits);
//   splits < 32 : tw = 64, the 4 groups share one row and split the splits;
//   splits >= 32: tw = 16, 16 groups share one row (the many-split layers have tiny gradients: without this a 512-split
//                 layer leaves ten blocks summing 128 partials in sequence -- the tail of the whole launch).
__host__ __device__ __forceinline__ void reduce_map(int splits, int* tw, int* rows) {
    *tw = splits >= 32 ? 16 : 64;
    *rows = splits < 4 ? 4 : 1;
}

// Few-split layers with C % 4 == 0 -- the deep levels (2x2 ... 8x8 maps, 256 ... 2048 channels), whose "partials" ARE the
// gradient (240 of the 265 MB of BASELINE configs[1]) in tap-major order -- take a flat map instead: a thread owns four
// consecutive input channels of one output row, reads one float4 per tap and split (1 KB contiguous per 64 lanes; the tile
// map above reads 256-byte pieces: ~1.8 TB/s measured in round 3, before the vector maps below existed) and writes its 4 * ntaps consecutive gradient floats from registers:
// no LDS, no barrier.  blocks = ceil(Cout * C / 4 / 256).
__host__ __device__ __forceinline__ bool reduce_flat(int splits, int C) { return splits < 4 && (C & 3) == 0; }

// the pseudo taps of a layout-2 descriptor whose slices hold partials: all 16, or the live four of a 1 x 1 source
// (MNK_REDUCE_UP1X1: the others were never written; every map takes them as +0.f and performs the same additions)
__device__ __forceinline__ unsigned reduce_live_taps(const MnkWgradReduceDesc& d) {
    return (d.layout == 2 && (d.flags & MNK_REDUCE_UP1X1)) ? up1x1_live_mask(false) : 0xffffu;
}

// out[e * NT + tp] = v[tp].e for the four channels e of a thread: the (tap, ci) -> (ci, tap) transposition in registers
template <int NT>
__device__ __forceinline__ void flat_store(const float4* v, float* __restrict__ dst, bool accumulate) {
    float o[4 * NT];
#pragma unroll
    for (int tp = 0; tp < NT; ++tp) {
        o[0 * NT + tp] = v[tp].x;
        o[1 * NT + tp] = v[tp].y;
        o[2 * NT + tp] = v[tp].z;
        o[3 * NT + tp] = v[tp].w;
    }
    if (((size_t)dst & 15) == 0) {
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            float4 w = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            if (accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(dst + 4 * k);
                w = make_float4(old.x + w.x, old.y + w.y, old.z + w.z, old.w + w.w);
            }
            *reinterpret_cast<float4*>(dst + 4 * k) = w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * NT; ++k) dst[k] = accumulate ? dst[k] + o[k] : o[k];
    }
}

template <int NIN, int NOUT, int LAYOUT, bool UP1X1 = false>      // taps read / written; LAYOUT 0 tap-major, 2 tap-major sub-pixel (16 -> 9), 1 parameter-major
__device__ __forceinline__ void reduce_flat_body(const MnkWgradReduceDesc& d, int co, int ci) {
    float4 acc[NIN];
#pragma unroll
    for (int tp = 0; tp < NIN; ++tp) acc[tp] = make_float4(0.f, 0.f, 0.f, 0.f);
    float* dst = d.dw + ((long)co * d.Cin_total + d.c_start + ci) * NOUT;
    if (LAYOUT == 1) {
        // part[s][co][ci * NOUT + tap]: the thread's 4 * NOUT floats are contiguous and already in gradient order
        const long NT = (long)d.C * NOUT, sstride = (long)d.Cout * NT;
        const float* src = d.part + (long)co * NT + (long)ci * NOUT;
        for (int sp = 0; sp < d.splits; ++sp) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                const float4 v = *reinterpret_cast<const float4*>(src + (long)sp * sstride + 4 * k);
                acc[k] = make_float4(acc[k].x + v.x, acc[k].y + v.y, acc[k].z + v.z, acc[k].w + v.w);
            }
        }
        if (((size_t)dst & 15) == 0) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                float4 w = acc[k];
                if (d.accumulate) {
                    const float4 old = *reinterpret_cast<const float4*>(dst + 4 * k);
                    w = make_float4(old.x + w.x, old.y + w.y, old.z + w.z, old.w + w.w);
                }
                *reinterpret_cast<float4*>(dst + 4 * k) = w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                const float e[4] = {acc[k].x, acc[k].y, acc[k].z, acc[k].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[4 * k + j] = d.accumulate ? dst[4 * k + j] + e[j] : e[j];
            }
        }
        return;
    }
    const long plane = (long)d.Cout * d.C, sstride = (long)NIN * plane;
    const float* src = d.part + (long)co * d.C + ci;
    for (int sp = 0; sp < d.splits; ++sp) {                      // NIN independent 16-byte loads in flight per split
#pragma unroll
        for (int tp = 0; tp < NIN; ++tp) {
            // UP1X1 (MNK_REDUCE_UP1X1): a dead pseudo tap's slice was never written -- its sum stays the +0.f it would be, no load
            if (UP1X1 && !up1x1_live(tp)) continue;
            const float4 v = *reinterpret_cast<const float4*>(src + (long)sp * sstride + (long)tp * plane);
            acc[tp] = make_float4(acc[tp].x + v.x, acc[tp].y + v.y, acc[tp].z + v.z, acc[tp].w + v.w);
        }
    }
    if (LAYOUT == 2) {                                           // fold the 16 pseudo taps into the nine kernel taps, per channel
        float ax[16], ay[16], az[16], aw[16];
#pragma unroll
        for (int tp = 0; tp < 16; ++tp) ax[tp] = acc[tp].x, ay[tp] = acc[tp].y, az[tp] = acc[tp].z, aw[tp] = acc[tp].w;
        float4 f[9];
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
            f[tp] = make_float4(up_fold(ax, tp / 3, tp % 3, 1), up_fold(ay, tp / 3, tp % 3, 1), up_fold(az, tp / 3, tp % 3, 1),
                                up_fold(aw, tp / 3, tp % 3, 1));
        flat_store<9>(f, dst, d.accumulate != 0);
    } else {
        flat_store<NOUT>(acc, dst, d.accumulate != 0);
    }
}

// parameter-major partials part[s][co][ci * ntaps + tap]: this thread's elements src[0], src[TW], ... (those below `left`)
// summed over the splits s0, s0 + sstep, ... into out[0], out[TW], ...; TW is a compile-time constant so that the eight
// elements of a pass share one address register pair (immediate offsets)
template <int TW>
__device__ __forceinline__ void reduce_param_major(const float* __restrict__ src, long sstride, int splits, int s0, int sstep,
                                                   int left, bool row_ok, float* __restrict__ out) {
    const int nk = (left + TW - 1) / TW;                         // elements of this thread (<= 0: none)
    for (int k0 = 0; k0 < nk; k0 += 8) {                         // eight elements x two splits in flight
        float a0[8], a1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a0[k] = a1[k] = 0.f;
        const float* sk = src + k0 * TW;
        int sp = s0;
        for (; sp + sstep < splits; sp += 2 * sstep) {
            const float* ps = sk + (long)sp * sstride;
            const float* pt = ps + (long)sstep * sstride;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k0 + k < nk) {
                    a0[k] += ps[k * TW];
                    a1[k] += pt[k * TW];
                }
        }
        if (sp < splits) {
            const float* ps = sk + (long)sp * sstride;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k0 + k < nk) a0[k] += ps[k * TW];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k0 + k < nk) out[(k0 + k) * TW] = row_ok ? a0[k] + a1[k] : 0.f;
    }
}

// ---- vector thread maps ("wgrad_reduce_vec" = 1): the same sums, every global load a float4 -----------------------------------
// The sum of one gradient element is what the maps above fix: G = 1 / 4 / 16 thread groups (splits < 4 / < 32 / >= 32), group g
// owns the splits g, g + G, ... and adds them in two chains (its 1st, 3rd, ... and its 2nd, 4th, ... split, each in increasing
// order from 0.f), the group's value is chain 0 + chain 1 (layout 2: up_fold of the group's 16 pseudo-tap values), the groups
// are added in order from 0.f (one group: taken as it is), `accumulate` adds dw last.  Only which lane loads what changes, so
// the results are the tile map's to the bit (tests/test_kernels_wgrad_reduce_vec.py).
enum { REDUCE_MAP_FLAT = 0, REDUCE_MAP_TILE = 1, REDUCE_MAP_VEC_TAP = 2, REDUCE_MAP_VEC_PARAM = 3 };
static int g_wgrad_reduce_vec = tuning_knob("wgrad_reduce_vec", &g_wgrad_reduce_vec, 1);      // 0: the flat and tile maps only

// which map a descriptor takes.  Contract: `part` is 16-byte aligned (mnk/optim.py's partial buffers are whole allocations);
// the kernel checks, and a layer whose partials are not keeps the tile map -- same bits, none of the speed, and
// mnk_wgrad_reduce_map, which sees no pointer, still names the vector map (tests/test_kernels_wgrad_reduce_vec.py runs one).
// On the 4- and 16-group maps a block covers four times the tile map's floats, so three quarters of such a layer's blocks
// (mnk_wgrad_reduce_blocks cannot know the layout) find their descriptor and return.
//   tap-major, (Cout * C) % 4 == 0, 3x3 / 4x4 taps: the [co][ci] plane of a (split, tap) is cut into quads regardless of rows
//   parameter-major, (C * ntaps) % 4 == 0: the tile map's tiles, read as quads along the gradient-ordered axis
// (the 45 -> 45 layers' planes of 2025 floats stay on the tile map)
__host__ __device__ __forceinline__ int reduce_map_id(int vec, int layout, int splits, int ntaps, int Cout, int C) {
    if (reduce_flat(splits, C) && (ntaps == 9 || ntaps == 16)) return REDUCE_MAP_FLAT;
    if (!vec) return REDUCE_MAP_TILE;
    if (layout == 1) return (((long)C * ntaps) & 3) == 0 ? REDUCE_MAP_VEC_PARAM : REDUCE_MAP_TILE;
    const long plane = (long)Cout * C;
    // (measured per class, profiles/wgrad_reduce_vec_ab.txt: the sub-pixel form with 4 ... 31 splits is the one class that is
    // slower on the vector map -- five of its six flagship layers, 5.5 ... 7.7 -> 8.1 ... 9.7 us alone -- and keeps the tile map)
    const bool taps_ok = layout == 2 ? (ntaps == 9 && (splits < 4 || splits >= 32)) : (layout == 0 && (ntaps == 9 || ntaps == 16));
    const int G = splits < 4 ? 1 : (splits < 32 ? 4 : 16), nin = layout == 2 ? 16 : ntaps;
    // (a lane's share of an address -- its group's first split and its quad -- is a 32-bit byte offset: reduce_vec_tap)
    return (taps_ok && (plane & 3) == 0 && ((long)(G - 1) * nin + 1) * plane < (1L << 30)) ? REDUCE_MAP_VEC_TAP : REDUCE_MAP_TILE;
}

__device__ __forceinline__ void add4(float4& a, const float4& x) { a = make_float4(a.x + x.x, a.y + x.y, a.z + x.z, a.w + x.w); }

// r[i] = chain 0 + chain 1 of the float4 at tap i over the group's splits g, g + G, ...: the k-th of them is read at
// ub + k * gstep + i * plane (block-uniform: scalar registers) + voff bytes (the lane's part, g * sstride + its quad: ONE vector
// register -- a 64-bit lane pointer per (split, tap) in flight made the kernel spill).  U = 2: four splits' loads are issued
// before the first add of a trip (the adds of a chain stay in split order)
__device__ __forceinline__ float4 vec_ld(const float* __restrict__ u, unsigned voff) {
#ifdef HIPEMU
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(u) + voff);
#else
    // partials are global memory, but a pointer read from the table is generic to the compiler (flat_load, a vector pointer
    // pair per address): say so, and the load takes its base from scalar registers
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) char* gchar;
    const f4v v = *reinterpret_cast<const __attribute__((address_space(1))) f4v*>((gchar)(const char*)u + voff);
    return make_float4(v.x, v.y, v.z, v.w);
#endif
}
template <int TP, int U>
__device__ __forceinline__ void vec_chain_pass(const float* __restrict__ ub, unsigned voff, long gstep, long plane, int splits,
                                               int g, int G, float4* r) {
    float4 a0[TP], a1[TP];
#pragma unroll
    for (int i = 0; i < TP; ++i) a0[i] = a1[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    if (U == 2) {
        for (; g + (k + 3) * G < splits; k += 4) {
            const float* p0 = ub + (long)k * gstep;
            const float* p1 = p0 + gstep;
            const float* p2 = p1 + gstep;
            const float* p3 = p2 + gstep;
            float4 x0[TP], x1[TP], x2[TP], x3[TP];
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                x0[i] = vec_ld(p0 + (long)i * plane, voff);
                x1[i] = vec_ld(p1 + (long)i * plane, voff);
                x2[i] = vec_ld(p2 + (long)i * plane, voff);
                x3[i] = vec_ld(p3 + (long)i * plane, voff);
            }
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                add4(a0[i], x0[i]);
                add4(a1[i], x1[i]);
                add4(a0[i], x2[i]);
                add4(a1[i], x3[i]);
            }
        }
    }
    for (; g + (k + 1) * G < splits; k += 2) {
        const float* p0 = ub + (long)k * gstep;
        const float* p1 = p0 + gstep;
        float4 x0[TP], x1[TP];
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            x0[i] = vec_ld(p0 + (long)i * plane, voff);
            x1[i] = vec_ld(p1 + (long)i * plane, voff);
        }
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            add4(a0[i], x0[i]);
            add4(a1[i], x1[i]);
        }
    }
    if (g + k * G < splits) {
        const float* p0 = ub + (long)k * gstep;
#pragma unroll
        for (int i = 0; i < TP; ++i) add4(a0[i], vec_ld(p0 + (long)i * plane, voff));
    }
#pragma unroll
    for (int i = 0; i < TP; ++i) r[i] = make_float4(a0[i].x + a1[i].x, a0[i].y + a1[i].y, a0[i].z + a1[i].z, a0[i].w + a1[i].w);
}

// LDS of the vector tap-major map: [group][quad][4 elements][NB taps], quad stride 4 * NB + 1 (odd: the lanes of a group write
// different banks); groups * quads per group = 256, so 256 * 37 floats with NB = 9
#define REDUCE_VEC_QS(NB) (4 * (NB) + 1)
#define REDUCE_SM_FLOATS (256 * REDUCE_VEC_QS(9))

template <int NB>
__device__ __forceinline__ void vec_put(float* __restrict__ smq, int j, const float4& v) {
    smq[0 * NB + j] = v.x;
    smq[1 * NB + j] = v.y;
    smq[2 * NB + j] = v.z;
    smq[3 * NB + j] = v.w;
}

// the block's 4 * qw plane elements x NB taps (gradient taps tb0 ...): groups added in order, stored as runs of NB floats per
// element -- consecutive threads write consecutive floats of a dw row whatever the slice's alignment
template <int NB>
__device__ __forceinline__ void vec_sum_groups_store(const MnkWgradReduceDesc& d, const float* __restrict__ sm, int groups, int qw,
                                                     unsigned p0, unsigned plane, int tb0) {
    constexpr int QS = REDUCE_VEC_QS(NB);
    const int n_out = qw * 4 * NB, gstride = qw * QS;
    for (int idx = threadIdx.x; idx < n_out; idx += 256) {
        const int q = idx / (4 * NB), r = idx - q * (4 * NB), k = r / NB, j = r - k * NB;
        const unsigned p = p0 + 4 * q + k;
        if (p >= plane) break;                                   // (p does not decrease with idx)
        const unsigned co = p / (unsigned)d.C, ci = p - co * (unsigned)d.C;
        const float* s = sm + q * QS + r;
        float v;
        if (groups == 1) {
            v = s[0];
        } else {
            v = 0.f;
            for (int gg = 0; gg < groups; ++gg) v += s[gg * gstride];       // fixed order: deterministic
        }
        float* dst = d.dw + ((long)co * d.Cin_total + d.c_start + ci) * d.ntaps + tb0 + j;
        *dst = d.accumulate ? *dst + v : v;
    }
}

// tap-major partials part[s][tap][co][ci] (layout 2: 16 pseudo taps) on the vector map: block `local` owns the 1024 / G plane
// floats from local * 1024 / G on, a lane one quad of them for its group's splits.  The taps go in passes of three or four (16
// taps x two chains x float4 do not fit in 128 registers; different taps are different bytes, nothing is read twice); the
// sub-pixel form's pass is one phase (pseudo taps 4 * phase ...), folded into the nine kernel taps as up_fold does: phase by
// phase from 0.f.
__device__ __forceinline__ void reduce_vec_tap(const MnkWgradReduceDesc& d, int local, float* __restrict__ sm) {
    const int groups = d.splits < 4 ? 1 : (d.splits < 32 ? 4 : 16), qw = 256 / groups;
    const unsigned plane = (unsigned)d.Cout * (unsigned)d.C;
    const unsigned p0 = (unsigned)local * (unsigned)(4 * qw);
    if (p0 >= plane) return;                                     // a surplus block (block-uniform: no barrier is missed)
    const int t = threadIdx.x, g = t / qw, q = t - g * qw;
    const bool ok = p0 + 4 * q < plane;
    const int nin = d.layout == 2 ? 16 : d.ntaps;
    const long sstride = (long)nin * plane;
    const float* src = d.part + p0;                              // block-uniform
    // the lane's part of every address, in bytes (< 2^32: reduce_map_id; lanes past the plane read the block's first quad)
    const unsigned voff = (unsigned)(((long)g * sstride + (ok ? 4 * q : 0)) * 4);
    const long gstep = (long)groups * sstride;
    if (d.layout == 2) {
        float4 f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
        for (int ph = 0; ph < 4; ++ph) {                        // (not unrolled: four copies of the split loop spill)
            float4 r[4];
            vec_chain_pass<4, 1>(src + (long)(4 * ph) * plane, voff, gstep, plane, d.splits, g, groups, r);
            // up_fold_pairs: phase (a, b) = (ph >> 1, ph & 1) gives kernel row 0 its pseudo taps u = 0, row 2 u = 1, row 1
            // u = 1 if a == 0 else 0; columns likewise with b and v.  Pseudo tap (u, v) is r[2 * u + v].
            const bool a0 = (ph >> 1) == 0, b0 = (ph & 1) == 0;
            const float4 m0 = a0 ? r[2] : r[0], m1 = a0 ? r[3] : r[1];
            const float4 row[3][2] = {{r[0], r[1]}, {m0, m1}, {r[2], r[3]}};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                add4(f[ky * 3 + 0], row[ky][0]);
                add4(f[ky * 3 + 1], b0 ? row[ky][1] : row[ky][0]);
                add4(f[ky * 3 + 2], row[ky][1]);
            }
        }
        float* smq = sm + (g * qw + q) * REDUCE_VEC_QS(9);
#pragma unroll
        for (int i = 0; i < 9; ++i) vec_put<9>(smq, i, f[i]);
        __syncthreads();
        vec_sum_groups_store<9>(d, sm, groups, qw, p0, plane, 0);
    } else if (d.ntaps == 9) {
        float* smq = sm + (g * qw + q) * REDUCE_VEC_QS(9);
#pragma unroll
        for (int ps = 0; ps < 3; ++ps) {
            float4 r[3];
            vec_chain_pass<3, 2>(src + (long)(3 * ps) * plane, voff, gstep, plane, d.splits, g, groups, r);
#pragma unroll
            for (int i = 0; i < 3; ++i) vec_put<9>(smq, 3 * ps + i, r[i]);
        }
        __syncthreads();
        vec_sum_groups_store<9>(d, sm, groups, qw, p0, plane, 0);
    } else {                                                     // 16 taps: two batches of eight (the LDS holds nine per element)
        float* smq = sm + (g * qw + q) * REDUCE_VEC_QS(8);
        for (int tb = 0; tb < 16; tb += 8) {
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                float4 r[4];
                vec_chain_pass<4, 1>(src + (long)(tb + 4 * ps) * plane, voff, gstep, plane, d.splits, g, groups, r);
#pragma unroll
                for (int i = 0; i < 4; ++i) vec_put<8>(smq, 4 * ps + i, r[i]);
            }
            __syncthreads();
            vec_sum_groups_store<8>(d, sm, groups, qw, p0, plane, tb);
            __syncthreads();
        }
    }
}

// parameter-major partials on the vector map: the tile map's tile (lim = cw * ntaps contiguous floats, a multiple of four that
// starts on a quad), this thread's quads c, c + TW, ... (those below `nq`) summed over the splits s0, s0 + sstep, ... into
// out[4 * c ...], out[4 * (c + TW) ...]: per element the sums of reduce_param_major
template <int TW>
__device__ __forceinline__ void reduce_param_major_vec(const float* __restrict__ src, long sstride, int splits, int s0, int sstep,
                                                       int nq, bool row_ok, float* __restrict__ out) {
    const int nk = (nq + TW - 1) / TW;                           // quads of this thread (<= 0: none)
    for (int k0 = 0; k0 < nk; k0 += 4) {                         // four quads x two splits in flight
        float4 a0[4], a1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a0[k] = a1[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* sk = src + (long)k0 * TW * 4;
        int sp = s0;
        for (; sp + sstep < splits; sp += 2 * sstep) {
            const float* ps = sk + (long)sp * sstride;
            const float* pt = ps + (long)sstep * sstride;
            float4 x0[4], x1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < nk) {
                    x0[k] = *reinterpret_cast<const float4*>(ps + k * TW * 4);
                    x1[k] = *reinterpret_cast<const float4*>(pt + k * TW * 4);
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < nk) {
                    add4(a0[k], x0[k]);
                    add4(a1[k], x1[k]);
                }
        }
        if (sp < splits) {
            const float* ps = sk + (long)sp * sstride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < nk) add4(a0[k], *reinterpret_cast<const float4*>(ps + k * TW * 4));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k0 + k < nk)
                *reinterpret_cast<float4*>(out + (long)(k0 + k) * TW * 4) =
                    row_ok ? make_float4(a0[k].x + a1[k].x, a0[k].y + a1[k].y, a0[k].z + a1[k].z, a0[k].w + a1[k].w)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// (four waves per SIMD.  The parent of the vector maps needed 132 registers unconstrained, i.e. three waves; capped at 128 it
// reduced the generator's 692 MB of partials in 311 instead of 361 us, and five waves -- 96 registers -- spilled: 765 us.  With
// the vector maps: 128 registers, no scratch, 37892 bytes of LDS -- four blocks are 151.6 of a CU's 160 KB, so REDUCE_SM_FLOATS
// has no room to grow: 2 KB more per block and only three blocks are resident -- and the same 692 MB in 219 us, the
// discriminator's 179 MB in 40 instead of 91 us.  tools/reduce_probe.py, tools/isa_report.py, profiles/wgrad_reduce_vec_ab.txt)
__global__ void __launch_bounds__(256, 4) wgrad_reduce_multi_kernel(const MnkWgradReduceDesc* __restrict__ descs, int n, int vec) {
    // tile map: [group][channel * ntaps + tap], group stride tw * 16 (16 * 16 * 16 + 64 floats); vector map: reduce_vec_tap
    __shared__ __attribute__((aligned(16))) float sm[REDUCE_SM_FLOATS];
    __shared__ int sh_idx;
    const int b = blockIdx.x;
    const int di = find_desc(&descs[0].block_begin, (int)(sizeof(MnkWgradReduceDesc) / sizeof(int)), n, b, &sh_idx);
    // (the descriptor is block-uniform: scalar registers -- as vector registers its 14 words made the vector maps spill)
    const MnkWgradReduceDesc d = descs[__builtin_amdgcn_readfirstlane(di)];
    const int local = b - d.block_begin;
    if (reduce_flat(d.splits, d.C) && (d.ntaps == 9 || d.ntaps == 16)) {      // (block-uniform: no barrier follows on this path)
        const int q4 = d.C >> 2;
        const long item = (long)local * 256 + threadIdx.x;
        if (item >= (long)d.Cout * q4) return;
        const int co = (int)(item / q4), ci = 4 * (int)(item - (long)co * q4);
        if (d.layout == 2 && reduce_live_taps(d) != 0xffffu)
            reduce_flat_body<16, 9, 2, true>(d, co, ci);
        else if (d.layout == 2)
            reduce_flat_body<16, 9, 2>(d, co, ci);
        else if (d.layout == 0 && d.ntaps == 9)
            reduce_flat_body<9, 9, 0>(d, co, ci);
        else if (d.layout == 0)
            reduce_flat_body<16, 16, 0>(d, co, ci);
        else if (d.ntaps == 9)
            reduce_flat_body<9, 9, 1>(d, co, ci);
        else
            reduce_flat_body<16, 16, 1>(d, co, ci);
        return;
    }
    // (block-uniform; unaligned partials -- no caller of this library has them -- keep the tile map; so do the partials of a
    // 1 x 1 source, MNK_REDUCE_UP1X1: only the flat and the tile map know the slices that hold nothing -- a few frames' worth of
    // partials per layer, and the same bits on every map)
    const int map = ((size_t)d.part & 15) == 0 && reduce_live_taps(d) == 0xffffu
                        ? reduce_map_id(vec, d.layout, d.splits, d.ntaps, d.Cout, d.C) : REDUCE_MAP_TILE;
    if (map == REDUCE_MAP_VEC_TAP) {
        reduce_vec_tap(d, local, sm);
        return;
    }
    int tw, rpb;
    reduce_map(d.splits, &tw, &rpb);
    const int groups = 256 / tw, gstride = tw * 16;
    const int ctiles = (d.C + tw - 1) / tw;
    const int rq = local / ctiles, ci0 = (local - rq * ctiles) * tw;
    const int t = threadIdx.x, g = t / tw, c = t - g * tw;
    const int ntaps = d.ntaps;
    const int cw = d.C - ci0 < tw ? d.C - ci0 : tw;          // channels of this tile
    const int lim = cw * ntaps;                              // gradient floats of this tile (per row)
    const int co = rpb == 1 ? rq : rq * 4 + g;               // the row this thread group reads
    const bool row_ok = co < d.Cout;
    const int s0 = rpb == 1 ? g : 0, sstep = rpb == 1 ? groups : 1;
    float* smg = sm + g * gstride;
    if (d.layout == 0 || d.layout == 2) {
        // part[s][tap][co][ci]; layout 2: 16 pseudo taps of the sub-pixel form, folded into the 9 kernel taps below
        const int nin = d.layout == 2 ? 16 : ntaps;
        const long plane = (long)d.Cout * d.C, sstride = (long)nin * plane;
        const bool ok = c < cw && row_ok;
        const float* src = d.part + (long)(row_ok ? co : 0) * d.C + ci0 + (ok ? c : 0);
        float acc[16], acc2[16];
#pragma unroll
        for (int tp = 0; tp < 16; ++tp) acc[tp] = acc2[tp] = 0.f;
        int sp = s0;
        if (reduce_live_taps(d) != 0xffffu) {
            // MNK_REDUCE_UP1X1 (block-uniform): the same two chains over the four live pseudo taps; a dead one's sums stay the +0.f
            // its slice would hold, and nothing of it is loaded
            for (; sp + sstep < d.splits; sp += 2 * sstep) {
                const float* ps = src + (long)sp * sstride;
                const float* pt = ps + (long)sstep * sstride;
#pragma unroll
                for (int ph = 0; ph < 4; ++ph) {
                    acc[up1x1_live_tap(ph)] += ps[(long)up1x1_live_tap(ph) * plane];
                    acc2[up1x1_live_tap(ph)] += pt[(long)up1x1_live_tap(ph) * plane];
                }
            }
            if (sp < d.splits) {
                const float* ps = src + (long)sp * sstride;
#pragma unroll
                for (int ph = 0; ph < 4; ++ph) acc[up1x1_live_tap(ph)] += ps[(long)up1x1_live_tap(ph) * plane];
            }
            sp = d.splits;
        }
        for (; sp + sstep < d.splits; sp += 2 * sstep) {       // two splits per trip: 2 * ntaps loads in flight
            const float* ps = src + (long)sp * sstride;
            const float* pt = ps + (long)sstep * sstride;
#pragma unroll
            for (int tp = 0; tp < 16; ++tp)
                if (tp < nin) {
                    acc[tp] += ps[(long)tp * plane];
                    acc2[tp] += pt[(long)tp * plane];
                }
        }
        if (sp < d.splits) {
            const float* ps = src + (long)sp * sstride;
#pragma unroll
            for (int tp = 0; tp < 16; ++tp)
                if (tp < nin) acc[tp] += ps[(long)tp * plane];
        }
#pragma unroll
        for (int tp = 0; tp < 16; ++tp) acc[tp] += acc2[tp];
        if (d.layout == 2) {
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) smg[c * 9 + tp] = ok ? up_fold(acc, tp / 3, tp % 3, 1) : 0.f;
        } else {
#pragma unroll
            for (int tp = 0; tp < 16; ++tp)
                if (tp < ntaps) smg[c * ntaps + tp] = ok ? acc[tp] : 0.f;      // already in (ci, tap) order
        }
    } else {
        // part[s][co][ci * ntaps + tap]
        const long NT = (long)d.C * ntaps, sstride = (long)d.Cout * NT;
        // a thread owns the elements c, c + tw, ... of the tile's lim = cw * ntaps contiguous floats (at most ntaps of them)
        // and walks the splits with eight of them in flight (one at a time meant two loads in flight and ntaps passes over
        // the splits: the 512-split 45 -> 45 layers' blocks were the tail of the launch)
        const float* src = d.part + (long)(row_ok ? co : 0) * NT + (long)ci0 * ntaps + c;
        if (map == REDUCE_MAP_VEC_PARAM) {
            if (tw == 16)
                reduce_param_major_vec<16>(src + 3 * c, sstride, d.splits, s0, sstep, (lim >> 2) - c, row_ok, smg + 4 * c);
            else
                reduce_param_major_vec<64>(src + 3 * c, sstride, d.splits, s0, sstep, (lim >> 2) - c, row_ok, smg + 4 * c);
        } else if (tw == 16)
            reduce_param_major<16>(src, sstride, d.splits, s0, sstep, lim - c, row_ok, smg + c);
        else
            reduce_param_major<64>(src, sstride, d.splits, s0, sstep, lim - c, row_ok, smg + c);
    }
    __syncthreads();
    if (rpb == 1) {
        float* dst = d.dw + ((long)rq * d.Cin_total + d.c_start + ci0) * ntaps;
        for (int idx = t; idx < lim; idx += 256) {
            float v = 0.f;
            for (int gg = 0; gg < groups; ++gg) v += sm[gg * gstride + idx];       // fixed order: deterministic
            dst[idx] = d.accumulate ? dst[idx] + v : v;
        }
    } else if (row_ok) {
        float* dst = d.dw + ((long)co * d.Cin_total + d.c_start + ci0) * ntaps;
        for (int idx = c; idx < lim; idx += tw) dst[idx] = d.accumulate ? dst[idx] + smg[idx] : smg[idx];
    }
}

// ---- launch plans (defaults from the MI355X sweeps in profiles/README.md; tuning_knob: settable by name through
// mnk_set_tuning / MNK_TUNING for tuning runs) --------------------------------------------------------------------------------
// (the weight-gradient splits are deterministic partials + a reduce kernel; an fp32-atomic form measured equal in round 1 and
// was removed in round 6 together with -munsafe-fp-atomics: no floating-point atomic exists in this library)
static int g_wsplit_tiles = tuning_knob("wsplit_tiles", &g_wsplit_tiles, 512), g_wsplit_target = tuning_knob("wsplit_target", &g_wsplit_target, 1024),
           g_wsplit_minsteps = tuning_knob("wsplit_minsteps", &g_wsplit_minsteps, 8);

// 1: the tap-major weight-gradient kernels on the bf16 matrix cores too (wgrad_tap_body_h: transposing loader)
static int g_wgrad_bf16x3 = tuning_knob("wgrad_bf16x3", &g_wgrad_bf16x3, 0);

struct WPlan {
    int bm, gm, gn, splits;
    long pix_per_split;
};

// LDS-halo wgrad plan
struct HPlan {
    bool use;
    int TR, TC, tiles_w, tiles_per_img, gm, gn, splits;
    long total_tiles, tiles_per_split;
};
static int g_wgrad_halo = tuning_knob("wgrad_halo", &g_wgrad_halo, 1), g_whalo_target = tuning_knob("whalo_target", &g_whalo_target, 768),
           g_whalo_mintiles = tuning_knob("whalo_mintiles", &g_whalo_mintiles, 8);

static HPlan make_hplan(int N, int H, int W, int Cout, int C) {
    HPlan p;
    // measured on the MI355X (profiles/README.md): the halo kernel wins when its 64x64 (co, ci) slab is reasonably
    // full; narrow layers (3 input channels, 10/13/32 output channels with ragged ci) stay on the gather kernel
    const double fill = ((double)C / round_up(C, 64)) * ((double)Cout / round_up(Cout, 64));
    p.use = g_wgrad_halo && W >= 16 && (W % 2) == 0 && H >= 2 && fill >= 0.45;
    if (!p.use) return p;
    p.TC = W < 64 ? W : 64;
    if (64 % p.TC != 0) {        // widths that do not divide the 64-pixel tile: keep the gather kernel
        p.use = false;
        return p;
    }
    p.TR = 64 / p.TC;
    p.tiles_w = ceil_div(W, p.TC);
    p.tiles_per_img = ceil_div(H, p.TR) * p.tiles_w;
    p.total_tiles = (long)N * p.tiles_per_img;
    p.gm = ceil_div(Cout, 64);
    p.gn = ceil_div(C, 64);
    long base = (long)p.gm * p.gn * 3;                             // x3: one block per tap row
    long splits = (g_whalo_target + base - 1) / base;
    if (splits > p.total_tiles / g_whalo_mintiles) splits = p.total_tiles / g_whalo_mintiles;   // tiles per block
    if (splits < 1) splits = 1;
    p.tiles_per_split = (p.total_tiles + splits - 1) / splits;
    p.splits = (int)((p.total_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
    return p;
}

static WPlan make_wplan(long M, int Cout, int C, int ntaps = 9) {
    WPlan p;
    p.bm = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
    p.gm = ceil_div(Cout, p.bm);
    p.gn = ceil_div(ntaps * C, 128);
    long tiles = (long)p.gm * p.gn;
    long steps = (M + BK - 1) / BK;
    long splits = 1;
    if (tiles < g_wsplit_tiles) {
        splits = (g_wsplit_target + tiles - 1) / tiles;
        long max_splits = steps / g_wsplit_minsteps;       // >= 128 pixels per split
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
    }
    long steps_per = (steps + splits - 1) / splits;
    p.pix_per_split = steps_per * BK;
    p.splits = (int)((steps + steps_per - 1) / steps_per);
    return p;
}

// narrow-layer (16x16 tiles, nine taps per block) wgrad plan
struct NPlan {
    bool use;
    int gm, gn, tiles_w, tiles_per_img, splits;
    long total_tiles, tiles_per_split;
};
static int g_wgrad_n16 = tuning_knob("wgrad_n16", &g_wgrad_n16, 1), g_wn16_target = tuning_knob("wn16_target", &g_wn16_target, 512),
           g_wn16_mintiles = tuning_knob("wn16_mintiles", &g_wn16_mintiles, 2), g_wn16_minc = tuning_knob("wn16_minc", &g_wn16_minc, 1);

// blocks per layer of a grouped nine-tap launch: layers with all 3 x 3 channel tiles in use come in numbers (the eight
// 45 -> 45 convolutions of the refinement stack), the narrower ones are one or two per launch and need more blocks each
static int g_wn16_group_target = tuning_knob("wn16_group_target", &g_wn16_group_target, 128), g_wn16_group_target_few = tuning_knob("wn16_group_few", &g_wn16_group_target_few, 256);
static int n16_group_target(int Cout, int C) { return (Cout > 32 && C > 32) ? g_wn16_group_target : g_wn16_group_target_few; }

static NPlan make_nplan(int N, int H, int W, int Cout, int C, int ld_x, int target = 0) {
    NPlan p;
    p.use = g_wgrad_n16 && C <= 64 && Cout <= 64 && C >= g_wn16_minc && H % 8 == 0 && W % 8 == 0 && ld_x % 4 == 0 &&
            ld_x >= round_up(C, 4) && (long)N * H * W < (1L << 31);
    if (!p.use) return p;
    p.gm = ceil_div(Cout, 48);
    p.gn = ceil_div(C, 48);
    p.tiles_w = W / 8;
    p.tiles_per_img = (H / 8) * p.tiles_w;
    p.total_tiles = (long)N * p.tiles_per_img;
    const long base = (long)p.gm * p.gn;
    long splits = ((target > 0 ? target : g_wn16_target) + base - 1) / base;
    if (splits > p.total_tiles / g_wn16_mintiles) splits = p.total_tiles / g_wn16_mintiles;
    if (splits < 1) splits = 1;
    p.tiles_per_split = (p.total_tiles + splits - 1) / splits;
    p.splits = (int)((p.total_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
    return p;
}

// tap-major wgrad plan
struct TPlan {
    bool use;
    int bm, bn, gm, gn, splits;
    int groups, per_group;       // two-stage split reduction when splits > 12 (groups of ~8 splits), else groups = 0
    long pix_per_split;
};
static int g_wgrad_tap = tuning_knob("wgrad_tap", &g_wgrad_tap, 1), g_wtap_target = tuning_knob("wtap_target", &g_wtap_target, 768),
           g_wtap_minsteps = tuning_knob("wtap_minsteps", &g_wtap_minsteps, 8), g_wtap_minc = tuning_knob("wtap_minc", &g_wtap_minc, 16),
           g_wtap_bm_max = tuning_knob("wtap_bm_max", &g_wtap_bm_max, 128);       // 64: no 128-row tiles (A/B runs)

static TPlan make_tplan(long M, int Cout, int C, int ntaps, int ld_x) {
    TPlan p;
    // measured on the MI355X (profiles/README.md): the tap-major form wins (+10..35 %) once one of the channel counts
    // exceeds a 64-wide tile; narrow high-resolution layers (45 -> 45, 35 -> 10, 44 -> 64) keep the halo / gather
    // kernels, whose tiles span several taps of the same channels (higher arithmetic intensity per staged byte)
    p.use = g_wgrad_tap && C >= g_wtap_minc && (g_wgrad_tap > 1 || C > 64 || Cout > 64) && ntaps <= 16 &&
            ld_x % 4 == 0 && ld_x >= round_up(C, 4) && M < (1L << 31);
    if (!p.use) return p;
    p.bm = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
    if (p.bm > g_wtap_bm_max) p.bm = g_wtap_bm_max;
    p.bn = (C > 64 || p.bm <= 64) ? 128 : 64;   // tiles in use: 128x128, 128x64, 64x128, 32x128
    p.gm = ceil_div(Cout, p.bm);
    p.gn = ceil_div(C, p.bn);
    const long tiles = (long)p.gm * p.gn * ntaps;
    const long steps = (M + BK - 1) / BK;
    long splits = (g_wtap_target + tiles - 1) / tiles;
    const long max_splits = steps / g_wtap_minsteps;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    const long steps_per = (steps + splits - 1) / splits;
    p.pix_per_split = steps_per * BK;
    p.splits = (int)((steps + steps_per - 1) / steps_per);
    p.groups = p.splits > 12 ? ceil_div(p.splits, 8) : 0;     // == split_groups(splits)
    p.per_group = 8;
    return p;
}

// groups of the two-stage split reduction (0: single stage)
static inline int split_groups(int splits) { return splits > 12 ? ceil_div(splits, 8) : 0; }

// sum `splits` partials of n floats each (at ws) into dst rows: optional first stage over groups of 8 splits
static void launch_wgrad_reduce(float* ws, int splits, int Cout, int NT, float* dst, long ld_out, hipStream_t s) {
    const long n = (long)Cout * NT;
    const float* src = ws;
    int nsum = splits;
    const int groups = split_groups(splits);
    if (groups) {
        float* part2 = ws + (size_t)splits * n;
        hipLaunchKernelGGL(conv3x3_wgrad_group_sum_kernel, dim3(grid_for(n, 1024), groups), dim3(256), 0, s, ws, n, splits, 8,
                           part2, 0L);
        src = part2;
        nsum = groups;
    }
    hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3(grid_for(n * 4, 8192)), dim3(256), 0, s, src, nsum, Cout, NT, dst,
                       ld_out);
}

// ---- grouped tap-major weight gradients: plan / build / launch --------------------------------------------------------
static int g_wgroup_chunk = tuning_knob("wgroup_chunk", &g_wgroup_chunk, 256);
static int g_wgroup_long = tuning_knob("wgroup_long", &g_wgroup_long, 1), g_wgroup_long_from = tuning_knob("wgroup_long_from", &g_wgroup_long_from, 128);
static int g_up_subpixel = tuning_knob("up_subpixel", &g_up_subpixel, 1);     // weight gradients of up-sampled convolutions: sub-pixel form

// the sub-pixel tap-major plan of an up-sampled 3x3 layer (flags: UPSAMPLED | CLEAN_PADS), or use = false
static TPlan make_up_tplan(int N, int Ho, int Wo, int Cout, int C, int kh, int kw, int pad, int ld_x, int flags) {
    TPlan tp;
    tp.use = false;
    if (!(g_up_subpixel && (flags & MNK_CONV_UPSAMPLED) && (flags & MNK_CONV_CLEAN_PADS) && kh == 3 && kw == 3 && pad == 1 &&
          Ho % 2 == 0 && Wo % 2 == 0))
        return tp;
    TPlan base = make_tplan((long)N * Ho * Wo, Cout, C, 9, ld_x);
    if (!base.use) return tp;                       // narrow layers keep their own kernels
    return make_tplan((long)N * (Ho / 2) * (Wo / 2), Cout, C, 16, ld_x);
}     // pixels per block of a grouped launch (multiple of 16)

// pixel splits of one job of a grouped launch: chunks of ~g_wgroup_chunk pixels, at least 8 K steps each
static void grouped_split(long M, int* splits, long* pix_per_split) {
    const long steps = (M + BK - 1) / BK;
    long chunk = g_wgroup_chunk;
    if (g_wgroup_long > 1 && M / chunk >= g_wgroup_long_from) chunk *= g_wgroup_long;     // long layers: longer chunks, fewer partials
    long sp = (M + chunk - 1) / chunk;
    const long max_sp = steps / 8;
    if (sp > max_sp) sp = max_sp;
    if (sp < 1) sp = 1;
    const long steps_per = (steps + sp - 1) / sp;
    *pix_per_split = steps_per * BK;
    *splits = (int)((steps + steps_per - 1) / steps_per);
}

// small maps: the tap-major kernel's K runs over the (pixel, tap) pairs inside the source only (WgradTapArgs::compact);
// wtap_compact = the largest H * W (of the dy geometry; the low resolution for the sub-pixel form) that takes this form, 0: off
static int g_wtap_compact = tuning_knob("wtap_compact", &g_wtap_compact, 64);
static bool tap_compact_ok(int H, int W, long M, int kh, int kw, int pad, int ups, int subpix) {
    if (g_wtap_compact <= 0 || (long)H * W > g_wtap_compact || M >= (1L << 20)) return false;
    return subpix || (!ups && kh == 3 && kw == 3 && pad == 1);
}
// 1: a sub-pixel job on a 1 x 1 low-resolution source makes tiles for its four live pseudo taps only (pack_tile.h: up1x1_live) and
// the readers of its partials, and the optimiser kernel's pack emission, leave the dead slices alone; 0: all 16, as for any source
static int g_up1x1_dead_taps = tuning_knob("up1x1_dead_taps", &g_up1x1_dead_taps, 1);
// ONE rule for the GEMM that leaves the dead slices unwritten and for everybody who must then not read them (H, W: the low
// resolution; the tile index of the live taps lives in the compact K form)
static bool up1x1_skips(int H, int W, long M) { return g_up1x1_dead_taps && H == 1 && W == 1 && tap_compact_ok(H, W, M, 3, 3, 1, 0, 1); }
// (pixel, tap) pairs a compact job multiplies: 3x3 pad 1: (3H - 2)(3W - 2) per frame; sub-pixel form (offsets {-1, 0} / {0, +1}
// per phase and axis): (4H - 2)(4W - 2) per frame
static double tap_compact_pairs(long frames, int H, int W, int subpix) {
    return subpix ? (double)frames * (4.0 * H - 2.0) * (4.0 * W - 2.0) : (double)frames * (3.0 * H - 2.0) * (3.0 * W - 2.0);
}

// variant id of a tap-major job: 4 * tile + mode; tile 0: 128x128, 1: 128x64, 2: 64x128, 3: 32x128; mode 3: sub-pixel form
static int tap_tile_id(const TPlan& tp) {
    if (tp.bm == 128 && tp.bn == 128) return 0;
    if (tp.bm == 128) return 1;
    if (tp.bm == 64) return 2;
    return 3;
}

struct GroupedHeader {
    int magic, n, nvariants, reserved;
    int first[32], count[32], blocks[32];     // per variant: first record, records, blocks (records are sorted by variant)
};

// ---- which form a weight-gradient job runs -----------------------------------------------------------------------------------
// ONE decision for the single-layer entry (mnk_conv2d_wgrad), its plan query (mnk_conv2d_wgrad_plan2) and the grouped launch
// (mnk_wgrad_grouped_plan / _build): the caller sizes its partial buffers from what a query says and a launch writes what it
// selects, so both read the same value.  The shape of a job travels as a MnkWgradJob (x / dy / part may be null in a query).
enum WgradForm { WG_SUBPIX, WG_TAP, WG_N16, WG_HALO, WG_GATHER };      // in the order they are tried

struct WgradSel {
    WgradForm form;
    int variant;            // grouped jobs: the grouped launch's kernel (tap-major: 4 * tile + loader mode; nine-tap: 16 + 3 * (co
                            // tiles - 1) + (ci tiles - 1)); -1: the grouped launch does not take the job
    TPlan t;                // the plan of `form`: WG_SUBPIX / WG_TAP,
    NPlan n;                // WG_N16,
    HPlan h;                // WG_HALO,
    WPlan w;                // WG_GATHER
    // the tap-major forms: the geometry the kernel walks (WG_SUBPIX: the LOW resolution, 16 pseudo taps), its pixel range per
    // split and its loader (tap_mode)
    int H, W, ntaps, mode, sw, sh, sn;
    long M, pix_per_split;
    int splits;             // split partials the GEMM leaves behind; 0: it writes dw itself (nothing to reduce)
    int layout;             // of the partials (MnkWgradPlan::layout)
    bool dead1x1;           // WG_SUBPIX on a 1 x 1 source (up1x1_skips): tiles of the four live pseudo taps only, the dead slices of
                            // the partials stay unwritten -- the reduction must carry MNK_REDUCE_UP1X1
    size_t part_floats;     // the partials = the workspace of the single-layer entry under MNK_WGRAD_DEFER
    size_t ws_floats;       // ... and without it: + the group sums of a two-stage reduction
};

// 16-wide co / ci tiles of the nine-tap kernel in use (its template arguments)
static int n16_tiles(int channels) { return channels > 32 ? 3 : (channels > 16 ? 2 : 1); }

static MnkWgradJob wgrad_job(const float* x, const float* dy, float* part, int N, int Ho, int Wo, int Hi, int Wi, int C, int Cout,
                             int kh, int kw, int pad, int ld_x, int ld_dy, int flags) {
    MnkWgradJob j = {};
    j.x = x, j.dy = dy, j.part = part, j.ld_x = ld_x, j.C = C, j.flags = flags, j.ld_dy = ld_dy, j.Cout = Cout;
    j.N = N, j.Ho = Ho, j.Wo = Wo, j.Hi = Hi, j.Wi = Wi, j.kh = kh, j.kw = kw, j.pad = pad;
    return j;
}

// loader mode + walk constants (s.sw / sh / sn) of the tap-major kernel for the pixel range length s.pix_per_split
static int tap_mode(WgradSel& s, const MnkWgradJob& j, bool subpix) {
    const int H = j.Ho, W = j.Wo, ups = j.flags & MNK_CONV_UPSAMPLED;
    s.sw = s.sh = s.sn = 0;
    if (subpix) return 3;
    if (tap_compact_ok(H, W, (long)j.N * H * W, j.kh, j.kw, j.pad, ups, 0)) return 0;      // compact K lives in the generic loader
    const long span_a = s.pix_per_split * (long)j.ld_dy * 4, span_b = (s.pix_per_split + 2L * W + 2 * BK) * j.ld_x * 4;
    bool walk = true;          // can a 16-pixel step be walked as columns / rows / frames with single wraps?
    s.sw = BK;
    if (W < BK) {
        s.sw = 0;
        const int r = BK / W;
        if (BK % W != 0)
            walk = false;
        else if (r < H)
            s.sh = r;
        else if (r % H == 0)
            s.sn = r / H;
        else
            walk = false;
    }
    // fast loader: 3x3 pad 1, clean pads, rows of >= 16 pixels, split ranges inside the 2^30-byte buffer window
    return (g_fast_loader && (j.flags & MNK_CONV_CLEAN_PADS) && j.kh == 3 && j.kw == 3 && j.pad == 1 && walk &&
            span_a < (1L << 29) && span_b < (1L << 29) && (!ups || (long)j.N * (j.Hi / 2) * (j.Wi / 2) * j.ld_x * 4 < (1L << 29)))
               ? (ups ? 2 : 1) : 0;
}

// aligned: x and dy are 16-byte aligned (the single-layer entry looks at its operands; its queries assume it; the grouped
// build requires it).  grouped: the job is planned for mnk_wgrad_grouped_*, which differs from the single-layer entry in
//   * tap-major jobs: pixel chunks of grouped_split instead of TPlan::splits (the tiles of all layers fill the chip);
//   * nine-tap jobs: n16_group_target blocks per layer, and only jobs that are split (the kernel writes partials);
//   * LDS-halo, gather and the other K x K shapes are not taken: variant -1, nothing planned.
static WgradSel wgrad_select(const MnkWgradJob& j, bool aligned, bool grouped) {
    WgradSel s = {};
    const bool k3 = j.kh == 3 && j.kw == 3 && j.pad == 1;
    s.form = WG_GATHER;
    s.variant = -1;
    s.H = j.Ho, s.W = j.Wo, s.ntaps = j.kh * j.kw;
    s.M = (long)j.N * j.Ho * j.Wo;
    if (aligned || grouped) {       // the tap-major and nine-tap kernels read float4s
        // up-sampled 3x3 layer with clean sources: the sub-pixel form (16 pseudo taps over the LOW-resolution pixels)
        s.t = make_up_tplan(j.N, j.Ho, j.Wo, j.Cout, j.C, j.kh, j.kw, j.pad, j.ld_x, j.flags);
        const bool subpix = s.t.use;
        if (subpix)
            s.H = j.Ho / 2, s.W = j.Wo / 2, s.ntaps = 16, s.M = (long)j.N * s.H * s.W;
        else
            s.t = make_tplan(s.M, j.Cout, j.C, s.ntaps, j.ld_x);
        if (s.t.use) {
            s.form = subpix ? WG_SUBPIX : WG_TAP;
            s.layout = subpix ? 2 : 0;
            s.splits = s.t.splits, s.pix_per_split = s.t.pix_per_split;
            if (grouped) grouped_split(s.M, &s.splits, &s.pix_per_split);
            s.mode = tap_mode(s, j, subpix);
            s.dead1x1 = subpix && up1x1_skips(s.H, s.W, s.M);
            if (grouped) s.variant = 4 * tap_tile_id(s.t) + s.mode;
        } else if (k3 && (!grouped || g_wn16_group_target > 0)) {
            s.n = make_nplan(j.N, j.Ho, j.Wo, j.Cout, j.C, j.ld_x, grouped ? n16_group_target(j.Cout, j.C) : 0);
            if (s.n.use && (!grouped || s.n.splits > 1)) {
                s.form = WG_N16;
                s.splits = s.n.splits > 1 ? s.n.splits : 0;       // tap-major partials: layout 0
                if (grouped) s.variant = 16 + 3 * (n16_tiles(j.Cout) - 1) + (n16_tiles(j.C) - 1);
            }
        }
    }
    if (grouped && s.variant < 0) return s;
    if (s.form == WG_GATHER && k3) {
        s.h = make_hplan(j.N, j.Ho, j.Wo, j.Cout, j.C);
        if (s.h.use) s.form = WG_HALO, s.splits = s.h.splits > 1 ? s.h.splits : 0;
    }
    if (s.form == WG_GATHER) {
        s.w = make_wplan(s.M, j.Cout, j.C, s.ntaps);
        s.splits = s.w.splits > 1 ? s.w.splits : 0;
    }
    if (s.form >= WG_HALO && s.splits) s.layout = 1;              // parameter-major partials
    const size_t per = (size_t)s.ntaps * j.Cout * j.C;
    s.part_floats = s.splits * per;
    s.ws_floats = (s.splits + split_groups(s.splits)) * per;
    return s;
}

// tiles of a tap-major job along its taps
static int tap_tiles(const WgradSel& s) { return s.dead1x1 ? 4 : s.ntaps; }

static void fill_tap_args(WgradTapArgs& g, const MnkWgradJob& j, const WgradSel& s, int xcd) {
    const bool subpix = s.form == WG_SUBPIX;
    const int ups = subpix ? 0 : (j.flags & MNK_CONV_UPSAMPLED);        // the sub-pixel form reads the source as it is
    g.x = j.x, g.ld_x = j.ld_x, g.C = j.C, g.ups = ups, g.dy = j.dy, g.ld_dy = j.ld_dy, g.Cout = j.Cout;
    g.H = s.H, g.W = s.W, g.Hi = subpix ? s.H : j.Hi, g.Wi = subpix ? s.W : j.Wi;
    g.ntaps = s.ntaps, g.kw = subpix ? 4 : j.kw, g.pad = subpix ? 0 : j.pad;
    g.M = s.M, g.pix_per_split = s.pix_per_split, g.gn = s.t.gn, g.part = j.part, g.xcd = xcd;
    g.clean = (j.flags & MNK_CONV_CLEAN_PADS) ? 1 : 0;
    fast_div_consts((unsigned)s.W, &g.mulW, &g.shW);
    fast_div_consts((unsigned)s.H, &g.mulH, &g.shH);
    g.sw = s.sw, g.sh = s.sh, g.sn = s.sn;
    g.compact = tap_compact_ok(s.H, s.W, s.M, j.kh, j.kw, j.pad, ups, subpix) ? (s.dead1x1 ? 2 : 1) : 0;
    g.nsplits = s.splits;
}

static void fill_n16_args(WgradN16Args& g, const MnkWgradJob& j, const NPlan& np, float* out, long ld_out) {
    g.x = j.x, g.ld_x = j.ld_x, g.C = j.C, g.ups = j.flags & MNK_CONV_UPSAMPLED, g.dy = j.dy, g.ld_dy = j.ld_dy, g.Cout = j.Cout;
    g.H = j.Ho, g.W = j.Wo, g.tiles_w = np.tiles_w, g.tiles_per_img = np.tiles_per_img;
    g.total_tiles = np.total_tiles, g.tiles_per_split = np.tiles_per_split;
    g.NT = 9 * j.C, g.splits = np.splits, g.out = out, g.ld_out = ld_out;
}

// the tap-major kernel of a tile (tap_tile_id) and loader mode; bf16x3: one generic-loader form per tile (plain / sub-pixel)
// one_plane (MNK_WGRAD_BF16): the one-plane form of the same kernel; it wins over the tuning value
template <int BM, int BN, int WM, int WN>
static void launch_tap_tile(int mode, dim3 grid, hipStream_t st, const WgradTapArgs& g, bool one_plane) {
    if (one_plane) {
        if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_h_kernel<BM, BN, WM, WN, true, 1>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((conv3x3_wgrad_tap_h_kernel<BM, BN, WM, WN, false, 1>), grid, dim3(256), 0, st, g);
    } else if (g_wgrad_bf16x3) {
        if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_h_kernel<BM, BN, WM, WN, true>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((conv3x3_wgrad_tap_h_kernel<BM, BN, WM, WN, false>), grid, dim3(256), 0, st, g);
    } else if (mode == 1) hipLaunchKernelGGL((conv3x3_wgrad_tap_kernel<BM, BN, WM, WN, 1>), grid, dim3(256), 0, st, g);
    else if (mode == 2) hipLaunchKernelGGL((conv3x3_wgrad_tap_kernel<BM, BN, WM, WN, 2>), grid, dim3(256), 0, st, g);
    else if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_kernel<BM, BN, WM, WN, 3>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((conv3x3_wgrad_tap_kernel<BM, BN, WM, WN, 0>), grid, dim3(256), 0, st, g);
}
template <int BM, int BN, int WM, int WN>
static void launch_tap_tile_grouped(int mode, int blocks, hipStream_t st, const TapJobRec* rv, int cnt, bool one_plane) {
    if (one_plane) {
        if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_h_kernel<BM, BN, WM, WN, true, 1>), dim3(blocks), dim3(256), 0, st, rv, cnt);
        else hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_h_kernel<BM, BN, WM, WN, false, 1>), dim3(blocks), dim3(256), 0, st, rv, cnt);
    } else if (g_wgrad_bf16x3) {
        if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_h_kernel<BM, BN, WM, WN, true>), dim3(blocks), dim3(256), 0, st, rv, cnt);
        else hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_h_kernel<BM, BN, WM, WN, false>), dim3(blocks), dim3(256), 0, st, rv, cnt);
    } else if (mode == 1) hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_kernel<BM, BN, WM, WN, 1>), dim3(blocks), dim3(256), 0, st, rv, cnt);
    else if (mode == 2) hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_kernel<BM, BN, WM, WN, 2>), dim3(blocks), dim3(256), 0, st, rv, cnt);
    else if (mode == 3) hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_kernel<BM, BN, WM, WN, 3>), dim3(blocks), dim3(256), 0, st, rv, cnt);
    else hipLaunchKernelGGL((conv3x3_wgrad_tap_grouped_kernel<BM, BN, WM, WN, 0>), dim3(blocks), dim3(256), 0, st, rv, cnt);
}

// sum the `splits` tap-major partials at ws into dw (fold: the 16 pseudo taps of the sub-pixel form into the nine kernel taps):
// optional first stage over groups of 8 splits, then the (tap, ci) -> (ci, tap) transposing reduction.  fold == 2: the partials of
// a 1 x 1 source (WgradSel::dead1x1) -- neither stage reads the slices of the dead pseudo taps
static void launch_tap_reduce(float* ws, int splits, int ntaps, int Cout, int C, float* dst, long ld_out, int fold, hipStream_t s) {
    const long n = (long)ntaps * Cout * C;
    const float* src = ws;
    int nsum = splits;
    const int groups = split_groups(splits);
    if (groups) {
        float* part2 = ws + (size_t)splits * n;
        hipLaunchKernelGGL(conv3x3_wgrad_group_sum_kernel, dim3(grid_for(n, 1024), groups), dim3(256), 0, s, ws, n, splits, 8,
                           part2, fold == 2 ? (long)Cout * C : 0L);
        src = part2;
        nsum = groups;
    }
    hipLaunchKernelGGL(conv3x3_wgrad_tap_reduce_kernel, dim3(ceil_div(C, 64), Cout), dim3(256), 0, s, src, nsum, ntaps, Cout, C,
                       dst, ld_out, fold);
}

}  // namespace

extern "C" {

size_t mnk_conv2d_wgrad_workspace_floats(int N, int Ho, int Wo, int C, int Cout, int kh, int kw, int pad) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || Cout <= 0 || kh <= 0 || kw <= 0) return 0;
    const int ntaps = kh * kw;
    {   // the caller's ld_x is not known here: size for the tap-major form whenever the shape allows it
        TPlan tp = make_tplan((long)N * Ho * Wo, Cout, C, ntaps, round_up(C, 4));
        if (tp.use) return (size_t)(tp.splits + tp.groups) * ntaps * Cout * C;
    }
    if (kh == 3 && kw == 3 && pad == 1) {
        NPlan np = make_nplan(N, Ho, Wo, Cout, C, round_up(C, 4));
        HPlan hp = make_hplan(N, Ho, Wo, Cout, C);
        size_t need = 0;        // the caller's ld_x / alignment may still demote the n16 form: size for both
        if (np.use && np.splits > 1) need = (size_t)(np.splits + split_groups(np.splits)) * Cout * 9 * C;
        if (hp.use) {
            const size_t nh = hp.splits > 1 ? (size_t)(hp.splits + split_groups(hp.splits)) * Cout * 9 * C : 0;
            return nh > need ? nh : need;
        }
        if (np.use) {
            WPlan p = make_wplan((long)N * Ho * Wo, Cout, C, ntaps);
            const size_t ng = p.splits > 1 ? (size_t)(p.splits + split_groups(p.splits)) * Cout * ntaps * C : 0;
            return ng > need ? ng : need;
        }
    }
    WPlan p = make_wplan((long)N * Ho * Wo, Cout, C, ntaps);
    return p.splits > 1 ? (size_t)(p.splits + split_groups(p.splits)) * Cout * ntaps * C : 0;
}

size_t mnk_conv3x3_up_wgrad_workspace_floats(int N, int Ho, int Wo, int C, int Cout) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || Cout <= 0) return 0;
    TPlan up = make_up_tplan(N, Ho, Wo, Cout, C, 3, 3, 1, round_up(C, 4), MNK_CONV_UPSAMPLED | MNK_CONV_CLEAN_PADS);
    const size_t a = up.use ? (size_t)(up.splits + up.groups) * 16 * Cout * C : 0;
    const size_t b = mnk_conv2d_wgrad_workspace_floats(N, Ho, Wo, C, Cout, 3, 3, 1);
    return a > b ? a : b;
}

int mnk_conv2d_wgrad(const float* x, int ld_x, int C, int flags, int Hi, int Wi, int kh, int kw, int pad, const float* dy,
                     int ld_dy, int Cout, float* dw, int Cin_total, int c_start, int N, int Ho, int Wo, float* ws,
                     size_t ws_floats, void* stream) {
    MNK_REQUIRE(flags >= 0 && flags <= 15);
    const int ups = flags & MNK_CONV_UPSAMPLED;
    // MNK_WGRAD_BF16: the tap-major forms run their one-plane bf16 kernel; the plan (and every other form) does not look at it
    const bool one_plane = (flags & MNK_WGRAD_BF16) != 0;
    // MNK_WGRAD_DEFER: leave the split partials in `ws` (layout / size: mnk_conv2d_wgrad_plan) and skip the reduction --
    // the caller reduces the partials of many layers in one launch (mnk_wgrad_reduce_multi)
    const bool defer = (flags & MNK_WGRAD_DEFER) != 0;
    const bool aligned = (size_t)x % 16 == 0 && (size_t)dy % 16 == 0;
    MNK_REQUIRE(x && dy && dw && N > 0 && Ho > 0 && Wo > 0 && C > 0 && Cout > 0 && kh > 0 && kw > 0 && pad >= 0);
    MNK_REQUIRE(!defer || aligned);      // the plan query assumes aligned operands
    MNK_REQUIRE(Ho == Hi + 2 * pad - kh + 1 && Wo == Wi + 2 * pad - kw + 1);
    MNK_REQUIRE(ld_x >= C && ld_dy % 4 == 0 && ld_dy >= Cout);
    MNK_REQUIRE(c_start >= 0 && c_start + C <= Cin_total && (!ups || (Hi % 2 == 0 && Wi % 2 == 0)));
    const MnkWgradJob j = wgrad_job(x, dy, ws, N, Ho, Wo, Hi, Wi, C, Cout, kh, kw, pad, ld_x, ld_dy, flags);
    const WgradSel s = wgrad_select(j, aligned, false);
    const size_t need = defer ? s.part_floats : s.ws_floats;
    if (need && (!ws || ws_floats < need)) {
        set_error("mnk_conv2d_wgrad: workspace too small (%zu < %zu floats)", ws_floats, need);
        return MNK_EWORKSPACE;
    }
    const int ntaps = kh * kw, NT = ntaps * C;
    float* dst = dw + (long)c_start * ntaps;
    const long ld_dst = (long)Cin_total * ntaps;
    // the nine-tap, LDS-halo and gather kernels write parameter rows: a split's partial, or dw itself when there is one split
    float* out = s.splits ? ws : dst;
    const long ld_out = s.splits ? NT : ld_dst;
    const double flop = 2.0 * (double)N * Ho * Wo * Cout * (double)ntaps * C;
    hipStream_t st = (hipStream_t)stream;
    switch (s.form) {
        case WG_SUBPIX:
        case WG_TAP: {
            WgradTapArgs g;
            fill_tap_args(g, j, s, g_xcd_remap);
            const bool subpix = s.form == WG_SUBPIX;      // (its 16 pseudo taps run at the low resolution)
            ProfScope prof(K_CONV_WGRAD, st, flop, g.compact ? 2.0 * tap_compact_pairs(N, s.H, s.W, subpix) * Cout * C
                                                   : subpix ? 2.0 * (double)s.M * Cout * 16.0 * C : -1.0);
            const dim3 grid(s.t.gm, s.t.gn * tap_tiles(s), s.splits);
            switch (tap_tile_id(s.t)) {
                case 0: launch_tap_tile<128, 128, 2, 2>(s.mode, grid, st, g, one_plane); break;
                case 1: launch_tap_tile<128, 64, 2, 2>(s.mode, grid, st, g, one_plane); break;
                case 2: launch_tap_tile<64, 128, 1, 4>(s.mode, grid, st, g, one_plane); break;
                default: launch_tap_tile<32, 128, 1, 4>(s.mode, grid, st, g, one_plane); break;
            }
            break;
        }
        case WG_N16: {
            WgradN16Args g;
            fill_n16_args(g, j, s.n, out, ld_out);
            ProfScope prof(K_CONV_WGRAD, st, flop);
            const int nct = n16_tiles(Cout), nci = n16_tiles(C);
            const dim3 gridn(s.n.gm, s.n.gn, s.n.splits);
#define MNK_N16(T, I)                                                                                      \
    if (nct == T && nci == I) hipLaunchKernelGGL((conv3x3_wgrad_n16_kernel<T, I>), gridn, dim3(256), 0, st, g)
            MNK_N16(3, 3); MNK_N16(3, 2); MNK_N16(3, 1);
            MNK_N16(2, 3); MNK_N16(2, 2); MNK_N16(2, 1);
            MNK_N16(1, 3); MNK_N16(1, 2); MNK_N16(1, 1);
#undef MNK_N16
            break;
        }
        case WG_HALO: {
            const HPlan& hp = s.h;
            WgradHaloArgs h;
            h.x = x, h.ld_x = ld_x, h.C = C, h.ups = ups, h.dy = dy, h.ld_dy = ld_dy, h.Cout = Cout, h.N = N, h.H = Ho, h.W = Wo;
            h.TR = hp.TR, h.TC = hp.TC, h.tiles_w = hp.tiles_w, h.tiles_per_img = hp.tiles_per_img, h.gn = hp.gn;
            h.total_tiles = hp.total_tiles, h.tiles_per_split = hp.tiles_per_split;
            h.NT = NT, h.splits = hp.splits, h.out = out, h.ld_out = ld_out;
            ProfScope prof(K_CONV_WGRAD, st, flop);
            hipLaunchKernelGGL(conv3x3_wgrad_halo_kernel, dim3(hp.gm, hp.gn * 3, hp.splits), dim3(256), 0, st, h);
            break;
        }
        case WG_GATHER: {
            const WPlan& p = s.w;
            WgradArgs a;
            a.x = x, a.ld_x = ld_x, a.C = C, a.ups = ups, a.dy = dy, a.ld_dy = ld_dy, a.Cout = Cout, a.N = N, a.H = Ho, a.W = Wo;
            a.Hi = Hi, a.Wi = Wi, a.ntaps = ntaps, a.kw = kw, a.pad = pad, a.M = s.M, a.NT = NT;
            a.pix_per_split = p.pix_per_split, a.splits = p.splits, a.out = out, a.ld_out = ld_out;
            ProfScope prof(K_CONV_WGRAD, st, flop);
            if (p.bm == 128)
                hipLaunchKernelGGL((conv3x3_wgrad_kernel<128>), dim3(p.gm, p.gn, p.splits), dim3(256), 0, st, a);
            else if (p.bm == 64)
                hipLaunchKernelGGL((conv3x3_wgrad_kernel<64>), dim3(p.gm, p.gn, p.splits), dim3(256), 0, st, a);
            else
                hipLaunchKernelGGL((conv3x3_wgrad_kernel<32>), dim3(p.gm, p.gn, p.splits), dim3(256), 0, st, a);
            break;
        }
    }
    if (s.splits && !defer) {
        const bool tap_major = s.form <= WG_N16;        // (the tap-major forms' figure counts the write of dw too)
        ProfScope prof(K_CONV_REDUCE, st, (double)(s.splits + (s.form <= WG_TAP ? 1 : 0)) * s.ntaps * Cout * C * 4);
        if (tap_major)
            launch_tap_reduce(ws, s.splits, s.ntaps, Cout, C, dst, ld_dst, s.form == WG_SUBPIX ? (s.dead1x1 ? 2 : 1) : 0, st);
        else
            launch_wgrad_reduce(ws, s.splits, Cout, NT, dst, ld_dst, st);
    }
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

// which weight-gradient form mnk_conv2d_wgrad runs for a shape (16-byte aligned operands assumed) and what it leaves behind
// under MNK_WGRAD_DEFER: layout 0 = tap-major partials [split][tap][Cout][C], 1 = parameter-major [split][Cout][C*ntaps];
// splits == 0: the GEMM writes dw itself (nothing to reduce)
int mnk_conv2d_wgrad_plan(int N, int Ho, int Wo, int C, int Cout, int kh, int kw, int pad, int ld_x, MnkWgradPlan* plan) {
    return mnk_conv2d_wgrad_plan2(N, Ho, Wo, C, Cout, kh, kw, pad, ld_x, 0, plan);
}

int mnk_conv2d_wgrad_plan2(int N, int Ho, int Wo, int C, int Cout, int kh, int kw, int pad, int ld_x, int flags,
                           MnkWgradPlan* plan) {
    MNK_REQUIRE(plan && N > 0 && Ho > 0 && Wo > 0 && C > 0 && Cout > 0 && kh > 0 && kw > 0 && pad >= 0 && ld_x >= C);
    // (the input size and ld_dy only choose the tap-major loader, which a plan does not report)
    const WgradSel s = wgrad_select(wgrad_job(nullptr, nullptr, nullptr, N, Ho, Wo, Ho - 2 * pad + kh - 1, Wo - 2 * pad + kw - 1,
                                              C, Cout, kh, kw, pad, ld_x, round_up(Cout, 4), flags), true, false);
    plan->layout = s.layout;
    plan->splits = s.splits;
    plan->part_floats = s.part_floats;
    return MNK_OK;
}

int mnk_wgrad_grouped_plan(MnkWgradJob* jobs, int n) {
    MNK_REQUIRE(jobs && n > 0);
    for (int i = 0; i < n; ++i) {
        MnkWgradJob& j = jobs[i];
        MNK_REQUIRE(j.N > 0 && j.Ho > 0 && j.Wo > 0 && j.C > 0 && j.Cout > 0 && j.kh > 0 && j.kw > 0 && j.pad >= 0);
        const WgradSel s = wgrad_select(j, true, true);       // (not taken: variant -1, nothing planned)
        j.variant = s.variant;
        j.splits = s.splits;
        j.part_floats = s.part_floats;
        j.layout = s.layout;
    }
    return MNK_OK;
}

size_t mnk_wgrad_grouped_table_bytes(int n) { return n > 0 ? sizeof(GroupedHeader) + (size_t)n * sizeof(TapJobRec) : 0; }

int mnk_wgrad_grouped_build(const MnkWgradJob* jobs, int n, void* host_table, size_t table_bytes) {
    MNK_REQUIRE(jobs && n > 0 && host_table && table_bytes >= mnk_wgrad_grouped_table_bytes(n));
    GroupedHeader* hd = (GroupedHeader*)host_table;
    TapJobRec* recs = (TapJobRec*)((char*)host_table + sizeof(GroupedHeader));
    hd->magic = 0x4d4e4b47;
    hd->n = n;
    hd->nvariants = 25;
    hd->reserved = 0;       // 1: the tap-major jobs run the one-plane bf16 form (MNK_WGRAD_BF16) -- all of them or none
    int k = 0, tap_jobs = 0, tap_bf16 = 0;
    for (int i = 0; i < n; ++i)
        if (jobs[i].variant >= 0 && jobs[i].variant < 16) ++tap_jobs, tap_bf16 += (jobs[i].flags & MNK_WGRAD_BF16) ? 1 : 0;
    MNK_REQUIRE(tap_bf16 == 0 || tap_bf16 == tap_jobs);
    hd->reserved = tap_bf16 ? 1 : 0;
    for (int v = 0; v < 25; ++v) {
        hd->first[v] = k;
        int blocks = 0;
        for (int i = 0; i < n; ++i) {
            const MnkWgradJob& j = jobs[i];
            MNK_REQUIRE(j.variant >= 0 && j.variant < 25);
            if (j.variant != v) continue;
            MNK_REQUIRE(j.x && j.dy && j.part && ((size_t)j.x % 16) == 0 && ((size_t)j.dy % 16) == 0);
            // the job array has crossed the C-ABI since mnk_wgrad_grouped_plan: what it carries must still be what is selected
            const WgradSel s = wgrad_select(j, true, true);
            if (v >= 16) {          // nine-tap 16x16 job
                MNK_REQUIRE(s.form == WG_N16 && s.splits == j.splits);
                N16JobRec& r = reinterpret_cast<N16JobRec*>(recs)[k];
                fill_n16_args(r.a, j, s.n, j.part, 9 * j.C);
                r.gm = s.n.gm, r.gn = s.n.gn, r.splits = s.splits, r.block_begin = blocks;
                blocks += r.gm * r.gn * r.splits;
                ++k;
                continue;
            }
            MNK_REQUIRE(s.form <= WG_TAP && tap_tile_id(s.t) == v / 4);
            MNK_REQUIRE(s.splits == j.splits);
            MNK_REQUIRE(s.mode == v % 4);
            TapJobRec& r = recs[k];
            fill_tap_args(r.a, j, s, 0);
            r.gm = s.t.gm;
            r.gnt = s.t.gn * tap_tiles(s);
            r.splits = s.splits;
            r.block_begin = blocks;
            blocks += r.gm * r.gnt * r.splits;
            ++k;
        }
        hd->count[v] = k - hd->first[v];
        hd->blocks[v] = blocks;
    }
    MNK_REQUIRE(k == n);
    return MNK_OK;
}

int mnk_wgrad_grouped_launch(const void* device_table, const void* host_table, void* stream) {
    MNK_REQUIRE(device_table && host_table);
    const GroupedHeader* hd = (const GroupedHeader*)host_table;
    MNK_REQUIRE(hd->magic == 0x4d4e4b47 && hd->n > 0 && (hd->reserved == 0 || hd->reserved == 1));
    const bool one_plane = hd->reserved == 1;
    const TapJobRec* hrecs = (const TapJobRec*)((const char*)host_table + sizeof(GroupedHeader));
    const TapJobRec* drecs = (const TapJobRec*)((const char*)device_table + sizeof(GroupedHeader));
    hipStream_t st = (hipStream_t)stream;
    for (int v = 0; v < 16; ++v) {
        const int cnt = hd->count[v], blocks = hd->blocks[v];
        if (!cnt) continue;
        double flop = 0.0, issued = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const WgradTapArgs& g = hrecs[hd->first[v] + i].a;      // algorithmic: the sub-pixel form stands for 9 taps at 4 M pixels
            flop += v % 4 == 3 ? 2.0 * 4.0 * (double)g.M * g.Cout * 9.0 * g.C : 2.0 * (double)g.M * g.Cout * (double)g.ntaps * g.C;
            issued += g.compact ? 2.0 * tap_compact_pairs(g.M / ((long)g.H * g.W), g.H, g.W, v % 4 == 3) * g.Cout * g.C
                                : 2.0 * (double)g.M * g.Cout * (double)g.ntaps * g.C;
        }
        ProfScope prof(K_CONV_WGRAD, st, flop, issued);
        const TapJobRec* rv = drecs + hd->first[v];
        const int mode = v % 4;
        switch (v / 4) {
            case 0: launch_tap_tile_grouped<128, 128, 2, 2>(mode, blocks, st, rv, cnt, one_plane); break;
            case 1: launch_tap_tile_grouped<128, 64, 2, 2>(mode, blocks, st, rv, cnt, one_plane); break;
            case 2: launch_tap_tile_grouped<64, 128, 1, 4>(mode, blocks, st, rv, cnt, one_plane); break;
            default: launch_tap_tile_grouped<32, 128, 1, 4>(mode, blocks, st, rv, cnt, one_plane); break;
        }
    }
    for (int v = 16; v < 25; ++v) {
        const int cnt = hd->count[v], blocks = hd->blocks[v];
        if (!cnt) continue;
        const N16JobRec* hn = reinterpret_cast<const N16JobRec*>(hrecs) + hd->first[v];
        double flop = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const WgradN16Args& g = hn[i].a;
            flop += 2.0 * (double)g.total_tiles * 64.0 * g.Cout * 9.0 * g.C;
        }
        ProfScope prof(K_CONV_WGRAD, st, flop);
        const N16JobRec* rv = reinterpret_cast<const N16JobRec*>(drecs) + hd->first[v];
        const int nct = (v - 16) / 3 + 1, nci = (v - 16) % 3 + 1;
#define MNK_N16G(T, I)                                                                                                  \
    if (nct == T && nci == I) hipLaunchKernelGGL((conv3x3_wgrad_n16_grouped_kernel<T, I>), dim3(blocks), dim3(256), 0, st, rv, cnt)
        MNK_N16G(3, 3); MNK_N16G(3, 2); MNK_N16G(3, 1);
        MNK_N16G(2, 3); MNK_N16G(2, 2); MNK_N16G(2, 1);
        MNK_N16G(1, 3); MNK_N16G(1, 2); MNK_N16G(1, 1);
#undef MNK_N16G
    }
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_wgrad_reduce_blocks(int splits, int Cout, int C) {
    if (splits <= 0 || Cout <= 0 || C <= 0) return 0;
    // (the flat map is taken for 3x3 / 4x4 kernels only; any other tap count still gets enough blocks from it: the tile map
    // needs ceil(Cout / 4) * ceil(C / 64) <= ceil(Cout * C / 1024))
    if (reduce_flat(splits, C)) {
        const long flat = ((long)Cout * (C >> 2) + 255) / 256, tile = (long)ceil_div(Cout, 4) * ceil_div(C, 64);
        return (int)(flat > tile ? flat : tile);
    }
    int tw, rows;
    reduce_map(splits, &tw, &rows);
    return ceil_div(Cout, rows) * ceil_div(C, tw);
}

int mnk_wgrad_reduce_map(int layout, int splits, int ntaps, int Cout, int C) {
    if (splits <= 0 || Cout <= 0 || C <= 0 || ntaps <= 0) return -1;
    return reduce_map_id(g_wgrad_reduce_vec != 0, layout, splits, ntaps, Cout, C);
}

int mnk_up1x1_live_mask(int dgrad) { return (int)up1x1_live_mask(dgrad != 0); }

int mnk_up1x1_dead_taps(int N, int Hs, int Ws) {
    return N > 0 && Hs > 0 && Ws > 0 && up1x1_skips(Hs, Ws, (long)N * Hs * Ws) ? 1 : 0;
}

int mnk_wgrad_reduce_multi(const MnkWgradReduceDesc* descs_device, int n, int total_blocks, void* stream) {
    MNK_REQUIRE(descs_device && n > 0 && total_blocks > 0);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(K_CONV_REDUCE, s, 0.0);
    hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(total_blocks), dim3(256), 0, s, descs_device, n, g_wgrad_reduce_vec != 0);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

size_t mnk_conv3x3_wgrad_workspace_floats(int N, int H, int W, int C, int Cout) {
    return mnk_conv2d_wgrad_workspace_floats(N, H, W, C, Cout, 3, 3, 1);
}
int mnk_conv3x3_wgrad(const float* x, int ld_x, int C, int flags, const float* dy, int ld_dy, int Cout, float* dw,
                      int Cin_total, int c_start, int N, int H, int W, float* ws, size_t ws_floats, void* stream) {
    return mnk_conv2d_wgrad(x, ld_x, C, flags, H, W, 3, 3, 1, dy, ld_dy, Cout, dw, Cin_total, c_start, N, H, W, ws, ws_floats,
                            stream);
}
}
