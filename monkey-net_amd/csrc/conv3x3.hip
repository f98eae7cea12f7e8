// 3x3 / pad 1 / stride 1 convolution on folded NHWC frames as an implicit GEMM on the gfx950 fp32 matrix
// cores (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD, 157 TFLOP/s chip peak).
//
// Replaces nn.Conv3d(kernel (1,3,3), padding (0,1,1)) of the reference (modules/util.py:52-55,79,98,176) in
// forward and data-gradient form (same kernel, flipped/transposed packed weights); the weight-gradient GEMMs are in
// conv3x3_wgrad.hip, what both files share in conv_common.h.
//
//   forward / dgrad GEMM:  Y[m][r] = sum_{chunk,tap,k} X[pix(m)+off(tap)][16*chunk+k] * W(r, 16*chunk+k, tap)
//       M = N*H*W pixels (rows, NHWC so channels are contiguous), N = output channels, K = 9 * (C0p + C1p).
//       K is walked chunk-major / tap-minor: the nine taps of one 16-channel chunk touch the same (halo of) pixel
//       rows and the same 36-byte (row, k) weight groups back to back, so both operands are re-read from L1.
//       The weights are re-packed per use to Wp[row][chunk][tap][16] (forward: row = co; data gradient: row = ci with
//       flipped taps), so a K step is one contiguous 64-byte read per row.  (Reading the parameter in place with
//       36-byte strides was measured 20 % slower: a 128 x 16 tile then spans 72 KB of cache lines per chunk.)
//       In LDS both operands are K-contiguous, so each lane fetches its MFMA fragment as one ds_read_b128:
//       lane (i = l&31, kk = l>>5) holds k = 8*kh + 4*kk + e (e = 0..3) of row i -- a permutation of K inside the
//       16-wide K step that is applied identically to A and B, hence harmless.
//
// Tiling: 256 threads = 4 waves; block tile BM x BN (128x128 default) staged through LDS in 16-deep K steps,
// double buffered with register prefetch (one barrier per step); wave tile = (BM/WM) x (BN/WN) as 32x32 MFMA
// tiles, i.e. 64 accumulator VGPRs for 64x64.  LDS rows are padded to 20 floats (80 B = 5 x 16 B, odd) so the
// 16-lane groups of a ds_read_b128 hit 16 distinct 16-B slots (no bank conflicts).
// Small problems (deep hourglass levels: 4x4 / 2x2 maps with 1024 channels) are split along K across blockIdx.z
// with a deterministic second-pass reduction (no atomics), which also applies bias and the residual add.
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <type_traits>

#include "conv_common.h"
#include "pack_tile.h"

using namespace mnk;

// shared with conv3x3_wgrad.hip (declared in conv_common.h): one slot each
int mnk::g_xcd_remap = tuning_knob("xcd_remap", &mnk::g_xcd_remap, 1);
int mnk::g_fast_loader = tuning_knob("fast_loader", &mnk::g_fast_loader, 1);

namespace {

__device__ __forceinline__ int round_up16(int v) { return (v + 15) & ~15; }

// The BatchNorm (+ activation) layer whose OUTPUT this launch's output is the gradient of (a data-gradient launch: dz of the
// layer in front).  With it the fused column sums of the epilogue are that layer's backward statistics
//     sum g,  sum g * xhat      g = act'((y - mean) * scale + beta) * dz,   xhat = (y - mean) * invstd
// (sync_batchnorm/batchnorm.py's backward through F.batch_norm; what colsum2_partial_kernel<BwdLoader> makes in a pass of its
// own over y and dz) instead of sum v, sum v^2 -- the tile of dz is in registers here, only y is read.  slope: < 0 no
// activation, 0 ReLU, > 0 LeakyReLU.  y == nullptr: plain statistics.
struct BnBwdSrc {
    const float* y;
    const float *mean, *invstd, *scale, *beta;
    int ld;
    float slope;
};

// The EVALUATION-mode norm layer (+ activation, + 2x2 average pool) behind a forward launch, applied in the launch's own epilogue
// (sync_batchnorm/batchnorm.py:50-53 with running statistics, behind modules/util.py:63-65,83-88,103-108): the store becomes
//     z = act_apply(fmaf(v - mean[co], scale[co], beta[co]), slope)        v = the value the plain launch stores (bn_apply1)
// and the convolution's own output never reaches memory.  mean / scale / beta: what mnk_bn_eval_coeffs makes; slope as in
// act_apply.  (z, ld_z): where the launch writes -- the launch's y / ld_y are set to the same pair; with pool they describe the
// (N, H/2, W/2) map and the kernel is a window-major instantiation (row_pixel).  Only the EN != 0 instantiations of the kernels
// read the record, and only an unsplit launch without residual, statistics and bnb takes one (conv2d_fwd_impl checks).
struct EvalNorm {
    const float *mean, *scale, *beta;
    float slope;
    float* z;
    int ld_z;
};

// The SECOND output of a pair launch (conv3x3_igemm_kernel<..., PAIR>): two GEMMs that read the same A operand with the same M, K,
// geometry and loader -- the data gradients of an up-sampled convolution w.r.t. its two sources [previous output | skip] -- in
// one grid.  Everything a launch's N side owns, with the plan the source has on its own (make_plan): weight pack, output, width
// and N tiles, split-K partials and split ranges, statistics.  A block takes these in place of ConvArgs' own fields when its
// N-tile index is past the first output's tiles and then runs the single launch's code: every output element keeps its bits.
struct ConvOut {
    const float* wp;
    float* y;
    int ld_y, Cout, gn;
    float* ws;
    int ldw, splits, ksteps_per_split;
    float* stats;
    BnBwdSrc bnb;
};

struct ConvArgs {
    const float* x0;
    const float* x1;
    int ld0, ld1, C0, C1, C0p, C1p;
    int ups;
    const float* wp;  // packed weights [rows][chunks][9][16]
    const float* bias;
    const float* residual;
    int ld_res;
    float* y;
    int ld_y;
    int N, H, W, Cout;   // output frames / height / width / channels
    int Hi, Wi;          // input height / width (before the optional x2 up-sampling view): H,W for 3x3 pad 1
    int ntaps, kw, pad;  // kernel taps (kh*kw), kernel width, zero padding (3x3: 9, 3, 1; discriminator 4x4: 16, 4, 0)
    long M;
    int chunks;        // (C0p + C1p) / 16
    int ksteps;        // ntaps * chunks, step s = chunk * ntaps + tap
    int ksteps_per_split;
    int splits;
    float* ws;         // [splits][M][ldw] partial sums when splits > 1
    int ldw;
    float* stats;      // optional [gridDim.x][2][ld_y]: per-block column sums / sums of squares of the written output
    int xcd;           // re-chunk the launch order per XCD (xcd_tile)
    int clean;         // the sources' pad channels [C, ld) hold zeros (finite values): the 3x3 fast loader may be used
    unsigned mulW, shW, mulH, shH;   // division of an output pixel index (< 2^31) by W and H (fast_div)
    // ---- K x K loader generalisations (ActLoaderK) ---------------------------------------------------------------
    int stride;        // input pixel of output (h, w), tap (ky, kx): (h * stride + ky - pad_y, w * stride + kx - pad_x)
    int pad_x;         // left padding (`pad` is the top padding); -1: same as `pad`
    // ---- sub-pixel ("phase") form of [nearest x2 up-sampling -> 3x3 / pad 1] (UpBlock3D, modules/util.py:83-85) -------
    // Output pixel (2i + a, 2j + b) only sees the 2 x 2 low-resolution neighbourhood rows {i + a - 1, i + a}, columns
    // {j + b - 1, j + b}, with weights that are sums of the 3x3 taps falling on the same input pixel: four 2x2
    // convolutions on the low-resolution input (one per phase (a, b)) instead of one 3x3 convolution on the 4x larger
    // up-sampled view -- 4 instead of 9 multiply-adds per output and channel pair, same result up to the rounding of the
    // pre-summed weights.  phases = 4: tile bx belongs to phase bx / tiles_per_phase; H, W, M are the LOW-resolution
    // geometry of one phase; the weights of phase p start at wp + p * phase_wstride; output rows are scattered to
    // (2i + a, 2j + b) of the (N, 2H, 2W) tensor.
    int phases, tiles_per_phase;
    long phase_wstride;
    BnBwdSrc bnb;
    // ---- position-major launches (the PM kernels; conv2d_fwd_impl decides) --------------------------------------------------
    unsigned mulF, shF;     // division of a GEMM row by the frame count N (fast_div)
    unsigned mulKW, shKW;   // division of a tap index by kw
    // ---- evaluation-mode norm layer in the epilogue (the EN = 1 / 2 kernels); window-major launches (EN = 2) -----------------
    EvalNorm en;
    unsigned mulWo, shWo, mulHo, shHo;   // division of a pool-window index by W / 2 and H / 2 (fast_div)
    // ---- pair launches (the PAIR kernels; up_dgrad_pair_impl decides) -------------------------------------------------------
    int gn0;           // N tiles of the first output: tile rows [gn0, gridDim.y) of the launch belong to `o1`
    ConvOut o1;
};

// GEMM row -> output pixel.  Frame-major (the memory order): m = (fr * H + h) * W + w -- 64 consecutive rows of a small map
// cover every position, so every tap is inside the source for SOME row of a tile.  Position-major: m = (h * W + w) * N + fr --
// the rows of a tile share one position (N >= BM) or BM / N neighbouring ones, and a tap that falls into the padding does so
// for the whole tile: the block leaves its K steps out (TapCursor).  Only the row <-> pixel map of the launch changes; every
// tensor, and the split-K workspace [split][phase][M][ldw], keeps its frame-major memory order.
// Window-major (RM = 2; H, W even): m = ((fr * H/2 + ho) * W/2 + wo) * 4 + 2 dy + dx is pixel (2 ho + dy, 2 wo + dx) -- four
// consecutive rows are one 2x2 pool window in the pooling kernels' order of additions, and the accumulator layouts keep four
// consecutive rows of a column in one lane: the epilogue of a launch with an EvalNorm pools in registers and writes row m / 4 of
// the pooled map (its frame-major order).
template <int RM>         // 0 frame-major, 1 position-major, 2 window-major (a bool PM converts to 0 / 1)
__device__ __forceinline__ void row_pixel(const ConvArgs& a, unsigned m, unsigned& fr, unsigned& h, unsigned& w) {
    if constexpr (RM == 2) {
        const unsigned q = m >> 2, tt = fast_div(q, a.mulWo, a.shWo);
        fr = fast_div(tt, a.mulHo, a.shHo);
        w = 2u * (q - tt * ((unsigned)a.W >> 1)) + (m & 1u);
        h = 2u * (tt - fr * ((unsigned)a.H >> 1)) + ((m >> 1) & 1u);
    } else if constexpr (RM == 1) {
        const unsigned p = fast_div(m, a.mulF, a.shF);
        fr = m - p * (unsigned)a.N;
        h = fast_div(p, a.mulW, a.shW);
        w = p - h * (unsigned)a.W;
    } else {
        const unsigned tt = fast_div(m, a.mulW, a.shW);
        fr = fast_div(tt, a.mulH, a.shH);
        w = m - tt * (unsigned)a.W;
        h = tt - fr * (unsigned)a.H;
    }
}

// K cursor of a tap-skipping block: walks the steps s = chunk * ntaps + tap whose tap bit is set in the block's mask (bit t: tap
// t lies inside the source for at least one row of the tile), in step order, without divisions: the next set bit above the
// current tap, or the lowest one of the next chunk.  Everything is wave-uniform (scalar registers).
// A skipped step would have multiplied activations that are exactly zero: fma(0, w, acc) = acc for finite w, and the order of
// the steps that remain, the split ranges and the two alternating accumulator sets are untouched -- every output keeps its
// value (up to the sign of a zero).  A NON-FINITE weight is the exception: it used to poison the rows whose tap is outside
// (0 * inf = NaN) and no longer does where the step is skipped.
struct TapCursor {
    unsigned mask;
    int chunk, tap;
    // first set step at or behind s (mask != 0)
    __device__ __forceinline__ void seek(unsigned mask_, int s, int ntaps) {
        mask = mask_;
        chunk = s / ntaps;
        const int t0 = s - chunk * ntaps;
        const unsigned rem = mask >> t0;
        tap = rem ? t0 + __builtin_ctz(rem) : __builtin_ctz(mask);
        chunk += rem ? 0 : 1;
    }
    __device__ __forceinline__ void next() {
        const unsigned rem = (mask >> tap) >> 1;
        tap = rem ? tap + 1 + __builtin_ctz(rem) : __builtin_ctz(mask);
        chunk += rem ? 0 : 1;
    }
    // set steps in [s0, s1)
    __device__ __forceinline__ static int count(unsigned mask, int s0, int s1, int ntaps) {
        const int c0 = s0 / ntaps, t0 = s0 - c0 * ntaps, c1 = s1 / ntaps, t1 = s1 - c1 * ntaps;
        return (c1 - c0) * __builtin_popcount(mask) + __builtin_popcount(mask & ((1u << t1) - 1u)) -
               __builtin_popcount(mask & ((1u << t0) - 1u));
    }
};

// ---- the activation-side loader of the implicit GEMM (shared by the 32x32 and 16x16 tile kernels) -------------------
// Everything a K step needs per row is precomputed (frame base, row / column, validity bit masks of the kernel rows
// and columns); the per-step gather is branch-free: a tap outside the image reads the clamped pixel and is zeroed on
// its way to LDS, rows beyond M are clamped to the last pixel (their results are never stored).  K-step cursor
// (step = chunk * ntaps + ky * kw + kx) advances without divisions or branches.
template <int RA, int NST = 1>      // NST: register stages (K steps in flight between their global loads and their LDS stores)
struct ActLoader {
    int prow[RA], ph[RA], pw[RA];
    unsigned pmask[RA];            // bits 0..7: kernel rows inside the image, bits 8..15: kernel columns
    float4 ra[NST][RA];
    int tail[NST][RA];             // real channels in ra[st][j] (<= 0: tap outside the image / chunk beyond C)
    int chunk, ky, kx, khh, Hs, Ws, hmax, wmax, lq;

    __device__ __forceinline__ void setup(const ConvArgs& a, long m0, int lrow, int lq_, int s_begin, int, int) {
        lq = lq_;
        Hs = a.ups ? a.Hi >> 1 : a.Hi;
        Ws = a.ups ? a.Wi >> 1 : a.Wi;
        khh = a.ntaps / a.kw;
        hmax = a.Hi - 1;
        wmax = a.Wi - 1;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            long ml = m0 + lrow + 64 * j;
            if (ml > a.M - 1) ml = a.M - 1;
            const unsigned m = (unsigned)ml, tt = fast_div(m, a.mulW, a.shW), fr = fast_div(tt, a.mulH, a.shH);
            pw[j] = (int)(m - tt * (unsigned)a.W);
            ph[j] = (int)(tt - fr * (unsigned)a.H);
            prow[j] = (int)fr * Hs * Ws;
            unsigned mk = 0;
            for (int y = 0; y < khh; ++y) {
                const int hh = ph[j] + y - a.pad;
                if (hh >= 0 && hh < a.Hi) mk |= 1u << y;
            }
            for (int x = 0; x < a.kw; ++x) {
                const int ww = pw[j] + x - a.pad;
                if (ww >= 0 && ww < a.Wi) mk |= 256u << x;
            }
            pmask[j] = mk;
#pragma unroll
            for (int st = 0; st < NST; ++st) tail[st][j] = 0;
        }
        chunk = s_begin / a.ntaps;
        ky = (s_begin - chunk * a.ntaps) / a.kw;
        kx = (s_begin - chunk * a.ntaps) - ky * a.kw;
    }
    // issue the global loads of the cursor's K step into register stage ST, then advance the cursor
    template <int ST = 0>
    __device__ __forceinline__ void load(const ConvArgs& a) {
        const int c0 = chunk * BK;
        const bool second = c0 >= a.C0p;
        const int cbase = second ? c0 - a.C0p : c0;
        const float* src = second ? a.x1 : a.x0;
        const int ld = second ? a.ld1 : a.ld0, C = second ? a.C1 : a.C0;
        const int ch = cbase + lq * 4;
        const int tl = C - ch;
        const int che = tl > 0 ? ch : 0;
        const int dy = ky - a.pad, dx = kx - a.pad;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const bool ok = (pmask[j] >> ky) & (pmask[j] >> (8 + kx)) & 1u;
            int hh = ph[j] + dy, ww = pw[j] + dx;     // clamped into the image: the load is unconditional
            hh = hh < 0 ? 0 : (hh > hmax ? hmax : hh);
            ww = ww < 0 ? 0 : (ww > wmax ? wmax : ww);
            const unsigned off = (unsigned)(prow[j] + (hh >> a.ups) * Ws + (ww >> a.ups)) * (unsigned)ld + (unsigned)che;
            ra[ST][j] = *reinterpret_cast<const float4*>(src + off);
            tail[ST][j] = ok ? tl : 0;
        }
        const int kx1 = kx + 1;
        const bool wx = kx1 == a.kw;
        kx = wx ? 0 : kx1;
        const int ky1 = ky + (wx ? 1 : 0);
        const bool wy = ky1 == khh;
        ky = wy ? 0 : ky1;
        chunk += wy ? 1 : 0;
    }
    // row j on its way to LDS: pad channels of the producer may hold anything, taps outside the image are zero
    template <int ST = 0>
    __device__ __forceinline__ float4 masked(int j) const {
        float4 v = ra[ST][j];
        v.x = tail[ST][j] < 1 ? 0.f : v.x;
        v.y = tail[ST][j] < 2 ? 0.f : v.y;
        v.z = tail[ST][j] < 3 ? 0.f : v.z;
        v.w = tail[ST][j] < 4 ? 0.f : v.w;
        return v;
    }
};

// ---- the same loader for the hot case (3x3, pad 1, sources with clean pad channels) with the fewest instructions per
// K step -- every vector instruction between two MFMAs costs matrix-pipe time on this hardware (profiles/README.md:
// dropping only the data masks of the generic loader was worth +9 %).  Raw buffer loads relative to a per-block base
// (offsets stay far below 2^30; num_records = 2^30): an out-of-image tap or a chunk beyond the channel count gets bit
// 30 added to its offset and the hardware returns zeros -- no clamping, no data masks, no branches.  Per row and step:
// one add, one bit-field extract, one and-or (+ five for the parity shifts of the nearest x2 up-sampling view).
// PM: the rows are position-major (row_pixel) and the K cursor is `cur`, which the kernel points at the block's first step
// (TapCursor).  The rows of such a tile lie a whole frame apart, so the buffer window starts at the tensor (the host checks
// that the sources fit it).
// WIN: the rows are window-major (row_pixel): per-row base offsets and out-of-image masks follow the map, the K loop does not
// care.  A tile's rows are the pool windows from its first one on in frame-major window order, so the lowest pixel row a tile
// touches is the upper row of its first window.
template <int RA, bool UPS, int NST = 1, bool PM = false, bool WIN = false>
struct ActLoader3 {
    static_assert(!WIN || (!UPS && !PM), "window-major rows: the plain 3x3 loader, frame order of the windows");
    unsigned b0[RA], b1[RA];       // byte offset of the row's centre pixel in source 0 / 1 (relative to the block base)
    unsigned inv[RA];              // bit t: tap t lies outside the image
    unsigned par[RA];              // up-sampling: bit 0 h even, 1 h odd, 2 w even, 3 w odd (bit 4 stays 0)
    float4 ra[NST][RA];
    __amdgpu_buffer_rsrc_t r0, r1;
    int chunk, ky, kx, Ws, lq4;
    TapCursor cur;

    // taps that are outside for EVERY row this thread loads
    __device__ __forceinline__ unsigned inv_all() const {
        unsigned v = inv[0];
#pragma unroll
        for (int j = 1; j < RA; ++j) v &= inv[j];
        return v;
    }

    __device__ __forceinline__ void setup(const ConvArgs& a, long m0, int lrow, int lq_, int s_begin, int, int) {
        lq4 = lq_ * 16;
        const int Hs = UPS ? a.Hi >> 1 : a.Hi;
        Ws = UPS ? a.Wi >> 1 : a.Wi;
        long pbase = 0;            // position-major: the window starts at the tensor
        if constexpr (!PM) {
            const unsigned mb = (unsigned)(m0 < a.M ? m0 : a.M - 1);
            unsigned fb, hb, wb;
            row_pixel<WIN ? 2 : 0>(a, mb, fb, hb, wb);
            if constexpr (WIN) hb &= ~1u;
            const long rowidx0 = (long)fb * Hs + ((int)hb >> (UPS ? 1 : 0));
            pbase = rowidx0 * Ws - Ws - 1;
            if (pbase < 0) pbase = 0;
        }
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x0 + pbase * a.ld0), 0, 0x40000000, 0x00020000);
        r1 = __builtin_amdgcn_make_buffer_rsrc((void*)((a.x1 ? a.x1 : a.x0) + pbase * (a.x1 ? a.ld1 : a.ld0)), 0, 0x40000000,
                                               0x00020000);
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            long ml = m0 + lrow + 64 * j;
            if (ml > a.M - 1) ml = a.M - 1;
            unsigned fr, hu, wu;
            row_pixel<WIN ? 2 : (PM ? 1 : 0)>(a, (unsigned)ml, fr, hu, wu);
            const int w = (int)wu, h = (int)hu;
            const long rel = ((long)fr * Hs + (h >> (UPS ? 1 : 0))) * Ws + (w >> (UPS ? 1 : 0)) - pbase;
            b0[j] = (unsigned)(rel * a.ld0 * 4);
            b1[j] = (unsigned)(rel * a.ld1 * 4);
            unsigned mk = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
                if (hh < 0 || hh >= a.Hi || ww < 0 || ww >= a.Wi) mk |= 1u << t;
            }
            inv[j] = mk;
            par[j] = ((h & 1) ? 2u : 1u) | ((w & 1) ? 8u : 4u);
        }
        if constexpr (PM) return;
        chunk = s_begin / 9;
        ky = (s_begin - chunk * 9) / 3;
        kx = (s_begin - chunk * 9) - ky * 3;
    }
    template <int ST = 0>
    __device__ __forceinline__ void load(const ConvArgs& a) {
        if constexpr (PM) {
            chunk = cur.chunk;
            ky = (cur.tap * 11) >> 5;      // tap / 3 for tap < 9
            kx = cur.tap - 3 * ky;
        }
        const int c0 = chunk * BK;
        const bool second = c0 >= a.C0p;
        const int cbase = second ? c0 - a.C0p : c0;
        const int ldb = (second ? a.ld1 : a.ld0) * 4, C = second ? a.C1 : a.C0;
        const __amdgpu_buffer_rsrc_t rs = second ? r1 : r0;
        const int tap = ky * 3 + kx;
        // per thread: channel offset, + bit 30 when the whole float4 lies beyond the channel count
        unsigned st = (unsigned)(cbase * 4 + lq4);
        st += (cbase * 4 + lq4 >= C * 4) ? 0x40000000u : 0u;
        int s_dr = 0, s_dc = 0, rbit = 4, cbit = 4;
        if (UPS) {
            s_dr = ky == 0 ? -Ws * ldb : (ky == 2 ? Ws * ldb : 0);
            s_dc = kx == 0 ? -ldb : (kx == 2 ? ldb : 0);
            rbit = ky == 0 ? 0 : (ky == 2 ? 1 : 4);
            cbit = kx == 0 ? 2 : (kx == 2 ? 3 : 4);
        } else {
            st += (unsigned)(((ky - 1) * Ws + (kx - 1)) * ldb);
        }
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            unsigned off = (second ? b1[j] : b0[j]) + st;
            if (UPS) {
                const int nr = __builtin_amdgcn_sbfe(par[j], rbit, 1), nc = __builtin_amdgcn_sbfe(par[j], cbit, 1);
                off += (unsigned)(nr & s_dr) + (unsigned)(nc & s_dc);
            }
            const int bad = __builtin_amdgcn_sbfe(inv[j], tap, 1);            // 0 or -1
            off = ((unsigned)bad & 0x40000000u) | off;
            ra[ST][j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
        if constexpr (PM) {
            cur.next();
            return;
        }
        const int kx1 = kx + 1;
        const bool wx = kx1 == 3;
        kx = wx ? 0 : kx1;
        const int ky1 = ky + (wx ? 1 : 0);
        const bool wy = ky1 == 3;
        ky = wy ? 0 : ky1;
        chunk += wy ? 1 : 0;
    }
    template <int ST = 0>
    __device__ __forceinline__ float4 masked(int j) const { return ra[ST][j]; }
};

// ---- the same idea for any K x K kernel with stride 1 and padding `pad` (the discriminator's 4x4 / pad 0 forward and its
// pad 3 data gradient), sources with clean pad channels, no up-sampled view: per-row base offset + one validity bit per
// tap (K*K <= 32); an out-of-image tap or a channel chunk beyond C reads zeros through the buffer range check.
template <int RA, int NST = 1, bool PM = false>       // PM: see ActLoader3
struct ActLoaderK {
    unsigned b0[RA], b1[RA];       // byte offset of input pixel (h * stride, w * stride) -- tap (pad_y, pad_x) -- relative to the
                                   // block base; may lie outside the image (pad > 0): it is only a base for the tap arithmetic
    unsigned inv[RA];              // bit ky * kw + kx: the tap lies outside the image
    float4 ra[NST][RA];
    __amdgpu_buffer_rsrc_t r0, r1;
    int chunk, ky, kx, khh, lq4, pady, padx;
    TapCursor cur;

    __device__ __forceinline__ unsigned inv_all() const {
        unsigned v = inv[0];
#pragma unroll
        for (int j = 1; j < RA; ++j) v &= inv[j];
        return v;
    }

    __device__ __forceinline__ void setup(const ConvArgs& a, long m0, int lrow, int lq_, int s_begin, int pad_y, int pad_x) {
        lq4 = lq_ * 16;
        khh = a.ntaps / a.kw;
        pady = pad_y;
        padx = pad_x;
        const int sd = a.stride;
        long pbase = 0;            // position-major: the window starts at the tensor
        if constexpr (!PM) {
            const unsigned mb = (unsigned)(m0 < a.M ? m0 : a.M - 1), tb = fast_div(mb, a.mulW, a.shW),
                           fb = fast_div(tb, a.mulH, a.shH);
            // lowest address a valid tap of this block can have: input pixel (h0 * stride - pad_y, -pad_x) of the first row's frame
            pbase = ((long)fb * a.Hi + (int)(tb - fb * (unsigned)a.H) * sd - pad_y) * a.Wi - pad_x;
            if (pbase < 0) pbase = 0;
        }
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x0 + pbase * a.ld0), 0, 0x40000000, 0x00020000);
        r1 = __builtin_amdgcn_make_buffer_rsrc((void*)((a.x1 ? a.x1 : a.x0) + pbase * (a.x1 ? a.ld1 : a.ld0)), 0, 0x40000000,
                                               0x00020000);
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            long ml = m0 + lrow + 64 * j;
            if (ml > a.M - 1) ml = a.M - 1;
            unsigned fr, hu, wu;
            row_pixel<PM>(a, (unsigned)ml, fr, hu, wu);
            const int w = (int)wu * sd, h = (int)hu * sd;
            const long rel = ((long)fr * a.Hi + h) * a.Wi + w - pbase;
            b0[j] = (unsigned)(rel * a.ld0 * 4);
            b1[j] = (unsigned)(rel * a.ld1 * 4);
            unsigned mk = 0, bit = 1;
            for (int y = 0; y < khh; ++y) {
                const int hh = h + y - pad_y;
                const bool rowbad = hh < 0 || hh >= a.Hi;
                for (int x = 0; x < a.kw; ++x, bit <<= 1) {
                    const int ww = w + x - pad_x;
                    if (rowbad || ww < 0 || ww >= a.Wi) mk |= bit;
                }
            }
            inv[j] = mk;
        }
        if constexpr (PM) return;
        chunk = s_begin / a.ntaps;
        ky = (s_begin - chunk * a.ntaps) / a.kw;
        kx = (s_begin - chunk * a.ntaps) - ky * a.kw;
    }
    template <int ST = 0>
    __device__ __forceinline__ void load(const ConvArgs& a) {
        if constexpr (PM) {
            chunk = cur.chunk;
            ky = (int)fast_div((unsigned)cur.tap, a.mulKW, a.shKW);
            kx = cur.tap - ky * a.kw;
        }
        const int c0 = chunk * BK;
        const bool second = c0 >= a.C0p;
        const int cbase = second ? c0 - a.C0p : c0;
        const int ldb = (second ? a.ld1 : a.ld0) * 4, C = second ? a.C1 : a.C0;
        const __amdgpu_buffer_rsrc_t rs = second ? r1 : r0;
        const int tap = ky * a.kw + kx;
        unsigned st = (unsigned)(cbase * 4 + lq4);
        st += (cbase * 4 + lq4 >= C * 4) ? 0x40000000u : 0u;
        st += (unsigned)(((ky - pady) * a.Wi + (kx - padx)) * ldb);
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            unsigned off = (second ? b1[j] : b0[j]) + st;
            const int bad = __builtin_amdgcn_sbfe(inv[j], tap, 1);            // 0 or -1
            off = ((unsigned)bad & 0x40000000u) | off;
            ra[ST][j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
        if constexpr (PM) {
            cur.next();
            return;
        }
        const int kx1 = kx + 1;
        const bool wx = kx1 == a.kw;
        kx = wx ? 0 : kx1;
        const int ky1 = ky + (wx ? 1 : 0);
        const bool wy = ky1 == khh;
        ky = wy ? 0 : ky1;
        chunk += wy ? 1 : 0;
    }
    template <int ST = 0>
    __device__ __forceinline__ float4 masked(int j) const { return ra[ST][j]; }
};

template <int RA, int MODE, int NST = 1, bool PM = false, bool WIN = false> struct LoaderSel { typedef ActLoader<RA, NST> type; };
template <int RA, int NST, bool PM, bool WIN> struct LoaderSel<RA, 3, NST, PM, WIN> { typedef ActLoaderK<RA, NST, PM> type; };
template <int RA, int NST, bool PM, bool WIN> struct LoaderSel<RA, 1, NST, PM, WIN> { typedef ActLoader3<RA, false, NST, PM, WIN> type; };
template <int RA, int NST, bool PM, bool WIN> struct LoaderSel<RA, 2, NST, PM, WIN> { typedef ActLoader3<RA, true, NST, PM> type; };

#ifndef MNK_IGEMM_OCC
#define MNK_IGEMM_OCC 3                       // waves per SIMD = blocks per CU the register budget is held to
#endif
#ifndef MNK_IGEMM_NACC
#define MNK_IGEMM_NACC 2                      // accumulator sets of a one-tile wave (64x64 / 128x32 block tiles)
#endif
#ifndef MNK_IGEMM_NST
#define MNK_IGEMM_NST 2                       // register stages: K steps between a step's global loads and its LDS stores
#endif

// -DMNK_PHASE_CLOCKS (an experiment build, tools/phase_probe.py): thread 0 of every block of the 32x32-tile kernel stamps the
// 100 MHz wall clock at its entry, in front of its K loop, behind it and at its exit
#ifdef MNK_PHASE_CLOCKS
__device__ unsigned long long mnk_phase_log[4 * 16384];
__device__ unsigned long long mnk_phase_sclk[2 * 16384];      // the shader clock (s_memtime) in front of / behind the K loop
#define MNK_PHASE(i)                                                                                              \
    do {                                                                                                          \
        const unsigned lin__ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                    \
        if (threadIdx.x == 0 && lin__ < 16384u) {                                                                 \
            mnk_phase_log[4 * lin__ + (i)] = wall_clock64();                                                      \
            if ((i) == 1 || (i) == 2) mnk_phase_sclk[2 * lin__ + (i) - 1] = clock64();                            \
        }                                                                                                         \
    } while (0)
#else
#define MNK_PHASE(i) ((void)0)
#endif

constexpr int LDS_H = 24;     // padded LDS row of the bf16 planes (16 + 8 halves = 48 bytes: conflict-free b128 fragment reads)

// GM: 0 -- v_mfma_f32_32x32x2_f32 on fp32 tiles; 1 -- the same products on the bf16 matrix cores: the loaders split every fp32
// operand into three bf16 planes on its way to LDS and a K step of 16 is six v_mfma_f32_32x32x16_bf16 per tile (mnk_common.h);
// 2 -- the one-pass form (MNK_CONV_BF16): the loaders round every fp32 operand to ONE bf16 plane (nearest even) and a K step is
// one v_mfma_f32_32x32x16_bf16 per tile; fp32 accumulation, and everything behind the accumulator is the fp32 epilogue
// PM: position-major rows + block-uniform tap skipping (row_pixel, TapCursor): fast loaders and fp32 products only, and only
// launches whose epilogue leaves no per-block column sums -- those are fp32 sums over the rows of a tile, and another row
// order would change their bits
// EN: the launch has an EvalNorm -- 1: applied per element (any row map; the buffer-load loaders); 2: with the 2x2 average pool, on
// window-major rows (row_pixel): the plain 3x3 fast loader, and the epilogue writes the pooled map.  A template parameter, not a
// test of a.en: the training instantiations (EN = 0) stay the code they were (profiles/eval_norm_fused.txt, section 2)
// PAIR: the launch has two outputs (ConvOut): grid y covers the N tiles of both, grid z the larger split count.  A block picks
// its output once, from its N-tile index (block-uniform), leaves at once when its split is past that output's count, and is
// then a block of the single launch.  A template parameter like EN: the other instantiations stay the code they were
template <int BM, int BN, int WM, int WN, int MODE, int GM = 0, bool PM = false, int EN = 0, bool PAIR = false>     // MODE: 0 generic loader, 1 / 2 the 3x3 fast loader (plain / x2 up-sampled)
__global__ void __launch_bounds__(256, MNK_IGEMM_OCC) conv3x3_igemm_kernel(ConvArgs a_in) {
    static_assert(!PAIR || (MODE == 3 && GM == 0 && EN == 0), "pair launches: the K x K buffer loader, fp32 products");
    ConvArgs a_own;                           // PAIR: the block's own view of the launch
    const ConvArgs& a = PAIR ? a_own : a_in;
    if constexpr (PAIR) a_own = a_in;
    static_assert(!PM || (MODE != 0 && GM == 0), "position-major rows: buffer-load loaders, fp32 products");
    constexpr bool WIN = EN == 2;
    static_assert(!WIN || (MODE == 1 && !PM), "window-major rows: the plain 3x3 fast loader");
    static_assert(EN == 0 || MODE != 0, "an EvalNorm launch: buffer-load loaders");
    MNK_PHASE(0);
    constexpr int RA = BM / 64;               // A rows per thread per K step
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    // A wave that owns ONE 32x32 tile would run all its MFMAs as one dependent chain on one accumulator: an MFMA that follows
    // its predecessor on the same accumulator with other instructions in between waits for the write-back (the back-to-back
    // forwarding path only serves adjacent issues), and the loop has loads, LDS traffic and address arithmetic between every
    // pair.  Two accumulator sets fed by alternating K elements make neighbours independent; they are added once at the end
    // (which also halves the length of the fp32 summation chain: K = 9 * Cin <= 18 522 terms).
    constexpr int NACC = (TM * TN == 1) ? MNK_IGEMM_NACC : 1;
    // 8 (16) registers per stage; the 128x128 tile has none to spare, and the bf16x3 form measured 0.05 ms per iteration
    // faster with one stage (profiles/r06_knob_ab_log.txt, v16): its six MFMAs per K step already cover the load latency
    // (the one-pass form, GM = 2, takes the fp32 rule: its one MFMA per tile covers even less latency, and two stages spill at 128x128)
    constexpr int NST = (BM * BN <= 64 * 128 && GM != 1) ? MNK_IGEMM_NST : 1;
    static_assert(WM * WN == 4, "4 waves per block");
    static_assert(NST == 1 || NST == 2, "one or two register stages");
    // one LDS image, three views: fp32 rows [2][rows][LDS_K] (GM 0) / three bf16 planes [2][3][rows][LDS_H] (GM 1) / one bf16
    // plane [2][rows][LDS_H] (GM 2)
    constexpr int NPL = GM == 2 ? 1 : 3;
    constexpr int A_BYTES = GM ? 2 * NPL * BM * LDS_H * 2 : 2 * BM * LDS_K * 4, B_BYTES = GM ? 2 * NPL * BN * LDS_H * 2 : 2 * BN * LDS_K * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem_a[A_BYTES], smem_b[B_BYTES];
    float (*const As)[BM][LDS_K] = reinterpret_cast<float (*)[BM][LDS_K]>(smem_a);
    float (*const Bs)[BN][LDS_K] = reinterpret_cast<float (*)[BN][LDS_K]>(smem_b);
    unsigned short (*const Ah)[3][BM][LDS_H] = reinterpret_cast<unsigned short (*)[3][BM][LDS_H]>(smem_a);
    unsigned short (*const Bh)[3][BN][LDS_H] = reinterpret_cast<unsigned short (*)[3][BN][LDS_H]>(smem_b);
    unsigned short (*const Ao)[BM][LDS_H] = reinterpret_cast<unsigned short (*)[BM][LDS_H]>(smem_a);
    unsigned short (*const Bo)[BN][LDS_H] = reinterpret_cast<unsigned short (*)[BN][LDS_H]>(smem_b);

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int bx, by;
    xcd_tile(a.xcd, bx, by);
    if constexpr (PAIR) {
        if (by >= a_in.gn0) {                 // block-uniform: a tile of the second output
            by -= a_in.gn0;
            a_own.wp = a_in.o1.wp;
            a_own.y = a_in.o1.y;
            a_own.ld_y = a_in.o1.ld_y;
            a_own.Cout = a_in.o1.Cout;
            a_own.ws = a_in.o1.ws;
            a_own.ldw = a_in.o1.ldw;
            a_own.splits = a_in.o1.splits;
            a_own.ksteps_per_split = a_in.o1.ksteps_per_split;
            a_own.stats = a_in.o1.stats;
            a_own.bnb = a_in.o1.bnb;
        }
        if ((int)blockIdx.z >= a_own.splits) return;      // grid z is the larger split count of the two
    }
    // sub-pixel form: the M tiles of phase (pa, pb) are [phase * tiles_per_phase, ...); each phase has its own weights
    // and its own top / left padding (rows i + pa - 1, i + pa of the low-resolution input)
    const int phase = a.phases > 1 ? bx / a.tiles_per_phase : 0;
    const int pa = phase >> 1, pb = phase & 1;
    const long m0 = (long)(bx - phase * a.tiles_per_phase) * BM;
    const int n0 = by * BN;
    const int split = blockIdx.z;
    const int s_begin = split * a.ksteps_per_split;
    int s_end = s_begin + a.ksteps_per_split;
    if (s_end > a.ksteps) s_end = a.ksteps;
    const float* const wpb = a.wp + (long)phase * a.phase_wstride;

    // ---- per-thread global->LDS assignment: row inside a 64-row slab, float4 column (4 channels) --------------
    const int lrow = t >> 2, lq = t & 3;
    typename LoaderSel<RA, MODE, NST, PM, WIN>::type L;
    L.setup(a, m0, lrow, lq, s_begin, a.pad - pa, (a.pad_x < 0 ? a.pad : a.pad_x) - pb);
    int n = s_end - s_begin;                  // K steps of this block
    if constexpr (PM) {
        // the tile's tap mask: a tap is skipped when it is outside for every row of every thread (rows beyond M repeat row M - 1)
        __shared__ unsigned tap_red[4];
        unsigned v = L.inv_all();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v &= __shfl_xor(v, o);
        if (lane == 0) tap_red[wave] = v;
        __syncthreads();
        v = tap_red[0] & tap_red[1] & tap_red[2] & tap_red[3];
        const unsigned all_taps = a.ntaps >= 32 ? ~0u : (1u << a.ntaps) - 1u;
        const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((int)(~v & all_taps));
        n = mask ? TapCursor::count(mask, s_begin, s_end, a.ntaps) : 0;
        if (n > 0) L.cur.seek(mask, s_begin, a.ntaps);
    }
    constexpr int RB = (BN + 63) / 64;        // B rows per thread per K step
    const long KT = (long)a.ksteps * BK;     // packed row length
    static_assert(RB <= 2, "at most two weight rows per thread");
    const int wco0 = n0 + lrow, wco1 = n0 + lrow + 64;    // rows beyond Cout: clamped, never stored
    const unsigned woff0 = (unsigned)((wco0 < a.Cout ? wco0 : a.Cout - 1) * KT) + lq * 4;
    const unsigned woff1 = (unsigned)((wco1 < a.Cout ? wco1 : a.Cout - 1) * KT) + lq * 4;
    float4 rb0a, rb0b, rb1a, rb1b;            // weight rows of register stage 0 (a) / 1 (b): scalars, not arrays -- an array
                                              // captured by the lambdas below ends up in scratch memory

    // global loads of K step s into register stage ST (the activation loader keeps its own cursor: steps in order)
    auto load_step = [&](int s, auto st_tag) __attribute__((always_inline)) {
        constexpr int ST = decltype(st_tag)::value;
        if constexpr (PM) s = L.cur.chunk * a.ntaps + L.cur.tap;      // the cursor's step: the steps in between are skipped
        L.template load<ST>(a);
        const float* wsrc_ptr = wpb + (long)s * BK;
        if constexpr (ST == 0) {
            rb0a = *reinterpret_cast<const float4*>(wsrc_ptr + woff0);
            if constexpr (RB > 1) rb1a = *reinterpret_cast<const float4*>(wsrc_ptr + woff1);
        } else {
            rb0b = *reinterpret_cast<const float4*>(wsrc_ptr + woff0);
            if constexpr (RB > 1) rb1b = *reinterpret_cast<const float4*>(wsrc_ptr + woff1);
        }
    };
    auto store_step = [&](int buf, auto st_tag) __attribute__((always_inline)) {
        constexpr int ST = decltype(st_tag)::value;
        if constexpr (GM == 0) {
#pragma unroll
            for (int j = 0; j < RA; ++j) *reinterpret_cast<float4*>(&As[buf][lrow + 64 * j][lq * 4]) = L.template masked<ST>(j);
            if (BN >= 64 || lrow < BN) *reinterpret_cast<float4*>(&Bs[buf][lrow][lq * 4]) = ST == 0 ? rb0a : rb0b;
            if constexpr (RB > 1) *reinterpret_cast<float4*>(&Bs[buf][lrow + 64][lq * 4]) = ST == 0 ? rb1a : rb1b;
        } else if constexpr (GM == 2) {
#pragma unroll
            for (int j = 0; j < RA; ++j)
                *reinterpret_cast<uint2*>(&Ao[buf][lrow + 64 * j][lq * 4]) = mnk_round_bf16x4(L.template masked<ST>(j));
            if (BN >= 64 || lrow < BN) *reinterpret_cast<uint2*>(&Bo[buf][lrow][lq * 4]) = mnk_round_bf16x4(ST == 0 ? rb0a : rb0b);
            if constexpr (RB > 1) *reinterpret_cast<uint2*>(&Bo[buf][lrow + 64][lq * 4]) = mnk_round_bf16x4(ST == 0 ? rb1a : rb1b);
        } else {
            uint2 p0, p1, p2;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                mnk_split3(L.template masked<ST>(j), p0, p1, p2);
                *reinterpret_cast<uint2*>(&Ah[buf][0][lrow + 64 * j][lq * 4]) = p0;
                *reinterpret_cast<uint2*>(&Ah[buf][1][lrow + 64 * j][lq * 4]) = p1;
                *reinterpret_cast<uint2*>(&Ah[buf][2][lrow + 64 * j][lq * 4]) = p2;
            }
            if (BN >= 64 || lrow < BN) {
                mnk_split3(ST == 0 ? rb0a : rb0b, p0, p1, p2);
                *reinterpret_cast<uint2*>(&Bh[buf][0][lrow][lq * 4]) = p0;
                *reinterpret_cast<uint2*>(&Bh[buf][1][lrow][lq * 4]) = p1;
                *reinterpret_cast<uint2*>(&Bh[buf][2][lrow][lq * 4]) = p2;
            }
            if constexpr (RB > 1) {
                mnk_split3(ST == 0 ? rb1a : rb1b, p0, p1, p2);
                *reinterpret_cast<uint2*>(&Bh[buf][0][lrow + 64][lq * 4]) = p0;
                *reinterpret_cast<uint2*>(&Bh[buf][1][lrow + 64][lq * 4]) = p1;
                *reinterpret_cast<uint2*>(&Bh[buf][2][lrow + 64][lq * 4]) = p2;
            }
        }
    };

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
    const int a_row0 = wm * (BM / WM) + fi, b_row0 = wn * (BN / WN) + fi;

    auto mfma_step = [&](int buf) __attribute__((always_inline)) {
        if constexpr (GM == 2) {
            // lane (fi, fk) holds k = 8 fk .. 8 fk + 7 of its row: one b128 per operand row, one MFMA per tile
            mnk_bf16x8 ha[TM], hb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) ha[i] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Ao[buf][a_row0 + 32 * i][fk * 8]));
#pragma unroll
            for (int j = 0; j < TN; ++j) hb[j] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Bo[buf][b_row0 + 32 * j][fk * 8]));
            if constexpr (NACC == 2) {
                // a one-tile wave: even K steps (LDS buffer 0) feed one accumulator set, odd ones the other -- neighbours independent
                if (buf) acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0], hb[0], acc[1][0][0], 0, 0, 0);
                else acc[0][0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0], hb[0], acc[0][0][0], 0, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[i], hb[j], acc[0][i][j], 0, 0, 0);
            }
            return;
        }
        if constexpr (GM == 1) {
            // lane (fi, fk) holds k = 8 fk .. 8 fk + 7 of its row in every plane: one b128 per plane and operand row
            mnk_bf16x8 ha[3][TM], hb[3][TN];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    ha[pl][i] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Ah[buf][pl][a_row0 + 32 * i][fk * 8]));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    hb[pl][j] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Bh[buf][pl][b_row0 + 32 * j][fk * 8]));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    constexpr int Q = NACC - 1;       // (two accumulator sets of a one-tile wave: neighbours independent)
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[1][i], hb[1][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[2][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[2][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[1][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[1][j], acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[0][i], hb[0][j], acc[Q][i][j], 0, 0, 0);
                }
            return;
        }
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            float4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                fa[i] = *reinterpret_cast<const float4*>(&As[buf][a_row0 + 32 * i][kh * 8 + fk * 4]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                fb[j] = *reinterpret_cast<const float4*>(&Bs[buf][b_row0 + 32 * j][kh * 8 + fk * 4]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    constexpr int Q = NACC - 1;
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[Q][i][j], 0, 0, 0);
                    acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[0][i][j], 0, 0, 0);
                    acc[Q][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[Q][i][j], 0, 0, 0);
                }
        }
    };
    using St0 = std::integral_constant<int, 0>;
    using St1 = std::integral_constant<int, NST - 1>;

    // Pipeline.  K step t (relative to s_begin) travels in register stage t % NST and lands in LDS buffer t & 1.
    //   NST = 1: the registers always hold the step after the one in LDS.  In step s the wave parks step s+1 in the other
    //            LDS buffer (loaded a whole step ago), issues the global loads of step s+2 and then runs the MFMAs of step s.
    //   NST = 2: two steps are in flight in registers: step s parks step s+1, issues the loads of step s+3 into the stage
    //            that store just freed, runs the MFMAs of step s -- a load has two whole steps to arrive (one step of eight
    //            MFMAs does not cover an HBM miss when few waves share the SIMD).
    // Loads, address arithmetic and LDS writes sit in the MFMA shadow; one barrier per step; the steady-state loop body is
    // branch-free (two steps per trip: LDS buffer and register stage are compile-time constants); the tail is peeled.
    // (Two steps per barrier -- four LDS buffers, half the barriers -- was built and measured in round 3: the per-layer
    // bench unchanged, the whole step 10.90 vs 10.79 ms with 40 KB of LDS per block: removed.  profiles/r03_knob_ab_log.txt)
    if (n > 0) {
        load_step(s_begin, St0{});
        store_step(0, St0{});
        if (n > 1) load_step(s_begin + 1, St1{});
        if (NST == 2 && n > 2) load_step(s_begin + 2, St0{});
    }
    if (NST == 2) MNK_WAIT_VMEM();            // exact wait counts inside the loop (see the macro)
    __syncthreads();
    MNK_PHASE(1);
    int s = 0;
    if constexpr (NST == 2) {
        for (; s + 4 < n; s += 2) {
            store_step(1, St1{});
            load_step(s_begin + s + 3, St1{});
            mfma_step(0);
            __syncthreads();
            store_step(0, St0{});
            load_step(s_begin + s + 4, St0{});
            mfma_step(1);
            __syncthreads();
        }
        for (; s < n; ++s) {                  // at most four steps (s is even here)
            if ((s & 1) == 0) {
                if (s + 1 < n) store_step(1, St1{});
                if (s + 3 < n) load_step(s_begin + s + 3, St1{});
                mfma_step(0);
            } else {
                if (s + 1 < n) store_step(0, St0{});
                if (s + 3 < n) load_step(s_begin + s + 3, St0{});
                mfma_step(1);
            }
            __syncthreads();
        }
    } else {
        for (; s + 3 < n; s += 2) {
            store_step(1, St0{});
            load_step(s_begin + s + 2, St0{});
            mfma_step(0);
            __syncthreads();
            store_step(0, St0{});
            load_step(s_begin + s + 3, St0{});
            mfma_step(1);
            __syncthreads();
        }
        for (; s < n; ++s) {
            if (s + 1 < n) store_step((s & 1) ^ 1, St0{});
            if (s + 2 < n) load_step(s_begin + s + 2, St0{});
            mfma_step(s & 1);
            __syncthreads();                  // (the last one: the epilogue reuses As for the column sums)
        }
    }
    MNK_PHASE(2);
    if constexpr (NACC == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][0][r] += acc[1][0][0][r];
    }

    // ---- epilogue: D[row][col], col = lane&31 (-> co), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (-> pixel) ------
    // bias is fetched once per column, residual values are fetched as a batch before the stores (no per-element
    // load -> wait -> store chains), stores are predicated.
    const bool split_out = a.splits > 1;
    const unsigned ldo = split_out ? (unsigned)a.ldw : (unsigned)a.ld_y;          // 32-bit element offsets (host check)
    // split partials of the sub-pixel form are phase-major: [split][phase][M][ldw]
    float* const obase = split_out ? a.ws + ((long)split * a.phases + phase) * a.M * a.ldw : a.y;
    const int co_lim = split_out ? a.ldw : a.ld_y;
    const bool use_res = !split_out && a.residual;
    const bool full = m0 + BM <= a.M;             // every row of the tile is a real pixel: no per-row guards
    const unsigned mrow0 = (unsigned)m0 + wm * (BM / WM) + 4 * fk, Mu = (unsigned)a.M;
    const bool scatter = a.phases > 1 && !split_out;   // row m = (n, i, j) of the phase -> pixel (2i + pa, 2j + pb) of y
    // GEMM row -> row of the output tensor (of the split-K partials: their own frame-major order)
    auto out_row = [&](unsigned m) __attribute__((always_inline)) -> unsigned {
        if (!PM && !scatter) return m;
        unsigned fr, i, j;
        row_pixel<PM>(a, m, fr, i, j);
        if (PM && !scatter) return (fr * (unsigned)a.H + i) * (unsigned)a.W + j;
        return ((fr * (unsigned)a.H + i) * 2u + (unsigned)pa) * (2u * (unsigned)a.W) + 2u * j + (unsigned)pb;
    };
    int cov[TN];
    float bv[TN], s1[TN], s2[TN];
    const bool bnb = !PM && a.bnb.y != nullptr && a.stats && !split_out;     // the column sums are a BatchNorm layer's backward statistics
    // an evaluation-mode norm layer applied here (EN; never together with bnb, statistics, a residual or a split): its
    // per-column coefficients take bnb's registers.  Guarded loads: the coefficients of a pad column are zero
    constexpr bool en = EN != 0;
    const float *const cmean = en ? a.en.mean : a.bnb.mean, *const cscale = en ? a.en.scale : a.bnb.scale,
                *const cbeta = en ? a.en.beta : a.bnb.beta;
    const float eslope = en ? a.en.slope : -1.f;
    float bm[TN], bis[TN], bsc[TN], bbe[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        cov[j] = n0 + wn * (BN / WN) + 32 * j + fi;
        bv[j] = (!split_out && a.bias && cov[j] < a.Cout) ? a.bias[cov[j]] : 0.f;
        s1[j] = s2[j] = 0.f;
        const bool real = bnb && cov[j] < a.Cout, coef = (bnb || en) && cov[j] < a.Cout;
        bm[j] = coef ? cmean[cov[j]] : 0.f;
        bis[j] = real ? a.bnb.invstd[cov[j]] : 0.f;
        bsc[j] = coef ? cscale[cov[j]] : 0.f;
        bbe[j] = coef ? cbeta[cov[j]] : 0.f;
    }
    auto emit = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int co = cov[j];
                const bool c_real = co < a.Cout, c_store = co < co_lim;
                const unsigned mb = mrow0 + 32 * i;
                const unsigned off0 = mb * ldo + (unsigned)co, roff0 = mb * (unsigned)a.ld_res + (unsigned)co;
                if constexpr (WIN) {
                    // a lane's register quad 4 g .. 4 g + 3 = rows mb + 8 g .. + 3 = pool window (mb + 8 g) / 4, its pixels in
                    // bn_apply4_pool's order of additions; v is the plain launch's expression (no residual: + 0)
                    if (c_store) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            float o = 0.f;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                o += bn_apply1((acc[0][i][j][4 * g + k] + bv[j]) + 0.f, bm[j], bsc[j], bbe[j], eslope);
                            o *= 0.25f;
                            const unsigned mw = mb + 8 * g;          // M is a multiple of 4: a window is inside or outside
                            if (FULL || mw < Mu) obase[(mw >> 2) * ldo + (unsigned)co] = c_real ? o : 0.f;
                        }
                    }
                    continue;
                }
                if (c_store) {
                    float rv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[r] = 0.f;
                    if (use_res && c_real) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned ro = (r & 3) + 8 * (r >> 2);
                            if (FULL || mb + ro < Mu)
                                rv[r] = PM ? a.residual[out_row(mb + ro) * (unsigned)a.ld_res + (unsigned)co]
                                           : a.residual[roff0 + ro * (unsigned)a.ld_res];
                        }
                    }
                    float yv[16];
                    if (bnb) {
                        const unsigned yoff0 = mb * (unsigned)a.bnb.ld + (unsigned)co;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned ro = (r & 3) + 8 * (r >> 2);
                            yv[r] = (c_real && (FULL || mb + ro < Mu)) ? a.bnb.y[yoff0 + ro * (unsigned)a.bnb.ld] : 0.f;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned ro = (r & 3) + 8 * (r >> 2);
                        float v = acc[0][i][j][r];
                        if (!split_out) v = c_real ? (v + bv[j]) + rv[r] : 0.f;
                        if constexpr (EN == 1) {
                            if (c_real) v = bn_apply1(v, bm[j], bsc[j], bbe[j], eslope);          // pad columns stay zero
                        }
                        if (FULL || mb + ro < Mu) {
                            if (PM || scatter)
                                obase[out_row(mb + ro) * ldo + (unsigned)co] = v;
                            else
                                obase[off0 + ro * ldo] = v;
                            if (bnb) {
                                const float d = yv[r] - bm[j];
                                float g = v;
                                if (a.bnb.slope >= 0.f && !(fmaf(d, bsc[j], bbe[j]) > 0.f)) g *= a.bnb.slope;
                                s1[j] += g;
                                s2[j] = fmaf(g, d * bis[j], s2[j]);
                            } else {
                                s1[j] += v;
                                s2[j] = fmaf(v, v, s2[j]);
                            }
                        }
                    }
                }
            }
    };
    if (full)
        emit(TrueTag{});
    else
        emit(FalseTag{});
    // ---- fused BatchNorm statistics of the tensor just written (sync_batchnorm/batchnorm.py:60-62): per-block
    // column sums -> stats[blockIdx.x][2][ld_y]; the tiny final reduction over blocks is mnk_bn_stats_finish.
    if (!PM && a.stats && !split_out) {
        float* red = reinterpret_cast<float*>(smem_a);          // the main loop ended with a barrier: LDS is free
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            s1[j] += __shfl_xor(s1[j], 32);
            s2[j] += __shfl_xor(s2[j], 32);
            if (fk == 0) {
                const int col = wn * (BN / WN) + 32 * j + fi;
                red[(wm * 2 + 0) * BN + col] = s1[j];
                red[(wm * 2 + 1) * BN + col] = s2[j];
            }
        }
        __syncthreads();
        if (t < BN && n0 + t < a.ld_y) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                t1 += red[(w * 2 + 0) * BN + t];
                t2 += red[(w * 2 + 1) * BN + t];
            }
            float* sp = a.stats + (long)bx * 2 * a.ld_y;
            sp[n0 + t] = t1;
            sp[a.ld_y + n0 + t] = t2;
        }
    }
#ifdef MNK_PHASE_CLOCKS
    __builtin_amdgcn_s_waitcnt(0);            // the output stores of this wave have left (vmcnt / lgkmcnt / expcnt = 0)
#endif
    MNK_PHASE(3);
}

// ---- narrow-output variant on v_mfma_f32_16x16x4_f32 -----------------------------------------------------------
// For Cout <= 48 (the 45-channel refinement stack, the 10 / 13-channel heads, dgrad into 45 channels) a 32-wide MFMA
// tile wastes up to 3/4 of the matrix pipe.  Here the block tile is 128 pixels x BN (16 / 48) channels built from
// 16x16 tiles: 4 waves x 32 rows, each wave covers all BN columns (2 x BN/16 accumulator tiles of 4 VGPRs).
// Fragment layout of the 16x16x4 form: lane l holds A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; with K-contiguous
// LDS rows a lane reads the float4 at k = 4*(l>>4) .. +3 and feeds element e to MFMA e (K permuted identically for A
// and B); D: col = l&15, row = 4*(l>>4) + reg.  Loader, K order, split-K and epilogue semantics are those of the
// 32x32 kernel above.

// GM = 1 (round 6): the products on the bf16 matrix cores (mnk_common.h).  v_mfma_f32_16x16x32_bf16 spans K = 32 = TWO K steps:
// the loop works on PAIRS of steps -- step 2p lands in LDS buffer 0, step 2p + 1 in buffer 1 (zeros behind an odd count), lane
// (fi, fk) reads k = 8 fk .. 8 fk + 7 of its row from buffer fk >> 1 -- six MFMAs per 16x16 tile and pair.  Two register stages
// hold the next pair while the MFMAs of this one run; two barriers per pair.
// GM = 2: the one-pass form (MNK_CONV_BF16) -- the same pairs with ONE rounded plane per operand and one MFMA per tile and pair.
template <int BN, int MODE, int GM = 0, int EN = 0>       // EN: see conv3x3_igemm_kernel
__global__ void __launch_bounds__(256) conv3x3_igemm16_kernel(ConvArgs a) {
    constexpr bool WIN = EN == 2;
    static_assert(!WIN || MODE == 1, "window-major rows: the plain 3x3 fast loader");
    static_assert(EN == 0 || MODE != 0, "an EvalNorm launch: buffer-load loaders");
    constexpr int BM = 128, RA = 2, TM = 2, TN = BN / 16;
    constexpr int NSTG = GM ? 2 : 1;
    constexpr int NPL = GM == 2 ? 1 : 3;      // bf16 planes per operand
    constexpr int A_BYTES = GM ? 2 * NPL * BM * LDS_H * 2 : 2 * BM * LDS_K * 4, B_BYTES = GM ? 2 * NPL * BN * LDS_H * 2 : 2 * BN * LDS_K * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem_a[A_BYTES], smem_b[B_BYTES];
    float (*const As)[BM][LDS_K] = reinterpret_cast<float (*)[BM][LDS_K]>(smem_a);
    float (*const Bs)[BN][LDS_K] = reinterpret_cast<float (*)[BN][LDS_K]>(smem_b);
    unsigned short (*const Ah)[3][BM][LDS_H] = reinterpret_cast<unsigned short (*)[3][BM][LDS_H]>(smem_a);
    unsigned short (*const Bh)[3][BN][LDS_H] = reinterpret_cast<unsigned short (*)[3][BN][LDS_H]>(smem_b);
    unsigned short (*const Ao)[BM][LDS_H] = reinterpret_cast<unsigned short (*)[BM][LDS_H]>(smem_a);
    unsigned short (*const Bo)[BN][LDS_H] = reinterpret_cast<unsigned short (*)[BN][LDS_H]>(smem_b);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int bx, by;
    xcd_tile(a.xcd, bx, by);
    const long m0 = (long)bx * BM;
    const int n0 = by * BN;
    const int split = blockIdx.z;
    const int s_begin = split * a.ksteps_per_split;
    int s_end = s_begin + a.ksteps_per_split;
    if (s_end > a.ksteps) s_end = a.ksteps;
    const int lrow = t >> 2, lq = t & 3;
    typename LoaderSel<RA, MODE, NSTG, false, WIN>::type L;
    L.setup(a, m0, lrow, lq, s_begin, a.pad, a.pad_x < 0 ? a.pad : a.pad_x);
    const long KT = (long)a.ksteps * BK;
    const int wco = n0 + (lrow < BN ? lrow : 0);           // rows beyond BN / Cout: clamped, never stored
    const unsigned woff = (unsigned)((wco < a.Cout ? wco : a.Cout - 1) * KT) + lq * 4;
    float4 rb, rb1;
    auto load_step = [&](int s) __attribute__((always_inline)) {
        L.load(a);
        rb = *reinterpret_cast<const float4*>(a.wp + (long)s * BK + woff);
    };
    auto store_step = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < RA; ++j) *reinterpret_cast<float4*>(&As[buf][lrow + 64 * j][lq * 4]) = L.masked(j);
        if (lrow < BN) *reinterpret_cast<float4*>(&Bs[buf][lrow][lq * 4]) = rb;
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    const int fi = lane & 15, fk = lane >> 4;     // row/col inside a 16-tile, k group 0..3
    if constexpr (GM != 0) {
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        // loads of K step s into register stage ST (the activation loader keeps its own cursor: steps in order)
        auto load_h = [&](int s, auto st_tag) __attribute__((always_inline)) {
            constexpr int ST = decltype(st_tag)::value;
            L.template load<ST>(a);
            const float4 w = *reinterpret_cast<const float4*>(a.wp + (long)s * BK + woff);
            if constexpr (ST == 0) rb = w; else rb1 = w;
        };
        // stage ST -> the three planes of LDS buffer ST (zero: the missing second half of an odd pair)
        auto store_h = [&](auto st_tag, bool zero) __attribute__((always_inline)) {
            constexpr int ST = decltype(st_tag)::value;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (GM == 2) {
#pragma unroll
                for (int j = 0; j < RA; ++j)
                    *reinterpret_cast<uint2*>(&Ao[ST][lrow + 64 * j][lq * 4]) = mnk_round_bf16x4(zero ? z : L.template masked<ST>(j));
                if (lrow < BN) *reinterpret_cast<uint2*>(&Bo[ST][lrow][lq * 4]) = mnk_round_bf16x4(zero ? z : (ST == 0 ? rb : rb1));
                return;
            }
            uint2 p0, p1, p2;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                mnk_split3(zero ? z : L.template masked<ST>(j), p0, p1, p2);
                *reinterpret_cast<uint2*>(&Ah[ST][0][lrow + 64 * j][lq * 4]) = p0;
                *reinterpret_cast<uint2*>(&Ah[ST][1][lrow + 64 * j][lq * 4]) = p1;
                *reinterpret_cast<uint2*>(&Ah[ST][2][lrow + 64 * j][lq * 4]) = p2;
            }
            if (lrow < BN) {
                mnk_split3(zero ? z : (ST == 0 ? rb : rb1), p0, p1, p2);
                *reinterpret_cast<uint2*>(&Bh[ST][0][lrow][lq * 4]) = p0;
                *reinterpret_cast<uint2*>(&Bh[ST][1][lrow][lq * 4]) = p1;
                *reinterpret_cast<uint2*>(&Bh[ST][2][lrow][lq * 4]) = p2;
            }
        };
        const int kb = fk >> 1, ko = (fk & 1) * 8;      // this lane's k group: LDS buffer and offset inside the step
        auto mfma_pair = [&]() __attribute__((always_inline)) {
            if constexpr (GM == 2) {
                mnk_bf16x8 oa[TM], ob[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) oa[i] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Ao[kb][wave * 32 + 16 * i + fi][ko]));
#pragma unroll
                for (int j = 0; j < TN; ++j) ob[j] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Bo[kb][16 * j + fi][ko]));
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa[i], ob[j], acc[i][j], 0, 0, 0);
                return;
            }
            mnk_bf16x8 ha[3][TM], hb[3][TN];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    ha[pl][i] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Ah[kb][pl][wave * 32 + 16 * i + fi][ko]));
#pragma unroll
                for (int j = 0; j < TN; ++j) hb[pl][j] = mnk_as_bf16x8(*reinterpret_cast<const uint4*>(&Bh[kb][pl][16 * j + fi][ko]));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[1][i], hb[1][j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[2][i], hb[0][j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[0][i], hb[2][j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[1][i], hb[0][j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[0][i], hb[1][j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[0][i], hb[0][j], acc[i][j], 0, 0, 0);
                }
        };
        const int n = s_end - s_begin;
        if (n > 0) load_h(s_begin, S0{});
        if (n > 1) load_h(s_begin + 1, S1{});
        for (int s = 0; s < n; s += 2) {
            store_h(S0{}, false);
            store_h(S1{}, s + 1 >= n);
            __syncthreads();
            if (s + 2 < n) load_h(s_begin + s + 2, S0{});
            if (s + 3 < n) load_h(s_begin + s + 3, S1{});
            mfma_pair();
            __syncthreads();                      // (also in front of the epilogue's reuse of the LDS image)
        }
    } else {
    auto mfma_step = [&](int buf) __attribute__((always_inline)) {
        float4 fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
            fa[i] = *reinterpret_cast<const float4*>(&As[buf][wave * 32 + 16 * i + fi][fk * 4]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const float4*>(&Bs[buf][16 * j + fi][fk * 4]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
            }
    };
    // same pipeline as conv3x3_igemm_kernel: registers hold step s+1, loads of step s+2 precede the MFMAs of step s
    if (s_begin < s_end) {
        load_step(s_begin);
        store_step(0);
        if (s_begin + 1 < s_end) load_step(s_begin + 1);
    }
    __syncthreads();
    int s = s_begin;
    for (; s + 2 < s_end; ++s) {
        const int buf = (s - s_begin) & 1;
        store_step(buf ^ 1);
        load_step(s + 2);
        mfma_step(buf);
        __syncthreads();
    }
    if (s + 1 < s_end) {
        const int buf = (s - s_begin) & 1;
        store_step(buf ^ 1);
        mfma_step(buf);
        __syncthreads();
        ++s;
    }
    if (s < s_end) mfma_step((s - s_begin) & 1);
    __syncthreads();                          // the epilogue reuses As for the column sums
    }
    const bool split_out = a.splits > 1;
    const unsigned ldo = split_out ? (unsigned)a.ldw : (unsigned)a.ld_y;          // 32-bit element offsets (host check)
    float* const obase = split_out ? a.ws + (long)split * a.M * a.ldw : a.y;
    const int co_lim = split_out ? a.ldw : a.ld_y;
    const bool use_res = !split_out && a.residual;
    const bool full = m0 + BM <= a.M;
    const unsigned mrow0 = (unsigned)m0 + wave * 32 + 4 * fk, Mu = (unsigned)a.M;
    float s1[TN], s2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) s1[j] = s2[j] = 0.f;
    const bool bnb = a.bnb.y != nullptr && a.stats && !split_out;     // (see BnBwdSrc)
    constexpr bool en = EN != 0;                                      // (see EvalNorm; the coefficients take bnb's registers)
    const float *const cmean = en ? a.en.mean : a.bnb.mean, *const cscale = en ? a.en.scale : a.bnb.scale,
                *const cbeta = en ? a.en.beta : a.bnb.beta;
    const float eslope = en ? a.en.slope : -1.f;
    auto emit = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int co = n0 + 16 * j + fi;
            const bool c_real = co < a.Cout, c_store = co < co_lim;
            const float bv = (!split_out && a.bias && c_real) ? a.bias[co] : 0.f;
            const bool breal = bnb && c_real, coef = (bnb || en) && c_real;
            const float bm = coef ? cmean[co] : 0.f, bis = breal ? a.bnb.invstd[co] : 0.f,
                        bsc = coef ? cscale[co] : 0.f, bbe = coef ? cbeta[co] : 0.f;
            if (c_store) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const unsigned mb = mrow0 + 16 * i;
                    const unsigned off0 = mb * ldo + (unsigned)co, roff0 = mb * (unsigned)a.ld_res + (unsigned)co;
                    if constexpr (WIN) {
                        // the lane's four registers = rows mb .. mb + 3 = pool window mb / 4 (see the 32x32-tile kernel)
                        float o = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) o += bn_apply1((acc[i][j][r] + bv) + 0.f, bm, bsc, bbe, eslope);
                        o *= 0.25f;
                        if (FULL || mb < Mu) obase[(mb >> 2) * ldo + (unsigned)co] = c_real ? o : 0.f;
                        continue;
                    }
                    float rv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f};
                    if (use_res && c_real) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (FULL || mb + r < Mu) rv[r] = a.residual[roff0 + r * (unsigned)a.ld_res];
                    }
                    if (breal) {
                        const unsigned yoff0 = mb * (unsigned)a.bnb.ld + (unsigned)co;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (FULL || mb + r < Mu) yv[r] = a.bnb.y[yoff0 + r * (unsigned)a.bnb.ld];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[i][j][r];
                        if (!split_out) v = c_real ? (v + bv) + rv[r] : 0.f;
                        if constexpr (EN == 1) {
                            if (c_real) v = bn_apply1(v, bm, bsc, bbe, eslope);                   // pad columns stay zero
                        }
                        if (FULL || mb + r < Mu) {
                            obase[off0 + r * ldo] = v;
                            if (bnb) {
                                const float d = yv[r] - bm;
                                float g = v;
                                if (a.bnb.slope >= 0.f && !(fmaf(d, bsc, bbe) > 0.f)) g *= a.bnb.slope;
                                s1[j] += g;
                                s2[j] = fmaf(g, d * bis, s2[j]);
                            } else {
                                s1[j] += v;
                                s2[j] = fmaf(v, v, s2[j]);
                            }
                        }
                    }
                }
            }
        }
    };
    if (full)
        emit(TrueTag{});
    else
        emit(FalseTag{});
    if (a.stats && !split_out) {
        float* red = reinterpret_cast<float*>(smem_a);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            s1[j] += __shfl_xor(s1[j], 16);
            s1[j] += __shfl_xor(s1[j], 32);
            s2[j] += __shfl_xor(s2[j], 16);
            s2[j] += __shfl_xor(s2[j], 32);
            if (fk == 0) {
                red[(wave * 2 + 0) * BN + 16 * j + fi] = s1[j];
                red[(wave * 2 + 1) * BN + 16 * j + fi] = s2[j];
            }
        }
        __syncthreads();
        if (t < BN && n0 + t < a.ld_y) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                t1 += red[(w * 2 + 0) * BN + t];
                t2 += red[(w * 2 + 1) * BN + t];
            }
            float* sp = a.stats + (long)bx * 2 * a.ld_y;
            sp[n0 + t] = t1;
            sp[a.ld_y + n0 + t] = t2;
        }
    }
}

// Split-K reductions: 64 outputs x 4 split-groups per block -- each thread sums every 4th partial (4x the loads in
// flight of a one-thread-per-output loop), the groups are combined through LDS in a fixed order (deterministic).
__global__ void __launch_bounds__(256) conv3x3_splitk_reduce_kernel(const float* __restrict__ ws, int splits, long M,
                                                                    int ldw, const float* __restrict__ bias,
                                                                    const float* __restrict__ residual, int ld_res,
                                                                    float* __restrict__ y, int ld_y, int Cout, int phases,
                                                                    int H, int W) {
    // phases = 4: partials are [split][phase][M][ldw] over the low-resolution pixels (n, i, j) of each sub-pixel phase;
    // the sum goes to pixel (2i + pa, 2j + pb) of the (N, 2H, 2W) output
    __shared__ float sm[4][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long rows = M * phases, total = rows * ld_y;
    for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {
        const long i = base + o;
        long m = 0;
        int co = 0;
        float v = 0.f;
        if (i < total) {
            m = i / ld_y;
            co = (int)(i - m * ld_y);
            if (co < Cout)
                for (int s = g; s < splits; s += 4) v += ws[((long)s * rows + m) * ldw + co];
        }
        sm[g][o] = v;
        __syncthreads();
        if (g == 0 && i < total) {
            float r = 0.f;
            long orow = m;
            if (phases > 1) {
                const long ph = m / M, mm = m - ph * M;
                const long tt = mm / W, fr = tt / H;
                const long jj = mm - tt * W, ii = tt - fr * H;
                orow = ((fr * H + ii) * 2 + (ph >> 1)) * (2L * W) + 2 * jj + (ph & 1);
            }
            if (co < Cout) {
                r = (sm[0][o] + sm[1][o]) + (sm[2][o] + sm[3][o]);
                if (bias) r += bias[co];
                if (residual) r += residual[orow * ld_res + co];
            }
            y[orow * ld_y + co] = r;
        }
        __syncthreads();
    }
}

// The same reduction for a layer whose BatchNorm follows (sync_batchnorm/batchnorm.py:60-62 wants sum and sum of squares of
// what is written here): a block owns `rows_per_block` output rows x tx_n channel quads, every thread sums the splits of its
// float4 in the order of the kernel above (four interleaved groups, (g0 + g1) + (g2 + g3): the same bits), writes it and
// keeps the two column sums; stats[row_block][2][ld_y] are the per-block partials that the conv epilogue leaves for an
// unsplit launch (finished by bn_final_finalize / mnk_bn_stats_finish).  One launch instead of reduction + statistics pass.
struct RSMap {
    int tx, ty, col_tiles, row_blocks;
    long rows_per_block;
};
// rows per thread before a layer is cut into more row blocks (A/B with every split-K reduction on this kernel, visit 48:
// 1 / 2 / 4 -> 10.92 / 10.97 / 11.10 ms; the 64 x 4-group kernel: 10.95)
static int g_rs_rpt = tuning_knob("rs_rpt", &g_rs_rpt, 1);
static RSMap make_rsmap(long rows, int ld) {
    RSMap m;
    const int nv = ld / 4;
    int tx = 1;
    while (tx < nv && tx < 64) tx <<= 1;
    m.tx = tx;
    m.ty = 256 / tx;
    m.col_tiles = (nv + tx - 1) / tx;
    long want = 1024 / m.col_tiles;
    if (want < 1) want = 1;
    const long min_rows = (long)m.ty * (g_rs_rpt > 0 ? g_rs_rpt : 1);
    long rb = (rows + min_rows - 1) / min_rows;
    if (rb > want) rb = want;
    if (rb < 1) rb = 1;
    m.row_blocks = (int)rb;
    m.rows_per_block = (rows + rb - 1) / rb;
    return m;
}

// (the body of the kernel: block (bix, biy) of the reduction's own grid -- the pair form below runs it for either output)
template <bool STATS>
__device__ __forceinline__ void splitk_reduce_stats_block(float4 (*red)[256], const unsigned bix, const unsigned biy,
                                                          const float* __restrict__ ws, int splits, long M, int ldw,
                                                          const float* __restrict__ bias, const float* __restrict__ residual,
                                                          int ld_res, float* __restrict__ y, int ld_y, int Cout, int phases, int H,
                                                          int W, int tx_n, int ty_n, long rows_per_block,
                                                          float* __restrict__ stats, const BnBwdSrc& bnb) {
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
    const int q = bix * tx_n + tx, nv = ld_y / 4, c = q * 4;
    const long rows = M * phases;
    const long r0 = (long)biy * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (q < nv) {
        const bool k0 = c < Cout, k1 = c + 1 < Cout, k2 = c + 2 < Cout, k3 = c + 3 < Cout;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) bv = make_float4(k0 ? bias[c] : 0.f, k1 ? bias[c + 1] : 0.f, k2 ? bias[c + 2] : 0.f, k3 ? bias[c + 3] : 0.f);
        const long sstride = rows * ldw;
        for (long m = r0 + ty; m < r1; m += ty_n) {
            const float* p = ws + m * ldw + c;
            float4 g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            int s = c < ldw ? 0 : splits;        // quads beyond the partial rows (ld_y > ldw): zero columns, nothing to read
            for (; s + 4 <= splits; s += 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 v = *reinterpret_cast<const float4*>(p + (long)(s + e) * sstride);
                    g[e].x += v.x;
                    g[e].y += v.y;
                    g[e].z += v.z;
                    g[e].w += v.w;
                }
            }
#pragma unroll
            for (int e = 0; e < 3; ++e)          // up to three left over: compile-time indices keep g[] in registers
                if (s + e < splits) {
                    const float4 v = *reinterpret_cast<const float4*>(p + (long)(s + e) * sstride);
                    g[e].x += v.x;
                    g[e].y += v.y;
                    g[e].z += v.z;
                    g[e].w += v.w;
                }
            long orow = m;
            if (phases > 1) {
                const long ph = m / M, mm = m - ph * M;
                const long tt = mm / W, fr = tt / H;
                const long jj = mm - tt * W, ii = tt - fr * H;
                orow = ((fr * H + ii) * 2 + (ph >> 1)) * (2L * W) + 2 * jj + (ph & 1);
            }
            float4 r;
            r.x = (g[0].x + g[1].x) + (g[2].x + g[3].x);
            r.y = (g[0].y + g[1].y) + (g[2].y + g[3].y);
            r.z = (g[0].z + g[1].z) + (g[2].z + g[3].z);
            r.w = (g[0].w + g[1].w) + (g[2].w + g[3].w);
            if (bias) {
                r.x += bv.x;
                r.y += bv.y;
                r.z += bv.z;
                r.w += bv.w;
            }
            if (residual) {
                const float* rp = residual + orow * ld_res + c;
                if (k0) r.x += rp[0];
                if (k1) r.y += rp[1];
                if (k2) r.z += rp[2];
                if (k3) r.w += rp[3];
            }
            r.x = k0 ? r.x : 0.f;
            r.y = k1 ? r.y : 0.f;
            r.z = k2 ? r.z : 0.f;
            r.w = k3 ? r.w : 0.f;
            *reinterpret_cast<float4*>(y + orow * ld_y + c) = r;
            if (!STATS) continue;
            if (bnb.y) {         // the sums are a BatchNorm layer's backward statistics (see BnBwdSrc)
                const float* yp = bnb.y + orow * bnb.ld + c;
                const float rr[4] = {r.x, r.y, r.z, r.w};
                float a1[4], a2[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a1[e] = a2[e] = 0.f;
                    if (c + e < Cout) {
                        const float d = yp[e] - bnb.mean[c + e];
                        float g = rr[e];
                        if (bnb.slope >= 0.f && !(fmaf(d, bnb.scale[c + e], bnb.beta[c + e]) > 0.f)) g *= bnb.slope;
                        a1[e] = g;
                        a2[e] = g * (d * bnb.invstd[c + e]);
                    }
                }
                s1.x += a1[0], s1.y += a1[1], s1.z += a1[2], s1.w += a1[3];
                s2.x += a2[0], s2.y += a2[1], s2.z += a2[2], s2.w += a2[3];
                continue;
            }
            s1.x += r.x;
            s1.y += r.y;
            s1.z += r.z;
            s1.w += r.w;
            s2.x = fmaf(r.x, r.x, s2.x);
            s2.y = fmaf(r.y, r.y, s2.y);
            s2.z = fmaf(r.z, r.z, s2.z);
            s2.w = fmaf(r.w, r.w, s2.w);
        }
    }
    if (!STATS) return;          // STATS = false: the plain reduction as float4 rows (no LDS hop, every thread busy for any split count)
    red[0][threadIdx.x] = s1;
    red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int s = ty_n >> 1; s > 0; s >>= 1) {
        if (ty < s) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float4 a = red[k][threadIdx.x], b = red[k][threadIdx.x + s * tx_n];
                red[k][threadIdx.x] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
            }
        }
        __syncthreads();
    }
    if (ty == 0 && q < nv) {
        float* o = stats + (long)biy * 2 * ld_y;
        *reinterpret_cast<float4*>(o + c) = red[0][tx];
        *reinterpret_cast<float4*>(o + ld_y + c) = red[1][tx];
    }
}

template <bool STATS>
__global__ void __launch_bounds__(256) conv3x3_splitk_reduce_stats_kernel(const float* __restrict__ ws, int splits, long M,
                                                                          int ldw, const float* __restrict__ bias,
                                                                          const float* __restrict__ residual, int ld_res,
                                                                          float* __restrict__ y, int ld_y, int Cout,
                                                                          int phases, int H, int W, int tx_n, int ty_n,
                                                                          long rows_per_block, float* __restrict__ stats,
                                                                          BnBwdSrc bnb = BnBwdSrc{}) {
    __shared__ float4 red[2][256];
    splitk_reduce_stats_block<STATS>(red, blockIdx.x, blockIdx.y, ws, splits, M, ldw, bias, residual, ld_res, y, ld_y, Cout, phases,
                                     H, W, tx_n, ty_n, rows_per_block, stats, bnb);
}

// ---- one reduction for the two outputs of a pair launch (conv3x3_igemm_kernel<..., PAIR>) whose plans both split K ------------
// Block columns [0, s0.col_tiles) sum the first output's partials, the rest the second's; each output keeps the row / column map
// it has on its own (make_rsmap: thread shape, rows per block, row blocks -- its statistics partials are sums in that map's
// order), grid y is the larger row-block count and blocks past their output's count leave at once.  A block runs the single
// reduction's body: the partials are added in split order, every dx element and every statistics partial keeps its bits.
struct RsOut {
    const float* ws;
    int splits, ldw;
    float* y;
    int ld_y, Cout, tx_n, ty_n, col_tiles, row_blocks;
    long rows_per_block;
    float* stats;      // nullptr: this output leaves no statistics
    BnBwdSrc bnb;
};
__global__ void __launch_bounds__(256) conv3x3_splitk_reduce_pair_kernel(RsOut s0, RsOut s1, long M, int H, int W) {
    __shared__ float4 red[2][256];
    const bool second = blockIdx.x >= (unsigned)s0.col_tiles;
    const unsigned bix = second ? blockIdx.x - (unsigned)s0.col_tiles : blockIdx.x;
    if (second) s0 = s1;
    if (blockIdx.y >= (unsigned)s0.row_blocks) return;
    if (s0.stats)
        splitk_reduce_stats_block<true>(red, bix, blockIdx.y, s0.ws, s0.splits, M, s0.ldw, nullptr, nullptr, 0, s0.y, s0.ld_y, s0.Cout,
                                        1, H, W, s0.tx_n, s0.ty_n, s0.rows_per_block, s0.stats, s0.bnb);
    else
        splitk_reduce_stats_block<false>(red, bix, blockIdx.y, s0.ws, s0.splits, M, s0.ldw, nullptr, nullptr, 0, s0.y, s0.ld_y, s0.Cout,
                                         1, H, W, s0.tx_n, s0.ty_n, s0.rows_per_block, s0.stats, s0.bnb);
}

// ---- weight packing: Wp[row][chunk][tap][16] --------------------------------------------------------------------
__global__ void __launch_bounds__(256) pack_fwd_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                                                       int C0, int C1, int C0p, int C1p, int ntaps) {
    const int Cin = C0 + C1, chunks = (C0p + C1p) / 16;
    const long total = (long)Cout * chunks * ntaps * 16;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k16 = (int)(i & 15);
        long t = i >> 4;
        const int tap = (int)(t % ntaps);
        t /= ntaps;
        const int chunk = (int)(t % chunks);
        const int co = (int)(t / chunks);
        const int k = chunk * 16 + k16;
        int ci = -1;
        if (k < C0p) {
            if (k < C0) ci = k;
        } else if (k - C0p < C1) {
            ci = C0 + k - C0p;
        }
        wp[i] = ci >= 0 ? w[((long)co * Cin + ci) * ntaps + tap] : 0.f;
    }
}

__global__ void __launch_bounds__(256) pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                                                         int Cin_total, int c_start, int c_count, int chunks,
                                                         int ntaps) {
    const long total = (long)c_count * chunks * ntaps * 16;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k16 = (int)(i & 15);
        long t = i >> 4;
        const int tap = (int)(t % ntaps);
        t /= ntaps;
        const int chunk = (int)(t % chunks);
        const int ci = (int)(t / chunks);
        const int co = chunk * 16 + k16;
        wp[i] = co < Cout ? w[((long)co * Cin_total + c_start + ci) * ntaps + (ntaps - 1 - tap)] : 0.f;
    }
}

// ---- packs of the sub-pixel forms of [nearest x2 up-sampling -> 3x3 / pad 1] (ConvArgs::phases) -----------------------
// S(a, u): the 3x3 kernel rows that fall on low-resolution row i + a - 1 + u for an output row 2i + a:
//   S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2}                       (same sets for columns)
// D(t): the 3x3 kernel rows whose gradient reaches low-resolution row i from up-sampled-output row 2i - 1 + t:
//   D(0) = {2}, D(1) = {1,2}, D(2) = {0,1}, D(3) = {0}
__device__ __forceinline__ void phase_set(int a, int u, int& lo, int& hi) { up_phase_set(a, u, lo, hi); }
__device__ __forceinline__ void dgrad_set(int t, int& lo, int& hi) { up_dgrad_set(t, lo, hi); }

// forward: wp[phase][co][chunk][tap4 = 2u + v][16] = sum_{ky in S(a,u)} sum_{kx in S(b,v)} w[co][ci][ky][kx], phase = 2a + b
__global__ void __launch_bounds__(256) pack_up_fwd_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                                                          int C0, int C1, int C0p, int C1p) {
    const int Cin = C0 + C1, chunks = (C0p + C1p) / 16;
    const long per_phase = (long)Cout * chunks * 64, total = 4 * per_phase;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int phase = (int)(i / per_phase);
        long t = i - phase * per_phase;
        const int k16 = (int)(t & 15);
        t >>= 4;
        const int tap = (int)(t & 3);
        t >>= 2;
        const int chunk = (int)(t % chunks), co = (int)(t / chunks);
        const int k = chunk * 16 + k16;
        int ci = -1;
        if (k < C0p) {
            if (k < C0) ci = k;
        } else if (k - C0p < C1) {
            ci = C0 + k - C0p;
        }
        float v = 0.f;
        if (ci >= 0) {
            int y0, y1, x0, x1;
            phase_set(phase >> 1, tap >> 1, y0, y1);
            phase_set(phase & 1, tap & 1, x0, x1);
            const float* wr = w + ((long)co * Cin + ci) * 9;
            for (int ky = y0; ky <= y1; ++ky)
                for (int kx = x0; kx <= x1; ++kx) v += wr[ky * 3 + kx];
        }
        wp[i] = v;
    }
}

// data gradient w.r.t. the low-resolution input, source channels [c_start, c_start + c_count): a 4x4 / stride 2 / pad 1
// convolution over dy:  wp[ci][chunk(co)][tap16 = 4 ty + tx][16] = sum_{ky in D(ty)} sum_{kx in D(tx)} w[co][c_start+ci][ky][kx]
__global__ void __launch_bounds__(256) pack_up_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                                                            int Cin_total, int c_start, int c_count, int chunks) {
    const long total = (long)c_count * chunks * 256;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k16 = (int)(i & 15);
        long t = i >> 4;
        const int tap = (int)(t & 15);
        t >>= 4;
        const int chunk = (int)(t % chunks), ci = (int)(t / chunks);
        const int co = chunk * 16 + k16;
        float v = 0.f;
        if (co < Cout) {
            int y0, y1, x0, x1;
            dgrad_set(tap >> 2, y0, y1);
            dgrad_set(tap & 3, x0, x1);
            const float* wr = w + ((long)co * Cin_total + c_start + ci) * 9;
            for (int ky = y0; ky <= y1; ++ky)
                for (int kx = x0; kx <= x1; ++kx) v += wr[ky * 3 + kx];
        }
        wp[i] = v;
    }
}

template <int NT>
__global__ void __launch_bounds__(256) pack_all_kernel(const float* __restrict__ w, float* __restrict__ wf,
                                                       float* __restrict__ wd0, float* __restrict__ wd1, int Cout, int C0,
                                                       int C1, int C0p, int C1p, int ntaps_rt) {
    __shared__ float T[16 * (16 * 17 + 1)];
    pack_tile<NT>(T, w, wf, wd0, wd1, Cout, C0, C1, C0p, C1p, ntaps_rt, blockIdx.x, blockIdx.y);
}

// every 3x3 layer of a model in ONE launch: block b works on tile (b - tile_begin) of the layer whose
// [tile_begin, tile_begin + tiles) range contains it (binary search over the descriptor table in device memory)
__global__ void __launch_bounds__(256) pack_multi_kernel(const MnkPackDesc* __restrict__ descs, int n) {
    __shared__ float T[16 * (16 * 17 + 1)];
    int lo = 0, hi = n - 1;
    const int b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].tile_begin <= b)
            lo = mid;
        else
            hi = mid - 1;
    }
    const MnkPackDesc d = descs[lo];
    const int local = b - d.tile_begin;
    const int C0p = round_up16(d.C0), C1p = d.C1 > 0 ? round_up16(d.C1) : 0, tiles_x = (C0p + C1p) / 16;
    const int cot = local / tiles_x, cc = local - cot * tiles_x;
    pack_tile<9>(T, d.w, d.wp_fwd, d.wp_d0, d.wp_d1, d.Cout, d.C0, d.C1, C0p, C1p, 9, cc, cot, d.flags & 1);
}

struct Plan {
    int bm, bn, gm, gn, splits, ksteps, ksteps_per_split, ldw;
};

// split-K plan values (defaults from the MI355X sweeps in profiles/README.md; tuning_knob: settable by name through
// mnk_set_tuning / MNK_TUNING for tuning runs, no environment switch of their own)
static int g_split_tiles = tuning_knob("split_tiles", &g_split_tiles, 192), g_split_target = tuning_knob("split_target", &g_split_target, 512),
           g_split_minsteps = tuning_knob("split_minsteps", &g_split_minsteps, 6);
// 1 (default): a split-K forward launch that was asked for BatchNorm statistics sums its partials with
// conv3x3_splitk_reduce_stats_kernel (one launch for reduction + statistics pass); 0: no statistics from split launches
static int g_splitk_stats = tuning_knob("splitk_stats", &g_splitk_stats, 1);
// 1: every split-K reduction runs the float4-row kernel (the statistics kernel without its statistics; the same bits);
// 0: conv3x3_splitk_reduce_kernel (64 outputs x 4 split groups per block, combined through LDS)
static int g_reduce_v4 = tuning_knob("reduce_v4", &g_reduce_v4, 1);

// mid-size layers (fewer than ~2 blocks per CU with 128-row tiles) use 64-row tiles: twice the blocks, so every SIMD
// has a second wave to overlap loads with MFMA, and less (or no) split-K
static int g_bm64_tiles = tuning_knob("bm64_tiles", &g_bm64_tiles, 512);
static int g_split64_tiles = tuning_knob("split64_tiles", &g_split64_tiles, 384), g_split64_target = tuning_knob("split64_target", &g_split64_target, 1024),
           g_split64_deep = tuning_knob("split64_deep", &g_split64_deep, 32), g_split64_minsteps = tuning_knob("split64_minsteps", &g_split64_minsteps, 16),
           g_split64_tiny = tuning_knob("split64_tiny", &g_split64_tiny, 4);      // K steps per split of the tiny-problem rule; 0: off
static int g_bn128_kwork = tuning_knob("bn128_kwork", &g_bn128_kwork, 8388);   // 1000 pixels x channels from which 128-wide tiles are used
static int g_kxk_fast = tuning_knob("kxk_fast", &g_kxk_fast, 1);     // buffer-load loader for K x K / any pad (MODE 3)
static int g_mfma16 = tuning_knob("mfma16", &g_mfma16, 1);
// 1: the 32x32-tile implicit-GEMM kernels (forward / data gradient) run their products on the bf16 matrix cores through the exact
// three-way split of both fp32 operands (conv3x3_igemm_kernel<..., GM = 1>, mnk_common.h); 0: v_mfma_f32_32x32x2_f32
static int g_gemm_bf16x3 = tuning_knob("gemm_bf16x3", &g_gemm_bf16x3, 0);
// with gemm_bf16x3, 1: 33 .. 48 output channels (the 45-channel refinement stack) take the 64-wide 32x32-tile kernel -- 45 of 64
// columns at 2.67x the matrix rate -- instead of the 48-wide 16x16x4 fp32 kernel.  Measured SLOWER (10.08 vs 9.92 ms per step,
// profiles/r06_knob_ab_log.txt): 0 keeps the 16x16 kernel
// 1: the 16x16-tile kernels (Cout <= 16, 33 .. 48: the 45-channel refinement stack) too: pairs of K steps on v_mfma_f32_16x16x32_bf16
static int g_gemm16_bf16x3 = tuning_knob("gemm16_bf16x3", &g_gemm16_bf16x3, 0);
static int g_gemm_bf16x3_n48 = tuning_knob("gemm_bf16x3_n48", &g_gemm_bf16x3_n48, 0);
static bool narrow48_on_wide_tiles() { return g_gemm_bf16x3 && g_gemm_bf16x3_n48; }

struct PlanRow {
    long M;
    int Cout, chunks, ntaps, phases, bm, bn, splits;
};
static const PlanRow g_tuned_rows[] = {
#include "plan_table.h"
    {0, 0, 0, 0, 0, 0, 0, 0}};
static const PlanRow g_tuned_rows_bf16x3[] = {
#include "plan_table_bf16x3.h"
    {0, 0, 0, 0, 0, 0, 0, 0}};
static int g_plan_table = tuning_knob("plan_table", &g_plan_table, 1), g_force_bm = tuning_knob("force_bm", &g_force_bm, 0),
           g_force_bn = tuning_knob("force_bn", &g_force_bn, 0);
}  // namespace
// shared with conv_skinny.hip (declared in conv_common.h): the forced split count and the plan mnk_last_plan reports
int mnk::g_force_splits = tuning_knob("force_splits", &mnk::g_force_splits, 0);
long mnk::g_last_plan[8];
namespace {

// block tiles the GEMM kernels are instantiated for (conv2d_fwd_impl's dispatch)
static bool plan_tile_ok(int bm, int bn, int Cout, int phases) {
    if (bn == 48 && narrow48_on_wide_tiles()) return false;
    if (bn == 16 || bn == 48) return bm == 128 && phases == 1 && g_mfma16 && Cout <= bn;
    if (bn == 32) return bm == 128;
    return (bn == 64 || bn == 128) && (bm == 64 || bm == 128);
}

static Plan make_plan(long M, int Cout, int chunks, int ntaps = 9, int phases = 1) {
    // phases > 1 (sub-pixel form): M = pixels of ONE phase, p.gm = tiles of one phase; the launch has phases * gm M tiles
    Plan p;
    p.bn = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
    if (g_mfma16 && phases == 1) {   // narrow outputs: 16x16x4 MFMA tiles (BN = 16 / 48), see conv3x3_igemm16_kernel
        if (Cout <= 16) p.bn = 16;
        else if (Cout > 32 && Cout <= 48 && !narrow48_on_wide_tiles()) p.bn = 48;
    }
    // measured on the MI355X over both benchmark configurations' layer shapes (tools/plan_tune.py, profiles/r02_plan_tune_*.txt):
    // the 64x64 tile (56 registers, 20 KB of LDS: 8 blocks per CU) is the fastest instantiation for every layer wider than
    // 48 channels -- by 5..40 % where 128-wide tiles left CUs idle or forced a split-K the 64x64 plan does not need -- except
    // large layers whose width is a multiple of 128 (>= 65536 pixels x 128 channels: level with the 128x128 tile)
    // (bn128_kwork < 0: the previous rule -- 128-wide tiles for every layer wider than 64 channels -- for A/B runs)
    const bool small_tiles = g_bn128_kwork >= 0;
    if (small_tiles && p.bn == 128 && (Cout % 128 != 0 || (double)M * phases * Cout < (double)g_bn128_kwork * 1000.0)) p.bn = 64;
    p.gn = ceil_div(Cout, p.bn);
    p.bm = 128;
    if ((small_tiles && p.bn == 64) || (p.bn >= 64 && (long)ceil_div(M, 128) * p.gn * phases < g_bm64_tiles)) p.bm = 64;
    p.gm = ceil_div(M, p.bm);
    p.ksteps = ntaps * chunks;
    long tiles = (long)p.gm * p.gn * phases;
    int splits = 1;
    if (small_tiles && p.bn == 64 && p.bm == 64) {
        // 64x64 tiles (same sweep): a CU holds eight of these blocks, and the fastest plans put ~1024 blocks on the 256 CUs
        // with >= 16 K steps each; layers that already have a block per CU only gain once a split is >= 32 steps deep (the
        // partials cross HBM twice and, in front of a BatchNorm, a split plan's epilogue cannot produce the statistics)
        if (tiles < g_split64_tiles) {
            splits = (int)((g_split64_target + tiles / 2) / tiles);
            if (splits > p.ksteps / g_split64_minsteps) splits = p.ksteps / g_split64_minsteps;
            if (splits < 1) splits = 1;
            if (tiles >= 192 && p.ksteps / splits < g_split64_deep) splits = 1;
            // (round 6) tiny problems -- the per-frame evaluation loops at batch 1 (reconstruction.py:45-62): 4 ... 32 tiles with
            // 36 ... 150 K steps -- are one serial K loop per block on a mostly idle chip: a launch's time is its loop length, so
            // splits as short as 4 steps pay until ~256 blocks exist (tools/plan_tune.py --eval, profiles/r06_plan_tune_eval_*:
            // 18.4 -> 13.2 us for conv + reduction of a 256-pixel layer).  Plans that already fill half the chip are left alone.
            if (g_split64_tiny && tiles < 64 && tiles * splits < 128) {
                int s2 = (int)(256 / tiles);
                if (s2 > p.ksteps / g_split64_tiny) s2 = p.ksteps / g_split64_tiny;
                if (s2 > splits) splits = s2;
            }
        }
    } else if (tiles < g_split_tiles) {
        splits = (int)((g_split_target + tiles - 1) / tiles);
        int max_splits = p.ksteps / g_split_minsteps;      // keep >= 6 K steps (96 deep) per split
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
    }
    // measured plans: the benchmark configurations' layer shapes were swept on the MI355X (tools/plan_tune.py -> plan_table.h);
    // a forced plan (mnk_set_tuning MNK_FORCE_BM / _BN / _SPLITS) is what that sweep drives.  Anything the kernels have no
    // instantiation for keeps the rule's choice.
    int want_bm = 0, want_bn = 0, want_splits = 0;
    if (g_plan_table) {
        const PlanRow* tables[2] = {g_gemm_bf16x3 ? g_tuned_rows_bf16x3 : g_tuned_rows, g_gemm_bf16x3 ? g_tuned_rows : nullptr};
        for (int ti = 0; ti < 2 && !want_bm && !want_splits; ++ti)
            for (const PlanRow* r = tables[ti]; r && r->M; ++r)
                if (r->M == M && r->Cout == Cout && r->chunks == chunks && r->ntaps == ntaps && r->phases == phases) {
                    want_bm = r->bm, want_bn = r->bn, want_splits = r->splits;
                    break;
                }
    }
    if (g_force_bm) want_bm = g_force_bm;
    if (g_force_bn) want_bn = g_force_bn;
    if (g_force_splits) want_splits = g_force_splits;
    if (want_bm || want_bn) {
        const int bm = want_bm ? want_bm : p.bm, bn = want_bn ? want_bn : p.bn;
        if (plan_tile_ok(bm, bn, Cout, phases)) {
            p.bm = bm, p.bn = bn;
            p.gn = ceil_div(Cout, p.bn);
            p.gm = ceil_div(M, p.bm);
        }
    }
    if (want_splits > 0) splits = want_splits > p.ksteps ? p.ksteps : want_splits;
    p.ksteps_per_split = (p.ksteps + splits - 1) / splits;
    p.splits = (p.ksteps + p.ksteps_per_split - 1) / p.ksteps_per_split;
    p.ldw = round_up(Cout, 4);
    g_last_plan[0] = M, g_last_plan[1] = Cout, g_last_plan[2] = chunks, g_last_plan[3] = ntaps, g_last_plan[4] = phases;
    g_last_plan[5] = p.bm, g_last_plan[6] = p.bn, g_last_plan[7] = p.splits;
    return p;
}

// What one forward / data-gradient launch needs: its plan and the floats of the caller's two buffers -- the split-K partials
// (0: the plan does not split) and the BatchNorm statistics (0: a split plan without splitk_stats).  The size queries answer
// from it and conv2d_fwd_impl launches from it.
struct Launch {
    Plan p;
    size_t ws_floats, stats_floats;
};
// (ntaps, phases): the form's geometry -- (kh * kw, 1); sub-pixel forward (4, 4), sub-pixel data gradient (16, 1).  (H, W): the
// map ONE phase writes.  A shape no launch takes: all zero, and no plan is made.
static Launch plan_launch(int ntaps, int phases, int N, int H, int W, int C0, int C1, int Cout) {
    Launch l{};
    if (N <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0 || ntaps <= 0) return l;
    const long M = (long)N * H * W;
    const int ldw = round_up(Cout, 4);
    l.p = make_plan(M, Cout, (round_up(C0, 16) + (C1 > 0 ? round_up(C1, 16) : 0)) / 16, ntaps, phases);
    if (l.p.splits > 1) {
        l.ws_floats = (size_t)l.p.splits * phases * M * l.p.ldw;
        l.stats_floats = g_splitk_stats ? (size_t)make_rsmap(M * phases, ldw).row_blocks * 2 * ldw : 0;
    } else
        l.stats_floats = (size_t)phases * l.p.gm * 2 * ldw;
    return l;
}

// ---- position-major rows + tap skipping (conv3x3_igemm_kernel<..., PM>) -----------------------------------------------------
// 1: launches that can leave K steps out run position-major; 0: every launch keeps the frame-major order and all its steps
static int g_ktap_skip = tuning_knob("ktap_skip", &g_ktap_skip, 1);
// the least share of a launch's (row, tap) pairs, in per cent, that must fall away for the position-major order to be used.
// Its rows lie a frame apart, so a tile re-reads nothing of its neighbours' halo, and the launch keeps the split count that
// was chosen for the full K.  Measured per launch (profiles/tap_skip_ab.txt): the groups that lose 41 % and more got faster
// (the discriminator's 2x2 -> 5x5 data gradient 38.8 -> 18.6 us, 2x2-map layers 14 ... 24 %, 10x10 -> 13x13 2 %); 3x3 layers
// on 4x4 maps (31 %) came out level in sum, 8x8 (16 %) and 16x16 maps (8 %) level or slower, and the discriminator's
// 27x27 -> 30x30 data gradient (19 %) 4 % slower: those keep the frame-major order
static int g_ktap_skip_min = tuning_knob("ktap_skip_min", &g_ktap_skip_min, 35);

// sum over the M tiles of a position-major launch (every phase) of rows(tile) * taps(tile), taps(tile) = the taps that lie inside
// the source for at least one position of the tile: the (row, tap) pairs the launch issues -- M * phases * ntaps without skipping.
// This is the PLAN's count, made on the host from the geometry with the rule the blocks apply to their own rows (the AND of
// the rows' out-of-image bits); nothing is read back from the device.
struct TapGeom {
    int bm, N, H, W, Hi, Wi, kh, kw, pad, stride, phases;
    bool operator==(const TapGeom& o) const {
        return bm == o.bm && N == o.N && H == o.H && W == o.W && Hi == o.Hi && Wi == o.Wi && kh == o.kh && kw == o.kw &&
               pad == o.pad && stride == o.stride && phases == o.phases;
    }
};
static double count_row_taps(const TapGeom& g) {
    const long M = (long)g.N * g.H * g.W;
    double total = 0.0;
    for (int phase = 0; phase < g.phases; ++phase) {
        const int pad_y = g.pad - (phase >> 1), pad_x = g.pad - (phase & 1);
        for (long m0 = 0; m0 < M; m0 += g.bm) {
            const long m1 = m0 + g.bm < M ? m0 + g.bm : M;
            unsigned mask = 0;
            for (long p = m0 / g.N; p <= (m1 - 1) / g.N; ++p) {
                const int h = (int)(p / g.W) * g.stride, w = (int)(p % g.W) * g.stride;
                for (int ky = 0; ky < g.kh; ++ky)
                    for (int kx = 0; kx < g.kw; ++kx) {
                        const int hh = h + ky - pad_y, ww = w + kx - pad_x;
                        if (hh >= 0 && hh < g.Hi && ww >= 0 && ww < g.Wi) mask |= 1u << (ky * g.kw + kx);
                    }
            }
            total += (double)(m1 - m0) * __builtin_popcount(mask);
        }
    }
    return total;
}
// the count of a geometry is remembered (a training step launches the same few dozen shapes again and again): a small table
// under a lock, the oldest entry is replaced when it is full
static double issued_row_taps(const TapGeom& g) {
    constexpr int SLOTS = 128;
    static std::mutex lock;
    static TapGeom memo_g[SLOTS];
    static double memo_v[SLOTS];
    static int memo_n = 0, memo_next = 0;
    {
        std::lock_guard<std::mutex> hold(lock);
        for (int i = 0; i < memo_n; ++i)
            if (memo_g[i] == g) return memo_v[i];
    }
    const double total = count_row_taps(g);
    std::lock_guard<std::mutex> hold(lock);
    memo_g[memo_next] = g;
    memo_v[memo_next] = total;
    memo_next = (memo_next + 1) % SLOTS;
    if (memo_n < SLOTS) ++memo_n;
    return total;
}

// Does this launch run position-major?  Only the 32x32-tile fp32 kernels through a buffer-load loader have the form (not the
// bf16x3 kernels, not a one-pass MNK_CONV_BF16 launch); the
// sources must fit the loaders' window from the start of the tensor (the rows of a tile lie a frame apart); an unsplit launch
// with a column-sum epilogue keeps the frame-major order (its sums are sums over a tile's rows; a split launch's sums come
// from the reduction, which walks memory order); and the order must pay: ktap_skip_min.  *row_taps: the pairs it issues.
static bool plan_taps(const Plan& p, int mode, bool one_pass, bool column_sums, const TapGeom& g, long src_bytes, double* row_taps) {
    const double all = (double)g.N * g.H * g.W * g.phases * g.kh * g.kw;
    *row_taps = all;
    if (!g_ktap_skip || g_gemm_bf16x3 || one_pass || p.bn == 16 || p.bn == 48 || mode < 1 || mode > 3) return false;
    if (column_sums || src_bytes >= (1L << 29) || g.kh * g.kw > 32) return false;
    // no tile order can skip more than the (position, tap) pairs that are outside: a product of two one-dimensional counts
    double inside = 0.0;
    for (int phase = 0; phase < g.phases; ++phase) {
        long vy = 0, vx = 0;
        for (int h = 0; h < g.H; ++h)
            for (int ky = 0; ky < g.kh; ++ky) vy += h * g.stride + ky - (g.pad - (phase >> 1)) >= 0 && h * g.stride + ky - (g.pad - (phase >> 1)) < g.Hi;
        for (int w = 0; w < g.W; ++w)
            for (int kx = 0; kx < g.kw; ++kx) vx += w * g.stride + kx - (g.pad - (phase & 1)) >= 0 && w * g.stride + kx - (g.pad - (phase & 1)) < g.Wi;
        inside += (double)vy * (double)vx * g.N;
    }
    if ((all - inside) * 100.0 < all * (double)g_ktap_skip_min) return false;
    const double issued = issued_row_taps(g);
    if (issued >= all || (all - issued) * 100.0 < all * (double)g_ktap_skip_min) return false;
    *row_taps = issued;
    return true;
}

// The activation-side loader of a forward / data-gradient launch (LoaderSel): 1 / 2 -- the 3x3 / pad 1 fast form (plain / through
// the x2 up-sampled view) when the caller vouches for clean pad channels and a block's pixel span fits the 2^30-byte buffer
// window (always, short of ~2 M-float pixel rows); 3 -- any other K x K / pad (the discriminator's 4x4 convolutions and their
// pad-3 data gradients, the sub-pixel forms): ActLoaderK.  A block's 128 output pixels span at most 128 * kh * kw + (kh + 3) * Wi
// input pixels (a 1x1 output per frame advances a whole kh x kw input frame per output pixel; plus the rows of the taps);
// 0 -- the generic loader.  ldmax: the larger leading dimension of the sources; aligned: both sources start on 16 bytes.
static long kxk_span_bytes(int kh, int kw, int stride, int Wi, int ldmax) {
    return (128L * kh * kw * stride * stride + (long)(kh + 3) * Wi) * ldmax * 4;
}
static int loader_mode(bool clean, int ups, int kh, int kw, int pad, int stride, int phases, int Wi, int ldmax, bool aligned) {
    const long span = ((long)BK * 8 + 3L * (ups ? Wi / 2 : Wi) + 8) * ldmax * 4;
    if (g_fast_loader && clean && kh == 3 && kw == 3 && pad == 1 && stride == 1 && phases == 1 && span < (1L << 29) && aligned)
        return ups ? 2 : 1;
    if (g_fast_loader && g_kxk_fast && clean && !ups && kh * kw <= 32 && pad >= 0 && pad < kh && pad < kw &&
        kxk_span_bytes(kh, kw, stride, Wi, ldmax) < (1L << 29) && aligned)
        return 3;
    return 0;
}

// How a forward launch with an EvalNorm runs (mnk_conv3x3_evalnorm_form): 0 -- it cannot (the plan splits K; the generic loader;
// a pooled layer whose launch has no window-major kernel: another loader than the plain 3x3 fast one, or a position-major plan,
// whose blocks would lose their tap skipping); 1 -- per element; 2 -- with the pool.  A window-major tile of 128 rows spans at most
// 128 + 7 W pixels of its source (32 windows of one or more window rows, each two pixel rows, plus the taps' halo).
static int evalnorm_form_of(const Plan& p, int mode, bool pm, int pool, int Wi, int ldmax) {
    if (p.splits > 1 || mode == 0) return 0;        // (the generic loader -- sources without clean pads -- has no such kernel)
    if (!pool) return (p.bn == 16 || p.bn == 48) && mode == 3 ? 0 : 1;
    return (mode == 1 && !pm && ((long)BK * 8 + 8L * Wi + 8) * ldmax * 4 < (1L << 29)) ? 2 : 0;
}
static int g_last_evalnorm_form = 0;     // of the last forward / data-gradient launch (0: a plain launch)

}  // namespace

extern "C" {

// ---- general K x K entry points (3x3 pad 1 of the hot path; 4x4 pad 0 of the discriminator, its data gradient = 4x4 pad 3)
size_t mnk_conv2d_packed_floats(int Cout, int C0, int C1, int ntaps) {
    if (Cout <= 0 || C0 <= 0 || C1 < 0 || ntaps <= 0) return 0;
    return (size_t)Cout * ntaps * (round_up(C0, 16) + (C1 > 0 ? round_up(C1, 16) : 0));
}

int mnk_conv2d_pack_fwd(const float* w, float* wp, int Cout, int C0, int C1, int ntaps, void* stream) {
    MNK_REQUIRE(w && wp && Cout > 0 && C0 > 0 && C1 >= 0 && ntaps > 0);
    hipStream_t s = (hipStream_t)stream;
    const int C0p = round_up(C0, 16), C1p = C1 > 0 ? round_up(C1, 16) : 0;
    const long total = (long)Cout * ntaps * (C0p + C1p);
    ProfScope prof(K_CONV_REDUCE, s, (double)total * 8);
    hipLaunchKernelGGL(pack_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, w, wp, Cout, C0, C1, C0p, C1p, ntaps);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_conv2d_pack_dgrad(const float* w, float* wp, int Cout, int Cin_total, int c_start, int c_count, int ntaps,
                          void* stream) {
    MNK_REQUIRE(w && wp && Cout > 0 && Cin_total > 0 && c_start >= 0 && c_count > 0 && c_start + c_count <= Cin_total);
    MNK_REQUIRE(ntaps > 0);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = round_up(Cout, 16) / 16;
    const long total = (long)c_count * chunks * ntaps * 16;
    ProfScope prof(K_CONV_REDUCE, s, (double)total * 8);
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, s, w, wp, Cout, Cin_total, c_start,
                       c_count, chunks, ntaps);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_conv2d_pack_all(const float* w, float* wp_fwd, float* wp_d0, float* wp_d1, int Cout, int C0, int C1, int ntaps,
                        void* stream) {
    MNK_REQUIRE(w && wp_fwd && Cout > 0 && C0 > 0 && C1 >= 0 && ntaps > 0 && (!wp_d1 || C1 > 0));
    hipStream_t s = (hipStream_t)stream;
    const int C0p = round_up(C0, 16), C1p = C1 > 0 ? round_up(C1, 16) : 0;
    const long dper = (long)round_up(Cout, 16) * ntaps;
    const long total = (long)Cout * ntaps * (C0p + C1p) + (wp_d0 ? C0 * dper : 0) + (wp_d1 ? C1 * dper : 0);
    MNK_REQUIRE(total < (1L << 31) && ((size_t)wp_fwd % 16) == 0 && ((size_t)wp_d0 % 16) == 0 && ((size_t)wp_d1 % 16) == 0);
    ProfScope prof(K_CONV_REDUCE, s, (double)total * 8);
    MNK_REQUIRE(ntaps <= 16);
    const dim3 grid((C0p + C1p) / 16, ceil_div(Cout, 16));
    if (ntaps == 9)
        hipLaunchKernelGGL(pack_all_kernel<9>, grid, dim3(256), 0, s, w, wp_fwd, wp_d0, wp_d1, Cout, C0, C1, C0p, C1p, ntaps);
    else
        hipLaunchKernelGGL(pack_all_kernel<0>, grid, dim3(256), 0, s, w, wp_fwd, wp_d0, wp_d1, Cout, C0, C1, C0p, C1p, ntaps);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_conv3x3_pack_multi(const MnkPackDesc* descs_device, int n, int total_tiles, void* stream) {
    MNK_REQUIRE(descs_device && n > 0 && total_tiles > 0);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(K_CONV_REDUCE, s, (double)total_tiles * 16 * 16 * 9 * 12);
    hipLaunchKernelGGL(pack_multi_kernel, dim3(total_tiles), dim3(256), 0, s, descs_device, n);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

size_t mnk_conv2d_workspace_floats(int N, int Ho, int Wo, int C0, int C1, int Cout, int ntaps) {
    return plan_launch(ntaps, 1, N, Ho, Wo, C0, C1, Cout).ws_floats;
}
size_t mnk_conv2d_stats_floats(int N, int Ho, int Wo, int C0, int C1, int Cout, int ntaps) {
    return plan_launch(ntaps, 1, N, Ho, Wo, C0, C1, Cout).stats_floats;
}

}  // extern "C"

// ---- the GEMM kernel of a plan: block tile (plan_tile_ok) x loader mode x GEMM mode --------------------------------------------
struct IgemmLaunch {
    dim3 grid;
    hipStream_t s;
    bool timed;               // the roofline kernel is timed by its own begin / end stamps
    hipEvent_t ev0, ev1;
    bool pm;                  // the position-major, tap-skipping instantiation (plan_taps)
    int en;                   // the EvalNorm instantiation: 0 none, 1 per element (loader modes 1 .. 3), 2 pooled (loader mode 1)
};
static void launch_igemm(void (*kernel)(ConvArgs), const IgemmLaunch& L, const ConvArgs& a) {
    if (L.timed) hipExtLaunchKernelGGL(kernel, L.grid, dim3(256), 0, L.s, L.ev0, L.ev1, 0, a);
    else hipLaunchKernelGGL(kernel, L.grid, dim3(256), 0, L.s, a);
}
// the 32x32-MFMA kernel of a tile / the 16x16-MFMA kernel of a width, by loader mode; GM: 1 = bf16x3 products, 2 = one-pass bf16
template <int BM, int BN, int WM, int WN, int GM>
static void launch_tile(int mode, const IgemmLaunch& L, const ConvArgs& a) {
    if (L.en == 1) {      // per element (evalnorm_form_of vouches for mode 1 .. 3)
        if constexpr (GM == 0) {
            if (L.pm) {
                if (mode == 1) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 1, 0, true, 1>, L, a);
                else if (mode == 2) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 2, 0, true, 1>, L, a);
                else launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 3, 0, true, 1>, L, a);
                return;
            }
        }
        if (mode == 1) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 1, GM, false, 1>, L, a);
        else if (mode == 2) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 2, GM, false, 1>, L, a);
        else launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 3, GM, false, 1>, L, a);
        return;
    }
    if constexpr (GM == 0) {
        if (L.pm) {       // position-major rows + tap skipping (plan_taps vouches for mode 1 .. 3)
            if (mode == 1) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 1, 0, true>, L, a);
            else if (mode == 2) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 2, 0, true>, L, a);
            else launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 3, 0, true>, L, a);
            return;
        }
    }
    if (mode == 1) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 1, GM>, L, a);
    else if (mode == 2) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 2, GM>, L, a);
    else if (mode == 3) launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 3, GM>, L, a);
    else launch_igemm(conv3x3_igemm_kernel<BM, BN, WM, WN, 0, GM>, L, a);
}
template <int BN, int GM>
static void launch_tile16(int mode, const IgemmLaunch& L, const ConvArgs& a) {
    if (L.en == 1) {      // per element: 3x3 / pad 1 launches only (plan_tile_ok: phases == 1), loader mode 1 or 2
        if (mode == 1) launch_igemm(conv3x3_igemm16_kernel<BN, 1, GM, 1>, L, a);
        else launch_igemm(conv3x3_igemm16_kernel<BN, 2, GM, 1>, L, a);
        return;
    }
    if (mode == 1) launch_igemm(conv3x3_igemm16_kernel<BN, 1, GM>, L, a);
    else if (mode == 2) launch_igemm(conv3x3_igemm16_kernel<BN, 2, GM>, L, a);
    else if (mode == 3) launch_igemm(conv3x3_igemm16_kernel<BN, 3, GM>, L, a);
    else launch_igemm(conv3x3_igemm16_kernel<BN, 0, GM>, L, a);
}
// the window-major kernels: every tile of plan_tile_ok, the plain 3x3 fast loader
template <int GM>
static void launch_plan_tile_win(const Plan& p, const IgemmLaunch& L, const ConvArgs& a) {
    if (p.bn == 16) launch_igemm(conv3x3_igemm16_kernel<16, 1, GM, 2>, L, a);
    else if (p.bn == 48) launch_igemm(conv3x3_igemm16_kernel<48, 1, GM, 2>, L, a);
    else if (p.bn == 128 && p.bm == 128) launch_igemm(conv3x3_igemm_kernel<128, 128, 2, 2, 1, GM, false, 2>, L, a);
    else if (p.bn == 128) launch_igemm(conv3x3_igemm_kernel<64, 128, 1, 4, 1, GM, false, 2>, L, a);
    else if (p.bn == 64 && p.bm == 128) launch_igemm(conv3x3_igemm_kernel<128, 64, 2, 2, 1, GM, false, 2>, L, a);
    else if (p.bn == 64) launch_igemm(conv3x3_igemm_kernel<64, 64, 2, 2, 1, GM, false, 2>, L, a);
    else launch_igemm(conv3x3_igemm_kernel<128, 32, 4, 1, 1, GM, false, 2>, L, a);
}
template <int GM>
static void launch_plan_tile(const Plan& p, int mode, const IgemmLaunch& L, const ConvArgs& a) {
    if (L.en == 2) return launch_plan_tile_win<GM>(p, L, a);
    if (p.bn == 16) launch_tile16<16, GM>(mode, L, a);
    else if (p.bn == 48) launch_tile16<48, GM>(mode, L, a);
    else if (p.bn == 128 && p.bm == 128) launch_tile<128, 128, 2, 2, GM>(mode, L, a);
    else if (p.bn == 128) launch_tile<64, 128, 1, 4, GM>(mode, L, a);
    else if (p.bn == 64 && p.bm == 128) launch_tile<128, 64, 2, 2, GM>(mode, L, a);
    else if (p.bn == 64) launch_tile<64, 64, 2, 2, GM>(mode, L, a);
    else launch_tile<128, 32, 4, 1, GM>(mode, L, a);
}

// the reduction behind ONE split-K launch: sums its partials into y (+ bias, residual) and, with stats_partial, leaves the statistics
static void launch_splitk_reduce(hipStream_t s, float* ws, int splits, long M, int ldw, const float* bias, const float* residual,
                                 int ld_res, float* y, int ld_y, int Cout, int phases, int H, int W, float* stats_partial,
                                 const BnBwdSrc& bnb) {
    ProfScope prof(K_CONV_REDUCE, s, (double)splits * M * ldw * 4);
    if (stats_partial) {
        const RSMap m = make_rsmap(M * phases, ld_y);
        hipLaunchKernelGGL(conv3x3_splitk_reduce_stats_kernel<true>, dim3(m.col_tiles, m.row_blocks), dim3(256), 0, s, ws, splits, M,
                           ldw, bias, residual, ld_res, y, ld_y, Cout, phases, H, W, m.tx, m.ty, m.rows_per_block, stats_partial, bnb);
    } else if (g_reduce_v4 && (size_t)y % 16 == 0 && (size_t)ws % 16 == 0) {
        const RSMap m = make_rsmap(M * phases, ld_y);
        hipLaunchKernelGGL(conv3x3_splitk_reduce_stats_kernel<false>, dim3(m.col_tiles, m.row_blocks), dim3(256), 0, s, ws, splits, M,
                           ldw, bias, residual, ld_res, y, ld_y, Cout, phases, H, W, m.tx, m.ty, m.rows_per_block, (float*)nullptr,
                           BnBwdSrc{});
    } else
        hipLaunchKernelGGL(conv3x3_splitk_reduce_kernel, dim3(grid_for(M * phases * ld_y * 4, 8192)), dim3(256), 0, s, ws, splits, M,
                           ldw, bias, residual, ld_res, y, ld_y, Cout, phases, H, W);
}

// general form behind mnk_conv2d_fwd / mnk_conv3x3_up_fwd / mnk_conv3x3_up_dgrad:
//   phases == 1: Ho x Wo outputs, input pixel of output (h, w), tap (ky, kx) = (h * stride + ky - pad, w * stride + kx - pad)
//   phases == 4: the sub-pixel form of [nearest x2 -> 3x3 / pad 1] (ConvArgs): kh = kw = 2, pad = 1, (Hi, Wi) = (Ho, Wo) =
//                the LOW resolution; y is the (N, 2 Ho, 2 Wo) tensor; wp = four per-phase packs
static int conv2d_fwd_impl(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, int Hi, int Wi, int kh,
                           int kw, int pad, int stride, int phases, const float* wp, const float* bias, const float* residual,
                           int ld_res, float* y, int ld_y, int N, int Ho, int Wo, int Cout, float* ws, size_t ws_floats,
                           float* stats_partial, void* stream, const BnBwdSrc* bnb = nullptr, const EvalNorm* en = nullptr,
                           int pool = 0) {
    // en: the evaluation-mode norm layer applied in the epilogue; (y, ld_y) is then where z goes -- with pool the (N, Ho/2, Wo/2) map
    MNK_REQUIRE(flags >= 0 && flags <= 31);
    MNK_REQUIRE(!en || (en->mean && en->scale && en->beta && !residual && !stats_partial && !bnb &&
                        !(flags & (MNK_CONV_DEFER_SPLITK | MNK_CONV_BF16_TRAIN))));
    MNK_REQUIRE(!pool || (en && phases == 1 && kh == 3 && kw == 3 && pad == 1 && stride == 1 && Ho % 2 == 0 && Wo % 2 == 0));
    const int ups = flags & MNK_CONV_UPSAMPLED, clean = (flags & MNK_CONV_CLEAN_PADS) ? 1 : 0;
    // MNK_CONV_BF16 / MNK_CONV_BF16_TRAIN: the one-pass bf16 products (GM = 2) -- a property of this launch; tile and split are
    // those of the fp32 plan.  MNK_CONV_BF16 is the inference request: the column sums of the epilogue are a training request and
    // stay refused with it.  MNK_CONV_BF16_TRAIN is the training request (mixed precision: the data- and weight-gradient launches
    // of the layer round the same way): the same products, with the fp32 statistics / BatchNorm-backward epilogues behind them
    const bool one_pass = (flags & (MNK_CONV_BF16 | MNK_CONV_BF16_TRAIN)) != 0;
    MNK_REQUIRE(!(flags & MNK_CONV_BF16) || (!stats_partial && !bnb));
    // MNK_CONV_DEFER_SPLITK: a split-K launch leaves its partials in `ws` ([split][phase][M][ldw], bias not added) and the
    // caller sums them (mnk_bn_small_fwd does, together with the normalisation that follows)
    const bool defer_splitk = (flags & MNK_CONV_DEFER_SPLITK) != 0;
    MNK_REQUIRE(x0 && wp && y && N > 0 && Ho > 0 && Wo > 0 && Cout > 0 && C0 > 0 && C1 >= 0);
    MNK_REQUIRE(kh > 0 && kw > 0 && pad >= 0 && Hi > 0 && Wi > 0 && stride >= 1 && (phases == 1 || phases == 4));
    if (phases == 4)
        MNK_REQUIRE(kh == 2 && kw == 2 && pad == 1 && stride == 1 && Ho == Hi && Wo == Wi && !ups && clean && !residual);
    else
        MNK_REQUIRE(Ho == (Hi + 2 * pad - kh) / stride + 1 && Wo == (Wi + 2 * pad - kw) / stride + 1);
    MNK_REQUIRE(stride == 1 || (clean && !ups));
    MNK_REQUIRE(ld0 % 4 == 0 && ld0 >= C0 && ld_y % 4 == 0 && ld_y >= Cout && ld_y <= round_up(Cout, 16));
    MNK_REQUIRE(C1 == 0 || (x1 && ld1 % 4 == 0 && ld1 >= C1));
    MNK_REQUIRE(!ups || (Hi % 2 == 0 && Wi % 2 == 0));
    MNK_REQUIRE(!residual || (ld_res >= Cout));
    const int ntaps = kh * kw;
    ConvArgs a;
    a.x0 = x0;
    a.x1 = x1;
    a.ld0 = ld0;
    a.ld1 = ld1;
    a.C0 = C0;
    a.C1 = C1;
    a.C0p = round_up(C0, 16);
    a.C1p = C1 > 0 ? round_up(C1, 16) : 0;
    a.ups = ups;
    a.clean = clean;
    a.wp = wp;
    a.bias = bias;
    a.residual = residual;
    a.ld_res = ld_res;
    a.y = y;
    a.ld_y = ld_y;
    a.N = N;
    a.H = Ho;
    a.W = Wo;
    a.Hi = Hi;
    a.Wi = Wi;
    a.ntaps = ntaps;
    a.kw = kw;
    a.pad = pad;
    a.Cout = Cout;
    a.M = (long)N * Ho * Wo;
    MNK_REQUIRE(a.M * phases < (1L << 31) && a.M * phases * round_up(Cout, 16) < (1L << 32) &&
                (!residual || a.M * ld_res < (1L << 32)));
    fast_div_consts((unsigned)Wo, &a.mulW, &a.shW);
    fast_div_consts((unsigned)Ho, &a.mulH, &a.shH);
    a.chunks = (a.C0p + a.C1p) / 16;
    a.stride = stride;
    a.pad_x = -1;
    const Launch l = plan_launch(ntaps, phases, N, Ho, Wo, C0, C1, Cout);
    const Plan& p = l.p;
    a.phases = phases;
    a.tiles_per_phase = p.gm;
    a.phase_wstride = (long)Cout * ntaps * (a.C0p + a.C1p);
    a.ksteps = p.ksteps;
    a.ksteps_per_split = p.ksteps_per_split;
    a.splits = p.splits;
    a.ws = ws;
    a.ldw = p.ldw;
    a.stats = stats_partial;
    a.bnb = bnb ? *bnb : BnBwdSrc{};
    a.en = en ? *en : EvalNorm{};
    a.en.z = y, a.en.ld_z = ld_y;
    fast_div_consts((unsigned)(Wo > 1 ? Wo / 2 : 1), &a.mulWo, &a.shWo);
    fast_div_consts((unsigned)(Ho > 1 ? Ho / 2 : 1), &a.mulHo, &a.shHo);
    MNK_REQUIRE(!bnb || (stats_partial && bnb->y && bnb->mean && bnb->invstd && bnb->scale && bnb->beta && bnb->ld >= Cout &&
                         phases == 1 && !defer_splitk));
    a.xcd = g_xcd_remap;
    // statistics: only where the query answers > 0, and not from partials that are left to the caller
    MNK_REQUIRE(!stats_partial || (ld_y == round_up(Cout, 4) && l.stats_floats && (p.splits == 1 || !defer_splitk)));
    if (en && p.splits > 1) {      // (in front of the workspace check: such a launch has no workspace to offer)
        set_error("a convolution with the evaluation-mode norm layer in its epilogue is not possible at this shape and tuning "
                  "(mnk_conv3x3_evalnorm_form answers 0: the plan splits K %d times)", p.splits);
        return MNK_EINVAL;
    }
    if (l.ws_floats && (!ws || ws_floats < l.ws_floats)) {
        set_error("mnk_conv2d_fwd: workspace too small (%zu < %zu floats)", ws_floats, l.ws_floats);
        return MNK_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(p.gm * phases, p.gn, p.splits);
    {
        // algorithmic FLOPs of the convolution this launch stands for: the sub-pixel form computes a 3x3 convolution on
        // 4 M output pixels; a stride-2 4x4 data gradient stands for the 3x3 data gradient at 4 M pixels
        const double alg = phases == 4 ? 2.0 * 4.0 * (double)a.M * Cout * 9.0 * (C0 + C1)
                                       : (stride == 2 ? 2.0 * 4.0 * (double)a.M * Cout * 9.0 * (C0 + C1)
                                                      : 2.0 * (double)a.M * Cout * (double)ntaps * (C0 + C1));
        const int ldmax = ld0 > ld1 ? ld0 : ld1;
        const bool aligned = (size_t)x0 % 16 == 0 && (!x1 || (size_t)x1 % 16 == 0);
        const int mode = loader_mode(a.clean, ups, kh, kw, pad, stride, phases, Wi, ldmax, aligned);
        MNK_REQUIRE((stride == 1 && phases == 1) ||
                    (g_fast_loader && g_kxk_fast && ntaps <= 32 && kxk_span_bytes(kh, kw, stride, Wi, ldmax) < (1L << 29) &&
                     aligned));                                // strided / sub-pixel forms exist for the K x K buffer loader only
        // position-major rows where that lets blocks skip the K steps of taps that only read padding (plan_taps)
        const TapGeom tg = {p.bm, N, Ho, Wo, Hi, Wi, kh, kw, pad, stride, phases};
        const long src_pixels = (long)N * (ups ? Hi / 2 : Hi) * (ups ? Wi / 2 : Wi);
        double row_taps;
        const bool pm = plan_taps(p, mode, one_pass, stats_partial && p.splits == 1, tg, src_pixels * (ld0 > ld1 ? ld0 : ld1) * 4, &row_taps);
        fast_div_consts((unsigned)N, &a.mulF, &a.shF);
        fast_div_consts((unsigned)kw, &a.mulKW, &a.shKW);
        // a launch that applies the norm layer behind it: refused where the form query answers 0, never computed another way
        const int en_form = en ? evalnorm_form_of(p, mode, pm, pool, Wi, ldmax) : 0;
        if (en && !en_form) {
            set_error("a convolution with the evaluation-mode norm layer in its epilogue is not possible at this shape and tuning "
                      "(mnk_conv3x3_evalnorm_form answers 0: loader %d, %s rows%s)", mode, pm ? "position-major" : "frame-major",
                      pool ? ", pooled" : "");
            return MNK_EINVAL;
        }
        g_last_evalnorm_form = en_form;
        // what the launch issues: the sub-pixel forms run 4 (forward) / 16 at a quarter of the pixels (data gradient) taps; a
        // position-major launch only the (row, tap) pairs of the taps its tiles do not skip
        ProfScope prof(K_CONV_FWD, s, alg, 2.0 * row_taps * Cout * (double)(C0 + C1));
        // the roofline kernel is timed by its own begin / end stamps (bench.py `roofline`, agrees with rocprofv3)
        hipEvent_t ev0, ev1;
        const bool timed = prof.kernel_events(&ev0, &ev1);
        // (padding a block's LDS request so that exactly ceil(blocks / CUs) blocks fit a CU was built and measured in round 4: the
        // dispatcher already puts 1024 blocks on 256 CUs four by four -- tools/microbench/launch_gap.hip (e) -- and the step did
        // not move, 10.33 vs 10.32 ms: removed.  profiles/r04_knob_ab_log.txt)
        const IgemmLaunch L = {grid, s, timed, ev0, ev1, pm, en_form};
        if (one_pass) launch_plan_tile<2>(p, mode, L, a);
        else if (p.bn == 16 || p.bn == 48 ? g_gemm16_bf16x3 : g_gemm_bf16x3) launch_plan_tile<1>(p, mode, L, a);
        else launch_plan_tile<0>(p, mode, L, a);
    }
    if (p.splits > 1 && !defer_splitk)
        launch_splitk_reduce(s, ws, p.splits, a.M, p.ldw, bias, residual, ld_res, y, ld_y, Cout, phases, a.H, a.W, stats_partial, a.bnb);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

// ---- the data gradients of an up-sampled convolution w.r.t. BOTH of its sources [previous output | skip] in one launch ----------
// Each source's launch is described as conv2d_fwd_impl describes it on its own (4x4 / stride 2 / pad 1 over dy: plan, loader,
// row order, work); the two are one grid when the kernel can be one instantiation for both.
static int g_dgrad_pair = tuning_knob("dgrad_pair", &g_dgrad_pair, 1);      // 0: the two launches of the single entries (A/B runs, tests)

struct UpDgradSide {
    Launch l;
    int mode;
    bool pm;
    double row_taps, alg;
};
// bn: the launch is asked for the backward statistics of the norm layer in front.  (H, W): the low resolution
static UpDgradSide up_dgrad_side(int ld_dy, bool aligned, int Cout, int N, int H, int W, int C, bool bn) {
    UpDgradSide d;
    d.l = plan_launch(16, 1, N, H, W, Cout, 0, C);
    d.mode = loader_mode(true, 0, 4, 4, 1, 2, 1, 2 * W, ld_dy, aligned);
    const TapGeom tg = {d.l.p.bm, N, H, W, 2 * H, 2 * W, 4, 4, 1, 2, 1};
    d.pm = plan_taps(d.l.p, d.mode, false, bn && d.l.p.splits == 1, tg, (long)N * 2 * H * 2 * W * ld_dy * 4, &d.row_taps);
    d.alg = 2.0 * 4.0 * (double)N * H * W * C * 9.0 * Cout;
    return d;
}
// the tiles the pair kernels are instantiated for (up_dgrad_pair_impl): the ones the flagship's thirteen pairs run on
static bool pair_tile_ok(const Plan& p) { return p.bn == 64 && (p.bm == 64 || p.bm == 128); }
// 0: two launches; 1: one GEMM launch (+ a reduction per source that splits); 2: one GEMM launch and one reduction.
// One kernel instantiation must serve both: the same block tile (both in the 32x32-MFMA family), loader, row order, fp32 products
static int up_dgrad_pair_form(const UpDgradSide& d0, const UpDgradSide& d1, bool bn0, bool bn1, bool reduce_aligned) {
    if (!g_dgrad_pair || g_gemm_bf16x3) return 0;
    const Plan &p0 = d0.l.p, &p1 = d1.l.p;
    if (d0.l.p.gm <= 0 || d1.l.p.gm <= 0 || !pair_tile_ok(p0) || !pair_tile_ok(p1) || p0.bm != p1.bm || p0.bn != p1.bn) return 0;
    if (d0.mode != 3 || d1.mode != 3 || d0.pm != d1.pm) return 0;
    if (d0.pm && p0.bm != 64) return 0;       // (the position-major 128-row tile needs 134 registers: not instantiated as a pair)
    if (p0.splits == 1 || p1.splits == 1) return 1;
    // the merged reduction is the float4-row kernel: each source must take that kernel on its own
    return ((bn0 || (g_reduce_v4 && reduce_aligned)) && (bn1 || (g_reduce_v4 && reduce_aligned))) ? 2 : 1;
}


struct UpDgradOut {
    const float* wp;
    float* dx;
    int ld_dx, C;
    float* stats;
    const BnBwdSrc* bnb;
};
static int up_dgrad_pair_impl(const char* who, const float* dy, int ld_dy, int Cout, const UpDgradOut (&o)[2], int N, int H, int W,
                              float* ws, size_t ws_floats, void* stream) {
    MNK_REQUIRE_FOR(who, dy && N > 0 && H > 0 && W > 0 && Cout > 0 && ld_dy % 4 == 0 && ld_dy >= Cout);
    UpDgradSide d[2];
    for (int i = 0; i < 2; ++i) {
        MNK_REQUIRE_FOR(who, o[i].wp && o[i].dx && o[i].C > 0 && o[i].ld_dx % 4 == 0 && o[i].ld_dx >= o[i].C &&
                                 o[i].ld_dx <= round_up(o[i].C, 16));
        MNK_REQUIRE_FOR(who, (long)N * H * W < (1L << 31) && (long)N * H * W * round_up(o[i].C, 16) < (1L << 32));
        MNK_REQUIRE_FOR(who, (o[i].stats != nullptr) == (o[i].bnb != nullptr));
        d[i] = up_dgrad_side(ld_dy, (size_t)dy % 16 == 0, Cout, N, H, W, o[i].C, o[i].stats != nullptr);
        const BnBwdSrc* b = o[i].bnb;
        MNK_REQUIRE_FOR(who, !b || (b->y && b->mean && b->invstd && b->scale && b->beta && b->ld >= o[i].C &&
                                    o[i].ld_dx == round_up(o[i].C, 4) && d[i].l.stats_floats));
    }
    const size_t ws0 = d[0].l.ws_floats, ws1 = d[1].l.ws_floats;       // (multiples of 4 floats: ldw is)
    float* const wsv[2] = {ws, ws ? ws + ws0 : nullptr};
    const bool reduce_aligned = (size_t)ws % 16 == 0 && (size_t)o[0].dx % 16 == 0 && (size_t)o[1].dx % 16 == 0;
    const int form = up_dgrad_pair_form(d[0], d[1], o[0].stats != nullptr, o[1].stats != nullptr, reduce_aligned);
    if (!form) {
        set_error("%s: this pair is not one launch at this shape and tuning (mnk_conv3x3_up_dgrad_pair_form answers 0): run the "
                  "two single launches", who);
        return MNK_EINVAL;
    }
    if (ws0 + ws1 && (!ws || ws_floats < ws0 + ws1)) {
        set_error("%s: workspace too small (%zu < %zu floats)", who, ws_floats, ws0 + ws1);
        return MNK_EWORKSPACE;
    }
    const Plan &p0 = d[0].l.p, &p1 = d[1].l.p;
    ConvArgs a{};
    a.x0 = dy, a.ld0 = ld_dy, a.C0 = Cout, a.C0p = round_up(Cout, 16);
    a.clean = 1;
    a.N = N, a.H = H, a.W = W, a.Hi = 2 * H, a.Wi = 2 * W;
    a.ntaps = 16, a.kw = 4, a.pad = 1, a.stride = 2, a.pad_x = -1;
    a.M = (long)N * H * W;
    a.chunks = a.C0p / 16;
    a.phases = 1, a.tiles_per_phase = p0.gm;
    a.ksteps = p0.ksteps;
    a.xcd = g_xcd_remap;
    fast_div_consts((unsigned)W, &a.mulW, &a.shW);
    fast_div_consts((unsigned)H, &a.mulH, &a.shH);
    fast_div_consts((unsigned)N, &a.mulF, &a.shF);
    fast_div_consts(4u, &a.mulKW, &a.shKW);
    fast_div_consts((unsigned)(W > 1 ? W / 2 : 1), &a.mulWo, &a.shWo);
    fast_div_consts((unsigned)(H > 1 ? H / 2 : 1), &a.mulHo, &a.shHo);
    a.wp = o[0].wp, a.y = o[0].dx, a.ld_y = o[0].ld_dx, a.Cout = o[0].C;
    a.phase_wstride = (long)o[0].C * 16 * a.C0p;
    a.ksteps_per_split = p0.ksteps_per_split, a.splits = p0.splits, a.ws = wsv[0], a.ldw = p0.ldw;
    a.stats = o[0].stats;
    a.bnb = o[0].bnb ? *o[0].bnb : BnBwdSrc{};
    a.gn0 = p0.gn;
    a.o1.wp = o[1].wp, a.o1.y = o[1].dx, a.o1.ld_y = o[1].ld_dx, a.o1.Cout = o[1].C, a.o1.gn = p1.gn;
    a.o1.ksteps_per_split = p1.ksteps_per_split, a.o1.splits = p1.splits, a.o1.ws = wsv[1], a.o1.ldw = p1.ldw;
    a.o1.stats = o[1].stats;
    a.o1.bnb = o[1].bnb ? *o[1].bnb : BnBwdSrc{};
    hipStream_t s = (hipStream_t)stream;
    g_last_evalnorm_form = 0;
    {
        // ONE launch in the recorder, with the work of both
        ProfScope prof(K_CONV_FWD, s, d[0].alg + d[1].alg, 2.0 * Cout * (d[0].row_taps * o[0].C + d[1].row_taps * o[1].C));
        hipEvent_t ev0, ev1;
        const bool timed = prof.kernel_events(&ev0, &ev1);
        const IgemmLaunch L = {dim3(p0.gm, p0.gn + p1.gn, p0.splits > p1.splits ? p0.splits : p1.splits), s, timed, ev0, ev1, d[0].pm, 0};
        if (p0.bm == 128) launch_igemm(conv3x3_igemm_kernel<128, 64, 2, 2, 3, 0, false, 0, true>, L, a);
        else if (d[0].pm) launch_igemm(conv3x3_igemm_kernel<64, 64, 2, 2, 3, 0, true, 0, true>, L, a);
        else launch_igemm(conv3x3_igemm_kernel<64, 64, 2, 2, 3, 0, false, 0, true>, L, a);
    }
    if (form == 2) {
        ProfScope prof(K_CONV_REDUCE, s, ((double)p0.splits * p0.ldw + (double)p1.splits * p1.ldw) * a.M * 4);
        RsOut r[2];
        for (int i = 0; i < 2; ++i) {
            const Plan& p = d[i].l.p;
            const RSMap m = make_rsmap(a.M, o[i].ld_dx);
            r[i].ws = wsv[i], r[i].splits = p.splits, r[i].ldw = p.ldw, r[i].y = o[i].dx, r[i].ld_y = o[i].ld_dx, r[i].Cout = o[i].C;
            r[i].tx_n = m.tx, r[i].ty_n = m.ty, r[i].col_tiles = m.col_tiles, r[i].row_blocks = m.row_blocks;
            r[i].rows_per_block = m.rows_per_block;
            r[i].stats = o[i].stats;
            r[i].bnb = o[i].bnb ? *o[i].bnb : BnBwdSrc{};
        }
        hipLaunchKernelGGL(conv3x3_splitk_reduce_pair_kernel,
                           dim3(r[0].col_tiles + r[1].col_tiles, r[0].row_blocks > r[1].row_blocks ? r[0].row_blocks : r[1].row_blocks),
                           dim3(256), 0, s, r[0], r[1], a.M, H, W);
    } else {
        // a source that does not split has no partials to sum; the other keeps the reduction it has on its own
        for (int i = 0; i < 2; ++i)
            if (d[i].l.p.splits > 1)
                launch_splitk_reduce(s, wsv[i], d[i].l.p.splits, a.M, d[i].l.p.ldw, nullptr, nullptr, 0, o[i].dx, o[i].ld_dx, o[i].C, 1, H,
                                     W, o[i].stats, o[i].bnb ? *o[i].bnb : BnBwdSrc{});
    }
    MNK_LAUNCH_CHECK_FOR(who);
    return MNK_OK;
}

extern "C" {

int mnk_conv2d_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, int Hi, int Wi, int kh,
                   int kw, int pad, const float* wp, const float* bias, const float* residual, int ld_res, float* y,
                   int ld_y, int N, int Ho, int Wo, int Cout, float* ws, size_t ws_floats, float* stats_partial,
                   void* stream) {
    return conv2d_fwd_impl(x0, ld0, C0, x1, ld1, C1, flags, Hi, Wi, kh, kw, pad, 1, 1, wp, bias, residual, ld_res, y, ld_y, N,
                           Ho, Wo, Cout, ws, ws_floats, stats_partial, stream);
}

// launch-plan switches are read from the environment when the library is loaded; this sets one afterwards (A/B runs, tests)
// the last forward / data-gradient launch plan that was made: {M, Cout, chunks, taps, phases, bm, bn, splits}
int mnk_last_plan(long* out8) {
    MNK_REQUIRE(out8);
    for (int i = 0; i < 8; ++i) out8[i] = g_last_plan[i];
    return MNK_OK;
}

// ---- sub-pixel forms of UpBlock3D's [nearest x2 -> 3x3 / pad 1] (modules/util.py:83-85): (H, W) = LOW resolution -----------
size_t mnk_conv3x3_up_packed_floats(int Cout, int C0, int C1) {
    if (Cout <= 0 || C0 <= 0 || C1 < 0) return 0;
    return (size_t)16 * Cout * (round_up(C0, 16) + (C1 > 0 ? round_up(C1, 16) : 0));
}
size_t mnk_conv3x3_up_dgrad_packed_floats(int Cout, int c_count) {
    if (Cout <= 0 || c_count <= 0) return 0;
    return (size_t)c_count * 16 * round_up(Cout, 16);
}
int mnk_conv3x3_up_pack_fwd(const float* w, float* wp, int Cout, int C0, int C1, void* stream) {
    MNK_REQUIRE(w && wp && Cout > 0 && C0 > 0 && C1 >= 0);
    hipStream_t s = (hipStream_t)stream;
    const int C0p = round_up(C0, 16), C1p = C1 > 0 ? round_up(C1, 16) : 0;
    const long total = (long)16 * Cout * (C0p + C1p);
    ProfScope prof(K_CONV_REDUCE, s, (double)total * 8);
    hipLaunchKernelGGL(pack_up_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, w, wp, Cout, C0, C1, C0p, C1p);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}
int mnk_conv3x3_up_pack_dgrad(const float* w, float* wp, int Cout, int Cin_total, int c_start, int c_count, void* stream) {
    MNK_REQUIRE(w && wp && Cout > 0 && Cin_total > 0 && c_start >= 0 && c_count > 0 && c_start + c_count <= Cin_total);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = round_up(Cout, 16) / 16;
    const long total = (long)c_count * chunks * 256;
    ProfScope prof(K_CONV_REDUCE, s, (double)total * 8);
    hipLaunchKernelGGL(pack_up_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, s, w, wp, Cout, Cin_total, c_start, c_count,
                       chunks);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}
size_t mnk_conv3x3_up_workspace_floats(int N, int H, int W, int C0, int C1, int Cout) {
    return plan_launch(4, 4, N, H, W, C0, C1, Cout).ws_floats;
}
size_t mnk_conv3x3_up_stats_floats(int N, int H, int W, int C0, int C1, int Cout) {
    return plan_launch(4, 4, N, H, W, C0, C1, Cout).stats_floats;
}
int mnk_conv3x3_up_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, const float* wp_up,
                       const float* bias, float* y, int ld_y, int N, int H, int W, int Cout, float* ws, size_t ws_floats,
                       float* stats_partial, void* stream) {
    MNK_REQUIRE((flags & ~(MNK_CONV_DEFER_SPLITK | MNK_CONV_BF16 | MNK_CONV_BF16_TRAIN)) == 0);
    return conv2d_fwd_impl(x0, ld0, C0, x1, ld1, C1, MNK_CONV_CLEAN_PADS | flags, H, W, 2, 2, 1, 1, 4, wp_up, bias, nullptr, 0, y,
                           ld_y, N, H, W, Cout, ws, ws_floats, stats_partial, stream);
}
// pixel-independent K splits of the launches above (1: no split): what a caller that sums the partials itself must know
int mnk_conv3x3_splits(int N, int H, int W, int C0, int C1, int Cout) { return plan_launch(9, 1, N, H, W, C0, C1, Cout).p.splits; }
int mnk_conv3x3_up_splits(int N, int H, int W, int C0, int C1, int Cout) { return plan_launch(4, 4, N, H, W, C0, C1, Cout).p.splits; }
// data gradient w.r.t. one low-resolution source of an up-sampled convolution: dy (N, 2H, 2W, Cout) -> dx (N, H, W, C)
size_t mnk_conv3x3_up_dgrad_workspace_floats(int N, int H, int W, int Cout, int C) {
    return plan_launch(16, 1, N, H, W, Cout, 0, C).ws_floats;
}
// the data-gradient entries without a `flags` argument have an _ex form that takes one: 0 or MNK_CONV_BF16_TRAIN
int mnk_conv3x3_up_dgrad_ex(const float* dy, int ld_dy, int Cout, const float* wp_up_dgrad, float* dx, int ld_dx, int N, int H,
                            int W, int C, float* ws, size_t ws_floats, int flags, void* stream) {
    MNK_REQUIRE((flags & ~MNK_CONV_BF16_TRAIN) == 0);
    return conv2d_fwd_impl(dy, ld_dy, Cout, nullptr, 0, 0, MNK_CONV_CLEAN_PADS | flags, 2 * H, 2 * W, 4, 4, 1, 2, 1, wp_up_dgrad,
                           nullptr, nullptr, 0, dx, ld_dx, N, H, W, C, ws, ws_floats, nullptr, stream);
}
int mnk_conv3x3_up_dgrad(const float* dy, int ld_dy, int Cout, const float* wp_up_dgrad, float* dx, int ld_dx, int N, int H,
                         int W, int C, float* ws, size_t ws_floats, void* stream) {
    return mnk_conv3x3_up_dgrad_ex(dy, ld_dy, Cout, wp_up_dgrad, dx, ld_dx, N, H, W, C, ws, ws_floats, 0, stream);
}

// ---- data-gradient launches that also leave the backward statistics of the BatchNorm layer in front (round 4) ------------------
static BnBwdSrc bnb_of(const float* bn_y, int ld_bny, const float* mean, const float* invstd, const float* scale, const float* beta,
                       float slope) {
    BnBwdSrc b;
    b.y = bn_y, b.ld = ld_bny, b.mean = mean, b.invstd = invstd, b.scale = scale, b.beta = beta, b.slope = slope;
    return b;
}
int mnk_conv3x3_dgrad_bnstats_ex(const float* dy, int ld_dy, int Cout, const float* wp_dgrad, const float* residual, int ld_res,
                                 float* dx, int ld_dx, int N, int H, int W, int C, float* ws, size_t ws_floats, float* stats_partial,
                                 const float* bn_y, int ld_bny, const float* bn_mean, const float* bn_invstd, const float* bn_scale,
                                 const float* bn_beta, float slope, int flags, void* stream) {
    MNK_REQUIRE((flags & ~MNK_CONV_BF16_TRAIN) == 0);
    const BnBwdSrc b = bnb_of(bn_y, ld_bny, bn_mean, bn_invstd, bn_scale, bn_beta, slope);
    return conv2d_fwd_impl(dy, ld_dy, Cout, nullptr, 0, 0, MNK_CONV_CLEAN_PADS | flags, H, W, 3, 3, 1, 1, 1, wp_dgrad, nullptr,
                           residual, ld_res, dx, ld_dx, N, H, W, C, ws, ws_floats, stats_partial, stream, &b);
}
int mnk_conv3x3_dgrad_bnstats(const float* dy, int ld_dy, int Cout, const float* wp_dgrad, const float* residual, int ld_res,
                              float* dx, int ld_dx, int N, int H, int W, int C, float* ws, size_t ws_floats, float* stats_partial,
                              const float* bn_y, int ld_bny, const float* bn_mean, const float* bn_invstd, const float* bn_scale,
                              const float* bn_beta, float slope, void* stream) {
    return mnk_conv3x3_dgrad_bnstats_ex(dy, ld_dy, Cout, wp_dgrad, residual, ld_res, dx, ld_dx, N, H, W, C, ws, ws_floats,
                                        stats_partial, bn_y, ld_bny, bn_mean, bn_invstd, bn_scale, bn_beta, slope, 0, stream);
}
size_t mnk_conv3x3_up_dgrad_stats_floats(int N, int H, int W, int Cout, int C) {
    return plan_launch(16, 1, N, H, W, Cout, 0, C).stats_floats;
}
int mnk_conv3x3_up_dgrad_bnstats_ex(const float* dy, int ld_dy, int Cout, const float* wp_up_dgrad, float* dx, int ld_dx, int N,
                                    int H, int W, int C, float* ws, size_t ws_floats, float* stats_partial, const float* bn_y,
                                    int ld_bny, const float* bn_mean, const float* bn_invstd, const float* bn_scale,
                                    const float* bn_beta, float slope, int flags, void* stream) {
    MNK_REQUIRE((flags & ~MNK_CONV_BF16_TRAIN) == 0);
    const BnBwdSrc b = bnb_of(bn_y, ld_bny, bn_mean, bn_invstd, bn_scale, bn_beta, slope);
    return conv2d_fwd_impl(dy, ld_dy, Cout, nullptr, 0, 0, MNK_CONV_CLEAN_PADS | flags, 2 * H, 2 * W, 4, 4, 1, 2, 1, wp_up_dgrad,
                           nullptr, nullptr, 0, dx, ld_dx, N, H, W, C, ws, ws_floats, stats_partial, stream, &b);
}
int mnk_conv3x3_up_dgrad_bnstats(const float* dy, int ld_dy, int Cout, const float* wp_up_dgrad, float* dx, int ld_dx, int N, int H,
                                 int W, int C, float* ws, size_t ws_floats, float* stats_partial, const float* bn_y, int ld_bny,
                                 const float* bn_mean, const float* bn_invstd, const float* bn_scale, const float* bn_beta,
                                 float slope, void* stream) {
    return mnk_conv3x3_up_dgrad_bnstats_ex(dy, ld_dy, Cout, wp_up_dgrad, dx, ld_dx, N, H, W, C, ws, ws_floats, stats_partial, bn_y,
                                           ld_bny, bn_mean, bn_invstd, bn_scale, bn_beta, slope, 0, stream);
}

// ---- the pair form: both sources' data gradients of an up-sampled two-source convolution in one launch ------------------------
int mnk_conv3x3_up_dgrad_pair_form(int N, int H, int W, int Cout, int C0, int C1, int bn0, int bn1) {
    if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || C0 <= 0 || C1 <= 0) return 0;
    const int ld_dy = round_up(Cout, 4);
    const UpDgradSide d0 = up_dgrad_side(ld_dy, true, Cout, N, H, W, C0, bn0 != 0), d1 = up_dgrad_side(ld_dy, true, Cout, N, H, W, C1, bn1 != 0);
    if ((bn0 && !d0.l.stats_floats) || (bn1 && !d1.l.stats_floats)) return 0;
    return up_dgrad_pair_form(d0, d1, bn0 != 0, bn1 != 0, true);
}
size_t mnk_conv3x3_up_dgrad_pair_workspace_floats(int N, int H, int W, int Cout, int C0, int C1) {
    return plan_launch(16, 1, N, H, W, Cout, 0, C0).ws_floats + plan_launch(16, 1, N, H, W, Cout, 0, C1).ws_floats;
}
size_t mnk_conv3x3_up_dgrad_pair_stats_floats(int N, int H, int W, int Cout, int C0, int C1) {
    return plan_launch(16, 1, N, H, W, Cout, 0, C0).stats_floats + plan_launch(16, 1, N, H, W, Cout, 0, C1).stats_floats;
}
int mnk_conv3x3_up_dgrad_pair(const float* dy, int ld_dy, int Cout, const float* wp0, const float* wp1, float* dx0, int ld_dx0,
                              float* dx1, int ld_dx1, int N, int H, int W, int C0, int C1, float* ws, size_t ws_floats,
                              void* stream) {
    const UpDgradOut o[2] = {{wp0, dx0, ld_dx0, C0, nullptr, nullptr}, {wp1, dx1, ld_dx1, C1, nullptr, nullptr}};
    return up_dgrad_pair_impl(__func__, dy, ld_dy, Cout, o, N, H, W, ws, ws_floats, stream);
}
int mnk_conv3x3_up_dgrad_pair_bnstats(const float* dy, int ld_dy, int Cout, const float* wp0, const float* wp1, float* dx0,
                                      int ld_dx0, float* dx1, int ld_dx1, int N, int H, int W, int C0, int C1, float* ws,
                                      size_t ws_floats, float* stats0, const float* bn_y0, int ld_bny0, const float* bn_mean0,
                                      const float* bn_invstd0, const float* bn_scale0, const float* bn_beta0, float slope0,
                                      float* stats1, const float* bn_y1, int ld_bny1, const float* bn_mean1,
                                      const float* bn_invstd1, const float* bn_scale1, const float* bn_beta1, float slope1,
                                      void* stream) {
    const BnBwdSrc b0 = bnb_of(bn_y0, ld_bny0, bn_mean0, bn_invstd0, bn_scale0, bn_beta0, slope0),
                   b1 = bnb_of(bn_y1, ld_bny1, bn_mean1, bn_invstd1, bn_scale1, bn_beta1, slope1);
    const UpDgradOut o[2] = {{wp0, dx0, ld_dx0, C0, stats0, stats0 ? &b0 : nullptr}, {wp1, dx1, ld_dx1, C1, stats1, stats1 ? &b1 : nullptr}};
    return up_dgrad_pair_impl(__func__, dy, ld_dy, Cout, o, N, H, W, ws, ws_floats, stream);
}

// ---- 3x3 / pad 1 forms (the hot path's nn.Conv3d (1,3,3)) ------------------------------------------------------------
size_t mnk_conv3x3_packed_floats(int Cout, int C0, int C1) { return mnk_conv2d_packed_floats(Cout, C0, C1, 9); }
int mnk_conv3x3_pack_fwd(const float* w, float* wp, int Cout, int C0, int C1, void* stream) {
    return mnk_conv2d_pack_fwd(w, wp, Cout, C0, C1, 9, stream);
}
int mnk_conv3x3_pack_all(const float* w, float* wp_fwd, float* wp_d0, float* wp_d1, int Cout, int C0, int C1,
                         void* stream) {
    return mnk_conv2d_pack_all(w, wp_fwd, wp_d0, wp_d1, Cout, C0, C1, 9, stream);
}
int mnk_conv3x3_pack_dgrad(const float* w, float* wp, int Cout, int Cin_total, int c_start, int c_count, void* stream) {
    return mnk_conv2d_pack_dgrad(w, wp, Cout, Cin_total, c_start, c_count, 9, stream);
}
size_t mnk_conv3x3_workspace_floats(int N, int H, int W, int C0, int C1, int Cout) {
    return mnk_conv2d_workspace_floats(N, H, W, C0, C1, Cout, 9);
}
size_t mnk_conv3x3_stats_floats(int N, int H, int W, int C0, int C1, int Cout) {
    return mnk_conv2d_stats_floats(N, H, W, C0, C1, Cout, 9);
}
int mnk_conv3x3_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, const float* wp,
                    const float* bias, const float* residual, int ld_res, float* y, int ld_y, int N, int H, int W,
                    int Cout, float* ws, size_t ws_floats, float* stats_partial, void* stream) {
    return mnk_conv2d_fwd(x0, ld0, C0, x1, ld1, C1, flags, H, W, 3, 3, 1, wp, bias, residual, ld_res, y, ld_y, N, H, W, Cout,
                          ws, ws_floats, stats_partial, stream);
}

// ---- forward launches that apply the evaluation-mode norm layer behind them (EvalNorm) ------------------------------------------
// what the launch entries below will do at this shape under the current tuning: 0 refuse, 1 per element, 2 with the pool.  The
// query assumes what the library's own activations have: sources on 16-byte boundaries with leading dimension round_up(C, 4)
int mnk_conv3x3_evalnorm_form(int N, int H, int W, int C0, int C1, int Cout, int flags, int up, int pool) {
    if (N <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0 || flags < 0 || flags > 31) return 0;
    if (flags & (MNK_CONV_DEFER_SPLITK | MNK_CONV_BF16_TRAIN)) return 0;
    if (up && (pool || (flags & ~MNK_CONV_BF16))) return 0;
    if (pool && (H % 2 || W % 2)) return 0;
    const int ups = up ? 0 : (flags & MNK_CONV_UPSAMPLED), kk = up ? 2 : 3, phases = up ? 4 : 1;
    if (ups && (H % 2 || W % 2)) return 0;
    const Launch l = plan_launch(kk * kk, phases, N, H, W, C0, C1, Cout);
    const int ldmax = round_up(C0 > C1 ? C0 : C1, 4);
    const int mode = loader_mode(up || (flags & MNK_CONV_CLEAN_PADS), ups, kk, kk, 1, 1, phases, W, ldmax, true);
    if (up && mode != 3) return 0;           // the sub-pixel form exists for the K x K buffer loader only
    const TapGeom tg = {l.p.bm, N, H, W, H, W, kk, kk, 1, 1, phases};
    const long src_pixels = (long)N * (ups ? H / 2 : H) * (ups ? W / 2 : W);
    double row_taps;
    const bool pm = plan_taps(l.p, mode, (flags & MNK_CONV_BF16) != 0, false, tg, src_pixels * ldmax * 4, &row_taps);
    return evalnorm_form_of(l.p, mode, pm, pool, W, ldmax);
}
// the form of the last forward launch: 0 a plain launch, 1 / 2 as above (tests: what the query promised is what ran)
int mnk_conv3x3_last_evalnorm_form(void) { return g_last_evalnorm_form; }

static EvalNorm evalnorm_of(const float* mean, const float* scale, const float* beta, int relu) {
    EvalNorm e;
    e.mean = mean, e.scale = scale, e.beta = beta, e.slope = relu ? 0.f : -1.f, e.z = nullptr, e.ld_z = 0;
    return e;
}
int mnk_conv3x3_fwd_evalnorm(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, const float* wp,
                             const float* bias, const float* mean, const float* scale, const float* beta, int relu, int pool,
                             float* z, int ld_z, int N, int H, int W, int Cout, void* stream) {
    MNK_REQUIRE(mean && scale && beta && z && (flags & ~(MNK_CONV_UPSAMPLED | MNK_CONV_CLEAN_PADS | MNK_CONV_BF16)) == 0);
    const EvalNorm e = evalnorm_of(mean, scale, beta, relu);
    return conv2d_fwd_impl(x0, ld0, C0, x1, ld1, C1, flags, H, W, 3, 3, 1, 1, 1, wp, bias, nullptr, 0, z, ld_z, N, H, W, Cout, nullptr,
                           0, nullptr, stream, nullptr, &e, pool ? 1 : 0);
}
int mnk_conv3x3_up_fwd_evalnorm(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, const float* wp_up,
                                const float* bias, const float* mean, const float* scale, const float* beta, int relu, float* z,
                                int ld_z, int N, int H, int W, int Cout, void* stream) {
    MNK_REQUIRE(mean && scale && beta && z && (flags & ~MNK_CONV_BF16) == 0);
    const EvalNorm e = evalnorm_of(mean, scale, beta, relu);
    return conv2d_fwd_impl(x0, ld0, C0, x1, ld1, C1, MNK_CONV_CLEAN_PADS | flags, H, W, 2, 2, 1, 1, 4, wp_up, bias, nullptr, 0, z, ld_z,
                           N, H, W, Cout, nullptr, 0, nullptr, stream, nullptr, &e, 0);
}
}

#ifdef MNK_PHASE_CLOCKS
extern "C" int mnk_phase_sclk_read(void* host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(mnk_phase_sclk), bytes) == hipSuccess ? MNK_OK : MNK_ELAUNCH;
}
extern "C" int mnk_phase_log_read(void* host, size_t bytes, int clear) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(mnk_phase_log), bytes) != hipSuccess) return MNK_ELAUNCH;
    if (clear) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(mnk_phase_log)) != hipSuccess) return MNK_ELAUNCH;
        if (hipMemset(p, 0, sizeof(unsigned long long) * 4 * 16384) != hipSuccess) return MNK_ELAUNCH;
    }
    return MNK_OK;
}
#endif
