// Weight-streaming ("skinny") 3x3 convolutions for batch-1 evaluation (modules/util.py:79-88,98-108 of the reference, called one
// frame at a time by reconstruction.py:57-62 / transfer.py:65-79): a convolution whose output has at most 64 rows (N * H * W) is
// a GEMV with a few columns -- all of its time is the weight stream.  The implicit-GEMM kernels of conv3x3.hip work on 64-row
// tiles and LDS-staged weights; this form reads every weight ONCE per block, straight into registers with 16-byte loads (several
// in flight per lane, no LDS round trip), keeps the block's tiny slice of the activations in LDS, and multiplies with plain fmaf
// in a fixed order.  The grid is (32-channel tiles of Cout) x (K splits) [x 16-row groups] so that every CU streams; a block
// writes its partial tile to the workspace [split][row][round_up(Cout, 4)] and mnk_bn_eval_split_fwd sums the splits in order
// (+ bias, norm affine, ReLU, pool).  No atomics, no flags, no block waits for another.
//
// K axis: k = tap * (C0 + C1) + ci (tap-major: neighbouring k are neighbouring channels of one pixel, so the gather is
// coalesced), padded with zero weights to a multiple of 64.  Pack: [cout tile][k pair][channel quad (8)][k parity (2)][4] --
// a block's stream over its K range is one contiguous run, whatever the split count; a thread's 32 bytes (fp32) or 16 bytes
// (bf16) hold the two k of a pair for its four output channels.  Both element types give every thread the same k in the same
// order: the bf16 pack computes bit for bit what the fp32 pack of pre-rounded weights does.
// Up-sampled form (MNK_CONV_UPSAMPLED): the plain nine taps on sources read at (y >> 1, x >> 1) -- 9/16 of the weight bytes of
// the sub-pixel packs, which is what counts here.
#include "conv_common.h"

using namespace mnk;

namespace {

constexpr int SK_CT = 32;                    // output channels of a block
constexpr int SK_NQ = SK_CT / 4;             // channel quads of a block: a thread owns one ...
constexpr int SK_NKS = 256 / SK_NQ;          // ... in one of these thread groups, which share the k of a load round
constexpr int SK_KR = 2 * SK_NKS;            // k values of one load round: a pair per thread group
constexpr int SK_ROUNDS = 4;                 // load rounds of a staged chunk
constexpr int SK_KB = SK_KR * SK_ROUNDS;     // k values of a staged chunk: one per thread of the gather
static_assert(SK_KB == 256, "the gather maps one k of a chunk to each of the 256 threads");
constexpr int SK_MAX_ROWS = 64;

struct SkinnyArgs {
    const float *x0, *x1;
    const void* wp;
    float* ws;
    int ld0, ld1, C0, C1;
    int H, W, Hs, Ws, ups;        // (H, W): the output; (Hs, Ws): the sources
    int R, Cout, ldw, K, Kp, k_per_split;
};

__device__ __forceinline__ float bf16_round1(float v) {
    return __uint_as_float((mnk_round_bf16x4(make_float4(v, 0.f, 0.f, 0.f)).x & 0xffffu) << 16);
}

// RT: rows of a block (4: one group of <= 4 rows; 16: blockIdx.z walks groups of 16)
template <int RT, bool BF16>
__global__ void __launch_bounds__(256) conv_skinny_kernel(SkinnyArgs a) {
    __shared__ float lds[SK_KB * RT + 4 * RT * SK_CT];
    float* xs = lds;                         // [k of the chunk][RT]
    float* red = lds + SK_KB * RT;           // [wave][RT][SK_CT]
    const int t = threadIdx.x, cq = t & (SK_NQ - 1), ks = t / SK_NQ;
    const int ct = blockIdx.x, split = blockIdx.y, row0 = blockIdx.z * RT;
    const int k_begin = split * a.k_per_split;
    const int k_end = k_begin + a.k_per_split < a.Kp ? k_begin + a.k_per_split : a.Kp;
    const int Cin = a.C0 + a.C1, HW = a.H * a.W;
    // the gather: thread -> one k of the chunk, every row
    constexpr int RH = RT;
    const int gk = t, gr0 = 0;

    float acc[RT][4];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;

    const size_t pair0 = (size_t)ct * (a.Kp / 2);
    for (int kb = k_begin; kb < k_end; kb += SK_KB) {
        const int nr = (k_end - kb) / SK_KR < SK_ROUNDS ? (k_end - kb) / SK_KR : SK_ROUNDS;
        // 1. the activations of this chunk: every load is issued (masked ones at a clamped address), then selected
        float xv[RH];
        {
            const int k = kb + gk;
            const bool kok = k < a.K;
            const int tap = kok ? k / Cin : 0, ci = kok ? k - tap * Cin : 0;
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            const bool s1 = ci >= a.C0;
            const float* src = s1 ? a.x1 : a.x0;
            const int ld = s1 ? a.ld1 : a.ld0, c = s1 ? ci - a.C0 : ci;
            bool ok[RH];
            const float* p[RH];
#pragma unroll
            for (int i = 0; i < RH; ++i) {
                const int row = row0 + gr0 + i;
                const int n = row / HW, rem = row - n * HW, Y = rem / a.W, X = rem - Y * a.W;
                const int yy = Y + dy, xx = X + dx;
                ok[i] = kok && row < a.R && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
                const int ysrc = a.ups ? yy >> 1 : yy, xsrc = a.ups ? xx >> 1 : xx;
                p[i] = ok[i] ? src + ((long)(n * a.Hs + ysrc) * a.Ws + xsrc) * ld + c : a.x0;
            }
#pragma unroll
            for (int i = 0; i < RH; ++i) xv[i] = *p[i];
#pragma unroll
            for (int i = 0; i < RH; ++i) {
                xv[i] = ok[i] ? xv[i] : 0.f;
                if constexpr (BF16) xv[i] = bf16_round1(xv[i]);
            }
        }
        // 2. the weights of this chunk, straight into registers (rounds past the end of the K range re-read round 0: no branch
        //    around a load)
        float4 wf[SK_ROUNDS][2];
        uint4 wh[SK_ROUNDS];
#pragma unroll
        for (int j = 0; j < SK_ROUNDS; ++j) {
            const size_t pair = pair0 + (size_t)((kb + (j < nr ? j : 0) * SK_KR) / 2 + ks);
            if constexpr (BF16) {
                wh[j] = reinterpret_cast<const uint4*>(a.wp)[pair * SK_NQ + cq];
            } else {
                const float4* q = reinterpret_cast<const float4*>(a.wp) + (pair * SK_NQ + cq) * 2;
                wf[j][0] = q[0];
                wf[j][1] = q[1];
            }
        }
        // 3. activations -> LDS
#pragma unroll
        for (int i = 0; i < RH; ++i) xs[gk * RT + gr0 + i] = xv[i];
        __syncthreads();
        // 4. products, in the order of k
#pragma unroll
        for (int j = 0; j < SK_ROUNDS; ++j) {
            if (j < nr) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    float4 w;
                    if constexpr (BF16) {
                        const unsigned lo = e ? wh[j].z : wh[j].x, hi = e ? wh[j].w : wh[j].y;
                        w = make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                                        __uint_as_float(hi & 0xffff0000u));
                    } else {
                        w = wf[j][e];
                    }
                    const float* xr = xs + (j * SK_KR + ks * 2 + e) * RT;
#pragma unroll
                    for (int r4 = 0; r4 < RT; r4 += 4) {
                        const float4 xq = *reinterpret_cast<const float4*>(xr + r4);
                        const float xa[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[r4 + i][0] = fmaf(xa[i], w.x, acc[r4 + i][0]);
                            acc[r4 + i][1] = fmaf(xa[i], w.y, acc[r4 + i][1]);
                            acc[r4 + i][2] = fmaf(xa[i], w.z, acc[r4 + i][2]);
                            acc[r4 + i][3] = fmaf(xa[i], w.w, acc[r4 + i][3]);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

    // the thread groups of a channel quad: those inside each wave (lanes l ^ SK_NQ, l ^ 2 SK_NQ, ...), then the four waves in order
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = acc[r][c];
#pragma unroll
            for (int o = SK_NQ; o < 64; o <<= 1) v += __shfl_xor(v, o);
            acc[r][c] = v;
        }
    if ((t & 63) < SK_NQ) {
        const int wave = t >> 6;
#pragma unroll
        for (int r = 0; r < RT; ++r)
            *reinterpret_cast<float4*>(red + (wave * RT + r) * SK_CT + cq * 4) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
    __syncthreads();
    if (t < RT * SK_NQ) {
        const int r = t / SK_NQ, row = row0 + r, col = ct * SK_CT + cq * 4;
        if (row < a.R && col < a.ldw) {
            float4 s = *reinterpret_cast<const float4*>(red + r * SK_CT + cq * 4);
#pragma unroll
            for (int wv = 1; wv < 4; ++wv) {
                const float4 o = *reinterpret_cast<const float4*>(red + (wv * RT + r) * SK_CT + cq * 4);
                s.x += o.x, s.y += o.y, s.z += o.z, s.w += o.w;
            }
            *reinterpret_cast<float4*>(a.ws + ((size_t)split * a.R + row) * a.ldw + col) = s;
        }
    }
}

// w (Cout, Cin, 1, 3, 3) -> the pack above; one thread per element, zeros where k >= 9 Cin or the channel >= Cout
__global__ void __launch_bounds__(256) conv_skinny_pack_kernel(const float* __restrict__ w, void* wp, int Cout, int Cin, int Kp,
                                                               long total, int bf16) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i & 3), e = (int)((i >> 2) & 1), q = (int)((i >> 3) & (SK_NQ - 1));
        const long pr = i / (8 * SK_NQ);
        const int pair = (int)(pr % (Kp / 2)), ct = (int)(pr / (Kp / 2));
        const int k = pair * 2 + e, co = ct * SK_CT + q * 4 + c4;
        float v = 0.f;
        if (k < 9 * Cin && co < Cout) {
            const int tap = k / Cin, ci = k - tap * Cin;
            v = w[((long)co * Cin + ci) * 9 + tap];
        }
        if (bf16)
            reinterpret_cast<unsigned short*>(wp)[i] = (unsigned short)(mnk_round_bf16x4(make_float4(v, 0.f, 0.f, 0.f)).x & 0xffffu);
        else
            reinterpret_cast<float*>(wp)[i] = v;
    }
}

// rows up to which the form is taken (0: never).  Default from profiles/eval_skinny.txt
int g_skinny_rows = tuning_knob("skinny_rows", &g_skinny_rows, 16);
// blocks a launch aims at: one per CU of the MI355X's 256.  More blocks stream faster but mean more splits, and the second stage
// (mnk_bn_eval_split_fwd) walks the splits of an output one after another: measured, 256 beats 128, 512 and 1024
// (profiles/eval_skinny.txt)
int g_skinny_blocks = tuning_knob("skinny_blocks", &g_skinny_blocks, 256);
// up-sampled layers with fewer weights (9 Cin Cout) keep today's sub-pixel launch, except bf16 launches of at most 4 rows
int g_skinny_up_min_weights = tuning_knob("skinny_up_min_weights", &g_skinny_up_min_weights, 8 << 20);
// the shortest K range of a split the rule makes (k values; a multiple of 64)
int g_skinny_min_k = tuning_knob("skinny_min_k", &g_skinny_min_k, 256);

struct SkinnyPlan {
    int R, rt, row_groups, ctiles, K, Kp, slots, slots_per_split, splits, ldw;
};

inline int skinny_kp(int C0, int C1) { return round_up(9 * (C0 + C1), SK_KR); }

bool skinny_takes(int N, int H, int W, int C0, int C1, int Cout, int flags, int pool) {
    if (N <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0) return false;
    if (flags & ~(MNK_CONV_UPSAMPLED | MNK_CONV_CLEAN_PADS | MNK_CONV_DEFER_SPLITK | MNK_CONV_BF16)) return false;
    const int limit = g_skinny_rows < SK_MAX_ROWS ? g_skinny_rows : SK_MAX_ROWS;
    if ((long)N * H * W > limit) return false;
    if ((flags & MNK_CONV_UPSAMPLED) && (H % 2 || W % 2)) return false;
    if (pool && (H % 2 || W % 2)) return false;
    // measured (profiles/eval_skinny.txt): against the sub-pixel form, which skips the dead pseudo taps of a 1 x 1 source and runs
    // 16 splits, an up-sampled layer only gains where the weight stream is long -- or where MNK_CONV_BF16 halves it and the
    // second stage walks few rows
    if ((flags & MNK_CONV_UPSAMPLED) && 9L * (C0 + C1) * Cout < g_skinny_up_min_weights &&
        !((flags & MNK_CONV_BF16) && (long)N * H * W <= 4))
        return false;
    return true;
}

SkinnyPlan skinny_plan(int N, int H, int W, int C0, int C1, int Cout) {
    SkinnyPlan p;
    p.R = N * H * W;
    p.rt = p.R <= 4 ? 4 : 16;
    p.row_groups = ceil_div(p.R, p.rt);
    p.ctiles = ceil_div(Cout, SK_CT);
    p.K = 9 * (C0 + C1);
    p.Kp = skinny_kp(C0, C1);
    p.slots = p.Kp / SK_KR;
    // the rule: enough splits for skinny_blocks blocks, none shorter than skinny_min_k
    int splits = ceil_div(g_skinny_blocks, (long)p.ctiles * p.row_groups);
    const int min_slots = g_skinny_min_k / SK_KR > 1 ? g_skinny_min_k / SK_KR : 1;
    if (splits > p.slots / min_slots) splits = p.slots / min_slots;
    if (g_force_splits > 0) splits = g_force_splits;
    if (splits > p.slots) splits = p.slots;
    if (splits < 1) splits = 1;
    p.slots_per_split = ceil_div(p.slots, splits);
    p.splits = ceil_div(p.slots, p.slots_per_split);
    p.ldw = round_up(Cout, 4);
    return p;
}

}  // namespace

extern "C" {

size_t mnk_conv3x3_skinny_packed_floats(int Cout, int C0, int C1, int bf16) {
    if (Cout <= 0 || C0 <= 0 || C1 < 0) return 0;
    const size_t n = (size_t)ceil_div(Cout, SK_CT) * skinny_kp(C0, C1) * SK_CT;
    return bf16 ? n / 2 : n;
}

int mnk_conv3x3_skinny_pack(const float* w, float* wp, int Cout, int C0, int C1, int bf16, void* stream) {
    MNK_REQUIRE(w && wp && Cout > 0 && C0 > 0 && C1 >= 0 && (bf16 == 0 || bf16 == 1) && (size_t)wp % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int Kp = skinny_kp(C0, C1);
    const long total = (long)ceil_div(Cout, SK_CT) * Kp * SK_CT;
    ProfScope prof(K_CONV_REDUCE, s, (double)total * (bf16 ? 2 : 4) + (double)Cout * (C0 + C1) * 9 * 4);
    hipLaunchKernelGGL(conv_skinny_pack_kernel, dim3(grid_for(total)), dim3(256), 0, s, w, (void*)wp, Cout, C0 + C1, Kp, total, bf16);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_conv3x3_skinny_form(int N, int H, int W, int C0, int C1, int Cout, int flags, int pool) {
    return skinny_takes(N, H, W, C0, C1, Cout, flags, pool) ? 1 : 0;
}

int mnk_conv3x3_skinny_splits(int N, int H, int W, int C0, int C1, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0 || (long)N * H * W > SK_MAX_ROWS) return 0;
    return skinny_plan(N, H, W, C0, C1, Cout).splits;
}

size_t mnk_conv3x3_skinny_workspace_floats(int N, int H, int W, int C0, int C1, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0 || (long)N * H * W > SK_MAX_ROWS) return 0;
    const SkinnyPlan p = skinny_plan(N, H, W, C0, C1, Cout);
    return (size_t)p.splits * p.R * p.ldw;
}

int mnk_conv3x3_skinny_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, int flags, const float* wp, int N,
                           int H, int W, int Cout, float* ws, size_t ws_floats, void* stream) {
    MNK_REQUIRE(x0 && wp && ws && (C1 == 0 || x1) && ld0 >= C0 && (C1 == 0 || ld1 >= C1) && (size_t)wp % 16 == 0 && (size_t)ws % 16 == 0);
    if (!skinny_takes(N, H, W, C0, C1, Cout, flags, 0)) {
        set_error("%s: invalid argument: this launch does not take the weight-streaming form (mnk_conv3x3_skinny_form answers 0: "
                  "%ld rows, skinny_rows %d, flags %d)", __func__, (long)N * H * W, g_skinny_rows, flags);
        return MNK_EINVAL;
    }
    const SkinnyPlan p = skinny_plan(N, H, W, C0, C1, Cout);
    if (ws_floats < (size_t)p.splits * p.R * p.ldw) {
        set_error("%s: workspace too small", __func__);
        return MNK_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    SkinnyArgs a;
    a.x0 = x0, a.x1 = C1 ? x1 : x0, a.wp = wp, a.ws = ws;
    a.ld0 = ld0, a.ld1 = C1 ? ld1 : ld0, a.C0 = C0, a.C1 = C1;
    a.ups = flags & MNK_CONV_UPSAMPLED ? 1 : 0;
    a.H = H, a.W = W, a.Hs = a.ups ? H / 2 : H, a.Ws = a.ups ? W / 2 : W;
    a.R = p.R, a.Cout = Cout, a.ldw = p.ldw, a.K = p.K, a.Kp = p.Kp, a.k_per_split = p.slots_per_split * SK_KR;
    g_last_plan[0] = p.R, g_last_plan[1] = Cout, g_last_plan[2] = p.slots, g_last_plan[3] = 9, g_last_plan[4] = 1;
    g_last_plan[5] = p.rt, g_last_plan[6] = SK_CT, g_last_plan[7] = p.splits;
    const bool bf16 = (flags & MNK_CONV_BF16) != 0;
    ProfScope prof(K_CONV_FWD, s, 2.0 * p.R * Cout * p.K);
    const dim3 grid(p.ctiles, p.splits, p.row_groups);
    if (p.rt == 4) {
        if (bf16)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_skinny_kernel<4, true>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_skinny_kernel<4, false>), grid, dim3(256), 0, s, a);
    } else {
        if (bf16)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_skinny_kernel<16, true>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_skinny_kernel<16, false>), grid, dim3(256), 0, s, a);
    }
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

}  // extern "C"
