// The prediction task around its GRU (prediction.py:28-32,94-133): the key-point data path and the loss of the training loop,
// and the end of the roll-out, on the device.  The GRU itself is gru.hip.
//
// A key-point ROW is what modules/prediction_module.py:28-33 feeds the GRU for one frame: I = K * 2 floats, all means [K][2], or
// with 'var' I = K * 6: all means, then all covariances [K][2][2].  The linear layer's output row y is interleaved per key point,
// [K][F] with F = 2 or 6 (m0 m1 v00 v01 v10 v11): the head kernels below read y in that order and the ground truth in row order.
//
// Kernels (one C-ABI entry point each, include/monkeynet_hip.h):
//   kp_window_gather     x, gt [B][T][I] from a pool of rows and B window starts held on the device: one launch for
//                        KPDataset.__getitem__, the collation, .cuda(), the clones and the masking
//   gru_head_l1_fwd      loss = mean |gt_mean - tanh(y_mean)| (+ mean |gt_var - V^T V|) over the frames >= init_frames, the
//                        predicted key points never written.  TWO launches: per-block partial sums (mean and covariance terms
//                        apart: each has its own element count), then one block that adds the partials in index order, divides
//                        and -- one thread -- adds the loss to the epoch's running sum.  (One launch would need either a single
//                        block over the whole batch, 476 160 elements at B 256 x T 32 x K 10, or a "last block finishes" ticket;
//                        a second launch on the same stream costs about 1.5 us.)
//   gru_head_l1_bwd      dy for an upstream gradient of 1: -sign(gt - p) / count through the head's adjoint (gru_head.h, shared
//                        with gru_head_bwd_kernel); rows of the initial frames are zeros
//   kp_rollout_finish    prediction.py:127-131: the initial frames written back, the covariance of frame init_frames - 1 copied to
//                        every frame
// No atomics: every sum has a fixed order, two runs are bit-identical.  No scratch memory, no grid-wide hand-off.
#include "mnk_common.h"
#include "gru_head.h"

using namespace mnk;

namespace {

constexpr int L1_MAX_BLOCKS = 1024;     // partial sums of the loss: at most this many blocks of 256 (row, key point) items a pass

int l1_blocks(long n) { return std::max(1, std::min(L1_MAX_BLOCKS, ceil_div(n, 256))); }

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }      // sign(0) = 0, as torch.abs'

// ---- window gather ------------------------------------------------------------------------------------------------------------
// one thread: V consecutive floats of one output row (V = 4: float4 when I, ld and the three bases allow it; else V = 1)
template <int V>
__global__ void __launch_bounds__(256) kp_window_gather_kernel(const float* __restrict__ pool, long rows, long ld,
                                                               const int64_t* __restrict__ starts, int B, int T, int init_frames,
                                                               int I, float* __restrict__ x, float* __restrict__ gt) {
    const int per_row = I / V;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * T * per_row) return;
    const long row = e / per_row;                       // b * T + t
    const int i = (int)(e - row * per_row) * V;
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const long r = (long)starts[b] + t;
    const bool ok = r >= 0 && r < rows;                 // a window past the pool reads nothing and shows as NaN
    const long o = row * I + i;
    if (V == 4) {
        const float nan = __builtin_nanf("");
        float4 v = make_float4(nan, nan, nan, nan);
        if (ok) v = *reinterpret_cast<const float4*>(pool + r * ld + i);
        *reinterpret_cast<float4*>(gt + o) = v;
        *reinterpret_cast<float4*>(x + o) = t < init_frames ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const float v = ok ? pool[r * ld + i] : __builtin_nanf("");
        gt[o] = v;
        x[o] = t < init_frames ? v : 0.f;
    }
}

// ---- L1 loss fused with the head ------------------------------------------------------------------------------------------------
// item e = (row, key point); block `blk` takes items blk * 256 + thread + pass * (gridDim.x * 256): part[2 blk] = its sum of
// |gt_mean - tanh(y_mean)|, part[2 blk + 1] = its sum of |gt_var - V^T V|
__global__ void __launch_bounds__(256) gru_head_l1_part_kernel(const float* __restrict__ y, const float* __restrict__ gt, long n, int T,
                                                               int K, int F, int has_var, int init_frames,
                                                               float* __restrict__ part) {
    __shared__ float red[4];
    const int I = K * F;
    float sm = 0.f, sv = 0.f;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long row = e / K;
        const int k = (int)(e - row * K);
        if ((int)(row % T) < init_frames) continue;
        const float* v = y + e * F;
        const float* g = gt + row * I;
        float m0, m1;
        head_mean(v, m0, m1);
        sm += fabsf(g[2 * k] - m0) + fabsf(g[2 * k + 1] - m1);
        if (has_var) {
            float p[4];
            head_var(v, p);
            const float* gv = g + 2 * K + 4 * k;
            sv += (fabsf(gv[0] - p[0]) + fabsf(gv[1] - p[1])) + (fabsf(gv[2] - p[2]) + fabsf(gv[3] - p[3]));
        }
    }
    sm = block_sum_256(sm, red);
    sv = block_sum_256(sv, red);
    if (threadIdx.x == 0) part[2 * blockIdx.x] = sm, part[2 * blockIdx.x + 1] = sv;
}

// one block: the partials in index order (thread t: t, t + 256, ...; then the block's fixed tree), the two means, their sum;
// thread 0 alone touches the epoch's accumulator -- launches of one stream run in order, so the epoch sum has iteration order
__global__ void __launch_bounds__(256) gru_head_l1_finish_kernel(const float* __restrict__ part, int nb, float cnt_mean, float cnt_var,
                                                                 float* __restrict__ loss, float* __restrict__ epoch_acc,
                                                                 float* __restrict__ loss_log, int log_cap) {
    __shared__ float red[4];
    float sm = 0.f, sv = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) sm += part[2 * i], sv += part[2 * i + 1];
    sm = block_sum_256(sm, red);
    sv = block_sum_256(sv, red);
    if (threadIdx.x != 0) return;
    float l = sm / cnt_mean;
    if (cnt_var > 0.f) l += sv / cnt_var;
    loss[0] = l;
    if (epoch_acc) {
        const int it = (int)epoch_acc[1];
        if (loss_log && it < log_cap) loss_log[it] = l;
        epoch_acc[0] += l;
        epoch_acc[1] = (float)(it + 1);
    }
}

__global__ void __launch_bounds__(256) gru_head_l1_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gt, long n, int T,
                                                              int K, int F, int has_var, int init_frames, float inv_mean,
                                                              float inv_var, float* __restrict__ dy) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;        // (row, key point)
    if (e >= n) return;
    const long row = e / K;
    const int k = (int)(e - row * K);
    const float* v = y + e * F;
    float* o = dy + e * F;
    if ((int)(row % T) < init_frames) {
        for (int f = 0; f < F; ++f) o[f] = 0.f;
        return;
    }
    const float* g = gt + row * (long)(K * F);
    float m0, m1;
    head_mean(v, m0, m1);
    // d|gt - p| / dp = -sign(gt - p); the mean's 1 / count
    head_mean_bwd(-sign_of(g[2 * k] - m0) * inv_mean, -sign_of(g[2 * k + 1] - m1) * inv_mean, m0, m1, o);
    if (has_var) {
        float p[4], gr[4];
        head_var(v, p);
        const float* gv = g + 2 * K + 4 * k;
        for (int q = 0; q < 4; ++q) gr[q] = -sign_of(gv[q] - p[q]) * inv_var;
        head_var_bwd(v, gr, o);
    }
}

// ---- the end of the roll-out ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) kp_rollout_finish_kernel(const float* __restrict__ kp_init, long ld, long n, int T, int K,
                                                                int has_var, int init_frames, int copy_var, float* __restrict__ mean,
                                                                float* __restrict__ var) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;        // (b, t, key point)
    if (e >= n) return;
    const long row = e / K;
    const int k = (int)(e - row * K);
    const int t = (int)(row % T);
    const float* src = kp_init + row * ld;
    if (t < init_frames) {
        mean[2 * e] = src[2 * k];
        mean[2 * e + 1] = src[2 * k + 1];
    }
    if (!has_var) return;
    if (copy_var) src = kp_init + (row - t + (init_frames - 1)) * ld;      // frame init_frames - 1 of the same video
    else if (t >= init_frames) return;
    const float* sv = src + 2 * K + 4 * k;
    float* o = var + 4 * e;
    o[0] = sv[0], o[1] = sv[1], o[2] = sv[2], o[3] = sv[3];
}

bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" {

int mnk_kp_window_gather(const float* pool, long rows, long ld, const int64_t* starts, int B, int T, int init_frames, int I, float* x,
                         float* gt, void* stream) {
    MNK_REQUIRE(rows >= 0 && B >= 0 && T >= 0 && I >= 0 && ld >= I && init_frames >= 0);
    const long n = (long)B * T * I;
    if (n == 0) return MNK_OK;
    MNK_REQUIRE(pool && starts && x && gt);
    hipStream_t s = (hipStream_t)stream;
    if (I % 4 == 0 && ld % 4 == 0 && aligned16(pool) && aligned16(x) && aligned16(gt))
        hipLaunchKernelGGL(kp_window_gather_kernel<4>, dim3(ceil_div(n / 4, 256)), dim3(256), 0, s, pool, rows, ld, starts, B, T,
                           init_frames, I, x, gt);
    else
        hipLaunchKernelGGL(kp_window_gather_kernel<1>, dim3(ceil_div(n, 256)), dim3(256), 0, s, pool, rows, ld, starts, B, T,
                           init_frames, I, x, gt);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

size_t mnk_gru_head_l1_workspace_floats(int B, int T, int K) {
    if (B <= 0 || T <= 0 || K <= 0) return 0;
    return 2 * (size_t)l1_blocks((long)B * T * K);
}

int mnk_gru_head_l1_fwd(const float* y, const float* gt, int B, int T, int K, int feats, int has_var, int init_frames, float* loss,
                        float* epoch_acc, float* loss_log, int log_cap, float* ws, size_t ws_floats, void* stream) {
    MNK_REQUIRE(B > 0 && K > 0 && feats == (has_var ? 6 : 2) && init_frames >= 0 && T > init_frames && log_cap >= 0);
    const long n = (long)B * T * K;
    const int nb = l1_blocks(n);
    MNK_REQUIRE(y && gt && loss && ws && ws_floats >= 2 * (size_t)nb);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gru_head_l1_part_kernel, dim3(nb), dim3(256), 0, s, y, gt, n, T, K, feats, has_var, init_frames, ws);
    MNK_LAUNCH_CHECK();
    const double frames = (double)B * (T - init_frames) * K;
    hipLaunchKernelGGL(gru_head_l1_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, nb, (float)(2.0 * frames),
                       has_var ? (float)(4.0 * frames) : 0.f, loss, epoch_acc, loss_log, log_cap);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_head_l1_bwd(const float* y, const float* gt, int B, int T, int K, int feats, int has_var, int init_frames, float* dy,
                        void* stream) {
    MNK_REQUIRE(B > 0 && K > 0 && feats == (has_var ? 6 : 2) && init_frames >= 0 && T > init_frames);
    MNK_REQUIRE(y && gt && dy);
    const long n = (long)B * T * K;
    const double frames = (double)B * (T - init_frames) * K;
    hipLaunchKernelGGL(gru_head_l1_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, y, gt, n, T, K, feats, has_var,
                       init_frames, 1.f / (float)(2.0 * frames), has_var ? 1.f / (float)(4.0 * frames) : 0.f, dy);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_kp_rollout_finish(const float* kp_init, long ld, int B, int T, int K, int has_var, int init_frames, int predict_variance,
                          float* mean, float* var, void* stream) {
    MNK_REQUIRE(B >= 0 && T >= 0 && K >= 0 && init_frames >= 0 && init_frames <= T && ld >= (long)K * (has_var ? 6 : 2));
    const long n = (long)B * T * K;
    if (n == 0) return MNK_OK;
    MNK_REQUIRE(kp_init && mean && (!has_var || var));
    const int copy_var = has_var && predict_variance;
    MNK_REQUIRE(!copy_var || init_frames >= 1);
    hipLaunchKernelGGL(kp_rollout_finish_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, kp_init, ld, n, T, K, has_var,
                       init_frames, copy_var, mean, var);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

}  // extern "C"
