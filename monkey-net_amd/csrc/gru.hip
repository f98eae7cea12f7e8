// GRU key-point predictor of the prediction task (modules/prediction_module.py: nn.GRU(batch_first=True) + nn.Linear,
// trained and rolled out by prediction.py:97-132), forward and backward, PyTorch GRU semantics with gate order (r, z, n):
//   r = sigma(Gi_r + h W_hr^T + b_hr),  z = sigma(Gi_z + h W_hz^T + b_hz),  hn = h W_hn^T + b_hn
//   n = tanh(Gi_n + r * hn),            h' = (1 - z) * n + z * h               with Gi = x W_ih^T + b_ih
//
// Kernels (one C-ABI entry point each, include/monkeynet_hip.h):
//   gru_gemm          C = op(A) op(B) (+ bias) on v_mfma_f32_32x32x2_f32: the input projection of all steps at once, the output
//                     head's linear layer and every weight / data gradient GEMM of the backward pass; split-K partials are
//                     summed in a fixed order (deterministic)
//   gru_step_fwd      one time step: h_{t-1} W_hh^T for a 32-row x 32-unit tile of all three gates (unpacked [3H, H] weight, row
//                     blocks j, H + j, 2H + j) with the gate epilogue fused; saves r, z, n, hn for backward.  Small batches
//                     (prediction.py's batch-1 roll-out) take a GEMV form: one wave per hidden unit, all batch rows at once
//   gru_step_bwd      dh_{t-1} = dGh_t W_hh + dh_t * z_t (+ the output's gradient at t - 1), with the gate backward of step t - 1
//                     fused into its epilogue
//   gru_gates_bwd     the gate backward of the last step (the loop's first)
//   gru_head_fwd/bwd  mean = tanh(Y[..., :2]), var = V^T V (V = Y[..., 2:6] as 2x2; prediction_module.py:33-42) and their adjoint
//   gru_colsum        bias gradients: column sums in a fixed order (two stages)
// No floating-point atomics, no persistent kernel, no grid-wide barrier.
#include "mnk_common.h"
#include "gru_head.h"

using namespace mnk;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// batch rows up to which a forward step takes the GEMV form (at most GEMV_MAX_B)
constexpr int GEMV_MAX_B = 8;
static int g_gru_gemv_rows = tuning_knob("gru_gemv_rows", &g_gru_gemv_rows, 4);

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// row r of a grouped-row matrix: (r / grp) * ld_grp + (r % grp) * ld   (grp <= 0 never reaches a kernel: the host makes it M or K)
__device__ __forceinline__ long row_off(unsigned r, unsigned grp, long ld, long ld_grp) {
    const unsigned q = r / grp;
    return (long)q * ld_grp + (long)(r - q * grp) * ld;
}

// ---- generic GEMM ------------------------------------------------------------------------------------------------------------
constexpr int GB_M = 64, GB_N = 64, GB_K = 16, G_LDS = 96;     // row pitch 96: the two lane halves of an MFMA read hit disjoint banks

struct Opnd {
    const float* p;
    long ld, ld_grp;
    unsigned grp;
};

// element (i, k) of an operand (i: m for A, n for B); KMAJOR: stored [K][i], else stored [i][K]
template <bool KMAJOR>
__device__ __forceinline__ float ld_op(const Opnd& o, int i, int k, int nI, int K) {
    if (i >= nI || k >= K) return 0.f;
    return KMAJOR ? o.p[row_off((unsigned)k, o.grp, o.ld, o.ld_grp) + i] : o.p[row_off((unsigned)i, o.grp, o.ld, o.ld_grp) + k];
}

// thread t's four elements of a 64 x 16 tile: stored [i][k] (k contiguous): i = t / 16 + 16 q, k = t % 16; stored [k][i]:
// k = t / 64 + 4 q, i = t % 64 -- coalesced along the stored row either way
template <bool KMAJOR>
__device__ __forceinline__ void tile_pos(int t, int q, int& i, int& k) {
    if (KMAJOR) k = (t >> 6) + 4 * q, i = t & 63;
    else i = (t >> 4) + 16 * q, k = t & 15;
}

// A "K-major" operand is stored with k as its row index: A with transA, B without transB
template <bool A_KMAJOR, bool B_KMAJOR>
__global__ void __launch_bounds__(256) gru_gemm_kernel(Opnd A, Opnd B, const float* __restrict__ bias, float* __restrict__ C,
                                                       long ldc, int M, int N, int K, int kchunk) {
    __shared__ float As[GB_K][G_LDS], Bs[GB_K][G_LDS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m0 = blockIdx.y * GB_M, n0 = blockIdx.x * GB_N;
    const int kb = blockIdx.z * kchunk, ke = K < kb + kchunk ? K : kb + kchunk;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int i, k;
            tile_pos<A_KMAJOR>(t, q, i, k);
            ra[q] = k0 + k < ke ? ld_op<A_KMAJOR>(A, m0 + i, k0 + k, M, K) : 0.f;
            tile_pos<B_KMAJOR>(t, q, i, k);
            rb[q] = k0 + k < ke ? ld_op<B_KMAJOR>(B, n0 + i, k0 + k, N, K) : 0.f;
        }
    };
    if (kb < ke) load(kb);
    for (int k0 = kb; k0 < ke; k0 += GB_K) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int i, k;
            tile_pos<A_KMAJOR>(t, q, i, k);
            As[k][i] = ra[q];
            tile_pos<B_KMAJOR>(t, q, i, k);
            Bs[k][i] = rb[q];
        }
        __syncthreads();
        if (k0 + GB_K < ke) load(k0 + GB_K);
#pragma unroll
        for (int s = 0; s < GB_K; s += 2) {
            const float a = As[s + (lane >> 5)][wm + (lane & 31)];
            const float b = Bs[s + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    // split z > 0 (or any split of a multi-split launch) writes its partial plane; the reduce kernel adds the bias
    float* out = C + (long)blockIdx.z * (gridDim.z > 1 ? (long)M * N : 0);
    const long ldo = gridDim.z > 1 ? N : ldc;
    const int n = n0 + wn + (lane & 31);
    if (n >= N) return;
    const float bv = (bias && gridDim.z == 1) ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M) out[(long)m * ldo + n] = acc[r] + bv;
    }
}

__global__ void __launch_bounds__(256) gru_splitk_reduce_kernel(const float* __restrict__ ws, int splits, const float* __restrict__ bias,
                                                                float* __restrict__ C, long ldc, int M, int N) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)M * N) return;
    const int m = (int)(i / N), n = (int)(i - (long)m * N);
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += ws[(long)s * M * N + i];
    C[(long)m * ldc + n] = v + (bias ? bias[n] : 0.f);
}

int gemm_splits(int M, int N, int K) {
    const long tiles = (long)ceil_div(M, GB_M) * ceil_div(N, GB_N);
    if (tiles >= 128 || K < 1024) return 1;
    int s = (int)((256 + tiles - 1) / tiles);
    s = std::min(s, K / 512);
    s = std::min(s, 16);
    return std::max(s, 1);
}

// ---- recurrent step, forward -------------------------------------------------------------------------------------------------
// four consecutive floats of row `row` at column k (zero past `n` or for a row outside the matrix)
__device__ __forceinline__ float4 ld4(const float* row, int k, int n, bool ok, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok || k >= n) return v;
    if (vec) return *reinterpret_cast<const float4*>(row + k);
    v.x = row[k];
    if (k + 1 < n) v.y = row[k + 1];
    if (k + 2 < n) v.z = row[k + 2];
    if (k + 3 < n) v.w = row[k + 3];
    return v;
}

__device__ __forceinline__ void gate_fwd(int b, int j, int H, float hr, float hz, float hn, const float* __restrict__ gi, long ld_gi,
                                         const float* __restrict__ b_hh, const float* __restrict__ h_prev, long ld_hp,
                                         float* __restrict__ h, long ld_h, float* __restrict__ gates) {
    hr += b_hh[j], hz += b_hh[H + j], hn += b_hh[2 * H + j];
    const float* g = gi + (long)b * ld_gi;
    const float r = sigmoidf_(g[j] + hr);
    const float z = sigmoidf_(g[H + j] + hz);
    const float n = tanhf(g[2 * H + j] + r * hn);
    h[(long)b * ld_h + j] = (1.f - z) * n + z * h_prev[(long)b * ld_hp + j];
    if (gates) {
        float* s = gates + (long)b * 4 * H;
        s[j] = r, s[H + j] = z, s[2 * H + j] = n, s[3 * H + j] = hn;
    }
}

// one workgroup: batch rows b0..b0+31 x hidden units j0..j0+31 of all three gates; the four waves split K = H in 32-wide chunks
// (wave w takes chunks w, w + 4, ...) and meet in LDS, summed in wave order.  Lane half hh of a chunk covers k = 16 hh + 4 q + e:
// the MFMA's two k of one issue are k and k + 16, the same permutation on both operands.
__global__ void __launch_bounds__(256) gru_step_fwd_kernel(const float* __restrict__ h_prev, long ld_hp, const float* __restrict__ w_hh,
                                                           const float* __restrict__ b_hh, const float* __restrict__ gi, long ld_gi,
                                                           float* __restrict__ h, long ld_h, float* __restrict__ gates, int B, int H,
                                                           int vec) {
    __shared__ float red[4][3][32][33];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, hh = lane >> 5;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int i = lane & 31;
    const bool arow = b0 + i < B, brow = j0 + i < H;
    const float* ap = h_prev + (long)(arow ? b0 + i : 0) * ld_hp;
    const float* bp0 = w_hh + (long)(brow ? j0 + i : 0) * H;
    f32x16 acc[3];
    for (int g = 0; g < 3; ++g)
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    const int nchunks = (H + 31) / 32;
    for (int c = w; c < nchunks; c += 4) {
        float4 a[4], bq[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = c * 32 + 16 * hh + 4 * q;
            a[q] = ld4(ap, k, H, arow, vec);
#pragma unroll
            for (int g = 0; g < 3; ++g) bq[g][q] = ld4(bp0 + (long)g * H * H, k, H, brow, vec);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, bq[g][q].x, acc[g], 0, 0, 0);
                acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, bq[g][q].y, acc[g], 0, 0, 0);
                acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, bq[g][q].z, acc[g], 0, 0, 0);
                acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, bq[g][q].w, acc[g], 0, 0, 0);
            }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[w][g][(r & 3) + 8 * (r >> 2) + 4 * hh][i] = acc[g][r];
    __syncthreads();
    for (int e = t; e < 32 * 32; e += 256) {
        const int row = e >> 5, col = e & 31, b = b0 + row, j = j0 + col;
        if (b >= B || j >= H) continue;
        float s[3];
        for (int g = 0; g < 3; ++g) s[g] = ((red[0][g][row][col] + red[1][g][row][col]) + red[2][g][row][col]) + red[3][g][row][col];
        gate_fwd(b, j, H, s[0], s[1], s[2], gi, ld_gi, b_hh, h_prev, ld_hp, h, ld_h, gates);
    }
}

// GEMV form (B <= GEMV_MAX_B): wave w of a workgroup owns hidden unit j = 4 blockIdx.x + w and sums its three weight rows against
// every batch row in one pass over k
__global__ void __launch_bounds__(256) gru_step_fwd_gemv_kernel(const float* __restrict__ h_prev, long ld_hp, const float* __restrict__ w_hh,
                                                                const float* __restrict__ b_hh, const float* __restrict__ gi, long ld_gi,
                                                                float* __restrict__ h, long ld_h, float* __restrict__ gates, int B,
                                                                int H, int vec) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= H) return;
    float acc[GEMV_MAX_B][3];
#pragma unroll
    for (int b = 0; b < GEMV_MAX_B; ++b) acc[b][0] = acc[b][1] = acc[b][2] = 0.f;
    const float* wr = w_hh + (long)j * H;
    const long gs = (long)H * H;
    for (int k = 4 * lane; k < H; k += 256) {
        const float4 w0 = ld4(wr, k, H, true, vec), w1 = ld4(wr + gs, k, H, true, vec), w2 = ld4(wr + 2 * gs, k, H, true, vec);
#pragma unroll
        for (int b = 0; b < GEMV_MAX_B; ++b) {
            if (b >= B) break;
            const float4 x = ld4(h_prev + (long)b * ld_hp, k, H, true, vec);
            acc[b][0] += x.x * w0.x + x.y * w0.y + x.z * w0.z + x.w * w0.w;
            acc[b][1] += x.x * w1.x + x.y * w1.y + x.z * w1.z + x.w * w1.w;
            acc[b][2] += x.x * w2.x + x.y * w2.y + x.z * w2.z + x.w * w2.w;
        }
    }
#pragma unroll
    for (int b = 0; b < GEMV_MAX_B; ++b) {
        if (b >= B) break;
        const float s0 = wave_sum(acc[b][0]), s1 = wave_sum(acc[b][1]), s2 = wave_sum(acc[b][2]);
        if (lane == 0) gate_fwd(b, j, H, s0, s1, s2, gi, ld_gi, b_hh, h_prev, ld_hp, h, ld_h, gates);
    }
}

// ---- recurrent step, backward ------------------------------------------------------------------------------------------------
// gate backward of one (b, j) given dh = dL/dh_t: dGi = d(Gi) (= d(x W_ih^T + b_ih)), dGh = d(h W_hh^T + b_hh), carry = dh * z
__device__ __forceinline__ void gate_bwd(int b, int j, int H, float dh, const float* __restrict__ gates, const float* __restrict__ h_prev,
                                         long ld_hp, float* __restrict__ dgi, float* __restrict__ dgh, float* __restrict__ carry) {
    const float* s = gates + (long)b * 4 * H;
    const float r = s[j], z = s[H + j], n = s[2 * H + j], hn = s[3 * H + j];
    const float hp = h_prev[(long)b * ld_hp + j];
    const float dnp = dh * (1.f - z) * (1.f - n * n);
    const float dzp = dh * (hp - n) * z * (1.f - z);
    const float drp = dnp * hn * r * (1.f - r);
    float* gi = dgi + (long)b * 3 * H;
    float* gh = dgh + (long)b * 3 * H;
    gi[j] = drp, gi[H + j] = dzp, gi[2 * H + j] = dnp;
    gh[j] = drp, gh[H + j] = dzp, gh[2 * H + j] = dnp * r;
    carry[(long)b * H + j] = dh * z;
}

__global__ void __launch_bounds__(256) gru_gates_bwd_kernel(const float* __restrict__ dy, long ld_dy, const float* __restrict__ dh_n,
                                                            const float* __restrict__ gates, const float* __restrict__ h_prev, long ld_hp,
                                                            float* __restrict__ dgi, float* __restrict__ dgh, float* __restrict__ carry,
                                                            int B, int H) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * H) return;
    const int b = (int)(e / H), j = (int)(e - (long)b * H);
    float dh = dy ? dy[(long)b * ld_dy + j] : 0.f;
    if (dh_n) dh += dh_n[e];
    gate_bwd(b, j, H, dh, gates, h_prev, ld_hp, dgi, dgh, carry);
}

// dh_{t-1}[b][j] = sum_{k < 3H} dGh_t[b][k] W_hh[k][j] + carry[b][j] + dy_prev[b][j]: a 32 x 32 tile, K = 3H split over the four
// waves as in the forward step.  A (dGh rows) is read four k at a time, B (W_hh columns) one row of 32 units per k.
__global__ void __launch_bounds__(256) gru_step_bwd_kernel(const float* __restrict__ dgh, const float* __restrict__ w_hh,
                                                           float* __restrict__ carry, const float* __restrict__ dy_prev, long ld_dy,
                                                           const float* __restrict__ gates_prev, const float* __restrict__ h_pp, long ld_hp,
                                                           float* __restrict__ dgi_prev, float* __restrict__ dgh_prev,
                                                           float* __restrict__ dh_out, long ld_out, int B, int H, int vec) {
    __shared__ float red[4][32][33];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, hh = lane >> 5;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int i = lane & 31, K = 3 * H;
    const bool arow = b0 + i < B, bcol = j0 + i < H;
    const float* ap = dgh + (long)(arow ? b0 + i : 0) * K;
    const float* bp = w_hh + (bcol ? j0 + i : 0);
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nchunks = (K + 31) / 32;
    for (int c = w; c < nchunks; c += 4) {
        float4 a[4];
        float bv[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = c * 32 + 16 * hh + 4 * q;
            a[q] = ld4(ap, k, K, arow, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[q][e] = (bcol && k + e < K) ? bp[(long)(k + e) * H] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, bv[q][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, bv[q][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, bv[q][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, bv[q][3], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[w][(r & 3) + 8 * (r >> 2) + 4 * hh][i] = acc[r];
    __syncthreads();
    for (int e = t; e < 32 * 32; e += 256) {
        const int row = e >> 5, col = e & 31, b = b0 + row, j = j0 + col;
        if (b >= B || j >= H) continue;
        float dh = ((red[0][row][col] + red[1][row][col]) + red[2][row][col]) + red[3][row][col];
        dh += carry[(long)b * H + j];
        if (dy_prev) dh += dy_prev[(long)b * ld_dy + j];
        if (dh_out) dh_out[(long)b * ld_out + j] = dh;
        if (gates_prev) gate_bwd(b, j, H, dh, gates_prev, h_pp, ld_hp, dgi_prev, dgh_prev, carry);
    }
}

// ---- output head ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gru_head_fwd_kernel(const float* __restrict__ y, long n, int F, int has_var, float* __restrict__ mean,
                                                           float* __restrict__ var) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;        // (row, key point)
    if (e >= n) return;
    const float* v = y + e * F;
    head_mean(v, mean[2 * e], mean[2 * e + 1]);
    if (has_var) head_var(v, var + 4 * e);                      // (the per-key-point formulas: gru_head.h)
}

__global__ void __launch_bounds__(256) gru_head_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dmean,
                                                           const float* __restrict__ dvar, long n, int F, int has_var,
                                                           float* __restrict__ dy) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float* v = y + e * F;
    float* o = dy + e * F;
    for (int f = 0; f < F; ++f) o[f] = 0.f;
    if (dmean) {
        float m0, m1;
        head_mean(v, m0, m1);
        head_mean_bwd(dmean[2 * e], dmean[2 * e + 1], m0, m1, o);
    }
    if (has_var && dvar) head_var_bwd(v, dvar + 4 * e, o);      // dV = V (G + G^T)
}

// ---- column sums (bias gradients) ------------------------------------------------------------------------------------------
constexpr int CS_ROWS = 128;      // rows per first-stage block
constexpr int CS_MAX_RB = 64;

int colsum_row_blocks(long rows) { return std::max(1, std::min(CS_MAX_RB, ceil_div(rows, CS_ROWS))); }

__global__ void __launch_bounds__(256) gru_colsum_kernel(const float* __restrict__ x, long ld, long rows, int cols, long rpb,
                                                         float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const long r0 = (long)blockIdx.y * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += x[r * ld + c];
    part[(long)blockIdx.y * cols + c] = s;
}

__global__ void __launch_bounds__(256) gru_colsum_finish_kernel(const float* __restrict__ part, int nb, int cols, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += part[(long)b * cols + c];
    out[c] = s;
}

bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t mnk_gru_gemm_workspace_floats(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int s = gemm_splits(M, N, K);
    return s > 1 ? (size_t)s * M * N : 0;
}

int mnk_gru_gemm(int transA, int transB, int M, int N, int K, const float* A, long lda, int a_grp, long lda_grp, const float* B,
                 long ldb, int b_grp, long ldb_grp, const float* bias, float* C, long ldc, float* ws, size_t ws_floats,
                 void* stream) {
    MNK_REQUIRE(M >= 0 && N >= 0 && K >= 0);
    if (M == 0 || N == 0) return MNK_OK;
    MNK_REQUIRE(C && ldc >= N);
    hipStream_t s = (hipStream_t)stream;
    if (K == 0) {                                               // empty sum: the bias alone
        hipLaunchKernelGGL(gru_splitk_reduce_kernel, dim3(ceil_div((long)M * N, 256)), dim3(256), 0, s, (const float*)nullptr, 0, bias, C,
                           ldc, M, N);
        MNK_LAUNCH_CHECK();
        return MNK_OK;
    }
    MNK_REQUIRE(A && B && lda >= 0 && ldb >= 0);
    const int a_rows = transA ? K : M, b_rows = transB ? N : K;
    Opnd oa{A, lda, a_grp > 0 ? lda_grp : 0, (unsigned)(a_grp > 0 ? a_grp : a_rows)};
    Opnd ob{B, ldb, b_grp > 0 ? ldb_grp : 0, (unsigned)(b_grp > 0 ? b_grp : b_rows)};
    const int splits = gemm_splits(M, N, K);
    const int kchunk = splits > 1 ? round_up(ceil_div(K, splits), GB_K) : round_up(K, GB_K);
    const int nz = ceil_div(K, kchunk);
    if (nz > 1) {
        MNK_REQUIRE(ws && ws_floats >= (size_t)nz * M * N);
    }
    float* out = nz > 1 ? ws : C;
    dim3 grid(ceil_div(N, GB_N), ceil_div(M, GB_M), nz);
    // A is K-major when transposed (stored [K][M]); B is K-major when NOT transposed (stored [K][N])
    if (transA && transB) hipLaunchKernelGGL((gru_gemm_kernel<true, false>), grid, dim3(256), 0, s, oa, ob, bias, out, ldc, M, N, K, kchunk);
    else if (transA) hipLaunchKernelGGL((gru_gemm_kernel<true, true>), grid, dim3(256), 0, s, oa, ob, bias, out, ldc, M, N, K, kchunk);
    else if (transB) hipLaunchKernelGGL((gru_gemm_kernel<false, false>), grid, dim3(256), 0, s, oa, ob, bias, out, ldc, M, N, K, kchunk);
    else hipLaunchKernelGGL((gru_gemm_kernel<false, true>), grid, dim3(256), 0, s, oa, ob, bias, out, ldc, M, N, K, kchunk);
    MNK_LAUNCH_CHECK();
    if (nz > 1) {
        hipLaunchKernelGGL(gru_splitk_reduce_kernel, dim3(ceil_div((long)M * N, 256)), dim3(256), 0, s, (const float*)ws, nz, bias, C, ldc,
                           M, N);
        MNK_LAUNCH_CHECK();
    }
    return MNK_OK;
}

size_t mnk_gru_colsum_workspace_floats(long rows, int cols) {
    return cols > 0 ? (size_t)colsum_row_blocks(rows) * cols : 0;
}

int mnk_gru_colsum(const float* x, long ld, long rows, int cols, float* out, float* ws, size_t ws_floats, void* stream) {
    MNK_REQUIRE(rows >= 0 && cols >= 0 && ld >= cols);
    if (cols == 0) return MNK_OK;
    const int nb = colsum_row_blocks(rows);
    MNK_REQUIRE(out && ws && ws_floats >= (size_t)nb * cols && (rows == 0 || x));
    const long rpb = (rows + nb - 1) / nb;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gru_colsum_kernel, dim3(ceil_div(cols, 256), nb), dim3(256), 0, s, x, ld, rows, cols, rpb, ws);
    MNK_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_colsum_finish_kernel, dim3(ceil_div(cols, 256)), dim3(256), 0, s, (const float*)ws, nb, cols, out);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_step_fwd(const float* h_prev, long ld_hp, const float* w_hh, const float* b_hh, const float* gi, long ld_gi, float* h,
                     long ld_h, float* gates, int B, int H, void* stream) {
    MNK_REQUIRE(B >= 0 && H >= 0);
    if (B == 0 || H == 0) return MNK_OK;
    MNK_REQUIRE(h_prev && w_hh && b_hh && gi && h && ld_hp >= H && ld_gi >= 3 * H && ld_h >= H);
    hipStream_t s = (hipStream_t)stream;
    const int vec = (H % 4 == 0 && ld_hp % 4 == 0 && aligned16(h_prev) && aligned16(w_hh)) ? 1 : 0;
    if (B <= std::min(g_gru_gemv_rows, GEMV_MAX_B))
        hipLaunchKernelGGL(gru_step_fwd_gemv_kernel, dim3(ceil_div(H, 4)), dim3(256), 0, s, h_prev, ld_hp, w_hh, b_hh, gi, ld_gi, h, ld_h,
                           gates, B, H, vec);
    else
        hipLaunchKernelGGL(gru_step_fwd_kernel, dim3(ceil_div(H, 32), ceil_div(B, 32)), dim3(256), 0, s, h_prev, ld_hp, w_hh, b_hh, gi,
                           ld_gi, h, ld_h, gates, B, H, vec);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_gates_bwd(const float* dy, long ld_dy, const float* dh_n, const float* gates, const float* h_prev, long ld_hp, float* dgi,
                      float* dgh, float* carry, int B, int H, void* stream) {
    MNK_REQUIRE(B >= 0 && H >= 0);
    if (B == 0 || H == 0) return MNK_OK;
    MNK_REQUIRE(gates && h_prev && dgi && dgh && carry && ld_hp >= H && (!dy || ld_dy >= H));
    hipLaunchKernelGGL(gru_gates_bwd_kernel, dim3(ceil_div((long)B * H, 256)), dim3(256), 0, (hipStream_t)stream, dy, ld_dy, dh_n, gates,
                       h_prev, ld_hp, dgi, dgh, carry, B, H);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_step_bwd(const float* dgh, const float* w_hh, float* carry, const float* dy_prev, long ld_dy, const float* gates_prev,
                     const float* h_pp, long ld_hp, float* dgi_prev, float* dgh_prev, float* dh_out, long ld_out, int B, int H,
                     void* stream) {
    MNK_REQUIRE(B >= 0 && H >= 0);
    if (B == 0 || H == 0) return MNK_OK;
    MNK_REQUIRE(dgh && w_hh && carry && (!dy_prev || ld_dy >= H) && (!dh_out || ld_out >= H));
    MNK_REQUIRE(!gates_prev || (h_pp && ld_hp >= H && dgi_prev && dgh_prev));
    const int vec = ((3 * H) % 4 == 0 && aligned16(dgh)) ? 1 : 0;
    hipLaunchKernelGGL(gru_step_bwd_kernel, dim3(ceil_div(H, 32), ceil_div(B, 32)), dim3(256), 0, (hipStream_t)stream, dgh, w_hh, carry,
                       dy_prev, ld_dy, gates_prev, h_pp, ld_hp, dgi_prev, dgh_prev, dh_out, ld_out, B, H, vec);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_head_fwd(const float* y, long rows, int num_kp, int feats, int has_var, float* mean, float* var, void* stream) {
    MNK_REQUIRE(rows >= 0 && num_kp >= 0 && feats >= (has_var ? 6 : 2));
    const long n = rows * num_kp;
    if (n == 0) return MNK_OK;
    MNK_REQUIRE(y && mean && (!has_var || var));
    hipLaunchKernelGGL(gru_head_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, y, n, feats, has_var, mean, var);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_gru_head_bwd(const float* y, const float* dmean, const float* dvar, long rows, int num_kp, int feats, int has_var, float* dy,
                     void* stream) {
    MNK_REQUIRE(rows >= 0 && num_kp >= 0 && feats >= (has_var ? 6 : 2));
    const long n = rows * num_kp;
    if (n == 0) return MNK_OK;
    MNK_REQUIRE(y && dy);
    hipLaunchKernelGGL(gru_head_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, y, dmean, dvar, n, feats, has_var,
                       dy);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

}  // extern "C"
