// Device-side output path: the uint8 image grids of the reference's Visualizer and the PNG strips of its evaluation loops.
//
// Replaces
//   logger.py:97-106    Visualizer.draw_video_with_kp   (skimage.draw.circle per key point and frame, in a Python loop)
//   logger.py:108-126   create_video_column[_with_kp], create_image_grid  (border, np.concatenate along rows and width)
//   logger.py:128-175   visualize_transfer / visualize_reconstruction: four to six fp32 videos copied to the host, transposed,
//                       `.repeat(1, 1, d, 1, 1)` of the source frame and key points, `(255 * image).astype(np.uint8)`
//   reconstruction.py:66-68, prediction.py:137-139   the uint8 frame strip that is saved as .png
// which the reference runs on the host in numpy.  Here the videos stay where the generator left them; one launch reads every
// column through its own strides (a stride of 0 IS the repeat) and writes the uint8 grid, the only bytes that cross PCIe.
// HBM-bound byte work: a thread owns a run of 4 output pixels of one row of one column (12 bytes, three packed dword stores; the
// threads of a wave cover consecutive runs of an output row), reads one float4 per channel plane (coalesced along W) and tests
// its pixels against the K <= 32 key points of its (column, video, frame) in float64 -- the arithmetic of numpy and
// scikit-image 0.14, statement by statement, so that every byte equals the reference's.
#include "frame_bytes.h"      // vis_byte: `(255 * image).astype(np.uint8)`

using namespace mnk;

namespace {

#pragma clang fp contract(off)      // (every product and sum rounds on its own, as numpy's do)

constexpr int VIS_MAX_COLS = 8;
constexpr int VIS_MAX_KP = 32;
constexpr int VIS_RUN = 4;          // output pixels per thread

struct VisColumns {                 // the column table, by value in the kernel arguments
    MnkVisColumn c[VIS_MAX_COLS];
};

// One axis of skimage.draw.ellipse's bounding box (scikit-image 0.14, draw.py: upper_left = ceil(center - radii) clipped to 0,
// lower_right = floor(center + radii) clipped to shape - 1, shifted_center = center - upper_left), all in float64.  The box
// corners are integers held in doubles (numpy's int64 -> float64 conversion of the same integers is exact).
struct VisAxis {
    double ul, lr, shifted;
};
__device__ __forceinline__ VisAxis vis_axis(float kp, int size, double r) {
    // logger.py:99-100 as numpy evaluates it: `kp_array + 1` in float32, int64 size * float32 -> float64, / 2 in float64
    // (the arithmetic of kp_pixel_index_kernel, keypoints.hip)
    const float t = __fadd_rn(kp, 1.f);
    const double centre = (double)size * (double)t / 2.0;
    VisAxis a;
    a.ul = ceil(centre - r);
    a.ul = a.ul > 0.0 ? a.ul : 0.0;                     // np.maximum(upper_left, 0); a NaN centre gives an empty box below
    a.lr = floor(centre + r);
    a.lr = a.lr < (double)(size - 1) ? a.lr : (double)(size - 1);
    if (!(centre == centre)) a.lr = -1.0;               // NaN: numpy's box is empty (lower_right = INT_MIN)
    a.shifted = centre - a.ul;
    return a;
}
// _ellipse_in_shape's term of one axis: ((p' - shifted) / radius) ** 2 for p' = p - upper_left, p inside the box
__device__ __forceinline__ double vis_term(const VisAxis& a, int p, double r) {
    const double q = (((double)p - a.ul) - a.shifted) / r;
    return q * q;
}

// grid: ceil(d * B * H * ncol * ceil(W / 4) / 256) blocks of 256 threads; thread -> (frame, video, row, column, run) in the
// order of the output bytes.  VEC: W % 4 == 0 and every plane 16-byte aligned (float4 loads, dword stores).
template <bool VEC>
__global__ void __launch_bounds__(256) vis_grid_kernel(const VisColumns cols, int ncol, int B, int d, int H, int W, int K, double r,
                                                       int draw_border, const float* __restrict__ colors,
                                                       unsigned char* __restrict__ out) {
    const int runs = (W + VIS_RUN - 1) / VIS_RUN;
    const long total = (long)d * B * H * ncol * runs;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int run = (int)(i % runs);
    long q = i / runs;
    const int col = (int)(q % ncol);
    q /= ncol;
    const int h = (int)(q % H);
    q /= H;
    const int b = (int)(q % B);
    const int f = (int)(q / B);
    const int w0 = run * VIS_RUN;
    const int n = W - w0 < VIS_RUN ? W - w0 : VIS_RUN;
    const MnkVisColumn& c = cols.c[col];

    float v[3][VIS_RUN];
    const float* src = c.video + (long)b * c.batch_stride + (long)f * c.frame_stride + (long)h * W + w0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* p = src + (long)ch * c.chan_stride;
        if (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(p);
            v[ch][0] = x.x, v[ch][1] = x.y, v[ch][2] = x.z, v[ch][3] = x.w;
        } else {
#pragma unroll
            for (int j = 0; j < VIS_RUN; ++j) v[ch][j] = j < n ? p[j] : 0.f;
        }
    }

    if (c.kp != nullptr) {
        const float* kp = c.kp + (long)b * c.kp_batch_stride + (long)f * c.kp_frame_stride;
        int owner[VIS_RUN] = {-1, -1, -1, -1};          // the last key point painted over each pixel
        for (int k = 0; k < K; ++k) {
            // circle(kp[1], kp[0], kp_size, shape=(H, W)): kp[0] is the column (x, scaled by W), kp[1] the row (y, by H)
            const VisAxis ay = vis_axis(kp[2 * k + 1], H, r);
            if (!((double)h >= ay.ul && (double)h <= ay.lr)) continue;
            const VisAxis ax = vis_axis(kp[2 * k], W, r);
            const double ty = vis_term(ay, h, r);
#pragma unroll
            for (int j = 0; j < VIS_RUN; ++j) {
                const int x = w0 + j;
                if ((double)x >= ax.ul && (double)x <= ax.lr && ty + vis_term(ax, x, r) < 1.0) owner[j] = k;
            }
        }
#pragma unroll
        for (int j = 0; j < VIS_RUN; ++j)
            if (owner[j] >= 0) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][j] = colors[3 * owner[j] + ch];
            }
    }
    if (draw_border) {                                  // after the key points: the border wins (logger.py:113-116)
        const bool row = h == 0 || h == H - 1;
#pragma unroll
        for (int j = 0; j < VIS_RUN; ++j)
            if (row || w0 + j == 0 || w0 + j == W - 1) v[0][j] = v[1][j] = v[2][j] = 1.f;
    }

    unsigned char* o = out + ((((long)f * B + b) * H + h) * ((long)ncol * W) + (long)col * W + w0) * 3;
    if (VEC) {
        unsigned by[12];
#pragma unroll
        for (int j = 0; j < VIS_RUN; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) by[3 * j + ch] = vis_byte(v[ch][j]);
        unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int t = 0; t < 3; ++t) o32[t] = by[4 * t] | (by[4 * t + 1] << 8) | (by[4 * t + 2] << 16) | (by[4 * t + 3] << 24);
    } else {
        for (int j = 0; j < n; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * j + ch] = (unsigned char)vis_byte(v[ch][j]);
    }
}

// grid: ceil(H * D * ceil(W / 4) / 256) blocks; thread -> (row, frame, run) in the order of the strip's bytes
template <bool VEC>
__global__ void __launch_bounds__(256) frames_to_strip_kernel(const float* __restrict__ video, long chan_stride, long frame_stride,
                                                              int D, int H, int W, unsigned char* __restrict__ out) {
    const int runs = (W + VIS_RUN - 1) / VIS_RUN;
    const long total = (long)H * D * runs;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int run = (int)(i % runs);
    const long q = i / runs;
    const int f = (int)(q % D), h = (int)(q / D);
    const int w0 = run * VIS_RUN;
    const int n = W - w0 < VIS_RUN ? W - w0 : VIS_RUN;
    const float* src = video + (long)f * frame_stride + (long)h * W + w0;
    unsigned char* o = out + (((long)h * D + f) * W + w0) * 3;
    if (VEC) {
        unsigned by[12];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float4 x = *reinterpret_cast<const float4*>(src + (long)ch * chan_stride);
            by[ch] = vis_byte(x.x), by[3 + ch] = vis_byte(x.y), by[6 + ch] = vis_byte(x.z), by[9 + ch] = vis_byte(x.w);
        }
        unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int t = 0; t < 3; ++t) o32[t] = by[4 * t] | (by[4 * t + 1] << 8) | (by[4 * t + 2] << 16) | (by[4 * t + 3] << 24);
    } else {
        for (int j = 0; j < n; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * j + ch] = (unsigned char)vis_byte(src[(long)ch * chan_stride + j]);
    }
}

inline bool vis_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int mnk_vis_grid(const MnkVisColumn* cols, int ncol, int B, int C, int d, int H, int W, int K, double kp_size, int draw_border,
                 const float* colors, uint8_t* out, void* stream) {
    MNK_REQUIRE(cols && out && ncol > 0 && ncol <= VIS_MAX_COLS && C == 3);
    MNK_REQUIRE(B > 0 && d > 0 && H > 0 && W > 0 && K >= 0 && K <= VIS_MAX_KP);
    MNK_REQUIRE((long)d * B * H * ncol * W <= (1L << 31));
    VisColumns table;
    memset(&table, 0, sizeof(table));
    bool vec = W % 4 == 0 && vis_aligned(out, 4), any_kp = false;
    for (int i = 0; i < ncol; ++i) {
        const MnkVisColumn& c = cols[i];
        MNK_REQUIRE(c.video != nullptr && c.batch_stride >= 0 && c.chan_stride >= 0 && c.frame_stride >= 0);
        MNK_REQUIRE(c.kp == nullptr || (c.kp_batch_stride >= 0 && c.kp_frame_stride >= 0));
        any_kp = any_kp || c.kp != nullptr;
        vec = vec && vis_aligned(c.video, 16) && c.batch_stride % 4 == 0 && c.chan_stride % 4 == 0 && c.frame_stride % 4 == 0;
        table.c[i] = c;
    }
    MNK_REQUIRE(!any_kp || (K > 0 && colors != nullptr && kp_size > 0.0));
    hipStream_t s = (hipStream_t)stream;
    const long threads = (long)d * B * H * ncol * ((W + VIS_RUN - 1) / VIS_RUN);
    ProfScope prof(K_LAYOUT, s, (double)d * B * H * ncol * W * (12.0 + 3.0));
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(vis_grid_kernel<true>, grid, dim3(256), 0, s, table, ncol, B, d, H, W, K, kp_size, draw_border, colors,
                           (unsigned char*)out);
    else
        hipLaunchKernelGGL(vis_grid_kernel<false>, grid, dim3(256), 0, s, table, ncol, B, d, H, W, K, kp_size, draw_border, colors,
                           (unsigned char*)out);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

int mnk_frames_to_strip(const float* video, int C, long chan_stride, long frame_stride, int D, int H, int W, uint8_t* out,
                        void* stream) {
    MNK_REQUIRE(video && out && C == 3 && D > 0 && H > 0 && W > 0 && chan_stride >= 0 && frame_stride >= 0);
    MNK_REQUIRE((long)D * H * W <= (1L << 31));
    hipStream_t s = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && vis_aligned(out, 4) && vis_aligned(video, 16) && chan_stride % 4 == 0 && frame_stride % 4 == 0;
    const long threads = (long)H * D * ((W + VIS_RUN - 1) / VIS_RUN);
    ProfScope prof(K_LAYOUT, s, (double)D * H * W * (12.0 + 3.0));
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(frames_to_strip_kernel<true>, grid, dim3(256), 0, s, video, chan_stride, frame_stride, D, H, W,
                           (unsigned char*)out);
    else
        hipLaunchKernelGGL(frames_to_strip_kernel<false>, grid, dim3(256), 0, s, video, chan_stride, frame_stride, D, H, W,
                           (unsigned char*)out);
    MNK_LAUNCH_CHECK();
    return MNK_OK;
}

}  // extern "C"
