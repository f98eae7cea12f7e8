// What the two convolution translation units share: conv3x3.hip (forward / data-gradient implicit GEMM, packs) and
// conv3x3_wgrad.hip (weight-gradient GEMMs, their plans and reductions).
#pragma once
#include "mnk_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// tuning values both dispatches read (forward: conv2d_fwd_impl; weight gradient: tap_mode / the single-layer launch).  ONE slot
// each, defined in conv3x3.hip: mnk_set_tuning writes the first slot registered under a name and stops
namespace mnk {
extern __attribute__((visibility("hidden"))) int g_xcd_remap, g_fast_loader;
// "force_splits" and the plan mnk_last_plan reports ({M, Cout, chunks, taps, phases, bm, bn, splits}): conv3x3.hip's, also read and
// written by the weight-streaming form (conv_skinny.hip)
extern __attribute__((visibility("hidden"))) int g_force_splits;
extern __attribute__((visibility("hidden"))) long g_last_plan[8];
}

namespace {

constexpr int BK = 16;        // K step (floats)
constexpr int LDS_K = 20;     // padded LDS row (floats)

// buffer resource from values the compiler cannot prove wave-uniform (e.g. derived from a 64-bit division): pin the
// pointer into scalar registers, otherwise every buffer load becomes a readfirstlane "waterfall" loop
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* p, unsigned num_records) {
    unsigned long v = (unsigned long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    const unsigned nr = __builtin_amdgcn_readfirstlane((int)num_records);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long)hi << 32) | lo), 0, (int)nr, 0x00020000);
}

struct TrueTag { static constexpr bool value = true; };
struct FalseTag { static constexpr bool value = false; };

// n / d for n < 2^31 with host-made constants (fast_div_consts): mulhi + shift, or a shift alone when mul == 0
__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned mul, unsigned sh) {
    return mul ? __umulhi(n, mul) >> sh : n >> sh;
}

// Workgroups are handed to the 8 XCDs round-robin in launch order (x fastest), and every XCD has its own L2: with the
// plain mapping each XCD touches every weight tile and every pixel tile of a layer, so both operands cross the fabric
// up to 8 times.  Re-chunking the launch order -- XCD class c = L % 8 works on the contiguous range
// [start(c), start(c) + count(c)) of the logical (x fastest, then y) tile order -- gives each XCD a few complete rows
// of the tile grid: one operand is fetched once per chip, the other once per XCD that needs it.  (Placement is not
// guaranteed by the hardware; this is a locality heuristic only -- any mapping is correct.)
__device__ __forceinline__ void xcd_tile(int enable, int& bx, int& by) {
    bx = blockIdx.x;
    by = blockIdx.y;
    const unsigned gx = gridDim.x, per_z = gx * gridDim.y;
    if (!enable || per_z < 16) return;
    const unsigned L = blockIdx.x + gx * blockIdx.y, c = L & 7u, base = per_z >> 3, rem = per_z & 7u;
    const unsigned logical = c * base + (c < rem ? c : rem) + (L >> 3);
    by = (int)(logical / gx);
    bx = (int)(logical - (unsigned)by * gx);
}

// n / d for n < 2^31 as (mulhi(n, mul) >> sh), or (n >> sh) when mul == 0 (d a power of two)
static void fast_div_consts(unsigned d, unsigned* mul, unsigned* sh) {
    unsigned s = 0;
    while ((1u << s) < d) ++s;
    if ((1u << s) == d) {
        *mul = 0;
        *sh = s;
        return;
    }
    const unsigned long long num = 1ull << (31 + s);
    *mul = (unsigned)((num + d - 1) / d);
    *sh = s - 1;
}

static inline int grid_for(long total, int cap = 4096) {
    long b = (total + 255) / 256;
    if (b < 1) b = 1;
    return (int)(b < cap ? b : cap);
}

}  // namespace
