// The two conversions between uint8 frames and the fp32 values of the hot path, one expression each, so that every kernel
// that reads or writes frame bytes agrees with the others bit for bit.
#pragma once
#include "mnk_common.h"

namespace mnk {

// img_as_float32 on uint8 (frames_dataset.py:26): uint8 * float32(1 / 255) -- the expression of frames_gather_kernel
__device__ __forceinline__ float byte_unit(unsigned b) {
    return (float)b * (1.f / 255.f);
}

// `(255 * image).astype(np.uint8)` (logger.py:151, :174; demo.py:69-71; reconstruction.py:66-68): a float32 product (255 is a
// Python int: the array stays float32), truncated toward zero
__device__ __forceinline__ unsigned vis_byte(float v) {
    return (unsigned)(int)__fmul_rn(255.f, v) & 255u;
}

inline bool ptr_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace mnk
