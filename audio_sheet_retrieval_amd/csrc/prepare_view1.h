// model.prepare of the sheet view (models/mutopia_ccal_cont.py:170-190, _rsz.py:170-190) as ONE device expression,
// shared by every kernel that turns a raw sheet into the prepared float32 image: block 1 of the embedding
// (conv_kernels.hip: conv1_kernel) and the training step's prepare kernel (train_fwd_kernels.hip:
// prepare_view1_kernel).  Both evaluate exactly prepare_plain / prepare_rsz (models/_common.py), bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/asr_hip.h"

namespace asr {

// The 256 correctly rounded quotients v / 255.0f of a uint8 input, one per entry of `tab` (LDS), written by the
// block's threads; the caller synchronises before reading.  The IEEE division costs ~10 VALU instructions per tap.
__device__ __forceinline__ void fill_div255(float *tab) {
    for (unsigned i = threadIdx.x; i < 256u; i += blockDim.x) tab[i] = (float)i / 255.0f;
}

// tab (uint8 inputs only; may be null): the table fill_div255 writes.
template <int IN_MODE>
__device__ __forceinline__ float load_prepared(const void *in, size_t img_off_raw, int Wraw,
                                               int y, int x, int H, int W, int rsz, const float *tab = nullptr) {
    // returns the prepared pixel (y,x) of the network-resolution image, 0 outside
    if (y < 0 || y >= H || x < 0 || x >= W) return 0.0f;
    if (IN_MODE == ASR_IN_F32_PREPARED) {
        return ((const float *)in)[img_off_raw + (size_t)y * W + x];
    }
    auto rawn = [&](int yy, int xx) -> float {          // raw value / 255 (model.prepare)
        if (IN_MODE == ASR_IN_U8_RAW) {
            const unsigned char v = ((const unsigned char *)in)[img_off_raw + (size_t)yy * Wraw + xx];
            return tab ? tab[v] : (float)v / 255.0f;
        }
        return ((const float *)in)[img_off_raw + (size_t)yy * Wraw + xx] / 255.0f;
    };
    if (!rsz) return rawn(y, x);
    // rsz prepare: /255, then bilinear factor-2 = (.5,.5) horizontally, then vertically
    const float a = rawn(2 * y, 2 * x), b = rawn(2 * y, 2 * x + 1);
    const float c = rawn(2 * y + 1, 2 * x), d = rawn(2 * y + 1, 2 * x + 1);
    const float top = a * 0.5f + b * 0.5f, bot = c * 0.5f + d * 0.5f;
    return top * 0.5f + bot * 0.5f;
}

}  // namespace asr
