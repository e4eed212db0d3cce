// Staff-system detector (sheet_utils/system_detector.py, bar_detector.py): the U-Net forward of a batch of tiles and the
// sliding-window stitch, fp32 activations in NCHW per tile (omr_kernels.hip).  Host side: asr_api_omr.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace asr {

// one page of a call: pixels at `offset` (elements of the page buffer, row-major h x w)
struct SegPage {
    int64_t offset;
    int32_t h, w;
};

// one tile of the forward: page, origin of the tile in page coordinates (negative inside the top/left padding)
struct SegTile {
    int32_t page, y0, x0, pad_;
};

// stitch of one page (SegmentationNetwork._predict_proba_sliding_window)
struct SegStitch {
    int64_t out_offset;             // first pixel of the page in the output map
    int32_t h, w;                   // page size (= the crop)
    int32_t pad_top, pad_left;      // padding of the page to a multiple of the tile
    int32_t n_rows, n_cols;         // tile grid; tile (r, c) starts at (r * step_h, c * step_w) in padded coordinates
    int32_t step_h, step_w;
    int32_t first_tile;             // index of tile (0, 0) in the tile-probability buffer, row-major grid
    int32_t direct;                 // page == tile: the network output as it is
};

// in_mode of the first block, as asr_embed_*: 0 prepared float32, 1 raw float32, 2 raw uint8 (prepare_image: / page max)
// page_max: one float per page (modes 1, 2)
hipError_t launch_seg_page_max(hipStream_t s, const void *pages, int in_mode, const SegPage *desc, int n_pages,
                               float *page_max);

// 3x3 'same' conv (flip_filters=True) + BN + ELU over n tiles of H x W.
//   w: [ci][3][3][co] of the flipped kernel; bn: mean[co] scale[co] beta[co] (scale = gamma * inv_std)
//   pooled != nullptr: the 2x2/2 max-pool of the output as well; head != nullptr (ci = co = 8): the 1x1 conv + sigmoid
//   head (w[8], b) instead, one channel out
//   first block (ci = 1): `in` is the page buffer read through `tiles` / `pages` (zero outside page and tile)
struct SegConvArgs {
    const float *in = nullptr;
    const void *pages = nullptr;
    const SegPage *page_desc = nullptr;
    const SegTile *tiles = nullptr;
    const float *page_max = nullptr;
    int in_mode = 0;
    const float *w = nullptr, *bn = nullptr, *head = nullptr;
    float *out = nullptr, *pooled = nullptr;
    int ci = 0, co = 0, H = 0, W = 0, n = 0;
};
hipError_t launch_seg_conv3(hipStream_t s, const SegConvArgs &a);

// decoder level: TransposedConv2D 2x2/2 (w: [ci][2][2][co], already in output orientation) + BN + ReLU, + skip, + BN.
// in: n x ci x h x w; skip, out: n x co x 2h x 2w
hipError_t launch_seg_up(hipStream_t s, const float *in, const float *w, const float *bn1, const float *bn2,
                         const float *skip, float *out, int ci, int co, int h, int wd, int n);

// gather stitch: out[p] = sum_t P_t * win / sum_t win over the tiles covering p, float64, in the reference's tile order
hipError_t launch_seg_stitch(hipStream_t s, const float *tile_p, const double *win, int th, int tw,
                             const SegStitch *desc, int n_pages, int max_pixels, double *out);

}  // namespace asr
