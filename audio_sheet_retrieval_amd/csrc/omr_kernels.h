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

#ifdef __HIPCC__
// one prepared pixel (prepare_image folded in: an IEEE divide by the page maximum unless that is 0)
__device__ __forceinline__ float seg_load_page(const void *pages, int in_mode, int64_t off, float mx) {
    if (in_mode == 2) {
        const float v = (float)((const uint8_t *)pages)[off];
        return mx != 0.0f ? __fdiv_rn(v, mx) : v;
    }
    const float v = ((const float *)pages)[off];
    if (in_mode == 1 && mx != 0.0f) return __fdiv_rn(v, mx);
    return v;
}
#endif

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

// ---- systems_from_maps on the device (omr_post_kernels.hip; host side: asr_systems_from_maps_dev) -------------------
constexpr int POST_MIN_AREA = 50000;       // detect_systems: smallest system blob
constexpr int POST_MAX_LEAVES = 1024;      // leaves of numpy's pairwise row sum that one row may have (width <= 65536)
constexpr int POST_MAX_CHUNK_PAGES = 65535; // pages of one chunk: the y dimension of the launch grids

// one leaf (8 <= len <= 128 elements at `off`) of numpy's pairwise sum over a row
struct PostLeaf {
    int32_t off, len;
};

// one page of a chunk: where its pixels, maps and workspace sections start
struct PostPage {
    int64_t page_off;               // first pixel in the page buffer (elements)
    int64_t map_off;                // first pixel in the probability maps
    int64_t px_off;                 // first pixel in the per-pixel workspace arrays
    int32_t h, w;
    int32_t row_off;                // first row in the per-row workspace arrays
    int32_t leaf_off, n_leaves;     // the row-sum leaves of width w, and the postfix program that combines them
    int32_t prog_off, n_prog;       // (0: push the next leaf sum, 1: add the two topmost values)
    int32_t page;                   // index of the page in the call (page maxima)
};

// per page, written by the kernels and read back by the host
struct PostState {
    double thr2;                    // Otsu threshold of the cleaned system map
    double edges2_first, edges2_last;
    int32_t status;                 // 0 ok, 1 no row below the projection threshold, 3 not decided here
    int32_t nonfinite;              // a NaN / infinity in a map or in the page signal
    uint32_t n_kept;                // blobs of at least POST_MIN_AREA pixels (may exceed the capacity)
    int32_t pad_;
};

// per kept blob: bounding box (inclusive) from the labelling, then the result of shrink + snap
struct PostBlob {
    int32_t root;                   // smallest linear pixel index of the blob
    int32_t min_r, min_c, max_r, max_c;
    int32_t status;                 // 0 ok, 2 no edge candidate, 3 not decided here
    int32_t out[4];                 // min_row, max_row, min_col, max_col
    int32_t pad_[2];
};

struct PostArgs {
    const PostPage *pages = nullptr;
    int n_pages = 0, max_h = 0, max_w = 0, cap = 0;
    int64_t max_px = 0;
    const void *page_buf = nullptr;
    int in_mode = 0;
    const float *page_max = nullptr;
    const double *sys_maps = nullptr, *bar_maps = nullptr;     // bar_maps may be NULL
    const PostLeaf *leaves = nullptr;
    const uint8_t *prog = nullptr;
    PostState *state = nullptr;
    PostBlob *blobs = nullptr;      // n_pages x cap
    double *proj = nullptr, *rmin = nullptr, *rmax = nullptr;  // per row
    float *ysig = nullptr;          // per row: snap_system_to_grid's y edge signal
    uint8_t *rowzero = nullptr;     // per row: zeroed by the gap clean-up
    double *edges2 = nullptr;       // n_pages x 257
    uint32_t *hist2 = nullptr;      // n_pages x 256
    uint8_t *fg = nullptr, *tmp = nullptr;                     // per pixel
    int32_t *label = nullptr, *area = nullptr;                 // per pixel
    float *xsig = nullptr;          // n_pages x cap x max_w
    int32_t *changed = nullptr;     // one flag of the labelling passes
};

// the stages in call order; launch_post_label_pass is repeated until *changed stays 0
hipError_t launch_post_rows(hipStream_t s, const PostArgs &a);       // row sums, row extrema, y edge signal
hipError_t launch_post_threshold(hipStream_t s, const PostArgs &a);  // Otsu 1, gap clean-up, histogram + Otsu 2
hipError_t launch_post_close(hipStream_t s, const PostArgs &a);      // threshold, 15x1 closing, run labels
hipError_t launch_post_label_pass(hipStream_t s, const PostArgs &a);
hipError_t launch_post_blobs(hipStream_t s, const PostArgs &a);      // areas, kept blobs, boxes, shrink + snap

// ---- bars and note heads from the maps (omr_detect_kernels.hip; host side: asr_notes_from_map_dev,
// asr_bars_from_map_dev).  Pages are PostPage (map_off, px_off, row_off, h, w), the per-page state is PostState
// (status, nonfinite, thr2 = the Otsu threshold, n_kept = peaks / blobs found), so that the labelling passes of
// omr_post_kernels.hip run on the same tables.
constexpr int DET_MAX_DISTANCE = 8;        // largest min_distance of the peak search: the halo of its LDS tile
constexpr int DET_TILE_H = 32, DET_TILE_W = 64;   // page pixels one workgroup of the peak search decides
constexpr int DET_BLOB_FIELDS = 10;        // area, min_row, min_col, max_row, max_col, sum r, c, r*r, c*c, r*c

struct DetArgs {
    const PostPage *pages = nullptr;
    int n_pages = 0, max_h = 0, max_w = 0, cap = 0;            // cap: peaks / blobs per page the outputs hold
    int64_t max_px = 0;
    const double *maps = nullptr;
    PostState *state = nullptr;
    unsigned long long *minmax = nullptr;   // per page: ~key(min), key(max) of the order-preserving integer key
    double threshold_abs = 0.0, threshold_rel = 0.0;           // NaN: not given
    int distance = 0;
    int32_t *rowcnt = nullptr;              // per row: flagged pixels, then their exclusive prefix sum over the page
    uint8_t *mask = nullptr;                // notes, per pixel: is a peak
    int32_t *coords = nullptr;              // notes: n_pages x cap x (row, col)
    double *edges = nullptr;                // bars: n_pages x 257
    uint32_t *hist = nullptr;               // bars: n_pages x 256
    int32_t *label = nullptr, *slot = nullptr;                 // bars, per pixel: root; at a root: its blob index
    long long *blobs = nullptr;             // bars: n_pages x cap x DET_BLOB_FIELDS
};

hipError_t launch_det_minmax(hipStream_t s, const DetArgs &a);        // page extrema, non-finite flag, status
hipError_t launch_det_peaks(hipStream_t s, const DetArgs &a);         // peak mask, row counts, scan, ordered write
hipError_t launch_det_bar_threshold(hipStream_t s, const DetArgs &a); // np.histogram + Otsu, map > t, run labels
hipError_t launch_det_bar_blobs(hipStream_t s, const DetArgs &a);     // roots in raster order, the ten integers each

}  // namespace asr
