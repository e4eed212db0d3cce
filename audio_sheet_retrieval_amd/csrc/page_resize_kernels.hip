// Score pages of any resolution to the width the OMR networks were trained on (asr_resize_pages_dev; include/asr_hip.h
// carries the definition): exact area resampling in integers, separable, uint8 -> uint8.
//
//   resize_pages_kernel : all pages of all pieces in one launch.  The output of every page is cut into tiles of
//                         RESIZE_TILE_H rows x RESIZE_TILE_W columns, the tiles of all pages are numbered through
//                         (tile_first[p] = number of the first tile of page p, n_pages + 1 entries, column tiles fastest)
//                         and one 64-thread workgroup - one wave - takes one tile: it finds its page by binary search (as
//                         resample_batch_kernel does for its tiles), and lane l owns output column c0 + l.
//
// The source rows of a tile are walked top to bottom in chunks of as many rows as fit RESIZE_LDS_BYTES.  A chunk is
// staged in LDS with aligned 16-byte loads: row j of the tile needs bytes [a, a + span) of the page buffer, and the lanes
// load the 16-byte pieces from a & ~15 on that hold at least one of them - consecutive lanes consecutive pieces, several
// rows per instruction when a row needs fewer than 64, RESIZE_BATCH instructions in flight.  An aligned piece that holds
// one valid byte lies in that byte's memory page, so the bytes before `a` and behind the span are read (they belong to the neighbouring row, page or
// allocation slack) and never used; nothing is read that is not in such a piece.  Rows start at any alignment (w_in is
// odd more often than not), so every row has its own head = a & 15, and the readers add it back.
//
// Then, per source row, every lane forms the horizontal sum of its column's footprint once - first and last source pixel
// with their partial weights, the ones between with weight w_out, at most 255 * w_in < 2^32 - and the wave merges the row
// grid of the source with that of the output: the sum goes with weight wy into the one output row (or, where the source
// row straddles a border, the two; when enlarging, the several) it overlaps, in a 64-bit accumulator per lane.  An output
// row is finished when the walk reaches its lower border: out = (2 * S + D) / (2 * D), D = h_in * w_in.  The quotient is
// at most 255, so it is estimated in float32 (relative error < 1e-6: off by one at most) and corrected with the exact
// 64-bit remainder.  All positions are kept relative to the tile's first source row / column: with every dimension at
// most 2^24 and ratios up to RESIZE_MAX_DOWN they stay below 2^31.  The row walk depends on the tile alone and is uniform
// over the wave.
#include "asr_kernels.h"

namespace asr {

// exact (num / den) for a quotient known to be at most 255: den < 2^32, num < 2^41
__device__ __forceinline__ uint32_t small_quotient(uint64_t num, uint32_t den) {
    uint32_t q = (uint32_t)((float)num * __builtin_amdgcn_rcpf((float)den));
    int64_t rem = (int64_t)num - (int64_t)((uint64_t)q * den);
    if (rem < 0) { --q; rem += den; }
    if (rem >= (int64_t)den) ++q;
    return q;
}

// x / d and x % d for x < 2^53 and a quotient below 2^32, without the 64-bit integer division: the float64 quotient is
// the exact one rounded, so its integer part is the floor or one more
__device__ __forceinline__ uint32_t floor_div(uint64_t x, uint32_t d, uint32_t &rem) {
    uint32_t q = (uint32_t)((double)x / (double)d);
    int64_t r = (int64_t)x - (int64_t)((uint64_t)q * d);
    if (r < 0) { --q; r += d; }
    if (r >= (int64_t)d) { ++q; r -= d; }
    rem = (uint32_t)r;
    return q;
}

__global__ __launch_bounds__(64) void resize_pages_kernel(const uint8_t *__restrict__ pages, uint8_t *__restrict__ out,
                                                          const int64_t *__restrict__ tile_first,
                                                          const ResizePage *__restrict__ table, int n_pages) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[RESIZE_LDS_BYTES];
    const int64_t g = blockIdx.x;
    int lo = 0, hi = n_pages - 1;                                   // last p with tile_first[p] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const ResizePage pg = table[lo];
    const uint32_t h_in = pg.h_in, w_in = pg.w_in, h_out = pg.h_out, w_out = pg.w_out;
    const uint32_t t = (uint32_t)(g - tile_first[lo]);
    const uint32_t r0 = (t / pg.tiles_x) * RESIZE_TILE_H, c0 = (t % pg.tiles_x) * RESIZE_TILE_W;
    const uint32_t th = min((uint32_t)RESIZE_TILE_H, h_out - r0), tw = min((uint32_t)RESIZE_TILE_W, w_out - c0);
    const uint32_t lane = threadIdx.x;

    // columns: positions in units of 1 / (w_in * w_out) of the width, relative to the left border of source column k_lo
    uint32_t rem_x, rem_y;
    const uint32_t k_lo = floor_div((uint64_t)c0 * w_in, w_out, rem_x);
    const uint32_t span = (rem_x + tw * w_in + w_out - 1) / w_out;  // source columns k_lo .. k_lo + span - 1
    // lanes past the tile's last column repeat it (their reads stay inside the span) and store nothing
    const uint32_t x0 = rem_x + min(lane, tw - 1) * w_in, x1 = x0 + w_in;
    const uint32_t k0 = x0 / w_out, k1 = (x1 + w_out - 1) / w_out;  // the column's footprint: k0 .. k1 - 1 (relative)
    const uint32_t n_mid = k1 - k0 > 2 ? k1 - k0 - 2 : 0;
    const uint32_t w_first = min((k0 + 1) * w_out, x1) - x0;
    const uint32_t w_last = k1 - k0 > 1 ? x1 - (k1 - 1) * w_out : 0;
    const uint32_t last = k1 - k0 - 1;                              // offset of the footprint's last pixel (0: w_last = 0)

    // rows: the same along the height, relative to the upper border of source row j_lo
    const uint32_t j_lo = floor_div((uint64_t)r0 * h_in, h_out, rem_y);
    const uint32_t n_src = (rem_y + th * h_in + h_out - 1) / h_out; // source rows j_lo .. j_lo + n_src - 1

    // staging geometry: `pieces` 16-byte pieces per row (head <= 15), `lpr` lanes per row (a power of two), `cpr` pieces
    // per lane and row (2 only when a row needs more than 64)
    const uint32_t pieces = (span + 30) / 16, pitch = pieces * 16;
    uint32_t lpr_shift = 0;
    while ((1u << lpr_shift) < pieces && lpr_shift < 6) ++lpr_shift;
    const uint32_t lpr = 1u << lpr_shift, cpr = (pieces + lpr - 1) >> lpr_shift, rows_per_pass = 64u >> lpr_shift;
    const uint32_t lane_row = lane >> lpr_shift, lane_piece = lane & (lpr - 1);
    const uint32_t chunk_rows = RESIZE_LDS_BYTES / pitch;
    const uint8_t *src0 = pages + pg.src + (uint64_t)j_lo * w_in + k_lo;     // first byte the tile needs

    const uint32_t den = 2u * h_in * w_in;                          // 2 * D < 2^32
    uint8_t *dst = out + pg.dst + (uint64_t)r0 * w_out + c0 + lane;
    uint32_t i = 0;                                                 // output row of the tile being accumulated
    uint32_t y_out = rem_y + h_in;                                  // its lower border
    uint32_t y_pos = rem_y;                                         // how far the walk has come
    uint64_t acc = 0;

    for (uint32_t first = 0; first < n_src; first += chunk_rows) {
        const uint32_t n_rows = min(chunk_rows, n_src - first);
        __syncthreads();                                            // the previous chunk has been read
        // RESIZE_BATCH loads in flight per lane and no branch between them: a lane with nothing of its own to load in
        // a pass takes the chunk's last row / the row's last piece again and stores the same bytes to the same place
        const uint32_t passes = ((n_rows + rows_per_pass - 1) / rows_per_pass) * cpr;
        for (uint32_t q0 = 0; q0 < passes; q0 += RESIZE_BATCH) {
            uint4 v[RESIZE_BATCH];
            uint32_t at[RESIZE_BATCH];
#pragma unroll
            for (int u = 0; u < RESIZE_BATCH; ++u) {
                const uint32_t q = min(q0 + u, passes - 1);
                const uint32_t rr = min((cpr == 2 ? q >> 1 : q) * rows_per_pass + lane_row, n_rows - 1);
                const uint8_t *a = src0 + (uint64_t)(first + rr) * w_in;
                const uint32_t head = (uint32_t)((uintptr_t)a & 15);
                const uint32_t piece = min(lane_piece + (cpr == 2 ? (q & 1) << 6 : 0), (head + span - 1) >> 4);
                v[u] = *(const uint4 *)(a - head + 16 * piece);
                at[u] = rr * pitch + 16 * piece;
            }
#pragma unroll
            for (int u = 0; u < RESIZE_BATCH; ++u) *(uint4 *)(rows + at[u]) = v[u];
        }
        __syncthreads();
        for (uint32_t rr = 0; rr < n_rows && i < th; ++rr) {
            const uint32_t head = (uint32_t)((uintptr_t)(src0 + (uint64_t)(first + rr) * w_in) & 15);
            const uint8_t *px = rows + rr * pitch + head + k0;
            uint32_t mid = 0;
            for (uint32_t m = 1; m <= n_mid; ++m) mid += px[m];
            const uint32_t hs = w_first * px[0] + w_out * mid + w_last * px[last];
            const uint32_t y_src = (first + rr + 1) * h_out;        // lower border of this source row
            for (;;) {
                const uint32_t y_next = min(y_src, y_out);
                acc += (uint64_t)(y_next - y_pos) * hs;
                y_pos = y_next;
                if (y_next == y_out) {                              // output row i is complete
                    if (lane < tw) dst[(uint64_t)i * w_out] = (uint8_t)small_quotient(2 * acc + (den >> 1), den);
                    acc = 0;
                    ++i;
                    y_out += h_in;
                }
                if (y_next == y_src || i == th) break;
            }
        }
    }
}

hipError_t launch_resize_pages(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                               const ResizePage *table, int n_pages, int64_t total_tiles) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_pages_kernel, dim3((unsigned)total_tiles), dim3(64), 0, s, pages, out, tile_first, table,
                       n_pages);
    return hipGetLastError();
}

}  // namespace asr
