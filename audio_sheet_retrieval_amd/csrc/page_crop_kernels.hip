// Scanner borders of scanned score pages (asr_crop_estimate_dev, asr_crop_pages_dev; include/asr_hip.h carries the
// definition): the paper's rectangle from counts of dark pixels, and its copy.  All in integers, uint8 -> uint8.
//
//   crop_counts_kernel : the row counts and the column counts of all pages in one launch.  Every page is cut into tiles of
//                        CROP_TILE_H rows x CROP_TILE_W columns, the tiles of all pages are numbered through (tile_first,
//                        as resize_pages_kernel's) and one workgroup of four waves takes one tile.  Wave v takes the 256
//                        columns x0 + 256 v .. of every row of the tile and lane l four of them: one 4-byte load per
//                        lane, 256 contiguous bytes per wave, at whatever alignment the row has (a lane whose four
//                        columns cross the row's end loads the row's last four bytes instead), four rows in flight
//                        (with sixteen, 64 pages of 3508 x 2480 took 0.33 ms instead of 0.20 ms).
//                        A row is counted over the central band of the columns and a column over the central band of
//                        the rows, so a lane reads only where one of the two bands is - the four corner sixteenths of a
//                        page are never touched.
//                        Row count: the dark flags of the lanes' j-th columns are one ballot word, the wave's share of
//                        the row's count is four population counts; the four waves' shares meet in LDS.
//                        Column count: a lane sums its four columns over the tile's rows in registers.
//                        The tile's shares are then added to the counts with one atomic per row and per column, 64
//                        neighbouring counts per wave.  The counts are int32 in zeroed workspace and integer addition
//                        commutes: the order of the atomics does not show in the result.
//   crop_rects_kernel  : one workgroup of four waves per page, a wave per side (top, bottom, left, right).  A wave walks
//                        its counts from its edge, 64 at a time; the ballot of "not a border" ends the walk and its lowest
//                        bit is the run's length.  Thread 0 then applies the rule: margin, undecided, rect, status.
//   crop_copy_kernel   : the rects of all pages in one launch, one workgroup per CROP_COPY_ROWS rows of a rect, a wave per
//                        row.  Source and destination rows start at any byte: the destination's first bytes up to its
//                        4-byte boundary and its last bytes go one per lane, the words between as aligned 4-byte stores
//                        of 4-byte loads at the source's alignment.
//
// No scratch memory, no floating point.
#include "asr_kernels.h"

namespace asr {

namespace {

// last p with tile_first[p] <= g
__device__ __forceinline__ int crop_page_of_tile(const int64_t *__restrict__ tile_first, int n_pages, int64_t g) {
    int lo = 0, hi = n_pages - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(CROP_THREADS) void crop_counts_kernel(const uint8_t *__restrict__ pages,
                                                                   const int64_t *__restrict__ tile_first,
                                                                   const CropPage *__restrict__ table, int n_pages,
                                                                   int floor_, int32_t *__restrict__ row_counts,
                                                                   int32_t *__restrict__ col_counts) {
    constexpr int WAVES = CROP_THREADS / 64, WAVE_W = 4 * 64;       // four columns per lane
    static_assert(CROP_TILE_W == WAVES * WAVE_W && CROP_TILE_H <= CROP_THREADS, "a wave per 256 columns; a thread per row sum");
    __shared__ int row_part[WAVES][CROP_TILE_H];
    __shared__ int col_part[CROP_TILE_W];
    const int64_t g = blockIdx.x;
    const int pi = crop_page_of_tile(tile_first, n_pages, g);
    const CropPage pg = table[pi];
    const int h = pg.h, w = pg.w;
    const int t = (int)(g - tile_first[pi]);
    const int y0 = (t / pg.tiles_x) * CROP_TILE_H, x0 = (t % pg.tiles_x) * CROP_TILE_W;
    const int y1 = min(y0 + CROP_TILE_H, h), x1 = min(x0 + CROP_TILE_W, w);
    const int cb0 = w / 4, cb1 = w - w / 4, rb0 = h / 4, rb1 = h - h / 4;
    const bool tile_cols = x0 < cb1 && x1 > cb0;                    // the tile meets the column band: its rows count
    const bool tile_rows = y0 < rb1 && y1 > rb0;                    // ... the row band: its columns count
    if (!tile_cols && !tile_rows) return;                           // a corner of the page (the whole workgroup)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xw = x0 + wave * WAVE_W, c = xw + 4 * lane;
    const bool wave_cols = xw < cb1 && xw + WAVE_W > cb0 && xw < w;
    const bool lane_cols = c < cb1 && c + 4 > cb0;
    bool banded[4];                                                 // column c + j lies in the column band
#pragma unroll
    for (int j = 0; j < 4; ++j) banded[j] = c + j >= cb0 && c + j < cb1;
    const uint8_t *src = pages + pg.off;
    // a lane whose four columns cross the row's end loads the row's last four bytes and shifts its own down: cl is the
    // column it loads at and sh the shift; the bytes beyond the row become 255.  (A page of fewer than four columns is
    // read byte by byte.)
    const bool narrow = w < 4;
    const int cl = narrow ? c : min(c, w - 4), sh = 8 * (c - cl);
    const uint32_t beyond = sh ? ~(0xffffffffu >> sh) : 0u;
    int cnt[4] = {0, 0, 0, 0};
    constexpr int AHEAD = 4;                                        // rows whose loads are in flight together: 1 KB a wave
    static_assert(CROP_TILE_H % AHEAD == 0, "whole groups of rows");
    for (int ya = y0; ya < y1; ya += AHEAD) {
        uint32_t v[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            const int y = ya + a;
            v[a] = 0xffffffffu;                                     // an absent byte is 255: dark at no floor
            if (y < y1 && ((y >= rb0 && y < rb1) || lane_cols) && c < w) {
                const uint8_t *p = src + (int64_t)y * w + cl;
                if (!narrow) {
                    uint32_t raw;
                    __builtin_memcpy(&raw, p, 4);
                    v[a] = (raw >> sh) | beyond;
                } else {                                            // c = 0: 1 .. 3 bytes
                    v[a] = 0xffffff00u | p[0];
                    if (w > 1) v[a] = (v[a] & 0xffff00ffu) | ((uint32_t)p[1] << 8);
                    if (w > 2) v[a] = (v[a] & 0xff00ffffu) | ((uint32_t)p[2] << 16);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            const int y = ya + a;
            if (y >= y1) break;
            const bool in_rows = y >= rb0 && y < rb1;
            int in_row = 0;
            if (in_rows || wave_cols) {                             // (uniform over the wave)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool dark = (int)((v[a] >> (8 * j)) & 0xffu) < floor_;
                    cnt[j] += dark && in_rows ? 1 : 0;
                    in_row += __builtin_popcountll(__builtin_amdgcn_ballot_w64(dark && banded[j]));
                }
            }
            if (lane == 0) row_part[wave][y - y0] = in_row;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) col_part[wave * WAVE_W + 4 * lane + j] = cnt[j];
    __syncthreads();
    // the tile's shares, one atomic per row and per column, 64 neighbouring counts per wave
    const int r = (int)threadIdx.x;
    if (r < y1 - y0) {
        int total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) total += row_part[v][r];
        if (total) atomicAdd(&row_counts[pg.row_at + y0 + r], total);
    }
#pragma unroll
    for (int i = 0; i < CROP_TILE_W / CROP_THREADS; ++i) {
        const int col = x0 + i * CROP_THREADS + (int)threadIdx.x;
        const int total = col_part[i * CROP_THREADS + threadIdx.x];
        if (col < w && total) atomicAdd(&col_counts[pg.col_at + col], total);
    }
}

__global__ __launch_bounds__(256) void crop_rects_kernel(const CropPage *__restrict__ table, int share,
                                                         const int32_t *__restrict__ row_counts,
                                                         const int32_t *__restrict__ col_counts,
                                                         int32_t *__restrict__ rects, int32_t *__restrict__ status) {
    __shared__ int run[4];
    const CropPage pg = table[blockIdx.x];
    const int h = pg.h, w = pg.w;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool rows = wave < 2, from_end = (wave & 1) != 0;         // top, bottom, left, right
    const int n = rows ? h : w, band = rows ? w - w / 4 - w / 4 : h - h / 4 - h / 4;
    const int32_t *cnt = rows ? row_counts + pg.row_at : col_counts + pg.col_at;
    const int limit = share * band;                                 // at most 2^24
    int len = n;                                                    // no index stops the run: the whole axis
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool stop = i < n && 1024 * cnt[from_end ? n - 1 - i : i] < limit;
        const unsigned long long found = __ballot(stop);
        if (found != 0ull) {
            len = base + __builtin_ctzll(found);
            break;
        }
    }
    if (lane == 0) run[wave] = len;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int64_t top = run[0], bottom = run[1], left = run[2], right = run[3], m = pg.margin;
    int64_t r0 = top + (top ? m : 0), r1 = h - bottom - (bottom ? m : 0);
    int64_t c0 = left + (left ? m : 0), c1 = w - right - (right ? m : 0);
    const bool undecided = top + bottom >= h || left + right >= w || r1 - r0 < 1 || c1 - c0 < 1;
    if (undecided) { r0 = 0; r1 = h; c0 = 0; c1 = w; }
    int32_t *r = rects + 4 * (int64_t)blockIdx.x;
    r[0] = (int32_t)r0; r[1] = (int32_t)r1; r[2] = (int32_t)c0; r[3] = (int32_t)c1;
    status[blockIdx.x] = undecided ? 1 : 0;
}

__global__ __launch_bounds__(CROP_THREADS) void crop_copy_kernel(const uint8_t *__restrict__ pages,
                                                                 uint8_t *__restrict__ out,
                                                                 const int64_t *__restrict__ tile_first,
                                                                 const CropCopy *__restrict__ table, int n_pages) {
    constexpr int WAVES = CROP_THREADS / 64;
    const int64_t g = blockIdx.x;
    const int pi = crop_page_of_tile(tile_first, n_pages, g);
    const CropCopy cp = table[pi];
    const int y0 = (int)(g - tile_first[pi]) * CROP_COPY_ROWS, y1 = min(y0 + CROP_COPY_ROWS, cp.h);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int y = y0 + wave; y < y1; y += WAVES) {
        const uint8_t *s = pages + cp.src + (int64_t)y * cp.stride;
        uint8_t *d = out + cp.dst + (int64_t)y * cp.w;
        const int head = min((int)((4u - (unsigned)((uintptr_t)d & 3u)) & 3u), cp.w);   // bytes before d's 4-byte boundary
        const int words = (cp.w - head) >> 2, tail = cp.w - head - 4 * words;
        if (lane < head) d[lane] = s[lane];
        const uint8_t *sw = s + head;
        uint32_t *dw = (uint32_t *)(d + head);
#pragma unroll 4
        for (int k = lane; k < words; k += 64) {
            uint32_t v;
            __builtin_memcpy(&v, sw + 4 * k, 4);
            dw[k] = v;
        }
        if (lane < tail) d[head + 4 * words + lane] = s[head + 4 * words + lane];
    }
}

}  // namespace

hipError_t launch_crop_counts(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const CropPage *table,
                              int n_pages, int64_t total_tiles, int floor_, int32_t *row_counts, int32_t *col_counts) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_counts_kernel, dim3((unsigned)total_tiles), dim3(CROP_THREADS), 0, s, pages, tile_first, table,
                       n_pages, floor_, row_counts, col_counts);
    return hipGetLastError();
}

hipError_t launch_crop_rects(hipStream_t s, const CropPage *table, int n_pages, int share, const int32_t *row_counts,
                             const int32_t *col_counts, int32_t *rects, int32_t *status) {
    if (n_pages == 0) return hipSuccess;
    hipLaunchKernelGGL(crop_rects_kernel, dim3((unsigned)n_pages), dim3(256), 0, s, table, share, row_counts, col_counts,
                       rects, status);
    return hipGetLastError();
}

hipError_t launch_crop_copy(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                            const CropCopy *table, int n_pages, int64_t total_tiles) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_copy_kernel, dim3((unsigned)total_tiles), dim3(CROP_THREADS), 0, s, pages, out, tile_first,
                       table, n_pages);
    return hipGetLastError();
}

}  // namespace asr
