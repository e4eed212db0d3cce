// Paper of scanned score pages (asr_flatten_pages_dev; include/asr_hip.h carries the definition): the grey closing B of a
// page by a (2r + 1)-square and the page divided by it.  All in integers, uint8 -> uint8.
//
//   flatten_pass_kernel<false> : dilate.  D over the page's r-neighbourhood, (H + 2r) x (W + 2r), into workspace.
//   flatten_pass_kernel<true>  : erode and divide.  B = the sliding minimum of D, out = 255 * P / B where B >= floor.
//
// Both are the same sliding extremum.  With the page padded by 2r absent pixels on every side (index a = y + 2r) and D kept
// at index i = y' + r, either pass is  out[i][j] = ext { src[i + dy][j + dx] : 0 <= dy, dx <= 2r }:  a tile of FLATTEN_TILE
// x FLATTEN_TILE results reads the source rows and columns i0 .. i0 + FLATTEN_TILE + 2r - 1, which one workgroup stages in
// LDS as bytes (absent pixels as the extremum's neutral value, 0 or 255).  The tiles of all pages are numbered through
// (tile_first, as resize_pages_kernel's), so a pass is one launch whatever the number of pages.
//
// The sliding extremum is van Herk / Gil-Werman, rows first, then columns: a line is cut into blocks of w = 2r + 1, h[x]
// is the extremum from x to the end of its block, g[x] from the start of its block to x, and the window [x, x + 2r] is
// ext(h[x], g[x + 2r]) - about three comparisons per pixel at any r.  One thread takes one (line, block): it walks the
// block backwards and stores h where a result is due (the first FLATTEN_TILE positions of a line), then, after a barrier,
// walks it forwards with g in a register and folds g into the stored h of position x - 2r, which no other thread touches.
// g is never stored, the staged source is only read, and the columns' h reuse the source's LDS once the rows are done.
// In the row pass a wave's lanes are consecutive rows at one column: the pitches are 4 * odd bytes, so 32 rows lie in
// 32 banks.  In the column pass the lanes are consecutive columns: adjacent bytes.
// At r = 127 a tile's source is 318 x 324 bytes and the rows' result 318 x 68: 122 KiB of the 160.
#include "asr_kernels.h"

namespace asr {

namespace {

// last p with tile_first[p] <= g
__device__ __forceinline__ int flatten_page_of_tile(const int64_t *__restrict__ tile_first, int n_pages, int64_t g) {
    int lo = 0, hi = n_pages - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__host__ __device__ inline int flatten_pitch(int n) { return 4 * (((n + 3) >> 2) | 1); }

template <bool MIN>
__device__ __forceinline__ int flatten_ext(int a, int b) { return MIN ? min(a, b) : max(a, b); }

template <bool ERODE>
__global__ __launch_bounds__(FLATTEN_THREADS) void flatten_pass_kernel(const uint8_t *__restrict__ pages,
                                                                      uint8_t *__restrict__ dws,
                                                                      const int64_t *__restrict__ tile_first,
                                                                      const FlattenPage *__restrict__ table, int n_pages,
                                                                      int floor_, uint8_t *__restrict__ out,
                                                                      uint8_t *__restrict__ background) {
    extern __shared__ __attribute__((aligned(16))) uint8_t flatten_lds[];
    constexpr int T = FLATTEN_TILE, NEUTRAL = ERODE ? 255 : 0;
    const int64_t gt = blockIdx.x;
    const int pi = flatten_page_of_tile(tile_first, n_pages, gt);
    const FlattenPage pg = table[pi];
    const int h = pg.h, w = pg.w, r = pg.r, r2 = 2 * r, win = r2 + 1;
    const int dh = h + r2, dw = w + r2;                             // D
    const int out_h = ERODE ? h : dh, out_w = ERODE ? w : dw;
    const int tiles_x = ERODE ? pg.tiles_x_p : pg.tiles_x_d;
    const int t = (int)(gt - tile_first[pi]);
    const int i0 = (t / tiles_x) * T, j0 = (t % tiles_x) * T;
    const int S = T + r2;                                           // source rows and columns of the tile
    const int pin = flatten_pitch(S), pmid = flatten_pitch(T);
    uint8_t *in = flatten_lds, *mid = flatten_lds + S * pin, *hc = flatten_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // stage the source: a row per wave at a time
    const uint8_t *page = pages + pg.off;
    const uint8_t *D = dws + pg.d;
    for (int sy = wave; sy < S; sy += FLATTEN_THREADS / 64) {
        const int a = i0 + sy;
        for (int sx = lane; sx < S; sx += 64) {
            const int b = j0 + sx;
            int v = NEUTRAL;
            if (ERODE) {
                if (a < dh && b < dw) v = D[(int64_t)a * dw + b];
            } else {
                const int y = a - r2, x = b - r2;
                if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) v = page[(int64_t)y * w + x];
            }
            in[sy * pin + sx] = (uint8_t)v;
        }
    }
    __syncthreads();

    // rows: mid[row][j] = ext in[row][j .. j + 2r], j < T
    const int nb = (S + win - 1) / win, row_items = S * nb;
    for (int it = tid; it < row_items; it += FLATTEN_THREADS) {
        const int k = it / S, row = it - k * S, x0 = k * win;
        if (x0 >= T) continue;
        const uint8_t *src = in + row * pin;
        uint8_t *dst = mid + row * pmid;
        int s = NEUTRAL;
        for (int x = min(x0 + win, S) - 1; x >= x0; --x) {
            s = flatten_ext<ERODE>(s, src[x]);
            if (x < T) dst[x] = (uint8_t)s;
        }
    }
    __syncthreads();
    for (int it = tid; it < row_items; it += FLATTEN_THREADS) {
        const int k = it / S, row = it - k * S, x0 = k * win, x1 = min(x0 + win, S);
        const uint8_t *src = in + row * pin;
        uint8_t *dst = mid + row * pmid;
        int g = NEUTRAL;
        for (int x = x0; x < x1; ++x) {
            g = flatten_ext<ERODE>(g, src[x]);
            const int j = x - r2;                                   // < T, as x < S
            if (j >= 0) dst[j] = (uint8_t)flatten_ext<ERODE>(dst[j], g);
        }
    }
    __syncthreads();

    // columns: result[i][j] = ext mid[i .. i + 2r][j], i < T; the h of the columns goes where the source was
    const int col_items = nb * T;
    for (int it = tid; it < col_items; it += FLATTEN_THREADS) {
        const int k = it / T, j = it - k * T, y0 = k * win;
        if (y0 >= T) continue;
        int s = NEUTRAL;
        for (int y = min(y0 + win, S) - 1; y >= y0; --y) {
            s = flatten_ext<ERODE>(s, mid[y * pmid + j]);
            if (y < T) hc[y * pmid + j] = (uint8_t)s;
        }
    }
    __syncthreads();
    const int lowest = max(floor_, 1);
    for (int it = tid; it < col_items; it += FLATTEN_THREADS) {
        const int k = it / T, j = it - k * T, y0 = k * win, y1 = min(y0 + win, S);
        const int gj = j0 + j;
        if (gj >= out_w) continue;
        int g = NEUTRAL;
        for (int y = y0; y < y1; ++y) {
            g = flatten_ext<ERODE>(g, mid[y * pmid + j]);
            const int i = y - r2, gi = i0 + i;                      // i < T, as y < S
            if (i < 0 || gi >= out_h) continue;
            const int v = flatten_ext<ERODE>(hc[i * pmid + j], g);
            const int64_t at = (int64_t)gi * out_w + gj;
            if (ERODE) {
                const uint32_t P = page[at], B = (uint32_t)v;
                out[pg.off + at] = (uint8_t)((int)B >= lowest ? (510u * P + B) / (2u * B) : P);
                if (background) background[pg.off + at] = (uint8_t)B;
            } else {
                dws[pg.d + at] = (uint8_t)v;
            }
        }
    }
}

template <bool ERODE>
hipError_t flatten_launch(hipStream_t s, const uint8_t *pages, uint8_t *dws, const int64_t *tile_first,
                          const FlattenPage *table, int n_pages, int64_t total_tiles, int max_radius, int floor_,
                          uint8_t *out, uint8_t *background) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL || max_radius < 1 || max_radius > FLATTEN_MAX_RADIUS) return hipErrorInvalidValue;
    const size_t bytes = flatten_lds_bytes(max_radius);
    if (bytes > 65536) {                                            // above the default dynamic-LDS limit (gfx950: 160 KiB)
        hipError_t e = hipFuncSetAttribute((const void *)flatten_pass_kernel<ERODE>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    flatten_pass_kernel<ERODE><<<dim3((unsigned)total_tiles), dim3(FLATTEN_THREADS), bytes, s>>>(
        pages, dws, tile_first, table, n_pages, floor_, out, background);
    return hipGetLastError();
}

}  // namespace

size_t flatten_lds_bytes(int radius) {
    const int S = FLATTEN_TILE + 2 * radius;
    return (size_t)S * (flatten_pitch(S) + flatten_pitch(FLATTEN_TILE));
}

hipError_t launch_flatten_dilate(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const FlattenPage *table,
                                 int n_pages, int64_t total_tiles, int max_radius, uint8_t *dws) {
    return flatten_launch<false>(s, pages, dws, tile_first, table, n_pages, total_tiles, max_radius, 0, nullptr, nullptr);
}

hipError_t launch_flatten_erode(hipStream_t s, const uint8_t *pages, const uint8_t *dws, const int64_t *tile_first,
                                const FlattenPage *table, int n_pages, int64_t total_tiles, int max_radius, int floor_,
                                uint8_t *out, uint8_t *background) {
    return flatten_launch<true>(s, pages, const_cast<uint8_t *>(dws), tile_first, table, n_pages, total_tiles, max_radius,
                                floor_, out, background);
}

}  // namespace asr
