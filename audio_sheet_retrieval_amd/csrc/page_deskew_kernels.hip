// Skew of scanned score pages (asr_skew_estimate_dev, asr_deskew_pages_dev; include/asr_hip.h carries the definition): the
// slope of the staves from projection profiles, and the correction by two shears.  All in integers, uint8 -> uint8.
//
//   skew_profiles_kernel : the profiles P_k of all slopes of all pages in one launch.  Every page is cut into tiles of
//                          SKEW_TILE_H rows x SKEW_TILE_W columns, the tiles of all pages are numbered through
//                          (tile_first, as resize_pages_kernel's) and one workgroup of SKEW_WAVES waves takes one tile.
//   skew_scores_kernel   : one workgroup per (page, slope): score = sum of P^2 in 64 bits.
//   skew_select_kernel   : one thread per page: the slope of largest score in the visiting order 0, -1, +1, -2, ...
//   deskew_pages_kernel  : both shears in one pass, one thread per output column of a tile of DESKEW_TILE_H rows.
//
// A tile's share of a profile.  The workgroup writes the running row sums of the tile's ink (255 - pixel) to LDS:
// S[row][i] = sum of the first i columns of the row inside the tile (a wave takes a row at a time, seven columns per
// lane, the lanes' totals scanned across the wave; rows below the page count as blank).  d_k(x) is monotone in x, so
// the columns of the tile with d_k(x) == d are one run [xa, xb), and the run's ink of a row is S[row][xb] - S[row][xa]:
// two LDS reads instead of one add per pixel.  The run borders - the first column with d_k(x) >= d - are one division
// each, done once per slope and tile, one border per lane, and handed round the wave with readlane;
// d_-k(x) = d_k(w - 1 - x), so a negative slope has the same borders with the tile mirrored.  Wave v takes the slopes
// |k| = v + 1, v + 1 + SKEW_WAVES, ...; for a slope the tile touches the profile rows y0 - dhi .. y0 + SKEW_TILE_H - 1 -
// dlo (dlo, dhi: d at the tile's first and last column), lane a owns row y0 - dhi + a and walks the runs d = dlo .. dhi
// in step with the other lanes - the run borders are uniform over the wave, the row it reads is a - (dhi - d) - and
// adds its sum to the page's profile with one atomic (none where the sum is 0).  Integer addition commutes, so the
// profiles do not depend on the order.  Sixteen waves share a tile's 57 KB of sums: two tiles per CU are 32 waves, and
// it is the waves in flight that cover the LDS round trips of the walk (4 waves per tile: 6.2 ms for 64 pages of
// 3508 x 2480 at max_slope 64, 8: 3.0 ms, 16: 2.4 ms).
#include "asr_kernels.h"

namespace asr {

__device__ __forceinline__ int skew_d(int k, int x, int w) { return (k * (2 * x - (w - 1)) + 1024) >> 11; }

// the first column x with d_k(x) >= d, k >= 1: ceil((2048 d - 1024 + k (w - 1)) / 2k), 0 where that is not positive.  The
// numerator stays below 2^23: the float quotient is off by one at most and is corrected with the exact remainder.
__device__ __forceinline__ int skew_first_column(int k, int d, int w) {
    const int num = 2048 * d - 1024 + k * (w - 1), den = 2 * k;
    if (num <= 0) return 0;
    const int up = num + den - 1;
    int q = (int)((float)up * __builtin_amdgcn_rcpf((float)den));
    int rem = up - q * den;
    if (rem < 0) { --q; rem += den; }
    if (rem >= den) ++q;
    return q;
}

// last p with tile_first[p] <= g
__device__ __forceinline__ int page_of_tile(const int64_t *__restrict__ tile_first, int n_pages, int64_t g) {
    int lo = 0, hi = n_pages - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(64 * SKEW_WAVES) void skew_profiles_kernel(const uint8_t *__restrict__ pages,
                                                            const int64_t *__restrict__ tile_first,
                                                            const SkewPage *__restrict__ table, int n_pages,
                                                            int max_slope, uint32_t *__restrict__ prof) {
    static_assert(SKEW_MAX_SLOPE * (SKEW_TILE_W - 1) / 1024 + 3 <= 64, "a slope's run borders of a tile: one per lane");
    __shared__ uint32_t S[SKEW_TILE_H][SKEW_TILE_W + 1];
    const int64_t g = blockIdx.x;
    const int pi = page_of_tile(tile_first, n_pages, g);
    const SkewPage pg = table[pi];
    const int h = pg.h, w = pg.w, len = pg.len, dm = pg.dm;
    const int t = (int)(g - tile_first[pi]);
    const int y0 = (t / pg.tiles_x) * SKEW_TILE_H, c0 = (t % pg.tiles_x) * SKEW_TILE_W;
    const int rh = min(SKEW_TILE_H, h - y0), cw = min(SKEW_TILE_W, w - c0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // lane l takes the columns l * PER .. l * PER + PER - 1 of a row: running sums in registers, one scan of the lanes'
    // totals across the wave, PER stores (PER is odd: the lanes' words lie in different banks)
    constexpr int PER = SKEW_TILE_W / 64;
    for (int row = wave; row < SKEW_TILE_H; row += SKEW_WAVES) {
        const uint8_t *src = pages + pg.src + (int64_t)(y0 + row) * w + c0;
        uint32_t v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = lane * PER + j;
            v[j] = (row < rh && c < cw) ? 255u - src[c] : 0u;
        }
#pragma unroll
        for (int j = 1; j < PER; ++j) v[j] += v[j - 1];
        uint32_t x = v[PER - 1];                                    // inclusive scan of the lanes' totals
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t below = __shfl_up(x, off, 64);
            if (lane >= off) x += below;
        }
        const uint32_t before = x - v[PER - 1];
        if (lane == 0) S[row][0] = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) S[row][lane * PER + j + 1] = before + v[j];
    }
    __syncthreads();

    uint32_t *P = prof + pg.prof;
    if (wave == SKEW_WAVES - 1 && lane < SKEW_TILE_H) {             // slope 0: the rows' sums
        const uint32_t sum = S[lane][cw];
        const int idx = y0 + lane + dm;
        if (sum && idx < len) atomicAdd(&P[(int64_t)max_slope * len + idx], sum);
    }
    for (int k = 1 + wave; k <= max_slope; k += SKEW_WAVES) {
        for (int sign = 0; sign < 2; ++sign) {                      // +k: the tile's columns; -k: mirrored, w - 1 - x
            const int m0 = sign ? w - (c0 + cw) : c0, m1 = m0 + cw;
            const int dlo = skew_d(k, m0, w), dhi = skew_d(k, m1 - 1, w);
            const int win = SKEW_TILE_H + dhi - dlo;                // profile rows the tile touches
            // lane j: the border between the runs dlo + j - 1 and dlo + j as a column of the tile, 0 .. cw
            // (dhi - dlo + 2 borders: at most SKEW_MAX_SLOPE * (SKEW_TILE_W - 1) / 1024 + 3 <= 64)
            const int border = min(max(skew_first_column(k, dlo + lane, w), m0), m1) - m0;
            const int col = sign ? cw - border : border;
            uint32_t *Pk = P + (int64_t)(sign ? max_slope - k : max_slope + k) * len;
            for (int a0 = 0; a0 < win; a0 += 64) {
                const int a = a0 + lane;
                uint32_t sum = 0;
                const int d_first = max(dlo, dhi - (a0 + 63)), d_last = min(dhi, dhi - a0 + SKEW_TILE_H - 1);
#pragma unroll 4
                for (int d = d_first; d <= d_last; ++d) {
                    const int from = __builtin_amdgcn_readlane(col, d - dlo);
                    const int to = __builtin_amdgcn_readlane(col, d - dlo + 1);
                    const int row = a - (dhi - d);
                    const uint32_t *Sr = S[min(max(row, 0), SKEW_TILE_H - 1)];       // read in any case, use in range
                    const uint32_t ink = Sr[to] - Sr[from];
                    sum += (unsigned)row < (unsigned)SKEW_TILE_H ? ink : 0u;
                }
                if (sign) sum = 0u - sum;                           // mirrored: the run is [to, from)
                const int idx = y0 + a - dhi + dm;                  // profile row y0 + a - dhi
                if (sum && (unsigned)idx < (unsigned)len) atomicAdd(&Pk[idx], sum);
            }
        }
    }
}

__global__ __launch_bounds__(256) void skew_scores_kernel(const SkewPage *__restrict__ table, int max_slope,
                                                          const uint32_t *__restrict__ prof, int64_t *__restrict__ scores) {
    __shared__ uint64_t part[256];
    const int n_slopes = 2 * max_slope + 1;
    const int p = blockIdx.x / n_slopes, j = blockIdx.x % n_slopes;
    const int len = table[p].len;
    const uint32_t *P = prof + table[p].prof + (int64_t)j * len;
    uint64_t s = 0;
    for (int i = threadIdx.x; i < len; i += 256) {
        const uint64_t v = P[i];
        s += v * v;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) scores[blockIdx.x] = (int64_t)part[0];
}

__global__ __launch_bounds__(64) void skew_select_kernel(int n_pages, int max_slope, const int64_t *__restrict__ scores,
                                                         int32_t *__restrict__ slopes) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pages) return;
    const int64_t *sc = scores + (int64_t)p * (2 * max_slope + 1) + max_slope;
    int best = 0;
    int64_t top = sc[0];
    for (int m = 1; m <= max_slope; ++m) {
        if (sc[-m] > top) { top = sc[-m]; best = -m; }
        if (sc[m] > top) { top = sc[m]; best = m; }
    }
    slopes[p] = best;
}

// pixel (y, xx) of the vertical pass
__device__ __forceinline__ int sheared_down(const uint8_t *__restrict__ src, int h, int w, int k, int fill, int y,
                                            int xx) {
    if ((unsigned)xx >= (unsigned)w) return fill;
    const int t = k * (2 * xx - (w - 1)), q = t >> 11, f = t - (q << 11), r = y + q;
    const int i0 = (unsigned)r < (unsigned)h ? src[(int64_t)r * w + xx] : fill;
    const int i1 = (unsigned)(r + 1) < (unsigned)h ? src[(int64_t)(r + 1) * w + xx] : fill;
    return ((2048 - f) * i0 + f * i1 + 1024) >> 11;
}

__global__ __launch_bounds__(256) void deskew_pages_kernel(const uint8_t *__restrict__ pages, uint8_t *__restrict__ out,
                                                           const int64_t *__restrict__ tile_first,
                                                           const DeskewPage *__restrict__ table, int n_pages, int fill) {
    const int64_t g = blockIdx.x;
    const int pi = page_of_tile(tile_first, n_pages, g);
    const DeskewPage pg = table[pi];
    const int h = pg.h, w = pg.w, k = pg.k;
    const int t = (int)(g - tile_first[pi]);
    const int y0 = (t / pg.tiles_x) * DESKEW_TILE_H, x = (t % pg.tiles_x) * DESKEW_TILE_W + (int)threadIdx.x;
    if (x >= w) return;
    const uint8_t *src = pages + pg.off;
    uint8_t *dst = out + pg.off;
    const int y1 = min(y0 + DESKEW_TILE_H, h);
    for (int y = y0; y < y1; ++y) {
        const int u = -k * (2 * y - (h - 1)), p = u >> 11, gq = u - (p << 11);
        const int a0 = sheared_down(src, h, w, k, fill, y, x + p), a1 = sheared_down(src, h, w, k, fill, y, x + p + 1);
        dst[(int64_t)y * w + x] = (uint8_t)(((2048 - gq) * a0 + gq * a1 + 1024) >> 11);
    }
}

hipError_t launch_skew_profiles(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const SkewPage *table,
                                int n_pages, int64_t total_tiles, int max_slope, uint32_t *prof) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(skew_profiles_kernel, dim3((unsigned)total_tiles), dim3(64 * SKEW_WAVES), 0, s, pages, tile_first,
                       table, n_pages, max_slope, prof);
    return hipGetLastError();
}

hipError_t launch_skew_scores(hipStream_t s, const SkewPage *table, int n_pages, int max_slope, const uint32_t *prof,
                              int64_t *scores, int32_t *slopes) {
    if (n_pages == 0) return hipSuccess;
    const int64_t blocks = (int64_t)n_pages * (2 * max_slope + 1);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(skew_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, s, table, max_slope, prof, scores);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(skew_select_kernel, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, s, n_pages, max_slope,
                       scores, slopes);
    return hipGetLastError();
}

hipError_t launch_deskew_pages(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                               const DeskewPage *table, int n_pages, int64_t total_tiles, int fill) {
    if (total_tiles == 0 || n_pages == 0) return hipSuccess;
    if (total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deskew_pages_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, pages, out, tile_first, table,
                       n_pages, fill);
    return hipGetLastError();
}

}  // namespace asr
