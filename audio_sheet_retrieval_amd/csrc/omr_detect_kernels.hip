// gfx950 kernels of asr_notes_from_map_dev and asr_bars_from_map_dev: what sheet_utils/omr.py notes_from_map and
// bar_blobs_from_map do on the host after a probability map exists, for all pages of a call.  Built with
// floating-point contraction off (build.py; the pragma below says the same): the Otsu threshold of the bar map is the
// restatement of omr_post_shared.h, and the relative threshold of the peak search is one float64 product.
//
//   det_minmax_kernel     : page minimum, maximum and a NaN / infinity flag.  Workgroups reduce in float64 and combine
//                           through 64-bit integer atomics on an order-preserving key of the double.
//   det_peak_kernel       : peak_local_max in two dimensions.  One workgroup per DET_TILE_H x DET_TILE_W pixels: the
//                           tile and a halo of min_distance (zero beyond the page) in LDS, the row maximum over
//                           2 d + 1 columns, then the column maximum over 2 d + 1 rows of those; a pixel is a peak if
//                           it equals that maximum, lies at least d pixels off every border and is strictly above the
//                           threshold.  A constant page has none.
//   det_rowcount_kernel, det_rowscan_kernel, det_emit_kernel : flagged pixels (peaks; roots of the labelling) per row,
//                           their exclusive prefix over the page, and the ordered write: a pixel's rank in raster
//                           order is its row's prefix plus the flagged pixels to its left.  Peaks are written at
//                           count - 1 - rank (the host returns them in reversed raster order); a root's rank is its
//                           label - 1, kept in slot[root].  No sort anywhere.
//   det_edges_kernel, det_hist_kernel, det_otsu_kernel : threshold_otsu of the whole map.
//   det_fg_label_kernel   : map > t and the first labels, one wave per row: every foreground pixel points at the first
//                           pixel of its run.  The 8-connected equivalence is launch_post_label_pass.
//   det_stats_kernel      : area, bounding box and the raw sums of r, c, r*r, c*c, r*c per blob: lanes of a wave that
//                           share a root reduce among themselves, one lane issues the 64-bit integer atomics.
// Every index is bounded by the page geometry in PostPage; writes into coords / blobs are guarded by the capacity.
#pragma clang fp contract(off)
#include "omr_kernels.h"
#include "omr_post_shared.h"

namespace asr {

namespace {

struct OpAddLL { __device__ long long operator()(long long a, long long b) const { return a + b; } };

// doubles ordered as unsigned integers (negative values below positive ones)
__device__ __forceinline__ unsigned long long det_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

__device__ __forceinline__ double det_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k & 0x7fffffffffffffffull : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double det_page_min(const DetArgs &a, int p) { return det_unkey(~a.minmax[2 * p]); }
__device__ __forceinline__ double det_page_max(const DetArgs &a, int p) { return det_unkey(a.minmax[2 * p + 1]); }

__global__ __launch_bounds__(PT) void det_minmax_kernel(DetArgs a) {
    __shared__ double red[PT / 64];
    __shared__ int red_i[PT / 64];
    const int p = blockIdx.y, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i0 = (int64_t)blockIdx.x * PX_PER_BLOCK;
    if (i0 >= n) return;
    const double *map = a.maps + P.map_off;
    const int64_t i1 = i0 + PX_PER_BLOCK < n ? i0 + PX_PER_BLOCK : n;
    double mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (int64_t i = i0 + tid; i < i1; i += PT) {
        const double v = map[i];
        bad |= !isfinite(v);
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    mn = block_reduce(mn, OpMinD(), red);
    mx = block_reduce(mx, OpMaxD(), red);
    bad = block_reduce(bad, OpOrI(), red_i);
    if (tid == 0) {
        atomicMax(&a.minmax[2 * p], ~det_key(mn));
        atomicMax(&a.minmax[2 * p + 1], det_key(mx));
        if (bad) atomicOr(&a.state[p].nonfinite, 1);
    }
}

__global__ __launch_bounds__(PT) void det_status_kernel(DetArgs a) {
    const int p = blockIdx.x * PT + threadIdx.x;
    if (p < a.n_pages) a.state[p].status = a.state[p].nonfinite ? 3 : 0;
}

__global__ __launch_bounds__(PT) void det_peak_kernel(DetArgs a) {
    constexpr int LH = DET_TILE_H + 2 * DET_MAX_DISTANCE, LW = DET_TILE_W + 2 * DET_MAX_DISTANCE;
    __shared__ double tile[LH][LW];
    __shared__ double rmax[LH][DET_TILE_W];
    const int p = blockIdx.y, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    const int ntx = (a.max_w + DET_TILE_W - 1) / DET_TILE_W;   // the tiles of a page are the x dimension of the grid
    const int h = P.h, w = P.w, r0 = (int)(blockIdx.x / ntx) * DET_TILE_H, c0 = (int)(blockIdx.x % ntx) * DET_TILE_W;
    if (r0 >= h || c0 >= w || a.state[p].status) return;
    const int d = a.distance, rows = DET_TILE_H + 2 * d, cols = DET_TILE_W + 2 * d;
    const double *map = a.maps + P.map_off;
    const double mn = det_page_min(a, p), mx = det_page_max(a, p);
    double thr = a.threshold_abs != a.threshold_abs ? mn : a.threshold_abs;
    if (a.threshold_rel == a.threshold_rel) {
        const double t = a.threshold_rel * mx;
        thr = t > thr ? t : thr;
    }
    for (int i = tid; i < rows * cols; i += PT) {
        const int lr = i / cols, lc = i - lr * cols, r = r0 - d + lr, c = c0 - d + lc;
        tile[lr][lc] = r >= 0 && r < h && c >= 0 && c < w ? map[(int64_t)r * w + c] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < rows * DET_TILE_W; i += PT) {
        const int lr = i / DET_TILE_W, lc = i - lr * DET_TILE_W;
        double m = tile[lr][lc];
        for (int k = 1; k <= 2 * d; ++k) m = fmax(m, tile[lr][lc + k]);
        rmax[lr][lc] = m;
    }
    __syncthreads();
    uint8_t *mask = a.mask + P.px_off;
    for (int i = tid; i < DET_TILE_H * DET_TILE_W; i += PT) {
        const int lr = i / DET_TILE_W, lc = i - lr * DET_TILE_W, r = r0 + lr, c = c0 + lc;
        if (r >= h || c >= w) continue;
        double m = rmax[lr][lc];
        for (int k = 1; k <= 2 * d; ++k) m = fmax(m, rmax[lr + k][lc]);
        const double v = tile[lr + d][lc + d];
        const bool inner = r >= d && r < h - d && c >= d && c < w - d;
        mask[(int64_t)r * w + c] = mn != mx && inner && v == m && v > thr;
    }
}

// the pixels that are counted and written in raster order: peaks (the mask), or roots of the labelling
template <bool ROOTS>
__device__ __forceinline__ bool det_flag(const DetArgs &a, const PostPage &P, int r, int c) {
    const int64_t i = (int64_t)r * P.w + c;
    if (ROOTS) return a.label[P.px_off + i] == (int)i;
    return a.mask[P.px_off + i] != 0;
}

template <bool ROOTS>
__global__ __launch_bounds__(64) void det_rowcount_kernel(DetArgs a) {
    const int p = blockIdx.y, r = blockIdx.x, lane = threadIdx.x;
    const PostPage P = a.pages[p];
    if (r >= P.h || a.state[p].status) return;
    int cnt = 0;
    for (int c0 = 0; c0 < P.w; c0 += 64) {
        const int c = c0 + lane;
        const bool f = c < P.w && det_flag<ROOTS>(a, P, r, c);
        cnt += (int)__popcll(__ballot(f));
    }
    if (lane == 0) a.rowcnt[P.row_off + r] = cnt;
}

// exclusive prefix of the row counts of one page, in place; the total in state.n_kept
__global__ __launch_bounds__(PT) void det_rowscan_kernel(DetArgs a) {
    __shared__ int part[PT];
    const int p = blockIdx.x, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    if (a.state[p].status) return;
    int32_t *cnt = a.rowcnt + P.row_off;
    const int per = (P.h + PT - 1) / PT, lo = tid * per < P.h ? tid * per : P.h, hi = lo + per < P.h ? lo + per : P.h;
    int s = 0;
    for (int r = lo; r < hi; ++r) s += cnt[r];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < PT; ++i) {
            const int t = part[i];
            part[i] = run;
            run += t;
        }
        a.state[p].n_kept = (uint32_t)run;
    }
    __syncthreads();
    int run = part[tid];
    for (int r = lo; r < hi; ++r) {
        const int t = cnt[r];
        cnt[r] = run;
        run += t;
    }
}

template <bool ROOTS>
__global__ __launch_bounds__(64) void det_emit_kernel(DetArgs a) {
    const int p = blockIdx.y, r = blockIdx.x, lane = threadIdx.x;
    const PostPage P = a.pages[p];
    if (r >= P.h || a.state[p].status) return;
    const int64_t total = (int64_t)a.state[p].n_kept;
    int64_t base = a.rowcnt[P.row_off + r];
    for (int c0 = 0; c0 < P.w; c0 += 64) {
        const int c = c0 + lane;
        const bool f = c < P.w && det_flag<ROOTS>(a, P, r, c);
        const unsigned long long m = __ballot(f);
        if (f) {
            const int64_t k = base + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (ROOTS) {
                a.slot[P.px_off + (int64_t)r * P.w + c] = (int)k;
                if (k < a.cap) {
                    long long *B = a.blobs + ((size_t)p * a.cap + (size_t)k) * DET_BLOB_FIELDS;
                    B[0] = 0; B[1] = LLONG_MAX; B[2] = LLONG_MAX; B[3] = 0; B[4] = 0;
                    B[5] = 0; B[6] = 0; B[7] = 0; B[8] = 0; B[9] = 0;
                }
            } else {
                const int64_t pos = total - 1 - k;
                if (pos < a.cap) {
                    int32_t *o = a.coords + ((size_t)p * a.cap + (size_t)pos) * 2;
                    o[0] = r;
                    o[1] = c;
                }
            }
        }
        base += (int64_t)__popcll(m);
    }
}

__global__ __launch_bounds__(PT) void det_edges_kernel(DetArgs a) {
    __shared__ double e[257];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (a.state[p].status) return;
    const double mn = det_page_min(a, p), mx = det_page_max(a, p);
    for (int i = tid; i <= 256; i += PT) post_edge(mn, mx, i, e);
    __syncthreads();
    for (int i = tid; i <= 256; i += PT) a.edges[(size_t)p * 257 + i] = e[i];
    if (tid == 0) a.state[p].status = post_edges_ok(mn, mx, e) ? 0 : 3;
}

__global__ __launch_bounds__(PT) void det_hist_kernel(DetArgs a) {
    __shared__ double e[257];
    __shared__ unsigned hist[256];
    const int p = blockIdx.y, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i0 = (int64_t)blockIdx.x * PX_PER_BLOCK;
    if (i0 >= n || a.state[p].status) return;
    for (int i = tid; i <= 256; i += PT) e[i] = a.edges[(size_t)p * 257 + i];
    hist[tid] = 0;
    __syncthreads();
    const double *map = a.maps + P.map_off;
    const int64_t i1 = i0 + PX_PER_BLOCK < n ? i0 + PX_PER_BLOCK : n;
    for (int64_t i = i0 + tid; i < i1; i += PT) atomicAdd(&hist[post_bin(map[i], e)], 1u);
    __syncthreads();
    if (hist[tid]) atomicAdd(&a.hist[(size_t)p * 256 + tid], hist[tid]);
}

__global__ __launch_bounds__(64) void det_otsu_kernel(DetArgs a) {
    __shared__ double e[257], hc[256], m2[256], w2[256];
    __shared__ unsigned hist[256];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (a.state[p].status) return;
    for (int i = tid; i <= 256; i += 64) e[i] = a.edges[(size_t)p * 257 + i];
    for (int i = tid; i < 256; i += 64) hist[i] = a.hist[(size_t)p * 256 + i];
    __syncthreads();
    if (tid == 0) a.state[p].thr2 = post_otsu(hist, e, hc, m2, w2);
}

// one wave per row: map > t, and every foreground pixel gets the linear index of the first pixel of its run
__global__ __launch_bounds__(64) void det_fg_label_kernel(DetArgs a) {
    const int p = blockIdx.y, r = blockIdx.x, lane = threadIdx.x;
    const PostPage P = a.pages[p];
    if (r >= P.h || a.state[p].status) return;
    const int w = P.w;
    const double thr = a.state[p].thr2;
    const double *map = a.maps + P.map_off + (int64_t)r * w;
    int32_t *label = a.label + P.px_off + (int64_t)r * w;
    const int base = r * w;                   // h * w <= 2^28
    int carry = -1;                           // start of the run that reaches the chunk's left edge, or -1
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int c = c0 + lane;
        const bool e = c < w && map[c] > thr;
        const int start = post_run_start(e, c0, lane, carry);
        if (c < w) label[c] = e ? base + start : -1;
    }
}

__global__ __launch_bounds__(PT) void det_stats_kernel(DetArgs a) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    const bool in = i < n && !a.state[p].status;
    const int L = in ? a.label[P.px_off + i] : -1;
    int k = L >= 0 ? a.slot[P.px_off + L] : -1;
    if (k >= a.cap) k = -1;
    const int r = in ? (int)(i / P.w) : 0, c = in ? (int)(i - (int64_t)r * P.w) : 0;
    bool active = k >= 0;
    for (;;) {
        const unsigned long long todo = __ballot(active);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int kr = __shfl(k, leader);
        const bool same = active && k == kr;
        const long long cnt = (long long)__popcll(__ballot(same));
        const long long rr = same ? r : 0, cc = same ? c : 0;
        const int r_lo = wave_reduce(same ? r : INT_MAX, OpMinI()), r_hi = wave_reduce(same ? r : -1, OpMaxI());
        const int c_lo = wave_reduce(same ? c : INT_MAX, OpMinI()), c_hi = wave_reduce(same ? c : -1, OpMaxI());
        const long long s_r = wave_reduce(rr, OpAddLL()), s_c = wave_reduce(cc, OpAddLL());
        const long long s_rr = wave_reduce(rr * rr, OpAddLL()), s_cc = wave_reduce(cc * cc, OpAddLL());
        const long long s_rc = wave_reduce(rr * cc, OpAddLL());
        if (lane == leader) {
            long long *B = a.blobs + ((size_t)p * a.cap + (size_t)kr) * DET_BLOB_FIELDS;
            atomicAdd((unsigned long long *)&B[0], (unsigned long long)cnt);
            atomicMin(&B[1], (long long)r_lo);
            atomicMin(&B[2], (long long)c_lo);
            atomicMax(&B[3], (long long)r_hi + 1);
            atomicMax(&B[4], (long long)c_hi + 1);
            atomicAdd((unsigned long long *)&B[5], (unsigned long long)s_r);
            atomicAdd((unsigned long long *)&B[6], (unsigned long long)s_c);
            atomicAdd((unsigned long long *)&B[7], (unsigned long long)s_rr);
            atomicAdd((unsigned long long *)&B[8], (unsigned long long)s_cc);
            atomicAdd((unsigned long long *)&B[9], (unsigned long long)s_rc);
        }
        if (same) active = false;
    }
}

dim3 det_px_grid(const DetArgs &a, int per_block) {
    return dim3((unsigned)((a.max_px + per_block - 1) / per_block), (unsigned)a.n_pages);
}

}  // namespace

hipError_t launch_det_minmax(hipStream_t s, const DetArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(det_minmax_kernel, det_px_grid(a, PX_PER_BLOCK), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_status_kernel, dim3((a.n_pages + PT - 1) / PT), dim3(PT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_det_peaks(hipStream_t s, const DetArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    // (h * w <= 2^28 per page: at most 2^28 / 32 tiles in x)
    const dim3 tiles((unsigned)(((a.max_w + DET_TILE_W - 1) / DET_TILE_W) * ((a.max_h + DET_TILE_H - 1) / DET_TILE_H)),
                     (unsigned)a.n_pages);
    hipLaunchKernelGGL(det_peak_kernel, tiles, dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_rowcount_kernel<false>, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    hipLaunchKernelGGL(det_rowscan_kernel, dim3(a.n_pages), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_emit_kernel<false>, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_det_bar_threshold(hipStream_t s, const DetArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(det_edges_kernel, dim3(a.n_pages), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_hist_kernel, det_px_grid(a, PX_PER_BLOCK), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_otsu_kernel, dim3(a.n_pages), dim3(64), 0, s, a);
    hipLaunchKernelGGL(det_fg_label_kernel, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_det_bar_blobs(hipStream_t s, const DetArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(det_rowcount_kernel<true>, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    hipLaunchKernelGGL(det_rowscan_kernel, dim3(a.n_pages), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(det_emit_kernel<true>, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    hipLaunchKernelGGL(det_stats_kernel, det_px_grid(a, PT), dim3(PT), 0, s, a);
    return hipGetLastError();
}

}  // namespace asr
