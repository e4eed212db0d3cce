// gfx950 kernels of asr_systems_from_maps_dev: what sheet_utils/omr.py systems_from_maps does on the host after the two
// probability maps exist, restated so that every comparison sees the bits numpy sees.  This translation unit is built
// with floating-point contraction off (build.py; the pragma below says the same): one fused multiply-add moves a bin
// edge.
//
//   post_rows_kernel      : one wave per page row.  projection = maps.sum(1) in numpy's pairwise order (the leaves of
//                           the row - at most 128 elements each - eight lanes per leaf, one lane per interleaved
//                           accumulator, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder sequentially;
//                           lane 0 then adds the leaf sums in the order of the recursion, which the host uploads as a
//                           postfix program).  The same order in float32 gives imagey.mean(axis=1) of the snap, which
//                           depends on the page only.  Row extrema of the system map and a NaN / infinity flag.
//   post_otsu1_kernel     : one workgroup per page.  np.histogram + threshold_otsu of the projection, the gap clean-up
//                           run loop (sequential, as the host's), extrema and bin edges of the cleaned system map.
//   post_hist2_kernel     : np.histogram of the cleaned system map, LDS counters flushed with integer atomics.
//   post_otsu2_kernel     : threshold_otsu of that histogram.
//   post_fg_kernel, post_dilate_kernel, post_erode_label_kernel : map > t, the 15x1 closing with OpenCV's border rule,
//                           and the initial labels: every foreground pixel points at the first pixel of its row run.
//   post_scan_kernel, post_flatten_kernel : 8-connected label equivalence.  scan links the root of a pixel to the
//                           smallest neighbouring label (atomicMin), flatten makes every pixel point at its root.
//                           Labels only ever decrease towards the smallest linear index of the component; the host
//                           repeats the pair until a scan changes nothing.  Kernel boundaries are the only
//                           synchronisation.
//   post_area_kernel, post_keep_kernel, post_sort_kernel, post_bbox_kernel : area per root (wave-aggregated integer
//                           atomics), the roots of at least POST_MIN_AREA pixels sorted by index (= the host's raster
//                           order of labels), their bounding boxes.
//   post_blob_kernel      : one workgroup per kept blob: shrink_bounding_box on label == root and snap_system_to_grid
//                           (peak_local_max in one dimension, argmin ties to the larger coordinate, the x-direction's
//                           comparison against max_row).  Whatever the host would answer with an IndexError from the
//                           shrink loops or could not be restated exactly is reported as status 3, never guessed.
// numpy version: the uniform-bin index of np.histogram is restated as numpy 2.x computes it, ((x - first) / (last -
// first)) * bins before the two edge corrections (numpy 1.x multiplies by bins / (last - first)); the restatement is
// checked against numpy 2.2.6, and a host with numpy 1.x has to pass the equality tests before it trusts this path.
// Every index is bounded by the page geometry in PostPage; no kernel writes outside its page's workspace sections.
#pragma clang fp contract(off)
#include "omr_kernels.h"
#include "omr_post_shared.h"

#include <climits>
#include <cmath>

namespace asr {

namespace {

// numpy's pairwise sum of one row by one wave (a workgroup of 64 threads).  elem(c): element c of the row.  The result is
// valid in lane 0.  leaf_sum: POST_MAX_LEAVES elements of LDS, stack: 64.
template <typename T, typename F>
__device__ __forceinline__ T wave_pairwise_sum(F elem, const PostLeaf *__restrict__ leaves, int n_leaves,
                                               const uint8_t *__restrict__ prog, int n_prog, T *leaf_sum, T *stack) {
    const int lane = threadIdx.x & 63, sub = lane & 7, grp = lane >> 3;
    for (int k0 = 0; k0 < n_leaves; k0 += 8) {
        const int k = k0 + grp;
        const bool on = k < n_leaves;
        int off = 0, len = 0;
        if (on) { off = leaves[k].off; len = leaves[k].len; }
        const int m = len - (len & 7);
        T r = (T)0;
        if (on) {
            r = elem(off + sub);
            for (int i = 8; i < m; i += 8) r = r + elem(off + i + sub);
        }
        r = r + __shfl_xor(r, 1);
        r = r + __shfl_xor(r, 2);
        r = r + __shfl_xor(r, 4);
        if (on && sub == 0) {
            for (int i = m; i < len; ++i) r = r + elem(off + i);
            leaf_sum[k] = r;
        }
    }
    __syncthreads();
    T res = (T)0;
    if (lane == 0) {
        int sp = 0, k = 0;
        for (int i = 0; i < n_prog; ++i) {
            if (prog[i] == 0) {
                stack[sp++] = leaf_sum[k++];
            } else {
                const T b = stack[sp - 1], x = stack[sp - 2];
                sp -= 1;
                stack[sp - 1] = x + b;
            }
        }
        res = stack[0];
    }
    __syncthreads();
    return res;
}

// 1.0 - image of snap_system_to_grid, float32
__device__ __forceinline__ float post_pixel(const PostArgs &a, const PostPage &P, float mx, int r, int c) {
    return 1.0f - seg_load_page(a.page_buf, a.in_mode, P.page_off + (int64_t)r * P.w + c, mx);
}

__global__ __launch_bounds__(64) void post_rows_kernel(PostArgs a) {
    __shared__ double leaf_sum[POST_MAX_LEAVES];
    __shared__ double stack[64];
    const PostPage P = a.pages[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x, w = P.w;
    if (r >= P.h) return;
    const PostLeaf *leaves = a.leaves + P.leaf_off;
    const uint8_t *prog = a.prog + P.prog_off;
    const double *sys = a.sys_maps + P.map_off + (int64_t)r * w;
    const double *bar = a.bar_maps ? a.bar_maps + P.map_off + (int64_t)r * w : nullptr;
    const double *src = bar ? bar : sys;
    const double s = wave_pairwise_sum<double>([&](int c) { return src[c]; }, leaves, P.n_leaves, prog, P.n_prog,
                                               leaf_sum, stack);
    double mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (int c = lane; c < w; c += 64) {
        const double v = sys[c];
        bad |= !isfinite(v);
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        if (bar) bad |= !isfinite(bar[c]);
    }
    mn = wave_reduce(mn, OpMinD());
    mx = wave_reduce(mx, OpMaxD());
    bad = wave_reduce(bad, OpOrI());
    // imagey = blur(1.0 - image, (3, 1)): three columns, REFLECT_101, float64 sum times 1.0 / 3, float32
    const float pmx = a.in_mode ? a.page_max[P.page] : 0.0f;
    const float ys = wave_pairwise_sum<float>(
        [&](int c) {
            const int cm = c > 0 ? c - 1 : 1, cp = c < w - 1 ? c + 1 : w - 2;
            double t = (double)post_pixel(a, P, pmx, r, cm);
            t = t + (double)post_pixel(a, P, pmx, r, c);
            t = t + (double)post_pixel(a, P, pmx, r, cp);
            return (float)(t * (1.0 / 3));
        },
        leaves, P.n_leaves, prog, P.n_prog, (float *)leaf_sum, (float *)stack);
    if (lane == 0) {
        a.proj[P.row_off + r] = s;
        a.rmin[P.row_off + r] = mn;
        a.rmax[P.row_off + r] = mx;
        a.ysig[P.row_off + r] = __fdiv_rn(ys, (float)w);
        if (bad) atomicOr(&a.state[blockIdx.y].nonfinite, 1);
    }
}

__global__ __launch_bounds__(PT) void post_otsu1_kernel(PostArgs a) {
    __shared__ double e[257], hc[256], m2[256], w2[256], red[PT / 64];
    __shared__ unsigned hist[256];
    __shared__ int s_status;
    const int p = blockIdx.x, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    PostState &S = a.state[p];
    if (S.nonfinite) {
        if (tid == 0) S.status = 3;
        return;
    }
    const double *proj = a.proj + P.row_off;
    uint8_t *rowzero = a.rowzero + P.row_off;
    double mn = INFINITY, mx = -INFINITY;
    for (int r = tid; r < P.h; r += PT) {
        mn = fmin(mn, proj[r]);
        mx = fmax(mx, proj[r]);
        rowzero[r] = 0;
    }
    mn = block_reduce(mn, OpMinD(), red);
    mx = block_reduce(mx, OpMaxD(), red);
    for (int i = tid; i <= 256; i += PT) post_edge(mn, mx, i, e);
    hist[tid] = 0;
    __syncthreads();
    if (tid == 0) s_status = post_edges_ok(mn, mx, e) ? 0 : 3;
    __syncthreads();
    if (s_status) {
        if (tid == 0) S.status = s_status;
        return;
    }
    for (int r = tid; r < P.h; r += PT) atomicAdd(&hist[post_bin(proj[r], e)], 1u);
    __syncthreads();
    if (tid == 0) {
        const double thr = post_otsu(hist, e, hc, m2, w2);
        // the run loop of detect_systems over np.nonzero(projection < thresh)
        int n_space = 0, start = 0, prev = 0;
        for (int r = 0; r < P.h; ++r) {
            if (!(proj[r] < thr)) continue;
            if (n_space == 0) {
                start = prev = r;
            } else if (r - prev == 1) {
                prev = r;
            } else {
                if (prev - start > 15)
                    for (int q = start; q < prev; ++q) rowzero[q] = 1;
                start = prev = r;
            }
            ++n_space;
        }
        if (n_space == 0) s_status = 1;
    }
    __syncthreads();
    if (s_status) {
        if (tid == 0) S.status = s_status;
        return;
    }
    mn = INFINITY; mx = -INFINITY;
    for (int r = tid; r < P.h; r += PT) {
        mn = fmin(mn, rowzero[r] ? 0.0 : a.rmin[P.row_off + r]);
        mx = fmax(mx, rowzero[r] ? 0.0 : a.rmax[P.row_off + r]);
    }
    mn = block_reduce(mn, OpMinD(), red);
    mx = block_reduce(mx, OpMaxD(), red);
    for (int i = tid; i <= 256; i += PT) post_edge(mn, mx, i, e);
    __syncthreads();
    for (int i = tid; i <= 256; i += PT) a.edges2[(size_t)p * 257 + i] = e[i];
    if (tid == 0) S.status = post_edges_ok(mn, mx, e) ? 0 : 3;
}

__global__ __launch_bounds__(PT) void post_hist2_kernel(PostArgs a) {
    __shared__ double e[257];
    __shared__ unsigned hist[256];
    const int p = blockIdx.y, tid = threadIdx.x;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i0 = (int64_t)blockIdx.x * PX_PER_BLOCK;
    if (i0 >= n || a.state[p].status) return;
    for (int i = tid; i <= 256; i += PT) e[i] = a.edges2[(size_t)p * 257 + i];
    hist[tid] = 0;
    __syncthreads();
    const double *sys = a.sys_maps + P.map_off;
    const uint8_t *rowzero = a.rowzero + P.row_off;
    const int64_t i1 = i0 + PX_PER_BLOCK < n ? i0 + PX_PER_BLOCK : n;
    for (int64_t i = i0 + tid; i < i1; i += PT) {
        const double v = rowzero[i / P.w] ? 0.0 : sys[i];
        atomicAdd(&hist[post_bin(v, e)], 1u);
    }
    __syncthreads();
    if (hist[tid]) atomicAdd(&a.hist2[(size_t)p * 256 + tid], hist[tid]);
}

__global__ __launch_bounds__(64) void post_otsu2_kernel(PostArgs a) {
    __shared__ double e[257], hc[256], m2[256], w2[256];
    __shared__ unsigned hist[256];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (a.state[p].status) return;
    for (int i = tid; i <= 256; i += 64) e[i] = a.edges2[(size_t)p * 257 + i];
    for (int i = tid; i < 256; i += 64) hist[i] = a.hist2[(size_t)p * 256 + i];
    __syncthreads();
    if (tid == 0) a.state[p].thr2 = post_otsu(hist, e, hc, m2, w2);
}

__global__ __launch_bounds__(PT) void post_fg_kernel(PostArgs a) {
    const int p = blockIdx.y;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n || a.state[p].status) return;
    const double v = a.rowzero[P.row_off + i / P.w] ? 0.0 : a.sys_maps[P.map_off + i];
    a.fg[P.px_off + i] = v > a.state[p].thr2;
}

// dilation of the 15x1 closing: rows r - 7 .. r + 7, outside the page counts as 0
__global__ __launch_bounds__(PT) void post_dilate_kernel(PostArgs a) {
    const int p = blockIdx.y;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n || a.state[p].status) return;
    const int r = (int)(i / P.w), c = (int)(i - (int64_t)r * P.w);
    const int r0 = r - 7 < 0 ? 0 : r - 7, r1 = r + 7 > P.h - 1 ? P.h - 1 : r + 7;
    const uint8_t *fg = a.fg + P.px_off;
    uint8_t d = 0;
    for (int q = r0; q <= r1; ++q) d |= fg[(int64_t)q * P.w + c];
    a.tmp[P.px_off + i] = d;
}

// erosion of the closing (outside the page counts as 1) and the first labels: one wave per row, every foreground pixel
// gets the linear index of the first pixel of its horizontal run
__global__ __launch_bounds__(64) void post_erode_label_kernel(PostArgs a) {
    const int p = blockIdx.y, r = blockIdx.x, lane = threadIdx.x;
    const PostPage P = a.pages[p];
    if (r >= P.h || a.state[p].status) return;
    const int w = P.w;
    const int r0 = r - 7 < 0 ? 0 : r - 7, r1 = r + 7 > P.h - 1 ? P.h - 1 : r + 7;
    const uint8_t *dil = a.tmp + P.px_off;
    uint8_t *fg = a.fg + P.px_off + (int64_t)r * w;
    int32_t *label = a.label + P.px_off + (int64_t)r * w;
    const int base = r * w;                   // h * w <= 2^28
    int carry = -1;                           // start of the run that reaches the chunk's left edge, or -1
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int c = c0 + lane;
        uint8_t e = 0;
        if (c < w) {
            e = 1;
            for (int q = r0; q <= r1; ++q) e &= dil[(int64_t)q * w + c];
            fg[c] = e;
        }
        const int start = post_run_start(e != 0, c0, lane, carry);
        if (c < w) label[c] = e ? base + start : -1;
    }
}

__global__ __launch_bounds__(PT) void post_scan_kernel(PostArgs a) {
    const int p = blockIdx.y;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n || a.state[p].status) return;
    int32_t *label = a.label + P.px_off;
    const int L = label[i];
    if (L < 0) return;
    const int r = (int)(i / P.w), c = (int)(i - (int64_t)r * P.w);
    int m = L;
    for (int dr = -1; dr <= 1; ++dr) {
        const int q = r + dr;
        if (q < 0 || q >= P.h) continue;
        for (int dc = -1; dc <= 1; ++dc) {
            const int x = c + dc;
            if (x < 0 || x >= P.w) continue;
            const int v = label[(int64_t)q * P.w + x];
            if (v >= 0 && v < m) m = v;
        }
    }
    if (m < L) {
        atomicMin(&label[L], m);
        *a.changed = 1;
    }
}

__global__ __launch_bounds__(PT) void post_flatten_kernel(PostArgs a) {
    const int p = blockIdx.y;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n || a.state[p].status) return;
    int32_t *label = a.label + P.px_off;
    int r = label[i];
    if (r < 0) return;
    for (int q = label[r]; q != r; q = label[r]) r = q;      // labels decrease along the chain: it ends at a root
    label[i] = r;
}

__global__ __launch_bounds__(PT) void post_area_kernel(PostArgs a) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    const bool in = i < n && !a.state[p].status;
    const int L = in ? a.label[P.px_off + i] : -1;
    bool active = L >= 0;
    for (;;) {
        const unsigned long long todo = __ballot(active);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int Lr = __shfl(L, leader);
        const bool same = active && L == Lr;
        const unsigned long long grp = __ballot(same);
        if (lane == leader) atomicAdd(&a.area[P.px_off + Lr], (int)__popcll(grp));
        if (same) active = false;
    }
}

__global__ __launch_bounds__(PT) void post_keep_kernel(PostArgs a) {
    const int p = blockIdx.y;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (i >= n || a.state[p].status) return;
    if (a.label[P.px_off + i] != (int)i || a.area[P.px_off + i] < POST_MIN_AREA) return;
    const unsigned slot = atomicAdd(&a.state[p].n_kept, 1u);
    if (slot < (unsigned)a.cap) a.blobs[(size_t)p * a.cap + slot].root = (int)i;
}

// kept roots in index order; area[root] becomes -(slot + 1) so that a pixel finds its blob through its label
__global__ void post_sort_kernel(PostArgs a) {
    const int p = blockIdx.x;
    if (threadIdx.x || a.state[p].status) return;
    const PostPage P = a.pages[p];
    PostBlob *B = a.blobs + (size_t)p * a.cap;
    if (a.state[p].n_kept > (unsigned)a.cap) {
        a.state[p].status = 3;
        return;
    }
    const int n = (int)a.state[p].n_kept;
    for (int i = 1; i < n; ++i) {
        const int v = B[i].root;
        int j = i;
        for (; j > 0 && B[j - 1].root > v; --j) B[j].root = B[j - 1].root;
        B[j].root = v;
    }
    for (int i = 0; i < n; ++i) {
        B[i].min_r = B[i].min_c = INT_MAX;
        B[i].max_r = B[i].max_c = -1;
        B[i].status = 3;
        a.area[P.px_off + B[i].root] = -(i + 1);
    }
}

__global__ __launch_bounds__(PT) void post_bbox_kernel(PostArgs a) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const PostPage P = a.pages[p];
    const int64_t n = (int64_t)P.h * P.w, i = (int64_t)blockIdx.x * PT + threadIdx.x;
    const bool in = i < n && !a.state[p].status;
    const int L = in ? a.label[P.px_off + i] : -1;
    int k = -1;
    if (L >= 0) {
        const int v = a.area[P.px_off + L];
        if (v < 0) k = -v - 1;
    }
    const int r = in ? (int)(i / P.w) : 0, c = in ? (int)(i - (int64_t)r * P.w) : 0;
    bool active = k >= 0;
    for (;;) {
        const unsigned long long todo = __ballot(active);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int kr = __shfl(k, leader);
        const bool same = active && k == kr;
        const int r_lo = wave_reduce(same ? r : INT_MAX, OpMinI()), r_hi = wave_reduce(same ? r : -1, OpMaxI());
        const int c_lo = wave_reduce(same ? c : INT_MAX, OpMinI()), c_hi = wave_reduce(same ? c : -1, OpMaxI());
        if (lane == leader && kr < a.cap) {
            PostBlob &B = a.blobs[(size_t)p * a.cap + kr];
            atomicMin(&B.min_r, r_lo);
            atomicMax(&B.max_r, r_hi);
            atomicMin(&B.min_c, c_lo);
            atomicMax(&B.max_c, c_hi);
        }
        if (same) active = false;
    }
}

// key of an edge candidate at coordinate x for a target: smallest distance first, ties to the larger coordinate (the
// host's candidates are in reversed order and np.argmin takes the first minimum)
__device__ __forceinline__ long long post_cand_key(int target, int x) {
    const int d = target > x ? target - x : x - target;
    return ((long long)d << 32) | (long long)(unsigned)(INT_MAX - x);
}

__global__ __launch_bounds__(PT) void post_blob_kernel(PostArgs a) {
    __shared__ int red_i[PT / 64];
    __shared__ float red_f[PT / 64];
    __shared__ long long red_l[PT / 64];
    const int p = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    if (a.state[p].status) return;
    if ((unsigned)k >= a.state[p].n_kept || k >= a.cap) return;
    const PostPage P = a.pages[p];
    PostBlob &B = a.blobs[(size_t)p * a.cap + k];
    const int h = P.h, w = P.w, root = B.root;
    const int32_t *label = a.label + P.px_off;
    const int bmin_r = B.min_r, bmin_c = B.min_c, bmax_r = B.max_r, bmax_c = B.max_c;
    if (bmax_r < bmin_r || bmax_c < bmin_c) return;          // (status stays 3)

    // ---- shrink_bounding_box on label == root; regionprops' box is half open
    int min_row = bmin_r, min_col = bmin_c;
    int max_row = bmax_r + 1 < h - 1 ? bmax_r + 1 : h - 1, max_col = bmax_c + 1 < w - 1 ? bmax_c + 1 : w - 1;
    const int max_row0 = max_row, max_col0 = max_col;
    const int n_cols = max_col - min_col;
    if (n_cols <= 0) return;
    for (;;) {
        int cnt = 0;
        for (int c = min_col + tid; c < max_col; c += PT) cnt += label[(int64_t)min_row * w + c] == root;
        cnt = block_reduce(cnt, OpAddI(), red_i);
        if (!((double)cnt / (double)n_cols < 0.9)) break;
        if (++min_row > max_row0) return;                    // the host runs off the blob: IndexError
    }
    for (;;) {
        int cnt = 0;
        for (int c = min_col + tid; c < max_col; c += PT) cnt += label[(int64_t)max_row * w + c] == root;
        cnt = block_reduce(cnt, OpAddI(), red_i);
        if (!((double)cnt / (double)n_cols < 0.9)) break;
        if (--max_row < bmin_r) return;
    }
    const int n_rows = max_row - min_row;
    if (n_rows <= 0) return;
    for (;;) {
        int cnt = 0;
        for (int r = min_row + tid; r < max_row; r += PT) cnt += label[(int64_t)r * w + min_col] == root;
        cnt = block_reduce(cnt, OpAddI(), red_i);
        if (!((double)cnt / (double)n_rows < 0.9)) break;
        if (++min_col > max_col0) return;
    }
    for (;;) {
        int cnt = 0;
        for (int r = min_row + tid; r < max_row; r += PT) cnt += label[(int64_t)r * w + max_col] == root;
        cnt = block_reduce(cnt, OpAddI(), red_i);
        if (!((double)cnt / (double)n_rows < 0.9)) break;
        if (--max_col < bmin_c) return;
    }

    // ---- snap_system_to_grid, y-direction: the page's signal
    int status = 0;
    {
        const float *ys = a.ysig + P.row_off;
        float mn = INFINITY, mx = -INFINITY;
        int bad = 0;
        for (int r = tid; r < h; r += PT) {
            bad |= !isfinite(ys[r]);
            mn = fminf(mn, ys[r]);
            mx = fmaxf(mx, ys[r]);
        }
        bad = block_reduce(bad, OpOrI(), red_i);
        mn = block_reduce(mn, OpMinF(), red_f);
        mx = block_reduce(mx, OpMaxF(), red_f);
        if (bad) return;
        const float t = fmaxf(mn, 0.5f * mx);
        long long k_min = LLONG_MAX, k_max = LLONG_MAX;
        if (mn != mx)
            for (int r = 1 + tid; r < h - 1; r += PT) {
                const float v = ys[r];
                if (v >= ys[r - 1] && v >= ys[r + 1] && v > t) {
                    const long long k1 = post_cand_key(min_row, r), k2 = post_cand_key(max_row, r);
                    k_min = k1 < k_min ? k1 : k_min;
                    k_max = k2 < k_max ? k2 : k_max;
                }
            }
        k_min = block_reduce(k_min, OpMinLL(), red_l);
        k_max = block_reduce(k_max, OpMinLL(), red_l);
        if (k_min == LLONG_MAX) {
            status = 2;
        } else if ((k_min >> 32) < 10 && (k_max >> 32) < 10) {
            min_row = INT_MAX - (int)(unsigned)(k_min & 0xffffffffll);
            max_row = INT_MAX - (int)(unsigned)(k_max & 0xffffffffll);
        }
    }
    if (status) {
        if (tid == 0) B.status = status;
        return;
    }

    // ---- x-direction: imagex[min_row:max_row].mean(axis=0), row after row in float32
    const int n_mean = max_row - min_row;
    if (n_mean <= 0) return;                                 // empty slice
    float *xs = a.xsig + ((size_t)p * a.cap + k) * a.max_w;
    const float pmx = a.in_mode ? a.page_max[P.page] : 0.0f;
    for (int c = tid; c < w; c += PT) {
        float acc = 0.0f;
        float up = post_pixel(a, P, pmx, min_row > 0 ? min_row - 1 : 1, c), mid = post_pixel(a, P, pmx, min_row, c);
        for (int r = min_row; r < max_row; ++r) {
            const float dn = post_pixel(a, P, pmx, r < h - 1 ? r + 1 : h - 2, c);
            double t = (double)up;
            t = t + (double)mid;
            t = t + (double)dn;
            acc = acc + (float)(t * (1.0 / 3));
            up = mid;
            mid = dn;
        }
        xs[c] = __fdiv_rn(acc, (float)n_mean);
    }
    __syncthreads();
    {
        float mn = INFINITY, mx = -INFINITY;
        int bad = 0;
        for (int c = tid; c < w; c += PT) {
            bad |= !isfinite(xs[c]);
            mn = fminf(mn, xs[c]);
            mx = fmaxf(mx, xs[c]);
        }
        bad = block_reduce(bad, OpOrI(), red_i);
        mn = block_reduce(mn, OpMinF(), red_f);
        mx = block_reduce(mx, OpMaxF(), red_f);
        if (bad) return;
        const float t = fmaxf(mn, 0.5f * mx);
        long long k_min = LLONG_MAX, k_max = LLONG_MAX;
        if (mn != mx)
            for (int c = 1 + tid; c < w - 1; c += PT) {
                const float v = xs[c];
                if (v >= xs[c - 1] && v >= xs[c + 1] && v > t) {
                    const long long k1 = post_cand_key(min_col, c), k2 = post_cand_key(max_row, c);   // (max_row: as the host)
                    k_min = k1 < k_min ? k1 : k_min;
                    k_max = k2 < k_max ? k2 : k_max;
                }
            }
        k_min = block_reduce(k_min, OpMinLL(), red_l);
        k_max = block_reduce(k_max, OpMinLL(), red_l);
        if (k_min == LLONG_MAX) {
            status = 2;
        } else if ((k_min >> 32) < 10 && (k_max >> 32) < 10) {
            min_col = INT_MAX - (int)(unsigned)(k_min & 0xffffffffll);
            max_col = INT_MAX - (int)(unsigned)(k_max & 0xffffffffll);
        }
    }
    if (tid == 0) {
        B.out[0] = min_row; B.out[1] = max_row; B.out[2] = min_col; B.out[3] = max_col;
        B.status = status;
    }
}

dim3 px_grid(const PostArgs &a, int per_block) {
    return dim3((unsigned)((a.max_px + per_block - 1) / per_block), (unsigned)a.n_pages);
}

}  // namespace

hipError_t launch_post_rows(hipStream_t s, const PostArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(post_rows_kernel, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_post_threshold(hipStream_t s, const PostArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(post_otsu1_kernel, dim3(a.n_pages), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_hist2_kernel, px_grid(a, PX_PER_BLOCK), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_otsu2_kernel, dim3(a.n_pages), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_post_close(hipStream_t s, const PostArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(post_fg_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_dilate_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_erode_label_kernel, dim3(a.max_h, a.n_pages), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_post_label_pass(hipStream_t s, const PostArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(post_scan_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_flatten_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_post_blobs(hipStream_t s, const PostArgs &a) {
    if (a.n_pages < 1) return hipSuccess;
    hipLaunchKernelGGL(post_area_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_keep_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_sort_kernel, dim3(a.n_pages), dim3(64), 0, s, a);
    hipLaunchKernelGGL(post_bbox_kernel, px_grid(a, PT), dim3(PT), 0, s, a);
    hipLaunchKernelGGL(post_blob_kernel, dim3(a.cap, a.n_pages), dim3(PT), 0, s, a);
    return hipGetLastError();
}

}  // namespace asr
