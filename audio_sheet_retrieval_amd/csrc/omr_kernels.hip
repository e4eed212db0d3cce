// gfx950 kernels of the staff-system detector (asr_seg_predict_dev; sheet_utils/omr.py, system_detector.py): the
// 15-layer U-Net of SegmentationNetwork in inference mode, over a batch of tiles, and the sliding-window stitch.
//
//   seg_page_max_kernel : page maximum for prepare_image (raw float32 / uint8 pages), one workgroup per page.
//   seg_conv3_kernel    : 3x3 'same' conv + BN + ELU.  One thread per 2x2 output quad and CO_T output channels: a 4x4
//                         input patch per input channel feeds 4 x 9 x CO_T FMAs, and the wave-uniform weights come
//                         through the scalar cache.  The epilogue optionally writes the 2x2/2 max-pool as well (the
//                         encoder's dual output: pre-pool skip + pooled tensor) or, for the last block, the 1x1 conv
//                         + sigmoid head instead of the activation.  The first block reads the pages through the tile
//                         table (no materialised tiles): zero outside the page and outside the tile, prepare folded
//                         in (an IEEE divide by the page max, bit-identical to host-prepared input).
//   seg_up_kernel       : one decoder level: TransposedConv2D 2x2/2 as a per-pixel GEMM row (K = ci, N = 4 x CO_T),
//                         BN + ReLU, the skip add and the second BN, one thread per input pixel.
//   seg_stitch_kernel   : one thread per page pixel gathers w * P over the tiles covering it in the reference's tile
//                         order (rows outer, columns inner), float64, no contraction, then R / V (0 / 0 = NaN where no
//                         tile covers the pixel, as in the reference).  No atomics: bit-identical to the numpy loop.
// Every index is bounded by the tile / page geometry passed in; no kernel writes outside its own output rows.
#include "omr_kernels.h"

#include <cmath>

namespace asr {

namespace {

constexpr int SEG_THREADS = 256;

__global__ __launch_bounds__(SEG_THREADS) void seg_page_max_kernel(const void *__restrict__ pages, int in_mode,
                                                                   const SegPage *__restrict__ desc,
                                                                   float *__restrict__ page_max) {
    __shared__ float red[SEG_THREADS];
    const SegPage P = desc[blockIdx.x];
    const int64_t n = (int64_t)P.h * P.w;
    float m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += SEG_THREADS) {
        const float v = in_mode == 2 ? (float)((const uint8_t *)pages)[P.offset + i] : ((const float *)pages)[P.offset + i];
        m = fmaxf(m, v);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int k = SEG_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) page_max[blockIdx.x] = red[0];
}

__device__ __forceinline__ float seg_elu(float v) { return v > 0.0f ? v : expm1f(v); }

// theano's float32 scalar sigmoid (tensor/nnet/sigm.py ScalarSigmoid.c_code): clamped at -88 and 15
__device__ __forceinline__ float seg_sigmoid(float z) {
    return z < -88.0f ? 0.0f : z > 15.0f ? 1.0f : 1.0f / (1.0f + expf(-z));
}

// grid: x = quad blocks of one tile, y = output-channel groups of CO_T, z = tiles
template <int CI, int CO_T, bool PAGE, bool POOL, bool HEAD>
__global__ __launch_bounds__(SEG_THREADS) void seg_conv3_kernel(SegConvArgs a) {
    const int H = a.H, W = a.W, CO = a.co;
    const int QW = W >> 1, nq = (H >> 1) * QW;
    const int q = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (q >= nq) return;
    const int qy = q / QW, qx = q - qy * QW;
    const int y0 = 2 * qy - 1, x0 = 2 * qx - 1;      // patch origin in tile coordinates
    const int t = blockIdx.z, co0 = blockIdx.y * CO_T;
    const int64_t plane = (int64_t)H * W;

    // PAGE: the tile is a window of its page; the conv's zero padding is at the tile border
    int64_t poff = 0;
    int ty = 0, tx = 0, ph = 0, pw = 0;
    float mx = 0.0f;
    if (PAGE) {
        const SegTile T = a.tiles[t];
        const SegPage P = a.page_desc[T.page];
        poff = P.offset; ph = P.h; pw = P.w; ty = T.y0; tx = T.x0;
        mx = a.in_mode ? a.page_max[T.page] : 0.0f;
    }
    const float *in_t = PAGE ? nullptr : a.in + (int64_t)t * CI * plane;

    float acc[4][CO_T];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < CO_T; ++k) acc[i][k] = 0.0f;

    for (int ci = 0; ci < CI; ++ci) {
        float p[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int x = x0 + c;
                float v = 0.0f;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    if (PAGE) {
                        const int py = ty + y, px = tx + x;
                        if (py >= 0 && py < ph && px >= 0 && px < pw)
                            v = seg_load_page(a.pages, a.in_mode, poff + (int64_t)py * pw + px, mx);
                    } else {
                        v = in_t[(int64_t)ci * plane + (int64_t)y * W + x];
                    }
                }
                p[r][c] = v;
            }
        }
        const float *wc = a.w + (int64_t)ci * 9 * CO + co0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float *wt = wc + (dy * 3 + dx) * CO;
#pragma unroll
                for (int k = 0; k < CO_T; ++k) {
                    const float wv = wt[k];
                    acc[0][k] = fmaf(wv, p[dy][dx], acc[0][k]);
                    acc[1][k] = fmaf(wv, p[dy][dx + 1], acc[1][k]);
                    acc[2][k] = fmaf(wv, p[dy + 1][dx], acc[2][k]);
                    acc[3][k] = fmaf(wv, p[dy + 1][dx + 1], acc[3][k]);
                }
            }
    }

    const float *mean = a.bn, *scale = a.bn + CO, *beta = a.bn + 2 * CO;
    const int64_t o = (int64_t)(2 * qy) * W + 2 * qx;
    if (HEAD) {
        float z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = a.head[8];
#pragma unroll
        for (int k = 0; k < CO_T; ++k) {
            const float m = mean[co0 + k], sc = scale[co0 + k], b = beta[co0 + k], hw = a.head[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = fmaf(hw, seg_elu((acc[i][k] - m) * sc + b), z[i]);
        }
        float *out = a.out + (int64_t)t * plane;
        *(float2 *)(out + o) = make_float2(seg_sigmoid(z[0]), seg_sigmoid(z[1]));
        *(float2 *)(out + o + W) = make_float2(seg_sigmoid(z[2]), seg_sigmoid(z[3]));
        return;
    }
#pragma unroll
    for (int k = 0; k < CO_T; ++k) {
        const int co = co0 + k;
        const float m = mean[co], sc = scale[co], b = beta[co];
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = seg_elu((acc[i][k] - m) * sc + b);
        float *out = a.out + ((int64_t)t * CO + co) * plane;
        *(float2 *)(out + o) = make_float2(v[0], v[1]);
        *(float2 *)(out + o + W) = make_float2(v[2], v[3]);
        if (POOL)
            a.pooled[((int64_t)t * CO + co) * (plane >> 2) + q] = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    }
}

// grid: x = input-pixel blocks of one tile, y = output-channel groups of CO_T, z = tiles
template <int CI, int CO_T>
__global__ __launch_bounds__(SEG_THREADS) void seg_up_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                             const float *__restrict__ bn1, const float *__restrict__ bn2,
                                                             const float *__restrict__ skip, float *__restrict__ out,
                                                             int CO, int h, int wd) {
    const int npx = h * wd;
    const int pxl = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (pxl >= npx) return;
    const int i = pxl / wd, j = pxl - i * wd;
    const int t = blockIdx.z, co0 = blockIdx.y * CO_T;
    const float *in_t = in + (int64_t)t * CI * npx + pxl;

    float acc[4][CO_T];
#pragma unroll
    for (int ab = 0; ab < 4; ++ab)
#pragma unroll
        for (int k = 0; k < CO_T; ++k) acc[ab][k] = 0.0f;
    for (int ci = 0; ci < CI; ++ci) {
        const float x = in_t[(int64_t)ci * npx];
        const float *wc = w + (int64_t)ci * 4 * CO + co0;
#pragma unroll
        for (int ab = 0; ab < 4; ++ab)
#pragma unroll
            for (int k = 0; k < CO_T; ++k) acc[ab][k] = fmaf(x, wc[ab * CO + k], acc[ab][k]);
    }
    const int W2 = 2 * wd;
    const int64_t plane2 = (int64_t)4 * npx;
    const int64_t o = (int64_t)(2 * i) * W2 + 2 * j;
#pragma unroll
    for (int k = 0; k < CO_T; ++k) {
        const int co = co0 + k;
        const float m1 = bn1[co], s1 = bn1[CO + co], b1 = bn1[2 * CO + co];
        const float m2 = bn2[co], s2 = bn2[CO + co], b2 = bn2[2 * CO + co];
        const int64_t base = ((int64_t)t * CO + co) * plane2 + o;
        const float2 s0 = *(const float2 *)(skip + base), sk1 = *(const float2 *)(skip + base + W2);
        const float sv[4] = {s0.x, s0.y, sk1.x, sk1.y};
        float v[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const float r = fmaxf((acc[ab][k] - m1) * s1 + b1, 0.0f);
            v[ab] = ((sv[ab] + r) - m2) * s2 + b2;
        }
        *(float2 *)(out + base) = make_float2(v[0], v[1]);
        *(float2 *)(out + base + W2) = make_float2(v[2], v[3]);
    }
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(SEG_THREADS) void seg_stitch_kernel(const float *__restrict__ tile_p,
                                                                 const double *__restrict__ win, int th, int tw,
                                                                 const SegStitch *__restrict__ desc,
                                                                 double *__restrict__ out) {
    const SegStitch D = desc[blockIdx.y];
    const int64_t n = (int64_t)D.h * D.w;
    const int64_t pix = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (pix >= n) return;
    const int r = (int)(pix / D.w), c = (int)(pix - (int64_t)r * D.w);
    const int64_t tile_px = (int64_t)th * tw;
    if (D.direct) {
        out[D.out_offset + pix] = (double)tile_p[(int64_t)D.first_tile * tile_px + pix];
        return;
    }
    const int pr = r + D.pad_top, pc = c + D.pad_left;     // padded coordinates
    // tiles k with k * step <= p < k * step + tile
    const int kr0 = pr >= th ? (pr - th) / D.step_h + 1 : 0, kr1 = min(D.n_rows - 1, pr / D.step_h);
    const int kc0 = pc >= tw ? (pc - tw) / D.step_w + 1 : 0, kc1 = min(D.n_cols - 1, pc / D.step_w);
    double R = 0.0, V = 0.0;
    for (int kr = kr0; kr <= kr1; ++kr) {
        const int ly = pr - kr * D.step_h;
        for (int kc = kc0; kc <= kc1; ++kc) {
            const int lx = pc - kc * D.step_w;
            const double wv = win[(int64_t)ly * tw + lx];
            const int64_t tile = D.first_tile + (int64_t)kr * D.n_cols + kc;
            R = R + (double)tile_p[tile * tile_px + (int64_t)ly * tw + lx] * wv;
            V = V + wv;
        }
    }
    out[D.out_offset + pix] = R / V;
}
#pragma clang fp contract(on)

template <int CI, int CO_T, bool PAGE, bool POOL, bool HEAD>
hipError_t conv3_go(hipStream_t s, const SegConvArgs &a) {
    const int nq = (a.H / 2) * (a.W / 2);
    dim3 grid((nq + SEG_THREADS - 1) / SEG_THREADS, a.co / CO_T, a.n);
    hipLaunchKernelGGL((seg_conv3_kernel<CI, CO_T, PAGE, POOL, HEAD>), grid, dim3(SEG_THREADS), 0, s, a);
    return hipGetLastError();
}

template <int CI, int CO_T>
hipError_t conv3_pool(hipStream_t s, const SegConvArgs &a) {
    return a.pooled ? conv3_go<CI, CO_T, false, true, false>(s, a) : conv3_go<CI, CO_T, false, false, false>(s, a);
}

template <int CI, int CO_T>
hipError_t up_go(hipStream_t s, const float *in, const float *w, const float *bn1, const float *bn2, const float *skip,
                 float *out, int co, int h, int wd, int n) {
    dim3 grid((h * wd + SEG_THREADS - 1) / SEG_THREADS, co / CO_T, n);
    hipLaunchKernelGGL((seg_up_kernel<CI, CO_T>), grid, dim3(SEG_THREADS), 0, s, in, w, bn1, bn2, skip, out, co, h, wd);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_seg_page_max(hipStream_t s, const void *pages, int in_mode, const SegPage *desc, int n_pages,
                               float *page_max) {
    if (n_pages <= 0) return hipSuccess;
    hipLaunchKernelGGL(seg_page_max_kernel, dim3(n_pages), dim3(SEG_THREADS), 0, s, pages, in_mode, desc, page_max);
    return hipGetLastError();
}

hipError_t launch_seg_conv3(hipStream_t s, const SegConvArgs &a) {
    if (a.n <= 0) return hipSuccess;
    if ((a.H & 1) || (a.W & 1)) return hipErrorInvalidValue;
    const bool pool = a.pooled != nullptr;
    if (a.ci == 1 && a.co == 8 && !pool && !a.head) return conv3_go<1, 8, true, false, false>(s, a);
    if (a.ci == 8 && a.co == 8 && a.head) return conv3_go<8, 8, false, false, true>(s, a);
    if (a.head) return hipErrorInvalidValue;
    if (a.ci == 8 && a.co == 8) return conv3_pool<8, 8>(s, a);
    if (a.ci == 8 && a.co == 16 && !pool) return conv3_go<8, 16, false, false, false>(s, a);
    if (a.ci == 16 && a.co == 16) return conv3_pool<16, 16>(s, a);
    if (a.ci == 16 && a.co == 32 && !pool) return conv3_go<16, 16, false, false, false>(s, a);
    if (a.ci == 32 && a.co == 32) return conv3_pool<32, 16>(s, a);
    if (a.ci == 32 && a.co == 64 && !pool) return conv3_go<32, 16, false, false, false>(s, a);
    if (a.ci == 64 && a.co == 64 && !pool) return conv3_go<64, 16, false, false, false>(s, a);
    return hipErrorInvalidValue;
}

hipError_t launch_seg_up(hipStream_t s, const float *in, const float *w, const float *bn1, const float *bn2,
                         const float *skip, float *out, int ci, int co, int h, int wd, int n) {
    if (n <= 0) return hipSuccess;
    if (ci == 64 && co == 32) return up_go<64, 8>(s, in, w, bn1, bn2, skip, out, co, h, wd, n);
    if (ci == 32 && co == 16) return up_go<32, 8>(s, in, w, bn1, bn2, skip, out, co, h, wd, n);
    if (ci == 16 && co == 8) return up_go<16, 8>(s, in, w, bn1, bn2, skip, out, co, h, wd, n);
    return hipErrorInvalidValue;
}

hipError_t launch_seg_stitch(hipStream_t s, const float *tile_p, const double *win, int th, int tw,
                             const SegStitch *desc, int n_pages, int max_pixels, double *out) {
    if (n_pages <= 0 || max_pixels <= 0) return hipSuccess;
    dim3 grid((max_pixels + SEG_THREADS - 1) / SEG_THREADS, n_pages);
    hipLaunchKernelGGL(seg_stitch_kernel, grid, dim3(SEG_THREADS), 0, s, tile_p, win, th, tw, desc, out);
    return hipGetLastError();
}

}  // namespace asr
