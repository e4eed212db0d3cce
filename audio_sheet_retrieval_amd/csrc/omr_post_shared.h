// Device code shared by the translation units that restate numpy on the maps of the segmentation networks
// (omr_post_kernels.hip: systems; omr_detect_kernels.hip: bars and note heads): workgroup reductions, np.histogram's
// 256 uniform bins, threshold_otsu on them, and the run labels of a row.  Both units are built with floating-point contraction off.
#pragma once
#include "omr_kernels.h"

#include <climits>
#include <cmath>

namespace asr {

namespace {

constexpr int PT = 256;
constexpr int PX_PER_BLOCK = PT * 8;

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    for (int k = 1; k < 64; k <<= 1) v = op(v, __shfl_xor(v, k));
    return v;
}

// reduction over a workgroup of PT threads; the result in every thread.  red: PT / 64 elements of LDS
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T *red) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = red[0];
    for (int k = 1; k < PT / 64; ++k) r = op(r, red[k]);
    __syncthreads();
    return r;
}

struct OpMinD { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMaxD { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
struct OpMinF { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct OpMaxF { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct OpAddI { __device__ int operator()(int a, int b) const { return a + b; } };
struct OpOrI { __device__ int operator()(int a, int b) const { return a | b; } };
struct OpMinI { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct OpMaxI { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpMinLL { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };

// np.histogram(x, 256)'s edges: _get_outer_edges + np.linspace(first, last, 257).  Thread i writes e[i] (i <= 256).
__device__ __forceinline__ void post_edge(double first, double last, int i, double *e) {
    if (first == last) { first = first - 0.5; last = last + 0.5; }
    const double step = (last - first) / 256.0;
    e[i] = i == 256 ? last : (double)i * step + first;
}

// what np.histogram / np.linspace reject or handle specially: not decided here
__device__ __forceinline__ bool post_edges_ok(double first, double last, const double *e) {
    if (!isfinite(first) || !isfinite(last)) return false;
    if (first == last) { first = first - 0.5; last = last + 0.5; }
    if ((last - first) / 256.0 == 0.0 || !isfinite(last - first)) return false;
    for (int i = 0; i < 256; ++i)
        if (!(e[i] < e[i + 1])) return false;
    return true;
}

// bin of x (e[0] <= x <= e[256]) as np.histogram's uniform-bin path finds it
__device__ __forceinline__ int post_bin(double x, const double *e) {
    const double first = e[0], denom = e[256] - e[0];
    int idx = (int)(((x - first) / denom) * 256.0);
    idx = idx < 0 ? 0 : idx > 256 ? 256 : idx;
    if (idx == 256) idx -= 1;
    if (x < e[idx] && idx > 0) idx -= 1;
    if (x >= e[idx + 1] && idx != 255) idx += 1;
    return idx;
}

// threshold_otsu on 256 counts and their edges, by one thread; hc, m2, w2: 256 doubles of LDS each
__device__ double post_otsu(const unsigned *hist, const double *e, double *hc, double *m2, double *w2) {
    for (int i = 0; i < 256; ++i) hc[i] = (double)hist[i] * ((e[i] + e[i + 1]) / 2.0);
    double cw = 0.0, cs = 0.0;
    for (int i = 255; i >= 0; --i) {         // the cumulative sums of the reversed arrays
        cw = cw + (double)hist[i];
        cs = cs + hc[i];
        w2[i] = cw;
        m2[i] = cs / cw;
    }
    cw = 0.0; cs = 0.0;
    double best = 0.0;
    int idx = 0;
    for (int i = 0; i < 255; ++i) {
        cw = cw + (double)hist[i];
        cs = cs + hc[i];
        const double d = cs / cw - m2[i + 1];
        const double v = (cw * w2[i + 1]) * (d * d);
        if (i == 0) best = v;
        if (v != v) { idx = i; break; }       // np.argmax: the first NaN
        if (v > best) { best = v; idx = i; }
    }
    return (e[idx] + e[idx + 1]) / 2.0;
}

// Run labels of one row by one wave, 64 columns at a time.  e: this lane's pixel is foreground; c0: first column of the
// chunk; carry: start of the run that reaches the chunk's left edge, or -1 (updated for the next chunk).  Returns the
// column where the run of this lane's pixel starts (meaningful where e is set).
__device__ __forceinline__ int post_run_start(bool e, int c0, int lane, int &carry) {
    const unsigned long long mask = __ballot(e);
    const unsigned long long below = lane ? ~mask & ((1ull << lane) - 1ull) : 0ull;    // gaps left of this lane
    int start;
    if (below == 0ull) start = carry >= 0 ? carry : c0;
    else start = c0 + (63 - __clzll((long long)below)) + 1;
    if (mask >> 63) {
        const unsigned long long gaps = ~mask;
        carry = gaps == 0ull ? (carry >= 0 ? carry : c0) : c0 + (63 - __clzll((long long)gaps)) + 1;
    } else {
        carry = -1;
    }
    return start;
}

}  // namespace

}  // namespace asr
