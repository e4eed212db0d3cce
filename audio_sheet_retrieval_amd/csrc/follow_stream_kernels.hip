// gfx950 kernels of score following for parallel live streams whose state stays on the device
// (asr_follow_stream_windows_dev, asr_follow_stream_log_dev): per round of new columns the query windows on the step
// grid of every stream, cut from [tail | new block], and per stream a linear log of its last window codes that
// asr_dtw_follow_batch_dev reads as its query buffer.  Pure data movement - no LDS, no atomics: the host knows every
// count, so the order of the windows and of the log rows is fixed before anything is launched.
//
//   follow_stream_window_kernel : one workgroup per window.  Window i of a stream = columns c0 + i * step .. + width - 1
//                                 of [tail | new]: consecutive lanes write consecutive floats of the window (rows of
//                                 width floats, coalesced) - four per lane as one 128-bit store where bins * width is a
//                                 multiple of 4 and the buffer is aligned - and read consecutive floats of a tail or
//                                 block row, which neighbouring windows share and the cache serves.
//   follow_stream_tail_kernel   : track_stream_tail_kernel's discipline, launched behind the windows: new tail = the
//                                 last width - 1 columns of [tail | new]; an element's source lies n_new floats further
//                                 in the same row, so the workgroup goes through the tail in ascending chunks, reads a
//                                 chunk's sources, waits at a barrier and writes the chunk - no chunk writes what a later
//                                 one still reads.
//   follow_stream_log_kernel    : one workgroup per stream with new rows.  The last `kept` rows of the log move to its
//                                 front by the same chunk-and-barrier walk (a row's source lies further on in the same
//                                 log), then the new code rows are copied behind them; 128 bits per lane where dim and
//                                 the offsets are multiples of 4.
// Every index is checked against the sizes the host validated.  The kernels only move floats; fp contract is off here
// and in build.py like in the neighbouring files.
#pragma clang fp contract(off)
#include "asr_kernels.h"

namespace asr {

namespace {

constexpr int FWIN_THREADS = 256;
constexpr int FTAIL_THREADS = 256;
constexpr int FLOG_THREADS = 256;

// stream of window g: the last s with first <= g; streams without windows share their successor's value and are never
// the last
__device__ __forceinline__ int stream_of_window(const FollowStreamRec *__restrict__ recs, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// element (row b, column c) of [tail | new] of stream R; the tail counts as zeros while the stream has no columns
__device__ __forceinline__ float ext_elem(const FollowStreamWinArgs &a, const FollowStreamRec &R, int b, int64_t c) {
    const int t = a.width - 1;
    if (c < t) return R.has_tail ? a.tail[R.tail_off + (int64_t)b * t + c] : 0.0f;
    return a.cols[R.col_off + (int64_t)b * R.n_new + (c - t)];
}

__global__ __launch_bounds__(FWIN_THREADS) void follow_stream_window_kernel(FollowStreamWinArgs a, int vec4) {
    const int64_t g = blockIdx.x;
    if (g >= a.total_win) return;
    const FollowStreamRec R = a.recs[stream_of_window(a.recs, a.n_streams, g)];
    const int64_t i = g - R.first;
    if (i < 0 || i >= R.n_win) return;
    const int64_t c = R.c0 + i * a.step;                      // the window's first column within [tail | new]
    if (c < 0 || c + a.width > (int64_t)(a.width - 1) + R.n_new) return;
    const uint32_t w = (uint32_t)a.width, n = (uint32_t)a.bins * w;
    float *out = a.win + g * (int64_t)n;
    if (vec4) {                                               // n % 4 == 0 and win 16-byte aligned: the host checked
        for (uint32_t e = threadIdx.x * 4u; e < n; e += FWIN_THREADS * 4u) {
            float v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t b = (e + k) / w, j = (e + k) - b * w;
                v[k] = ext_elem(a, R, (int)b, c + j);
            }
            *reinterpret_cast<float4 *>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (uint32_t e = threadIdx.x; e < n; e += FWIN_THREADS) {
            const uint32_t b = e / w, j = e - b * w;
            out[e] = ext_elem(a, R, (int)b, c + j);
        }
    }
}

__global__ __launch_bounds__(FTAIL_THREADS) void follow_stream_tail_kernel(FollowStreamWinArgs a) {
    if ((int)blockIdx.x >= a.n_streams) return;
    const FollowStreamRec R = a.recs[blockIdx.x];
    if (R.n_new <= 0) return;                                 // the whole workgroup: no barrier is left waiting
    const int t = a.width - 1;
    const int64_t n = (int64_t)a.bins * t;
    float *tail = a.tail + R.tail_off;
    for (int64_t base = 0; base < n; base += FTAIL_THREADS) {
        const int64_t e = base + threadIdx.x;
        float v = 0.0f;
        if (e < n) {
            const int b = (int)(e / t);
            v = ext_elem(a, R, b, (e - (int64_t)b * t) + R.n_new);
        }
        __syncthreads();                                      // every source of the chunk is read; later chunks' are ahead
        if (e < n) tail[e] = v;
    }
}

// dst[0 .. n) = src[0 .. n) for dst < src inside one buffer (the ranges may overlap): ascending chunks, a chunk's sources
// read before the barrier and the chunk written after it.  T = float or float4; n in units of T, the same in every thread.
template <typename T>
__device__ __forceinline__ void move_down(T *dst, const T *src, int64_t n) {
    for (int64_t base = 0; base < n; base += FLOG_THREADS) {
        const int64_t e = base + threadIdx.x;
        T v = T();
        if (e < n) v = src[e];
        __syncthreads();
        if (e < n) dst[e] = v;
    }
}

__global__ __launch_bounds__(FLOG_THREADS) void follow_stream_log_kernel(FollowStreamLogArgs a, int vec4) {
    if ((int)blockIdx.x >= a.n_streams) return;
    const FollowStreamLogRec R = a.recs[blockIdx.x];
    if (R.n_new <= 0) return;                                 // the whole workgroup: no barrier is left waiting
    if (R.kept < 0 || R.kept > R.rows_in_log || R.src_row < 0 || R.src_row + R.n_new > a.n_rows) return;
    const int64_t d = a.dim;
    float *log = a.log + R.log_off;
    const float *src = a.codes + R.src_row * d;
    const int64_t shift = (int64_t)(R.rows_in_log - R.kept) * d, n_keep = (int64_t)R.kept * d, n_copy = (int64_t)R.n_new * d;
    const bool v4 = vec4 && (R.log_off & 3) == 0;             // dim % 4 == 0 and both buffers aligned: the host checked
    if (shift > 0 && n_keep > 0) {
        if (v4) move_down(reinterpret_cast<float4 *>(log), reinterpret_cast<const float4 *>(log + shift), n_keep >> 2);
        else move_down(log, log + shift, n_keep);
    }
    __syncthreads();                                          // the old rows are read before new ones land on them
    if (v4) {
        float4 *dst = reinterpret_cast<float4 *>(log + n_keep);
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        for (int64_t e = threadIdx.x; e < (n_copy >> 2); e += FLOG_THREADS) dst[e] = s4[e];
    } else {
        for (int64_t e = threadIdx.x; e < n_copy; e += FLOG_THREADS) log[n_keep + e] = src[e];
    }
}

}  // namespace

hipError_t launch_follow_stream_windows(hipStream_t s, const FollowStreamWinArgs &a) {
    if (a.n_streams <= 0) return hipSuccess;
    const int vec4 = (((int64_t)a.bins * a.width) & 3) == 0 && ((uintptr_t)a.win & 15) == 0;
    if (a.total_win > 0) follow_stream_window_kernel<<<(int)a.total_win, FWIN_THREADS, 0, s>>>(a, vec4);
    follow_stream_tail_kernel<<<a.n_streams, FTAIL_THREADS, 0, s>>>(a);        // behind the readers of the old tails
    return hipGetLastError();
}

hipError_t launch_follow_stream_log(hipStream_t s, const FollowStreamLogArgs &a) {
    if (a.n_streams <= 0 || a.n_rows <= 0) return hipSuccess;
    const int vec4 = (a.dim & 3) == 0 && ((uintptr_t)a.log & 15) == 0 && ((uintptr_t)a.codes & 15) == 0;
    follow_stream_log_kernel<<<a.n_streams, FLOG_THREADS, 0, s>>>(a, vec4);
    return hipGetLastError();
}

}  // namespace asr
