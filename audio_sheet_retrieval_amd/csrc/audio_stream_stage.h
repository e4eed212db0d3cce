// The first stage of a streamed frame, written down once: audio_stream_frame_kernel (audio_stream_kernels.hip, the direct
// DFT) and audio_stream_fft_frame_kernel (audio_stream_fft_kernels.hip, the FFT) both find their stream with
// stream_of_frame and resample the frame's frame_size samples into LDS with stream_resample_frame - the arithmetic of
// resample_batch_kernel on the logical concatenation [state | block].
//
// The sum of a resampled sample starts at 0.0 and runs over t = 0 .. T-1 in ascending order, one rounding per product and
// one per sum.  Both users are built with the default flags (the frame arithmetic behind this stage is contracted, and
// the stream has to reproduce those bits), so the loop of the sum alone is compiled under `#pragma clang fp contract(off)`.
// (__dmul_rn / __dadd_rn would not do: this toolchain defines them as plain `*` and `+`, which the default flags fuse
// into v_fmac_f64, and a float64 tap times a float32 sample is not exact in float64.)  Every index product is int64.
#pragma once
#include "asr_kernels.h"

namespace asr {

__device__ __forceinline__ float stream_input(const StreamRow &w, const float *st, const float *bl, int64_t j) {
    if (j < w.keep0 || j >= w.n1) return 0.0f;                     // keep0 >= 0: also every index before the stream
    return j < w.n0 ? st[j - w.keep0] : bl[j - w.n0];
}

// the stream of new frame g of the call: the last s with frame_first[s] <= g (n_streams + 1 running frame counts), as
// spectrogram_batch_kernel finds its recording
__device__ __forceinline__ int stream_of_frame(const int64_t *__restrict__ frame_first, int n_streams, int64_t g) {
    int lo = 0, hi = n_streams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// samples start .. start + F - 1 of stream w at the front-end's rate -> ys[0 .. F), by the whole 256-thread workgroup.
// xs: r.span floats of LDS for the staged inputs (not touched at the front-end's own rate); st / bl: the stream's state
// and block.  On return every lane sees ys and xs is free for other use.
template <bool UP1>
__device__ __forceinline__ void stream_resample_frame(const StreamRow &w, const float *__restrict__ st,
                                                      const float *__restrict__ bl, int64_t start, int F,
                                                      const StreamResample &r, float *xs, float *ys) {
    constexpr int PER = 4;
    const int T = r.taps_per_phase;
    if (!r.taps) {                                                  // the front-end's own rate: y = x
        for (int t = threadIdx.x; t < F; t += 256) ys[t] = stream_input(w, st, bl, start + t);
    } else {
        const int64_t base = (start * r.down + r.half) / r.up - (T - 1);   // first input the frame's first sample reads
        for (int i = threadIdx.x; i < r.span; i += 256) xs[i] = stream_input(w, st, bl, base + i);
        __syncthreads();
        for (int t0 = 0; t0 < F; t0 += 256 * PER) {
            int rel[PER];                                           // j0 - base of the lane's samples
            const double *tp[PER];
            double acc[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                // samples past the end of the frame are computed on its last one and not stored
                const int t = min(t0 + (int)threadIdx.x + 256 * k, F - 1);
                const int64_t c = (start + t) * r.down + r.half;
                rel[k] = (int)(c / r.up - base);
                tp[k] = UP1 ? r.taps : r.taps + (c % r.up) * T;
                acc[k] = 0.0;
            }
            for (int t = 0; t < T; ++t) {
#pragma clang fp contract(off)
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const double prod = tp[k][t] * (double)xs[rel[k] - t];
                    acc[k] = acc[k] + prod;
                }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int t = t0 + (int)threadIdx.x + 256 * k;
                if (t >= F) continue;
                double v = acc[k];
                if (r.round_int16) {                                // np.clip(np.rint(v), -32768, 32767): a NaN stays one
                    v = rint(v);
                    v = v < -32768.0 ? -32768.0 : v;
                    v = v > 32767.0 ? 32767.0 : v;
                }
                ys[t] = start + t < w.y_len ? (float)v : 0.0f;      // the recording ends at y_len: zeros from there on
            }
        }
    }
    __syncthreads();                                                // ys is complete; xs is read no more
}

}  // namespace asr
