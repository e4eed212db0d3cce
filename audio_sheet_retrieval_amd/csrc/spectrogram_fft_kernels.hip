// asr_spectrogram_fft_batch_dev: the spectrograms of asr_spectrogram_batch_dev with the magnitudes taken from a real-input
// FFT instead of the direct DFT of spectrogram_frame.h (4.5 MFLOP per frame there, 57 kFLOP here).  frame_size is
// 2048, the reference's only value.  include/asr_hip.h carries the contract; audio_frontend.spectrogram_fft_host restates
// the plan below in numpy.
//
// Plan of one frame (one 256-thread workgroup per frame, grid-stride over the frames of all recordings; the
// frame-to-recording lookup is spectrogram_batch_kernel's):
//   packing    z[n] = x[2n] * window[2n] + i * x[2n + 1] * window[2n + 1], n = 0 .. 1023; samples past the end of the frame's
//              own recording read as zero.  Lane t loads z[t + 256 k], k = 0 .. 3, straight into registers: two scalar
//              loads per value, so any alignment of the frame's start (odd offsets, odd starts) is as good as another,
//              and neighbouring lanes still share their cache lines.
//   passes     Z = FFT_1024(z) by five radix-4 Stockham passes (autosort: natural order in, natural order out).  Pass
//              j = 0 .. 4 has stride S = 4^j and sub-length n = 1024 / S: lane t = q + S p (q < S) takes
//              v[k] = in[t + 256 k], forms
//                  y0 = (v0 + v2) + (v1 + v3)                y2 = w^2p ((v0 + v2) - (v1 + v3))
//                  y1 = w^p ((v0 - v2) - i (v1 - v3))        y3 = w^3p ((v0 - v2) + i (v1 - v3)),   w = exp(-2 pi i / n)
//              and writes out[q + S (4 p + k)] = y_k.  The last pass has p = 0: no multiplications.
//   post-pass  X[k] = (Z[k] + conj Z[1024 - k]) / 2 - i W^k (Z[k] - conj Z[1024 - k]) / 2, W = exp(-2 pi i / 2048),
//              k = 0 .. 1023 (Z[1024] = Z[0]); mag[k] = 0.5 * sqrt(re^2 + im^2) of twice that.
//   then       the filterbank loop and log10f(mul * s + add) of spectrogram_frame, unchanged.
// Twiddles: one table tw[t] = exp(-2 pi i t / 2048), t = 0 .. 2047, float32 rounded from float64, computed once on the
// host (asr_api_umc.hip) and kept in the context's workspace.  w^(p k) of a pass is tw[2 S p k], W^k is tw[k]; which
// entries a lane needs depends on its number only, so it reads its 16 twiddles and 8 window values once and keeps them in
// registers for all its frames.
// LDS: two buffers of complex values that the passes write alternately (one barrier per pass), and the magnitudes.  A
// pass always reads in[t + 256 k]: consecutive lanes, consecutive 8-byte values.  Its writes are strided: with stride
// S = 1 or 4 sixteen consecutive lanes of a ds_write_b64 would meet 4 of the 16 eight-byte bank pairs (4-way conflicts),
// so the value with index i lies at i + (i >> 4) after the first pass and at i + (i >> 2) after the second (16 lanes,
// 16 bank pairs; the reads of the next pass then take 2 cycles per 32 lanes instead of 1); from S = 16 on the plain
// layout is conflict-free both ways.
// Flags: the file is built with the default flags (-ffp-contract=fast), as spectrogram_frame.h's users are.  Contraction
// is decided at compile time, every frame runs the same instructions on its own 2048 samples and no sum crosses a frame,
// so a recording's result cannot depend on the batch, its order or `transposed` with either setting;
// -ffp-contract=off would only add roundings to the complex products.
// The passes, the post-pass and the filterbank are in spectrogram_fft_frame.h, which the streamed route
// (audio_stream_fft_kernels.hip) includes too.
#include "asr_kernels.h"
#include "spectrogram_fft_frame.h"      // the frame body: fft_lane_tables, fft_frame_magnitudes, fft_frame_filterbank

namespace asr {

struct SpecFftArgs {
    const float *samples;                           // base of the concatenated recordings
    const int64_t *frame_first, *sample_off, *sample_cnt, *out_off;    // as SpecBatchArgs (piece_vote_kernels.hip)
    int n_rec; int64_t total_frames;
    const float2 *tw;                               // [2048] exp(-2 pi i t / 2048)
    const float2 *window;                           // [1024] pairs window[2n], window[2n + 1]
    double hop;
    const int32_t *fb_start, *fb_len, *fb_off; const float *fb_w; int nf;
    float mul, add;
    float *out; int transposed;
};

__global__ __launch_bounds__(256) void spectrogram_fft_batch_kernel(SpecFftArgs a) {
    __shared__ float2 buf_a[FFT_BUF], buf_b[FFT_BUF];
    __shared__ float mag[1024];
    const int tid = threadIdx.x;
    FftLane l;                                  // the lane's 8 window values and 16 twiddles, kept for all its frames
    fft_lane_tables(l, a.tw, a.window, tid);
    for (int64_t g = blockIdx.x; g < a.total_frames; g += gridDim.x) {
        int lo = 0, hi = a.n_rec - 1;                               // last r with frame_first[r] <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.frame_first[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const int64_t n_frames = a.frame_first[lo + 1] - a.frame_first[lo];
        const int64_t frame = g - a.frame_first[lo];
        const float *__restrict__ samples = a.samples + a.sample_off[lo];
        const int64_t n_samples = a.sample_cnt[lo];
        float *__restrict__ out = a.out + a.out_off[lo];
        const int64_t start = (int64_t)((double)frame * a.hop);    // int(index * hop_size), origin 'future'
        float2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = start + 2 * (tid + 256 * k);
            const float x0 = i < n_samples ? samples[i] : 0.0f;
            const float x1 = i + 1 < n_samples ? samples[i + 1] : 0.0f;
            v[k] = make_float2(x0 * l.win[k].x, x1 * l.win[k].y);
        }
        fft_frame_magnitudes(v, l, buf_a, buf_b, mag, tid);
        fft_frame_filterbank(mag, a.fb_start, a.fb_len, a.fb_off, a.fb_w, a.nf, a.mul, a.add, out, n_frames, frame,
                             a.transposed, tid);
        // the next frame writes buf_a before its first barrier and mag after its fifth: buf_a was last read before the
        // last barrier of fft_frame_magnitudes, mag is read here - no further barrier needed
    }
}

hipError_t launch_spectrogram_fft_batch(hipStream_t s, const float *samples, const int64_t *frame_first,
                                        const int64_t *sample_off, const int64_t *sample_cnt, const int64_t *out_off,
                                        int n_rec, int64_t total_frames, const float *twiddles, const float *window,
                                        double hop, const int32_t *fb_start, const int32_t *fb_len, const int32_t *fb_off,
                                        const float *fb_w, int nf, float mul, float add, float *out, int transposed) {
    if (total_frames == 0 || n_rec == 0) return hipSuccess;
    SpecFftArgs a{samples, frame_first, sample_off, sample_cnt, out_off, n_rec, total_frames, (const float2 *)twiddles,
                  (const float2 *)window, hop, fb_start, fb_len, fb_off, fb_w, nf, mul, add, out, transposed};
    const int grid = (int)std::min<int64_t>(total_frames, 2048);
    hipLaunchKernelGGL(spectrogram_fft_batch_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace asr
