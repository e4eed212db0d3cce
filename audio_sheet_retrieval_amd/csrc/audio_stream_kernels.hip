// Spectrogram columns from streamed audio blocks (asr_audio_stream_push_dev; include/asr_hip.h carries the definition):
// per stream the call gets a block of new input samples, and a range of a caller-owned device buffer carries the input
// samples the frames not yet emitted still read (the "state").
//
//   audio_stream_frame_kernel : one 256-thread workgroup per new frame of all streams (frame_first[s] = number of the
//                               first new frame of stream s, n_streams + 1 entries; the stream is found by binary search,
//                               as spectrogram_batch_kernel finds its recording).  The workgroup stages the input span of
//                               its frame in LDS from the logical concatenation [state | block] - zeros outside
//                               [keep0, n1) - resamples the frame's frame_size samples at the front-end's rate into LDS
//                               with resample_batch_kernel's arithmetic, and runs spectrogram_frame on them.  Overlapping
//                               frames resample the samples they share once each: that buys one carried buffer (inputs)
//                               instead of two (inputs and resampled samples) and one launch fewer per block.
//                               When a call has fewer frames than the device has CUs, a frame's filters are split over
//                               parts.n workgroups (StreamParts: filters f[p] .. f[p + 1] - 1 and the DFT bins they read);
//                               each repeats the staging and the resampling and computes its own bins - at most about
//                               one bin per lane instead of three for the product's frames.  A bin is summed by one lane
//                               in the same order wherever it is computed: no bit changes.
//   audio_stream_carry_kernel : one workgroup per stream slides the inputs the next frame reads, [state | block] from
//                               keep1 on, to the front of the state.  keep1 >= keep0, so a destination index is never
//                               above its source index: an ascending copy, chunk by chunk, every chunk read completely
//                               (into registers), then a barrier, then written.  It runs after the frame kernel on the
//                               same stream.
//
// The staging and the resampling are audio_stream_stage.h's, shared with the FFT route of the stream
// (audio_stream_fft_kernels.hip); the note on the flags of the resampler's sum is there.  This file is built with the
// default flags, as piece_vote_kernels.hip is (spectrogram_frame's re * re + im * im and mul * s + add are contracted
// there, and the stream has to reproduce those bits).
//
// LDS of the frame kernel, in floats: [ max(3 * frame_size, span) | frame_size | max_bin ].  The staged inputs (span) share
// their place with the windowed frame and the twiddle table, which are written after the resampling is done.
#include "asr_kernels.h"
#include "audio_stream_stage.h"
#include "spectrogram_frame.h"

namespace asr {

template <bool UP1>
__global__ __launch_bounds__(256) void audio_stream_frame_kernel(SpecArgs a, const float *__restrict__ blocks,
                                                                 const float *__restrict__ state,
                                                                 const int64_t *__restrict__ frame_first,
                                                                 const StreamRow *__restrict__ rows, int n_streams,
                                                                 StreamResample r, StreamParts parts) {
    extern __shared__ __attribute__((aligned(16))) float sl[];
    const int F = a.frame_size;
    const int head = 3 * F > r.span ? 3 * F : r.span;
    float *x = sl, *tc = sl + F, *ts = sl + 2 * F, *xs = sl, *ys = sl + head, *mag = ys + F;
    const int64_t g = blockIdx.x / parts.n;                         // the frame; the workgroup takes part blockIdx.x % n of it
    const int part = blockIdx.x % parts.n;
    const int lo = stream_of_frame(frame_first, n_streams, g);
    const StreamRow w = rows[lo];
    const int64_t col = g - frame_first[lo];
    const int64_t frame = w.first_frame + col;
    const int64_t start = (int64_t)((double)frame * a.hop);        // spectrogram_frame's
    stream_resample_frame<UP1>(w, state + w.state_off, blocks + w.block_off, start, F, r, xs, ys);
    // xs is read no more: the twiddles take its place
    spectrogram_twiddles(F, tc, ts);
    spectrogram_frame(a, ys, start, start + F, frame, a.out + w.out_off, col, w.n_new, x, tc, ts, mag, parts.f[part],
                      parts.f[part + 1], parts.k0[part], parts.k1[part]);
}

constexpr int CARRY_PER = 8;

__global__ __launch_bounds__(256) void audio_stream_carry_kernel(const float *__restrict__ blocks, float *state,
                                                                 const StreamRow *__restrict__ rows) {
    const StreamRow w = rows[blockIdx.x];
    if (w.n1 == w.n0 && w.keep1 == w.keep0) return;                // nothing arrived, nothing emitted
    const int64_t len = w.n1 - w.keep1;
    float *st = state + w.state_off;
    const float *bl = blocks + w.block_off;
    for (int64_t c0 = 0; c0 < len; c0 += 256 * CARRY_PER) {
        float v[CARRY_PER];
#pragma unroll
        for (int k = 0; k < CARRY_PER; ++k) {
            const int64_t d = c0 + threadIdx.x + 256 * k;
            const int64_t j = w.keep1 + d;
            v[k] = d < len ? (j < w.n0 ? st[j - w.keep0] : bl[j - w.n0]) : 0.0f;
        }
        // the chunk's sources lie at or above its destinations, and above every destination of the chunks before it
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CARRY_PER; ++k) {
            const int64_t d = c0 + threadIdx.x + 256 * k;
            if (d < len) st[d] = v[k];
        }
    }
}

int audio_stream_span(int frame_size, int up, int down, int taps_per_phase) {
    return (int)(((int64_t)(frame_size - 1) * down + up - 1) / up) + taps_per_phase;
}

size_t audio_stream_lds(int frame_size, int max_bin, int span) {
    return ((size_t)std::max(3 * frame_size, span) + frame_size + max_bin) * sizeof(float);
}

hipError_t launch_audio_stream_frames(hipStream_t s, const float *blocks, const float *state, const int64_t *frame_first,
                                      const StreamRow *rows, int n_streams, int64_t total_frames, const StreamResample &r,
                                      const StreamParts &parts, const float *window, int frame_size, double hop, int max_bin,
                                      const int32_t *fb_start, const int32_t *fb_len, const int32_t *fb_off,
                                      const float *fb_w, int nf, float mul, float add, float *out, int transposed) {
    if (total_frames == 0 || n_streams == 0) return hipSuccess;
    const size_t lds = audio_stream_lds(frame_size, max_bin, r.span);
    if (lds > AUDIO_STREAM_MAX_LDS || parts.n < 1 || parts.n > STREAM_MAX_PARTS || total_frames * parts.n > 0x7fffffffLL)
        return hipErrorInvalidValue;
    SpecArgs a{nullptr, 0, window, frame_size, hop, max_bin, fb_start, fb_len, fb_off, fb_w, nf, mul, add, out, 0, transposed};
    const void *fn = r.up == 1 ? reinterpret_cast<const void *>(audio_stream_frame_kernel<true>)
                               : reinterpret_cast<const void *>(audio_stream_frame_kernel<false>);
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AUDIO_STREAM_MAX_LDS);
    if (r.up == 1)
        hipLaunchKernelGGL(audio_stream_frame_kernel<true>, dim3((unsigned)(total_frames * parts.n)), dim3(256), lds, s, a,
                           blocks, state, frame_first, rows, n_streams, r, parts);
    else
        hipLaunchKernelGGL(audio_stream_frame_kernel<false>, dim3((unsigned)(total_frames * parts.n)), dim3(256), lds, s, a,
                           blocks, state, frame_first, rows, n_streams, r, parts);
    return hipGetLastError();
}

hipError_t launch_audio_stream_carry(hipStream_t s, const float *blocks, float *state, const StreamRow *rows,
                                     int n_streams) {
    if (n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(audio_stream_carry_kernel, dim3((unsigned)n_streams), dim3(256), 0, s, blocks, state, rows);
    return hipGetLastError();
}

}  // namespace asr
