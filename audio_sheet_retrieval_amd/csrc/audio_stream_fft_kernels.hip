// Spectrogram columns from streamed audio blocks with the magnitudes from the real-input FFT
// (asr_audio_stream_push_fft_dev; include/asr_hip.h carries the contract): the stream of audio_stream_kernels.hip with
// the frame plan of spectrogram_fft_kernels.hip in place of spectrogram_frame's direct DFT.  frame_size is 2048.
//
//   audio_stream_fft_frame_kernel : one 256-thread workgroup per new frame of all streams, found by stream_of_frame.
//       stage 1  stream_resample_frame (audio_stream_stage.h): the frame's input span from [state | block] into LDS,
//                its 2048 samples at the front-end's rate into LDS - what audio_stream_frame_kernel does, bit for bit
//                what asr_resample_batch_dev gives for those samples.
//       stage 2  lane t packs z[t + 256 k] = ys[2n] * window[2n] + i ys[2n + 1] * window[2n + 1], n = t + 256 k, from
//                LDS and runs fft_frame_magnitudes and fft_frame_filterbank (spectrogram_fft_frame.h): the instructions
//                of spectrogram_fft_batch_kernel on the same 2048 values, so the column has the bits of
//                asr_spectrogram_fft_batch_dev's.  A sample past the end of the recording is a zero in ys here and a zero
//                selected at the load there; both are multiplied by the window value.
//   The state is slid by audio_stream_carry_kernel (audio_stream_kernels.hip) as for the direct stream: it holds input
//   samples, and the plan and state_cap do not depend on how the frame is transformed.
//
// A frame is one workgroup whatever the number of frames in the call: the FFT leaves about 57 kFLOP per frame, nothing
// that a split over workgroups (StreamParts of the direct kernel) could shorten.  The lane's 8 window values and 16
// twiddles are loaded before the resampling, so their latency is hidden behind it.
//
// LDS, in floats: [ max(span, 4 * FFT_BUF) | 2048 ].  The staged inputs (span) share their place with the two FFT buffers,
// which are written after the resampling is done (the barrier that ends stream_resample_frame); the resampled samples
// share theirs with the 1024 magnitudes, which are written after the fifth barrier of the passes, when every lane has
// packed its samples into registers (before the first).  That is never more than the direct kernel's
// max(3 * 2048, span) + 2048 + max_bin, so every ratio the direct stream takes fits here.
//
// Flags: the default ones, as for spectrogram_fft_kernels.hip - the shared frame body is contracted the same way in
// both files; the resampler's sum carries its own `#pragma clang fp contract(off)`.
#include "asr_kernels.h"
#include "audio_stream_stage.h"
#include "spectrogram_fft_frame.h"

namespace asr {

struct StreamFftArgs {
    const float2 *tw;                               // [2048] exp(-2 pi i t / 2048)
    const float2 *window;                           // [1024] pairs window[2n], window[2n + 1]
    double hop;
    const int32_t *fb_start, *fb_len, *fb_off; const float *fb_w; int nf;
    float mul, add;
    float *out; int transposed;
};

constexpr int STREAM_FFT_FRAME = 2048;

template <bool UP1>
__global__ __launch_bounds__(256) void audio_stream_fft_frame_kernel(StreamFftArgs a, const float *__restrict__ blocks,
                                                                     const float *__restrict__ state,
                                                                     const int64_t *__restrict__ frame_first,
                                                                     const StreamRow *__restrict__ rows, int n_streams,
                                                                     StreamResample r) {
    extern __shared__ __attribute__((aligned(16))) float sl[];
    constexpr int F = STREAM_FFT_FRAME;
    const int tid = threadIdx.x;
    const int head = 4 * FFT_BUF > r.span ? 4 * FFT_BUF : r.span;
    float *xs = sl, *ys = sl + head, *mag = ys;
    float2 *buf_a = (float2 *)sl, *buf_b = buf_a + FFT_BUF;
    FftLane l;
    fft_lane_tables(l, a.tw, a.window, tid);
    const int64_t g = blockIdx.x;
    const int lo = stream_of_frame(frame_first, n_streams, g);
    const StreamRow w = rows[lo];
    const int64_t col = g - frame_first[lo];
    const int64_t start = (int64_t)((double)(w.first_frame + col) * a.hop);    // int(index * hop_size), origin 'future'
    stream_resample_frame<UP1>(w, state + w.state_off, blocks + w.block_off, start, F, r, xs, ys);
    float2 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = 2 * (tid + 256 * k);
        v[k] = make_float2(ys[n] * l.win[k].x, ys[n + 1] * l.win[k].y);
    }
    fft_frame_magnitudes(v, l, buf_a, buf_b, mag, tid);
    fft_frame_filterbank(mag, a.fb_start, a.fb_len, a.fb_off, a.fb_w, a.nf, a.mul, a.add, a.out + w.out_off, w.n_new, col,
                         a.transposed, tid);
}

size_t audio_stream_fft_lds(int span) {
    return ((size_t)std::max(4 * FFT_BUF, span) + STREAM_FFT_FRAME) * sizeof(float);
}

hipError_t launch_audio_stream_fft_frames(hipStream_t s, const float *blocks, const float *state,
                                          const int64_t *frame_first, const StreamRow *rows, int n_streams,
                                          int64_t total_frames, const StreamResample &r, const float *twiddles,
                                          const float *window, double hop, const int32_t *fb_start, const int32_t *fb_len,
                                          const int32_t *fb_off, const float *fb_w, int nf, float mul, float add,
                                          float *out, int transposed) {
    if (total_frames == 0 || n_streams == 0) return hipSuccess;
    const size_t lds = audio_stream_fft_lds(r.span);
    if (r.span < 0 || lds > AUDIO_STREAM_MAX_LDS || total_frames > 0x7fffffffLL) return hipErrorInvalidValue;
    StreamFftArgs a{(const float2 *)twiddles, (const float2 *)window, hop, fb_start, fb_len, fb_off, fb_w, nf, mul, add,
                    out, transposed};
    const void *fn = r.up == 1 ? reinterpret_cast<const void *>(audio_stream_fft_frame_kernel<true>)
                               : reinterpret_cast<const void *>(audio_stream_fft_frame_kernel<false>);
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AUDIO_STREAM_MAX_LDS);
    if (r.up == 1)
        hipLaunchKernelGGL(audio_stream_fft_frame_kernel<true>, dim3((unsigned)total_frames), dim3(256), lds, s, a, blocks,
                           state, frame_first, rows, n_streams, r);
    else
        hipLaunchKernelGGL(audio_stream_fft_frame_kernel<false>, dim3((unsigned)total_frames), dim3(256), lds, s, a, blocks,
                           state, frame_first, rows, n_streams, r);
    return hipGetLastError();
}

}  // namespace asr
