// The arithmetic of one spectrogram frame, written down once: spectrogram_kernel and spectrogram_batch_kernel
// (piece_vote_kernels.hip) and audio_stream_frame_kernel (audio_stream_kernels.hip) all call spectrogram_frame, which is
// what makes the batched and the streamed result bit-identical with the single one.  Both files are compiled with the
// default flags: re * re + im * im and mul * s + add are contracted, the same way in either.
//
// The madmom chain of the reference (tutorials/Embedding Tutorial.ipynb cell 28; msmd.midi_parser.processor):
// FramedSignal(frame_size 2048, fps 20, origin 'future') -> |STFT| with a Hann window -> LogarithmicFilterbank
// (16 bands/octave, 30..6000 Hz: 92 triangular filters) -> log10(1 + x).  One workgroup per frame: windowed frame
// and a 2048-entry twiddle table in LDS, direct DFT of the bins the filterbank touches (<= 558 of 1024: 2.3 MFLOP
// per frame), magnitudes in LDS, filterbank + logarithm.  The loop runs at 8.5 TFLOP/s, 5 % of the fp32 rate: an FFT
// does pay (spectrogram_fft_kernels.hip computes the same frames about 55 times faster), but it sums in another order,
// so it is a route of its own (asr_spectrogram_fft_batch_dev) and this one stays what every bit-parity statement -
// single, batched, streamed - is about.
#pragma once
#include "asr_kernels.h"

namespace asr {

struct SpecArgs {
    const float *samples; int64_t n_samples;
    const float *window;            // [frame_size]
    int frame_size; double hop;
    int max_bin;                    // DFT bins 0 .. max_bin-1 are needed
    const int32_t *fb_start, *fb_len, *fb_off;   // per filter: first bin, number of bins, offset into fb_w
    const float *fb_w; int nf;
    float mul, add;
    float *out; int64_t n_frames; int transposed;      // out: (n_frames, nf) or (nf, n_frames)
};

// twiddle table of the workgroup: tc[t] = cos(2 pi t / F), ts[t] = sin(2 pi t / F)
__device__ __forceinline__ void spectrogram_twiddles(int F, float *tc, float *ts) {
    for (int t = threadIdx.x; t < F; t += 256) {
        double s, c;
        sincospi(2.0 * (double)t / (double)F, &s, &c);
        tc[t] = (float)c; ts[t] = (float)s;
    }
}

// frame `frame` of one recording by the whole workgroup.  The recording has n_samples samples, of which `samples` holds
// those from index `origin` on (origin 0: the whole recording; the stream hands over the frame's own samples in LDS);
// the frame is written as column / row `col` of an output of n_frames frames at out (the recording's own: col == frame).
// The workgroup computes the filters f0 .. f1-1 and the DFT bins k0 .. k1-1, which must cover what those filters read
// (all of them: 0, a.nf, 0, a.max_bin; the stream splits a frame's filters over several workgroups).  A bin is summed by
// one lane in the same order whichever workgroup takes it, so the split does not change a bit.
__device__ __forceinline__ void spectrogram_frame(const SpecArgs &a, const float *__restrict__ samples, int64_t origin,
                                                  int64_t n_samples, int64_t frame, float *__restrict__ out, int64_t col,
                                                  int64_t n_frames, float *x, const float *tc, const float *ts,
                                                  float *mag, int f0, int f1, int k0, int k1) {
    const int F = a.frame_size;
    const int tid = threadIdx.x;
    const int64_t start = (int64_t)((double)frame * a.hop);        // int(index * hop_size), origin 'future'
    __syncthreads();
    for (int t = tid; t < F; t += 256) {
        const int64_t i = start + t;
        x[t] = (i < n_samples ? samples[i - origin] : 0.0f) * a.window[t];
    }
    __syncthreads();
    for (int k = k0 + tid; k < k1; k += 256) {
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int n = 0; n < F; ++n) {
            re = fmaf(x[n], tc[idx], re);
            im = fmaf(-x[n], ts[idx], im);
            idx = (idx + k) & (F - 1);                              // (k * n) mod F, F a power of two
        }
        mag[k] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    for (int f = f0 + tid; f < f1; f += 256) {
        const float *w = a.fb_w + a.fb_off[f];
        const int b0 = a.fb_start[f];
        float s = 0.0f;
        for (int q = 0; q < a.fb_len[f]; ++q) s = fmaf(mag[b0 + q], w[q], s);
        const float v = log10f(a.mul * s + a.add);
        if (a.transposed) out[(int64_t)f * n_frames + col] = v;
        else out[col * a.nf + f] = v;
    }
}

}  // namespace asr
