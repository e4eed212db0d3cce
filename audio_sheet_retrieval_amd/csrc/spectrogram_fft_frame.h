// The FFT plan of one spectrogram frame, written down once: spectrogram_fft_batch_kernel (spectrogram_fft_kernels.hip)
// and audio_stream_fft_frame_kernel (audio_stream_fft_kernels.hip) both run fft_frame_magnitudes and
// fft_frame_filterbank on a frame's 1024 packed values, which is what makes the streamed FFT columns bit-identical with
// the batched ones.  Both files are compiled with the default flags (-ffp-contract=fast): the complex products, the
// re * re + im * im of the magnitudes and mul * s + add are contracted, the same way in either.  The plan itself -
// packing, five radix-4 Stockham passes, post-pass, the padded LDS layouts - is described at the top of
// spectrogram_fft_kernels.hip.
#pragma once
#include "asr_kernels.h"

namespace asr {

constexpr int FFT_BUF = 1024 + 256;      // complex values per buffer: 1024 and the padding of i + (i >> 2)

template <int SH> __device__ __forceinline__ int fft_pad(int i) { return SH ? i + (i >> SH) : i; }

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// one radix-4 pass of lane tid on v (in[tid + 256 k]); stride S = 1 << LOG_S; the results go to dst, value i at
// fft_pad<PAD>(i)
template <int LOG_S, int PAD>
__device__ __forceinline__ void fft_pass(const float2 (&v)[4], const float2 *w, float2 *dst, int tid) {
    constexpr int S = 1 << LOG_S;
    const float2 apc = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), amc = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 bpd = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), bmd = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
    float2 y0 = make_float2(apc.x + bpd.x, apc.y + bpd.y);
    float2 y1 = make_float2(amc.x + bmd.y, amc.y - bmd.x);          // (v0 - v2) - i (v1 - v3)
    float2 y2 = make_float2(apc.x - bpd.x, apc.y - bpd.y);
    float2 y3 = make_float2(amc.x - bmd.y, amc.y + bmd.x);          // (v0 - v2) + i (v1 - v3)
    if (S < 256) {
        y1 = cmul(y1, w[0]); y2 = cmul(y2, w[1]); y3 = cmul(y3, w[2]);
    }
    const int base = (tid & (S - 1)) + 4 * S * (tid >> LOG_S);
    dst[fft_pad<PAD>(base)] = y0;
    dst[fft_pad<PAD>(base + S)] = y1;
    dst[fft_pad<PAD>(base + 2 * S)] = y2;
    dst[fft_pad<PAD>(base + 3 * S)] = y3;
}

template <int PAD> __device__ __forceinline__ void fft_read(float2 (&v)[4], const float2 *src, int tid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = src[fft_pad<PAD>(tid + 256 * k)];
}

// what depends on the lane only: its window values, the twiddles of the four multiplying passes and of the post-pass.
// tw: [2048] exp(-2 pi i t / 2048); window: [1024] pairs window[2n], window[2n + 1]
struct FftLane { float2 win[4], w0[3], w1[3], w2[3], w3[3], wp[4]; };

__device__ __forceinline__ void fft_lane_tables(FftLane &l, const float2 *__restrict__ tw,
                                                const float2 *__restrict__ window, int tid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        l.win[k] = window[tid + 256 * k];
        l.wp[k] = tw[tid + 256 * k];
    }
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        l.w0[k - 1] = tw[2 * tid * k];                  // S = 1:  p = tid,      2 S p k <= 1530
        l.w1[k - 1] = tw[8 * (tid >> 2) * k];           // S = 4:  p = tid / 4
        l.w2[k - 1] = tw[32 * (tid >> 4) * k];          // S = 16: p = tid / 16
        l.w3[k - 1] = tw[128 * (tid >> 6) * k];         // S = 64: p = tid / 64
    }
}

// v[k] = z[tid + 256 k], the frame's packed and windowed values, by the whole workgroup -> mag[0 .. 1023] in LDS, visible
// to every lane on return.  buf_a, buf_b: FFT_BUF values each.  Neither buffer is read before the first barrier inside,
// mag is not written before the fifth.
__device__ __forceinline__ void fft_frame_magnitudes(float2 (&v)[4], const FftLane &l, float2 *buf_a, float2 *buf_b,
                                                     float *mag, int tid) {
    fft_pass<0, 4>(v, l.w0, buf_a, tid);
    __syncthreads();
    fft_read<4>(v, buf_a, tid);
    fft_pass<2, 2>(v, l.w1, buf_b, tid);
    __syncthreads();
    fft_read<2>(v, buf_b, tid);
    fft_pass<4, 0>(v, l.w2, buf_a, tid);
    __syncthreads();
    fft_read<0>(v, buf_a, tid);
    fft_pass<6, 0>(v, l.w3, buf_b, tid);
    __syncthreads();
    fft_read<0>(v, buf_b, tid);
    fft_pass<8, 0>(v, l.w3, buf_a, tid);                            // p = 0: the twiddles are not used
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int k = tid + 256 * m;
        const float2 zk = buf_a[k], zn = buf_a[(1024 - k) & 1023];
        const float2 s = make_float2(zk.x + zn.x, zk.y - zn.y);             // Z[k] + conj Z[N - k]
        const float2 t = cmul(make_float2(zk.x - zn.x, zk.y + zn.y), l.wp[m]);  // W^k (Z[k] - conj Z[N - k])
        const float re = s.x + t.y, im = s.y - t.x;                         // ... - i t
        mag[k] = 0.5f * sqrtf(re * re + im * im);
    }
    __syncthreads();
}

// the filterbank and the logarithm of spectrogram_frame on mag; the frame is written as column / row `col` of an output
// of n_frames frames at out
__device__ __forceinline__ void fft_frame_filterbank(const float *mag, const int32_t *__restrict__ fb_start,
                                                     const int32_t *__restrict__ fb_len,
                                                     const int32_t *__restrict__ fb_off, const float *__restrict__ fb_w,
                                                     int nf, float mul, float add, float *__restrict__ out,
                                                     int64_t n_frames, int64_t col, int transposed, int tid) {
    for (int f = tid; f < nf; f += 256) {
        const float *w = fb_w + fb_off[f];
        const int b0 = fb_start[f];
        float s = 0.0f;
        for (int q = 0; q < fb_len[f]; ++q) s = fmaf(mag[b0 + q], w[q], s);
        const float r = log10f(mul * s + add);
        if (transposed) out[(int64_t)f * n_frames + col] = r;
        else out[col * nf + f] = r;
    }
}

}  // namespace asr
