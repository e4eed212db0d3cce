// Recordings at any sample rate to the front-end's rate (asr_resample_batch_dev; include/asr_hip.h carries the
// definition): a rational polyphase resampler, up / down in lowest terms, taps in float64, phase-major.
//
//   resample_batch_kernel : all recordings of one (up, down, integer) group in one launch.  The outputs of every recording
//                           are cut into tiles of RESAMPLE_TILE consecutive outputs, the tiles of all recordings are
//                           numbered through (tile_first[r] = number of the first tile of recording r, n_rec + 1
//                           entries), and one 256-thread workgroup takes one tile: it finds its recording by binary
//                           search (as spectrogram_batch_kernel does for frames), stages the input span the tile reads
//                           in LDS - zeros outside the recording, so the inner loop has no range test; a zero product
//                           leaves a float64 sum as it is - and every lane computes RESAMPLE_TILE / 256 outputs, 256
//                           apart, so that the stores of a wave are consecutive floats.
//
// The sum of an output starts at 0.0 and runs over t = 0 .. T-1 in ascending order, one rounding per product and one per
// sum (the file is built with -ffp-contract=off): the numpy restatement audio_frontend.resample_host computes the same
// bits.  Every index product is int64: m * down passes 2^31 within the first hour of a 96 kHz recording.
//
// The taps stay in global memory (phase p at taps + p * T): 520 bytes at 44.1 kHz, 82 KB at 48 kHz, read-only and
// resident in L2.  With up == 1 there is one phase, the tap address is the same in every lane and the compiler reads the
// tap through the scalar cache (UP1 = true); otherwise every output has its own phase and its lane gathers.
#include "asr_kernels.h"

namespace asr {

template <bool UP1>
__global__ __launch_bounds__(256) void resample_batch_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                             const int64_t *__restrict__ tile_first,
                                                             const int64_t *__restrict__ in_off,
                                                             const int64_t *__restrict__ in_cnt,
                                                             const int64_t *__restrict__ out_off,
                                                             const int64_t *__restrict__ out_cnt, int n_rec, int up,
                                                             int down, int half, int T, int span,
                                                             const double *__restrict__ taps, int round_int16) {
    extern __shared__ __attribute__((aligned(16))) float xs[];      // `span` samples from input index `base` on
    constexpr int PER = RESAMPLE_TILE / 256;
    const int64_t g = blockIdx.x;
    int lo = 0, hi = n_rec - 1;                                     // last r with tile_first[r] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int64_t n_in = in_cnt[lo], n_out = out_cnt[lo];
    const float *x = in + in_off[lo];
    float *y = out + out_off[lo];
    const int64_t m0 = (g - tile_first[lo]) * RESAMPLE_TILE;        // first output of the tile
    const int64_t base = (m0 * down + half) / up - (T - 1);         // first input sample any output of the tile reads
    for (int i = threadIdx.x; i < span; i += 256) {
        const int64_t j = base + i;
        xs[i] = (j >= 0 && j < n_in) ? x[j] : 0.0f;
    }
    __syncthreads();
    int rel[PER];                                                   // j0 - base of the lane's outputs
    const double *tp[PER];
    double acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        // outputs past the end of the recording are computed on the tile's last valid one and not stored: their reads
        // stay inside the staged span
        const int64_t m = min(m0 + threadIdx.x + 256 * k, n_out - 1);
        const int64_t c = m * down + half;
        rel[k] = (int)(c / up - base);
        tp[k] = UP1 ? taps : taps + (c % up) * T;
        acc[k] = 0.0;
    }
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const double prod = tp[k][t] * (double)xs[rel[k] - t];
            acc[k] = acc[k] + prod;
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t m = m0 + threadIdx.x + 256 * k;
        if (m >= n_out) continue;
        double v = acc[k];
        if (round_int16) {                                          // np.clip(np.rint(v), -32768, 32767): a NaN stays one
            v = rint(v);
            v = v < -32768.0 ? -32768.0 : v;
            v = v > 32767.0 ? 32767.0 : v;
        }
        y[m] = (float)v;
    }
}

int resample_span(int up, int down, int taps_per_phase) {
    return (int)(((int64_t)RESAMPLE_TILE * down + up - 1) / up) + taps_per_phase + 1;
}

hipError_t launch_resample_batch(hipStream_t s, const float *in, float *out, const int64_t *tile_first,
                                 const int64_t *in_off, const int64_t *in_cnt, const int64_t *out_off,
                                 const int64_t *out_cnt, int n_rec, int64_t total_tiles, int up, int down, int half,
                                 int taps_per_phase, const double *taps, int round_int16) {
    if (total_tiles == 0 || n_rec == 0) return hipSuccess;
    const int span = resample_span(up, down, taps_per_phase);
    const size_t lds = (size_t)span * sizeof(float);
    if (lds > RESAMPLE_MAX_LDS || total_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    if (up == 1)
        hipLaunchKernelGGL(resample_batch_kernel<true>, dim3((unsigned)total_tiles), dim3(256), lds, s, in, out, tile_first,
                           in_off, in_cnt, out_off, out_cnt, n_rec, up, down, half, taps_per_phase, span, taps, round_int16);
    else
        hipLaunchKernelGGL(resample_batch_kernel<false>, dim3((unsigned)total_tiles), dim3(256), lds, s, in, out, tile_first,
                           in_off, in_cnt, out_off, out_cnt, n_rec, up, down, half, taps_per_phase, span, taps, round_int16);
    return hipGetLastError();
}

}  // namespace asr
