// gfx950 kernels of the music gate at the level of what has been heard so far (asr_track_gate_running_dev,
// asr_track_stream_gate_running_dev): _detect_music (audio_sheet_server.py:524-528) divides by the maximum column sum of
// the finished spectrogram, which a live stream does not have; here frame i is gated with
//     level_i = fmaxf(floor, max{ c_j : max(0, i - L + 1) <= j <= i })        (L = memory; 0: every j <= i)
// A sequence (a recording, or the round of one stream) is ext = [carried column sums in frame order | new column sums];
// the carried ones are the stream's ring of L - 1 floats (frame f in slot f mod (L - 1)), or with L == 0 the one float
// that holds the maximum so far - a ring of one entry that already is a maximum.
//
//   track_level_suffix_kernel      : L > 0 only.  One workgroup per sequence walks ext backwards in chunks of
//                                    LEVEL_THREADS and writes per entry the maximum from it to the end of its block of L
//                                    entries (van Herk / Gil-Werman): a segmented inclusive scan - cross-lane moves
//                                    inside a wave, the wave totals through LDS, a carry from chunk to chunk.
//   track_level_prefix_kernel      : one workgroup per sequence, forwards: the maximum from the start of the entry's block
//                                    (L == 0: of ext) to the entry, by the same scan, and per new frame
//                                    level = fmaxf(floor, fmaxf(suffix[i - L + 1], prefix[i])) - the two pieces cover
//                                    exactly the L entries that end at i; before ext holds L entries the prefix alone.
//                                    No frame rescans its window: O(carried + new) per sequence whatever L is.
//   track_gate_running_kernel      : track_gate_kernel with the frame's own level.
//   track_stream_gate_running_kernel: track_stream_gate_kernel (gate, window numbering) with the frame's own level.
//   track_level_state_kernel       : behind every launch of the call that reads the carried values, one workgroup per
//                                    stream with new frames: its last min(n_new, L - 1) column sums go to their slots
//                                    (L == 0: the maximum so far to its float).  With n_new < L - 1 old and new entries
//                                    coexist in the ring.
// max is exact on finite values, so neither the scan order nor the cut into blocks or rounds changes a bit.  The gate
// is track_music_prob of track_shared.h, shared with the fixed-level kernels.  Every index comes from sizes the host
// validated; no atomics; no scratch memory.
#pragma clang fp contract(off)
#include "asr_kernels.h"
#include "track_shared.h"

namespace asr {

namespace {

constexpr int LEVEL_THREADS = 256;

// Inclusive maximum over the thread's segment, the threads of all chunks taken in scan order: `before` = the entries of
// its segment in front of this thread's.  carry = the result of the last thread of the chunk before (the same in every
// thread) and is replaced by this chunk's.  Every thread of the workgroup calls it; one past the end passes -inf.
__device__ __forceinline__ float level_scan_max(float v, uint32_t before, float &carry, float *s_wave, float *s_carry) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off);
        if (off <= lane && off <= before) v = fmaxf(v, o);
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < LEVEL_THREADS / 64; ++k) {       // an earlier wave whose last entry lies in the segment
        const float t = s_wave[k];
        if (k < wave && tid - (64u * k + 63u) <= before) v = fmaxf(v, t);
    }
    if (before > tid) v = fmaxf(v, carry);                    // the segment began in an earlier chunk
    if (tid == LEVEL_THREADS - 1) *s_carry = v;
    __syncthreads();                                          // (the next chunk writes s_wave behind this barrier)
    carry = *s_carry;
    return v;
}

// ring slot of ext entry 0 (L > 0): frame frames_before - n_hist
__device__ __forceinline__ uint32_t level_slot0(const TrackLevelArgs &a, const TrackLevelSeq &Q) {
    return a.memory > 0 ? (uint32_t)((Q.frames_before - Q.n_hist) % (int64_t)(a.memory - 1)) : 0u;
}
// ext entry j < n_hist + n_new; slot0 + j < 2^32 (n_hist < 2^20, n_new <= 2^30)
__device__ __forceinline__ float level_ext(const TrackLevelArgs &a, const TrackLevelSeq &Q, uint32_t slot0, uint32_t j) {
    if (j >= (uint32_t)Q.n_hist) return a.colsum[Q.cs_first + (j - (uint32_t)Q.n_hist)];
    return a.state[Q.state_off + (a.memory > 0 ? (slot0 + j) % (uint32_t)(a.memory - 1) : 0u)];
}

__global__ __launch_bounds__(LEVEL_THREADS) void track_level_suffix_kernel(TrackLevelArgs a) {
    __shared__ float s_wave[LEVEL_THREADS / 64];
    __shared__ float s_carry;
    const TrackLevelSeq Q = a.seqs[blockIdx.x];
    if (Q.n_new <= 0 || a.memory <= 0) return;                // the whole workgroup: no barrier is left waiting
    const uint32_t n = (uint32_t)Q.n_hist + (uint32_t)Q.n_new, L = (uint32_t)a.memory;
    const uint32_t slot0 = level_slot0(a, Q);
    float carry = -INFINITY;
    for (uint32_t base = 0; base < n; base += LEVEL_THREADS) {
        const uint32_t r = base + threadIdx.x;                // entry n - 1 - r
        const bool in = r < n;
        const uint32_t j = in ? n - 1 - r : 0;
        const uint32_t block_end = min(j - j % L + (L - 1), n - 1);
        const float v = level_scan_max(in ? level_ext(a, Q, slot0, j) : -INFINITY, in ? block_end - j : 0u, carry, s_wave,
                                       &s_carry);
        if (in) a.suffix[Q.sfx_first + j] = v;
    }
}

__global__ __launch_bounds__(LEVEL_THREADS) void track_level_prefix_kernel(TrackLevelArgs a) {
    __shared__ float s_wave[LEVEL_THREADS / 64];
    __shared__ float s_carry;
    const TrackLevelSeq Q = a.seqs[blockIdx.x];
    if (Q.n_new <= 0) return;
    const uint32_t h = (uint32_t)Q.n_hist, n = h + (uint32_t)Q.n_new, L = (uint32_t)a.memory;
    const uint32_t slot0 = level_slot0(a, Q);
    float carry = -INFINITY;
    for (uint32_t base = 0; base < n; base += LEVEL_THREADS) {
        const uint32_t j = base + threadIdx.x;
        const bool in = j < n;
        const float v = level_scan_max(in ? level_ext(a, Q, slot0, j) : -INFINITY, in ? (L ? j % L : j) : 0u, carry, s_wave,
                                       &s_carry);
        if (in && j >= h) {
            const float m = (L && j >= L - 1) ? fmaxf(a.suffix[Q.sfx_first + (j - (L - 1))], v) : v;
            a.level[Q.out_first + (j - h)] = fmaxf(a.floor, m);
            if (!L && j == n - 1) a.last[blockIdx.x] = m;
        }
    }
}

__global__ __launch_bounds__(LEVEL_THREADS) void track_level_state_kernel(TrackLevelArgs a) {
    const TrackLevelSeq Q = a.seqs[blockIdx.x];
    if (Q.n_new <= 0) return;
    if (a.memory <= 0) {
        if (threadIdx.x == 0) a.state[Q.state_off] = a.last[blockIdx.x];
        return;
    }
    const uint32_t keep = (uint32_t)a.memory - 1, n_new = (uint32_t)Q.n_new;
    const uint32_t nk = min(n_new, keep), skip = n_new - nk;                  // only the last nk column sums stay
    const uint32_t slot0 = (uint32_t)((Q.frames_before + skip) % (int64_t)keep);
    for (uint32_t e = threadIdx.x; e < nk; e += LEVEL_THREADS)
        a.state[Q.state_off + (slot0 + e) % keep] = a.colsum[Q.cs_first + skip + e];
}

__global__ __launch_bounds__(GATE_THREADS) void track_gate_running_kernel(TrackGateArgs a, const float *frame_level) {
    const int64_t g = (int64_t)blockIdx.x * GATE_THREADS + threadIdx.x;
    if (g >= a.total_frames) return;
    track_gate_frame(a, a.recs[track_rec_of(a.recs, a.n_rec, g)], g, frame_level[g]);
}

__global__ __launch_bounds__(SGATE_THREADS) void track_stream_gate_running_kernel(TrackStreamGateArgs a,
                                                                                  const float *frame_level) {
    __shared__ int s_wave[SGATE_THREADS / 64];
    track_stream_gate_stage(a, s_wave, [=](const TrackStreamRec &, int64_t g) { return frame_level[g]; });
}

}  // namespace

hipError_t launch_track_level(hipStream_t s, const TrackLevelArgs &a) {
    if (a.n_seq <= 0) return hipSuccess;
    if (a.memory > 0) track_level_suffix_kernel<<<a.n_seq, LEVEL_THREADS, 0, s>>>(a);
    track_level_prefix_kernel<<<a.n_seq, LEVEL_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_level_state(hipStream_t s, const TrackLevelArgs &a) {
    if (a.n_seq <= 0) return hipSuccess;
    track_level_state_kernel<<<a.n_seq, LEVEL_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_gate_running(hipStream_t s, const TrackGateArgs &a, const float *frame_level) {
    if (a.total_frames <= 0 || a.n_rec <= 0) return hipSuccess;
    track_gate_running_kernel<<<(int)((a.total_frames + GATE_THREADS - 1) / GATE_THREADS), GATE_THREADS, 0, s>>>(
        a, frame_level);
    return hipGetLastError();
}

hipError_t launch_track_stream_gate_running(hipStream_t s, const TrackStreamGateArgs &a, const float *frame_level) {
    if (a.total_frames <= 0 || a.n_streams <= 0) return hipSuccess;
    track_stream_gate_running_kernel<<<1, SGATE_THREADS, 0, s>>>(a, frame_level);
    return hipGetLastError();
}

}  // namespace asr
