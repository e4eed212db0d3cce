// gfx950 kernels of the running piece vote for parallel live streams whose state stays on the device
// (asr_track_stream_gate_dev, asr_track_stream_vote_dev): what track_kernels.hip computes for whole recordings, per
// round of new columns.  A stream carries the last w - 1 columns (its tail) and the top-k index rows of its last
// running_frames - 1 voiced frames (a ring); both are read and updated in place.
//
//   track_stream_colsum_kernel : one thread per column of [tail | new] of every stream that brings columns.  The rows
//                                added one after the other in float32 (track_colsum_kernel); a tail that is not read
//                                (frames_before == 0) sums to 0.
//   track_stream_gate_kernel   : one workgroup.  Per new frame track_gate_kernel's m_prob and voiced from the w column
//                                sums that end at it, and in the same pass the exclusive running count of the voiced
//                                frames (ballot + popcount per wave, the wave totals through LDS, a carry from chunk
//                                to chunk): the window a voiced frame writes, in stream and frame order.  n_voiced per
//                                stream is the difference of two counts.
//   track_stream_window_kernel : one workgroup per new frame; an unvoiced one returns.  Window (bins, w) = columns
//                                i - w + 1 .. i of [tail | new]: consecutive threads write consecutive floats of the
//                                window (rows of w floats, coalesced) and read consecutive floats of a tail or block
//                                row, which up to w windows share and the cache serves.
//   track_stream_tail_kernel   : one workgroup per stream that brought columns, launched behind the two kernels that
//                                read the old tails.  New tail = the last w - 1 columns of [tail | new].  With
//                                n_new < w - 1 it overlaps the old one: an element's source lies n_new floats further
//                                in the same row, so the workgroup goes through the tail in ascending chunks of
//                                TAIL_THREADS floats, reads a chunk's sources, waits at a barrier, and writes the chunk -
//                                no chunk writes what a later one still reads.
//   track_stream_vote_kernel   : track_vote_kernel with the table [ring rows in frame order | new rows]: one wave per
//                                segment of a stream's new voiced frames.  Only reads the ring.
//   track_stream_ring_kernel   : behind the votes of the whole call, one workgroup per stream with new rows: its last
//                                min(n_new, running_frames - 1) new rows go to slots v mod (running_frames - 1) - each
//                                replaces exactly the row of frame v - (running_frames - 1).
// The order of the windows comes from counts and a scan, never from the order in which atomics land; counts are
// integers and every float operation has a fixed order (fp contract off here and in build.py).  Every index is checked
// against the sizes the host validated.
#pragma clang fp contract(off)
#include "asr_kernels.h"
#include "track_shared.h"

namespace asr {

namespace {

constexpr int TAIL_THREADS = 256;

// element (row b, column c) of [tail | new] of stream R; the tail counts as zeros while the stream has no frames
__device__ __forceinline__ float ext_elem(const TrackStreamGateArgs &a, const TrackStreamRec &R, int b, int64_t c) {
    const int t = a.width - 1;
    if (c < t) return R.frames_before > 0 ? a.tail[R.tail_off + (int64_t)b * t + c] : 0.0f;
    return a.cols[R.col_off + (int64_t)b * R.n_new + (c - t)];
}

__global__ __launch_bounds__(SGATE_THREADS) void track_stream_colsum_kernel(TrackStreamGateArgs a) {
    const int64_t x = (int64_t)blockIdx.x * SGATE_THREADS + threadIdx.x;
    if (x >= a.total_ext) return;
    const TrackStreamRec R = a.recs[stream_of_ext(a.recs, a.n_streams, x)];
    const int64_t c = x - R.ext_first;
    if (c < 0 || c >= (int64_t)(a.width - 1) + R.n_new) return;
    float s = ext_elem(a, R, 0, c);
    for (int b = 1; b < a.bins; ++b) s = s + ext_elem(a, R, b, c);
    a.colsum[x] = s;
}

__global__ __launch_bounds__(SGATE_THREADS) void track_stream_gate_kernel(TrackStreamGateArgs a) {
    __shared__ int s_wave[SGATE_THREADS / 64];
    track_stream_gate_stage(a, s_wave, [](const TrackStreamRec &R, int64_t) { return R.level; });
}

__global__ __launch_bounds__(SGATE_THREADS) void track_stream_window_kernel(TrackStreamGateArgs a) {
    const int64_t g = blockIdx.x;
    if (g >= a.total_frames || !a.voiced[g]) return;
    const int64_t k = a.slot[g];
    if (k < 0 || k >= a.total_frames) return;                 // total_frames <= win_cap: the host checked
    const TrackStreamRec R = a.recs[stream_of_frame(a.recs, a.n_streams, g)];
    const int64_t i = g - R.first;
    const uint32_t w = (uint32_t)a.width, n = (uint32_t)a.bins * w;
    float *out = a.win + k * (int64_t)n;
    for (uint32_t e = threadIdx.x; e < n; e += SGATE_THREADS) {
        const uint32_t b = e / w, j = e - b * w;
        out[e] = ext_elem(a, R, (int)b, i + j);
    }
}

__global__ __launch_bounds__(TAIL_THREADS) void track_stream_tail_kernel(TrackStreamGateArgs a) {
    const TrackStreamRec R = a.recs[blockIdx.x];
    if (R.n_new <= 0) return;                                 // the whole workgroup: no barrier is left waiting
    const int t = a.width - 1;
    const int64_t n = (int64_t)a.bins * t;
    float *tail = a.tail + R.tail_off;
    for (int64_t base = 0; base < n; base += TAIL_THREADS) {
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

// ---- sliding vote over [ring | new rows] -----------------------------------------------------------------------------
// voiced frame v of the segment's stream votes with weight d
template <bool GLOBAL>
__device__ __forceinline__ void stream_vote_row(const TrackStreamVoteArgs &a, const TrackStreamSeg &S, int32_t *hist,
                                                int64_t v, int32_t d) {
    const int32_t *e;
    if (v >= S.vb) {
        const int64_t row = S.row0 + (v - S.vb);
        if (row < 0 || row >= a.n_rows) return;
        e = a.idx + row * a.n_candidates;
    } else {
        if (v < 0 || a.running_frames < 2) return;
        e = a.ring + S.hist_off + (v % (a.running_frames - 1)) * a.n_candidates;
    }
    track_vote_entries<GLOBAL>(e, a.n_candidates, a.ids, a.n_db, a.n_pieces, hist, d);
}

template <bool GLOBAL>
__global__ __launch_bounds__(TRACK_THREADS) void track_stream_vote_kernel(TrackStreamVoteArgs a) {
    __shared__ int32_t s_hist[GLOBAL ? 1 : TRACK_LDS_PIECES];
    int32_t *hist = GLOBAL ? a.hist_ws + (int64_t)blockIdx.x * a.n_pieces : s_hist;
    const int lane = threadIdx.x;
    for (int64_t si = blockIdx.x; si < a.n_segs; si += gridDim.x) {
        const TrackStreamSeg S = a.segs[si];
        if (!GLOBAL)
            for (int p = lane; p < a.n_pieces; p += TRACK_THREADS) hist[p] = 0;
        __syncthreads();
        // the history before the segment: frames max(0, v0 - (running_frames - 1)) .. v0 - 1, from the ring below vb
        const int64_t h0 = S.v0 > (int64_t)(a.running_frames - 1) ? S.v0 - (a.running_frames - 1) : 0;
        for (int64_t v = h0; v < S.v0; ++v) stream_vote_row<GLOBAL>(a, S, hist, v, 1);
        for (int64_t v = S.v0; v < S.v0 + S.n; ++v) {
            stream_vote_row<GLOBAL>(a, S, hist, v, 1);
            if (v > S.v0 && v >= a.running_frames) stream_vote_row<GLOBAL>(a, S, hist, v - a.running_frames, -1);
            __syncthreads();
            const int64_t o = S.row0 + (v - S.vb);
            track_emit_topk<GLOBAL>(hist, a.n_pieces, a.top_k, a.pieces + o * a.top_k, a.counts + o * a.top_k, a.n_out + o);
            __syncthreads();                              // the next frame's atomics come after this frame's reads
        }
        if (GLOBAL) {                                     // leave the slice zeroed: take back what is still counted
            const int64_t end = S.v0 + S.n;
            const int64_t l0 = end > (int64_t)a.running_frames ? end - a.running_frames : 0;
            for (int64_t v = l0; v < end; ++v) stream_vote_row<GLOBAL>(a, S, hist, v, -1);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SGATE_THREADS) void track_stream_ring_kernel(TrackStreamVoteArgs a) {
    if ((int)blockIdx.x >= a.n_keep || a.running_frames < 2) return;
    const TrackStreamKeep K = a.keeps[blockIdx.x];
    const int64_t keep = a.running_frames - 1, C = a.n_candidates;
    const int64_t nk = K.n_new < keep ? K.n_new : keep, skip = K.n_new - nk;       // only the last nk rows stay
    for (int64_t e = threadIdx.x; e < nk * C; e += SGATE_THREADS) {
        const int64_t r = e / C, c = e - r * C;
        const int64_t row = K.row0 + skip + r, v = K.vb + skip + r;
        if (row < 0 || row >= a.n_rows) continue;
        a.ring[K.hist_off + (v % keep) * C + c] = a.idx[row * C + c];
    }
}

}  // namespace

hipError_t launch_track_stream_colsum(hipStream_t s, const TrackStreamGateArgs &a) {
    if (a.total_frames <= 0 || a.n_streams <= 0) return hipSuccess;
    track_stream_colsum_kernel<<<(int)((a.total_ext + SGATE_THREADS - 1) / SGATE_THREADS), SGATE_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_stream_gate(hipStream_t s, const TrackStreamGateArgs &a) {
    if (a.total_frames <= 0 || a.n_streams <= 0) return hipSuccess;
    track_stream_colsum_kernel<<<(int)((a.total_ext + SGATE_THREADS - 1) / SGATE_THREADS), SGATE_THREADS, 0, s>>>(a);
    track_stream_gate_kernel<<<1, SGATE_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_stream_windows(hipStream_t s, const TrackStreamGateArgs &a) {
    if (a.total_frames <= 0 || a.n_streams <= 0) return hipSuccess;
    track_stream_window_kernel<<<(int)a.total_frames, SGATE_THREADS, 0, s>>>(a);
    track_stream_tail_kernel<<<a.n_streams, TAIL_THREADS, 0, s>>>(a);          // behind the readers of the old tails
    return hipGetLastError();
}

hipError_t launch_track_stream_vote(hipStream_t s, const TrackStreamVoteArgs &a, int grid, bool global_path) {
    if (a.n_segs <= 0 || grid <= 0) return hipSuccess;
    if (global_path) {
        hipError_t e = hipMemsetAsync(a.hist_ws, 0, (size_t)grid * a.n_pieces * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        track_stream_vote_kernel<true><<<grid, TRACK_THREADS, 0, s>>>(a);
    } else {
        track_stream_vote_kernel<false><<<grid, TRACK_THREADS, 0, s>>>(a);
    }
    if (a.n_keep > 0 && a.running_frames > 1)                                   // behind every vote of the call
        track_stream_ring_kernel<<<a.n_keep, SGATE_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace asr
