// gfx950 kernels of the running piece vote (asr_track_gate_dev, asr_track_vote_batch_dev): the loop of the reference's
// live server, AudioSheetServer.run (audio_sheet_server.py:83-211), over whole recordings.
//
//   track_colsum_kernel : one thread per frame.  colsum[t] = spec[:, t].sum(): the rows added one after the other in
//                         float32, as running_spec.sum(axis=0) adds them (:526).
//   track_level_kernel  : one workgroup per recording.  spec.sum(axis=0).max() (:527; a NaN column sum gives NaN), or the
//                         caller's normaliser in its place.
//   track_gate_kernel   : one thread per frame.  _detect_music (:524-528) on the last w column sums (zeros before the
//                         recording's start): their mean as numpy's pairwise sum of w <= 128 float32 values computes it
//                         (eight interleaved accumulators over the full blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+
//                         (r6+r7)), the remainder added in order) divided by float32(w); divided by float32(level *
//                         float32(0.15)); clipped to [0, 1] (NaN stays NaN).  voiced = m_prob > 0.5 and frame >= w (:117).
//   track_vote_kernel   : one wave per segment of a recording's voiced frames.  The vote histogram (:126-132) of the
//                         frames in the history before the segment's first frame is rebuilt with integer atomics, then
//                         slid frame by frame: the n_candidates piece ids of the entering frame are added, those of the
//                         frame that leaves the history removed, and the top_k keys (count << 32 | piece) selected by
//                         repeated wave-wide maxima below the previous one - votes descending, equal votes the larger
//                         piece id first (asr_piece_vote_dev's order).  The counters live in LDS (template <false>,
//                         n_pieces <= TRACK_LDS_PIECES) or in the workgroup's slice of a zeroed global workspace
//                         (<true>), which it leaves zeroed for its next segment.
// Counts are integers and every float operation has a fixed order: results do not depend on the batch composition, the
// segment length or the histogram path.  No add is contracted or reordered (fp contract off here and in build.py).
// Every index is checked against the table sizes the host validated; a data-base index outside [0, n_db) or a piece id
// outside [0, n_pieces) is ignored, as asr_piece_vote_batch_dev ignores it.
#pragma clang fp contract(off)
#include "asr_kernels.h"
#include "track_shared.h"

namespace asr {

namespace {

__global__ __launch_bounds__(GATE_THREADS) void track_colsum_kernel(TrackGateArgs a) {
    const int64_t g = (int64_t)blockIdx.x * GATE_THREADS + threadIdx.x;
    if (g >= a.total_frames) return;
    const TrackRec R = a.recs[track_rec_of(a.recs, a.n_rec, g)];
    const float *p = a.src + R.off + (g - R.first);
    float s = p[0];
    for (int b = 1; b < R.bins; ++b) s = s + p[(int64_t)b * R.frames];
    a.colsum[g] = s;
}

__global__ __launch_bounds__(GATE_THREADS) void track_level_kernel(TrackGateArgs a) {
    __shared__ float s_max[GATE_THREADS / 64];
    __shared__ int s_nan[GATE_THREADS / 64];
    const TrackRec R = a.recs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (R.has_norm) {
        if (tid == 0) a.level[blockIdx.x] = R.norm;
        return;
    }
    float m = -INFINITY;
    int bad = 0;
    for (int64_t t = tid; t < R.frames; t += GATE_THREADS) {
        const float v = a.colsum[R.first + t];
        bad |= v != v;
        m = fmaxf(m, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = fmaxf(m, __shfl_xor(m, off));
        bad |= __shfl_xor(bad, off);
    }
    if (lane == 0) { s_max[wave] = m; s_nan[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < GATE_THREADS / 64; ++w) { m = fmaxf(m, s_max[w]); bad |= s_nan[w]; }
        a.level[blockIdx.x] = bad ? NAN : m;
    }
}

__global__ __launch_bounds__(GATE_THREADS) void track_gate_kernel(TrackGateArgs a) {
    const int64_t g = (int64_t)blockIdx.x * GATE_THREADS + threadIdx.x;
    if (g >= a.total_frames) return;
    const int ri = track_rec_of(a.recs, a.n_rec, g);
    track_gate_frame(a, a.recs[ri], g, a.level[ri]);
}

// ---- sliding vote ----------------------------------------------------------------------------------------------------
// the n_candidates entries of table row `row` vote with weight d
template <bool GLOBAL>
__device__ __forceinline__ void track_vote_row(const TrackVoteArgs &a, int32_t *hist, int64_t row, int32_t d) {
    track_vote_entries<GLOBAL>(a.idx + row * a.n_candidates, a.n_candidates, a.ids, a.n_db, a.n_pieces, hist, d);
}

template <bool GLOBAL>
__global__ __launch_bounds__(TRACK_THREADS) void track_vote_kernel(TrackVoteArgs a) {
    __shared__ int32_t s_hist[GLOBAL ? 1 : TRACK_LDS_PIECES];
    int32_t *hist = GLOBAL ? a.hist_ws + (int64_t)blockIdx.x * a.n_pieces : s_hist;
    const int lane = threadIdx.x;
    for (int64_t si = blockIdx.x; si < a.n_segs; si += gridDim.x) {
        const TrackSeg S = a.segs[si];
        if (!GLOBAL)
            for (int p = lane; p < a.n_pieces; p += TRACK_THREADS) hist[p] = 0;
        __syncthreads();
        // the history before the segment: frames max(0, f0 - (running_frames - 1)) .. f0 - 1
        const int64_t h0 = S.f0 > (int64_t)(a.running_frames - 1) ? S.f0 - (a.running_frames - 1) : 0;
        for (int64_t f = h0; f < S.f0; ++f) track_vote_row<GLOBAL>(a, hist, S.row0 + f, 1);
        for (int64_t f = S.f0; f < S.f0 + S.n; ++f) {
            track_vote_row<GLOBAL>(a, hist, S.row0 + f, 1);
            if (f > S.f0 && f >= a.running_frames) track_vote_row<GLOBAL>(a, hist, S.row0 + f - a.running_frames, -1);
            __syncthreads();
            const int64_t o = S.out0 + (f - S.f0);
            int32_t *op = a.pieces + o * a.top_k, *oc = a.counts + o * a.top_k;
            track_emit_topk<GLOBAL>(hist, a.n_pieces, a.top_k, op, oc, a.n_out + o);
            __syncthreads();                              // the next frame's atomics come after this frame's reads
        }
        if (GLOBAL) {                                     // leave the slice zeroed: take back what is still counted
            const int64_t end = S.f0 + S.n;
            const int64_t l0 = end > (int64_t)a.running_frames ? end - a.running_frames : 0;
            for (int64_t f = l0; f < end; ++f) track_vote_row<GLOBAL>(a, hist, S.row0 + f, -1);
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_track_colsum(hipStream_t s, const TrackGateArgs &a) {
    if (a.total_frames <= 0 || a.n_rec <= 0) return hipSuccess;
    track_colsum_kernel<<<(int)((a.total_frames + GATE_THREADS - 1) / GATE_THREADS), GATE_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_gate(hipStream_t s, const TrackGateArgs &a) {
    if (a.total_frames <= 0 || a.n_rec <= 0) return hipSuccess;
    const int grid = (int)((a.total_frames + GATE_THREADS - 1) / GATE_THREADS);
    track_colsum_kernel<<<grid, GATE_THREADS, 0, s>>>(a);
    track_level_kernel<<<a.n_rec, GATE_THREADS, 0, s>>>(a);
    track_gate_kernel<<<grid, GATE_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_track_vote(hipStream_t s, const TrackVoteArgs &a, int grid, bool global_path) {
    if (a.n_segs <= 0 || grid <= 0) return hipSuccess;
    if (global_path) {
        hipError_t e = hipMemsetAsync(a.hist_ws, 0, (size_t)grid * a.n_pieces * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        track_vote_kernel<true><<<grid, TRACK_THREADS, 0, s>>>(a);
    } else {
        track_vote_kernel<false><<<grid, TRACK_THREADS, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace asr
