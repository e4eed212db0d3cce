// Device functions of the running piece vote that track_kernels.hip (whole recordings), track_stream_kernels.hip
// (streams with carried device state) and track_level_kernels.hip (both, with the level of what has been heard so far)
// share: the gate's arithmetic, the gate of a frame and of a round of streams, and the vote histogram with its top-k
// selection.  All three files are compiled without contraction; every float operation here has a fixed order.
#pragma once
#include "asr_kernels.h"

namespace asr {

constexpr int TRACK_THREADS = 64;      // one wave: the slide is a chain of small steps, barriers would dominate it

// _detect_music (:524-528) on the w column sums elem(0) .. elem(w - 1): their mean as numpy's pairwise sum of w <= 128
// float32 values computes it (eight interleaved accumulators over the full blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+
// (r6+r7)), the remainder added in order) divided by float32(w); divided by float32(level * float32(0.15)); clipped to
// [0, 1] (NaN stays NaN)
template <typename Elem>
__device__ __forceinline__ float track_music_prob(Elem elem, int w, float level) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = elem(j);
    const int full = w - (w & 7);
    for (int i = 8; i < full; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + elem(i + j);
    }
    float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = full; i < w; ++i) s = s + elem(i);
    float m = __fdiv_rn(s, (float)w);
    m = __fdiv_rn(m, __fmul_rn(level, 0.15f));
    if (m == m) m = fminf(fmaxf(m, 0.0f), 1.0f);
    return m;
}

// ---- the gate of one frame, at a level the caller chooses (the recording's, the stream's, or the frame's own) ----------
constexpr int GATE_THREADS = 256;
constexpr int SGATE_THREADS = 256;

// recording of concatenated frame g: the last r with recs[r].first <= g
__device__ __forceinline__ int track_rec_of(const TrackRec *__restrict__ recs, int n_rec, int64_t g) {
    int lo = 0, hi = n_rec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// m_prob and voiced of concatenated frame g of recording R from the last w column sums (zeros before its start)
__device__ __forceinline__ void track_gate_frame(const TrackGateArgs &a, const TrackRec &R, int64_t g, float level) {
    const int w = a.width;
    const int64_t c0 = g - R.first - (w - 1);                  // first column of the window (negative: zeros)
    const float *cs = a.colsum + R.first;
    auto elem = [&](int j) { const int64_t c = c0 + j; return c >= 0 ? cs[c] : 0.0f; };
    const float m = track_music_prob(elem, w, level);
    a.m_prob[g] = m;
    a.voiced[g] = (m > 0.5f && R.frame0 + (g - R.first) >= (int64_t)w) ? 1 : 0;
}

// stream of concatenated frame g / column sum x: the last s with first (ext_first) <= the index; streams without new
// columns share their successor's value and are never the last
__device__ __forceinline__ int stream_of_frame(const TrackStreamRec *__restrict__ recs, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int stream_of_ext(const TrackStreamRec *__restrict__ recs, int n, int64_t x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].ext_first <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One workgroup of SGATE_THREADS: per new frame g of every stream m_prob and voiced from the w column sums that end at
// it, at level_of(R, g), and in the same pass the exclusive running count of the voiced frames (ballot + popcount per
// wave, the wave totals through LDS, a carry from chunk to chunk): the window a voiced frame writes, in stream and frame
// order.  n_voiced per stream is the difference of two counts.  s_wave: SGATE_THREADS / 64 ints of LDS.
template <typename Level>
__device__ __forceinline__ void track_stream_gate_stage(const TrackStreamGateArgs &a, int *s_wave, Level level_of) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.width;
    int carry = 0;                                            // voiced frames before this chunk (the same in every thread)
    for (int64_t base = 0; base < a.total_frames; base += SGATE_THREADS) {
        const int64_t g = base + tid;
        int v = 0;
        if (g < a.total_frames) {
            const TrackStreamRec R = a.recs[stream_of_frame(a.recs, a.n_streams, g)];
            const int64_t i = g - R.first;                    // window of frame i: column sums i .. i + w - 1
            const float *cs = a.colsum + R.ext_first + i;
            auto elem = [&](int j) { return cs[j]; };
            const float m = track_music_prob(elem, w, level_of(R, g));
            v = (m > 0.5f && R.frames_before + i >= (int64_t)w) ? 1 : 0;
            a.m_prob[g] = m;
            a.voiced[g] = (uint8_t)v;
        }
        const unsigned long long bal = __ballot(v);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
        for (int k = 0; k < SGATE_THREADS / 64; ++k) {
            const int c = s_wave[k];
            if (k < wave) before += c;
            total += c;
        }
        if (g < a.total_frames) a.slot[g] = carry + before;
        carry += total;
        __syncthreads();                                      // s_wave is rewritten by the next chunk
    }
    if (tid == 0) a.slot[a.total_frames] = carry;
    __syncthreads();
    for (int s = tid; s < a.n_streams; s += SGATE_THREADS) {
        const TrackStreamRec R = a.recs[s];
        a.n_voiced[s] = a.slot[R.first + R.n_new] - a.slot[R.first];
    }
}

template <bool GLOBAL>
__device__ __forceinline__ void hist_add(int32_t *h, int32_t p, int32_t d) {
    if (GLOBAL) __hip_atomic_fetch_add(h + p, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else atomicAdd(h + p, d);
}
// the global counters are read where the atomics work, past the vector cache: a line fetched before a later atomic
// would still hold the old count
template <bool GLOBAL>
__device__ __forceinline__ int32_t hist_get(const int32_t *h, int32_t p) {
    return GLOBAL ? __hip_atomic_load(h + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : h[p];
}

// the n_candidates data-base indices at e vote with weight d; an index outside [0, n_db) or a piece id outside
// [0, n_pieces) is ignored
template <bool GLOBAL>
__device__ __forceinline__ void track_vote_entries(const int32_t *__restrict__ e, int n_candidates,
                                                   const int32_t *__restrict__ ids, int64_t n_db, int32_t n_pieces,
                                                   int32_t *hist, int32_t d) {
    for (int c = threadIdx.x; c < n_candidates; c += TRACK_THREADS) {
        const int32_t j = e[c];
        if (j < 0 || j >= n_db) continue;
        const int32_t p = ids[j];
        if (p >= 0 && p < n_pieces) hist_add<GLOBAL>(hist, p, d);
    }
}

// one wave: the top_k keys (count << 32 | piece) of the histogram by repeated wave-wide maxima below the previous one -
// votes descending, equal votes the larger piece id first; piece -1 / count 0 past the voted pieces
template <bool GLOBAL>
__device__ __forceinline__ void track_emit_topk(const int32_t *hist, int32_t n_pieces, int top_k, int32_t *op, int32_t *oc,
                                                int32_t *n_out) {
    const int lane = threadIdx.x;
    unsigned long long prev = ~0ull;
    int n = 0;
    while (n < top_k) {
        unsigned long long best = 0;
        for (int p = lane; p < n_pieces; p += TRACK_THREADS) {
            const int32_t c = hist_get<GLOBAL>(hist, p);
            const unsigned long long key = c > 0 ? ((unsigned long long)(uint32_t)c << 32) | (uint32_t)p : 0;
            if (key < prev && key > best) best = key;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off);
            if (other > best) best = other;
        }
        if (best == 0) break;                     // fewer voted pieces than top_k
        if (lane == 0) { op[n] = (int32_t)(uint32_t)best; oc[n] = (int32_t)(best >> 32); }
        prev = best;
        ++n;
    }
    for (int r = n + lane; r < top_k; r += TRACK_THREADS) { op[r] = -1; oc[r] = 0; }
    if (lane == 0) *n_out = n;
}

}  // namespace asr
