// Device functions of the running piece vote that track_kernels.hip (whole recordings) and track_stream_kernels.hip
// (streams with carried device state) share: the gate's arithmetic and the vote histogram with its top-k selection.
// Both files are compiled without contraction; every float operation here has a fixed order.
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
