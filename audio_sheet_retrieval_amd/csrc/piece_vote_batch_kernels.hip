// gfx950 kernel of the batched piece-identification vote (asr_piece_vote_batch_dev): the vote of
// detect_score / detect_performance (audio_sheet_server.py:228-244) for n_groups query pieces in one launch, plus the
// full-eval rank of each query's target piece (:640-645, sheet_audio_server.py:85-90).
//
//   vote_batch_kernel : one workgroup per group (grid-stride over the groups).
//     1. histogram of the piece ids of the group's retrieved entries: integer atomics on a per-piece counter array,
//        in LDS (template <false>, n_pieces <= VOTE_LDS_PIECES) or in a zeroed global workspace (<true>);
//     2. every voted piece becomes one 64-bit key (count << 32) | piece, appended with one LDS atomic per wave;
//     3. bitonic sort of the keys in descending order (padded with 0 keys to a power of two): votes descending and,
//        for equal votes, the larger piece id first - asr_piece_vote_dev's order;
//     4. the first top_k keys are written (piece -1 / count 0 past the voted pieces), the target is ranked from its
//        position and its ratio is count / (sum of the returned counts) in float64.
//   Counts are integers, so the histogram is order-independent and every result is deterministic.  Groups do not
//   communicate: neither batch composition nor order changes a group's result.
#include "asr_kernels.h"

namespace asr {

namespace {

constexpr int VOTE_THREADS = 256;

template <bool GLOBAL>
__global__ __launch_bounds__(VOTE_THREADS) void vote_batch_kernel(VoteBatchArgs a) {
    // LDS path: 16 KiB of counters + 32 KiB of keys, three workgroups per CU
    __shared__ int32_t s_hist[GLOBAL ? 1 : VOTE_LDS_PIECES];
    __shared__ uint64_t s_keys[GLOBAL ? 1 : VOTE_LDS_PIECES];
    __shared__ int s_nv, s_pos;
    __shared__ unsigned long long s_sum;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        int32_t *hist = GLOBAL ? a.hist_ws + g * a.n_pieces : s_hist;
        uint64_t *keys = GLOBAL ? a.keys_ws + g * a.keys_cap : s_keys;
        if (!GLOBAL)
            for (int p = tid; p < a.n_pieces; p += VOTE_THREADS) hist[p] = 0;
        if (tid == 0) { s_nv = 0; s_pos = -1; s_sum = 0; }
        __syncthreads();

        const int32_t *gi = a.idx + g * a.per_group;
        for (int64_t e = tid; e < a.per_group; e += VOTE_THREADS) {
            const int32_t j = gi[e];
            if (j < 0 || j >= a.n_db) continue;          // -1: fewer than k data-base entries
            const int32_t p = a.ids[j];
            if (p >= 0 && p < a.n_pieces) atomicAdd(&hist[p], 1);
        }
        __syncthreads();

        // voted pieces -> keys (append order is irrelevant: the sort below orders them)
        for (int p0 = 0; p0 < a.n_pieces; p0 += VOTE_THREADS) {
            const int p = p0 + tid;
            const int32_t c = p < a.n_pieces ? hist[p] : 0;
            const unsigned long long m = __ballot(c > 0);
            int base = 0;
            if (lane == 0 && m) base = atomicAdd(&s_nv, __popcll(m));
            base = __shfl(base, 0);
            if (c > 0) keys[base + __popcll(m & ((1ull << lane) - 1ull))] = ((uint64_t)(uint32_t)c << 32) | (uint32_t)p;
        }
        __syncthreads();
        const int nv = s_nv;
        int P = 1;
        while (P < nv) P <<= 1;                           // nv <= keys capacity, a power of two
        for (int i = nv + tid; i < P; i += VOTE_THREADS) keys[i] = 0;
        __syncthreads();

        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += VOTE_THREADS) {
                    const int i = (t / j) * 2 * j + (t % j), l = i + j;
                    const uint64_t x = keys[i], y = keys[l];
                    if ((i & k) == 0 ? x < y : x > y) { keys[i] = y; keys[l] = x; }
                }
                __syncthreads();
            }

        const int n = min(a.top_k, nv);
        const int32_t target = a.targets ? a.targets[g] : -1;
        int32_t *op = a.pieces + g * a.top_k, *oc = a.counts + g * a.top_k;
        unsigned long long part = 0;
        for (int r = tid; r < a.top_k; r += VOTE_THREADS) {
            const uint64_t key = r < n ? keys[r] : 0;
            const int32_t c = (int32_t)(key >> 32), p = r < n ? (int32_t)(uint32_t)key : -1;
            op[r] = p;
            oc[r] = c;
            part += (unsigned long long)c;
            if (r < n && p == target) s_pos = r;         // piece ids are unique: at most one writer
        }
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
        if (lane == 0 && part) atomicAdd(&s_sum, part);
        __syncthreads();
        if (tid == 0) {
            a.n_out[g] = n;
            if (a.targets) {
                const int pos = s_pos;
                a.ranks[g] = pos >= 0 ? pos + 1 : n;      // no votes: n = 0
                a.ratios[g] = pos >= 0 ? (double)(keys[pos] >> 32) / (double)s_sum : 0.0;
            }
        }
        __syncthreads();                                  // s_* and the LDS arrays are reused by the next group
    }
}

}  // namespace

hipError_t launch_piece_vote_batch(hipStream_t s, const VoteBatchArgs &a, bool global_path) {
    if (a.n_groups <= 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>(a.n_groups, 65536);
    if (global_path) {
        hipError_t e = hipMemsetAsync(a.hist_ws, 0, (size_t)a.n_groups * a.n_pieces * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        vote_batch_kernel<true><<<grid, VOTE_THREADS, 0, s>>>(a);
    } else {
        vote_batch_kernel<false><<<grid, VOTE_THREADS, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace asr
