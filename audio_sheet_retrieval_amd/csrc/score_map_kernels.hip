// Measures of the pieces in strip coordinates (asr_score_map_dev; include/asr_hip.h carries the definition): from the bar
// network's float64 maps, which exist only on the device, to a few hundred int32 rows.  One comparison per map element,
// integers from there on.
//
//   score_map_counts_kernel : one workgroup per SCORE_MAP_CHUNK = 64 columns of a system, the chunks of all systems
//                             numbered through (ScoreSystem::chunk_first), so it is one launch whatever the number of pages
//                             and systems.  Lane l of every wave is column c0 + 64 * chunk + l: a wave reads 512 contiguous
//                             bytes of a map row.  The band's rows go round the four waves (the counts are integers, the
//                             order is free), the four partial counts meet in LDS, and wave 0 writes the 64 flags
//                             count >= min_rows as one 64-bit word (a column beyond the system's width: 0).
//   score_map_lines_kernel  : one wave per system over its flag words, in column order.  A lane whose column ends a run
//                             (flag set, next flag clear) finds the run's first column by counting the set flags below it
//                             - in its word, then in the words before it - and takes the centre (first + last) / 2.  The
//                             interior centres are compacted in column order by a scan: the lane's rank among the wave's
//                             interior lines (a ballot and a population count below the lane) plus the count carried from
//                             the words before.  n_lines holds the full count also when it exceeds max_lines.
//   score_map_table_kernel  : one workgroup.  A scan of n_lines + 1 over the systems that restarts at every piece gives a
//                             system's first measure within its piece; the last system of a piece leaves the piece's count,
//                             a scan of those gives piece_first; then every (system, measure) writes its row.  A system
//                             with more than max_lines interior lines: header[1] = the first such system and no row is
//                             written.
//
// No atomics, no scratch memory: every output has one writer, so the table is deterministic.
#include "asr_kernels.h"

namespace asr {

namespace {

// last i with table[i].chunk_first <= g
__device__ __forceinline__ int score_map_system_of_chunk(const ScoreSystem *__restrict__ table, int n_systems, int64_t g) {
    int lo = 0, hi = n_systems - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk_first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(SCORE_MAP_THREADS) void score_map_counts_kernel(const double *__restrict__ maps,
                                                                            const ScoreSystem *__restrict__ table,
                                                                            int n_systems, double threshold, int min_rows,
                                                                            unsigned long long *__restrict__ flags) {
    constexpr int WAVES = SCORE_MAP_THREADS / 64;
    __shared__ int partial[WAVES][SCORE_MAP_CHUNK];
    const int64_t g = blockIdx.x;
    const int si = score_map_system_of_chunk(table, n_systems, g);
    const int64_t map0 = table[si].map, first = table[si].chunk_first;
    const int stride = table[si].stride, rows = table[si].rows, width = table[si].width;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (int)(g - first) * SCORE_MAP_CHUNK + lane;           // within the system
    int count = 0;
    if (col < width) {
        const double *p = maps + map0 + col;
#pragma unroll 4
        for (int r = wave; r < rows; r += WAVES) count += p[(int64_t)r * stride] > threshold ? 1 : 0;
    }
    partial[wave][lane] = count;
    __syncthreads();
    if (wave == 0) {
        int total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) total += partial[v][lane];
        const unsigned long long word = __ballot(col < width && total >= min_rows);
        if (lane == 0) flags[g] = word;
    }
}

__global__ __launch_bounds__(64) void score_map_lines_kernel(const ScoreSystem *__restrict__ table,
                                                             const unsigned long long *__restrict__ flags, int tol,
                                                             int max_lines, int32_t *__restrict__ n_lines,
                                                             int32_t *__restrict__ lines) {
    const int si = blockIdx.x, lane = threadIdx.x;
    const int width = table[si].width, c0 = table[si].c0;
    const unsigned long long *f = flags + table[si].chunk_first;
    const int n_words = (width + SCORE_MAP_CHUNK - 1) / SCORE_MAP_CHUNK;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t *out = lines + (int64_t)si * max_lines;
    int kept = 0;                                                          // interior lines of the words before: uniform
    unsigned long long word = f[0];
    for (int w = 0; w < n_words; ++w) {
        const unsigned long long next = w + 1 < n_words ? f[w + 1] : 0ull;
        const bool set = (word >> lane) & 1ull;
        const bool next_set = lane < 63 ? ((word >> (lane + 1)) & 1ull) != 0ull : (next & 1ull) != 0ull;
        bool interior = false;
        int centre = 0;
        if (set && !next_set) {                                            // this column ends a run
            const int last = w * SCORE_MAP_CHUNK + lane;
            const unsigned long long clear = ~word & below;                // clear flags below the lane, in this word
            int first;
            if (clear != 0ull) {
                first = w * SCORE_MAP_CHUNK + 64 - __clzll((long long)clear);
            } else {                                                       // the run began in an earlier word
                first = 0;
                for (int v = w - 1; v >= 0; --v) {
                    const unsigned long long c = ~f[v];
                    if (c != 0ull) {
                        first = v * SCORE_MAP_CHUNK + 64 - __clzll((long long)c);
                        break;
                    }
                }
            }
            centre = c0 + ((first + last) >> 1);                           // = ((c0 + first) + (c0 + last)) / 2
            interior = centre - c0 > tol && (c0 + width - 1) - centre > tol;
        }
        const unsigned long long found = __ballot(interior);
        if (interior) {
            const int k = kept + __popcll(found & below);
            if (k < max_lines) out[k] = centre;
        }
        kept += __popcll(found);
        word = next;
    }
    if (lane == 0) n_lines[si] = kept;
}

struct SegPair {
    int sum;                // of the values since the last start (inclusive), or since the pair's left end
    int start;              // whether a segment starts inside the pair's range
};

__device__ __forceinline__ SegPair seg_join(SegPair a, SegPair b) {      // a before b
    SegPair r;
    r.sum = b.start ? b.sum : a.sum + b.sum;
    r.start = a.start | b.start;
    return r;
}

constexpr int TABLE_THREADS = 256;

// inclusive scan over the block's TABLE_THREADS values, in LDS; the caller's barrier discipline: both buffers are free
__device__ __forceinline__ SegPair block_seg_scan(SegPair v, SegPair (*buf)[TABLE_THREADS]) {
    const int t = threadIdx.x;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < TABLE_THREADS; d <<= 1) {
        SegPair x = buf[cur][t];
        if (t >= d) x = seg_join(buf[cur][t - d], x);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const SegPair r = buf[cur][t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TABLE_THREADS) void score_map_table_kernel(const ScoreSystem *__restrict__ table, int n_systems,
                                                                        int n_pieces, int max_lines,
                                                                        const int32_t *__restrict__ n_lines,
                                                                        const int32_t *__restrict__ lines,
                                                                        int32_t *__restrict__ piece_count,
                                                                        int32_t *__restrict__ piece_first,
                                                                        int32_t *__restrict__ header,
                                                                        int32_t *__restrict__ sys_first,
                                                                        int32_t *__restrict__ measures) {
    __shared__ SegPair buf[2][TABLE_THREADS];
    __shared__ int overflow;
    const int t = threadIdx.x;
    if (t == 0) overflow = 0x7fffffff;
    for (int q = t; q < n_pieces; q += TABLE_THREADS) piece_count[q] = 0;
    __syncthreads();
    // the first system with too many lines: every thread takes the smallest of its own, thread after thread joins in LDS
    int mine = 0x7fffffff;
    for (int i = t; i < n_systems; i += TABLE_THREADS)
        if (n_lines[i] > max_lines) mine = min(mine, i);
    buf[0][t].sum = mine;
    __syncthreads();
    for (int d = TABLE_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) buf[0][t].sum = min(buf[0][t].sum, buf[0][t + d].sum);
        __syncthreads();
    }
    if (t == 0) overflow = buf[0][0].sum;
    __syncthreads();
    const bool over = overflow != 0x7fffffff;
    __syncthreads();
    // measures before a system within its piece: the scan restarts where the piece changes
    SegPair carry = {0, 0};
    for (int base = 0; base < n_systems; base += TABLE_THREADS) {
        const int i = base + t;
        SegPair v = {0, 0};
        if (i < n_systems) {
            v.sum = (over ? 0 : n_lines[i]) + 1;
            v.start = i == 0 || table[i].piece != table[i - 1].piece;
        }
        SegPair incl = block_seg_scan(v, buf);
        incl = seg_join(carry, incl);
        if (i < n_systems) {
            sys_first[i] = incl.sum - v.sum;
            if (i == n_systems - 1 || table[i + 1].piece != table[i].piece) piece_count[table[i].piece] = incl.sum;
        }
        if (t == TABLE_THREADS - 1) buf[0][0] = incl;
        __syncthreads();
        carry = buf[0][0];
        carry.start = 0;
        __syncthreads();
    }
    // the first row of every piece: a plain scan of the pieces' counts
    int before = 0;
    for (int base = 0; base < n_pieces; base += TABLE_THREADS) {
        const int q = base + t;
        SegPair v = {q < n_pieces ? piece_count[q] : 0, 0};
        const SegPair incl = block_seg_scan(v, buf);
        if (q < n_pieces) piece_first[q] = over ? 0 : before + incl.sum - v.sum;
        if (t == TABLE_THREADS - 1) buf[0][0] = incl;
        __syncthreads();
        before += buf[0][0].sum;
        __syncthreads();
    }
    if (t == 0) {
        piece_first[n_pieces] = over ? 0 : before;
        header[0] = over ? 0 : before;
        header[1] = over ? overflow : -1;
    }
    if (over) return;
    __syncthreads();                                                       // piece_first and sys_first of other threads
    for (int i = t; i < n_systems; i += TABLE_THREADS) {
        const ScoreSystem s = table[i];
        const int n = n_lines[i];
        const int32_t *b = lines + (int64_t)i * max_lines;
        int32_t *row = measures + ((int64_t)piece_first[s.piece] + sys_first[i]) * 8;
        int left = s.c0;
        for (int j = 0; j <= n; ++j, row += 8) {
            const int right = j < n ? b[j] : s.c0 + s.width;
            row[0] = s.x0 + (left - s.c0);
            row[1] = s.x0 + (right - s.c0);
            row[2] = s.page;
            row[3] = s.system;
            row[4] = left;
            row[5] = right;
            row[6] = s.r0;
            row[7] = s.r1;
            left = right;
        }
    }
}

}  // namespace

hipError_t launch_score_map_counts(hipStream_t s, const double *maps, const ScoreSystem *table, int n_systems,
                                   int64_t total_chunks, double threshold, int min_rows, unsigned long long *flags) {
    if (total_chunks <= 0) return hipSuccess;
    score_map_counts_kernel<<<dim3((unsigned)total_chunks), dim3(SCORE_MAP_THREADS), 0, s>>>(maps, table, n_systems,
                                                                                          threshold, min_rows, flags);
    return hipGetLastError();
}

hipError_t launch_score_map_lines(hipStream_t s, const ScoreSystem *table, int n_systems, const unsigned long long *flags,
                                  int tol, int max_lines, int32_t *n_lines, int32_t *lines) {
    if (n_systems <= 0) return hipSuccess;
    score_map_lines_kernel<<<dim3((unsigned)n_systems), dim3(64), 0, s>>>(table, flags, tol, max_lines, n_lines, lines);
    return hipGetLastError();
}

hipError_t launch_score_map_table(hipStream_t s, const ScoreSystem *table, int n_systems, int n_pieces, int max_lines,
                                  const int32_t *n_lines, const int32_t *lines, int32_t *piece_count, int32_t *piece_first,
                                  int32_t *header, int32_t *sys_first, int32_t *measures) {
    score_map_table_kernel<<<dim3(1), dim3(TABLE_THREADS), 0, s>>>(table, n_systems, n_pieces, max_lines, n_lines, lines,
                                                                   piece_count, piece_first, header, sys_first, measures);
    return hipGetLastError();
}

}  // namespace asr
