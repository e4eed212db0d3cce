// gfx950 kernels of the batched alignment DTW (asr_dtw_batch_dev).  Every (a, b) code-sequence
// pair of a batch is aligned as dtw_by_dist(cdist(a, b, "cosine")) (utils/dtw_by_dist.py:5-34, _traceback :76-91),
// bit-exact with asr_dtw_dev (tail_rank_kernels.hip: dtw_dist_kernel / dtw_accumulate_kernel), all pairs per launch:
//
//   dtw_batch_dist_kernel      : the float64 cosine distance of every cell of every pair (dot2acc + cos_dist, the
//                                arithmetic of dtw_dist_kernel), one workgroup per anti-diagonal over the whole grid,
//                                stored anti-diagonal-major per pair (the order the wavefront reads it); optionally a
//                                row-major copy for the caller
//   dtw_batch_wave_kernel      : one workgroup per pair.  The accumulated cost lives in three rotating anti-diagonal
//                                buffers - in LDS (template <false>), or, for pairs whose diagonals do not fit, in a
//                                per-pair global ring (<true>).  Per cell it stores one byte: which predecessor won
//                                (0 diagonal, 1 up (i-1,j), 2 left (i,j-1)), chosen with _traceback's strict-< first
//                                minimum on the same accumulated values, i.e. exactly the traceback's argmin
//   dtw_batch_traceback_kernel : one wave per pair walks the direction bytes back from (R-1, C-1).  It stages the bytes
//                                of the next 64 anti-diagonals around the current cell (rows i-64..i) in LDS and walks
//                                from there, >= 32 steps per global round trip; writes the path in forward order and
//                                the first-entry projections (align_pydtw's `np.flatnonzero(path[0] == col)[0]`)
//
// Pairs are independent: no inter-workgroup communication, so neither batch composition nor order changes a result.
#include "asr_kernels.h"
#include "dist64.h"

namespace asr {

namespace {

constexpr int WAVE_THREADS = 512;
constexpr int WAVE_PREFETCH = 14;        // next-diagonal distances held per thread: 512 * 14 >= 6826 LDS slots
constexpr int TB_SPAN = 64;              // anti-diagonals staged per traceback round trip

// cells on the anti-diagonals 0 .. d-1 of an R x C matrix (diagonal d: i + j == d)
__device__ __forceinline__ int64_t diag_first_cell(int64_t d, int64_t R, int64_t C) {
    const int64_t s1 = d <= R ? d * (d + 1) / 2 : R * (R + 1) / 2 + (d - R) * R;
    const int64_t m = d - C;
    return s1 - (m > 0 ? m * (m + 1) / 2 : 0);
}

}  // namespace

// one workgroup per anti-diagonal (grid-stride over the chunk's diagonals); cell k of diagonal d = row ilo(d) + k
__global__ __launch_bounds__(256) void dtw_batch_dist_kernel(const DtwPair *__restrict__ pairs, int n_pairs,
                                                             int64_t n_diags, const float *__restrict__ a,
                                                             const double *__restrict__ na, const float *__restrict__ b,
                                                             const double *__restrict__ nb, int dim,
                                                             double *__restrict__ cost, double *__restrict__ rm_out) {
    for (int64_t g = blockIdx.x; g < n_diags; g += gridDim.x) {
        int lo = 0, hi = n_pairs - 1;                      // the pair whose diagonals contain g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pairs[mid].diag <= g) lo = mid; else hi = mid - 1;
        }
        const DtwPair P = pairs[lo];
        const int d = (int)(g - P.diag);
        const int ilo = max(0, d - P.C + 1), ihi = min(d, P.R - 1);
        double *out = cost + P.cell + diag_first_cell(d, P.R, P.C) - ilo;
        for (int i = ilo + (int)threadIdx.x; i <= ihi; i += blockDim.x) {
            const int j = d - i;
            const int64_t ra = P.a_row + i, rb = P.b_row + j;
            const double v = cos_dist(dot2acc(a + ra * dim, b + rb * dim, dim), na[ra], nb[rb]);
            out[i] = v;
            if (P.rm >= 0) rm_out[P.rm + (int64_t)i * P.C + j] = v;
        }
    }
}

// Accumulated cost acc(i,j) = cost(i,j) + min(acc(i-1,j-1), acc(i-1,j), acc(i,j-1)) with acc(-1,-1) = 0 and an
// infinite border.  A diagonal buffer has S = min(R,C) + 1 slots, slot = (row if R <= C, else column) + 1; slot 0 is
// the border (infinite from diagonal -1 on; the corner 0 sits in diagonal -2's buffer).  Border cells of column / row
// -1 land in slots no earlier diagonal of that buffer wrote (those stay infinite from the initialisation).  Diagonal t
// uses buffer (t + 2) % 3.
template <bool GLOBAL_RING>
__global__ __launch_bounds__(WAVE_THREADS) void dtw_batch_wave_kernel(const DtwPair *__restrict__ pairs,
                                                                      const double *__restrict__ cost,
                                                                      uint8_t *__restrict__ dir, double *__restrict__ ring,
                                                                      double *__restrict__ min_dist) {
    extern __shared__ double lds_diag[];
    const DtwPair P = pairs[blockIdx.x];
    if ((P.ring >= 0) != GLOBAL_RING) return;             // the other instance handles this pair
    const int R = P.R, C = P.C, tid = threadIdx.x, nd = R + C - 1;
    const bool by_row = R <= C;
    const int S = (by_row ? R : C) + 1;
    double *buf = GLOBAL_RING ? ring + P.ring : lds_diag;
    for (int s = tid; s < 3 * S; s += WAVE_THREADS) buf[s] = s == 0 ? 0.0 : (double)INFINITY;
    if (GLOBAL_RING) __threadfence_block();
    __syncthreads();
    const double *cp = cost + P.cell;
    uint8_t *dp = dir + P.cell;

    double pf[WAVE_PREFETCH];                              // LDS variant: distances of the next diagonal, in flight
    if (!GLOBAL_RING) {
#pragma unroll
        for (int m = 0; m < WAVE_PREFETCH; ++m) pf[m] = tid + m * WAVE_THREADS < 1 ? cp[tid + m * WAVE_THREADS] : 0.0;
    }
    int64_t off = 0;                                       // first cell of diagonal d
    for (int d = 0; d < nd; ++d) {
        double *cur = buf + ((d + 2) % 3) * S;
        const double *prev = buf + ((d + 1) % 3) * S, *prev2 = buf + (d % 3) * S;
        const int ilo = max(0, d - C + 1), ihi = min(d, R - 1), len = ihi - ilo + 1;
        if (tid == 0) cur[0] = (double)INFINITY;
        auto cell = [&](int k, double c) {
            const int i = ilo + k, j = d - i;
            const int s = (by_row ? i : j) + 1;
            const double up = by_row ? prev[s - 1] : prev[s];
            const double left = by_row ? prev[s] : prev[s - 1];
            const double dg = prev2[s - 1];
            uint8_t w = 0;                                 // _traceback: argmin over (diagonal, up, left), strict <
            double best = dg;
            if (up < best) { best = up; w = 1; }
            if (left < best) w = 2;
            const double v = c + fmin(dg, fmin(up, left)); // dtw_accumulate_kernel's D += min3
            cur[s] = v;
            dp[off + k] = w;
            if (d == nd - 1) min_dist[blockIdx.x] = v / (double)(R + C);
        };
        if (!GLOBAL_RING) {
            double cv[WAVE_PREFETCH];
#pragma unroll
            for (int m = 0; m < WAVE_PREFETCH; ++m) cv[m] = pf[m];
            if (d + 1 < nd) {                              // issue the next diagonal's loads before this one's work
                const int nlen = min(d + 1, R - 1) - max(0, d + 2 - C) + 1;
#pragma unroll
                for (int m = 0; m < WAVE_PREFETCH; ++m) {
                    const int k = tid + m * WAVE_THREADS;
                    if (k < nlen) pf[m] = cp[off + len + k];
                }
            }
#pragma unroll
            for (int m = 0; m < WAVE_PREFETCH; ++m) {
                const int k = tid + m * WAVE_THREADS;
                if (k < len) cell(k, cv[m]);
            }
        } else {
            for (int k = tid; k < len; k += WAVE_THREADS) cell(k, cp[off + k]);
            __threadfence_block();
        }
        off += len;
        __syncthreads();
    }
}

// One wave per pair.  path_*: capacity R + C entries at P.path; the walk writes them backwards from the end of the
// capacity, then the wave moves the path to the front (forward order).  first_a[i]: column of the first path entry in
// row i; first_b[j]: row of the first path entry in column j.
__global__ __launch_bounds__(64) void dtw_batch_traceback_kernel(const DtwPair *__restrict__ pairs,
                                                                 const uint8_t *__restrict__ dir,
                                                                 int32_t *__restrict__ path_a, int32_t *__restrict__ path_b,
                                                                 int32_t *__restrict__ path_len,
                                                                 int32_t *__restrict__ first_a,
                                                                 int32_t *__restrict__ first_b) {
    __shared__ uint8_t tile[TB_SPAN][TB_SPAN + 1];         // [d0 - diagonal][row - (i0 - 64)]
    __shared__ int sh_state[3];
    const DtwPair P = pairs[blockIdx.x];
    const int R = P.R, C = P.C, lane = threadIdx.x, cap = R + C;
    const uint8_t *dp = dir + P.cell;
    int32_t *pa = path_a + P.path, *pb = path_b + P.path;
    int i = R - 1, j = C - 1, n = 1;
    if (lane == 0) { pa[cap - 1] = i; pb[cap - 1] = j; }
    while (i > 0 || j > 0) {
        const int d0 = i + j, r0 = i - TB_SPAN;
        for (int t = 0; t < TB_SPAN && d0 - t >= 0; ++t) {
            const int d = d0 - t;
            const int ilo = max(0, d - C + 1), ihi = min(d, R - 1);
            const uint8_t *row = dp + diag_first_cell(d, R, C) - ilo;
            for (int c = lane; c <= TB_SPAN; c += 64) {
                const int r = r0 + c;
                if (r >= ilo && r <= ihi) tile[t][c] = row[r];
            }
        }
        __syncthreads();
        if (lane == 0) {
            while ((i > 0 || j > 0) && i + j > d0 - TB_SPAN) {
                const int w = tile[d0 - (i + j)][i - r0];
                if (w != 1 && first_b) first_b[P.fb + j] = i;      // the walk leaves column j: (i, j) is its first entry
                if (w != 2 && first_a) first_a[P.fa + i] = j;
                i -= w != 2;
                j -= w != 1;
                ++n;
                pa[cap - n] = i;
                pb[cap - n] = j;
            }
            sh_state[0] = i; sh_state[1] = j; sh_state[2] = n;
        }
        __syncthreads();
        i = sh_state[0]; j = sh_state[1]; n = sh_state[2];
    }
    if (lane == 0) {
        if (first_b) first_b[P.fb] = 0;
        if (first_a) first_a[P.fa] = 0;
        path_len[blockIdx.x] = n;
    }
    __threadfence_block();
    __syncthreads();
    const int shift = cap - n;                             // >= 0; every chunk is read before it is written
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        int32_t va = 0, vb = 0;
        if (k < n) { va = pa[shift + k]; vb = pb[shift + k]; }
        __syncthreads();
        if (k < n) { pa[k] = va; pb[k] = vb; }
    }
}

int dtw_batch_lds_slots(int device) {
    int bytes = 0;
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) bytes = 65536;
    return std::min(bytes / (3 * (int)sizeof(double)), WAVE_PREFETCH * WAVE_THREADS + 1);   // + the prefetch registers
}

hipError_t launch_dtw_batch_dist(hipStream_t s, const DtwPair *pairs, int n_pairs, int64_t n_diags, const float *a,
                                 const double *na, const float *b, const double *nb, int dim, double *cost,
                                 double *rm_out) {
    const int blocks = (int)std::min<int64_t>(n_diags, 65536);
    dtw_batch_dist_kernel<<<blocks, 256, 0, s>>>(pairs, n_pairs, n_diags, a, na, b, nb, dim, cost, rm_out);
    return hipGetLastError();
}

hipError_t launch_dtw_batch_wave(hipStream_t s, const DtwPair *pairs, int n_pairs, int lds_slots, bool any_ring,
                                 const double *cost, uint8_t *dir, double *ring, double *min_dist) {
    if (lds_slots > 0) {
        const size_t bytes = (size_t)3 * lds_slots * sizeof(double);
        if (bytes > 65536) {                               // above the default dynamic-LDS limit (gfx950: 160 KiB)
            hipError_t e = hipFuncSetAttribute((const void *)dtw_batch_wave_kernel<false>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
        dtw_batch_wave_kernel<false><<<n_pairs, WAVE_THREADS, bytes, s>>>(pairs, cost, dir, ring, min_dist);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (any_ring) dtw_batch_wave_kernel<true><<<n_pairs, WAVE_THREADS, 0, s>>>(pairs, cost, dir, ring, min_dist);
    return hipGetLastError();
}

hipError_t launch_dtw_batch_traceback(hipStream_t s, const DtwPair *pairs, int n_pairs, const uint8_t *dir,
                                      int32_t *path_a, int32_t *path_b, int32_t *path_len, int32_t *first_a,
                                      int32_t *first_b) {
    dtw_batch_traceback_kernel<<<n_pairs, 64, 0, s>>>(pairs, dir, path_a, path_b, path_len, first_a, first_b);
    return hipGetLastError();
}

}  // namespace asr
