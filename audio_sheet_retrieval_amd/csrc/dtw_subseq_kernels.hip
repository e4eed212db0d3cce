// gfx950 kernel of the batched subsequence DTW (asr_dtw_subseq_batch_dev; include/asr_hip.h has the definition): where
// in a reference of S code rows does a query of Q <= 1024 code rows lie?  Distances, accumulated cost and traceback in
// one launch, one workgroup per pair, one lane per query row; the anti-diagonal is the time step: at step t lane i
// computes cell (i, t - i).
//
//   * a lane keeps its query row (float32) and norm in registers for the whole pair; the float64 cosine distance of a
//     cell (dot2acc + cos_dist of dist64.h, bit-exact with asr_dtw_dev) is computed where it is consumed and never
//     stored: the only per-cell traffic to device memory is one direction byte, cell (i, j) at (i + j) * Q + i, so a
//     step's stores are contiguous
//   * `left` is the lane's own previous value; `up` is lane i-1's previous value - one cross-lane move per step inside a
//     wave, two LDS slots (step parity) per wave boundary - and `diagonal` is the `up` of the step before
//   * reference rows are shared along the diagonal (lane i+1 needs at step t+1 the row lane i used at step t): they are
//     staged through a ring of 64 * waves + 2 * TILE rows in LDS, loaded a tile ahead (global loads issued at the start
//     of a tile of steps, written to LDS at its end).  The row stride is padded by 16 bytes to an odd number of 16-byte
//     slots, so the 16-byte reads of 64 lanes at consecutive rows spread over all banks; the pad carries the odd-dim
//     tail element and the row's float64 norm.  A workgroup whose ring does not fit (dim > 33 with more than 512 query
//     rows) reads the rows from global memory instead: same arithmetic, same results
//   * a pair with Q <= 64 is one wave and has no barrier; workgroups are launched per size class (64 * ceil(Q/64))
//   * lane Q-1 keeps the running first minimum of the last row; afterwards wave 0 walks the direction bytes back from
//     (Q-1, end), staging the bytes of 64 anti-diagonals x 65 rows around the current cell in LDS as
//     dtw_batch_traceback_kernel does, and writes start, path_len and pos
//
// Pairs are independent: no inter-workgroup communication, so neither batch composition nor order changes a result.
#include "asr_kernels.h"
#include "dist64.h"
#include <type_traits>

namespace asr {

namespace {

constexpr int SUB_TB_SPAN = 64;          // anti-diagonals staged per traceback round trip
constexpr int SUB_TILE_F4 = 128;         // 16-byte pieces of one staged tile of reference rows (2 per lane of one wave)
constexpr int SUB_STATIC_LDS = 8192;     // upper bound of the kernel's static LDS (traceback tile, boundary slots)

template <int NP> struct SubCfg {        // NP: pairs of elements a lane keeps of its query row (dim <= 2 * NP + 1)
    static constexpr int ROW = 2 * NP;                    // floats of the paired part of a row
    static constexpr int STRIDE = ROW + 4;                // + tail element [ROW], float64 norm [ROW + 2 .. ROW + 3]
    static constexpr int TILE = SUB_TILE_F4 * 4 / ROW;    // rows per staged tile: 16 (NP 16) / 8 (NP 32)
};

template <bool MULTI> __device__ __forceinline__ void sub_sync() {
    if (MULTI) {
        __syncthreads();
    } else {                                              // one wave: its LDS operations complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

}  // namespace

template <int NP, bool MULTI, bool REF_GLOBAL>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void dtw_subseq_kernel(
    const SubseqPair *__restrict__ pairs, const float *__restrict__ q, const double *__restrict__ nq,
    const float *__restrict__ r, const double *__restrict__ nr, int dim, uint8_t *__restrict__ dir,
    double *__restrict__ cost, int32_t *__restrict__ start, int32_t *__restrict__ end, int32_t *__restrict__ path_len,
    int32_t *__restrict__ pos) {
    using Cfg = SubCfg<NP>;
    constexpr int ROW = Cfg::ROW, STRIDE = Cfg::STRIDE, TILE = Cfg::TILE, F4_ROW = ROW / 4;
    extern __shared__ float4 sub_ring4[];
    __shared__ double bnd[2][16];                          // [step parity][wave]: the wave's lane 63 value
    __shared__ uint8_t tb_tile[SUB_TB_SPAN][SUB_TB_SPAN + 1];
    __shared__ int sh_end;
    float *ring = (float *)sub_ring4;

    const SubseqPair P = pairs[blockIdx.x];
    const int Q = P.Q, S = P.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
    const int m = dim & ~1;
    const bool odd = dim & 1;
    const int RING = nthr + 2 * TILE;
    const float *rp = r + P.r_row * dim;
    const double *nrp = nr + P.r_row;
    uint8_t *dp = dir + P.dir;
    const bool vec = (dim & 3) == 0 && (((uintptr_t)rp) & 15) == 0;

    // the lane's query row: pairs padded with zeros (adding an exact +0 changes no bit), the odd tail kept apart
    const int i = tid;
    const bool row_ok = i < Q;
    const int64_t qr = P.q_row + min(i, Q - 1);
    const float *qp = q + qr * dim;
    // (NP 16: as float64, converted once; NP 32: as float32, 64 registers - see qval)
    using QT = typename std::conditional<NP == 16, double, float>::type;
    QT qv[ROW];
#pragma unroll
    for (int k = 0; k < ROW; ++k) qv[k] = k < m ? (QT)qp[k] : (QT)0;
    auto qval = [&](int k) -> double {
        if constexpr (NP == 32) {
            // an empty statement the compiler cannot look through: without it the 64 conversions are hoisted out of
            // the step loop as 128 registers of float64
            asm volatile("" : "+v"(qv[k]));
        }
        return (double)qv[k];
    };
    const float qt = odd ? qp[dim - 1] : 0.f;
    const double qn = nq[qr];

    float4 pf[2];                                          // the tile in flight: 16-byte pieces tid + k * nthr
    float pft = 0.f;
    double pfn = 0.0;
    auto load_tile = [&](int row0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int f = tid + k * nthr;
            pf[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int row = row0 + f / F4_ROW, c = (f % F4_ROW) * 4;
            if (f < SUB_TILE_F4 && row < S && c < m) {
                const float *src = rp + (int64_t)row * dim + c;
                if (vec) {
                    pf[k] = *(const float4 *)src;
                } else {
                    pf[k].x = src[0];
                    pf[k].y = src[1];                      // c + 1 < m: c and m are even
                    if (c + 2 < m) { pf[k].z = src[2]; pf[k].w = src[3]; }
                }
            }
        }
        pft = 0.f;
        pfn = 1.0;
        if (tid < TILE && row0 + tid < S) {
            if (odd) pft = rp[(int64_t)(row0 + tid) * dim + dim - 1];
            pfn = nrp[row0 + tid];
        }
    };
    auto store_tile = [&](int row0) {
        const int s0 = row0 % RING;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int f = tid + k * nthr;
            if (f < SUB_TILE_F4) {
                int slot = s0 + f / F4_ROW;
                if (slot >= RING) slot -= RING;
                *(float4 *)(ring + slot * STRIDE + (f % F4_ROW) * 4) = pf[k];
            }
        }
        if (tid < TILE) {
            int slot = s0 + tid;
            if (slot >= RING) slot -= RING;
            ring[slot * STRIDE + ROW] = pft;
            *(double *)(ring + slot * STRIDE + ROW + 2) = pfn;
        }
    };

    if (tid < 32) bnd[tid >> 4][tid & 15] = (double)INFINITY;
    if (!REF_GLOBAL) {
        load_tile(0);
        store_tile(0);
    }
    sub_sync<MULTI>();

    const int nsteps = S + Q - 1;
    double cur = (double)INFINITY, diag = (double)INFINITY, best = (double)INFINITY;
    int bestj = 0;
    int slot = i == 0 ? 0 : RING - i;                      // ring slot of reference row t - i, once that is >= 0
    for (int t0 = 0; t0 < nsteps; t0 += TILE) {
        if (!REF_GLOBAL) load_tile(t0 + TILE);             // lands while this tile's steps run
        const int tend = min(t0 + TILE, nsteps);
        for (int t = t0; t < tend; ++t) {
            const int j = t - i;
            double up = __shfl_up(cur, 1);                 // lane i-1's value of step t-1: A[i-1][j]
            if (lane == 0) up = (MULTI && wave > 0) ? bnd[(t + 1) & 1][wave - 1] : (double)INFINITY;
            if (row_ok && j >= 0 && j < S) {
                double a0 = 0.0, a1 = 0.0, xt, nrj;
                if (!REF_GLOBAL) {
                    const float *row = ring + slot * STRIDE;
#pragma unroll
                    for (int k = 0; k < F4_ROW; ++k) {
                        const float4 x = *(const float4 *)(row + 4 * k);
                        a0 = __fma_rn(qval(4 * k), (double)x.x, a0);       // float32 products are exact in float64:
                        a1 = __fma_rn(qval(4 * k + 1), (double)x.y, a1);   // the fused form is dot2acc's mul + add
                        a0 = __fma_rn(qval(4 * k + 2), (double)x.z, a0);
                        a1 = __fma_rn(qval(4 * k + 3), (double)x.w, a1);
                    }
                    xt = (double)row[ROW];
                    nrj = *(const double *)(row + ROW + 2);
                } else {
                    const float *row = rp + (int64_t)j * dim;
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        if (2 * k < m) {
                            a0 = __fma_rn(qval(2 * k), (double)row[2 * k], a0);
                            a1 = __fma_rn(qval(2 * k + 1), (double)row[2 * k + 1], a1);
                        }
                    }
                    xt = odd ? (double)row[dim - 1] : 0.0;
                    nrj = nrp[j];
                }
                double sacc = __dadd_rn(a0, a1);
                if (odd) sacc = __dadd_rn(sacc, __dmul_rn((double)qt, xt));
                const double d = cos_dist(sacc, qn, nrj);
                uint8_t w = 0;                             // _traceback: argmin over (diagonal, up, left), strict <
                double bst = diag;
                if (up < bst) { bst = up; w = 1; }
                if (cur < bst) w = 2;
                const double v = i == 0 ? d : __dadd_rn(d, fmin(diag, fmin(up, cur)));   // row 0: free start
                cur = v;
                dp[(int64_t)t * Q + i] = w;
                if (i == Q - 1 && v < best) { best = v; bestj = j; }
            }
            diag = up;
            if (++slot == RING) slot = 0;
            if (MULTI) {
                if (lane == 63) bnd[t & 1][wave] = cur;
                __syncthreads();
            }
        }
        if (!REF_GLOBAL) {
            store_tile(t0 + TILE);
            sub_sync<MULTI>();
        }
    }

    if (i == Q - 1) {
        cost[P.out] = __ddiv_rn(best, (double)Q);
        end[P.out] = bestj;
        sh_end = bestj;
    }
    __threadfence_block();
    __syncthreads();                                       // the direction bytes of every wave are visible to wave 0
    if (tid >= 64) return;

    int ti = Q - 1, tj = sh_end, n = 1;
    int32_t *pp = pos ? pos + P.pos : nullptr;
    while (ti > 0) {
        const int d0 = ti + tj, r0 = ti - SUB_TB_SPAN;
        for (int tt = 0; tt < SUB_TB_SPAN && d0 - tt >= 0; ++tt) {
            const int d = d0 - tt;
            for (int c = lane; c <= SUB_TB_SPAN; c += 64) {
                const int rr = r0 + c, jj = d - rr;
                if (rr >= 0 && rr < Q && jj >= 0 && jj < S) tb_tile[tt][c] = dp[(int64_t)d * Q + rr];
            }
        }
        sub_sync<false>();
        if (lane == 0) {
            while (ti > 0 && ti + tj > d0 - SUB_TB_SPAN) {
                int w = tb_tile[d0 - (ti + tj)][ti - r0];
                if (tj == 0) w = 1;                        // column 0 has one finite predecessor (guards NaN input)
                if (w != 2 && pp) pp[ti] = tj;             // the walk leaves row ti: tj is its smallest column
                ti -= w != 2;
                tj -= w != 1;
                ++n;
            }
        }
        ti = __shfl(ti, 0);
        tj = __shfl(tj, 0);
        n = __shfl(n, 0);
        sub_sync<false>();                                 // the tile is read before the next round overwrites it
    }
    if (lane == 0) {
        if (pp) pp[0] = tj;
        start[P.out] = tj;
        path_len[P.out] = n;
    }
}

namespace {

template <int NP>
hipError_t launch_subseq_np(hipStream_t s, const SubseqPair *pairs, int n_pairs, int waves, size_t lds_limit,
                            const float *q, const double *nq, const float *r, const double *nr, int dim, uint8_t *dir,
                            double *cost, int32_t *start, int32_t *end, int32_t *path_len, int32_t *pos) {
    const size_t bytes = dtw_subseq_lds_bytes(waves, dim);
    const int threads = 64 * waves;
    if (waves == 1) {
        dtw_subseq_kernel<NP, false, false><<<n_pairs, threads, bytes, s>>>(pairs, q, nq, r, nr, dim, dir, cost, start,
                                                                            end, path_len, pos);
    } else if (bytes + SUB_STATIC_LDS <= lds_limit) {
        if (bytes + SUB_STATIC_LDS > 65536) {              // above the default dynamic-LDS limit (gfx950: 160 KiB)
            hipError_t e = hipFuncSetAttribute((const void *)dtw_subseq_kernel<NP, true, false>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
        dtw_subseq_kernel<NP, true, false><<<n_pairs, threads, bytes, s>>>(pairs, q, nq, r, nr, dim, dir, cost, start,
                                                                           end, path_len, pos);
    } else {
        dtw_subseq_kernel<NP, true, true><<<n_pairs, threads, 0, s>>>(pairs, q, nq, r, nr, dim, dir, cost, start, end,
                                                                      path_len, pos);
    }
    return hipGetLastError();
}

}  // namespace

size_t dtw_subseq_lds_bytes(int waves, int dim) {
    if (dim < 1 || dim > 64 || waves < 1 || waves > 16) return 0;
    const int stride = dim <= 33 ? SubCfg<16>::STRIDE : SubCfg<32>::STRIDE;
    const int tile = dim <= 33 ? SubCfg<16>::TILE : SubCfg<32>::TILE;
    return (size_t)(64 * waves + 2 * tile) * stride * sizeof(float);
}

hipError_t launch_dtw_subseq(hipStream_t s, const SubseqPair *pairs, int n_pairs, int waves, size_t lds_limit,
                             const float *q, const double *nq, const float *r, const double *nr, int dim, uint8_t *dir,
                             double *cost, int32_t *start, int32_t *end, int32_t *path_len, int32_t *pos) {
    if (dim <= 33)
        return launch_subseq_np<16>(s, pairs, n_pairs, waves, lds_limit, q, nq, r, nr, dim, dir, cost, start, end,
                                    path_len, pos);
    return launch_subseq_np<32>(s, pairs, n_pairs, waves, lds_limit, q, nq, r, nr, dim, dir, cost, start, end, path_len,
                                pos);
}

}  // namespace asr
