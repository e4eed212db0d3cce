// gfx950 kernel of the streaming subsequence DTW (asr_dtw_follow_batch_dev; include/asr_hip.h has the definition): a
// block of B <= 1024 new query rows continues the accumulated-cost matrix of a stream against a reference of S code rows
// from the one row it kept, and reports per new row where the best path so far ends and where it started.
//
// The schedule is dtw_subseq_kernel's (dtw_subseq_kernels.hip): one workgroup per pair, one lane per block row, the
// anti-diagonal is the time step (at step t lane i computes cell (i, t - i)), workgroups launched per size class
// 64 * ceil(B / 64), reference rows staged through the padded LDS ring a tile ahead or read from global memory when the
// ring does not fit.  SubCfg, the ring layout and the arithmetic of a cell are copies of that file's, so a cell's value
// is the same sequence of correctly rounded float64 operations.  What differs:
//
//   * lane 0's predecessors are the carried row: up = acc[j], diagonal = acc[j - 1] (the `up` of the step before),
//     unless the pair is fresh (n0 == 0: row 0 is the free start and the state is not read).  The state is staged a
//     tile ahead like the reference rows - lanes TILE..2*TILE-1 load acc / org of the next tile's columns at the start
//     of a tile of steps and write them to one of two LDS buffers at its end - so lane 0's read of a step is an LDS
//     read at an address that depends on t alone.  (Those lanes carry the state in the registers in which lanes
//     0..TILE-1 carry the rows' tail element and norm, and every lane has one 16-byte piece of a tile in flight - a one-
//     wave workgroup stages tiles of half the rows - which keeps every instantiation within 128 VGPRs)
//   * every cell carries the column at which its best path started: `org` travels with `cur` (a second __shfl_up, an
//     int beside the double in the wave-boundary slots) and a cell takes the origin of the predecessor _traceback's
//     rule picks (diagonal, up, left; strict <).  There are no direction bytes and there is no traceback
//   * every lane keeps the running first minimum of its own row (value, column, origin) and writes its three outputs
//     once, after its row
//   * the lane of the last block row writes acc[j] / org[j] at every step: afterwards the state is row n0 + B - 1
//
// The state is updated in place.  Index j is read by the prefetch at the start of the tile of steps before the one that
// holds step j (the first tile: before the loop) and the loaded registers are consumed by the LDS write and the
// workgroup barrier that end that tile; index j is written at step j + B - 1 >= j, which lies after that barrier.  So
// every read of an index completes before its write is issued, for every B >= 1.  Keep this order.
//
// Pairs are independent (their state ranges must not overlap): neither batch composition nor order changes a result.
#include "asr_kernels.h"
#include "dist64.h"
#include <type_traits>

namespace asr {

namespace {

// 16-byte pieces of one staged tile of reference rows: one per lane in flight (several waves: of the first two waves)
constexpr int fol_tile_f4(bool multi) { return multi ? 128 : 64; }
constexpr int FOL_STATIC_LDS = 1024;     // upper bound of the kernel's static LDS (boundary slots, state tiles)

template <int NP, bool MULTI> struct FolCfg {   // SubCfg of dtw_subseq_kernels.hip; one wave stages half its tile
    static constexpr int ROW = 2 * NP;                    // floats of the paired part of a row
    static constexpr int STRIDE = ROW + 4;                // + tail element [ROW], float64 norm [ROW + 2 .. ROW + 3]
    static constexpr int TILE_F4 = fol_tile_f4(MULTI);
    static constexpr int TILE = TILE_F4 * 4 / ROW;        // rows per staged tile: 16 (NP 16) / 8 (NP 32); one wave 8 / 4
};

template <bool MULTI> __device__ __forceinline__ void fol_sync() {
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
__global__ __launch_bounds__(MULTI ? 1024 : 64) void dtw_follow_kernel(
    const FollowPair *__restrict__ pairs, const float *__restrict__ q, const double *__restrict__ nq,
    const float *__restrict__ r, const double *__restrict__ nr, int dim, double *acc, int32_t *org,
    double *__restrict__ cost, int32_t *__restrict__ start, int32_t *__restrict__ pos) {
    using Cfg = FolCfg<NP, MULTI>;
    constexpr int ROW = Cfg::ROW, STRIDE = Cfg::STRIDE, TILE = Cfg::TILE, F4_ROW = ROW / 4, TILE_F4 = Cfg::TILE_F4;
    extern __shared__ float4 fol_ring4[];
    __shared__ double bnd[2][16];                          // [step parity][wave]: the wave's lane 63 value ...
    __shared__ int32_t bnd_o[2][16];                       // ... and its origin
    __shared__ double st_acc[2][TILE];                     // [tile parity][step of the tile]: the carried row
    __shared__ int32_t st_org[2][TILE];
    float *ring = (float *)fol_ring4;

    const FollowPair P = pairs[blockIdx.x];
    const int B = P.B, S = P.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
    const bool fresh = P.n0 == 0;
    const int m = dim & ~1;
    const bool odd = dim & 1;
    const int RING = nthr + 2 * TILE;
    const float *rp = r + P.r_row * dim;
    const double *nrp = nr + P.r_row;
    double *accp = acc + P.state;
    int32_t *orgp = org + P.state;
    const bool vec = (dim & 3) == 0 && (((uintptr_t)rp) & 15) == 0;

    // the lane's query row: pairs padded with zeros (adding an exact +0 changes no bit), the odd tail kept apart
    const int i = tid;
    const bool row_ok = i < B;
    const int64_t qr = P.q_row + min(i, B - 1);
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

    float4 pf;                                             // the tile in flight: 16-byte piece tid
    // one float and one double per lane carry the rest: lanes [0, TILE) the rows' tail element and norm, lanes
    // [TILE, 2 * TILE) the state of the tile's columns (org as bits, acc)
    float pft = 0.f;
    double pfn = 0.0;
    auto load_tile = [&](int row0) {
        if (!REF_GLOBAL) {
            pf = make_float4(0.f, 0.f, 0.f, 0.f);
            const int row = row0 + tid / F4_ROW, c = (tid % F4_ROW) * 4;
            if (tid < TILE_F4 && row < S && c < m) {
                const float *src = rp + (int64_t)row * dim + c;
                if (vec) {
                    pf = *(const float4 *)src;
                } else {
                    pf.x = src[0];
                    pf.y = src[1];                         // c + 1 < m: c and m are even
                    if (c + 2 < m) { pf.z = src[2]; pf.w = src[3]; }
                }
            }
        }
        pft = 0.f;
        pfn = tid < TILE ? 1.0 : (double)INFINITY;
        if (tid < TILE) {
            if (!REF_GLOBAL && row0 + tid < S) {
                if (odd) pft = rp[(int64_t)(row0 + tid) * dim + dim - 1];
                pfn = nrp[row0 + tid];
            }
        } else if (tid < 2 * TILE && !fresh && row0 + tid - TILE < S) {
            pfn = accp[row0 + tid - TILE];
            pft = __int_as_float(orgp[row0 + tid - TILE]);
        }
    };
    auto store_tile = [&](int row0) {
        if (!REF_GLOBAL) {
            const int s0 = row0 % RING;
            if (tid < TILE_F4) {
                int slot = s0 + tid / F4_ROW;
                if (slot >= RING) slot -= RING;
                *(float4 *)(ring + slot * STRIDE + (tid % F4_ROW) * 4) = pf;
            }
            if (tid < TILE) {
                int slot = s0 + tid;
                if (slot >= RING) slot -= RING;
                ring[slot * STRIDE + ROW] = pft;
                *(double *)(ring + slot * STRIDE + ROW + 2) = pfn;
            }
        }
        if (tid >= TILE && tid < 2 * TILE) {
            st_acc[(row0 / TILE) & 1][tid - TILE] = pfn;
            st_org[(row0 / TILE) & 1][tid - TILE] = __float_as_int(pft);
        }
    };

    if (tid < 32) {
        bnd[tid >> 4][tid & 15] = (double)INFINITY;
        bnd_o[tid >> 4][tid & 15] = 0;
    }
    load_tile(0);
    store_tile(0);
    fol_sync<MULTI>();

    const int nsteps = S + B - 1;
    double cur = (double)INFINITY, diag = (double)INFINITY, best = (double)INFINITY;
    int32_t ocur = 0, odiag = 0, bestj = 0, besto = 0;
    int slot = i == 0 ? 0 : RING - i;                      // ring slot of reference row t - i, once that is >= 0
    for (int t0 = 0; t0 < nsteps; t0 += TILE) {
        load_tile(t0 + TILE);                              // lands while this tile's steps run
        const int tend = min(t0 + TILE, nsteps), par = (t0 / TILE) & 1;
        for (int t = t0; t < tend; ++t) {
            const int j = t - i;
            double up = __shfl_up(cur, 1);                 // lane i-1's value of step t-1: A[i-1][j] ...
            int32_t oup = __shfl_up(ocur, 1);              // ... and its origin
            if (lane == 0) {
                if (MULTI && wave > 0) {
                    up = bnd[(t + 1) & 1][wave - 1];
                    oup = bnd_o[(t + 1) & 1][wave - 1];
                } else {                                   // the carried row (+inf when fresh or past column S - 1)
                    up = st_acc[par][t - t0];
                    oup = st_org[par][t - t0];
                }
            }
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
                int32_t o = odiag;                         // _traceback: argmin over (diagonal, up, left), strict <
                double bst = diag;
                if (up < bst) { bst = up; o = oup; }
                if (cur < bst) o = ocur;
                double v = __dadd_rn(d, fmin(diag, fmin(up, cur)));
                if (i == 0 && fresh) { v = d; o = j; }     // global row 0: free start
                cur = v;
                ocur = o;
                if (v < best) { best = v; bestj = j; besto = o; }
                if (i == B - 1) {                          // in place: see the note on the order at the top
                    accp[j] = v;
                    orgp[j] = o;
                }
            }
            diag = up;
            odiag = oup;
            if (++slot == RING) slot = 0;
            if (MULTI) {
                if (lane == 63) {
                    bnd[t & 1][wave] = cur;
                    bnd_o[t & 1][wave] = ocur;
                }
                __syncthreads();
            }
        }
        store_tile(t0 + TILE);
        fol_sync<MULTI>();
    }

    if (row_ok) {
        if (cost) cost[P.out + i] = __ddiv_rn(best, (double)(P.n0 + i + 1));
        if (start) start[P.out + i] = besto;
        if (pos) pos[P.out + i] = bestj;
    }
}

namespace {

template <int NP>
hipError_t launch_follow_np(hipStream_t s, const FollowPair *pairs, int n_pairs, int waves, size_t lds_limit,
                            const float *q, const double *nq, const float *r, const double *nr, int dim, double *acc,
                            int32_t *org, double *cost, int32_t *start, int32_t *pos) {
    const size_t bytes = dtw_follow_lds_bytes(waves, dim);
    const int threads = 64 * waves;
    if (waves == 1) {                                      // one wave's ring (at most 10 KiB) always fits
        dtw_follow_kernel<NP, false, false><<<n_pairs, threads, bytes, s>>>(pairs, q, nq, r, nr, dim, acc, org, cost,
                                                                            start, pos);
    } else if (bytes + FOL_STATIC_LDS <= lds_limit) {
        if (bytes + FOL_STATIC_LDS > 65536) {              // above the default dynamic-LDS limit (gfx950: 160 KiB)
            hipError_t e = hipFuncSetAttribute((const void *)dtw_follow_kernel<NP, true, false>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
        dtw_follow_kernel<NP, true, false><<<n_pairs, threads, bytes, s>>>(pairs, q, nq, r, nr, dim, acc, org, cost,
                                                                           start, pos);
    } else {
        dtw_follow_kernel<NP, true, true><<<n_pairs, threads, 0, s>>>(pairs, q, nq, r, nr, dim, acc, org, cost, start,
                                                                      pos);
    }
    return hipGetLastError();
}

}  // namespace

size_t dtw_follow_lds_bytes(int waves, int dim) {
    if (dim < 1 || dim > 64 || waves < 1 || waves > 16) return 0;
    const int stride = dim <= 33 ? FolCfg<16, true>::STRIDE : FolCfg<32, true>::STRIDE;
    const int tile = waves > 1 ? (dim <= 33 ? FolCfg<16, true>::TILE : FolCfg<32, true>::TILE)
                               : (dim <= 33 ? FolCfg<16, false>::TILE : FolCfg<32, false>::TILE);
    return (size_t)(64 * waves + 2 * tile) * stride * sizeof(float);
}

hipError_t launch_dtw_follow(hipStream_t s, const FollowPair *pairs, int n_pairs, int waves, size_t lds_limit,
                             const float *q, const double *nq, const float *r, const double *nr, int dim, double *acc,
                             int32_t *org, double *cost, int32_t *start, int32_t *pos) {
    if (dim <= 33)
        return launch_follow_np<16>(s, pairs, n_pairs, waves, lds_limit, q, nq, r, nr, dim, acc, org, cost, start, pos);
    return launch_follow_np<32>(s, pairs, n_pairs, waves, lds_limit, q, nq, r, nr, dim, acc, org, cost, start, pos);
}

}  // namespace asr
