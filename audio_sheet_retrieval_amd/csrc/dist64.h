// float64 cosine distance of float32 code rows in scipy cdist_cosine's operation order - the bit-exact distance of the
// ranking (tail_rank_kernels.hip) and alignment (dtw_batch_kernels.hip) paths.
#pragma once
#include <hip/hip_runtime.h>

namespace asr {

// two accumulators (even k / odd k, summed at the end; odd tail element last).  Products of float32 values are exact
// in float64, so fma vs mul+add cannot differ; the explicit __dadd_rn/__dmul_rn only keep the compiler from
// re-associating.
__device__ __forceinline__ double dot2acc(const float *__restrict__ u, const float *__restrict__ v, int dim) {
    double a0 = 0.0, a1 = 0.0;
    const int m = dim & ~1;
    for (int k = 0; k < m; k += 2) {
        a0 = __dadd_rn(a0, __dmul_rn((double)u[k], (double)v[k]));
        a1 = __dadd_rn(a1, __dmul_rn((double)u[k + 1], (double)v[k + 1]));
    }
    double sacc = __dadd_rn(a0, a1);
    if (dim & 1) sacc = __dadd_rn(sacc, __dmul_rn((double)u[dim - 1], (double)v[dim - 1]));
    return sacc;
}

__device__ __forceinline__ double cos_dist(double dot, double na, double nb) {
    double c = __ddiv_rn(dot, __dmul_rn(na, nb));
    if (fabs(c) > 1.0) c = copysign(1.0, c);
    return __dsub_rn(1.0, c);
}

}  // namespace asr
