// gfx950 kernel for the unrolled score strips of scanned pages (reference: umc_a2s_server.py:136-158, the loop that
// cuts every detected staff system out of its page and puts the systems of a piece side by side).
//
//   unroll_systems_kernel : all systems of all pages of all pieces in one launch.  One workgroup per (system, strip
//                           row): the row is contiguous in the uint8 page and in the float32 strip, so consecutive
//                           lanes read consecutive bytes and write consecutive floats.  Rows below the last source
//                           row repeat it (np.pad mode="edge", :156).  A pure copy: HBM bound, 1 byte in, 4 bytes out
//                           per pixel.
#include "asr_kernels.h"

namespace asr {

__global__ __launch_bounds__(256) void unroll_systems_kernel(const uint8_t *__restrict__ pages,
                                                             const UnrollSystem *__restrict__ systems, int64_t n_jobs,
                                                             int system_height, float *__restrict__ strips) {
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int i = (int)(job / system_height);
        const int y = (int)(job - (int64_t)i * system_height);
        const UnrollSystem s = systems[i];
        const int sy = y < s.rows ? y : s.rows - 1;
        const uint8_t *src = pages + s.src + (int64_t)sy * s.src_stride;
        float *dst = strips + s.dst + (int64_t)y * s.dst_stride;
        for (int x = threadIdx.x; x < s.width; x += 256) dst[x] = (float)src[x];
    }
}

hipError_t launch_unroll_systems(hipStream_t s, const uint8_t *pages, const UnrollSystem *systems_dev, int n_systems,
                                 int system_height, float *strips) {
    const int64_t n_jobs = (int64_t)n_systems * system_height;
    if (n_jobs == 0) return hipSuccess;
    const int blocks = (int)std::min<int64_t>(n_jobs, 1 << 16);
    unroll_systems_kernel<<<blocks, 256, 0, s>>>(pages, systems_dev, n_jobs, system_height, strips);
    return hipGetLastError();
}

}  // namespace asr
