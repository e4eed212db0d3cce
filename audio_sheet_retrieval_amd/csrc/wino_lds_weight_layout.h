// Where conv3x3_wino (conv_wino_kernels.hip, the LDS-patch kernel) keeps a transformed weight in LDS, as plain integer
// arithmetic shared by the kernel's staging loop, its operand reads, the launcher's LDS request (enumerate_wino) and
// a host test (tests/test_wino_lds_weight_layout_host.py builds tests/wino_lds_weight_layout_harness.cpp for the CPU
// under ASan + UBSan).  conv3x3_winog has its own header, wino_weight_layout.h.
//
// The packed weights in global memory are wpk[row][coutp] with row = (k-step * 16 + position) * 4 + g (g = the
// channel inside the k-step of 4) and a workgroup stages the NTW n-tiles of its group: columns col = nt * 16 + n.
// Lane (g, n) of a wave feeds its MFMAs element (g, n) of every (k-step, position, n-tile).
//
//   row-major form:  [row][stride]: one dword per operand.  NTW = 2 pads the stride to 48 (32 puts lane groups g and
//                    g + 1 on the same banks) and reads the two n-tiles as a pair of dwords 16 apart, whose 8-bit
//                    offsets need a new base register every 1 KiB.
//   dense form:      every read is ONE aligned 8-byte read per lane, 512 contiguous bytes per wave (conflict-free),
//                    at a 16-bit immediate offset from one base register:
//                      NTW = 2: [k-step][position][g][n][nt]           - the lane's two n-tiles of a (k-step, position)
//                      NTW = 1: [k-step][position pair][g][n][2]       - the lane's operands of positions 2j and 2j + 1
//                    Read r of the kernel (r = k-step * 16 + position, or k-step * 8 + pair) starts 128 r floats past
//                    the lane's offset.  No pad column: 16 * C_in * 16 NTW floats.
//
// Which form an instantiation takes is a compile-time choice (wino_lw_dense): the producer builds (PW > 0) keep the
// row-major form, and so would any build that the dense form made spill or drop an occupancy step.
#pragma once

#if defined(__HIPCC__)
#define ASR_LWLAY_HD __host__ __device__ __forceinline__ constexpr
#else
#define ASR_LWLAY_HD inline constexpr
#endif

namespace asr {

ASR_LWLAY_HD bool wino_lw_dense(int ntw, int pw) { return pw == 0 && (ntw == 1 || ntw == 2); }

// row stride of the row-major form
ASR_LWLAY_HD int wino_lw_row_stride(int ntw) { return ntw == 2 ? 48 : 16 * ntw; }

// floats the staged weights take: what the launcher requests (x 4 bytes)
ASR_LWLAY_HD int wino_lw_lds_floats(int cin, int ntw, bool dense) {
    return 16 * cin * (dense ? 16 * ntw : wino_lw_row_stride(ntw));
}

// staging map: element (row, col) of the group's weights -> LDS float offset
ASR_LWLAY_HD int wino_lw_stage_off(int ntw, bool dense, int row, int col) {
    if (!dense) return row * wino_lw_row_stride(ntw) + col;
    if (ntw == 2) return (row * 16 + (col & 15)) * 2 + (col >> 4);
    const int ks = row >> 6, p = (row >> 2) & 15, g = row & 3;
    return (((ks * 8 + (p >> 1)) * 4 + g) * 16 + col) * 2 + (p & 1);
}

// lane (g, n): float offset of its operand of k-step 0, position 0, n-tile 0
ASR_LWLAY_HD int wino_lw_lane_off(int ntw, bool dense, int g, int n) {
    return dense ? (g * 16 + n) * 2 : g * wino_lw_row_stride(ntw) + n;
}

// dense form: reads (of two operands each) per k-step, and the float offset of read r past the lane's offset
ASR_LWLAY_HD int wino_lw_reads_per_kstep(int ntw) { return 8 * ntw; }
ASR_LWLAY_HD int wino_lw_read_off(int r) { return r * 128; }
// operand e (0 or 1) of read r: k-step, position and n-tile
ASR_LWLAY_HD int wino_lw_read_kstep(int ntw, int r) { return r / (8 * ntw); }
ASR_LWLAY_HD int wino_lw_read_pos(int ntw, int r, int e) { return ntw == 2 ? r % 16 : 2 * (r % 8) + e; }
ASR_LWLAY_HD int wino_lw_read_ntile(int ntw, int e) { return ntw == 2 ? e : 0; }

// row-major form: operand (k-step, position, n-tile), floats past the lane's offset
ASR_LWLAY_HD int wino_lw_rowmajor_off(int ntw, int ks, int p, int nt) {
    return (ks * 16 + p) * 4 * wino_lw_row_stride(ntw) + nt * 16;
}

}  // namespace asr
