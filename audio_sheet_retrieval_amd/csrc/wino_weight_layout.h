// Where conv3x3_winog (conv_wino_kernels.hip) keeps a transformed weight in LDS, as plain integer arithmetic shared by
// the kernel's staging loop, its operand reads, the launcher's LDS request and a host test
// (tests/test_wino_weight_layout_host.py builds tests/wino_weight_layout_harness.cpp for the CPU under ASan + UBSan).
//
// The packed weights in global memory are wpk[row][coutp] with row = (k-step * 16 + position) * 4 + k (k = the
// channel inside the k-step of 4) and a workgroup stages the NT n-tiles of its group: columns col = nt * 16 + n.
// Lane (g, n) of a wave feeds its MFMAs element (k = g, n) of every (k-step, position, n-tile).
//
//   row-major form:  [row][stride]: the lane reads NT dwords 16 apart.  NT = 2 pads the stride to 48 (32 puts lane
//                    groups g and g + 1 on the same banks); read as pairs of dwords, whose two offsets are 8-bit
//                    dword counts, it needs a new base register every 1 KiB.
//   dense form:      [k-step][position][g][n][nt], NT = 2 with C_in a multiple of 8: the lane's two n-tiles of one
//                    (k-step, position) are 8 contiguous bytes, the 64 lanes cover 512 contiguous bytes (one
//                    conflict-free 64-bit read), a k-step is 8 KiB and every operand of a channel block (two k-steps),
//                    and of the next one, lies within the read's 16-bit byte offset of one base register.
//
// NT = 1 is the same in both forms; NT = 3 would need a 96-bit read.  C_in = 12 at NT = 2 (one channel block and a
// remainder k-step) stays row-major: its two-wave build has no register to spare and spilled 120 bytes around the
// dense staging loop.
#pragma once

#if defined(__HIPCC__)
#define ASR_WLAY_HD __host__ __device__ __forceinline__ constexpr
#else
#define ASR_WLAY_HD inline constexpr
#endif

namespace asr {

ASR_WLAY_HD bool wino_w_dense(int cin, int nt) { return nt == 2 && cin % 8 == 0; }

// row stride of the row-major form
ASR_WLAY_HD int wino_w_row_stride(int nt) { return nt == 2 ? 48 : 16 * nt; }

// floats of one k-step: 16 positions x 4 channels x (16 NT columns | a row)
ASR_WLAY_HD int wino_w_kstep_floats(int cin, int nt) {
    return 64 * (wino_w_dense(cin, nt) ? 16 * nt : wino_w_row_stride(nt));
}

// floats the staged weights take: what the launcher requests (x 4 bytes)
ASR_WLAY_HD int wino_w_lds_floats(int cin, int nt) { return (cin / 4) * wino_w_kstep_floats(cin, nt); }

// staging map: element (row, col) of the group's weights -> LDS float offset
ASR_WLAY_HD int wino_w_stage_off(int cin, int nt, int row, int col) {
    return wino_w_dense(cin, nt) ? (row * 16 + (col & 15)) * nt + (col >> 4) : row * wino_w_row_stride(nt) + col;
}

// lane (g, n): float offset of its operand of k-step 0, position 0, n-tile 0
ASR_WLAY_HD int wino_w_lane_off(int cin, int nt, int g, int n) {
    return wino_w_dense(cin, nt) ? (g * 16 + n) * nt : g * wino_w_row_stride(nt) + n;
}

// operand q of a channel block (k-step q / (16 NT), position (q / NT) % 16, n-tile q % NT): floats past the lane's
// offset of the block's first k-step.  q may run past the block (32 NT operands) into the next one.
ASR_WLAY_HD int wino_w_q_off(int cin, int nt, int q) {
    return wino_w_dense(cin, nt) ? (q / nt) * (64 * nt) + q % nt
                                 : (q / nt) * (4 * wino_w_row_stride(nt)) + (q % nt) * 16;
}

}  // namespace asr
