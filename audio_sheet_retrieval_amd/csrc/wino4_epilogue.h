// Store classification of conv3x3_wino4s's consumer epilogue (conv_wino4_kernels.hip), as plain integer arithmetic
// shared by the kernel, its launcher and a host test (tests/test_wino4_epilogue_host.py builds
// tests/wino4_epilogue_harness.cpp for the CPU under AddressSanitizer + UBSan).
//
// A lane of a consumer stores the outputs of four 4x4 tiles (2x2 when the block pools) of an M-tile's 16.  The guarded
// epilogue tests every value against its tile's extent word - a branch around every store.  The fast epilogue runs on
// M-tiles whose tiles all have every output ROW (or lie past the end of the tile list): the row is then a scalar offset
// common to the wave, and the columns a tile does not have are folded into the lane's 32-bit byte offsets as a sentinel
// that the buffer store's range check drops.  That check compares the vector offset alone with num_records, so the
// sentinel is out of range whatever the row - provided the tensor is smaller than the sentinel (the launcher's rule).
// The other M-tiles of the un-pooled builds take the general form: the row test selects between the offset and the
// sentinel per store.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ASR_EPI_HD __host__ __device__ __forceinline__
#else
#define ASR_EPI_HD inline
#endif

namespace asr {

constexpr unsigned kWino4StoreSentinel = 0x80000000u;

// output rows / columns of a full tile: 4x4, or 2x2 pooled
ASR_EPI_HD int wino4_tile_span(bool pool) { return pool ? 2 : 4; }

// extent word of the tile at (tile row tty, tile column ttx) of an OH x OW output map: rows | columns << 8, 0 for a
// tile past the end of the list (or one that feeds no kept output): nothing to store
ASR_EPI_HD int wino4_extent(bool pool, int OH, int OW, int tty, int ttx, bool tvalid) {
    const int s = wino4_tile_span(pool);
    const int nr = OH - s * tty < s ? OH - s * tty : s, nc = OW - s * ttx < s ? OW - s * ttx : s;
    return (tvalid && nr > 0 && nc > 0) ? (nr | (nc << 8)) : 0;
}
ASR_EPI_HD int wino4_ext_rows(int ext) { return ext & 0xff; }
ASR_EPI_HD int wino4_ext_cols(int ext) { return ext >> 8; }

// the guarded epilogue's rule: the tile has output (row i, column j)
ASR_EPI_HD bool wino4_guard_stores(int ext, int i, int j) { return i < wino4_ext_rows(ext) && j < wino4_ext_cols(ext); }

// a tile that does not keep its M-tile off the fast epilogue: every row, or nothing at all.  An M-tile is rows-full when
// all 16 of its tiles are.
ASR_EPI_HD bool wino4_rows_full(int ext, bool pool) { return ext == 0 || wino4_ext_rows(ext) == wino4_tile_span(pool); }

// byte offset of (column c, channel chn) of a tile whose first output element is tile_off (in elements), or the sentinel
// when the tile does not have that column; the row is added as a scalar (wino4_row_bytes)
ASR_EPI_HD unsigned wino4_store_offset(unsigned tile_off, int ext, int chn, int c, int cout) {
    return c < wino4_ext_cols(ext) ? (tile_off + (unsigned)chn + (unsigned)(c * cout)) * 4u : kWino4StoreSentinel;
}
ASR_EPI_HD unsigned wino4_row_bytes(int i, int OW, int cout) { return (unsigned)(i * OW * cout) * 4u; }

// M-tiles that are not rows-full: the same stores with the row test folded into the lane offset too (one select per
// store).  Measured faster than the guarded epilogue in the un-pooled builds only, so only they use it.
ASR_EPI_HD constexpr bool wino4_general_form(bool pool) { return !pool; }
ASR_EPI_HD unsigned wino4_store_offset_row(unsigned col_off, int ext, int i) {
    return i < wino4_ext_rows(ext) ? col_off : kWino4StoreSentinel;
}

// num_records of the output tensor's buffer descriptor; the fast epilogue is admitted only when every byte offset of
// the tensor is below the sentinel
inline int64_t wino4_out_bytes(int64_t N, int OH, int OW, int cout) { return N * OH * OW * cout * 4; }
inline bool wino4_fast_epilogue_admitted(int64_t N, int OH, int OW, int cout) {
    return wino4_out_bytes(N, OH, OW, cout) < (int64_t)kWino4StoreSentinel;
}

}  // namespace asr
