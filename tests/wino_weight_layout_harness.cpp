// Host harness for csrc/wino_weight_layout.h (built with -fsanitize=address,undefined by
// tests/test_wino_weight_layout_host.py).  For every (C_in, NT, padded C_out) that conv3x3_winog is instantiated with:
//   1. the staging map sends the (row, column) elements of every n-tile group into the LDS size the launcher
//      requests, no two to the same float (the buffer has exactly that size: a stray offset is an ASan report), and
//      the dense form leaves no float unwritten;
//   2. for every lane, channel block (and the remainder k-step of C_in = 12) and operand q - the window of WD operands
//      that runs into the next block included - the lane's read offset holds the weight element that the row-major
//      form's w_lane[wq_off(q)] names ([row][WS], WS = 48 at NT = 2, else 16 NT: the kernel before this header);
//   3. the dense form's operands q, q + 1 of one (k-step, position) are one aligned 8-byte read, and every offset of
//      a channel block and of the window behind it is below 64 KiB (the immediate of ds_read_b64).
// Prints the number of operand reads compared.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audio_sheet_retrieval_amd/csrc/wino_weight_layout.h"

using namespace asr;

struct Case { int cin, cout, nt; };
// g_winog of conv_wino_kernels.hip, one line per distinct (C_in, C_out, NT)
static const Case kCases[] = {{12, 12, 1}, {12, 24, 2}, {24, 24, 2}, {24, 48, 3}, {48, 48, 3}, {48, 96, 3}, {96, 96, 1},
                              {24, 12, 1}, {48, 24, 2}, {96, 48, 1}};

static long fail(const char *what, const Case &c, int a, int b, int d) {
    fprintf(stderr, "FAIL %s: cin %d cout %d nt %d at (%d, %d, %d)\n", what, c.cin, c.cout, c.nt, a, b, d);
    exit(1);
}

int main() {
    long compared = 0;
    for (const Case &c : kCases) {
        const int cin = c.cin, nt = c.nt, coutp = (c.cout + 15) / 16 * 16;
        const int wrow = 16 * nt, rows = 16 * cin, ks = cin / 4, nb = cin / 8;
        const bool rem = cin % 8 != 0, dense = wino_w_dense(cin, nt);
        const int ngroups = (coutp / 16 + nt - 1) / nt;
        const int lds_floats = wino_w_lds_floats(cin, nt);
        const int ws_old = nt == 2 ? 48 : wrow;
        if (lds_floats * 4 > 160 * 1024) fail("lds size", c, lds_floats, 0, 0);
        if (!dense && lds_floats != rows * ws_old) fail("row-major size", c, lds_floats, rows * ws_old, 0);
        if (dense && lds_floats != rows * wrow) fail("dense size", c, lds_floats, rows * wrow, 0);
        for (int ng = 0; ng < ngroups; ++ng) {
            // element id = row * wrow + col + 1 (0: never written), as the staging loop writes them
            std::vector<int> lds((size_t)lds_floats, 0);
            for (int row = 0; row < rows; ++row)
                for (int col = 0; col < wrow; ++col) {
                    const int off = wino_w_stage_off(cin, nt, row, col);
                    if (off < 0) fail("negative offset", c, row, col, off);
                    int &slot = lds[(size_t)off];          // out of range: AddressSanitizer
                    if (slot != 0) fail("two elements in one float", c, row, col, off);
                    slot = row * wrow + col + 1;
                }
            if (dense)
                for (int i = 0; i < lds_floats; ++i)
                    if (lds[(size_t)i] == 0) fail("float never written", c, i, 0, 0);
            const int wq = 32 * nt, wd = 4 * nt, kf = wino_w_kstep_floats(cin, nt);
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, n = lane & 15;
                const int base = wino_w_lane_off(cin, nt, g, n);
                const int base_old = g * ws_old + n;
                // blocks t = 0 .. nb - 1 hold 2 k-steps, the remainder "block" nb one
                for (int t = 0; t < nb + (rem ? 1 : 0); ++t) {
                    const int here = t < nb ? wq : 16 * nt;                      // operands of this block
                    const bool next = t + 1 < nb + (rem ? 1 : 0);                  // the window runs into block t + 1
                    const int avail = next ? here + wd : here;
                    for (int q = 0; q < avail && 2 * t * 16 + q / nt < ks * 16; ++q) {
                        const int off = base + 2 * t * kf + wino_w_q_off(cin, nt, q);
                        const int off_old = base_old + 2 * t * (16 * 4 * ws_old) + (q / nt) * 4 * ws_old + (q % nt) * 16;
                        const int want = (off_old / ws_old) * wrow + off_old % ws_old + 1;
                        if (off_old % ws_old >= wrow) fail("old offset in the padding", c, lane, t, q);
                        if (off < 0 || off >= lds_floats) fail("read offset out of range", c, lane, t, q);
                        if (lds[(size_t)off] != want) fail("read names another element", c, lane, t, q);
                        // and that element is (k-step, position, k = g, n-tile, n) of the packed weights
                        const int row = ((2 * t + q / (16 * nt)) * 16 + (q / nt) % 16) * 4 + g;
                        if (want != row * wrow + (q % nt) * 16 + n + 1) fail("old form names another element", c, lane, t, q);
                        if (dense) {
                            if (q % 2 == 0 && (off % 2 != 0 || base + 2 * t * kf + wino_w_q_off(cin, nt, q + 1) != off + 1))
                                fail("pair not one aligned 8-byte read", c, lane, t, q);
                            if ((base + wino_w_q_off(cin, nt, q)) * 4 + 7 > 0xffff) fail("offset beyond the immediate", c, lane, t, q);
                        }
                        ++compared;
                    }
                }
            }
        }
    }
    printf("%ld\n", compared);
    return 0;
}
