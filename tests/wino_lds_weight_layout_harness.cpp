// Host harness for csrc/wino_lds_weight_layout.h, the dense weight layout of conv3x3_wino (built with
// -fsanitize=address,undefined by tests/test_wino_lds_weight_layout_host.py).  For (C_in, C_out, NTW) in
// (12,12,1), (12,24,2), (12,24,1), (24,24,2), (48,48,1) and every n-tile group:
//   1. the staging loop, run as the kernel runs it (one float4 of wpk per step, four scalar writes), writes every float
//      of the LDS request exactly once (the buffer has exactly the requested size: a stray offset is an ASan report),
//      and the request is 16 * C_in * 16 NTW floats: no pad column;
//   2. every (k-step, position, g, n, nt) is read by lane (g, n) in exactly one (read, element), at a distinct offset
//      inside the request, and that float holds wpk[(k-step * 16 + position) * 4 + g][group column nt * 16 + n];
//   3. every read's offset past the lane's base fits a 16-bit immediate in bytes, read and base are 8-byte aligned,
//      and a wave's 64 lanes cover 512 contiguous bytes;
//   4. the reads walk the operands in the order of the row-major form: k-step, position, n-tile.
// The row-major form (the producer builds) is checked against the same packed weights.
// Prints the number of operands compared.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audio_sheet_retrieval_amd/csrc/wino_lds_weight_layout.h"

using namespace asr;

struct Case { int cin, cout, ntw; };
static const Case kCases[] = {{12, 12, 1}, {12, 24, 2}, {12, 24, 1}, {24, 24, 2}, {48, 48, 1}};

static void fail(const char *what, const Case &c, int a, int b, int d) {
    fprintf(stderr, "FAIL %s: cin %d cout %d ntw %d at (%d, %d, %d)\n", what, c.cin, c.cout, c.ntw, a, b, d);
    exit(1);
}

int main() {
    long compared = 0;
    for (const Case &c : kCases) {
        const int cin = c.cin, ntw = c.ntw, coutp = (c.cout + 15) / 16 * 16;
        const int wrow = 16 * ntw, ks = cin / 4, rows = 16 * ks * 4;
        const int ngroups = (coutp / 16 + ntw - 1) / ntw;
        for (int dense = 0; dense < 2; ++dense) {
            if (dense && !wino_lw_dense(ntw, 0)) fail("the consumer builds are dense", c, 0, 0, 0);
            if (wino_lw_dense(ntw, 4)) fail("the producer builds are row-major", c, 0, 0, 0);
            const int lds_floats = wino_lw_lds_floats(cin, ntw, dense);
            if (dense && lds_floats != rows * wrow) fail("dense size", c, lds_floats, rows * wrow, 0);
            if (!dense && lds_floats != rows * (ntw == 2 ? 48 : wrow)) fail("row-major size", c, lds_floats, 0, 0);
            for (int ng = 0; ng < ngroups; ++ng) {
                // wpk element id = row * coutp + col + 1; 0: zero fill (columns past coutp) / never written (-1)
                std::vector<long> lds((size_t)lds_floats, -1);
                for (int i = 0; i < rows * (wrow / 4); ++i) {               // the kernel's staging loop
                    const int row = i / (wrow / 4), q = i - row * (wrow / 4);
                    const int col = ng * wrow + q * 4;
                    for (int e = 0; e < 4; ++e) {
                        const int off = wino_lw_stage_off(ntw, dense, row, q * 4 + e);
                        if (off < 0) fail("negative offset", c, row, q, e);
                        long &slot = lds[(size_t)off];                      // out of range: AddressSanitizer
                        if (slot != -1) fail("float written twice", c, row, q, e);
                        slot = col < coutp ? (long)row * coutp + col + e + 1 : 0;
                    }
                }
                if (dense)
                    for (int i = 0; i < lds_floats; ++i)
                        if (lds[(size_t)i] == -1) fail("float never written", c, i, 0, 0);
                std::vector<int> seen((size_t)lds_floats, 0);
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, n = lane & 15;
                    const int base = wino_lw_lane_off(ntw, dense, g, n);
                    int next = 0;                                            // operands in the order k-step, position, n-tile
                    auto check = [&](int off, int kstep, int p, int nt) {
                        if (off < 0 || off >= lds_floats) fail("read offset out of range", c, lane, kstep, p);
                        if (seen[(size_t)off]++) fail("two operands at one offset", c, lane, kstep, p);
                        const int col = ng * wrow + nt * 16 + n;
                        const long want = col < coutp ? (long)((kstep * 16 + p) * 4 + g) * coutp + col + 1 : 0;
                        if (lds[(size_t)off] != want) fail("read names another element", c, lane, kstep, p);
                        if ((kstep * 16 + p) * ntw + nt != next++) fail("operands out of order", c, lane, kstep, p);
                        ++compared;
                    };
                    if (dense) {
                        if (base % 2 != 0 || base != lane * 2) fail("lanes not 8 contiguous bytes each", c, lane, base, 0);
                        for (int r = 0; r < ks * wino_lw_reads_per_kstep(ntw); ++r) {
                            const int ro = wino_lw_read_off(r);
                            if (ro % 2 != 0 || ro * 4 + 7 > 0xffff) fail("read offset: alignment / immediate", c, lane, r, ro);
                            for (int e = 0; e < 2; ++e)
                                check(base + ro + e, wino_lw_read_kstep(ntw, r), wino_lw_read_pos(ntw, r, e),
                                      wino_lw_read_ntile(ntw, e));
                        }
                    } else {
                        for (int kstep = 0; kstep < ks; ++kstep)
                            for (int p = 0; p < 16; ++p)
                                for (int nt = 0; nt < ntw; ++nt) check(base + wino_lw_rowmajor_off(ntw, kstep, p, nt), kstep, p, nt);
                    }
                    if (next != ks * 16 * ntw) fail("operands missing", c, lane, next, 0);
                }
                if (dense)
                    for (int i = 0; i < lds_floats; ++i)
                        if (seen[(size_t)i] != 1) fail("float not read exactly once", c, i, seen[(size_t)i], 0);
            }
        }
    }
    printf("%ld\n", compared);
    return 0;
}
