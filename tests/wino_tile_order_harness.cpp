// Host build of conv3x3_winog's tile decode (csrc/wino_tile_order.h) against the closed form it replaced: for every
// tile number of a launch, lanes past the end included, the image, tile row and tile column - and the image offsets the
// lane walk accumulates - must be the ones the three divisions gave.  Built with AddressSanitizer + UBSan by
// tests/test_wino_tile_order_host.py; prints the number of tiles compared, exits 1 on the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../audio_sheet_retrieval_amd/csrc/wino_tile_order.h"

// the closed form of the kernel's setup() before the decode moved to the scalar unit (S = strips, shift = log2 S)
static void reference(int tnum, int tiles, int ty_img, int tx_img, int S, int shift, int *img_o, int *tty_o, int *ttx_o) {
    const int per_img = ty_img * tx_img;
    const int tcl = std::min(tnum, tiles - 1);
    const int img = tcl / per_img;
    const int trest = tcl - img * per_img;
    int tty, ttx;
    const int strip_tiles = S * tx_img;
    const int sidx = trest / strip_tiles, q = trest - sidx * strip_tiles;
    const int rows_here = std::min(S, ty_img - sidx * S);
    if (rows_here == S) {
        ttx = q >> shift;
        tty = sidx * S + (q - (ttx << shift));
    } else {
        ttx = q / rows_here;
        tty = sidx * S + (q - ttx * rows_here);
    }
    *img_o = img; *tty_o = tty; *ttx_o = ttx;
}

int main() {
    static const int geom[6][2] = {{27, 19}, {26, 18}, {3, 1}, {1, 1}, {7, 5}, {80, 100}};
    long compared = 0;
    for (const auto &gm : geom)
        for (int S : {1, 2, 4, 8})
            for (int N : {1, 2, 5}) {
                const int ty = gm[0], tx = gm[1];
                const int64_t in_img = (int64_t)(2 * ty) * (2 * tx) * 24;
                const unsigned out_img = 3000000011u;             // wraps modulo 2^32 after two images, as the kernel's offsets may
                asr::WinoTileOrder o;
                if (!asr::wino_tile_order_make(&o, ty, tx, S, in_img, out_img)) {
                    fprintf(stderr, "geometry %dx%d S=%d refused\n", ty, tx, S);
                    return 1;
                }
                const int tiles = N * ty * tx, total = (tiles + 15) / 16;
                for (int mt = 0; mt < total; ++mt) {
                    const int tnum0 = mt * 16, dmax = tiles - 1 - tnum0;
                    int img0, sidx0, q0;
                    asr::wino_tile_base(o, tnum0, img0, sidx0, q0);
                    for (int m = 0; m < 16; ++m) {
                        unsigned ioff = 0;                                // bytes past image img0
                        unsigned ooff = (unsigned)img0 * o.out_img;
                        int tty, ttx;
                        asr::wino_tile_lane(o, sidx0, q0 + std::min(m, dmax), ioff, ooff, tty, ttx);
                        int rimg, rty, rtx;
                        reference(tnum0 + m, tiles, ty, tx, S, o.strip_shift, &rimg, &rty, &rtx);
                        if (tty != rty || ttx != rtx || (int64_t)ioff != (int64_t)(rimg - img0) * in_img * 4 || ooff != (unsigned)rimg * out_img ||
                            rty >= ty || rtx >= tx || rimg >= N) {
                            fprintf(stderr, "mismatch %dx%d S=%d N=%d tile %d: (%lld, %d, %d) != (%d, %d, %d)\n", ty, tx, S, N,
                                    tnum0 + m, (long long)(img0 + ioff / (in_img * 4)), tty, ttx, rimg, rty, rtx);
                            return 1;
                        }
                        ++compared;
                    }
                }
            }
    // the reciprocal division on its own: small, odd, power-of-two and large divisors at the ends of the 31-bit range
    static const unsigned ds[] = {1, 2, 3, 5, 6, 7, 9, 16, 17, 35, 100, 130, 468, 513, 2000, 8000, 65535, 65536, 65537,
                                  1000003, 0x3fffffffu, 0x40000000u, 0x40000001u, 0x7fffffffu};
    for (unsigned d : ds) {
        unsigned mul, sh, one;
        asr::wino_udiv_make(d, &mul, &sh, &one);
        for (unsigned k = 0; k < 70000u; ++k) {
            const unsigned ns[] = {k, 0x7fffffffu - k, (unsigned)(((unsigned long long)k * d) & 0x7fffffffu),
                                   (unsigned)(((unsigned long long)k * d - 1) & 0x7fffffffu)};
            for (unsigned n : ns)
                if (asr::wino_udiv(n, mul, sh, one) != n / d) {
                    fprintf(stderr, "wino_udiv(%u / %u) = %u\n", n, d, asr::wino_udiv(n, mul, sh, one));
                    return 1;
                }
        }
    }
    // the short last strip's 16-bit reciprocal over its whole admitted range
    for (int rows = 1; rows <= 7; ++rows) {
        const unsigned mul = 65536u / (unsigned)rows + 1u;
        for (int q = 0; q < asr::kWinoLastTilesMax; ++q)
            if ((int)(((unsigned)q * mul) >> 16) != q / rows) {
                fprintf(stderr, "last strip: %d / %d\n", q, rows);
                return 1;
            }
    }
    printf("%ld\n", compared);
    return 0;
}
