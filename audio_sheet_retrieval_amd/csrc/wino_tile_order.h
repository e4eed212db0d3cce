// Tile-list order of conv3x3_winog (conv_wino_kernels.hip), as plain integer arithmetic shared by the kernel and a host
// test (tests/test_wino_tile_order_host.py builds it for the CPU under AddressSanitizer + UBSan).
//
// The batch's Winograd tiles are listed image by image, inside an image strip by strip of S = 1, 2, 4 or 8 tile rows
// (a last strip may be shorter) and column-major inside a strip.  An M-tile is 16 consecutive tiles of that list; lane
// m of a wave owns tile 16 * mtile + m.  Turning that number into (image, tile row, tile column) in closed form takes
// three divisions by launch constants per lane and M-tile - quarter-rate multiplies and reciprocals on the vector unit
// that the fp32 MFMAs of the same SIMD do not hide.  Here the divisions are done ONCE per M-tile for its first tile, on
// wave-uniform values (multiply-high by a precomputed reciprocal: the scalar unit, idle in that kernel), and every lane
// walks its 0..15 tiles forward from there with compares: over the end of a strip, of an image, of several of them
// when the geometry is tiny.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ASR_TILE_HD __host__ __device__ __forceinline__
#else
#define ASR_TILE_HD inline
#endif

namespace asr {

struct WinoTileOrder {
    int per_img;                 // tiles per image = ty_img * tx_img
    int strip_shift;             // log2(S)
    int nfull, nstrips;          // strips of S rows; all strips (one more when ty_img is no multiple of S)
    int strip_tiles;             // S * tx_img
    int last_rows, last_tiles;   // height of the short last strip (0: none) and its tiles
    int max_wraps;               // strip ends that 16 consecutive tiles can span at most (1 or 2 unless the map is tiny)
    unsigned last_mul;           // q / last_rows == (q * last_mul) >> 16 for q < last_tiles (<= kWinoLastTilesMax)
    unsigned img_mul, img_sh, img_one;          // n / per_img     for n < 2^31 (wino_udiv)
    unsigned strip_mul, strip_sh, strip_one;    // n / strip_tiles
    int64_t in_img;              // input elements per image
    unsigned in_img_bytes;       // the same in bytes: what a lane adds to its 32-bit offsets per image it steps over
    unsigned out_img;            // output elements per image (mod 2^32, like the kernel's output offsets)
};

// q * (65536 / d + 1) >> 16 == q / d needs q * d < 65536 (d <= 7) and the product below 2^32
constexpr int kWinoLastTilesMax = 9362;

// n / d for every n < 2^31 as (n * mul) >> (32 + sh) (Granlund & Montgomery 1994, N = 31: mul = ceil(2^(31 + l) / d)
// with l = ceil(log2 d) fits 32 bits for d >= 2); d == 1 is flagged instead
inline void wino_udiv_make(unsigned d, unsigned *mul, unsigned *sh, unsigned *one) {
    *one = d <= 1 ? 1u : 0u;
    *mul = 0; *sh = 0;
    if (d <= 1) return;
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    *mul = (unsigned)(((1ull << (31 + l)) + d - 1) / d);
    *sh = l - 1;
}

ASR_TILE_HD unsigned wino_udiv(unsigned n, unsigned mul, unsigned sh, unsigned one) {
    return one ? n : (unsigned)(((uint64_t)n * mul) >> 32) >> sh;
}

// false: this geometry cannot be listed with strips of S rows (a short last strip of more than kWinoLastTilesMax tiles),
// or the images that 16 consecutive tiles can touch do not fit the lanes' 32-bit byte offsets from the first one's base
inline bool wino_tile_order_make(WinoTileOrder *o, int ty_img, int tx_img, int S, int64_t in_img, unsigned out_img) {
    o->per_img = ty_img * tx_img;
    o->strip_shift = S == 8 ? 3 : S == 4 ? 2 : S == 2 ? 1 : 0;
    S = 1 << o->strip_shift;
    o->nfull = ty_img >> o->strip_shift;
    o->last_rows = ty_img - (o->nfull << o->strip_shift);
    o->nstrips = o->nfull + (o->last_rows ? 1 : 0);
    o->strip_tiles = S * tx_img;
    o->last_tiles = o->last_rows * tx_img;
    o->last_mul = o->last_rows ? 65536u / (unsigned)o->last_rows + 1u : 0u;
    wino_udiv_make((unsigned)o->per_img, &o->img_mul, &o->img_sh, &o->img_one);
    wino_udiv_make((unsigned)o->strip_tiles, &o->strip_mul, &o->strip_sh, &o->strip_one);
    o->in_img = in_img;
    o->in_img_bytes = (unsigned)(in_img * 4);
    o->out_img = out_img;
    // most strip ends between a tile and the one 15 places on: the walk starts on the last tile of a strip, and the
    // short strip - the one that adds least - comes as early as it can
    o->max_wraps = 0;
    for (int start : {0, o->nstrips - 1, o->nstrips - 2}) {
        int s = start < 0 ? 0 : start, left = 15, wraps = 0;
        while (left > 0 && o->per_img > 0) {
            s = s + 1 == o->nstrips ? 0 : s + 1;
            left -= s < o->nfull ? o->strip_tiles : o->last_tiles;
            ++wraps;
        }
        if (wraps > o->max_wraps) o->max_wraps = wraps;
    }
    const int64_t span = o->per_img > 0 ? (15 + o->per_img - 1) / o->per_img + 1 : 1;      // images of one M-tile
    return o->last_tiles <= kWinoLastTilesMax && span * in_img * 4 <= 0xffffffffll;
}

// first tile of an M-tile (tnum0 = 16 * mtile < tiles of the launch; wave-uniform): its image, strip and place in the strip
ASR_TILE_HD void wino_tile_base(const WinoTileOrder &o, int tnum0, int &img, int &sidx, int &q) {
    img = (int)wino_udiv((unsigned)tnum0, o.img_mul, o.img_sh, o.img_one);
    const int trest = tnum0 - img * o.per_img;
    sidx = (int)wino_udiv((unsigned)trest, o.strip_mul, o.strip_sh, o.strip_one);
    q = trest - sidx * o.strip_tiles;
}

// the tile q places into strip sidx, where q may run past the strip's end (by less than 16): steps over strip and image
// ends (in_off, in bytes, and out_off, in elements, advance by an image each time) and yields the tile's row and column
ASR_TILE_HD void wino_tile_lane(const WinoTileOrder &o, int sidx, int q, unsigned &in_off, unsigned &out_off, int &tty,
                                int &ttx) {
    // (a wave-uniform trip count and selects instead of a per-lane loop: no divergent control flow inside the kernel's
    // M-tile loop, whose register allocation is tight)
    for (int k = 0; k < o.max_wraps; ++k) {
        const int st = sidx < o.nfull ? o.strip_tiles : o.last_tiles;
        const bool over = q >= st;
        q -= over ? st : 0;
        sidx += over ? 1 : 0;
        const bool next_img = sidx == o.nstrips;
        sidx = next_img ? 0 : sidx;
        in_off += next_img ? o.in_img_bytes : 0u;
        out_off += next_img ? o.out_img : 0u;
    }
    int r;
    if (sidx < o.nfull) {
        ttx = q >> o.strip_shift;
        r = q - (ttx << o.strip_shift);
    } else {
        ttx = (int)(((unsigned)q * o.last_mul) >> 16);
        r = q - ttx * o.last_rows;
    }
    tty = (sidx << o.strip_shift) + r;
}

}  // namespace asr
