// Host build of the store classification of conv3x3_wino4s's epilogue (csrc/wino4_epilogue.h): for every M-tile of a
// launch, lanes past the end of the tile list included, the branch-free rule (per-tile column offsets or the sentinel, a
// row offset common to the M-tile, the buffer's range check on the lane offset alone) must store exactly what the guarded
// rule stores, every element once, every address inside the tensor.  M-tiles that are not rows-full go through the
// general form (the row test selects the sentinel too) where the build has it, else through the guarded rule; at the end
// every output element of the channels walked has been written exactly once.
// Built with AddressSanitizer + UBSan by tests/test_wino4_epilogue_host.py.  Prints the share of rows-full M-tiles per
// case and, last, the number of stores checked; exits 1 on the first violation.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audio_sheet_retrieval_amd/csrc/wino4_epilogue.h"

static const int kCout = 48;
static const int kChans[3] = {0, 17, 47};

static int fail(const char *what, int H, int W, int pool, int N, int mt, int m, int i, int c) {
    fprintf(stderr, "%s: map %dx%d pool=%d N=%d M-tile %d lane tile %d row %d column %d\n", what, H, W, pool, N, mt, m, i, c);
    return 1;
}

// one launch; returns nonzero on a violation
static int run_case(int H, int W, bool pool, int N, long *stores, long *full_out, long *total_out) {
    const int OH = pool ? H / 2 : H, OW = pool ? W / 2 : W;
    const int s = asr::wino4_tile_span(pool);
    // the tile lists of conv_candidates_wino4: pooled blocks list only the tiles that feed a kept output
    const int ty = ((pool ? 2 * OH : H) + 3) / 4, tx = ((pool ? 2 * OW : W) + 3) / 4;
    const int per_img = ty * tx, tiles = N * per_img, total = (tiles + 15) / 16;
    *full_out = 0; *total_out = total;
    if (total == 0) return 0;                                  // (the launcher returns before it launches)
    if (!asr::wino4_fast_epilogue_admitted(N, OH, OW, kCout)) return fail("not admitted", H, W, pool, N, 0, 0, 0, 0);
    const int64_t num_records = asr::wino4_out_bytes(N, OH, OW, kCout);
    std::vector<unsigned char> seen((size_t)(num_records / 4), 0);
    long written = 0;
    for (int mt = 0; mt < total; ++mt) {
        int ext[16], img[16], tty[16], ttx[16];
        unsigned off[16];
        bool full = true;
        for (int m = 0; m < 16; ++m) {                         // the kernel's tile_of: lanes past the end are clamped
            const int tnum = mt * 16 + m;
            const bool tvalid = tnum < tiles;
            const int tcl = std::min(tnum, tiles - 1);
            img[m] = tcl / per_img;
            const int trest = tcl - img[m] * per_img;
            tty[m] = trest / tx;
            ttx[m] = trest - tty[m] * tx;
            off[m] = (((unsigned)img[m] * OH + s * tty[m]) * OW + s * ttx[m]) * kCout;
            ext[m] = asr::wino4_extent(pool, OH, OW, tty[m], ttx[m], tvalid);
            full = full && asr::wino4_rows_full(ext[m], pool);
        }
        *full_out += full ? 1 : 0;
        for (int m = 0; m < 16; ++m)
            for (int chn : kChans)
                for (int i = 0; i < s; ++i)
                    for (int c = 0; c < s; ++c) {
                        const bool guard = asr::wino4_guard_stores(ext[m], i, c);
                        const int64_t want = ((((int64_t)img[m] * OH + s * tty[m] + i) * OW + s * ttx[m] + c) * kCout + chn) * 4;
                        if (full || asr::wino4_general_form(pool)) {
                            unsigned vo = asr::wino4_store_offset(off[m], ext[m], chn, c, kCout);
                            if (!full) vo = asr::wino4_store_offset_row(vo, ext[m], i);          // the general form
                            const bool dropped = (int64_t)vo >= num_records;          // the range check: lane offset alone
                            if (vo != asr::kWino4StoreSentinel && dropped) return fail("offset past the tensor", H, W, pool, N, mt, m, i, c);
                            if (dropped != !guard) return fail("fast and guarded rules differ", H, W, pool, N, mt, m, i, c);
                            if (dropped) continue;
                            const int64_t addr = (int64_t)vo + asr::wino4_row_bytes(i, OW, kCout);
                            if (addr != want || addr + 4 > num_records) return fail("wrong address", H, W, pool, N, mt, m, i, c);
                        } else if (!guard) {
                            continue;
                        }
                        if (want < 0 || want + 4 > num_records) return fail("guarded store past the tensor", H, W, pool, N, mt, m, i, c);
                        if (seen[(size_t)(want / 4)]++) return fail("element stored twice", H, W, pool, N, mt, m, i, c);
                        ++written;
                    }
    }
    if (written != (long)N * OH * OW * 3) {
        fprintf(stderr, "map %dx%d pool=%d N=%d: %ld stores for %ld elements\n", H, W, pool, N, written, (long)N * OH * OW * 3);
        return 1;
    }
    *stores += written;
    return 0;
}

int main() {
    static const int geom[12][2] = {{40, 50}, {20, 25}, {23, 10}, {11, 5}, {26, 18}, {13, 9}, {24, 16}, {18, 25},
                                    {4, 4}, {3, 2}, {1, 1}, {2, 3}};
    long stores = 0;
    for (const auto &gm : geom)
        for (int pool = 0; pool < 2; ++pool)
            for (int N : {1, 5, 1000}) {
                long full = 0, total = 0;
                if (run_case(gm[0], gm[1], pool != 0, N, &stores, &full, &total)) return 1;
                printf("%dx%d pool=%d N=%d: rows-full %ld of %ld M-tiles (%.1f %%)\n", gm[0], gm[1], pool, N, full, total,
                       total ? 100.0 * full / total : 0.0);
                // the headline's maps: every M-tile takes the fast epilogue
                if ((gm[0] == 40 || gm[0] == 20) && full != total) {
                    fprintf(stderr, "%dx%d pool=%d N=%d: only %ld of %ld M-tiles are rows-full\n", gm[0], gm[1], pool, N, full, total);
                    return 1;
                }
            }
    // the admission rule at its edge: 2^31 bytes is refused, one element less is admitted
    if (asr::wino4_fast_epilogue_admitted(1 << 20, 16, 16, 2) || !asr::wino4_fast_epilogue_admitted((1 << 20) - 1, 16, 16, 2) ||
        !asr::wino4_fast_epilogue_admitted(1000, 40, 50, 48) || asr::wino4_fast_epilogue_admitted(1000, 160, 200, 48)) {
        fprintf(stderr, "admission rule\n");
        return 1;
    }
    printf("%ld\n", stores);
    return 0;
}
