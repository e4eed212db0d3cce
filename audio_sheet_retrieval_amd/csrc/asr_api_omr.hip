// C-ABI layer of the staff-system detector: asr_seg_create / asr_seg_destroy / asr_seg_predict_dev
// (sheet_utils/omr.py SegmentationNetwork.load + predict_proba; include/asr_hip.h for the contract) and
// asr_systems_from_maps_dev (systems_from_maps: the maps to system corners), asr_notes_from_map_dev and
// asr_bars_from_map_dev (notes_from_map, bar_blobs_from_map).  Kernels: omr_kernels.hip, omr_post_kernels.hip,
// omr_detect_kernels.hip.
#include "asr_ctx.h"
#include "omr_kernels.h"

#include <cmath>

namespace {

// the 15 conv blocks of system_detector.build_model() (nf0 = 8), in graph order: input channels, output channels,
// level (0 = full tile), index of the layer's W in the reference's parameter list
struct SegConvSpec { int ci, co, level, p; };
constexpr SegConvSpec SEG_CONV[14] = {
    {1, 8, 0, 0},   {8, 8, 0, 5},   {8, 16, 1, 10}, {16, 16, 1, 15}, {16, 32, 2, 20}, {32, 32, 2, 25}, {32, 64, 3, 30},
    {64, 64, 3, 35}, {32, 32, 2, 49}, {32, 32, 2, 54}, {16, 16, 1, 68}, {16, 16, 1, 73}, {8, 8, 0, 87}, {8, 8, 0, 92}};
// decoder levels: TransposedConv2D W (ci, co, 2, 2) at p, BN at p + 1, BN after the skip add at p + 5
struct SegUpSpec { int ci, co, p; };
constexpr SegUpSpec SEG_UP[3] = {{64, 32, 40}, {32, 16, 59}, {16, 8, 78}};
constexpr int SEG_N_PARAMS = 99, SEG_HEAD_W = 97, SEG_HEAD_B = 98;

size_t seg_align(size_t x) { return (x + 255) & ~(size_t)255; }

int64_t seg_env(const char *name, int64_t dflt) {
    const char *v = getenv(name);
    return v && *v ? atoll(v) : dflt;
}

}  // namespace

struct asr_seg {
    asr_ctx *owner = nullptr;
    int th = 0, tw = 0;
    float *w = nullptr;                   // packed device weights (offsets below, in floats)
    size_t conv_w[14] = {}, conv_bn[14] = {}, up_w[3] = {}, up_bn1[3] = {}, up_bn2[3] = {}, head = 0;
    double *win = nullptr;                // sqrt(outer(hamming(th), hamming(tw))), computed as numpy does
    void *ws = nullptr;                   // per call: descriptors, page maxima, tile probabilities, one chunk's activations
    size_t ws_bytes = 0;
};

namespace {

// BN of Lasagne's batch_norm(): (x - mean) * (gamma * inv_std) + beta; parameters beta, gamma, mean, inv_std at p
void seg_pack_bn(std::vector<float> &dst, const float *const *a, int p, int c) {
    const float *beta = a[p], *gamma = a[p + 1], *mean = a[p + 2], *inv_std = a[p + 3];
    for (int k = 0; k < c; ++k) dst.push_back(mean[k]);
    for (int k = 0; k < c; ++k) dst.push_back(gamma[k] * inv_std[k]);
    for (int k = 0; k < c; ++k) dst.push_back(beta[k]);
}

// floats of one tile's activation buffers at tile size th x tw (plane = th * tw): A, B (8 planes each), the skips
// p1 (8), p2 (4), p3 (2)
int64_t seg_tile_floats(int64_t plane) { return 30 * plane; }

int seg_check(asr_ctx *ctx, const asr_seg *seg, const char *who) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!seg || seg->owner != ctx) return fail(ctx, ASR_ERR_INVALID, "%s: not a segmentation network of this context", who);
    return ASR_OK;
}

}  // namespace

extern "C" {

int asr_seg_create(asr_ctx *ctx, int tile_h, int tile_w, const float *const *arrays, const int64_t *sizes, int n_arrays,
                   asr_seg **out) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!out) return fail(ctx, ASR_ERR_INVALID, "seg_create: NULL output");
    *out = nullptr;
    if (tile_h < 8 || tile_w < 8 || tile_h % 8 || tile_w % 8 || (int64_t)tile_h * tile_w > (1 << 24))
        return fail(ctx, ASR_ERR_INVALID, "seg_create: tile %d x %d must be a multiple of 8 on each side (U-Net of "
                    "three 2x2 pools)", tile_h, tile_w);
    if (n_arrays != SEG_N_PARAMS || !arrays || !sizes)
        return fail(ctx, ASR_ERR_INVALID, "seg_create: expected the reference's %d arrays, got %d", SEG_N_PARAMS, n_arrays);
    // expected sizes, in the reference's order
    std::vector<int64_t> want(SEG_N_PARAMS, 0);
    for (const SegConvSpec &c : SEG_CONV) {
        want[c.p] = (int64_t)c.co * c.ci * 9;
        for (int k = 1; k <= 4; ++k) want[c.p + k] = c.co;
    }
    for (const SegUpSpec &u : SEG_UP) {
        want[u.p] = (int64_t)u.ci * u.co * 4;
        for (int k = 1; k <= 8; ++k) want[u.p + k] = u.co;
    }
    want[SEG_HEAD_W] = 8;
    want[SEG_HEAD_B] = 1;
    for (int i = 0; i < SEG_N_PARAMS; ++i) {
        if (sizes[i] != want[i])
            return fail(ctx, ASR_ERR_INVALID, "seg_create: array %d has %lld floats, the U-Net needs %lld", i,
                        (long long)sizes[i], (long long)want[i]);
        if (!arrays[i]) return fail(ctx, ASR_ERR_INVALID, "seg_create: array %d is NULL", i);
    }
    std::unique_ptr<asr_seg> seg(new asr_seg());
    seg->owner = ctx; seg->th = tile_h; seg->tw = tile_w;

    std::vector<float> pk;
    auto pad = [&]() { while (pk.size() % 64) pk.push_back(0.0f); };
    for (int l = 0; l < 14; ++l) {
        const SegConvSpec &c = SEG_CONV[l];
        const float *W = arrays[c.p];                     // (co, ci, 3, 3), flip_filters=True
        seg->conv_w[l] = pk.size();
        for (int ci = 0; ci < c.ci; ++ci)
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx)
                    for (int co = 0; co < c.co; ++co) pk.push_back(W[((co * c.ci + ci) * 3 + (2 - dy)) * 3 + (2 - dx)]);
        pad();
        seg->conv_bn[l] = pk.size();
        seg_pack_bn(pk, arrays, c.p + 1, c.co);
        pad();
    }
    for (int u = 0; u < 3; ++u) {
        const SegUpSpec &s = SEG_UP[u];
        const float *W = arrays[s.p];                     // (ci, co, 2, 2); out[2i+a, 2j+b] reads W[ci, co, 1-a, 1-b]
        seg->up_w[u] = pk.size();
        for (int ci = 0; ci < s.ci; ++ci)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int co = 0; co < s.co; ++co) pk.push_back(W[((ci * s.co + co) * 2 + (1 - a)) * 2 + (1 - b)]);
        pad();
        seg->up_bn1[u] = pk.size();
        seg_pack_bn(pk, arrays, s.p + 1, s.co);
        pad();
        seg->up_bn2[u] = pk.size();
        seg_pack_bn(pk, arrays, s.p + 5, s.co);
        pad();
    }
    seg->head = pk.size();
    for (int k = 0; k < 8; ++k) pk.push_back(arrays[SEG_HEAD_W][k]);
    pk.push_back(arrays[SEG_HEAD_B][0]);
    pad();

    // np.hamming(M): 0.54 - 0.46 cos(2 pi n / (M - 1)); weight sqrt(outer(h, w))
    std::vector<double> hh(tile_h), hw(tile_w), win((size_t)tile_h * tile_w);
    for (int i = 0; i < tile_h; ++i) hh[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (tile_h - 1));
    for (int j = 0; j < tile_w; ++j) hw[j] = 0.54 - 0.46 * std::cos(2.0 * M_PI * j / (tile_w - 1));
    for (int i = 0; i < tile_h; ++i)
        for (int j = 0; j < tile_w; ++j) win[(size_t)i * tile_w + j] = std::sqrt(hh[i] * hw[j]);

    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipError_t e = hipMalloc((void **)&seg->w, pk.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&seg->win, win.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(seg->w, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(seg->win, win.data(), win.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (seg->w) hipFree(seg->w);
        if (seg->win) hipFree(seg->win);
        return fail(ctx, ASR_ERR_HIP, "seg_create: %s", hipGetErrorString(e));
    }
    *out = seg.release();
    return ASR_OK;
}

int asr_seg_set_window(asr_ctx *ctx, asr_seg *seg, const double *win_host) {
    int rc = seg_check(ctx, seg, "seg_set_window");
    if (rc != ASR_OK) return rc;
    if (!win_host) return fail(ctx, ASR_ERR_INVALID, "seg_set_window: NULL window");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = sync_all(ctx);
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, hipMemcpy(seg->win, win_host, (size_t)seg->th * seg->tw * sizeof(double), hipMemcpyHostToDevice));
    return ASR_OK;
}

int asr_seg_destroy(asr_ctx *ctx, asr_seg *seg) {
    if (!seg) return ASR_OK;
    int rc = seg_check(ctx, seg, "seg_destroy");
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = sync_all(ctx);
    if (seg->w) hipFree(seg->w);
    if (seg->win) hipFree(seg->win);
    if (seg->ws) hipFree(seg->ws);
    seg->owner = nullptr;
    delete seg;
    return rc;
}

int asr_seg_predict_dev(asr_ctx *ctx, asr_seg *seg, const void *pages_dev, int in_mode, const int64_t *page_offsets,
                        const int32_t *heights, const int32_t *widths, int n_pages, double overlap, double *proba_dev) {
    int rc = seg_check(ctx, seg, "seg_predict");
    if (rc != ASR_OK) return rc;
    if (n_pages < 0 || in_mode < 0 || in_mode > 2)
        return fail(ctx, ASR_ERR_INVALID, "seg_predict: bad n_pages=%d in_mode=%d", n_pages, in_mode);
    if (n_pages == 0) return ASR_OK;
    if (!pages_dev || !page_offsets || !heights || !widths || !proba_dev)
        return fail(ctx, ASR_ERR_INVALID, "seg_predict: NULL argument");
    const int th = seg->th, tw = seg->tw;
    // SegmentationNetwork._predict_proba_sliding_window: np.arange(0, Hp - th + 1, int(th * (1 - overlap)))
    const int step_h = (int)(th * (1.0 - overlap)), step_w = (int)(tw * (1.0 - overlap));
    if (!(overlap >= 0.0) || step_h < 1 || step_w < 1)
        return fail(ctx, ASR_ERR_INVALID, "seg_predict: overlap %g leaves no tile step", overlap);

    std::vector<asr::SegPage> pdesc(n_pages);
    std::vector<asr::SegStitch> sdesc(n_pages);
    std::vector<asr::SegTile> tiles;
    int64_t out_off = 0, max_px = 0;
    for (int p = 0; p < n_pages; ++p) {
        const int h = heights[p], w = widths[p];
        if (h < 1 || w < 1 || (int64_t)h * w > (1 << 28) || page_offsets[p] < 0)
            return fail(ctx, ASR_ERR_INVALID, "seg_predict: page %d has bad geometry %d x %d at %lld", p, h, w,
                        (long long)page_offsets[p]);
        pdesc[p] = {page_offsets[p], h, w};
        asr::SegStitch &S = sdesc[p];
        S.out_offset = out_off; S.h = h; S.w = w;
        S.first_tile = (int32_t)tiles.size();
        S.direct = h == th && w == tw;
        if (S.direct) {
            S.n_rows = S.n_cols = 1; S.step_h = step_h; S.step_w = step_w;
            tiles.push_back({p, 0, 0, 0});
        } else {
            const int hp = (int)(th * std::ceil((double)h / th)), wp = (int)(tw * std::ceil((double)w / tw));
            S.pad_top = (hp - h) / 2; S.pad_left = (wp - w) / 2;
            S.step_h = step_h; S.step_w = step_w;
            S.n_rows = (hp - th) / step_h + 1; S.n_cols = (wp - tw) / step_w + 1;
            for (int r = 0; r < S.n_rows; ++r)
                for (int c = 0; c < S.n_cols; ++c)
                    tiles.push_back({p, r * step_h - S.pad_top, c * step_w - S.pad_left, 0});
        }
        out_off += (int64_t)h * w;
        max_px = std::max<int64_t>(max_px, (int64_t)h * w);
    }
    const int64_t n_tiles = (int64_t)tiles.size(), plane = (int64_t)th * tw;

    // ASR_OMR_BUDGET_MB: device workspace of one chunk of tiles (activations); whole tiles, at least one per chunk
    const size_t budget = (size_t)std::max<int64_t>(seg_env("ASR_OMR_BUDGET_MB", 4096), 1) << 20;
    const size_t per_tile = (size_t)seg_tile_floats(plane) * sizeof(float);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)(budget / per_tile)));
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += seg_align(bytes); return at; };
    const size_t o_pd = take(pdesc.size() * sizeof(asr::SegPage)), o_sd = take(sdesc.size() * sizeof(asr::SegStitch));
    const size_t o_td = take(tiles.size() * sizeof(asr::SegTile)), o_mx = take((size_t)n_pages * sizeof(float));
    const size_t o_tp = take((size_t)n_tiles * plane * sizeof(float)), o_act = take((size_t)chunk * per_tile);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (o > seg->ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (seg->ws) ASR_HIP(ctx, hipFree(seg->ws));
        seg->ws = nullptr; seg->ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&seg->ws, o));
        seg->ws_bytes = o;
    }
    char *ws = (char *)seg->ws;
    asr::SegPage *d_pd = (asr::SegPage *)(ws + o_pd);
    asr::SegStitch *d_sd = (asr::SegStitch *)(ws + o_sd);
    asr::SegTile *d_td = (asr::SegTile *)(ws + o_td);
    float *d_mx = (float *)(ws + o_mx), *tile_p = (float *)(ws + o_tp), *act = (float *)(ws + o_act);
    hipStream_t st = ctx->stream;
    ASR_HIP(ctx, hipMemcpyAsync(d_pd, pdesc.data(), pdesc.size() * sizeof(asr::SegPage), hipMemcpyHostToDevice, st));
    ASR_HIP(ctx, hipMemcpyAsync(d_sd, sdesc.data(), sdesc.size() * sizeof(asr::SegStitch), hipMemcpyHostToDevice, st));
    ASR_HIP(ctx, hipMemcpyAsync(d_td, tiles.data(), tiles.size() * sizeof(asr::SegTile), hipMemcpyHostToDevice, st));
    if (in_mode != 0) ASR_HIP(ctx, asr::launch_seg_page_max(st, pages_dev, in_mode, d_pd, n_pages, d_mx));

    // direct-form FLOP of one tile (3x3 blocks, transposed convs, head) for the profiler
    double tile_flop = 0.0;
    for (const SegConvSpec &c : SEG_CONV) tile_flop += 2.0 * 9 * c.ci * c.co * (double)(plane >> (2 * c.level));
    for (int u = 0; u < 3; ++u) tile_flop += 2.0 * 4 * SEG_UP[u].ci * SEG_UP[u].co * (double)(plane >> (2 * (3 - u)));
    tile_flop += 2.0 * 8 * (double)plane;

    const float *W = seg->w;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, n_tiles - t0);
        ProfScope ps(ctx, "seg_unet", 0, tile_flop * n, 4.0 * (double)plane * n * 31);
        float *A = act, *B = A + (size_t)n * 8 * plane, *P1 = B + (size_t)n * 8 * plane;
        float *P2 = P1 + (size_t)n * 8 * plane, *P3 = P2 + (size_t)n * 4 * plane;
        auto conv = [&](int l, const float *in, float *out, float *pooled, bool head, int level) {
            asr::SegConvArgs a;
            a.in = in; a.w = W + seg->conv_w[l]; a.bn = W + seg->conv_bn[l];
            a.head = head ? W + seg->head : nullptr;
            a.out = out; a.pooled = pooled;
            a.ci = SEG_CONV[l].ci; a.co = SEG_CONV[l].co; a.H = th >> level; a.W = tw >> level; a.n = n;
            if (l == 0) {
                a.pages = pages_dev; a.page_desc = d_pd; a.tiles = d_td + t0; a.page_max = d_mx; a.in_mode = in_mode;
            }
            return asr::launch_seg_conv3(st, a);
        };
        auto up = [&](int u, const float *in, const float *skip, float *out) {
            const int lv = 3 - u;                          // level of the input
            return asr::launch_seg_up(st, in, W + seg->up_w[u], W + seg->up_bn1[u], W + seg->up_bn2[u], skip, out,
                                      SEG_UP[u].ci, SEG_UP[u].co, th >> lv, tw >> lv, n);
        };
        // encoder
        ASR_HIP(ctx, conv(0, nullptr, A, nullptr, false, 0));
        ASR_HIP(ctx, conv(1, A, P1, B, false, 0));
        ASR_HIP(ctx, conv(2, B, A, nullptr, false, 1));
        ASR_HIP(ctx, conv(3, A, P2, B, false, 1));
        ASR_HIP(ctx, conv(4, B, A, nullptr, false, 2));
        ASR_HIP(ctx, conv(5, A, P3, B, false, 2));
        ASR_HIP(ctx, conv(6, B, A, nullptr, false, 3));
        ASR_HIP(ctx, conv(7, A, B, nullptr, false, 3));
        // decoder
        ASR_HIP(ctx, up(0, B, P3, A));
        ASR_HIP(ctx, conv(8, A, B, nullptr, false, 2));
        ASR_HIP(ctx, conv(9, B, A, nullptr, false, 2));
        ASR_HIP(ctx, up(1, A, P2, B));
        ASR_HIP(ctx, conv(10, B, A, nullptr, false, 1));
        ASR_HIP(ctx, conv(11, A, B, nullptr, false, 1));
        ASR_HIP(ctx, up(2, B, P1, A));
        ASR_HIP(ctx, conv(12, A, B, nullptr, false, 0));
        ASR_HIP(ctx, conv(13, B, tile_p + (size_t)t0 * plane, nullptr, true, 0));
    }
    {
        ProfScope ps(ctx, "seg_stitch", 0, 3.0 * (double)out_off, 12.0 * (double)out_off);
        ASR_HIP(ctx, asr::launch_seg_stitch(st, tile_p, seg->win, th, tw, d_sd, n_pages, (int)max_px, proba_dev));
    }
    return mark_main(ctx);
}

namespace {

// the leaves of numpy's pairwise sum over n >= 8 contiguous elements and the postfix program that adds them up in the
// order of the recursion (0: push the next leaf, 1: add the two topmost values)
void post_leaves(int off, int n, std::vector<asr::PostLeaf> &leaves, std::vector<uint8_t> &prog) {
    if (n <= 128) {
        leaves.push_back({off, n});
        prog.push_back(0);
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    post_leaves(off, n2, leaves, prog);
    post_leaves(off + n2, n - n2, leaves, prog);
    prog.push_back(1);
}

}  // namespace

int asr_systems_from_maps_dev(asr_ctx *ctx, const void *pages_dev, int in_mode, const int64_t *page_offsets,
                              const int32_t *heights, const int32_t *widths, int n_pages, const double *system_maps_dev,
                              const double *bar_maps_dev, const asr_seg *system_seg, const asr_seg *bar_seg,
                              int max_systems, int32_t *status, int32_t *counts, int32_t *systems,
                              int32_t *label_passes) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || in_mode < 0 || in_mode > 2 || max_systems < 0)
        return fail(ctx, ASR_ERR_INVALID, "systems_from_maps: bad n_pages=%d in_mode=%d max_systems=%d", n_pages, in_mode,
                    max_systems);
    if (label_passes) *label_passes = 0;
    if (n_pages == 0) return ASR_OK;
    if (!pages_dev || !page_offsets || !heights || !widths || !system_maps_dev || !status || !counts ||
        (max_systems && !systems))
        return fail(ctx, ASR_ERR_INVALID, "systems_from_maps: NULL argument");
    for (const asr_seg *g : {system_seg, bar_seg})
        if (g && g->owner != ctx)
            return fail(ctx, ASR_ERR_INVALID, "systems_from_maps: not a segmentation network of this context");
    for (int p = 0; p < n_pages; ++p) {
        const int h = heights[p], w = widths[p];
        if (h < 1 || w < 1 || (int64_t)h * w > (1 << 28) || page_offsets[p] < 0)
            return fail(ctx, ASR_ERR_INVALID, "systems_from_maps: page %d has bad geometry %d x %d at %lld", p, h, w,
                        (long long)page_offsets[p]);
        if ((int64_t)h * w / asr::POST_MIN_AREA > max_systems)
            return fail(ctx, ASR_ERR_INVALID, "systems_from_maps: page %d (%d x %d) can hold %lld systems, max_systems "
                        "is %d", p, h, w, (long long)((int64_t)h * w / asr::POST_MIN_AREA), max_systems);
    }
    const int cap = std::max(max_systems, 1);

    // pages that are decided here, their geometry tables; every other page is status 3 from the start
    std::vector<asr::SegPage> sdesc(n_pages);
    std::vector<asr::PostPage> all;
    std::vector<asr::PostLeaf> leaves;
    std::vector<uint8_t> prog;
    int64_t map_off = 0;
    for (int p = 0; p < n_pages; ++p) {
        const int h = heights[p], w = widths[p];
        sdesc[p] = {page_offsets[p], h, w};
        status[p] = 3;
        counts[p] = 0;
        const bool tile = (system_seg && h == system_seg->th && w == system_seg->tw) ||
                          (bar_seg && h == bar_seg->th && w == bar_seg->tw);      // the host works on float32 maps there
        if (!tile && h >= 3 && w >= 8) {
            asr::PostPage P{};
            P.page_off = page_offsets[p]; P.map_off = map_off; P.h = h; P.w = w; P.page = p;
            // one table per distinct width; a width of more leaves than a wave holds gets none and stays status 3
            bool found = false;
            for (const asr::PostPage &Q : all)
                if (Q.w == w) { P.leaf_off = Q.leaf_off; P.n_leaves = Q.n_leaves; P.prog_off = Q.prog_off; P.n_prog = Q.n_prog; found = true; break; }
            if (!found) {
                std::vector<asr::PostLeaf> lv;
                std::vector<uint8_t> pg;
                post_leaves(0, w, lv, pg);
                P.leaf_off = (int32_t)leaves.size(); P.prog_off = (int32_t)prog.size();
                P.n_leaves = (int32_t)lv.size(); P.n_prog = (int32_t)pg.size();
                if (P.n_leaves <= asr::POST_MAX_LEAVES) {
                    leaves.insert(leaves.end(), lv.begin(), lv.end());
                    prog.insert(prog.end(), pg.begin(), pg.end());
                }
            }
            if (P.n_leaves <= asr::POST_MAX_LEAVES) all.push_back(P);
        }
        map_off += (int64_t)h * w;
    }
    if (max_systems) memset(systems, 0, (size_t)n_pages * max_systems * 4 * sizeof(int32_t));
    if (all.empty()) return ASR_OK;

    // chunks of whole pages under ASR_OMR_BUDGET_MB (at least one page each) and the workspace of the largest
    const size_t budget = (size_t)std::max<int64_t>(seg_env("ASR_OMR_BUDGET_MB", 4096), 1) << 20;
    struct Lay { size_t pd, st, bl, e2, h2, proj, rmin, rmax, ys, rz, fg, tmp, lab, area, xs, chg, end; };
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += seg_align(bytes); return at; };
    const size_t o_sd = take(sdesc.size() * sizeof(asr::SegPage)), o_mx = take((size_t)n_pages * sizeof(float));
    const size_t o_lv = take(leaves.size() * sizeof(asr::PostLeaf)), o_pg = take(prog.size());
    const size_t fixed = o;
    auto layout = [&](int n, int64_t px, int64_t rows, int max_w) {
        Lay L;
        o = fixed;
        L.pd = take((size_t)n * sizeof(asr::PostPage));
        // cleared before every chunk: state .. changed flag (contiguous)
        L.st = take((size_t)n * sizeof(asr::PostState));
        L.bl = take((size_t)n * cap * sizeof(asr::PostBlob));
        L.h2 = take((size_t)n * 256 * sizeof(uint32_t));
        L.chg = take(sizeof(int32_t));
        L.area = take((size_t)px * sizeof(int32_t));
        L.e2 = take((size_t)n * 257 * sizeof(double));
        L.proj = take((size_t)rows * sizeof(double)); L.rmin = take((size_t)rows * sizeof(double));
        L.rmax = take((size_t)rows * sizeof(double)); L.ys = take((size_t)rows * sizeof(float));
        L.rz = take((size_t)rows);
        L.fg = take((size_t)px); L.tmp = take((size_t)px);
        L.lab = take((size_t)px * sizeof(int32_t));
        L.xs = take((size_t)n * cap * max_w * sizeof(float));
        L.end = o;
        return L;
    };
    struct Chunk { int first, n, max_h, max_w; int64_t px, rows, max_px; };
    std::vector<Chunk> chunks;
    size_t need = 0;
    for (int i = 0; i < (int)all.size();) {
        Chunk c{i, 0, 0, 0, 0, 0, 0};
        while (i < (int)all.size()) {
            const asr::PostPage &P = all[i];
            const int64_t px = c.px + (int64_t)P.h * P.w, rows = c.rows + P.h;
            const int mw = std::max(c.max_w, P.w);
            // (the pages of a chunk are the y dimension of every launch grid)
            if (c.n && (c.n >= asr::POST_MAX_CHUNK_PAGES || layout(c.n + 1, px, rows, mw).end > budget ||
                        px > (1ll << 30))) break;
            c.n += 1; c.px = px; c.rows = rows; c.max_w = mw; c.max_h = std::max(c.max_h, P.h);
            c.max_px = std::max<int64_t>(c.max_px, (int64_t)P.h * P.w);
            ++i;
        }
        need = std::max(need, layout(c.n, c.px, c.rows, c.max_w).end);
        chunks.push_back(c);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (need > ctx->post_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->post_ws) ASR_HIP(ctx, hipFree(ctx->post_ws));
        ctx->post_ws = nullptr; ctx->post_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->post_ws, need));
        ctx->post_ws_bytes = need;
    }
    char *ws = (char *)ctx->post_ws;
    hipStream_t st = ctx->stream;
    asr::SegPage *d_sd = (asr::SegPage *)(ws + o_sd);
    float *d_mx = (float *)(ws + o_mx);
    ASR_HIP(ctx, hipMemcpyAsync(d_sd, sdesc.data(), sdesc.size() * sizeof(asr::SegPage), hipMemcpyHostToDevice, st));
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_lv, leaves.data(), leaves.size() * sizeof(asr::PostLeaf), hipMemcpyHostToDevice, st));
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_pg, prog.data(), prog.size(), hipMemcpyHostToDevice, st));
    if (in_mode != 0) ASR_HIP(ctx, asr::launch_seg_page_max(st, pages_dev, in_mode, d_sd, n_pages, d_mx));

    std::vector<asr::PostState> h_state;
    std::vector<asr::PostBlob> h_blobs;
    int passes = 0;
    for (const Chunk &c : chunks) {
        const Lay L = layout(c.n, c.px, c.rows, c.max_w);
        std::vector<asr::PostPage> pd(all.begin() + c.first, all.begin() + c.first + c.n);
        int64_t px = 0;
        int32_t rows = 0;
        for (asr::PostPage &P : pd) {
            P.px_off = px; P.row_off = rows;
            px += (int64_t)P.h * P.w; rows += P.h;
        }
        asr::PostArgs a;
        a.pages = (const asr::PostPage *)(ws + L.pd);
        a.n_pages = c.n; a.max_h = c.max_h; a.max_w = c.max_w; a.cap = cap; a.max_px = c.max_px;
        a.page_buf = pages_dev; a.in_mode = in_mode; a.page_max = d_mx;
        a.sys_maps = system_maps_dev; a.bar_maps = bar_maps_dev;
        a.leaves = (const asr::PostLeaf *)(ws + o_lv); a.prog = (const uint8_t *)(ws + o_pg);
        a.state = (asr::PostState *)(ws + L.st); a.blobs = (asr::PostBlob *)(ws + L.bl);
        a.proj = (double *)(ws + L.proj); a.rmin = (double *)(ws + L.rmin); a.rmax = (double *)(ws + L.rmax);
        a.ysig = (float *)(ws + L.ys); a.rowzero = (uint8_t *)(ws + L.rz);
        a.edges2 = (double *)(ws + L.e2); a.hist2 = (uint32_t *)(ws + L.h2);
        a.fg = (uint8_t *)(ws + L.fg); a.tmp = (uint8_t *)(ws + L.tmp);
        a.label = (int32_t *)(ws + L.lab); a.area = (int32_t *)(ws + L.area);
        a.xsig = (float *)(ws + L.xs); a.changed = (int32_t *)(ws + L.chg);
        ASR_HIP(ctx, hipMemcpyAsync(ws + L.pd, pd.data(), pd.size() * sizeof(asr::PostPage), hipMemcpyHostToDevice, st));
        ASR_HIP(ctx, hipMemsetAsync(ws + L.st, 0, L.e2 - L.st, st));
        const double dpx = (double)c.px;
        {
            ProfScope ps(ctx, "post_rows", 0, 4.0 * dpx, 17.0 * dpx);
            ASR_HIP(ctx, asr::launch_post_rows(st, a));
        }
        {
            ProfScope ps(ctx, "post_threshold", 0, 6.0 * dpx, 8.0 * dpx);
            ASR_HIP(ctx, asr::launch_post_threshold(st, a));
        }
        {
            ProfScope ps(ctx, "post_close", 0, 0.0, 8.0 * dpx + 15.0 * 2 * dpx + 6.0 * dpx);
            ASR_HIP(ctx, asr::launch_post_close(st, a));
        }
        // label equivalence: until a scan changes nothing (every changing pass lowers a label, so this ends)
        for (;;) {
            int32_t changed = 0;
            ASR_HIP(ctx, hipMemsetAsync(a.changed, 0, sizeof(int32_t), st));
            {
                ProfScope ps(ctx, "post_label_pass", 0, 0.0, 48.0 * dpx);
                ASR_HIP(ctx, asr::launch_post_label_pass(st, a));
            }
            ASR_HIP(ctx, hipMemcpyAsync(&changed, a.changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            ASR_HIP(ctx, hipStreamSynchronize(st));
            ++passes;
            if (!changed) break;
        }
        {
            ProfScope ps(ctx, "post_blobs", 0, 0.0, 24.0 * dpx);
            ASR_HIP(ctx, asr::launch_post_blobs(st, a));
        }
        h_state.resize(c.n);
        h_blobs.resize((size_t)c.n * cap);
        ASR_HIP(ctx, hipMemcpyAsync(h_state.data(), a.state, h_state.size() * sizeof(asr::PostState), hipMemcpyDeviceToHost, st));
        ASR_HIP(ctx, hipMemcpyAsync(h_blobs.data(), a.blobs, h_blobs.size() * sizeof(asr::PostBlob), hipMemcpyDeviceToHost, st));
        ASR_HIP(ctx, hipStreamSynchronize(st));
        for (int j = 0; j < c.n; ++j) {
            const int p = pd[j].page;
            const asr::PostState &S = h_state[j];
            if (S.status != 0) {
                status[p] = S.status == 1 ? 1 : 3;
                continue;
            }
            if (S.n_kept > (uint32_t)max_systems) continue;          // (cannot happen: the capacity was checked)
            int worst = 0;
            for (uint32_t k = 0; k < S.n_kept; ++k) {
                const int bs = h_blobs[(size_t)j * cap + k].status;
                worst = bs == 3 || worst == 3 ? 3 : std::max(worst, bs);
            }
            status[p] = worst;
            if (worst) continue;
            counts[p] = (int32_t)S.n_kept;
            for (uint32_t k = 0; k < S.n_kept; ++k)
                memcpy(systems + ((size_t)p * max_systems + k) * 4, h_blobs[(size_t)j * cap + k].out, 4 * sizeof(int32_t));
        }
    }
    if (label_passes) *label_passes = passes;
    return mark_main(ctx);
}

}  // extern "C"

namespace {

// asr_notes_from_map_dev / asr_bars_from_map_dev: the pages the device decides, cut into chunks of whole pages whose
// workspace fits ASR_OMR_BUDGET_MB (at least one page each).  bytes(n, px, rows): the workspace of such a chunk.
struct DetChunk { int first, n, max_h, max_w; int64_t px, rows, max_px; };

template <typename Bytes>
std::vector<DetChunk> det_chunks(const std::vector<asr::PostPage> &all, Bytes bytes, size_t *need) {
    const size_t budget = (size_t)std::max<int64_t>(seg_env("ASR_OMR_BUDGET_MB", 4096), 1) << 20;
    std::vector<DetChunk> chunks;
    *need = 0;
    for (int i = 0; i < (int)all.size();) {
        DetChunk c{i, 0, 0, 0, 0, 0, 0};
        while (i < (int)all.size()) {
            const asr::PostPage &P = all[i];
            const int64_t px = c.px + (int64_t)P.h * P.w, rows = c.rows + P.h;
            if (c.n && (c.n >= asr::POST_MAX_CHUNK_PAGES || bytes(c.n + 1, px, rows) > budget || px > (1ll << 30) ||
                        rows > INT32_MAX))
                break;
            c.n += 1; c.px = px; c.rows = rows;
            c.max_w = std::max(c.max_w, P.w); c.max_h = std::max(c.max_h, P.h);
            c.max_px = std::max<int64_t>(c.max_px, (int64_t)P.h * P.w);
            ++i;
        }
        *need = std::max(*need, bytes(c.n, c.px, c.rows));
        chunks.push_back(c);
    }
    return chunks;
}

// the context's post-processing workspace, at least `need` bytes
int det_workspace(asr_ctx *ctx, size_t need) {
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (need > ctx->post_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->post_ws) ASR_HIP(ctx, hipFree(ctx->post_ws));
        ctx->post_ws = nullptr; ctx->post_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->post_ws, need));
        ctx->post_ws_bytes = need;
    }
    return ASR_OK;
}

// argument checks and the page table both calls share; pages of the tile size (the host works on float32 maps
// there) and pages `skip` rejects stay status 3
template <typename Skip>
int det_pages(asr_ctx *ctx, const char *who, const int32_t *heights, const int32_t *widths, int n_pages,
              const asr_seg *seg, int32_t *status, int32_t *counts, Skip skip, std::vector<asr::PostPage> &all) {
    if (seg && seg->owner != ctx) return fail(ctx, ASR_ERR_INVALID, "%s: not a segmentation network of this context", who);
    for (int p = 0; p < n_pages; ++p)
        if (heights[p] < 1 || widths[p] < 1 || (int64_t)heights[p] * widths[p] > (1 << 28))
            return fail(ctx, ASR_ERR_INVALID, "%s: page %d has bad geometry %d x %d", who, p, heights[p], widths[p]);
    int64_t map_off = 0;
    for (int p = 0; p < n_pages; ++p) {
        const int h = heights[p], w = widths[p];
        status[p] = 3;
        counts[p] = 0;
        if (!(seg && h == seg->th && w == seg->tw) && !skip(h, w)) {
            asr::PostPage P{};
            P.map_off = map_off; P.h = h; P.w = w; P.page = p;
            all.push_back(P);
        }
        map_off += (int64_t)h * w;
    }
    return ASR_OK;
}

// the chunk's page table with its workspace offsets
std::vector<asr::PostPage> det_chunk_pages(const std::vector<asr::PostPage> &all, const DetChunk &c) {
    std::vector<asr::PostPage> pd(all.begin() + c.first, all.begin() + c.first + c.n);
    int64_t px = 0;
    int32_t rows = 0;
    for (asr::PostPage &P : pd) {
        P.px_off = px; P.row_off = rows;
        px += (int64_t)P.h * P.w; rows += P.h;
    }
    return pd;
}

}  // namespace

extern "C" {

int asr_notes_from_map_dev(asr_ctx *ctx, const double *maps_dev, const int32_t *heights, const int32_t *widths,
                           int n_pages, const asr_seg *seg, double threshold_abs, double threshold_rel,
                           int min_distance, int max_peaks, int32_t *status, int32_t *counts, int32_t *coords) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || max_peaks < 0 || min_distance < 1 || min_distance > asr::DET_MAX_DISTANCE)
        return fail(ctx, ASR_ERR_INVALID, "notes_from_map: bad n_pages=%d max_peaks=%d min_distance=%d (1..%d)", n_pages,
                    max_peaks, min_distance, asr::DET_MAX_DISTANCE);
    if (std::isinf(threshold_abs) || std::isinf(threshold_rel))
        return fail(ctx, ASR_ERR_INVALID, "notes_from_map: an infinite threshold");
    if (n_pages == 0) return ASR_OK;
    if (!maps_dev || !heights || !widths || !status || !counts || (max_peaks && !coords))
        return fail(ctx, ASR_ERR_INVALID, "notes_from_map: NULL argument");
    std::vector<asr::PostPage> all;
    int rc = det_pages(ctx, "notes_from_map", heights, widths, n_pages, seg, status, counts,
                       [](int, int) { return false; }, all);
    if (rc != ASR_OK) return rc;
    if (all.empty()) return ASR_OK;
    const int cap = std::max(max_peaks, 1);

    struct Lay { size_t pd, st, mm, rc, mask, co, end; };
    auto layout = [&](int n, int64_t px, int64_t rows) {
        Lay L;
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += seg_align(bytes); return at; };
        L.pd = take((size_t)n * sizeof(asr::PostPage));
        L.st = take((size_t)n * sizeof(asr::PostState));      // cleared before every chunk: state, extrema
        L.mm = take((size_t)n * 2 * sizeof(uint64_t));
        L.rc = take((size_t)rows * sizeof(int32_t));
        L.mask = take((size_t)px);
        L.co = take((size_t)n * cap * 2 * sizeof(int32_t));
        L.end = o;
        return L;
    };
    size_t need = 0;
    const std::vector<DetChunk> chunks =
        det_chunks(all, [&](int n, int64_t px, int64_t rows) { return layout(n, px, rows).end; }, &need);
    rc = det_workspace(ctx, need);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->post_ws;
    hipStream_t st = ctx->stream;

    std::vector<asr::PostState> h_state;
    std::vector<int32_t> h_coords;
    for (const DetChunk &c : chunks) {
        const Lay L = layout(c.n, c.px, c.rows);
        const std::vector<asr::PostPage> pd = det_chunk_pages(all, c);
        asr::DetArgs a;
        a.pages = (const asr::PostPage *)(ws + L.pd);
        a.n_pages = c.n; a.max_h = c.max_h; a.max_w = c.max_w; a.cap = cap; a.max_px = c.max_px;
        a.maps = maps_dev;
        a.state = (asr::PostState *)(ws + L.st); a.minmax = (unsigned long long *)(ws + L.mm);
        a.threshold_abs = threshold_abs; a.threshold_rel = threshold_rel; a.distance = min_distance;
        a.rowcnt = (int32_t *)(ws + L.rc); a.mask = (uint8_t *)(ws + L.mask); a.coords = (int32_t *)(ws + L.co);
        ASR_HIP(ctx, hipMemcpyAsync(ws + L.pd, pd.data(), pd.size() * sizeof(asr::PostPage), hipMemcpyHostToDevice, st));
        ASR_HIP(ctx, hipMemsetAsync(ws + L.st, 0, L.rc - L.st, st));
        const double dpx = (double)c.px;
        {
            ProfScope ps(ctx, "det_minmax", 0, 2.0 * dpx, 8.0 * dpx);
            ASR_HIP(ctx, asr::launch_det_minmax(st, a));
        }
        {
            ProfScope ps(ctx, "det_peaks", 0, 4.0 * min_distance * dpx, 12.0 * dpx);
            ASR_HIP(ctx, asr::launch_det_peaks(st, a));
        }
        h_state.resize(c.n);
        h_coords.resize((size_t)c.n * cap * 2);
        ASR_HIP(ctx, hipMemcpyAsync(h_state.data(), a.state, h_state.size() * sizeof(asr::PostState), hipMemcpyDeviceToHost, st));
        ASR_HIP(ctx, hipMemcpyAsync(h_coords.data(), a.coords, h_coords.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ASR_HIP(ctx, hipStreamSynchronize(st));
        for (int j = 0; j < c.n; ++j) {
            const int p = pd[j].page;
            const asr::PostState &S = h_state[j];
            if (S.status != 0) continue;                         // (stays 3)
            counts[p] = (int32_t)S.n_kept;
            if (S.n_kept > (uint32_t)max_peaks) {
                status[p] = 4;
                continue;
            }
            status[p] = 0;
            if (S.n_kept)
                memcpy(coords + (size_t)p * max_peaks * 2, h_coords.data() + (size_t)j * cap * 2,
                       (size_t)S.n_kept * 2 * sizeof(int32_t));
        }
    }
    return mark_main(ctx);
}

int asr_bars_from_map_dev(asr_ctx *ctx, const double *maps_dev, const int32_t *heights, const int32_t *widths,
                          int n_pages, const asr_seg *seg, int max_blobs, int32_t *status, int32_t *counts,
                          int64_t *blobs, int32_t *label_passes) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || max_blobs < 0)
        return fail(ctx, ASR_ERR_INVALID, "bars_from_map: bad n_pages=%d max_blobs=%d", n_pages, max_blobs);
    if (label_passes) *label_passes = 0;
    if (n_pages == 0) return ASR_OK;
    if (!maps_dev || !heights || !widths || !status || !counts || (max_blobs && !blobs))
        return fail(ctx, ASR_ERR_INVALID, "bars_from_map: NULL argument");
    std::vector<asr::PostPage> all;
    // the largest raw sum of a blob is below h * w * max(h, w)^2: it has to fit a signed 64-bit integer
    auto too_large = [](int h, int w) {
        const long double m = (long double)std::max(h, w);
        return (long double)h * (long double)w * m * m >= 9223372036854775807.0L;
    };
    int rc = det_pages(ctx, "bars_from_map", heights, widths, n_pages, seg, status, counts, too_large, all);
    if (rc != ASR_OK) return rc;
    if (all.empty()) return ASR_OK;
    const int cap = std::max(max_blobs, 1);

    struct Lay { size_t pd, st, mm, hist, chg, ed, rc, lab, slot, bl, end; };
    auto layout = [&](int n, int64_t px, int64_t rows) {
        Lay L;
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += seg_align(bytes); return at; };
        L.pd = take((size_t)n * sizeof(asr::PostPage));
        L.st = take((size_t)n * sizeof(asr::PostState));      // cleared before every chunk: state .. changed flag
        L.mm = take((size_t)n * 2 * sizeof(uint64_t));
        L.hist = take((size_t)n * 256 * sizeof(uint32_t));
        L.chg = take(sizeof(int32_t));
        L.ed = take((size_t)n * 257 * sizeof(double));
        L.rc = take((size_t)rows * sizeof(int32_t));
        L.lab = take((size_t)px * sizeof(int32_t));
        L.slot = take((size_t)px * sizeof(int32_t));
        L.bl = take((size_t)n * cap * asr::DET_BLOB_FIELDS * sizeof(int64_t));
        L.end = o;
        return L;
    };
    size_t need = 0;
    const std::vector<DetChunk> chunks =
        det_chunks(all, [&](int n, int64_t px, int64_t rows) { return layout(n, px, rows).end; }, &need);
    rc = det_workspace(ctx, need);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->post_ws;
    hipStream_t st = ctx->stream;

    std::vector<asr::PostState> h_state;
    int passes = 0;
    for (const DetChunk &c : chunks) {
        const Lay L = layout(c.n, c.px, c.rows);
        const std::vector<asr::PostPage> pd = det_chunk_pages(all, c);
        asr::DetArgs a;
        a.pages = (const asr::PostPage *)(ws + L.pd);
        a.n_pages = c.n; a.max_h = c.max_h; a.max_w = c.max_w; a.cap = cap; a.max_px = c.max_px;
        a.maps = maps_dev;
        a.state = (asr::PostState *)(ws + L.st); a.minmax = (unsigned long long *)(ws + L.mm);
        a.rowcnt = (int32_t *)(ws + L.rc);
        a.edges = (double *)(ws + L.ed); a.hist = (uint32_t *)(ws + L.hist);
        a.label = (int32_t *)(ws + L.lab); a.slot = (int32_t *)(ws + L.slot); a.blobs = (long long *)(ws + L.bl);
        asr::PostArgs la;                                        // the labelling passes of systems_from_maps
        la.pages = a.pages; la.n_pages = c.n; la.max_px = c.max_px; la.state = a.state; la.label = a.label;
        la.changed = (int32_t *)(ws + L.chg);
        ASR_HIP(ctx, hipMemcpyAsync(ws + L.pd, pd.data(), pd.size() * sizeof(asr::PostPage), hipMemcpyHostToDevice, st));
        ASR_HIP(ctx, hipMemsetAsync(ws + L.st, 0, L.ed - L.st, st));
        const double dpx = (double)c.px;
        {
            ProfScope ps(ctx, "det_minmax", 0, 2.0 * dpx, 8.0 * dpx);
            ASR_HIP(ctx, asr::launch_det_minmax(st, a));
        }
        {
            ProfScope ps(ctx, "det_bar_threshold", 0, 6.0 * dpx, 20.0 * dpx);
            ASR_HIP(ctx, asr::launch_det_bar_threshold(st, a));
        }
        for (;;) {                                               // until a scan changes nothing
            int32_t changed = 0;
            ASR_HIP(ctx, hipMemsetAsync(la.changed, 0, sizeof(int32_t), st));
            {
                ProfScope ps(ctx, "post_label_pass", 0, 0.0, 48.0 * dpx);
                ASR_HIP(ctx, asr::launch_post_label_pass(st, la));
            }
            ASR_HIP(ctx, hipMemcpyAsync(&changed, la.changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            ASR_HIP(ctx, hipStreamSynchronize(st));
            ++passes;
            if (!changed) break;
        }
        {
            ProfScope ps(ctx, "det_bar_blobs", 0, 0.0, 20.0 * dpx);
            ASR_HIP(ctx, asr::launch_det_bar_blobs(st, a));
        }
        h_state.resize(c.n);
        ASR_HIP(ctx, hipMemcpyAsync(h_state.data(), a.state, h_state.size() * sizeof(asr::PostState), hipMemcpyDeviceToHost, st));
        ASR_HIP(ctx, hipStreamSynchronize(st));
        for (int j = 0; j < c.n; ++j) {
            const int p = pd[j].page;
            const asr::PostState &S = h_state[j];
            if (S.status != 0) continue;                         // (stays 3)
            counts[p] = (int32_t)S.n_kept;
            if (S.n_kept > (uint32_t)max_blobs) {
                status[p] = 4;
                continue;
            }
            status[p] = 0;
            if (S.n_kept)
                ASR_HIP(ctx, hipMemcpyAsync(blobs + (size_t)p * max_blobs * asr::DET_BLOB_FIELDS,
                                            a.blobs + (size_t)j * cap * asr::DET_BLOB_FIELDS,
                                            (size_t)S.n_kept * asr::DET_BLOB_FIELDS * sizeof(int64_t),
                                            hipMemcpyDeviceToHost, st));
        }
        ASR_HIP(ctx, hipStreamSynchronize(st));
    }
    if (label_passes) *label_passes = passes;
    return mark_main(ctx);
}

}  // extern "C"
