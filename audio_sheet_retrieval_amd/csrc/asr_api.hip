// C-ABI layer of libasr_hip.so (see include/asr_hip.h for the contract and the
// reference interfaces each entry point replaces).
#include "asr_ctx.h"


namespace asr_detail {

thread_local std::string g_create_error;

int fail(asr_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}


void build_geometry(Tower &t, int nf, int H, int W) {
    const int ch[9][2] = {{1, nf}, {nf, nf}, {nf, 2 * nf}, {2 * nf, 2 * nf}, {2 * nf, 4 * nf},
                          {4 * nf, 4 * nf}, {4 * nf, 4 * nf}, {4 * nf, 4 * nf}, {4 * nf, 32}};
    t.in_h = H; t.in_w = W;
    int h = H, w = W;
    for (int b = 0; b < 9; ++b) {
        LayerGeom &g = t.g[b];
        g.cin = ch[b][0]; g.cout = ch[b][1];
        g.k = b < 8 ? 3 : 1;
        g.pool = (b == 1 || b == 3 || b == 5 || b == 7) ? 1 : 0;
        g.H = h; g.W = w;
        g.OH = g.pool ? h / 2 : h;
        g.OW = g.pool ? w / 2 : w;
        h = g.OH; w = g.OW;
    }
}

ProfRec *prof_rec(asr_ctx *ctx, const std::string &name, double flops, double bytes) {
    for (auto &r : ctx->prof)
        if (r->name == name) { r->flops = flops; r->bytes = bytes; return r.get(); }
    ctx->prof.emplace_back(new ProfRec());
    ProfRec *r = ctx->prof.back().get();
    r->name = name; r->flops = flops; r->bytes = bytes;
    return r;
}

void prof_fold(ProfRec *r) {
    for (auto &p : r->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
            r->total_ms += ms;
            r->launches += 1;
        }
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    r->pending.clear();
}


// (re)derive the per-block launch plans of one tower from its geometry
int plan_tower(asr_ctx *ctx, Tower &tw, int view) {
    if (tw.g[8].H < 1 || tw.g[8].W < 1)
        return fail(ctx, ASR_ERR_INVALID, "view %d input %dx%d too small for four 2x2 pools", view, tw.in_h, tw.in_w);
    // ASR_FUSE1=1/3 starts from a fused plan; otherwise the autotuner decides (autotune_tower): the fused block 2
    // pays block 1's VALU work inside its staging phase (VALU does not hide under the fp32 MFMAs) but the largest
    // activation of the network (3 MB/pair written and read back) never reaches HBM.
    tw.fuse1 = getenv("ASR_FUSE1") != nullptr && (getenv("ASR_FUSE1")[0] == '1' || getenv("ASR_FUSE1")[0] == '3') &&
               getenv("ASR_NO_FUSE1") == nullptr &&
               asr::plan_conv(tw.g[1].cin, tw.g[1].cout, tw.g[1].pool, tw.g[1].H, tw.g[1].W, &tw.plan[1], 0, 1);
    for (int b = tw.fuse1 ? 2 : 1; b < 8; ++b) {
        const LayerGeom &g = tw.g[b];
        if (!asr::plan_conv_v2(g.cin, g.cout, g.pool, g.H, g.W, &tw.plan[b]) &&
            !asr::plan_conv(g.cin, g.cout, g.pool, g.H, g.W, &tw.plan[b]))
            return fail(ctx, ASR_ERR_INVALID, "no conv kernel for %d->%d pool=%d at %dx%d", g.cin, g.cout, g.pool,
                        g.H, g.W);
    }
    for (int b = 0; b < 8; ++b) tw.act_floats[b] = (size_t)tw.g[b].OH * tw.g[b].OW * tw.g[b].cout;
    return ASR_OK;
}

int check_cfg(const asr_config *cfg) {
    if (!cfg) return fail(nullptr, ASR_ERR_INVALID, "asr_create: cfg is NULL");
    if (cfg->struct_size != (int32_t)sizeof(asr_config) && cfg->struct_size != ASR_CONFIG_SIZE_V1)
        return fail(nullptr, ASR_ERR_INVALID, "asr_create: struct_size %d != %d (ABI mismatch)", cfg->struct_size,
                    (int)sizeof(asr_config));
    if (cfg->struct_size == (int32_t)sizeof(asr_config) && cfg->pool_ties != ASR_POOL_TIES_ALL &&
        cfg->pool_ties != ASR_POOL_TIES_FIRST)
        return fail(nullptr, ASR_ERR_INVALID, "asr_create: pool_ties must be 0 (every tied element) or 1 (first), got %d",
                    cfg->pool_ties);
    if (cfg->num_filters != 12 && cfg->num_filters != 24)
        return fail(nullptr, ASR_ERR_INVALID, "asr_create: num_filters must be 12 or 24, got %d", cfg->num_filters);
    if (cfg->dim_latent != 32) return fail(nullptr, ASR_ERR_INVALID, "asr_create: dim_latent must be 32");
    if (cfg->h1 < 16 || cfg->w1 < 16 || cfg->h2 < 16 || cfg->w2 < 16 || cfg->h1 > 4096 || cfg->w1 > 4096 ||
        cfg->h2 > 4096 || cfg->w2 > 4096)
        return fail(nullptr, ASR_ERR_INVALID, "asr_create: input sizes out of range");
    return ASR_OK;
}

void free_train(asr_ctx *ctx) {
    if (!ctx->train) return;
    TrainState &T = *ctx->train;
    for (auto &t : T.tw) {
        for (int b = 0; b < 9; ++b) {
            if (t.x[b]) hipFree(t.x[b]);
            if (t.z[b]) hipFree(t.z[b]);
            if (t.stats[b]) hipFree(t.stats[b]);
            if (t.zsel[b]) hipFree(t.zsel[b]);
            if (t.ztie[b]) hipFree(t.ztie[b]);
            if (t.wdgrad[b]) hipFree(t.wdgrad[b]);
        }
        float *fp[] = {t.dz, t.dz2, t.dA, t.dB, t.H, t.dH, t.lv, t.wpartial};
        for (float *q : fp) if (q) hipFree(q);
        if (t.wstream) {                                        // tower 1's is the context's wside_stream: not destroyed here
            (void)hipStreamSynchronize(t.wstream);
            if (t.wstream != ctx->wside_stream) (void)hipStreamDestroy(t.wstream);
        }
        for (int k = 0; k < 2; ++k) {
            if (t.e_dz[k]) hipEventDestroy(t.e_dz[k]);
            if (t.e_wg[k]) hipEventDestroy(t.e_wg[k]);
        }
        if (t.partial) hipFree(t.partial);
        if (t.fstats) hipFree(t.fstats);
        if (t.ticket) hipFree(t.ticket);
        if (t.sums && &t == &T.tw[0]) hipFree(t.sums);         // (tower 2's is the second half of tower 1's)
    }
    float *fp[] = {T.pmaster, T.pgrad, T.adam_m, T.adam_v, T.loss_dev, T.lvv[0], T.lvv[1],
                   T.Hg[0], T.Hg[1], T.dHg[0], T.dHg[1], T.lvg[0], T.lvg[1], T.Hpad[0], T.Hpad[1]};
    for (float *q : fp) if (q) hipFree(q);
    if (T.mask) hipFree(T.mask);
    if (T.raw1) hipFree(T.raw1);
    if (T.repack_dev) hipFree(T.repack_dev);
    if (T.cca_ws) hipFree(T.cca_ws);
    if (T.l2_dev) hipFree(T.l2_dev);
    if (T.cca_done) hipEventDestroy(T.cca_done);
    for (hipEvent_t e : T.gate) if (e) hipEventDestroy(e);
    ctx->train.reset();
}

void free_comm(asr_ctx *ctx) {
    if (!ctx->comm) return;
    Comm &c = *ctx->comm;
    for (auto &pr : c.timed) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    c.timed.clear();
    if (c.nccl && c.pCommDestroy) (void)c.pCommDestroy(c.nccl);
    if (c.dl) dlclose(c.dl);
    ctx->comm.reset();
    ctx->exch = asr::Exchange{};
}

void free_pipe(asr_ctx *ctx) {
    auto &P = ctx->pipe;
    for (int s = 0; s < 2; ++s) {
        void *bufs[] = {P.in1[s], P.in2[s], P.lv1[s], P.lv2[s], P.ranks[s], P.ties[s], P.dstar[s]};
        for (void *b : bufs) if (b) (void)hipFree(b);
        hipEvent_t evs[] = {P.ready[s], P.done[s], P.out[s]};
        for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    }
    if (P.h2d && P.h2d != ctx->copy_streams[0]) (void)hipStreamDestroy(P.h2d);     // (the context's own streams stay)
    if (P.d2h && P.d2h != ctx->copy_streams[1]) (void)hipStreamDestroy(P.d2h);
    P = asr_ctx::Pipe{};
}

void free_hpipe(asr_ctx *ctx) {
    auto &H = ctx->hpipe;
    for (int s = 0; s < asr_ctx::HostPipe::NSLOT; ++s) {
        if (H.pin[s]) (void)hipHostFree(H.pin[s]);
        if (H.dev[s]) (void)hipFree(H.dev[s]);
        if (H.copied[s]) (void)hipEventDestroy(H.copied[s]);
        if (H.consumed[s]) (void)hipEventDestroy(H.consumed[s]);
        H.pin[s] = H.dev[s] = nullptr; H.copied[s] = H.consumed[s] = nullptr; H.used[s] = false;
    }
    H.slot_bytes = 0;
    if (H.out_dev) (void)hipFree(H.out_dev);
    H.out_dev = nullptr; H.out_floats = 0;
    if (H.h2d && H.h2d != ctx->copy_streams[2]) (void)hipStreamDestroy(H.h2d);
    H.h2d = nullptr;
    H.pool.reset();
}

void free_ctx_buffers(asr_ctx *ctx) {
    free_train(ctx);
    free_comm(ctx);
    free_pipe(ctx);
    free_hpipe(ctx);
    for (auto &t : ctx->tw) {
        for (int b = 0; b < 9; ++b) { if (t.w_dev[b]) hipFree(t.w_dev[b]); if (t.bn_dev[b]) hipFree(t.bn_dev[b]); }
        for (int b = 0; b < 8; ++b) if (t.act[b]) hipFree(t.act[b]);
    }
    if (ctx->cca_dev) hipFree(ctx->cca_dev);
    for (int v = 0; v < 2; ++v) {
        if (ctx->in_stage[v]) hipFree(ctx->in_stage[v]);
        if (ctx->out_stage[v]) hipFree(ctx->out_stage[v]);
        if (ctx->vdone[v]) hipEventDestroy(ctx->vdone[v]);
        if (ctx->vstream[v]) hipStreamDestroy(ctx->vstream[v]);
    }
    if (ctx->main_done) hipEventDestroy(ctx->main_done);
    if (ctx->wside_stream) { (void)hipStreamSynchronize(ctx->wside_stream); (void)hipStreamDestroy(ctx->wside_stream); }
    for (hipStream_t &cs : ctx->copy_streams)
        if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); cs = nullptr; }
    if (ctx->norm1) hipFree(ctx->norm1);
    if (ctx->norm2) hipFree(ctx->norm2);
    if (ctx->cca_ws) hipFree(ctx->cca_ws);
    if (ctx->topk_ws) hipFree(ctx->topk_ws);
    if (ctx->dtw_ws) hipFree(ctx->dtw_ws);
    if (ctx->subseq_ws) hipFree(ctx->subseq_ws);
    if (ctx->vote_ws) hipFree(ctx->vote_ws);
    if (ctx->post_ws) hipFree(ctx->post_ws);
    if (ctx->resample_ws) hipFree(ctx->resample_ws);
    if (ctx->specfft_ws) hipFree(ctx->specfft_ws);
    if (ctx->resize_ws) hipFree(ctx->resize_ws);
    if (ctx->skew_ws) hipFree(ctx->skew_ws);
    if (ctx->stream_ws) hipFree(ctx->stream_ws);
    if (ctx->stream_taps) hipFree(ctx->stream_taps);
    if (ctx->topk_tickets) hipFree(ctx->topk_tickets);
    if (ctx->unit_ws) hipFree(ctx->unit_ws);
    if (ctx->rank_io) hipFree(ctx->rank_io);
    if (ctx->valid_ws) hipFree(ctx->valid_ws);
    for (auto &r : ctx->prof) prof_fold(r.get());
    if (ctx->stream) hipStreamDestroy(ctx->stream);
}

// stats / stats_rows: train-mode forward only - a RAW Winograd plan also writes the BatchNorm partial sums of its outputs
// (*stats_rows > 0 on return); every other plan leaves *stats_rows at 0 and the caller runs the separate pass
hipError_t launch_conv_any(asr_ctx *ctx, hipStream_t st, const asr::ConvPlan &p, const float *in, const float *w,
                           const float *bn, float *out, int n, const asr::Fuse1Args *f1, double *stats, int *stats_rows) {
    if (stats_rows) *stats_rows = 0;
    if (p.variant >= 4000)
        return asr::launch_conv_wino4(st, p, in, w + asr::conv_wpack_floats(p.cin, p.cout) + asr::wino_wpack_floats(p.cin, p.cout),
                                      bn, out, n, ctx->num_cus, stats, stats_rows);
    if (p.variant >= 3000)
        return asr::launch_conv_wino(st, p, in, w + asr::conv_wpack_floats(p.cin, p.cout), bn, out, n, ctx->num_cus,
                                     stats, stats_rows, p.fuse1 ? f1 : nullptr);
    if (p.variant >= 2000) return asr::launch_conv_v3(st, p, in, w, bn, out, n, ctx->num_cus, p.fuse1 ? f1 : nullptr);
    return p.variant >= 1000 ? asr::launch_conv_v2(st, p, in, w, bn, out, n, ctx->num_cus)
                             : asr::launch_conv(st, p, in, w, bn, out, n, ctx->num_cus, f1);
}

// "Measure, don't guess": for every MFMA conv block, time the cheapest few tilings of both schedules (by the
// planner's model) on the real buffers at the context's chunk size and keep the fastest.  ~0.5 s once per context.
// 31-bit tag of this build (asr_version() carries the source hash) for the lines of an ASR_TUNE_CACHE file
int tune_cache_tag() {
    static int tag = -1;
    if (tag < 0) {
        unsigned h = 2166136261u;
        for (const char *p = asr_version(); *p; ++p) h = (h ^ (unsigned char)*p) * 16777619u;
        tag = (int)(h & 0x7fffffffu);
    }
    return tag;
}

int autotune_tower(asr_ctx *ctx, int view) {
    Tower &t = ctx->tw[view - 1];
    hipStream_t st = ctx->estream[view - 1];
    const int n = ctx->chunk;
    hipEvent_t e0, e1;
    ASR_HIP(ctx, hipEventCreate(&e0));
    ASR_HIP(ctx, hipEventCreate(&e1));
    const bool dbg = getenv("ASR_DEBUG") != nullptr;
    for (int b = 1; b < 8; ++b) {
        const LayerGeom &g = t.g[b];
        std::vector<asr::ConvPlan> cands;
        cands.push_back(t.plan[b]);                                   // the model's choice stays a candidate
        // block 2 may absorb block 1 (ConvPlan.fuse1): ASR_FUSE1=auto - the tuner decides by time, counting block 1's
        // own kernel against the unfused candidates; "1" / "3" always fused; unset or "0" never
        const char *fenv = getenv("ASR_FUSE1");
        const bool forced = (b == 1 && t.fuse1);
        // default (unset): not tried - on the 160x200 tower fusion wins by ~2 % only, and which of the two nearly
        // equal schedules a context ends up with would vary from run to run; "auto" lets the tuner decide
        const bool try_fused = (b == 1) && fenv && fenv[0] != '0' && fenv[0] != 'w' && getenv("ASR_NO_FUSE1") == nullptr;
        // block 1 evaluated by producer waves inside the Winograd block 2 (conv3x3_wino, PW > 0): part of the default
        // candidate set wherever the build exists (C_in = 12: the `cont` model); ASR_FUSE1=0 keeps it out, =w forces it
        const bool try_wfused = (b == 1) && !(fenv && fenv[0] == '0') && getenv("ASR_NO_FUSE1") == nullptr &&
                                !(view == 1 && ctx->cfg.resize_view1) && !forced;
        const bool only_wfused = try_wfused && fenv && fenv[0] == 'w';
        if (!forced) {
            asr::conv_candidates_v1(g.cin, g.cout, g.pool, g.H, g.W, 0, 5, &cands, 0);
            asr::conv_candidates_v2(g.cin, g.cout, g.pool, g.H, g.W, 5, &cands);
            asr::conv_candidates_v3(g.cin, g.cout, g.pool, g.H, g.W, 6, &cands, 0);
            asr::conv_candidates_wino(g.cin, g.cout, g.pool, g.H, g.W,
                                      getenv("ASR_WINO_CANDS") ? atoi(getenv("ASR_WINO_CANDS")) : 4, &cands);
            asr::conv_candidates_wino4(g.cin, g.cout, g.pool, g.H, g.W, &cands);
        } else {
            asr::conv_candidates_v1(g.cin, g.cout, g.pool, g.H, g.W, 0, 5, &cands, 1);
        }
        if (try_fused) asr::conv_candidates_v3(g.cin, g.cout, g.pool, g.H, g.W, 6, &cands, 1);
        if (try_wfused) {
            asr::conv_candidates_wino_fused(g.cin, g.cout, g.pool, g.H, g.W, 3, &cands);
            if (only_wfused) {
                std::vector<asr::ConvPlan> only;
                for (auto &c : cands)
                    if (c.variant >= 3000 && c.variant < 3500 && c.fuse1) only.push_back(c);
                if (!only.empty()) cands.swap(only);
            }
        }
        if (b == 1 && fenv && fenv[0] == '3') {      // tests: only the v3 fused schedule
            std::vector<asr::ConvPlan> only;
            for (auto &c : cands)
                if (c.variant >= 2000 && c.fuse1) only.push_back(c);
            if (!only.empty()) cands.swap(only);
        }
        // ASR_TUNE_ONLY=direct|wino|winog|wino4 (tests, experiments): keep one family of schedules where the block has it
        if (const char *only_env = getenv("ASR_TUNE_ONLY")) {
            const int lo = !strcmp(only_env, "wino4") ? 4000 : !strcmp(only_env, "winog") ? 3500 : !strcmp(only_env, "wino") ? 3000 : 0;
            const int hi = !strcmp(only_env, "wino4") ? 5000 : !strcmp(only_env, "winog") ? 4000 : !strcmp(only_env, "wino") ? 3500 : 3000;
            std::vector<asr::ConvPlan> only;
            for (auto &c : cands)
                if (c.variant >= lo && c.variant < hi) only.push_back(c);
            if (!only.empty()) cands.swap(only);
        }
        // a fused block 2 reads the raw input: time it on the (0.5-filled) block-1 buffer taken as a prepared image
        asr::Fuse1Args f1{t.act[0], t.w_dev[0], t.bn_dev[0], ASR_IN_F32_PREPARED, 0, g.H, g.W};
        const asr::Fuse1Args *pf1 = &f1;
        double conv1_ms = 0.0;
        bool any_fused = false;
        for (auto &c : cands) any_fused = any_fused || c.fuse1;
        if (b == 1 && any_fused && !forced) {
            // what the unfused candidates pay on top: block 1's own kernel (input: block 2's output buffer as an image)
            const LayerGeom &g0 = t.g[0];
            ASR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)t.act[1], 0x3f000000, (size_t)g0.H * g0.W * n, st));
            (void)asr::launch_conv1(st, t.act[1], ASR_IN_F32_PREPARED, 0, t.w_dev[0], t.bn_dev[0], t.act[0], n, g0.H, g0.W,
                                    g0.H, g0.W, g0.cout);
            ASR_HIP(ctx, hipEventRecord(e0, st));
            for (int r = 0; r < 2; ++r)
                (void)asr::launch_conv1(st, t.act[1], ASR_IN_F32_PREPARED, 0, t.w_dev[0], t.bn_dev[0], t.act[0], n, g0.H,
                                        g0.W, g0.H, g0.W, g0.cout);
            ASR_HIP(ctx, hipEventRecord(e1, st));
            ASR_HIP(ctx, hipEventSynchronize(e1));
            float ms = 0.f;
            ASR_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
            conv1_ms = ms / 2;
            if (dbg) fprintf(stderr, "[asr] tune v%d conv1 alone: %.4f ms\n", view, conv1_ms);
        }
        // defined input values (0.5f): timing must not depend on stale NaN / denormal bit patterns.
        // ASR_TUNE_VERIFY=1: a deterministic pattern instead, and every (unfused) candidate's output is compared
        // with the first one's - all schedules evaluate the same fp32 FMA chains in the same order.
        const bool verify = getenv("ASR_TUNE_VERIFY") != nullptr;
        const size_t out_floats = t.act_floats[b] * (size_t)n;
        float *vref = nullptr;
        uint32_t *vbits = nullptr;
        bool have_ref = false;
        if (verify) {
            ASR_HIP(ctx, asr::launch_fill_pattern(st, t.act[b - 1], (int64_t)t.act_floats[b - 1] * n));
            ASR_HIP(ctx, hipMalloc((void **)&vref, out_floats * sizeof(float) + 16));
            vbits = reinterpret_cast<uint32_t *>(vref + out_floats);
        } else
        ASR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)t.act[b - 1], 0x3f000000, t.act_floats[b - 1] * n, st));
        double best_ms = 1e30;
        int best = -1;
        // ASR_TUNE_CACHE=<file>: choices of an earlier run on the same geometry are re-used (and new ones appended),
        // so that a server restart or a profiled run does not repeat the timing launches
        const char *cache = getenv("ASR_TUNE_CACHE");
        const int nf = ctx->cfg.num_filters;
        if (cache) {
            // lines carry the build's tag (variant numbers are table indices: a cache written by another build of the
            // library would name other kernels); lines of other builds or formats are skipped
            if (FILE *fp = fopen(cache, "r")) {
                char line[256];
                while (fgets(line, sizeof line, fp)) {
                    int k[10], tag = 0;
                    if (sscanf(line, "v2 %d %d %d %d %d %d %d %d %d %d %d", &tag, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5],
                               &k[6], &k[7], &k[8], &k[9]) != 11 || tag != tune_cache_tag())
                        continue;
                    if (k[0] != nf || k[1] != view || k[2] != b || k[3] != g.H || k[4] != g.W || k[5] != n) continue;
                    for (size_t c = 0; c < cands.size(); ++c)
                        if (cands[c].variant == k[6] && cands[c].TH == k[7] && cands[c].TW == k[8] && cands[c].NI == k[9])
                            best = (int)c;
                }
                fclose(fp);
            }
        }
        if (best >= 0) {
            t.plan[b] = cands[best];
            if (b == 1) t.fuse1 = cands[best].fuse1 != 0;
            if (dbg) fprintf(stderr, "[asr] tuned v%d conv%d from cache%s\n", view, b + 1, t.fuse1 && b == 1 ? " (fused)" : "");
            continue;
        }
        best = 0;
        for (size_t c = 0; c < cands.size(); ++c) {
            // every candidate starts from NaNs: an output it leaves unwritten must not pass on the correct value that
            // the candidate before it left in the same buffer
            if (verify) ASR_HIP(ctx, hipMemsetAsync(t.act[b], 0xff, out_floats * sizeof(float), st));
            hipError_t e = launch_conv_any(ctx, st, cands[c], t.act[b - 1], t.w_dev[b], t.bn_dev[b], t.act[b], n, pf1);
            if (e != hipSuccess) { (void)hipGetLastError(); continue; }          // e.g. LDS request refused
            if (verify && !cands[c].fuse1) {
                if (!have_ref) {
                    ASR_HIP(ctx, hipMemcpyAsync(vref, t.act[b], out_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
                    have_ref = true;
                } else {
                    uint32_t bits = 0;
                    ASR_HIP(ctx, asr::launch_max_abs_diff(st, t.act[b], vref, (int64_t)out_floats, vbits));
                    ASR_HIP(ctx, hipMemcpyAsync(&bits, vbits, sizeof bits, hipMemcpyDeviceToHost, st));
                    ASR_HIP(ctx, hipStreamSynchronize(st));
                    float diff;
                    memcpy(&diff, &bits, sizeof diff);
                    ctx->tune_checked += 1;
                    // the Winograd schedule sums in a different order: same fp32, 1e-4 instead of 1e-5
                    if (!(diff <= (cands[c].variant >= 3000 ? 1e-4f : 1e-5f))) {
                        ctx->tune_bad += 1;
                        fprintf(stderr, "[asr] TUNE VERIFY MISMATCH view %d conv%d variant %d tile %dx%d x%d: max |diff| %g\n",
                                view, b + 1, cands[c].variant, cands[c].TH, cands[c].TW, cands[c].NI, (double)diff);
                    }
                    if (diff > ctx->tune_max_diff || diff != diff) ctx->tune_max_diff = diff;
                }
            }
            ASR_HIP(ctx, hipEventRecord(e0, st));
            for (int r = 0; r < 2; ++r)
                (void)launch_conv_any(ctx, st, cands[c], t.act[b - 1], t.w_dev[b], t.bn_dev[b], t.act[b], n, pf1);
            ASR_HIP(ctx, hipEventRecord(e1, st));
            ASR_HIP(ctx, hipEventSynchronize(e1));
            float ms = 0.f;
            ASR_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
            if (dbg)
                fprintf(stderr, "[asr] tune v%d conv%d%s %s#%d tile %dx%d x%d lds %d bpc %d: %.4f ms\n", view, b + 1,
                        cands[c].fuse1 ? "+1" : "",
                        cands[c].variant >= 4000 ? "wino4" : cands[c].variant >= 3000 ? "wino" : cands[c].variant >= 2000 ? "v3" : cands[c].variant >= 1000 ? "v2" : "v1",
                        cands[c].variant % 1000, cands[c].TH, cands[c].TW,
                        cands[c].NI, cands[c].lds_bytes, cands[c].blocks_per_cu, ms / 2);
            // the row-major tile order of the global-A Winograd kernel re-reads up to 1.6x its input from HBM: it has to
            // beat the two-row strips by more than 2 % to be chosen
            const bool rowmajor_winog = cands[c].variant >= 3500 && cands[c].variant < 4000 && cands[c].TH == 1;
            // F(4x4) rounds ten times coarser than F(2x2) and differs from it in the last bits: where the two tie (conv5,
            // within 0.3 % since the global-A F(2x2) kernels lost their per-lane divisions) the pick must not hang on
            // timing noise - two engines of one process would embed the same input to different bits - so F(4x4) has
            // to win by more than 2 % as well (elsewhere it wins by 8 % or more, or loses)
            const bool wino4 = cands[c].variant >= 4000;
            const double cost = (ms / 2) * ((rowmajor_winog || wino4) ? 1.02 : 1.0) + (cands[c].fuse1 ? 0.0 : conv1_ms);
            if (cost < best_ms) { best_ms = cost; best = (int)c; }
        }
        if (vref) (void)hipFree(vref);
        t.plan[b] = cands[best];
        if (b == 1) t.fuse1 = cands[best].fuse1 != 0;
        if (cache) {
            if (FILE *fp = fopen(cache, "a")) {
                fprintf(fp, "v2 %d %d %d %d %d %d %d %d %d %d %d\n", tune_cache_tag(), nf, view, b, g.H, g.W, n,
                        cands[best].variant, cands[best].TH, cands[best].TW, cands[best].NI);
                fclose(fp);
            }
        }
        if (dbg)
            fprintf(stderr, "[asr] tuned v%d conv%d -> %s#%d tile %dx%d x%d (%.4f ms for %d samples)\n", view, b + 1,
                    cands[best].variant >= 4000 ? "wino4" : cands[best].variant >= 3000 ? "wino" : cands[best].variant >= 2000 ? "v3" : cands[best].variant >= 1000 ? "v2" : "v1",
                    cands[best].variant % 1000, cands[best].TH,
                    cands[best].TW, cands[best].NI, best_ms, n);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ASR_OK;
}

// activation / staging buffers are allocated on the first embed call, so that a
// context used only for ranking or CCA fitting stays small
int ensure_workspace(asr_ctx *ctx, int view) {
    Tower &t = ctx->tw[view - 1];
    for (int b = 0; b < 8; ++b)
        if (!t.act[b]) ASR_HIP(ctx, hipMalloc((void **)&t.act[b], t.act_floats[b] * ctx->chunk * sizeof(float)));
    if (!t.tuned) {
        t.tuned = true;
        const char *e = getenv("ASR_AUTOTUNE");
        if (!(e && e[0] == '0')) return autotune_tower(ctx, view);
    }
    return ASR_OK;
}

int ensure_staging(asr_ctx *ctx, int view) {
    const int v = view - 1;
    if (!ctx->in_stage[v]) ASR_HIP(ctx, hipMalloc(&ctx->in_stage[v], ctx->in_stage_bytes));
    if (!ctx->out_stage[v])
        ASR_HIP(ctx, hipMalloc((void **)&ctx->out_stage[v], (size_t)ctx->chunk * 32 * sizeof(float)));
    return ASR_OK;
}

// the main stream consumes what the tower streams produced
int join_views(asr_ctx *ctx) {
    for (int v = 0; v < 2; ++v)
        if (ctx->vpending[v]) {
            ASR_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->vdone[v], 0));
            ctx->vpending[v] = false;
        }
    return ASR_OK;
}

int mark_main(asr_ctx *ctx) {
    ASR_HIP(ctx, hipEventRecord(ctx->main_done, ctx->stream));
    ctx->main_pending = true;
    return ASR_OK;
}

int sync_all(asr_ctx *ctx) {
    for (int v = 0; v < 2; ++v) ASR_HIP(ctx, hipStreamSynchronize(ctx->vstream[v]));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->vpending[0] = ctx->vpending[1] = false;
    ctx->main_pending = false;
    return ASR_OK;
}


// one tower, one chunk already on the device
int run_tower(asr_ctx *ctx, int view, const void *x_dev, int in_mode, int n, float *features_dev, float *latent_dev) {
    Tower &t = ctx->tw[view - 1];
    const asr_config &c = ctx->cfg;
    hipStream_t st = ctx->estream[view - 1];
    const int rsz = (view == 1) ? c.resize_view1 : 0;
    const int hraw = (view == 1) ? c.h1 : c.h2, wraw = (view == 1) ? c.w1 : c.w2;
    if (!t.fuse1) {
        const LayerGeom &g = t.g[0];
        ProfScope ps(ctx, "conv1", view, 2.0 * n * g.H * g.W * 9.0 * g.cout,
                     (double)n * g.H * g.W * (4.0 + 4.0 * g.cout), asr::conv1_symbol(g.cout, in_mode, rsz, n, g.H, g.W, hraw, wraw));
        ASR_HIP(ctx, asr::launch_conv1(st, x_dev, in_mode, rsz, t.w_dev[0], t.bn_dev[0], t.act[0], n, hraw,
                                       wraw, g.H, g.W, g.cout));
    }
    for (int b = 1; b < 8; ++b) {
        const LayerGeom &g = t.g[b];
        const bool fused = (b == 1 && t.fuse1);
        char name[32];
        snprintf(name, sizeof name, fused ? "conv1+%d" : "conv%d", b + 1);
        ProfScope ps(ctx, name, view,
                     2.0 * n * g.H * g.W * 9.0 * g.cin * g.cout + (fused ? 2.0 * n * g.H * g.W * 9.0 * g.cin : 0.0),
                     4.0 * n * ((double)g.H * g.W * (fused ? 1 : g.cin) + (double)g.OH * g.OW * g.cout),
                     fused ? asr::conv_wino_symbol(t.plan[b], in_mode) : t.plan[b].symbol);
        asr::Fuse1Args f1{x_dev, t.w_dev[0], t.bn_dev[0], in_mode, rsz, hraw, wraw};
        ASR_HIP(ctx, launch_conv_any(ctx, st, t.plan[b], t.act[b - 1], t.w_dev[b], t.bn_dev[b], t.act[b], n,
                                     fused ? &f1 : nullptr));
    }
    {
        const LayerGeom &g = t.g[8];
        ProfScope ps(ctx, "tail", view, 2.0 * n * (g.H * g.W * (double)g.cin * 32 + 32.0 * 32),
                     4.0 * n * ((double)g.H * g.W * g.cin + 64));
        const float *mean = ctx->cca_dev + 2048 + (view == 1 ? 0 : 32);
        const float *proj = ctx->cca_dev + (view == 1 ? 0 : 1024);
        ASR_HIP(ctx, asr::launch_tail(st, t.act[7], n, g.H, g.W, g.cin, t.w_dev[8], t.bn_dev[8], mean, proj,
                                      features_dev, latent_dev));
    }
    ctx->last_n[view - 1] = n;
    return ASR_OK;
}

size_t input_bytes_per_sample(const asr_ctx *ctx, int view, int in_mode) {
    const asr_config &c = ctx->cfg;
    if (view == 2) return (size_t)c.h2 * c.w2 * 4;
    if (in_mode == ASR_IN_F32_PREPARED) return (size_t)ctx->tw[0].in_h * ctx->tw[0].in_w * 4;
    return (size_t)c.h1 * c.w1 * (in_mode == ASR_IN_U8_RAW ? 1 : 4);
}

int embed_common(asr_ctx *ctx, int view, const void *x, int in_mode, int64_t n, int out_kind, float *out,
                 bool on_device) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!ctx->params_set) return fail(ctx, ASR_ERR_STATE, "embed: asr_set_params has not been called");
    if (n < 0 || (n > 0 && (!x || !out))) return fail(ctx, ASR_ERR_INVALID, "embed: NULL buffer or negative n");
    if (in_mode < 0 || in_mode > 2 || (view == 2 && in_mode != ASR_IN_F32_PREPARED))
        return fail(ctx, ASR_ERR_INVALID, "embed: bad in_mode %d for view %d", in_mode, view);
    if (out_kind != ASR_OUT_LATENT && out_kind != ASR_OUT_FEATURES)
        return fail(ctx, ASR_ERR_INVALID, "embed: bad out_kind %d", out_kind);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (n > 0) {
        int rcw = ensure_workspace(ctx, view);
        if (rcw != ASR_OK) return rcw;
    }
    if (ctx->wino_stale) {
        int rcr = refresh_wino_weights(ctx);
        if (rcr != ASR_OK) return rcr;
    }
    const size_t bps = input_bytes_per_sample(ctx, view, in_mode);
    hipStream_t st = ctx->estream[view - 1];
    if (n > 0 && !on_device) {
        int rcs = ensure_staging(ctx, view);
        if (rcs != ASR_OK) return rcs;
    }
    if (n > 0 && on_device && ctx->main_pending)      // the previous consumer may still read out_dev
        ASR_HIP(ctx, hipStreamWaitEvent(st, ctx->main_done, 0));
    for (int64_t s0 = 0; s0 < n; s0 += ctx->chunk) {
        const int nc = (int)std::min<int64_t>(ctx->chunk, n - s0);
        const void *xin;
        float *o;
        if (on_device) {
            xin = (const char *)x + (size_t)s0 * bps;
            o = out + (size_t)s0 * 32;
        } else {
            ASR_HIP(ctx, hipMemcpyAsync(ctx->in_stage[view - 1], (const char *)x + (size_t)s0 * bps,
                                        (size_t)nc * bps, hipMemcpyHostToDevice, st));
            xin = ctx->in_stage[view - 1];
            o = ctx->out_stage[view - 1];
        }
        int rc = run_tower(ctx, view, xin, in_mode, nc, out_kind == ASR_OUT_FEATURES ? o : nullptr,
                           out_kind == ASR_OUT_LATENT ? o : nullptr);
        if (rc != ASR_OK) return rc;
        if (!on_device) {
            ASR_HIP(ctx, hipMemcpyAsync(out + (size_t)s0 * 32, o, (size_t)nc * 32 * sizeof(float),
                                        hipMemcpyDeviceToHost, st));
            ASR_HIP(ctx, hipStreamSynchronize(st));
        }
    }
    if (n > 0 && on_device) {
        ASR_HIP(ctx, hipEventRecord(ctx->vdone[view - 1], st));
        ctx->vpending[view - 1] = true;
    }
    return ASR_OK;
}

bool host_pointer_is_pinned(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {      // plain malloc'ed memory: "invalid value"
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Host-buffer embedding of any length (what RetrievalWrapper.compute_view_1/2, run_eval.py:107-108 and
// refine_cca.py:95-97 ask for, chunk by chunk, through batch_compute1/2).  Rows are independent in deterministic
// mode, so the caller's chunking is not observable; here the array is cut into granules (125, 250, 500, 500 ...
// samples) and the H2D of granule k+1 on the copy stream overlaps the tower of granule k (with ASR_HOST_STAGE=1 also
// the staging copy of granule k+2, pageable -> page-locked; skipped when the caller's memory is page-locked already).
// Every embedding lands in one device buffer and returns in a single D2H; one host synchronisation per call.
// With `loss` (asr_valid_output_in) the two jobs are the two views of the same pairs: the main stream joins both towers,
// rank_loss_kernel reads the latents in place, and the loss returns with them.
int embed_host(asr_ctx *ctx, const HostJob *jobs, int njobs, float *loss) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!ctx->params_set) return fail(ctx, ASR_ERR_STATE, "embed: asr_set_params has not been called");
    if (loss && (njobs != 2 || jobs[0].view != 1 || jobs[1].view != 2 || jobs[0].n != jobs[1].n || jobs[0].n < 2 ||
                 jobs[0].out_kind != ASR_OUT_LATENT || jobs[1].out_kind != ASR_OUT_LATENT))
        return fail(ctx, ASR_ERR_INVALID, "valid_output: two views of the same n >= 2 pairs, latents");
    int64_t total = 0;
    size_t max_bps = 0;
    for (int j = 0; j < njobs; ++j) {
        const HostJob &J = jobs[j];
        if (J.n < 0 || (J.n > 0 && (!J.x || (!J.out && !loss)))) return fail(ctx, ASR_ERR_INVALID, "embed: NULL buffer or negative n");
        if (J.in_mode < 0 || J.in_mode > 2 || (J.view == 2 && J.in_mode != ASR_IN_F32_PREPARED))
            return fail(ctx, ASR_ERR_INVALID, "embed: bad in_mode %d for view %d", J.in_mode, J.view);
        if (J.out_kind != ASR_OUT_LATENT && J.out_kind != ASR_OUT_FEATURES)
            return fail(ctx, ASR_ERR_INVALID, "embed: bad out_kind %d", J.out_kind);
        total += J.n;
        if (J.n > 0) max_bps = std::max(max_bps, input_bytes_per_sample(ctx, J.view, J.in_mode));
    }
    if (total == 0) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    for (int j = 0; j < njobs; ++j)
        if (jobs[j].n > 0) {
            int rcw = ensure_workspace(ctx, jobs[j].view);
            if (rcw != ASR_OK) return rcw;
        }
    if (ctx->wino_stale) {
        int rcr = refresh_wino_weights(ctx);
        if (rcr != ASR_OK) return rcr;
    }
    auto &H = ctx->hpipe;
    constexpr int NS = asr_ctx::HostPipe::NSLOT;
    // ASR_HOST_STAGE=1: copy pageable caller memory into the page-locked slots first (CopyPool) instead of handing it
    // to hipMemcpyAsync directly.  Measured on the MI355X box (2000 pairs through RetrievalWrapper, uint8 / float32
    // sheets): direct 9.2 / 9.6 ms, staged with 4 + 1 copy threads 10.6 / 13.4 ms - the runtime's own pageable path
    // (pin in place) is faster than any host-side copy here, so direct is the default.
    // The switch is read ONCE, when the pipe is set up, and latched: the page-locked slots and the copy threads exist or
    // not for the life of the context (a value flipped to 1 later met slots without page-locked memory: a copy to NULL).
    // `granule` marks a completed set-up and is written last: a failed stream / event creation leaves the pipe unset
    // and the next call tries again instead of running on null handles.
    if (!H.granule) {
        H.staged = getenv("ASR_HOST_STAGE") && getenv("ASR_HOST_STAGE")[0] == '1';
        const char *g = getenv("ASR_HOST_GRANULE"), *g0 = getenv("ASR_HOST_GRANULE_FIRST");
        const int granule = std::max(1, std::min(ctx->chunk, g ? atoi(g) : 500));
        H.granule_first = std::max(1, std::min(granule, g0 ? atoi(g0) : 125));
        const char *t = getenv("ASR_COPY_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        const int nt = !H.staged ? 0 : t ? atoi(t) : std::max(0, std::min(4, hw / 2 - 1));
        H.pool.reset(new CopyPool(std::max(0, std::min(nt, 32))));
        if (!H.h2d) {
            if (ctx->copy_streams[2]) H.h2d = ctx->copy_streams[2];
            else ASR_HIP(ctx, hipStreamCreateWithFlags(&H.h2d, hipStreamNonBlocking));
        }
        for (int s = 0; s < NS; ++s) {
            if (!H.copied[s]) ASR_HIP(ctx, hipEventCreateWithFlags(&H.copied[s], hipEventDisableTiming));
            if (!H.consumed[s]) ASR_HIP(ctx, hipEventCreateWithFlags(&H.consumed[s], hipEventDisableTiming));
        }
        H.granule = granule;
    }
    const bool staged = H.staged;
    const int G = H.granule;
    // a job's largest granule: G samples, or what 16 MiB hold when samples are small (spectrograms: 1000)
    auto granule_of = [&](size_t bps) { return std::min(ctx->chunk, std::max(G, (int)((16u << 20) / bps))); };
    size_t need = 0;
    for (int j = 0; j < njobs; ++j)
        if (jobs[j].n > 0) {
            const size_t bps = input_bytes_per_sample(ctx, jobs[j].view, jobs[j].in_mode);
            need = std::max(need, (size_t)std::min<int64_t>(granule_of(bps), jobs[j].n) * bps);
        }
    if (H.slot_bytes < need) {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
        ASR_HIP(ctx, hipStreamSynchronize(H.h2d));
        const size_t sz = std::max(need, (size_t)G * std::min<size_t>(max_bps, 1 << 16));      // (room for the usual sizes at once)
        for (int s = 0; s < NS; ++s) {
            if (H.pin[s]) { ASR_HIP(ctx, hipHostFree(H.pin[s])); H.pin[s] = nullptr; }
            if (H.dev[s]) { ASR_HIP(ctx, hipFree(H.dev[s])); H.dev[s] = nullptr; }
            H.used[s] = false;
        }
        H.slot_bytes = 0;
        for (int s = 0; s < NS; ++s) {
            if (staged) ASR_HIP(ctx, hipHostMalloc(&H.pin[s], sz, hipHostMallocDefault));      // (page-locked slots only when used)
            ASR_HIP(ctx, hipMalloc(&H.dev[s], sz));
        }
        H.slot_bytes = sz;
    }
    if (H.out_floats < (size_t)total * 32) {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
        if (H.out_dev) { ASR_HIP(ctx, hipFree(H.out_dev)); H.out_dev = nullptr; H.out_floats = 0; }
        const size_t fl = std::max((size_t)total * 32, (size_t)ctx->chunk * 32);
        ASR_HIP(ctx, hipMalloc((void **)&H.out_dev, fl * sizeof(float)));
        H.out_floats = fl;
    }
    if (loss && ctx->valid_ws_floats < 64) {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
        if (ctx->valid_ws) { ASR_HIP(ctx, hipFree(ctx->valid_ws)); ctx->valid_ws = nullptr; ctx->valid_ws_floats = 0; }
        ASR_HIP(ctx, hipMalloc((void **)&ctx->valid_ws, 64 * sizeof(float)));
        ctx->valid_ws_floats = 64;
    }
    // results of an earlier "_dev" call may still be read by the main stream
    for (int v = 0; v < 2; ++v)
        if (ctx->main_pending) ASR_HIP(ctx, hipStreamWaitEvent(ctx->estream[v], ctx->main_done, 0));
    int64_t out_row = 0;
    int slot = 0;
    for (int j = 0; j < njobs; ++j) {
        const HostJob &J = jobs[j];
        if (J.n == 0) continue;
        const size_t bps = input_bytes_per_sample(ctx, J.view, J.in_mode);
        const bool direct = !staged || host_pointer_is_pinned(J.x);
        hipStream_t st = ctx->estream[J.view - 1];
        // the first granule's copy is exposed (nothing to overlap it with): start small, double up to G
        // (at least ~4 MiB: a 125-sample granule of spectrograms is 1.9 MB and nine tiny kernels)
        const int Gj = granule_of(bps);
        int g_now = std::min(Gj, std::max(H.granule_first, (int)((4u << 20) / bps)));
        for (int64_t s0 = 0; s0 < J.n;) {
            const int nc = (int)std::min<int64_t>(g_now, J.n - s0);
            g_now = std::min(Gj, g_now * 2);
            const int s = slot;
            slot = (slot + 1) % NS;
            const char *src = (const char *)J.x + (size_t)s0 * bps;
            const size_t bytes = (size_t)nc * bps;
            if (H.used[s]) ASR_HIP(ctx, hipStreamWaitEvent(H.h2d, H.consumed[s], 0));     // dev[s] has been read
            if (!direct) {
                if (H.used[s]) ASR_HIP(ctx, hipEventSynchronize(H.copied[s]));            // pin[s] is free
                H.pool->run(H.pin[s], src, bytes);
                src = (const char *)H.pin[s];
            }
            ASR_HIP(ctx, hipMemcpyAsync(H.dev[s], src, bytes, hipMemcpyHostToDevice, H.h2d));
            ASR_HIP(ctx, hipEventRecord(H.copied[s], H.h2d));
            H.used[s] = true;
            ASR_HIP(ctx, hipStreamWaitEvent(st, H.copied[s], 0));
            float *o = H.out_dev + (size_t)(out_row + s0) * 32;
            int rc = run_tower(ctx, J.view, H.dev[s], J.in_mode, nc, J.out_kind == ASR_OUT_FEATURES ? o : nullptr,
                               J.out_kind == ASR_OUT_LATENT ? o : nullptr);
            if (rc != ASR_OK) { (void)sync_all(ctx); (void)hipStreamSynchronize(H.h2d); return rc; }
            ASR_HIP(ctx, hipEventRecord(H.consumed[s], st));
            s0 += nc;
        }
        out_row += J.n;
    }
    if (loss) {      // enqueued before the copy-outs, which may block the host
        const int64_t n = jobs[0].n;
        hipError_t e = hipSuccess;
        for (int v = 0; v < 2 && e == hipSuccess; ++v) {
            e = hipEventRecord(ctx->vdone[v], ctx->estream[v]);
            if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->vdone[v], 0);
        }
        if (e == hipSuccess)
            e = asr::launch_rank_loss(ctx->stream, H.out_dev, H.out_dev + (size_t)n * 32, (int)n, ctx->cfg.gamma,
                                      ctx->valid_ws, ctx->loss_weight, ctx->loss_symmetric);
        if (e != hipSuccess) {
            (void)sync_all(ctx);
            (void)hipStreamSynchronize(H.h2d);
            return fail(ctx, ASR_ERR_HIP, "valid_output: %s", hipGetErrorString(e));
        }
    }
    // copy-outs last: into pageable memory they block the host until the job's tower is through
    out_row = 0;
    for (int j = 0; j < njobs; ++j) {
        const HostJob &J = jobs[j];
        if (J.n == 0) continue;
        if (J.out)
            ASR_HIP(ctx, hipMemcpyAsync(J.out, H.out_dev + (size_t)out_row * 32, (size_t)J.n * 32 * sizeof(float),
                                        hipMemcpyDeviceToHost, ctx->estream[J.view - 1]));
        out_row += J.n;
    }
    if (loss) ASR_HIP(ctx, hipMemcpyAsync(loss, ctx->valid_ws, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(H.h2d));
    return sync_all(ctx);
}

int ensure_norms(asr_ctx *ctx, int64_t n1, int64_t n2) {
    if (n1 > ctx->norm_cap1) {
        if (ctx->norm1) hipFree(ctx->norm1);
        ctx->norm1 = nullptr; ctx->norm_cap1 = 0;
        ASR_HIP(ctx, hipMalloc((void **)&ctx->norm1, (size_t)n1 * sizeof(double)));
        ctx->norm_cap1 = n1;
    }
    if (n2 > ctx->norm_cap2) {
        if (ctx->norm2) hipFree(ctx->norm2);
        ctx->norm2 = nullptr; ctx->norm_cap2 = 0;
        ASR_HIP(ctx, hipMalloc((void **)&ctx->norm2, (size_t)n2 * sizeof(double)));
        ctx->norm_cap2 = n2;
    }
    return ASR_OK;
}

int rank_check(asr_ctx *ctx, int64_t n1, int64_t ld1, int64_t n2, int64_t ld2, int dim, int64_t query_offset,
               int64_t n1_global) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n1 < 0 || n2 < 0 || dim < 1 || dim > 64 || ld1 < dim || ld2 < dim || query_offset < 0 ||
        n1_global < query_offset + n1)
        return fail(ctx, ASR_ERR_INVALID, "rank: bad sizes n1=%lld n2=%lld dim=%d ld=(%lld,%lld) off=%lld n1g=%lld",
                    (long long)n1, (long long)n2, dim, (long long)ld1, (long long)ld2, (long long)query_offset,
                    (long long)n1_global);
    if (n1 > 0 && n2 == 0) return fail(ctx, ASR_ERR_INVALID, "rank: empty candidate list");
    return ASR_OK;
}

}  // namespace asr_detail


extern "C" {

const char *asr_last_error(const asr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int asr_create(const asr_config *cfg, asr_ctx **out) {
    if (!out) return fail(nullptr, ASR_ERR_INVALID, "asr_create: out is NULL");
    *out = nullptr;
    int rc = check_cfg(cfg);
    if (rc != ASR_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, ASR_ERR_HIP, "asr_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, ASR_ERR_INVALID, "asr_create: device %d out of range (%d devices)", cfg->device, ndev);
    std::unique_ptr<asr_ctx> ctx(new asr_ctx());
    // the 64-byte struct of the first ABI has no pool_ties member: read only what the caller owns
    ctx->cfg = asr_config{};
    memcpy(&ctx->cfg, cfg, (size_t)cfg->struct_size);
    ctx->cfg.struct_size = (int32_t)sizeof(asr_config);
    asr_ctx *c = ctx.get();
#define CREATE_HIP(call)                                                                                   \
    do {                                                                                                   \
        hipError_t e__ = (call);                                                                           \
        if (e__ != hipSuccess) {                                                                           \
            free_ctx_buffers(c);                                                                           \
            return fail(nullptr, ASR_ERR_HIP, "asr_create: %s failed: %s", #call, hipGetErrorString(e__)); \
        }                                                                                                  \
    } while (0)
    CREATE_HIP(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    CREATE_HIP(hipGetDeviceProperties(&prop, cfg->device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    CREATE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    // Both towers on one stream by default: the persistent conv kernels fill the chip on their own, every kernel's
    // measured duration is its own (bench.py's roofline, rocprofv3), and letting the towers overlap on two streams
    // (ASR_TWO_STREAMS=1) buys under 3 % of throughput
    {
        const char *two = getenv("ASR_TWO_STREAMS");
        c->single_stream = !(two && two[0] == '1') || getenv("ASR_SINGLE_STREAM") != nullptr;
    }
    for (int v = 0; v < 2; ++v) {
        CREATE_HIP(hipStreamCreateWithFlags(&c->vstream[v], hipStreamNonBlocking));
        c->estream[v] = c->single_stream ? c->stream : c->vstream[v];
        CREATE_HIP(hipEventCreateWithFlags(&c->vdone[v], hipEventDisableTiming));
    }
    // (see asr_ctx.h; ASR_EARLY_WSIDE=0: created in asr_train_begin as in rounds 3-5, for A/B runs)
    if (!(getenv("ASR_EARLY_WSIDE") && getenv("ASR_EARLY_WSIDE")[0] == '0'))
        CREATE_HIP(hipStreamCreateWithFlags(&c->wside_stream, hipStreamNonBlocking));
    if (!(getenv("ASR_EARLY_COPY") && getenv("ASR_EARLY_COPY")[0] == '0') && c->wside_stream)     // (see asr_ctx.h)
        for (hipStream_t &cs : c->copy_streams) CREATE_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    CREATE_HIP(hipEventCreateWithFlags(&c->main_done, hipEventDisableTiming));
    c->chunk = cfg->max_chunk > 0 ? cfg->max_chunk : 1000;

    const int nf = cfg->num_filters;
    const int H1 = cfg->resize_view1 ? cfg->h1 / 2 : cfg->h1, W1 = cfg->resize_view1 ? cfg->w1 / 2 : cfg->w1;
    build_geometry(c->tw[0], nf, H1, W1);
    build_geometry(c->tw[1], nf, cfg->h2, cfg->w2);

    // parameter table in the reference's order
    for (int t = 0; t < 2; ++t)
        for (int b = 0; b < 9; ++b) {
            const LayerGeom &g = c->tw[t].g[b];
            c->pshape.push_back({g.cout, g.cin, g.k, g.k});
            for (int q = 0; q < 4; ++q) c->pshape.push_back({g.cout});
        }
    c->pshape.push_back({32, 32}); c->pshape.push_back({32, 32});
    c->pshape.push_back({32}); c->pshape.push_back({32});
    c->pshape.push_back({32, 32}); c->pshape.push_back({32, 32}); c->pshape.push_back({32, 32});
    for (auto &s : c->pshape) {
        int64_t n = 1;
        for (auto d : s) n *= d;
        c->params.emplace_back((size_t)n, 0.0f);
    }

    for (int t = 0; t < 2; ++t) {
        Tower &tw = c->tw[t];
        for (int b = 0; b < 9; ++b) {
            const LayerGeom &g = tw.g[b];
            size_t wfl;
            if (b == 0) wfl = (size_t)g.cout * 9;
            else if (b < 8) wfl = asr::conv_wpack_floats(g.cin, g.cout) + asr::wino_wpack_floats(g.cin, g.cout) +
                                  asr::wino4_wpack_floats(g.cin, g.cout);
            else wfl = (size_t)32 * g.cin;
            CREATE_HIP(hipMalloc((void **)&tw.w_dev[b], wfl * sizeof(float)));
            const int coutp = (g.cout + 15) / 16 * 16;
            CREATE_HIP(hipMalloc((void **)&tw.bn_dev[b], (size_t)3 * coutp * sizeof(float)));
        }
        int rcp = plan_tower(nullptr, tw, t + 1);
        if (rcp != ASR_OK) { free_ctx_buffers(c); return rcp; }
    }
    CREATE_HIP(hipMalloc((void **)&c->cca_dev, (size_t)(2048 + 64) * sizeof(float)));
    CREATE_HIP(hipMemsetAsync(c->cca_dev, 0, (size_t)(2048 + 64) * sizeof(float), c->stream));
    c->in_stage_bytes = (size_t)c->chunk * std::max((size_t)cfg->h1 * cfg->w1, (size_t)cfg->h2 * cfg->w2) * 4;
    CREATE_HIP(hipStreamSynchronize(c->stream));
#undef CREATE_HIP
    *out = ctx.release();
    return ASR_OK;
}

void asr_destroy(asr_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->cfg.device);
    for (int v = 0; v < 2; ++v)
        if (ctx->vstream[v]) hipStreamSynchronize(ctx->vstream[v]);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    free_ctx_buffers(ctx);
    delete ctx;
}

int asr_sync(asr_ctx *ctx) {
    if (!ctx) return ASR_ERR_INVALID;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    return sync_all(ctx);
}

int asr_set_input_size(asr_ctx *ctx, int view, int h, int w) {
    if (!ctx || view < 1 || view > 2) return ASR_ERR_INVALID;
    if (h < 16 || w < 16 || h > 4096 || w > 4096)
        return fail(ctx, ASR_ERR_INVALID, "set_input_size: %dx%d out of range", h, w);
    asr_config &c = ctx->cfg;
    if (view == 1 && c.h1 == h && c.w1 == w) return ASR_OK;
    if (view == 2 && c.h2 == h && c.w2 == w) return ASR_OK;
    if (ctx->train)       // the training buffers and plans were sized for the current geometry
        return fail(ctx, ASR_ERR_STATE, "set_input_size: a training state is active (sized for %dx%d / %dx%d); call "
                                        "asr_train_end first", c.h1, c.w1, c.h2, c.w2);
    ASR_HIP(ctx, hipSetDevice(c.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    Tower saved = ctx->tw[view - 1];
    Tower &tw = ctx->tw[view - 1];
    const int nh = (view == 1 && c.resize_view1) ? h / 2 : h, nw = (view == 1 && c.resize_view1) ? w / 2 : w;
    build_geometry(tw, c.num_filters, nh, nw);
    int rc = plan_tower(ctx, tw, view);
    if (rc != ASR_OK) { ctx->tw[view - 1] = saved; return rc; }
    for (int b = 0; b < 8; ++b) {       // activation buffers are re-allocated lazily at the new size
        if (tw.act[b]) ASR_HIP(ctx, hipFree(tw.act[b]));
        tw.act[b] = nullptr;
    }
    tw.tuned = false;
    if (view == 1) { c.h1 = h; c.w1 = w; } else { c.h2 = h; c.w2 = w; }
    for (int v = 0; v < 2; ++v)
        if (ctx->in_stage[v]) { ASR_HIP(ctx, hipFree(ctx->in_stage[v])); ctx->in_stage[v] = nullptr; }
    ctx->in_stage_bytes = (size_t)ctx->chunk * std::max((size_t)c.h1 * c.w1, (size_t)c.h2 * c.w2) * 4;
    ctx->last_n[view - 1] = 0;
    return ASR_OK;
}

int asr_param_count(const asr_ctx *ctx) { return ctx ? (int)ctx->params.size() : -1; }

int asr_param_size(const asr_ctx *ctx, int index, int64_t *n_elements) {
    if (!ctx || !n_elements || index < 0 || index >= (int)ctx->params.size()) return ASR_ERR_INVALID;
    *n_elements = (int64_t)ctx->params[index].size();
    return ASR_OK;
}

static int upload_network(asr_ctx *ctx) {
    for (int t = 0; t < 2; ++t) {
        Tower &tw = ctx->tw[t];
        for (int b = 0; b < 9; ++b) {
            const LayerGeom &g = tw.g[b];
            const int base = 45 * t + 5 * b;
            const std::vector<float> &W = ctx->params[base];
            const float *beta = ctx->params[base + 1].data(), *gamma = ctx->params[base + 2].data();
            const float *mean = ctx->params[base + 3].data(), *istd = ctx->params[base + 4].data();
            std::vector<float> wdev;
            if (b == 0) {              // [co][9] correlation-form taps: W[co][0][2-a][2-b]
                wdev.resize((size_t)g.cout * 9);
                for (int co = 0; co < g.cout; ++co)
                    for (int a = 0; a < 3; ++a)
                        for (int bb = 0; bb < 3; ++bb)
                            wdev[(size_t)co * 9 + a * 3 + bb] = W[((size_t)co * 1 + 0) * 9 + (2 - a) * 3 + (2 - bb)];
            } else if (b < 8) {        // [tap][ci][co] correlation form -> MFMA fragment order
                std::vector<float> wc((size_t)9 * g.cin * g.cout);
                for (int co = 0; co < g.cout; ++co)
                    for (int ci = 0; ci < g.cin; ++ci)
                        for (int a = 0; a < 3; ++a)
                            for (int bb = 0; bb < 3; ++bb)
                                wc[((size_t)(a * 3 + bb) * g.cin + ci) * g.cout + co] =
                                    W[((size_t)co * g.cin + ci) * 9 + (2 - a) * 3 + (2 - bb)];
                wdev.resize(asr::conv_wpack_floats(g.cin, g.cout));
                asr::pack_conv_weights(wc.data(), g.cin, g.cout, wdev.data());
            } else {                   // 1x1: [o][c]
                wdev.assign(W.begin(), W.end());
            }
            ASR_HIP(ctx, hipMemcpyAsync(tw.w_dev[b], wdev.data(), wdev.size() * sizeof(float), hipMemcpyHostToDevice,
                                        ctx->stream));
            if (b >= 1 && b < 8) {     // Winograd-domain weights behind the direct-form fragments, transformed on the device
                float *raw = nullptr;
                ASR_HIP(ctx, hipMalloc((void **)&raw, W.size() * sizeof(float)));
                hipError_t e1 = hipMemcpyAsync(raw, W.data(), W.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
                if (e1 == hipSuccess)
                    e1 = asr::launch_wino_pack(ctx->stream, raw, g.cin, g.cout, tw.w_dev[b] + wdev.size());
                if (e1 == hipSuccess)
                    e1 = asr::launch_wino4_pack(ctx->stream, raw, g.cin, g.cout,
                                                tw.w_dev[b] + wdev.size() + asr::wino_wpack_floats(g.cin, g.cout));
                if (e1 == hipSuccess) e1 = hipStreamSynchronize(ctx->stream);
                (void)hipFree(raw);
                ASR_HIP(ctx, e1);
            }
            const int coutp = (g.cout + 15) / 16 * 16;
            std::vector<float> bn((size_t)3 * coutp, 0.0f);
            for (int co = 0; co < g.cout; ++co) {
                bn[co] = mean[co];
                bn[coutp + co] = gamma[co] * istd[co];   // fp32 product, as (gamma * inv_std) in the reference
                bn[2 * coutp + co] = beta[co];
            }
            ASR_HIP(ctx, hipMemcpyAsync(tw.bn_dev[b], bn.data(), bn.size() * sizeof(float), hipMemcpyHostToDevice,
                                        ctx->stream));
            ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // staging vectors die at scope end
        }
    }
    std::vector<float> cca(2048 + 64);
    memcpy(cca.data(), ctx->params[90].data(), 1024 * sizeof(float));
    memcpy(cca.data() + 1024, ctx->params[91].data(), 1024 * sizeof(float));
    memcpy(cca.data() + 2048, ctx->params[92].data(), 32 * sizeof(float));
    memcpy(cca.data() + 2080, ctx->params[93].data(), 32 * sizeof(float));
    ASR_HIP(ctx, hipMemcpyAsync(ctx->cca_dev, cca.data(), cca.size() * sizeof(float), hipMemcpyHostToDevice,
                                ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_OK;
}

int asr_set_params(asr_ctx *ctx, const float *const *arrays, const int64_t *sizes, int n_arrays) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!arrays || !sizes || n_arrays != (int)ctx->params.size())
        return fail(ctx, ASR_ERR_INVALID, "set_params: expected %d arrays, got %d", (int)ctx->params.size(), n_arrays);
    for (int i = 0; i < n_arrays; ++i)
        if (!arrays[i] || sizes[i] != (int64_t)ctx->params[i].size())
            return fail(ctx, ASR_ERR_INVALID, "set_params: array %d has %lld elements, expected %lld", i,
                        (long long)sizes[i], (long long)ctx->params[i].size());
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);      // towers in flight still read the old weights
        if (rcs != ASR_OK) return rcs;
    }
    for (int i = 0; i < n_arrays; ++i) memcpy(ctx->params[i].data(), arrays[i], (size_t)sizes[i] * sizeof(float));
    int rc = upload_network(ctx);
    if (rc == ASR_OK) ctx->params_set = true;
    if (rc == ASR_OK && ctx->train) rc = train_upload_master(ctx);
    return rc;
}

int asr_get_params(asr_ctx *ctx, float *const *arrays, const int64_t *sizes, int n_arrays) {
    if (!ctx) return ASR_ERR_INVALID;
    if (ctx->train && ctx->train->master_dirty) {
        int rcd = train_download_master(ctx);
        if (rcd != ASR_OK) return rcd;
    }
    if (!arrays || !sizes || n_arrays != (int)ctx->params.size())
        return fail(ctx, ASR_ERR_INVALID, "get_params: expected %d arrays, got %d", (int)ctx->params.size(), n_arrays);
    for (int i = 0; i < n_arrays; ++i) {
        if (!arrays[i] || sizes[i] != (int64_t)ctx->params[i].size())
            return fail(ctx, ASR_ERR_INVALID, "get_params: array %d has %lld elements, expected %lld", i,
                        (long long)sizes[i], (long long)ctx->params[i].size());
        memcpy(arrays[i], ctx->params[i].data(), (size_t)sizes[i] * sizeof(float));
    }
    return ASR_OK;
}

int asr_set_cca(asr_ctx *ctx, const float *U, const float *V, const float *mean1, const float *mean2) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!U || !V || !mean1 || !mean2) return fail(ctx, ASR_ERR_INVALID, "set_cca: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    // training moved the device master: the host mirror train_upload_master() rebuilds it from must be current
    if (ctx->train && ctx->train->master_dirty) {
        int rcd = train_download_master(ctx);
        if (rcd != ASR_OK) return rcd;
    }
    memcpy(ctx->params[90].data(), U, 1024 * sizeof(float));
    memcpy(ctx->params[91].data(), V, 1024 * sizeof(float));
    memcpy(ctx->params[92].data(), mean1, 32 * sizeof(float));
    memcpy(ctx->params[93].data(), mean2, 32 * sizeof(float));
    std::vector<float> cca(2048 + 64);
    memcpy(cca.data(), U, 1024 * sizeof(float));
    memcpy(cca.data() + 1024, V, 1024 * sizeof(float));
    memcpy(cca.data() + 2048, mean1, 32 * sizeof(float));
    memcpy(cca.data() + 2080, mean2, 32 * sizeof(float));
    ASR_HIP(ctx, hipMemcpyAsync(ctx->cca_dev, cca.data(), cca.size() * sizeof(float), hipMemcpyHostToDevice,
                                ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->train) return train_upload_master(ctx);
    return ASR_OK;
}

// ASR_HOST_PIPE=0: the round-2 form (one synchronous copy-in / tower / copy-out per chunk), kept for A/B timing
static bool host_pipe_off() {
    static const bool off = getenv("ASR_HOST_PIPE") && getenv("ASR_HOST_PIPE")[0] == '0';
    return off;
}
int asr_embed_view1(asr_ctx *ctx, const void *x, int in_mode, int64_t n, int out_kind, float *out) {
    if (host_pipe_off()) return embed_common(ctx, 1, x, in_mode, n, out_kind, out, false);
    const HostJob job{1, x, in_mode, n, out_kind, out};
    return embed_host(ctx, &job, 1);
}
int asr_embed_view2(asr_ctx *ctx, const float *z, int64_t n, int out_kind, float *out) {
    if (host_pipe_off()) return embed_common(ctx, 2, z, ASR_IN_F32_PREPARED, n, out_kind, out, false);
    const HostJob job{2, z, ASR_IN_F32_PREPARED, n, out_kind, out};
    return embed_host(ctx, &job, 1);
}
int asr_embed_both(asr_ctx *ctx, const void *x, int in_mode, const float *z, int64_t n, int out_kind, float *out1,
                   float *out2) {
    if (host_pipe_off()) {
        int rc = embed_common(ctx, 1, x, in_mode, n, out_kind, out1, false);
        if (rc != ASR_OK) return rc;
        return embed_common(ctx, 2, z, ASR_IN_F32_PREPARED, n, out_kind, out2, false);
    }
    // one pass of the pipeline over both views: no host synchronisation between the towers
    const HostJob jobs[2] = {{1, x, in_mode, n, out_kind, out1}, {2, z, ASR_IN_F32_PREPARED, n, out_kind, out2}};
    return embed_host(ctx, jobs, 2);
}
int asr_embed_view1_dev(asr_ctx *ctx, const void *x_dev, int in_mode, int64_t n, int out_kind, float *out_dev) {
    return embed_common(ctx, 1, x_dev, in_mode, n, out_kind, out_dev, true);
}
int asr_embed_view2_dev(asr_ctx *ctx, const float *z_dev, int64_t n, int out_kind, float *out_dev) {
    return embed_common(ctx, 2, z_dev, ASR_IN_F32_PREPARED, n, out_kind, out_dev, true);
}

int asr_cca_fit_dev(asr_ctx *ctx, const float *H1_dev, const float *H2_dev, int64_t n, float *U_dev, float *V_dev,
                    float *means_dev, double *coeffs_dev) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n < 2) return fail(ctx, ASR_ERR_INVALID, "cca_fit: needs at least 2 samples, got %lld", (long long)n);
    if (!H1_dev || !H2_dev || !U_dev || !V_dev || !means_dev || !coeffs_dev)
        return fail(ctx, ASR_ERR_INVALID, "cca_fit: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t need = asr::cca_workspace_bytes(n);
    if (need > ctx->cca_ws_bytes) {
        if (ctx->cca_ws) ASR_HIP(ctx, hipFree(ctx->cca_ws));
        ctx->cca_ws = nullptr; ctx->cca_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->cca_ws, need));
        ctx->cca_ws_bytes = need;
    }
    {
        int rcj = join_views(ctx);
        if (rcj != ASR_OK) return rcj;
    }
    {
        ProfScope ps(ctx, "cca_fit", 0, 6.0 * 32 * 32 * (double)n, 2.0 * 256.0 * (double)n);
        ASR_HIP(ctx, asr::launch_cca_fit(ctx->stream, H1_dev, H2_dev, n, ctx->cfg.r1, ctx->cfg.r2, ctx->cca_ws,
                                         U_dev, V_dev, means_dev, coeffs_dev));
    }
    return mark_main(ctx);
}

int asr_cca_fit(asr_ctx *ctx, const float *H1, const float *H2, int64_t n, float *U, float *V, float *mean1,
                float *mean2, double *coeffs) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n < 2) return fail(ctx, ASR_ERR_INVALID, "cca_fit: needs at least 2 samples, got %lld", (long long)n);
    if (!H1 || !H2 || !U || !V || !mean1 || !mean2) return fail(ctx, ASR_ERR_INVALID, "cca_fit: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float *d = nullptr;       // H1 | H2 | U | V | means ; then coeffs (double)
    double *dc = nullptr;
    const size_t hf = (size_t)n * 32;
    auto cleanup = [&]() { (void)hipFree(d); (void)hipFree(dc); };
#define CCA_HIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess) {                                                                       \
            cleanup();                                                                                 \
            return fail(ctx, ASR_ERR_HIP, "asr_cca_fit: %s failed: %s", #call, hipGetErrorString(e__)); \
        }                                                                                              \
    } while (0)
    CCA_HIP(hipMalloc((void **)&d, (2 * hf + 2048 + 64) * sizeof(float)));
    CCA_HIP(hipMalloc((void **)&dc, 32 * sizeof(double)));
    CCA_HIP(hipMemcpyAsync(d, H1, hf * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    CCA_HIP(hipMemcpyAsync(d + hf, H2, hf * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    int rc = asr_cca_fit_dev(ctx, d, d + hf, n, d + 2 * hf, d + 2 * hf + 1024, d + 2 * hf + 2048, dc);
    if (rc != ASR_OK) { cleanup(); return rc; }
    CCA_HIP(hipMemcpyAsync(U, d + 2 * hf, 1024 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CCA_HIP(hipMemcpyAsync(V, d + 2 * hf + 1024, 1024 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CCA_HIP(hipMemcpyAsync(mean1, d + 2 * hf + 2048, 32 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CCA_HIP(hipMemcpyAsync(mean2, d + 2 * hf + 2080, 32 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (coeffs) CCA_HIP(hipMemcpyAsync(coeffs, dc, 32 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CCA_HIP(hipStreamSynchronize(ctx->stream));
#undef CCA_HIP
    cleanup();
    return ASR_OK;
}

/* ---- host-buffer pipeline ---------------------------------------------------------------------------------- */
int asr_host_alloc(asr_ctx *ctx, size_t bytes, void **hptr) {
    if (!ctx || !hptr) return ASR_ERR_INVALID;
    *hptr = nullptr;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipError_t e = hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_NOMEM, "host_alloc(%zu): %s", bytes, hipGetErrorString(e));
    return ASR_OK;
}
int asr_host_free(asr_ctx *ctx, void *hptr) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!hptr) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    ASR_HIP(ctx, hipHostFree(hptr));
    return ASR_OK;
}

int asr_eval_batches(asr_ctx *ctx, const void *const *x, int in_mode, const float *const *z, int n_batches, int64_t n,
                     int32_t *const *ranks, double *const *dstar, int32_t *const *ties, float *const *lv1,
                     float *const *lv2) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!ctx->params_set) return fail(ctx, ASR_ERR_STATE, "eval_batches: asr_set_params has not been called");
    if (n_batches < 0 || n < 1 || n > (1 << 24) || in_mode < 0 || in_mode > 2)
        return fail(ctx, ASR_ERR_INVALID, "eval_batches: bad sizes (n_batches %d, n %lld, in_mode %d)", n_batches,
                    (long long)n, in_mode);
    if (n_batches == 0) return ASR_OK;
    if (!x || !z || !ranks) return fail(ctx, ASR_ERR_INVALID, "eval_batches: NULL argument");
    for (int k = 0; k < n_batches; ++k)
        if (!x[k] || !z[k] || !ranks[k]) return fail(ctx, ASR_ERR_INVALID, "eval_batches: batch %d has a NULL buffer", k);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    auto &P = ctx->pipe;
    const size_t b1 = (size_t)n * input_bytes_per_sample(ctx, 1, in_mode), b2 = (size_t)n * input_bytes_per_sample(ctx, 2, 0);
    if (P.n != n || P.b1 < b1 || P.b2 < b2) {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
        free_pipe(ctx);
        if (ctx->copy_streams[0] && ctx->copy_streams[1]) {
            P.h2d = ctx->copy_streams[0]; P.d2h = ctx->copy_streams[1];
        } else {
            // ASR_EARLY_COPY=0: created here, as in rounds 2-5.  ASR_COPY_STEER=n (probe): n throw-away streams are created
            // first and destroyed afterwards, which moves the two copy streams n places along the runtime's least-used-queue
            // order - n = 3 behind a fresh context's four streams is the layout that costs 22 % (asr_ctx.h)
            const int steer = getenv("ASR_COPY_STEER") ? std::max(0, std::min(8, atoi(getenv("ASR_COPY_STEER")))) : 0;
            hipStream_t dummy[8] = {};
            for (int i = 0; i < steer; ++i) (void)hipStreamCreateWithFlags(&dummy[i], hipStreamNonBlocking);
            hipError_t e1 = hipStreamCreateWithFlags(&P.h2d, hipStreamNonBlocking);
            hipError_t e2 = hipStreamCreateWithFlags(&P.d2h, hipStreamNonBlocking);
            for (int i = 0; i < steer; ++i) if (dummy[i]) (void)hipStreamDestroy(dummy[i]);
            ASR_HIP(ctx, e1);
            ASR_HIP(ctx, e2);
        }
        for (int s = 0; s < 2; ++s) {
            ASR_HIP(ctx, hipMalloc(&P.in1[s], b1));
            ASR_HIP(ctx, hipMalloc((void **)&P.in2[s], b2));
            ASR_HIP(ctx, hipMalloc((void **)&P.lv1[s], (size_t)n * 32 * sizeof(float)));
            ASR_HIP(ctx, hipMalloc((void **)&P.lv2[s], (size_t)n * 32 * sizeof(float)));
            ASR_HIP(ctx, hipMalloc((void **)&P.ranks[s], (size_t)n * sizeof(int32_t)));
            ASR_HIP(ctx, hipMalloc((void **)&P.ties[s], (size_t)n * sizeof(int32_t)));
            ASR_HIP(ctx, hipMalloc((void **)&P.dstar[s], (size_t)n * sizeof(double)));
            ASR_HIP(ctx, hipEventCreateWithFlags(&P.ready[s], hipEventDisableTiming));
            ASR_HIP(ctx, hipEventCreateWithFlags(&P.done[s], hipEventDisableTiming));
            ASR_HIP(ctx, hipEventCreateWithFlags(&P.out[s], hipEventDisableTiming));
        }
        P.n = n; P.b1 = b1; P.b2 = b2;
    }
    // the pipeline starts from an idle context: whatever the compute streams still hold is older than batch 0
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    auto upload = [&](int k) -> int {
        const int s = k & 1;
        if (k >= 2) ASR_HIP(ctx, hipStreamWaitEvent(P.h2d, P.done[s], 0));          // batch k-2 has read in[s]
        ASR_HIP(ctx, hipMemcpyAsync(P.in1[s], x[k], b1, hipMemcpyHostToDevice, P.h2d));
        ASR_HIP(ctx, hipMemcpyAsync(P.in2[s], z[k], b2, hipMemcpyHostToDevice, P.h2d));
        ASR_HIP(ctx, hipEventRecord(P.ready[s], P.h2d));
        return ASR_OK;
    };
    // every exit after the first enqueued copy drains the copy streams: asynchronous copies into or out of the caller's
    // host buffers must not be in flight when the caller gets control back (and frees them)
    auto run = [&]() -> int {
        int rc = upload(0);
        if (rc != ASR_OK) return rc;
        for (int k = 0; k < n_batches; ++k) {
            const int s = k & 1;
            if (k + 1 < n_batches && (rc = upload(k + 1)) != ASR_OK) return rc;      // overlaps the compute of batch k
            for (int v = 0; v < 2; ++v) {
                ASR_HIP(ctx, hipStreamWaitEvent(ctx->estream[v], P.ready[s], 0));
                if (k >= 2) ASR_HIP(ctx, hipStreamWaitEvent(ctx->estream[v], P.out[s], 0));   // outputs of k-2 are on the host
            }
            if ((rc = embed_common(ctx, 1, P.in1[s], in_mode, n, ASR_OUT_LATENT, P.lv1[s], true)) != ASR_OK) return rc;
            if ((rc = embed_common(ctx, 2, P.in2[s], ASR_IN_F32_PREPARED, n, ASR_OUT_LATENT, P.lv2[s], true)) != ASR_OK) return rc;
            if (k >= 2) ASR_HIP(ctx, hipStreamWaitEvent(ctx->stream, P.out[s], 0));
            if ((rc = asr_rank_dev(ctx, P.lv1[s], n, 32, P.lv2[s], n, 32, 32, 0, n, P.ranks[s], P.dstar[s], P.ties[s])) != ASR_OK)
                return rc;
            ASR_HIP(ctx, hipEventRecord(P.done[s], ctx->stream));
            ASR_HIP(ctx, hipStreamWaitEvent(P.d2h, P.done[s], 0));
            ASR_HIP(ctx, hipMemcpyAsync(ranks[k], P.ranks[s], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, P.d2h));
            if (dstar && dstar[k])
                ASR_HIP(ctx, hipMemcpyAsync(dstar[k], P.dstar[s], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, P.d2h));
            if (ties && ties[k])
                ASR_HIP(ctx, hipMemcpyAsync(ties[k], P.ties[s], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, P.d2h));
            if (lv1 && lv1[k])
                ASR_HIP(ctx, hipMemcpyAsync(lv1[k], P.lv1[s], (size_t)n * 32 * sizeof(float), hipMemcpyDeviceToHost, P.d2h));
            if (lv2 && lv2[k])
                ASR_HIP(ctx, hipMemcpyAsync(lv2[k], P.lv2[s], (size_t)n * 32 * sizeof(float), hipMemcpyDeviceToHost, P.d2h));
            ASR_HIP(ctx, hipEventRecord(P.out[s], P.d2h));
        }
        return ASR_OK;
    };
    const int rc = run();
    const std::string first_error = rc != ASR_OK ? ctx->err : std::string();
    const hipError_t e1 = hipStreamSynchronize(P.h2d), e2 = hipStreamSynchronize(P.d2h);
    const int rcs = sync_all(ctx);
    if (rc != ASR_OK) { ctx->err = first_error; return rc; }
    if (e1 != hipSuccess || e2 != hipSuccess)
        return fail(ctx, ASR_ERR_HIP, "eval_batches: copy stream failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return rcs;
}

int asr_dev_alloc(asr_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return ASR_ERR_INVALID;
    *dptr = nullptr;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_NOMEM, "dev_alloc(%zu): %s", bytes, hipGetErrorString(e));
    return ASR_OK;
}
int asr_dev_free(asr_ctx *ctx, void *dptr) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!dptr) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    ASR_HIP(ctx, hipFree(dptr));
    return ASR_OK;
}
int asr_dev_upload(asr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!ctx || (bytes && (!dst_dev || !src_host))) return ASR_ERR_INVALID;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    ASR_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_OK;
}
int asr_dev_download(asr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx || (bytes && (!dst_host || !src_dev))) return ASR_ERR_INVALID;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    ASR_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_OK;
}

int asr_profile_enable(asr_ctx *ctx, int on) {
    if (!ctx) return ASR_ERR_INVALID;
    ctx->profiling = on != 0;
    return ASR_OK;
}
int asr_profile_filter(asr_ctx *ctx, const char *symbol) {
    if (!ctx) return ASR_ERR_INVALID;
    ctx->prof_filter = symbol ? symbol : "";
    return ASR_OK;
}
int asr_profile_reset(asr_ctx *ctx) {
    if (!ctx) return ASR_ERR_INVALID;
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    for (auto &r : ctx->prof) prof_fold(r.get());
    ctx->prof.clear();
    return ASR_OK;
}
int asr_profile_count(asr_ctx *ctx) { return ctx ? (int)ctx->prof.size() : -1; }
int asr_profile_get(asr_ctx *ctx, int index, char *name, int name_cap, int64_t *launches, double *total_ms,
                    double *flops, double *bytes) {
    if (!ctx || index < 0 || index >= (int)ctx->prof.size()) return ASR_ERR_INVALID;
    ProfRec *r = ctx->prof[index].get();
    prof_fold(r);
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", r->name.c_str());
    if (launches) *launches = r->launches;
    if (total_ms) *total_ms = r->total_ms;
    if (flops) *flops = r->flops;
    if (bytes) *bytes = r->bytes;
    return ASR_OK;
}

int asr_profile_symbol(asr_ctx *ctx, int index, char *symbol, int symbol_cap) {
    if (!ctx || index < 0 || index >= (int)ctx->prof.size() || !symbol || symbol_cap < 1) return ASR_ERR_INVALID;
    snprintf(symbol, (size_t)symbol_cap, "%s", ctx->prof[index]->symbol.c_str());
    return ASR_OK;
}

int asr_debug_activation(asr_ctx *ctx, int view, int block, int64_t n, float *out, int *h, int *w, int *c) {
    if (!ctx || view < 1 || view > 2 || block < 0 || block > 7) return ASR_ERR_INVALID;
    const Tower &t = ctx->tw[view - 1];
    const LayerGeom &g = t.g[block];
    if (h) *h = g.OH;
    if (w) *w = g.OW;
    if (c) *c = g.cout;
    if (!out) return ASR_OK;
    if (block == 0 && t.fuse1)
        return fail(ctx, ASR_ERR_STATE, "debug_activation: block 1 is fused into block 2 and never materialised; "
                                        "create the context with ASR_NO_FUSE1=1 to inspect it");
    if (n < 0 || n > ctx->last_n[view - 1] || !t.act[block])
        return fail(ctx, ASR_ERR_INVALID, "debug_activation: n=%lld but the last chunk held %d samples", (long long)n,
                    ctx->last_n[view - 1]);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
    }
    ASR_HIP(ctx, hipMemcpyAsync(out, t.act[block], (size_t)n * t.act_floats[block] * sizeof(float),
                                hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_OK;
}

}  // extern "C"
