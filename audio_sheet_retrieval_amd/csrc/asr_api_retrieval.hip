// C-ABI layer, retrieval side: eval_retrieval ranks, top-k, the resident code data base and its shard pieces, window
// slicing, DTW alignment, the audio front-end, window gathering, the piece vote (include/asr_hip.h for the contract and
// the reference interfaces each entry point replaces).  Context and shared helpers: asr_ctx.h.
#include "asr_ctx.h"

// workspace of one chunk of asr_dtw_batch_dev: byte offsets into ctx->dtw_ws (256-byte aligned sections)
namespace {
struct DtwChunk {
    int p0 = 0, n = 0;                                    // pairs [p0, p0 + n)
    int64_t cells = 0, diags = 0, paths = 0, rows_a = 0, rows_b = 0, ring = 0;
    int lds_slots = 0;
    bool any_ring = false;
    size_t o_pairs = 0, o_cost = 0, o_rm = 0, o_dir = 0, o_ring = 0, o_md = 0, o_len = 0, o_pa = 0, o_pb = 0, o_fa = 0,
           o_fb = 0, bytes = 0;
};

size_t dtw_align(size_t x) { return (x + 255) & ~(size_t)255; }

// section layout of a chunk; `wave`: accumulated cost + traceback are needed (not only the distances)
void dtw_layout(DtwChunk &c, bool wave, bool rm, bool fa, bool fb) {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += dtw_align(bytes); return at; };
    c.o_pairs = take((size_t)c.n * sizeof(asr::DtwPair));
    c.o_cost = take((size_t)c.cells * sizeof(double));
    c.o_rm = rm ? take((size_t)c.cells * sizeof(double)) : 0;
    if (wave) {
        c.o_dir = take((size_t)c.cells);
        c.o_ring = take((size_t)c.ring * sizeof(double));
        c.o_md = take((size_t)c.n * sizeof(double));
        c.o_len = take((size_t)c.n * sizeof(int32_t));
        c.o_pa = take((size_t)c.paths * sizeof(int32_t));
        c.o_pb = take((size_t)c.paths * sizeof(int32_t));
        c.o_fa = fa ? take((size_t)c.rows_a * sizeof(int32_t)) : 0;
        c.o_fb = fb ? take((size_t)c.rows_b * sizeof(int32_t)) : 0;
    }
    c.bytes = o;
}

int64_t dtw_env(const char *name, int64_t dflt) {
    const char *v = getenv(name);
    return v && *v ? atoll(v) : dflt;
}
}  // namespace

extern "C" {

int asr_rank_dev(asr_ctx *ctx, const float *lv1, int64_t n1, int64_t ld1, const float *lv2, int64_t n2, int64_t ld2,
                 int dim, int64_t query_offset, int64_t n1_global, int32_t *ranks, double *dstar, int32_t *ties) {
    int rc = rank_check(ctx, n1, ld1, n2, ld2, dim, query_offset, n1_global);
    if (rc != ASR_OK) return rc;
    if (n1 == 0) return ASR_OK;
    if (!lv1 || !lv2) return fail(ctx, ASR_ERR_INVALID, "rank: NULL embeddings");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = ensure_norms(ctx, n1, n2);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // utils/train_dcca_pool.py:35-36 (py2 integer division)
    const int64_t k = n2 > n1_global ? n2 / n1_global : 1;
    const int64_t h = n1_global > n2 ? n1_global / n2 : 1;
    if ((query_offset + n1 - 1) / h * k >= n2)
        return fail(ctx, ASR_ERR_INVALID, "rank: query %lld has no correct candidate (n2=%lld)",
                    (long long)(query_offset + n1 - 1), (long long)n2);
    {
        ProfScope ps(ctx, "row_norms", 0, 2.0 * dim * (double)(n1 + n2), 4.0 * dim * (double)(n1 + n2));
        ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, lv1, n1, ld1, dim, ctx->norm1));
        ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, lv2, n2, ld2, dim, ctx->norm2));
    }
    {
        ProfScope ps(ctx, "rank", 0, 2.0 * dim * (double)n1 * (double)n2, 4.0 * dim * (double)(n1 + n2));
        const size_t need = asr::rank_workspace_bytes(n1, n2);           // shares the top-k scratch buffer
        if (need > ctx->topk_ws_bytes) {
            if (ctx->topk_ws) ASR_HIP(ctx, hipFree(ctx->topk_ws));
            ctx->topk_ws = nullptr; ctx->topk_ws_bytes = 0;
            ASR_HIP(ctx, hipMalloc(&ctx->topk_ws, need));
            ctx->topk_ws_bytes = need;
        }
        ASR_HIP(ctx, asr::launch_rank(ctx->stream, lv1, ctx->norm1, n1, ld1, lv2, ctx->norm2, n2, ld2, dim,
                                      query_offset, k, h, ranks, dstar, ties, ctx->topk_ws));
    }
    return mark_main(ctx);
}

int asr_rank(asr_ctx *ctx, const float *lv1, int64_t n1, int64_t ld1, const float *lv2, int64_t n2, int64_t ld2,
             int dim, int64_t query_offset, int64_t n1_global, int32_t *ranks, double *dstar, int32_t *ties) {
    int rc = rank_check(ctx, n1, ld1, n2, ld2, dim, query_offset, n1_global);
    if (rc != ASR_OK) return rc;
    if (n1 == 0) return ASR_OK;
    if (!lv1 || !lv2) return fail(ctx, ASR_ERR_INVALID, "rank: NULL embeddings");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    // one growable device scratch for the host-buffer variant (five hipMalloc / hipFree pairs per call were half of
    // eval_retrieval's 0.33 ms at n = 2000)
    const size_t b1 = ((size_t)n1 * ld1 * sizeof(float) + 255) & ~(size_t)255, b2 = ((size_t)n2 * ld2 * sizeof(float) + 255) & ~(size_t)255;
    const size_t bd = ((size_t)n1 * sizeof(double) + 255) & ~(size_t)255, bi = ((size_t)n1 * sizeof(int32_t) + 255) & ~(size_t)255;
    const size_t need = b1 + b2 + bd + 2 * bi;
    if (need > ctx->rank_io_bytes) {
        int rcs = sync_all(ctx);
        if (rcs != ASR_OK) return rcs;
        if (ctx->rank_io) ASR_HIP(ctx, hipFree(ctx->rank_io));
        ctx->rank_io = nullptr; ctx->rank_io_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->rank_io, need));
        ctx->rank_io_bytes = need;
    }
    char *base = (char *)ctx->rank_io;
    float *d1 = (float *)base, *d2 = (float *)(base + b1);
    double *dd = (double *)(base + b1 + b2);
    int32_t *dr = (int32_t *)(base + b1 + b2 + bd), *dt = (int32_t *)(base + b1 + b2 + bd + bi);
#define RANK_HIP(call)                                                                                  \
    do {                                                                                                \
        hipError_t e__ = (call);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            (void)hipStreamSynchronize(ctx->stream);                                                    \
            return fail(ctx, ASR_ERR_HIP, "asr_rank: %s failed: %s", #call, hipGetErrorString(e__));    \
        }                                                                                               \
    } while (0)
    RANK_HIP(hipMemcpyAsync(d1, lv1, (size_t)n1 * ld1 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RANK_HIP(hipMemcpyAsync(d2, lv2, (size_t)n2 * ld2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = asr_rank_dev(ctx, d1, n1, ld1, d2, n2, ld2, dim, query_offset, n1_global, dr, dd, dt);
    if (rc != ASR_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if (ranks) RANK_HIP(hipMemcpyAsync(ranks, dr, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (dstar) RANK_HIP(hipMemcpyAsync(dstar, dd, (size_t)n1 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (ties) RANK_HIP(hipMemcpyAsync(ties, dt, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    RANK_HIP(hipStreamSynchronize(ctx->stream));
#undef RANK_HIP
    return ASR_OK;
}

static int ensure_topk_tickets(asr_ctx *ctx);

int asr_topk_dev(asr_ctx *ctx, const float *db, int64_t n_db, int64_t ld_db, const float *q, int64_t n_q, int64_t ld_q,
                 int dim, int k, int64_t idx_offset, int32_t *idx, double *dist) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_db < 0 || n_q < 0 || dim < 1 || dim > 64 || ld_db < dim || ld_q < dim || k < 1 || k > 128)
        return fail(ctx, ASR_ERR_INVALID, "topk: bad sizes n_db=%lld n_q=%lld dim=%d k=%d (k <= 128)", (long long)n_db,
                    (long long)n_q, dim, k);
    if (n_q == 0) return ASR_OK;
    if (!q || !idx || !dist || (n_db > 0 && !db)) return fail(ctx, ASR_ERR_INVALID, "topk: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_norms(ctx, n_q, n_db > 0 ? n_db : 1);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // A large pool of packed 32-d rows is searched the way a resident data base is (asr_db_*): one pass derives the
    // float64 norms - which this call needs anyway - AND the unit-length copy the filter reads (0.02 ms at 250 k rows,
    // 0.1 ms at 2 M), and the seeded, one-compare-per-four-distances filter does the rest: 1024 queries x 250 k codes
    // 0.97 -> 0.55 ms, 64 x 2 M 0.72 -> 0.40 against the filter on raw rows.  A caller that keeps its pool creates an
    // asr_db and skips the pass.
    const bool as_db = dim == 32 && ld_db == 32 && ld_q == 32 && n_db >= 16384 && (reinterpret_cast<uintptr_t>(db) & 15) == 0 &&
                       !(getenv("ASR_TOPK_UNIT") && getenv("ASR_TOPK_UNIT")[0] == '0');
    float *unit = nullptr, *rn = nullptr;
    if (as_db) {
        const size_t n_pad = (size_t)((n_db + 3) & ~(int64_t)3), need_f = (size_t)n_db * 32 + n_pad;
        if (need_f > ctx->unit_ws_floats) {
            rc = sync_all(ctx);
            if (rc != ASR_OK) return rc;
            if (ctx->unit_ws) ASR_HIP(ctx, hipFree(ctx->unit_ws));
            ctx->unit_ws = nullptr; ctx->unit_ws_floats = 0;
            ASR_HIP(ctx, hipMalloc((void **)&ctx->unit_ws, need_f * sizeof(float)));
            ctx->unit_ws_floats = need_f;
        }
        unit = ctx->unit_ws;
        rn = ctx->unit_ws + (size_t)n_db * 32;
    }
    {
        ProfScope ps(ctx, "row_norms", 0, 2.0 * dim * (double)(n_q + n_db), (as_db ? 8.0 : 4.0) * dim * (double)(n_q + n_db));
        ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, q, n_q, ld_q, dim, ctx->norm1));
        if (as_db) ASR_HIP(ctx, asr::launch_db_prepare(ctx->stream, db, n_db, ctx->norm2, rn, unit));
        else ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, db, n_db, ld_db, dim, ctx->norm2));
    }
    {
        ProfScope ps(ctx, "topk", 0, 2.0 * dim * (double)n_q * (double)n_db, 4.0 * dim * (double)n_db * (double)n_q);
        const size_t need = asr::topk_workspace_bytes(n_db, n_q, k, as_db, false);
        if (need > ctx->topk_ws_bytes) {
            if (ctx->topk_ws) ASR_HIP(ctx, hipFree(ctx->topk_ws));
            ctx->topk_ws = nullptr; ctx->topk_ws_bytes = 0;
            ASR_HIP(ctx, hipMalloc(&ctx->topk_ws, need));
            ctx->topk_ws_bytes = need;
        }
        int rc2 = ensure_topk_tickets(ctx);                    // (the state block of the sort-free exact refine)
        if (rc2 != ASR_OK) return rc2;
        ASR_HIP(ctx, asr::launch_topk(ctx->stream, db, ctx->norm2, n_db, ld_db, q, ctx->norm1, n_q, ld_q, dim, k,
                                      idx_offset, idx, dist, ctx->topk_ws, unit, rn, nullptr, ctx->topk_tickets));
    }
    return mark_main(ctx);
}

// ---- resident code data base (audio_sheet_server.py:496-522: the server loads its code data base once and queries it
// per frame, :530-563) -------------------------------------------------------------------------------------------------
struct asr_db {
    asr_ctx *owner = nullptr;
    const float *codes = nullptr;       // caller-owned device rows (n, ld)
    int64_t n = 0, ld = 0;
    int dim = 0;
    double *norms = nullptr;            // float64 row norms
    float *rn = nullptr;                // fp32 reciprocal norms, zero padded to a multiple of 4
    float *unit = nullptr;              // unit-length copy (32-d packed rows only)
};

static int ensure_topk_tickets(asr_ctx *ctx) {
    if (ctx->topk_tickets) return ASR_OK;
    // [0, 1024): last-arriver tickets (ASR_TOPK_FOLD); [1024, 3072): survivor counts and scan flags of the sort-free refine
    ASR_HIP(ctx, hipMalloc((void **)&ctx->topk_tickets, 4096 * sizeof(unsigned)));
    ASR_HIP(ctx, hipMemsetAsync(ctx->topk_tickets, 0, 4096 * sizeof(unsigned), ctx->stream));
    return ASR_OK;
}

static int grow_topk_ws(asr_ctx *ctx, size_t need) {
    if (need > ctx->topk_ws_bytes) {
        int rc = sync_all(ctx);                      // an earlier launch may still read the old buffer
        if (rc != ASR_OK) return rc;
        if (ctx->topk_ws) ASR_HIP(ctx, hipFree(ctx->topk_ws));
        ctx->topk_ws = nullptr; ctx->topk_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->topk_ws, need));
        ctx->topk_ws_bytes = need;
    }
    return ASR_OK;
}

static int db_check(asr_ctx *ctx, const asr_db *db, const char *who) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!db || db->owner != ctx) return fail(ctx, ASR_ERR_INVALID, "%s: not a data base of this context", who);
    return ASR_OK;
}

int asr_db_refresh(asr_ctx *ctx, asr_db *db) {
    int rc = db_check(ctx, db, "db_refresh");
    if (rc != ASR_OK) return rc;
    if (db->n == 0) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    ProfScope ps(ctx, "db_prepare", 0, 2.0 * db->dim * (double)db->n, (db->unit ? 8.0 : 4.0) * db->dim * (double)db->n);
    if (db->unit)
        ASR_HIP(ctx, asr::launch_db_prepare(ctx->stream, db->codes, db->n, db->norms, db->rn, db->unit));
    else
        ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, db->codes, db->n, db->ld, db->dim, db->norms));
    return mark_main(ctx);
}

int asr_db_create(asr_ctx *ctx, const float *codes_dev, int64_t n, int64_t ld, int dim, asr_db **out) {
    if (!ctx) return ASR_ERR_INVALID;
    if (!out) return fail(ctx, ASR_ERR_INVALID, "db_create: NULL output");
    *out = nullptr;
    if (n < 0 || dim < 1 || dim > 64 || ld < dim || (n > 0 && !codes_dev))
        return fail(ctx, ASR_ERR_INVALID, "db_create: bad sizes n=%lld ld=%lld dim=%d", (long long)n, (long long)ld, dim);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    std::unique_ptr<asr_db> db(new asr_db());
    db->owner = ctx; db->codes = codes_dev; db->n = n; db->ld = ld; db->dim = dim;
    const bool packed32 = dim == 32 && ld == 32 && (reinterpret_cast<uintptr_t>(codes_dev) & 15) == 0;
    const size_t n_pad = (size_t)((n + 3) & ~(int64_t)3);
    hipError_t e = hipMalloc((void **)&db->norms, std::max<size_t>(1, (size_t)n) * sizeof(double));
    if (e == hipSuccess && packed32) e = hipMalloc((void **)&db->rn, std::max<size_t>(4, n_pad) * sizeof(float));
    if (e == hipSuccess && packed32) e = hipMalloc((void **)&db->unit, std::max<size_t>(1, (size_t)n) * 32 * sizeof(float));
    if (e != hipSuccess) {
        if (db->norms) hipFree(db->norms);
        if (db->rn) hipFree(db->rn);
        if (db->unit) hipFree(db->unit);
        return fail(ctx, ASR_ERR_HIP, "db_create: %s", hipGetErrorString(e));
    }
    int rc = asr_db_refresh(ctx, db.get());
    if (rc != ASR_OK) {
        hipFree(db->norms);
        if (db->rn) hipFree(db->rn);
        if (db->unit) hipFree(db->unit);
        return rc;
    }
    *out = db.release();
    return ASR_OK;
}

int asr_db_destroy(asr_ctx *ctx, asr_db *db) {
    if (!db) return ASR_OK;
    int rc = db_check(ctx, db, "db_destroy");
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = sync_all(ctx);
    if (db->norms) hipFree(db->norms);
    if (db->rn) hipFree(db->rn);
    if (db->unit) hipFree(db->unit);
    db->owner = nullptr;
    delete db;
    return rc;
}

int asr_db_size(asr_ctx *ctx, const asr_db *db, int64_t *n, int *dim) {
    int rc = db_check(ctx, db, "db_size");
    if (rc != ASR_OK) return rc;
    if (n) *n = db->n;
    if (dim) *dim = db->dim;
    return ASR_OK;
}

// shared front of the three query entry points: argument checks, the queries' norms
// norms_later: the caller's launcher computes the query norms itself (asr::launch_topk, norm_q_pending)
static int db_query_begin(asr_ctx *ctx, const asr_db *db, const float *q, int64_t n_q, int64_t ld_q, const char *who,
                          bool norms_later = false) {
    int rc = db_check(ctx, db, who);
    if (rc != ASR_OK) return rc;
    if (n_q < 0 || ld_q < db->dim) return fail(ctx, ASR_ERR_INVALID, "%s: bad sizes n_q=%lld ld_q=%lld", who, (long long)n_q, (long long)ld_q);
    if (n_q == 0) return ASR_OK;
    if (!q) return fail(ctx, ASR_ERR_INVALID, "%s: NULL queries", who);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = ensure_norms(ctx, n_q, 1);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (norms_later) return ASR_OK;
    ProfScope ps(ctx, "row_norms", 0, 2.0 * db->dim * (double)n_q, 4.0 * db->dim * (double)n_q);
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, q, n_q, ld_q, db->dim, ctx->norm1));
    return ASR_OK;
}

// global indices are returned as int32: offset + row must stay below 2^31
static int db_offset_fits(asr_ctx *ctx, const asr_db *db, int64_t offset, const char *what) {
    if (offset < 0 || offset + db->n > (int64_t)INT32_MAX)
        return fail(ctx, ASR_ERR_INVALID, "%s: index offset %lld + %lld rows does not fit the int32 indices returned", what,
                    (long long)offset, (long long)db->n);
    return ASR_OK;
}

int asr_topk_db_dev(asr_ctx *ctx, const asr_db *db, const float *q, int64_t n_q, int64_t ld_q, int k, int64_t idx_offset,
                    int32_t *idx, double *dist) {
    int rc = db_query_begin(ctx, db, q, n_q, ld_q, "topk_db", true);
    if (rc != ASR_OK || n_q == 0) return rc;
    if (k < 1 || k > 128 || !idx || !dist) return fail(ctx, ASR_ERR_INVALID, "topk_db: k=%d (1..128) / NULL output", k);
    if ((rc = db_offset_fits(ctx, db, idx_offset, "topk_db")) != ASR_OK) return rc;
    ProfScope ps(ctx, "topk", 0, 2.0 * db->dim * (double)n_q * (double)db->n, 4.0 * db->dim * (double)db->n);
    rc = grow_topk_ws(ctx, asr::topk_workspace_bytes(db->n, n_q, k, db->unit != nullptr, false));
    if (rc != ASR_OK) return rc;
    if ((rc = ensure_topk_tickets(ctx)) != ASR_OK) return rc;
    // (the query norms are formed inside the call: by the seeding kernel where that path runs)
    ASR_HIP(ctx, asr::launch_topk(ctx->stream, db->codes, db->norms, db->n, db->ld, q, ctx->norm1, n_q, ld_q, db->dim, k,
                                  idx_offset, idx, dist, ctx->topk_ws, db->unit, db->rn, ctx->norm1, ctx->topk_tickets));
    return mark_main(ctx);
}

static int db_rank_geometry(asr_ctx *ctx, const asr_db *db, int64_t n1, int64_t query_offset, int64_t n1_global,
                            int64_t *k, int64_t *h) {
    if (n1_global < 1 || query_offset < 0 || query_offset + n1 > n1_global)
        return fail(ctx, ASR_ERR_INVALID, "rank_db: queries [%lld, %lld) outside the %lld of the job", (long long)query_offset,
                    (long long)(query_offset + n1), (long long)n1_global);
    *k = db->n > n1_global ? db->n / n1_global : 1;            // utils/train_dcca_pool.py:35-36 (py2 integer division)
    *h = n1_global > db->n ? n1_global / db->n : 1;
    if (db->n < 1 || (query_offset + n1 - 1) / *h * *k >= db->n)
        return fail(ctx, ASR_ERR_INVALID, "rank_db: query %lld has no correct candidate (n2=%lld)",
                    (long long)(query_offset + n1 - 1), (long long)db->n);
    return ASR_OK;
}

int asr_rank_db_dev(asr_ctx *ctx, const asr_db *db, const float *lv1, int64_t n1, int64_t ld1, int64_t query_offset,
                    int64_t n1_global, int32_t *ranks, double *dstar, int32_t *ties) {
    int rc = db_query_begin(ctx, db, lv1, n1, ld1, "rank_db");
    if (rc != ASR_OK || n1 == 0) return rc;
    if (!ranks || !dstar || !ties) return fail(ctx, ASR_ERR_INVALID, "rank_db: NULL output");
    int64_t k, h;
    if ((rc = db_rank_geometry(ctx, db, n1, query_offset, n1_global, &k, &h)) != ASR_OK) return rc;
    ProfScope ps(ctx, "rank", 0, 2.0 * db->dim * (double)n1 * (double)db->n, 4.0 * db->dim * (double)(n1 + db->n));
    rc = grow_topk_ws(ctx, asr::rank_workspace_bytes(n1, db->n));
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, asr::launch_rank(ctx->stream, lv1, ctx->norm1, n1, ld1, db->codes, db->norms, db->n, db->ld, db->dim,
                                  query_offset, k, h, ranks, dstar, ties, ctx->topk_ws, db->rn));
    return mark_main(ctx);
}

int asr_topk_rank_db_dev(asr_ctx *ctx, const asr_db *db, const float *q, int64_t n_q, int64_t ld_q, int k,
                         int64_t idx_offset, int32_t *idx, double *dist, int64_t query_offset, int64_t n1_global,
                         int32_t *ranks, double *dstar, int32_t *ties) {
    int rc = db_query_begin(ctx, db, q, n_q, ld_q, "topk_rank_db");
    if (rc != ASR_OK || n_q == 0) return rc;
    if (k < 1 || k > 128 || !idx || !dist || !ranks || !dstar || !ties)
        return fail(ctx, ASR_ERR_INVALID, "topk_rank_db: k=%d (1..128) / NULL output", k);
    if ((rc = db_offset_fits(ctx, db, idx_offset, "topk_rank_db")) != ASR_OK) return rc;
    int64_t kk, hh;
    if ((rc = db_rank_geometry(ctx, db, n_q, query_offset, n1_global, &kk, &hh)) != ASR_OK) return rc;
    if (db->unit && ld_q == 32 && asr::topk_rank_fusable(db->n, kk)) {
        // one walk over the pool's item tiles feeds the top-k candidate buffers and the rank counters
        ProfScope ps(ctx, "topk_rank", 0, 2.0 * 32 * (double)n_q * (double)db->n, 128.0 * (double)db->n);
        rc = grow_topk_ws(ctx, asr::topk_workspace_bytes(db->n, n_q, k, true, true));
        if (rc != ASR_OK) return rc;
        ASR_HIP(ctx, asr::launch_topk_rank_db(ctx->stream, db->codes, db->unit, db->norms, db->n, q, ctx->norm1, n_q, k,
                                              idx_offset, idx, dist, query_offset, kk, hh, ranks, dstar, ties,
                                              ctx->topk_ws));
        return mark_main(ctx);
    }
    {
        ProfScope ps(ctx, "topk", 0, 2.0 * db->dim * (double)n_q * (double)db->n, 4.0 * db->dim * (double)db->n);
        rc = grow_topk_ws(ctx, asr::topk_workspace_bytes(db->n, n_q, k, db->unit != nullptr, false));
        if (rc != ASR_OK) return rc;
        if ((rc = ensure_topk_tickets(ctx)) != ASR_OK) return rc;
        ASR_HIP(ctx, asr::launch_topk(ctx->stream, db->codes, db->norms, db->n, db->ld, q, ctx->norm1, n_q, ld_q, db->dim,
                                      k, idx_offset, idx, dist, ctx->topk_ws, db->unit, db->rn, nullptr, ctx->topk_tickets));
    }
    {
        ProfScope ps(ctx, "rank", 0, 2.0 * db->dim * (double)n_q * (double)db->n, 4.0 * db->dim * (double)(n_q + db->n));
        rc = grow_topk_ws(ctx, asr::rank_workspace_bytes(n_q, db->n));
        if (rc != ASR_OK) return rc;
        ASR_HIP(ctx, asr::launch_rank(ctx->stream, q, ctx->norm1, n_q, ld_q, db->codes, db->norms, db->n, db->ld, db->dim,
                                      query_offset, kk, hh, ranks, dstar, ties, ctx->topk_ws, db->rn));
    }
    return mark_main(ctx);
}

// ---- a data base that is one SHARD of a larger pool: what each rank of a query-sharded retrieval computes ------------
int asr_rank_dstar_db_dev(asr_ctx *ctx, const asr_db *db, const float *q, int64_t n_q, int64_t ld_q, int64_t item_offset,
                          int64_t n2_global, int64_t query_offset, int64_t n1_global, double *dstar, int64_t *jstar) {
    int rc = db_query_begin(ctx, db, q, n_q, ld_q, "rank_dstar_db");
    if (rc != ASR_OK || n_q == 0) return rc;
    if (db->dim != 32 || db->ld != 32 || ld_q != 32) return fail(ctx, ASR_ERR_INVALID, "rank_dstar_db: 32-d packed rows only");
    if (!dstar || !jstar || n1_global < 1 || n2_global < db->n + item_offset || item_offset < 0 || query_offset < 0 ||
        query_offset + n_q > n1_global)
        return fail(ctx, ASR_ERR_INVALID, "rank_dstar_db: bad geometry");
    const int64_t kk = n2_global > n1_global ? n2_global / n1_global : 1, hh = n1_global > n2_global ? n1_global / n2_global : 1;
    const int64_t first = (query_offset / hh) * kk, last = ((query_offset + n_q - 1) / hh) * kk + kk;
    if (first < item_offset || std::min(last, n2_global) > item_offset + db->n)
        return fail(ctx, ASR_ERR_INVALID, "rank_dstar_db: the correct candidates [%lld, %lld) of these queries are not all in "
                    "this shard [%lld, %lld)", (long long)first, (long long)last, (long long)item_offset,
                    (long long)(item_offset + db->n));
    ProfScope ps(ctx, "rank_dstar", 0, 64.0 * (double)n_q * (double)kk, 128.0 * (double)n_q * (double)kk);
    ASR_HIP(ctx, asr::launch_rank_dstar(ctx->stream, q, ctx->norm1, n_q, db->codes, db->norms, db->n, item_offset, n2_global,
                                        query_offset, kk, hh, dstar, jstar));
    return mark_main(ctx);
}

int asr_topk_count_db_dev(asr_ctx *ctx, const asr_db *db, const float *q, int64_t n_q, int64_t ld_q, int k,
                          int64_t item_offset, int32_t *idx, double *dist, const double *dstar, const int64_t *jstar,
                          int32_t *counts) {
    int rc = db_query_begin(ctx, db, q, n_q, ld_q, "topk_count_db");
    if (rc != ASR_OK || n_q == 0) return rc;
    if (k < 1 || k > 128 || !idx || !dist || !dstar || !jstar || !counts)
        return fail(ctx, ASR_ERR_INVALID, "topk_count_db: k=%d (1..128) / NULL argument", k);
    if (!db->unit || ld_q != 32 || db->n < 16384)
        return fail(ctx, ASR_ERR_INVALID, "topk_count_db: needs a data base of >= 16384 packed 32-d rows");
    if ((rc = db_offset_fits(ctx, db, item_offset, "topk_count_db")) != ASR_OK) return rc;
    ProfScope ps(ctx, "topk_count", 0, 2.0 * 32 * (double)n_q * (double)db->n, 128.0 * (double)db->n);
    rc = grow_topk_ws(ctx, asr::topk_workspace_bytes(db->n, n_q, k, true, true));
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, asr::launch_topk_count_db(ctx->stream, db->codes, db->unit, db->norms, db->n, q, ctx->norm1, n_q, k,
                                           item_offset, idx, dist, dstar, jstar, counts, ctx->topk_ws));
    return mark_main(ctx);
}

int asr_topk_merge_dev(asr_ctx *ctx, const int32_t *part_idx, const double *part_dist, int n_parts, int64_t n_q_total,
                       int64_t q_lo, int64_t n_q, int k, int32_t *idx, double *dist) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_q == 0) return ASR_OK;
    if (!part_idx || !part_dist || !idx || !dist || n_parts < 1 || k < 1 || (int64_t)n_parts * k > 2048 || q_lo < 0 ||
        q_lo + n_q > n_q_total)
        return fail(ctx, ASR_ERR_INVALID, "topk_merge: %d lists of %d keys (product <= 2048), queries [%lld, %lld) of %lld",
                    n_parts, k, (long long)q_lo, (long long)(q_lo + n_q), (long long)n_q_total);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, asr::launch_topk_merge(ctx->stream, part_idx, part_dist, n_parts, n_q_total, q_lo, n_q, k, idx, dist));
    return mark_main(ctx);
}

int asr_rank_finish_dev(asr_ctx *ctx, const int32_t *counts, const double *dstar, int64_t n, int32_t *ranks,
                        double *dstar_out, int32_t *ties) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n == 0) return ASR_OK;
    if (!counts || !dstar) return fail(ctx, ASR_ERR_INVALID, "rank_finish: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    ASR_HIP(ctx, asr::launch_rank_finish(ctx->stream, counts, dstar, n, ranks, dstar_out, ties));
    return mark_main(ctx);
}

int asr_slice_windows_dev(asr_ctx *ctx, const float *src_dev, int64_t rows, int64_t T, int r0, int win_h, int win_w,
                          const int32_t *starts, int n, float *out_dev) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n < 0 || win_h < 1 || win_w < 1 || r0 < 0 || r0 + win_h > rows || win_w > T)
        return fail(ctx, ASR_ERR_INVALID, "slice_windows: window %dx%d at row %d does not fit %lld x %lld", win_h, win_w,
                    r0, (long long)rows, (long long)T);
    if (n == 0) return ASR_OK;
    if (!src_dev || !starts || !out_dev) return fail(ctx, ASR_ERR_INVALID, "slice_windows: NULL argument");
    for (int i = 0; i < n; ++i)
        if (starts[i] < 0 || starts[i] + win_w > T)
            return fail(ctx, ASR_ERR_INVALID, "slice_windows: start %d = %d outside [0, %lld]", i, starts[i],
                        (long long)(T - win_w));
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int32_t *d_starts = nullptr;
    ASR_HIP(ctx, hipMalloc((void **)&d_starts, (size_t)n * sizeof(int32_t)));
    hipError_t e = hipMemcpyAsync(d_starts, starts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = asr::launch_slice_windows(ctx->stream, src_dev, T, r0, win_h, win_w, d_starts, n, out_dev);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_starts);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "slice_windows: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_dtw_dev(asr_ctx *ctx, const float *a_dev, int64_t n_a, const float *b_dev, int64_t n_b, int dim, double *dists,
                int32_t *path_a, int32_t *path_b, int32_t *path_len, double *min_dist) {
    if (!ctx || !path_a || !path_b || !path_len) return ASR_ERR_INVALID;
    if (n_a < 1 || n_b < 1 || dim < 1 || dim > 64 || n_a > 100000 || n_b > 100000 || (n_a + 1) * (n_b + 1) > (1ll << 31))
        return fail(ctx, ASR_ERR_INVALID, "dtw: bad sizes n_a=%lld n_b=%lld dim=%d", (long long)n_a, (long long)n_b, dim);
    if (!a_dev || !b_dev) return fail(ctx, ASR_ERR_INVALID, "dtw: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_norms(ctx, n_a, n_b);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    const size_t cells = (size_t)(n_a + 1) * (n_b + 1);
    double *D = nullptr, *dout = nullptr;
    int32_t *pbuf = nullptr;
    auto cleanup = [&]() { (void)hipFree(D); (void)hipFree(dout); (void)hipFree(pbuf); };
    hipError_t e = hipMalloc((void **)&D, (cells + 1) * sizeof(double));
    if (e == hipSuccess && dists) e = hipMalloc((void **)&dout, (size_t)n_a * n_b * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&pbuf, (size_t)(2 * (n_a + n_b) + 1) * sizeof(int32_t));
    int32_t *pi = pbuf, *pj = pbuf ? pbuf + (n_a + n_b) : nullptr, *plen = pbuf ? pbuf + 2 * (n_a + n_b) : nullptr;
    if (e == hipSuccess) {
        ProfScope ps(ctx, "dtw", 0, 2.0 * dim * (double)n_a * (double)n_b, 8.0 * (double)cells);
        e = asr::launch_row_norms(ctx->stream, a_dev, n_a, dim, dim, ctx->norm1);
        if (e == hipSuccess) e = asr::launch_row_norms(ctx->stream, b_dev, n_b, dim, dim, ctx->norm2);
        if (e == hipSuccess)
            e = asr::launch_dtw(ctx->stream, a_dev, ctx->norm1, n_a, dim, b_dev, ctx->norm2, n_b, dim, dim, D, dout, pi, pj,
                                plen, D + cells);
    }
    int32_t len = 0;
    double md = 0.0;
    if (e == hipSuccess) e = hipMemcpyAsync(&len, plen, sizeof len, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&md, D + cells, sizeof md, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && dists)
        e = hipMemcpyAsync(dists, dout, (size_t)n_a * n_b * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && len > 0) {
        std::vector<int32_t> ri(len), rj(len);
        e = hipMemcpy(ri.data(), pi, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(rj.data(), pj, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost);
        for (int32_t k = 0; k < len && e == hipSuccess; ++k) {      // the kernel walks from the end to the origin
            path_a[k] = ri[len - 1 - k];
            path_b[k] = rj[len - 1 - k];
        }
    }
    cleanup();
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "dtw: %s", hipGetErrorString(e));
    *path_len = len;
    if (min_dist) *min_dist = md;
    return mark_main(ctx);
}

int asr_dtw_batch_dev(asr_ctx *ctx, const float *a_dev, const float *b_dev, const int64_t *n_a, const int64_t *n_b,
                      int n_pairs, int dim, double *min_dist, int32_t *path_len, int32_t *path_a, int32_t *path_b,
                      double *dists, int32_t *first_a, int32_t *first_b) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pairs < 0 || dim < 1 || dim > 64)
        return fail(ctx, ASR_ERR_INVALID, "dtw_batch: bad sizes n_pairs=%d dim=%d (1..64)", n_pairs, dim);
    if (n_pairs == 0) return ASR_OK;
    if (!a_dev || !b_dev || !n_a || !n_b) return fail(ctx, ASR_ERR_INVALID, "dtw_batch: NULL argument");
    if ((path_a != nullptr) != (path_b != nullptr) || (path_a && !path_len))
        return fail(ctx, ASR_ERR_INVALID, "dtw_batch: path_a, path_b and path_len go together");
    int64_t tot_a = 0, tot_b = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (n_a[p] < 1 || n_b[p] < 1 || n_a[p] > 100000 || n_b[p] > 100000 || (n_a[p] + 1) * (n_b[p] + 1) > (1ll << 31))
            return fail(ctx, ASR_ERR_INVALID, "dtw_batch: pair %d has bad sizes n_a=%lld n_b=%lld", p, (long long)n_a[p],
                        (long long)n_b[p]);
        tot_a += n_a[p];
        tot_b += n_b[p];
    }
    const bool wave = min_dist || path_len || path_a || first_a || first_b;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_norms(ctx, tot_a, tot_b);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // ASR_DTW_LDS_CAP=<slots>: pairs with min(n_a, n_b) + 1 above it take the global-ring wavefront (a debug switch
    // that exercises the large-pair path at small sizes); ASR_DTW_BUDGET_MB: device workspace per chunk of pairs
    const int lds_cap = (int)std::min<int64_t>(asr::dtw_batch_lds_slots(ctx->cfg.device), dtw_env("ASR_DTW_LDS_CAP", 1 << 30));
    const size_t budget = (size_t)std::max<int64_t>(dtw_env("ASR_DTW_BUDGET_MB", 4096), 1) << 20;

    // chunks of consecutive pairs whose workspace fits the budget (a pair larger than it gets a chunk of its own)
    std::vector<DtwChunk> chunks;
    DtwChunk c;
    for (int p = 0; p < n_pairs; ++p) {
        DtwChunk t = c;
        const int64_t R = n_a[p], C = n_b[p], S = std::min(R, C) + 1;
        t.n += 1;
        t.cells += R * C;
        t.diags += R + C - 1;
        t.paths += R + C;
        t.rows_a += R;
        t.rows_b += C;
        if (S > lds_cap) { t.ring += 3 * S; t.any_ring = true; }
        else t.lds_slots = std::max<int>(t.lds_slots, (int)S);
        dtw_layout(t, wave, dists != nullptr, first_a != nullptr, first_b != nullptr);
        if (t.bytes > budget && c.n > 0) {
            chunks.push_back(c);
            DtwChunk f;
            f.p0 = p;
            c = f;
            --p;
            continue;
        }
        c = t;
    }
    chunks.push_back(c);
    size_t need = 0;
    for (const DtwChunk &k : chunks) need = std::max(need, k.bytes);
    if (need > ctx->dtw_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->dtw_ws) ASR_HIP(ctx, hipFree(ctx->dtw_ws));
        ctx->dtw_ws = nullptr; ctx->dtw_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->dtw_ws, need));
        ctx->dtw_ws_bytes = need;
    }

    int64_t tot_cells = 0;
    for (const DtwChunk &k : chunks) tot_cells += k.cells;
    ProfScope ps(ctx, "dtw_batch", 0, 2.0 * dim * (double)tot_cells, (wave ? 17.0 : 8.0) * (double)tot_cells);
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, a_dev, tot_a, dim, dim, ctx->norm1));
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, b_dev, tot_b, dim, dim, ctx->norm2));
    char *ws = (char *)ctx->dtw_ws;
    int64_t row_a = 0, row_b = 0, host_cell = 0, host_path = 0;   // global offsets of the chunk's first pair
    std::vector<asr::DtwPair> desc;
    for (const DtwChunk &k : chunks) {
        desc.assign(k.n, asr::DtwPair());
        int64_t cell = 0, diag = 0, path = 0, ring = 0, ra = 0, rb = 0;
        for (int q = 0; q < k.n; ++q) {
            const int p = k.p0 + q;
            asr::DtwPair &P = desc[q];
            P.R = (int32_t)n_a[p]; P.C = (int32_t)n_b[p];
            P.a_row = row_a + ra; P.b_row = row_b + rb;
            P.cell = cell; P.diag = diag; P.rm = dists ? cell : -1; P.path = path;
            P.fa = ra; P.fb = rb;
            const int64_t S = std::min(n_a[p], n_b[p]) + 1;
            P.ring = S > lds_cap ? ring : -1;
            if (S > lds_cap) ring += 3 * S;
            cell += n_a[p] * n_b[p]; diag += n_a[p] + n_b[p] - 1; path += n_a[p] + n_b[p]; ra += n_a[p]; rb += n_b[p];
        }
        asr::DtwPair *d_pairs = (asr::DtwPair *)(ws + k.o_pairs);
        double *cost = (double *)(ws + k.o_cost), *rm = dists ? (double *)(ws + k.o_rm) : nullptr;
        ASR_HIP(ctx, hipMemcpyAsync(d_pairs, desc.data(), desc.size() * sizeof(asr::DtwPair), hipMemcpyHostToDevice,
                                    ctx->stream));
        ASR_HIP(ctx, asr::launch_dtw_batch_dist(ctx->stream, d_pairs, k.n, k.diags, a_dev, ctx->norm1, b_dev, ctx->norm2,
                                                dim, cost, rm));
        if (wave) {
            uint8_t *dir = (uint8_t *)(ws + k.o_dir);
            double *md = (double *)(ws + k.o_md);
            int32_t *len = (int32_t *)(ws + k.o_len), *pa = (int32_t *)(ws + k.o_pa), *pb = (int32_t *)(ws + k.o_pb);
            int32_t *fa = first_a ? (int32_t *)(ws + k.o_fa) : nullptr, *fb = first_b ? (int32_t *)(ws + k.o_fb) : nullptr;
            ASR_HIP(ctx, asr::launch_dtw_batch_wave(ctx->stream, d_pairs, k.n, k.lds_slots, k.any_ring, cost, dir,
                                                    (double *)(ws + k.o_ring), md));
            ASR_HIP(ctx, asr::launch_dtw_batch_traceback(ctx->stream, d_pairs, k.n, dir, pa, pb, len, fa, fb));
            if (min_dist)
                ASR_HIP(ctx, hipMemcpyAsync(min_dist + k.p0, md, k.n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            if (path_len)
                ASR_HIP(ctx, hipMemcpyAsync(path_len + k.p0, len, k.n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            if (path_a) {
                ASR_HIP(ctx, hipMemcpyAsync(path_a + host_path, pa, k.paths * sizeof(int32_t), hipMemcpyDeviceToHost,
                                            ctx->stream));
                ASR_HIP(ctx, hipMemcpyAsync(path_b + host_path, pb, k.paths * sizeof(int32_t), hipMemcpyDeviceToHost,
                                            ctx->stream));
            }
            if (first_a)
                ASR_HIP(ctx, hipMemcpyAsync(first_a + row_a, fa, k.rows_a * sizeof(int32_t), hipMemcpyDeviceToHost,
                                            ctx->stream));
            if (first_b)
                ASR_HIP(ctx, hipMemcpyAsync(first_b + row_b, fb, k.rows_b * sizeof(int32_t), hipMemcpyDeviceToHost,
                                            ctx->stream));
        }
        if (dists)
            ASR_HIP(ctx, hipMemcpyAsync(dists + host_cell, rm, k.cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the next chunk reuses the workspace; `desc` is rebuilt
        row_a += k.rows_a; row_b += k.rows_b; host_cell += k.cells; host_path += k.paths;
    }
    return mark_main(ctx);
}

int asr_dtw_subseq_batch_dev(asr_ctx *ctx, const float *q_dev, int64_t q_rows, const float *r_dev, int64_t r_rows,
                             const int64_t *q_row, const int64_t *n_q, const int64_t *r_row, const int64_t *n_r,
                             int n_pairs, int dim, double *cost, int32_t *start, int32_t *end, int32_t *path_len,
                             int32_t *pos) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pairs < 0 || dim < 1 || dim > 64 || q_rows < 0 || r_rows < 0)
        return fail(ctx, ASR_ERR_INVALID, "dtw_subseq: bad sizes n_pairs=%d dim=%d (1..64) q_rows=%lld r_rows=%lld", n_pairs,
                    dim, (long long)q_rows, (long long)r_rows);
    if (n_pairs == 0) return ASR_OK;
    if (!q_dev || !r_dev || !q_row || !n_q || !r_row || !n_r) return fail(ctx, ASR_ERR_INVALID, "dtw_subseq: NULL argument");
    for (int p = 0; p < n_pairs; ++p) {
        if (n_q[p] < 1 || n_q[p] > 1024 || n_r[p] < 1 || n_r[p] > 100000 || n_q[p] * (n_r[p] + n_q[p]) >= (1ll << 31))
            return fail(ctx, ASR_ERR_INVALID, "dtw_subseq: pair %d has bad sizes n_q=%lld (1..1024) n_r=%lld (1..100000)", p,
                        (long long)n_q[p], (long long)n_r[p]);
        if (q_row[p] < 0 || q_row[p] > q_rows - n_q[p] || r_row[p] < 0 || r_row[p] > r_rows - n_r[p])
            return fail(ctx, ASR_ERR_INVALID, "dtw_subseq: pair %d reads rows outside its buffers (q %lld+%lld of %lld, r "
                        "%lld+%lld of %lld)", p, (long long)q_row[p], (long long)n_q[p], (long long)q_rows,
                        (long long)r_row[p], (long long)n_r[p], (long long)r_rows);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_norms(ctx, q_rows, r_rows);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // ASR_DTW_BUDGET_MB: device workspace per chunk of pairs; ASR_DTW_SUBSEQ_LDS_CAP=<bytes> (debug): workgroups whose
    // staging ring is larger read the reference rows from global memory (exercises that path at small sizes)
    const size_t budget = (size_t)std::max<int64_t>(dtw_env("ASR_DTW_BUDGET_MB", 4096), 1) << 20;
    int lds_dev = 0;
    if (hipDeviceGetAttribute(&lds_dev, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->cfg.device) != hipSuccess)
        lds_dev = 65536;
    const size_t lds_limit = (size_t)std::min<int64_t>(lds_dev, dtw_env("ASR_DTW_SUBSEQ_LDS_CAP", 1 << 30));

    // chunks of consecutive pairs whose workspace fits the budget (a pair larger than it gets a chunk of its own):
    // pair table | direction bytes | cost | start | end | path_len | pos, 256-byte aligned sections
    struct Chunk { int p0 = 0, n = 0; int64_t dir = 0, rows = 0; size_t o_dir = 0, o_cost = 0, o_start = 0, o_end = 0,
                   o_len = 0, o_pos = 0, bytes = 0; };
    auto layout = [](Chunk &c) {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += dtw_align(bytes); return at; };
        take((size_t)c.n * sizeof(asr::SubseqPair));
        c.o_dir = take((size_t)c.dir);
        c.o_cost = take((size_t)c.n * sizeof(double));
        c.o_start = take((size_t)c.n * sizeof(int32_t));
        c.o_end = take((size_t)c.n * sizeof(int32_t));
        c.o_len = take((size_t)c.n * sizeof(int32_t));
        c.o_pos = take((size_t)c.rows * sizeof(int32_t));
        c.bytes = o;
    };
    std::vector<Chunk> chunks;
    Chunk c;
    for (int p = 0; p < n_pairs; ++p) {
        Chunk t = c;
        t.n += 1;
        t.dir += n_q[p] * (n_r[p] + n_q[p] - 1);
        t.rows += n_q[p];
        layout(t);
        if (t.bytes > budget && c.n > 0) {
            chunks.push_back(c);
            Chunk f;
            f.p0 = p;
            c = f;
            --p;
            continue;
        }
        c = t;
    }
    chunks.push_back(c);
    size_t need = 0;
    for (const Chunk &k : chunks) need = std::max(need, k.bytes);
    if (need > ctx->subseq_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->subseq_ws) ASR_HIP(ctx, hipFree(ctx->subseq_ws));
        ctx->subseq_ws = nullptr; ctx->subseq_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->subseq_ws, need));
        ctx->subseq_ws_bytes = need;
    }

    double tot_cells = 0;
    for (int p = 0; p < n_pairs; ++p) tot_cells += (double)n_q[p] * (double)n_r[p];
    ProfScope ps(ctx, "dtw_subseq", 0, 2.0 * dim * tot_cells, tot_cells);
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, q_dev, q_rows, dim, dim, ctx->norm1));
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, r_dev, r_rows, dim, dim, ctx->norm2));
    char *ws = (char *)ctx->subseq_ws;
    int64_t host_pos = 0;
    std::vector<asr::SubseqPair> desc;
    for (const Chunk &k : chunks) {
        // the table is ordered by size class (waves = ceil(n_q / 64)): one launch per class present in the chunk
        desc.clear();
        int class_n[17] = {0};
        std::vector<int64_t> dir_at(k.n), pos_at(k.n);
        int64_t dir = 0, rows = 0;
        for (int q = 0; q < k.n; ++q) {
            const int p = k.p0 + q;
            dir_at[q] = dir; pos_at[q] = rows;
            dir += n_q[p] * (n_r[p] + n_q[p] - 1); rows += n_q[p];
            class_n[(n_q[p] + 63) / 64] += 1;
        }
        for (int w = 1; w <= 16; ++w)
            for (int q = 0; q < k.n && class_n[w] > 0; ++q) {
                const int p = k.p0 + q;
                if ((n_q[p] + 63) / 64 != w) continue;
                asr::SubseqPair P;
                P.Q = (int32_t)n_q[p]; P.S = (int32_t)n_r[p];
                P.q_row = q_row[p]; P.r_row = r_row[p];
                P.dir = dir_at[q]; P.pos = pos_at[q]; P.out = q; P.pad = 0;
                desc.push_back(P);
            }
        asr::SubseqPair *d_pairs = (asr::SubseqPair *)ws;
        uint8_t *d_dir = (uint8_t *)(ws + k.o_dir);
        double *d_cost = (double *)(ws + k.o_cost);
        int32_t *d_start = (int32_t *)(ws + k.o_start), *d_end = (int32_t *)(ws + k.o_end);
        int32_t *d_len = (int32_t *)(ws + k.o_len), *d_pos = (int32_t *)(ws + k.o_pos);
        ASR_HIP(ctx, hipMemcpyAsync(d_pairs, desc.data(), desc.size() * sizeof(asr::SubseqPair), hipMemcpyHostToDevice,
                                    ctx->stream));
        {
            ProfScope pk(ctx, "dtw_subseq_wave", 0, 0.0, 0.0);  // the kernels alone (the outer scope has the copies too)
            int at = 0;
            for (int w = 1; w <= 16; ++w) {
                if (class_n[w] == 0) continue;
                ASR_HIP(ctx, asr::launch_dtw_subseq(ctx->stream, d_pairs + at, class_n[w], w, lds_limit, q_dev,
                                                    ctx->norm1, r_dev, ctx->norm2, dim, d_dir, d_cost, d_start, d_end,
                                                    d_len, pos ? d_pos : nullptr));
                at += class_n[w];
            }
        }
        if (cost) ASR_HIP(ctx, hipMemcpyAsync(cost + k.p0, d_cost, k.n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (start)
            ASR_HIP(ctx, hipMemcpyAsync(start + k.p0, d_start, k.n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (end) ASR_HIP(ctx, hipMemcpyAsync(end + k.p0, d_end, k.n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (path_len)
            ASR_HIP(ctx, hipMemcpyAsync(path_len + k.p0, d_len, k.n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (pos)
            ASR_HIP(ctx, hipMemcpyAsync(pos + host_pos, d_pos, k.rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the next chunk reuses the workspace; `desc` is rebuilt
        host_pos += k.rows;
    }
    return mark_main(ctx);
}

int asr_dtw_follow_batch_dev(asr_ctx *ctx, const float *q_dev, int64_t q_rows, const float *r_dev, int64_t r_rows,
                             const int64_t *q_row, const int64_t *n_q, const int64_t *r_row, const int64_t *n_r,
                             const int64_t *rows_before, int n_pairs, int dim, double *acc_dev, int32_t *org_dev,
                             int64_t state_len, const int64_t *state_off, double *cost, int32_t *start, int32_t *pos) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pairs < 0 || dim < 1 || dim > 64 || q_rows < 0 || r_rows < 0 || state_len < 0)
        return fail(ctx, ASR_ERR_INVALID, "dtw_follow: bad sizes n_pairs=%d dim=%d (1..64) q_rows=%lld r_rows=%lld "
                    "state_len=%lld", n_pairs, dim, (long long)q_rows, (long long)r_rows, (long long)state_len);
    if (n_pairs == 0) return ASR_OK;
    if (!q_dev || !r_dev || !q_row || !n_q || !r_row || !n_r || !rows_before || !acc_dev || !org_dev || !state_off)
        return fail(ctx, ASR_ERR_INVALID, "dtw_follow: NULL argument");
    int64_t tot_rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (n_q[p] < 1 || n_q[p] > 1024 || n_r[p] < 1 || n_r[p] > 100000 || rows_before[p] < 0 ||
            rows_before[p] >= (1ll << 31) - n_q[p])
            return fail(ctx, ASR_ERR_INVALID, "dtw_follow: pair %d has bad sizes n_q=%lld (1..1024) n_r=%lld (1..100000) "
                        "rows_before=%lld (rows_before + n_q < 2^31)", p, (long long)n_q[p], (long long)n_r[p],
                        (long long)rows_before[p]);
        if (q_row[p] < 0 || q_row[p] > q_rows - n_q[p] || r_row[p] < 0 || r_row[p] > r_rows - n_r[p])
            return fail(ctx, ASR_ERR_INVALID, "dtw_follow: pair %d reads rows outside its buffers (q %lld+%lld of %lld, r "
                        "%lld+%lld of %lld)", p, (long long)q_row[p], (long long)n_q[p], (long long)q_rows,
                        (long long)r_row[p], (long long)n_r[p], (long long)r_rows);
        if (state_off[p] < 0 || state_off[p] > state_len - n_r[p])
            return fail(ctx, ASR_ERR_INVALID, "dtw_follow: pair %d keeps its state outside the buffers (%lld+%lld of %lld)",
                        p, (long long)state_off[p], (long long)n_r[p], (long long)state_len);
        tot_rows += n_q[p];
    }
    {   // two pairs that share state entries would race
        std::vector<int> by_off(n_pairs);
        for (int p = 0; p < n_pairs; ++p) by_off[p] = p;
        std::sort(by_off.begin(), by_off.end(), [&](int a, int b) { return state_off[a] < state_off[b]; });
        for (int k = 1; k < n_pairs; ++k) {
            const int a = by_off[k - 1], b = by_off[k];
            if (state_off[a] + n_r[a] > state_off[b])
                return fail(ctx, ASR_ERR_INVALID, "dtw_follow: the states of pairs %d and %d overlap", a, b);
        }
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_norms(ctx, q_rows, r_rows);
    if (rc != ASR_OK) return rc;
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // ASR_DTW_SUBSEQ_LDS_CAP=<bytes> (debug): as in asr_dtw_subseq_batch_dev.  ASR_DTW_BUDGET_MB has nothing to chunk:
    // the workspace is the pair table and 16 bytes per new query row
    int lds_dev = 0;
    if (hipDeviceGetAttribute(&lds_dev, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->cfg.device) != hipSuccess)
        lds_dev = 65536;
    const size_t lds_limit = (size_t)std::min<int64_t>(lds_dev, dtw_env("ASR_DTW_SUBSEQ_LDS_CAP", 1 << 30));

    // pair table | cost | start | pos, 256-byte aligned sections
    const size_t o_cost = dtw_align((size_t)n_pairs * sizeof(asr::FollowPair));
    const size_t o_start = o_cost + dtw_align((size_t)tot_rows * sizeof(double));
    const size_t o_pos = o_start + dtw_align((size_t)tot_rows * sizeof(int32_t));
    const size_t need = o_pos + dtw_align((size_t)tot_rows * sizeof(int32_t));
    if (need > ctx->subseq_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->subseq_ws) ASR_HIP(ctx, hipFree(ctx->subseq_ws));
        ctx->subseq_ws = nullptr; ctx->subseq_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->subseq_ws, need));
        ctx->subseq_ws_bytes = need;
    }

    double tot_cells = 0;
    for (int p = 0; p < n_pairs; ++p) tot_cells += (double)n_q[p] * (double)n_r[p];
    ProfScope ps(ctx, "dtw_follow", 0, 2.0 * dim * tot_cells, 0.0);
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, q_dev, q_rows, dim, dim, ctx->norm1));
    ASR_HIP(ctx, asr::launch_row_norms(ctx->stream, r_dev, r_rows, dim, dim, ctx->norm2));
    // the table is ordered by size class (waves = ceil(n_q / 64)): one launch per class present
    std::vector<asr::FollowPair> desc;
    desc.reserve(n_pairs);
    std::vector<int64_t> out_at(n_pairs);
    int class_n[17] = {0};
    int64_t rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        out_at[p] = rows;
        rows += n_q[p];
        class_n[(n_q[p] + 63) / 64] += 1;
    }
    for (int w = 1; w <= 16; ++w)
        for (int p = 0; p < n_pairs && class_n[w] > 0; ++p) {
            if ((n_q[p] + 63) / 64 != w) continue;
            asr::FollowPair P;
            P.B = (int32_t)n_q[p]; P.S = (int32_t)n_r[p];
            P.q_row = q_row[p]; P.r_row = r_row[p];
            P.state = state_off[p]; P.out = out_at[p]; P.n0 = (int32_t)rows_before[p]; P.pad = 0;
            desc.push_back(P);
        }
    char *ws = (char *)ctx->subseq_ws;
    asr::FollowPair *d_pairs = (asr::FollowPair *)ws;
    double *d_cost = (double *)(ws + o_cost);
    int32_t *d_start = (int32_t *)(ws + o_start), *d_pos = (int32_t *)(ws + o_pos);
    ASR_HIP(ctx, hipMemcpyAsync(d_pairs, desc.data(), desc.size() * sizeof(asr::FollowPair), hipMemcpyHostToDevice,
                                ctx->stream));
    {
        ProfScope pk(ctx, "dtw_follow_wave", 0, 0.0, 0.0);      // the kernels alone (the outer scope has the copies too)
        int at = 0;
        for (int w = 1; w <= 16; ++w) {
            if (class_n[w] == 0) continue;
            ASR_HIP(ctx, asr::launch_dtw_follow(ctx->stream, d_pairs + at, class_n[w], w, lds_limit, q_dev, ctx->norm1,
                                                r_dev, ctx->norm2, dim, acc_dev, org_dev, d_cost, d_start, d_pos));
            at += class_n[w];
        }
    }
    if (cost) ASR_HIP(ctx, hipMemcpyAsync(cost, d_cost, tot_rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (start) ASR_HIP(ctx, hipMemcpyAsync(start, d_start, tot_rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (pos) ASR_HIP(ctx, hipMemcpyAsync(pos, d_pos, tot_rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));       // `desc` is read by the copy; the outputs are the caller's
    return mark_main(ctx);
}

int asr_spectrogram_dev(asr_ctx *ctx, const float *samples_dev, int64_t n_samples, int frame_size, double hop,
                        const float *window, const int32_t *fb_start, const int32_t *fb_len, const float *fb_weights,
                        int n_filters, float mul, float add, int64_t n_frames, int transposed, float *out_dev) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_samples < 0 || n_frames < 0 || frame_size < 64 || frame_size > 8192 || (frame_size & (frame_size - 1)) ||
        !(hop > 0.0) || n_filters < 1 || n_filters > 4096)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram: bad sizes (frame_size must be a power of two in [64, 8192])");
    if (n_frames == 0) return ASR_OK;
    if (!samples_dev || !window || !fb_start || !fb_len || !fb_weights || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram: NULL argument");
    std::vector<int32_t> off(n_filters);
    int64_t total_w = 0;
    int max_bin = 0;
    for (int f = 0; f < n_filters; ++f) {
        if (fb_start[f] < 0 || fb_len[f] < 0 || fb_start[f] + fb_len[f] > frame_size / 2)
            return fail(ctx, ASR_ERR_INVALID, "spectrogram: filter %d covers bins [%d, %d) outside [0, %d)", f, fb_start[f],
                        fb_start[f] + fb_len[f], frame_size / 2);
        off[f] = (int32_t)total_w;
        total_w += fb_len[f];
        max_bin = std::max(max_bin, fb_start[f] + fb_len[f]);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    char *buf = nullptr;
    const size_t b_win = (size_t)frame_size * 4, b_i = (size_t)n_filters * 4, b_w = (size_t)std::max<int64_t>(total_w, 1) * 4;
    ASR_HIP(ctx, hipMalloc((void **)&buf, b_win + 3 * b_i + b_w));
    float *d_win = (float *)buf;
    int32_t *d_start = (int32_t *)(buf + b_win), *d_len = d_start + n_filters, *d_off = d_len + n_filters;
    float *d_w = (float *)(buf + b_win + 3 * b_i);
    hipError_t e = hipMemcpyAsync(d_win, window, b_win, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_start, fb_start, b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_len, fb_len, b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && total_w) e = hipMemcpyAsync(d_w, fb_weights, (size_t)total_w * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "spectrogram", 0, 4.0 * frame_size * (double)max_bin * (double)n_frames,
                     4.0 * hop * (double)n_frames);
        e = asr::launch_spectrogram(ctx->stream, samples_dev, n_samples, d_win, frame_size, hop, max_bin, d_start, d_len,
                                    d_off, d_w, n_filters, mul, add, out_dev, n_frames, transposed);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "spectrogram: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_gather_windows_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, const double *desc, int n, int out_h,
                           int out_w, float *out_dev) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n < 0 || out_h < 1 || out_w < 1) return fail(ctx, ASR_ERR_INVALID, "gather_windows: bad sizes");
    if (n == 0) return ASR_OK;
    if (!src_dev || !desc || !out_dev) return fail(ctx, ASR_ERR_INVALID, "gather_windows: NULL argument");
    for (int i = 0; i < n; ++i) {       // every reachable source index must lie inside the pool buffer
        const double *d = desc + (size_t)i * 9;
        const double lo = d[0] + d[8], hi = d[0] + d[4] * d[1] + d[8] + d[7];
        if (!(d[1] >= 1 && d[4] >= 0 && d[7] >= 0 && lo >= 0 && hi < (double)src_floats && d[3] > 0 && d[6] > 0))
            return fail(ctx, ASR_ERR_INVALID, "gather_windows: descriptor %d addresses [%g, %g] outside the %lld-float pool",
                        i, lo, hi, (long long)src_floats);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    double *d_desc = nullptr;
    ASR_HIP(ctx, hipMalloc((void **)&d_desc, (size_t)n * 9 * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d_desc, desc, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = asr::launch_gather_windows(ctx->stream, src_dev, d_desc, n, out_h, out_w, out_dev);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_desc);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "gather_windows: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_piece_vote_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_idx, const int32_t *ids_dev, int64_t n_db,
                       int32_t n_pieces, int top_k, int32_t *pieces, int32_t *counts, int32_t *n_out) {
    if (!ctx || !pieces || !counts || !n_out) return ASR_ERR_INVALID;
    if (n_idx < 0 || n_db < 0 || n_pieces < 1 || top_k < 1 || top_k > 1024)
        return fail(ctx, ASR_ERR_INVALID, "piece_vote: bad sizes n_idx=%lld n_db=%lld n_pieces=%d top_k=%d",
                    (long long)n_idx, (long long)n_db, n_pieces, top_k);
    if (n_idx > 0 && (!idx_dev || !ids_dev)) return fail(ctx, ASR_ERR_INVALID, "piece_vote: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int32_t *ws = nullptr;
    ASR_HIP(ctx, hipMalloc((void **)&ws, ((size_t)n_pieces + 2 * (size_t)top_k) * sizeof(int32_t)));
    int32_t *d_piece = ws + n_pieces, *d_count = d_piece + top_k;
    hipError_t e;
    {
        ProfScope ps(ctx, "piece_vote", 0, 0.0, 8.0 * (double)n_idx);
        e = asr::launch_piece_vote(ctx->stream, idx_dev, n_idx, ids_dev, n_db, n_pieces, top_k, ws, d_piece, d_count);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pieces, d_piece, (size_t)top_k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d_count, (size_t)top_k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(ws);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "piece_vote: %s", hipGetErrorString(e));
    int m = 0;
    while (m < top_k && pieces[m] >= 0) ++m;
    *n_out = m;
    return mark_main(ctx);
}

int asr_piece_vote_batch_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_groups, int64_t per_group,
                             const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k, const int32_t *targets,
                             int32_t *pieces, int32_t *counts, int32_t *n_out, int32_t *ranks, double *ratios) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_groups < 0 || n_groups > INT32_MAX || per_group < 0 || n_db < 0 || n_db > INT32_MAX || n_pieces < 1 ||
        n_pieces > (1 << 30) || top_k < 1 || (per_group > 0 && n_groups > (INT64_MAX / 8) / per_group))
        return fail(ctx, ASR_ERR_INVALID,
                    "piece_vote_batch: bad sizes n_groups=%lld per_group=%lld n_db=%lld n_pieces=%d top_k=%d",
                    (long long)n_groups, (long long)per_group, (long long)n_db, n_pieces, top_k);
    if (!pieces || !counts || !n_out || (targets && (!ranks || !ratios)))
        return fail(ctx, ASR_ERR_INVALID, "piece_vote_batch: NULL output (pieces, counts, n_out; ranks, ratios with targets)");
    if (n_groups > 0 && per_group > 0 && (!idx_dev || (n_db > 0 && !ids_dev)))
        return fail(ctx, ASR_ERR_INVALID, "piece_vote_batch: NULL argument");
    if (n_groups == 0) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;

    // ASR_VOTE_LDS_PIECES=<n> (debug): groups with n_pieces above it take the global-workspace path, which exercises
    // it at small sizes; ASR_VOTE_BUDGET_MB: global-path counters + keys per launch (more groups run in chunks)
    const int64_t lds_pieces = std::min<int64_t>(asr::VOTE_LDS_PIECES, dtw_env("ASR_VOTE_LDS_PIECES", 1 << 30));
    const bool global_path = n_pieces > lds_pieces;
    int64_t keys_cap = 1;
    while (keys_cap < std::min<int64_t>(n_pieces, per_group)) keys_cap <<= 1;
    const size_t per_group_ws = (size_t)n_pieces * sizeof(int32_t) + (size_t)keys_cap * sizeof(uint64_t);
    const size_t budget = (size_t)std::max<int64_t>(dtw_env("ASR_VOTE_BUDGET_MB", 1024), 1) << 20;
    const int64_t chunk = global_path ? std::max<int64_t>(1, std::min<int64_t>(n_groups, budget / per_group_ws)) : n_groups;

    // results block (downloaded in one copy): pieces | counts (n_groups x top_k) | n_out | ranks | ratios
    const size_t G = (size_t)n_groups, GK = G * (size_t)top_k;
    const size_t o_counts = GK * 4, o_nout = 2 * GK * 4, o_ranks = o_nout + G * 4;
    const size_t o_ratios = dtw_align(o_ranks + G * 4), res_bytes = o_ratios + G * 8;
    const size_t o_targets = dtw_align(res_bytes), o_hist = dtw_align(o_targets + G * 4);
    const size_t o_keys = dtw_align(o_hist + (global_path ? (size_t)chunk * n_pieces * 4 : 0));
    const size_t need = o_keys + (global_path ? (size_t)chunk * keys_cap * 8 : 0);
    if (need > ctx->vote_ws_bytes) {
        rc = sync_all(ctx);
        if (rc != ASR_OK) return rc;
        if (ctx->vote_ws) ASR_HIP(ctx, hipFree(ctx->vote_ws));
        ctx->vote_ws = nullptr; ctx->vote_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->vote_ws, need));
        ctx->vote_ws_bytes = need;
    }
    char *ws = (char *)ctx->vote_ws;
    int32_t *d_targets = targets ? (int32_t *)(ws + o_targets) : nullptr;
    if (targets) ASR_HIP(ctx, hipMemcpyAsync(d_targets, targets, G * 4, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "piece_vote_batch", 0, 0.0, 8.0 * (double)n_groups * (double)per_group + 8.0 * (double)GK);
        for (int64_t g0 = 0; g0 < n_groups; g0 += chunk) {
            asr::VoteBatchArgs a;
            a.n_groups = std::min<int64_t>(chunk, n_groups - g0);
            a.per_group = per_group;
            a.idx = idx_dev ? idx_dev + g0 * per_group : nullptr;
            a.ids = ids_dev; a.n_db = n_db; a.n_pieces = n_pieces; a.top_k = top_k;
            a.targets = d_targets ? d_targets + g0 : nullptr;
            a.pieces = (int32_t *)ws + g0 * top_k;
            a.counts = (int32_t *)(ws + o_counts) + g0 * top_k;
            a.n_out = (int32_t *)(ws + o_nout) + g0;
            a.ranks = (int32_t *)(ws + o_ranks) + g0;
            a.ratios = (double *)(ws + o_ratios) + g0;
            a.hist_ws = (int32_t *)(ws + o_hist);
            a.keys_ws = (uint64_t *)(ws + o_keys);
            a.keys_cap = keys_cap;
            ASR_HIP(ctx, asr::launch_piece_vote_batch(ctx->stream, a, global_path));
        }
    }
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(pieces, host.data(), GK * 4);
    memcpy(counts, host.data() + o_counts, GK * 4);
    memcpy(n_out, host.data() + o_nout, G * 4);
    if (targets) {
        memcpy(ranks, host.data() + o_ranks, G * 4);
        memcpy(ratios, host.data() + o_ratios, G * 8);
    }
    return mark_main(ctx);
}

// ---- running piece vote (track_kernels.hip) ---------------------------------------------------------------------------
// both calls keep their tables and results in the vote workspace of the context
static int track_ws(asr_ctx *ctx, size_t need) {
    if (need <= ctx->vote_ws_bytes) return ASR_OK;
    int rc = sync_all(ctx);
    if (rc != ASR_OK) return rc;
    if (ctx->vote_ws) ASR_HIP(ctx, hipFree(ctx->vote_ws));
    ctx->vote_ws = nullptr; ctx->vote_ws_bytes = 0;
    ASR_HIP(ctx, hipMalloc(&ctx->vote_ws, need));
    ctx->vote_ws_bytes = need;
    return ASR_OK;
}

int asr_track_gate_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, int n_rec, const int64_t *offsets,
                       const int32_t *bins, const int32_t *frames, const int64_t *frame0, const float *norm, int width,
                       float *m_prob, uint8_t *voiced, float *level) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_rec < 0 || src_floats < 0 || width < 8 || width > 128)
        return fail(ctx, ASR_ERR_INVALID, "track_gate: bad sizes n_rec=%d width=%d (8..128)", n_rec, width);
    if (n_rec == 0) return ASR_OK;
    if (!src_dev || !offsets || !bins || !frames || !m_prob || !voiced)
        return fail(ctx, ASR_ERR_INVALID, "track_gate: NULL argument");
    std::vector<asr::TrackRec> recs(n_rec);
    int64_t total = 0;
    for (int r = 0; r < n_rec; ++r) {
        if (bins[r] < 1 || frames[r] < 1 || offsets[r] < 0 || offsets[r] > src_floats ||
            (int64_t)bins[r] * frames[r] > src_floats - offsets[r])
            return fail(ctx, ASR_ERR_INVALID, "track_gate: recording %d (%d x %d at %lld) lies outside the %lld-float buffer",
                        r, bins[r], frames[r], (long long)offsets[r], (long long)src_floats);
        asr::TrackRec &R = recs[r];
        R.off = offsets[r]; R.first = total; R.frame0 = frame0 ? frame0[r] : 0;
        R.bins = bins[r]; R.frames = frames[r];
        R.has_norm = norm && norm[r] == norm[r];
        R.norm = R.has_norm ? norm[r] : 0.0f;
        total += frames[r];
        if (total > INT32_MAX) return fail(ctx, ASR_ERR_INVALID, "track_gate: more than 2^31 - 1 frames");
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // results (one download): m_prob | level | voiced; then the recording table and the column sums
    const size_t T = (size_t)total, o_level = T * 4, o_voiced = o_level + (size_t)n_rec * 4, res_bytes = o_voiced + T;
    const size_t o_recs = dtw_align(res_bytes), o_colsum = dtw_align(o_recs + recs.size() * sizeof(asr::TrackRec));
    rc = track_ws(ctx, o_colsum + T * 4);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_recs, recs.data(), recs.size() * sizeof(asr::TrackRec), hipMemcpyHostToDevice,
                                ctx->stream));
    {
        ProfScope ps(ctx, "track_gate", 0, 0.0, 4.0 * (double)src_floats);
        asr::TrackGateArgs a;
        a.src = src_dev; a.recs = (const asr::TrackRec *)(ws + o_recs); a.n_rec = n_rec; a.total_frames = total;
        a.width = width;
        a.colsum = (float *)(ws + o_colsum); a.level = (float *)(ws + o_level);
        a.m_prob = (float *)ws; a.voiced = (uint8_t *)(ws + o_voiced);
        ASR_HIP(ctx, asr::launch_track_gate(ctx->stream, a));
    }
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // (also: `recs` was read by the upload)
    memcpy(m_prob, host.data(), T * 4);
    if (level) memcpy(level, host.data() + o_level, (size_t)n_rec * 4);
    memcpy(voiced, host.data() + o_voiced, T);
    return mark_main(ctx);
}

// the running level's rule: memory 0 or width .. 2^20 (a shorter memory would not cover the columns of the mean), a
// floor that is a number or -inf
static bool track_running_bad(int memory, float floor, int width) {
    return memory < 0 || (memory > 0 && memory < width) || memory > (1 << 20) || floor != floor || floor == INFINITY;
}

int asr_track_gate_running_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, int n_rec, const int64_t *offsets,
                               const int32_t *bins, const int32_t *frames, int width, int memory, float floor,
                               float *m_prob, uint8_t *voiced, float *level) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_rec < 0 || src_floats < 0 || width < 8 || width > 128)
        return fail(ctx, ASR_ERR_INVALID, "track_gate_running: bad sizes n_rec=%d width=%d (8..128)", n_rec, width);
    if (track_running_bad(memory, floor, width))
        return fail(ctx, ASR_ERR_INVALID, "track_gate_running: memory=%d (0, or width=%d..2^20) floor=%g (not NaN, not +inf)",
                    memory, width, (double)floor);
    if (n_rec == 0) return ASR_OK;
    if (!src_dev || !offsets || !bins || !frames || !m_prob || !voiced)
        return fail(ctx, ASR_ERR_INVALID, "track_gate_running: NULL argument");
    std::vector<asr::TrackRec> recs(n_rec);
    std::vector<asr::TrackLevelSeq> seqs(n_rec);
    int64_t total = 0;
    for (int r = 0; r < n_rec; ++r) {
        if (bins[r] < 1 || frames[r] < 1 || offsets[r] < 0 || offsets[r] > src_floats ||
            (int64_t)bins[r] * frames[r] > src_floats - offsets[r])
            return fail(ctx, ASR_ERR_INVALID,
                        "track_gate_running: recording %d (%d x %d at %lld) lies outside the %lld-float buffer", r, bins[r],
                        frames[r], (long long)offsets[r], (long long)src_floats);
        asr::TrackRec &R = recs[r];
        R.off = offsets[r]; R.first = total; R.frame0 = 0; R.bins = bins[r]; R.frames = frames[r];
        R.has_norm = 0; R.norm = 0.0f;
        asr::TrackLevelSeq &Q = seqs[r];
        Q.cs_first = Q.out_first = Q.sfx_first = total; Q.state_off = 0; Q.frames_before = 0;
        Q.n_new = frames[r]; Q.n_hist = 0;
        total += frames[r];
        if (total > INT32_MAX / 2) return fail(ctx, ASR_ERR_INVALID, "track_gate_running: more than 2^30 - 1 frames");
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // results (one download): m_prob | level per frame | voiced; then the two tables, the column sums, the suffix maxima
    // and the (unused) carried maxima
    const size_t T = (size_t)total, o_level = T * 4, o_voiced = 2 * T * 4, res_bytes = o_voiced + T;
    const size_t o_recs = dtw_align(res_bytes), o_seqs = dtw_align(o_recs + recs.size() * sizeof(asr::TrackRec));
    const size_t o_colsum = dtw_align(o_seqs + seqs.size() * sizeof(asr::TrackLevelSeq));
    const size_t o_sfx = dtw_align(o_colsum + T * 4), o_last = dtw_align(o_sfx + (memory > 0 ? T * 4 : 0));
    rc = track_ws(ctx, o_last + (size_t)n_rec * 4);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_recs, recs.data(), recs.size() * sizeof(asr::TrackRec), hipMemcpyHostToDevice,
                                ctx->stream));
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_seqs, seqs.data(), seqs.size() * sizeof(asr::TrackLevelSeq), hipMemcpyHostToDevice,
                                ctx->stream));
    {
        ProfScope ps(ctx, "track_gate_running", 0, 0.0, 4.0 * (double)src_floats);
        asr::TrackGateArgs a;
        a.src = src_dev; a.recs = (const asr::TrackRec *)(ws + o_recs); a.n_rec = n_rec; a.total_frames = total;
        a.width = width;
        a.colsum = (float *)(ws + o_colsum); a.level = nullptr;
        a.m_prob = (float *)ws; a.voiced = (uint8_t *)(ws + o_voiced);
        asr::TrackLevelArgs l;
        l.colsum = a.colsum; l.seqs = (const asr::TrackLevelSeq *)(ws + o_seqs); l.n_seq = n_rec; l.memory = memory;
        l.floor = floor; l.state = nullptr;
        l.suffix = (float *)(ws + o_sfx); l.last = (float *)(ws + o_last); l.level = (float *)(ws + o_level);
        ASR_HIP(ctx, asr::launch_track_colsum(ctx->stream, a));
        ASR_HIP(ctx, asr::launch_track_level(ctx->stream, l));
        ASR_HIP(ctx, asr::launch_track_gate_running(ctx->stream, a, l.level));
    }
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // (also: the tables were read by the uploads)
    memcpy(m_prob, host.data(), T * 4);
    if (level) memcpy(level, host.data() + o_level, T * 4);
    memcpy(voiced, host.data() + o_voiced, T);
    return mark_main(ctx);
}

int asr_track_vote_batch_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_rows, int n_rec, const int64_t *row_first,
                             const int64_t *row_count, const int64_t *emit_from, int n_candidates, int running_frames,
                             const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k, int32_t *pieces,
                             int32_t *counts, int32_t *n_out) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_rec < 0 || n_rows < 0 || top_k < 1 || top_k > 64 || n_candidates < 1 || running_frames < 1 ||
        n_db < n_candidates || n_db > INT32_MAX || n_pieces < 1 || n_pieces > (1 << 30) ||
        n_rows > (INT64_MAX / 4) / n_candidates)
        return fail(ctx, ASR_ERR_INVALID,
                    "track_vote_batch: bad sizes n_rows=%lld n_rec=%d n_candidates=%d running_frames=%d n_db=%lld "
                    "n_pieces=%d top_k=%d (1..64)", (long long)n_rows, n_rec, n_candidates, running_frames,
                    (long long)n_db, n_pieces, top_k);
    if (n_rec == 0) return ASR_OK;
    if (!row_first || !row_count) return fail(ctx, ASR_ERR_INVALID, "track_vote_batch: NULL argument");
    const int64_t seg_frames = std::max<int64_t>(1, dtw_env("ASR_TRACK_SEG_FRAMES", 64));
    std::vector<asr::TrackSeg> segs;
    int64_t n_emit = 0;
    for (int r = 0; r < n_rec; ++r) {
        const int64_t from = emit_from ? emit_from[r] : 0;
        if (row_first[r] < 0 || row_count[r] < 0 || row_first[r] > n_rows || row_count[r] > n_rows - row_first[r] ||
            from < 0 || from > row_count[r])
            return fail(ctx, ASR_ERR_INVALID, "track_vote_batch: recording %d: rows [%lld, +%lld) emit_from %lld of %lld rows",
                        r, (long long)row_first[r], (long long)row_count[r], (long long)from, (long long)n_rows);
        for (int64_t f = from; f < row_count[r]; f += seg_frames) {
            asr::TrackSeg S;
            S.row0 = row_first[r]; S.f0 = f; S.out0 = n_emit + (f - from);
            S.n = (int32_t)std::min<int64_t>(seg_frames, row_count[r] - f); S.pad = 0;
            segs.push_back(S);
        }
        n_emit += row_count[r] - from;
    }
    if (n_emit == 0) return ASR_OK;
    if (n_emit > INT32_MAX) return fail(ctx, ASR_ERR_INVALID, "track_vote_batch: more than 2^31 - 1 frames");
    if (!idx_dev || !ids_dev || !pieces || !counts || !n_out)
        return fail(ctx, ASR_ERR_INVALID, "track_vote_batch: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;

    // ASR_TRACK_SEG_FRAMES=<n> (debug): frames per segment (default 64); ASR_TRACK_LDS_PIECES=<n> (debug): n_pieces above
    // it take the global-workspace path; ASR_VOTE_BUDGET_MB bounds that workspace (fewer workgroups, more segments each)
    const int64_t lds_pieces = std::min<int64_t>(asr::TRACK_LDS_PIECES, dtw_env("ASR_TRACK_LDS_PIECES", 1 << 30));
    const bool global_path = n_pieces > lds_pieces;
    const size_t budget = (size_t)std::max<int64_t>(dtw_env("ASR_VOTE_BUDGET_MB", 1024), 1) << 20;
    int64_t grid = std::min<int64_t>((int64_t)segs.size(), 65536);
    if (global_path) grid = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(grid, 4096), budget / ((size_t)n_pieces * 4)));

    // results block (one download): pieces | counts (n_emit x top_k) | n_out; then the segment table and the counters
    const size_t E = (size_t)n_emit, EK = E * (size_t)top_k;
    const size_t o_counts = EK * 4, o_nout = 2 * EK * 4, res_bytes = o_nout + E * 4;
    const size_t o_segs = dtw_align(res_bytes), o_hist = dtw_align(o_segs + segs.size() * sizeof(asr::TrackSeg));
    rc = track_ws(ctx, o_hist + (global_path ? (size_t)grid * n_pieces * 4 : 0));
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_segs, segs.data(), segs.size() * sizeof(asr::TrackSeg), hipMemcpyHostToDevice,
                                ctx->stream));
    {
        ProfScope ps(ctx, "track_vote_batch", 0, 0.0, 4.0 * (double)n_rows * n_candidates + 8.0 * (double)EK);
        asr::TrackVoteArgs a;
        a.idx = idx_dev; a.segs = (const asr::TrackSeg *)(ws + o_segs); a.n_segs = (int64_t)segs.size();
        a.n_candidates = n_candidates; a.running_frames = running_frames;
        a.ids = ids_dev; a.n_db = n_db; a.n_pieces = n_pieces; a.top_k = top_k;
        a.pieces = (int32_t *)ws; a.counts = (int32_t *)(ws + o_counts); a.n_out = (int32_t *)(ws + o_nout);
        a.hist_ws = (int32_t *)(ws + o_hist);
        ASR_HIP(ctx, asr::launch_track_vote(ctx->stream, a, (int)grid, global_path));
    }
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(pieces, host.data(), EK * 4);
    memcpy(counts, host.data() + o_counts, EK * 4);
    memcpy(n_out, host.data() + o_nout, E * 4);
    return mark_main(ctx);
}

// ---- the running vote for parallel streams, state on the device (track_stream_kernels.hip) --------------------------
// true when the slices [off[s], off[s] + len) do not all lie inside [0, total) or two of them overlap
static bool track_slices_bad(const int64_t *off, int n, int64_t len, int64_t total) {
    std::vector<int64_t> sorted(off, off + n);
    std::sort(sorted.begin(), sorted.end());
    for (int s = 0; s < n; ++s) {
        if (sorted[s] < 0 || sorted[s] > total || len > total - sorted[s]) return true;
        if (s > 0 && sorted[s] - sorted[s - 1] < len) return true;
    }
    return false;
}

// the level of what has been heard so far in place of a given one (track_level_kernels.hip): the rule, the streams'
// carried column sums and the optional per-frame output
struct TrackRunning {
    int memory; float floor;
    float *state_dev; int64_t state_floats; const int64_t *state_off;
    float *level_out;
};

// asr_track_stream_gate_dev (level, run == NULL) and asr_track_stream_gate_running_dev (level == NULL, run)
static int track_stream_gate(asr_ctx *ctx, const char *fn, const float *cols_dev, int64_t cols_floats, int n_streams,
                             const int64_t *col_off, const int32_t *n_new, const int64_t *frames_before,
                             const float *level, const TrackRunning *run, int bins, int width, float *tail_dev,
                             int64_t tail_floats, const int64_t *tail_off, float *win_dev, int64_t win_cap,
                             float *m_prob, uint8_t *voiced, int32_t *n_voiced) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_streams < 1 || bins < 1 || width < 8 || width > 128 || cols_floats < 0 || tail_floats < 0 || win_cap < 0)
        return fail(ctx, ASR_ERR_INVALID, "%s: bad sizes n_streams=%d bins=%d width=%d (8..128)", fn,
                    n_streams, bins, width);
    if (!col_off || !n_new || !frames_before || (!level && !run) || !tail_dev || !tail_off || !n_voiced)
        return fail(ctx, ASR_ERR_INVALID, "%s: NULL argument", fn);
    const int64_t state_len = run ? (run->memory > 0 ? run->memory - 1 : 1) : 0;
    if (run && track_running_bad(run->memory, run->floor, width))
        return fail(ctx, ASR_ERR_INVALID, "%s: memory=%d (0, or width=%d..2^20) floor=%g (not NaN, not +inf)", fn,
                    run->memory, width, (double)run->floor);
    if (run && (!run->state_dev || !run->state_off || run->state_floats < 0))
        return fail(ctx, ASR_ERR_INVALID, "%s: NULL argument", fn);
    std::vector<asr::TrackStreamRec> recs(n_streams);
    int64_t total = 0, total_ext = 0;
    for (int s = 0; s < n_streams; ++s) {
        if (n_new[s] < 0 || frames_before[s] < 0 || col_off[s] < 0 || col_off[s] > cols_floats ||
            (int64_t)bins * n_new[s] > cols_floats - col_off[s])
            return fail(ctx, ASR_ERR_INVALID,
                        "%s: stream %d (%d x %d at %lld, %lld frames before) lies outside the "
                        "%lld-float buffer", fn, s, bins, n_new[s], (long long)col_off[s], (long long)frames_before[s],
                        (long long)cols_floats);
        asr::TrackStreamRec &R = recs[s];
        R.col_off = col_off[s]; R.tail_off = tail_off[s]; R.frames_before = frames_before[s];
        R.first = total; R.ext_first = total_ext; R.n_new = n_new[s]; R.level = level ? level[s] : 0.0f;
        total += n_new[s];
        if (n_new[s] > 0) total_ext += (int64_t)(width - 1) + n_new[s];
        if (total > INT32_MAX / 2) return fail(ctx, ASR_ERR_INVALID, "%s: more than 2^30 - 1 frames", fn);
    }
    if (track_slices_bad(tail_off, n_streams, (int64_t)bins * (width - 1), tail_floats))
        return fail(ctx, ASR_ERR_INVALID,
                    "%s: a tail (%d x %d) lies outside the %lld-float buffer or two tails overlap", fn,
                    bins, width - 1, (long long)tail_floats);
    if (run && track_slices_bad(run->state_off, n_streams, state_len, run->state_floats))
        return fail(ctx, ASR_ERR_INVALID,
                    "%s: a level state (%lld floats) lies outside the %lld-float buffer or two level states overlap", fn,
                    (long long)state_len, (long long)run->state_floats);
    if (total > win_cap)
        return fail(ctx, ASR_ERR_INVALID, "%s: %lld new frames for %lld windows", fn, (long long)total,
                    (long long)win_cap);
    if (total > 0 && (!cols_dev || !win_dev || !m_prob || !voiced))
        return fail(ctx, ASR_ERR_INVALID, "%s: NULL argument", fn);
    if (total == 0) {
        memset(n_voiced, 0, (size_t)n_streams * sizeof(int32_t));
        return ASR_OK;
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    // results (one download): m_prob | n_voiced | voiced (| level per frame); then the stream table, the column sums and
    // the window slots (and the level's sequence table, suffix maxima and carried maxima)
    const size_t T = (size_t)total, o_nv = T * 4, o_voiced = o_nv + (size_t)n_streams * 4;
    const size_t o_lvl = dtw_align(o_voiced + T), res_bytes = run ? o_lvl + T * 4 : o_voiced + T;
    const size_t o_recs = dtw_align(res_bytes), o_colsum = dtw_align(o_recs + recs.size() * sizeof(asr::TrackStreamRec));
    const size_t o_slot = dtw_align(o_colsum + (size_t)total_ext * 4);
    size_t need = o_slot + (T + 1) * 4, o_seqs = 0, o_sfx = 0, o_last = 0;
    std::vector<asr::TrackLevelSeq> seqs;
    if (run) {
        seqs.resize(n_streams);
        int64_t sfx = 0;
        for (int s = 0; s < n_streams; ++s) {
            asr::TrackLevelSeq &Q = seqs[s];
            Q.cs_first = recs[s].ext_first + (width - 1); Q.out_first = recs[s].first; Q.sfx_first = sfx;
            Q.state_off = run->state_off[s]; Q.frames_before = frames_before[s]; Q.n_new = n_new[s];
            Q.n_hist = (int32_t)std::min<int64_t>(frames_before[s], state_len);
            if (n_new[s] > 0 && run->memory > 0) sfx += (int64_t)Q.n_hist + n_new[s];
        }
        o_seqs = dtw_align(need); o_sfx = dtw_align(o_seqs + seqs.size() * sizeof(asr::TrackLevelSeq));
        o_last = dtw_align(o_sfx + (size_t)sfx * 4);
        need = o_last + (size_t)n_streams * 4;
    }
    rc = track_ws(ctx, need);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_recs, recs.data(), recs.size() * sizeof(asr::TrackStreamRec), hipMemcpyHostToDevice,
                                ctx->stream));
    asr::TrackStreamGateArgs a;
    a.cols = cols_dev; a.tail = tail_dev; a.recs = (const asr::TrackStreamRec *)(ws + o_recs); a.n_streams = n_streams;
    a.total_frames = total; a.total_ext = total_ext; a.bins = bins; a.width = width;
    a.colsum = (float *)(ws + o_colsum); a.slot = (int32_t *)(ws + o_slot); a.win = win_dev;
    a.m_prob = (float *)ws; a.voiced = (uint8_t *)(ws + o_voiced); a.n_voiced = (int32_t *)(ws + o_nv);
    asr::TrackLevelArgs l;
    if (!run) {
        ProfScope ps(ctx, "track_stream_gate", 0, 0.0, 4.0 * (double)total_ext * bins);
        ASR_HIP(ctx, asr::launch_track_stream_gate(ctx->stream, a));
    } else {
        ASR_HIP(ctx, hipMemcpyAsync(ws + o_seqs, seqs.data(), seqs.size() * sizeof(asr::TrackLevelSeq),
                                    hipMemcpyHostToDevice, ctx->stream));
        l.colsum = a.colsum; l.seqs = (const asr::TrackLevelSeq *)(ws + o_seqs); l.n_seq = n_streams;
        l.memory = run->memory; l.floor = run->floor; l.state = run->state_dev;
        l.suffix = (float *)(ws + o_sfx); l.last = (float *)(ws + o_last); l.level = (float *)(ws + o_lvl);
        ProfScope ps(ctx, "track_stream_gate_running", 0, 0.0, 4.0 * (double)total_ext * bins);
        ASR_HIP(ctx, asr::launch_track_stream_colsum(ctx->stream, a));
        ASR_HIP(ctx, asr::launch_track_level(ctx->stream, l));
        ASR_HIP(ctx, asr::launch_track_stream_gate_running(ctx->stream, a, l.level));
    }
    {   // bytes: every new frame voiced
        ProfScope ps(ctx, "track_stream_windows", 0, 0.0, 4.0 * (double)total * bins * width);
        ASR_HIP(ctx, asr::launch_track_stream_windows(ctx->stream, a));
    }
    if (run) ASR_HIP(ctx, asr::launch_track_level_state(ctx->stream, l));  // behind every reader of the carried values
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // (also: `recs` was read by the upload)
    memcpy(m_prob, host.data(), T * 4);
    memcpy(n_voiced, host.data() + o_nv, (size_t)n_streams * 4);
    memcpy(voiced, host.data() + o_voiced, T);
    if (run && run->level_out) memcpy(run->level_out, host.data() + o_lvl, T * 4);
    return mark_main(ctx);
}

int asr_track_stream_gate_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                              const int64_t *col_off, const int32_t *n_new, const int64_t *frames_before,
                              const float *level, int bins, int width, float *tail_dev, int64_t tail_floats,
                              const int64_t *tail_off, float *win_dev, int64_t win_cap, float *m_prob, uint8_t *voiced,
                              int32_t *n_voiced) {
    return track_stream_gate(ctx, "asr_track_stream_gate_dev", cols_dev, cols_floats, n_streams, col_off, n_new,
                             frames_before, level, nullptr, bins, width, tail_dev, tail_floats, tail_off, win_dev, win_cap,
                             m_prob, voiced, n_voiced);
}

int asr_track_stream_gate_running_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                                      const int64_t *col_off, const int32_t *n_new, const int64_t *frames_before,
                                      int memory, float floor, int bins, int width, float *tail_dev, int64_t tail_floats,
                                      const int64_t *tail_off, float *level_dev, int64_t level_floats,
                                      const int64_t *level_off, float *win_dev, int64_t win_cap, float *m_prob,
                                      uint8_t *voiced, int32_t *n_voiced, float *level) {
    const TrackRunning run = {memory, floor, level_dev, level_floats, level_off, level};
    return track_stream_gate(ctx, "asr_track_stream_gate_running_dev", cols_dev, cols_floats, n_streams, col_off, n_new,
                             frames_before, nullptr, &run, bins, width, tail_dev, tail_floats, tail_off, win_dev, win_cap,
                             m_prob, voiced, n_voiced);
}


int asr_track_stream_vote_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_rows, int n_streams,
                              const int32_t *row_count, const int64_t *voiced_before, int n_candidates,
                              int running_frames, const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k,
                              int32_t *hist_dev, int64_t hist_len, const int64_t *hist_off, int32_t *pieces,
                              int32_t *counts, int32_t *n_out) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_streams < 1 || n_rows < 0 || n_rows > INT32_MAX || top_k < 1 || top_k > 64 || n_candidates < 1 ||
        running_frames < 1 || n_db < n_candidates || n_db > INT32_MAX || n_pieces < 1 || n_pieces > (1 << 30) ||
        n_rows > (INT64_MAX / 4) / n_candidates || hist_len < 0 ||
        (int64_t)(running_frames - 1) > (INT64_MAX / 4) / n_candidates)
        return fail(ctx, ASR_ERR_INVALID,
                    "asr_track_stream_vote_dev: bad sizes n_rows=%lld n_streams=%d n_candidates=%d running_frames=%d "
                    "n_db=%lld n_pieces=%d top_k=%d (1..64)", (long long)n_rows, n_streams, n_candidates, running_frames,
                    (long long)n_db, n_pieces, top_k);
    const int64_t keep = running_frames - 1, slice = keep * n_candidates;
    if (!row_count || !voiced_before || (keep > 0 && (!hist_dev || !hist_off)))
        return fail(ctx, ASR_ERR_INVALID, "asr_track_stream_vote_dev: NULL argument");
    const int64_t seg_frames = std::max<int64_t>(1, dtw_env("ASR_TRACK_SEG_FRAMES", 64));
    std::vector<asr::TrackStreamSeg> segs;
    std::vector<asr::TrackStreamKeep> keeps;
    int64_t row0 = 0;
    for (int s = 0; s < n_streams; ++s) {
        if (row_count[s] < 0 || voiced_before[s] < 0 || row_count[s] > n_rows - row0 ||
            voiced_before[s] > INT64_MAX / 2)
            return fail(ctx, ASR_ERR_INVALID, "asr_track_stream_vote_dev: stream %d: %d rows from row %lld of %lld, %lld before",
                        s, row_count[s], (long long)row0, (long long)n_rows, (long long)voiced_before[s]);
        const int64_t off = keep > 0 ? hist_off[s] : 0;
        for (int64_t f = 0; f < row_count[s]; f += seg_frames) {
            asr::TrackStreamSeg S;
            S.row0 = row0; S.v0 = voiced_before[s] + f; S.vb = voiced_before[s]; S.hist_off = off;
            S.n = (int32_t)std::min<int64_t>(seg_frames, row_count[s] - f); S.pad = 0;
            segs.push_back(S);
        }
        if (keep > 0 && row_count[s] > 0) {
            asr::TrackStreamKeep K;
            K.row0 = row0; K.vb = voiced_before[s]; K.hist_off = off; K.n_new = row_count[s]; K.pad = 0;
            keeps.push_back(K);
        }
        row0 += row_count[s];
    }
    if (row0 != n_rows)
        return fail(ctx, ASR_ERR_INVALID, "asr_track_stream_vote_dev: the row counts add up to %lld, not n_rows=%lld",
                    (long long)row0, (long long)n_rows);
    if (keep > 0 && track_slices_bad(hist_off, n_streams, slice, hist_len))
        return fail(ctx, ASR_ERR_INVALID,
                    "asr_track_stream_vote_dev: a history (%lld x %d) lies outside the %lld entries or two overlap",
                    (long long)keep, n_candidates, (long long)hist_len);
    if (n_rows == 0) return ASR_OK;
    if (!idx_dev || !ids_dev || !pieces || !counts || !n_out)
        return fail(ctx, ASR_ERR_INVALID, "asr_track_stream_vote_dev: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;

    // the debug switches and the workspace bound of asr_track_vote_batch_dev
    const int64_t lds_pieces = std::min<int64_t>(asr::TRACK_LDS_PIECES, dtw_env("ASR_TRACK_LDS_PIECES", 1 << 30));
    const bool global_path = n_pieces > lds_pieces;
    const size_t budget = (size_t)std::max<int64_t>(dtw_env("ASR_VOTE_BUDGET_MB", 1024), 1) << 20;
    int64_t grid = std::min<int64_t>((int64_t)segs.size(), 65536);
    if (global_path) grid = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(grid, 4096), budget / ((size_t)n_pieces * 4)));

    // results block (one download): pieces | counts (n_rows x top_k) | n_out; then the two tables and the counters
    const size_t E = (size_t)n_rows, EK = E * (size_t)top_k;
    const size_t o_counts = EK * 4, o_nout = 2 * EK * 4, res_bytes = o_nout + E * 4;
    const size_t o_segs = dtw_align(res_bytes), o_keeps = dtw_align(o_segs + segs.size() * sizeof(asr::TrackStreamSeg));
    const size_t o_hist = dtw_align(o_keeps + keeps.size() * sizeof(asr::TrackStreamKeep));
    rc = track_ws(ctx, o_hist + (global_path ? (size_t)grid * n_pieces * 4 : 0));
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws + o_segs, segs.data(), segs.size() * sizeof(asr::TrackStreamSeg), hipMemcpyHostToDevice,
                                ctx->stream));
    if (!keeps.empty())
        ASR_HIP(ctx, hipMemcpyAsync(ws + o_keeps, keeps.data(), keeps.size() * sizeof(asr::TrackStreamKeep),
                                    hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "track_stream_vote", 0, 0.0, 4.0 * (double)n_rows * n_candidates + 8.0 * (double)EK);
        asr::TrackStreamVoteArgs a;
        a.idx = idx_dev; a.segs = (const asr::TrackStreamSeg *)(ws + o_segs); a.n_segs = (int64_t)segs.size();
        a.n_rows = n_rows; a.keeps = (const asr::TrackStreamKeep *)(ws + o_keeps); a.n_keep = (int)keeps.size();
        a.n_candidates = n_candidates; a.running_frames = running_frames;
        a.ids = ids_dev; a.n_db = n_db; a.n_pieces = n_pieces; a.top_k = top_k;
        a.ring = hist_dev;
        a.pieces = (int32_t *)ws; a.counts = (int32_t *)(ws + o_counts); a.n_out = (int32_t *)(ws + o_nout);
        a.hist_ws = (int32_t *)(ws + o_hist);
        ASR_HIP(ctx, asr::launch_track_stream_vote(ctx->stream, a, (int)grid, global_path));
    }
    std::vector<char> host(res_bytes);
    ASR_HIP(ctx, hipMemcpyAsync(host.data(), ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // (also: the tables were read by the uploads)
    memcpy(pieces, host.data(), EK * 4);
    memcpy(counts, host.data() + o_counts, EK * 4);
    memcpy(n_out, host.data() + o_nout, E * 4);
    return mark_main(ctx);
}

// ---- score following for parallel streams, state on the device (follow_stream_kernels.hip) ---------------------------
int asr_follow_stream_windows_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                                  const int64_t *col_off, const int32_t *n_new, const int64_t *cols_before, int bins,
                                  int width, int step, float *tail_dev, int64_t tail_floats, const int64_t *tail_off,
                                  float *win_dev, int64_t win_cap, int32_t *n_win) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_streams < 1 || bins < 1 || width < 8 || width > 128 || step < 1 || cols_floats < 0 || tail_floats < 0 ||
        win_cap < 0)
        return fail(ctx, ASR_ERR_INVALID,
                    "asr_follow_stream_windows_dev: bad sizes n_streams=%d bins=%d width=%d (8..128) step=%d (>= 1)",
                    n_streams, bins, width, step);
    if (!col_off || !n_new || !cols_before || !tail_dev || !tail_off || !n_win)
        return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_windows_dev: NULL argument");
    std::vector<asr::FollowStreamRec> recs(n_streams);
    std::vector<int32_t> counts(n_streams);
    int64_t total = 0, total_new = 0;
    auto done = [&](int64_t T) { return T < width ? (int64_t)0 : (T - width) / step + 1; };
    for (int s = 0; s < n_streams; ++s) {
        if (n_new[s] < 0 || cols_before[s] < 0 || cols_before[s] > INT64_MAX / 4 || col_off[s] < 0 ||
            col_off[s] > cols_floats || (int64_t)bins * n_new[s] > cols_floats - col_off[s])
            return fail(ctx, ASR_ERR_INVALID,
                        "asr_follow_stream_windows_dev: stream %d (%d x %d at %lld, %lld columns before) lies outside the "
                        "%lld-float buffer", s, bins, n_new[s], (long long)col_off[s], (long long)cols_before[s],
                        (long long)cols_floats);
        const int64_t k0 = done(cols_before[s]), k1 = done(cols_before[s] + n_new[s]);
        asr::FollowStreamRec &R = recs[s];
        R.col_off = col_off[s]; R.tail_off = tail_off[s]; R.first = total; R.n_new = n_new[s];
        R.n_win = (int32_t)(k1 - k0);                         // <= n_new: a window per new column at the most
        R.c0 = k0 * step - cols_before[s] + (width - 1);      // >= 0 where n_win > 0: such a window ends in a new column
        R.has_tail = cols_before[s] > 0 ? 1 : 0; R.pad = 0;
        counts[s] = R.n_win;
        total += R.n_win;
        total_new += n_new[s];
        if (total_new > INT32_MAX / 2)
            return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_windows_dev: more than 2^30 - 1 columns");
    }
    if (track_slices_bad(tail_off, n_streams, (int64_t)bins * (width - 1), tail_floats))
        return fail(ctx, ASR_ERR_INVALID,
                    "asr_follow_stream_windows_dev: a tail (%d x %d) lies outside the %lld-float buffer or two tails overlap",
                    bins, width - 1, (long long)tail_floats);
    if (total > win_cap)
        return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_windows_dev: %lld windows for a buffer of %lld",
                    (long long)total, (long long)win_cap);
    if ((total_new > 0 && !cols_dev) || (total > 0 && !win_dev))
        return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_windows_dev: NULL argument");
    memcpy(n_win, counts.data(), (size_t)n_streams * sizeof(int32_t));
    if (total_new == 0) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = track_ws(ctx, recs.size() * sizeof(asr::FollowStreamRec));
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws, recs.data(), recs.size() * sizeof(asr::FollowStreamRec), hipMemcpyHostToDevice,
                                ctx->stream));
    asr::FollowStreamWinArgs a;
    a.cols = cols_dev; a.tail = tail_dev; a.win = win_dev; a.recs = (const asr::FollowStreamRec *)ws;
    a.n_streams = n_streams; a.total_win = total; a.bins = bins; a.width = width; a.step = step;
    {   // bytes: the windows and the tails written
        ProfScope ps(ctx, "follow_stream_windows", 0, 0.0,
                     4.0 * ((double)total * bins * width + (double)n_streams * bins * (width - 1)));
        ASR_HIP(ctx, asr::launch_follow_stream_windows(ctx->stream, a));
    }
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // `recs` was read by the upload
    return mark_main(ctx);
}

int asr_follow_stream_log_dev(asr_ctx *ctx, const float *codes_dev, int64_t n_rows, int n_streams,
                              const int32_t *row_count, const int32_t *rows_in_log, int keep, int dim, float *log_dev,
                              int64_t log_floats, const int64_t *log_off) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_streams < 1 || n_rows < 0 || n_rows > INT32_MAX || keep < 0 || dim < 1 || dim > 64 || log_floats < 0)
        return fail(ctx, ASR_ERR_INVALID,
                    "asr_follow_stream_log_dev: bad sizes n_rows=%lld n_streams=%d keep=%d (>= 0) dim=%d (1..64)",
                    (long long)n_rows, n_streams, keep, dim);
    if (!row_count || !rows_in_log || !log_dev || !log_off)
        return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_log_dev: NULL argument");
    std::vector<asr::FollowStreamLogRec> recs(n_streams);
    std::vector<std::pair<int64_t, int64_t>> regions(n_streams);                   // (first float, floats)
    int64_t row0 = 0;
    for (int s = 0; s < n_streams; ++s) {
        if (row_count[s] < 0 || rows_in_log[s] < 0 || row_count[s] > n_rows - row0)
            return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_log_dev: stream %d: %d rows from row %lld of %lld, %d in the log",
                        s, row_count[s], (long long)row0, (long long)n_rows, rows_in_log[s]);
        const int64_t kept = std::min<int64_t>(rows_in_log[s], keep);
        const int64_t need = std::max<int64_t>(rows_in_log[s], kept + row_count[s]) * dim;
        if (log_off[s] < 0 || log_off[s] > log_floats || need > log_floats - log_off[s])
            return fail(ctx, ASR_ERR_INVALID,
                        "asr_follow_stream_log_dev: the log of stream %d (%lld floats at %lld) lies outside the %lld-float buffer",
                        s, (long long)need, (long long)log_off[s], (long long)log_floats);
        asr::FollowStreamLogRec &R = recs[s];
        R.log_off = log_off[s]; R.src_row = row0; R.rows_in_log = rows_in_log[s]; R.kept = (int32_t)kept;
        R.n_new = row_count[s]; R.pad = 0;
        regions[s] = std::make_pair(log_off[s], need);
        row0 += row_count[s];
    }
    if (row0 != n_rows)
        return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_log_dev: the row counts add up to %lld, not n_rows=%lld",
                    (long long)row0, (long long)n_rows);
    std::sort(regions.begin(), regions.end());
    for (int s = 1; s < n_streams; ++s)
        if (regions[s].first - regions[s - 1].first < regions[s - 1].second)
            return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_log_dev: two logs overlap (at floats %lld and %lld)",
                        (long long)regions[s - 1].first, (long long)regions[s].first);
    if (n_rows == 0) return ASR_OK;
    if (!codes_dev) return fail(ctx, ASR_ERR_INVALID, "asr_follow_stream_log_dev: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = track_ws(ctx, recs.size() * sizeof(asr::FollowStreamLogRec));
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->vote_ws;
    ASR_HIP(ctx, hipMemcpyAsync(ws, recs.data(), recs.size() * sizeof(asr::FollowStreamLogRec), hipMemcpyHostToDevice,
                                ctx->stream));
    asr::FollowStreamLogArgs a;
    a.codes = codes_dev; a.log = log_dev; a.recs = (const asr::FollowStreamLogRec *)ws; a.n_streams = n_streams;
    a.dim = dim; a.n_rows = n_rows;
    {   // bytes: the new rows written (the kept rows move only where a log is full)
        ProfScope ps(ctx, "follow_stream_log", 0, 0.0, 4.0 * (double)n_rows * dim);
        ASR_HIP(ctx, asr::launch_follow_stream_log(ctx->stream, a));
    }
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));    // `recs` was read by the upload
    return mark_main(ctx);
}

int asr_topk(asr_ctx *ctx, const float *db, int64_t n_db, int64_t ld_db, const float *q, int64_t n_q, int64_t ld_q,
             int dim, int k, int64_t idx_offset, int32_t *idx, double *dist) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_db < 0 || n_q < 0 || ld_db < 1 || ld_q < 1 || k < 1) return fail(ctx, ASR_ERR_INVALID, "topk: bad sizes");
    if (n_q == 0) return ASR_OK;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float *d_db = nullptr, *d_q = nullptr;
    int32_t *d_idx = nullptr;
    double *d_dist = nullptr;
    auto cleanup = [&]() { (void)hipFree(d_db); (void)hipFree(d_q); (void)hipFree(d_idx); (void)hipFree(d_dist); };
#define TOPK_HIP(call)                                                                               \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            cleanup();                                                                               \
            return fail(ctx, ASR_ERR_HIP, "asr_topk: %s failed: %s", #call, hipGetErrorString(e__)); \
        }                                                                                            \
    } while (0)
    TOPK_HIP(hipMalloc((void **)&d_db, (size_t)std::max<int64_t>(n_db, 1) * ld_db * sizeof(float)));
    TOPK_HIP(hipMalloc((void **)&d_q, (size_t)n_q * ld_q * sizeof(float)));
    TOPK_HIP(hipMalloc((void **)&d_idx, (size_t)n_q * k * sizeof(int32_t)));
    TOPK_HIP(hipMalloc((void **)&d_dist, (size_t)n_q * k * sizeof(double)));
    if (n_db > 0) TOPK_HIP(hipMemcpyAsync(d_db, db, (size_t)n_db * ld_db * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TOPK_HIP(hipMemcpyAsync(d_q, q, (size_t)n_q * ld_q * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    int rc = asr_topk_dev(ctx, d_db, n_db, ld_db, d_q, n_q, ld_q, dim, k, idx_offset, d_idx, d_dist);
    if (rc != ASR_OK) { cleanup(); return rc; }
    TOPK_HIP(hipMemcpyAsync(idx, d_idx, (size_t)n_q * k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TOPK_HIP(hipMemcpyAsync(dist, d_dist, (size_t)n_q * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TOPK_HIP(hipStreamSynchronize(ctx->stream));
#undef TOPK_HIP
    cleanup();
    return ASR_OK;
}

}  // extern "C"
