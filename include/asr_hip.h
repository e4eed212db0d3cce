/* asr_hip.h - C ABI of libasr_hip.so, the MI355X (gfx950) implementation of the
 * audio<->sheet retrieval hot path of CPJKU/audio_sheet_retrieval.
 *
 * The reference has no FFI; its seam is Python-level: Theano
 * "compiled callables" on C-contiguous NCHW NumPy arrays plus Lasagne's
 * get/set_all_param_values.  Every entry point below names the reference
 * interface it replaces (paths relative to audio_sheet_retrieval/).  The
 * Python host code binds these with ctypes (audio_sheet_retrieval_amd/_lib.py,
 * INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns ASR_OK (0) or an ASR_ERR_* code; no exceptions
 *     cross the ABI; asr_last_error() gives the message of the last failure;
 *   - host buffers are caller-owned, C-contiguous; "_dev" variants take
 *     device pointers obtained from asr_dev_alloc (plain void*);
 *   - one asr_ctx is used from one thread at a time (the reference's compiled
 *     functions are not re-entrant either); distinct contexts are independent;
 *   - all work is enqueued on the context's own HIP stream; host-buffer
 *     variants return after the results are in the caller's memory,
 *     "_dev" variants return after enqueueing (call asr_sync()).
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_OK           0
#define ASR_ERR_INVALID  1   /* bad argument                                  */
#define ASR_ERR_HIP      2   /* HIP runtime / kernel launch failure           */
#define ASR_ERR_STATE    3   /* call order (e.g. embed before set_params)     */
#define ASR_ERR_COMM     4   /* RCCL failure                                  */
#define ASR_ERR_NOMEM    5

typedef struct asr_ctx asr_ctx;

/* Model hyper-parameters = the module constants of
 * models/mutopia_ccal_cont.py:23-51 (and _rsz.py) + geometry from
 * exp_configs/mutopia_full_aug.yaml:1-4. */
typedef struct asr_config {
    int32_t struct_size;    /* sizeof(asr_config): ABI check                   */
    int32_t device;         /* HIP device ordinal (reference: THEANO_FLAGS)    */
    int32_t num_filters;    /* num_filters_1: 12 (cont :74) or 24 (rsz :77)    */
    int32_t resize_view1;   /* 1 = rsz prepare: halve the sheet (rsz :179-185) */
    int32_t h1, w1;         /* raw sheet snippet, 160 x 200                    */
    int32_t h2, w2;         /* spectrogram excerpt, 92 x 42                    */
    int32_t dim_latent;     /* DIM_LATENT = 32 (:35); only 32 is supported     */
    int32_t max_chunk;      /* samples per internal launch, 0 = default        */
    float r1, r2, rT;       /* CCALayer regularisers (:42-43)                  */
    float alpha;            /* CCALayer running-average factor ALPHA (:49)     */
    float gamma;            /* ranking-loss margin GAMMA (:51)                 */
    float l2;               /* weight decay L2 (:39)                           */
    /* Gradient of MaxPool2DLayer (models/mutopia_ccal_cont.py:79,83,87,91,104,108,
     * 112,116) at windows with several equal maxima.  ASR_POOL_TIES_ALL (0, the
     * default): every element equal to the window maximum receives the upstream
     * gradient - Theano's CPU MaxPoolGrad, the path the reference's CPU runs take.
     * ASR_POOL_TIES_FIRST (1): only the first one in row-major order (what a
     * cuDNN-style pooling backward does; unverified offline).  Added in round 5:
     * a caller that passes the 64-byte struct of the earlier ABI gets 0.
     * "Equal" is decided on the float32 BatchNorm output y, BEFORE the ELU; the
     * reference pools float32 elu(y).  ELU is monotone (same maximum) but not
     * injective in float32 for y < 0 (about five neighbouring floats share an
     * image near y = -3; everything below about -17 is -1.0f): distinct y that tie
     * only after the ELU receive the gradient in the reference and not here.
     * The additional gradient is scaled by ELU'(y) = exp(y) <= 1; tied windows of
     * blank paper are bit-identical patches and tie either way (0 windows differ
     * on the synthetic and mostly-blank pages: oracle/train.py:elu_tie_deviation,
     * tests/test_oracle_train.py::test_ties_decided_before_or_after_the_float32_elu). */
    int32_t pool_ties;
} asr_config;
#define ASR_POOL_TIES_ALL   0
#define ASR_POOL_TIES_FIRST 1
#define ASR_CONFIG_SIZE_V1  64   /* sizeof(asr_config) before pool_ties existed */

/* ---- life cycle ------------------------------------------------------- */
/* build_model() (models/mutopia_ccal_cont.py:61-149): allocates the network
 * state on the device.  On failure *out is NULL and asr_last_error(NULL)
 * holds the message. */
int asr_create(const asr_config *cfg, asr_ctx **out);
void asr_destroy(asr_ctx *ctx);
const char *asr_last_error(const asr_ctx *ctx);
const char *asr_version(void);
int asr_sync(asr_ctx *ctx);                      /* wait for the ctx stream     */
/* The reference network is shape-agnostic (GlobalPoolLayer,
 * models/mutopia_ccal_cont.py:96,121; INPUT_SHAPE_1 is declared 120x200 but fed
 * 160x200).  Changes the raw input size of `view` (1|2): launch
 * plans are re-derived, activation buffers re-allocated on the next embed. */
int asr_set_input_size(asr_ctx *ctx, int view, int h, int w);

/* ---- parameters --------------------------------------------------------
 * lasagne.layers.get_all_param_values / set_all_param_values on the layer
 * list (utils/train_dcca_pool.py:395-401, run_eval.py:74-82,
 * retrieval_wrapper.py:27-29): a flat list of 97 float32 arrays,
 *   tower 1 blocks 1..9: W (O,I,kh,kw), beta, gamma, mean, inv_std   [0..44]
 *   tower 2 likewise                                                 [45..89]
 *   CCALayer U, V, mean1, mean2, S12, S11, S22 (layers/cca.py:69-77) [90..96]
 * The library repacks W (filter flip + MFMA fragment order) internally. */
int asr_param_count(const asr_ctx *ctx);
int asr_param_size(const asr_ctx *ctx, int index, int64_t *n_elements);
int asr_set_params(asr_ctx *ctx, const float *const *arrays, const int64_t *sizes, int n_arrays);
int asr_get_params(asr_ctx *ctx, float *const *arrays, const int64_t *sizes, int n_arrays);
/* refine_cca.py:104-107: cca_layer.mean1/mean2/U/V.set_value(...) */
int asr_set_cca(asr_ctx *ctx, const float *U, const float *V, const float *mean1, const float *mean2);

/* ---- embedding (deterministic forward) ----------------------------------
 * compute_v1_latent / compute_v2_latent (run_eval.py:92-95,
 * retrieval_wrapper.py:33-38) when out_kind = ASR_OUT_LATENT: tower -> CCALayer
 * deterministic branch (layers/cca.py:185-201) -> LengthNormLayer (:39-40);
 * the tower-only functions of refine_cca.py:86-89 when ASR_OUT_FEATURES.
 * View-1 input modes fold model.prepare (models/mutopia_ccal_cont.py:170-190)
 * into the first kernel:
 *   ASR_IN_F32_PREPARED  float32 (n,1,H,W) already /255 (and halved for rsz):
 *                        exactly what the reference's compiled function takes;
 *   ASR_IN_F32_RAW       float32 (n,1,h1,w1) holding 0..255 (pool output);
 *   ASR_IN_U8_RAW        uint8   (n,1,h1,w1) (what the servers pass,
 *                        audio_sheet_server.py:331,472).
 * out: (n, 32) float32. */
#define ASR_IN_F32_PREPARED 0
#define ASR_IN_F32_RAW      1
#define ASR_IN_U8_RAW       2
#define ASR_OUT_LATENT      0
#define ASR_OUT_FEATURES    1
int asr_embed_view1(asr_ctx *ctx, const void *x, int in_mode, int64_t n, int out_kind, float *out);
int asr_embed_view2(asr_ctx *ctx, const float *z, int64_t n, int out_kind, float *out);
int asr_embed_view1_dev(asr_ctx *ctx, const void *x_dev, int in_mode, int64_t n, int out_kind, float *out_dev);
int asr_embed_view2_dev(asr_ctx *ctx, const float *z_dev, int64_t n, int out_kind, float *out_dev);
/* compute_output of create_iter_functions (utils/train_dcca_pool.py:158): both views of the same n pairs in one call
 * -> [v1 latent, v2 latent].  Equivalent to asr_embed_view1 + asr_embed_view2. */
int asr_embed_both(asr_ctx *ctx, const void *x, int in_mode, const float *z, int64_t n, int out_kind,
                   float *out1, float *out2);

/* ---- ranking --------------------------------------------------------------
 * eval_retrieval (utils/train_dcca_pool.py:28-82): float64 cosine distances
 * (scipy cdist order, see oracle/retrieval.py) of lv1 (n1,dim) vs lv2 (n2,dim)
 * and, per query i, the 1-based rank of its correct item in a stable ascending
 * sort, computed by counting instead of sorting:
 *    k = n2 / n1_global if n2 > n1_global else 1   (:35)
 *    h = n1_global / n2 if n1_global > n2 else 1   (:36)
 *    correct(i) = { j : j / k == (i + query_offset) / h }
 *    d*   = min_{j in correct(i)} d_ij , j* the first index attaining it
 *    rank = 1 + #{ j : d_ij < d* } + #{ j < j* : d_ij == d* }
 * dstar[i] = d* (= diag(dists) for equal list sizes, :77), ties[i] = number of
 * other candidates with d_ij == d*.  ld1/ld2: row strides in floats (>= dim;
 * run_eval.py:160-162 clips dimensions by slicing columns).
 * query_offset / n1_global describe a shard of the query list (multi-GPU);
 * pass 0 / n1 for the single-device case.  Any output pointer may be NULL. */
int asr_rank(asr_ctx *ctx, const float *lv1, int64_t n1, int64_t ld1,
             const float *lv2, int64_t n2, int64_t ld2, int dim,
             int64_t query_offset, int64_t n1_global,
             int32_t *ranks, double *dstar, int32_t *ties);
int asr_rank_dev(asr_ctx *ctx, const float *lv1_dev, int64_t n1, int64_t ld1,
                 const float *lv2_dev, int64_t n2, int64_t ld2, int dim,
                 int64_t query_offset, int64_t n1_global,
                 int32_t *ranks_dev, double *dstar_dev, int32_t *ties_dev);

/* ---- top-k retrieval ---------------------------------------------------------
 * _retrieve_sheet_snippet_ids / _retrieve_perform_excerpt_ids
 * (audio_sheet_server.py:530-563): dists = cdist(db_codes, query, "cosine");
 * sorted_idx = argsort(dists)[:n_candidates].  For every query row of q
 * (n_q, dim) the k smallest float64 cosine distances to db (n_db, dim) in
 * ascending order, ties by ascending index (= NumPy's stable argsort);
 * idx[i*k + r] = index + idx_offset (int32; -1 and dist = +inf when n_db < k).
 * idx_offset makes the indices global when db is one shard of a larger pool
 * (multi-GPU: per-shard top-k, then a k-way merge of the gathered lists).
 * k <= 128, dim <= 64. */
int asr_topk(asr_ctx *ctx, const float *db, int64_t n_db, int64_t ld_db,
             const float *q, int64_t n_q, int64_t ld_q, int dim, int k,
             int64_t idx_offset, int32_t *idx, double *dist);
int asr_topk_dev(asr_ctx *ctx, const float *db_dev, int64_t n_db, int64_t ld_db,
                 const float *q_dev, int64_t n_q, int64_t ld_q, int dim, int k,
                 int64_t idx_offset, int32_t *idx_dev, double *dist_dev);

/* ---- resident code data base ------------------------------------------------------
 * The reference's server loads its code data base ONCE (audio_sheet_server.py:496-522 load_*_db_file ->
 * self.sheet_snippet_codes / self.spec_codes) and queries it for every incoming frame (:530-563
 * _retrieve_*_ids_for_*: cdist against the whole data base -> argsort[:n_candidates]); eval_retrieval
 * (utils/train_dcca_pool.py:40-74) likewise derives the top ranks AND the rank of the correct item from one
 * distance row.  An asr_db holds what such a data base needs beyond its rows, computed once instead of per
 * call: float64 row norms, their fp32 reciprocals and (32-d packed rows) a unit-length fp32 copy the MFMA
 * filter stages read.  codes_dev (n, ld) float32 stays OWNED BY THE CALLER and must outlive the handle; after
 * changing rows in place (e.g. an all-gather landing new shards in the same buffer) call asr_db_refresh.
 *   asr_topk_db_dev       = asr_topk_dev against the data base (same results, bit for bit)
 *   asr_rank_db_dev       = asr_rank_dev with the data base as the candidate side
 *   asr_topk_rank_db_dev  = both for the same queries from ONE walk over the pool: every 16 x 16 tile of fp32
 *                           cosines feeds the top-k candidate buffers and the rank counters (n >= 16384, 32-d
 *                           packed rows; otherwise the two passes run back to back).  Results identical to
 *                           the two separate calls.
 * query_offset / n1_global as in asr_rank_dev.  A handle belongs to the context that created it. */
typedef struct asr_db asr_db;
int asr_db_create(asr_ctx *ctx, const float *codes_dev, int64_t n, int64_t ld, int dim, asr_db **out);
int asr_db_refresh(asr_ctx *ctx, asr_db *db);
int asr_db_destroy(asr_ctx *ctx, asr_db *db);
int asr_db_size(asr_ctx *ctx, const asr_db *db, int64_t *n, int *dim);
int asr_topk_db_dev(asr_ctx *ctx, const asr_db *db, const float *q_dev, int64_t n_q, int64_t ld_q, int k,
                    int64_t idx_offset, int32_t *idx_dev, double *dist_dev);
int asr_rank_db_dev(asr_ctx *ctx, const asr_db *db, const float *lv1_dev, int64_t n1, int64_t ld1,
                    int64_t query_offset, int64_t n1_global, int32_t *ranks_dev, double *dstar_dev, int32_t *ties_dev);
int asr_topk_rank_db_dev(asr_ctx *ctx, const asr_db *db, const float *q_dev, int64_t n_q, int64_t ld_q, int k,
                         int64_t idx_offset, int32_t *idx_dev, double *dist_dev, int64_t query_offset,
                         int64_t n1_global, int32_t *ranks_dev, double *dstar_dev, int32_t *ties_dev);

/* A data base that is one SHARD of a larger pool (rows [item_offset, item_offset + n) of n2_global): the pieces of a
 * QUERY-sharded retrieval.  BASELINE configs[4] ("2M-snippet candidate pool sharded, RCCL all-gather 32-d embeddings,
 * global top-k") can gather the pool's embeddings (256 MB per step) or the QUERIES' (0.5 MB): every rank then searches
 * its own shard for all queries, the k-lists (n_q x k keys) are all-gathered and merged, the rank counters all-reduced
 * (ASR_DTYPE_I32) - the same integers, two orders of magnitude less traffic (bench.py --workload pool2m --exchange queries).
 *   asr_rank_dstar_db_dev : d* and the GLOBAL index j* of queries whose correct candidates (utils/train_dcca_pool.py:
 *                           35-36, 52-55) lie in this shard
 *   asr_topk_count_db_dev : top-k of the queries against the shard (indices + item_offset) and, d* / j* given, their
 *                           rank counters counts[n_q][3] = (#d < d*, #d == d*, #d == d* before j*) over the shard
 *   asr_topk_merge_dev    : the k smallest (distance, index) keys of queries [q_lo, q_lo + n_q) among n_parts lists
 *                           laid out [part][n_q_total][k] (n_parts * k <= 2048)
 *   asr_rank_finish_dev   : ranks = 1 + less + equal-before, ties = equal - 1 from summed counters */
int asr_rank_dstar_db_dev(asr_ctx *ctx, const asr_db *db, const float *q_dev, int64_t n_q, int64_t ld_q, int64_t item_offset,
                          int64_t n2_global, int64_t query_offset, int64_t n1_global, double *dstar_dev, int64_t *jstar_dev);
int asr_topk_count_db_dev(asr_ctx *ctx, const asr_db *db, const float *q_dev, int64_t n_q, int64_t ld_q, int k,
                          int64_t item_offset, int32_t *idx_dev, double *dist_dev, const double *dstar_dev,
                          const int64_t *jstar_dev, int32_t *counts_dev);
int asr_topk_merge_dev(asr_ctx *ctx, const int32_t *part_idx_dev, const double *part_dist_dev, int n_parts,
                       int64_t n_q_total, int64_t q_lo, int64_t n_q, int k, int32_t *idx_dev, double *dist_dev);
int asr_rank_finish_dev(asr_ctx *ctx, const int32_t *counts_dev, const double *dstar_dev, int64_t n, int32_t *ranks_dev,
                        double *dstar_out_dev, int32_t *ties_dev);

/* ---- CCA re-estimation -----------------------------------------------------
 * CCA(method='svd').fit(H1, H2) (utils/cca.py:25-53, 199-211) as driven by
 * refine_cca.py:100-107: float32 means and centring, second moments / (n-1)
 * rounded to float32, + r1/r2 on the diagonal in float64 (regularisers from
 * asr_config), then S11^-1/2, S22^-1/2, T, svd(T) in float64; outputs cast to
 * float32 exactly like refine_cca.py:104-107.  H1, H2: (n,32) float32 pre-CCA
 * tower outputs (ASR_OUT_FEATURES).  U, V: (32,32) row-major; columns are
 * defined up to a JOINT sign per canonical dimension (U[:,j], V[:,j]) ->
 * (-U[:,j], -V[:,j]), which leaves every cross-view cosine score unchanged.
 * coeffs (32 canonical correlations, descending, float64) may be NULL.
 * The result is NOT installed into the context: call asr_set_cca. */
int asr_cca_fit(asr_ctx *ctx, const float *H1, const float *H2, int64_t n,
                float *U, float *V, float *mean1, float *mean2, double *coeffs);
/* device variant: means_dev receives mean1 | mean2 (64 floats) */
int asr_cca_fit_dev(asr_ctx *ctx, const float *H1_dev, const float *H2_dev, int64_t n,
                    float *U_dev, float *V_dev, float *means_dev, double *coeffs_dev);

/* ---- piece identification on top of top-k ------------------------
 * detect_score / detect_performance (audio_sheet_server.py:213-300): n_samples sliding windows of one recording
 * (or one unrolled score) are embedded, each retrieves its n_candidates nearest data-base codes (asr_topk_dev),
 * the piece ids of all retrieved entries are counted and the top_k pieces by votes returned.
 *   asr_slice_windows_dev: out[i,0,r,c] = src[r0 + r, starts[i] + c]; src (rows, T) float32 row-major on the
 *     device, starts: n host int32 (np.linspace(0, T - win_w, n).astype(int), :217-218), out (n,1,win_h,win_w).
 *   asr_piece_vote_dev: idx_dev = the (n_q * k) int32 indices asr_topk_dev wrote (-1 entries ignored), ids_dev[j]
 *     = piece id of data-base entry j (sheet_snippet_ids, :520); pieces/counts (host, top_k): pieces ordered by
 *     votes descending, equal votes: larger piece id first (np.unique + argsort(counts)[::-1], :235-238, whose
 *     tie order NumPy leaves open); *n_out = number of pieces returned (<= top_k, only pieces with votes). */
int asr_slice_windows_dev(asr_ctx *ctx, const float *src_dev, int64_t rows, int64_t T, int r0, int win_h, int win_w,
                          const int32_t *starts, int n, float *out_dev);
int asr_piece_vote_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_idx, const int32_t *ids_dev, int64_t n_db,
                       int32_t n_pieces, int top_k, int32_t *pieces, int32_t *counts, int32_t *n_out);

/* ---- batched piece vote: the full evaluation of audio_sheet_server.py / sheet_audio_server.py --full_eval -----------
 * asr_piece_vote_dev for n_groups query pieces in one launch, each group's result bit-identical with asr_piece_vote_dev
 * on that group's slice.  idx_dev: the (n_groups * per_group) int32 indices of one asr_topk_db_dev / asr_topk_dev call,
 * group g = entries [g * per_group, (g + 1) * per_group) (its n_samples x n_candidates indices); entries -1 or outside
 * [0, n_db) and piece ids outside [0, n_pieces) are ignored.  Outputs (host):
 *   pieces / counts (n_groups x top_k): per group the voted pieces by votes descending, equal votes larger piece id
 *     first; slots past the voted pieces hold piece -1 / count 0.  top_k is not capped (--full_eval: the test pieces);
 *   n_out[g] = min(top_k, number of voted pieces);
 *   with targets (n_groups host int32, or NULL): the reference's full-eval rule (:640-645) - target among the n_out[g]
 *     returned pieces: ranks[g] = position + 1, ratios[g] = its count / sum of the returned counts (float64);
 *     otherwise ranks[g] = n_out[g] (0 for a group without valid votes) and ratios[g] = 0.0.  ranks / ratios may be
 *     NULL without targets.
 * Limits: n_groups, n_db <= 2^31 - 1; 1 <= n_pieces <= 2^30; top_k >= 1.  One workgroup per group; with n_pieces <=
 * 4096 the counters and the bitonic-sorted (count << 32 | piece) keys stay in LDS (48 KiB, any per_group); above that
 * they live in a device workspace of n_pieces * 4 + 8 * pow2ceil(min(n_pieces, per_group)) bytes per group (groups in
 * chunks of ASR_VOTE_BUDGET_MB, default 1024), with the same results.  One launch per chunk, one download; the
 * workspace stays on the context (freed by asr_destroy).  ASR_VOTE_LDS_PIECES=<n> (debug) sends n_pieces > n to the
 * workspace path. */
int asr_piece_vote_batch_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_groups, int64_t per_group,
                             const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k, const int32_t *targets,
                             int32_t *pieces, int32_t *counts, int32_t *n_out, int32_t *ranks, double *ratios);

/* ---- running piece vote: the live loop of audio_sheet_server.py (AudioSheetServer.run, :83-211) over recordings ------
 * The reference slides a (bins, w) window over the spectrogram frame by frame (:110), gates every frame by its music
 * probability (_detect_music, :524-528; :117), embeds the window of a frame with music, retrieves its n_candidates
 * nearest data-base entries (:120-123), keeps the piece ids of the last running_frames such frames (:126-129) and ranks
 * the pieces by their votes over that history (:132-138).  Window cutting, tower and top-k are the existing calls
 * (asr_gather_windows_dev, asr_embed_view2_dev, asr_topk_db_dev); these two are the gate and the sliding vote.
 *
 * asr_track_gate_dev: n_rec recordings (bins[r], frames[r]) float32 row-major at float offsets[r] of src_dev (src_floats
 *   floats; every recording is checked against it).  Per frame i of recording r, concatenated in recording order:
 *     m_prob = clip(mean(colsum[i-w+1 .. i]) / (level * 0.15), 0, 1), colsum[t] = the float32 sum of column t over the
 *       bins, added row after row (zero before the recording's start), the mean as numpy >= 2 computes the float32
 *       .mean() of w values (pairwise sum: eight accumulators over the full blocks of eight, combined ((r0+r1)+(r2+r3))+
 *       ((r4+r5)+(r6+r7)), the remainder added in order; divided by float32(w)), the divisor float32(level *
 *       float32(0.15)); level = max_t colsum[t] (:527), or norm[r] where norm is given and norm[r] is not NaN - what a
 *       stream, which cannot know its maximum, passes.  A silent recording gives 0 / 0 = NaN;
 *     voiced = m_prob > 0.5 and frame0[r] + i >= w (:117; frame0: the stream position of column 0, NULL: 0).
 *   Outputs (host): m_prob (float32) and voiced (bytes), sum(frames) each; level (n_rec, may be NULL): the divisor's
 *   level per recording.  8 <= width <= 128 (numpy sums other lengths in another order), bins, frames >= 1; anything else
 *   returns ASR_ERR_INVALID.  Compiled without contraction: bit-equal with numpy on finite inputs.
 *
 * asr_track_vote_batch_dev: idx_dev = (n_rows x n_candidates) int32 data-base indices, one row per voiced frame (what
 *   asr_topk_db_dev wrote for the voiced frames of all recordings); recording r owns rows row_first[r] .. row_first[r] +
 *   row_count[r] - 1 in frame order; ids_dev[j] = piece id of data-base entry j.  For frame f >= emit_from[r] (NULL: 0)
 *   of recording r the votes of frames max(0, f - running_frames + 1) .. f are counted per piece and the first top_k
 *   pieces with votes returned: votes descending, equal votes the larger piece id first (asr_piece_vote_dev's rule).
 *   Frames before emit_from[r] only feed the history (a stream passes the rows of its last running_frames - 1 voiced
 *   frames in front of the new ones).  Outputs (host), one row per emitted frame in recording order: pieces / counts
 *   (x top_k; piece -1 / count 0 past the voted pieces), n_out = pieces returned.  Indices outside [0, n_db) and piece
 *   ids outside [0, n_pieces) are ignored.  ASR_ERR_INVALID before anything is launched: top_k outside 1..64,
 *   n_candidates < 1, running_frames < 1, n_db < n_candidates, n_pieces < 1 (or > 2^30), a row range outside the table,
 *   emit_from outside [0, row_count].  One wave per segment of 64 frames rebuilds the histogram of the history before
 *   its first frame, then adds the entering and removes the leaving frame's ids per frame; the counters live in LDS up
 *   to n_pieces = 4096 and in a per-workgroup device workspace above (bounded by ASR_VOTE_BUDGET_MB).  Results do not
 *   depend on either; ASR_TRACK_SEG_FRAMES=<n> / ASR_TRACK_LDS_PIECES=<n> (debug) set the segment length and send
 *   n_pieces > n to the workspace path. */
int asr_track_gate_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, int n_rec, const int64_t *offsets,
                       const int32_t *bins, const int32_t *frames, const int64_t *frame0, const float *norm, int width,
                       float *m_prob, uint8_t *voiced, float *level);
int asr_track_vote_batch_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_rows, int n_rec, const int64_t *row_first,
                             const int64_t *row_count, const int64_t *emit_from, int n_candidates, int running_frames,
                             const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k, int32_t *pieces,
                             int32_t *counts, int32_t *n_out);

/* ---- the running vote for n_streams parallel live streams, state on the device (track_stream_kernels.hip) ------------
 * The two calls above, per round of new columns, for streams that arrive block by block.  Like asr_dtw_follow_batch_dev
 * and asr_audio_stream_push_dev they keep a stream's state in the caller's device buffers and update it in place; the
 * counters the host knows anyway (frames_before, voiced_before) are arguments, and a counter of 0 means "new stream: the
 * state is not read and need not be initialised".  Between the two calls the caller runs asr_embed_view2_dev and
 * asr_topk_db_dev over the windows of all streams.  All streams of a call share bins, width, n_candidates and
 * running_frames.
 *
 * asr_track_stream_gate_dev: stream s brings n_new[s] >= 0 new columns as a (bins, n_new[s]) float32 row-major block at
 *   float col_off[s] of cols_dev (cols_floats floats; asr_audio_stream_push_dev's transposed output).  Its state is the
 *   (bins, width - 1) row-major block at float tail_off[s] of tail_dev (tail_floats floats): the last width - 1 columns
 *   of the stream so far, zeros where it had not started (running_spec[:, 1:], :92, :110).  With frames_before[s] == 0
 *   the tail counts as zeros and is not read.
 *     m_prob, voiced (host; sum(n_new) each, in stream order): per new frame what asr_track_gate_dev returns for the
 *       recording [tail | new] with norm = level[s] and frame0 = frames_before[s] - (width - 1), without its first
 *       width - 1 entries - the same float32 operations in the same order (column sums row after row, the
 *       eight-accumulator mean, the two divisions, the clip, m_prob > 0.5 and frame >= width).
 *     win_dev (device, win_cap windows of bins x width floats): the window (1, bins, width) = columns i - width + 1 .. i
 *       of the stream of every voiced frame i, ordered by stream and then by frame - an order fixed by a count and a
 *       scan, not by atomics; nothing is written past the last window.  n_voiced (host, n_streams): windows per stream.
 *   Afterwards the tail of every stream with n_new[s] > 0 holds the last width - 1 columns of [tail | new]; a stream
 *   with n_new[s] == 0 is left untouched.  ASR_ERR_INVALID before anything is launched and with no state touched:
 *   width outside 8..128, bins < 1, n_streams < 1, a negative n_new or frames_before, a block outside cols_floats, a
 *   tail outside tail_floats, two tails that overlap, sum(n_new) > win_cap.  Four launches whatever n_streams is: the
 *   column sums, the gate with the window numbering (one workgroup), the windows (one workgroup per voiced frame, rows
 *   of width floats written coalesced, [tail | new] read through the cache), and behind them the tails (one workgroup
 *   per stream: a chunk's sources are read before a barrier and the chunk written after it).
 *
 * asr_track_stream_vote_dev: idx_dev = (n_rows x n_candidates) int32 data-base indices, the new rows of all streams
 *   (what asr_topk_db_dev wrote for win_dev); stream s owns row_count[s] >= 0 consecutive rows in stream order,
 *   sum(row_count) = n_rows.  Its state is (running_frames - 1) x n_candidates int32 at hist_off[s] of hist_dev
 *   (hist_len entries), a ring: the row of the stream's v-th voiced frame (v from 0) lives in slot
 *   v mod (running_frames - 1); voiced_before[s] = the voiced frames before this call, so the slots of the last
 *   min(voiced_before, running_frames - 1) frames are valid.  With voiced_before[s] == 0 the ring is not read;
 *   running_frames == 1 has no history and hist_dev / hist_off may be NULL.
 *     pieces / counts (host, n_rows x top_k), n_out (n_rows): per new row what asr_track_vote_batch_dev returns for the
 *       table [ring rows in frame order | new rows] with emit_from = the number of ring rows: the same order
 *       (count << 32 | piece), -1 / 0 padding, ignored invalid entries and limits; counters in LDS up to 4096 pieces,
 *       in the workspace above; ASR_TRACK_SEG_FRAMES / ASR_TRACK_LDS_PIECES / ASR_VOTE_BUDGET_MB as there.
 *   Afterwards the ring holds the rows of the last running_frames - 1 voiced frames: a launch behind all votes of the
 *   call stores the last min(row_count, running_frames - 1) new rows.  ASR_ERR_INVALID before anything is launched and
 *   with no state touched: the size limits of asr_track_vote_batch_dev, n_streams < 1, a negative row_count or
 *   voiced_before, sum(row_count) != n_rows, a ring outside hist_len, two rings that overlap. */
int asr_track_stream_gate_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                              const int64_t *col_off, const int32_t *n_new, const int64_t *frames_before,
                              const float *level, int bins, int width, float *tail_dev, int64_t tail_floats,
                              const int64_t *tail_off, float *win_dev, int64_t win_cap, float *m_prob, uint8_t *voiced,
                              int32_t *n_voiced);
int asr_track_stream_vote_dev(asr_ctx *ctx, const int32_t *idx_dev, int64_t n_rows, int n_streams,
                              const int32_t *row_count, const int64_t *voiced_before, int n_candidates,
                              int running_frames, const int32_t *ids_dev, int64_t n_db, int32_t n_pieces, int top_k,
                              int32_t *hist_dev, int64_t hist_len, const int64_t *hist_off, int32_t *pieces,
                              int32_t *counts, int32_t *n_out);

/* ---- the music gate at the level of what has been heard so far (track_level_kernels.hip) ----------------------------
 * _detect_music (:524-528) divides by spec.sum(axis=0).max() of the finished spectrogram; the reference's microphone
 * branch (spec=None) cannot run it, and a live stream has no such number.  The causal rule is the reference's own rule
 * applied to what has been heard, optionally with a bounded memory so that one loud bang does not deafen the gate for
 * the rest of a session.
 *
 * Inputs, for a stream or recording with columns 0, 1, ...: c_j = the float32 sum of column j over the bins, added row
 *   after row (what the two gate calls above compute); width = w; memory = L: 0 (unbounded) or w <= L <= 2^20; floor =
 *   F: a float32, or -inf for none.
 * Rule, per frame i:
 *     level_i  = fmaxf(F, max{ c_j : max(0, i - L + 1) <= j <= i })            (L == 0: 0 <= j <= i)
 *     m_prob_i = the gate of asr_track_gate_dev - the eight-accumulator mean of the w column sums that end at i (zeros
 *                before column 0) divided by float32(w), divided by float32(level_i * float32(0.15)), clipped to
 *                [0, 1], NaN stays NaN - the same device function, at level_i
 *     voiced_i = m_prob_i > 0.5 and i >= w                                     (i: the stream position)
 * Consequences:
 *   - With F = -inf and L == 0, (m_prob_i, voiced_i) is the last entry of asr_track_gate_dev on columns 0 .. i.
 *   - With F = -inf and L >= w, m_prob_i is the last m_prob entry of asr_track_gate_dev on columns
 *     max(0, i - L + 1) .. i.  This needs L >= w - the mean would otherwise read columns the level does not cover - so
 *     0 < L < w is rejected.
 *   - A silent prefix gives 0 / 0 = NaN and is unvoiced, as there.
 *   - Inputs must be finite: a non-finite column sum leaves the results unspecified (nothing faults).  max is exact on
 *     finite values, so no scan order, no cut into blocks and no neighbour in the batch changes a bit.
 *
 * asr_track_gate_running_dev: whole recordings - the causal gate of finished recordings, which is how one evaluates
 *   offline what a live session will do.  Arguments as in asr_track_gate_dev without norm and frame0; level (host,
 *   sum(frames) floats, may be NULL) receives level_i per frame.  ASR_ERR_INVALID as there, and for memory negative, in
 *   1 .. width - 1 or above 2^20, and for floor NaN or +inf.  Four launches whatever n_rec is (three with memory == 0):
 *   the column sums; with memory > 0 per recording the maxima from every column to the end of its block of L columns;
 *   per recording the maxima from the start of the block, combined per frame with the former (van Herk / Gil-Werman:
 *   level_i = fmaxf(F, fmaxf(suffix[i - L + 1], prefix[i])), no frame rescans its window); the gate.  Both maxima are
 *   segmented workgroup scans, one workgroup per recording.
 *
 * asr_track_stream_gate_running_dev: asr_track_stream_gate_dev in every respect - blocks, tails, windows in stream and
 *   frame order, m_prob, voiced, n_voiced, validation, nothing launched and no state touched on error - except that
 *   the `level` array is replaced by memory and floor, and that a stream carries a level state at float level_off[s]
 *   of level_dev (level_floats floats), updated in place:
 *     L == 0: one float, the maximum column sum so far;
 *     L > 0 : L - 1 floats, a ring with c_f in slot f mod (L - 1), valid for the last min(frames_before, L - 1) frames.
 *   With frames_before[s] == 0 the state is not read and need not be initialised; a stream with n_new[s] == 0 leaves
 *   it untouched.  level (host, sum(n_new) floats, may be NULL): level_i per new frame.  Per frame the results are
 *   those of asr_track_gate_running_dev on the stream's columns so far, whatever the cut into blocks and whatever the
 *   other streams bring.  Further ASR_ERR_INVALID cases: memory negative, in 1 .. width - 1 or above 2^20; floor NaN or
 *   +inf; a level state outside level_floats; two level states that overlap.  Seven launches whatever n_streams is
 *   (six with memory == 0): the column sums, the suffix maxima over [valid ring entries in frame order | new column
 *   sums] (memory > 0), the prefix maxima and levels, the gate with the window numbering, the windows, the tails, and
 *   behind every reader of the old state the level states (one workgroup per stream: its last min(n_new, L - 1) column
 *   sums to their slots - with fewer old and new entries coexist in the ring).  Work per call is O(state + new
 *   frames) per stream. */
int asr_track_gate_running_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, int n_rec, const int64_t *offsets,
                               const int32_t *bins, const int32_t *frames, int width, int memory, float floor,
                               float *m_prob, uint8_t *voiced, float *level);
int asr_track_stream_gate_running_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                                      const int64_t *col_off, const int32_t *n_new, const int64_t *frames_before,
                                      int memory, float floor, int bins, int width, float *tail_dev, int64_t tail_floats,
                                      const int64_t *tail_off, float *level_dev, int64_t level_floats,
                                      const int64_t *level_off, float *win_dev, int64_t win_cap, float *m_prob,
                                      uint8_t *voiced, int32_t *n_voiced, float *level);

/* ---- audio front-end -------------------------------------------------
 * The madmom chain the reference feeds its spectrogram tower with (tutorials/Embedding Tutorial.ipynb cell 28,
 * msmd.midi_parser.processor; audio_sheet_server.py:632,678 `processor.process(audio_file).T`):
 *   FramedSignalProcessor(frame_size, fps, origin='future'): frame i = samples[int(i*hop) : int(i*hop)+frame_size],
 *     zero padded past the end, hop = sample_rate / fps (fractional);
 *   magnitude STFT with `window` (np.hanning(frame_size); divided by 32767 for int16 input - the caller's choice);
 *   filterbank: filter f = fb_len[f] weights starting at FFT bin fb_start[f] (weights concatenated in fb_weights);
 *   out = log10(mul * x + add).
 * samples_dev: float32 mono samples on the device; out_dev: (n_frames, n_filters), or (n_filters, n_frames) when
 * transposed != 0 (the layout detect_score / asr_slice_windows_dev take).  window / fb_*: host arrays. */
int asr_spectrogram_dev(asr_ctx *ctx, const float *samples_dev, int64_t n_samples, int frame_size, double hop,
                        const float *window, const int32_t *fb_start, const int32_t *fb_len, const float *fb_weights,
                        int n_filters, float mul, float add, int64_t n_frames, int transposed, float *out_dev);

/* ---- alignment: distance matrix + DTW -----------------------------
 * compute_alignment / align_pydtw (utils/alignment.py:120-186) on dtw_by_dist (utils/dtw_by_dist.py:5-34,76-91):
 * dists = cdist(a, b, "cosine") in float64 (same arithmetic as asr_rank), accumulated cost
 * D1[i,j] += min(D0[i,j], D0[i,j+1], D0[i+1,j]) as an anti-diagonal wavefront, traceback with argmin over
 * (diagonal, up, left), first minimum winning.  a_dev (n_a,dim), b_dev (n_b,dim) float32 on the device, rows of the
 * cost matrix = a.  The reference transposes when the matrix is wider than tall (:13-15) - the caller passes the
 * longer sequence as `a` (audio_sheet_retrieval_amd/alignment.py does).  Outputs (host): dists n_a*n_b doubles (may
 * be NULL), path_a / path_b (capacity n_a + n_b) = _traceback's (p, q), *path_len, *min_dist = D1[-1,-1] / (n_a+n_b). */
int asr_dtw_dev(asr_ctx *ctx, const float *a_dev, int64_t n_a, const float *b_dev, int64_t n_b, int dim,
                double *dists, int32_t *path_a, int32_t *path_b, int32_t *path_len, double *min_dist);

/* ---- batched alignment DTW (audio2sheet_align.py over a whole test split) ---------------
 * asr_dtw_dev for n_pairs independent pairs in one call, every result bit-identical with asr_dtw_dev on the pair alone
 * (batch composition and order change nothing).  a_dev / b_dev: the pairs' code rows concatenated (pair p's rows
 * start at sum_{q<p} n_a[q] / n_b[q]), float32, row length dim, on the device.  n_a / n_b: host arrays of n_pairs.
 * Outputs (host, each may be NULL):
 *   min_dist[p] = D1[-1,-1] / (n_a[p] + n_b[p]); path_len[p];
 *   path_a / path_b: pair p's path (_traceback's (p, q), forward order) at offset sum_{q<p} (n_a[q] + n_b[q])
 *     (capacity n_a + n_b; entries past path_len[p] unspecified) - path_a, path_b and path_len go together;
 *   dists: pair p's n_a x n_b cosine distances, row-major, at offset sum_{q<p} n_a[q] * n_b[q];
 *   first_a: per row i of pair p, the column of the first path entry in row i, at offset sum_{q<p} n_a[q];
 *   first_b: per column j, the row of the first path entry in column j (align_pydtw's projection), at sum n_b[q].
 * With min_dist, path_*, first_* all NULL only the distances are computed.
 * Limits: 1 <= dim <= 64; per pair 1 <= n_a, n_b <= 100000 and (n_a+1)(n_b+1) <= 2^31 (asr_dtw_dev's).  The
 * wavefront keeps three anti-diagonals of min(n_a,n_b) + 1 doubles in one workgroup's LDS (160 KiB on gfx950:
 * min(n_a,n_b) <= 6825); a larger pair keeps them in a global ring instead, with the same results.  Device memory:
 * ~17 bytes per cell of the pairs in flight (9 without dists), kept on the context between calls and freed by
 * asr_destroy; a batch above ASR_DTW_BUDGET_MB (default 4096) runs in chunks of consecutive pairs.  ASR_DTW_LDS_CAP=<n>
 * (debug) sends pairs with min(n_a,n_b) + 1 > n to the global-ring path. */
int asr_dtw_batch_dev(asr_ctx *ctx, const float *a_dev, const float *b_dev, const int64_t *n_a, const int64_t *n_b,
                      int n_pairs, int dim, double *min_dist, int32_t *path_len, int32_t *path_a, int32_t *path_b,
                      double *dists, int32_t *first_a, int32_t *first_b);

/* ---- batched subsequence DTW: where in a long reference does a short query lie? -----------
 * For a query of Q code rows and a reference of S code rows let D[i][j] be the float64 cosine distance of query row i
 * and reference row j in exactly asr_dtw_dev's arithmetic (dot2acc and cos_dist of csrc/dist64.h, row norms as the
 * DTW path computes them).  The accumulated cost is
 *     A[0][j] = D[0][j]                                                     (free start on the reference axis)
 *     A[i][j] = D[i][j] + fmin(A[i-1][j-1], fmin(A[i-1][j], A[i][j-1]))      for i >= 1,
 *               every out-of-range predecessor = +inf
 * and from it
 *     end      = the smallest j that minimises A[Q-1][j] (first minimum);
 *     cost     = A[Q-1][end] / Q, one correctly rounded float64 division;
 *     the traceback starts at (Q-1, end) and, while i > 0, picks the predecessor by _traceback's rule (the one of
 *     asr_dtw_batch_dev): order (diagonal, up (i-1,j), left (i,j-1)), strict <, first minimum wins;
 *     start    = j when i reaches 0;
 *     path_len = the cells of the path, both ends included;
 *     pos[i]   = the smallest j the path visits in row i, i.e. the column of row i's first entry in forward order
 *                (align_pydtw's projection, from the query side).
 * The code rows are embeddings: a row of zero norm makes the result unspecified.  Every A value is one fixed sequence
 * of correctly rounded float64 operations, so the order in which cells are scheduled cannot change a bit.
 *
 * q_dev (q_rows, dim) and r_dev (r_rows, dim): float32 code rows on the device; r_dev may be the resident code buffer
 * of a data base.  q_row / n_q / r_row / n_r: host arrays of n_pairs, each pair's first row and length in either
 * buffer; pairs may share a query or a reference.  Outputs (host, each may be NULL): cost, start, end, path_len of
 * n_pairs; pos holds pair p's n_q[p] entries at offset sum_{q<p} n_q[q].  Pairs are independent: neither batch
 * composition nor order changes a result.
 * Limits (ASR_ERR_INVALID otherwise, nothing is launched): 1 <= dim <= 64; per pair 1 <= n_q <= 1024,
 * 1 <= n_r <= 100000, the row ranges inside the two buffers, n_q * (n_r + n_q) < 2^31.  A longer query is
 * asr_dtw_batch_dev's job.  One workgroup per pair, one lane per query row; no distance or accumulated value is
 * written to device memory, only one direction byte per cell (n_q * (n_r + n_q - 1) per pair), kept with the pair
 * table on the context between calls and freed by asr_destroy; a batch above ASR_DTW_BUDGET_MB (default 4096) runs in
 * chunks of consecutive pairs with identical results. */
int asr_dtw_subseq_batch_dev(asr_ctx *ctx, const float *q_dev, int64_t q_rows, const float *r_dev, int64_t r_rows,
                             const int64_t *q_row, const int64_t *n_q, const int64_t *r_row, const int64_t *n_r,
                             int n_pairs, int dim, double *cost, int32_t *start, int32_t *end,
                             int32_t *path_len, int32_t *pos);

/* ---- streaming subsequence DTW: where in the reference is the stream now? -----------------
 * asr_dtw_subseq_batch_dev's matrix, one block of query rows at a time: the recurrence needs only the last accumulated
 * row from the past, and when every cell also carries the column at which its best path started, no traceback is
 * needed.  D[i][j] is the float64 cosine distance in asr_dtw_subseq_batch_dev's arithmetic.  A pair is one stream
 * against one reference of S rows; its state is acc[S] (float64), org[S] (int32) and the number n0 of query rows it
 * has consumed.  A call gives the pair B new query rows, global rows n0 .. n0 + B - 1:
 *     n0 == 0: global row 0 is the free start, A[0][j] = D[0][j], O[0][j] = j; the state is not read and need not be
 *              initialised;
 *     n0 > 0:  row n0 - 1 is the state, A[n0-1][j] = acc[j], O[n0-1][j] = org[j];
 *     every further row: A[i][j] = D[i][j] + fmin(A[i-1][j-1], fmin(A[i-1][j], A[i][j-1])), out-of-range predecessors
 *              = +inf; w = the first minimum in the order (diagonal, up, left) with strict < (_traceback's rule, the
 *              direction byte of the subsequence kernel); O[i][j] = O of predecessor w.
 * Per new row i:
 *     pos[i]   = the smallest j that minimises A[i][.];
 *     cost[i]  = A[i][pos[i]] / (i + 1), one correctly rounded float64 division, i global;
 *     start[i] = O[i][pos[i]].
 * Afterwards acc and org hold row n0 + B - 1 (updated in place on the device).  For every i this is
 * asr_dtw_subseq_batch_dev on rows 0..i: end = pos[i], start = start[i], cost = cost[i] - independent of how the rows
 * were cut into calls.  A row of zero norm or a non-finite value leaves the result unspecified.
 *
 * q_dev, q_rows, r_dev, r_rows, q_row, n_q, r_row, n_r as in asr_dtw_subseq_batch_dev (r_dev may be a data base's
 * resident code buffer; pairs may share query rows and reference rows); rows_before: n0 per pair.  acc_dev / org_dev:
 * device buffers of state_len elements; pair p's state is n_r[p] entries at state_off[p] of both.  cost, start, pos:
 * host arrays of sum n_q, pair p's entries at offset sum_{q<p} n_q[q]; each may be NULL, and a call with all three
 * NULL still advances the state.
 * Limits (ASR_ERR_INVALID otherwise; nothing is launched and no state is touched): 1 <= dim <= 64; per pair
 * 1 <= n_q <= 1024, 1 <= n_r <= 100000, 0 <= rows_before, rows_before + n_q < 2^31, the row ranges inside the two
 * buffers, the state range inside state_len; the state ranges of two pairs of one call must not overlap (they would
 * race).  A longer block is several calls.  One workgroup per pair, one lane per block row.  There is no per-cell
 * memory: the workspace (kept on the context, freed by asr_destroy) is the pair table and the three per-row outputs,
 * 16 bytes per query row, so ASR_DTW_BUDGET_MB has nothing to chunk and is not read.  ASR_DTW_SUBSEQ_LDS_CAP (debug)
 * applies as in asr_dtw_subseq_batch_dev. */
int asr_dtw_follow_batch_dev(asr_ctx *ctx, const float *q_dev, int64_t q_rows, const float *r_dev, int64_t r_rows,
                             const int64_t *q_row, const int64_t *n_q, const int64_t *r_row, const int64_t *n_r,
                             const int64_t *rows_before, int n_pairs, int dim,
                             double *acc_dev, int32_t *org_dev, int64_t state_len, const int64_t *state_off,
                             double *cost, int32_t *start, int32_t *pos);

/* ---- score following for n_streams parallel live streams, state on the device (follow_stream_kernels.hip) ------------
 * What a session around asr_dtw_follow_batch_dev needs per round of new columns when the streams' state is to stay on
 * the device: the query windows on the step grid cut from [tail | new block], and per stream a linear log of its last
 * window codes, so that a candidate that enters late can be followed from `keep` windows back and entering and
 * continuing pairs of one follow call address the same rows.  Between the two calls the caller runs asr_embed_view2_dev
 * over win_dev; behind them asr_dtw_follow_batch_dev with q_dev = log_dev.  Both calls move floats only, use no atomics
 * (every order comes from counts the host knows) and check every index against the sizes validated here.
 *
 * The contract of a session built on them (piece_identification.ScoreFollowerBank): per window i (counted over the
 * stream's life) a slot that holds a piece since window `since` reports what asr_dtw_subseq_batch_dev gives for the
 * stream's windows since .. i against that piece: end = row, start = start_row, and cost = A / (i - since + 1) - the
 * accumulated cost already normalised by the rows consumed, which is what makes a late entrant comparable with slots
 * that have followed for longer.
 *
 * asr_follow_stream_windows_dev: cols_dev, cols_floats, n_streams, col_off, n_new, bins, width, tail_dev, tail_floats,
 *   tail_off as in asr_track_stream_gate_dev (the tail layout is the same; the tail counts as zeros and is not read when
 *   cols_before[s] == 0).  cols_before[s]: columns of the stream before this call.  The windows of a stream are those
 *   that begin at stream column k * step (follow_window_plan's rule, whatever the block cut): with
 *   done(T) = T < width ? 0 : (T - width) / step + 1 the call writes windows done(cols_before) <= k <
 *   done(cols_before + n_new) as (bins, width) row-major blocks to win_dev (room for win_cap windows), ordered by stream
 *   and then by k; nothing is written past the last window.  n_win (host, n_streams): windows per stream.  A window
 *   written by a call ends in a new column, so it never starts before the tail; with step > width the next unfinished
 *   window may start beyond the stream's end.  Afterwards the tail of every stream with n_new[s] > 0 holds the last
 *   width - 1 columns of [tail | new]; a stream with n_new[s] == 0 is left untouched.  ASR_ERR_INVALID before anything
 *   is launched and with no state touched: width outside 8..128, bins < 1, n_streams < 1, step < 1, a negative n_new or
 *   cols_before, a block outside cols_floats, a tail outside tail_floats, two tails that overlap, more windows than
 *   win_cap.  Two launches whatever n_streams is: the windows (one workgroup per window, rows of width floats written
 *   coalesced, 128 bits per lane where bins * width is a multiple of 4), and behind them the tails (one workgroup per
 *   stream: a chunk's sources are read before a barrier and the chunk written after it).
 *
 * asr_follow_stream_log_dev: codes_dev = (n_rows x dim) float32, the new code rows of all streams (what the tower
 *   wrote for win_dev); stream s owns row_count[s] >= 0 consecutive rows in stream order, sum(row_count) = n_rows.  Its
 *   log starts at float log_off[s] of log_dev (log_floats floats) and holds rows_in_log[s] valid rows at its front.
 *   For a stream with row_count[s] > 0 and kept = min(rows_in_log[s], keep): the last kept rows move to the front of
 *   the log (in place, overlap-safe: chunk by chunk, sources read before a barrier) and the new rows are copied behind
 *   them, so the log is [kept | new] and the caller sets rows_in_log = kept + row_count.  A stream with
 *   row_count[s] == 0 is left untouched.  ASR_ERR_INVALID before anything is launched and with no state touched:
 *   n_streams < 1, dim outside 1..64, keep < 0, a negative row_count or rows_in_log, sum(row_count) != n_rows, a log
 *   that cannot hold max(rows_in_log, kept + row_count) rows inside log_floats, two logs that overlap.  One launch,
 *   one workgroup per stream; 128 bits per lane where dim and the log's offset are multiples of 4. */
int asr_follow_stream_windows_dev(asr_ctx *ctx, const float *cols_dev, int64_t cols_floats, int n_streams,
                                  const int64_t *col_off, const int32_t *n_new, const int64_t *cols_before, int bins,
                                  int width, int step, float *tail_dev, int64_t tail_floats, const int64_t *tail_off,
                                  float *win_dev, int64_t win_cap, int32_t *n_win);
int asr_follow_stream_log_dev(asr_ctx *ctx, const float *codes_dev, int64_t n_rows, int n_streams,
                              const int32_t *row_count, const int32_t *rows_in_log, int keep, int dim, float *log_dev,
                              int64_t log_floats, const int64_t *log_off);

/* ---- training-pool batch assembly on the device ----------------------
 * AudioScoreRetrievalPool.__getitem__ (utils/data_pools.py:127-228): every sample is a window of one strip (unrolled
 * score image or spectrogram) of a pool that stays resident on the device, with the augmentations of
 * exp_configs/mutopia_full_aug.yaml - sheet_scaling (cv2.resize INTER_NEAREST), system_translation, onset_translation,
 * spec_padding (np.pad mode="edge").  The host draws the random numbers in the reference's order and reduces a sample
 * to 9 doubles desc[i] = {off, stride, y0, sy, ymax, x0, sx, xmax, xadd}; then
 *   out[i,0,y,x] = src[off + clamp(floor((y0+y)*sy), 0, ymax) * stride + xadd + clamp(floor((x0+x)*sx), 0, xmax)].
 * src_dev: the pool (src_floats float32, strips concatenated); out_dev: (n,1,out_h,out_w) float32. */
int asr_gather_windows_dev(asr_ctx *ctx, const float *src_dev, int64_t src_floats, const double *desc, int n,
                           int out_h, int out_w, float *out_dev);

/* ---- host-buffer pipeline ---------------------------------------------------------------------
 * The evaluation loop of run_eval.py:102-108,174 (and the per-call copies of utils/batch_iterators.py:90-109) for a
 * stream of host batches: batch k = n (sheet, spectrogram) pairs x[k] / z[k] in host memory (in_mode as in
 * asr_embed_view1) -> both towers -> all-pairs ranking of the batch's n queries against its n candidates ->
 * ranks[k] (n int32), and optionally dstar[k] (n float64), ties[k] (n int32), lv1[k] / lv2[k] (n x 32 float32) back
 * in host memory (the array pointers, or single entries, may be NULL).  Inputs are double-buffered on the device:
 * the host-to-device copy of batch k+1 and the device-to-host copy of batch k-1 run on their own copy streams while
 * batch k computes.  Host buffers from asr_host_alloc (page-locked) make the copies truly asynchronous; ordinary
 * memory works, slower.  Returns when every output is in place. */
int asr_host_alloc(asr_ctx *ctx, size_t bytes, void **hptr);
int asr_host_free(asr_ctx *ctx, void *hptr);
int asr_eval_batches(asr_ctx *ctx, const void *const *x, int in_mode, const float *const *z, int n_batches, int64_t n,
                     int32_t *const *ranks, double *const *dstar, int32_t *const *ties, float *const *lv1,
                     float *const *lv2);

/* Self-check of the kernel autotuner.  With ASR_TUNE_VERIFY=1 in the environment the first embed call of each tower
 * runs every candidate schedule / tiling of every conv block on one deterministic input and compares its output with
 * the first candidate's (all evaluate the same fp32 FMA chains, so they must agree to <= 1e-5).  Returns the number of
 * comparisons made, of mismatches, and the largest deviation seen. */
int asr_debug_tune_report(asr_ctx *ctx, int32_t *checked, int32_t *mismatches, float *max_diff);

/* ---- multi-GPU: one process and one context per GPU -------------------
 * The reference is single-device; these entry points are what a sharded deployment binds.  Pairs are sharded
 * by contiguous ranges, rank r of `world` holding [r*n_local, (r+1)*n_local).
 *   retrieval: embedding needs no communication; asr_rank_sharded_dev all-gathers the candidate-side
 *     embeddings (n_local x 32 floats per rank) and ranks this rank's queries against all of them - integer
 *     results identical to the single-GPU asr_rank on the concatenated data;
 *   training: asr_train_step / asr_burn_in shard the batch: each rank passes its rows - batch/world of them, or,
 *     after asr_train_set_global_batch(n), its contiguous share of n rows (the first n % world ranks hold one row
 *     more), so that the reference's BATCH_SIZE = 100 (models/mutopia_ccal_cont.py:26) trains on all 100 rows on 3 or
 *     8 GPUs.  The per-channel BatchNorm sums are all-reduced forward and backward, the 32-d tower outputs are
 *     all-gathered and every rank evaluates CCALayer + loss on the full batch, the parameter gradients are
 *     all-reduced before Adam: every rank ends the step with the same parameters the single-GPU step over the
 *     whole batch produces (float32 summation order aside).
 * Transport: RCCL (asr_comm_unique_id on rank 0, hand the 128 bytes to every rank, asr_comm_init on all; the
 * collectives are enqueued on the context's stream), or caller-supplied host callbacks (asr_comm_init_custom:
 * the library drains the stream, then calls the callback, which must return with the result in place - used by
 * the tests to run two ranks on one GPU, and by deployments with another transport).
 * Initialise the communicator before asr_train_begin. */
#define ASR_COMM_ID_BYTES 128
#define ASR_DTYPE_F32 0
#define ASR_DTYPE_F64 1
#define ASR_DTYPE_I32 2
typedef int (*asr_allreduce_fn)(void *user, void *buf_dev, int64_t count, int dtype);       /* in-place sum */
typedef int (*asr_allgather_fn)(void *user, const void *send_dev, void *recv_dev, int64_t bytes_per_rank);
int asr_comm_unique_id(void *id_out /* ASR_COMM_ID_BYTES */);
int asr_comm_init(asr_ctx *ctx, int rank, int world, const void *unique_id);
int asr_comm_init_custom(asr_ctx *ctx, int rank, int world, asr_allreduce_fn allreduce, asr_allgather_fn allgather,
                         void *user);
int asr_comm_destroy(asr_ctx *ctx);
int asr_comm_info(asr_ctx *ctx, int *rank, int *world);
/* Collectives this context has issued through its communicator since the last reset: counts[0..3] = all-reduce calls,
 * all-reduce payload bytes, all-gather calls, all-gather bytes sent per rank.  What `bench.py --workload train`
 * reports as the exchange cost of one data-parallel update (the reference's single-device step,
 * utils/train_dcca_pool.py:203-205, has none). */
int asr_comm_stats(asr_ctx *ctx, int64_t *counts, int reset);
/* Time spent in those collectives: while enabled every collective is bracketed by two HIP events on the stream it is
 * enqueued on (RCCL) or timed on the host clock (callbacks).  Each call waits for the context's streams, returns the
 * summed duration (ms) and the number of collectives since the previous call, resets both and sets the switch to
 * `enable`.  ms / calls may be NULL.  (New with the multi-GPU path; the reference has no collectives.) */
int asr_comm_timing(asr_ctx *ctx, int enable, double *ms, int64_t *calls);
/* File the RCCL entry points of this context's communicator were bound from ("" without an RCCL communicator).  The
 * library is looked up as ASR_RCCL_LIB, $ROCM_PATH/lib/librccl.so, /opt/rocm/lib/librccl.so, then by bare name. */
int asr_comm_library(asr_ctx *ctx, char *path, int cap);
/* The communicator's two collectives on caller-owned device buffers, enqueued on the context's stream like the
 * library's own exchange steps: in-place sum over all ranks of `count` values (ASR_DTYPE_F32 / _F64) and the
 * concatenation of every rank's bytes_per_rank bytes in rank order.  What the host code uses for the hit counters,
 * the max-over-ranks timing and the epoch decisions fit() takes on rank 0 (utils/train_dcca_pool.py:391-411,
 * 492-520 run in one process in the reference).  With no communicator (or a world of one) the all-reduce leaves
 * the buffer unchanged and the all-gather copies send -> recv. */
int asr_comm_allreduce_dev(asr_ctx *ctx, void *buf_dev, int64_t count, int dtype);
int asr_comm_allgather_dev(asr_ctx *ctx, const void *send_dev, void *recv_dev, int64_t bytes_per_rank);
/* lv1_dev, lv2_dev: (n_local,32) device; lv2_all_dev: (world*n_local,32) device workspace that receives the
 * gathered candidates; ranks/dstar/ties: n_local device outputs as in asr_rank_dev. */
int asr_rank_sharded_dev(asr_ctx *ctx, const float *lv1_dev, const float *lv2_dev, int64_t n_local,
                         float *lv2_all_dev, int32_t *ranks, double *dstar, int32_t *ties);

/* ---- training ------------------------------------------------------------------
 * The compiled functions of create_iter_functions (utils/train_dcca_pool.py:85-167):
 *   asr_train_step  = iter_funcs['train'](X1, X2) -> [loss, corr]      (:154)
 *   asr_valid_loss  = iter_funcs['valid'](X1, X2) -> [loss]            (:155)
 * asr_train_step runs, entirely on the device: both towers with batch statistics
 * (BatchNormLayer train branch + EMA of mean / inv_std), the CCALayer
 * train branch (layers/cca.py:91-182; the four eigh's and their EighGrad as
 * float64 Jacobi iterations in one workgroup; the layer's running U, V, means,
 * S12, S11, S22 are overwritten like its default_updates do), LengthNormLayer, the
 * contrastive cos loss (models/objectives.py:30-69, gamma from asr_config), the
 * full backward pass, the L2 penalty l2 * sum p^2 over W, beta, gamma (:141-142)
 * and lasagne.updates.adam (beta1 .9, beta2 .999, eps 1e-8, step
 * lr*sqrt(1-b2^t)/(1-b1^t); models/mutopia_ccal_cont.py:158-162).
 * x1: (batch,1,H1,W1) float32 ALREADY prepared (the reference applies model.prepare
 * in the batch iterator, utils/batch_iterators.py:220-221); x2: (batch,1,h2,w2).
 * loss = ranking loss + L2 penalty (as Theano reports it), corr: 32 canonical
 * correlations (ascending, layers/cca.py:161-164).  lr is passed per call
 * (fit() mutates the shared learning rate, :343,520,525).
 * asr_train_begin allocates the device state for batches up to batch_size and
 * starts Adam from zero moments; asr_get/set_opt_state expose (m, v, t) for the
 * refinement restarts of fit() (:396,515-516): flat float32 arrays over the
 * tower parameters in the order of asr_get_params (asr_opt_state_size values;
 * non-trainable slots are zero). */
int asr_train_begin(asr_ctx *ctx, int batch_size);
int asr_train_end(asr_ctx *ctx);
/* Data parallel (asr_comm_init*), batches that are not a multiple of the world size: the following asr_train_step /
 * asr_burn_in / asr_compute_gradients calls carry this rank's rows [lo, hi) of ONE batch of n_global rows, lo / hi by
 * the contiguous rule (rank r: lo = r*(n/world) + min(r, n%world); the first n%world ranks hold one row more); a call
 * whose `batch` is not that count fails.  BatchNorm means, the CCALayer covariances and the loss run over exactly
 * n_global rows - nothing is padded or dropped - which is what iter_funcs['train'](X1, X2) computes on one device
 * (utils/train_dcca_pool.py:154, :203-205).  n_global = 0 restores the default (batch * world, equal shards).  Needs
 * asr_train_begin with batch_size >= ceil(n_global / world). */
int asr_train_set_global_batch(asr_ctx *ctx, int64_t n_global);
int asr_train_step(asr_ctx *ctx, const float *x1, const float *x2, int64_t batch, float lr,
                   float *loss, float *corr);
int asr_train_step_dev(asr_ctx *ctx, const float *x1_dev, const float *x2_dev, int64_t batch, float lr,
                       float *loss, float *corr);
int asr_valid_loss(asr_ctx *ctx, const float *x1, const float *x2, int64_t n, float *loss);
/* objectives() of the model module (models/mutopia_ccal_cont.py:152-155) =
 * get_contrastive_cos_loss(weight, gamma, symmetric) (models/objectives.py:30-69): the loss asr_train_step,
 * asr_compute_gradients and asr_valid_loss evaluate.  Default: weight 1, gamma = asr_config.gamma, symmetric 0 - what
 * both models bind.  symmetric = 1 adds the transposed direction (:53-65: the same hinge with the views swapped);
 * weight scales loss and gradients (:67).  Takes effect from the next call. */
int asr_set_objective(asr_ctx *ctx, float weight, float gamma, int symmetric);
/* iter_funcs['init_cca'](X1, X2) of create_iter_functions(init_cca=True) (utils/train_dcca_pool.py:160-162), the
 * burn-in pass of pretrain() (:170-182): one TRAIN-mode forward whose only side effects are the default updates of the
 * graph - BatchNorm running mean / inv_std and the CCALayer running means, covariances, U, V.  No gradients, no Adam
 * step, Adam's t unchanged.  lv1 / lv2 (batch,32) receive the train-mode outputs (may be NULL).  Needs
 * asr_train_begin. */
int asr_burn_in(asr_ctx *ctx, const float *x1, const float *x2, int64_t batch, float *lv1, float *lv2);
/* iter_funcs['compute_gradients'](X1, X2) (utils/train_dcca_pool.py:164-167: theano.function(input_vars, all_grads)):
 * the gradient of the train loss (ranking loss + l2 * sum p^2) wrt every trainable parameter, WITHOUT the Adam step.
 * grads: flat float32 array of asr_opt_state_size values in the order of asr_get_params (non-trainable slots zero).
 * Like every function compiled from the train-mode graph it applies the graph's default updates (BatchNorm and
 * CCALayer running values move exactly as in asr_burn_in); Adam's moments and t stay untouched.  loss may be NULL. */
int asr_compute_gradients(asr_ctx *ctx, const float *x1, const float *x2, int64_t batch, float *grads, int64_t n,
                          float *loss);
/* The same five functions on RAW sheet batches - what the reference's training loop produces before model.prepare:
 * train() (utils/train_dcca_pool.py:154-162 via :185-231) iterates MultiviewPoolIteratorUnsupervised
 * (utils/batch_iterators.py:114-141, 163-221), whose transform applies prepare_plain / prepare_rsz on the host
 * (models/_common.py; x.astype(np.float32); x /= 255 on 512 x 160 x 200 pixels per batch).  Here the host passes the
 * pool's window as it is:
 *   in_mode  ASR_IN_F32_PREPARED: x1 exactly as asr_train_step & co. take it (these calls ARE those then);
 *            ASR_IN_U8_RAW / ASR_IN_F32_RAW: x1 (batch,1,h1,w1) uint8 / float32 0..255 at the context's raw size
 *            (asr_config.h1 x w1, as asr_embed_view1 takes it; for a resize_view1 model that is 2H x 2W of the network
 *            input).  The training step copies the raw batch into a staging buffer of the training state (sized at
 *            asr_train_begin) and one kernel writes the prepared float32 tensor the step reads - bit for bit what
 *            prepare_plain / prepare_rsz give, so every result equals the prepared call's.  A uint8 batch moves a
 *            quarter of the bytes.  asr_valid_loss_in embeds through asr_embed_view1 with the mode.
 *   x2, batch, lr, outputs and data parallel (this rank's rows) as in the functions above.
 * asr_train_step_in_dev takes device pointers (e.g. the window buffers of asr_gather_windows_dev, un-normalised
 * float32 = ASR_IN_F32_RAW) and, like asr_train_step_dev, returns after the step. */
int asr_train_step_in(asr_ctx *ctx, const void *x1, int in_mode, const float *x2, int64_t batch, float lr,
                      float *loss, float *corr);
int asr_train_step_in_dev(asr_ctx *ctx, const void *x1_dev, int in_mode, const float *x2_dev, int64_t batch,
                          float lr, float *loss, float *corr);
int asr_burn_in_in(asr_ctx *ctx, const void *x1, int in_mode, const float *x2, int64_t batch, float *lv1, float *lv2);
int asr_compute_gradients_in(asr_ctx *ctx, const void *x1, int in_mode, const float *x2, int64_t batch,
                             float *grads, int64_t n, float *loss);
int asr_valid_loss_in(asr_ctx *ctx, const void *x1, int in_mode, const float *x2, int64_t n, float *loss);
/* iter_funcs['valid'] + iter_funcs['compute_output'] on the same batch (utils/train_dcca_pool.py:155,158), which train()
 * calls one after the other on every evaluation batch (:277-285; _collect_outputs here): ONE deterministic-mode forward of
 * both towers, the contrastive loss of the objective set by asr_set_objective on the latents where they lie on the
 * device, and both latents.  *loss equals asr_valid_loss_in's bit for bit, lv1 / lv2 (n,32) equal asr_embed_both's
 * (ASR_OUT_LATENT) bit for bit.  in_mode as asr_valid_loss_in; n >= 2.  Eval mode: no BatchNorm, CCALayer or Adam
 * state moves; works with a live training state, after asr_train_end and without one.
 *   asr_valid_output_in: host buffers; lv1 / lv2 may be NULL (asr_valid_loss and asr_valid_loss_in are this call with
 *     both NULL).  One pass of the host pipeline over the two views, the loss kernel on the pipeline's output buffer,
 *     the copies back, one host synchronisation; no allocation per call.
 *   asr_valid_output_in_dev: device pointers (e.g. the window buffers of asr_gather_windows_dev, ASR_IN_F32_RAW);
 *     loss_dev is ONE float slot (a validation loop passes losses_dev + i), lv1_dev / lv2_dev (n,32) may be NULL (the
 *     context's workspace then holds them).  Returns after enqueueing, without a host synchronisation.  Ordering,
 *     by events inside the context - the caller needs no double buffering: the loss runs on the context's main
 *     stream after both towers, so every later call of the context that touches the main stream or waits for it
 *     (asr_gather_windows_dev into the same windows, asr_dev_download, asr_sync, asr_rank_dev, the next *_dev embed or
 *     training step) runs after the towers have read x1_dev / x2_dev and sees loss_dev and lv*_dev complete.  Work the
 *     caller enqueues on its own streams must wait for asr_sync first. */
int asr_valid_output_in(asr_ctx *ctx, const void *x1, int in_mode, const float *x2, int64_t n, float *loss,
                        float *lv1, float *lv2);
int asr_valid_output_in_dev(asr_ctx *ctx, const void *x1_dev, int in_mode, const float *x2_dev, int64_t n,
                            float *loss_dev, float *lv1_dev, float *lv2_dev);
int asr_opt_state_size(asr_ctx *ctx, int64_t *n);
int asr_get_opt_state(asr_ctx *ctx, float *m, float *v, int64_t n, int32_t *t);
int asr_set_opt_state(asr_ctx *ctx, const float *m, const float *v, int64_t n, int32_t t);
/* test aids: intermediate tensors of the last training step
 * (kind: 0 raw conv output z, 1 block input x, 2 batch stats [mu|inv_std], 3 H,
 * 4 dL/dH, 5 train-mode embedding, 6 gradient of parameter `index`, 7 device
 * value of parameter `index`, 8 [loss | corr], 9 pooled block `index`: the raw conv output of the element every 2x2
 * pooling window selected - (batch, H/2, W/2, C), the FIRST maximal element; 10 pooled block `index`: the set of
 * window elements whose BatchNorm output equals the window maximum, as the backward pass decides it - (batch, H/2, W/2,
 * C) floats holding 4-bit sets, bit 2*dy+dx; derived on request from z, the batch statistics and the scale / shift
 * the forward pass kept); and the
 * CCALayer + loss stage
 * alone on host arrays (cca_in/cca_out: U V mean1 mean2 S12 S11 S22, 5184 floats). */
int asr_debug_train_tensor(asr_ctx *ctx, int kind, int view, int index, int64_t batch,
                           float *out, int64_t cap, int64_t *n_out);
int asr_cca_train_debug(asr_ctx *ctx, const float *H1, const float *H2, int64_t batch,
                        const float *cca_in, float *cca_out, float *loss_corr,
                        float *lv1, float *lv2, float *dH1, float *dH2);
/* test aid: ONE candidate of the lists asr_train_begin's tuner times for a 3x3 block (`block` 1..7 = conv2..conv8 of
 * `view`), alone, through the production launcher, on host arrays (NHWC, `batch` <= the training state's batch size):
 *   kind 0 forward convolution   a = x (batch,H,W,cin)            -> out = z (batch,H,W,cout), stats = [mu | inv_std]
 *        1 data gradient         a = dz (batch,H,W,cout)          -> out = dx (batch,H,W,cin)
 *        2 weight gradient       a = x, b = dz                    -> out = dW (cout,cin,3,3), the parameter's layout
 * `index` counts into the tuner's own list (the model's plan first); past its end the call fails with
 * ASR_ERR_INVALID and a message that ends in "has <length> candidates".  The output buffer, the BatchNorm statistics
 * table (kind 0), the partial sums and the gradient slot (kind 2) are filled with 0xff bytes first, so an element or a
 * table row the schedule does not write comes back as NaN; every Winograd-domain weight copy is rebuilt from the device
 * master before the launch.  kind 0, when the schedule gathers the statistics itself (info[1] > 0): the table is
 * finished as the training step does (eps 1e-4) into stats (2*cout floats; NaN otherwise).
 * out = NULL: nothing runs, info [2..11] and desc alone are filled (a caller sizes and checks its arrays by them).
 *   info (12 values): [0] 1 launched / 0 the launcher refused the schedule (the tuner skips such a candidate; out is
 *   NaN), [1] rows of the statistics table the launcher reported, [2] work items (M-tiles of 16 tiles; regions for the
 *   LDS-patch Winograd form; tiles for kind 2), [3] workgroups along x, [4] family 0 direct / 1 winog (global-A F(2x2))
 *   / 2 wino (LDS-patch F(2x2); kind 2: the Winograd-domain weight gradient) / 3 wino4 (F(4x4)), [5] variant,
 *   [6] [7] the plan's TH, TW, [8..11] the block's H, W, cin, cout.  desc: one line in the tuner's ASR_DEBUG format, e.g. "winog#3515 tile 2x32 x16".
 * Afterwards the gradient slot is zero again and plans, parameters, Adam state and the repack table are as before. */
int asr_debug_train_candidate(asr_ctx *ctx, int view, int block, int kind, int index, int64_t batch,
                              const float *a, const float *b, float *out, int64_t cap, float *stats,
                              int32_t *info, char *desc, int64_t desc_cap);

/* ---- staff-system detection (sheet_utils/omr.py, system_detector.py, bar_detector.py) ----------------
 * One U-Net of SegmentationNetwork (system_detector.build_model(), bar_detector's graph at its own input size) as a
 * handle of the context that created it, like asr_db.
 *   asr_seg_create      = build_model(in_shape=(1, tile_h, tile_w)) + SegmentationNetwork.load(pkl): `arrays` are the
 *                         reference's 99 parameter arrays in pickle order (float32, C order), sizes[i] their element
 *                         counts, checked against the graph (nf0 = 8).  tile_h, tile_w: multiples of 8.
 *   asr_seg_set_window  = the tile weight sqrt(outer(hamming(tile_h), hamming(tile_w))) as float64, tile_h x tile_w
 *                         (optional: asr_seg_create computes it; a caller that wants numpy's bits passes numpy's)
 *   asr_seg_predict_dev = predict_proba(page, squeeze=True, overlap) for n_pages pages in one call: page p is
 *                         heights[p] x widths[p], row-major at element page_offsets[p] of pages_dev; in_mode as
 *                         asr_embed_view1 (0 prepared float32, 1 raw float32, 2 raw uint8: prepare_image is folded
 *                         in).  A page of exactly the tile size goes through the network directly; any other is
 *                         zero-padded to a multiple of the tile and cut into tiles with the reference's steps, and the
 *                         float64 map R / V is cropped back (NaN where no tile covers a pixel).  proba_dev: float64,
 *                         the pages' maps back to back.  All tiles of all pages form one forward, in chunks of whole
 *                         tiles under ASR_OMR_BUDGET_MB of device workspace (default 4096). */
typedef struct asr_seg asr_seg;
int asr_seg_create(asr_ctx *ctx, int tile_h, int tile_w, const float *const *arrays, const int64_t *sizes,
                   int n_arrays, asr_seg **out);
int asr_seg_set_window(asr_ctx *ctx, asr_seg *seg, const double *win_host);
int asr_seg_destroy(asr_ctx *ctx, asr_seg *seg);
int asr_seg_predict_dev(asr_ctx *ctx, asr_seg *seg, const void *pages_dev, int in_mode, const int64_t *page_offsets,
                        const int32_t *heights, const int32_t *widths, int n_pages, double overlap,
                        double *proba_dev);

/* asr_systems_from_maps_dev = detect_systems after the two probability maps exist (sheet_utils/omr.py
 *   systems_from_maps: Otsu of the row projection, gap clean-up, Otsu of the system map, the 15x1 closing, 8-connected
 *   labelling, bounding-box shrink and the snap to the staff-line grid) for n_pages pages in one call, the maps never
 *   leaving the device.  pages_dev / in_mode / page_offsets / heights / widths: the pages exactly as
 *   asr_seg_predict_dev reads them (prepare_image folded in for raw pages).  system_maps_dev: the float64 system maps
 *   back to back as asr_seg_predict_dev writes them; bar_maps_dev: the bar maps in the same layout, or NULL (the
 *   projection is then taken from the system map, as in the reference).  system_seg / bar_seg: the networks the maps
 *   came from, or NULL; they only tell which page shapes equal a tile (below).
 *   Host outputs, per page p: status[p], counts[p] and, for status 0, counts[p] rows of int32
 *   (min_row, max_row, min_col, max_col) at systems + (p * max_systems + k) * 4, in the order the host returns them.
 *   A page cannot hold more than heights[p] * widths[p] / 50000 blobs of MIN_AREA; a smaller max_systems is rejected
 *   before anything is launched.
 *       status 0  ok
 *              1  no row of the projection lies below its Otsu threshold (the host raises IndexError)
 *              2  the snap found no edge candidate (the host raises ValueError)
 *              3  not decided on the device: the caller runs the host path for this page
 *   The integers are those of the host path: every comparison that decides a pixel, a row or a peak is made on the
 *   bits numpy would see (row sums in numpy's pairwise order, np.histogram's bin rule, no contraction).  Status 3,
 *   never a guess, is returned for what is not restated exactly: a page of a network's tile size (the host casts
 *   those maps to float32), a NaN or an infinity in a map or in the page, histogram edges numpy would reject, a
 *   shrink loop that leaves the blob's bounding box, an empty row slice in the snap, pages narrower than 8 columns,
 *   lower than 3 rows or wider than 65536 columns.
 *   np.histogram's uniform-bin index is computed as numpy 2.x computes it, ((x - first) / (last - first)) * bins,
 *   followed by its two corrections against the edges; numpy 1.x multiplies by bins / (last - first) instead.  The
 *   device path is specified and tested against numpy >= 2 (2.2.6) only: under numpy 1.x the equality tests against the
 *   host path are the judge, not this restatement.
 *   Workspace belongs to the context; pages are processed in chunks of whole pages under ASR_OMR_BUDGET_MB (at least
 *   one page per chunk).  label_passes (may be NULL): the number of labelling passes of the call, over all chunks. */
int asr_systems_from_maps_dev(asr_ctx *ctx, const void *pages_dev, int in_mode, const int64_t *page_offsets,
                              const int32_t *heights, const int32_t *widths, int n_pages,
                              const double *system_maps_dev, const double *bar_maps_dev, const asr_seg *system_seg,
                              const asr_seg *bar_seg, int max_systems, int32_t *status, int32_t *counts,
                              int32_t *systems, int32_t *label_passes);

/* asr_notes_from_map_dev = detect_notes after the note map exists (sheet_utils/omr.py notes_from_map: peak_local_max
 *   in two dimensions) and asr_bars_from_map_dev = detect_bars after the bar map exists, up to and including the
 *   region properties (bar_blobs_from_map: threshold_otsu of the whole map, map > t, 8-connected labels, blob_stats),
 *   for n_pages pages in one call each.  maps_dev: the float64 maps back to back exactly as asr_seg_predict_dev
 *   writes them - page p is heights[p] x widths[p] at element sum of heights[q] * widths[q] over q < p; the page
 *   pixels themselves are not read, so the table has no page_offsets.  seg: the network the maps came from, or NULL;
 *   it only tells which page shape equals the tile.  Outputs are host arrays.
 *   notes: a pixel is a peak if it equals the maximum of its (2 min_distance + 1)^2 neighbourhood (zero beyond the
 *   page), lies at least min_distance pixels off every border and is strictly above max(threshold_abs,
 *   threshold_rel * page maximum).  A NaN threshold argument means "not given"; without threshold_abs the page
 *   minimum takes its place.  min_distance: 1..8.  A constant page has no peaks.  coords: counts[p] int32 (row, col)
 *   pairs at coords + p * max_peaks * 2, in the host's order (raster order reversed).
 *   bars: blobs holds counts[p] rows of 10 int64 at blobs + p * max_blobs * 10 in label order (raster order of each
 *   blob's first pixel): area, min_row, min_col, max_row, max_col (max exclusive), and the sums of r, c, r*r, c*c,
 *   r*c over the blob's pixels in page coordinates.  Rows beyond counts[p] are not written.  The filters of
 *   detect_bars (bars_from_stats) and the alignment with the systems run on the host, on these integers.
 *       status 0  decided
 *              3  not decided on the device: the caller runs the host path for this page.  A page of the tile size
 *                 (the host works on a float32 map there), a NaN or an infinity in the map; for bars also histogram
 *                 edges numpy would reject and a page with h * w * max(h, w)^2 >= 2^63.
 *              4  more than max_peaks / max_blobs results: counts[p] holds the true number, nothing is written
 *   The np.histogram restatement is that of asr_systems_from_maps_dev (numpy >= 2).  Workspace belongs to the
 *   context; pages are processed in chunks of whole pages under ASR_OMR_BUDGET_MB (at least one page per chunk).
 *   label_passes (may be NULL): the number of labelling passes of the call, over all chunks. */
int asr_notes_from_map_dev(asr_ctx *ctx, const double *maps_dev, const int32_t *heights, const int32_t *widths,
                           int n_pages, const asr_seg *seg, double threshold_abs, double threshold_rel,
                           int min_distance, int max_peaks, int32_t *status, int32_t *counts, int32_t *coords);
int asr_bars_from_map_dev(asr_ctx *ctx, const double *maps_dev, const int32_t *heights, const int32_t *widths,
                          int n_pages, const asr_seg *seg, int max_blobs, int32_t *status, int32_t *counts,
                          int64_t *blobs, int32_t *label_passes);

/* ---- scanned scores and recordings to strips and spectrograms (umc_a2s_server.py / umc_s2a_server.py) ----------
 * asr_unroll_systems_dev = the unrolling loop of load_umc_sheets (umc_a2s_server.py:136-158) for all systems of all
 *   pages of all pieces in one launch.  pages_dev: the uint8 pages exactly as asr_seg_predict_dev (in_mode 2) reads
 *   them (page p is heights[p] x widths[p], row-major at byte page_offsets[p]; pages_bytes = size of the buffer).
 *   systems: n_systems rows of 8 int32 that the host computes with the reference's integer rules (:139-147):
 *       page, r0, r1, c0, c1, pad, piece, dst_col
 *   rows r0..r1-1 and columns c0..c1-1 of the page go to columns dst_col.. of the piece's strip; the last `pad` rows of
 *   the strip repeat row r1-1 (np.pad mode="edge", :156); r1 - r0 + pad == system_height.  Systems the reference skips
 *   (:153-155) are simply not in the table.  Strip of piece q: (system_height, strip_widths[q]) float32 holding the
 *   0..255 values, row-major at float strip_offsets[q] of strips_dev (strips_floats = size of that buffer in floats) -
 *   the layout asr_gather_windows_dev and asr_slice_windows_dev read.  Every row is checked against the page, the
 *   strip and both buffer sizes before anything is launched; columns of a strip that no system covers are left as
 *   they are.
 * asr_spectrogram_batch_dev = asr_spectrogram_dev (processor.process(audio_path), umc_a2s_server.py:35-45, :238) for
 *   n_recordings recordings of different lengths in one launch.  Recording i: sample_counts[i] samples at float
 *   sample_offsets[i] of samples_dev (samples_floats = size of that buffer), n_frames[i] frames, written at float
 *   out_offsets[i] of out_dev (out_floats = its size) as (n_filters, n_frames[i]) if transposed else
 *   (n_frames[i], n_filters).  Every recording's output is bit-identical with asr_spectrogram_dev on it alone: a frame
 *   is computed by the same device code, only the frame-to-recording lookup is added.  Recordings of zero samples /
 *   zero frames and n_recordings == 0 are valid and write nothing.
 * asr_spectrogram_fft_batch_dev = asr_spectrogram_batch_dev, same arguments and layouts, with the magnitudes taken from
 *   a real-input FFT in float32 instead of the direct DFT (csrc/spectrogram_fft_kernels.hip; about 80 times fewer
 *   operations).  The definition:
 *     frame      frame i of a recording starts at sample (int64)((double)i * hop) and has frame_size samples; samples past
 *                the end of the frame's own recording read as zero, also when another recording follows immediately in
 *                the buffer; sample t of the frame is multiplied by window[t] in float32
 *     magnitude  of bins 0 .. frame_size / 2 - 1: equal to the DFT's within float32 rounding, summation order unspecified
 *     result     filter f: s = sum of magnitude[fb_start[f] + q] * fb_weights[...][q] in ascending q (fmaf), then
 *                log10f(mul * s + add), as asr_spectrogram_dev
 *     tolerance  against the same chain in float64 (float64 product of sample and float32 window, float64 FFT, float64
 *                filterbank with the float32 weights, float64 log10) the result deviates by at most 1e-4, and by no
 *                more than asr_spectrogram_batch_dev's does on the same input (tests/test_gpu_spectrogram_fft.py)
 *     bit for bit  a recording's output does not depend on which other recordings are in the call, on their order or
 *                on `transposed` (the two layouts are exact transposes), and repeated calls agree.  It is NOT
 *                bit-identical with asr_spectrogram_batch_dev or asr_audio_stream_push_dev; the stream that reproduces
 *                its bits is asr_audio_stream_push_fft_dev.
 *   Checked before anything is launched: everything asr_spectrogram_batch_dev checks, frame_size == 2048 (the
 *   reference's only value) and every filter inside bins 0 .. 1023.  A violation returns ASR_ERR_INVALID with a message
 *   and launches nothing.  n_recordings == 0 and recordings of zero samples or zero frames are valid and write nothing;
 *   floats of out_dev that belong to no recording are left as they are.  The twiddle table (float32 rounded from
 *   float64, computed once on the host) and the per-call tables are workspace of the context.
 * asr_resample_batch_dev = what madmom's SignalProcessor(sample_rate=22050) has its decoder do to a recording at
 *   another rate, for n_recordings recordings of one input rate in one launch, between the upload and
 *   asr_spectrogram_batch_dev.  The reference's resampler (ffmpeg's) is not restated; the yardstick is this definition,
 *   which audio_frontend.resample_host restates in numpy and the device reproduces bit for bit (finite samples):
 *     ratio   g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g (both >= 1)
 *     taps    q = max(up, down), half = 16 * q; float64, i = 0 .. 2 * half:
 *             h[i] = sinc((i - half) / q) * kaiser(2 * half + 1, beta 8.6)[i], scaled so that sum(h) == up
 *             (up to rounding scipy.signal.firwin(2 * half + 1, 1 / q, window=("kaiser", 8.6)) * up)
 *     table   taps_phase_major[p * taps_per_phase + t] = h[p + t * up], 0 past the end of h; p = 0 .. up-1,
 *             taps_per_phase = ceil((2 * half + 1) / up)     (65 at 44.1 kHz, 70 at 48 kHz, 33 when upsampling)
 *     output  n_out = ceil(n_in * up / down); for output m, in int64: c = m * down + half, p = c % up, j0 = c / up,
 *             y[m] = sum over t = 0 .. taps_per_phase-1 with 0 <= j0 - t < n_in of
 *                    taps_phase_major[p][t] * (double)x[j0 - t]
 *             starting from 0.0, in ascending t, one rounding per product and one per sum (no fused multiply-add)
 *             = scipy.signal.resample_poly(x, up, down, window=h / up)
 *     result  round_int16 == 0: (float)y[m];  != 0 (integer PCM): (float)clip(rint(y[m]), -32768, 32767), rint to even
 *   Recording i: in_counts[i] floats at float in_offsets[i] of in_dev (in_floats = size of that buffer); its
 *   out_counts[i] outputs go to float out_offsets[i] of out_dev (out_floats = its size); floats of out_dev that belong
 *   to no recording are left as they are.  taps_phase_major is a host array of up * taps_per_phase doubles; the copy on
 *   the device and the per-recording tables are workspace of the context.  Before anything is launched every row is
 *   checked against both buffer sizes and out_counts[i] against ceil(in_counts[i] * up / down), and up, down >= 1,
 *   taps_per_phase * up >= 2 * half + 1 and the size of a tile's input span (ratios down / up up to 13 fit) are
 *   checked: a violation returns ASR_ERR_INVALID with a message.  Recordings of zero samples and n_recordings == 0 are
 *   valid and write nothing.
 * asr_audio_stream_push_dev = asr_resample_batch_dev followed by asr_spectrogram_batch_dev for recordings that arrive
 *   block by block: for n_streams streams of one input rate, one call takes a block of new input samples per stream and
 *   writes the spectrogram frames those samples complete; the input samples that later frames still read stay on the
 *   device, in a buffer the caller owns.
 *     sequences  x_s[0 .. N) is every input sample stream s has been given so far; N0 = samples_before[s] (the host keeps
 *                count), N1 = N0 + block_counts[s].  y_s[m] is output m of asr_resample_batch_dev's definition on x_s with
 *                the same up, down, half, taps_phase_major, taps_per_phase, round_int16.  Output m is final once
 *                (m * down + half) / up < N: every input it reads has arrived.  M(N) = max(0, ceil((N * up - half) / down)),
 *                capped at ceil(N * up / down), is the number of final outputs.  up == down == 1 with taps_phase_major ==
 *                NULL is the front-end's own rate: y = x, M(N) = N, no filter (taps_per_phase, half, round_int16 unused).
 *     frames     frame i is asr_spectrogram_dev's frame i on y_s, starting at (int64)((double)i * hop).  A stream that is
 *                not flushed (final[s] == 0) has emitted frame i once start + frame_size <= M(N1): no zero is invented
 *                for a sample that has not arrived.  A flushed stream (final[s] != 0) takes y_s as the whole recording,
 *                of length ceil(N1 * up / down) and zero beyond, and emits every remaining frame up to
 *                ceil(length / hop) (SpectrogramProcessor.num_frames).  The host does not push to a flushed stream again.
 *     property   whatever the cut into calls, the concatenation of a stream's outputs is bit-identical with
 *                asr_spectrogram_batch_dev on asr_resample_batch_dev of the whole recording; before the flush the outputs
 *                are a prefix of it.
 *     state      stream s owns floats state_offsets[s] .. + state_cap of state_dev (state_floats = size of that buffer).
 *                After a call it holds input samples keep_from .. N1 - 1, keep_from = the first input the next frame not
 *                yet emitted reads: (start_next * down + half) / up - (taps_per_phase - 1), clamped to [0, N1]
 *                (start_next at the front-end's own rate).  It is read where N0 > 0 and rewritten in place by the call,
 *                on the device, after the frames; N0 == 0 is a reset and does not read it.  N1 - keep_from never exceeds
 *                ceil((frame_size - 1) * down / up) + taps_per_phase - 1 (frame_size - 1 at the front-end's own rate:
 *                2047 floats at 22.05 kHz, 4158 at 44.1 kHz, 4526 at 48 kHz), whatever the block lengths;
 *                state_cap must be at least that (audio_frontend.audio_stream_state_len).
 *     arguments  block s: block_counts[s] floats (0 is valid) at float block_offsets[s] of blocks_dev (blocks_floats = size
 *                of that buffer).  first_frames[s] / n_new_frames[s]: the first frame this call emits and how many - the
 *                host needs them for out_offsets (audio_frontend.audio_stream_plan); the library recomputes both from
 *                samples_before, block_counts and final, and a mismatch is an error.  The frames go to float
 *                out_offsets[s] of out_dev (out_floats = its size) as (n_filters, n_new_frames[s]) if transposed else
 *                (n_new_frames[s], n_filters); floats that belong to no stream are left as they are.  window, fb_start,
 *                fb_len, fb_weights, mul, add: as asr_spectrogram_batch_dev.
 *   Before anything is launched: every block, state and output range is checked against its buffer, no two state ranges
 *   may overlap, state_cap against the bound above, frame_size (a power of two in [64, 8192]) and the filter bank as in
 *   asr_spectrogram_batch_dev, the resampler arguments as in asr_resample_batch_dev, the frame counts, and the LDS a
 *   frame's input span needs at this ratio against the 160 KB of a workgroup.  A violation returns ASR_ERR_INVALID with a
 *   message; a failing call touches no state and writes no output.  n_streams == 0 and all-empty blocks are valid and
 *   write nothing.  One workgroup per new frame resamples the frame's own samples (overlapping frames resample the
 *   samples they share once each), then one workgroup per stream slides the state.
 * asr_audio_stream_push_fft_dev = asr_audio_stream_push_dev, same arguments, state and plan, with the magnitudes of a
 *   frame taken from the real-input FFT of asr_spectrogram_fft_batch_dev instead of the direct DFT
 *   (csrc/audio_stream_fft_kernels.hip): asr_resample_batch_dev followed by asr_spectrogram_fft_batch_dev for recordings
 *   that arrive block by block.
 *     property   the frames a call emits are bit-identical with the corresponding columns of asr_spectrogram_fft_batch_dev
 *                on asr_resample_batch_dev of the whole recording (at the front-end's own rate: on the recording itself),
 *                whatever the cut into calls, whatever the other streams of the call, and in both output layouts (the two
 *                are exact transposes); before the flush the emitted frames are a prefix of that result.  They are NOT
 *                bit-identical with asr_audio_stream_push_dev's.
 *     state      as asr_audio_stream_push_dev: input samples, the same keep_from and the same bound on state_cap, slid by
 *                the same kernel.  A stream's state does not record which of the two calls wrote it.
 *   Checked before anything is launched: everything asr_audio_stream_push_dev checks, frame_size == 2048 and every filter
 *   inside bins [0, 1024).  A frame needs no more LDS than the direct call's at the same ratio, so every ratio that call
 *   takes (input rates from 4 to 192 kHz) is taken here.  A violation returns ASR_ERR_INVALID with a message that starts
 *   with "audio_stream_push_fft:"; a failing call touches no state and writes no output.  The twiddle table is the
 *   context's (asr_spectrogram_fft_batch_dev's); the call puts it on the device where no FFT call has done so before.
 *   One workgroup per new frame: the filters of a frame are never split over workgroups (ASR_STREAM_PARTS does not apply).
 * asr_resize_pages_dev = what scripts/prepare_umc_data.py:17-22 does to a scan before the OMR networks see it (width
 *   835, height int(835.0 / W * H), cv2.resize), for n_pages pages of any sizes in one launch, between the upload and
 *   asr_seg_predict_dev.  OpenCV's fixed-point bilinear rule is not restated; the yardstick is this definition, exact
 *   area resampling (a box filter over each output pixel's footprint), separable, in integers, which
 *   sheet_utils/omr.resize_page_host restates in numpy and the device reproduces byte for byte:
 *     axis    n_in source and n_out output pixels, in units of 1 / (n_in * n_out) of the axis: source pixel j covers
 *             [j * n_out, (j + 1) * n_out), output pixel i covers [i * n_in, (i + 1) * n_in), and the weight w(i, j) is
 *             the integer length of their overlap; the weights of an output pixel sum to n_in
 *     sum     S(r, c) = sum over j, k of wy(r, j) * wx(c, k) * src[j, k], an exact integer <= 255 * h_in * w_in (64 bits:
 *             it passes 2^32 from about 600 dpi on)
 *     result  out[r, c] = (2 * S + D) / (2 * D), D = h_in * w_in, integer division: the mean rounded, a half goes up
 *   n_out == n_in reproduces the input, an integer ratio gives the exact block mean, n_out > n_in replicates pixels
 *   and blends the seams.  Page p: heights[p] x widths[p] uint8, row-major at byte page_offsets[p] of pages_dev
 *   (pages_bytes = size of that buffer) - the layout asr_seg_predict_dev (in_mode 2) and asr_unroll_systems_dev read,
 *   rows at any alignment; its out_heights[p] x out_widths[p] result goes to byte out_offsets[p] of out_dev (out_bytes =
 *   its size) in the same layout.  Bytes of out_dev that belong to no page are left as they are.  The host chooses the
 *   output shape (the drivers: sheet_utils/omr.resized_shape, the reference's rule).  The page-to-tile table is
 *   workspace of the context.  Before anything is launched every page and every output is checked against its buffer
 *   size, and per page: all four dimensions at least 1 and at most 2^24, h_in * w_in < 2^31, and per axis
 *   n_out / 4 <= n_in <= 16 * n_out (ratios n_in / n_out from 1/4 to 16: what a tile's source rows in LDS are sized
 *   for).  A violation returns ASR_ERR_INVALID with a message.  n_pages == 0 is valid and writes nothing.
 * asr_skew_estimate_dev / asr_deskew_pages_dev = straightening a scan whose staves are not horizontal, between the upload
 *   and asr_resize_pages_dev.  The reference has no such stage; the yardstick is this definition, all in integers, which
 *   sheet_utils/omr.skew_scores_host / estimate_skew_host / shear_page_host restate in numpy and the device reproduces
 *   exactly.  Pages are uint8, dark ink on light paper, in the layout of asr_resize_pages_dev.  A slope k is an integer in
 *   units of 1/1024 pixel per pixel; >> is the arithmetic shift (floor division).
 *     profile   t_k(x) = k * (2 * x - (W - 1)), in 1/2048 pixel; d_k(x) = (t_k(x) + 1024) >> 11;
 *               P_k[r] = sum over all pixels (y, x) with y - d_k(x) == r of (255 - page[y][x]), r over every value that
 *               occurs (no pixel is dropped); score_k = sum over r of P_k[r]^2 in int64 (P fits 32 bits, the score stays
 *               below 2^59)
 *     estimate  the k in [-max_slope, max_slope] of largest score; the candidates are visited in the order 0, -1, +1, -2,
 *               +2, ... and one replaces the best only on strict >: a blank or ambiguous page gives 0
 *     shear     by slope k with fill in 0 .. 255, two passes, each rounded to uint8.  Vertical: q = t_k(x) >> 11,
 *               f = t_k(x) - 2048 * q, A[y][x] = ((2048 - f) * I(y + q, x) + f * I(y + q + 1, x) + 1024) >> 11 with
 *               I(r, x) = page[r][x] inside the page and fill outside.  Horizontal: u(y) = -k * (2 * y - (H - 1)),
 *               p = u >> 11, g = u - 2048 * p, out[y][x] = ((2048 - g) * A(y, x + p) + g * A(y, x + p + 1) + 1024) >> 11
 *               with A = fill outside its columns.  k = 0 is the identity; the output has the input's shape; shearing by
 *               the estimate straightens the page (the two shears are a rotation up to a scale of 1 - s^2).
 *   asr_skew_estimate_dev: all pages and all slopes in one call.  slopes: host int32[n_pages].  scores: host
 *   int64[n_pages * (2 * max_slope + 1)], the score of slope k of page p at p * (2 * max_slope + 1) + k + max_slope, or
 *   NULL.  d_k is constant over runs of about 1024 / |k| columns, so a profile costs two reads of a row's prefix sums per
 *   (row, run), not one add per pixel.  The profiles are workspace of the context; batches whose profiles exceed
 *   ASR_OMR_BUDGET_MB (default 4096) run in chunks of whole pages with identical results.
 *   asr_deskew_pages_dev: page p sheared by slopes[p] (host int32[n_pages]) goes to the same byte offset of out_dev
 *   (out_bytes = its size), which must not overlap pages_dev.  Bytes of out_dev that belong to no page are left as they
 *   are.
 *   Both: rows at any alignment.  Before anything is launched: 1 <= H, W <= 16384, 0 <= max_slope <= 128,
 *   |slopes[p]| <= 128, 0 <= fill <= 255, and every page inside the buffers.  A violation returns ASR_ERR_INVALID with a
 *   message and writes nothing.  n_pages == 0 is valid and writes nothing.
 * asr_flatten_pages_dev = taking the paper out of a scan - a spine shadow, a gradient, yellowed paper - between the upload
 *   and the deskew.  The reference has no such stage; the yardstick is this definition, all in integers, which
 *   sheet_utils/omr.page_background_host / flatten_page_host restate in numpy / scipy and the device reproduces exactly.
 *   A page P is H x W uint8, dark ink on light paper, in the layout of asr_resize_pages_dev; a radius r is 1 .. 127, a
 *   floor f 0 .. 255.
 *     dilate  D(y', x') = max { P[y][x] : |y - y'| <= r, |x - x'| <= r, (y, x) inside the page }
 *             for y' in [-r, H-1+r], x' in [-r, W-1+r]  (the page's r-neighbourhood; every such window meets the page)
 *     erode   B[y][x]   = min { D(y', x') : |y' - y| <= r, |x' - x| <= r }      for (y, x) inside the page
 *     result  out[y][x] = (510 * P + B) / (2 * B)  if B >= max(f, 1)   (integer division: 255 * P / B, a half goes up)
 *                         P                        otherwise           (not paper: a black scanner border stays)
 *   B is the grey closing of the page by a (2r+1)-square on an unbounded plane where the outside is absent: B >= P, so
 *   out <= 255; where B == 255 the result is P; a page without ink that is monotone along each axis gives B == P (hence
 *   the extended grid of D: with windows merely clipped to the page a shadow at a border would stay).  The passes are row
 *   max, column max, then row min and column min - not a row closing followed by a column closing.
 *   Page p goes to the same byte offset of out_dev (out_bytes = its size), which must not overlap pages_dev;
 *   background_dev, unless NULL, receives B in the same layout and must overlap neither.  Bytes that belong to no page are
 *   left as they are.  radii: host int32[n_pages] (sheet_utils/omr.flatten_radius: min(127, max(1, (W + 32) / 64))).
 *   Rows at any alignment; two launches per call whatever n_pages is; D is workspace of the context, and batches whose D
 *   exceed ASR_OMR_BUDGET_MB (default 4096) run in chunks of whole pages with identical results.  Before anything is
 *   launched: 1 <= H, W <= 16384, 1 <= radii[p] <= 127, 0 <= floor <= 255, every page inside the buffers, and the
 *   overlaps above.  A violation returns ASR_ERR_INVALID with a message that starts with "flatten_pages:" and writes
 *   nothing.  n_pages == 0 is valid and writes nothing.
 * asr_crop_estimate_dev / asr_crop_pages_dev = taking a flat-bed scanner's black frame off a scan of a page smaller than
 *   the glass, between the upload and the flatten.  The reference has no such stage; the yardstick is this definition, all
 *   in integers, which sheet_utils/omr.crop_counts_host / crop_rect_host / crop_page_host restate in numpy and the device
 *   reproduces exactly.  A page is H x W uint8, dark ink on light paper, in the layout of asr_resize_pages_dev; floor is
 *   0 .. 255 (a grey level), share 1 .. 1024 (in 1/1024), margins[p] >= 0 (pixels; host int32[n_pages];
 *   sheet_utils/omr.crop_margin: (W + 32) / 64).
 *     dark       dark(y, x) = page[y][x] < floor                          (floor 0: nothing is dark)
 *     bands      columns cb0 = W / 4, cb1 = W - W / 4; rows rb0 = H / 4, rb1 = H - H / 4   (integer divisions; non-empty)
 *     counts     rowcount[r] = #{ x in [cb0, cb1) : dark(r, x) },  colcount[c] = #{ y in [rb0, rb1) : dark(y, c) }
 *                (each axis over the central band of the other: the frame of the other two sides and the corners never
 *                enter a count)
 *     border     row r: 1024 * rowcount[r] >= share * (cb1 - cb0);  column c: 1024 * colcount[c] >= share * (rb1 - rb0)
 *     runs       top = the length of the maximal run of border rows that starts at row 0, bottom = of the one that ends at
 *                row H - 1; left, right the same for columns.  Only a run that touches the edge counts.
 *     rect       r0 = top + (top ? margin : 0), r1 = H - bottom - (bottom ? margin : 0); c0, c1 the same.  Status 0.
 *     undecided  top + bottom >= H, or left + right >= W, or r1 - r0 < 1, or c1 - c0 < 1: the rect is the whole page
 *                (0, H, 0, W) and the status is 1 - an all-dark page, a margin larger than the paper.
 *     result     out = page[r0:r1, c0:c1]
 *   A page without a dark edge is returned as it is; an axis-aligned frame of any widths up to a quarter of the page is
 *   removed exactly.
 *   asr_crop_estimate_dev writes rects (host int32[n_pages * 4]: r0 r1 c0 c1), status (host int32[n_pages]) and, unless
 *   NULL, row_counts / col_counts (host int32, the pages' rows / columns back to back: sum of H / sum of W entries).  Two
 *   launches whatever n_pages is: the counts - the three quarters of every page that lie in a band are read once, 4 bytes
 *   per lane, and the tiles' partial counts are added with int32 atomics to zeroed workspace of the context, so the
 *   counts do not depend on the order - then the runs and the rule, one wave per page and side.
 *   asr_crop_pages_dev copies rows [r0, r1) x columns [c0, c1) of page p to byte out_offsets[p] of out_dev (out_bytes its
 *   size), rows of c1 - c0 bytes back to back, in one launch; out_dev must not overlap pages_dev; bytes that belong to no
 *   output page are left as they are.  The rects are the caller's: the estimate's, or any other.
 *   Both: rows at any alignment on both sides.  Before anything is launched: 1 <= H, W <= 16384, the ranges above,
 *   0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W, every page and every output inside its buffer, and the overlap above.  A
 *   violation returns ASR_ERR_INVALID with a message that starts with "crop_pages:" and writes nothing.  n_pages == 0 is
 *   valid and writes nothing.
 * asr_score_map_dev = the measures of every piece in strip coordinates: the way back from a column x of an unrolled strip
 *   to a bar, a page, a staff system and a page position.  The reference has no such stage (its detect_bars gives blobs on
 *   a page, its alignment raises for a system without a bar and knows nothing of strips); the yardstick is this
 *   definition, all in integers after one comparison, which sheet_utils/omr.strip_bar_counts_host / strip_bar_lines_host
 *   / score_map_host restate in numpy and the device reproduces exactly.
 *   Inputs: the bar network's float64 maps of all pages back to back on the device (page p of H x W at the sum of the
 *   sizes before it, as asr_seg_predict_dev writes and asr_bars_from_map_dev reads them; maps_doubles = their total);
 *   `systems`, the table asr_unroll_systems_dev takes - host int32[n_systems * 8]: page, r0, r1, c0, c1, pad, piece,
 *   strip x0 - with the pieces in non-decreasing order; system_index: host int32[n_systems], the system's index among
 *   its page's detected systems; page_in_piece: host int32[n_pages], the page's index within its piece.
 *     count     count[c] = #{ r in [r0, r1) : map[r][c] > threshold }  for c in [c0, c1)     (a NaN is not above)
 *     lines     a bar line is a maximal run of consecutive columns with count >= min_rows; its column is
 *               b = (first + last) / 2 (integer division)
 *     interior  a line is interior when b - c0 > tol and (c1 - 1) - b > tol; the others merge into the system's edges
 *     bounds    B = c0, the interior lines in ascending order, c1
 *     measures  measure j of a system covers page columns B[j] .. B[j+1] - 1; a system without an interior line is one
 *               measure.  The measures of a piece are numbered from 0 in the table's order (the systems of a page, then
 *               the pages of the piece).  One int32 row of 8 per measure:
 *                 x0, x1 (strip columns, half open: strip x0 + B[j] - c0, strip x0 + B[j+1] - c0), page (within its
 *                 piece), system (on its page), col0 = B[j], col1 = B[j+1], row0 = r0, row1 = r1
 *   Outputs (host): measures int32[n_systems * (max_lines + 1) * 8], of which the first *n_measures rows are written, the
 *   pieces back to back; piece_first int32[n_pieces + 1], the first row of every piece and the total (a piece without a
 *   kept system has none); *overflow_system = -1, or the first system with more than max_lines interior lines - then no
 *   row is written and *n_measures is 0 (the call still returns ASR_OK: the caller names the system).
 *   Three launches whatever n_pages and n_systems are (score_map_kernels.hip): the counts and the flags of 64 columns per
 *   workgroup, lanes along the columns; the runs, their centres and the interior lines in column order by a scan, one
 *   wave per system; the numbering by a scan over the systems that restarts at every piece.  No atomics: the table is
 *   deterministic.  Every element of every band is read once.  Before anything is launched: every page inside
 *   maps_doubles, every system inside its page (0 <= r0 < r1 <= H, 0 <= c0 < c1 <= W), 1 <= min_rows, 0 <= tol,
 *   0 <= max_lines, pieces in [0, n_pieces) and in order, threshold not a NaN.  A violation returns ASR_ERR_INVALID with a
 *   message that starts with "score_map:" and writes nothing.  n_systems == 0 is valid: piece_first is all 0. */
int asr_score_map_dev(asr_ctx *ctx, const double *maps_dev, int64_t maps_doubles, const int32_t *heights,
                      const int32_t *widths, int n_pages, const int32_t *page_in_piece, const int32_t *systems,
                      const int32_t *system_index, int n_systems, int n_pieces, double threshold, int min_rows, int tol,
                      int max_lines, int32_t *measures, int32_t *piece_first, int32_t *n_measures,
                      int32_t *overflow_system);
int asr_unroll_systems_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                           const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *systems,
                           int n_systems, int system_height, const int64_t *strip_offsets, const int32_t *strip_widths,
                           int n_pieces, float *strips_dev, int64_t strips_floats);
int asr_spectrogram_batch_dev(asr_ctx *ctx, const float *samples_dev, int64_t samples_floats,
                              const int64_t *sample_offsets, const int64_t *sample_counts, const int64_t *n_frames,
                              const int64_t *out_offsets, int n_recordings, int frame_size, double hop,
                              const float *window, const int32_t *fb_start, const int32_t *fb_len,
                              const float *fb_weights, int n_filters, float mul, float add, int transposed,
                              float *out_dev, int64_t out_floats);
int asr_spectrogram_fft_batch_dev(asr_ctx *ctx, const float *samples_dev, int64_t samples_floats,
                                  const int64_t *sample_offsets, const int64_t *sample_counts, const int64_t *n_frames,
                                  const int64_t *out_offsets, int n_recordings, int frame_size, double hop,
                                  const float *window, const int32_t *fb_start, const int32_t *fb_len,
                                  const float *fb_weights, int n_filters, float mul, float add, int transposed,
                                  float *out_dev, int64_t out_floats);
int asr_resample_batch_dev(asr_ctx *ctx, const float *in_dev, int64_t in_floats, const int64_t *in_offsets,
                           const int64_t *in_counts, const int64_t *out_offsets, const int64_t *out_counts,
                           int n_recordings, int up, int down, const double *taps_phase_major, int taps_per_phase,
                           int half, int round_int16, float *out_dev, int64_t out_floats);
int asr_audio_stream_push_dev(asr_ctx *ctx, const float *blocks_dev, int64_t blocks_floats, const int64_t *block_offsets,
                              const int64_t *block_counts, const int64_t *samples_before, const int32_t *final,
                              const int64_t *first_frames, const int64_t *n_new_frames, const int64_t *out_offsets,
                              int n_streams, int up, int down, const double *taps_phase_major, int taps_per_phase,
                              int half, int round_int16, float *state_dev, int64_t state_floats,
                              const int64_t *state_offsets, int64_t state_cap, int frame_size, double hop,
                              const float *window, const int32_t *fb_start, const int32_t *fb_len,
                              const float *fb_weights, int n_filters, float mul, float add, int transposed,
                              float *out_dev, int64_t out_floats);
int asr_audio_stream_push_fft_dev(asr_ctx *ctx, const float *blocks_dev, int64_t blocks_floats,
                                  const int64_t *block_offsets, const int64_t *block_counts,
                                  const int64_t *samples_before, const int32_t *final, const int64_t *first_frames,
                                  const int64_t *n_new_frames, const int64_t *out_offsets, int n_streams, int up, int down,
                                  const double *taps_phase_major, int taps_per_phase, int half, int round_int16,
                                  float *state_dev, int64_t state_floats, const int64_t *state_offsets, int64_t state_cap,
                                  int frame_size, double hop, const float *window, const int32_t *fb_start,
                                  const int32_t *fb_len, const float *fb_weights, int n_filters, float mul, float add,
                                  int transposed, float *out_dev, int64_t out_floats);
int asr_resize_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                         const int32_t *heights, const int32_t *widths, int n_pages, const int64_t *out_offsets,
                         const int32_t *out_heights, const int32_t *out_widths, void *out_dev, int64_t out_bytes);
int asr_skew_estimate_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, int max_slope, int32_t *slopes,
                          int64_t *scores);
int asr_deskew_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                         const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *slopes, int fill,
                         void *out_dev, int64_t out_bytes);
int asr_flatten_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *radii, int floor,
                          void *out_dev, int64_t out_bytes, void *background_dev);
int asr_crop_estimate_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, int floor, int share,
                          const int32_t *margins, int32_t *rects, int32_t *status, int32_t *row_counts,
                          int32_t *col_counts);
int asr_crop_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                       const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *rects,
                       const int64_t *out_offsets, void *out_dev, int64_t out_bytes);

/* ---- device memory (plain pointers; library-owned allocations) ---------- */
int asr_dev_alloc(asr_ctx *ctx, size_t bytes, void **dptr);
int asr_dev_free(asr_ctx *ctx, void *dptr);
int asr_dev_upload(asr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int asr_dev_download(asr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- per-kernel timing (HIP events on the ctx stream) -------------------
 * The reference only prints wall-clock "ups" (utils/train_dcca_pool.py:221-231);
 * bench.py needs per-kernel durations for the roofline line. */
int asr_profile_enable(asr_ctx *ctx, int on);
/* symbol != NULL / "": only launches of that kernel symbol are bracketed by events (the measurement then costs two
 * events per step instead of two per kernel); NULL or "" = every kernel */
int asr_profile_filter(asr_ctx *ctx, const char *symbol);
int asr_profile_reset(asr_ctx *ctx);
int asr_profile_count(asr_ctx *ctx);
int asr_profile_get(asr_ctx *ctx, int index, char *name, int name_cap,
                    int64_t *launches, double *total_ms, double *flops, double *bytes);
/* kernel symbol (as rocprofv3 --kernel-trace prints it) behind record `index`;
 * empty for labels that cover several kernels */
int asr_profile_symbol(asr_ctx *ctx, int index, char *symbol, int symbol_cap);

/* ---- debugging aid for the parity tests ---------------------------------
 * Copies the NHWC activation of conv block `block` (0..7, after BN/ELU and the
 * max-pool where the block has one) of tower `view` (1|2), as left by the last
 * embed call, for its first n samples; *h,*w,*c receive its geometry.  `out`
 * may be NULL to query the geometry only. */
int asr_debug_activation(asr_ctx *ctx, int view, int block, int64_t n,
                         float *out, int *h, int *w, int *c);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
