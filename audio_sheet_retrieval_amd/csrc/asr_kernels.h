// Internal launcher interface between the C-ABI layer (asr_api*.hip, asr_ctx.h) and the
// gfx950 kernels.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include <algorithm>

namespace asr {

// Train-mode BatchNorm output of one raw element, y = (v - mu) * (gamma * inv_std) + beta, as ONE explicit sequence
// (subtract, fused multiply-add): the pooling forward (bn_apply_elu_pool_kernel), both passes of the backward
// (bn_bwd_*_kernel) and the debug export (pool_mask_kernel) decide "is this element a maximum of its window" by comparing
// these values for EQUALITY, so all of them must round the same way whatever the compiler would have contracted.
__device__ __forceinline__ float bn_affine(float v, float mu, float sc, float be) { return __fmaf_rn(v - mu, sc, be); }

// ---- first block: conv3x3 (C_in = 1) + BN + ELU, prepare() folded in -------
// in_mode: ASR_IN_* of asr_hip.h.  Hraw/Wraw: raw sheet size; H/W: network
// resolution (= raw, or raw/2 when rsz).  w: [COUT][9] correlation-form taps,
// bnp: [3][COUTP] (mean, gamma*inv_std, beta).
hipError_t launch_conv1(hipStream_t s, const void *in, int in_mode, int rsz,
                        const float *w, const float *bnp, float *out,
                        int N, int Hraw, int Wraw, int H, int W, int cout);

const char *conv1_symbol(int cout, int in_mode, int rsz, int N, int H, int W, int Hraw, int Wraw);

// ---- blocks 2..8: conv3x3 (C_in >= 12) as implicit GEMM on fp32 MFMA -------
struct ConvPlan {           // chosen on the host per layer geometry
    int cin, cout, pool;
    int H, W, OH, OW;
    int TH, TW, NI;         // tile: NI images x TH x TW output pixels (pre-pool)
    int tiles_y, tiles_x;
    int threads, lds_bytes, blocks_per_cu;
    int tile_floats;        // v2: floats of one LDS tile buffer
    double cost;            // planner's model cost (relative)
    int fuse1;              // block 1 evaluated inside this (block 2) kernel
    int variant;            // index into the instantiation table
    const char *symbol;     // kernel symbol as rocprofv3 prints it
    int c4p, rp;            // Winograd schedule: LDS patch layout (chunks per pixel / per row)
    int epi;                // conv3x3_wino4s: rows-full M-tiles take the branch-free epilogue (ASR_WINO4_EPI)
};
// Returns false when no instantiation exists for (cin, cout, pool).
// raw = 1: plain convolution output (no BN/ELU/pool) - train-mode forward and data gradients
bool plan_conv(int cin, int cout, int pool, int H, int W, ConvPlan *plan, int raw = 0, int fuse1 = 0);
struct Fuse1Args {          // what a fuse1 plan needs instead of the block-1 activation
    const void *raw; const float *w1; const float *bn1; int in_mode, rsz, Hraw, Wraw;
};
void conv_candidates_v1(int cin, int cout, int pool, int H, int W, int raw, int max_count, std::vector<ConvPlan> *out,
                        int fuse1 = 0);
void conv_candidates_v2(int cin, int cout, int pool, int H, int W, int max_count, std::vector<ConvPlan> *out);
// second-generation schedule (conv_v2_kernels.hip); plan.variant >= 1000 marks a v2 plan
bool plan_conv_v2(int cin, int cout, int pool, int H, int W, ConvPlan *plan);
hipError_t launch_conv_v2(hipStream_t s, const ConvPlan &p, const float *in, const float *wpk,
                          const float *bnp, float *out, int N, int num_cus);
// third schedule for the small-K blocks (conv_v3_kernels.hip); plan.variant >= 2000 marks a v3 plan
void conv_candidates_v3(int cin, int cout, int pool, int H, int W, int max_count, std::vector<ConvPlan> *out,
                        int fuse1 = 0);
bool plan_conv_v3_raw(int cin, int cout, int H, int W, ConvPlan *plan);
hipError_t launch_conv_v3(hipStream_t s, const ConvPlan &p, const float *in, const float *wpk,
                          const float *bnp, float *out, int N, int num_cus, const Fuse1Args *f1 = nullptr);
// Winograd F(2x2,3x3) schedule (conv_wino_kernels.hip); plan.variant >= 3000 marks such a plan (plan.NI = MY).
// Its transformed weights live behind the direct-form fragments in the same buffer: wpk + conv_wpack_floats().
void conv_candidates_wino(int cin, int cout, int pool, int H, int W, int max_count, std::vector<ConvPlan> *out);
// stats / stats_rows: RAW (training) plans only - the kernel also writes the partial table of its outputs'
// per-channel sums for the BatchNorm statistics ([rows][2][C_out] float64; launch_bn_stats_final reduces it)
// f1: plans with fuse1 set (block 1 evaluated inside by producer waves) read the raw input instead of `in`
hipError_t launch_conv_wino(hipStream_t s, const ConvPlan &p, const float *in, const float *wino_wpk,
                            const float *bnp, float *out, int N, int num_cus, double *stats = nullptr,
                            int *stats_rows = nullptr, const Fuse1Args *f1 = nullptr);
// what launch_conv_wino launches for plan p on N images: its work items (M-tiles of 16 tiles in the global-A form,
// regions in the LDS-patch form) and its workgroups along x (each repeated per group of n-tiles)
void conv_wino_launch_shape(const ConvPlan &p, int N, int num_cus, int *items, int *grid_x);
void conv_candidates_wino_fused(int cin, int cout, int pool, int H, int W, int max_count, std::vector<ConvPlan> *out);
const char *conv_wino_symbol(const ConvPlan &p, int in_mode);
int conv_wino_stats_rows_max(int num_cus);
size_t wino_wpack_floats(int cin, int cout);
// W: master weights [cout][cin][3][3] (Lasagne convolution form) on the device
// dgrad = 1: the data-gradient convolution's weights (contraction over cout, outputs cin)
hipError_t launch_wino_pack(hipStream_t s, const float *W, int cin, int cout, float *wino_wpk, int dgrad = 0);
bool plan_conv_wino_raw(int cin, int cout, int H, int W, ConvPlan *plan);
void conv_candidates_wino_raw(int cin, int cout, int H, int W, int max_count, std::vector<ConvPlan> *out);
// Winograd F(4x4,3x3), global-A form (conv_wino4_kernels.hip); plan.variant >= 4000.  Its weights follow the
// F(2x2,3x3) ones in the layer's weight buffer: wpk + conv_wpack_floats() + wino_wpack_floats()
void conv_candidates_wino4(int cin, int cout, int pool, int H, int W, std::vector<ConvPlan> *out);
hipError_t launch_conv_wino4(hipStream_t s, const ConvPlan &p, const float *in, const float *wino4_wpk,
                             const float *bnp, float *out, int N, int num_cus, double *stats = nullptr,
                             int *stats_rows = nullptr);
// M-tiles and workgroups along x of launch_conv_wino4 for plan p on N images
void conv_wino4_launch_shape(const ConvPlan &p, int N, int num_cus, int *items, int *grid_x);
// RAW (training) builds of conv3x3_wino4s: candidates of the training step's tuner for a block's forward convolution
// (cin, cout; dgrad = 0: only with ASR_TRAIN_WINO4=1, see conv_wino4_kernels.hip) or data gradient (cout, cin; dgrad =
// 1); their statistics table has one row per workgroup
void conv_candidates_wino4_raw(int cin, int cout, int H, int W, std::vector<ConvPlan> *out, int dgrad);
bool conv_wino4_is_raw(const ConvPlan &p);
int conv_wino4_stats_rows_max(int num_cus);
size_t wino4_wpack_floats(int cin, int cout);
hipError_t launch_wino4_pack(hipStream_t s, const float *W, int cin, int cout, float *wino4_wpk, int dgrad = 0);
size_t conv_wpack_floats(int cin, int cout);
// Wcorr: [9][cin][cout] correlation-form taps -> MFMA fragment order.
void pack_conv_weights(const float *wcorr, int cin, int cout, float *wpk);
hipError_t launch_conv(hipStream_t s, const ConvPlan &p, const float *in, const float *wpk,
                       const float *bnp, float *out, int N, int num_cus, const Fuse1Args *f1 = nullptr);

// ---- tail: 1x1 conv + BN + global mean (+ CCA projection + length norm) ----
// a8: [N, h, w, c8] NHWC; w9: [32][c8]; bnp9: [3][32]; cca_mean: [32];
// cca_proj: [32][32] (U or V, row-major, rows = input dim).
// features (N,32) and/or latent (N,32) may be null.
hipError_t launch_tail(hipStream_t s, const float *a8, int N, int h, int w, int c8,
                       const float *w9, const float *bnp9, const float *cca_mean,
                       const float *cca_proj, float *features, float *latent);

// ---- ranking ---------------------------------------------------------------
hipError_t launch_row_norms(hipStream_t s, const float *x, int64_t n, int64_t ld, int dim, double *norms);
// rn2_pre (may be null): (float)(1 / norm2[j]) of every candidate, padded to a multiple of 4 - a resident data base
// brings them along, otherwise they are derived into the workspace
hipError_t launch_rank(hipStream_t s, const float *lv1, const double *norm1, int64_t n1, int64_t ld1,
                       const float *lv2, const double *norm2, int64_t n2, int64_t ld2, int dim,
                       int64_t query_offset, int64_t k, int64_t h,
                       int32_t *ranks, double *dstar, int32_t *ties, void *workspace = nullptr,
                       const float *rn2_pre = nullptr);
// workspace of the MFMA counting path of launch_rank (candidate sets >= 2048)
size_t rank_workspace_bytes(int64_t n1, int64_t n2);

// resident code data base (32-d packed rows): float64 norms [n], fp32 reciprocal norms [n rounded up to 4, zero
// padded], unit-length fp32 copy of the rows [n][32] - one pass over the pool
hipError_t launch_db_prepare(hipStream_t s, const float *x, int64_t n, double *norms, float *rn, float *unit);

// top-k smallest cosine distances per query (exact float64, stable index order); k <= 128
// workspace (topk_workspace_bytes; may be null): enables the fp32-MFMA filter stage in front of the exact scan
// unit / rn_db_pre (may be null): the resident data base's unit-length rows / reciprocal norms
size_t topk_workspace_bytes(int64_t n_db, int64_t n_q, int k, bool unit, bool fuse_rank);
hipError_t launch_topk(hipStream_t s, const float *db, const double *norm_db, int64_t n_db, int64_t ld_db,
                       const float *q, const double *norm_q, int64_t n_q, int64_t ld_q, int dim, int k,
                       int64_t idx_offset, int32_t *idx_out, double *dist_out, void *workspace,
                       const float *unit = nullptr, const float *rn_db_pre = nullptr, double *norm_q_pending = nullptr,
                       unsigned *tickets = nullptr);
// tickets (may be null): 4096 zero-initialised ints that stay zero between calls (1024 tickets, then the sort-free refine's
// per-query counts and flags) - the small dependent launches of
// the few-queries shape (threshold select, merge of the partial lists) are then done by the last workgroup to arrive in
// the kernel in front of them
// (norm_q_pending == norm_q: the query norms are NOT computed yet - launch_topk does it, inside the seeding kernel where
// that path runs, by launch_row_norms otherwise)
// a shard of a larger pool (rows [item_offset, ...) of n2_global): d* / global j* of the queries whose correct candidates
// it holds; the fused pass with d* / j* given, leaving the rank COUNTERS [n_q][3] (summed over the shards by the caller);
// the merge of top-k lists gathered from the shards ([part][n_q_total][k]); counters -> ranks
hipError_t launch_rank_dstar(hipStream_t s, const float *q, const double *norm_q, int64_t n_q, const float *db,
                             const double *norm_db, int64_t n_db, int64_t item_offset, int64_t n2_global,
                             int64_t query_offset, int64_t kk, int64_t hh, double *dstar, int64_t *jstar);
hipError_t launch_topk_count_db(hipStream_t s, const float *db, const float *unit, const double *norm_db, int64_t n_db,
                                const float *q, const double *norm_q, int64_t n_q, int k, int64_t idx_offset,
                                int32_t *idx_out, double *dist_out, const double *dstar, const int64_t *jstar,
                                int32_t *counts, void *workspace);
hipError_t launch_topk_merge(hipStream_t s, const int32_t *part_idx, const double *part_dist, int n_parts, int64_t n_q_total,
                             int64_t q_lo, int64_t n_q, int k, int32_t *idx_out, double *dist_out);
hipError_t launch_rank_finish(hipStream_t s, const int32_t *counts, const double *dstar, int64_t n, int32_t *ranks,
                              double *dstar_out, int32_t *ties);
// top-k and eval_retrieval ranks from one walk over the pool (needs topk_rank_fusable; 32-d packed rows)
bool topk_rank_fusable(int64_t n_db, int64_t kk);
hipError_t launch_topk_rank_db(hipStream_t s, const float *db, const float *unit, const double *norm_db, int64_t n_db,
                               const float *q, const double *norm_q, int64_t n_q, int k, int64_t idx_offset,
                               int32_t *idx_out, double *dist_out, int64_t query_offset, int64_t kk, int64_t hh,
                               int32_t *ranks, double *dstar, int32_t *ties, void *workspace);

// ---- alignment: cosine distance matrix + DTW (utils/alignment.py, utils/dtw_by_dist.py) ----
// D: (R+1)*(C+1) doubles workspace; dist_out: R*C doubles or null; path_*: R+C entries, reversed order
hipError_t launch_dtw(hipStream_t s, const float *a, const double *na, int64_t R, int64_t lda, const float *b,
                      const double *nb, int64_t C, int64_t ldb, int dim, double *D, double *dist_out, int32_t *path_i,
                      int32_t *path_j, int32_t *path_len, double *min_dist);

// ---- batched alignment DTW (dtw_batch_kernels.hip): every pair of a batch in one launch per stage ----
// one pair of a chunk; offsets count elements of the chunk's device arrays
struct DtwPair {
    int32_t R, C;          // rows (a) / columns (b) of the pair's cost matrix
    int64_t a_row, b_row;  // first code row of the pair in a / b
    int64_t cell;          // first cell in the anti-diagonal-major cost / direction arrays (R*C cells per pair)
    int64_t diag;          // first anti-diagonal in the chunk's numbering (R+C-1 per pair)
    int64_t rm;            // first element of the row-major distance copy, or -1
    int64_t path;          // first path entry (capacity R+C)
    int64_t ring;          // first double of the pair's global ring (3*(min(R,C)+1)), or -1: the ring is in LDS
    int64_t fa, fb;        // first entry of the pair's first-entry projections (R / C entries)
};
// anti-diagonal slots (min(R,C)+1) one workgroup can keep in LDS: 3 buffers of doubles
int dtw_batch_lds_slots(int device);
hipError_t launch_dtw_batch_dist(hipStream_t s, const DtwPair *pairs, int n_pairs, int64_t n_diags, const float *a,
                                 const double *na, const float *b, const double *nb, int dim, double *cost,
                                 double *rm_out);
// lds_slots: dynamic LDS of the LDS-ring pairs (0: none); any_ring: some pair has a global ring
hipError_t launch_dtw_batch_wave(hipStream_t s, const DtwPair *pairs, int n_pairs, int lds_slots, bool any_ring,
                                 const double *cost, uint8_t *dir, double *ring, double *min_dist);
// first_a / first_b may be null
hipError_t launch_dtw_batch_traceback(hipStream_t s, const DtwPair *pairs, int n_pairs, const uint8_t *dir,
                                      int32_t *path_a, int32_t *path_b, int32_t *path_len, int32_t *first_a,
                                      int32_t *first_b);

// ---- batched subsequence DTW (dtw_subseq_kernels.hip): distances, wavefront and traceback fused, one workgroup per pair
struct SubseqPair {
    int32_t Q, S;          // query rows (one lane each, <= 1024) / reference rows
    int64_t q_row, r_row;  // first code row in q / r
    int64_t dir;           // first direction byte: cell (i, j) at (i + j) * Q + i, Q * (S + Q - 1) bytes
    int64_t pos;           // first entry of the pair's pos (Q entries) in the chunk's array
    int32_t out;           // index of the pair's cost / start / end / path_len in the chunk's arrays
    int32_t pad;
};
// LDS one workgroup of `waves` waves needs to stage reference rows of `dim` floats (0: dim out of range)
size_t dtw_subseq_lds_bytes(int waves, int dim);
// `pairs`: n_pairs entries that all take `waves` = ceil(Q / 64) waves.  lds_limit: LDS one workgroup may use; a
// workgroup whose staging ring does not fit reads the reference rows from global memory instead (same results).
// nq / nr: float64 norms of the rows of q / r, indexed like q / r.  pos may be null.
hipError_t launch_dtw_subseq(hipStream_t s, const SubseqPair *pairs, int n_pairs, int waves, size_t lds_limit,
                             const float *q, const double *nq, const float *r, const double *nr, int dim, uint8_t *dir,
                             double *cost, int32_t *start, int32_t *end, int32_t *path_len, int32_t *pos);

// ---- streaming subsequence DTW (dtw_follow_kernels.hip): a block of query rows continues a carried row, one workgroup
// per pair, no per-cell memory
struct FollowPair {
    int32_t B, S;          // new query rows (one lane each, <= 1024) / reference rows
    int64_t q_row, r_row;  // first code row in q / r
    int64_t state;         // first of the pair's S entries in acc / org
    int64_t out;           // first of the pair's B entries in cost / start / pos
    int32_t n0;            // query rows the state has consumed (0: fresh, the state is not read)
    int32_t pad;
};
// as dtw_subseq_lds_bytes (same ring)
size_t dtw_follow_lds_bytes(int waves, int dim);
// `pairs`: n_pairs entries that all take `waves` = ceil(B / 64) waves; lds_limit, nq / nr as for launch_dtw_subseq.
// acc / org: the state buffers, updated in place; the pairs' ranges must not overlap.
hipError_t launch_dtw_follow(hipStream_t s, const FollowPair *pairs, int n_pairs, int waves, size_t lds_limit,
                             const float *q, const double *nq, const float *r, const double *nr, int dim, double *acc,
                             int32_t *org, double *cost, int32_t *start, int32_t *pos);

// ---- piece-identification vote (audio_sheet_server.py:213-300) -----------------
hipError_t launch_slice_windows(hipStream_t s, const float *src, int64_t T, int r0, int win_h, int win_w,
                                const int32_t *starts_dev, int n, float *out);
// counts_ws: n_pieces int32 workspace; out_piece/out_count: top_k entries (piece -1 / count 0 when fewer voted)
hipError_t launch_piece_vote(hipStream_t s, const int32_t *idx, int64_t n_idx, const int32_t *ids, int64_t n_db,
                             int32_t n_pieces, int top_k, int32_t *counts_ws, int32_t *out_piece, int32_t *out_count);

// ---- batched piece vote (piece_vote_batch_kernels.hip): n_groups query pieces in one launch ----
// groups with n_pieces <= VOTE_LDS_PIECES keep counters and sort keys in LDS (48 KiB per workgroup); larger ones use
// hist_ws (n_groups * n_pieces int32, zeroed by the launcher) and keys_ws (n_groups * keys_cap uint64, keys_cap a power
// of two >= min(n_pieces, per_group)).  All pointers on the device; targets / ranks / ratios may be null together.
constexpr int VOTE_LDS_PIECES = 4096;
struct VoteBatchArgs {
    const int32_t *idx; int64_t n_groups, per_group;
    const int32_t *ids; int64_t n_db; int32_t n_pieces; int top_k;
    const int32_t *targets;
    int32_t *pieces, *counts, *n_out, *ranks; double *ratios;
    int32_t *hist_ws; uint64_t *keys_ws; int64_t keys_cap;
};
hipError_t launch_piece_vote_batch(hipStream_t s, const VoteBatchArgs &a, bool global_path);

// ---- running piece vote (track_kernels.hip): AudioSheetServer.run (audio_sheet_server.py:83-211) over recordings ----
// music gate: recordings (bins, frames) float32 row-major at float offset `off` of src; `first` = the recording's first
// entry in the concatenated per-frame arrays (ascending); frame0 = the stream position of its column 0 (0 offline);
// has_norm: norm replaces spec.sum(axis=0).max().  All pointers on the device.
struct TrackRec {
    int64_t off, first, frame0;
    int32_t bins, frames;
    float norm; int32_t has_norm;
};
struct TrackGateArgs {
    const float *src; const TrackRec *recs; int n_rec; int64_t total_frames; int width;
    float *colsum, *level;              // workspace: total_frames / n_rec floats
    float *m_prob; uint8_t *voiced;     // total_frames each
};
hipError_t launch_track_gate(hipStream_t s, const TrackGateArgs &a);
hipError_t launch_track_colsum(hipStream_t s, const TrackGateArgs &a);                  // its first launch alone
// sliding vote: one wave per segment = frames f0 .. f0 + n - 1 of a recording whose frame f is row row0 + f of the
// (rows x n_candidates) top-k index table; frame f0 + i writes output row out0 + i.  n_pieces <= TRACK_LDS_PIECES keeps
// the counters in LDS (16 KiB), larger ones use hist_ws (grid * n_pieces int32, zeroed by the launcher).
constexpr int TRACK_LDS_PIECES = 4096;
struct TrackSeg { int64_t row0, f0, out0; int32_t n, pad; };
struct TrackVoteArgs {
    const int32_t *idx; const TrackSeg *segs; int64_t n_segs;
    int n_candidates, running_frames;
    const int32_t *ids; int64_t n_db; int32_t n_pieces; int top_k;
    int32_t *pieces, *counts, *n_out;
    int32_t *hist_ws;
};
hipError_t launch_track_vote(hipStream_t s, const TrackVoteArgs &a, int grid, bool global_path);

// ---- the same loop for parallel streams with carried device state (track_stream_kernels.hip) ----
// gate: stream s brings n_new columns as a (bins, n_new) row-major block at float col_off of cols; its state is the
// (bins, width - 1) row-major block at tail_off of tail (not read with frames_before == 0).  first = its first entry in
// the per-frame arrays, ext_first = its first entry in colsum, which holds the width - 1 + n_new column sums of
// [tail | new] for every stream with n_new > 0.  slot (total_frames + 1): the exclusive running count of voiced frames
// = the window a voiced frame writes; win = total voiced windows (bins x width).  All pointers on the device.
struct TrackStreamRec {
    int64_t col_off, tail_off, frames_before, first, ext_first;
    int32_t n_new; float level;
};
struct TrackStreamGateArgs {
    const float *cols; float *tail; const TrackStreamRec *recs; int n_streams; int64_t total_frames, total_ext;
    int bins, width;
    float *colsum; int32_t *slot;       // workspace: total_ext floats / total_frames + 1 counts
    float *win;
    float *m_prob; uint8_t *voiced; int32_t *n_voiced;
};
hipError_t launch_track_stream_gate(hipStream_t s, const TrackStreamGateArgs &a);       // column sums, gate, slots
hipError_t launch_track_stream_colsum(hipStream_t s, const TrackStreamGateArgs &a);     // its first launch alone
hipError_t launch_track_stream_windows(hipStream_t s, const TrackStreamGateArgs &a);    // windows, then the tails
// vote: one wave per segment = voiced frames v0 .. v0 + n - 1 (counted over the stream's life) of a stream with vb
// voiced frames before this call, whose new rows start at row row0 of idx; frame v >= vb is row row0 + v - vb (its
// output row too), an earlier one slot v mod (running_frames - 1) of the ring at hist_off of ring.  After the votes the
// last min(n_new, running_frames - 1) new rows of every stream in `keeps` (n_keep entries) are stored in their slots.
struct TrackStreamSeg { int64_t row0, v0, vb, hist_off; int32_t n, pad; };
struct TrackStreamKeep { int64_t row0, vb, hist_off; int32_t n_new, pad; };
struct TrackStreamVoteArgs {
    const int32_t *idx; const TrackStreamSeg *segs; int64_t n_segs; int64_t n_rows;
    const TrackStreamKeep *keeps; int n_keep;
    int n_candidates, running_frames;
    const int32_t *ids; int64_t n_db; int32_t n_pieces; int top_k;
    int32_t *ring;
    int32_t *pieces, *counts, *n_out;
    int32_t *hist_ws;
};
hipError_t launch_track_stream_vote(hipStream_t s, const TrackStreamVoteArgs &a, int grid, bool global_path);

// ---- the gate at the level of what has been heard so far (track_level_kernels.hip) ----
// level of new frame k of sequence q (a recording, or a stream's round) = fmaxf(floor, max of the last `memory` column
// sums up to its own; memory == 0: of all).  A sequence is ext = [its n_hist carried values in frame order | its n_new
// new column sums, colsum[cs_first ..]]: with memory > 0 the carried values are the last n_hist = min(frames_before,
// memory - 1) column sums, frame f in slot f mod (memory - 1) of the ring at state_off of `state`; with memory == 0 the
// one float there, the maximum so far (n_hist = frames_before > 0).  out_first = its first entry in `level`, sfx_first =
// its first entry in `suffix` (n_hist + n_new floats per sequence, memory > 0 only), which holds per ext entry the
// maximum from it to the end of its block of `memory` entries.  last (n_seq): the maximum that memory == 0 carries on.
// All pointers on the device; state may be NULL where every n_hist is 0.
struct TrackLevelSeq {
    int64_t cs_first, out_first, sfx_first, state_off, frames_before;
    int32_t n_new, n_hist;
};
struct TrackLevelArgs {
    const float *colsum; const TrackLevelSeq *seqs; int n_seq; int memory; float floor;
    float *state;
    float *suffix, *last;               // workspace
    float *level;                       // per new frame
};
hipError_t launch_track_level(hipStream_t s, const TrackLevelArgs &a);                  // (suffix maxima,) levels
hipError_t launch_track_level_state(hipStream_t s, const TrackLevelArgs &a);            // behind them: the carried state
// the two gates with TrackLevelArgs::level per frame in place of the recording's / the stream's level
hipError_t launch_track_gate_running(hipStream_t s, const TrackGateArgs &a, const float *frame_level);
hipError_t launch_track_stream_gate_running(hipStream_t s, const TrackStreamGateArgs &a, const float *frame_level);

// ---- score following for parallel streams: the windows on the step grid and the code logs (follow_stream_kernels.hip) ----
// windows: stream s brings n_new columns as a (bins, n_new) row-major block at float col_off of cols; its state is the
// (bins, width - 1) block at tail_off of tail, counted as zeros and not read with has_tail == 0.  It completes n_win
// windows, numbered first .. first + n_win - 1 in win; window i of them starts at column c0 + i * step of [tail | new].
struct FollowStreamRec {
    int64_t col_off, tail_off, first, c0;
    int32_t n_new, n_win, has_tail, pad;
};
struct FollowStreamWinArgs {
    const float *cols; float *tail; float *win; const FollowStreamRec *recs; int n_streams; int64_t total_win;
    int bins, width, step;
};
hipError_t launch_follow_stream_windows(hipStream_t s, const FollowStreamWinArgs &a);   // windows, then the tails
// log: the last `kept` of the rows_in_log rows (dim floats each) at float log_off of log move to its front, and the
// n_new rows from row src_row of codes are copied behind them
struct FollowStreamLogRec { int64_t log_off, src_row; int32_t rows_in_log, kept, n_new, pad; };
struct FollowStreamLogArgs {
    const float *codes; float *log; const FollowStreamLogRec *recs; int n_streams; int dim; int64_t n_rows;
};
hipError_t launch_follow_stream_log(hipStream_t s, const FollowStreamLogArgs &a);

// autotuner self-check (ASR_TUNE_VERIFY=1): deterministic input pattern, max |a - b| as float bits
hipError_t launch_fill_pattern(hipStream_t s, float *p, int64_t n);
hipError_t launch_max_abs_diff(hipStream_t s, const float *a, const float *b, int64_t n, uint32_t *out_bits);
// audio front-end: framed, windowed |DFT| -> filterbank -> log10(mul * x + add); all pointers on the device
hipError_t launch_spectrogram(hipStream_t s, const float *samples, int64_t n_samples, const float *window, int frame_size,
                              double hop, int max_bin, const int32_t *fb_start, const int32_t *fb_len,
                              const int32_t *fb_off, const float *fb_w, int nf, float mul, float add, float *out,
                              int64_t n_frames, int transposed);
// the same for n_rec recordings in one launch: frame_first (n_rec + 1 running frame counts), sample_off / sample_cnt /
// out_off (per recording, in floats) on the device; bit-identical per recording with launch_spectrogram
hipError_t launch_spectrogram_batch(hipStream_t s, const float *samples, const int64_t *frame_first,
                                    const int64_t *sample_off, const int64_t *sample_cnt, const int64_t *out_off, int n_rec,
                                    int64_t total_frames, const float *window, int frame_size, double hop, int max_bin,
                                    const int32_t *fb_start, const int32_t *fb_len, const int32_t *fb_off, const float *fb_w,
                                    int nf, float mul, float add, float *out, int transposed);
// the batched spectrogram with the magnitudes from a real-input FFT (spectrogram_fft_kernels.hip; frame_size 2048 only):
// the per-recording tables as launch_spectrogram_batch; twiddles: 2048 (cos, -sin) pairs of exp(-2 pi i t / 2048),
// float32 rounded from float64; window: the 2048 floats, 8-byte aligned.  Magnitudes equal to the DFT's within float32
// rounding; per recording bit-identical whatever else is in the launch
hipError_t launch_spectrogram_fft_batch(hipStream_t s, const float *samples, const int64_t *frame_first,
                                        const int64_t *sample_off, const int64_t *sample_cnt, const int64_t *out_off,
                                        int n_rec, int64_t total_frames, const float *twiddles, const float *window,
                                        double hop, const int32_t *fb_start, const int32_t *fb_len, const int32_t *fb_off,
                                        const float *fb_w, int nf, float mul, float add, float *out, int transposed);
// unrolled score strips (umc_kernels.hip): one row of the table per staff system, offsets resolved by the host
struct UnrollSystem {
    int64_t src;            // byte offset of (r0, c0) in the uint8 page buffer
    int64_t dst;            // float offset of (0, dst_col) in the strip buffer
    int32_t src_stride;     // page width
    int32_t dst_stride;     // strip width
    int32_t rows;           // r1 - r0: strip rows >= rows repeat source row rows - 1
    int32_t width;          // c1 - c0
};
hipError_t launch_unroll_systems(hipStream_t s, const uint8_t *pages, const UnrollSystem *systems_dev, int n_systems,
                                 int system_height, float *strips);
// recordings at another sample rate (resample_kernels.hip): rational polyphase resampling, one workgroup per tile of
// RESAMPLE_TILE consecutive outputs of one recording.  tile_first (n_rec + 1 running tile counts), in_off / in_cnt /
// out_off / out_cnt (per recording, in floats) and the phase-major float64 taps (up x taps_per_phase) on the device.
// A tile stages resample_span() input samples in LDS, which has to fit RESAMPLE_MAX_LDS bytes.
constexpr int RESAMPLE_TILE = 1024;
constexpr size_t RESAMPLE_MAX_LDS = 64 * 1024;
int resample_span(int up, int down, int taps_per_phase);
hipError_t launch_resample_batch(hipStream_t s, const float *in, float *out, const int64_t *tile_first,
                                 const int64_t *in_off, const int64_t *in_cnt, const int64_t *out_off,
                                 const int64_t *out_cnt, int n_rec, int64_t total_tiles, int up, int down, int half,
                                 int taps_per_phase, const double *taps, int round_int16);
// spectrogram columns from streamed blocks (audio_stream_kernels.hip): one workgroup per new frame stages the frame's input
// span from [state | block], resamples its frame_size samples into LDS and runs the frame arithmetic; then one workgroup
// per stream slides the inputs the next frame reads to the front of the state.  One row per stream, on the device:
struct StreamRow {
    int64_t n0, n1;             // input samples of the stream before / after the call
    int64_t keep0, keep1;       // first input sample the state holds before / after the call (n0 == 0: keep0 = 0)
    int64_t first_frame, n_new; // the call's frames
    int64_t y_len;              // ceil(n1 * up / down): samples at the front-end's rate from here on are zero
    int64_t block_off, state_off, out_off;      // in floats
};
struct StreamResample {
    int up, down, half, taps_per_phase, span, round_int16;
    const double *taps;         // phase-major, on the device; nullptr: the front-end's own rate, y = x
};
// a frame's filters split over n workgroups: part p computes filters f[p] .. f[p + 1] - 1 and DFT bins k0[p] .. k1[p] - 1
constexpr int STREAM_MAX_PARTS = 8;
struct StreamParts { int n; int f[STREAM_MAX_PARTS + 1], k0[STREAM_MAX_PARTS], k1[STREAM_MAX_PARTS]; };
constexpr size_t AUDIO_STREAM_MAX_LDS = 160 * 1024;
// input samples one frame reads: ceil((frame_size - 1) * down / up) + taps_per_phase
int audio_stream_span(int frame_size, int up, int down, int taps_per_phase);
size_t audio_stream_lds(int frame_size, int max_bin, int span);
hipError_t launch_audio_stream_frames(hipStream_t s, const float *blocks, const float *state, const int64_t *frame_first,
                                      const StreamRow *rows, int n_streams, int64_t total_frames, const StreamResample &r,
                                      const StreamParts &parts, const float *window, int frame_size, double hop, int max_bin,
                                      const int32_t *fb_start, const int32_t *fb_len, const int32_t *fb_off,
                                      const float *fb_w, int nf, float mul, float add, float *out, int transposed);
hipError_t launch_audio_stream_carry(hipStream_t s, const float *blocks, float *state, const StreamRow *rows,
                                     int n_streams);
// the same frames with the magnitudes from the real-input FFT (audio_stream_fft_kernels.hip; frame_size 2048 only): stage 1
// as launch_audio_stream_frames, then the frame plan of launch_spectrogram_fft_batch (twiddles, window: as there) - per
// frame bit-identical with it on the resampled recording.  One workgroup per frame, no split; the state is slid by
// launch_audio_stream_carry.  Its LDS never exceeds audio_stream_lds at the same span.
size_t audio_stream_fft_lds(int span);
hipError_t launch_audio_stream_fft_frames(hipStream_t s, const float *blocks, const float *state,
                                          const int64_t *frame_first, const StreamRow *rows, int n_streams,
                                          int64_t total_frames, const StreamResample &r, const float *twiddles,
                                          const float *window, double hop, const int32_t *fb_start, const int32_t *fb_len,
                                          const int32_t *fb_off, const float *fb_w, int nf, float mul, float add,
                                          float *out, int transposed);
// score pages at another resolution (page_resize_kernels.hip): exact integer area resampling, one 64-thread workgroup
// per tile of RESIZE_TILE_H x RESIZE_TILE_W output pixels of one page.  tile_first (n_pages + 1 running tile counts) and
// the page table on the device.  A tile stages its source rows in RESIZE_LDS_BYTES of LDS, chunk by chunk; one row of a
// tile at the ratio RESIZE_MAX_DOWN is 1025 bytes + alignment, so at least 7 rows fit.
constexpr int RESIZE_TILE_W = 64;
constexpr int RESIZE_TILE_H = 16;
constexpr int RESIZE_LDS_BYTES = 8 * 1024;
constexpr int RESIZE_BATCH = 8;             // 16-byte loads a lane issues before it waits for the first
constexpr int RESIZE_MAX_DOWN = 16;         // n_in <= RESIZE_MAX_DOWN * n_out per axis
constexpr int RESIZE_MAX_UP = 4;            // n_out <= RESIZE_MAX_UP * n_in per axis
constexpr int RESIZE_MAX_DIM = 1 << 24;     // every dimension: tile-relative positions and 255 * w_in stay in 32 bits
struct ResizePage {
    int64_t src;            // byte offset of the page in the source buffer
    int64_t dst;            // byte offset of the resized page in the output buffer
    int32_t h_in, w_in, h_out, w_out;
    int32_t tiles_x;        // column tiles of the output: ceil(w_out / RESIZE_TILE_W)
    int32_t pad;
};
hipError_t launch_resize_pages(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                               const ResizePage *table, int n_pages, int64_t total_tiles);
// skew of scanned pages (page_deskew_kernels.hip; include/asr_hip.h carries the definition).  Estimate: one 1024-thread
// workgroup per tile of SKEW_TILE_H rows x SKEW_TILE_W columns of one page keeps the tile's row prefix sums of the ink
// in LDS and adds, for every slope, the tile's share of the profile to the page's profiles in global memory (uint32
// atomics; integer addition commutes).  Then one workgroup per (page, slope) squares and sums a profile, and one thread
// per page picks the slope in the visiting order.
constexpr int SKEW_TILE_H = 32;
constexpr int SKEW_TILE_W = 448;            // a tile's prefix sums: 32 x 449 uint32 (the pitch is odd: no bank conflicts)
constexpr int SKEW_WAVES = 16;              // waves of a tile's workgroup: each takes every sixteenth slope
constexpr int SKEW_MAX_SLOPE = 128;
constexpr int SKEW_MAX_DIM = 16384;
struct SkewPage {
    int64_t src;            // byte offset of the page in the source buffer
    int64_t prof;           // first uint32 of the page's (2 * max_slope + 1) x len profiles in the profile workspace
    int32_t h, w;
    int32_t tiles_x;        // column tiles: ceil(w / SKEW_TILE_W)
    int32_t dm;             // d_max_slope(w - 1), the largest |d|: profile row r is kept at index r + dm
    int32_t len;            // h + 2 * dm
    int32_t pad;
};
hipError_t launch_skew_profiles(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const SkewPage *table,
                                int n_pages, int64_t total_tiles, int max_slope, uint32_t *prof);
hipError_t launch_skew_scores(hipStream_t s, const SkewPage *table, int n_pages, int max_slope, const uint32_t *prof,
                              int64_t *scores, int32_t *slopes);
// Correction: one 256-thread workgroup per tile of DESKEW_TILE_H rows x DESKEW_TILE_W columns of one output page, one
// column per thread; both shears in one pass (the intermediate pixel is rounded to uint8 as the definition says).
constexpr int DESKEW_TILE_H = 8;
constexpr int DESKEW_TILE_W = 256;
struct DeskewPage {
    int64_t off;            // byte offset of the page in the source buffer and of its result in the output buffer
    int32_t h, w;
    int32_t k;              // slope, in 1/1024
    int32_t tiles_x;        // column tiles: ceil(w / DESKEW_TILE_W)
};
hipError_t launch_deskew_pages(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                               const DeskewPage *table, int n_pages, int64_t total_tiles, int fill);
// paper of scanned pages (page_flatten_kernels.hip; include/asr_hip.h carries the definition).  Two launches: the dilate
// writes D, (h + 2r) x (w + 2r) bytes per page, to workspace; the erode reads it and writes the background and the divided
// page.  One 256-thread workgroup per tile of FLATTEN_TILE x FLATTEN_TILE results, its source with the halo of 2r in LDS.
constexpr int FLATTEN_TILE = 64;
constexpr int FLATTEN_THREADS = 256;
constexpr int FLATTEN_MAX_RADIUS = 127;
constexpr int FLATTEN_MAX_DIM = 16384;
struct FlattenPage {
    int64_t off;            // byte offset of the page in the source buffer, of its result and of its background
    int64_t d;              // byte offset of the page's D in the workspace of its chunk
    int32_t h, w;
    int32_t r;              // radius
    int32_t tiles_x_d;      // column tiles of D: ceil((w + 2r) / FLATTEN_TILE)
    int32_t tiles_x_p;      // column tiles of the page: ceil(w / FLATTEN_TILE)
    int32_t pad;
};
size_t flatten_lds_bytes(int radius);       // dynamic LDS of a workgroup at this radius (grows with it)
hipError_t launch_flatten_dilate(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const FlattenPage *table,
                                 int n_pages, int64_t total_tiles, int max_radius, uint8_t *dws);
hipError_t launch_flatten_erode(hipStream_t s, const uint8_t *pages, const uint8_t *dws, const int64_t *tile_first,
                                const FlattenPage *table, int n_pages, int64_t total_tiles, int max_radius, int floor_,
                                uint8_t *out, uint8_t *background);
// measures of the pieces in strip coordinates (score_map_kernels.hip; include/asr_hip.h carries the definition).  Three
// launches: the flags of SCORE_MAP_CHUNK columns per workgroup as one 64-bit word, the interior lines per system, the table.
constexpr int SCORE_MAP_CHUNK = 64;         // columns of a workgroup of the count kernel: one lane each
constexpr int SCORE_MAP_THREADS = 256;      // its threads: the band's rows go round its four waves
struct ScoreSystem {
    int64_t map;            // offset (doubles) of map[r0][c0] of the system's page
    int64_t chunk_first;    // the system's first flag word; it has ceil(width / SCORE_MAP_CHUNK)
    int32_t stride;         // the page's width
    int32_t rows, width;    // r1 - r0, c1 - c0
    int32_t r0, r1, c0;
    int32_t page, system;   // the page within its piece, the system on its page
    int32_t piece;
    int32_t x0;             // strip column of c0
};
// flags: one uint64 per chunk; n_lines: int32 per system; lines: max_lines int32 per system (page columns, ascending);
// piece_count, sys_first: n_pieces / n_systems int32 of workspace; header: total measures, first overflowing system or -1
hipError_t launch_score_map_counts(hipStream_t s, const double *maps, const ScoreSystem *table, int n_systems,
                                   int64_t total_chunks, double threshold, int min_rows, unsigned long long *flags);
hipError_t launch_score_map_lines(hipStream_t s, const ScoreSystem *table, int n_systems, const unsigned long long *flags,
                                  int tol, int max_lines, int32_t *n_lines, int32_t *lines);
hipError_t launch_score_map_table(hipStream_t s, const ScoreSystem *table, int n_systems, int n_pieces, int max_lines,
                                  const int32_t *n_lines, const int32_t *lines, int32_t *piece_count, int32_t *piece_first,
                                  int32_t *header, int32_t *sys_first, int32_t *measures);
// scanner borders of scanned pages (page_crop_kernels.hip; include/asr_hip.h carries the definition).  The estimate is two
// launches - the counts of dark pixels per row and per column (integer atomics on zeroed workspace), then the runs and the
// rect, one workgroup per page - and the copy is one.  One 256-thread workgroup per tile of CROP_TILE_H rows x CROP_TILE_W
// columns of a page (counts), or per CROP_COPY_ROWS rows of a rect (copy).
constexpr int CROP_THREADS = 256;
constexpr int CROP_TILE_W = 1024;                      // a wave reads 256 columns of a row, four per lane
constexpr int CROP_TILE_H = 64;
constexpr int CROP_COPY_ROWS = 8;
constexpr int CROP_MAX_DIM = 16384;
struct CropPage {
    int64_t off;            // byte offset of the page in the source buffer
    int64_t row_at, col_at; // the page's first entry in the row counts / in the column counts
    int32_t h, w;
    int32_t tiles_x;        // column tiles: ceil(w / CROP_TILE_W)
    int32_t margin;
};
struct CropCopy {
    int64_t src;            // byte offset of the rect's first byte in the source buffer
    int64_t dst;            // byte offset of the result in the output buffer
    int32_t stride;         // the page's width
    int32_t h, w;           // of the rect
    int32_t pad;
};
hipError_t launch_crop_counts(hipStream_t s, const uint8_t *pages, const int64_t *tile_first, const CropPage *table,
                              int n_pages, int64_t total_tiles, int floor_, int32_t *row_counts, int32_t *col_counts);
hipError_t launch_crop_rects(hipStream_t s, const CropPage *table, int n_pages, int share, const int32_t *row_counts,
                             const int32_t *col_counts, int32_t *rects, int32_t *status);
hipError_t launch_crop_copy(hipStream_t s, const uint8_t *pages, uint8_t *out, const int64_t *tile_first,
                            const CropCopy *table, int n_pages, int64_t total_tiles);
// batch assembly of the training pool: desc_dev holds n x 9 doubles (see piece_vote_kernels.hip)
hipError_t launch_gather_windows(hipStream_t s, const float *src, const double *desc_dev, int n, int out_h, int out_w,
                                 float *out);

// ---- CCA re-estimation (refine_cca.py / utils/cca.py 'svd') ------------------
size_t cca_workspace_bytes(int64_t n);
// H1,H2: [n][32] fp32 device; outputs device: U,V [32][32] fp32, means [64] fp32
// (m1 | m2), coeffs [32] fp64.
hipError_t launch_cca_fit(hipStream_t s, const float *H1, const float *H2, int64_t n, float r1, float r2,
                          void *workspace, float *U, float *V, float *means, double *coeffs);

// ---- data-parallel exchange points (null: single GPU) ------------------------------
// Training shards the batch over `world` ranks (shards may differ by one row: n_local of n_global samples live here);
// the per-channel BatchNorm sums (forward and
// backward) are all-reduced in place so that every rank normalises with the statistics of the FULL batch
// (SURVEY.md 8e).  allreduce sums `count` doubles in place on stream s (RCCL enqueues; a host callback synchronises).
struct Exchange {
    int (*allreduce_f64)(void *self, hipStream_t s, double *buf, int64_t count);
    void *self;
    int world;
    int n_local, n_global;      // this step's shard / whole batch, set by the training step before its first launch
    // 0: a launcher runs its local part, the all-reduce and the rest in one go.  The data-parallel step pairs the two
    // towers' exchanges - one all-reduce per block instead of two: 1 = local part only (the sums are left in `sums`),
    // 2 = only what follows the all-reduce (the caller has summed `sums` over the ranks in between)
    int phase;
};

// ---- training: forward with batch statistics --------------------------------
// model.prepare of raw sheets for the training step (prepare_view1.h): in (N, Hraw, Wraw) ASR_IN_U8_RAW / _F32_RAW ->
// out (N, H, W) float32 prepared; rsz: H, W = Hraw / 2, Wraw / 2 (2x2 blend), else H, W = Hraw, Wraw.
hipError_t launch_prepare_view1(hipStream_t s, const void *in, int in_mode, int rsz, int N, int Hraw, int Wraw, int H,
                                int W, float *out);
const char *prepare_view1_symbol(int in_mode, int rsz, int W);      // as rocprofv3 --kernel-trace prints it
// stats / stats_rows (may be null): partial table of the outputs' per-channel sums, [rows][2][cout] float64
// mode 0: z + statistics; 1: statistics only (z unused); 2: BatchNorm (bn = [mu | inv_std], gamma, beta) + ELU of the
// recomputed z written to `z` (block 1's output)
hipError_t launch_conv1_raw(hipStream_t s, const float *x, const float *w, float *z, int N, int H, int W, int cout,
                            double *stats, int *stats_rows, int mode = 0, const float *bn = nullptr,
                            const float *gamma = nullptr, const float *beta = nullptr);
// long float64 partial tables [nb][cols] are pre-summed 32 rows per workgroup into the space BEHIND the table (allocate
// colsum_stage_extra(doubles) more); returns the table the single-workgroup finish reads and updates *nb
size_t colsum_stage_extra(size_t partial_doubles);
double *colsum_stage(hipStream_t s, double *partial, int *nb, int cols);
int bn_stats_blocks(int64_t rows);
// z: rows x C; partial: bn_stats_blocks(rows)*2*C doubles; stats: [mu | inv_std]; run_*: EMA targets or null
// ex != null: `sums` (2*C doubles) carries the local column sums through the all-reduce; rows counts the local shard
hipError_t launch_bn_stats(hipStream_t s, const float *z, int64_t rows, int C, double *partial, float *stats,
                           float *run_mean, float *run_istd, float eps, float ema, const Exchange *ex = nullptr,
                           double *sums = nullptr, unsigned *ticket = nullptr);
// the same finish from a partial table the convolution wrote itself (nb rows of [2][C]); rows = count behind the sums
// ticket (single GPU: ex == null): one zero-initialised counter -> the reduction runs as ONE launch (colsum_final_kernel:
// 32-row groups, the last workgroup to arrive finishes); zero_rows: that launch also clears the rows it consumed (the
// convolutions' own statistics table stays all-zero between uses, so they need no memset before they write their rows;
// `staged` then has to lie OUTSIDE that table: ceil(nb / 32) rows of 2*C doubles; default: behind the nb rows)
hipError_t launch_bn_stats_final(hipStream_t s, double *partial, int nb, int64_t rows, int C, float *stats,
                                 float *run_mean, float *run_istd, float eps, float ema, const Exchange *ex = nullptr,
                                 double *sums = nullptr, unsigned *ticket = nullptr, bool zero_rows = false,
                                 double *staged = nullptr);
// zsel (pooled blocks, may be null): (N,OH,OW,C) raw value of each window's selected element, for launch_bn_bwd.
// ztie (with zsel, may be null): (N,OH,OW,C/4) bytes, two bits per channel = (number of window elements whose y equals the
// maximum) - 1: what the reduce pass of launch_bn_bwd multiplies by under the "every tied element" pooling gradient.
// snap (pooled blocks, may be null): 2*C floats that receive [gamma * inv_std | beta] as this pass used them.
hipError_t launch_bn_apply(hipStream_t s, const float *z, const float *stats, const float *gamma, const float *beta,
                           float *out, int N, int H, int W, int C, int pool, int elu, float *zsel = nullptr,
                           uint8_t *ztie = nullptr, float *snap = nullptr);
// debug export: (N,OH,OW,C) floats holding the 4-bit set {rr : y(window element rr) == max y} (bit rr = 2 dy + dx) - the
// elements a pooled block's backward pass feeds under ASR_POOL_TIES_ALL, bit for bit (same bn_affine on the same
// inputs: snap = what launch_bn_apply kept)
hipError_t launch_pool_mask(hipStream_t s, const float *z, const float *stats, const float *snap, float *mask, int N, int H,
                            int W, int C);
hipError_t launch_conv1x1_raw(hipStream_t s, const float *a8, const float *w9, float *z9, int64_t rows, int C8);
hipError_t launch_bn_gpool(hipStream_t s, const float *z9, const float *stats, const float *gamma, const float *beta,
                           float *Hout, int N, int npix);
// CCALayer train branch + length norm + ranking loss, forward and backward (single workgroup, float64)
size_t cca_train_ws_bytes(int B);
hipError_t launch_cca_train(hipStream_t s, const float *H1, const float *H2, int B, const float *cca_in,
                            float *cca_out, float r1, float r2, float rT, float alpha, float gamma, void *ws,
                            float *loss_out, float *lv1, float *lv2, float *dH1, float *dH2, float weight = 1.0f,
                            int symmetric = 0);

// get_contrastive_cos_loss(weight, gamma, symmetric) (models/objectives.py:30-69) of given embeddings, no gradients
hipError_t launch_rank_loss(hipStream_t s, const float *lv1, const float *lv2, int B, float gamma, float *loss_out,
                            float weight = 1.0f, int symmetric = 0);

// ---- training: backward + update ------------------------------------------------
int bn_bwd_blocks(int64_t opix);
// dz must not alias z for pooled blocks (dz = null: reduce pass and batch sums only).  partial: bn_bwd_blocks*2*C doubles;
// sums: 2*C doubles.  zsel (pooled blocks, may be null): what launch_bn_apply wrote - the reduce pass then reads it
// instead of the four window elements of z (the same values, the same sums).
// ties_first = 0 (ASR_POOL_TIES_ALL): every window element whose y equals the window maximum receives the pooled gradient
// (Theano's CPU MaxPoolGrad); with zsel the reduce pass needs ztie (launch_bn_apply) for the multiplicities.
// ties_first = 1: only the first such element in row-major order.
hipError_t launch_bn_bwd(hipStream_t s, const float *z, float *dz, const float *dout, const float *stats,
                         const float *gamma, const float *beta, double *partial, double *sums, float *dbeta,
                         float *dgamma, int N, int H, int W, int C, int pool, int elu, const Exchange *ex = nullptr,
                         const float *zsel = nullptr, const uint8_t *ztie = nullptr, int ties_first = 0,
                         unsigned *ticket = nullptr);
// One launch for "column sums of a partial table [nb][cols] (float64) + what follows": workgroup b sums rows 32b .. 32b+31
// into a staged row behind the table, the LAST workgroup to arrive (atomic ticket, reset to 0 for the next use) sums the
// staged rows in fixed order - deterministic for a given nb - and finishes.  mode 0: BatchNorm statistics (mu, inv_std,
// EMA of both); mode 1: sums[cols] only; mode 2: sums[cols] + dbeta / dgamma (BatchNorm backward).  Replaces
// colsum_stage_kernel + bn_stats_final_kernel / bn_bwd_final_kernel (two launches, and a memset before the producer).
struct ColsumFinalArgs {
    double *partial; int nb, cols; double *staged; unsigned *ticket; int zero_rows, mode, C;
    double count; float eps, ema; float *stats, *run_mean, *run_istd; double *sums; float *dbeta, *dgamma;
};
hipError_t launch_colsum_final(hipStream_t s, const ColsumFinalArgs &a);
struct WgradPlan {
    int cin, cout, H, W, TH, TW, tiles_y, tiles_x, lds_bytes, variant, grid_cap;
};
bool plan_wgrad(int cin, int cout, int H, int W, int num_cus, WgradPlan *p);
void wgrad_candidates(int cin, int cout, int H, int W, int num_cus, int max_count, std::vector<WgradPlan> *out);
size_t wgrad_partial_floats(const WgradPlan &p);
// tiles and workgroups of launch_wgrad for plan p on N images; whether p is a Winograd-domain form
void wgrad_launch_shape(const WgradPlan &p, int N, int *items, int *grid);
bool wgrad_is_wino(const WgradPlan &p);
hipError_t launch_wgrad(hipStream_t s, const WgradPlan &p, const float *x, const float *dz, int N, float *partial,
                        float *dW);
int conv1_wgrad_blocks();
// z != null: block 1's BatchNorm / ELU backward fused (launch_bn_bwd was called with dz = null: reduce pass only;
// `sums` are its batch sums); dz is then unused
hipError_t launch_conv1_wgrad(hipStream_t s, const float *x, const float *dz, int N, int H, int W, int cout,
                              double *partial, float *dW, const float *z = nullptr, const float *dout = nullptr,
                              const float *stats = nullptr, const float *gamma = nullptr, const float *beta = nullptr,
                              const double *sums = nullptr, int n_global = 0, const float *w1 = nullptr);
// block 1 without its raw tensor: reduce pass + batch sums of its BatchNorm backward with z recomputed from the image
// (w1: block 1's [C][9] taps); launch_conv1_wgrad(..., z = null, w1) applies dz the same way
hipError_t launch_bn_bwd_conv1(hipStream_t s, const float *x, const float *w1, const float *dout, const float *stats,
                               const float *gamma, const float *beta, double *partial, double *sums, float *dbeta,
                               float *dgamma, int N, int H, int W, int C, const Exchange *ex = nullptr);
int tail_dw_blocks(int64_t rows);
// partial: tail_dw_blocks(N * npix) * 32 * C8 + N * 64 doubles
hipError_t launch_tail_bwd(hipStream_t s, const float *dH, float *z9, const float *a8, const float *w9,
                           const float *stats, const float *gamma, int N, int npix, int C8, double *sums,
                           double *partial, float *dbeta, float *dgamma, float *dW9, float *da8,
                           const Exchange *ex = nullptr);
hipError_t launch_adam(hipStream_t s, float *p, const float *g, float *m, float *v, const unsigned char *mask,
                       int64_t n, float a_t, double beta1, double beta2, float eps, float l2);
hipError_t launch_l2_penalty(hipStream_t s, const float *p, const unsigned char *mask, int64_t n, double *out);
// one conv block's re-layout work for repack_all_kernel (train_bwd_kernels.hip); null pointers = not wanted
struct RepackDesc {
    const float *W, *beta, *gamma, *mean, *istd;      // master parameters of the block
    float *wfwd, *wdgrad;                             // direct-form fragments (kind 0: the [co][9] taps; kind 2: copy target)
    float *wino_fwd, *wino_dgrad;                     // Winograd-domain copies
    float *wino4_fwd, *wino4_dgrad;                   // F(4x4) Winograd-domain copies (where the step's plans use them)
    float *bnp;                                       // deterministic-path BN fold
    int cin, cout;                                    // kind 2: cin * cout = elements to copy
    int kind;                                         // 0: block 1 (C_in = 1), 1: 3x3 block, 2: plain copy
};
hipError_t launch_repack_all(hipStream_t s, const RepackDesc *descs_dev, int n_descs);
hipError_t launch_repack_conv(hipStream_t s, const float *W, int cin, int cout, float *wfwd, float *wdgrad);
hipError_t launch_repack_conv1(hipStream_t s, const float *W, int cout, float *w1);
hipError_t launch_bn_fold(hipStream_t s, const float *beta, const float *gamma, const float *mean, const float *istd,
                          int cout, float *bnp);

}  // namespace asr
