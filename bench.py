#!/usr/bin/env python
"""bench.py - snippet-pairs/sec embedded+ranked (32-d CCA) on N MI355X GPUs.  No PyTorch anywhere.

One "step" = the hot path of BASELINE.json configs[1] over one batch:
  1000 synthetic (sheet uint8 1x160x200, spectrogram f32 1x92x42) pairs per GPU,
  already resident in HBM  ->  both towers (mutopia_ccal_cont, deterministic)
  -> CCA projection -> L2 norm  ->  [N>1: all-gather of the candidate
  embeddings over the library's RCCL communicator]  ->  float64 all-pairs cosine
  ranking of this GPU's 1000 queries against all N*1000 candidates (integer ranks).
Weak scaling: per-GPU work is fixed; value = N*1000*K / max-over-ranks time.
Successive steps rotate through --batches (8) distinct resident batches.  The K timed steps are split into --repeats (5)
consecutive repeats (fewer when K is smaller), each timed on its own, and the MEDIAN repeat's time per step is reported
(min / max next to it).  Every repeat ends with a full synchronisation, so the drain of the queue is spread over K / 5
steps instead of K: on the MI355X, K = 20 split 5 ways and timed as one window gave the same ms_per_step within
run-to-run noise.  --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy.

A plain run does what the headline figure needs and nothing else: set-up, the W warm-up steps (whose last ones are
the surveyed ones), the K timed steps, --dump-outputs, the line.  Its "roofline" and "kernels" blocks come from those
same steps and from committed files; every leg that takes steps of its own is None / absent in its line.

--full adds the side legs, all after the timed steps and the dump, none of them part of the headline: N > 1 runs K more
steps with the exchange timed (comm_ms); N = 1 runs the host-buffer leg (--repeats windows of K batches each: its
double-buffered copies are timed over whole K-batch windows, so the pipeline's fill is not counted once per few steps),
the trained-weights recall leg (K + 1 steps), the CPU baseline leg (--cpu-pairs), and the fixed-size secondary and
reference-API legs.  --no-host-leg / --no-cpu-baseline / --no-secondary / --no-dropin / --no-isolated take single legs
out of a --full run.  The pool2m and train workloads are single measurements of their own and do not change with --full.

    python bench.py --gpus N --steps K --warmup W [--full]
        N > 1: this process (which never touches a GPU) starts one child per GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
        also works: RANK / LOCAL_RANK / WORLD_SIZE are read from the environment; torch itself is not imported

Control plane (communicator id, barriers, max-over-ranks): distributed.HubComm, plain TCP on 127.0.0.1.
Data plane: asr_comm_init (RCCL inside libasr_hip.so) + asr_rank_sharded_dev, enqueued on the library's stream; no
host synchronisation inside a step.

Prints ONE JSON line on rank 0 including "full" (whether --full was given) and
  "roofline":     dominant kernel, algorithmic FLOP / measured HIP-event time vs the dense fp32-MFMA peak
                  (157.3 TFLOP/s, MI355X_MICROARCH.md); HBM traffic and MFMA-pipe utilisation of that kernel from the
                  committed rocprofv3 PMC runs of this same command (profiles/, `traffic_source` names the file)
with --full only:
  "cpu_baseline": the CPU oracle (oracle/, a NumPy/C port of the reference path - NOT Theano, which cannot run here)
                  timed on a bounded sample on this host's cores (N=1 only)
  "value_host_buffers": the same step fed from page-locked HOST memory (H2D of the inputs and D2H of the ranks inside
                  the timed region, double-buffered against compute: asr_eval_batches), N=1 only.
  "value_dropin_api": pairs/s through the reference's OWN API on pageable host arrays - RetrievalWrapper.compute_view_1
                  (uint8 sheets) + compute_view_2 + eval_retrieval at n = 2000 (eval_models.sh:15); "dropin_api" holds the
                  breakdown and the float32-sheet figure; "refine_cca_s": wall time of refine_cca.py's work on 25 000
                  host pairs (tower outputs + CCA fit), N=1 only.
  "secondary":    BASELINE configs[2] (training step, batch 512), configs[3] (CCA fit, 25 000 samples), configs[4]'s
                  per-GPU shard (top-25 of 1024 queries x 250 k codes and of 64 queries x 2 M codes), each with its own
                  roofline block and the parity test that guards that size (tools/bench_secondary.py), N=1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PAIRS_PER_GPU = 1000
MODEL = os.environ.get("ASR_BENCH_MODEL", "mutopia_ccal_cont")     # the headline workload; _rsz for side measurements
FLOP_PER_PAIR = 552594048 if MODEL.endswith("_rsz") else 425302464   # BASELINE.md section 2 (conv MACs x 2, both towers)
PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md, dense fp32 matrix
PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md, dense bf16 matrix (the retrieval filter's split products)
PEAK_HBM_GBS = 8000.0
PROFILE_ROUND = "r06"              # profiles/<round>_hbm_traffic_by_symbol.json, <round>_mfma_busy_by_symbol.json, <round>_tune_cache.txt


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps in all (split over --repeats)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="the K timed steps are split into this many separately timed runs; median reported")
    ap.add_argument("--batches", type=int, default=8, help="distinct resident input batches the steps rotate through")
    ap.add_argument("--pairs", type=int, default=PAIRS_PER_GPU, help="pairs per GPU per step")
    ap.add_argument("--chunk", type=int, default=0, help="samples per internal launch (0 = library default)")
    ap.add_argument("--full", action="store_true",
                    help="pairs workload: after the timed steps also run the side legs - exchange timing (N > 1), "
                         "host-buffer leg, trained-weights recall, CPU baseline, secondary configs, reference-API legs. "
                         "Off by default: a plain run times the headline and prints its line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-host-leg", action="store_true", help="--full: skip the host-buffer (PCIe-inclusive) measurement")
    ap.add_argument("--no-isolated", action="store_true", help="--full: skip the informational single-stream pass")
    ap.add_argument("--profile-all", action="store_true",
                    help="bracket EVERY kernel with events inside the timed region too (tools/profile_round.sh: the "
                         "launch log then covers all timed launches)")
    ap.add_argument("--comm", choices=["rccl", "host"], default="rccl",
                    help="N>1 exchange: the library's RCCL communicator, or host callbacks over the TCP hub (several "
                         "ranks on ONE GPU - RCCL refuses that; tests only)")
    ap.add_argument("--cpu-pairs", type=int, default=2000, help="sample size of the CPU baseline leg")
    ap.add_argument("--workload", choices=["pairs", "pool2m", "train"], default="pairs",
                    help="pairs: configs[1], weak scaling (the default line). pool2m: configs[4] - a 2^21-code candidate "
                         "pool sharded over the GPUs, all-gather of the shards' embeddings, this GPU's share of 4096 "
                         "queries ranked + top-25 against all of it (strong scaling). train: configs[2] - one training "
                         "update at batch --train-batch (512) split over the GPUs (strong scaling)")
    ap.add_argument("--train-batch", type=int, default=512, help="train: rows of the whole batch")
    ap.add_argument("--pool", type=int, default=1 << 21, help="pool2m: candidate codes in the whole pool")
    ap.add_argument("--exchange", choices=["queries", "pool"], default="queries",
                    help="pool2m: what travels between the GPUs. queries (default): the QUERY embeddings are all-gathered "
                         "(0.5 MB), every GPU searches its own shard of the pool for all queries, the k-lists are "
                         "all-gathered and merged, the rank counters all-reduced. pool: the pool's embeddings are "
                         "all-gathered (256 MB) and every GPU searches all of it for its own queries")
    ap.add_argument("--queries", type=int, default=4096, help="pool2m: queries in the whole job")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the configs[2]/[3]/[4] measurements")
    ap.add_argument("--no-dropin", action="store_true", help="--full: skip the reference-API legs (RetrievalWrapper, refine_cca)")
    ap.add_argument("--refine-pairs", type=int, default=25000, help="host pairs of the refine_cca leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="pairs workload: write what the last timed step computed (embeddings of both views, ranks, d*, "
                         "ties) as DIR/<name>.npy, float32 / float64, at most 64 MB (a seeded sample of rows beyond)")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.workload != "pairs":
        ap.error("--dump-outputs: only the pairs workload (the headline step) writes its outputs")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays, rank=0, world=1):
    """Writes the outputs of one step as <path>/<name>.npy (float32 stays float32, everything else becomes float64:
    the integer ranks and tie counts are exact there).  All arrays share their first axis (one row per query / pair);
    when they would exceed DUMP_LIMIT_BYTES together, the same fixed, seeded sample of rows is taken from each and
    its indices are written as sample_rows.npy.  With several ranks every file name carries _rank<r>."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v, np.float32 if np.asarray(v).dtype == np.float32 else np.float64) for k, v in arrays.items()}
    n = len(next(iter(arrays.values())))
    row_bytes = sum(a.nbytes // max(1, len(a)) for a in arrays.values())
    keep = max(1, DUMP_LIMIT_BYTES // max(1, row_bytes + 8))
    if n > keep:
        rows = np.sort(np.random.default_rng(20240917).choice(n, size=keep, replace=False))
        arrays = dict({k: a[rows] for k, a in arrays.items()}, sample_rows=rows.astype(np.float64))
    sfx = "_rank%d" % rank if world > 1 else ""
    for k, a in arrays.items():
        np.save(os.path.join(path, k + sfx + ".npy"), a)
    return sorted(k + sfx for k in arrays)


def _repeat_sizes(steps, repeats):
    """--steps K is the number of timed steps in all: they are split into min(--repeats, K) consecutive repeats of
    K // R or K // R + 1 steps, each timed on its own"""
    steps = max(1, steps)
    r = min(max(1, repeats), steps)
    return [steps // r + (1 if i < steps % r else 0) for i in range(r)]


CPU_THREADS = 16      # the oracle's OpenMP/BLAS loops scale to ~16 threads on the EPYC host, then degrade


def _cpu_baseline_worker(n_pairs, seed):
    """Oracle (CPU port of the reference path) on a bounded sample: embed n_pairs in chunks of 100 like
    run_eval.py:107, float64 cdist + per-row argsort like utils/train_dcca_pool.py:28-82."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from oracle import network as onet, retrieval as oret
    sheet, spec = synth_data.synth_pairs(np.arange(n_pairs), seed=seed)
    params = synth_data.synth_params(onet.param_shapes(MODEL), seed=1, trained_like=True)
    warm = onet.prepare(sheet[:8], MODEL)
    onet.compute_output(warm, spec[:8], params)               # thread pools, page faults
    t0 = time.perf_counter()
    lv1, lv2 = [], []
    for s in range(0, n_pairs, 100):
        x = onet.prepare(sheet[s:s + 100], MODEL)
        a, b = onet.compute_output(x, spec[s:s + 100], params)
        lv1.append(a)
        lv2.append(b)
    lv1, lv2 = np.vstack(lv1), np.vstack(lv2)
    oret.eval_retrieval(lv1, lv2)
    return time.perf_counter() - t0


def cpu_baseline(n_pairs, seed):
    """Runs the oracle in a child process pinned to CPU_THREADS OpenMP/BLAS threads (thread counts are fixed at
    library load) and reports pairs/s of the bounded sample."""
    threads = max(1, min(CPU_THREADS, len(os.sched_getaffinity(0))))
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OPENBLAS_NUM_THREADS=str(threads),
               MKL_NUM_THREADS=str(threads))
    code = "import bench; print('CPU_BASELINE_S', bench._cpu_baseline_worker(%d, %d))" % (n_pairs, seed)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    dt = None
    for line in out.stdout.splitlines():
        if line.startswith("CPU_BASELINE_S"):
            dt = float(line.split()[1])
    if dt is None:
        raise RuntimeError("cpu baseline failed: " + out.stderr[-2000:])
    return dict(value=n_pairs / dt, unit="pairs/s", cores=threads, kind="port",
                note="oracle/ = NumPy + C restatement of the reference path; the Theano reference itself cannot run "
                     "here (Python 2, theano/lasagne absent)",
                sample="%d pairs embedded (chunks of 100) + %dx%d float64 cdist/argsort ranking, %.1f s of CPU work"
                       % (n_pairs, n_pairs, n_pairs, dt))


def spawn_ranks(argv, n):
    """`python bench.py --gpus N` from a plain shell: this process stays GPU-free (no HIP call, no library load) and
    starts one child per GPU (audio_sheet_retrieval_amd.launch.spawn_ranks); rank 0's JSON line goes straight to the
    inherited stdout.  The children are polled: when one exits non-zero the others are terminated (they would sit in
    the hub until its timeout) and this process prints a JSON line carrying "error" and returns that exit code within
    seconds."""
    from audio_sheet_retrieval_amd import launch

    def report(rank, code):
        print(json.dumps({"metric": "snippet-pairs/sec embedded+ranked (32-d CCA)", "value": None, "n_gpus": n,
                          "error": "rank %d exited with code %s; the other ranks were terminated" % (rank, code)}),
              flush=True)
    return launch.spawn_ranks([sys.executable, os.path.abspath(__file__)] + list(argv), n,
                              extra_env={"ASR_BENCH_SPAWNED": "1"}, on_failure=report)


def bench_params():
    """(parameters, description): ASR_BENCH_PARAMS=<pickle in the reference's 97-array format, e.g. written by
    tools/train_demo.py> runs the bench with trained weights (recall_at_1/5 then mean something); default: seeded
    HeUniform weights with trained-looking BatchNorm / CCA values - chance-level recall, same arithmetic."""
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes
    path = os.environ.get("ASR_BENCH_PARAMS")
    if path:
        from audio_sheet_retrieval_amd.retrieval_wrapper import load_params
        return load_params(path), "trained: " + os.path.basename(path)
    return synth_data.synth_params(param_shapes(MODEL), seed=1, trained_like=True), "random-init (HeUniform, seed 1)"


def _batch_indices(b, rank, world, n):
    """global pair indices of resident batch b on `rank`: batch 0 of a single GPU is pairs 0..n-1 (the set the parity
    test tests/test_gpu_bench_sizes.py checks against the oracle)"""
    first = (b * world + rank) * n
    return np.arange(first, first + n)


def _synth_batches(nb, rank, world, n):
    from concurrent.futures import ThreadPoolExecutor
    from audio_sheet_retrieval_amd.utils import synth_data
    with ThreadPoolExecutor(max_workers=min(nb, max(1, len(os.sched_getaffinity(0)) // max(1, world)))) as ex:
        return list(ex.map(lambda b: synth_data.synth_pairs(_batch_indices(b, rank, world, n), seed=23), range(nb)))


def _profile_table(kind):
    """committed rocprofv3 PMC summary of this same command (tools/profile_round.sh + tools/summarize_pmc.py):
    ({kernel symbol: {..., "layers": [...]}}, {layer label: {..., "symbol": ...}}, path) or (None, None, None)"""
    path = os.path.join(ROOT, "profiles", "%s_%s_by_symbol.json" % (PROFILE_ROUND, kind))
    if os.path.exists(path):
        with open(path) as fp:
            doc = json.load(fp)
        return doc["kernels"], doc.get("layers"), os.path.relpath(path, ROOT)
    return None, None, None


def _lookup_counters(by_symbol, by_layer, sym, live_layers, fields):
    """Counter figures of the committed profile FOR THE LAUNCHES THAT RAN HERE.  Which layers a kernel symbol serves is
    the tuner's choice (round 4's driver box had one conv4 build serve both towers, the committed profile only the
    spectrogram tower's: its by-symbol traffic described no launch of that run).  So:
      - the profile's record of `sym` is used only when it served exactly the layers it served here;
      - otherwise the figures are re-assembled per layer - the mean over the live layers, each taken from the profile's
        record of that LAYER, which must have run the same symbol there;
      - otherwise nothing is reported, with the reason.
    -> ({field: value}, how) or (None, reason)"""
    if by_symbol is None:
        return None, "no committed %s profile" % PROFILE_ROUND
    live = sorted(live_layers)
    rec = by_symbol.get(sym)
    if rec is not None and sorted(rec.get("layers", [])) == live:
        return {f: rec.get(f) for f in fields}, "by symbol (same layers as in the profile: %s)" % ", ".join(live)
    if by_layer:
        rows = [by_layer.get(lab) for lab in live]
        if all(r is not None and r.get("symbol") == sym for r in rows):
            out = {}
            for f in fields:
                vals = [r.get(f) for r in rows]
                out[f] = None if any(v is None for v in vals) or not all(isinstance(v, (int, float)) for v in vals) \
                    else sum(vals) / len(vals)
            return out, "mean over the live layers (%s), each from the profile's record of that layer under the same symbol" \
                % ", ".join(live)
    prof_layers = None if rec is None else rec.get("layers")
    return None, ("the committed profile does not describe this run: here %s served %s, in the profile %s"
                  % (sym, live, "it did not run" if rec is None else "it served %s" % prof_layers))


def _committed_tune_cache():
    """The schedules the committed profile was taken with (profiles/<round>_tune_cache.txt), copied to a scratch file
    (the tuner appends what it does not find): the default bench run executes exactly the kernels the profile
    describes.  ASR_BENCH_RETUNE=1 lets this box time the schedules itself."""
    src = os.path.join(ROOT, "profiles", "%s_tune_cache.txt" % PROFILE_ROUND)
    if os.environ.get("ASR_BENCH_RETUNE") == "1" or not os.path.exists(src):
        return None
    import shutil
    import tempfile
    dst = os.path.join(tempfile.mkdtemp(prefix="asr_bench_"), "tune_cache.txt")
    shutil.copy(src, dst)
    return dst


def _cache_lines(path):
    """the inference-schedule lines ("v2 ...") of a tune cache; the training tuner's own lines ("t1" / "t2": plans timed
    at asr_train_begin, per box, never part of the committed cache) are not what the roofline block's lookups depend on"""
    try:
        with open(path) as fp:
            return [ln for ln in fp.read().splitlines() if ln.strip() and not ln.startswith(("t1 ", "t2 "))]
    except OSError:
        return []


def _tune_source_after_run(pinned, pinned_lines, claimed):
    """a cache line carries tune_cache_tag() (a hash of the build); after any edit under csrc/ the tuner
    skips every committed line, times the schedules on this box and APPENDS its own picks to the scratch copy.  The
    line must then not claim the committed profile's schedules ran."""
    if not pinned:
        return claimed
    now = _cache_lines(pinned)
    appended = len(now) - len(pinned_lines)
    if appended > 0:
        return ("timed on this box: the tuner appended %d lines to the copy of profiles/%s_tune_cache.txt (its %d lines did "
                "not all match this build / these shapes)" % (appended, PROFILE_ROUND, len(pinned_lines)))
    return claimed


POOL_BLOCK = 8192


def _pool_block(blk, seed):
    x = np.random.default_rng([seed, blk]).standard_normal((POOL_BLOCK, 32), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def pool_codes(lo, hi, seed=23):
    """rows [lo, hi) of the synthetic candidate pool: unit float32 codes, generated in blocks of POOL_BLOCK rows from
    per-block seeds so that every rank (and every GPU count) sees the same row under the same global index"""
    parts = []
    for blk in range(lo // POOL_BLOCK, -(-hi // POOL_BLOCK)):
        a, b = max(lo, blk * POOL_BLOCK), min(hi, (blk + 1) * POOL_BLOCK)
        parts.append(_pool_block(blk, seed)[a - blk * POOL_BLOCK:b - blk * POOL_BLOCK])
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def pool_queries(lo, hi, n_queries, n_pool, seed=23):
    """queries [lo, hi): noisy copies of candidate (i * n_pool / n_queries) - the first of the n_pool / n_queries
    candidates eval_retrieval counts as query i's correct items (utils/train_dcca_pool.py:35-36, k_mult)"""
    k = n_pool // n_queries
    out = np.empty((hi - lo, 32), np.float32)
    blk, rows = -1, None
    for i in range(lo, hi):
        if (i * k) // POOL_BLOCK != blk:
            blk = (i * k) // POOL_BLOCK
            rows = _pool_block(blk, seed)
        noise = np.float32(0.03 + 0.3 * ((i * 2654435761) % 1000) / 1000.0)      # easy to hopeless: ranks 1 .. thousands
        q = rows[i * k - blk * POOL_BLOCK] + noise * np.random.default_rng([seed, 1 << 30, i]).standard_normal(32, dtype=np.float32)
        out[i - lo] = q / np.linalg.norm(q)
    return out


def run_pool2m(args):
    """BASELINE configs[4]: "2M-snippet candidate pool sharded, RCCL all-gather 32-d embeddings over xGMI, global top-k
    retrieval at 1/2/4/8 GPUs".  The pool's embeddings start out sharded by contiguous ranges (where the towers of each
    GPU left them); a step = all-gather of the shards (asr_comm_allgather_dev: the library's RCCL communicator, on the
    context's stream) -> top-25 of this GPU's queries against the WHOLE pool (asr_topk_dev; the path of
    audio_sheet_server.py:530-563) -> their eval_retrieval ranks (asr_rank_dev with query_offset; n2 = 512 n1).
    Strong scaling: the job's work is fixed (4096 queries x 2^21 codes), the queries are what is divided."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    from audio_sheet_retrieval_amd import _lib, distributed as D
    use_dist = world > 1 or os.environ.get("ASR_BENCH_FORCE_DIST", "0") == "1"
    same_gpu = os.environ.get("ASR_BENCH_SAME_GPU", "0") == "1"
    hub = D.HubComm(rank, world) if use_dist else None
    n_pool, n_q, k = args.pool, args.queries, 25
    if n_pool % world or n_q % world or n_pool % n_q:
        raise SystemExit("pool2m: --pool must be a multiple of --queries and both of the GPU count")
    shard, q_local = n_pool // world, n_q // world
    eng = _lib.Engine(MODEL, device=0 if same_gpu else local_rank)
    if use_dist:
        if world == 1:
            os.environ["ASR_COMM_FORCE"] = "1"
        D.init_data_parallel(eng, transport=args.comm, comm=hub)
    comm_rank, comm_world = eng.comm_info()
    codes = pool_codes(rank * shard, (rank + 1) * shard)
    queries = pool_queries(rank * q_local, (rank + 1) * q_local, n_q, n_pool)
    d_shard = eng.alloc(codes.nbytes).upload(codes)
    d_all = eng.alloc(n_pool * 128)
    d_q = eng.alloc(queries.nbytes).upload(queries)
    d_idx, d_dist = eng.alloc(q_local * k * 4), eng.alloc(q_local * k * 8)
    d_ranks, d_dstar, d_ties = eng.alloc(q_local * 4), eng.alloc(q_local * 8), eng.alloc(q_local * 4)

    # the gathered pool is a resident data base (asr_db_*): after each all-gather its norms / unit-length copy are
    # refreshed in one pass, then ONE walk over the pool gives the top-25 and the ranks (asr_topk_rank_db_dev).
    # ASR_POOL2M_SEPARATE=1: round 3's two stateless passes (top-k, then ranking), for A/B timing - same results.
    separate = os.environ.get("ASR_POOL2M_SEPARATE", "0") == "1"
    by_queries = args.exchange == "queries" and not separate
    pool_db = None if (separate or by_queries) else eng.db_create(d_all.ptr, n_pool)
    if by_queries:
        # Query-sharded exchange: the pool never moves.  Per step: all-gather of the queries (n_q x 128 B), d* / j* of
        # this rank's queries from its own shard (their correct candidates live there: blocks of n_pool / n_q rows) and
        # their all-gather, top-25 + rank counters of ALL queries against this shard (one fused pass), all-reduce of the
        # integer counters, all-gather of the k-lists, merge of this rank's queries.  ~2 MB on the wire instead of 256.
        shard_db = eng.db_create(d_shard.ptr, shard)
        d_qall = eng.alloc(n_q * 128)
        d_ds_loc, d_js_loc = eng.alloc(q_local * 8), eng.alloc(q_local * 8)
        d_ds_all, d_js_all = eng.alloc(n_q * 8), eng.alloc(n_q * 8)
        d_sidx, d_sdist = eng.alloc(n_q * k * 4), eng.alloc(n_q * k * 8)
        d_pidx, d_pdist = eng.alloc(world * n_q * k * 4), eng.alloc(world * n_q * k * 8)
        d_counts = eng.alloc(n_q * 12)

    def step_by_queries():
        shard_db.refresh()                       # the shard's embeddings are new every step (norms, unit-length copy)
        eng.comm_allgather_dev(d_q.ptr, d_qall.ptr, q_local * 128)
        shard_db.rank_dstar_dev(d_q.ptr, q_local, rank * shard, n_pool, rank * q_local, n_q, d_ds_loc.ptr, d_js_loc.ptr)
        eng.comm_allgather_dev(d_ds_loc.ptr, d_ds_all.ptr, q_local * 8)
        eng.comm_allgather_dev(d_js_loc.ptr, d_js_all.ptr, q_local * 8)
        shard_db.topk_count_dev(d_qall.ptr, n_q, k, rank * shard, d_sidx.ptr, d_sdist.ptr, d_ds_all.ptr, d_js_all.ptr,
                                d_counts.ptr)
        eng.comm_allreduce_dev(d_counts.ptr, n_q * 3, _lib.DTYPE_I32)
        eng.comm_allgather_dev(d_sidx.ptr, d_pidx.ptr, n_q * k * 4)
        eng.comm_allgather_dev(d_sdist.ptr, d_pdist.ptr, n_q * k * 8)
        eng.topk_merge_dev(d_pidx.ptr, d_pdist.ptr, world, n_q, rank * q_local, q_local, k, d_idx.ptr, d_dist.ptr)
        eng.rank_finish_dev(d_counts.offset(rank * q_local * 12), d_ds_all.offset(rank * q_local * 8), q_local, d_ranks.ptr,
                            d_dstar.ptr, d_ties.ptr)

    def step():
        if by_queries:
            return step_by_queries()
        eng.comm_allgather_dev(d_shard.ptr, d_all.ptr, shard * 128)
        if separate:
            eng.topk_dev(d_all.ptr, n_pool, d_q.ptr, q_local, k, d_idx.ptr, d_dist.ptr)
            eng.rank_dev(d_q.ptr, q_local, d_all.ptr, n_pool, d_ranks.ptr, d_dstar.ptr, d_ties.ptr,
                         query_offset=rank * q_local, n1_global=n_q)
        else:
            pool_db.refresh()
            pool_db.topk_rank_dev(d_q.ptr, q_local, k, d_idx.ptr, d_dist.ptr, d_ranks.ptr, d_dstar.ptr, d_ties.ptr,
                                  query_offset=rank * q_local, n1_global=n_q)

    def fence():
        eng.sync()
        if hub:
            hub.barrier()
    for _ in range(max(1, args.warmup)):
        step()
    fence()
    eng.profile_reset(); eng.profile_enable(True)
    step()
    fence()
    eng.profile_enable(False)
    survey = [p for p in eng.profile() if p["launches"] > 0]
    times = []                                  # per repeat: its time per step, scaled to --steps steps
    for k_rep in _repeat_sizes(args.steps, args.repeats):
        fence()
        t0 = time.perf_counter()
        for _ in range(k_rep):
            step()
        eng.sync()
        dt = time.perf_counter() - t0
        if hub:
            dt = hub.all_reduce_max(dt)
        times.append(dt / k_rep * args.steps)
    dt = float(np.median(times))
    idx = d_idx.download((q_local, k), np.int32)
    ranks = d_ranks.download((q_local,), np.int32)
    # order-independent integer fingerprints of the job's results: the same for every GPU count
    w = np.arange(1, k + 1, dtype=np.int64)
    qid = np.arange(rank * q_local, (rank + 1) * q_local, dtype=np.int64)[:, None] + 1
    sums = np.array([float(((idx.astype(np.int64) * w) % 1000003 * (qid % 997)).sum() % (1 << 52)),
                     float(ranks.astype(np.int64).sum()), float(np.count_nonzero(ranks <= 1)),
                     float(np.count_nonzero(idx[:, 0] // (n_pool // n_q) == qid[:, 0] - 1))])
    if use_dist:
        sums = eng.allreduce_host(sums)
    if rank == 0:
        dom = max(survey, key=lambda p: p["total_ms"]) if survey else None
        out = {"metric": "queries/sec: top-25 + eval_retrieval rank against a sharded %d-code pool" % n_pool,
               "value": n_q * args.steps / dt, "unit": "queries/s", "n_gpus": world, "steps": args.steps,
               "warmup": max(1, args.warmup) + 1, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": "f32 (filter products on two bf16 planes of the bf16 MFMA, |error| <= 4.9e-5, thresholds and exact band widened to it) + f64 exact distances", "data": "synthetic",
               "config": {"workload": "configs[4]: %d-code candidate pool sharded over %d GPU(s), all-gather of the 32-d "
                                      "embeddings, global top-%d + ranks of %d queries" % (n_pool, world, k, n_q),
                          "pool": n_pool, "queries": n_q, "k": k, "queries_per_gpu": q_local, "shard_codes": shard,
                          "exchange": "queries" if by_queries else "pool",
                          "allgather_bytes_per_gpu": (q_local * (128 + 16) + n_q * k * 12) if by_queries else shard * 128,
                          "allreduce_bytes": n_q * 12 if by_queries else 0,
                          "retrieval": "two passes (asr_topk_dev, asr_rank_dev)" if separate else
                                       "query-sharded: every GPU searches its own shard for all queries (asr_topk_count_db_dev), "
                                       "k-lists all-gathered and merged, rank counters all-reduced" if by_queries else
                                       "resident data base, one fused pass (asr_db_refresh + asr_topk_rank_db_dev)"},
               "repeats": {"n": len(times), "min_ms_per_step": min(times) / args.steps * 1e3,
                           "max_ms_per_step": max(times) / args.steps * 1e3},
               "pair_distances_per_s": 2.0 * n_q * n_pool * args.steps / dt,
               "comm": None if not use_dist else {"transport": args.comm, "rccl_ranks": comm_world, "rank": comm_rank,
                                                  "control_plane": "tcp hub (no torch)", "librccl": eng.comm_library()},
               "checksum": {"topk_idx": int(sums[0]) % (1 << 52), "rank_sum": int(sums[1]), "hits_at_1": int(sums[2]),
                            "top1_is_a_correct_item": int(sums[3])},
               "recall_at_1": sums[2] / n_q,
               "kernels": {p["name"]: round(p["total_ms"] / p["launches"], 4) for p in survey},
               "roofline": None if dom is None else {
                   "bound": "mfma", "kernel": dom["symbol"] or dom["name"],
                   "achieved": dom["flops"] / (dom["total_ms"] / dom["launches"] * 1e-3) / 1e12 if dom["flops"] else None,
                   "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                   "frac": dom["flops"] / (dom["total_ms"] / dom["launches"] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS
                   if dom["flops"] else None, "traffic": None, "avg_launch_ms": dom["total_ms"] / dom["launches"],
                   # the filter's products run on the bf16 MFMA on the two leading bf16 planes of the float32 values
                   # (round 5; three planes and six MFMAs before): three v_mfma_f32_16x16x32_bf16 per 16 x 16 x 32 tile
                   # product, i.e. 3 x the algorithmic FLOP executed; the kernel is bound by instruction issue (the
                   # per-tile threshold tests and appends), not by the matrix cores
                   "effective": True,
                   "note": "achieved / frac: algorithmic fp32 FLOP (2 x 32 per pair) against the fp32-MFMA peak; the "
                           "products execute as 3 bf16 MFMAs (two bf16 planes, error bound 4.9e-5, every candidate and "
                           "every pair inside the widened band is re-evaluated in float64: DESIGN.md section 4, "
                           "'Round 5: few queries')",
                   "executed_bf16_tflops": 3.0 * dom["flops"] / (dom["total_ms"] / dom["launches"] * 1e-3) / 1e12
                   if dom["flops"] else None,
                   "executed_frac_of_bf16_peak": 3.0 * dom["flops"] / (dom["total_ms"] / dom["launches"] * 1e-3) / 1e12 /
                   PEAK_BF16_MFMA_TFLOPS if dom["flops"] else None},
               "cpu_baseline": None, "torch_imported": "torch" in sys.modules}
        print(json.dumps(out), flush=True)
    if pool_db is not None:
        pool_db.close()
    if by_queries:
        shard_db.close()
    if hub:
        hub.barrier()
        hub.close()
    eng.close()


def run_train_dp(args):
    """BASELINE configs[2] over N GPUs: "full training step (pairwise ranking loss + CCA layer bwd), batch=512".  The
    batch is sharded by contiguous ranges (distributed.shard_range - sizes may differ by one row), every rank keeps its
    rows resident and a step = asr_train_step_dev on them: towers forward with the BatchNorm sums all-reduced, all-gather
    of the 32-d tower outputs, CCALayer + loss on the whole batch on every rank, backward with the BatchNorm-backward
    sums all-reduced, gradient all-reduce, Adam (utils/train_dcca_pool.py:203-205 on one device).  Strong scaling: the
    batch is fixed, value = updates/s.  `loss_first_update` is the loss of the very first update from the seeded
    parameters - the same number for every N up to float32 summation order (1e-5)."""
    import ctypes
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    from audio_sheet_retrieval_amd import _lib, distributed as D
    from audio_sheet_retrieval_amd.utils import synth_data
    use_dist = world > 1 or os.environ.get("ASR_BENCH_FORCE_DIST", "0") == "1"
    same_gpu = os.environ.get("ASR_BENCH_SAME_GPU", "0") == "1"
    hub = D.HubComm(rank, world) if use_dist else None
    B = args.train_batch
    if B < max(2, world):
        raise SystemExit("train: --train-batch %d cannot be split over %d GPUs" % (B, world))
    eng = _lib.Engine(MODEL, device=0 if same_gpu else local_rank)
    if use_dist:
        if world == 1:
            os.environ["ASR_COMM_FORCE"] = "1"
        D.init_data_parallel(eng, transport=args.comm, comm=hub)
    comm_rank, comm_world = eng.comm_info()
    weights, weights_note = bench_params()
    eng.set_params(weights)
    flag_barrier = D.hub_flag_barrier(hub) if hub else (lambda flag=0.0: flag)
    if hub:
        D.tune_in_rank_order(eng, flag_barrier, rank)
    lo, hi = D.shard_range(B, rank, world)
    sheet, spec = synth_data.synth_pairs(np.arange(lo, hi), seed=23)
    x1 = sheet.astype(np.float32) / np.float32(255)
    if MODEL.endswith("_rsz"):
        x1 = np.ascontiguousarray(0.25 * (x1[:, :, 0::2, 0::2] + x1[:, :, 0::2, 1::2] + x1[:, :, 1::2, 0::2] + x1[:, :, 1::2, 1::2]))
    cap = -(-B // world)
    if hub:           # rank 0 times the training schedules, the others read its picks from the job's tune cache
        D.tune_in_rank_order(eng, flag_barrier, rank, trigger=lambda: eng.train_begin(cap))
    else:
        eng.train_begin(cap)
    if use_dist:
        eng.train_set_global_batch(B)
    d1, d2 = eng.alloc(x1.nbytes).upload(x1), eng.alloc(spec.nbytes).upload(spec)
    loss = ctypes.c_float()
    corr = np.empty(32, np.float32)
    n_local = hi - lo

    def step():
        eng._check(eng.lib.asr_train_step_dev(eng.ctx, d1.ptr, d2.ptr, n_local, 0.002, ctypes.byref(loss), corr.ctypes.data))

    def fence():
        eng.sync()
        if hub:
            hub.barrier()
    step()
    loss_first = float(loss.value)
    for _ in range(max(0, args.warmup - 1)):
        step()
    fence()
    eng.comm_stats(reset=True)
    times = []                                  # per repeat: its time per step, scaled to --steps steps
    for k_rep in _repeat_sizes(args.steps, args.repeats):
        fence()
        t0 = time.perf_counter()
        for _ in range(k_rep):
            step()                                  # returns with the loss on the host: one synchronisation per update
        dt = time.perf_counter() - t0
        if hub:
            dt = hub.all_reduce_max(dt)
        times.append(dt / k_rep * args.steps)
    dt = float(np.median(times))
    cs = eng.comm_stats()
    n_steps = max(1, args.steps)
    # ---- what the collectives cost: the same steps once more with every collective bracketed by HIP events on the
    # stream it is enqueued on (asr_comm_timing).  In the data-parallel step both towers and all collectives share ONE
    # stream, so that time is exposed by construction; what the step loses beyond it (no tower overlap, no side stream
    # for the weight gradients) shows as the difference to the same update without a communicator - measurable in this
    # process only for one rank (ASR_BENCH_FORCE_DIST=1).
    comm_ms = comm_calls = exposed = plain_ms = None
    if use_dist:
        eng.comm_timing(True)
        fence()
        for _ in range(args.steps):
            step()
        cms, ccalls = eng.comm_timing(False)
        comm_ms, comm_calls = cms / args.steps, ccalls / args.steps
    eng.profile_reset(); eng.profile_enable(True)
    for _ in range(3):
        step()
    eng.sync(); eng.profile_enable(False)
    prof = sorted([p for p in eng.profile() if p["launches"] > 0], key=lambda p: -p["total_ms"])
    last_loss = float(loss.value)
    p90 = eng.debug_train_tensor("master", index=0)
    fingerprint = np.array([float(np.abs(p90.astype(np.float64)).sum())])       # parameters after the same number of updates
    if use_dist:
        both = eng.allgather_host(fingerprint)
        replicas_equal = bool(np.all(both == both[0]))
    else:
        replicas_equal = None
    if use_dist and world == 1:
        eng.train_end()
        plain = _lib.Engine(MODEL, device=0 if same_gpu else local_rank)
        plain.set_params(weights)
        plain.train_begin(cap)
        p1, p2 = plain.alloc(x1.nbytes).upload(x1), plain.alloc(spec.nbytes).upload(spec)

        def plain_step():
            plain._check(plain.lib.asr_train_step_dev(plain.ctx, p1.ptr, p2.ptr, n_local, 0.002, ctypes.byref(loss),
                                                      corr.ctypes.data))
        for _ in range(3):
            plain_step()
        plain.sync()
        ptimes = []                             # the same split of --steps as the timed region
        for k_rep in _repeat_sizes(args.steps, args.repeats):
            t0 = time.perf_counter()
            for _ in range(k_rep):
                plain_step()
            ptimes.append((time.perf_counter() - t0) / k_rep)
        plain_ms = float(np.median(ptimes)) * 1e3
        exposed = dt / args.steps * 1e3 - plain_ms
        plain.train_end()
        plain.close()
        eng.train_begin(cap)
    if rank == 0:
        fwd_flop = 552594048 if MODEL.endswith("_rsz") else 425302464
        tfl = 3.0 * B * fwd_flop / (dt / args.steps) / 1e12
        out = {"metric": "training updates/sec, batch %d (pairwise ranking loss + CCALayer bwd + Adam)" % B,
               "value": args.steps / dt, "unit": "updates/s", "n_gpus": world, "steps": args.steps,
               "warmup": max(1, args.warmup), "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "configs[2]: full training step (%s), batch %d over %d GPU(s)" % (MODEL, B, world),
                          "batch": B, "rows_per_gpu": [D.shard_range(B, r, world)[1] - D.shard_range(B, r, world)[0]
                                                       for r in range(world)], "lr": 0.002},
               "pairs_per_s": B * args.steps / dt,
               "repeats": {"n": len(times), "min_ms_per_step": min(times) / args.steps * 1e3,
                           "max_ms_per_step": max(times) / args.steps * 1e3},
               "loss_first_update": loss_first, "loss_last_update": last_loss, "replicas_equal": replicas_equal,
               "collectives_per_update": None if not use_dist else {
                   "allreduce_calls": cs["allreduce_calls"] / n_steps, "allreduce_bytes": cs["allreduce_bytes"] / n_steps,
                   "allgather_calls": cs["allgather_calls"] / n_steps,
                   "allgather_bytes_per_rank": cs["allgather_bytes_per_rank"] / n_steps},
               "comm": None if not use_dist else {"transport": args.comm, "rccl_ranks": comm_world, "rank": comm_rank,
                                                  "control_plane": "tcp hub (no torch)", "librccl": eng.comm_library()},
               # per update, rank 0: time inside the collectives (HIP events on their stream; host clock for callbacks),
               # their number, and - one rank only - what the data-parallel form of the step costs over the plain one
               "comm_ms": comm_ms, "comm_calls": comm_calls,
               "exposed_comm_ms": exposed if exposed is not None else comm_ms,
               "exposed_comm_note": None if not use_dist else (
                   "ms_per_step minus the same update on a context without a communicator (%.3f ms: two tower streams + a "
                   "weight-gradient side stream instead of one stream)" % plain_ms if exposed is not None else
                   "= comm_ms: towers and collectives share one stream in the data-parallel step, nothing overlaps them"),
               "weights": weights_note,
               "roofline": {"bound": "mfma", "achieved": tfl, "peak": PEAK_F32_MFMA_TFLOPS * world, "unit": "TFLOP/s",
                            "frac": tfl / (PEAK_F32_MFMA_TFLOPS * world), "traffic": None,
                            "work": "3 x forward conv FLOP (fwd + dgrad + wgrad, SURVEY 8d) x %d pairs per update; peak "
                                    "= %d x the dense fp32-MFMA peak" % (B, world)},
               "kernel_ms": {p["name"]: round(p["total_ms"] / 3, 3) for p in prof[:16]},
               "cpu_baseline": None, "torch_imported": "torch" in sys.modules}
        print(json.dumps(out), flush=True)
    eng.train_end()
    if hub:
        hub.barrier()
        hub.close()
    eng.close()


def run_rank(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world

    from audio_sheet_retrieval_amd import _lib, distributed as D
    from audio_sheet_retrieval_amd.utils import synth_data
    from audio_sheet_retrieval_amd.utils.param_layout import param_shapes

    # ASR_BENCH_FORCE_DIST=1 with one rank exercises the communicator hand-off on a single GPU
    use_dist = world > 1 or os.environ.get("ASR_BENCH_FORCE_DIST", "0") == "1"
    same_gpu = os.environ.get("ASR_BENCH_SAME_GPU", "0") == "1"      # all ranks on device 0 (needs --comm host)
    hub = D.HubComm(rank, world) if use_dist else None

    n, nb = args.pairs, max(1, args.batches)
    if hub:
        D.share_tune_cache(hub)                     # one cache file per job: rank 0 times, the others read
    tune_source = "ASR_TUNE_CACHE from the environment"
    pinned = pinned_lines = None
    if "ASR_TUNE_CACHE" not in os.environ:          # the isolated pass below re-uses the tuner's choices
        import tempfile
        pinned = _committed_tune_cache() if (world == 1 and MODEL == "mutopia_ccal_cont") else None
        os.environ["ASR_TUNE_CACHE"] = pinned or os.path.join(tempfile.mkdtemp(prefix="asr_bench_"), "tune_rank%d.txt" % rank)
        tune_source = ("profiles/%s_tune_cache.txt (the schedules the committed profile ran; ASR_BENCH_RETUNE=1 times them "
                       "on this box)" % PROFILE_ROUND) if pinned else "timed on this box"
        pinned_lines = _cache_lines(pinned) if pinned else None
    eng = _lib.Engine(MODEL, device=0 if same_gpu else local_rank, max_chunk=args.chunk)
    if use_dist:
        if world == 1:
            os.environ["ASR_COMM_FORCE"] = "1"
        D.init_data_parallel(eng, transport=args.comm, comm=hub)
    comm_rank, comm_world = eng.comm_info()
    weights, weights_note = bench_params()
    eng.set_params(weights)
    if hub:
        D.tune_in_rank_order(eng, D.hub_flag_barrier(hub), rank)

    # ---- synthetic shard of this rank, nb distinct batches resident in HBM before the timed region
    host = _synth_batches(nb, rank, world, n)
    d_sheet = [eng.alloc(s.nbytes).upload(s) for s, _ in host]
    d_spec = [eng.alloc(z.nbytes).upload(z) for _, z in host]
    d_lv1 = eng.alloc(n * 32 * 4)
    d_lv2 = eng.alloc(n * 32 * 4)
    d_all = eng.alloc(world * n * 32 * 4) if use_dist else None
    d_ranks = eng.alloc(n * 4)
    d_dstar = eng.alloc(n * 8)
    d_ties = eng.alloc(n * 4)

    def step(i):
        b = i % nb
        eng.embed_view1_dev(d_sheet[b].ptr, _lib.IN_U8_RAW, n, d_lv1.ptr)
        eng.embed_view2_dev(d_spec[b].ptr, n, d_lv2.ptr)
        if use_dist:      # all-gather of the candidates + ranking of this rank's queries, all on the library's stream
            eng.rank_sharded_dev(d_lv1.ptr, d_lv2.ptr, n, d_all.ptr, d_ranks.ptr, d_dstar.ptr, d_ties.ptr)
        else:
            eng.rank_dev(d_lv1.ptr, n, d_lv2.ptr, n, d_ranks.ptr, d_dstar.ptr, d_ties.ptr)

    def fence():
        eng.sync()
        if hub:
            hub.barrier()

    # Untimed warm-up; its last steps (at least one) run with every kernel bracketed by HIP events: they give the
    # per-kernel table and identify the dominant kernel symbol.  In the TIMED region only that kernel's launches carry
    # events (the contract's live roofline measurement) - two events per kernel on all ~20 launches of a step cost
    # 1.5 % of the step, which is instrumentation, not the product path.
    it = 0
    # exactly --warmup untimed steps: the last three of them (all of them when fewer are asked for, at least one) are
    # the surveyed ones; the first embed call also times the kernel schedules (the autotuner) - once per context
    warmup_ran = max(1, args.warmup)                          # what the JSON line reports as "warmup"
    survey_steps = min(3, max(1, warmup_ran - 1))             # (the very first step - first touch, tuner - stays plain)
    plain_warmup = warmup_ran - survey_steps
    for _ in range(plain_warmup):
        step(it)
        it += 1
    fence()
    eng.profile_reset()
    eng.profile_filter(None)
    eng.profile_enable(True)
    for _ in range(survey_steps):
        step(it)
        it += 1
    fence()
    eng.profile_enable(False)
    survey = [p for p in eng.profile() if p["launches"] > 0]
    by_sym_ms = {}
    for p in survey:
        if p["symbol"]:
            by_sym_ms[p["symbol"]] = by_sym_ms.get(p["symbol"], 0.0) + p["total_ms"]
    dom_symbol = max(by_sym_ms.items(), key=lambda kv: kv[1])[0] if by_sym_ms else None
    eng.profile_reset()
    eng.profile_filter(None if args.profile_all else dom_symbol)
    eng.profile_enable(True)
    times = []                                    # per repeat: its time per step, scaled to --steps steps
    for k_rep in _repeat_sizes(args.steps, args.repeats):
        fence()
        t0 = time.perf_counter()
        for _ in range(k_rep):
            step(it)
            it += 1
        eng.sync()
        dt = time.perf_counter() - t0
        if hub:
            dt = hub.all_reduce_max(dt)          # the slowest rank defines the step
        times.append(dt / k_rep * args.steps)
    eng.profile_enable(False)
    fence()
    eng.profile_filter(None)
    dt = float(np.median(times))
    it_last_timed = it - 1                      # index of the last timed step (its batch: it_last_timed % --batches)
    dumped = None
    if args.dump_outputs:           # before anything else runs on these buffers: the results of the last timed step
        dumped = dump_outputs(args.dump_outputs, dict(
            lv1=d_lv1.download((n, 32), np.float32), lv2=d_lv2.download((n, 32), np.float32),
            ranks=d_ranks.download((n,), np.int32), dstar=d_dstar.download((n,), np.float64),
            ties=d_ties.download((n,), np.int32)), rank, world)
    comm_ms = comm_calls = None
    if use_dist and args.full:                     # the all-gather of the candidate embeddings, per step (asr_comm_timing)
        eng.comm_timing(True)
        fence()
        for _ in range(args.steps):
            step(it)
            it += 1
        cms, ccalls = eng.comm_timing(False)
        comm_ms, comm_calls = cms / args.steps, ccalls / args.steps

    last_b = (it - 1) % nb
    ranks = d_ranks.download((n,), np.int32)
    ties = d_ties.download((n,), np.int32)
    hits = np.array([np.count_nonzero(ranks <= k) for k in (1, 5)], dtype=np.float64)
    if use_dist:
        hits = eng.allreduce_host(hits)          # over the communicator (RCCL / host callbacks)
    prof = eng.profile()

    # ---- host-buffer leg (--full, N=1): the same step fed from page-locked host memory, copies inside the timed region
    host_leg = None
    if args.full and world == 1 and not use_dist and not args.no_host_leg:
        pin = []
        for s, z in host:
            ps, pz = eng.host_array(s.shape, s.dtype), eng.host_array(z.shape, z.dtype)
            ps[...] = s
            pz[...] = z
            pin.append((ps, pz))
        k_steps = args.steps
        outs = dict(ranks=[eng.host_array((n,), np.int32) for _ in range(k_steps)],
                    dstar=[eng.host_array((n,), np.float64) for _ in range(k_steps)],
                    ties=[eng.host_array((n,), np.int32) for _ in range(k_steps)])
        xs = [pin[i % nb][0] for i in range(k_steps)]
        zs = [pin[i % nb][1] for i in range(k_steps)]
        eng.eval_batches(xs[:2], zs[:2], out={k: v[:2] for k, v in outs.items()})        # buffers, first touch
        htimes = []
        for _ in range(max(1, args.repeats)):
            eng.sync()
            t0 = time.perf_counter()
            eng.eval_batches(xs, zs, out=outs)         # returns with every rank list in host memory
            htimes.append(time.perf_counter() - t0)
        hdt = float(np.median(htimes))
        same = bool(np.array_equal(outs["ranks"][last_b], ranks)) if last_b < k_steps else None
        in_bytes = host[0][0].nbytes + host[0][1].nbytes
        host_leg = dict(value=n * k_steps / hdt, unit="pairs/s", ms_per_step=hdt / k_steps * 1e3,
                        min_ms_per_step=min(htimes) / k_steps * 1e3, max_ms_per_step=max(htimes) / k_steps * 1e3,
                        h2d_bytes_per_step=in_bytes, d2h_bytes_per_step=n * 16,
                        h2d_gbs=in_bytes / (hdt / k_steps) / 1e9,
                        ranks_equal_device_leg=same,
                        note="asr_eval_batches: pinned host inputs, H2D of batch k+1 and D2H of batch k-1 on copy "
                             "streams while batch k computes")

    # ---- only with --full and ASR_TWO_STREAMS=1 (towers overlapping on two streams, which stretches every kernel's own duration):
    # the same kernels WITHOUT the other tower sharing the GPU, a few untimed steps, reported next to the timed figures.
    iso = None
    if args.full and rank == 0 and world == 1 and not use_dist and not args.no_isolated and \
            os.environ.get("ASR_TWO_STREAMS") == "1":
        os.environ["ASR_TWO_STREAMS"] = "0"
        eng2 = _lib.Engine(MODEL, device=local_rank, max_chunk=args.chunk)
        os.environ["ASR_TWO_STREAMS"] = "1"
        eng2.set_params(weights)
        e_lv1, e_lv2 = eng2.alloc(n * 128), eng2.alloc(n * 128)
        e_sheet = eng2.alloc(host[0][0].nbytes).upload(host[0][0])
        e_spec = eng2.alloc(host[0][1].nbytes).upload(host[0][1])
        for j in range(6):
            if j == 1:
                eng2.sync(); eng2.profile_reset(); eng2.profile_enable(True)
            eng2.embed_view1_dev(e_sheet.ptr, _lib.IN_U8_RAW, n, e_lv1.ptr)
            eng2.embed_view2_dev(e_spec.ptr, n, e_lv2.ptr)
        eng2.sync(); eng2.profile_enable(False)
        iso = {}
        for p in eng2.profile():
            if p["launches"] > 0:
                a = iso.setdefault(p["symbol"] or p["name"], dict(ms=0.0, launches=0, flops=0.0))
                a["ms"] += p["total_ms"]; a["launches"] += p["launches"]; a["flops"] += p["flops"] * p["launches"]
        eng2.close()

    if rank == 0:
        total_pairs = world * n * args.steps
        value = total_pairs / dt
        recs = [p for p in prof if p["launches"] > 0] or survey       # timed region: the dominant kernel's launches
        if args.profile_all:
            recs = [p for p in recs if p["symbol"] == dom_symbol] or recs
        # aggregate per kernel SYMBOL, exactly like `rocprofv3 --kernel-trace --stats` does: one template
        # instantiation serves the same block of both towers (e.g. conv2 of view 1 and of view 2)
        by_sym = {}
        for p in recs:
            a = by_sym.setdefault(p["symbol"] or p["name"], dict(ms=0.0, launches=0, flops=0.0, bytes=0.0, labels=[]))
            a["ms"] += p["total_ms"]
            a["launches"] += p["launches"]
            a["flops"] += p["flops"] * p["launches"]
            a["bytes"] += p["bytes"] * p["launches"]
            a["labels"].append(p["name"])
        dom_sym, dom = max(by_sym.items(), key=lambda kv: kv[1]["ms"])
        # which symbol is "dominant" can be a 2 % coin-flip between the conv2 and conv4 builds (the tuner's picks
        # aggregate per symbol): the two largest symbols of the surveyed steps, each with its own fraction
        sv = {}
        for p in survey:
            if p["symbol"]:
                a = sv.setdefault(p["symbol"], dict(ms=0.0, launches=0, flops=0.0))
                a["ms"] += p["total_ms"]; a["launches"] += p["launches"]; a["flops"] += p["flops"] * p["launches"]
        top_two = []
        for sym, a in sorted(sv.items(), key=lambda kv: -kv[1]["ms"])[:2]:
            tf = a["flops"] / max(a["ms"] * 1e-3, 1e-12) / 1e12
            top_two.append({"kernel": sym, "avg_launch_ms": a["ms"] / a["launches"], "achieved": tf,
                            "frac": tf / PEAK_F32_MFMA_TFLOPS, "time_share": a["ms"] / max(1e-12, sum(q["total_ms"] for q in survey))})
        avg_s = dom["ms"] / dom["launches"] * 1e-3
        achieved = dom["flops"] / dom["launches"] / avg_s / 1e12
        # per-kernel table, conv aggregate and time shares: the surveyed warm-up steps (all kernels bracketed)
        conv_ms = sum(p["total_ms"] for p in survey if p["name"].startswith("conv") or p["name"].startswith("tail"))
        conv_fl = sum(p["flops"] * p["launches"] for p in survey
                      if p["name"].startswith("conv") or p["name"].startswith("tail"))
        survey_dom_ms = sum(p["total_ms"] for p in survey if p["symbol"] == dom_sym)
        # PMC counters cannot be read from inside this process: traffic / MFMA-busy are the committed rocprofv3
        # measurements of this same command (tools/pmc_traffic.sh, tools/pmc_wino.sh), per launch of the dominant symbol
        standard = n == PAIRS_PER_GPU and (eng.cfg.max_chunk or 1000) == 1000
        ttab, tlay, tsrc = _profile_table("hbm_traffic") if standard else (None, None, None)
        mtab, mlay, msrc = _profile_table("mfma_busy") if standard else (None, None, None)
        live_layers = sorted(set(dom["labels"]))
        trec, thow = _lookup_counters(ttab, tlay, dom_sym, live_layers, ("hbm_bytes_per_launch", "hbm_read_bytes_per_launch",
                                                                        "hbm_write_bytes_per_launch"))
        mrec, mhow = _lookup_counters(mtab, mlay, dom_sym, live_layers, ("mfma_busy",))
        traffic = trec.get("hbm_bytes_per_launch") if trec else None
        alg_bytes = dom["bytes"] / dom["launches"]
        traffic_ratio = None if traffic is None or alg_bytes <= 0 else traffic / alg_bytes
        traffic_note = thow
        if traffic_ratio is not None and not (0.8 <= traffic_ratio <= 2.0):
            # a counter figure far from the algorithmic bytes of the launches it is quoted for is a mis-attribution or a
            # kernel that re-reads: either way not a number to print without looking at it
            traffic_note = ("withheld: %.3g B per launch from %s is %.2f x the algorithmic %.3g B of the live launches "
                            "(accepted: 0.8-2.0)" % (traffic, tsrc, traffic_ratio, alg_bytes))
            traffic = None
        wino = "wino" in dom_sym
        roof = {"bound": "mfma", "kernel": dom_sym, "layers": dom["labels"], "achieved": achieved,
                "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_F32_MFMA_TFLOPS,
                # Winograd F(2x2,3x3) executes 2.25x fewer multiply-adds than the direct form whose FLOP `achieved`
                # counts (SURVEY 8d's per-unit figure): `frac` is an EFFECTIVE rate, not MFMA-pipe utilisation
                "effective": bool(wino), "direct_to_executed_mac_ratio": 2.25 if wino else 1.0,
                "executed_frac": achieved / (2.25 if wino else 1.0) / PEAK_F32_MFMA_TFLOPS,
                "mfma_busy": mrec.get("mfma_busy") if mrec else None,
                "traffic": traffic,
                "traffic_over_algorithmic": traffic_ratio if traffic is not None else None,
                "traffic_source": ("committed rocprofv3 --pmc run of this command: %s, %s; not measured in this process"
                                   % (tsrc, traffic_note)) if traffic is not None else traffic_note,
                "mfma_busy_source": ("%s, %s" % (msrc, mhow)) if mrec else mhow,
                "schedules": _tune_source_after_run(pinned, pinned_lines, tune_source),
                "algorithmic_bytes_per_launch": alg_bytes,
                "hbm_gbs": None if traffic is None else traffic / avg_s / 1e9,
                "hbm_frac": None if traffic is None else traffic / avg_s / 1e9 / PEAK_HBM_GBS,
                "avg_launch_ms": avg_s * 1e3, "launches": dom["launches"],
                "all_conv_tflops": conv_fl / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else None,
                "flop_per_launch": dom["flops"] / dom["launches"],
                "whole_step_tflops": n * FLOP_PER_PAIR / (dt / args.steps) / 1e12,
                "gpu_time_share": survey_dom_ms / max(1e-12, sum(p["total_ms"] for p in survey)),
                "largest_two_symbols": top_two,
                "timed_with": "HIP events around every launch of this kernel inside the timed region (%d launches); "
                              "the other kernels were timed in the %d warm-up steps before it" % (dom["launches"],
                                                                                               survey_steps)}
        out = {
            "metric": "snippet-pairs/sec embedded+ranked (32-d CCA)",
            "value": value, "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": warmup_ran,
            "full": bool(args.full),              # False: the legs below that take steps of their own did not run
            "warmup_requested": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[1]: twin-CNN fwd (%s) + 32-d CCA embed + all-pairs cosine ranking, "
                                   "%d pairs per GPU, %d candidates" % (MODEL, n, world * n),
                       # which figure is which: `value` follows the bench contract (inputs resident in HBM when the timed
                       # region starts); BASELINE.md section 3 counts input H2D and result D2H on the GPU side - that is
                       # `value_host_buffers` (page-locked host batches in, rank lists out, copies inside the timed region)
                       "contract_figure": "value_host_buffers is the BASELINE.md section-3 figure (input H2D and result D2H "
                                          "inside the timed region); value is the device-resident figure the bench "
                                          "contract asks for (inputs in HBM at the start of the timed region)",
                       "pairs_per_gpu": n, "candidates": world * n, "chunk": eng.cfg.max_chunk or 1000,
                       "resident_batches": nb,
                       "partitioning": "pairs sharded by rank; RCCL all-gather of candidate embeddings (%d x 32 f32 "
                                       "per GPU), each GPU ranks its %d queries against all %d candidates - the "
                                       "all-gather + per-shard ranking pattern of configs[4] at configs[1]'s batch"
                                       % (n, n, world * n) if world > 1 else "single GPU"},
            "repeats": {"n": len(times), "median_ms_per_step": dt / args.steps * 1e3,
                        "min_ms_per_step": min(times) / args.steps * 1e3,
                        "max_ms_per_step": max(times) / args.steps * 1e3},
            "torch_imported": "torch" in sys.modules,
            "comm": None if not use_dist else {"transport": args.comm, "rccl_ranks": comm_world, "rank": comm_rank,
                                               "control_plane": "tcp hub (no torch)",
                                               "librccl": eng.comm_library()},
            "comm_ms": comm_ms, "comm_calls": comm_calls,
            "exposed_comm_ms": comm_ms,           # embed + all-gather + rank run on one stream: nothing overlaps the exchange
            "weights": weights_note,
            "recall_at_1": float(hits[0]) / (world * n), "recall_at_5": float(hits[1]) / (world * n),
            "recall_chance_level": [1.0 / (world * n), 5.0 / (world * n)],
            "rank_ties": int(ties.sum()),
            "value_host_buffers": None if host_leg is None else host_leg["value"],
            "host_buffers": host_leg,
            "roofline": roof,
            "roofline_isolated": None if not iso or dom_sym not in iso else {
                "note": "same kernel symbol, single stream (no tower overlap), 5 untimed steps after the timed region",
                "achieved": iso[dom_sym]["flops"] / (iso[dom_sym]["ms"] * 1e-3) / 1e12,
                "frac": iso[dom_sym]["flops"] / (iso[dom_sym]["ms"] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                "avg_launch_ms": iso[dom_sym]["ms"] / iso[dom_sym]["launches"], "launches": iso[dom_sym]["launches"]},
            "kernels": {p["name"]: round(p["total_ms"] / p["launches"], 4) for p in survey},
            "dumped_outputs": None if dumped is None else {"dir": args.dump_outputs, "arrays": dumped,
                                                           "step": it_last_timed},
        }
        # ---- --full: Recall@k that means something: the timed region runs random-init weights (the contract's workload:
        # chance-level recall by construction); the same batch 0 - pairs the model never saw - embedded and ranked once
        # more, untimed, with the committed weights of a 600-update training run on the synthetic pool
        # (tests/golden/trained_cont_params.npz, written by tools/train_demo.py: batch 100, Adam, lr 0.002, then
        # refine_cca on 5000 pairs)
        trained = os.path.join(ROOT, "tests", "golden", "trained_cont_params.npz")
        if args.full and world == 1 and not use_dist and MODEL == "mutopia_ccal_cont" and os.path.exists(trained) and \
                not os.environ.get("ASR_BENCH_PARAMS"):
            try:
                with np.load(trained) as z:
                    tp = [z["p%02d" % i] for i in range(97)]
                    train_first = int(z["train_first_index"]) if "train_first_index" in z.files else None
                # the committed weights must come from a run that never saw the pairs timed here (tools/train_demo.py
                # trains on indices from 2^24 upwards and records that in the file)
                if train_first is None or train_first < nb * world * n:
                    raise RuntimeError("trained_cont_params.npz does not record a training index range beyond the bench's "
                                       "pairs (train_first_index = %r)" % (train_first,))
                eng.set_params(tp)

                def trained_step():
                    eng.embed_view1_dev(d_sheet[0].ptr, _lib.IN_U8_RAW, n, d_lv1.ptr)
                    eng.embed_view2_dev(d_spec[0].ptr, n, d_lv2.ptr)
                    eng.rank_dev(d_lv1.ptr, n, d_lv2.ptr, n, d_ranks.ptr, d_dstar.ptr, d_ties.ptr)
                trained_step()
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    trained_step()
                eng.sync()
                trained_dt = (time.perf_counter() - t0) / args.steps
                tr = d_ranks.download((n,), np.int32)
                out["recall_trained_weights"] = {
                    "recall_at_1": float(np.count_nonzero(tr <= 1)) / n, "recall_at_5": float(np.count_nonzero(tr <= 5)) / n,
                    "recall_at_25": float(np.count_nonzero(tr <= 25)) / n, "map": float(np.mean(1.0 / tr.astype(np.float64))),
                    "median_rank": float(np.median(tr)), "candidates": n,
                    "value": n / trained_dt, "unit": "pairs/s", "ms_per_step": trained_dt * 1e3, "steps": args.steps,
                    "train_first_index": train_first,
                    "weights": "tests/golden/trained_cont_params.npz (600 updates on the synthetic pool + refine_cca, "
                               "tools/train_demo.py); pairs 0..%d are held out" % (n - 1),
                    "chance": [1.0 / n, 5.0 / n]}
                eng.set_params(weights)
            except Exception as e:
                out["recall_trained_weights"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cpu_pairs, seed=23)
        else:
            out["cpu_baseline"] = None
        # ---- --full, N = 1: the other BASELINE configs and the reference's own API, after the timed region
        if args.full and ((world == 1 and not use_dist) or os.environ.get("ASR_BENCH_SECONDARY") == "1"):
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_secondary as BS

            def leg(fn, *a, **kw):
                t0 = time.perf_counter()
                try:
                    r = fn(*a, **kw)
                except Exception as e:          # a failing side leg must not take the headline line with it
                    r = {"error": "%s: %s" % (type(e).__name__, e)}
                r["leg_wall_s"] = round(time.perf_counter() - t0, 2)
                return r
            if not args.no_secondary:
                out["secondary"] = {
                    "configs[2]_train_step_b512": leg(BS.measure_train, eng),
                    "configs[3]_cca_fit_25000": leg(BS.measure_cca, eng),
                    "configs[4]_topk_1024x250k": leg(BS.measure_topk, eng, 250000, 1024),
                    "configs[4]_topk_64x2m": leg(BS.measure_topk, eng, 2000000, 64),
                    # the reference's own call: ONE query frame against the whole data base (audio_sheet_server.py:530-563)
                    "configs[4]_topk_1x2m": leg(BS.measure_topk, eng, 2000000, 1),
                    "rank_2000": leg(BS.measure_rank, eng, 2000),
                    # the variant the reference ships weights for and evaluates (eval_models.sh:5)
                    "rsz_headline_and_train": leg(BS.measure_model_headline, "mutopia_ccal_cont_rsz", n, args.steps),
                }
            if not args.no_dropin:
                two = [np.concatenate([host[b % nb][k] for b in range(-(-2000 // n))]) for k in (0, 1)]
                d = leg(BS.measure_dropin, 2000, args.repeats, two[0], two[1])
                out["dropin_api"] = d
                out["value_dropin_api"] = d.get("value_dropin_api")
                if out["value_host_buffers"] and d.get("value_dropin_api"):
                    d["host_buffers_over_dropin"] = out["value_host_buffers"] / d["value_dropin_api"]
                r = leg(BS.measure_refine, args.refine_pairs, n, host[0][0], host[0][1])
                out["refine_cca"] = r
                out["refine_cca_s"] = r.get("refine_cca_s")
        print(json.dumps(out), flush=True)
    if hub:
        hub.barrier()
        hub.close()
    eng.close()


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or os.environ.get("ASR_BENCH_FORCE_DIST", "0") == "1"):
        raise SystemExit(spawn_ranks(sys.argv[1:], max(1, args.gpus)))
    try:
        {"pool2m": run_pool2m, "train": run_train_dp}.get(args.workload, run_rank)(args)
    except BaseException as e:
        if isinstance(e, SystemExit) and not e.code:
            raise
        # under a launcher (torch.distributed.run) nobody else reports: rank 0 says why there is no measurement
        if int(os.environ.get("RANK", "0")) == 0 and os.environ.get("ASR_BENCH_SPAWNED") != "1":
            print(json.dumps({"metric": "snippet-pairs/sec embedded+ranked (32-d CCA)", "value": None,
                              "n_gpus": int(os.environ.get("WORLD_SIZE", "1")),
                              "error": "%s: %s" % (type(e).__name__, e)}), flush=True)
        raise


if __name__ == "__main__":
    main()
