#!/usr/bin/env python
"""Piece identification over whole test pieces (the paper's second experiment), audio -> sheet ("A2S").  Command line
of the reference's audio_sheet_server.py (:571-580):

    python -m audio_sheet_retrieval_amd.audio_sheet_server --model models/mutopia_ccal_cont.py --data synthetic:16 \
        --train_split splits/all_split.yaml --config exp_configs/mutopia_full_aug.yaml \
        --init_sheet_db --full_eval --dump_results [--n_candidates 25] [--estimate_UV]

--init_sheet_db embeds the sheet windows of every test piece (EmbeddingDB.from_pool: initialize_sheet_db, :309-354) and
saves them to sheet_db_file.pkl in the working directory; without it that file is loaded.  --full_eval queries the
data base with every piece's spectrogram: 100 windows per piece, n_candidates neighbours per window, the votes ranked
per piece (detect_score, :213-251) with top_k = number of test pieces, and the target piece ranked by the reference's
rule (:640-645).  --dump_results writes the ranks to retrieval_<tag>_A2S.yaml next to the parameters, the file
scripts/eval_piece_retrieval.py reads.

Here the windows of all pieces are cut on the device, embedded in one call per tower, and all pieces are voted on in one
asr_piece_vote_batch_dev call (piece_identification.detect_scores).

--track (A2S only) runs the reference's default mode, the running vote of AudioSheetServer.run (:83-211), over every
test piece's spectrogram instead of its microphone: every frame with music is embedded and looked up, and the vote over
the last --running_frames such frames ranks the pieces (piece_identification.track_scores, top_k = 7).  Per piece it
prints the first frame at which the target leads and the share of voiced frames at which it leads; --dump_results
writes the two lists to tracking_<tag>_A2S.yaml.

--locate (A2S only) answers the question between piece identification and whole-piece alignment: given an excerpt,
where in which score are we?  Per test piece a seeded excerpt of --excerpt_frames frames is cut from its spectrogram;
the vote names --locate_pieces candidates and a subsequence DTW (free start and end on the score axis) aligns the
excerpt's windows, one every --step_spec frames, with each candidate's ordered data-base codes
(piece_identification.locate_scores: one asr_dtw_subseq_batch_dev call for all excerpts and candidates).  Per piece it
prints the rank of the own piece by vote and by alignment cost and the pixel distance of the found start and end from
the onset map interpolated at the excerpt's first and last window centres; --dump_results writes them to
location_<tag>_A2S.yaml.  The error is a report, not a gate.

--follow (A2S only) is score following, --locate while the recording still streams: per test piece the candidates are
the top --locate_pieces of the vote on its first performance (detect_scores); the performance is then pushed through a
piece_identification.ScoreFollower in blocks of --block_frames frames, windows --step_spec frames apart (one
asr_dtw_follow_batch_dev call per block for all candidates; the session keeps one accumulated row per candidate, so a
block costs its own windows only and the recording may be of any length).  Per piece it prints whether the own piece is
a candidate, the share of windows at which it has the least cost, and the median absolute pixel distance of its found
position from the onset map interpolated at each window's centre; --dump_results writes them to
following_<tag>_A2S.yaml.  A report, not a gate.

--follow --bank is the same report for live streams, which have no finished recording to vote on: every test piece is
one of as many parallel streams (piece_identification.live_follow_scores), pushed in blocks of --block_frames frames
through a PieceTrackerBank, whose leaders of the round's last voiced frame (at most --locate_pieces) become the
stream's candidates, and through a ScoreFollowerBank - a fixed number of library calls per round whatever the number
of pieces.  A candidate that enters late is followed from --catch_up windows back (default 64).  best_share and
median_error are taken over the windows at which the own piece occupies a slot, and occupied_share is their share.

The microphone and the GUI of the live server, audio decoding (--real_audio) and MSMD loading are not part of this
implementation.  sheet_audio_server.py is the S2A direction (sheet -> audio) of the same driver.
"""
import argparse
import os

import numpy as np
import yaml

from . import audio2sheet_align
from .piece_identification import (EmbeddingDB, RunningLevel, ScoreFollower, detect_performances, detect_scores,
                                   live_follow_scores, locate_scores, rank_summary, track_scores)
from .utils.data_pools import NO_AUGMENT, AudioScoreRetrievalPool

# per direction: data-base flag, data-base file, data-base view, what a query finds (the reference's summary line)
DIRECTIONS = {
    "A2S": dict(init_flag="--init_sheet_db", db_file="sheet_db_file.pkl", db_view=1, found="scores"),
    "S2A": dict(init_flag="--init_audio_db", db_file="audio_db_file.pkl", db_view=2, found="performances"),
}


def common_arguments(p, init_flag, db_file, result_name):
    """the flags the MSMD drivers and the UMC drivers (umc_a2s_server.py) share"""
    p.add_argument("--model", help="model definition, e.g. models/mutopia_ccal_cont.py",
                   default="models/mutopia_ccal_cont.py")
    p.add_argument("--estimate_UV", action="store_true", help="use the parameters written by refine_cca")
    p.add_argument(init_flag, dest="init_db", action="store_true",
                   help="build the data base from the test pieces and save it to %s" % db_file)
    p.add_argument("--full_eval", action="store_true", help="rank every test piece")
    p.add_argument("--n_candidates", type=int, default=25, help="neighbours retrieved per query window")
    p.add_argument("--train_split", type=str, default=None)
    p.add_argument("--config", type=str, default=None)
    p.add_argument("--dump_results", action="store_true", help="write the ranks to %s" % result_name)
    return p


def _arguments(argv, direction):
    d = DIRECTIONS[direction]
    p = argparse.ArgumentParser(description="Identify every test piece: %s." %
                                ("audio -> sheet music" if direction == "A2S" else "sheet music -> audio"))
    common_arguments(p, d["init_flag"], d["db_file"], "retrieval_<tag>_%s.yaml" % direction)
    p.add_argument("--data", type=str, default="synthetic", help="test pieces ('synthetic[:n_pieces]')")
    if direction == "A2S":
        p.add_argument("--real_audio", action="store_true", help="(audio decoding is not part of this implementation)")
    p.add_argument("--running_frames", type=int, default=100,
                   help="voiced frames in the history of the running vote (--track)")
    if direction == "A2S":
        p.add_argument("--track", action="store_true",
                       help="run the live server's running vote over every test piece's spectrogram")
        p.add_argument("--locate", action="store_true",
                       help="locate a seeded excerpt of every test piece in the scores of the data base")
        p.add_argument("--excerpt_frames", type=int, default=400, help="frames of the excerpt (--locate)")
        p.add_argument("--locate_pieces", type=int, default=5,
                       help="candidates of the vote that are aligned (--locate, --follow)")
        p.add_argument("--step_spec", type=int, default=2, help="frames between the query windows (--locate, --follow)")
        p.add_argument("--follow", action="store_true",
                       help="follow every test piece's first performance through the scores of the vote's candidates")
        p.add_argument("--block_frames", type=int, default=20, help="frames pushed per block (--follow)")
        p.add_argument("--bank", action="store_true",
                       help="--follow for live streams: all test pieces in parallel, candidates from the running vote")
        p.add_argument("--catch_up", type=int, default=64,
                       help="windows of history a candidate that enters late is followed from (--follow --bank)")
        level_arguments(p, "--track, --follow --bank")
    p.add_argument("--seed", type=int, default=23)
    args = p.parse_args(argv)
    if getattr(args, "bank", False) and not args.follow:
        p.error("--bank goes with --follow")
    if direction == "A2S":
        check_level_arguments(p, args, args.track or (args.follow and args.bank),
                              "--level running goes with --track or with --follow --bank")
    if direction == "A2S" and not 0 <= args.catch_up <= 512:
        p.error("--catch_up must lie in 0..512")
    return args


def level_arguments(p, where):
    """the music gate's level: of the finished recording (the reference's rule), or of what has been heard so far"""
    p.add_argument("--level", choices=("recording", "running"), default="recording",
                   help="level of the music gate (%s): the maximum column sum of the finished recording, or `running`: "
                        "of the columns heard so far (piece_identification.RunningLevel) - what a microphone can know"
                        % where)
    p.add_argument("--level_memory", type=int, default=None,
                   help="--level running: the maximum over the last N columns only (at least the window width)")
    p.add_argument("--level_floor", type=float, default=None,
                   help="--level running: a level below which the gate's divisor does not fall")


def check_level_arguments(p, args, allowed, message):
    if args.level != "running" and (args.level_memory is not None or args.level_floor is not None):
        p.error("--level_memory and --level_floor go with --level running")
    if args.level == "running":
        if not allowed:
            p.error(message)
        try:
            level_rule(args)
        except ValueError as err:
            p.error(str(err))


def level_rule(args):
    """None for --level recording, the RunningLevel of --level running"""
    if getattr(args, "level", "recording") != "running":
        return None
    return RunningLevel(args.level_memory, args.level_floor)


def result_file(param_file, direction):
    """the reference's dump name (:651-653): a tag-less params.pkl gives params_<direction>.yaml"""
    return param_file.replace("params_", "retrieval_").replace(".pkl", "_%s.yaml") % direction


def identify(engine, db, direction, pool, names, n_candidates):
    """every piece of `pool` as a query against `db` (A2S: its spectrogram, S2A: its unrolled sheet), top_k = number of
    pieces -> (ranks int32, ratios float64, per-piece (names, votes))"""
    ids = {name: i for i, name in db.id_to_name.items()}
    targets = np.array([ids.get(n, -1) for n in names], np.int32)     # a piece missing from the data base: rank n_out
    if direction == "A2S":
        queries = [spec[0] for spec in pool.specs]
        res, ranks, ratios = detect_scores(engine, db, queries, top_k=len(names), n_candidates=n_candidates,
                                           spec_shape=tuple(pool.spec_dim), targets=targets)
    else:
        res, ranks, ratios = detect_performances(engine, db, pool.images, top_k=len(names), n_candidates=n_candidates,
                                                 sheet_shape=tuple(pool.sheet_dim), targets=targets)
    return ranks, ratios, res


TRACK_TOP_K = 7


def tracking_file(param_file, direction):
    """result_file's name with tracking_ in place of retrieval_"""
    return param_file.replace("params_", "tracking_").replace(".pkl", "_%s.yaml") % direction


def track(engine, db, pool, names, n_candidates, running_frames, level=None):
    """the running vote over every piece's spectrogram -> (names, per piece the first frame at which its own piece
    leads the ranking (-1: never), per piece the share of its voiced frames at which it leads (0.0 without voiced
    frames)).  level: track_scores' (None, or a RunningLevel)"""
    ids = {name: i for i, name in db.id_to_name.items()}
    results = track_scores(engine, db, [spec[0] for spec in pool.specs], top_k=TRACK_TOP_K, n_candidates=n_candidates,
                           running_frames=running_frames, spec_shape=tuple(pool.spec_dim),
                           **({} if level is None else {"level": level}))
    first_lead, lead_share = [], []
    for name, res in zip(names, results):
        leads = (res.n_out > 0) & (res.pieces[:, 0] == ids.get(name, -2)) if len(res.frames) else np.zeros(0, bool)
        first_lead.append(int(res.frames[np.argmax(leads)]) if leads.any() else -1)
        lead_share.append(float(leads.mean()) if leads.size else 0.0)
    return names, first_lead, lead_share


def report_tracking(names, first_lead, lead_share, res_file=None, level=None):
    """level: the RunningLevel the gate used, named in the report and in the file; None: the recording's own"""
    if level is not None:
        print("music gate at the level of what has been heard so far: %r" % (level,))
    for name, first, share in zip(names, first_lead, lead_share):
        print("leads from frame %5d, at %.2f of the voiced frames  %s" % (first, share, name))
    results = {"first_lead": [int(f) for f in first_lead], "lead_share": [float(v) for v in lead_share]}
    if level is not None:
        results["level"] = repr(level)
    if res_file is not None:
        with open(res_file, "w") as fp:
            yaml.dump(results, fp, default_flow_style=False)
        print("tracking of %d pieces written to %s" % (len(names), res_file))
    return results


def location_file(param_file, direction):
    """result_file's name with location_ in place of retrieval_"""
    return param_file.replace("params_", "location_").replace(".pkl", "_%s.yaml") % direction


def pool_sheet_columns(pool, n_rows):
    """the strip x-coordinate of every row of an EmbeddingDB.from_pool data base: the annotated coordinate of the row's
    (piece, performance, onset) entity, on which its sheet window is centred; None when `pool` does not describe a data
    base of n_rows rows (then locate_scores applies EmbeddingDB.from_images' rule)"""
    if int(pool.shape[0]) != n_rows:
        return None
    return np.array([pool.o2c_maps[p][f][o][1] for p, f, o in pool.train_entities], np.float64)


def cut_excerpts(specs, o2c_maps, excerpt_frames, step_spec, win_w, seed):
    """per piece a seeded excerpt of (at most) excerpt_frames frames of its first performance -> (excerpts, per piece
    the onset map's x at the centres of the excerpt's first and last window)"""
    rng = np.random.RandomState(seed)
    excerpts, truth = [], []
    for spec, o2c in zip(specs, o2c_maps):
        spec, o2c = spec[0], np.asarray(o2c[0], np.float64)
        n = min(int(excerpt_frames), spec.shape[1])
        f0 = int(rng.randint(0, spec.shape[1] - n + 1))
        excerpts.append(np.ascontiguousarray(spec[:, f0:f0 + n]))
        last = np.arange(0, n - win_w + 1, step_spec)[-1] if n >= win_w else 0
        centres = np.array([f0 + win_w // 2, f0 + last + win_w // 2], np.float64)
        truth.append(tuple(float(v) for v in np.interp(centres, o2c[:, 0], o2c[:, 1])))
    return excerpts, truth


def locate(engine, db, pool, names, n_candidates, excerpt_frames, n_pieces, step_spec, seed):
    """an excerpt of every piece located in the data base -> one dict per piece: name, vote_rank / cost_rank of the own
    piece among the candidates (0: not among them), start_x / end_x found for it, start_error / end_error in pixels
    against the onset map (None when the own piece is no candidate)"""
    excerpts, truth = cut_excerpts(pool.specs, pool.o2c_maps, excerpt_frames, step_spec, int(pool.spec_dim[1]), seed)
    found = locate_scores(engine, db, excerpts, n_pieces=n_pieces, step_spec=step_spec, n_candidates=n_candidates,
                          spec_shape=tuple(pool.spec_dim), sheet_columns=pool_sheet_columns(pool, len(db)))
    out = []
    for name, cands, (x0, x1) in zip(names, found, truth):
        entry = dict(name=str(name), vote_rank=0, cost_rank=0, start_x=None, end_x=None, start_error=None, end_error=None)
        for rank, cand in enumerate(cands):
            if cand["name"] == name:
                entry.update(vote_rank=int(cand["vote_rank"]), cost_rank=rank + 1, start_x=float(cand["start_x"]),
                             end_x=float(cand["end_x"]), start_error=float(abs(cand["start_x"] - x0)),
                             end_error=float(abs(cand["end_x"] - x1)))
                break
        out.append(entry)
    return out


def report_location(entries, res_file=None):
    for e in entries:
        if e["cost_rank"]:
            print("rank by vote %02d, by cost %02d, start off by %6.1f px, end off by %6.1f px  %s"
                  % (e["vote_rank"], e["cost_rank"], e["start_error"], e["end_error"], e["name"]))
        else:
            print("rank by vote --, by cost --, not among the candidates                      %s" % e["name"])
    hit = [e for e in entries if e["cost_rank"]]
    if hit:
        print("own piece first by vote: %d, by cost: %d of %d; median start / end error %.1f / %.1f px"
              % (sum(e["vote_rank"] == 1 for e in hit), sum(e["cost_rank"] == 1 for e in hit), len(entries),
                 float(np.median([e["start_error"] for e in hit])), float(np.median([e["end_error"] for e in hit]))))
    if res_file is not None:
        with open(res_file, "w") as fp:
            yaml.dump(entries, fp, default_flow_style=False)
        print("location of %d pieces written to %s" % (len(entries), res_file))
    return entries


def following_file(param_file, direction):
    """result_file's name with following_ in place of retrieval_"""
    return param_file.replace("params_", "following_").replace(".pkl", "_%s.yaml") % direction


def follow(engine, db, pool, names, n_candidates, n_pieces, step_spec, block_frames):
    """every piece's first performance streamed through a ScoreFollower against the vote's top n_pieces -> one dict per
    piece: name, candidate (is the own piece one?), windows, best_share (share of the windows at which the own piece has
    the least cost), median_error (median |x - truth| in pixels, truth = the onset map at each window's centre frame;
    None when the own piece is no candidate or no window was completed)"""
    if block_frames < 1:
        raise ValueError("block_frames must be >= 1")
    specs = [spec[0] for spec in pool.specs]
    win_w = int(pool.spec_dim[1])
    votes = detect_scores(engine, db, specs, top_k=n_pieces, n_candidates=n_candidates, spec_shape=tuple(pool.spec_dim))
    out = []
    for name, spec, o2c, (cands, _) in zip(names, specs, pool.o2c_maps, votes):
        session = ScoreFollower(engine, db, cands, step_spec=step_spec, spec_shape=tuple(pool.spec_dim),
                                sheet_columns=pool_sheet_columns(pool, len(db)))
        try:
            res = [session.push(spec[:, f:f + block_frames]) for f in range(0, spec.shape[1], block_frames)]
        finally:
            session.close()
        frames = np.concatenate([r.frames for r in res])
        entry = dict(name=str(name), candidate=name in cands, windows=int(len(frames)), best_share=0.0, median_error=None)
        if entry["candidate"] and len(frames):
            own = list(cands).index(name)
            o2c = np.asarray(o2c[0], np.float64)
            truth = np.interp(frames + win_w // 2, o2c[:, 0], o2c[:, 1])
            entry.update(best_share=float(np.mean(np.concatenate([r.best for r in res]) == own)),
                         median_error=float(np.median(np.abs(np.concatenate([r.x[:, own] for r in res]) - truth))))
        out.append(entry)
    return out


def follow_bank(engine, db, pool, names, n_candidates, n_pieces, step_spec, block_frames, running_frames, catch_up,
                level=None):
    """every piece's first performance as one of len(names) parallel live streams (live_follow_scores): blocks of
    block_frames frames go to the running vote, whose leaders (at most n_pieces) become the stream's candidates, and to
    a ScoreFollowerBank -> follow's dict per piece, with best_share and median_error over the windows at which the own
    piece occupies a slot, candidate = there is such a window, and occupied_share = their share of all windows.
    level: a RunningLevel for the vote's gate; None: every finished spectrogram's own maximum"""
    if block_frames < 1:
        raise ValueError("block_frames must be >= 1")
    specs = [np.ascontiguousarray(spec[0], dtype=np.float32) for spec in pool.specs]
    win_w = int(pool.spec_dim[1])
    levels = level if level is not None else [spec.sum(axis=0).max() if spec.shape[1] else 0.0 for spec in specs]
    ids = {name: i for i, name in db.id_to_name.items()}
    _, followed = live_follow_scores(engine, db, specs, levels, block_frames=block_frames, n_slots=n_pieces,
                                     top_k=n_pieces, n_candidates=n_candidates, running_frames=running_frames,
                                     step_spec=step_spec, catch_up=catch_up, spec_shape=tuple(pool.spec_dim),
                                     sheet_columns=pool_sheet_columns(pool, len(db)))
    out = []
    for name, o2c, res in zip(names, pool.o2c_maps, followed):
        own = res.piece == ids.get(name, -2)                 # (windows, slots): at most one slot per window
        at = np.flatnonzero(own.any(axis=1))
        entry = dict(name=str(name), candidate=bool(len(at)), windows=int(len(res.frames)), best_share=0.0,
                     median_error=None, occupied_share=float(len(at)) / len(res.frames) if len(res.frames) else 0.0)
        if len(at):
            slot = np.argmax(own[at], axis=1)
            o2c = np.asarray(o2c[0], np.float64)
            truth = np.interp(res.frames[at] + win_w // 2, o2c[:, 0], o2c[:, 1])
            entry.update(best_share=float(np.mean(res.best[at] == slot)),
                         median_error=float(np.median(np.abs(res.x[at, slot] - truth))))
        out.append(entry)
    return out


def report_following(entries, res_file=None, level=None):
    """level: the RunningLevel the vote's gate used, named in the report and in every entry of the file"""
    if level is not None:
        print("music gate at the level of what has been heard so far: %r" % (level,))
        for e in entries:
            e["level"] = repr(level)
    for e in entries:
        if e["median_error"] is not None:
            print("own piece a candidate, least cost at %.2f of %5d windows, median off by %6.1f px  %s"
                  % (e["best_share"], e["windows"], e["median_error"], e["name"]))
        else:
            print("own piece %s, %5d windows                                            %s"
                  % ("a candidate" if e["candidate"] else "not among the candidates", e["windows"], e["name"]))
    hit = [e for e in entries if e["median_error"] is not None]
    if hit:
        print("own piece a candidate: %d of %d; median share of windows with the least cost %.2f, median error %.1f px"
              % (len(hit), len(entries), float(np.median([e["best_share"] for e in hit])),
                 float(np.median([e["median_error"] for e in hit]))))
    if res_file is not None:
        with open(res_file, "w") as fp:
            yaml.dump(entries, fp, default_flow_style=False)
        print("following of %d pieces written to %s" % (len(entries), res_file))
    return entries


def run(argv, direction):
    d = DIRECTIONS[direction]
    args = _arguments(argv, direction)
    if getattr(args, "real_audio", False):
        raise SystemExit("--real_audio: audio decoding is not part of this implementation")
    data = audio2sheet_align.select_pieces(args.data, args.seed)
    engine, param_file = audio2sheet_align.load_network(args.model, args.estimate_UV, args.train_split, args.config)
    pool = AudioScoreRetrievalPool(engine, data["images"], data["specs"], data["o2c_maps"],
                                   data_augmentation=dict(NO_AUGMENT), shuffle=False)
    if args.init_db:
        db = EmbeddingDB.from_pool(engine, pool, d["db_view"], names=data["names"])
        print("%d %s codes of %d pieces collected" % (len(db), "sheet snippet" if d["db_view"] == 1 else "audio excerpt",
                                                      len(data["names"])))
        db.save(d["db_file"])
    else:
        db = EmbeddingDB.load(engine, d["db_file"])
    if getattr(args, "track", False):
        print("\nTracking every test piece:")
        return report_tracking(*track(engine, db, pool, data["names"], args.n_candidates, args.running_frames,
                                      level_rule(args)),
                               res_file=tracking_file(param_file, direction) if args.dump_results else None,
                               level=level_rule(args))
    if getattr(args, "locate", False):
        print("\nLocating an excerpt of every test piece:")
        return report_location(locate(engine, db, pool, data["names"], args.n_candidates, args.excerpt_frames,
                                      args.locate_pieces, args.step_spec, args.seed),
                               res_file=location_file(param_file, direction) if args.dump_results else None)
    if getattr(args, "follow", False):
        print("\nFollowing every test piece through the scores:")
        if args.bank:
            return report_following(follow_bank(engine, db, pool, data["names"], args.n_candidates, args.locate_pieces,
                                                args.step_spec, args.block_frames, args.running_frames, args.catch_up,
                                                level_rule(args)),
                                    res_file=following_file(param_file, direction) if args.dump_results else None,
                                    level=level_rule(args))
        return report_following(follow(engine, db, pool, data["names"], args.n_candidates, args.locate_pieces,
                                       args.step_spec, args.block_frames),
                                res_file=following_file(param_file, direction) if args.dump_results else None)
    if not args.full_eval:
        raise SystemExit("the live server loop (microphone, GUI) is not part of this implementation; use --full_eval")

    print("\nRunning full evaluation:")
    ranks, ratios, _ = identify(engine, db, direction, pool, data["names"], args.n_candidates)
    return report_ranks(data["names"], ranks, ratios, d["found"],
                        result_file(param_file, direction) if args.dump_results else None)


def report_ranks(names, ranks, ratios, found, res_file=None):
    """the per-piece rank lines, the "n of m retrieved ... ranked at position r." lines and the summary of a full
    evaluation; with res_file the ranks are dumped there as yaml (:647-657) -> the ranks as a list of int"""
    ranks = np.asarray(ranks)
    for name, rank, ratio in zip(names, ranks, ratios):
        print("rank: %02d (%.2f) %s" % (rank, ratio, name))
    n_queries = len(ranks)
    for r in range(1, n_queries + 1):
        n_correct = int(np.sum(ranks == r))
        if n_correct > 0:
            print("%d of %d retrieved %s ranked at position %d." % (n_correct, n_queries, found, r))
    for key, (cnt, frac) in rank_summary(ranks).items():
        print("rank %-4s %d (%.2f)" % (key, cnt, frac))
    results = [int(r) for r in ranks]
    if res_file is not None:
        with open(res_file, "w") as fp:
            yaml.dump(results, fp, default_flow_style=False)
        print("ranks of %d pieces written to %s" % (n_queries, res_file))
    return results


def main(argv=None):
    return run(argv, "A2S")


if __name__ == "__main__":
    main()
