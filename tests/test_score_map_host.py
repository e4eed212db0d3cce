"""CPU: the score map's definition (include/asr_hip.h, asr_score_map_dev) as sheet_utils/omr.score_map_host restates it,
against a derivation that walks every strip column of seeded random pieces; ScoreMap.at / measure_box / annotate / save /
load; and the recorded column counts of the tutorial page (tests/golden/omr_tutorial_bar_counts.npz, written by
tools/record_score_map_fixture.py), which must give the 13 measures the defaults were chosen on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))

from audio_sheet_retrieval_amd.score_map import ScoreMap  # noqa: E402
from audio_sheet_retrieval_amd.sheet_utils import omr as O  # noqa: E402

MIN_ROWS, TOL, THRESHOLD = 3, 10, 0.5


def _random_pieces(seed, n_pieces):
    """maps, page_rows (with the systems' indices; some systems dropped, some pages not unrolled), piece_of_page: 0 to 3
    pages per piece, 0 to 4 systems per page, widths from 1 column, lines at and within tol of both edges"""
    rng = np.random.default_rng(seed)
    maps, page_rows, piece_of_page = [], [], []
    for q in range(n_pieces):
        for _ in range(int(rng.integers(0, 4))):
            h, w = int(rng.integers(8, 40)), int(rng.choice([1, 2, 12, 23, 24, 60, 150, 300, 500]))
            m = rng.uniform(0.0, 0.4, (h, w))
            rows, top = [], 0
            for i in range(int(rng.integers(0, 5))):
                if top + 4 > h:
                    break
                r0, r1 = top, int(rng.integers(top + 4, h + 1))
                top = r1
                if rng.random() < 0.25:
                    continue                                  # a detected system the unroll drops: the indices skip it
                c0 = int(rng.integers(0, max(1, w // 4)))
                c1 = int(rng.integers(c0 + 1, w + 1))
                picks = [c0, c1 - 1, c0 + TOL, c0 + TOL + 1, c1 - 1 - TOL, c1 - 2 - TOL]
                cols = [c for c in picks if c0 <= c < c1 and rng.random() < 0.4]
                cols += list(rng.integers(c0, c1, int(rng.integers(0, 6))))
                for c in cols:
                    for cc in range(c, min(c1, c + int(rng.integers(1, 4)))):     # runs of one to three columns
                        m[rng.choice(np.arange(r0, r1), size=int(rng.integers(MIN_ROWS - 1, r1 - r0 + 1)), replace=False),
                          cc] = rng.choice([0.6, 0.9, 0.5, np.nan], p=[0.45, 0.45, 0.05, 0.05])
                rows.append((r0, r1, c0, c1, 160 - (r1 - r0), i))
            maps.append(m)
            page_rows.append(rows)
            piece_of_page.append(q)
    return maps, page_rows, piece_of_page


def _walk(maps, page_rows, piece_of_page, n_pieces):
    """per piece, for every strip column in order: (bar, page, system, page_row, page_col) - one Python step per page
    column, no array operation"""
    out = [[] for _ in range(n_pieces)]
    first_page = {}
    for p, rows in enumerate(page_rows):
        q = piece_of_page[p]
        first_page.setdefault(q, p)
        for r0, r1, c0, c1, _, index in rows:
            flags = []
            for c in range(c0, c1):
                n = 0
                for r in range(r0, r1):
                    if maps[p][r, c] > THRESHOLD:
                        n += 1
                flags.append(n >= MIN_ROWS)
            starts = {c0}
            c = c0
            while c < c1:
                if flags[c - c0]:
                    last = c
                    while last + 1 < c1 and flags[last + 1 - c0]:
                        last += 1
                    b = (c + last) // 2
                    if b - c0 > TOL and (c1 - 1) - b > TOL:
                        starts.add(b)
                    c = last
                c += 1
            bar = out[q][-1][0] if out[q] else -1
            for c in range(c0, c1):
                if c in starts:
                    bar += 1
                out[q].append((bar, p - first_page[q], index, (r0 + r1) // 2, c))
    return out


@pytest.fixture(scope="module")
def pieces():
    n_pieces = 300
    maps, page_rows, piece_of_page = _random_pieces(30, n_pieces)
    table, first = O.score_map_host(maps, page_rows, piece_of_page, n_pieces, THRESHOLD, MIN_ROWS, TOL)
    widths = np.zeros(n_pieces, np.int64)
    for p, rows in enumerate(page_rows):
        widths[piece_of_page[p]] += sum(c1 - c0 for _, _, c0, c1, _, _ in rows)
    return maps, page_rows, piece_of_page, n_pieces, table, first, widths


def test_host_table_against_the_column_walk(pieces):
    maps, page_rows, piece_of_page, n_pieces, table, first, widths = pieces
    walked = _walk(maps, page_rows, piece_of_page, n_pieces)
    assert [len(w) for w in walked] == widths.tolist()
    assert sum(len(w) for w in walked) > 20000 and min(widths) == 0 and table.dtype == np.int32
    sm = ScoreMap.from_table(["piece%03d" % q for q in range(n_pieces)], table, first, widths)
    several = 0
    for q, want in enumerate(walked):
        got = np.stack(sm.at(q, np.arange(len(want))), axis=1) if want else np.zeros((0, 5), np.int64)
        assert np.array_equal(got, np.asarray(want, np.int64).reshape(-1, 5)), q
        assert sm.n_bars(q) == (want[-1][0] + 1 if want else 0)
        several += sm.n_bars(q) > sum(len(rows) for p, rows in enumerate(page_rows) if piece_of_page[p] == q)
    assert several > 50                                       # interior lines do occur


def test_tables_tile_their_strips(pieces):
    _, _, _, n_pieces, table, first, widths = pieces
    assert first[0] == 0 and first[-1] == len(table) and np.all(np.diff(first) >= 0)
    for q in range(n_pieces):
        t = table[first[q]:first[q + 1]]
        if widths[q] == 0:
            assert len(t) == 0
            continue
        assert t[0, 0] == 0 and t[-1, 1] == widths[q]
        assert np.array_equal(t[1:, 0], t[:-1, 1]) and np.all(t[:, 1] > t[:, 0])
        assert np.array_equal(t[:, 1] - t[:, 0], t[:, 5] - t[:, 4])
        same = (t[1:, 2] == t[:-1, 2]) & (t[1:, 3] == t[:-1, 3])           # the next measure of the same system ...
        assert np.array_equal(t[1:, 4][same], t[:-1, 5][same])             # ... goes on where this one ends: page_col runs on
        assert np.all(np.diff(t[:, 2]) >= 0)


def test_at_clips_floors_and_marks_nothing():
    t = [[0, 5, 0, 0, 10, 15, 20, 31], [5, 12, 0, 0, 15, 22, 20, 31], [12, 13, 1, 2, 3, 4, 0, 160]]
    sm = ScoreMap(["a", "empty"], [t, np.zeros((0, 8))], [13, 0])
    bar, page, system, row, col = sm.at("a", [[-3.0, 0.0, 4.99], [5.0, 11.5, 12.0], [40.0, np.nan, 12.9]])
    assert bar.tolist() == [[0, 0, 0], [1, 1, 2], [2, -1, 2]] and bar.dtype == np.int64
    assert page.tolist() == [[0, 0, 0], [0, 0, 1], [1, -1, 1]] and system.tolist() == [[0, 0, 0], [0, 0, 2], [2, -1, 2]]
    assert row.tolist() == [[25, 25, 25], [25, 25, 80], [80, -1, 80]]
    assert col.tolist() == [[10, 10, 14], [15, 21, 3], [3, -1, 3]]
    assert [int(v) for v in sm.at(0, 7)] == [1, 0, 0, 25, 17] and sm.at("a", 7)[0].shape == ()
    assert all(v.tolist() == [-1, -1] for v in sm.at("empty", [0, 3]))
    assert sm.measure_box("a", 2) == (1, 2, 0, 160, 3, 4) and sm.n_bars("a") == 3 and sm.n_pages("a") == 2
    assert sm.n_pages("empty") == 0
    with pytest.raises(IndexError):
        sm.measure_box("a", 3)
    with pytest.raises(KeyError):
        sm.at("b", 0)
    with pytest.raises(ValueError, match="tile"):
        ScoreMap(["a"], [t], [14])
    with pytest.raises(ValueError, match="tile"):
        ScoreMap(["a"], [[t[0], t[2]]], [13])


def test_save_load_round_trip(pieces, tmp_path):
    _, _, _, n_pieces, table, first, widths = pieces
    sm = ScoreMap.from_table(["piece %d" % q for q in range(n_pieces)], table, first, widths)
    path = ScoreMap.path_for(str(tmp_path / "umc_sheet_db_file.pkl"))
    assert path.endswith("umc_sheet_db_file_score_map.npz")
    sm.save(path)
    back = ScoreMap.load(path)
    assert back.names == sm.names and np.array_equal(back.widths, sm.widths)
    assert all(np.array_equal(a, b) and b.dtype == np.int32 for a, b in zip(sm.tables, back.tables))


def test_annotate_hand_made_results():
    from audio_sheet_retrieval_amd.piece_identification import BankFollowResult, FollowResult
    a = [[0, 50, 0, 0, 10, 60, 0, 160], [50, 80, 0, 1, 10, 40, 200, 360], [80, 100, 1, 0, 5, 25, 40, 200]]
    b = [[0, 30, 0, 3, 7, 37, 100, 260]]
    sm = ScoreMap(["a", "b", "c"], [a, b, np.zeros((0, 8))], [100, 30, 0])
    # a candidate of locate_scores
    cand = dict(name="a", votes=1.0, vote_rank=1, cost=0.1, start_row=0, end_row=3, start_x=49.0, end_x=99.0,
                x=np.asarray([49.0, 50.0, 79.0, 99.0]))
    ann = sm.annotate(cand)
    assert sorted(ann) == ["end_x", "start_x", "x"] and sorted(ann["x"]) == sorted(["bar", "page", "system", "page_row", "page_col"])
    assert ann["x"]["bar"].tolist() == [0, 1, 1, 2] and ann["x"]["page"].tolist() == [0, 0, 0, 1]
    assert ann["x"]["system"].tolist() == [0, 1, 1, 0] and ann["x"]["page_col"].tolist() == [59, 10, 39, 24]
    assert ann["x"]["page_row"].tolist() == [80, 280, 280, 120]
    assert int(ann["start_x"]["bar"]) == 0 and int(ann["end_x"]["bar"]) == 2 and ann["start_x"]["bar"].shape == ()
    # a FollowResult: one column per candidate
    x = np.asarray([[10.0, 5.0, 0.0], [60.0, 29.0, 0.0]])
    res = FollowResult(np.asarray([0, 2]), np.zeros((2, 3)), np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32), x,
                       np.zeros((2, 3)), [0, 1, 2], ["a", "b", "c"])
    ann = sm.annotate(res)
    assert ann["x"]["bar"].tolist() == [[0, 0, -1], [1, 0, -1]] and ann["start_x"]["bar"].tolist() == [[0, 0, -1], [0, 0, -1]]
    assert ann["x"]["page_col"].tolist() == [[20, 12, -1], [20, 36, -1]] and ann["x"]["system"].tolist() == [[0, 3, -1], [1, 3, -1]]
    # a BankFollowResult: slots change their pieces and may be empty
    piece = np.asarray([[0, -1], [0, 1], [-1, 1]], np.int32)
    x = np.where(piece >= 0, np.asarray([[85.0, 0.0], [99.0, 29.0], [0.0, 1.0]]), np.nan)
    bank = BankFollowResult(np.asarray([0, 2, 4]), piece, np.where(piece >= 0, 0.5, np.inf), np.where(piece >= 0, 1, -1),
                            np.where(piece >= 0, 0, -1), x, np.where(piece >= 0, 0.0, np.nan),
                            np.where(piece >= 0, 0, -1).astype(np.int64), {0: "a", 1: "b", 2: "c"})
    ann = sm.annotate(bank)
    assert ann["x"]["bar"].tolist() == [[2, -1], [2, 0], [-1, 0]] and ann["x"]["page"].tolist() == [[1, -1], [1, 0], [-1, 0]]
    assert ann["x"]["page_col"].tolist() == [[10, -1], [24, 36], [-1, 8]]
    assert ann["start_x"]["bar"].tolist() == [[0, -1], [0, 0], [-1, 0]]
    assert ann["start_x"]["page_row"].tolist() == [[80, -1], [80, 180], [-1, 180]]


def test_unroll_rows_index_is_opt_in():
    systems = np.zeros((3, 4, 2))
    for k, (top, bottom) in enumerate([(70, 110), (5, 25), (300, 420)]):      # the second lies too close to the top edge:
        systems[k, :, 0] = [top, top, bottom, bottom]                         # 65 rows of padding, dropped
        systems[k, :, 1] = [7, 90, 90, 7]
    plain = O.unroll_rows((500, 100), systems)
    indexed = O.unroll_rows((500, 100), systems, with_index=True)
    assert plain == [(10, 170, 7, 90, 0), (280, 440, 7, 90, 0)]
    assert [r[:5] for r in indexed] == plain and [r[5] for r in indexed] == [0, 2]


def test_tutorial_page_counts_give_thirteen_measures():
    """the recorded counts of the six systems (float32 numpy U-Net, the reference's weights, threshold 0.5)"""
    z = np.load(os.path.join(GOLDEN, "omr_tutorial_bar_counts.npz"))
    rows = [tuple(int(v) for v in r) for r in z["rows"]]
    assert len(rows) == 6 and float(z["threshold"]) == 0.5
    cuts = np.cumsum([c1 - c0 for _, _, c0, c1, _, _ in rows])
    counts = np.split(z["counts"].astype(np.int64), cuts[:-1])
    table, first = O.score_map_host(None, [rows], [0], 1, counts=counts)       # the defaults: min_rows 60, tol 10
    assert first.tolist() == [0, 13]
    assert table[:, 0].tolist() == [0, 352, 693, 1102, 1444, 1847, 2196, 2595, 2939, 3197, 3427, 3689, 4095]
    assert table[-1, 1] == 4437 == cuts[-1]
    assert np.bincount(table[:, 3]).tolist() == [2, 2, 2, 2, 3, 2] and np.all(table[:, 2] == 0)
    interior = [t[4] for t in table.tolist() if t[4] != rows[t[3]][2]]
    assert interior == [452, 449, 442, 446, 300, 530, 448]
    for min_rows in (30, 60):                                 # the plateau the default sits on; 80 loses the shortest lines
        assert len(O.score_map_host(None, [rows], [0], 1, min_rows=min_rows, counts=counts)[0]) == 13
    assert len(O.score_map_host(None, [rows], [0], 1, min_rows=80, counts=counts)[0]) == 11
    with pytest.raises(ValueError, match="max_lines"):
        O.score_map_host(None, [rows], [0], 1, counts=counts, max_lines=1)
    assert len(O.score_map_host(None, [rows], [0], 1, counts=counts, max_lines=2)[0]) == 13


def test_the_loader_option_is_load_umc_scans_and_needs_the_device_route():
    """score_map is a keyword of load_umc_scans, off by default (load_umc_sheets' parameter list is pinned by earlier
    tests and stays); without return_device it is refused before anything is read or built"""
    import inspect
    from audio_sheet_retrieval_amd.sheet_utils import umc
    assert inspect.signature(umc.load_umc_scans).parameters["score_map"].default is False
    assert "score_map" not in inspect.signature(umc.load_umc_sheets).parameters
    with pytest.raises(ValueError, match="return_device"):
        umc.load_umc_scans("no such directory", score_map=True)
    from audio_sheet_retrieval_amd import umc_a2s_server
    args = umc_a2s_server._arguments(["--model", "m", "--locate", "--excerpt_frames", "60"], "A2S")
    assert args.locate and args.excerpt_frames == 60 and args.locate_pieces == 5 and args.step_spec == 2
    assert not umc_a2s_server._arguments(["--model", "m"], "A2S").locate
