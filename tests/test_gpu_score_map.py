"""GPU: the score map (asr_score_map_dev, csrc/score_map_kernels.hip) - the measures of every piece in strip coordinates,
integer for integer against the host restatement sheet_utils/omr.score_map_host (tests/test_score_map_host.py holds that
against a derivation that walks every strip column): hand-made maps around every edge of the kernels (a wave's 64
columns, a workgroup's chunk, the band's rows over four waves, tol, the threshold, a NaN), random maps, the overflow
report; then, with the real weights on the tutorial page, load_umc_scans(..., score_map=True) against the host on the
downloaded bar maps, the lines against detect_bars' blobs, ScoreMap.rows on a data base, and umc_a2s_server --locate."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

MODEL = "mutopia_ccal_cont"
R = 7                       # min_rows of the hand-made cases
LOW, HIGH = 0.25, 0.75      # map values below / above the threshold 0.5


@pytest.fixture(scope="module")
def eng():
    from audio_sheet_retrieval_amd import _lib
    engine = _lib.Engine(MODEL, device=0)
    yield engine
    engine.close()


def _paint(rng, m, r0, r1, cols, n_rows=None, value=HIGH):
    """n_rows random rows of the band (default: R to all of them) set to `value` at every column of cols"""
    for c in cols:
        k = int(rng.integers(R, r1 - r0 + 1)) if n_rows is None else n_rows
        m[rng.choice(np.arange(r0, r1), size=k, replace=False), c] = value


def _hand_made():
    """maps, page_rows, piece_of_page, n_pieces: three pieces - piece 1 has a page and no kept system, piece 2 a first
    page without a system and two pages with some - and a last page that is not unrolled"""
    rng = np.random.default_rng(30)
    shapes = [(70, 90), (45, 131), (33, 50), (45, 131), (200, 300), (30, 40)]
    maps = [rng.uniform(0.0, LOW, s) for s in shapes]
    rows = [[] for _ in shapes]

    # page 0, piece 0: widths 65, 64, 63 and 1; c0 odd; r0 = 0; a band that ends at the page's last row
    m = maps[0]
    rows[0].append((0, 41, 1, 66, 119, 0))                   # width 65: a run into the 65th column, a run of one column
    _paint(rng, m, 0, 41, range(1 + 62, 1 + 65))
    _paint(rng, m, 0, 41, [1 + 20])
    _paint(rng, m, 0, 41, [1 + 40], n_rows=R - 1)            # one row short: no line
    _paint(rng, m, 0, 41, [1 + 42], n_rows=R)                # exactly min_rows
    rows[0].append((41, 70, 3, 67, 131, 1))                  # width 64: the run is the whole system
    _paint(rng, m, 41, 70, range(3, 67))
    rows[0].append((10, 30, 7, 70, 140, 3))                  # width 63: runs touching c0 and c1 - 1, two runs one column apart
    _paint(rng, m, 10, 30, list(range(7, 10)) + list(range(67, 70)) + list(range(27, 30)) + list(range(31, 34)))
    rows[0].append((0, 21, 89, 90, 139, 4))                  # width 1
    _paint(rng, m, 0, 21, [89])

    # page 1, piece 1: detected systems, none kept.  page 2 ... 4, piece 2: the numbering runs on
    m = maps[3]
    rows[3].append((2, 22, 1, 130, 140, 0))                  # width 129: lines exactly tol from both edges, 62 .. 66 between
    _paint(rng, m, 2, 22, [1 + 10, 129 - 10] + list(range(1 + 62, 1 + 67)))
    rows[3].append((23, 45, 1, 130, 138, 1))                 # lines tol + 1 from both edges
    _paint(rng, m, 23, 45, [1 + 11, 129 - 11])
    m = maps[4]
    rows[4].append((0, 160, 0, 300, 0, 0))                   # a run over three words, a run from a word's first column
    _paint(rng, m, 0, 160, range(30, 170))
    _paint(rng, m, 0, 160, range(192, 196))
    m[0:160, 210] = 0.5                                      # equal to the threshold: not above
    m[0:160, 220] = np.nan
    _paint(rng, m, 0, 160, [230], n_rows=R)
    m[np.flatnonzero(m[0:160, 230] == HIGH)[0], 230] = np.nan   # the NaN takes the count below min_rows
    _paint(rng, m, 0, 160, range(255, 258))
    rows[4].append((160, 200, 5, 200, 120, 2))               # no line at all
    maps[5][:] = np.nan                                      # not unrolled: never read
    page_rows = [rows[0], [], rows[2], rows[3], rows[4], None]
    return maps, page_rows, [0, 1, 2, 2, 2, 0], 3


def _random_case(seed, n_pages=5):
    """random flags: every column of every system is a line column with probability 1/2, 1/4 or 3/4"""
    rng = np.random.default_rng(seed)
    maps, page_rows, piece_of_page = [], [], []
    for p in range(n_pages):
        h, w = int(rng.integers(20, 120)), int(rng.integers(1, 400))
        m = rng.uniform(0.0, LOW, (h, w))
        rows = []
        for i in range(int(rng.integers(0, 4))):
            r0 = int(rng.integers(0, h - R))
            r1 = int(rng.integers(r0 + R, h + 1))
            c0 = int(rng.integers(0, w))
            c1 = int(rng.integers(c0 + 1, w + 1))
            m[r0:r1] = rng.uniform(0.0, LOW, (r1 - r0, w))    # bands may overlap: the last one painted wins, for both sides
            cols = c0 + np.flatnonzero(rng.random(c1 - c0) < rng.choice([0.25, 0.5, 0.75]))
            _paint(rng, m, r0, r1, cols)
            rows.append((r0, r1, c0, c1, 0, i))
        maps.append(m)
        page_rows.append(rows)
        piece_of_page.append(p // 2)
    return maps, page_rows, piece_of_page, (n_pages + 1) // 2


def _device(eng, maps, page_rows, piece_of_page, n_pieces, **kw):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    dev = O.upload_maps(eng, maps)
    try:
        return O.score_map_dev(dev, page_rows, piece_of_page, n_pieces, **kw)
    finally:
        dev.free()


def test_hand_made_maps_equal_the_host(eng):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    maps, page_rows, piece_of_page, n_pieces = _hand_made()
    want, want_first = O.score_map_host(maps, page_rows, piece_of_page, n_pieces, min_rows=R)
    # what the cases are there for, on the host's table: fixed numbers
    per_system = [int(np.sum((want[:, 2] == pg) & (want[:, 3] == s) & (np.arange(len(want)) >= want_first[q])
                             & (np.arange(len(want)) < want_first[q + 1])))
                  for q, pg, s in [(0, 0, 0), (0, 0, 1), (0, 0, 3), (0, 0, 4), (2, 1, 0), (2, 1, 1), (2, 2, 0), (2, 2, 2)]]
    assert per_system == [5, 2, 3, 1, 2, 3, 4, 1]
    assert want_first.tolist() == [0, 11, 11, 21]
    got, first = _device(eng, maps, page_rows, piece_of_page, n_pieces, min_rows=R)
    assert got.dtype == np.int32 and first.dtype == np.int32
    assert np.array_equal(first, want_first) and np.array_equal(got, want)

    # every unrolled page alone: the rows it has in the batch, up to the strip offset and the page's index
    for p, rows in enumerate(page_rows):
        if not rows:
            continue
        alone, alone_first = _device(eng, [maps[p]], [rows], [0], 1, min_rows=R)
        q = piece_of_page[p]
        k = p - piece_of_page.index(q)
        mine = want[want_first[q]:want_first[q + 1]]
        mine = mine[mine[:, 2] == k]
        assert alone_first.tolist() == [0, len(mine)]
        assert np.array_equal(alone[:, 3:], mine[:, 3:]) and np.array_equal(alone[:, :2] - alone[0, 0], mine[:, :2] - mine[0, 0])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_maps_equal_the_host(eng, seed):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    maps, page_rows, piece_of_page, n_pieces = _random_case(seed)
    for tol in (0, 10):
        want, want_first = O.score_map_host(maps, page_rows, piece_of_page, n_pieces, min_rows=R, tol=tol)
        got, first = _device(eng, maps, page_rows, piece_of_page, n_pieces, min_rows=R, tol=tol, max_lines=200)
        assert np.array_equal(first, want_first) and np.array_equal(got, want)


def test_too_many_lines_are_reported(eng):
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    rng = np.random.default_rng(5)
    m = rng.uniform(0.0, LOW, (40, 140))
    _paint(rng, m, 5, 35, range(3, 132, 2))                  # every second column of the second system
    page_rows = [[(0, 5, 0, 140, 155, 0), (5, 35, 3, 132, 130, 1)]]
    want, want_first = O.score_map_host([m], page_rows, [0], 1, min_rows=R)
    assert len(want) == 1 + 54                                # 65 lines at 0, 2 .. 128 of 129 columns: the 53 at 12 .. 116 are interior
    for max_lines in (0, 3, 52):
        with pytest.raises(ValueError, match="system 1 .*max_lines = %d" % max_lines):
            _device(eng, [m], page_rows, [0], 1, min_rows=R, max_lines=max_lines)
        with pytest.raises(ValueError, match="max_lines"):
            O.score_map_host([m], page_rows, [0], 1, min_rows=R, max_lines=max_lines)
    for max_lines in (53, 64):
        got, first = _device(eng, [m], page_rows, [0], 1, min_rows=R, max_lines=max_lines)
        assert np.array_equal(first, want_first) and np.array_equal(got, want)


def test_no_system_and_bad_arguments(eng):
    from audio_sheet_retrieval_amd import _lib
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    m = np.zeros((20, 30))
    got, first = _device(eng, [m], [[]], [0], 2)
    assert got.shape == (0, 8) and first.tolist() == [0, 0, 0]
    for rows in ([(0, 21, 0, 30, 0, 0)], [(0, 20, 0, 31, 0, 0)], [(5, 5, 0, 30, 0, 0)]):
        with pytest.raises(_lib.AsrError, match="score_map: system 0"):
            _device(eng, [m], [rows], [0], 1)
    with pytest.raises(_lib.AsrError, match="score_map: min_rows"):
        _device(eng, [m], [[(0, 20, 0, 30, 0, 0)]], [0], 1, min_rows=0)
    with pytest.raises(ValueError, match="with_index"):
        O.score_map_host([m], [[(0, 20, 0, 30, 0)]], [0], 1)


# ---- the real weights: the tutorial page of tests/golden and its whited-out variants, as tests/test_gpu_umc.py --------
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """the small UMC directory loaded twice on the device route, without the score map by load_umc_sheets and with it by
    load_umc_scans (the pages as they are: load_umc_sheets' signature is pinned, the option is the scan loader's); what the loader handed
    to unroll_systems_dev and to score_map_dev (the bar maps downloaded there), and the bar network's runs"""
    import test_gpu_umc as U
    from audio_sheet_retrieval_amd.sheet_utils import umc
    data_dir = U._umc_dir(tmp_path_factory.mktemp("score_map"))
    seen = dict(unroll=[], score_map=[], bar_runs=[])
    real_unroll, real_map = umc.unroll_systems_dev, umc.score_map_dev

    def unroll(dev_pages, page_rows, piece_of_page, n_pieces, *a, **kw):
        seen["unroll"].append(([None if r is None else list(r) for r in page_rows], list(piece_of_page), n_pieces))
        return real_unroll(dev_pages, page_rows, piece_of_page, n_pieces, *a, **kw)

    def score_map(dev_maps, page_rows, piece_of_page, n_pieces, *a, **kw):
        seen["score_map"].append((dev_maps.download(), page_rows, list(piece_of_page), n_pieces))
        return real_map(dev_maps, page_rows, piece_of_page, n_pieces, *a, **kw)

    def counted(omr):
        real = omr.bar_detector.predict_pages_dev
        runs = []
        omr.bar_detector.predict_pages_dev = lambda *a, **kw: runs.append(1) or real(*a, **kw)
        seen["bar_runs"].append(runs)
        return omr

    umc.unroll_systems_dev, umc.score_map_dev = unroll, score_map
    try:
        plain = umc.load_umc_sheets(data_dir, require_performance=True, omr=counted(U._omr()), return_device=True)
        mapped = umc.load_umc_scans(data_dir, require_performance=True, omr=counted(U._omr()), return_device=True,
                                    page_width=None, deskew=False, score_map=True)       # load_umc_sheets' route, with the map
    finally:
        umc.unroll_systems_dev, umc.score_map_dev = real_unroll, real_map
    yield plain, mapped, seen
    plain[3].buf.free()
    mapped[3].buf.free()


def test_loader_map_equals_the_host_on_the_downloaded_maps(loaded):
    import test_gpu_umc as U
    from audio_sheet_retrieval_amd.score_map import ScoreMap
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    plain, mapped, seen = loaded
    assert len(plain) == 4 and len(mapped) == 5 and isinstance(mapped[4], ScoreMap)
    assert mapped[0] == plain[0] == U.KEPT and mapped[1] == plain[1]
    for a, b, c, d in zip(plain[2], mapped[2], U._download(plain[3]), U._download(mapped[3])):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    (rows_a, pieces_a, n_a), (rows_b, pieces_b, n_b) = seen["unroll"]
    assert pieces_a == pieces_b and n_a == n_b == len(U.KEPT)
    assert [None if r is None else [s[:5] for s in r] for r in rows_b] == rows_a           # the same systems, the index added
    assert [len(r) for r in seen["bar_runs"]] == [1, 1]                                    # the bar network ran once each
    (maps, page_rows, piece_of_page, n_pieces), = seen["score_map"]
    want, want_first = O.score_map_host(maps, page_rows, piece_of_page, n_pieces)
    sm = mapped[4]
    assert sm.names == U.KEPT and sm.widths.tolist() == [s.shape[1] for s in mapped[2]]
    assert np.array_equal(np.concatenate(sm.tables), want)
    assert np.cumsum([0] + [len(t) for t in sm.tables]).tolist() == want_first.tolist()
    # p2_two_pages: the whited-out page first, the full page second - the numbering runs on
    t = sm.tables[U.KEPT.index("p2_two_pages")]
    assert t[:, 2].tolist() == sorted(t[:, 2].tolist()) and set(t[:, 2].tolist()) == {0, 1}
    assert np.array_equal(t[t[:, 2] == 1][:, 2:], sm.tables[U.KEPT.index("p1_page")][:, 2:] + [1, 0, 0, 0, 0, 0])


def test_lines_of_the_full_page_against_detect_bars(loaded):
    """every interior bar of detect_bars_pages_dev has exactly one interior line of the score map within 2 px, and the
    reverse; per system 2, 2, 2, 2, 3, 2 measures - what the defaults were chosen on with the float32 numpy network
    (tests/test_score_map_host.py), here on the device's own maps"""
    import test_gpu_umc as U
    from audio_sheet_retrieval_amd.sheet_utils import omr as O
    sm = loaded[1][4]
    page = U._tutorial()
    omr = U._omr()
    systems, = omr.detect_systems_pages_dev([page])
    bars, = omr.detect_bars_pages_dev([page])
    t = sm.tables[U.KEPT.index("p1_page")]
    print("measures per system:", np.bincount(t[:, 3]).tolist())
    tol = O.BAR_MISSING_TOL
    for k, (s, mine) in enumerate(zip(systems, O.bars_by_systems(bars, systems))):
        c0, c1 = int(s[0, 1]), int(s[1, 1])
        cols = mine[:, 0, 1]
        inner = cols[(cols - c0 > tol) & ((c1 - 1) - cols > tol)]
        rows = t[t[:, 3] == k]
        lines = rows[1:, 4]
        print("system %d: detect_bars %s, score map %s" % (k, inner.tolist(), lines.tolist()))
        assert np.all(rows[:, 4:6] >= c0) and np.all(rows[:, 4:6] <= c1) and rows[0, 4] == c0 and rows[-1, 5] == c1
        for b in inner:
            assert np.sum(np.abs(lines - b) <= 2) == 1, (k, b, lines)
        for b in lines:
            assert np.sum(np.abs(inner - b) <= 2) == 1, (k, b, inner)
    assert np.bincount(t[:, 3]).tolist() == [2, 2, 2, 2, 3, 2]


def test_rows_of_a_data_base_agree_with_at(loaded):
    import test_gpu_umc as U
    from audio_sheet_retrieval_amd.piece_identification import EmbeddingDB, default_sheet_columns
    names, _, _, dev, sm = loaded[1]
    eng = U._engine()
    try:
        db = EmbeddingDB.from_images(eng, names, dev)
        try:
            got = sm.rows(db)
            cols = default_sheet_columns(db.ids, int(eng.cfg.w1))
            assert len(db) > 100 and all(g.shape == (len(db),) for g in got)
            for i in range(len(db)):
                want = sm.at(db.id_to_name[int(db.ids[i])], cols[i])
                assert [int(g[i]) for g in got] == [int(w) for w in want], i
            assert min(g.min() for g in got) >= 0
        finally:
            db.close()
    finally:
        eng.close()


from test_gpu_umc import exp_root  # noqa: E402,F401  (the experiment folder with the parameter pickles)


def test_driver_locates_in_bars_and_pages(exp_root, tmp_path, capsys):  # noqa: F811
    import yaml
    import test_gpu_umc as U
    from audio_sheet_retrieval_amd import umc_a2s_server
    from audio_sheet_retrieval_amd.score_map import ScoreMap
    data_dir = U._umc_dir(tmp_path)
    common = ["--model", "models/%s.py" % U.MODEL, "--data_dir", data_dir, "--train_split", U.SPLIT, "--config", U.CONFIG,
              "--n_candidates", "9", "--locate", "--excerpt_frames", "60", "--locate_pieces", "3"] + U._omr_flags(exp_root)
    entries = umc_a2s_server.main(common + ["--init_sheet_db", "--dump_results"])
    text = capsys.readouterr().out
    res_file = exp_root / U.MODEL / ("umc_location_%s_umc_test_A2S.yaml" % U.TAG)
    with open(res_file) as fp:
        assert yaml.safe_load(fp) == entries
    sm = ScoreMap.load("umc_sheet_db_file_score_map.npz")
    assert sm.names == U.KEPT and [e["name"] for e in entries] == [n for n in U.KEPT if n != "p7_no_score_ppq"]
    assert "location of 4 recordings written to" in text
    for e in entries:
        assert e["candidate"] in U.KEPT and 0 <= e["own_rank"] <= 3
        assert 1 <= e["first_bar"] <= e["last_bar"] <= sm.n_bars(e["candidate"])
        assert 0 <= e["start_page"] <= e["end_page"] < sm.n_pages(e["candidate"])
        assert (e["start_page"], e["start_system"]) == sm.measure_box(e["candidate"], e["first_bar"] - 1)[:2]
        assert (e["end_page"], e["end_system"]) == sm.measure_box(e["candidate"], e["last_bar"] - 1)[:2]
    # a run without --init_sheet_db loads the data base and the map: the same report
    assert umc_a2s_server.main(common) == entries
