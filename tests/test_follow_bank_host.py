"""CPU: the host side of score following for parallel streams - the candidate policy follow_slot_plan, the numpy
restatement follow_bank_host against alignment.follow_dtw_host composed by hand for a scripted schedule, and the
argument errors of audio_sheet_server --follow --bank."""
import numpy as np
import pytest


def test_slot_plan_keeps_frees_and_fills_in_order():
    from audio_sheet_retrieval_amd.piece_identification import follow_slot_plan
    assert follow_slot_plan([None] * 3, [4, 2]) == ([4, 2, None], [0, 1])
    assert follow_slot_plan([4, 2, None], [2, 7, 4]) == ([4, 2, 7], [2])               # kept where they are
    assert follow_slot_plan([4, 2, 7], [7, 9]) == ([9, None, 7], [0])                  # freed, the lowest free slot first
    assert follow_slot_plan([9, None, 7], [1, 3, 7]) == ([1, 3, 7], [0, 1])            # the given order, ascending slots
    assert follow_slot_plan([1, 3, 7], []) == ([1, 3, 7], [])                          # an empty wish changes nothing
    assert follow_slot_plan([1, 3, 7], [5]) == ([5, None, None], [0])
    slots = [1, None]
    follow_slot_plan(slots, [2])
    assert slots == [1, None]                                                          # pure
    with pytest.raises(ValueError, match="3 pieces wanted for 2 slots"):
        follow_slot_plan([None, None], [1, 2, 3])
    with pytest.raises(ValueError, match="twice"):
        follow_slot_plan([None, None], [1, 1])
    with pytest.raises(ValueError, match="no piece of the data base with a segment"):
        follow_slot_plan([None, None], [1, 5], segments={1: (0, 4)})
    assert follow_slot_plan([None, None], [1], segments={1: (0, 4)}) == ([1, None], [0])


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


COUNTS = [0, 4, 3, 0, 5, 2, 6, 3]                           # windows of stream 0 per round: 23 in all
# the wishes of stream 0 before each round: 1 waits a round without windows; 2 enters late; 3 is wished for and dropped
# before a window came; 0 enters late; 1 leaves and comes back
SCHEDULE = {0: [1], 2: [1, 2], 3: [1, 3], 4: [1, 0], 5: [0], 6: [0, 1]}


@pytest.mark.parametrize("catch_up", [0, 3, 100])
def test_bank_host_equals_follow_dtw_host_composed_by_hand(catch_up):
    from audio_sheet_retrieval_amd import alignment as al
    from audio_sheet_retrieval_amd import piece_identification as pid
    rng = np.random.default_rng(7 + catch_up)
    segments = {0: (0, 9), 1: (9, 14), 2: (23, 5), 3: (28, 11)}
    db_codes = _unit(rng.standard_normal((39, 32)))
    cols = rng.random(39) * 100.0
    codes = [_unit(rng.standard_normal((23, 32))), _unit(rng.standard_normal((23, 32))), _unit(rng.standard_normal((4, 32)))]
    # stream 1 never gets a candidate; stream 2 ends after round 1 and gets its candidate afterwards
    counts = [[m, m, 4 if r == 1 else 0] for r, m in enumerate(COUNTS)]
    schedule = {r: {0: w} for r, w in SCHEDULE.items()}
    schedule[2][2] = [3]
    got, state = pid.follow_bank_host(codes, counts, schedule, db_codes, segments, n_slots=3, catch_up=catch_up,
                                      sheet_columns=cols, step_spec=2)
    K = lambda W: min(W, catch_up)
    # (slot, piece, first reported window, since, end) of stream 0
    occupancies = [(0, 1, 0, 0, 12), (1, 2, 4, 4 - K(4), 7), (1, 0, 7, 7 - K(7), 23), (0, 1, 14, 14 - K(14), 23)]
    want = pid._bank_follow_result(np.arange(23) * 2, 3, None)
    last = {}
    for slot, piece, first, since, end in occupancies:
        r0, n = segments[piece]
        cost, start, pos, st = al.follow_dtw_host(al.cosine_dists_host(codes[0][since:end], db_codes[r0:r0 + n]))
        d = first - since
        want.piece[first:end, slot], want.since[first:end, slot] = piece, since
        want.cost[first:end, slot], want.row[first:end, slot], want.start_row[first:end, slot] = cost[d:], pos[d:], start[d:]
        want.x[first:end, slot], want.start_x[first:end, slot] = cols[r0 + pos[d:]], cols[r0 + start[d:]]
        last[slot] = (piece, since, st)
    res = got[0]
    for key in ("frames", "piece", "since", "cost", "row", "start_row", "x", "start_x"):
        g, w = getattr(res, key), getattr(want, key)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), key
    # best: the occupied slot of least cost, -1 where none is occupied
    assert res.best.dtype == np.int64
    for i in range(23):
        occ = np.flatnonzero(res.piece[i] >= 0)
        assert res.best[i] == (occ[np.argmin(res.cost[i, occ])] if len(occ) else -1)
    assert (res.best[12:14] == 1).all() and (res.piece[12:14, 0] == -1).all() and np.isinf(res.cost[12:14, 0]).all()
    assert (res.piece[:, 2] == -1).all()
    # the final states are the host's last accumulated rows
    for slot, (piece, since, st) in last.items():
        p, s, pending, have = state[0][slot]
        assert (p, s, pending) == (piece, since, False) and have[2] == st[2] == 23 - since
        assert np.array_equal(have[0], st[0]) and np.array_equal(have[1], st[1])
    assert state[0][2] is None
    # a stream without candidates; a stream whose candidate came when its windows were over: pending for good
    assert len(got[1].frames) == 23 and (got[1].piece == -1).all() and np.isinf(got[1].cost).all() and (got[1].best == -1).all()
    assert (got[1].row == -1).all() and np.isnan(got[1].x).all() and (got[1].since == -1).all()
    assert state[1] == [None] * 3
    assert len(got[2].frames) == 4 and (got[2].piece == -1).all() and (got[2].best == -1).all()
    assert state[2] == [(3, -1, True, None), None, None]


def test_bank_host_refuses_a_schedule_beyond_the_codes():
    from audio_sheet_retrieval_amd import piece_identification as pid
    codes = [_unit(np.ones((3, 4)))]
    with pytest.raises(ValueError, match="4 windows scheduled, 3 codes"):
        pid.follow_bank_host(codes, [[4]], {}, _unit(np.ones((2, 4))), {0: (0, 2)})
    with pytest.raises(ValueError, match="2 window counts for 1 streams"):
        pid.follow_bank_host(codes, [[1, 1]], {}, _unit(np.ones((2, 4))), {0: (0, 2)})


def test_driver_argument_errors(capsys):
    from audio_sheet_retrieval_amd import audio_sheet_server as drv
    with pytest.raises(SystemExit) as e:
        drv._arguments(["--bank"], "A2S")
    assert e.value.code == 2 and "--bank goes with --follow" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        drv._arguments(["--follow", "--bank", "--catch_up", "513"], "A2S")
    assert e.value.code == 2 and "--catch_up must lie in 0..512" in capsys.readouterr().err
    args = drv._arguments(["--follow", "--bank"], "A2S")
    assert args.bank and args.catch_up == 64
    assert not drv._arguments(["--follow"], "A2S").bank
