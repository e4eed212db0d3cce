"""CPU: the music gate at the level of what has been heard so far, restated in numpy
(piece_identification.RunningLevel, track_gate_host(level=RunningLevel(...))) - the yardstick of
asr_track_gate_running_dev and asr_track_stream_gate_running_dev.  Frame i of the running gate must be the last frame of
the reference's gate (track_gate_host at the recording's own level) on the columns heard so far, bit for bit."""
import numpy as np
import pytest

from audio_sheet_retrieval_amd import piece_identification as pid
from audio_sheet_retrieval_amd.piece_identification import RunningLevel, track_gate_host

#: (bins, w, T, L); L == 0: unbounded memory
CASES = [(5, 8, 300, 0), (5, 8, 300, 8), (5, 8, 300, 13), (3, 9, 120, 40), (92, 42, 200, 60), (92, 42, 200, 0)]
AMPLITUDES = [1, 1, 20, 1, 1, 1, 0.02, 1]


def level_signal(bins, T, seed=0):
    """noise times a per-frame amplitude in eight equal stretches: a loud one and a nearly silent one, so that the level
    of the whole recording, of the columns so far and of the last L columns differ in many frames"""
    rng = np.random.default_rng(seed)
    amp = np.repeat(np.asarray(AMPLITUDES, np.float32), -(-T // len(AMPLITUDES)))[:T]
    return np.ascontiguousarray(rng.random((bins, T), dtype=np.float32) * amp)


def running_level(L, floor=None):
    return RunningLevel(memory=L or None, floor=floor)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_the_three_gates_differ_on_the_test_signal():
    spec = level_signal(5, 300)
    n = [int(track_gate_host(spec, 8, lv)[1].sum()) for lv in (None, RunningLevel(), RunningLevel(memory=8))]
    assert n[0] < n[1] < n[2], n


@pytest.mark.parametrize("bins,w,T,L", CASES)
def test_frame_i_is_the_last_frame_of_the_reference_gate_on_the_columns_so_far(bins, w, T, L):
    spec = level_signal(bins, T)
    m_prob, voiced = track_gate_host(spec, w, running_level(L))
    assert m_prob.dtype == np.float32 and m_prob.shape == (T,) and voiced.shape == (T,)
    bad = []
    for i in range(T):
        lo = 0 if L == 0 else max(0, i - L + 1)
        excerpt = spec[:, lo:i + 1]
        if excerpt.shape[1] == 1:
            # numpy sums a (bins, 1) array along its only column pairwise, not row after row as it sums every wider
            # one and as the contract defines c_j (with 92 bins the last bit differs).  The zeros that stand before
            # column 0 anyway, written out, keep the reference on the row-after-row path; they change neither the
            # mean's window nor the maximum (column sums are >= 0 here).
            excerpt = np.hstack((np.zeros((bins, 1), np.float32), excerpt))
        m_ref, v_ref = track_gate_host(excerpt, w)           # (frame 0 or 1 of an excerpt: unvoiced either way, w >= 8)
        if bits(m_prob[i]) != bits(m_ref[-1]) or (L == 0 and bool(voiced[i]) != bool(v_ref[-1])):
            bad.append(i)
        if L and bool(voiced[i]) != (m_prob[i] > 0.5 and i >= w):       # the stream position, not the excerpt's
            bad.append(i)
    assert not bad, bad[:10]


@pytest.mark.parametrize("L", [0, 8, 13])
def test_the_levels_are_the_maxima_of_the_last_columns(L):
    c = level_signal(5, 300).sum(axis=0)
    want = np.array([c[(max(0, i - L + 1) if L else 0):i + 1].max() for i in range(c.size)], np.float32)
    assert np.array_equal(bits(running_level(L).levels(c)), bits(want))


@pytest.mark.parametrize("bins,w,T,L", CASES)
def test_a_floor_changes_frames_and_never_voices_one(bins, w, T, L):
    # A floor acts only where the level lies below it.  With a memory shorter than a stretch of the signal that is the
    # nearly silent stretch; otherwise only the frames before the maximum so far passes the median - frame 0 if its
    # column sum lies below the median, which it does with this seed.
    spec = level_signal(bins, T, seed=1)
    floor = float(np.median(spec.sum(axis=0)))
    m0, v0 = track_gate_host(spec, w, running_level(L))
    m1, v1 = track_gate_host(spec, w, running_level(L, floor))
    assert (bits(m0) != bits(m1)).any()
    assert not (v1 & ~v0).any()
    if 0 < L < T // len(AMPLITUDES):
        assert (v0 & ~v1).any()                             # the nearly silent stretch no longer counts as music


def test_a_silent_prefix_is_nan_and_unvoiced():
    spec = np.concatenate([np.zeros((5, 20), np.float32), level_signal(5, 40)], axis=1)
    m, v = track_gate_host(spec, 8, RunningLevel())
    assert np.isnan(m[:20]).all() and not v[:20].any() and np.isfinite(m[20:]).all()


def test_running_level_validates_its_fields():
    for kw in ({"memory": -1}, {"memory": (1 << 20) + 1}, {"memory": 2.5}, {"floor": float("nan")}, {"floor": float("inf")}):
        with pytest.raises(ValueError):
            RunningLevel(**kw)
    lv = RunningLevel(memory=1 << 20, floor=-np.inf)
    assert (lv.memory_arg, lv.floor_arg) == (1 << 20, -np.inf)
    assert (RunningLevel().memory_arg, RunningLevel().floor_arg) == (0, -np.inf)
    assert RunningLevel(memory=60, floor=2.5).floor_arg == 2.5
    spec = level_signal(5, 30)
    for memory in range(1, 8):                              # shorter than the window: at use
        with pytest.raises(ValueError):
            track_gate_host(spec, 8, RunningLevel(memory=memory))
    track_gate_host(spec, 8, RunningLevel(memory=8))


class _FakeDB(object):
    ids = np.zeros(8, np.int32)
    id_to_name = {0: "a"}
    n_pieces = 1

    def __len__(self):
        return 8


def test_the_host_state_sessions_refuse_a_running_level():
    with pytest.raises(ValueError, match="PieceTrackerBank"):
        pid.PieceTracker(None, _FakeDB(), RunningLevel())
    with pytest.raises(ValueError, match="PieceTrackerBank"):
        pid.live_track_scores(None, _FakeDB(), None, [np.zeros(100, np.float32)], [22050], 50, levels=RunningLevel(),
                              batched=False)


def test_n_streams_goes_with_a_running_level_and_only_with_one():
    with pytest.raises(ValueError, match="n_streams"):
        pid.PieceTrackerBank(None, _FakeDB(), RunningLevel())
    with pytest.raises(ValueError, match="n_streams"):
        pid.PieceTrackerBank(None, _FakeDB(), [1.0, 2.0], n_streams=2)
    with pytest.raises(ValueError):
        pid.PieceTrackerBank(None, _FakeDB(), RunningLevel(memory=8), n_streams=2)     # shorter than the 42-column window
