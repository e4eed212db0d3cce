"""CPU: the host half of the streamed audio front-end (asr_audio_stream_push_dev, include/asr_hip.h) -
audio_frontend.audio_stream_plan / audio_stream_state_len against brute force over random cuts, and
resample_stream_host (the restatement of the resampling half) against resample_host on the whole recording."""
import math

import numpy as np
import pytest

from audio_sheet_retrieval_amd import audio_frontend as af

F, HOP = af.FRAME_SIZE, af.SAMPLE_RATE / float(af.FPS)
RATES = [22050, 44100, 48000, 16000, 8000, 11025, 192000]


def _ratio(rate):
    """(up, down, half, taps_per_phase) without building the tap table (it is 41 k taps at 192 kHz)"""
    if rate == af.SAMPLE_RATE:
        return 1, 1, 0, 0
    g = math.gcd(rate, af.SAMPLE_RATE)
    up, down = af.SAMPLE_RATE // g, rate // g
    half = 16 * max(up, down)
    return up, down, half, -(-(2 * half + 1) // up)


def _brute_outputs(n, up, down, half, T):
    """final outputs by the definition: m with (m * down + half) // up < n, at most ceil(n * up / down)"""
    if not T:
        return n
    m = 0
    cap = -(-n * up // down)
    while m < cap and (m * down + half) // up < n:
        m += 1
    return m


def _brute_frames(m):
    i = 0
    while int(i * HOP) + F <= m:
        i += 1
    return i


def _cuts(rng, total):
    """block lengths summing to `total`: 0- and 1-sample blocks, short and long ones"""
    cuts, left = [], total
    while left:
        kind = rng.randint(5)
        n = (0, 1, rng.randint(2, 40), rng.randint(40, 3000), rng.randint(3000, 12000))[kind]
        n = min(n, left)
        cuts.append(n)
        left -= n
    return cuts


def test_the_ratio_helper_matches_resample_plan():
    for rate in (44100, 48000, 16000):
        up, down, half, taps = af.resample_plan(rate)
        assert _ratio(rate) == (up, down, half, taps.shape[1])


@pytest.mark.parametrize("rate", RATES)
def test_plan_against_brute_force_over_random_cuts(rate):
    up, down, half, T = _ratio(rate)
    rng = np.random.RandomState(rate % 1000)
    cap = af.audio_stream_state_len(F, up, down, T)
    total = int(0.45 * rate) + rng.randint(0, 50)           # about 9 hops: several complete frames at every rate
    n, frames, worst = 0, 0, 0
    for cnt in _cuts(rng, total):
        first, new, keep = af.audio_stream_plan(n, cnt, False, F, HOP, up, down, half, T)
        n += cnt
        want = _brute_frames(_brute_outputs(n, up, down, half, T))
        assert first == frames and first + new == want, (rate, n, cnt, first, new, want)
        frames = want
        s = int(frames * HOP)
        want_keep = max(0, min(n, ((s * down + half) // up - (T - 1)) if T else s))
        assert keep == want_keep and 0 <= keep <= n
        assert n - keep <= cap, (rate, n, keep, cap)
        worst = max(worst, n - keep)
    assert frames >= 3 and worst > cap // 2                 # the walk went through whole frames and filled the state
    first, new, keep = af.audio_stream_plan(n, 0, True, F, HOP, up, down, half, T)
    length = -(-n * up // down)
    assert first == frames and first + new == int(np.ceil(length / HOP))       # SpectrogramProcessor.num_frames
    assert n - keep <= cap


def test_state_lengths_of_the_common_rates():
    got = [af.audio_stream_state_len(F, *(_ratio(r)[:2] + _ratio(r)[3:])) for r in (22050, 44100, 48000, 192000)]
    assert got == [2047, 4158, 4526, 18103]


def test_a_frame_is_emitted_by_the_sample_that_completes_it():
    for i in (0, 1, 7):
        end = int(i * HOP) + F
        assert af.audio_stream_plan(0, end - 1, False, F, HOP)[:2] == (0, i)
        assert af.audio_stream_plan(end - 1, 1, False, F, HOP)[:2] == (i, 1)
        assert af.audio_stream_plan(0, end, False, F, HOP) == (0, i + 1, int((i + 1) * HOP))


def test_an_empty_stream_flushes_to_nothing():
    assert af.audio_stream_plan(0, 0, True, F, HOP) == (0, 0, 0)
    assert af.audio_stream_plan(0, 0, True, F, HOP, *_ratio(44100)) == (0, 0, 0)
    assert af.audio_stream_plan(0, 1, True, F, HOP)[:2] == (0, 1)


@pytest.mark.parametrize("rate", [44100, 48000, 16000])
@pytest.mark.parametrize("integer", [False, True])
def test_the_streamed_resampler_equals_the_whole_recording(rate, integer):
    rng = np.random.RandomState(rate // 100 + integer)
    n = 3000
    x = rng.randn(n).astype(np.float32)
    if integer:
        x = np.clip(np.rint(x * 15000), -32768, 32767).astype(np.float32)
    whole = af.resample_host(x, rate, integer)
    up, down, half, taps = af.resample_plan(rate)
    stream = af.resample_stream_host(rate, integer)
    parts, pos = [], 0
    for cnt in [0, 1, 5] + _cuts(rng, n - 6):
        parts.append(stream.push(x[pos:pos + cnt]))
        pos += cnt
        so_far = np.concatenate(parts)
        assert so_far.size == _brute_outputs(pos, up, down, half, taps.shape[1]) == stream.n_out
        assert np.array_equal(so_far, whole[:so_far.size])             # a prefix before the flush
        assert stream._tail.size <= taps.shape[1] + down                # the carried tail does not grow with the blocks
    assert pos == n
    parts.append(stream.flush())
    got = np.concatenate(parts)
    assert got.dtype == np.float32 and got.shape == whole.shape and np.array_equal(got, whole)
    with pytest.raises(ValueError):
        stream.push(x[:1])


def test_the_binding_is_declared():
    from audio_sheet_retrieval_amd import _lib
    assert "asr_audio_stream_push_dev" in _lib.EXPORTS
    assert hasattr(af.SpectrogramProcessor, "stream") and hasattr(af.AudioStream, "push_dev")


def test_the_driver_flags_parse_and_default_to_off():
    from audio_sheet_retrieval_amd import umc_a2s_server as drv
    args = drv._arguments([], "A2S")
    assert args.live is False and args.block_ms == 100.0 and args.resample is False
    args = drv._arguments(["--live", "--block_ms", "50", "--running_frames", "30"], "A2S")
    assert args.live is True and args.block_ms == 50.0 and args.running_frames == 30
    assert not hasattr(drv._arguments([], "S2A"), "live")
    assert drv.tracking_file("params_tag.pkl", "umc", False) == "umc_tracking_tag_umc_A2S.yaml"
    assert drv.tracking_file("params_tag.pkl", "umc", True) == "umc_tracking_tag_umc_A2S_real.yaml"
