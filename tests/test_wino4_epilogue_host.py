"""CPU: the store classification of conv3x3_wino4s's branch-free epilogue (csrc/wino4_epilogue.h: extent word, rows-full
rule, per-column byte offset or sentinel) built for the host with AddressSanitizer + UBSan
(tests/wino4_epilogue_harness.cpp) and compared, store by store, with the guarded rule it replaces: on rows-full
M-tiles, and in its general form (row test folded in) on the other M-tiles of the un-pooled builds.  Maps 40x50, 20x25,
23x10, 11x5, 26x18, 13x9, 24x16, 18x25 and four maps of one tile, pooled and not, 1, 5 and 1000 images; lanes past the
end of the list included.  The headline's maps (40x50, 20x25) must be rows-full everywhere."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(40, 50), (20, 25), (23, 10), (11, 5), (26, 18), (13, 9), (24, 16), (18, 25), (4, 4), (3, 2), (1, 1), (2, 3)]
BATCHES = (1, 5, 1000)
CHANNELS_WALKED = 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("wino4_epilogue") / "wino4_epilogue_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "wino4_epilogue_harness.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


def test_fast_epilogue_stores_what_the_guarded_one_stores_under_sanitizers(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.strip().split("\n")
    # every output element of the walked channels of every case was stored exactly once
    expected = 0
    for h, w in GEOMETRIES:
        for pool in (0, 1):
            oh, ow = (h // 2, w // 2) if pool else (h, w)
            expected += sum(n * oh * ow * CHANNELS_WALKED for n in BATCHES)
    assert int(lines[-1]) == expected
    shares = {}
    for ln in lines[:-1]:
        m = re.match(r"(\d+)x(\d+) pool=(\d) N=(\d+): rows-full (\d+) of (\d+) M-tiles", ln)
        assert m, ln
        h, w, pool, n, full, total = map(int, m.groups())
        shares[(h, w, pool, n)] = (full, total)
    assert len(shares) == len(GEOMETRIES) * 2 * len(BATCHES)
    for h, w in ((40, 50), (20, 25)):
        for pool in (0, 1):
            for n in BATCHES:
                full, total = shares[(h, w, pool, n)]
                assert total > 0 and full == total, (h, w, pool, n, full, total)
    # a map whose last tile row is ragged keeps some M-tiles on the guarded path
    full, total = shares[(18, 25, 0, 5)]
    assert 0 < full < total, (full, total)
