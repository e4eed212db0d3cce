"""CPU: the tile decode of conv3x3_winog (csrc/wino_tile_order.h: one reciprocal division per M-tile on wave-uniform
values, then a per-lane walk over strip and image ends) built for the host with AddressSanitizer + UBSan
(tests/wino_tile_order_harness.cpp) and compared, tile by tile, with the closed form of three divisions it replaced.
Geometries (tile rows x columns) 27x19, 26x18, 3x1, 1x1, 7x5, 80x100; strips of 1, 2, 4, 8 rows with their shorter last
strips; 1, 2, 5 images; lanes past the end of the list included."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(27, 19), (26, 18), (3, 1), (1, 1), (7, 5), (80, 100)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("wino_tile_order") / "wino_tile_order_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "wino_tile_order_harness.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


def test_tile_decode_matches_the_closed_form_under_sanitizers(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-3000:]
    # every lane slot of every M-tile of every case was compared
    expected = sum(16 * ((n * ty * tx + 15) // 16) for ty, tx in GEOMETRIES for _s in (1, 2, 4, 8) for n in (1, 2, 5))
    assert int(res.stdout.strip()) == expected
