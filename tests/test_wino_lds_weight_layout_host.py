"""CPU: where conv3x3_wino (the LDS-patch Winograd kernel) keeps its transformed weights in LDS
(csrc/wino_lds_weight_layout.h), built for the host with AddressSanitizer + UBSan
(tests/wino_lds_weight_layout_harness.cpp).  For (C_in, C_out, NTW) in (12,12,1), (12,24,2), (12,24,1), (24,24,2),
(48,48,1): the kernel's staging loop writes every float of the LDS request exactly once and from the right wpk element,
every (k-step, position, g, n, nt) is read at a distinct offset inside the request, and every read offset fits a 16-bit
immediate and is 8-byte aligned; the row-major form of the producer builds names the same elements."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(12, 12, 1), (12, 24, 2), (12, 24, 1), (24, 24, 2), (48, 48, 1)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("wino_lds_weight_layout") / "wino_lds_weight_layout_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "wino_lds_weight_layout_harness.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


def test_dense_layout_is_written_once_and_read_once_under_sanitizers(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-3000:]
    # every operand of every lane and n-tile group was compared, in the dense and in the row-major form
    expected = 0
    for cin, cout, ntw in CASES:
        groups = ((cout + 15) // 16 + ntw - 1) // ntw
        expected += 2 * groups * 64 * (cin // 4) * 16 * ntw
    assert int(res.stdout.strip()) == expected
