"""CPU: where conv3x3_winog keeps its transformed weights in LDS (csrc/wino_weight_layout.h: the dense
[k-step][position][g][n][nt] form of the NT = 2 builds and the row-major form of the others), built for the host with
AddressSanitizer + UBSan (tests/wino_weight_layout_harness.cpp).  For every instantiated (C_in, NT, padded C_out) the
staging map is one-to-one into the LDS size the launcher requests (onto it in the dense form), and every lane's read
offset for operand q - the window into the next channel block and the remainder k-step of C_in = 12 included - names the
weight element that the row-major w_lane[wq_off(q)] named before the header existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (C_in, C_out, NT) of g_winog in conv_wino_kernels.hip
CASES = [(12, 12, 1), (12, 24, 2), (24, 24, 2), (24, 48, 3), (48, 48, 3), (48, 96, 3), (96, 96, 1), (24, 12, 1),
         (48, 24, 2), (96, 48, 1)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("wino_weight_layout") / "wino_weight_layout_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "wino_weight_layout_harness.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


def test_weight_layout_is_one_to_one_and_names_the_old_elements_under_sanitizers(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-3000:]
    # every operand read of every lane, block and n-tile group was compared: per block its 32 NT operands (16 NT in the
    # remainder k-step) and, where another block follows, the 4 NT of the window
    expected = 0
    for cin, cout, nt in CASES:
        groups = ((cout + 15) // 16 + nt - 1) // nt
        blocks = [32 * nt] * (cin // 8) + ([16 * nt] if cin % 8 else [])
        expected += groups * 64 * (sum(blocks) + 4 * nt * (len(blocks) - 1))
    assert int(res.stdout.strip()) == expected
