"""The shortcut's data gradient on the merged quadratic tail by a kernel of its own (csrc/cin_shortdx.h: cin_shortcut_dx_kernel, selected by
cin_shortdx_used in csrc/cin.hip):   dX[m,f] = dP_2[m] * sum_h x1[m,h] wsum_2[h,f],   into the same dxT [M][F] as cin_last_bwd2_kernel's phase u.

Reference, bar and inputs are those of tests/test_cin_ghat_gpu.py: oracle/graph.py:cin under autograd in float64, 1e-5 norm-relative
(tests/test_gpu_parity.py's bar) on the output and on every gradient, x scaled by 10, biases of size 0.1; mode bit 64 (FIL_CIN_TAIL_ALWAYS)
brings these small batches onto the merged quadratic tail.  dx is what the kernel feeds; everything else shows that nothing else moved.
Each case asserts through fil_cin_shortdx_used that the new kernel is what ran.  FIL_CIN_SHORTDX=0 (the parent's kernel) is a knob read once
per process: the last test runs the same cases under it in a fresh child, where the same predicate must say that the old kernel ran."""
import os
import subprocess
import sys

import pytest

from tests.test_cin_ghat_gpu import TAIL_ALWAYS, compare, make_case, oracle, run

pytestmark = pytest.mark.gpu
NOQMERGE = 512                             # fil.h FIL_CIN_NOQMERGE

# each shape is the smallest at which one part of the kernel can go wrong (a wave is 32 rows of M = B K, a workgroup 128; fields are tiled
# 16 wide, the reduction over H_1 runs in two halves of 64, four k-groups of 16 each)
SHAPES = [
    (2, 39, 16, [128, 128, 128]),          # one wave
    (3, 39, 16, [128, 64, 32]),            # 48 rows: rows past M inside a wave
    (9, 39, 16, [100, 128, 128]),          # H_1 not a multiple of 64: zero columns of x1, zero rows of the operand image
    (8, 13, 8, [30, 16, 8]),               # H_1 not a multiple of 4 (and <= 64: an all-zero second half); F < 16: one field tile
    (4, 32, 16, [64, 64, 64]),             # F = 32: two full field tiles
    (4, 33, 16, [64, 64, 64]),             # F = 33: one field in the last tile
    (4, 39, 32, [128, 128, 128]),          # K = 32: a wave is one sample
    (16, 7, 4, [64, 32, 16]),              # K = 4: eight samples per wave
    (10, 39, 16, [128, 64, 32]),           # B K = 160 = 128 + 32: a workgroup with one live wave behind a full one
]
IDS = ["B%d-F%d-K%d-H%s" % (s[0], s[1], s[2], "x".join(map(str, s[3]))) for s in SHAPES]
KNOB_ON = os.environ.get("FIL_CIN_SHORTDX", "1") != "0"     # (the library reads it the same way, once)

ORACLES = {}      # shape index -> the float64 reference, computed once


def reference(i):
    if i not in ORACLES:
        ORACLES[i] = oracle(make_case(SHAPES[i]))
    return ORACLES[i]


def new_kernel_runs(shape, output_dim=1, mode=TAIL_ALWAYS):
    from ml_function_amd import functional as Fn
    B, F, K, H = shape
    return Fn.cin_shortdx_used(B, F, K, H, output_dim=output_dim, mode=mode)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_against_the_graph_oracle(i):
    assert new_kernel_runs(SHAPES[i]) is KNOB_ON, "FIL_CIN_SHORTDX=%s" % os.environ.get("FIL_CIN_SHORTDX")
    compare("shortdx", run(make_case(SHAPES[i]), TAIL_ALWAYS), reference(i))


def test_where_the_old_kernel_stays():
    """No Dense(1) head to fold (R saved as it was), or the two-launch tail: cin_last_bwd2_kernel / cin_bwd_qtail, as before; no rows: nothing."""
    shape = SHAPES[0]
    assert not new_kernel_runs(shape, output_dim=2)
    assert not new_kernel_runs(shape, mode=TAIL_ALWAYS | NOQMERGE)
    assert not new_kernel_runs(shape, mode=0)                         # a small batch stays on the fused tail
    assert not new_kernel_runs((0,) + shape[1:])
    assert new_kernel_runs((4096, 39, 16, [128, 128, 128]), mode=0) is KNOB_ON     # the benchmark's call


def test_oracle_cases_on_the_parent_kernel():
    """FIL_CIN_SHORTDX=0 in a fresh child (started before it touches the GPU): the same shapes through cin_last_bwd2_kernel's phase u."""
    env = dict(os.environ)
    env["FIL_CIN_SHORTDX"] = "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_cin_shortdx_gpu.py", "-x", "-q", "-m", "gpu", "-k", "against_the_graph_oracle",
                        "-p", "no:cacheprovider"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "FIL_CIN_SHORTDX=0:\n%s" % tail
    assert "%d passed" % len(SHAPES) in r.stdout, tail
