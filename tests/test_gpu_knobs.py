"""The launch-merging knobs of the CIN path (FIL_CIN_{HEADFOLD,FWDQ,DZ2,QMERGE,QTAIL}=0 select the older, un-merged launch sequences)
are read ONCE when the library is first used, so each setting needs a process of its own: every knob gets a fresh child that runs
the mode-64 column of test_cin_fused_tail (the merged quadratic tail forced at every tail shape, 19 cases against the fp64 closed
forms) with that knob off.  The fallbacks therefore stay part of what `pytest -m gpu` proves, not of a script somebody has to
remember to run (tools/gpu_knobs.sh runs the full 200-case subset).  The child is started before it touches the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["FIL_CIN_DWFOLD4", "FIL_CIN_PACKFOLD", "FIL_CIN_HEADFOLD", "FIL_CIN_FWDQ", "FIL_CIN_DZ2", "FIL_CIN_QMERGE", "FIL_CIN_QTAIL"])
def test_cin_parity_subset_with_one_knob_off(knob):
    env = dict(os.environ)
    env[knob] = "0"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py::test_cin_fused_tail", "-x", "-q", "-m", "gpu", "-k", "1-64-",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "%s=0:\n%s" % (knob, tail)
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["FIL_ATTN_KREG", "FIL_ATTN_DX_LDS"])
def test_attn_parity_subset_with_one_knob_off(knob):
    """The attention kernels' forms behind knobs: FIL_ATTN_KREG=0 = the forward with its k image in LDS at the shapes whose k fragments
    fit registers (up to 13 key tiles, f16 mode), FIL_ATTN_DX_LDS=0 = the backward's dx part through global memory (second visit).
    A fresh child runs the two-waves-per-head shapes (F = 170..300, both precisions) against the closed forms."""
    env = dict(os.environ)
    env[knob] = "0"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py::test_attn_two_waves_per_head", "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "%s=0:\n%s" % (knob, tail)
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.gpu
def test_attn_two_waves_per_head_forced_on_fewer_heads():
    """FIL_ATTN_WPH=2 forces the two-waves-per-head backward wherever there are more than 8 query blocks: test_attn_fused's
    (2, 230, 16, 2, 16) then runs it with TWO heads (wave w = head w mod 2, sub w / 2), fp32 -- the strict bar -- with and without the
    residual / LayerNorm branches; the shapes with up to 8 blocks keep one wave per head."""
    env = dict(os.environ)
    env["FIL_ATTN_WPH"] = "2"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py::test_attn_fused", "-x", "-q", "-m", "gpu", "-k", "230 or 200",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "FIL_ATTN_WPH=2:\n%s" % tail
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.gpu
@pytest.mark.parametrize("knob,value", [("FIL_ATTN_WPH", "2"), ("FIL_ATTN_DX_LDS", "0"), ("FIL_ATTN_KREG", "0")])
def test_attn_edges_with_one_knob(knob, value):
    """The constructed shape cases of tests/test_attn_edges_gpu.py with F >= 129 (the `big` ids: NB = 13 and 32, where the knobs act) in a fresh
    child per knob: FIL_ATTN_WPH=2 = two waves per head wherever it fits, FIL_ATTN_DX_LDS=0 = the dx part through global memory everywhere,
    FIL_ATTN_KREG=0 = the f16 forward's k image in LDS up to 13 key tiles.  Every case asserts fil_attn_plan == the restatement of
    tests/attn_edge_cases.py inside the child, and both read the knob, so the instantiation asserted follows it; the refused pairs stay refused."""
    env = dict(os.environ)
    env[knob] = value
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_attn_edges_gpu.py", "-x", "-q", "-m", "gpu", "-k",
                        "(shape_edges or refuses) and big", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "%s=%s:\n%s" % (knob, value, tail)
    assert "25 passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.gpu
def test_gemm_edges_with_one_wave_per_tile():
    """FIL_GEMM_KW=1 (read once per process) launches the dense GEMM with ONE wave per output tile -- the eight
    gemm_f32_kernel<*, *, *, 1> instantiations, no join of k halves through LDS.  A fresh child runs the constructed-edge cases of
    tests/test_dense_edges_gpu.py under it, bit for bit against the int64 products: all of the BN = 64 group and of the split-k group
    (every transposition), and the `kw1` slice of the BN = 32 group."""
    env = dict(os.environ)
    env["FIL_GEMM_KW"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_dense_edges_gpu.py", "-x", "-q", "-m", "gpu",
                        "-k", "gemm_bn64 or gemm_splitk or kw1", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "FIL_GEMM_KW=1:\n%s" % tail
    assert "44 passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.gpu
def test_dcn_edges_with_a_two_workgroup_grid():
    """FIL_DCN_GRID=2 (read once per process) caps the register-resident DCN kernels at two workgroups: 8 forward and 16 backward waves.
    A fresh child runs three groups of tests/test_dcn_edges_gpu.py under it.  The `walk` cases -- every menu shape with a
    register-resident direction at B = 37 -- are the ones where every forward wave loops (5 or 4 samples) and every backward wave walks
    3 or 2 samples through its prefetch chain, at every menu instantiation; they assert those trip counts when the grid is forced.  The
    grid cases with B <= 257 (`le257`) walk up to 17 samples per wave at <8, 4, 2> with one or two partials to reduce.  The path / menu
    cases (B <= 9) stay at one sample per wave: they show that the forced grid changes no result.  The cases size the workspace with the
    same override (tests/dcn_edge_cases.py reads the variable), so the child also proves that the library saw it."""
    env = dict(os.environ)
    env["FIL_DCN_GRID"] = "2"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_dcn_edges_gpu.py", "-x", "-q", "-m", "gpu",
                        "-k", "path_and_menu or le257 or walk", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "FIL_DCN_GRID=2:\n%s" % tail
    assert "47 passed" in r.stdout and "no tests ran" not in r.stdout, tail
