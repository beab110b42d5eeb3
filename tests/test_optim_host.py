"""Host-only checks of the Keras Adam (include/fil.h O1, ml_function_amd/optim.py): the entry points' argument validation through
ctypes, in-process and under the ASan/UBSan build, and the Python surface that needs no GPU."""
import os
import subprocess
import sys

import pytest
import torch

from ml_function_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_adam_entry_points_are_exported(lib):
    for name in ("fil_adam_multi", "fil_embed_adam_runs", "fil_embed_adam_sweep"):
        assert name in _lib.header_symbols() and hasattr(lib, name)


def test_adam_entry_points_validate(lib):
    from tests import host_calls_optim
    assert host_calls_optim.run(lib) >= 30


def test_adam_entry_points_under_asan_ubsan():
    """host_calls_optim.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_optim.py"), asan_lib], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "optim host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_descriptor_layout_matches_the_header():
    from ml_function_amd import optim
    import ctypes
    assert ctypes.sizeof(optim._Desc) == 48
    assert [f for f, _ in optim._Desc._fields_] == ["param", "grad", "m", "v", "numel", "l2", "reserved"]


def test_adam_keras_names_and_defaults():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adam([p])
    d = opt.defaults
    assert (d["learning_rate"], d["beta_1"], d["beta_2"], d["epsilon"]) == (1e-3, 0.9, 0.999, 1e-7)
    assert opt.lazy_tables is False and opt.iterations == 0
    for bad in (dict(learning_rate=-1.0), dict(beta_1=1.0), dict(beta_2=-0.1), dict(epsilon=-1e-7)):
        with pytest.raises(ValueError):
            optim.Adam([p], **bad)


def test_adam_refuses_cpu_parameters():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.FilError, match="GPU"):
        optim.Adam([p]).step()


def test_grad_mode_is_checked():
    from ml_function_amd import models
    from ml_function_amd.layers import SparseEmbed
    info = models.make_sparse_info([5, 7], embed_dim=4)
    assert SparseEmbed(info).grad_mode == "dense"
    assert SparseEmbed(info, grad_mode="runs").grad_mode == "runs"
    with pytest.raises(ValueError):
        SparseEmbed(info, grad_mode="sparse")
    with pytest.raises(ValueError):
        SparseEmbed(info, grad_mode="runs", sparse_grad=True)
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, tableGrad="runs")
    assert fi.sparse_embed.grad_mode == fi.linear_embed.grad_mode == "runs"
    assert models.FeatureInput(sparseInfo=info, useLinear=True).sparse_embed.grad_mode == "dense"
