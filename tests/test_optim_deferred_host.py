"""Host-only checks of deferred Keras mode (optim.Adam(sweep_period=N), include/fil.h O1): the new entry points' argument validation
through ctypes, in-process and under the ASan/UBSan build, and the Python surface that needs no GPU."""
import os
import subprocess
import sys

import pytest
import torch

from ml_function_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_embed_adam_ring_len", "fil_embed_adam_catchup_runs", "fil_embed_adam_runs_deferred", "fil_embed_adam_merged_deferred",
       "fil_embed_adam_roll")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_deferred_entry_points_are_exported(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.header_abi_version() == 216


def test_deferred_entry_points_validate(lib):
    from tests import host_calls_optim_deferred
    assert host_calls_optim_deferred.run(lib) >= 60


def test_deferred_entry_points_under_asan_ubsan():
    """host_calls_optim_deferred.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_optim_deferred.py"), asan_lib], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "optim deferred host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_sweep_period_is_validated():
    p = torch.nn.Parameter(torch.zeros(3))
    assert optim.Adam([p]).sweep_period is None
    assert optim.Adam([p], sweep_period=8).sweep_period == 8
    assert optim.Adam([p], sweep_period=optim.MAX_SWEEP_PERIOD).sweep_period == optim.MAX_SWEEP_PERIOD
    for bad in (2.0, "8", True, [4]):
        with pytest.raises(TypeError, match="sweep_period"):
            optim.Adam([p], sweep_period=bad)
    for bad in (0, -1, optim.MAX_SWEEP_PERIOD + 1):
        with pytest.raises(ValueError, match="sweep_period"):
            optim.Adam([p], sweep_period=bad)
    with pytest.raises(ValueError, match="lazy_tables"):
        optim.Adam([p], sweep_period=4, lazy_tables=True)


def test_deferred_mode_refuses_a_cpu_table():
    """A runs table joins deferred mode at construction: a CPU one raises there (there is no CPU path)."""
    p = torch.nn.Parameter(torch.zeros(10, 4))
    p._fil_runs_table = True
    with pytest.raises(_lib.FilError, match="deferred table"):
        optim.Adam([p], sweep_period=4)
    assert optim.deferred_optimizer(p) is None
    optim.Adam([p])          # Keras mode attaches nothing
    assert optim.deferred_optimizer(p) is None


def test_flush_without_deferred_tables_is_a_no_op():
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adam([p], sweep_period=3)
    opt.flush()
    assert opt._defer == {}


def test_train_ctr_accepts_sweep_period():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ctr.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--sweep-period" in r.stdout, r.stderr[-2000:]
