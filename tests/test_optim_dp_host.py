"""Host-only checks of the data-parallel runs exchange (include/fil.h O1, ml_function_amd/optim.py, dp.exchange_runs): the entry
points' argument validation through ctypes, in-process and under the ASan/UBSan build, and the Python surface that needs no GPU."""
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist

from ml_function_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_embed_runs_compact_workspace_bytes", "fil_embed_runs_compact", "fil_embed_adam_merged")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_dp_entry_points_are_exported(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.header_abi_version() == 216


def test_dp_entry_points_validate(lib):
    from tests import host_calls_optim_dp
    assert host_calls_optim_dp.run(lib) >= 30


def test_dp_entry_points_under_asan_ubsan():
    """host_calls_optim_dp.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_optim_dp.py"), asan_lib], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "optim dp host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_adam_accepts_process_group_and_force_exchange():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adam([p])
    assert opt.process_group is None and opt.force_exchange is False
    assert optim.Adam([p], force_exchange=True).force_exchange is True
    assert optim.Adam([p], process_group=None, force_exchange=False).process_group is None
    for bad in ("world", 2, object()):
        with pytest.raises(TypeError, match="process_group"):
            optim.Adam([p], process_group=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="force_exchange"):
            optim.Adam([p], force_exchange=bad)


def test_exchange_world_without_a_process_group():
    """No initialised torch.distributed: the one-GPU path (0) unless force_exchange (world 1)."""
    from ml_function_amd import optim
    assert not dist.is_initialized()
    p = torch.nn.Parameter(torch.zeros(3))
    assert optim.Adam([p])._exchange_world() == 0
    assert optim.Adam([p], force_exchange=True)._exchange_world() == 1


def test_exchange_runs_is_documented_beside_exchange_sparse_rows():
    from ml_function_amd import dp
    assert callable(dp.exchange_runs) and "exchange_sparse_rows" in dp.exchange_runs.__doc__
