"""Host-only checks of the Keras Adagrad and Ftrl (include/fil.h O2, ml_function_amd/optim.py): the new entry points in the header,
the binding and the library; their argument validation through ctypes, in-process and under the ASan/UBSan build; the Python
surface that needs no GPU (Keras' names, defaults and ValueErrors); and the float64 restatement of the rules the GPU tests use."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ml_function_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_rowopt_multi", "fil_embed_rowopt_runs", "fil_embed_rowopt_sweep", "fil_embed_rowopt_merged")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# float64 restatement of TF 2.1's functors (the GPU tests hold their own copy; this one is checked against itself below)
def adagrad64(p, g, acc, lr, eps):
    acc = acc + g * g
    return p - g * lr / (np.sqrt(acc) + eps), acc


def ftrl64(p, g, n, z, lr, lr_power=-0.5, l1=0.0, l2=0.0, shrinkage=0.0):
    gs = g + 2 * shrinkage * p if shrinkage > 0 else g
    n1 = n + g * g
    a = (lambda x: np.sqrt(x)) if lr_power == -0.5 else (lambda x: np.power(x, -lr_power))
    z = z + gs - (a(n1) - a(n)) / lr * p
    q = a(n1) / lr + 2 * l2
    p = np.where(np.abs(z) > l1, (np.sign(z) * l1 - z) / q, 0.0)
    return p, n1, z


def test_rowwise_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.FIL_OPT_ADAGRAD, _lib.FIL_OPT_FTRL) == (1, 2)
    assert ctypes.sizeof(_lib.RowoptHyper) == 24
    assert [f for f, _ in _lib.RowoptHyper._fields_] == ["lr", "epsilon", "lr_power", "l1", "l2", "l2_shrinkage"]


def test_rowwise_entry_points_validate(lib):
    from tests import host_calls_optim_rowwise
    assert host_calls_optim_rowwise.run(lib) >= 80


def test_rowwise_entry_points_under_asan_ubsan():
    """host_calls_optim_rowwise.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_optim_rowwise.py"), asan_lib], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "optim rowwise host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_adagrad_keras_names_defaults_and_errors():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adagrad([p])
    assert isinstance(opt, torch.optim.Optimizer)
    d = opt.defaults
    assert (d["learning_rate"], d["initial_accumulator_value"], d["epsilon"]) == (1e-3, 0.1, 1e-7)
    assert opt.iterations == 0 and opt.force_exchange is False and opt.process_group is None
    assert optim.Adagrad([p], epsilon=None).defaults["epsilon"] == 1e-7         # Keras: backend.epsilon()
    optim.Adagrad([p], initial_accumulator_value=0.0)
    with pytest.raises(ValueError, match="initial_accumulator_value"):
        optim.Adagrad([p], initial_accumulator_value=-0.1)
    with pytest.raises(TypeError):
        optim.Adagrad([p], force_exchange=1)


def test_ftrl_keras_names_defaults_and_errors():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    d = optim.Ftrl([p]).defaults
    assert d == dict(learning_rate=1e-3, learning_rate_power=-0.5, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
                     l2_regularization_strength=0.0, l2_shrinkage_regularization_strength=0.0)
    optim.Ftrl([p], learning_rate_power=0.0, initial_accumulator_value=0.0)
    for bad, needle in ((dict(initial_accumulator_value=-1e-3), "initial_accumulator_value"),
                        (dict(learning_rate_power=0.1), "learning_rate_power"),
                        (dict(l1_regularization_strength=-1.0), "l1_regularization_strength"),
                        (dict(l2_regularization_strength=-1.0), "l2_regularization_strength"),
                        (dict(l2_shrinkage_regularization_strength=-1.0), "l2_shrinkage_regularization_strength")):
        with pytest.raises(ValueError, match=needle):
            optim.Ftrl([p], **bad)
    with pytest.raises(TypeError):
        optim.Ftrl([p], beta=0.0)                   # TF 2.1 has no beta


@pytest.mark.parametrize("cls", ["Adagrad", "Ftrl"])
def test_rowwise_refuses_cpu_parameters(cls):
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.FilError, match="GPU"):
        getattr(optim, cls)([p]).step()


def test_float64_rules_are_self_consistent():
    """From p = 0, one Ftrl step with l1 = l2 = shrinkage = 0 and lr_power = -0.5 is one Adagrad step without epsilon:
    -lr g / sqrt(n0 + g^2); and a zero gradient leaves Adagrad's row as it is."""
    rng = np.random.default_rng(0)
    g = rng.standard_normal(1000) * 10.0 ** rng.integers(-6, 1, 1000)
    n0, lr = 0.1, 0.05
    p_f, n_f, z_f = ftrl64(np.zeros(1000), g, np.full(1000, n0), np.zeros(1000), lr)
    p_a, acc = adagrad64(np.zeros(1000), g, np.full(1000, n0), lr, 0.0)
    want = -lr * g / np.sqrt(n0 + g * g)
    np.testing.assert_allclose(p_f, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(p_a, want, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(n_f, acc)
    np.testing.assert_allclose(z_f, g, rtol=0, atol=0)                      # sigma p = 0 from p = 0
    p = rng.standard_normal(1000)
    assert np.array_equal(adagrad64(p, np.zeros(1000), np.full(1000, n0), lr, 1e-7)[0], p)
    # the general power form agrees with the square-root special case at lr_power = -0.5
    n = np.full(1000, n0)
    a = ftrl64(p, g, n, np.zeros(1000), lr, lr_power=-0.5, l1=1e-3, l2=1e-2, shrinkage=1e-2)
    b = ftrl64(p, g, n, np.zeros(1000), lr, lr_power=-0.5000000001, l1=1e-3, l2=1e-2, shrinkage=1e-2)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-6, atol=1e-12)
