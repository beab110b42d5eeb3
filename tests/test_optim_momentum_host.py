"""Host-only checks of the Keras SGD and RMSprop (include/fil.h O4, ml_function_amd/optim.py): the new entry points in the header, the
binding and the library; their argument validation through ctypes, in-process and under the ASan/UBSan build; the Python surface that
needs no GPU (Keras' names, defaults and errors); and the numpy restatement of the rules (tests/keras_sgd_rmsprop_ref.py) against
hand-computed two-step values of each variant and against Keras' row semantics on a tiny table."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from tests import keras_sgd_rmsprop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_momopt_multi", "fil_embed_momopt_runs", "fil_embed_momopt_sweep", "fil_embed_momopt_merged")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_momentum_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        for n in (name, name + "_lrdev"):
            assert n in _lib.header_symbols() and n in _lib.SIGNATURES and hasattr(lib, n), n
        # the O4 entry points take the argument lists of their O2 counterparts
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("momopt", "rowopt")]
        assert _lib.SIGNATURES[name + "_lrdev"] == _lib.SIGNATURES[name.replace("momopt", "rowopt") + "_lrdev"]
    assert (_lib.FIL_OPT_SGD, _lib.FIL_OPT_RMSPROP, _lib.FIL_MOMOPT_NESTEROV) == (3, 4, 1)
    assert ctypes.sizeof(_lib.MomoptHyper) == 24
    assert [f for f, _ in _lib.MomoptHyper._fields_] == ["lr", "epsilon", "rho", "momentum", "flags", "reserved"]
    header = open(_lib.HEADER_PATH).read()
    body = header[header.index("typedef struct {\n  float lr;\n  float epsilon;        /* RMSprop */"):]
    body = body[:body.index("fil_momopt_hyper;")]
    assert body.count("float ") == 4 and body.count("int32_t ") == 2            # 4 floats + 2 int32: 24 bytes
    assert "fil_momopt_hyper;     /* 24 bytes */" in header


def test_abi_version_and_rowopt_hyper_are_unchanged(lib):
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216
    assert ctypes.sizeof(_lib.RowoptHyper) == 24
    assert (_lib.FIL_OPT_ADAGRAD, _lib.FIL_OPT_FTRL) == (1, 2)


def test_momentum_entry_points_validate(lib):
    from tests import host_calls_optim_momentum
    assert host_calls_optim_momentum.run(lib) >= 250


def test_momentum_entry_points_under_asan_ubsan():
    """host_calls_optim_momentum.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_optim_momentum.py"), asan_lib], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "optim momentum host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_sgd_keras_names_defaults_and_errors():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.SGD([p])
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.defaults == dict(learning_rate=0.01, momentum=0.0, nesterov=False)
    assert opt.iterations == 0 and opt.force_exchange is False and opt.process_group is None
    assert opt._SLOTS == () and optim.SGD([p], momentum=0.9)._SLOTS == ("momentum",)
    assert optim.SGD([p], momentum=0.9, nesterov=True).defaults["nesterov"] is True
    optim.SGD([p], momentum=1.0)
    optim.SGD([p], momentum=0)
    for bad in (-0.1, 1.5, 2):
        with pytest.raises(ValueError) as e:
            optim.SGD([p], momentum=bad)
        assert str(e.value) == "`momentum` must be between [0, 1]."
    with pytest.raises(ValueError, match="decay cannot be less than 0"):
        optim.SGD([p], decay=-1.0)
    with pytest.raises(TypeError):
        optim.SGD([p], force_exchange=1)
    with pytest.raises(TypeError):
        optim.SGD([p], lazy_tables=True)            # no lazy or deferred mode
    with pytest.raises(TypeError):
        optim.SGD([p], sweep_period=4)
    assert "fil_embed_run_sum" in optim.SGD.__doc__ and "order" in optim.SGD.__doc__     # the duplicate-id note


def test_rmsprop_keras_names_defaults_and_errors():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.RMSprop([p])
    assert opt.defaults == dict(learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False)
    assert opt._SLOTS == ("rms",) and optim.RMSprop([p], momentum=0.5)._SLOTS == ("rms", "momentum")
    assert optim.RMSprop([p], epsilon=None).defaults["epsilon"] == 1e-7         # Keras: backend.epsilon()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError) as e:
            optim.RMSprop([p], momentum=bad)
        assert str(e.value) == "`momentum` must be between [0, 1]."
    with pytest.raises(NotImplementedError, match="third slot"):
        optim.RMSprop([p], centered=True)
    with pytest.raises(TypeError):
        optim.RMSprop([p], sweep_period=4)


@pytest.mark.parametrize("cls", ["SGD", "RMSprop"])
def test_momentum_optimizers_refuse_cpu_parameters(cls):
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.FilError, match="GPU"):
        getattr(optim, cls)([p]).step()


# ---- the restatement against two steps computed by hand: p0 = 1, g = 0.5 at both steps, lr 0.1, momentum 0.5, rho 0.9, epsilon 0
R1, R2 = 0.1 * 0.25, 0.9 * (0.1 * 0.25) + 0.1 * 0.25                 # rms after steps 1 and 2: 0.025, 0.0475
U1, U2 = 0.1 * 0.5 / math.sqrt(R1), 0.1 * 0.5 / math.sqrt(R2)        # lr g / sqrt(rms): 0.316227766..., 0.229415733...
HAND = dict(
    sgd=[(0.95, None, None), (0.90, None, None)],
    sgd_momentum=[(0.95, -0.05, None), (0.875, -0.075, None)],                          # a2 = -0.05 * 0.5 - 0.05
    sgd_nesterov=[(0.925, -0.05, None), (0.8375, -0.075, None)],                        # p += a * 0.5 - 0.05
    rmsprop=[(1 - U1, R1, None), (1 - U1 - U2, R2, None)],
    rmsprop_momentum=[(1 - U1, R1, U1), (1 - U1 - (0.5 * U1 + U2), R2, 0.5 * U1 + U2)],
)


# the hand values use the decimals 0.1, 0.5, 0.9; the restatement Keras' float32 hyper-parameters: float32(0.9) is 2.6e-8 off, so its
# 1 - rho is 2.4e-7 off (relative), float32(0.1) 1.5e-8; a dozen fp32 roundings of 6e-8 each come on top
RTOL = 2e-6


@pytest.mark.parametrize("touched", [False, True], ids=["dense", "touched"])
@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_restatement_matches_hand_computed_two_steps(variant, touched):
    assert abs(HAND["rmsprop"][1][0] - 0.4543565) < 1e-6 and abs(HAND["rmsprop_momentum"][1][0] - 0.2962426) < 1e-6   # the decimals
    h = ref.hyper(variant, lr=0.1, momentum=0.5, rho=0.9, epsilon=0.0)
    n = ref.N_SLOTS[variant]
    p, g = np.ones(5, F), np.full(5, 0.5, F)
    s = np.zeros(5, F) if n >= 1 else None
    z = np.zeros(5, F) if n >= 2 else None
    for want in HAND[variant]:
        p, s, z = ref.elem(h, p, s, z, g, touched)
        for got, w in zip((p, s, z), want):
            assert (got is None) == (w is None)
            if w is not None:
                assert got.dtype == np.float32
                np.testing.assert_allclose(got, w, rtol=RTOL, atol=0)
    p64 = ref.elem64(h, 1.0, 0.0, 0.0, 0.5, touched)
    p64 = ref.elem64(h, p64[0], p64[1], p64[2], 0.5, touched)
    np.testing.assert_allclose(p64[0], HAND[variant][1][0], rtol=RTOL)


def test_restatement_rms_forms_of_the_fused_variant_differ_in_rounding():
    """ApplyRMSProp's rms += (g g - rms)(1 - rho) and SparseApplyRMSProp's rms rho + g g (1 - rho) are different fp32 computations;
    the Python form's two orders (momentum == 0) are not."""
    rng = np.random.default_rng(0)
    p, s, z, g = (rng.standard_normal(4096).astype(F) for _ in range(4))
    s = np.abs(s)
    h = ref.hyper("rmsprop_momentum", lr=1e-3)
    assert not np.array_equal(ref.elem(h, p, s, z, g, True)[1], ref.elem(h, p, s, z, g, False)[1])
    h = ref.hyper("rmsprop", lr=1e-3)
    a, b = ref.elem(h, p, s, None, g, True), ref.elem(h, p, s, None, g, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_restatement_moves_the_rows_keras_moves(variant):
    """A table of four fields of 3 rows: regularised, unregularised, frozen, regularised; one touched row in each."""
    V, K = 12, 4
    rng = np.random.default_rng(1)
    n = ref.N_SLOTS[variant]
    p = rng.standard_normal((V, K)).astype(F)
    s = np.abs(rng.standard_normal((V, K))).astype(F) if n >= 1 else None
    z = rng.standard_normal((V, K)).astype(F) if n >= 2 else None
    row_l2 = np.repeat(np.array([1e-2, 0, 0, 3e-3], F), 3)
    frozen = np.repeat(np.array([False, False, True, False]), 3)
    touched = np.zeros(V, bool)
    touched[[1, 4, 7, 10]] = True                   # (row 7 is frozen: a real record never holds it; the restatement ignores it)
    G = rng.standard_normal((V, K)).astype(F)
    h = ref.hyper(variant, lr=1e-2)
    (p1, s1, z1), moved, decayed = ref.table_step(h, p, s, z, G, touched, row_l2, frozen)
    assert moved.tolist() == [True] * 3 + [False, True, False] + [False] * 3 + [True] * 3
    assert decayed.tolist() == ([False] * 3 + [True, False, True] + [False] * 6 if variant == "rmsprop" else [False] * V)
    assert (p1[moved] != p[moved]).all() and np.array_equal(p1[~moved], p[~moved])
    if z is not None:
        assert np.array_equal(z1[~moved], z[~moved])
    if s is not None:
        keep = ~moved & ~decayed
        assert np.array_equal(s1[keep], s[keep])
        assert np.array_equal(s1[decayed], s[decayed] * h["rho"])
    # a touched row of the unregularised field: the touched form on the run sum alone
    want = ref.elem(h, p[4], None if s is None else s[4], None if z is None else z[4], G[4], True)
    assert np.array_equal(p1[4], want[0])
    # an untouched row of a regularised field: the dense form on 2 l2 p
    want = ref.elem(h, p[0], None if s is None else s[0], None if z is None else z[0], (F(2) * F(1e-2)) * p[0], False)
    assert np.array_equal(p1[0], want[0])
