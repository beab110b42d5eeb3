"""Host-only checks of Keras' Adam(amsgrad=True) (include/fil.h O7, ml_function_amd/optim.py): the new entry points in the header, the
binding and the library; the five-array descriptor; the argument checks that return before any launch, through ctypes (no GPU is
touched: every call here either fails a check or has nothing to do); the Python surface that needs no GPU; and the float64
restatement (tests/keras_amsgrad_ref.py) on the inputs the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from tests import keras_amsgrad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_amsgrad_multi", "fil_embed_amsgrad_runs", "fil_embed_amsgrad_sweep", "fil_embed_amsgrad_merged")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
X = 0x1000                  # a non-NULL pointer nothing dereferences: every call below returns before a launch
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_amsgrad_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
        # one entry point each, with (lr, lr_dev): no _lrdev twins
        assert name + "_lrdev" not in _lib.SIGNATURES and name + "_lrdev" not in _lib.header_symbols()
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    header = open(_lib.HEADER_PATH).read()
    assert header.index(" * O6 ") < header.index(" * O7 ") < header.index("int fil_amsgrad_multi(") < header.index(" * M1 ")
    assert "lr_dev != NULL" in header[header.index(" * O7 "):header.index(" * M1 ")]       # fil.h says which form was picked
    # O1's Keras-mode lists with vhat and lr_dev added and the mode dropped
    for kind in ("runs", "merged"):
        assert len(_lib.SIGNATURES["fil_embed_amsgrad_" + kind][1]) == len(_lib.SIGNATURES["fil_embed_adam_" + kind][1]) + 1
    for new, old in (("fil_embed_amsgrad_sweep", "fil_embed_adam_sweep"), ("fil_amsgrad_multi", "fil_adam_multi")):
        assert len(_lib.SIGNATURES[new][1]) == len(_lib.SIGNATURES[old][1]) + (2 if "sweep" in new else 1)


def test_abi_version_and_adams_descriptor_are_unchanged(lib):
    from ml_function_amd import optim
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216
    assert ctypes.sizeof(optim._Desc) == 48
    assert [n for n, _ in optim._Desc._fields_] == ["param", "grad", "m", "v", "numel", "l2", "reserved"]


def test_amsgrad_descriptor_matches_the_header():
    D = _lib.AmsgradTensor
    assert ctypes.sizeof(D) == 56
    assert [n for n, _ in D._fields_] == ["param", "grad", "m", "v", "vhat", "numel", "l2", "reserved"]
    assert [t for _, t in D._fields_] == [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_float, ctypes.c_int32]
    assert (D.vhat.offset, D.numel.offset, D.l2.offset, D.reserved.offset) == (32, 40, 48, 52)
    header = open(_lib.HEADER_PATH).read()
    body = header[:header.index("} fil_amsgrad_tensor;")]
    body = body[body.rindex("typedef struct {"):]
    assert re.findall(r"^\s*((?:const )?float\*?|int64_t|int32_t) (\w+);", body, flags=re.M) == [
        ("float*", "param"), ("const float*", "grad"), ("float*", "m"), ("float*", "v"), ("float*", "vhat"), ("int64_t", "numel"),
        ("float", "l2"), ("int32_t", "reserved")]
    assert "fil_amsgrad_tensor;  /* 56 bytes */" in header


def _runs(lib, R=5, K=4, g_dtype=0, F=3, table=X, m=X, v=X, vhat=X, stamp=X, step=X, lr=1e-3, lr_dev=None, b1=0.9, b2=0.5, eps=1e-7):
    return lib.fil_embed_amsgrad_runs(X, X, X, R, K, g_dtype, F, None, table, m, v, vhat, stamp, step, lr, lr_dev, b1, b2, eps, None)


def _sweep(lib, V=5, K=4, F=3, table=X, m=X, v=X, vhat=X, stamp=X, step=X, lr=1e-3, lr_dev=None, b1=0.9, b2=0.5, eps=1e-7):
    return lib.fil_embed_amsgrad_sweep(table, m, v, vhat, stamp, V, K, X, None, None, F, step, lr, lr_dev, b1, b2, eps, None)


def _merged(lib, W=1, cap=5, K=4, F=3, V=5, table=X, m=X, v=X, vhat=X, stamp=X, step=X, lr=1e-3, lr_dev=None, b1=0.9, b2=0.5,
            eps=1e-7):
    return lib.fil_embed_amsgrad_merged(X, X, X, W, cap, K, X, None, F, table, m, v, vhat, stamp, V, step, lr, lr_dev, b1, b2, eps, None)


def _multi(lib, tensors=X, n=0, numel=0, step=X, lr=1e-3, lr_dev=None, b1=0.9, b2=0.5, eps=1e-7, advance=0):
    return lib.fil_amsgrad_multi(tensors, n, numel, step, lr, lr_dev, b1, b2, eps, advance, None)


def test_null_slots_are_reported_before_any_launch(lib):
    for call in (_runs, _sweep, _merged):
        for slot in ("table", "m", "v", "vhat", "stamp", "step"):
            assert call(lib, **{slot: None}) == ERR_ARG, (call.__name__, slot)
            assert slot in lib.fil_last_error().decode(), (call.__name__, slot)
    assert _multi(lib, step=None) == ERR_ARG
    assert _multi(lib, tensors=None, n=1, numel=4) == ERR_ARG


def test_nothing_to_do_succeeds_before_any_pointer_is_looked_at(lib):
    assert _runs(lib, R=0, table=None, m=None, v=None, vhat=None, stamp=None, step=None) == OK
    assert _sweep(lib, V=0, table=None, vhat=None) == OK
    assert _merged(lib, cap=0, vhat=None) == OK and _merged(lib, V=0, vhat=None) == OK
    assert _multi(lib, tensors=None, n=0) == OK                     # n = 0 without advance: no launch at all


@pytest.mark.parametrize("call,idle", [(_runs, dict(R=0)), (_sweep, dict(V=0)), (_merged, dict(cap=0)), (_multi, dict(n=0))],
                         ids=["runs", "sweep", "merged", "multi"])
def test_hyper_parameter_checks_are_adams(lib, call, idle):
    """lr, epsilon >= 0 and betas in [0, 1), a NaN refused; checked before the early return.  With a device rate the by-value lr is
    ignored, whatever it holds."""
    assert call(lib, **idle) == OK
    assert call(lib, lr=0.0, b1=0.0, b2=0.0, eps=0.0, **idle) == OK
    for bad in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.5), dict(eps=-1e-7), dict(lr=-1.0), dict(b1=NAN), dict(b2=NAN),
                dict(eps=NAN), dict(lr=NAN)):
        assert call(lib, **bad, **idle) == ERR_ARG, bad
        assert "hyper-parameters" in lib.fil_last_error().decode()
    assert call(lib, lr=-1.0, lr_dev=X, **idle) == OK and call(lib, lr=NAN, lr_dev=X, **idle) == OK
    assert call(lib, lr_dev=X, b2=1.0, **idle) == ERR_ARG


def test_shape_limits_and_flags(lib):
    assert _runs(lib, K=257) == ERR_UNSUPPORTED and _merged(lib, K=257) == ERR_UNSUPPORTED
    assert _sweep(lib, F=1025) == ERR_UNSUPPORTED and _merged(lib, F=1025) == ERR_UNSUPPORTED
    assert _runs(lib, K=256, R=0) == OK and _sweep(lib, F=1024, V=0) == OK
    assert _runs(lib, K=0) == ERR_ARG and _runs(lib, R=-1) == ERR_ARG and _runs(lib, g_dtype=2) == ERR_ARG and _runs(lib, F=0) == ERR_ARG
    assert _sweep(lib, V=-1) == ERR_ARG and _merged(lib, W=0) == ERR_ARG and _merged(lib, cap=-1) == ERR_ARG
    assert _multi(lib, advance=2) == ERR_ARG and _multi(lib, n=-1) == ERR_ARG and _multi(lib, numel=-1) == ERR_ARG


def test_adam_keyword_defaults_slots_and_exclusions():
    from ml_function_amd import optim, schedules
    p = torch.nn.Parameter(torch.zeros(3))
    plain, ams = optim.Adam([p]), optim.Adam([p], amsgrad=True)
    want = dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7)         # Keras' defaults; amsgrad is no group default
    assert plain.defaults == ams.defaults == want
    assert plain.amsgrad is False and ams.amsgrad is True
    assert plain._SLOTS == optim.Adam._SLOTS == ("m", "v") and ams._SLOTS == ("m", "v", "vhat") == ref.SLOT_NAMES
    assert plain._slot_init(None) == (0.0, 0.0) and ams._slot_init(None) == (0.0, 0.0, 0.0)
    import inspect
    assert list(inspect.signature(optim.Adam.__init__).parameters)[-1] == "amsgrad"
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(TypeError, match="amsgrad"):
            optim.Adam([p], amsgrad=bad)
    with pytest.raises(ValueError, match="sweep_period"):
        optim.Adam([p], amsgrad=True, sweep_period=4)
    with pytest.raises(ValueError, match="lazy_tables"):
        optim.Adam([p], amsgrad=True, lazy_tables=True)
    optim.Adam([p], amsgrad=False, sweep_period=4)
    optim.Adam([p], amsgrad=False, lazy_tables=True)
    # schedules and decay= are accepted
    optim.Adam([p], amsgrad=True, learning_rate=schedules.ExponentialDecay(1e-2, decay_steps=2, decay_rate=0.5), decay=0.5)
    assert "amsgrad" in optim.__doc__


def test_state_dict_flag_only_when_on():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    plain, ams = optim.Adam([p]), optim.Adam([p], amsgrad=True)
    sd = plain.state_dict()
    assert "amsgrad" not in sd and set(sd) == {"state", "param_groups", "iterations"}
    assert ams.state_dict()["amsgrad"] is True
    with pytest.raises(_lib.FilError, match="amsgrad"):
        plain.load_state_dict(ams.state_dict())
    with pytest.raises(_lib.FilError, match="amsgrad"):
        ams.load_state_dict(plain.state_dict())
    sd = ams.state_dict()
    sd["state"] = {0: {"m": torch.zeros(3), "v": torch.zeros(3)}}
    with pytest.raises(_lib.FilError, match="vhat"):
        ams.load_state_dict(sd)
    plain.load_state_dict(plain.state_dict())
    ams.load_state_dict(ams.state_dict())


def test_amsgrad_refuses_cpu_parameters():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.FilError, match="GPU"):
        optim.Adam([p], amsgrad=True).step()


def test_reference_inputs_separate_the_rule_from_plain_adam():
    """The GPU tests' dense inputs on the float64 reference alone: vhat > v on at least half of the elements after steps 2 and 5, and
    the update of a rule that ignores vhat is far outside every bar from step 2 on.  (beta_2 = 0.5; with Keras' 0.999 the difference
    would be of the order of the bars.)"""
    h = ref.hyper()
    rng = np.random.default_rng(0)
    p = rng.standard_normal(4096) * 0.5
    m, v, vhat = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    share, dist = [], []
    for t, s in enumerate(ref.SCALES, 1):
        g = rng.standard_normal(p.shape) * s
        wrong = ref.adam64(h, p, g, m, v, t)[0]
        q, m, v, vhat = ref.amsgrad64(h, p, g, m, v, vhat, t)
        share.append(float((vhat > v).mean()))
        dist.append(ref.nrel(wrong - p, q - p))
        p = q
    print("share of vhat > v:", share, "distance of plain Adam's update:", dist)
    assert share[0] == 0.0 and share[1] >= 0.5 and share[4] >= 0.5
    assert dist[0] == 0.0 and min(dist[1:]) > 0.1
    assert np.array_equal(ref.vhat_next32([1, 2, np.nan, 3], [2, 1, 5, np.nan]), np.array([2, 2, np.nan, 3], np.float32), equal_nan=True)


def test_train_ctr_offers_amsgrad():
    src = open(os.path.join(ROOT, "examples", "train_ctr.py")).read()
    for word in ('"--amsgrad"', "amsgrad=args.amsgrad"):
        assert word in src, word
