"""Host-only checks of the AFM pair-attention pooling (include/fil.h N3 fil_afm_*, functional.afm_pool, layers.AFMLayer,
AttentionBaseLayer(softmax_axis=1), models.AFM(pair_softmax=True)): the entry points in the header, the binding and the library; their
argument validation and the plan's arithmetic through ctypes; the Python surface that needs no GPU; and self-checks of the fp64
restatement (tests/afm_pool_ref.py) the GPU tests are held to."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import afm_pool_ref as ref

NEW = ("fil_afm_plan", "fil_afm_fwd", "fil_afm_bwd_workspace_bytes", "fil_afm_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, F, K, A):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_afm_plan(B, F, K, A, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def test_afm_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    assert "#define FIL_AFM_HIDDEN_RELU %d\n" % _lib.FIL_AFM_HIDDEN_RELU in open(_lib.HEADER_PATH).read()
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_afm_plan"] == (I, [I, I, I, I, P])
    assert _lib.SIGNATURES["fil_afm_fwd"] == (I, [P] * 6 + [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_afm_bwd_workspace_bytes"] == (Z, [I, I, I, I])
    assert _lib.SIGNATURES["fil_afm_bwd"] == (I, [P] * 12 + [Z] + [I] * 5 + [P])


def test_afm_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_afm_fwd(None, None, None, None, None, None, 0, 3, 4, 2, 0, None) == OK
    assert lib.fil_afm_bwd(*([None] * 12), 0, 0, 3, 4, 2, 1, None) == OK
    # NULL tensors with B > 0
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert lib.fil_afm_fwd(*args, 5, 3, 4, 2, 0, None) == ERR_ARG, hole
        assert "fil_afm_fwd" in _msg(lib)
    for hole in range(7):
        args = [p] * 12
        args[hole] = None
        assert lib.fil_afm_bwd(*args, 1 << 20, 5, 3, 4, 2, 0, None) == ERR_ARG, hole
    assert lib.fil_afm_bwd(*([p] * 7 + [None] * 5), 0, 5, 3, 4, 2, 0, None) == ERR_ARG     # nothing to compute
    # non-positive dimensions, unknown flag bits
    for dims in ((-1, 3, 4, 2), (5, 0, 4, 2), (5, 3, 0, 2), (5, 3, 4, 0)):
        assert lib.fil_afm_fwd(*([p] * 6), *dims, 0, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    assert lib.fil_afm_fwd(*([p] * 6), 5, 3, 4, 2, 2, None) == ERR_ARG
    assert lib.fil_afm_bwd(*([p] * 12), 1 << 20, 5, 3, 4, 2, 4, None) == ERR_ARG
    assert lib.fil_afm_plan(5, 3, 4, 2, None) == ERR_ARG
    # outside the menu: -4 from every entry point, the limit in the message; the workspace size of such a shape is 0
    for dims, word in (((5, 1, 4, 2), "F=1"), ((5, 65, 4, 2), "F=65"), ((5, 3, 6, 2), "K=6"), ((5, 3, 68, 2), "K=68"), ((5, 3, 4, 17), "A=17")):
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and "fil_afm_plan" in _msg(lib)
        assert lib.fil_afm_fwd(*([p] * 6), *dims, 0, None) == ERR_UNSUPPORTED
        assert lib.fil_afm_bwd(*([p] * 12), 1 << 20, *dims, 0, None) == ERR_UNSUPPORTED
        assert lib.fil_afm_bwd_workspace_bytes(*dims) == 0
    # the first included values on the other side of each limit
    for dims in ((5, 2, 4, 1), (5, 64, 4, 2), (5, 3, 64, 2), (5, 3, 4, 16), (5, 64, 64, 16)):
        assert _plan(lib, *dims)[0] == OK, dims
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
    need = lib.fil_afm_bwd_workspace_bytes(5, 3, 4, 2)
    assert need > 0
    assert lib.fil_afm_bwd(*([p] * 12), need - 1, 5, 3, 4, 2, 0, None) == ERR_ARG
    assert str(need) in _msg(lib) and "workspace" in _msg(lib)
    args = [p] * 12
    args[11] = None
    assert lib.fil_afm_bwd(*args, need, 5, 3, 4, 2, 0, None) == ERR_ARG


def test_afm_plan_arithmetic(lib):
    for F, K, A in ((2, 4, 1), (3, 4, 2), (39, 16, 4), (12, 64, 16), (64, 16, 4), (64, 4, 1), (64, 64, 16), (23, 16, 16), (5, 12, 3)):
        rc, (fwd_ok, bwd_ok, tile, grid, cap, parts, lds_f, lds_b) = _plan(lib, 4096, F, K, A)
        assert rc == OK and fwd_ok == 1 and bwd_ok == 1
        assert 1 <= tile <= 4 and cap >= 1
        assert 0 < lds_f <= LDS_LIMIT and 0 < lds_b <= LDS_LIMIT
        for B in (0, 1, tile - 1, tile, tile + 1, cap * tile, cap * tile + 1, 10 * cap * tile):
            rc, pl = _plan(lib, B, F, K, A)
            assert rc == OK and pl[2] == tile and pl[4] == cap and pl[6:] == [lds_f, lds_b]
            want_grid = min(-(-B // tile), cap)
            assert pl[3] == want_grid and pl[5] == want_grid, (B, pl)
            # one partial = dW [K,A] | db [A] | dh [A], fp32; the size is rounded up to 256 bytes
            ws = lib.fil_afm_bwd_workspace_bytes(B, F, K, A)
            assert ws == -(-(pl[5] * (K * A + 2 * A) * 4) // 256) * 256
    # the largest shape of the menu runs one wave per workgroup; the benchmark's shape four
    assert _plan(lib, 8, 64, 64, 16)[1][2] == 1 and _plan(lib, 8, 39, 16, 4)[1][2] == 4
    assert Fn.afm_plan(8, 39, 16, 4)["fits"] and Fn.afm_plan(8, 39, 16, 4)["tile"] == 4
    assert Fn.afm_plan(8, 39, 6, 4) == dict(fits=False) and Fn.afm_plan(8, 65, 16, 4) == dict(fits=False)
    with pytest.raises(FilError):
        Fn.afm_plan(8, 0, 16, 4)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("hidden_relu", [False, True])
def test_reference_backward_equals_fp64_autograd(hidden_relu):
    for shape in ((3, 2, 4, 1), (4, 5, 8, 3), (2, 9, 4, 16)):
        case = ref.make_case(*shape, hidden_relu, seed=3)
        auto = ref.torch_run(case, torch.float64)
        assert np.abs(auto["pooled"] - ref.forward(case["e"], case["W"], case["b"], case["h"], hidden_relu)).max() < 1e-12
        hand = ref.backward(case["e"], case["W"], case["b"], case["h"], case["g"], hidden_relu)
        for k in ("de", "dW", "db", "dh"):
            assert np.abs(auto[k].reshape(hand[k].shape) - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)


@pytest.mark.parametrize("hidden_relu", [False, True])
def test_reference_with_zero_h_is_the_fm_sum_over_p(hidden_relu):
    case = ref.make_case(5, 12, 8, 4, hidden_relu, seed=1)
    e = case["e"]
    pooled = ref.forward(e, case["W"], case["b"], np.zeros((4, 1)), hidden_relu)
    s = e.sum(1)
    fm = 0.5 * (s * s - (e * e).sum(1))
    assert np.abs(pooled - fm / 66).max() < 1e-13
    # one pair: the pooled vector IS the pair product, whatever the weights
    one = ref.make_case(4, 2, 4, 3, hidden_relu, seed=2)
    assert np.array_equal(ref.forward(one["e"], one["W"], one["b"], one["h"], hidden_relu), one["e"][:, 0] * one["e"][:, 1])


def test_make_case_keeps_the_relu_margin():
    for hidden_relu in (False, True):
        c = ref.make_case(9, 12, 8, 4, hidden_relu, seed=0)
        assert ref.relu_margin(c["e"], c["W"], c["b"], c["h"], hidden_relu).all()
        for k in ("e", "W", "b", "h", "g"):
            assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
        assert c["e"].shape == (9, 12, 8) and c["W"].shape == (8, 4) and c["b"].shape == (4,) and c["h"].shape == (4, 1)
    assert ref.delta(16, 4) == 4 * 24 * 2.0 ** -23
    assert ref.pair_index(4)[0].tolist() == [0, 0, 0, 1, 1, 2] and ref.pair_index(4)[1].tolist() == [1, 2, 3, 2, 3, 3]
    # a pre-activation placed inside the margin is seen
    c = ref.make_case(2, 3, 4, 1, False, seed=0)
    b0 = c["b"].copy()
    t = ((c["e"][0, 0] * c["e"][0, 1]) @ c["W"] + b0) @ c["h"]
    b0[0] -= float(t[0] / c["h"][0, 0])
    assert not ref.relu_margin(c["e"], c["W"], b0, c["h"], False)[0]


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.AFMLayer is layers.interactive_layer.AFMLayer and "AFMLayer" in layers.__all__
    assert _sig(layers.AFMLayer.__init__) == dict(attention_dim=4, seed=2020, output_dim=1, hidden_relu=False)
    assert _sig(layers.AttentionBaseLayer.__init__) == dict(attention_dim=4, seed=2020, output_dim=1, softmax_axis=-1, hidden_relu=False)
    assert _sig(models.AFM.__init__) == dict(pair_softmax=False, hidden_relu=False, attention_dim=4)
    s = _sig(Fn.afm_pool)
    assert list(s) == ["emb", "w", "b", "h", "hidden_relu"] and s["hidden_relu"] is False
    base = layers.AttentionBaseLayer()
    assert (base.softmax_axis, base.hidden_relu, base.atten_dim, base.seed) == (-1, False, 4, 2020)
    fused = layers.AFMLayer()
    assert (fused.softmax_axis, fused.hidden_relu, fused.atten_dim, fused.seed) == (1, False, 4, 2020)
    with pytest.raises(ValueError, match="softmax_axis"):
        layers.AttentionBaseLayer(softmax_axis=0)
    # the default model is the reference's: InnerLayer pairs + AttentionBaseLayer with the size-1 softmax
    m = models.AFM()
    assert isinstance(m.inner, layers.InnerLayer) and type(m.atten) is layers.AttentionBaseLayer and m.atten.softmax_axis == -1
    p = models.AFM(pair_softmax=True, hidden_relu=True, attention_dim=8)
    assert type(p.atten) is layers.AFMLayer and not hasattr(p, "inner") and p.atten.hidden_relu and p.atten.atten_dim == 8


def test_state_dict_moves_between_the_two_layers():
    K = 8
    a, b = layers.AttentionBaseLayer(attention_dim=3, output_dim=2), layers.AFMLayer(attention_dim=3, output_dim=2)
    a.build([(5, 1, K)] * 6)              # the pair list of F = 4
    b.build([(5, 1, K)] * 4)              # the field list
    a.output_layer.build((5, K))
    b.output_layer.build((5, K))
    sa, sb = a.state_dict(), b.state_dict()
    # (kernel_w / kernel_b: the reference's attribute names of the first two weights, which the module registers as well)
    assert list(sa) == list(sb) == ["single_score_w", "kernel_w", "single_score_b", "kernel_b", "single_mlp_kernel", "output_layer.kernel",
                                    "output_layer.bias"]
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()] == [(K, 3), (K, 3), (3,), (3,), (3, 1), (K, 2), (2,)]
    for k in ("single_score_w", "single_score_b", "single_mlp_kernel"):   # the same initialiser and seed: the same values
        assert torch.equal(sa[k], sb[k]), k
    b.load_state_dict(sa)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in sa.items())
    packed = layers.AFMLayer()
    packed.build((5, 4, K))               # a packed [B,F,K] block builds the same weights
    assert tuple(packed.kernel_w.shape) == (K, 4)


def test_no_cpu_fallback():
    e, w, b, h = torch.zeros(3, 4, 8), torch.zeros(8, 4), torch.zeros(4), torch.zeros(4, 1)
    with pytest.raises(FilError, match="GPU only"):
        Fn.afm_pool(e, w, b, h)
    with pytest.raises(FilError, match="GPU only"):
        layers.AFMLayer()(e)
    with pytest.raises(FilError, match="GPU only"):
        layers.AFMLayer()(torch.zeros(3, 4, 6))                    # outside the menu: the composed path has no CPU form either
    with pytest.raises(FilError, match="GPU only"):
        layers.AFMLayer()(list(e.split(1, dim=1)))
