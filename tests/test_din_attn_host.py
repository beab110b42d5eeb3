"""Host-only checks of the DIN attention pooling (include/fil.h N3 fil_din_*, functional.din_attention, layers.DinAttentionLayer,
models.DINInput / DIN): the entry points in the header, the binding and the library; their argument validation, the menu limits and
the plan's arithmetic through ctypes; the Python surface that needs no GPU; and self-checks of the fp64 restatement
(tests/din_attn_ref.py) the GPU tests are held to."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import din_attn_ref as ref

NEW = ("fil_din_plan", "fil_din_fwd", "fil_din_bwd_workspace_bytes", "fil_din_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
DIMS = (3, 4, 4, 2)        # T, K, H1, H2 of the small shape


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, H1, H2):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_din_plan(B, T, K, H1, H2, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def test_din_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    assert "#define FIL_DIN_SOFTMAX %d\n" % _lib.FIL_DIN_SOFTMAX in header and "#define FIL_DIN_SIGMOID %d\n" % _lib.FIL_DIN_SIGMOID in header
    assert (_lib.FIL_DIN_SOFTMAX, _lib.FIL_DIN_SIGMOID) == (1, 2)
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_din_plan"] == (I, [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_din_fwd"] == (I, [P] * 13 + [I] * 6 + [P])
    assert _lib.SIGNATURES["fil_din_bwd_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_din_bwd"] == (I, [P] * 25 + [Z] + [I] * 6 + [P])


# positions in the argument lists: q keys mask W1 b1 alpha1 W2 b2 alpha2 w3 b3 | out stats | g | dq dkeys + 8 parameter gradients | workspace
MASK, ALPHA1, ALPHA2 = 2, 5, 8


def test_din_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_din_fwd(*([None] * 13), 0, *DIMS, 0, None) == OK
    assert lib.fil_din_bwd(*([None] * 25), 0, 0, *DIMS, 3, None) == OK
    # NULL tensors with B > 0: every required one; mask may be NULL, and the slopes with the sigmoid only
    for hole in range(13):
        if hole == MASK:
            continue            # (mask = NULL is all live: a launch, which the GPU tests make)
        args = [p] * 13
        args[hole] = None
        assert lib.fil_din_fwd(*args, 5, *DIMS, 0, None) == ERR_ARG, hole
        assert "fil_din_fwd" in _msg(lib)
        if hole not in (ALPHA1, ALPHA2):
            assert lib.fil_din_fwd(*args, 5, *DIMS, _lib.FIL_DIN_SIGMOID, None) == ERR_ARG, hole
    for hole in range(14):
        if hole == MASK:
            continue
        args = [p] * 25
        args[hole] = None
        assert lib.fil_din_bwd(*args, 1 << 20, 5, *DIMS, 0, None) == ERR_ARG, hole
        assert "fil_din_bwd" in _msg(lib)
    assert lib.fil_din_bwd(*([p] * 14 + [None] * 11), 0, 5, *DIMS, 0, None) == ERR_ARG     # nothing to compute
    # non-positive dimensions, unknown flag bits
    for dims in ((-1, 3, 4, 4, 2), (5, 0, 4, 4, 2), (5, 3, 0, 4, 2), (5, 3, 4, 0, 2), (5, 3, 4, 4, 0)):
        assert lib.fil_din_fwd(*([p] * 13), *dims, 0, None) == ERR_ARG, dims
        assert lib.fil_din_bwd(*([p] * 25), 1 << 20, *dims, 0, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    assert lib.fil_din_fwd(*([p] * 13), 5, *DIMS, 4, None) == ERR_ARG
    assert lib.fil_din_bwd(*([p] * 25), 1 << 20, 5, *DIMS, 8, None) == ERR_ARG
    assert lib.fil_din_plan(5, *DIMS, None) == ERR_ARG
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
    need = lib.fil_din_bwd_workspace_bytes(5, *DIMS)
    assert need > 0
    assert lib.fil_din_bwd(*([p] * 25), need - 1, 5, *DIMS, 0, None) == ERR_ARG
    assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_din_bwd" in _msg(lib)
    args = [p] * 25
    args[24] = None
    assert lib.fil_din_bwd(*args, need, 5, *DIMS, 0, None) == ERR_ARG


def test_din_menu_limits_from_both_sides(lib):
    p = 4096
    outside = (((5, 3, 6, 4, 2), "K=6"), ((5, 3, 68, 4, 2), "K=68"), ((5, 257, 4, 4, 2), "T=257"), ((5, 3, 4, 129, 2), "H1=129"),
               ((5, 3, 4, 4, 65), "H2=65"), ((5, 3, 16, 128, 65), "H2=65"), ((5, 3, 32, 113, 17), "16385"))
    for dims, word in outside:
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and "fil_din_plan" in _msg(lib), (_msg(lib), word)
        assert lib.fil_din_fwd(*([p] * 13), *dims, 0, None) == ERR_UNSUPPORTED
        assert lib.fil_din_bwd(*([p] * 25), 1 << 20, *dims, 0, None) == ERR_UNSUPPORTED
        assert lib.fil_din_bwd_workspace_bytes(*dims) == 0
    # the bound from both sides: 113 (4 * 32 + 17) = 16385 is out, 128 (4 * 16 + 64) = 16384 and 127 (4 * 32 + 1) = 16383 are in
    assert 4 * 32 * 113 + 113 * 17 == 16385 and 4 * 16 * 128 + 128 * 64 == 16384 and 4 * 32 * 127 + 127 * 1 == 16383
    # the first included values on the other side of each limit, and every shape the GPU tests name
    inside = ((5, 3, 4, 4, 2), (5, 3, 8, 4, 2), (5, 3, 64, 4, 2), (5, 256, 4, 4, 2), (5, 1, 4, 1, 1), (5, 3, 4, 128, 2), (5, 3, 4, 4, 64),
              (5, 3, 16, 128, 64), (5, 256, 16, 128, 64), (5, 256, 64, 36, 16), (5, 50, 32, 80, 40), (5, 50, 16, 80, 40), (5, 129, 4, 5, 3),
              (5, 20, 12, 37, 9), (5, 64, 16, 36, 16), (5, 256, 64, 56, 36), (5, 256, 32, 121, 7), (5, 256, 32, 127, 1))
    for dims in inside:
        rc, pl = _plan(lib, *dims)
        assert rc == OK and pl[0] == 1 and pl[1] == 1, (dims, _msg(lib))
        assert 0 < pl[6] <= LDS_LIMIT and 0 < pl[7] <= LDS_LIMIT, (dims, pl)


def _n_out(K, H1, H2):
    return 4 * K * H1 + H1 * H2 + 2 * H1 + 3 * H2 + 1


def test_din_plan_arithmetic(lib):
    for T, K, H1, H2 in ((1, 4, 1, 1), (3, 4, 4, 2), (50, 16, 80, 40), (256, 16, 128, 64), (256, 64, 36, 16), (129, 4, 5, 3), (20, 12, 37, 9)):
        rc, (fwd_ok, bwd_ok, tile, grid, cap, parts, lds_f, lds_b) = _plan(lib, 4096, T, K, H1, H2)
        assert rc == OK and fwd_ok == 1 and bwd_ok == 1
        assert 1 <= tile <= 4 and cap >= 1
        assert 0 < lds_f <= LDS_LIMIT and 0 < lds_b <= LDS_LIMIT
        for B in (0, 1, tile - 1, tile, tile + 1, cap * tile, cap * tile + 1, 10 * cap * tile):
            rc, pl = _plan(lib, B, T, K, H1, H2)
            assert rc == OK and pl[2] == tile and pl[4] == cap and pl[6:] == [lds_f, lds_b]
            want_grid = min(-(-B // tile), cap)
            assert pl[3] == want_grid and pl[5] == want_grid, (B, pl)
            # one partial = dW1 | db1 | dalpha1 | dW2 | db2 | dalpha2 | dw3 | db3, fp32; the size is rounded up to 256 bytes
            ws = lib.fil_din_bwd_workspace_bytes(B, T, K, H1, H2)
            assert ws == -(-(pl[5] * _n_out(K, H1, H2) * 4) // 256) * 256
    # the menu's corner holds one sample per workgroup; the small shape four
    assert _plan(lib, 8, 256, 16, 128, 64)[1][2] == 1 and _plan(lib, 8, 3, 4, 4, 2)[1][2] == 4
    assert Fn.din_plan(8, 50, 16, 80, 40)["fits"] and 1 <= Fn.din_plan(8, 50, 16, 80, 40)["tile"] <= 4
    assert Fn.din_plan(8, 50, 6, 80, 40) == dict(fits=False) and Fn.din_plan(8, 50, 16, 130, 40) == dict(fits=False)
    with pytest.raises(FilError):
        Fn.din_plan(8, 0, 16, 80, 40)


# ------------------------------------------------------------------------------------------------ the reference
def _ragged_with_an_empty_sample(B, T, seed):
    m = ref.make_mask(B, T, "ragged", np.random.default_rng(seed))
    m[1] = 0
    return m


@pytest.mark.parametrize("softmax", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("activation", ["prelu", "sigmoid"])
def test_reference_backward_equals_fp64_autograd(activation, softmax):
    for shape in ((3, 3, 4, 4, 2), (4, 9, 8, 5, 3), (2, 5, 4, 16, 8)):
        case = ref.make_case(*shape, activation, softmax, seed=3, mask=_ragged_with_an_empty_sample(shape[0], shape[1], 5))
        auto = ref.torch_run(case, torch.float64)
        hand = ref.backward(case)
        assert np.abs(auto["out"] - ref.forward(case)).max() < 1e-12
        assert not ref.forward(case)[1].any() and not hand["dq"][1].any() and not hand["dkeys"][1].any()      # the all-masked sample
        for k in ref.GRADS:
            assert np.abs(auto[k].reshape(hand[k].shape) - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)
        assert not hand["dkeys"][np.asarray(case["mask"]) == 0].any()


def test_reference_exact_cases():
    # softmax with w3 = 0: the mean of the live keys; raw with w3 = 0, b3 = c: c times their sum; one live slot: that key
    case = ref.make_case(5, 7, 8, 4, 3, "sigmoid", True, seed=1)
    live = np.asarray(case["mask"], bool)
    zero = dict(case, w3=np.zeros(3))
    mean = (case["keys"] * live[:, :, None]).sum(1) / live.sum(1, keepdims=True)
    assert np.abs(ref.forward(zero) - mean).max() < 1e-14
    raw = dict(zero, softmax=False, b3=np.array([0.75]))
    assert np.abs(ref.forward(raw) - 0.75 * (case["keys"] * live[:, :, None]).sum(1)).max() < 1e-14
    one = np.zeros((5, 7), np.uint8)
    one[np.arange(5), [0, 6, 3, 3, 1]] = 1
    single = dict(case, mask=one)
    assert np.array_equal(ref.forward(single), case["keys"][np.arange(5), [0, 6, 3, 3, 1]])
    bw = ref.backward(single)
    assert not bw["ds"].any() and not bw["dq"].any() and not bw["dW1"].any()


def test_make_case_keeps_the_prelu_margin():
    for softmax in (False, True):
        c = ref.make_case(7, 50, 16, 80, 40, "prelu", softmax, seed=0)
        assert ref.prelu_margin(c).all()
        for k in ("q", "keys", "g") + ref.PARAMS:
            assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
        assert c["q"].shape == (7, 16) and c["keys"].shape == (7, 50, 16) and c["W1"].shape == (64, 80) and c["W2"].shape == (80, 40)
        assert c["w3"].shape == (40,) and c["b3"].shape == (1,) and c["mask"].shape == (7, 50) and c["mask"].sum(1).min() >= 1
        assert (c["alpha1"] >= 0).all() and (c["alpha1"] <= 0.3).all()
    s = ref.make_case(2, 3, 4, 4, 2, "sigmoid", False, seed=0)
    assert s["alpha1"] is None and s["alpha2"] is None and s["redrawn"] == 0
    assert ref.margins(16, 80) == (4 * 68 * 2.0 ** -23, 4 * 152 * 2.0 ** -23)
    # the loop ends on every PReLU shape of the GPU tests (the large shapes are sigmoid only)
    for shape in ((1, 1, 4, 1, 1), (3, 3, 4, 4, 2), (5, 63, 8, 16, 8), (5, 64, 8, 16, 8), (5, 65, 8, 16, 8), (3, 129, 4, 5, 3), (3, 20, 12, 37, 9),
                  (4, 64, 16, 36, 16)):
        assert ref.prelu_margin(ref.make_case(*shape, "prelu", True, seed=0)).all(), shape
    # the small edge cases are drawn until their cancelling sums are well conditioned
    for B in (1, 3, 4, 5):
        cc = ref.conditioned_case(B, 3, 4, 4, 2, "sigmoid", True)
        assert max(ref.backward(cc)["cond"].values()) <= ref.MAX_COND and cc["shape"] == (B, 3, 4, 4, 2)
    # a pre-activation of a live slot placed inside the margin is seen; the same one on a masked slot is not
    c = ref.make_case(2, 3, 4, 4, 2, "prelu", False, seed=0, mask=None)
    x0 = np.concatenate([c["q"][0], c["keys"][0, 1], c["q"][0] - c["keys"][0, 1], c["q"][0] * c["keys"][0, 1]])
    b1 = c["b1"].copy()
    b1[2] -= float(x0 @ c["W1"][:, 2] + b1[2])
    planted = dict(c, b1=b1)
    assert not ref.prelu_margin(planted)[0]
    mask = np.ones((2, 3), np.uint8)
    mask[0, 1] = 0
    assert ref.prelu_margin(dict(c, mask=mask))[0]


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.DinAttentionLayer is layers.behavior_layer.DinAttentionLayer and "DinAttentionLayer" in layers.__all__
    assert _sig(layers.DinAttentionLayer.__init__) == dict(hidden_units=(80, 40), activation="prelu", softmax=False, padding_id=0, seed=2020)
    assert _sig(models.DIN.__init__) == dict(att_hidden_units=(80, 40), att_activation="prelu", att_softmax=False, hidden_units=None)
    e = inspect.Parameter.empty
    assert _sig(models.DINInput.__init__) == dict(sparseInfo=e, behavior=e, denseInfo=None, padding_id=0, tableGrad="dense")
    s = _sig(Fn.din_attention)
    assert list(s) == ["q", "keys", "mask", "W1", "b1", "alpha1", "W2", "b2", "alpha2", "w3", "b3", "softmax", "activation"]
    assert s["softmax"] is False and s["activation"] == "prelu"
    assert list(_sig(Fn.din_plan)) == ["B", "T", "K", "H1", "H2"]
    layer = layers.DinAttentionLayer()
    assert (layer.hidden_units, layer.activation, layer.softmax, layer.padding_id, layer.seed) == ((80, 40), "prelu", False, 0, 2020)
    m = models.DIN()
    assert isinstance(m.dnn, layers.DnnLayer) and isinstance(m.score, layers.MergeScoreLayer) and isinstance(m.stack, layers.StackLayer)
    # FeatureInput and CTRModel are as they were
    assert list(_sig(models.CTRModel.__init__)) == ["feature_input", "body"] and list(_sig(models.CTRModel.forward)) == ["dense", "sparse_idx", "seq_idx"]
    for bad in ((80,), (80, 40, 20), ()):
        with pytest.raises(ValueError, match="hidden_units"):
            layers.DinAttentionLayer(hidden_units=bad)
    with pytest.raises(ValueError, match="activation"):
        layers.DinAttentionLayer(activation="dice")
    info = models.make_sparse_info([9, 5], embed_dim=8, names=["item", "user"])
    with pytest.raises(ValueError, match="runs"):
        models.DINInput(info, behavior=[("item", 4)], tableGrad="runs")
    with pytest.raises(ValueError, match="candidate"):
        models.DINInput(info, behavior=[("shop", 4)])


@pytest.mark.parametrize("activation", ["prelu", "relu", "sigmoid"])
def test_state_dict_names_and_shapes(activation):
    K, T = 8, 5
    layer = layers.DinAttentionLayer(hidden_units=(6, 3), activation=activation)
    layer.build([(2, 1, K), (2, T, K)])
    sd = layer.state_dict()
    names = ["att_w1", "att_b1", "att_alpha1", "att_w2", "att_b2", "att_alpha2", "att_w3", "att_b3"]
    shapes = [(4 * K, 6), (6,), (6,), (6, 3), (3,), (3,), (3, 1), (1,)]
    if activation == "sigmoid":
        names, shapes = [n for n in names if "alpha" not in n], [s for n, s in zip(names, shapes) if "alpha" not in n]
    assert list(sd) == names and [tuple(v.shape) for v in sd.values()] == shapes
    for n, v in sd.items():
        if n in ("att_w1", "att_w2", "att_w3"):          # glorot_uniform(seed): inside its limit, not all zero
            lim = np.sqrt(6.0 / sum(v.shape))
            assert float(v.abs().max()) <= lim and float(v.abs().max()) > 0
        else:
            assert not v.any(), n
    trainable = {n for n, p in layer.named_parameters() if p.requires_grad}
    assert ("att_alpha1" in trainable) == (activation == "prelu") and "att_w1" in trainable
    again = layers.DinAttentionLayer(hidden_units=(6, 3), activation=activation)
    again.build([(2, K), (2, T, K)])
    assert all(torch.equal(v, again.state_dict()[n]) for n, v in sd.items())


def test_no_cpu_fallback():
    B, T, K = 3, 5, 8
    q, keys, mask = torch.zeros(B, K), torch.zeros(B, T, K), torch.ones(B, T, dtype=torch.bool)
    w = [torch.zeros(s) for s in ((4 * K, 4), (4,), (4,), (4, 2), (2,), (2,), (2,), (1,))]
    with pytest.raises(FilError, match="GPU only"):
        Fn.din_attention(q, keys, mask, *w)
    with pytest.raises(FilError, match="GPU only"):
        Fn.din_attention(q, keys, None, *w, softmax=True, activation="sigmoid")
    with pytest.raises(FilError, match="GPU only"):
        layers.DinAttentionLayer(hidden_units=(4, 2))([q.unsqueeze(1), keys], mask=mask)
    with pytest.raises(FilError, match="GPU only"):
        layers.DinAttentionLayer(hidden_units=(130, 2))([q, keys])                         # outside the menu: the composed path
    with pytest.raises(FilError, match="GPU only"):
        layers.DinAttentionLayer(hidden_units=(4, 2))([torch.zeros(B, 6), torch.zeros(B, T, 6)])
    info = models.make_sparse_info([9, 5], embed_dim=8, names=["item", "user"])
    fi = models.DINInput(info, behavior=[("item", T)])
    with pytest.raises(FilError, match="GPU only"):
        fi((None, torch.zeros(B, 2, dtype=torch.int64), torch.zeros(B, 1, T, dtype=torch.int64)))
