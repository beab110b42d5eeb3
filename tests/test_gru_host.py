"""Host-only checks of the GRU / AUGRU / AGRU over a behaviour sequence (include/fil.h N3 fil_gru_*, functional.gru, layers.GRULayer,
models.DIEN): the entry points in the header, the binding and the library; their argument validation, the menu limits and the plan's
arithmetic through ctypes; the orthogonal initialiser; the Python surface that needs no GPU; and self-checks of the fp64
restatement (tests/gru_ref.py) the GPU tests are held to."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from ml_function_amd.layers import base
from tests import gru_ref as ref

NEW = ("fil_gru_plan", "fil_gru_saved_bytes", "fil_gru_fwd", "fil_gru_bwd_workspace_bytes", "fil_gru_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
GRID_CAP = 1024
DIMS = (3, 4, 8)        # T, K, H of the small shape
GRU, AUGRU, AGRU = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, H, mode=GRU):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_gru_plan(B, T, K, H, mode, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def test_gru_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    for name, val in (("GRU", _lib.FIL_GRU_GRU), ("AUGRU", _lib.FIL_GRU_AUGRU), ("AGRU", _lib.FIL_GRU_AGRU)):
        assert "#define FIL_GRU_%s %d\n" % (name, val) in header
    assert (_lib.FIL_GRU_GRU, _lib.FIL_GRU_AUGRU, _lib.FIL_GRU_AGRU) == (0, 1, 2)
    assert Fn.GRU_MODES == dict(gru=0, augru=1, agru=2)
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_gru_plan"] == (I, [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_gru_saved_bytes"] == (Z, [I] * 4)
    assert _lib.SIGNATURES["fil_gru_fwd"] == (I, [P] * 8 + [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_gru_bwd_workspace_bytes"] == (Z, [I] * 4)
    assert _lib.SIGNATURES["fil_gru_bwd"] == (I, [P] * 15 + [Z] + [I] * 5 + [P])


# positions:  fwd: x a mask W U b hs saved        bwd: x a mask W U hs saved g_hs g_last | dx da dW dU db | workspace
A, MASK = 1, 2


def test_gru_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_gru_fwd(*([None] * 8), 0, *DIMS, GRU, None) == OK
    assert lib.fil_gru_bwd(*([None] * 15), 0, 0, *DIMS, AUGRU, None) == OK
    # NULL tensors with B > 0: x, W, U, b, hs are required (saved = NULL is the inference call and mask = NULL all live: launches,
    # which the GPU tests make)
    for hole in (0, 3, 4, 5, 6):
        args = [p] * 8
        args[hole] = None
        assert lib.fil_gru_fwd(*args, 5, *DIMS, AUGRU, None) == ERR_ARG, hole
        assert "fil_gru_fwd" in _msg(lib)
    # the scores: given in the modes AUGRU and AGRU and only there
    no_a = [p] * 8
    no_a[A] = None
    assert lib.fil_gru_fwd(*no_a, 5, *DIMS, AUGRU, None) == ERR_ARG and lib.fil_gru_fwd(*no_a, 5, *DIMS, AGRU, None) == ERR_ARG
    assert lib.fil_gru_fwd(*([p] * 8), 5, *DIMS, GRU, None) == ERR_ARG
    for hole in (0, 3, 4, 5, 6):
        args = [p] * 15
        args[hole] = None
        assert lib.fil_gru_bwd(*args, 1 << 20, 5, *DIMS, AUGRU, None) == ERR_ARG, hole
        assert "fil_gru_bwd" in _msg(lib)
    no_a = [p] * 15
    no_a[A] = None
    assert lib.fil_gru_bwd(*no_a, 1 << 20, 5, *DIMS, AUGRU, None) == ERR_ARG
    assert lib.fil_gru_bwd(*([p] * 15), 1 << 20, 5, *DIMS, GRU, None) == ERR_ARG
    no_a[10] = p
    assert lib.fil_gru_bwd(*no_a, 1 << 20, 5, *DIMS, GRU, None) == ERR_ARG                 # da in the mode without scores
    both = [p] * 15
    both[7] = both[8] = None
    assert lib.fil_gru_bwd(*both, 1 << 20, 5, *DIMS, AUGRU, None) == ERR_ARG               # neither g_hs nor g_last
    assert lib.fil_gru_bwd(*([p] * 9 + [None] * 5 + [p]), 1 << 20, 5, *DIMS, AUGRU, None) == ERR_ARG     # nothing to compute
    # non-positive dimensions, unknown modes
    for dims in ((-1, 3, 4, 8), (5, 0, 4, 8), (5, 3, 0, 8), (5, 3, 4, 0)):
        assert lib.fil_gru_fwd(*([p] * 8), *dims, AUGRU, None) == ERR_ARG, dims
        assert lib.fil_gru_bwd(*([p] * 15), 1 << 20, *dims, AUGRU, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    for mode in (-1, 3):
        assert lib.fil_gru_fwd(*([p] * 8), 5, *DIMS, mode, None) == ERR_ARG
        assert lib.fil_gru_bwd(*([p] * 15), 1 << 20, 5, *DIMS, mode, None) == ERR_ARG
        assert _plan(lib, 5, *DIMS, mode)[0] == ERR_ARG
    assert lib.fil_gru_plan(5, *DIMS, GRU, None) == ERR_ARG
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
    need = lib.fil_gru_bwd_workspace_bytes(5, *DIMS)
    assert need > 0
    assert lib.fil_gru_bwd(*([p] * 15), need - 1, 5, *DIMS, AUGRU, None) == ERR_ARG
    assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_gru_bwd" in _msg(lib)
    args = [p] * 15
    args[14] = None
    assert lib.fil_gru_bwd(*args, need, 5, *DIMS, AUGRU, None) == ERR_ARG


def test_gru_menu_limits_from_both_sides(lib):
    p = 4096
    outside = (((5, 3, 6, 8), "K=6"), ((5, 3, 68, 8), "K=68"), ((5, 3, 4, 6), "H=6"), ((5, 3, 4, 68), "H=68"), ((5, 3, 64, 66), "H=66"))
    for dims, word in outside:
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and "<= 64" in _msg(lib) and "fil_gru_plan" in _msg(lib), (_msg(lib), word)
        assert lib.fil_gru_fwd(*([p] * 8), *dims, AUGRU, None) == ERR_UNSUPPORTED
        assert lib.fil_gru_bwd(*([p] * 15), 1 << 20, *dims, AUGRU, None) == ERR_UNSUPPORTED
        assert lib.fil_gru_bwd_workspace_bytes(*dims) == 0 and lib.fil_gru_saved_bytes(*dims) == 0
    # every K, H of the menu, at a small and at a large batch (the tile grows with B), any T
    for K in range(4, 65, 4):
        for H in range(4, 65, 4):
            for B in (1, 4096, 1 << 20):
                rc, pl = _plan(lib, B, 100000, K, H)
                assert rc == OK and pl[0] == 1 and pl[1] == 1, (K, H, _msg(lib))
                assert 0 < pl[6] <= LDS_LIMIT and 0 < pl[7] <= LDS_LIMIT, (K, H, pl)
    assert _plan(lib, 5, 3, 64, 64)[1][7] == 161024


def test_gru_plan_arithmetic(lib):
    for T, K, H in ((1, 4, 4), (3, 4, 8), (50, 16, 16), (7, 12, 20), (300, 8, 4), (256, 64, 64), (5, 64, 4), (5, 4, 64), (50, 32, 32)):
        quad = max(H, K // 4)                                   # threads per quad of samples
        g_max = 256 // quad
        g_low = max(min(g_max, -(-64 // quad)), -(-(K + H) // 32))
        assert 1 <= g_low <= g_max
        for B in (0, 1, 4 * g_low - 1, 4 * g_low, 4 * g_low + 1, 4096, GRID_CAP * 4 * g_max, GRID_CAP * 4 * g_max + 1, 1 << 22):
            rc, (fwd_ok, bwd_ok, tile, grid, cap, parts, lds_f, lds_b) = _plan(lib, B, T, K, H)
            assert rc == OK and fwd_ok == 1 and bwd_ok == 1 and cap == GRID_CAP
            g = min(g_max, max(g_low, -(-B // (4 * GRID_CAP))))
            assert tile == 4 * g, (B, T, K, H, tile)
            want_grid = min(-(-B // tile), cap)
            assert grid == want_grid and parts == want_grid
            assert (K + H) <= 32 * g                            # at most 32 rows of [dW ; dU] per thread
            # one partial = dW | dU | db, fp32; saved = (z, r, c, hp_h) per step; both rounded up to 256 bytes
            assert lib.fil_gru_bwd_workspace_bytes(B, T, K, H) == -(-(parts * (K + H + 2) * 3 * H * 4) // 256) * 256
            assert lib.fil_gru_saved_bytes(B, T, K, H) == -(-(B * T * 4 * H * 4) // 256) * 256
            nsp = tile + 4
            assert lds_f == 4 * ((K + H) * 3 * H + 6 * H + 2 * (K + H) * nsp + 4 * tile)
            assert lds_b == 4 * ((K + H) * 3 * H + 2 * (K + H) * nsp + 4 * H * nsp + tile * 4 * H + H * nsp + 4 * tile)
        # the plan does not depend on the mode or on T
        assert _plan(lib, 77, T, K, H, AUGRU) == _plan(lib, 77, T, K, H, GRU) == _plan(lib, 77, T + 1, K, H, AGRU)
    # past the grid cap a workgroup walks more than one tile
    rc, pl = _plan(lib, GRID_CAP * 16 + 1, 1, 4, 64)
    assert pl[2] == 16 and pl[3] == GRID_CAP
    assert Fn.gru_plan(8, 50, 16, 16)["fits"] and Fn.gru_plan(8, 50, 16, 16, "augru")["tile"] == 16
    assert Fn.gru_plan(8, 50, 6, 16) == dict(fits=False) and Fn.gru_plan(8, 50, 16, 68) == dict(fits=False)
    with pytest.raises(FilError):
        Fn.gru_plan(8, 0, 16, 16)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mode", ref.MODES)
def test_reference_backward_equals_fp64_autograd(mode):
    for shape, grads in (((3, 3, 4, 4), "both"), ((4, 9, 8, 12), "hs"), ((2, 5, 4, 16), "last"), ((1, 1, 4, 4), "both")):
        m = ref.make_mask(shape[0], shape[1], "ragged", np.random.default_rng(5))
        if shape[0] > 1:
            m[1] = 0
        case = ref.make_case(*shape, mode, seed=3, mask=m, grads=grads)
        auto = ref.torch_run(case, torch.float64)
        hand = ref.backward(case)
        hs = ref.forward(case)
        assert np.abs(auto["hs"] - hs).max() < 1e-12
        if shape[0] > 1:
            assert not hs[1].any() and not hand["dx"][1].any() and not hand["da"][1].any()      # the all-masked sample
        for k in ref.GRADS:
            assert np.abs(auto[k].reshape(hand[k].shape) - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)
        assert not hand["dx"][m == 0].any() and not hand["da"][m == 0].any()
        if mode != "gru":
            assert np.abs(hand["da"]).max() > 0 or shape == (1, 1, 4, 4)


def test_reference_exact_cases():
    case = ref.make_case(4, 6, 8, 4, "augru", seed=1, mask=None)
    ones = dict(case, a=np.ones((4, 6)))
    assert np.array_equal(ref.forward(ones), ref.forward(dict(case, mode="gru", a=None)))       # AUGRU with a = 1 is the GRU
    for mode in ("augru", "agru"):
        a = case["a"].copy()
        a[:, 3] = 0.0
        hs = ref.forward(dict(case, mode=mode, a=a))
        assert np.array_equal(hs[:, 3], hs[:, 2])                                                # a_t = 0 repeats the state
    m = np.ones((4, 6), np.uint8)
    m[:, :2] = 0
    m[:, 4] = 0
    hs = ref.forward(dict(case, mask=m))
    assert not hs[:, :2].any() and np.array_equal(hs[:, 4], hs[:, 3]) and hs[:, 2].any()
    # the last state's gradient is the sequence gradient that is zero except at T - 1
    g_hs = np.zeros((4, 6, 4))
    g_hs[:, -1] = case["g_last"]
    one, two = ref.backward(dict(case, g_hs=None)), ref.backward(dict(case, g_hs=g_hs, g_last=None))
    for k in ref.GRADS:
        assert np.array_equal(one[k], two[k]), k
    # the agru's z gate gets no gradient: the z columns of dW, dU and db are zero
    bw = ref.backward(dict(case, mode="agru"))
    assert not bw["dW"][:, :4].any() and not bw["dU"][:, :4].any() and not bw["db"][:, :4].any() and bw["dW"][:, 4:].any()


def test_make_case_draws_what_the_bars_were_sized_on():
    c = ref.make_case(7, 50, 16, 36, "augru", seed=0)
    for k in ("x", "a", "g_hs", "g_last") + ref.PARAMS:
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    assert c["x"].shape == (7, 50, 16) and c["a"].shape == (7, 50) and c["W"].shape == (16, 108) and c["U"].shape == (36, 108)
    assert c["b"].shape == (2, 108) and c["mask"].shape == (7, 50) and (c["a"] >= 0).all() and (c["a"] <= 1).all()
    assert ref.make_case(2, 3, 4, 4, "gru", seed=0)["a"] is None
    # the fp32 torch restatement's own error on shapes the bars were sized on: the 1e-5 floor binds
    for shape in ((1, 1, 4, 4), (3, 2, 4, 8), (5, 50, 16, 16)):
        for mode in ref.MODES:
            case = ref.make_case(*shape, mode, seed=0)
            _, _, e32 = ref.reference(case)
            assert set(ref.bars(e32).values()) == {1e-5}, (shape, mode, e32)        # the floor binds: 4 E32 < 1e-5
    for B in (1, 3, 15, 17):
        cc = ref.conditioned_case(B, 3, 4, 8, "augru")
        assert max(ref.backward(cc)["cond"].values()) <= ref.MAX_COND and cc["shape"] == (B, 3, 4, 8)


# ------------------------------------------------------------------------------------------------ the orthogonal initialiser
@pytest.mark.parametrize("shape", [(4, 12), (16, 48), (64, 192), (12, 4), (8, 8)])
def test_orthogonal_initialiser(shape):
    layer = base.Layer()
    w = layer.add_weight("w", shape, "orthogonal", seed=7)
    q = w.detach().double().numpy()
    small = min(shape)
    gram = q @ q.T if shape[0] <= shape[1] else q.T @ q
    assert np.abs(gram - np.eye(small)).max() < 1e-6                                   # Q Q^T = I
    again = base.Layer().add_weight("w", shape, "orthogonal", seed=7)
    assert torch.equal(w, again)                                                       # the same seed gives the same bits
    assert not torch.equal(w, base.Layer().add_weight("w", shape, "orthogonal", seed=8))
    with pytest.raises(ValueError, match="matrix"):
        base.Layer().add_weight("w", (4,), "orthogonal", seed=7)


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.GRULayer is layers.behavior_layer.GRULayer and "GRULayer" in layers.__all__
    assert _sig(layers.GRULayer.__init__) == dict(units=inspect.Parameter.empty, mode="gru", return_sequences=True, seed=2020)
    assert _sig(models.DIEN.__init__) == dict(gru_type="augru", hidden_units=None, seed=2020)
    s = _sig(Fn.gru)
    assert list(s) == ["x", "a", "mask", "W", "U", "b", "mode", "return_sequences"] and s["mode"] == "gru" and s["return_sequences"] is True
    assert list(_sig(Fn.gru_plan)) == ["B", "T", "K", "H", "mode"]
    m = models.DIEN()
    assert isinstance(m.dnn, layers.DnnLayer) and isinstance(m.score, layers.MergeScoreLayer) and isinstance(m.stack, layers.StackLayer)
    with pytest.raises(ValueError, match="mode"):
        layers.GRULayer(8, mode="aigru")
    with pytest.raises(ValueError, match="units"):
        layers.GRULayer(0)
    with pytest.raises(ValueError, match="gru_type"):
        models.DIEN(gru_type="lstm")
    with pytest.raises(ValueError, match="mode"):
        Fn.gru(torch.zeros(1, 1, 4), None, None, torch.zeros(4, 12), torch.zeros(4, 12), torch.zeros(2, 12), mode="lstm")


def test_state_dict_names_shapes_and_initialisers():
    K, T, H = 8, 5, 12
    layer = layers.GRULayer(H, mode="augru")
    layer.build([(2, T, K), (2, T)])
    sd = layer.state_dict()
    assert list(sd) == ["kernel", "recurrent_kernel", "bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(K, 3 * H), (H, 3 * H), (2, 3 * H)]
    assert float(sd["kernel"].abs().max()) <= np.sqrt(6.0 / (K + 3 * H)) and float(sd["kernel"].abs().max()) > 0
    u = sd["recurrent_kernel"].double().numpy()
    assert np.abs(u @ u.T - np.eye(H)).max() < 1e-6
    assert not sd["bias"].any()
    again = layers.GRULayer(H)
    again.build((2, T, K))
    assert all(torch.equal(v, again.state_dict()[n]) for n, v in sd.items())


def test_layer_shape_and_mask_validation():
    x, a = torch.zeros(3, 5, 8), torch.zeros(3, 5)
    gru, augru = layers.GRULayer(4), layers.GRULayer(4, mode="augru")
    with pytest.raises(ValueError, match=r"\[B,T,K\]"):
        gru(torch.zeros(3, 8))
    with pytest.raises(ValueError, match="takes x alone"):
        gru([x, a])
    with pytest.raises(ValueError, match=r"takes \[x, scores\]"):
        augru(x)
    with pytest.raises(ValueError, match="scores must be"):
        augru([x, torch.zeros(3, 4)])
    with pytest.raises(ValueError, match="mask must be"):
        gru(x, mask=torch.ones(3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask must be"):
        gru(x, mask=torch.ones(3, 5))


def test_no_cpu_fallback():
    x, a, mask = torch.zeros(3, 5, 8), torch.zeros(3, 5), torch.ones(3, 5, dtype=torch.bool)
    w = [torch.zeros(8, 12), torch.zeros(4, 12), torch.zeros(2, 12)]
    with pytest.raises(FilError, match="GPU only"):
        Fn.gru(x, None, mask, *w)
    with pytest.raises(FilError, match="GPU only"):
        Fn.gru(x, a, None, *w, mode="agru", return_sequences=False)
    with pytest.raises(FilError, match="GPU only"):
        layers.GRULayer(4)(x, mask=mask)
    with pytest.raises(FilError, match="GPU only"):
        layers.GRULayer(68, mode="augru")([x, a])                    # outside the menu: the composed path
    with pytest.raises(FilError, match="GPU only"):
        layers.GRULayer(4)(torch.zeros(3, 5, 6))
