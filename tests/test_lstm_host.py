"""Host-only checks of the LSTM over a sequence (include/fil.h N3 fil_lstm_*, functional.lstm, layers.LSTMLayer / BiLSTMLayer,
models.DSIN): the entry points in the header, the binding and the library; their argument validation, the menu limits and the plan's
arithmetic through ctypes; the Python surface that needs no GPU; and self-checks of the fp64 restatement (tests/lstm_ref.py) the GPU
tests are held to -- against fp64 autograd and, independently, against torch.nn.LSTM."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from ml_function_amd.layers import base
from ml_function_amd.layers.behavior_layer import lstm_graph
from tests import lstm_ref as ref

NEW = ("fil_lstm_plan", "fil_lstm_saved_bytes", "fil_lstm_fwd", "fil_lstm_bwd_workspace_bytes", "fil_lstm_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
GRID_CAP = 1024
DIMS = (3, 4, 8)        # T, K, H of the small shape
FORWARD, REVERSE, BIDIR = 0, 1, 2
FIRST_REFUSED = (56, 60)      # K, H: the first pair the plan refuses, H ascending, then K


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, H, dirs=FORWARD):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_lstm_plan(B, T, K, H, dirs, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def _layout(B, K, H):
    """The launchers' layout restated: (tile, forward LDS bytes, backward LDS bytes)."""
    quad = max(H, K // 4)                                   # threads per quad of samples
    g_max = 256 // quad
    g_low = max(min(g_max, -(-64 // quad)), -(-(K + H) // 32))
    g = min(g_max, max(g_low, -(-B // (4 * GRID_CAP))))
    ns = 4 * g
    nsp = ns + 4
    fwd = 4 * ((K + H) * 4 * H + 4 * H + 2 * (K + H) * nsp + 2 * ns)
    bwd = 4 * ((K + H) * 4 * H + 2 * (K + H) * nsp + 4 * H * nsp + ns * 4 * H + 2 * ns)
    return ns, fwd, bwd


def test_lstm_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    for name, val in (("FORWARD", _lib.FIL_LSTM_FORWARD), ("REVERSE", _lib.FIL_LSTM_REVERSE), ("BIDIR", _lib.FIL_LSTM_BIDIR)):
        assert "#define FIL_LSTM_%s %d\n" % (name, val) in header
    assert (_lib.FIL_LSTM_FORWARD, _lib.FIL_LSTM_REVERSE, _lib.FIL_LSTM_BIDIR) == (0, 1, 2)
    assert Fn.LSTM_DIRECTIONS == dict(forward=0, reverse=1, bidirectional=2)
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_lstm_plan"] == (I, [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_lstm_saved_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_lstm_fwd"] == (I, [P] * 7 + [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_lstm_bwd_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_lstm_bwd"] == (I, [P] * 13 + [Z] + [I] * 5 + [P])


# positions:  fwd: x mask W U b hs saved        bwd: x mask W U hs saved g_hs g_last | dx dW dU db | workspace
def test_lstm_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    for dirs in (FORWARD, REVERSE, BIDIR):
        # B == 0: a no-op that returns 0 before any pointer is looked at
        assert lib.fil_lstm_fwd(*([None] * 7), 0, *DIMS, dirs, None) == OK
        assert lib.fil_lstm_bwd(*([None] * 13), 0, 0, *DIMS, dirs, None) == OK
        # NULL tensors with B > 0: x, W, U, b, hs are required (saved = NULL is the inference call and mask = NULL all live: launches,
        # which the GPU tests make)
        for hole in (0, 2, 3, 4, 5):
            args = [p] * 7
            args[hole] = None
            assert lib.fil_lstm_fwd(*args, 5, *DIMS, dirs, None) == ERR_ARG, hole
            assert "fil_lstm_fwd" in _msg(lib)
        for hole in (0, 2, 3, 4, 5):          # x, W, U, hs, saved
            args = [p] * 13
            args[hole] = None
            assert lib.fil_lstm_bwd(*args, 1 << 20, 5, *DIMS, dirs, None) == ERR_ARG, hole
            assert "fil_lstm_bwd" in _msg(lib)
        both = [p] * 13
        both[6] = both[7] = None
        assert lib.fil_lstm_bwd(*both, 1 << 20, 5, *DIMS, dirs, None) == ERR_ARG               # neither g_hs nor g_last
        assert lib.fil_lstm_bwd(*([p] * 8 + [None] * 4 + [p]), 1 << 20, 5, *DIMS, dirs, None) == ERR_ARG     # nothing to compute
        # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
        need = lib.fil_lstm_bwd_workspace_bytes(5, *DIMS, dirs)
        assert need > 0
        assert lib.fil_lstm_bwd(*([p] * 13), need - 1, 5, *DIMS, dirs, None) == ERR_ARG
        assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_lstm_bwd" in _msg(lib)
        args = [p] * 13
        args[12] = None
        assert lib.fil_lstm_bwd(*args, need, 5, *DIMS, dirs, None) == ERR_ARG
    # both directions in one launch: dx alone needs the workspace too (the second direction's dx)
    only_dx = [p] * 9 + [None] * 3 + [None]
    assert lib.fil_lstm_bwd(*only_dx, 0, 5, *DIMS, BIDIR, None) == ERR_ARG and "workspace" in _msg(lib)
    # non-positive dimensions, unknown directions
    for dims in ((-1, 3, 4, 8), (5, 0, 4, 8), (5, 3, 0, 8), (5, 3, 4, 0)):
        assert lib.fil_lstm_fwd(*([p] * 7), *dims, BIDIR, None) == ERR_ARG, dims
        assert lib.fil_lstm_bwd(*([p] * 13), 1 << 20, *dims, BIDIR, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    for dirs in (-1, 3):
        assert lib.fil_lstm_fwd(*([p] * 7), 5, *DIMS, dirs, None) == ERR_ARG
        assert lib.fil_lstm_bwd(*([p] * 13), 1 << 20, 5, *DIMS, dirs, None) == ERR_ARG
        assert _plan(lib, 5, *DIMS, dirs)[0] == ERR_ARG
        assert lib.fil_lstm_saved_bytes(5, *DIMS, dirs) == 0 and lib.fil_lstm_bwd_workspace_bytes(5, *DIMS, dirs) == 0
    assert lib.fil_lstm_plan(5, *DIMS, FORWARD, None) == ERR_ARG


def test_lstm_menu_limits_from_both_sides(lib):
    p = 4096
    outside = (((5, 3, 6, 8), "K=6"), ((5, 3, 68, 8), "K=68"), ((5, 3, 4, 6), "H=6"), ((5, 3, 4, 68), "H=68"), ((5, 3, 68, 68), "K=68"))
    for dims, word in outside:
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and "<= 64" in _msg(lib) and "fil_lstm_plan" in _msg(lib), (_msg(lib), word)
        assert lib.fil_lstm_fwd(*([p] * 7), *dims, BIDIR, None) == ERR_UNSUPPORTED
        assert lib.fil_lstm_bwd(*([p] * 13), 1 << 20, *dims, BIDIR, None) == ERR_UNSUPPORTED
        assert lib.fil_lstm_bwd_workspace_bytes(*dims, BIDIR) == 0 and lib.fil_lstm_saved_bytes(*dims, BIDIR) == 0
    # every K, H up to 64, at a small and at a large batch (the tile grows with B), any T: inside exactly when the restated
    # layout fits; the required floor (H <= 56, and H = 64 with K <= 40) is inside
    refused = []
    for H in range(4, 65, 4):
        for K in range(4, 65, 4):
            answers = set()
            for B in (1, 4096, 1 << 20):
                rc, pl = _plan(lib, B, 100000, K, H, BIDIR)
                _, fwd, bwd = _layout(B, K, H)
                assert (rc == OK) == (max(fwd, bwd) <= LDS_LIMIT), (K, H, B, _msg(lib))
                if rc == OK:
                    assert pl[0] == 1 and pl[1] == 1 and pl[6] == fwd and pl[7] == bwd and 0 < pl[6] <= LDS_LIMIT and 0 < pl[7] <= LDS_LIMIT
                else:
                    assert rc == ERR_UNSUPPORTED
                answers.add(rc)
            assert len(answers) == 1, (K, H)                # the menu does not depend on the batch
            if answers == {ERR_UNSUPPORTED}:
                refused.append((K, H))
            assert (K, H) not in refused or not (H <= 56 or (H == 64 and K <= 40)), (K, H)
    assert refused == [(K, 60) for K in range(56, 65, 4)] + [(K, 64) for K in range(44, 65, 4)]
    assert refused[0] == FIRST_REFUSED
    assert _plan(lib, 5, 3, 64, 56)[1][6:] == [4 * ((64 + 56) * 224 + 224 + 2 * 120 * 20 + 32), 159104]
    assert _plan(lib, 5, 3, 40, 64)[0] == OK
    # the refusal names the needed and the allowed bytes, from every entry point
    for dims, need in (((5, 3, 64, 64), 188544), ((5, 3) + FIRST_REFUSED, _layout(5, *FIRST_REFUSED)[2])):
        assert need > LDS_LIMIT
        for call in (lambda: _plan(lib, *dims)[0], lambda: lib.fil_lstm_fwd(*([p] * 7), *dims, FORWARD, None),
                     lambda: lib.fil_lstm_bwd(*([p] * 13), 1 << 20, *dims, REVERSE, None)):
            assert call() == ERR_UNSUPPORTED
            assert str(need) in _msg(lib) and str(LDS_LIMIT) in _msg(lib) and "LDS" in _msg(lib), _msg(lib)
        assert lib.fil_lstm_bwd_workspace_bytes(*dims, FORWARD) == 0 and lib.fil_lstm_saved_bytes(*dims, FORWARD) == 0


def test_lstm_plan_arithmetic(lib):
    r256 = lambda n: -(-n // 256) * 256
    for T, K, H in ((1, 4, 4), (3, 4, 8), (2, 4, 4), (50, 16, 16), (7, 12, 20), (300, 8, 4), (64, 64, 56), (5, 40, 64), (5, 64, 4), (5, 4, 64),
                    (50, 32, 32)):
        tile1 = _layout(1, K, H)[0]
        tile_max = 4 * (256 // max(H, K // 4))
        for B in (0, 1, tile1 - 1, tile1, tile1 + 1, 4096, GRID_CAP * tile_max, GRID_CAP * tile_max + 1, 1 << 22):
            tile, fwd, bwd = _layout(B, K, H)
            want_grid = min(-(-B // tile), GRID_CAP)
            assert (K + H) * 4 <= 32 * tile                      # at most 32 rows of [dW ; dU] per thread
            for dirs, n in ((FORWARD, 1), (REVERSE, 1), (BIDIR, 2)):
                rc, pl = _plan(lib, B, T, K, H, dirs)
                # grid and cap count one direction's workgroups; every workgroup leaves a partial: BIDIR has twice as many
                assert rc == OK and pl == [1, 1, tile, want_grid, GRID_CAP, n * want_grid, fwd, bwd], (B, T, K, H, dirs, pl)
                # one partial = dW | dU | db, fp32, rounded up to 256 bytes; BIDIR: + the second direction's dx
                parts = r256(n * want_grid * (K + H + 1) * 4 * H * 4)
                assert lib.fil_lstm_bwd_workspace_bytes(B, T, K, H, dirs) == r256(parts + (B * T * K * 4 if n == 2 else 0))
                # saved = (i, f, g, o, c) per step and direction: within the ceiling of 6 H floats
                sv = lib.fil_lstm_saved_bytes(B, T, K, H, dirs)
                assert sv == r256(n * B * T * 5 * H * 4) and sv <= r256(6 * H * 4 * B * T * n)
        # the plan does not depend on T
        assert _plan(lib, 77, T, K, H, BIDIR) == _plan(lib, 77, T + 1, K, H, BIDIR)
    assert Fn.lstm_plan(8, 50, 16, 16)["fits"] and Fn.lstm_plan(8, 50, 16, 16, "bidirectional")["tile"] == 16
    assert Fn.lstm_plan(8, 50, 16, 16, "bidirectional")["partials"] == 2 * Fn.lstm_plan(8, 50, 16, 16, "reverse")["partials"] == 2
    assert Fn.lstm_plan(8, 50, 6, 16) == dict(fits=False) and Fn.lstm_plan(8, 50, 16, 68) == dict(fits=False)
    assert Fn.lstm_plan(8, 50, *FIRST_REFUSED) == dict(fits=False) and Fn.lstm_plan(8, 50, 64, 56, "bidirectional")["fits"]
    with pytest.raises(FilError):
        Fn.lstm_plan(8, 0, 16, 16)
    with pytest.raises(KeyError):
        Fn.lstm_plan(8, 5, 16, 16, "backward")


# ------------------------------------------------------------------------------------------------ the reference
directions = pytest.mark.parametrize("direction", ref.DIRECTIONS)


@directions
def test_reference_backward_equals_fp64_autograd(direction):
    for shape, grads in (((3, 3, 4, 4), "both"), ((4, 9, 8, 12), "hs"), ((2, 5, 4, 16), "last"), ((1, 1, 4, 4), "both")):
        m = ref.make_mask(shape[0], shape[1], "ragged", np.random.default_rng(5))
        if shape[0] > 1:
            m[1] = 0
        case = ref.make_case(*shape, direction, seed=3, mask=m, grads=grads)
        auto = ref.torch_run(case, torch.float64)
        hand = ref.backward(case)
        hs = ref.forward(case)
        assert hs.shape == shape[:2] + (ref.ndir(direction) * shape[3],)
        assert np.abs(auto["hs"] - hs).max() < 1e-12
        if shape[0] > 1:
            assert not hs[1].any() and not hand["dx"][1].any()                   # the all-masked sample gives zeros
        for k in ref.GRADS:
            assert hand[k].shape == np.asarray(case[k[1:]]).shape
            assert np.abs(auto[k] - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)
        assert not hand["dx"][m == 0].any()


@pytest.mark.parametrize("mask", ["prefix", None])
def test_reference_equals_torch_nn_lstm(mask):
    """Independent of the code under test: torch.nn.LSTM(bidirectional=True) in float64 on the CPU (gate order i, f, g, o as Keras'
    i, f, c, o; bias_ih = b, bias_hh = 0), pack_padded_sequence for the ragged lengths.  Agreement to 1e-12 norm-relative on the live
    outputs, the last states and every gradient; the one-direction references are the halves of the bidirectional one."""
    B, T, K, H = 5, 7, 8, 12
    case = ref.make_case(B, T, K, H, "bidirectional", seed=11, mask=mask)
    live = np.ones((B, T), bool) if mask is None else case["mask"].astype(bool)
    lens = live.sum(1)
    assert mask is None or (lens.min() < T and lens.min() >= 1)
    case["g_hs"] = case["g_hs"] * live[:, :, None]            # torch.nn.LSTM has no output past a sequence's end
    net = torch.nn.LSTM(K, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            getattr(net, "weight_ih_l0" + sfx).copy_(torch.tensor(case["W"][d].T))
            getattr(net, "weight_hh_l0" + sfx).copy_(torch.tensor(case["U"][d].T))
            getattr(net, "bias_ih_l0" + sfx).copy_(torch.tensor(case["b"][d]))
            getattr(net, "bias_hh_l0" + sfx).zero_()
    x = torch.tensor(case["x"], requires_grad=True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    out, (h_n, _) = net(packed)
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    last = torch.cat([h_n[0], h_n[1]], dim=1)
    ((out * torch.tensor(case["g_hs"])).sum() + (last * torch.tensor(case["g_last"])).sum()).backward()
    hs, bwd = ref.forward(case), ref.backward(case)
    D = lambda v: v.detach().numpy()
    assert ref.norm_rel(D(out) * live[:, :, None], hs * live[:, :, None]) < 1e-12
    assert ref.norm_rel(D(last), ref.last_of(hs, "bidirectional")) < 1e-12
    assert ref.norm_rel(D(x.grad), bwd["dx"]) < 1e-12
    for d, sfx in enumerate(("", "_reverse")):
        assert ref.norm_rel(D(getattr(net, "weight_ih_l0" + sfx).grad).T, bwd["dW"][d]) < 1e-12
        assert ref.norm_rel(D(getattr(net, "weight_hh_l0" + sfx).grad).T, bwd["dU"][d]) < 1e-12
        assert ref.norm_rel(D(getattr(net, "bias_ih_l0" + sfx).grad), bwd["db"][d]) < 1e-12
    # one direction = that half of the bidirectional case
    for d, direction in enumerate(("forward", "reverse")):
        cols = slice(d * H, (d + 1) * H)
        one = dict(case, direction=direction, W=case["W"][d], U=case["U"][d], b=case["b"][d], g_hs=case["g_hs"][:, :, cols],
                   g_last=case["g_last"][:, cols])
        assert np.array_equal(ref.forward(one), hs[:, :, cols])
        b1 = ref.backward(one)
        for k in ("dW", "dU", "db"):
            assert np.array_equal(b1[k], bwd[k][d]), k


def test_reference_exact_cases():
    B, T, K, H = 4, 6, 8, 4
    case = ref.make_case(B, T, K, H, "forward", seed=1, mask=None)
    # an all-masked sample gives zeros, whatever the direction
    m = np.ones((B, T), np.uint8)
    m[2] = 0
    for direction in ref.DIRECTIONS:
        c = ref.make_case(B, T, K, H, direction, seed=1, mask=m)
        assert not ref.forward(c)[2].any() and not ref.backward(c)["dx"][2].any()
    # f = 1, i = 0 carries c: saturated biases (sigmoid(+-800) is exactly 1 / 0 in fp64) and no weights into those gates
    W, U, b = case["W"].copy(), case["U"].copy(), case["b"].copy()
    W[:, :2 * H] = 0.0
    U[:, :2 * H] = 0.0
    b[:H], b[H:2 * H] = -800.0, 800.0
    x, live, Wn, Un, bn, revs = ref._inputs(dict(case, W=W, U=U, b=b))
    with np.errstate(over="ignore"):                                              # exp(800) = inf: 1 / (1 + inf) = 0
        _, keep = ref._steps(x, live, Wn[0], Un[0], bn[0], False)
    assert all(not s["cn"].any() for s in keep)                                   # c_0 = 0 is carried through every step
    with np.errstate(over="ignore"):                                              # and a cell that is there is carried unchanged
        h1, k1 = ref._steps(x[:, :1], live[:, :1], case["W"], case["U"], case["b"], False)
        c1 = k1[0]["cn"]
        f = lambda v, n: v[:, n * H:(n + 1) * H]
        z = x[:, 1] @ Wn[0] + h1[:, 0] @ Un[0] + bn[0]
        assert np.array_equal(ref._sig(f(z, 1)) * c1 + ref._sig(f(z, 0)) * np.tanh(f(z, 2)), c1) and c1.any()
    # masked steps carry the state; zeros before the first live step, in both walking directions
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0
    m[:, 4] = 0
    hs = ref.forward(dict(case, mask=m))
    assert not hs[:, :2].any() and np.array_equal(hs[:, 4], hs[:, 3]) and hs[:, 2].any()
    hs = ref.forward(dict(case, mask=m, direction="reverse"))
    assert np.array_equal(hs[:, 4], hs[:, 5]) and np.array_equal(hs[:, 0], hs[:, 2]) and np.array_equal(hs[:, 1], hs[:, 2])
    m[:, 5] = 0
    assert not ref.forward(dict(case, mask=m, direction="reverse"))[:, 4:].any()
    # the last states' gradient is the sequence gradient that is zero except at each direction's last step
    bi = ref.make_case(B, T, K, H, "bidirectional", seed=1)
    g_hs = np.zeros((B, T, 2 * H))
    g_hs[:, -1, :H] = bi["g_last"][:, :H]
    g_hs[:, 0, H:] = bi["g_last"][:, H:]
    one, two = ref.backward(dict(bi, g_hs=None)), ref.backward(dict(bi, g_hs=g_hs, g_last=None))
    for k in ref.GRADS:
        assert np.array_equal(one[k], two[k]), k
    # reverse on the time-reversed case is forward, time-reversed
    rc = dict(case, direction="reverse", x=case["x"][:, ::-1], g_hs=case["g_hs"][:, ::-1])
    assert np.array_equal(ref.forward(rc)[:, ::-1], ref.forward(case))
    assert np.array_equal(ref.backward(rc)["dx"][:, ::-1], ref.backward(case)["dx"])


FEW_STEP_SHAPES = [(B, 3, 4, 8) for B in (5, 31, 32, 33)]      # the shapes test_lstm_gpu.py takes conditioned cases at


def test_make_case_draws_what_the_bars_were_sized_on():
    c = ref.make_case(7, 50, 16, 36, "bidirectional", seed=0)
    for k in ("x", "g_hs", "g_last") + ref.PARAMS:
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    assert c["x"].shape == (7, 50, 16) and c["W"].shape == (2, 16, 144) and c["U"].shape == (2, 36, 144) and c["b"].shape == (2, 144)
    assert c["mask"].shape == (7, 50) and c["g_hs"].shape == (7, 50, 72) and c["g_last"].shape == (7, 72)
    assert ref.make_case(2, 3, 4, 4, "reverse", seed=0)["W"].shape == (4, 16)
    for shape in FEW_STEP_SHAPES:
        for direction in ref.DIRECTIONS:
            cc = ref.conditioned_case(*shape, direction)                       # such a seed exists
            assert max(ref.backward(cc)["cond"].values()) <= ref.MAX_COND and cc["shape"] == shape


@directions
@pytest.mark.parametrize("mask", ["ragged", None])
def test_lstm_graph_in_fp64_on_the_cpu_is_the_reference(direction, mask):
    case = ref.make_case(4, 6, 8, 12, direction, seed=4, mask=mask)
    t = {k: torch.tensor(case[k], requires_grad=True) for k in ("x",) + ref.PARAMS}
    m = None if mask is None else torch.tensor(case["mask"])
    hs = lstm_graph(t["x"], m, t["W"], t["U"], t["b"], direction=direction)
    last = lstm_graph(t["x"], m, t["W"], t["U"], t["b"], direction=direction, return_sequences=False)
    ((hs * torch.tensor(case["g_hs"])).sum() + (last * torch.tensor(case["g_last"])).sum()).backward()
    want, bwd = ref.forward(case), ref.backward(case)
    assert ref.norm_rel(hs.detach().numpy(), want) < 1e-12 and ref.norm_rel(last.detach().numpy(), ref.last_of(want, direction)) < 1e-12
    for k in ref.GRADS:
        assert ref.norm_rel(t[k[1:]].grad.numpy(), bwd[k]) < 1e-12, k


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.LSTMLayer is layers.behavior_layer.LSTMLayer and layers.BiLSTMLayer is layers.behavior_layer.BiLSTMLayer
    assert "LSTMLayer" in layers.__all__ and "BiLSTMLayer" in layers.__all__
    E = inspect.Parameter.empty
    assert _sig(layers.LSTMLayer.__init__) == dict(units=E, return_sequences=True, go_backwards=False, seed=2020)
    assert _sig(layers.BiLSTMLayer.__init__) == dict(units=E, merge_mode="concat", return_sequences=True, seed=2020)
    assert _sig(models.DSIN.__init__) == dict(sess_count=E, att_heads=2, att_hidden_units=(80, 40), ffn_units=None, hidden_units=None,
                                              seed=2020)
    s = _sig(Fn.lstm)
    assert list(s) == ["x", "mask", "W", "U", "b", "direction", "return_sequences"] and s["direction"] == "forward"
    assert s["return_sequences"] is True and list(_sig(Fn.lstm_plan)) == ["B", "T", "K", "H", "direction"]
    m = models.DSIN(3)
    assert isinstance(m, models._BehaviorModel) and isinstance(m.dnn, layers.DnnLayer) and isinstance(m.score, layers.MergeScoreLayer)
    assert isinstance(m.stack, layers.StackLayer)
    assert layers.LSTMLayer(4).direction == "forward" and layers.LSTMLayer(4, go_backwards=True).direction == "reverse"
    with pytest.raises(ValueError, match="units"):
        layers.LSTMLayer(0)
    with pytest.raises(ValueError, match="units"):
        layers.BiLSTMLayer(0)
    with pytest.raises(ValueError, match="merge_mode"):
        layers.BiLSTMLayer(8, merge_mode="mul")
    with pytest.raises(ValueError, match="sess_count"):
        models.DSIN(0)
    with pytest.raises(ValueError, match="direction"):
        Fn.lstm(torch.zeros(1, 1, 4), None, torch.zeros(4, 16), torch.zeros(4, 16), torch.zeros(16), direction="backward")


def test_state_dict_names_shapes_and_initialisers():
    K, T, H = 8, 5, 12
    layer = layers.LSTMLayer(H)
    layer.build((2, T, K))
    sd = layer.state_dict()
    assert list(sd) == ["kernel", "recurrent_kernel", "bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(K, 4 * H), (H, 4 * H), (4 * H,)]
    assert 0 < float(sd["kernel"].abs().max()) <= np.sqrt(6.0 / (K + 4 * H))
    u = sd["recurrent_kernel"].double().numpy()
    assert np.abs(u @ u.T - np.eye(H)).max() < 1e-6
    assert torch.equal(sd["recurrent_kernel"], base.Layer().add_weight("w", (H, 4 * H), "orthogonal", seed=2020))   # the existing initialiser
    want_bias = torch.zeros(4 * H)
    want_bias[H:2 * H] = 1.0                                                    # unit_forget_bias
    assert torch.equal(sd["bias"], want_bias)
    back = layers.LSTMLayer(H, go_backwards=True)
    back.build((2, T, K))
    assert all(torch.equal(v, back.state_dict()[n]) for n, v in sd.items())
    bi = layers.BiLSTMLayer(H, merge_mode="ave")
    bi.build((2, T, K))
    sb = bi.state_dict()
    assert list(sb) == ["forward_kernel", "forward_recurrent_kernel", "forward_bias", "backward_kernel", "backward_recurrent_kernel",
                        "backward_bias"]
    assert [tuple(v.shape) for v in sb.values()] == [(K, 4 * H), (H, 4 * H), (4 * H,)] * 2
    assert torch.equal(sb["forward_kernel"], sd["kernel"]) and torch.equal(sb["forward_recurrent_kernel"], sd["recurrent_kernel"])
    assert not torch.equal(sb["backward_kernel"], sb["forward_kernel"])
    ub = sb["backward_recurrent_kernel"].double().numpy()
    assert np.abs(ub @ ub.T - np.eye(H)).max() < 1e-6
    assert torch.equal(sb["forward_bias"], want_bias) and torch.equal(sb["backward_bias"], want_bias)
    assert all(p.requires_grad for p in bi.parameters())


def test_layer_shape_and_mask_validation():
    x = torch.zeros(3, 5, 8)
    for layer in (layers.LSTMLayer(4), layers.BiLSTMLayer(4)):
        with pytest.raises(ValueError, match=r"\[B,T,K\]"):
            layer(torch.zeros(3, 8))
        with pytest.raises(ValueError, match="mask must be"):
            layer(x, mask=torch.ones(3, 4, dtype=torch.bool))
        with pytest.raises(ValueError, match="mask must be"):
            layer(x, mask=torch.ones(3, 5))


def test_no_cpu_fallback():
    x, mask = torch.zeros(3, 5, 8), torch.ones(3, 5, dtype=torch.bool)
    w = [torch.zeros(8, 16), torch.zeros(4, 16), torch.zeros(16)]
    with pytest.raises(FilError, match="GPU only"):
        Fn.lstm(x, mask, *w)
    with pytest.raises(FilError, match="GPU only"):
        Fn.lstm(x, None, *[torch.stack([t, t]) for t in w], direction="bidirectional", return_sequences=False)
    with pytest.raises(FilError, match="GPU only"):
        layers.LSTMLayer(4)(x, mask=mask)
    with pytest.raises(FilError, match="GPU only"):
        layers.BiLSTMLayer(4, merge_mode="sum")(x)
    with pytest.raises(FilError, match="GPU only"):
        layers.BiLSTMLayer(68)(x)                                    # outside the menu: the composed path
    with pytest.raises(FilError, match="GPU only"):
        layers.LSTMLayer(4)(torch.zeros(3, 5, 6))


def test_dsin_needs_sessions_of_one_length():
    """T = 10 is not 3 sessions: ValueError on the first call, before anything runs."""
    K, T, B = 8, 10, 2
    info = models.make_sparse_info([12, 5], embed_dim=K, names=["item", "user"])
    fea = models.InputFeature(None, info, [(0, T)], [], [], [], None, [torch.zeros(B, 1, K), torch.zeros(B, 1, K)],
                              [[torch.zeros(B, T, K)], [torch.ones(B, T, dtype=torch.bool)]])
    with pytest.raises(ValueError, match="sess_count=3"):
        models.DSIN(3)(fea)
    with pytest.raises(ValueError, match="att_heads=3"):
        models.DSIN(5, att_heads=3)(fea)
