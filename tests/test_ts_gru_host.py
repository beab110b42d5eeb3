"""Host-only checks of the time-stream GRU (include/fil.h N5 fil_tsgru_*, functional.ts_gru, layers.TimeStreamGRULayer,
models.DTSInput / DTS): the entry points in the header, the binding and the library; their argument validation, the menu with the
corners the LDS limit leaves out and the plan's arithmetic through ctypes; the Python surface that needs no GPU; self-checks of the
fp64 restatement (tests/ts_gru_ref.py) the GPU tests are held to; and the condition their cases have to meet (tests/ts_gru_cases.py)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import gru_ref
from tests import ts_gru_cases as cases
from tests import ts_gru_ref as ref

NEW = ("fil_tsgru_plan", "fil_tsgru_saved_bytes", "fil_tsgru_fwd", "fil_tsgru_bwd_workspace_bytes", "fil_tsgru_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
GRID_CAP = 1024
DIMS = (3, 4, 8, 2)        # T, K, H, S of the small shape


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, H, S):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_tsgru_plan(B, T, K, H, S, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def test_tsgru_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_tsgru_plan"] == (I, [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_tsgru_saved_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_tsgru_fwd"] == (I, [P] * 12 + [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_tsgru_bwd_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_tsgru_bwd"] == (I, [P] * 18 + [Z] + [I] * 5 + [P])


# positions:  fwd: x dt dt_out mask W U b Wf bf hs z saved
#             bwd: x dt dt_out mask W U Wf saved g_hs g_last g_z | dx dW dU db dWf dbf | workspace
def test_tsgru_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_tsgru_fwd(*([None] * 12), 0, *DIMS, None) == OK
    assert lib.fil_tsgru_bwd(*([None] * 18), 0, 0, *DIMS, None) == OK
    # NULL tensors with B > 0: x, dt, W, U, b, Wf, bf, hs are required (mask = NULL is all live, saved = NULL the inference call)
    for hole in (0, 1, 4, 5, 6, 7, 8, 9):
        args = [p] * 12
        args[hole] = None
        assert lib.fil_tsgru_fwd(*args, 5, *DIMS, None) == ERR_ARG, hole
        assert "fil_tsgru_fwd" in _msg(lib)
    # dt_out and z: both or neither
    for hole in (2, 10):
        args = [p] * 12
        args[hole] = None
        assert lib.fil_tsgru_fwd(*args, 5, *DIMS, None) == ERR_ARG, hole
    for hole in (0, 1, 4, 5, 6, 7):
        args = [p] * 18
        args[hole] = None
        assert lib.fil_tsgru_bwd(*args, 1 << 20, 5, *DIMS, None) == ERR_ARG, hole
        assert "fil_tsgru_bwd" in _msg(lib)
    none = [p] * 18
    none[8] = none[9] = none[10] = None
    assert lib.fil_tsgru_bwd(*none, 1 << 20, 5, *DIMS, None) == ERR_ARG               # no upstream gradient
    gz = [p] * 18
    gz[2] = None
    assert lib.fil_tsgru_bwd(*gz, 1 << 20, 5, *DIMS, None) == ERR_ARG                 # g_z without dt_out
    assert lib.fil_tsgru_bwd(*([p] * 11 + [None] * 6 + [p]), 1 << 20, 5, *DIMS, None) == ERR_ARG     # nothing to compute
    # a wrong sign; S = 0 is an argument error, S = 9 is outside the menu; K % 4
    for dims in ((-1, 3, 4, 8, 2), (5, 0, 4, 8, 2), (5, 3, 0, 8, 2), (5, 3, 4, 0, 2), (5, 3, 4, 8, 0), (5, 3, 4, 8, -1)):
        assert lib.fil_tsgru_fwd(*([p] * 12), *dims, None) == ERR_ARG, dims
        assert lib.fil_tsgru_bwd(*([p] * 18), 1 << 20, *dims, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    for dims, word in (((5, 3, 4, 8, 9), "S=9"), ((5, 3, 6, 8, 2), "K=6"), ((5, 3, 4, 6, 2), "H=6"), ((5, 3, 68, 8, 2), "K=68"),
                       ((5, 3, 4, 68, 2), "H=68")):
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and "fil_tsgru_plan" in _msg(lib), (_msg(lib), word)
        assert lib.fil_tsgru_fwd(*([p] * 12), *dims, None) == ERR_UNSUPPORTED
        assert lib.fil_tsgru_bwd(*([p] * 18), 1 << 20, *dims, None) == ERR_UNSUPPORTED
        assert lib.fil_tsgru_bwd_workspace_bytes(*dims) == 0 and lib.fil_tsgru_saved_bytes(*dims) == 0
    # the first fault answers: a wrong sign in front of the menu, the menu in front of the NULLs
    assert lib.fil_tsgru_fwd(*([None] * 12), 5, 0, 6, 8, 9, None) == ERR_ARG
    assert lib.fil_tsgru_fwd(*([None] * 12), 5, 3, 6, 8, 2, None) == ERR_UNSUPPORTED
    assert lib.fil_tsgru_plan(5, *DIMS, None) == ERR_ARG
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
    need = lib.fil_tsgru_bwd_workspace_bytes(5, *DIMS)
    assert need > 0
    assert lib.fil_tsgru_bwd(*([p] * 18), need - 1, 5, *DIMS, None) == ERR_ARG
    assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_tsgru_bwd" in _msg(lib)
    args = [p] * 18
    args[17] = None
    assert lib.fil_tsgru_bwd(*args, need, 5, *DIMS, None) == ERR_ARG


def _layout(B, K, H):
    """rnn_tile.h's tile for (B, K, H) and the LDS bytes of both passes, restated: fil_gru_*'s sections with the scores' places (dt
    takes them), then Wf | bf | two state images in the forward, Wf^T | two substep images (h_s^T, q^T, q) in the backward."""
    quad = max(H, K // 4)
    g_max = 256 // quad
    g_low = max(min(g_max, -(-64 // quad)), -(-(K + H) // 32))
    g = min(g_max, max(g_low, -(-B // (4 * GRID_CAP))))
    tile = 4 * g
    nsp = tile + 4
    lds_f = 4 * ((K + H) * 3 * H + 6 * H + 2 * (K + H) * nsp + 4 * tile) + 4 * (H * H + H + 2 * H * nsp)
    lds_b = 4 * ((K + H) * 3 * H + 2 * (K + H) * nsp + 4 * H * nsp + tile * 4 * H + H * nsp + 4 * tile) + 4 * (H * H + 2 * (2 * H * nsp + tile * H))
    return tile, lds_f, lds_b


def test_tsgru_plan_arithmetic(lib):
    for T, K, H, S in ((1, 4, 4, 1), (3, 4, 8, 2), (50, 16, 16, 2), (7, 12, 20, 1), (40, 8, 4, 8), (5, 64, 4, 2), (5, 4, 64, 2), (50, 32, 32, 3)):
        for B in (0, 1, 15, 16, 17, 4096, GRID_CAP * 64 + 1, 1 << 22):
            tile, lds_f, lds_b = _layout(B, K, H)
            rc, (fwd_ok, bwd_ok, ptile, grid, cap, parts, plf, plb) = _plan(lib, B, T, K, H, S)
            assert rc == OK and fwd_ok == 1 and bwd_ok == 1 and cap == GRID_CAP, (B, T, K, H, S)
            assert ptile == tile and (plf, plb) == (lds_f, lds_b)
            want_grid = min(-(-B // tile), cap)
            assert grid == want_grid and parts == want_grid
            # one partial = dW | dU | db | dWf | dbf, fp32; saved = the GRU's four planes and (h_s, f_s) per substep of every step, then
            # the final evolution's pairs; both rounded up to 256 bytes
            n_out = (K + H + 2) * 3 * H + H * H + H
            assert lib.fil_tsgru_bwd_workspace_bytes(B, T, K, H, S) == -(-(parts * n_out * 4) // 256) * 256
            assert lib.fil_tsgru_saved_bytes(B, T, K, H, S) == -(-((B * T * (4 + 2 * S) + B * 2 * S) * H * 4) // 256) * 256
        # the plan depends neither on T nor on S: no section of the layout does
        assert _plan(lib, 77, T, K, H, S) == _plan(lib, 77, T + 1, K, H, 1) == _plan(lib, 77, 1, K, H, 8)
    assert Fn.ts_gru_plan(8, 50, 16, 16)["fits"] and Fn.ts_gru_plan(8, 50, 16, 16, 4)["tile"] == 16
    assert Fn.ts_gru_plan(8, 50, 6, 16) == dict(fits=False) == Fn.ts_gru_plan(8, 50, 16, 68) == Fn.ts_gru_plan(8, 50, 16, 16, 9)
    with pytest.raises(FilError):
        Fn.ts_gru_plan(8, 0, 16, 16)
    with pytest.raises(ValueError, match="steps"):
        Fn.ts_gru_plan(8, 5, 16, 16, 0)


def test_tsgru_menu_walk_pins_the_corners_the_lds_limit_leaves_out(lib):
    """Every (K, H) of the menu at a small, a middling and a large batch (the tile grows with B, and the LDS with it): the plan's
    answer is the restated arithmetic's, and the pairs that fall out are pinned."""
    out = {1: set(), 4096: set(), 1 << 20: set()}
    for K in range(4, 65, 4):
        for H in range(4, 65, 4):
            for B in out:
                tile, lds_f, lds_b = _layout(B, K, H)
                fits = max(lds_f, lds_b) <= LDS_LIMIT
                answers = {_plan(lib, B, 100000, K, H, S)[0] for S in (1, 2, 8)}
                assert answers == {OK if fits else ERR_UNSUPPORTED}, (B, K, H, answers)
                if fits:
                    pl = _plan(lib, B, 100000, K, H, 2)[1]
                    assert pl[0] == 1 and pl[1] == 1 and 0 < pl[6] <= pl[7] <= LDS_LIMIT
                else:
                    out[B].add((K, H))
                    assert str(LDS_LIMIT) in _msg(lib) and "LDS" in _msg(lib)
                    assert lib.fil_tsgru_saved_bytes(B, 5, K, H, 2) == 0
    # the backward beside Wf^T and the substep images decides.  H <= 52 is in whatever K and B.  H = 56: K >= 52 is out; H = 60: K >= 40,
    # at the large batch's tile of 16 samples K >= 36; H = 64: K >= 36, at the large batch K >= 20.  The largest square is 52.
    low = lambda B, H: min([K for K, h in out[B] if h == H], default=None)
    assert {H for B in out for _, H in out[B]} == {56, 60, 64}
    assert out[1] == out[4096] <= out[1 << 20]
    assert [low(1, H) for H in (56, 60, 64)] == [52, 40, 36] and [low(1 << 20, H) for H in (56, 60, 64)] == [52, 36, 20]
    assert all((K2, H) in out[B] for B in out for K, H in out[B] for K2 in range(K, 65, 4))          # out from some K upwards
    assert (52, 52) not in out[1 << 20] and (56, 56) in out[1] and (64, 64) in out[1]
    assert cases.largest_square() == 52
    assert _plan(lib, 3, 6, 52, 52, 2)[1][7] == 150016


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_backward_equals_fp64_autograd():
    for shape, grads, out in (((3, 3, 4, 4, 1), ("hs", "last", "z"), True), ((4, 9, 8, 12, 3), ("hs",), False), ((2, 5, 4, 16, 2), ("last",), True),
                              ((3, 4, 8, 4, 8), ("z",), True), ((1, 1, 4, 4, 2), ("last", "z"), True)):
        m = ref.make_mask(shape[0], shape[1], "ragged", np.random.default_rng(5))
        if shape[0] > 1:
            m[1] = 0
        case = ref.make_case(*shape, seed=3, mask=m, grads=grads, out=out)
        auto = ref.torch_run(case, torch.float64)
        hand = ref.backward(case)
        hs, z = ref.forward(case)
        assert np.abs(auto["hs"] - hs).max() < 1e-12 and (z is None) == (not out)
        if out:
            assert np.abs(auto["z"] - z).max() < 1e-12
        if shape[0] > 1:
            assert not hs[1].any() and not hand["dx"][1].any()       # the all-masked sample
            if out:
                assert z[1].any() or case["dt_out"][1] == 0          # ... still moves from zero to the prediction time
        for k in ref.GRADS:
            assert np.abs(auto[k].reshape(hand[k].shape) - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)
        assert not hand["dx"][m == 0].any()
        assert np.abs(hand["dWf"]).max() > 0 and np.abs(hand["dbf"]).max() > 0


def test_reference_backward_equals_central_differences():
    case = ref.conditioned_case(3, 3, 4, 4, 2)
    hand = ref.backward(case)

    def loss(c):
        hs, z = ref.forward(c)
        return (hs * c["g_hs"]).sum() + (hs[:, -1] * c["g_last"]).sum() + (z * c["g_z"]).sum()

    eps = 1e-6
    for k in ("x",) + ref.PARAMS:
        num = np.zeros_like(case[k])
        for i in np.ndindex(*case[k].shape):
            hi, lo = case[k].copy(), case[k].copy()
            hi[i] += eps
            lo[i] -= eps
            num[i] = (loss(dict(case, **{k: hi})) - loss(dict(case, **{k: lo}))) / (2 * eps)
        live = case["mask"].astype(bool)[:, :, None] if k == "x" else True
        assert np.abs(np.where(live, num, 0.0) - hand["d" + k]).max() < 1e-7 * max(1.0, np.abs(hand["d" + k]).max()), k


def test_reference_exact_cases():
    case = ref.make_case(4, 6, 8, 4, 3, seed=1)
    B, T = 4, 6
    gru_case = dict(mode="gru", a=None, **{k: case[k] for k in ("x", "mask", "W", "U", "b", "g_hs")})
    gru_case["g_last"] = case["g_last"] + case["g_z"]                    # z is the last state: its gradient joins g_last
    # dt = 0 and dt_out = 0: gru_ref's GRU exactly, whatever Wf
    still = dict(case, dt=np.zeros((B, T)), dt_out=np.zeros(B))
    hs, z = ref.forward(still)
    assert np.array_equal(hs, gru_ref.forward(gru_case)) and np.array_equal(z, hs[:, -1])
    bw, gbw = ref.backward(still), gru_ref.backward(gru_case)
    for k in ("dx", "dW", "dU", "db"):
        assert np.array_equal(bw[k], gbw[k]), k
    assert not bw["dWf"].any() and not bw["dbf"].any()
    # Wf = 0 and bf = 0: likewise for any dt
    flat = dict(case, Wf=np.zeros((4, 4)), bf=np.zeros(4))
    hs, z = ref.forward(flat)
    assert np.array_equal(hs, gru_ref.forward(gru_case)) and np.array_equal(z, hs[:, -1])
    # a masked step carries
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0
    m[:, 4] = 0
    hs, _ = ref.forward(dict(case, mask=m))
    assert not hs[:, :2].any() and np.array_equal(hs[:, 4], hs[:, 3]) and hs[:, 2].any()
    # ... and its x and dt are never used
    hs2, _ = ref.forward(dict(case, mask=m, x=np.where(m[:, :, None] != 0, case["x"], 7.0), dt=np.where(m != 0, case["dt"], 9.0)))
    assert np.array_equal(hs, hs2)
    # the gaps matter
    assert not np.array_equal(ref.forward(case)[0], ref.forward(dict(case, dt=case["dt"] * 0.5))[0])


def test_cases_meet_the_condition_the_bars_rest_on():
    c = ref.make_case(7, 50, 16, 36, 2, seed=0)
    for k in ("x", "dt", "dt_out", "g_hs", "g_last", "g_z") + ref.PARAMS:
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    assert c["dt"].shape == (7, 50) and c["dt_out"].shape == (7,) and c["Wf"].shape == (36, 36) and c["bf"].shape == (36,)
    assert (c["dt"] >= 0).all() and (c["dt"] <= 2).all() and (c["dt"] == 0).any() and (c["dt"] > 0).any()
    assert ref.make_case(2, 3, 4, 4, 1, seed=0, out=False)["dt_out"] is None
    todo = list(cases.parity_cases(52)) + [cases.large_case()] + [cases.edge_case(B) for B in (5, 31, 32, 33)]
    for case in todo:
        _, _, bwd, e32 = ref.reference(case)
        assert all(np.isfinite(v) for v in e32.values()), (case["shape"], e32)
        assert max(ref.bars(e32).values()) < 1e-3, (case["shape"], e32)
    for B in (5, 31, 32, 33):
        assert max(ref.backward(cases.edge_case(B))["cond"].values()) <= ref.MAX_COND == gru_ref.MAX_COND


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.TimeStreamGRULayer is layers.behavior_layer.TimeStreamGRULayer and "TimeStreamGRULayer" in layers.__all__
    assert _sig(layers.TimeStreamGRULayer.__init__) == dict(units=inspect.Parameter.empty, steps=2, return_sequences=False, seed=2020)
    assert _sig(models.DTS.__init__) == dict(steps=2, hidden_units=None, seed=2020)
    s = _sig(Fn.ts_gru)
    assert list(s) == ["x", "dt", "dt_out", "mask", "W", "U", "b", "Wf", "bf", "steps", "return_sequences"]
    assert s["steps"] == 2 and s["return_sequences"] is True and _sig(Fn.ts_gru_graph) == s
    assert list(_sig(Fn.ts_gru_plan)) == ["B", "T", "K", "H", "steps"]
    m = models.DTS()
    assert isinstance(m.dnn, layers.DnnLayer) and isinstance(m.score, layers.MergeScoreLayer) and isinstance(m.stack, layers.StackLayer)
    assert issubclass(models.DTSInput, models.DINInput)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="steps"):
            layers.TimeStreamGRULayer(8, steps=bad)
        with pytest.raises(ValueError, match="steps"):
            models.DTS(steps=bad)
    with pytest.raises(ValueError, match="units"):
        layers.TimeStreamGRULayer(0)


def test_state_dict_names_shapes_and_initialisers():
    K, T, H = 8, 5, 12
    layer = layers.TimeStreamGRULayer(H)
    layer.build([(2, T, K), (2, T), (2,)])
    sd = layer.state_dict()
    assert list(sd) == ["kernel", "recurrent_kernel", "bias", "ode_kernel", "ode_bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(K, 3 * H), (H, 3 * H), (2, 3 * H), (H, H), (H,)]
    gru = layers.GRULayer(H)
    gru.build((2, T, K))
    assert all(torch.equal(v, sd[n]) for n, v in gru.state_dict().items())          # GRULayer's weights under its names
    assert 0 < float(sd["ode_kernel"].abs().max()) <= np.sqrt(6.0 / (2 * H)) and not sd["ode_bias"].any()


def test_layer_asks_the_plan_at_its_batch():
    """The menu's LDS corners depend on the batch (the tile grows with it): the layer's answer, asked at the batch rounded up to the
    tile's step, is the plan's at the batch itself."""
    for K, H in ((16, 16), (20, 64), (36, 60), (36, 64), (52, 52), (56, 56), (6, 8)):
        layer = layers.TimeStreamGRULayer(H)
        for B in (0, 1, 4096, 4097, 3 * 4096, 12289, 16384, 16385, 1 << 20):
            assert layer.fits_kernel_menu(torch.empty(B, 1, K, device="meta")) == Fn.ts_gru_plan(B, 1, K, H, 2)["fits"], (K, H, B)
    assert not layers.TimeStreamGRULayer(8, steps=9).fits_kernel_menu(torch.empty(2, 1, 8, device="meta"))
    assert layers.TimeStreamGRULayer(64).fits_kernel_menu(torch.empty(4096, 1, 20, device="meta"))
    assert not layers.TimeStreamGRULayer(64).fits_kernel_menu(torch.empty(16384, 1, 20, device="meta"))


def test_composed_path_is_the_reference():
    """ts_gru_graph runs on the tensors given: on the CPU in float64 it is the restatement, forward and (by autograd) backward."""
    case = ref.make_case(4, 6, 8, 12, 3, seed=2)
    t = {k: torch.tensor(case[k], requires_grad=True) for k in ("x",) + ref.PARAMS}
    mask = torch.tensor(case["mask"].astype(bool))
    dt, dt_out = torch.tensor(case["dt"]), torch.tensor(case["dt_out"])
    hs, z = Fn.ts_gru_graph(t["x"], dt, dt_out, mask, *(t[k] for k in ref.PARAMS), steps=3)
    hs_ref, z_ref = ref.forward(case)
    assert np.abs(hs.detach().numpy() - hs_ref).max() < 1e-6 and np.abs(z.detach().numpy() - z_ref).max() < 1e-6       # (fp64 division here)
    ((hs * torch.tensor(case["g_hs"])).sum() + (hs[:, -1] * torch.tensor(case["g_last"])).sum() + (z * torch.tensor(case["g_z"])).sum()).backward()
    bwd = ref.backward(case)
    for k in ("x",) + ref.PARAMS:
        assert ref.norm_rel(t[k].grad.numpy(), bwd["d" + k]) < 1e-6, k
    last, z2 = Fn.ts_gru_graph(t["x"], dt, dt_out, mask, *(t[k] for k in ref.PARAMS), steps=3, return_sequences=False)
    assert torch.equal(last, hs[:, -1]) and torch.equal(z2, z)
    assert torch.equal(Fn.ts_gru_graph(t["x"], dt, None, mask, *(t[k] for k in ref.PARAMS), steps=3), hs)


def test_layer_and_input_validation_and_no_cpu_fallback():
    x, dt, dt_out = torch.zeros(3, 5, 8), torch.zeros(3, 5), torch.zeros(3)
    layer = layers.TimeStreamGRULayer(4)
    with pytest.raises(ValueError, match=r"\[x, dt, dt_out or None\]"):
        layer(x)
    with pytest.raises(ValueError, match=r"\[B,T,K\]"):
        layer([torch.zeros(3, 8), dt, None])
    with pytest.raises(ValueError, match="dt must be"):
        layer([x, torch.zeros(3, 4), None])
    with pytest.raises(ValueError, match="dt must be"):
        layer([x, dt, torch.zeros(4)])
    with pytest.raises(ValueError, match="mask must be"):
        layer([x, dt, dt_out], mask=torch.ones(3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="no gradient"):
        layer([x, dt.clone().requires_grad_(), None])
    with pytest.raises(ValueError, match="no gradient"):
        Fn.ts_gru(x, dt, dt_out.clone().requires_grad_(), None, *[torch.zeros(s) for s in ((8, 12), (4, 12), (2, 12), (4, 4), (4,))])
    w = [torch.zeros(8, 12), torch.zeros(4, 12), torch.zeros(2, 12), torch.zeros(4, 4), torch.zeros(4)]
    with pytest.raises(FilError, match="GPU only"):
        Fn.ts_gru(x, dt, dt_out, None, *w)
    with pytest.raises(FilError, match="GPU only"):
        layer([x, dt, dt_out])
    with pytest.raises(FilError, match="GPU only"):
        layers.TimeStreamGRULayer(68)([x, dt, None])                 # outside the menu: the composed path
    with pytest.raises(FilError, match="GPU only"):
        layers.TimeStreamGRULayer(4, steps=9)([x, dt, None])
    # DTSInput's shape checks come before anything touches the GPU
    info = models.make_sparse_info([12, 5], embed_dim=8, names=["item", "user"])
    inp = models.DTSInput(info, behavior=[("item", 5)])
    idx, hist = torch.ones(3, 2, dtype=torch.int64), torch.ones(3, 1, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="hist_idx, hist_dt, next_dt"):
        inp.call((None, idx, hist))
    with pytest.raises(ValueError, match="hist_dt must be"):
        inp.call((None, idx, (hist, torch.zeros(3, 1, 4), torch.zeros(3, 1))))
    with pytest.raises(ValueError, match="hist_dt must be"):
        inp.call((None, idx, (hist, torch.zeros(3, 1, 5), torch.zeros(3, 2))))
    with pytest.raises(ValueError, match="hist_dt must be"):
        inp.call((None, idx, (hist, torch.zeros(3, 1, 5, dtype=torch.int64), torch.zeros(3, 1))))
    with pytest.raises(ValueError, match="required"):
        inp.call((None, idx, (hist, None, torch.zeros(3, 1))))
    with pytest.raises(ValueError, match="no gaps"):
        models.DTS()(models.InputFeature(seqEmbedList=[[], []]))
