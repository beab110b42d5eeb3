"""Host-only checks of the Neural Turing Machine memory read / write over a sequence (include/fil.h N4 fil_ntm_*,
functional.ntm_memory, layers.NTMMemoryLayer, models.MIMN): the entry points in the header, the binding and the library; their
argument validation, the menu limits and the plan's arithmetic through ctypes; the Python surface that needs no GPU; the composed
graph on the CPU; and self-checks of the fp64 restatement (tests/ntm_ref.py) the GPU tests are held to.  Shapes are (B, T, H, m, D)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from ml_function_amd.layers import behavior_layer
from tests import gru_ref
from tests import ntm_ref as ref

NEW = ("fil_ntm_plan", "fil_ntm_saved_bytes", "fil_ntm_fwd", "fil_ntm_bwd_workspace_bytes", "fil_ntm_bwd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
GRID_CAP = 1024
DIMS = (3, 8, 2, 4)        # T, H, m, D of the small shape


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, H, m, D):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_ntm_plan(B, T, H, m, D, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def test_ntm_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_ntm_plan"] == (I, [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_ntm_saved_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_ntm_fwd"] == (I, [P] * 9 + [I] * 5 + [P])
    assert _lib.SIGNATURES["fil_ntm_bwd_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["fil_ntm_bwd"] == (I, [P] * 12 + [Z] + [I] * 5 + [P])


# positions:  fwd: h mask Wp bp M0 | rs r_last MT | saved        bwd: h mask Wp saved | g_rs g_last g_M | dh dWp dbp dM0 | workspace
def test_ntm_argument_validation(lib):
    p = 4096          # any non-NULL address: every call below returns before a pointer is followed
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_ntm_fwd(*([None] * 9), 0, *DIMS, None) == OK
    assert lib.fil_ntm_bwd(*([None] * 12), 0, 0, *DIMS, None) == OK
    # NULL tensors with B > 0: h, Wp, bp, M0 are required (saved = NULL is the inference call and mask = NULL all live: launches,
    # which the GPU tests make)
    for hole in (0, 2, 3, 4):
        args = [p] * 9
        args[hole] = None
        assert lib.fil_ntm_fwd(*args, 5, *DIMS, None) == ERR_ARG, hole
        assert "fil_ntm_fwd" in _msg(lib)
    assert lib.fil_ntm_fwd(*([p] * 5 + [None] * 3 + [p]), 5, *DIMS, None) == ERR_ARG          # no output at all
    for hole in (0, 2, 3):
        args = [p] * 12
        args[hole] = None
        assert lib.fil_ntm_bwd(*args, 1 << 20, 5, *DIMS, None) == ERR_ARG, hole
        assert "fil_ntm_bwd" in _msg(lib)
    assert lib.fil_ntm_bwd(*([p] * 4 + [None] * 3 + [p] * 5), 1 << 20, 5, *DIMS, None) == ERR_ARG      # no upstream gradient
    assert lib.fil_ntm_bwd(*([p] * 7 + [None] * 4 + [p]), 1 << 20, 5, *DIMS, None) == ERR_ARG          # nothing to compute
    # non-positive dimensions
    for dims in ((-1, 3, 8, 2, 4), (5, 0, 8, 2, 4), (5, 3, 0, 2, 4), (5, 3, 8, 0, 4), (5, 3, 8, 2, 0)):
        assert lib.fil_ntm_fwd(*([p] * 9), *dims, None) == ERR_ARG, dims
        assert lib.fil_ntm_bwd(*([p] * 12), 1 << 20, *dims, None) == ERR_ARG, dims
        assert _plan(lib, *dims)[0] == ERR_ARG
    assert lib.fil_ntm_plan(5, *DIMS, None) == ERR_ARG
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: -1 with the needed size in the message
    need = lib.fil_ntm_bwd_workspace_bytes(5, *DIMS)
    assert need > 0
    assert lib.fil_ntm_bwd(*([p] * 12), need - 1, 5, *DIMS, None) == ERR_ARG
    assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_ntm_bwd" in _msg(lib)
    args = [p] * 12
    args[11] = None
    assert lib.fil_ntm_bwd(*args, need, 5, *DIMS, None) == ERR_ARG


def test_ntm_menu_limits_from_both_sides(lib):
    p = 4096
    outside = (((5, 3, 6, 2, 4), "H=6", "<= 64"), ((5, 3, 68, 2, 4), "H=68", "<= 64"), ((5, 3, 8, 2, 6), "D=6", "<= 64"),
               ((5, 3, 8, 2, 68), "D=68", "<= 64"), ((5, 3, 8, 17, 4), "m=17", "<= 16"))
    for dims, word, limit in outside:
        assert _plan(lib, *dims)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and limit in _msg(lib) and "fil_ntm_plan" in _msg(lib), (_msg(lib), word)
        assert lib.fil_ntm_fwd(*([p] * 9), *dims, None) == ERR_UNSUPPORTED
        assert lib.fil_ntm_bwd(*([p] * 12), 1 << 20, *dims, None) == ERR_UNSUPPORTED
        assert lib.fil_ntm_bwd_workspace_bytes(*dims) == 0 and lib.fil_ntm_saved_bytes(*dims) == 0
    # the inner side of every limit, and every H, D of the menu with the fewest and the most slots, at a small and at a large batch
    # (the tile grows with B), any T.  The LDS limit excludes nothing: the largest shape stays inside it, the figures below.
    for dims in ((5, 3, 64, 2, 4), (5, 3, 8, 2, 64), (5, 3, 8, 16, 4), (5, 3, 4, 1, 4)):
        assert _plan(lib, *dims)[0] == OK, dims
    for H in range(4, 65, 4):
        for D in range(4, 65, 4):
            for m in (1, 16):
                for B in (1, 4096, 1 << 20):
                    rc, pl = _plan(lib, B, 100000, H, m, D)
                    assert rc == OK and pl[0] == 1 and pl[1] == 1, (H, m, D, _msg(lib))
                    assert 0 < pl[6] <= LDS_LIMIT and 0 < pl[7] <= LDS_LIMIT, (H, m, D, pl)
    big = _plan(lib, 1 << 20, 5, 64, 16, 64)[1]
    assert big[2] == 16 and (big[6], big[7]) == (129168, 128384)


def _layout(B, H, m, D):
    """The launcher's tile and thread arithmetic, restated."""
    lanes = D // 4
    per_sample = max(lanes, -(-H // 16))
    ns_max = 256 // per_sample
    ns_min = min(ns_max, -(-64 // per_sample))
    ns = min(ns_max, max(ns_min, -(-B // GRID_CAP)))
    threads = -(-ns * per_sample // 64) * 64
    blocks = (H // 4 + 1) * (D + 1)
    while -(-blocks // threads) > 5:
        threads += 64
    return lanes, ns, threads


def test_ntm_plan_arithmetic(lib):
    for T, H, m, D in ((1, 4, 1, 4), (3, 8, 2, 4), (50, 16, 4, 16), (7, 12, 3, 20), (300, 8, 16, 4), (6, 64, 16, 64), (5, 64, 1, 4),
                       (5, 4, 16, 64), (50, 32, 8, 32)):
        for B in (0, 1, 15, 16, 17, 4096, GRID_CAP * 256, GRID_CAP * 256 + 1, 1 << 22):
            rc, (fwd_ok, bwd_ok, tile, grid, cap, parts, lds_f, lds_b) = _plan(lib, B, T, H, m, D)
            assert rc == OK and fwd_ok == 1 and bwd_ok == 1 and cap == GRID_CAP
            lanes, ns, threads = _layout(B, H, m, D)
            assert tile == ns and threads <= 256, (B, T, H, m, D, tile)
            want_grid = min(-(-B // tile), cap)
            assert grid == want_grid and parts == want_grid
            # one partial = dWp | dbp | dM0, fp32; saved = M [m,D] | kr kw e a [4D] | 6 + 5m scalars padded to 4; rounded up to 256 bytes
            P = 4 * D + 2
            assert lib.fil_ntm_bwd_workspace_bytes(B, T, H, m, D) == -(-(parts * ((H + 1) * P + m * D) * 4) // 256) * 256
            step = m * D + 4 * D + -(-(6 + 5 * m) // 4) * 4
            assert lib.fil_ntm_saved_bytes(B, T, H, m, D) == -(-(B * T * step * 4) // 256) * 256
            r4 = lambda v: -(-v // 4) * 4
            assert lds_f == 4 * ((H + 1) * (P + 2) + 2 * tile * H + r4(2 * tile) + tile * (3 * m + 4) * lanes)
            assert lds_b == 4 * (r4(P * H) + 2 * tile * (H + 4) + r4(2 * tile) + tile * (P + 2) + r4(tile * 2 * m * lanes) + m * D)
        # the plan does not depend on T
        assert _plan(lib, 77, T, H, m, D) == _plan(lib, 77, T + 1, H, m, D)
    # past the grid cap a workgroup walks more than one tile
    rc, pl = _plan(lib, GRID_CAP * 256 + 1, 2, 4, 1, 4)
    assert pl[2] == 256 and pl[3] == GRID_CAP
    assert Fn.ntm_plan(8, 50, 16, 4, 16)["fits"] and Fn.ntm_plan(8, 50, 16, 4, 16)["tile"] == 16
    assert Fn.ntm_plan(8, 50, 6, 4, 16) == dict(fits=False) and Fn.ntm_plan(8, 50, 16, 17, 16) == dict(fits=False)
    with pytest.raises(FilError):
        Fn.ntm_plan(8, 0, 16, 4, 16)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("kind", ["ragged", "prefix", None])
@pytest.mark.parametrize("grads", ["both", "rs", "last", "M", "last+M"])
def test_reference_backward_equals_fp64_autograd(kind, grads):
    for shape in ((3, 3, 4, 2, 4), (4, 7, 8, 3, 12), (1, 1, 4, 1, 4)):
        m = ref.make_mask(shape[0], shape[1], kind, np.random.default_rng(5))
        if m is not None and shape[0] > 1:
            m[1] = 0
        case = ref.make_case(*shape, seed=3, mask=m, grads=grads)
        auto = ref.torch_run(case, torch.float64)
        hand = ref.backward(case)
        fwd = ref.forward(case)
        assert np.abs(auto["rs"] - fwd["rs"]).max() < 1e-12 and np.abs(auto["MT"] - fwd["MT"]).max() < 1e-12
        for k in ref.GRADS:
            assert np.abs(auto[k].reshape(hand[k].shape) - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (shape, k)
        if m is not None:
            assert not hand["dh"][m == 0].any()
            if shape[0] > 1:
                assert not fwd["rs"][1].any() and np.array_equal(fwd["MT"][1], case["M0"])      # the all-masked sample: zeros and M0


def test_reference_exact_cases():
    # m = 1: both weights are 1, the read is the previous row and the write is M (1 - e) + a
    case = ref.make_case(4, 5, 8, 1, 8, seed=1, mask=None)
    keep = ref._steps(case)["keep"]
    rs = ref.forward(case)["rs"]
    M = np.broadcast_to(case["M0"], (4, 1, 8))
    for t, s in enumerate(keep):
        assert np.array_equal(s["wr"], np.ones((4, 1))) and np.array_equal(s["ww"], np.ones((4, 1)))
        assert np.array_equal(rs[:, t], M[:, 0]) and np.array_equal(s["M"], M)
        M = M * (1.0 - s["e"][:, None, :]) + s["a"][:, None, :]
    assert np.array_equal(ref.forward(case)["MT"], M)
    # identical rows of M0 stay identical, the weights are 1 / m
    base = ref.make_case(5, 7, 16, 4, 16, seed=3)
    same = dict(base, M0=np.tile(base["M0"][:1], (4, 1)))
    p = ref._steps(same)
    for s in p["keep"]:
        assert np.array_equal(s["wr"], np.full((5, 4), 0.25)) and np.array_equal(s["ww"], np.full((5, 4), 0.25))
    assert all(np.array_equal(p["MT"][:, i], p["MT"][:, 0]) for i in range(1, 4))
    # an all-masked sample returns M0 and zeros, and sends g_M straight to dM0
    m = np.ones((5, 7), np.uint8)
    m[2] = 0
    fwd, bwd = ref.forward(dict(base, mask=m)), ref.backward(dict(base, mask=m))
    assert np.array_equal(fwd["MT"][2], base["M0"]) and not fwd["rs"][2].any() and not bwd["dh"][2].any()
    none = np.zeros((5, 7), np.uint8)
    assert np.array_equal(ref.backward(dict(base, mask=none))["dM0"], base["g_M"].sum(0))
    # masked steps carry the read
    m = np.ones((5, 7), np.uint8)
    m[:, :2] = 0
    m[:, 4] = 0
    rs = ref.forward(dict(base, mask=m))["rs"]
    assert not rs[:, :2].any() and np.array_equal(rs[:, 4], rs[:, 3]) and rs[:, 2].any()
    # the last read's gradient is the sequence gradient that is zero except at T - 1
    last = ref.make_case(5, 7, 16, 4, 16, seed=3, grads="last+M")
    g_rs = np.zeros((5, 7, 16))
    g_rs[:, -1] = last["g_last"]
    one, two = ref.backward(last), ref.backward(dict(last, g_rs=g_rs, g_last=None))
    for k in ref.GRADS:
        assert np.array_equal(one[k], two[k]), k
    # the cosine is smooth at a zero row and at a zero key
    zero = ref.make_case(5, 7, 16, 4, 16, seed=0, zero_row=True)
    assert not zero["M0"][0].any() and all(np.isfinite(v).all() for k, v in ref.backward(zero).items() if k != "cond")


SIZED_ON = ((3, 5, 8, 2, 4), (5, 7, 16, 4, 16), (9, 13, 32, 8, 32), (4, 50, 16, 4, 16), (3, 6, 64, 16, 64))


def test_make_case_draws_what_the_bars_were_sized_on():
    c = ref.make_case(7, 50, 16, 4, 36, seed=0)
    for k in ("h", "g_rs", "g_M") + ref.PARAMS:
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    assert c["h"].shape == (7, 50, 16) and c["Wp"].shape == (16, 146) and c["bp"].shape == (146,) and c["M0"].shape == (4, 36)
    assert c["mask"].shape == (7, 50) and c["g_rs"].shape == (7, 50, 36) and c["g_M"].shape == (7, 4, 36) and c["g_last"] is None
    assert 0.4 < c["h"].std() < 0.6 and 0.05 < c["M0"].std() < 0.15 and 0.05 < c["bp"].std() < 0.15
    assert abs(c["Wp"].std() / np.sqrt(2.0 / (16 + 146)) - 1) < 0.1
    assert ref.make_case(2, 3, 4, 2, 4, seed=0, grads="last")["g_M"] is None
    assert np.array_equal(ref.make_case(2, 3, 4, 2, 4, seed=0, scale=4.0)["h"], 4 * ref.make_case(2, 3, 4, 2, 4, seed=0)["h"])
    # the fp32 torch restatement's own error on the shapes the bars were sized on, plain seeds 0 .. 2: the 1e-5 floor binds, and
    # no sum over (b, t) is conditioned worse than gru_ref.MAX_COND -- read from the fp64 reference alone, so no seed is selected
    for shape in SIZED_ON:
        for seed in range(3):
            case = ref.make_case(*shape, seed)
            _, bwd, e32 = ref.reference(case)
            assert set(e32) == set(ref.OUTS + ref.GRADS), (shape, seed, e32)
            assert set(ref.bars(e32).values()) == {1e-5}, (shape, seed, e32)
            assert max(bwd["cond"].values()) <= gru_ref.MAX_COND, (shape, seed, bwd["cond"])
    for kw in (dict(zero_row=True), dict(scale=4.0)):
        _, bwd, e32 = ref.reference(ref.make_case(5, 7, 16, 4, 16, 0, **kw))
        assert set(ref.bars(e32).values()) == {1e-5} and max(bwd["cond"].values()) <= gru_ref.MAX_COND, (kw, e32)


# ------------------------------------------------------------------------------------------------ the composed graph
@pytest.mark.parametrize("seq", [True, False])
def test_composed_graph_on_the_cpu_in_fp64_equals_the_reference(seq):
    for kind in ("ragged", None):
        case = ref.make_case(4, 7, 8, 3, 12, seed=2, mask=kind, grads="both" if seq else "last+M")
        t = {k: torch.tensor(case[k], dtype=torch.float64, requires_grad=True) for k in ("h",) + ref.PARAMS}
        mask = None if case["mask"] is None else torch.tensor(case["mask"])          # uint8, as the layers pass it
        out, MT = behavior_layer.ntm_memory_graph(t["h"], mask, t["Wp"], t["bp"], t["M0"], return_sequences=seq)
        fwd, bwd = ref.forward(case), ref.backward(case)
        assert out.dtype == torch.float64 and out.shape == ((4, 7, 12) if seq else (4, 12)) and MT.shape == (4, 3, 12)
        assert np.abs(out.detach().numpy() - (fwd["rs"] if seq else fwd["rs"][:, -1])).max() < 1e-12
        assert np.abs(MT.detach().numpy() - fwd["MT"]).max() < 1e-12
        g = torch.tensor(case["g_rs"] if seq else case["g_last"])
        torch.autograd.backward([out, MT], [g, torch.tensor(case["g_M"])])
        for k in ("h",) + ref.PARAMS:
            assert np.abs(t[k].grad.numpy() - bwd["d" + k]).max() < 1e-12 * max(1.0, np.abs(bwd["d" + k]).max()), k
    f32 = behavior_layer.ntm_memory_graph(torch.zeros(2, 3, 8), None, torch.zeros(8, 18), torch.zeros(18), torch.ones(2, 4))[0]
    assert f32.dtype == torch.float32 and torch.equal(f32[:, 0], torch.ones(2, 4))     # equal rows: the first read is the row


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.NTMMemoryLayer is behavior_layer.NTMMemoryLayer and "NTMMemoryLayer" in layers.__all__
    assert _sig(layers.NTMMemoryLayer.__init__) == dict(memory_slots=4, memory_dim=None, return_sequences=False, seed=2020)
    assert _sig(models.MIMN.__init__) == dict(memory_slots=4, memory_dim=None, controller_units=None, hidden_units=None, seed=2020)
    s = _sig(Fn.ntm_memory)
    assert list(s) == ["h", "mask", "Wp", "bp", "M0", "return_sequences"] and s["return_sequences"] is True
    assert list(_sig(Fn.ntm_plan)) == ["B", "T", "H", "m", "D"]
    m = models.MIMN()
    assert isinstance(m, models._BehaviorModel) and isinstance(m.dnn, layers.DnnLayer) and isinstance(m.score, layers.MergeScoreLayer)
    assert isinstance(m.stack, layers.StackLayer)
    for bad in (dict(memory_slots=0), dict(memory_dim=0)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            layers.NTMMemoryLayer(**bad)
    for bad in (dict(memory_slots=0), dict(memory_dim=0), dict(controller_units=-1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            models.MIMN(**bad)


def test_state_dict_names_shapes_and_initialisers():
    H, T = 8, 5
    layer = layers.NTMMemoryLayer()
    layer.build((2, T, H))
    sd = layer.state_dict()
    assert list(sd) == ["read_write_kernel", "read_write_bias", "initial_memory"]
    assert [tuple(v.shape) for v in sd.values()] == [(H, 4 * H + 2), (4 * H + 2,), (4, H)]          # memory_dim=None: the input width
    assert 0 < float(sd["read_write_kernel"].abs().max()) <= np.sqrt(6.0 / (H + 4 * H + 2))
    assert not sd["read_write_bias"].any()
    M0 = sd["initial_memory"].double().numpy()
    assert 0.03 < M0.std() < 0.3 and all(not np.array_equal(M0[i], M0[j]) for i in range(4) for j in range(i))      # the rows differ
    again = layers.NTMMemoryLayer()
    again.build((2, T, H))
    assert all(torch.equal(v, again.state_dict()[n]) for n, v in sd.items())                        # the same seed, the same bits
    other = layers.NTMMemoryLayer(memory_slots=3, memory_dim=12, seed=7)
    other.build((2, T, H))
    so = other.state_dict()
    assert [tuple(v.shape) for v in so.values()] == [(H, 50), (50,), (3, 12)] and all(p.requires_grad for p in other.parameters())
    big = layers.NTMMemoryLayer(memory_slots=16, memory_dim=64)
    big.build((2, T, 64))
    assert abs(float(big.initial_memory.detach().std()) - 0.1) < 0.01                                        # normal, std 0.1


def test_layer_shape_and_mask_validation():
    h = torch.zeros(3, 5, 8)
    layer = layers.NTMMemoryLayer(2, 4)
    with pytest.raises(ValueError, match=r"\[B,T,H\]"):
        layers.NTMMemoryLayer(2, 4)(torch.zeros(3, 8))
    with pytest.raises(ValueError, match="mask must be"):
        layer(h, mask=torch.ones(3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask must be"):
        layer(h, mask=torch.ones(3, 5))
    with pytest.raises(ValueError, match="built for H = 8"):
        layer(torch.zeros(3, 5, 12))
    w = [torch.zeros(8, 18), torch.zeros(18), torch.zeros(2, 4)]
    for bad in ((torch.zeros(3, 8), None, *w), (h, None, torch.zeros(8, 16), *w[1:]), (h, None, w[0], torch.zeros(16), w[2]),
                (h, None, *w[:2], torch.zeros(4))):
        with pytest.raises(FilError):
            Fn.ntm_memory(*[t.cuda() if torch.is_tensor(t) and torch.cuda.is_available() else t for t in bad])


def test_no_cpu_fallback():
    h, mask = torch.zeros(3, 5, 8), torch.ones(3, 5, dtype=torch.bool)
    w = [torch.zeros(8, 18), torch.zeros(18), torch.zeros(2, 4)]
    with pytest.raises(FilError, match="GPU only"):
        Fn.ntm_memory(h, mask, *w)
    with pytest.raises(FilError, match="GPU only"):
        Fn.ntm_memory(h, None, *w, return_sequences=False)
    with pytest.raises(FilError, match="GPU only"):
        layers.NTMMemoryLayer(2, 4)(h, mask=mask)
    with pytest.raises(FilError, match="GPU only"):
        layers.NTMMemoryLayer(17, 4)(h)                              # outside the menu: the composed path
    with pytest.raises(FilError, match="GPU only"):
        layers.NTMMemoryLayer(2, 6)(h)
