"""The LSTM over a sequence on the GPU, one direction and both in one launch (include/fil.h N3 fil_lstm_*, functional.lstm,
layers.LSTMLayer / BiLSTMLayer, models.DSIN) against the fp64 restatement of tests/lstm_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (lstm_ref.bars).  The measured errors are printed."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import guarded
from tests import lstm_ref as ref
from tests.seq_common import behaviour_inputs, behaviour_model, bits, dev, dev_mask, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("x",) + ref.PARAMS
directions = pytest.mark.parametrize("direction", ref.DIRECTIONS)
ids_of = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def case_of(shape, direction, seed=0, mask="ragged", grads="both"):
    return ref.make_case(*shape, direction, seed, mask=mask, grads=grads)


def seq_gradient(case):
    """The [B,T,nH] gradient that stands for the case's g_hs and g_last together: g_last added at each direction's last step."""
    B, T, _, H = case["shape"]
    n = ref.ndir(case["direction"])
    g = np.zeros((B, T, n * H)) if case.get("g_hs") is None else np.array(case["g_hs"], np.float64)
    if case.get("g_last") is not None:
        for d in range(n):
            rev = d == 1 or case["direction"] == "reverse"
            g[:, 0 if rev else -1, d * H:(d + 1) * H] += case["g_last"][:, d * H:(d + 1) * H]
    return g.astype(np.float32)


def run_op(case, wanted=NAMES):
    """functional.lstm forward + backward on the case -> dict of float64 numpy arrays (hs and the gradients asked for).  A case with a
    g_hs runs return_sequences=True (g_last, if there, added at each direction's last step); g_last alone runs return_sequences=False."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES}
    seq = case.get("g_hs") is not None
    out = Fn.lstm(t["x"], dev_mask(case), t["W"], t["U"], t["b"], direction=case["direction"], return_sequences=seq)
    if any(v.requires_grad for v in t.values()):
        out.backward(dev(seq_gradient(case) if seq else case["g_last"]))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = dict(hs=D(out)) if seq else dict(last=D(out))
    for k, v in t.items():
        res["d" + k] = None if v.grad is None else D(v.grad)
    return res


def check_parity(got, case, keys=None, label=""):
    hs, bwd, e32 = ref.reference(case)
    got = {k: v for k, v in got.items() if v is not None and (keys is None or k in keys)}
    if "last" in got:
        got = dict(got)
        e_last = ref.norm_rel(got.pop("last"), ref.last_of(hs, case["direction"]))
        print("%s last %.2e" % (label, e_last))
        assert e_last <= max(1e-5, 4 * e32["hs"])
    err, bar = ref.errors(got, hs, bwd), ref.bars(e32)
    print("%s %s %s  " % (label, case["shape"], case["direction"])
          + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY_SHAPES = [(1, 1, 4, 4),           # the minimum
                 (3, 2, 4, 8),           # two steps
                 (5, 50, 16, 16),        # the benchmark's
                 (3, 5, 24, 24),         # NR = 16
                 (3, 7, 12, 20),         # K / 4 and H / 4 odd, K != H
                 (2, 300, 8, 4)]         # many steps, narrow state
CORNERS = [(3, 64, 64, 56), (2, 5, 40, 64), (2, 5, 64, 4), (2, 5, 4, 64)]      # the menu's edge towards the LDS limit, and the narrow sides


@directions
@pytest.mark.parametrize("shape", PARITY_SHAPES + CORNERS, ids=ids_of)
def test_parity_with_the_fp64_reference(shape, direction):
    case = case_of(shape, direction)
    check_parity(run_op(case), case)


@directions
def test_last_state_only(direction):
    case = case_of((5, 9, 8, 12), direction, grads="last")
    check_parity(run_op(case), case, label="last")


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
EDGE = (3, 4, 8)            # T, K, H


def run_raw(case, subset=ref.GRADS):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace guarded behind its
    bytes, `saved` guarded too (the gates of masked steps are never written and never used)."""
    lib = _lib.load()
    B, T, K, H = case["shape"]
    dirs = Fn.LSTM_DIRECTIONS[case["direction"]]
    n = ref.ndir(case["direction"])
    t = {k: (None if case.get(k) is None else dev(case[k])) for k in NAMES + ("g_hs", "g_last")}
    mask = dev_mask(case)
    shapes = dict(hs=(B, T, n * H), dx=(B, T, K), dW=case["W"].shape, dU=case["U"].shape, db=case["b"].shape)
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in ("hs",) + tuple(subset)}
    nsv = lib.fil_lstm_saved_bytes(B, T, K, H, dirs)
    assert n * B * T * 5 * H * 4 <= nsv <= -(-(n * B * T * 6 * H * 4) // 256) * 256
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    check(lib.fil_lstm_fwd(ptr(t["x"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), ptr(t["b"]), bufs["hs"].ptr, saved.ptr, B, T, K, H, dirs, stream_ptr()),
          "fil_lstm_fwd")
    nws = lib.fil_lstm_bwd_workspace_bytes(B, T, K, H, dirs)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    out = lambda k: bufs[k].ptr if k in bufs else None
    uses_ws = any(k in bufs for k in ("dW", "dU", "db")) or (n == 2 and "dx" in bufs)
    check(lib.fil_lstm_bwd(ptr(t["x"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), bufs["hs"].ptr, saved.ptr, ptr(t["g_hs"]), ptr(t["g_last"]), out("dx"),
                           out("dW"), out("dU"), out("db"), ptr(ws) if uses_ws else None, nws if uses_ws else 0, B, T, K, H, dirs, stream_ptr()),
          "fil_lstm_bwd")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_lstm_bwd", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64).reshape(shapes[k]) for k, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def edge_case(B, direction):
    """A few samples of three steps: the seed is the first whose sums over (b, t) are well conditioned in the fp64 reference
    (lstm_ref.conditioned_case, which says why; test_lstm_host.py asserts that such a seed exists; the seed is printed)."""
    return ref.conditioned_case(B, *EDGE, direction)


@directions
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which, direction):
    """T = 3, K = 4, H = 8.  tile - 1 (a partial tile) and tile: one workgroup per direction, one partial each; tile + 1: two, the
    second with one sample.  Every output and `saved` sit between guard words, the workspace has guard bytes behind it."""
    tile = Fn.lstm_plan(1, *EDGE, direction)["tile"]
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    plan = Fn.lstm_plan(B, *EDGE, direction)
    assert plan["tile"] == tile and plan["grid"] == (2 if which == "tile+1" else 1) and plan["partials"] == plan["grid"] * ref.ndir(direction)
    case = edge_case(B, direction)
    print("seed", case["seed"])
    check_parity(run_raw(case), case, label=which)


@directions
def test_past_the_grid_cap_a_workgroup_walks_a_second_tile(direction):
    """T = 2, K = 4, H = 4: the tile grows to 256 samples and B = cap * 256 + 1 leaves one workgroup a second tile of one sample."""
    T, K, H = 2, 4, 4
    cap = Fn.lstm_plan(1, T, K, H, direction)["cap"]
    tile = Fn.lstm_plan(1 << 30, T, K, H, direction)["tile"]
    B = cap * tile + 1
    plan = Fn.lstm_plan(B, T, K, H, direction)
    assert plan["tile"] == tile == 256 and plan["grid"] == cap and plan["partials"] == cap * ref.ndir(direction)
    case = case_of((B, T, K, H), direction, mask=None)
    check_parity(run_op(case), case, label="cap*tile+1")


@directions
def test_empty_batch_is_a_no_op(direction):
    n = ref.ndir(direction)
    lead = (2,) if n == 2 else ()
    x = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(lead + s, device="cuda", requires_grad=True) for s in ((4, 32), (8, 32), (32,))]
    out = Fn.lstm(x, None, *w, direction=direction)
    assert out.shape == (0, 3, n * 8)
    out.sum().backward()
    assert x.grad.shape == (0, 3, 4) and all(p.grad.shape == p.shape and not p.grad.any() for p in w)
    assert Fn.lstm(x, None, *w, direction=direction, return_sequences=False).shape == (0, n * 8)


@directions
@pytest.mark.parametrize("subset", [("dx",), ("dW", "dU", "db"), ("dU",)], ids=["dx", "params", "dU"])
def test_null_output_subsets_have_the_full_backwards_bits(subset, direction):
    case = edge_case(5, direction)
    full = run_raw(case)
    part = run_raw(case, subset=subset)
    assert set(part) == {"hs"} | set(subset)
    same_bits(part, full, subset)


def test_nothing_to_compute_is_an_argument_error():
    with pytest.raises(_lib.FilError):
        run_raw(edge_case(5, "forward"), subset=())


# ---------------------------------------------------------------------------------------------------- 3. exact properties
PROP = (6, 10, 8, 12)


def test_reverse_on_the_time_reversed_inputs_is_forward_bit_for_bit():
    fwd = case_of(PROP, "forward", seed=2)
    rev = dict(fwd, direction="reverse", x=fwd["x"][:, ::-1].copy(), mask=fwd["mask"][:, ::-1].copy(), g_hs=fwd["g_hs"][:, ::-1].copy())
    a, b = run_op(fwd), run_op(rev)
    assert np.array_equal(bits(a["hs"]), bits(b["hs"][:, ::-1])) and np.array_equal(bits(a["dx"]), bits(b["dx"][:, ::-1]))
    for k in ("dW", "dU", "db"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    check_parity(b, rev)


@pytest.mark.parametrize("shape,grads", [(PROP, "both"), ((40, 5, 16, 16), "last")], ids=["seq", "last"])
def test_one_bidirectional_launch_is_a_forward_and_a_reverse_call_bit_for_bit(shape, grads):
    H = shape[3]
    bi = case_of(shape, "bidirectional", seed=2, grads=grads)
    both = run_op(bi)
    halves = []
    for d, direction in enumerate(("forward", "reverse")):
        cols = slice(d * H, (d + 1) * H)
        one = dict(bi, direction=direction, W=bi["W"][d], U=bi["U"][d], b=bi["b"][d],
                   g_hs=None if bi["g_hs"] is None else bi["g_hs"][:, :, cols], g_last=bi["g_last"][:, cols])
        got = run_op(one)
        halves.append(got)
        out = "hs" if grads == "both" else "last"
        assert np.array_equal(bits(both[out][..., cols]), bits(got[out])), (direction, out)
        for k in ("dW", "dU", "db"):
            assert np.array_equal(bits(both[k][d]), bits(got[k])), (direction, k)
    dx = halves[0]["dx"].astype(np.float32) + halves[1]["dx"].astype(np.float32)
    assert np.array_equal(bits(both["dx"]), bits(dx))


def _prop_mask():
    B, T = PROP[:2]
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0           # leading padding
    m[:, 5] = 0
    m[1, 7:] = 0           # trailing padding
    m[4] = 0               # an all-masked sample
    return m


@directions
def test_masked_steps_carry_the_state_and_get_no_gradient(direction):
    B, T, K, H = PROP
    m = _prop_mask()
    case = ref.make_case(*PROP, direction, seed=2, mask=m)
    got = run_op(case)
    hs = got["hs"]
    if direction != "reverse":             # the forward columns: zeros before the first live step, the state repeated at masked ones
        f = hs[:, :, :H]
        assert not f[:, :2].any() and np.array_equal(bits(f[:, 5]), bits(f[:, 4])) and f[0, 2].any()
        for t in range(7, T):
            assert np.array_equal(bits(f[1, t]), bits(f[1, 6]))
    if direction != "forward":             # the reverse columns: the walk comes from T - 1
        r = hs[:, :, -H:]
        assert np.array_equal(bits(r[:, 5]), bits(r[:, 6])) and r[0, T - 1].any()
        assert np.array_equal(bits(r[:, 0]), bits(r[:, 2])) and np.array_equal(bits(r[:, 1]), bits(r[:, 2]))
        assert not r[1, 7:].any() and r[1, 6].any()
    assert not hs[4].any() and not got["dx"][4].any()
    assert not got["dx"][m == 0].any() and got["dx"][m != 0].any()
    check_parity(got, case, label="masked")


@directions
def test_no_mask_is_the_all_ones_mask_bit_for_bit(direction):
    case = case_of(PROP, direction, seed=2, mask=None)
    same_bits(run_op(case), run_op(dict(case, mask=np.ones(PROP[:2], np.uint8))))


@directions
def test_masked_inputs_are_never_used(direction):
    """NaN in every masked x row, and in the g_hs rows the kernel may skip: a masked step's output is the carried state, so its
    gradient counts -- except before the direction's first live step, where the state is the constant zero (forward columns: t before
    the first live slot; reverse columns: t after the last one; a sample without a live slot: every row)."""
    B, T, K, H = PROP
    m = _prop_mask()
    case = ref.make_case(*PROP, direction, seed=2, mask=m, grads="hs")
    live = m.astype(bool)
    seen_f = np.cumsum(live, axis=1) > 0                         # a live slot at or before t
    seen_r = np.cumsum(live[:, ::-1], axis=1)[:, ::-1] > 0       # a live slot at or after t
    dead = {"forward": [~seen_f], "reverse": [~seen_r], "bidirectional": [~seen_f, ~seen_r]}[direction]
    g = case["g_hs"].copy()
    for d, rows in enumerate(dead):
        assert rows.any() and not (rows & live).any()
        g[:, :, d * H:(d + 1) * H][rows] = np.nan
    poisoned = dict(case, x=np.where(live[:, :, None], case["x"], np.nan), g_hs=g)
    clean, dirty = run_op(case), run_op(poisoned)
    for k, v in dirty.items():
        assert np.isfinite(v).all(), k
    same_bits(clean, dirty)


@directions
def test_last_state_gradient_is_the_sequence_gradient_at_the_last_step(direction):
    base = case_of(PROP, direction, seed=2, grads="last")
    one = run_op(base)
    two = run_op(dict(base, g_hs=seq_gradient(base).astype(np.float64), g_last=None))
    assert np.array_equal(bits(one["last"]), bits(ref.last_of(two["hs"], direction)))
    for k in ref.GRADS:
        assert np.array_equal(bits(one[k]), bits(two[k])), k


@directions
def test_repeats_are_bit_identical(direction):
    case = case_of((300, 20, 16, 16), direction)
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    check_parity(first, case)


@directions
def test_needs_input_grad_is_honoured(direction):
    case = case_of((9, 6, 8, 12), direction)
    full = run_op(case)
    for wanted in (("x",), tuple(ref.PARAMS), ("U",), ("x", "b")):
        got = run_op(case, wanted=wanted)
        for k in NAMES:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["hs"]), bits(full["hs"]))
    assert run_op(case, wanted=())["dx"] is None


# ---------------------------------------------------------------------------------------------------- 4. layers and model
ONE = dict(W="kernel", U="recurrent_kernel", b="bias")


def _layer_of(direction, units, **kw):
    if direction == "bidirectional":
        return layers.BiLSTMLayer(units, **kw)
    return layers.LSTMLayer(units, go_backwards=direction == "reverse", **kw)


def _layer_params(layer, direction):
    """-> {case key: the layer's parameters behind it (one, or forward and backward)}"""
    if direction == "bidirectional":
        return {k: [getattr(layer, "forward_" + n), getattr(layer, "backward_" + n)] for k, n in ONE.items()}
    return {k: [getattr(layer, n)] for k, n in ONE.items()}


def _run_layer(layer, case, dtype=torch.float32):
    direction = case["direction"]
    x = dev(case["x"]).to(dtype).requires_grad_()
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    with torch.no_grad():
        layer(x, mask=mask)        # lazy build
        for k, ps in _layer_params(layer, direction).items():
            for d, p in enumerate(ps):
                p.copy_(dev(case[k][d] if direction == "bidirectional" else case[k]))
    layer.zero_grad()
    out = layer(x, mask=mask)
    assert out.dtype == torch.float32
    D = lambda v: v.detach().cpu().double().numpy()
    if getattr(layer, "merge_mode", "concat") != "concat":
        return dict(hs=D(out))
    assert out.shape == case["shape"][:2] + (ref.ndir(direction) * case["shape"][3],)
    out.backward(dev(seq_gradient(case)))
    torch.cuda.synchronize()
    res = dict(hs=D(out), dx=D(x.grad))
    for k, ps in _layer_params(layer, direction).items():
        gs = [D(p.grad) for p in ps]
        res["d" + k] = np.stack(gs) if direction == "bidirectional" else gs[0]
    return res


OUTSIDE = [(3, 5, 8, 68), (3, 5, 6, 8), (3, 5, 56, 60)]      # H past the menu, K % 4 != 0, the first pair the plan refuses for its LDS


@directions
@pytest.mark.parametrize("shape", OUTSIDE, ids=["H=68", "K=6", "first-refused"])
def test_layer_outside_the_menu_takes_the_composed_path(shape, direction):
    case = case_of(shape, direction, seed=9)
    layer = _layer_of(direction, shape[3])
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["x"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


@directions
def test_layer_inside_the_menu_is_the_op(direction):
    case = case_of((9, 6, 8, 12), direction)
    layer = _layer_of(direction, 12)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["x"]))
    same_bits(got, run_op(case))


@directions
def test_layer_last_state_inside_the_menu_is_the_op(direction):
    case = case_of((9, 6, 8, 12), direction, grads="last")
    layer = _layer_of(direction, 12, return_sequences=False)
    x = dev(case["x"])
    mask = dev(case["mask"], torch.uint8).bool()
    with torch.no_grad():
        layer(x, mask=mask)
        for k, ps in _layer_params(layer, direction).items():
            for d, p in enumerate(ps):
                p.copy_(dev(case[k][d] if direction == "bidirectional" else case[k]))
        out = layer(x, mask=mask)
    assert np.array_equal(bits(out.cpu().numpy()), bits(run_op(case, wanted=())["last"]))


@directions
def test_layer_computes_a_half_precision_input_in_fp32(direction):
    case = case_of((9, 6, 8, 12), direction, seed=6)
    r16 = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    case16 = dict(case, x=r16(case["x"]))
    half = _run_layer(_layer_of(direction, 12), case16, dtype=torch.bfloat16)     # asserts an fp32 output; dx comes back in bf16
    check_parity(half, case16, keys=("hs", "dW", "dU", "db"), label="bf16 in")


@pytest.mark.parametrize("merge_mode", ["sum", "ave"])
@pytest.mark.parametrize("seq", [True, False], ids=["seq", "last"])
def test_bilstm_merge_modes_are_torch_ops_on_the_halves_of_concat(merge_mode, seq):
    case = case_of((9, 6, 8, 12), "bidirectional")
    H = 12
    x, mask = dev(case["x"]), dev(case["mask"], torch.uint8).bool()
    outs = {}
    for mode in ("concat", merge_mode):
        layer = layers.BiLSTMLayer(H, merge_mode=mode, return_sequences=seq)
        with torch.no_grad():
            layer(x, mask=mask)
            for k, ps in _layer_params(layer, "bidirectional").items():
                for d, p in enumerate(ps):
                    p.copy_(dev(case[k][d]))
            outs[mode] = layer(x, mask=mask)
    cat = outs["concat"]
    assert cat.shape == ((9, 6, 2 * H) if seq else (9, 2 * H)) and outs[merge_mode].shape == cat.shape[:-1] + (H,)
    want = cat[..., :H] + cat[..., H:]
    if merge_mode == "ave":
        want = want * 0.5
    assert torch.equal(outs[merge_mode], want) and bool(want.any())


VOCAB, T_HIST, SESS, K_EMB, B_DSIN = (50, 20, 10), 12, 3, 8, 7


def _dsin_model(seed):
    return behaviour_model(lambda: models.DSIN(SESS, hidden_units=[32, 16]), list(VOCAB), T_HIST, K_EMB, seed)


def _dsin_inputs(seed):
    """behaviour_inputs with a sample whose middle session is empty (sample 0) and one whose history is empty (sample 1)."""
    _, idx, hist = behaviour_inputs(B_DSIN, list(VOCAB), T_HIST, seed=seed)
    ts = T_HIST // SESS
    hist[0, 0, :] = torch.arange(1, T_HIST + 1, device="cuda")
    hist[0, 0, ts:2 * ts] = 0
    hist[1, 0, :] = 0
    return idx, hist


def test_dsin_against_the_model_built_from_the_composed_layers(monkeypatch):
    """3 fields, one history of T = 12 in 3 sessions, B = 7.  The same weights with the LSTM, the self-attention and the DIN attention
    forced onto their composed paths (fp32 torch ops): the output and every parameter gradient agree within 1e-5, the floor of the
    component ops' bars max(1e-5, 4 E32) (no fp64 model is built here, so the term that could only widen the bar is left out)."""
    idx, hist = _dsin_inputs(1)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0], device="cuda")
    model = _dsin_model(3)

    def grads():
        model.zero_grad()
        p = model(None, idx, hist)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads()
    beh = model.body.behaviors[0]
    assert beh.interact.fits_kernel_menu(torch.empty(B_DSIN, SESS, K_EMB)) and beh.interact.merge_mode == "ave"
    assert beh.atten.fits_kernel_menu(torch.empty(B_DSIN * SESS, T_HIST // SESS, K_EMB))
    monkeypatch.setattr(layers.BiLSTMLayer, "fits_kernel_menu", lambda self, x: False)
    monkeypatch.setattr(layers.SeqSelfAttentionLayer, "fits_kernel_menu", lambda self, x: False)
    monkeypatch.setattr(layers.DinAttentionLayer, "fits_kernel_menu", lambda self, q, keys: False)
    comp = grads()
    monkeypatch.undo()
    assert set(fused) == set(comp)
    for name in ("interact.forward_recurrent_kernel", "interact.backward_kernel", "sess_bias", "pos_bias", "unit_bias", "atten.query_w",
                 "att_extract.att_w1", "att_interact.att_w1"):
        assert "body.behaviors.0." + name in fused, name
    assert np.isfinite(fused["out"]).all()
    worst = {}
    for k in sorted(fused):
        if k.endswith(".att_b3"):
            # softmax=True: a shift of every score changes nothing, this gradient is zero in exact arithmetic and what either path
            # returns is the rounding of a cancelling sum of the score gradients -- the terms that, weighted by activations of order
            # one, make up att_w3's gradient.  Both paths are held to 1e-5 of that gradient's norm; no ratio to zero is taken.
            scale = np.linalg.norm(comp[k[:-2] + "w3"])
            worst[k] = max(np.abs(fused[k]).max(), np.abs(comp[k]).max()) / scale
            print("DSIN %-50s |fused|, |composed| over |d att_w3| %.2e   bar 1.00e-05" % (k, worst[k]))
            continue
        worst[k] = ref.norm_rel(fused[k], comp[k])
        print("DSIN %-50s fused vs composed %.2e   bar 1.00e-05" % (k, worst[k]))
    for k, v in worst.items():
        assert v <= 1e-5, (k, v)
    assert np.abs(fused["body.behaviors.0.interact.backward_recurrent_kernel"]).max() > 0


def test_dsin_trains_under_captured_adam_and_replays_the_eager_bits():
    """The loss falls over 20 captured optim.Adam steps on one batch, and three captured steps on three batches leave every
    parameter with the bits of three eager steps."""
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        idx, hist = _dsin_inputs(40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B_DSIN), dtype=torch.float32, device="cuda")))

    def make():
        model = _dsin_model(7)
        model(None, batches[0][0], batches[0][1])
        opt = optim.Adam(model.parameters(), learning_rate=1e-2)

        def step(idx, hist, y):
            opt.zero_grad()
            p = model(None, idx, hist)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6)
            loss.backward()
            opt.step()
            return loss.detach()
        return model, opt, step

    model_e, _, step_e = make()
    for bt in batches:
        step_e(*bt)
    model_c, opt_c, step_c = make()
    init = {k: v.clone() for k, v in model_c.state_dict().items()}

    def restore():
        with torch.no_grad():
            for k, v in model_c.state_dict().items():
                v.copy_(init[k])
        opt_c.reset_()

    captured = capture.capture_step(step_c, *batches[0], restore=restore)
    for bt in batches:
        captured(*bt)
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(model_e.named_parameters(), model_c.named_parameters()):
        assert torch.equal(a, b), n
    name = "body.behaviors.0.interact.backward_recurrent_kernel"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
