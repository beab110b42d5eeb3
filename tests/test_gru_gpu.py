"""The GRU / AUGRU / AGRU over a behaviour sequence on the GPU (include/fil.h N3 fil_gru_*, functional.gru, layers.GRULayer,
models.DIEN) against the fp64 restatement of tests/gru_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (gru_ref.bars).  The measured errors are printed."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import gru_ref as ref
from tests import guarded
from tests.seq_common import behaviour_inputs, behaviour_model, bits, dev, dev_mask, same_bits

pytestmark = pytest.mark.gpu

MODES = list(ref.MODES)
NAMES = ("x", "a") + ref.PARAMS
modes = pytest.mark.parametrize("mode", MODES)
ids_of = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def case_of(shape, mode, seed=0, mask="ragged", grads="both"):
    return ref.make_case(*shape, mode, seed, mask=mask, grads=grads)


def run_op(case, wanted=NAMES):
    """functional.gru forward + backward on the case -> dict of float64 numpy arrays (hs and the gradients asked for).  A case with
    both upstream gradients runs return_sequences=True and adds g_last to the last step of g_hs; g_last alone runs
    return_sequences=False."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES if case.get(k) is not None}
    seq = case.get("g_hs") is not None
    out = Fn.gru(t["x"], t.get("a"), dev_mask(case), t["W"], t["U"], t["b"], mode=case["mode"], return_sequences=seq)
    if seq:
        g = np.array(case["g_hs"], np.float64)
        if case.get("g_last") is not None:
            g[:, -1] += case["g_last"]
        g = g.astype(np.float32)
    else:
        g = case["g_last"]
    if any(v.requires_grad for v in t.values()):
        out.backward(dev(g))
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
        last = got.pop("last")
        e_last = ref.norm_rel(last, hs[:, -1])
        print("%s last %.2e" % (label, e_last))
        assert e_last <= max(1e-5, 4 * e32["hs"])
    err, bar = ref.errors(got, hs, bwd), ref.bars(e32)
    print("%s %s %s  " % (label, case["shape"], case["mode"]) + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
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
CORNERS = [(3, 256, 64, 64), (2, 5, 64, 4), (2, 5, 4, 64)]


@modes
@pytest.mark.parametrize("shape", PARITY_SHAPES + CORNERS, ids=ids_of)
def test_parity_with_the_fp64_reference(shape, mode):
    case = case_of(shape, mode)
    check_parity(run_op(case), case)


@modes
def test_last_state_only(mode):
    case = case_of((5, 9, 8, 12), mode, grads="last")
    check_parity(run_op(case), case, label="last")


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
EDGE = (3, 4, 8)            # T, K, H


def run_raw(case, subset=ref.GRADS):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace guarded behind its
    bytes, `saved` NaN-filled before the forward (masked steps are never written and never used)."""
    lib = _lib.load()
    B, T, K, H = case["shape"]
    mode = Fn.GRU_MODES[case["mode"]]
    t = {k: (None if case.get(k) is None else dev(case[k])) for k in NAMES + ("g_hs", "g_last")}
    mask = dev_mask(case)
    shapes = dict(hs=(B, T, H), dx=(B, T, K), da=(B, T), dW=(K, 3 * H), dU=(H, 3 * H), db=(2, 3 * H))
    want = ["hs"] + [k for k in subset if not (k == "da" and case["mode"] == "gru")]
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in want}
    nsv = lib.fil_gru_saved_bytes(B, T, K, H)
    assert nsv >= B * T * 4 * H * 4
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    check(lib.fil_gru_fwd(ptr(t["x"]), ptr(t["a"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), ptr(t["b"]), bufs["hs"].ptr, saved.ptr, B, T, K, H, mode,
                          stream_ptr()), "fil_gru_fwd")
    nws = lib.fil_gru_bwd_workspace_bytes(B, T, K, H)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    out = lambda k: bufs[k].ptr if k in bufs else None
    params = any(k in bufs for k in ("dW", "dU", "db"))
    check(lib.fil_gru_bwd(ptr(t["x"]), ptr(t["a"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), bufs["hs"].ptr, saved.ptr, ptr(t["g_hs"]), ptr(t["g_last"]),
                          out("dx"), out("da"), out("dW"), out("dU"), out("db"), ptr(ws) if params else None, nws if params else 0, B, T, K, H, mode,
                          stream_ptr()), "fil_gru_bwd")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_gru_bwd", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64) for k, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def edge_case(B, mode):
    """A few samples of three steps: the seed is the first whose sums over (b, t) are well conditioned in the fp64 reference
    (gru_ref.conditioned_case, which says why; the seed is printed)."""
    return ref.conditioned_case(B, *EDGE, mode)


@modes
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which, mode):
    """T = 3, K = 4, H = 8.  tile - 1 (a partial tile) and tile: one workgroup, one partial; tile + 1: two, the second with one sample.
    Every output and `saved` sit between guard words, the workspace has guard bytes behind it."""
    tile = Fn.gru_plan(1, *EDGE)["tile"]
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    plan = Fn.gru_plan(B, *EDGE)
    assert plan["tile"] == tile and plan["partials"] == (2 if which == "tile+1" else 1)
    case = edge_case(B, mode)
    print("seed", case["seed"])
    check_parity(run_raw(case), case, label=which)


@modes
def test_past_the_grid_cap_a_workgroup_walks_a_second_tile(mode):
    """K = 4, H = 64: four sample quads at most, so the tile stops at 16 samples and B = cap * 16 + 1 leaves one workgroup a second
    tile of one sample.  T = 1 keeps the fp64 reference cheap."""
    T, K, H = 1, 4, 64
    cap = Fn.gru_plan(1, T, K, H)["cap"]
    B = cap * 16 + 1
    plan = Fn.gru_plan(B, T, K, H)
    assert plan["tile"] == 16 and plan["grid"] == cap and plan["partials"] == cap
    case = case_of((B, T, K, H), mode, mask=None)
    check_parity(run_op(case), case, label="cap*tile+1")


def test_empty_batch_is_a_no_op():
    x = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(s, device="cuda", requires_grad=True) for s in ((4, 24), (8, 24), (2, 24))]
    assert Fn.gru(x, None, None, *w).shape == (0, 3, 8)
    assert Fn.gru(x, None, None, *w, return_sequences=False).shape == (0, 8)


@modes
@pytest.mark.parametrize("subset", [("dx",), ("dW", "dU", "db"), ("da",), ("dU",)], ids=["dx", "params", "da", "dU"])
def test_null_output_subsets_have_the_full_backwards_bits(subset, mode):
    if mode == "gru" and subset == ("da",):
        # nothing is left to compute: FIL_ERR_ARG
        case = edge_case(5, mode)
        with pytest.raises(_lib.FilError):
            run_raw(case, subset=subset)
        return
    case = edge_case(5, mode)
    full = run_raw(case)
    part = run_raw(case, subset=subset)
    assert set(part) == {"hs"} | {k for k in subset if k in full}
    same_bits(part, full, subset)


# ---------------------------------------------------------------------------------------------------- 3. exact properties
PROP = (6, 10, 8, 12)


def test_gru_is_augru_with_ones_bit_for_bit():
    base = case_of(PROP, "augru", seed=2)
    gru = run_op(dict(base, mode="gru", a=None))
    aug = run_op(dict(base, a=np.ones(PROP[:2])))
    for k in ("hs", "dx", "dW", "dU", "db"):
        assert np.array_equal(bits(gru[k]), bits(aug[k])), k
    check_parity(gru, dict(base, mode="gru", a=None))


@pytest.mark.parametrize("mode", ["augru", "agru"])
def test_a_zero_score_repeats_the_state(mode):
    base = case_of(PROP, mode, seed=2, mask=None)
    a = base["a"].copy()
    a[:, 3] = 0.0
    a[2, 5:8] = 0.0
    got = run_op(dict(base, a=a))
    hs = got["hs"]
    assert np.array_equal(bits(hs[:, 3]), bits(hs[:, 2])) and hs[:, 2].any()
    for t in (5, 6, 7):
        assert np.array_equal(bits(hs[2, t]), bits(hs[2, 4]))


@modes
def test_masked_steps_carry_the_state_and_get_no_gradient(mode):
    B, T = PROP[:2]
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0           # leading padding
    m[:, 5] = 0
    m[1, 7:] = 0           # trailing padding
    m[4] = 0               # an all-masked sample
    case = ref.make_case(*PROP, mode, seed=2, mask=m)
    got = run_op(case)
    hs = got["hs"]
    assert not hs[:, :2].any() and np.array_equal(bits(hs[:, 5]), bits(hs[:, 4])) and hs[0, 2].any()
    for t in range(7, T):
        assert np.array_equal(bits(hs[1, t]), bits(hs[1, 6]))
    assert not hs[4].any() and not got["dx"][4].any()
    assert not got["dx"][m == 0].any()
    if mode != "gru":
        assert not got["da"][m == 0].any() and got["da"][m != 0].any()
    check_parity(got, case, label="masked")


@modes
def test_no_mask_is_the_all_ones_mask_bit_for_bit(mode):
    case = case_of(PROP, mode, seed=2, mask=None)
    same_bits(run_op(case), run_op(dict(case, mask=np.ones(PROP[:2], np.uint8))))


@modes
def test_masked_inputs_are_never_used(mode):
    case = case_of(PROP, mode, seed=2)
    live = case["mask"].astype(bool)
    poisoned = dict(case, x=np.where(live[:, :, None], case["x"], np.nan))
    if mode != "gru":
        poisoned["a"] = np.where(live, case["a"], np.nan)
    clean, dirty = run_op(case), run_op(poisoned)
    for k, v in dirty.items():
        if v is not None:
            assert np.isfinite(v).all(), k
    same_bits(clean, dirty)


@modes
def test_last_state_gradient_is_the_sequence_gradient_at_the_last_step(mode):
    base = case_of(PROP, mode, seed=2, grads="last")
    g_hs = np.zeros(PROP[:2] + (PROP[3],))
    g_hs[:, -1] = base["g_last"]
    one = run_op(base)
    two = run_op(dict(base, g_hs=g_hs, g_last=None))
    assert np.array_equal(bits(one["last"]), bits(two["hs"][:, -1]))
    for k in ("dx", "da", "dW", "dU", "db"):
        if one.get(k) is not None:
            assert np.array_equal(bits(one[k]), bits(two[k])), k


@modes
def test_repeats_are_bit_identical(mode):
    case = case_of((300, 20, 16, 16), mode)
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    check_parity(first, case)


@modes
def test_needs_input_grad_is_honoured(mode):
    case = case_of((9, 6, 8, 12), mode)
    full = run_op(case)
    present = [k for k in NAMES if case.get(k) is not None]
    for wanted in (("x",), tuple(ref.PARAMS), ("a",), ("x", "b")):
        got = run_op(case, wanted=wanted)
        for k in present:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["hs"]), bits(full["hs"]))


# ---------------------------------------------------------------------------------------------------- 4. layer and model
LAYER_NAMES = dict(W="kernel", U="recurrent_kernel", b="bias")


def _run_layer(layer, case, dtype=torch.float32):
    x = dev(case["x"]).to(dtype).requires_grad_()
    a = None if case.get("a") is None else dev(case["a"]).to(dtype).requires_grad_()
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    inputs = x if a is None else [x, a]
    with torch.no_grad():
        layer(inputs, mask=mask)        # lazy build
        for k, name in LAYER_NAMES.items():
            getattr(layer, name).copy_(dev(case[k]))
    layer.zero_grad()
    out = layer(inputs, mask=mask)
    assert out.dtype == torch.float32 and out.shape == (case["shape"][0], case["shape"][1], case["shape"][3])
    g = np.array(case["g_hs"], np.float64)
    g[:, -1] += case["g_last"]
    out.backward(dev(g.astype(np.float32)))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = dict(hs=D(out), dx=D(x.grad), da=None if a is None else D(a.grad))
    for k, name in LAYER_NAMES.items():
        res["d" + k] = D(getattr(layer, name).grad)
    return res


@modes
@pytest.mark.parametrize("shape", [(3, 5, 8, 68), (3, 5, 6, 8)], ids=["H=68", "K=6"])
def test_layer_outside_the_menu_takes_the_composed_path(shape, mode):
    case = case_of(shape, mode, seed=9)
    layer = layers.GRULayer(shape[3], mode=mode)
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["x"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


@modes
def test_layer_inside_the_menu_is_the_op(mode):
    case = case_of((9, 6, 8, 12), mode)
    layer = layers.GRULayer(12, mode=mode)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["x"]))
    same_bits(got, run_op(case))


@modes
def test_layer_computes_a_half_precision_input_in_fp32(mode):
    case = case_of((9, 6, 8, 12), mode, seed=6)
    r16 = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    case16 = dict(case, x=r16(case["x"]), a=None if case["a"] is None else r16(case["a"]))
    layer = layers.GRULayer(12, mode=mode)
    half = _run_layer(layer, case16, dtype=torch.bfloat16)          # asserts an fp32 output; the input gradients come back in bf16
    check_parity(half, case16, keys=("hs", "dW", "dU", "db"), label="bf16 in")


def _dien_model(vocab, T, K, seed, **kw):
    return behaviour_model(lambda: models.DIEN(hidden_units=[32, 16], **kw), vocab, T, K, seed)


@pytest.mark.parametrize("gru_type", ["augru", "agru"])
def test_dien_against_the_model_built_from_the_composed_layers(gru_type, monkeypatch):
    """3 fields, one history of T = 6, B = 5.  The same weights through the composed layers (gru_graph: fp32 torch ops): the output
    and every parameter gradient agree within 1e-5, the floor of the bars max(1e-5, 4 E32) (no fp64 model is built here, so the
    term that could only widen the bar is left out)."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    _, idx, hist = behaviour_inputs(B, vocab, T, seed=1)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], device="cuda")
    model = _dien_model(vocab, T, K, 3, gru_type=gru_type)

    def grads():
        model.zero_grad()
        p = model(None, idx, hist)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads()
    beh = model.body.behaviors[0]
    assert beh.extract.fits_kernel_menu(torch.empty(B, T, K)) and beh.evolve.mode == gru_type
    monkeypatch.setattr(layers.GRULayer, "fits_kernel_menu", lambda self, x: False)
    comp = grads()
    monkeypatch.undo()
    assert set(fused) == set(comp) and "body.behaviors.0.extract.recurrent_kernel" in fused and "body.behaviors.0.att_w" in fused
    for k in sorted(fused):
        direct = ref.norm_rel(fused[k], comp[k])
        print("DIEN %-45s fused vs composed %.2e   bar 1.00e-05" % (k, direct))
        assert direct <= 1e-5, k
    assert np.abs(fused["body.behaviors.0.evolve.recurrent_kernel"]).max() > 0


def test_dien_trains_under_captured_adam_and_replays_the_eager_bits():
    """The loss falls over 20 captured optim.Adam steps on one batch, and three captured steps on three batches leave every
    parameter with the bits of three eager steps."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx, hist = behaviour_inputs(B, vocab, T, seed=40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        model = _dien_model(vocab, T, K, 7)
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
    name = "body.behaviors.0.evolve.recurrent_kernel"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
