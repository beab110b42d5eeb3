"""The time-stream GRU over a behaviour sequence with event gaps on the GPU (include/fil.h N5 fil_tsgru_*, functional.ts_gru,
layers.TimeStreamGRULayer, models.DTSInput / DTS) against the fp64 restatement of tests/ts_gru_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (ts_gru_ref.bars).  The measured errors are printed."""
import functools
import itertools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import guarded
from tests import ts_gru_ref as ref
from tests.seq_common import behaviour_inputs, bits, dev, dev_mask, same_bits
from tests.ts_gru_cases import CORNERS, EDGE, LARGE, PARITY_SHAPES, case_of, edge_case, large_case, largest_square

pytestmark = pytest.mark.gpu

NAMES = ("x",) + ref.PARAMS
ids_of = lambda s: "x".join(map(str, s))


def run_op(case, wanted=NAMES, seq=None):
    """functional.ts_gru forward + backward on the case -> dict of float64 numpy arrays (hs or last, z, and the gradients asked for).
    With g_hs the op runs return_sequences=True and g_last is added to the last step of g_hs; without it return_sequences=`seq`
    (False unless said: g_last then enters as [B,H])."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES}
    if seq is None:
        seq = case.get("g_hs") is not None
    assert seq or case.get("g_hs") is None
    dt_out = None if case.get("dt_out") is None else dev(case["dt_out"])
    res = Fn.ts_gru(t["x"], dev(case["dt"]), dt_out, dev_mask(case), *(t[k] for k in ref.PARAMS), steps=case["S"], return_sequences=seq)
    out, z = (res, None) if dt_out is None else res
    outs, gs = [], []
    if seq and (case.get("g_hs") is not None or case.get("g_last") is not None):
        g = np.zeros(out.shape) if case.get("g_hs") is None else np.array(case["g_hs"], np.float64)
        if case.get("g_last") is not None:
            g[:, -1] += case["g_last"]
        outs, gs = [out], [dev(g.astype(np.float32))]
    elif case.get("g_last") is not None:
        outs, gs = [out], [dev(case["g_last"])]
    if case.get("g_z") is not None:
        outs.append(z)
        gs.append(dev(case["g_z"]))
    if any(v.requires_grad for v in t.values()):
        torch.autograd.backward(outs, gs)
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = {"hs" if seq else "last": D(out), "z": None if z is None else D(z)}
    for k, v in t.items():
        res["d" + k] = None if v.grad is None else D(v.grad)
    return res


def check_parity(got, case, keys=None, label=""):
    hs, z, bwd, e32 = ref.reference(case)
    got = {k: v for k, v in got.items() if v is not None and (keys is None or k in keys)}
    if "last" in got:
        last = got.pop("last")
        e_last = ref.norm_rel(last, hs[:, -1])
        print("%s last %.2e" % (label, e_last))
        assert np.isfinite(last).all() and e_last <= max(1e-5, 4 * e32["hs"])
    err, bar = ref.errors(got, hs, z, bwd), ref.bars(e32)
    print("%s %s  " % (label, case["shape"]) + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("seq", [True, False], ids=["seq", "last"])
@pytest.mark.parametrize("out", [True, False], ids=["dt_out", "no_dt_out"])
@pytest.mark.parametrize("shape", PARITY_SHAPES + CORNERS + ["largest-square"], ids=lambda s: s if isinstance(s, str) else ids_of(s))
def test_parity_with_the_fp64_reference(shape, out, seq):
    if shape == "largest-square":
        kh = largest_square()
        assert Fn.ts_gru_plan(3, 6, kh, kh, 2)["fits"] and not Fn.ts_gru_plan(3, 6, kh + 4, kh + 4, 2)["fits"]
        shape = (3, 6, kh, kh, 2)
    case = case_of(shape, out=out, seq=seq)
    check_parity(run_op(case, seq=seq), case)


SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(("hs", "last", "z"), n)]


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_every_subset_of_the_upstream_gradients(subset):
    case = ref.conditioned_case(5, *EDGE, grads=subset)
    print("seed", case["seed"])
    check_parity(run_op(case), case, label="+".join(subset))
    if "hs" not in subset:
        check_parity(run_op(case, seq=True), case, label="+".join(subset) + " seq")


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
def run_raw(case, subset=ref.GRADS, nan_saved=True):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace NaN-filled and guarded
    behind its bytes, `saved` NaN-filled before the forward (the guard's sentinel is a NaN: masked steps are never written and never
    used)."""
    lib = _lib.load()
    B, T, K, H, S = case["shape"]
    t = {k: (None if case.get(k) is None else dev(case[k])) for k in NAMES + ("dt", "dt_out", "g_hs", "g_last", "g_z")}
    mask = dev_mask(case)
    shapes = dict(hs=(B, T, H), z=(B, H), dx=(B, T, K), dW=(K, 3 * H), dU=(H, 3 * H), db=(2, 3 * H), dWf=(H, H), dbf=(H,))
    want = ["hs"] + (["z"] if t["dt_out"] is not None else []) + list(subset)
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in want}
    nsv = lib.fil_tsgru_saved_bytes(B, T, K, H, S)
    assert nsv >= (B * T * (4 + 2 * S) + B * 2 * S) * H * 4
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    out = lambda k: bufs[k].ptr if k in bufs else None
    check(lib.fil_tsgru_fwd(ptr(t["x"]), ptr(t["dt"]), ptr(t["dt_out"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), ptr(t["b"]), ptr(t["Wf"]),
                            ptr(t["bf"]), out("hs"), out("z"), saved.ptr, B, T, K, H, S, stream_ptr()), "fil_tsgru_fwd")
    nws = lib.fil_tsgru_bwd_workspace_bytes(B, T, K, H, S)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    params = any(k in bufs for k in ref.GRADS[1:])
    check(lib.fil_tsgru_bwd(ptr(t["x"]), ptr(t["dt"]), ptr(t["dt_out"]), ptr(mask), ptr(t["W"]), ptr(t["U"]), ptr(t["Wf"]), saved.ptr,
                            ptr(t["g_hs"]), ptr(t["g_last"]), ptr(t["g_z"]), out("dx"), out("dW"), out("dU"), out("db"), out("dWf"), out("dbf"),
                            ptr(ws) if params else None, nws if params else 0, B, T, K, H, S, stream_ptr()), "fil_tsgru_bwd")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_tsgru_bwd", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64) for k, b in bufs.items()}


@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which):
    """T = 3, K = 4, H = 8, S = 2.  tile - 1 (a partial tile) and tile: one workgroup, one partial; tile + 1: two, the second with one
    sample.  Every output and `saved` (NaN before the forward) sit between guard words, the NaN-filled workspace has guard bytes
    behind it; the backward is finite and inside the bars."""
    tile = Fn.ts_gru_plan(1, *EDGE)["tile"]
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    plan = Fn.ts_gru_plan(B, *EDGE)
    assert plan["tile"] == tile and plan["partials"] == (2 if which == "tile+1" else 1)
    case = edge_case(B)
    print("seed", case["seed"])
    check_parity(run_raw(case), case, label=which)


def test_past_the_grid_cap_a_workgroup_walks_a_second_tile():
    """K = 4, H = 64: the tile stops at 16 samples, so B = cap * 16 + 1 leaves one workgroup a second tile of one sample.  T = 2.  The
    first tile's samples, some from the middle and the one of the second walk, run again as a batch of their own, keep their bits."""
    T, K, H, S = 2, 4, 64, 2
    cap = Fn.ts_gru_plan(1, T, K, H, S)["cap"]
    B = cap * 16 + 1
    plan = Fn.ts_gru_plan(B, T, K, H, S)
    assert plan["tile"] == 16 and plan["grid"] == cap and plan["partials"] == cap
    case = ref.make_case(B, T, K, H, S, seed=0, mask="prefix")
    big = run_op(case, wanted=("x",))
    pick = np.array([0, 1, 2, 15, 16, 7777, B - 2, B - 1])
    sub = dict(case, shape=(len(pick), T, K, H, S), **{k: case[k][pick] for k in ("x", "dt", "dt_out", "mask", "g_hs", "g_last", "g_z")})
    small = run_op(sub, wanted=("x",))
    for k in ("hs", "z", "dx"):
        assert np.array_equal(bits(big[k][pick]), bits(small[k])), k
    check_parity(small, sub, keys=("hs", "z", "dx"), label="cap*tile+1")


def test_empty_batch_is_a_no_op():
    x = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(s, device="cuda", requires_grad=True) for s in ((4, 24), (8, 24), (2, 24), (8, 8), (8,))]
    dt, dt_out = torch.empty(0, 3, device="cuda"), torch.empty(0, device="cuda")
    assert Fn.ts_gru(x, dt, None, None, *w).shape == (0, 3, 8)
    last, z = Fn.ts_gru(x, dt, dt_out, None, *w, return_sequences=False)
    assert last.shape == (0, 8) and z.shape == (0, 8)


@pytest.mark.parametrize("subset", [("dx",), ("dW", "dU", "db", "dWf", "dbf"), ("dWf",)], ids=["dx", "params", "dWf"])
def test_null_output_subsets_have_the_full_backwards_bits(subset):
    case = edge_case(5)
    full = run_raw(case)
    part = run_raw(case, subset=subset)
    assert set(part) == {"hs", "z"} | set(subset)
    same_bits(part, full, subset)
    with pytest.raises(_lib.FilError):
        run_raw(case, subset=())              # nothing is left to compute: FIL_ERR_ARG


# ---------------------------------------------------------------------------------------------------- 3. exact properties
PROP = (6, 10, 8, 12, 2)


def _gru(case):
    """Fn.gru (mode "gru") on the case's x, mask, W, U, b -> hs as float64."""
    hs = Fn.gru(dev(case["x"]), None, dev_mask(case), dev(case["W"]), dev(case["U"]), dev(case["b"]), mode="gru")
    torch.cuda.synchronize()
    return hs.cpu().double().numpy()


@pytest.mark.parametrize("S", [1, 2, 5])
def test_zero_gaps_give_the_grus_bits_and_no_ode_gradient(S):
    base = case_of(PROP[:4] + (S,), seed=2)
    B, T = PROP[:2]
    case = dict(base, dt=np.zeros((B, T)), dt_out=np.zeros(B))
    got = run_op(case)
    assert np.array_equal(bits(got["hs"]), bits(_gru(case)))
    assert np.array_equal(bits(got["z"]), bits(got["hs"][:, -1]))
    assert not got["dWf"].any() and not got["dbf"].any()
    # the case's fp64 reference is gru_ref's GRU with g_z added to the last state's gradient (test_ts_gru_host.py)
    check_parity(got, case, keys=("hs", "z", "dx", "dW", "dU", "db"), label="dt=0")


def test_a_zero_ode_gives_the_grus_forward_bits_for_any_gaps():
    base = case_of(PROP, seed=2)
    H = PROP[3]
    case = dict(base, Wf=np.zeros((H, H)), bf=np.zeros(H))
    got = run_op(case, wanted=())
    assert np.array_equal(bits(got["hs"]), bits(_gru(case)))
    assert np.array_equal(bits(got["z"]), bits(got["hs"][:, -1]))


def test_repeats_are_bit_identical():
    case = case_of((300, 20, 16, 16, 2))
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    assert all(first[k] is not None for k in ("hs", "z") + ref.GRADS)


def test_a_sample_keeps_its_bits_alone_moved_and_in_another_batch():
    case = case_of((37, 7, 8, 12, 3), seed=4)
    full = run_op(case, wanted=("x",))
    per_sample = ("x", "dt", "dt_out", "mask", "g_hs", "g_last", "g_z")
    for pick in ([5], [36, 5, 0], list(range(20, 37)) + [5] + list(range(20))):
        pick = np.array(pick)
        sub = dict(case, shape=(len(pick),) + case["shape"][1:], **{k: case[k][pick] for k in per_sample})
        got = run_op(sub, wanted=("x",))
        for k in ("hs", "z", "dx"):
            assert np.array_equal(bits(got[k]), bits(full[k][pick])), (k, len(pick))


def test_masked_steps_carry_the_state_and_an_all_masked_sample_evolves_zero():
    B, T, K, H, S = PROP
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0           # leading padding
    m[:, 5] = 0
    m[1, 7:] = 0           # trailing padding
    m[4] = 0               # an all-masked sample
    case = ref.make_case(*PROP, seed=2, mask=m)
    case["dt_out"][4] = 1.25
    got = run_op(case)
    hs = got["hs"]
    assert not hs[:, :2].any() and np.array_equal(bits(hs[:, 5]), bits(hs[:, 4])) and hs[0, 2].any()
    for t in range(7, T):
        assert np.array_equal(bits(hs[1, t]), bits(hs[1, 6]))
    assert not hs[4].any() and not got["dx"][4].any() and not got["dx"][m == 0].any()
    # z of the all-masked sample: the zero state moved by dt_out, every unit the same chain from bf
    _, z_ref, _, _ = ref.reference(case)
    assert got["z"][4].any() and np.abs(got["z"][4] - z_ref[4]).max() <= 1e-6
    check_parity(got, case, label="masked")


def test_no_mask_is_the_all_ones_mask_bit_for_bit():
    case = case_of(PROP, seed=2, mask=None)
    same_bits(run_op(case), run_op(dict(case, mask=np.ones(PROP[:2], np.uint8))))


def test_masked_inputs_are_never_used():
    case = case_of(PROP, seed=2)
    live = case["mask"].astype(bool)
    poisoned = dict(case, x=np.where(live[:, :, None], case["x"], np.nan), dt=np.where(live, case["dt"], np.nan))
    clean, dirty = run_op(case), run_op(poisoned)
    for k, v in dirty.items():
        if v is not None:
            assert np.isfinite(v).all(), k
    same_bits(clean, dirty)


def test_needs_input_grad_is_honoured():
    case = case_of((9, 6, 8, 12, 2))
    full = run_op(case)
    for wanted in (("x",), tuple(ref.PARAMS), ("Wf", "bf"), ("x", "b")):
        got = run_op(case, wanted=wanted)
        for k in NAMES:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["hs"]), bits(full["hs"])) and np.array_equal(bits(got["z"]), bits(full["z"]))
    t = dev(case["dt"]).requires_grad_()
    with pytest.raises(ValueError, match="no gradient"):
        Fn.ts_gru(dev(case["x"]), t, None, None, *(dev(case[k]) for k in ref.PARAMS))


def test_large_values_are_finite_and_inside_their_bars():
    """x, W, U times 8 (saturated gates) and every gap 1e3: the state leaves the GRU's [-1, 1] by hundreds, the ODE's tanh saturates."""
    case = large_case()
    check_parity(run_op(case), case, label="large")


# ---------------------------------------------------------------------------------------------------- 4. layer and model
LAYER_NAMES = dict(W="kernel", U="recurrent_kernel", b="bias", Wf="ode_kernel", bf="ode_bias")


def _run_layer(layer, case):
    x = dev(case["x"]).requires_grad_()
    inputs = [x, dev(case["dt"]), None if case.get("dt_out") is None else dev(case["dt_out"])]
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    with torch.no_grad():
        layer(inputs, mask=mask)        # lazy build
        for k, name in LAYER_NAMES.items():
            getattr(layer, name).copy_(dev(case[k]))
    layer.zero_grad()
    out, z = layer(inputs, mask=mask)
    g = np.array(case["g_hs"], np.float64)
    g[:, -1] += case["g_last"]
    torch.autograd.backward([out, z], [dev(g.astype(np.float32)), dev(case["g_z"])])
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = dict(hs=D(out), z=D(z), dx=D(x.grad))
    for k, name in LAYER_NAMES.items():
        res["d" + k] = D(getattr(layer, name).grad)
    return res


@pytest.mark.parametrize("shape", [(3, 5, 6, 8, 2), (3, 5, 8, 68, 2), (3, 5, 8, 8, 9), (3, 5, 56, 56, 2)], ids=["K=6", "H=68", "S=9", "LDS"])
def test_layer_outside_the_menu_takes_the_composed_path(shape):
    case = case_of(shape, seed=9)
    layer = layers.TimeStreamGRULayer(shape[3], steps=shape[4], return_sequences=True)
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["x"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


def test_layer_inside_the_menu_is_the_op():
    case = case_of((9, 6, 8, 12, 2))
    layer = layers.TimeStreamGRULayer(12, steps=2, return_sequences=True)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["x"]))
    same_bits(got, run_op(case))


def _dts_inputs(B, vocab, T, seed):
    _, idx, hist = behaviour_inputs(B, vocab, T, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    hist_dt = torch.tensor(rng.uniform(0, 2, (B, 1, T)), dtype=torch.float32, device="cuda")
    next_dt = torch.tensor(rng.uniform(0, 2, (B, 1)), dtype=torch.float32, device="cuda")
    return idx, (hist, hist_dt, next_dt)


def _dts_model(vocab, T, K, seed, **kw):
    torch.manual_seed(seed)
    info = models.make_sparse_info(vocab, embed_dim=K, names=["item", "user", "ctx"][:len(vocab)])
    return models.CTRModel(models.DTSInput(info, behavior=[("item", T)]), models.DTS(hidden_units=[32, 16], **kw)).cuda()


def test_dts_against_the_model_built_from_the_composed_layer(monkeypatch):
    """3 fields, one history of T = 6, B = 5.  The same weights through the composed layer (ts_gru_graph: fp32 torch ops): the output
    and every parameter gradient agree within 1e-5, the floor of the bars max(1e-5, 4 E32) (no fp64 model is built here, so the term
    that could only widen the bar is left out).  Other gaps alone give another output."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    idx, seq = _dts_inputs(B, vocab, T, seed=1)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], device="cuda")
    model = _dts_model(vocab, T, K, 3)
    model(None, idx, seq)
    with torch.no_grad():      # the zero initialisers would leave the ODE's bias and the GRU's out of the comparison
        beh = model.body.behaviors[0]
        beh.ode_bias.copy_(torch.linspace(-0.2, 0.2, K, device="cuda"))
        beh.bias.copy_(torch.linspace(-0.1, 0.1, 6 * K, device="cuda").reshape(2, 3 * K))

    def grads(seq_in):
        model.zero_grad()
        p = model(None, idx, seq_in)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads(seq)
    assert beh.fits_kernel_menu(torch.empty(B, T, K)) and beh.steps == 2 and not beh.return_sequences
    other = grads((seq[0], seq[1] * 1.5 + 0.25, seq[2]))
    assert np.abs(other["out"] - fused["out"]).max() > 1e-6             # hist_dt alone moves the output
    monkeypatch.setattr(layers.TimeStreamGRULayer, "fits_kernel_menu", lambda self, x: False)
    comp = grads(seq)
    monkeypatch.undo()
    assert set(fused) == set(comp) and "body.behaviors.0.ode_kernel" in fused and "body.behaviors.0.ode_bias" in fused
    for k in sorted(fused):
        direct = ref.norm_rel(fused[k], comp[k])
        print("DTS %-45s fused vs composed %.2e   bar 1.00e-05" % (k, direct))
        assert direct <= 1e-5, k
    assert np.abs(fused["body.behaviors.0.ode_kernel"]).max() > 0


def test_dts_trains_under_captured_adam_and_replays_the_eager_bits():
    """Three captured optim.Adam steps on three batches leave every parameter with the bits of three eager steps, and the loss falls
    over 20 captured steps on one batch."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        idx, (hist, hist_dt, next_dt) = _dts_inputs(B, vocab, T, seed=40 + s)
        batches.append((idx, hist, hist_dt, next_dt, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        model = _dts_model(vocab, T, K, 7)
        model(None, batches[0][0], tuple(batches[0][1:4]))
        opt = optim.Adam(model.parameters(), learning_rate=1e-2)

        def step(idx, hist, hist_dt, next_dt, y):
            opt.zero_grad()
            p = model(None, idx, (hist, hist_dt, next_dt))[:, 0]
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
    name = "body.behaviors.0.ode_kernel"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
