"""The masked self-attention over a behaviour sequence on the GPU (include/fil.h N3 fil_seqattn_*, functional.seq_self_attention,
layers.SeqSelfAttentionLayer, models.BST) against the fp64 restatement of tests/seq_attn_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (seq_attn_ref.bars).  The measured errors are
printed.  Where the reference gradient is exactly zero the kernel's must be."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import guarded
from tests import seq_attn_ref as ref
from tests.seq_common import behaviour_inputs, behaviour_model, bits, dev, dev_mask, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("x",) + ref.PARAMS
ids_of = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def case_of(shape, seed=0, mask="ragged", w_scale=1.0, use_scale=True):
    return ref.make_case(*shape, seed, mask=mask, w_scale=w_scale, use_scale=use_scale)


def run_op(case, wanted=NAMES):
    """functional.seq_self_attention forward + backward on the case -> dict of float64 numpy arrays (out and the gradients asked for)."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES}
    out = Fn.seq_self_attention(t["x"], dev_mask(case), t["Wq"], t["Wk"], t["Wv"], case["heads"], use_scale=case.get("use_scale", True))
    if any(v.requires_grad for v in t.values()):
        out.backward(dev(case["g"]))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = dict(out=D(out))
    for k, v in t.items():
        res["d" + k] = None if v.grad is None else D(v.grad)
    return res


def check_parity(got, case, keys=None, label=""):
    out, bwd, e32 = ref.reference(case)
    got = {k: v for k, v in got.items() if v is not None and (keys is None or k in keys)}
    err, bar = ref.errors(got, out, bwd), ref.bars(e32)
    print("%s %s  " % (label, case["shape"]) + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
        want = out if k == "out" else bwd[k]
        assert not np.asarray(got[k]).reshape(want.shape)[want == 0].any(), (k, "not exactly zero where the reference is")
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY_SHAPES = [(1, 1, 4, 1, 4),          # the minimum
                 (3, 2, 4, 2, 4),          # two positions, two heads
                 (5, 50, 16, 2, 8),        # the benchmark's
                 (3, 7, 12, 3, 4),         # K / 4, H and T odd
                 (2, 63, 8, 1, 8), (2, 64, 8, 1, 8), (2, 65, 8, 1, 8),      # the wave-width edges of a key loop
                 (2, 256, 16, 4, 4)]       # the longest history
CORNERS = [(3, 64, 64, 8, 8), (2, 5, 64, 1, 64), (2, 5, 4, 1, 4)]


@pytest.mark.parametrize("shape", PARITY_SHAPES + CORNERS, ids=ids_of)
def test_parity_with_the_fp64_reference(shape):
    case = case_of(shape)
    check_parity(run_op(case), case)


@pytest.mark.parametrize("use_scale", [True, False])
def test_use_scale_both_ways(use_scale):
    case = case_of((4, 9, 8, 2, 4), seed=1, use_scale=use_scale)
    got = run_op(case)
    check_parity(got, case, label="use_scale=%s" % use_scale)
    other = run_op(dict(case, use_scale=not use_scale))
    assert not np.array_equal(got["out"], other["out"])


@pytest.mark.parametrize("shape", [(3, 7, 12, 3, 4), (5, 50, 16, 2, 8)], ids=ids_of)
def test_peaked_rows_keep_their_digits(shape):
    """Wq, Wk x 24: every softmax row has one weight near 1.  The bars are the same formula (E32 itself rises here)."""
    case = case_of(shape, w_scale=24.0)
    check_parity(run_op(case), case, label="peaked")


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
EDGE = (3, 4, 1, 4)            # T, K, H, D
SHAPES_OF = lambda B, T, K, H, D: dict(out=(B, T, H * D), dx=(B, T, K), dWq=(K, H * D), dWk=(K, H * D), dWv=(K, H * D))


def run_raw(case, subset=ref.GRADS):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace guarded behind its
    bytes, `saved` NaN-filled before the forward (masked positions are never written and never used)."""
    lib = _lib.load()
    B, T, K, H, D = case["shape"]
    us = int(case.get("use_scale", True))
    t = {k: dev(case[k]) for k in NAMES + ("g",)}
    mask = dev_mask(case)
    shapes = SHAPES_OF(B, T, K, H, D)
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in ["out"] + list(subset)}
    nsv = lib.fil_seqattn_saved_bytes(B, T, K, H, D)
    assert B * T * 3 * H * D * 4 <= nsv <= B * T * (3 * H * D + H) * 4 + 256
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    check(lib.fil_seqattn_fwd(ptr(t["x"]), ptr(mask), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), bufs["out"].ptr, saved.ptr, B, T, K, H, D, us,
                              stream_ptr()), "fil_seqattn_fwd")
    nws = lib.fil_seqattn_bwd_workspace_bytes(B, T, K, H, D)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    out = lambda k: bufs[k].ptr if k in bufs else None
    params = any(k in bufs for k in ("dWq", "dWk", "dWv"))
    check(lib.fil_seqattn_bwd(ptr(t["x"]), ptr(mask), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), bufs["out"].ptr, saved.ptr, ptr(t["g"]),
                              out("dx"), out("dWq"), out("dWk"), out("dWv"), ptr(ws) if params else None, nws if params else 0, B, T, K, H, D,
                              us, stream_ptr()), "fil_seqattn_bwd")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_seqattn_bwd", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64) for k, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def edge_case(B):
    """Samples of three positions: the seed is the first whose sums over (b, t) are well conditioned in the fp64 reference
    (seq_attn_ref.conditioned_case, which says why; the seed is printed)."""
    return ref.conditioned_case(B, *EDGE)


@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which):
    """T = 3, K = 4, one head of 4.  tile - 1 (a partial tile) and tile: one workgroup, one partial; tile + 1: two, the second with one
    sample.  Every output and `saved` sit between guard words, the workspace has guard bytes behind it."""
    tile = Fn.seq_attn_plan(1, *EDGE)["tile"]
    assert tile == 85                                             # floor(256 / 3): one (head, row) pair per thread
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    plan = Fn.seq_attn_plan(B, *EDGE)
    assert plan["tile"] == tile and plan["partials"] == (2 if which == "tile+1" else 1)
    case = edge_case(B)
    print("seed", case["seed"])
    check_parity(run_raw(case), case, label=which)


def test_inference_call_saves_nothing_and_has_the_training_calls_bits():
    case = edge_case(5)
    lib = _lib.load()
    B, T, K, H, D = case["shape"]
    t = {k: dev(case[k]) for k in NAMES}
    out = guarded.GuardedOutput((B, T, H * D), np.uint32, "out")
    check(lib.fil_seqattn_fwd(ptr(t["x"]), ptr(dev_mask(case)), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), out.ptr, None, B, T, K, H, D, 1,
                              stream_ptr()), "fil_seqattn_fwd")
    torch.cuda.synchronize()
    assert np.array_equal(out.read("out").view(np.int32), bits(run_raw(case)["out"]))
    x = dev(case["x"])
    with torch.no_grad():
        y = Fn.seq_self_attention(x, dev_mask(case), t["Wq"], t["Wk"], t["Wv"], H)
    assert np.array_equal(bits(y.cpu().numpy()), out.read("out").view(np.int32))


def test_past_the_grid_cap_a_workgroup_walks_a_second_tile():
    """T = 1, one head: a tile of 256 samples, one per thread, so B = cap * 256 + 1 leaves one workgroup a second tile of one
    sample."""
    T, K, H, D = 1, 4, 1, 4
    cap = Fn.seq_attn_plan(1, T, K, H, D)["cap"]
    B = cap * 256 + 1
    plan = Fn.seq_attn_plan(B, T, K, H, D)
    assert plan["tile"] == 256 and plan["grid"] == cap and plan["partials"] == cap
    case = case_of((B, T, K, H, D), mask=None)
    check_parity(run_op(case), case, label="cap*tile+1")


def test_empty_batch_is_a_no_op():
    x = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(4, 8, device="cuda", requires_grad=True) for _ in range(3)]
    out = Fn.seq_self_attention(x, None, *w, 2)
    assert out.shape == (0, 3, 8)
    out.sum().backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("subset", [("dx",), ("dWq", "dWk", "dWv"), ("dWk",)], ids=["dx", "params", "dWk"])
def test_null_output_subsets_have_the_full_backwards_bits(subset):
    case = edge_case(5)
    full = run_raw(case)
    part = run_raw(case, subset=subset)
    assert set(part) == {"out"} | set(subset)
    same_bits(part, full, subset)
    with pytest.raises(_lib.FilError):                                  # nothing is left to compute: FIL_ERR_ARG
        run_raw(case, subset=())


# ---------------------------------------------------------------------------------------------------- 3. exact properties
PROP = (6, 10, 8, 2, 4)


@pytest.mark.parametrize("shape", [PROP, (300, 20, 16, 2, 8)], ids=ids_of)
def test_repeats_are_bit_identical(shape):
    case = case_of(shape, seed=2)
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    check_parity(first, case)


def test_no_mask_is_the_all_ones_mask_bit_for_bit():
    case = case_of(PROP, seed=2, mask=None)
    same_bits(run_op(case), run_op(dict(case, mask=np.ones(PROP[:2], np.uint8))))


def test_masked_inputs_are_never_used():
    case = case_of(PROP, seed=2)
    live = case["mask"].astype(bool)
    assert not live.all() and live.any()
    poisoned = dict(case, x=np.where(live[:, :, None], case["x"], np.nan), g=np.where(live[:, :, None], case["g"], np.nan))
    clean, dirty = run_op(case), run_op(poisoned)
    for k, v in dirty.items():
        assert np.isfinite(v).all(), k
    same_bits(clean, dirty)


def test_masked_positions_are_exactly_zero_and_an_all_masked_sample_gives_nothing():
    B, T = PROP[:2]
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0           # leading padding
    m[:, 5] = 0
    m[1, 7:] = 0           # trailing padding
    m[4] = 0               # an all-masked sample
    case = ref.make_case(*PROP, seed=2, mask=m)
    got = run_op(case)
    assert not got["out"][m == 0].any() and not got["dx"][m == 0].any() and got["out"][m != 0].any() and got["dx"][m != 0].any()
    assert not got["out"][4].any() and not got["dx"][4].any()
    check_parity(got, case, label="masked")
    # ... and contributes nothing: without it the parameter gradients have the same bits (the tile holds every sample either way)
    keep = [0, 1, 2, 3, 5]
    less = dict(case, shape=(5,) + PROP[1:], x=case["x"][keep], g=case["g"][keep], mask=m[keep])
    without = run_op(less)
    for k in ("dWq", "dWk", "dWv"):
        assert np.array_equal(bits(without[k]), bits(got[k])), k


def test_a_sample_alone_has_the_bits_of_its_rows_in_the_batch():
    case = case_of(PROP, seed=2)
    got = run_op(case)
    for b in range(PROP[0]):
        one = dict(case, shape=(1,) + PROP[1:], x=case["x"][b:b + 1], g=case["g"][b:b + 1], mask=case["mask"][b:b + 1])
        alone = run_op(one)
        assert np.array_equal(bits(alone["out"][0]), bits(got["out"][b])) and np.array_equal(bits(alone["dx"][0]), bits(got["dx"][b])), b
    # ... and inside a batch large enough for another tile size and a second tile
    big = case_of((300, 10, 8, 2, 4), seed=3)
    assert Fn.seq_attn_plan(300, *PROP[1:])["tile"] == Fn.seq_attn_plan(1, *PROP[1:])["tile"] and Fn.seq_attn_plan(300, *PROP[1:])["grid"] > 1
    whole = run_op(big)
    b = 299
    one = dict(big, shape=(1,) + PROP[1:], x=big["x"][b:b + 1], g=big["g"][b:b + 1], mask=big["mask"][b:b + 1])
    alone = run_op(one)
    assert np.array_equal(bits(alone["out"][0]), bits(whole["out"][b])) and np.array_equal(bits(alone["dx"][0]), bits(whole["dx"][b]))


def test_one_live_slot_returns_its_value_row_and_no_score_gradient():
    B, T = PROP[:2]
    m = np.zeros((B, T), np.uint8)
    for b in range(B):
        m[b, (3 * b) % T] = 1
    case = ref.make_case(*PROP, seed=4, mask=m)
    out_ref, bwd, e32 = ref.reference(case)
    got = run_op(case)
    live = m.astype(bool)
    assert ref.norm_rel(got["out"][live], bwd["v_rows"][live]) <= ref.bars(e32)["out"]
    assert not bwd["dWq"].any() and not bwd["dWk"].any() and bwd["dWv"].any()
    assert not got["dWq"].any() and not got["dWk"].any()                    # ds = 0 exactly
    check_parity(got, case, label="one live slot")


def test_needs_input_grad_is_honoured():
    case = case_of((9, 6, 8, 2, 4))
    full = run_op(case)
    for wanted in (("x",), tuple(ref.PARAMS), ("Wk",), ("x", "Wv")):
        got = run_op(case, wanted=wanted)
        for k in NAMES:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["out"]), bits(full["out"]))
    none = run_op(case, wanted=())
    assert np.array_equal(bits(none["out"]), bits(full["out"]))


# ---------------------------------------------------------------------------------------------------- 4. layer and model
LAYER_NAMES = dict(Wq="query_w", Wk="key_w", Wv="value_w")


def _run_layer(layer, case, dtype=torch.float32):
    B, T, K, H, D = case["shape"]
    x = dev(case["x"]).to(dtype).requires_grad_()
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    with torch.no_grad():
        layer(x, mask=mask)        # lazy build
        for k, name in LAYER_NAMES.items():
            getattr(layer, name).copy_(dev(case[k]).reshape(K, H, D))
    layer.zero_grad()
    out = layer(x, mask=mask)
    assert out.dtype == torch.float32 and out.shape == (B, T, H * D)
    out.backward(dev(case["g"]))
    torch.cuda.synchronize()
    Dn = lambda v: v.detach().cpu().double().numpy()
    res = dict(out=Dn(out), dx=Dn(x.grad))
    for k, name in LAYER_NAMES.items():
        res["d" + k] = Dn(getattr(layer, name).grad).reshape(K, H * D)
    return res


@pytest.mark.parametrize("shape", [(3, 5, 6, 2, 4), (3, 5, 8, 1, 68), (2, 257, 8, 1, 4)], ids=["K=6", "HD=68", "T=257"])
def test_layer_outside_the_menu_takes_the_composed_path(shape):
    case = case_of(shape, seed=9)
    layer = layers.SeqSelfAttentionLayer(shape[3], shape[4])
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["x"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


def test_layer_inside_the_menu_is_the_op():
    case = case_of((9, 6, 8, 2, 4))
    layer = layers.SeqSelfAttentionLayer(2, 4)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["x"]))
    same_bits(got, run_op(case))


def test_layer_computes_a_half_precision_input_in_fp32():
    case = case_of((9, 6, 8, 2, 4), seed=6)
    r16 = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    case16 = dict(case, x=r16(case["x"]))
    layer = layers.SeqSelfAttentionLayer(2, 4)
    half = _run_layer(layer, case16, dtype=torch.bfloat16)          # asserts an fp32 output; the input gradient comes back in bf16
    check_parity(half, case16, keys=("out", "dWq", "dWk", "dWv"), label="bf16 in")


def _bst_model(vocab, T, K, seed, **kw):
    return behaviour_model(lambda: models.BST(hidden_units=[32, 16], **kw), vocab, T, K, seed)


def test_bst_against_the_model_built_from_the_composed_layer(monkeypatch):
    """3 fields, one history of T = 6, B = 5, K = 8, 2 heads.  The same weights through the composed layer (seq_self_attention_graph:
    fp32 torch ops): the output and every parameter gradient agree within 1e-5, the floor of the bars max(1e-5, 4 E32) (no fp64 model
    is built here, so the term that could only widen the bar is left out)."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    _, idx, hist = behaviour_inputs(B, vocab, T, seed=1)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], device="cuda")
    model = _bst_model(vocab, T, K, 3)

    def grads():
        model.zero_grad()
        p = model(None, idx, hist)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads()
    beh = model.body.behaviors[0]
    assert beh.atten.fits_kernel_menu(torch.empty(B, T + 1, K)) and beh.atten.heads == 2 and beh.atten.head_dim == 4
    monkeypatch.setattr(layers.SeqSelfAttentionLayer, "fits_kernel_menu", lambda self, x: False)
    comp = grads()
    monkeypatch.undo()
    names = ("atten.query_w", "atten.key_w", "atten.value_w", "pos_embed", "ffn1.kernel", "ffn2.bias", "ln1_gamma", "ln2_beta")
    assert set(fused) == set(comp) and all("body.behaviors.0." + n in fused for n in names), sorted(fused)
    for k in sorted(fused):
        direct = ref.norm_rel(fused[k], comp[k])
        print("BST %-45s fused vs composed %.2e   bar 1.00e-05" % (k, direct))
        assert direct <= 1e-5, k
    assert np.abs(fused["body.behaviors.0.atten.query_w"]).max() > 0


def test_bst_trains_under_captured_adam_and_replays_the_eager_bits():
    """The loss falls over 20 captured optim.Adam steps on one batch, and three captured steps on three batches leave every
    parameter with the bits of three eager steps."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx, hist = behaviour_inputs(B, vocab, T, seed=40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        model = _bst_model(vocab, T, K, 7)
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
    name = "body.behaviors.0.atten.query_w"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
