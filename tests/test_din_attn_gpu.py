"""The DIN attention pooling on the GPU (include/fil.h N3 fil_din_*, functional.din_attention, layers.DinAttentionLayer,
models.DINInput / DIN) against the fp64 restatement of tests/din_attn_ref.py.

Error measure: norm-relative against the fp64 reference for out and every gradient but db3; db3 (a cancelling sum, exactly zero in
softmax mode) in units of sum |ds_t|.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32 torch restatement of the same
graph on the same inputs, computed here on the CPU (din_attn_ref.bars).  The measured errors are printed."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import din_attn_ref as ref
from tests.seq_common import PAD, SENTINEL, behaviour_inputs, behaviour_model, bits, dev, dev_mask, guarded, guards_intact

pytestmark = pytest.mark.gpu

ACTS = ["prelu", "sigmoid"]
MODES = [False, True]
MODE_IDS = ["raw", "softmax"]
NAMES = ("q", "keys") + ref.PARAMS
both = lambda f: pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)(pytest.mark.parametrize("activation", ACTS)(f))


@functools.lru_cache(maxsize=None)
def case_of(shape, activation, softmax, seed=0, mask="ragged", alpha_max=0.3):
    return ref.make_case(*shape, activation, softmax, seed, mask=mask, alpha_max=alpha_max)


def run_op(case, wanted=NAMES):
    """functional.din_attention forward + backward on the case -> dict of float64 numpy arrays (out and the gradients asked for)."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES if case.get(k) is not None}
    out = Fn.din_attention(t["q"], t["keys"], dev_mask(case), t["W1"], t["b1"], t.get("alpha1"), t["W2"], t["b2"], t.get("alpha2"),
                           t["w3"], t["b3"], softmax=case["softmax"], activation=case["activation"])
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
    print("%s %s %s %s  " % (label, case["shape"], case["activation"], "softmax" if case["softmax"] else "raw")
          + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY_SHAPES = [(1, 1, 4, 1, 1),
                 (3, 3, 4, 4, 2),
                 (5, 63, 8, 16, 8), (5, 64, 8, 16, 8), (5, 65, 8, 16, 8),      # either side of one wave of slots
                 (3, 129, 4, 5, 3),          # a third trip; H not a multiple of 4
                 (7, 50, 16, 80, 40),        # the benchmark's
                 (3, 20, 12, 37, 9),         # K / 4 odd, odd widths
                 (4, 64, 16, 36, 16)]
CORNERS = [(2, 256, 16, 128, 64), (2, 256, 64, 36, 16), (3, 50, 32, 80, 40)]   # the menu's corners; 4 K H1 + H1 H2 = 16384 exactly
ids_of = lambda s: "x".join(map(str, s))


@both
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=ids_of)
def test_parity_with_the_fp64_reference(shape, activation, softmax):
    case = case_of(shape, activation, softmax)
    got = run_op(case)
    if softmax and shape[1] == 1:   # one slot: its weight is 1, ds = 0 and dq and every parameter gradient are exactly zero
        check_parity(got, case, keys=("out", "dkeys"))
        for k, v in got.items():
            if k not in ("out", "dkeys") and v is not None:
                assert not v.any(), k
    else:
        check_parity(got, case)


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", CORNERS, ids=ids_of)
def test_the_corners_of_the_menu(shape, softmax):
    """Sigmoid only: the PReLU margin rejects nearly every draw at these sizes."""
    case = case_of(shape, "sigmoid", softmax)
    check_parity(run_op(case), case)


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
def run_raw(case):
    """The two entry points called directly: outputs inside sentinel-guarded allocations, the workspace NaN-poisoned."""
    lib = _lib.load()
    B, T, K, H1, H2 = case["shape"]
    sig = case["activation"] == "sigmoid"
    flags = (_lib.FIL_DIN_SOFTMAX if case["softmax"] else 0) | (_lib.FIL_DIN_SIGMOID if sig else 0)
    t = {k: (None if case.get(k) is None else dev(case[k])) for k in NAMES + ("g",)}
    mask = dev_mask(case)
    ins = [ptr(t["q"]), ptr(t["keys"]), ptr(mask)] + [ptr(t[k]) for k in ref.PARAMS]
    stats = torch.full((B, T + 2), float("nan"), device="cuda")
    shapes = dict(out=(B, K), dq=(B, K), dkeys=(B, T, K), dW1=(4 * K, H1), db1=(H1,), dalpha1=(H1,), dW2=(H1, H2), db2=(H2,), dalpha2=(H2,),
                  dw3=(H2,), db3=(1,))
    bufs = {name: guarded(shape) for name, shape in shapes.items()}
    check(lib.fil_din_fwd(*ins, ptr(bufs["out"][1]), ptr(stats), B, T, K, H1, H2, flags, stream_ptr()), "fil_din_fwd")
    nws = lib.fil_din_bwd_workspace_bytes(B, T, K, H1, H2)
    ws_buf = torch.full((PAD + nws // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    ws_buf[:PAD] = SENTINEL
    ws_buf[-PAD:] = SENTINEL
    ws = ws_buf[PAD:PAD + nws // 4]
    check(lib.fil_din_bwd(*ins, ptr(bufs["out"][1]), ptr(stats), ptr(t["g"]), *[ptr(bufs[k][1]) for k in ref.GRADS], ptr(ws), nws, B, T, K,
                          H1, H2, flags, stream_ptr()), "fil_din_bwd")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert guards_intact(buf), name
    assert guards_intact(ws_buf)
    res = {k: v[1].detach().cpu().double().numpy() for k, v in bufs.items()}
    if sig:
        assert not res["dalpha1"].any() and not res["dalpha2"].any()
    return res


EDGE = (3, 4, 4, 2)


@functools.lru_cache(maxsize=None)
def edge_case(B, activation, softmax):
    """A few samples of three slots and two output units: the seed is the first whose cancelling sums are well conditioned in the
    fp64 reference (din_attn_ref.conditioned_case, which says why).  The batch of cap * tile + 1 samples is seed 0 as everywhere
    else: over thousands of terms the roundings average out and no single draw decides the digits."""
    if B > 8:
        return case_of((B,) + EDGE, activation, softmax)
    return ref.conditioned_case(B, *EDGE, activation, softmax)


@both
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1", "cap*tile+1"])
def test_batch_tile_and_grid_edges(which, activation, softmax):
    """T = 3, K = 4, H1 = 4, H2 = 2 (the fp64 reference costs nothing).  tile - 1 and tile: exactly one partial; tile + 1: two, the last
    workgroup with one sample; cap * tile + 1: a second trip through the grid-stride loop that one workgroup makes with one sample."""
    plan = Fn.din_plan(1, *EDGE)
    tile, cap = plan["tile"], plan["cap"]
    B = max(1, {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "cap*tile+1": cap * tile + 1}[which])
    parts = Fn.din_plan(B, *EDGE)["partials"]
    assert parts == {"tile-1": 1, "tile": 1, "tile+1": 2 if tile + 1 <= cap * tile else 1, "cap*tile+1": cap}[which]
    case = edge_case(B, activation, softmax)
    check_parity(run_raw(case), case, label=which)


def test_empty_batch_is_a_no_op():
    q = torch.empty(0, 4, device="cuda", requires_grad=True)
    keys = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(s, device="cuda", requires_grad=True) for s in ((16, 4), (4,), (4,), (4, 2), (2,), (2,), (2,), (1,))]
    out = Fn.din_attention(q, keys, None, *w)
    assert out.shape == (0, 4)


# ---------------------------------------------------------------------------------------------------- 3. mask
MASK_SHAPE = (6, 10, 8, 16, 8)


def _pattern(kind, B, T):
    m = np.zeros((B, T), np.uint8)
    if kind == "first":
        m[:, 0] = 1
    elif kind == "last":
        m[:, -1] = 1
    elif kind == "alternating":
        m[:, ::2] = 1
    else:
        m[:] = 1
    return m


@both
@pytest.mark.parametrize("kind", ["first", "last", "alternating"])
def test_mask_patterns(kind, activation, softmax):
    B, T = MASK_SHAPE[:2]
    case = ref.make_case(*MASK_SHAPE, activation, softmax, seed=2, mask=_pattern(kind, B, T))
    got = run_op(case)
    if softmax and kind != "alternating":      # one live slot: exact (section 4); dq and the parameter gradients are exactly zero
        check_parity(got, case, keys=("out", "dkeys"))
    else:
        check_parity(got, case, label=kind)
    assert not got["dkeys"][case["mask"] == 0].any()


@both
def test_no_mask_is_the_all_ones_mask_bit_for_bit(activation, softmax):
    case = case_of(MASK_SHAPE, activation, softmax, seed=2, mask=None)
    a = run_op(case)
    b = run_op(dict(case, mask=_pattern("all", *MASK_SHAPE[:2])))
    for k, v in a.items():
        if v is not None:
            assert np.array_equal(bits(v), bits(b[k])), k
    check_parity(a, case)


@both
@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
def test_masked_keys_are_never_used(fill, activation, softmax):
    case = case_of(MASK_SHAPE, activation, softmax, seed=2)
    live = case["mask"].astype(bool)
    zeroed = run_op(dict(case, keys=np.where(live[:, :, None], case["keys"], 0.0)))
    filled = run_op(dict(case, keys=np.where(live[:, :, None], case["keys"], fill)))
    for k, v in zeroed.items():
        if v is not None:
            assert np.isfinite(filled[k]).all(), k
            assert np.array_equal(bits(v), bits(filled[k])), k
    assert not filled["dkeys"][~live].any()


@both
def test_samples_without_a_live_slot(activation, softmax):
    B, T = MASK_SHAPE[:2]
    m = ref.make_mask(B, T, "ragged", np.random.default_rng(3))
    m[0] = 0
    m[3] = 0
    case = ref.make_case(*MASK_SHAPE, activation, softmax, seed=2, mask=m)
    got = run_op(case)
    for k in ("out", "dq", "dkeys"):
        assert not got[k][0].any() and not got[k][3].any(), k
    check_parity(got, case, label="empty samples")


# ---------------------------------------------------------------------------------------------------- 4. exact cases
@pytest.mark.parametrize("activation", ACTS)
@pytest.mark.parametrize("T", [1, 9])
def test_softmax_with_one_live_slot_is_that_key_bit_for_bit(T, activation):
    """The weight is exactly 1: out is the key, ds is exactly 0 (g.out is summed in the order of g.k), so dkeys of that slot is g and
    dq and every parameter gradient are exactly 0."""
    B, K = 6, 8
    rng = np.random.default_rng(7)
    pos = rng.integers(0, T, B)
    m = np.zeros((B, T), np.uint8)
    m[np.arange(B), pos] = 1
    case = ref.make_case(B, T, K, 16, 8, activation, True, seed=4, mask=m)
    got = run_op(case)
    key = case["keys"][np.arange(B), pos].astype(np.float32)
    assert np.array_equal(bits(got["out"]), bits(key))
    assert np.array_equal(bits(got["dkeys"][np.arange(B), pos]), bits(case["g"].astype(np.float32)))
    assert not got["dkeys"][m == 0].any()
    for k, v in got.items():
        if k not in ("out", "dkeys") and v is not None:
            assert not v.any(), k


@pytest.mark.parametrize("activation", ACTS)
def test_zero_w3(activation):
    """Softmax: every score is b3, out is the mean of the live keys.  Raw: a_t = b3 = c, out = c * the sum of the live keys, and
    nothing flows into the two hidden layers."""
    base = case_of(MASK_SHAPE, activation, True, seed=2)
    live = base["mask"].astype(bool)
    ksum = (base["keys"] * live[:, :, None]).sum(1)
    zero = dict(base, w3=np.zeros_like(base["w3"]))
    got = run_op(zero)
    assert ref.norm_rel(got["out"], ksum / live.sum(1, keepdims=True)) < 1e-6
    c = 0.75
    raw = dict(zero, softmax=False, b3=np.array([c]))
    got = run_op(raw)
    assert ref.norm_rel(got["out"], c * ksum) < 1e-6
    for k in ("dW1", "dW2", "db1", "db2", "dalpha1", "dalpha2"):
        if got.get(k) is not None:
            assert not got[k].any(), k
    assert not got["dq"].any()
    check_parity(got, raw, keys=("out", "dkeys", "dw3", "db3"), label="w3 = 0")


# ---------------------------------------------------------------------------------------------------- 5. range
@pytest.mark.parametrize("activation", ACTS)
def test_scores_of_a_thousand(activation):
    base = case_of(MASK_SHAPE, activation, True, seed=2)
    case = dict(base, w3=(base["w3"] * 1e3).astype(np.float32).astype(np.float64))
    got = run_op(case)
    for k, v in got.items():
        if v is not None:
            assert np.isfinite(v).all(), k
    check_parity(got, case, keys=("out",), label="w3 x 1e3")


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shift", [50.0, -50.0])
def test_saturated_sigmoid_units(shift, softmax):
    base = case_of(MASK_SHAPE, "sigmoid", softmax, seed=2)
    b1 = base["b1"].copy()
    b1[::2] += shift
    case = dict(base, b1=b1.astype(np.float32).astype(np.float64))
    check_parity(run_op(case), case, label="b1 %+g" % shift)


# ---------------------------------------------------------------------------------------------------- 6. PReLU particulars
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
def test_zero_slopes_without_gradient_are_relu(softmax):
    case = case_of(MASK_SHAPE, "prelu", softmax, seed=2, alpha_max=0.0)
    assert not case["alpha1"].any() and not case["alpha2"].any()
    got = run_op(case, wanted=tuple(k for k in NAMES if not k.startswith("alpha")))
    assert got["dalpha1"] is None and got["dalpha2"] is None
    p = ref._parts(case)
    assert np.array_equal(p["h1"], np.maximum(p["u1"], 0.0)) and (p["u1"] < 0).any()
    check_parity(got, case, label="relu")


def test_sigmoid_accepts_no_slopes():
    case = case_of(MASK_SHAPE, "sigmoid", False, seed=2)
    assert case["alpha1"] is None and case["alpha2"] is None
    with_none = run_op(case)
    with_junk = run_op(dict(case, alpha1=np.full(16, 7.0), alpha2=np.full(8, -3.0)))     # ignored
    assert np.array_equal(bits(with_none["out"]), bits(with_junk["out"])) and np.array_equal(bits(with_none["dW1"]), bits(with_junk["dW1"]))
    assert not with_junk["dalpha1"].any() and not with_junk["dalpha2"].any()


# ---------------------------------------------------------------------------------------------------- 7. determinism and selection
@both
def test_repeats_are_bit_identical(activation, softmax):
    case = case_of((300, 50, 16, 80, 40), activation, softmax)
    first, second = run_op(case), run_op(case)
    for k, v in first.items():
        if v is not None:
            assert np.array_equal(bits(v), bits(second[k])), k
    check_parity(first, case)


@both
def test_needs_input_grad_is_honoured(activation, softmax):
    """Only the gradients that are asked for are computed (q and keys alone: no parameter pass and no workspace), and each has the
    bits of the full backward."""
    case = case_of((9, 12, 8, 16, 8), activation, softmax)
    full = run_op(case)
    present = [k for k in NAMES if case.get(k) is not None]
    for wanted in (("q", "keys"), tuple(ref.PARAMS), ("w3",), ("keys", "b1")):
        got = run_op(case, wanted=wanted)
        for k in present:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["out"]), bits(full["out"]))


# ---------------------------------------------------------------------------------------------------- 8. layer and model
LAYER_NAMES = dict(W1="att_w1", b1="att_b1", alpha1="att_alpha1", W2="att_w2", b2="att_b2", alpha2="att_alpha2", w3="att_w3", b3="att_b3")


def _set_weights(layer, case):
    with torch.no_grad():
        for k, name in LAYER_NAMES.items():
            if case.get(k) is not None:
                getattr(layer, name).copy_(dev(case[k]).reshape(getattr(layer, name).shape))


def _run_layer(layer, case, composed=False, query_3d=True, dtype=torch.float32):
    q = dev(case["q"]).to(dtype).requires_grad_()
    keys = dev(case["keys"]).to(dtype).requires_grad_()
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    query = q.unsqueeze(1) if query_3d else q
    layer([query.detach(), keys.detach()], mask=mask)        # lazy build
    _set_weights(layer, case)
    layer.zero_grad()
    if composed:
        out = layer._composed(q, keys, mask).unsqueeze(1)
    else:
        out = layer([query, keys], mask=mask)
    assert out.shape == (q.shape[0], 1, q.shape[1]) and out.dtype == torch.float32
    out.backward(dev(case["g"]).unsqueeze(1))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = dict(out=D(out[:, 0]), dq=D(q.grad), dkeys=D(keys.grad))
    for k, name in LAYER_NAMES.items():
        p = getattr(layer, name, None)
        res["d" + k] = None if p is None or p.grad is None else D(p.grad).reshape(np.asarray(case[k]).shape)
    return res


@both
def test_layer_against_its_composed_path(activation, softmax):
    shape = (9, 12, 8, 16, 8)
    case = case_of(shape, activation, softmax, seed=6)
    out, bwd, _ = ref.reference(case)
    layer = layers.DinAttentionLayer(hidden_units=shape[3:], activation=activation, softmax=softmax)
    fused = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["q"]), dev(case["keys"]))
    comp = _run_layer(layer, case, composed=True)
    present = lambda d: {k: v for k, v in d.items() if v is not None}
    e32 = ref.errors(present(comp), out, bwd)                  # the fp32 torch graph's own error
    vs64 = ref.errors(present(fused), out, bwd)
    for k in e32:
        bar = max(1e-5, 4 * e32[k])
        if k == "db3":
            direct = float(np.abs(fused[k] - comp[k]).max() / bwd["ds_abs"])
        else:
            direct = ref.norm_rel(fused[k], comp[k])
        print("layer %-8s fused vs composed %.2e   fused vs fp64 %.2e   composed vs fp64 (E32) %.2e   bar %.2e" % (k, direct, vs64[k], e32[k], bar))
        assert direct <= bar and vs64[k] <= bar, k
    assert float(np.abs(fused["dW1"]).max()) > 0.0
    # a [B,K] query is the same call
    flat = _run_layer(layer, case, query_3d=False)
    for k, v in fused.items():
        if v is not None:
            assert np.array_equal(bits(v), bits(flat[k])), k


@both
@pytest.mark.parametrize("shape", [(3, 5, 6, 4, 2), (3, 5, 8, 130, 4)], ids=["K=6", "H1=130"])
def test_layer_outside_the_menu_takes_the_composed_path(shape, activation, softmax):
    case = case_of(shape, activation, softmax, seed=9)
    layer = layers.DinAttentionLayer(hidden_units=shape[3:], activation=activation, softmax=softmax)
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["q"]), dev(case["keys"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


def test_layer_computes_a_half_precision_input_in_fp32():
    case = case_of((9, 12, 8, 16, 8), "sigmoid", True, seed=6)
    r16 = lambda a: torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    case16 = dict(case, q=r16(case["q"]), keys=r16(case["keys"]))
    layer = layers.DinAttentionLayer(hidden_units=(16, 8), activation="sigmoid", softmax=True)
    half = _run_layer(layer, case16, dtype=torch.bfloat16)          # asserts an fp32 output
    full = _run_layer(layer, case16)                                 # the fused kernel on the same (bf16-representable) values
    assert ref.norm_rel(half["out"], full["out"]) < 1e-5


def _din_model(vocab, T, K, seed, **kw):
    return behaviour_model(lambda: models.DIN(att_hidden_units=(16, 8), hidden_units=[32, 16], **kw), vocab, T, K, seed)


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
def test_din_trains(softmax):
    vocab, T, K, B = [12, 5, 7], 6, 8, 64
    model = _din_model(vocab, T, K, 0, att_softmax=softmax)
    dense, idx, hist = behaviour_inputs(B, vocab, T, seed=1, n_dense=2)
    y = torch.tensor(np.random.default_rng(2).integers(0, 2, B), dtype=torch.float32, device="cuda")
    out = model(dense, idx, hist)
    assert out.shape == (B, 2)                      # MergeScoreLayer's softmax over two classes
    att = model.body.atten[0]
    assert att.fits_kernel_menu(torch.empty(B, K), torch.empty(B, T, K))
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    history = []
    w0 = att.att_w1.detach().clone()
    for _ in range(25):
        opt.zero_grad()
        p = model(dense, idx, hist)[:, 0]
        loss = torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y)
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    assert np.isfinite(history).all() and history[-1] < history[0] * 0.9, history[::6]
    assert not torch.equal(att.att_w1.detach(), w0)


def test_shared_table_gradient_is_the_sum_of_the_two_gathers():
    vocab, T, K, B = [12, 5], 6, 8, 33
    info = models.make_sparse_info(vocab, embed_dim=K, names=["item", "user"])
    fi = models.DINInput(info, behavior=[("item", T)]).cuda()
    _, idx, hist = behaviour_inputs(B, vocab, T, seed=3)
    fea = fi((None, idx, hist))
    keys, masks = fea.seq_embed_list
    assert len(fea.sparse_embed) == 2 and keys[0].shape == (B, T, K) and masks[0].shape == (B, T) and masks[0].dtype == torch.bool
    assert torch.equal(masks[0], hist[:, 0] != 0)
    table = fi.sparse_embed.embeddings
    assert torch.equal(keys[0], table[hist[:, 0]])                     # the candidate field's own rows (offset 0)
    r1 = torch.randn(B, 2, K, device="cuda")
    r2 = torch.randn(B, T, K, device="cuda")
    ((torch.cat(fea.sparse_embed, 1) * r1).sum() + (keys[0] * r2).sum()).backward()
    joint = table.grad.clone()
    emb = fi.sparse_embed
    parts = []
    for off, siz, ids, r in ((emb.offsets, emb.sizes, idx, r1), (emb.offsets[:1].repeat(T), emb.sizes[:1].repeat(T), hist[:, 0], r2)):
        t = table.detach().clone().requires_grad_()
        (Fn.embed_gather(t, off.contiguous(), ids.contiguous(), sizes=siz.contiguous()) * r).sum().backward()
        parts.append(t.grad)
    want = (parts[0] + parts[1]).double().cpu().numpy()
    assert np.abs(want).max() > 0 and ref.norm_rel(joint.double().cpu().numpy(), want) < 1e-6


def test_captured_din_step_replays_the_eager_steps_bits():
    vocab, T, K, B = [13, 7, 5], 6, 8, 256
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx, hist = behaviour_inputs(B, vocab, T, seed=40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        model = _din_model(vocab, T, K, 7)
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
    assert not torch.equal(model_c.body.atten[0].att_w1, init["body.atten.0.att_w1"])
