"""The AFM pair-attention pooling on the GPU (include/fil.h N3 fil_afm_*, functional.afm_pool, layers.AFMLayer,
models.AFM(pair_softmax=True)) against the fp64 restatement of tests/afm_pool_ref.py.

Error measure: norm-relative against the fp64 reference for pooled, de, dW, dh; db (a cancelling sum, exactly zero where no score is
clipped) in units of max_a sum |du_p[a]|.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32 torch restatement of the
same graph on the same inputs, computed here on the CPU (afm_pool_ref.bars).  The measured errors are printed."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import afm_pool_ref as ref
from tests.seq_common import PAD, SENTINEL, bits, dev, guarded, guards_intact

pytestmark = pytest.mark.gpu

FORMS = [False, True]
FORM_IDS = ["reference", "paper"]
KEYS = ("pooled", "de", "dW", "db", "dh")


@functools.lru_cache(maxsize=None)
def case_of(shape, hidden_relu, seed=0):
    return ref.make_case(*shape, hidden_relu, seed)


def run_op(case):
    """functional.afm_pool forward + backward on the case -> dict of float64 numpy arrays."""
    t = {k: dev(case[k]).requires_grad_() for k in ("e", "W", "b", "h")}
    pooled = Fn.afm_pool(t["e"], t["W"], t["b"], t["h"], hidden_relu=case["hidden_relu"])
    pooled.backward(dev(case["g"]))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    return dict(pooled=D(pooled), de=D(t["e"].grad), dW=D(t["W"].grad), db=D(t["b"].grad), dh=D(t["h"].grad))


def check_parity(got, case, keys=KEYS, label=""):
    pooled, bwd, e32 = ref.reference(case)
    err, bar = ref.errors(got, pooled, bwd), ref.bars(e32)
    print("%s %s %s  " % (label, case["shape"], "paper" if case["hidden_relu"] else "reference")
          + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in keys))
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY_SHAPES = [(1, 2, 4, 1),        # a single pair
                 (3, 3, 4, 4),
                 (5, 11, 8, 4), (5, 12, 8, 4),       # P = 55 / 66: either side of one wave of pairs
                 (7, 23, 16, 16),     # P = 253 = 4 * 64 - 3, A at its limit
                 (9, 39, 16, 1),
                 (17, 39, 16, 4),     # the benchmark's F, K, A
                 (3, 12, 64, 16),     # K and A at their limits
                 (2, 64, 16, 4), (2, 64, 4, 1),      # F at its limit, P = 2016
                 (3, 5, 12, 3),       # K / 4 odd and no divisor of 64: idle lanes in the k-quad and the k mappings
                 (5, 9, 48, 5)]       # the same past 32, A between the two register widths


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_fp64_reference(shape, hidden_relu):
    case = case_of(shape, hidden_relu)
    got = run_op(case)
    if shape[1] == 2:         # one pair: dW, db, dh are exactly zero (checked bit for bit below); their relative error has no scale
        check_parity(got, case, keys=("pooled", "de"))
        assert not got["dW"].any() and not got["db"].any() and not got["dh"].any()
    else:
        check_parity(got, case)


def test_the_largest_shape_of_the_menu_runs():
    """F, K and A all at their limits (one wave per workgroup, the LDS footprint at its largest): the reference form only -- the
    paper form's ReLU margin rejects nearly every draw at 2016 x 16 pre-activations per sample."""
    check_parity(run_op(case_of((2, 64, 64, 16), False)), case_of((2, 64, 64, 16), False))


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
def run_raw(case):
    """The two entry points called directly: outputs inside sentinel-guarded allocations, the workspace NaN-poisoned."""
    lib = _lib.load()
    B, F, K, A = case["shape"]
    flags = _lib.FIL_AFM_HIDDEN_RELU if case["hidden_relu"] else 0
    e, W, b, h, g = (dev(case[k]) for k in ("e", "W", "b", "h", "g"))
    stats = torch.empty(B, 2, device="cuda")
    bufs = {}
    for name, shape in (("pooled", (B, K)), ("de", (B, F, K)), ("dW", (K, A)), ("db", (A,)), ("dh", (A, 1))):
        bufs[name] = guarded(shape)
    check(lib.fil_afm_fwd(ptr(e), ptr(W), ptr(b), ptr(h), ptr(bufs["pooled"][1]), ptr(stats), B, F, K, A, flags, stream_ptr()), "fil_afm_fwd")
    nws = lib.fil_afm_bwd_workspace_bytes(B, F, K, A)
    ws_buf = torch.full((PAD + nws // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    ws_buf[:PAD] = SENTINEL
    ws_buf[-PAD:] = SENTINEL
    ws = ws_buf[PAD:PAD + nws // 4]
    check(lib.fil_afm_bwd(ptr(e), ptr(W), ptr(b), ptr(h), ptr(bufs["pooled"][1]), ptr(stats), ptr(g), ptr(bufs["de"][1]), ptr(bufs["dW"][1]),
                          ptr(bufs["db"][1]), ptr(bufs["dh"][1]), ptr(ws), nws, B, F, K, A, flags, stream_ptr()), "fil_afm_bwd")
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert guards_intact(buf), name
    assert guards_intact(ws_buf)
    return {k: v[1].detach().cpu().double().numpy() for k, v in bufs.items()}


def _edge_plan():
    plan = Fn.afm_plan(1, 3, 4, 2)
    return plan["tile"], plan["cap"]


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1", "cap*tile+1"])
def test_batch_tile_and_grid_edges(which, hidden_relu):
    """F = 3, K = 4, A = 2 (the fp64 reference costs nothing).  tile - 1 and tile: exactly one partial; tile + 1: two, the last
    workgroup with one sample; cap * tile + 1: a second trip through the grid-stride loop that only one wave of one workgroup makes."""
    tile, cap = _edge_plan()
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "cap*tile+1": cap * tile + 1}[which]
    if B < 1:
        B = 1                  # (a one-sample tile: tile - 1 would be the empty batch, which the no-op test below covers)
    parts = Fn.afm_plan(B, 3, 4, 2)["partials"]
    assert parts == {"tile-1": 1, "tile": 1, "tile+1": 2 if tile + 1 <= cap * tile else 1, "cap*tile+1": cap}[which]
    case = case_of((B, 3, 4, 2), hidden_relu)
    check_parity(run_raw(case), case, label=which)


def test_empty_batch_is_a_no_op():
    e = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w, b, h = (torch.randn(s, device="cuda", requires_grad=True) for s in ((4, 2), (2,), (2, 1)))
    out = Fn.afm_pool(e, w, b, h)
    assert out.shape == (0, 4)


# ---------------------------------------------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", [(6, 2, 8, 4), (5, 2, 64, 16), (3, 2, 4, 1)], ids=lambda s: "x".join(map(str, s)))
def test_one_pair_is_the_pair_product_bit_for_bit(shape, hidden_relu):
    """F = 2: one pair, its softmax weight is exactly 1 -- the reference's quirk recovered as the one-pair case."""
    case = case_of(shape, hidden_relu, seed=4)
    got = run_op(case)
    e, g = case["e"].astype(np.float32), case["g"].astype(np.float32)
    assert np.array_equal(bits(got["pooled"]), bits(e[:, 0] * e[:, 1]))
    assert np.array_equal(bits(got["de"][:, 0]), bits(g * e[:, 1])) and np.array_equal(bits(got["de"][:, 1]), bits(g * e[:, 0]))
    for k in ("dW", "db", "dh"):
        assert not got[k].any(), k


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_zero_h_is_the_fm_sum_over_p(hidden_relu):
    base = case_of((5, 12, 8, 4), hidden_relu)
    case = dict(base, h=np.zeros((4, 1)))          # (every score is 0: the ReLU margin does not apply)
    got = run_op(case)
    fm = Fn.fm(dev(case["e"])).cpu().double().numpy() / 66
    assert ref.norm_rel(got["pooled"], fm) < 1e-6
    assert not got["dW"].any() and not got["db"].any()
    pooled, bwd, e32 = ref.reference(case)
    err, bar = ref.norm_rel(got["dh"], bwd["dh"]), ref.bars(e32)["dh"]
    print("h = 0, %s: dh %.2e (bar %.2e)" % ("paper" if hidden_relu else "reference", err, bar))
    assert err <= bar
    if not hidden_relu:
        assert not got["dh"].any() and not bwd["dh"].any()      # relu'(0) = 0
    check_parity(got, case, keys=("pooled", "de"))


# ---------------------------------------------------------------------------------------------------- 4. range
@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_scores_of_a_thousand(hidden_relu):
    base = case_of((5, 12, 8, 4), hidden_relu)
    h = (base["h"] * 1e3).astype(np.float32).astype(np.float64)
    case = dict(base, h=h)
    assert ref.relu_margin(case["e"], case["W"], case["b"], h, hidden_relu).all()
    got = run_op(case)
    for k in KEYS:
        assert np.isfinite(got[k]).all(), k
    check_parity(got, case, keys=("pooled",), label="h x 1e3")


def test_every_score_clipped_is_uniform_attention():
    """Reference form with b shifted against h until every pre-activation is negative: s = 0 everywhere, a = 1/P, and nothing flows
    into W, b or h."""
    base = case_of((5, 12, 8, 4), False)
    e, W, b, h = base["e"], base["W"], base["b"], base["h"]
    I, J = ref.pair_index(12)
    t = ((e[:, I] * e[:, J]) @ W + b) @ h.reshape(-1)
    lam = 2.0 * (t.max() + 1.0) / float((h * h).sum())
    b2 = (b - lam * h.reshape(-1)).astype(np.float32).astype(np.float64)
    case = dict(base, b=b2)
    assert ((((e[:, I] * e[:, J]) @ W + b2) @ h.reshape(-1)) < -0.5).all()
    got = run_op(case)
    for k in ("dW", "db", "dh"):
        assert not got[k].any(), k
    assert ref.norm_rel(got["pooled"], Fn.fm(dev(e)).cpu().double().numpy() / 66) < 1e-6
    check_parity(got, case, keys=("pooled", "de"), label="all clipped")


# ---------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_repeats_are_bit_identical(hidden_relu):
    case = case_of((300, 39, 16, 4), hidden_relu)
    first, second = run_op(case), run_op(case)
    for k in KEYS:
        assert np.array_equal(bits(first[k]), bits(second[k])), k
    check_parity(first, case)


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_needs_input_grad_is_honoured(hidden_relu):
    """Only the gradients that are asked for are computed (embeddings alone: no parameter pass and no workspace; parameters alone:
    no embedding pass; a single parameter), and each has the bits of the full backward."""
    case = case_of((9, 12, 8, 4), hidden_relu)
    full = run_op(case)
    names = dict(e="de", W="dW", b="db", h="dh")
    for wanted in (("e",), ("W", "b", "h"), ("h",), ("e", "b")):
        t = {k: dev(case[k]).requires_grad_(k in wanted) for k in names}
        Fn.afm_pool(t["e"], t["W"], t["b"], t["h"], hidden_relu=hidden_relu).backward(dev(case["g"]))
        torch.cuda.synchronize()
        for k, key in names.items():
            if k in wanted:
                assert np.array_equal(bits(t[k].grad.cpu().numpy()), bits(full[key])), (wanted, k)
            else:
                assert t[k].grad is None, (wanted, k)


# ---------------------------------------------------------------------------------------------------- 6. layer and model
def _layer_reference(case, kernel, bias, dy):
    """AFMLayer = the pooling + Dense(output_dim) in fp64: out and the gradients of the embeddings and of every weight."""
    pooled = ref.forward(case["e"], case["W"], case["b"], case["h"], case["hidden_relu"])
    out = pooled @ kernel + bias
    bwd = ref.backward(case["e"], case["W"], case["b"], case["h"], dy @ kernel.T, case["hidden_relu"])
    return dict(out=out, de=bwd["de"], dW=bwd["dW"], db=bwd["db"], dh=bwd["dh"], dkernel=pooled.T @ dy, dbias=dy.sum(0), du_abs=bwd["du_abs"])


def _layer_errors(got, want):
    err = {k: ref.norm_rel(got[k].reshape(want[k].shape), want[k]) for k in ("out", "de", "dW", "dh", "dkernel", "dbias")}
    err["db"] = float(np.abs(got["db"].reshape(-1) - want["db"]).max() / want["du_abs"].max())
    return err


def _set_weights(layer, case, kernel, bias):
    with torch.no_grad():
        layer.kernel_w.copy_(dev(case["W"]))
        layer.kernel_b.copy_(dev(case["b"]))
        layer.single_mlp_kernel.copy_(dev(case["h"]))
        layer.output_layer.kernel.copy_(dev(kernel))
        layer.output_layer.bias.copy_(dev(bias))


def _run_layer(layer, inputs_of, case, kernel, bias, dy):
    emb = dev(case["e"]).requires_grad_()
    layer(inputs_of(emb.detach()))                 # lazy build
    _set_weights(layer, case, kernel, bias)
    layer.zero_grad()
    out = layer(inputs_of(emb))
    out.backward(dev(dy))
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    return dict(out=D(out), de=D(emb.grad), dW=D(layer.kernel_w.grad), db=D(layer.kernel_b.grad), dh=D(layer.single_mlp_kernel.grad),
                dkernel=D(layer.output_layer.kernel.grad), dbias=D(layer.output_layer.bias.grad))


def _dense(K, seed):
    rng = np.random.default_rng(seed)
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return r32(rng.standard_normal((K, 1)) * 0.5), r32(rng.standard_normal(1))


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_layer_against_the_composed_comparator(hidden_relu):
    """AFMLayer on the field embeddings against AttentionBaseLayer(softmax_axis=1) over InnerLayer's pairs, the same weights."""
    B, F, K, A = 17, 4, 8, 4
    case = case_of((B, F, K, A), hidden_relu, seed=6)
    kernel, bias = _dense(K, 7)
    dy = np.random.default_rng(8).standard_normal((B, 1)).astype(np.float32).astype(np.float64)
    want = _layer_reference(case, kernel, bias, dy)
    fused_layer = layers.AFMLayer(attention_dim=A, hidden_relu=hidden_relu)
    fused = _run_layer(fused_layer, lambda e: list(e.split(1, dim=1)), case, kernel, bias, dy)
    assert fused_layer.fits_kernel_menu(dev(case["e"]))
    inner = layers.InnerLayer()
    comp = _run_layer(layers.AttentionBaseLayer(attention_dim=A, softmax_axis=1, hidden_relu=hidden_relu), lambda e: inner(list(e.split(1, dim=1))),
                      case, kernel, bias, dy)
    e32 = _layer_errors(comp, want)                 # the fp32 torch graph's own error
    direct = {k: (ref.norm_rel(fused[k], comp[k]) if k != "db" else float(np.abs(fused[k] - comp[k]).max() / want["du_abs"].max()))
              for k in e32}
    vs64 = _layer_errors(fused, want)
    for k in e32:
        bar = max(1e-5, 4 * e32[k])
        print("layer %-8s fused vs composed %.2e   fused vs fp64 %.2e   composed vs fp64 (E32) %.2e   bar %.2e" % (k, direct[k], vs64[k], e32[k], bar))
        assert direct[k] <= bar and vs64[k] <= bar, k
    assert float(np.abs(fused["dW"]).max()) > 0.0          # the point of the feature: the score weights learn
    # a packed [B,F,K] block is the same call
    packed = fused_layer(dev(case["e"]))
    assert np.array_equal(bits(packed.detach().cpu().numpy()), bits(fused["out"]))


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", [(3, 5, 6, 4), (2, 65, 4, 2)], ids=["K=6", "F=65"])
def test_layer_outside_the_menu_takes_the_composed_path(shape, hidden_relu):
    B, F, K, A = shape
    case = case_of(shape, hidden_relu, seed=9)
    kernel, bias = _dense(K, 10)
    dy = np.random.default_rng(11).standard_normal((B, 1)).astype(np.float32).astype(np.float64)
    want = _layer_reference(case, kernel, bias, dy)
    layer = layers.AFMLayer(attention_dim=A, hidden_relu=hidden_relu)
    got = _run_layer(layer, lambda e: e, case, kernel, bias, dy)
    assert not layer.fits_kernel_menu(dev(case["e"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        Fn.afm_pool(dev(case["e"]), dev(case["W"]), dev(case["b"]), dev(case["h"]), hidden_relu=hidden_relu)
    # the bars of the pooling (E32 from the fp32 restatement on the CPU), the Dense on top held to the same
    _, _, e32p = ref.reference(case)
    err = _layer_errors(got, want)
    bar = dict(ref.bars(e32p), out=max(1e-5, 4 * e32p["pooled"]), dkernel=max(1e-5, 4 * e32p["pooled"]), dbias=1e-5)
    print("composed %s: " % (shape,) + "  ".join("%s %.2e (bar %.2e)" % (k, err[k], bar[k]) for k in err))
    for k in err:
        assert err[k] <= bar[k], k


def test_layer_computes_a_half_precision_input_in_fp32():
    case = case_of((17, 4, 8, 4), False, seed=6)
    layer = layers.AFMLayer()
    e16 = dev(case["e"]).to(torch.bfloat16)
    out = layer(e16)
    assert out.dtype == torch.float32
    again = layer(e16.float())                      # the fused kernel on the same (bf16-representable) values
    assert ref.norm_rel(out.detach().cpu().numpy(), again.detach().cpu().numpy()) < 1e-5


def _inputs(B, n_dense, vocab, seed=0):
    rng = np.random.default_rng(seed)
    dense = torch.tensor(rng.random((B, n_dense)), dtype=torch.float32, device="cuda")
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device="cuda")
    return dense, idx


@pytest.mark.parametrize("hidden_relu", FORMS, ids=FORM_IDS)
def test_afm_with_the_pair_softmax_trains(hidden_relu):
    """The loop of test_models_gpu.test_more_zoo_models_train."""
    torch.manual_seed(0)
    vocab = [9, 4, 6, 12, 5]
    B, K = 64, 8
    fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useFlattenLinear=True)
    model = models.CTRModel(fi, models.AFM(pair_softmax=True, hidden_relu=hidden_relu)).cuda()
    dense, idx = _inputs(B, 2, vocab, seed=1)
    y = torch.tensor(np.random.default_rng(2).integers(0, 2, B), dtype=torch.float32, device="cuda")
    out = model(dense, idx)
    assert out.shape == (B, 1) and not hasattr(model.body, "inner")
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    history = []
    w0 = model.body.atten.kernel_w.detach().clone()
    for _ in range(25):
        opt.zero_grad()
        p = model(dense, idx)[:, 0]
        loss = torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y)
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    assert np.isfinite(history).all() and history[-1] < history[0] * 0.9, history[::6]
    assert not torch.equal(model.body.atten.kernel_w.detach(), w0)


def test_captured_afm_step_replays_the_eager_steps_bits():
    vocab = [7, 11, 5, 13, 3, 17]
    B, K = 256, 8
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx = _inputs(B, 1, vocab, seed=40 + s)
        batches.append((idx, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        torch.manual_seed(7)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useFlattenLinear=True)
        model = models.CTRModel(fi, models.AFM(pair_softmax=True)).cuda()
        model(None, batches[0][0])
        opt = optim.Adam(model.parameters(), learning_rate=1e-2)

        def step(idx, y):
            opt.zero_grad()
            p = model(None, idx)[:, 0]
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
    assert not torch.equal(model_c.body.atten.kernel_w, init["body.atten.single_score_w"])


def test_the_default_afm_is_still_the_quirk():
    """models.AFM() keeps the reference's softmax over a size-1 axis: the score weights get a zero gradient (restated from
    test_models_gpu.test_afm_matches_oracle_composition); with the pair softmax they get one."""
    vocab = [7, 11, 5, 13]
    grads = {}
    for pair_softmax in (False, True):
        torch.manual_seed(3)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=8), useLinear=True, useFlattenLinear=True)
        model = models.CTRModel(fi, models.AFM(pair_softmax=pair_softmax)).cuda()
        _, idx = _inputs(17, 1, vocab, seed=3)
        model(None, idx).sum().backward()
        a = model.body.atten
        grads[pair_softmax] = [float(p.grad.abs().max()) for p in (a.kernel_w, a.kernel_b, a.single_mlp_kernel)]
        assert float(fi.sparse_embed.embeddings.grad.abs().max()) > 0.0
    assert grads[False] == [0.0, 0.0, 0.0]
    assert grads[True][0] > 0.0 and grads[True][2] > 0.0
