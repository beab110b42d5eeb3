"""The view-masked, pooled self-attention on the GPU (include/fil.h fil_seqattn_*_v, functional.seq_view_attention,
layers.SeqViewAttentionLayer, models.SeqFM) against the fp64 restatement of tests/seq_view_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (seq_attn_ref.bars).  The measured errors are
printed.  Where the reference is exactly zero the kernel's result must be."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import guarded
from tests import seq_view_ref as ref
from tests.seq_common import behaviour_inputs, behaviour_model, bits, dev, dev_mask, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("x",) + ref.PARAMS
POOL = pytest.mark.parametrize("pool", [False, True], ids=["rows", "pooled"])


def id_of(v):
    shape, view, split = v
    return "x".join(map(str, shape)) + "-" + view + (str(split) if view == "cross" else "")


@functools.lru_cache(maxsize=None)
def case_of(shape, view="full", split=0, pool=False, seed=0, mask="ragged", w_scale=1.0):
    return ref.make_case(*shape, seed, view=view, split=split, pool=pool, mask=mask, w_scale=w_scale)


def run_op(case, wanted=NAMES, fn=None):
    """functional.seq_view_attention forward + backward on the case (g, or gpool for the pooled form) -> dict of float64 numpy arrays
    (out and the gradients asked for)."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES}
    if fn is None:
        fn = lambda *a: Fn.seq_view_attention(*a, use_scale=case.get("use_scale", True), view=case["view"], split=case["split"], pool=case["pool"])
    out = fn(t["x"], dev_mask(case), t["Wq"], t["Wk"], t["Wv"], case["heads"])
    if any(v.requires_grad for v in t.values()):
        out.backward(dev(case["gpool" if case["pool"] else "g"]))
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
    print("%s %s %s%s %s  " % (label, case["shape"], case["view"], case["split"] or "", "pooled" if case["pool"] else "rows")
          + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
        want = out if k == "out" else bwd[k]
        assert not np.asarray(got[k]).reshape(want.shape)[want == 0].any(), (k, "not exactly zero where the reference is")
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY = [((1, 1, 4, 1, 4), "causal", 0),              # the minimum; one key per row: dWq = dWk = 0 exactly
          ((3, 2, 4, 1, 4), "cross", 1),               # one key per row as well
          ((3, 2, 4, 2, 4), "causal", 0),
          ((5, 20, 16, 1, 16), "causal", 0), ((5, 28, 16, 1, 16), "cross", 8),            # SeqFM's own: T = 20, F = 8
          ((3, 7, 12, 3, 4), "cross", 3),              # K / 4, H and T odd
          ((2, 63, 8, 1, 8), "causal", 0), ((2, 64, 8, 1, 8), "causal", 0),              # the wave-width edges of a key loop ...
          ((2, 65, 8, 1, 8), "cross", 64), ((2, 65, 8, 1, 8), "cross", 1),               # ... and both split edges
          ((2, 256, 16, 4, 4), "causal", 0), ((2, 256, 16, 4, 4), "cross", 128),         # the longest history
          ((3, 64, 64, 8, 8), "cross", 32), ((2, 5, 64, 1, 64), "causal", 0)]            # the menu's corners
ONE_KEY = PARITY[:2]


@POOL
@pytest.mark.parametrize("which", PARITY, ids=id_of)
def test_parity_with_the_fp64_reference(which, pool):
    shape, view, split = which
    case = case_of(shape, view, split, pool)
    got = run_op(case)
    check_parity(got, case)
    if which in ONE_KEY:
        _, bwd, _ = ref.reference(case)
        assert not bwd["dWq"].any() and not bwd["dWk"].any() and not got["dWq"].any() and not got["dWk"].any()


@POOL
@pytest.mark.parametrize("which", [((5, 20, 16, 1, 16), "causal", 0), ((5, 28, 16, 1, 16), "cross", 8)], ids=id_of)
def test_peaked_rows_keep_their_digits(which, pool):
    """Wq, Wk x 24: every softmax row has one weight near 1.  The bars are the same formula."""
    shape, view, split = which
    case = case_of(shape, view, split, pool, w_scale=24.0)
    check_parity(run_op(case), case, label="peaked")


# ---------------------------------------------------------------------------------------------------- 2. exact properties
PROP = (6, 10, 8, 2, 4)
PROP_VIEWS = [("full", 0), ("causal", 0), ("cross", 3)]
VIEW = pytest.mark.parametrize("view,split", PROP_VIEWS, ids=["full", "causal", "cross3"])


def test_the_full_view_with_rows_out_is_seq_self_attention_bit_for_bit():
    for shape in (PROP, (5, 50, 16, 2, 8), (2, 5, 64, 1, 64)):
        case = case_of(shape, seed=2)
        first = run_op(case, fn=lambda *a: Fn.seq_self_attention(*a))
        same_bits(first, run_op(case))
        assert first["dx"].any()


def _np_pool(out, live):
    """The kernel's pooling restated in numpy fp32: the live rows added in position order from 0, then one division."""
    B, T, C = out.shape
    res = np.zeros((B, C), np.float32)
    for b in range(B):
        acc, n = np.zeros(C, np.float32), 0
        for i in range(T):
            if live[b, i]:
                acc = acc + out[b, i].astype(np.float32)
                n += 1
        if n:
            res[b] = acc / np.float32(n)
    return res


@VIEW
def test_pooled_is_the_sequential_fp32_mean_of_the_rows(view, split):
    for shape in (PROP, (5, 28, 16, 1, 16)):
        split_ = split if shape == PROP or view != "cross" else 8
        case = case_of(shape, view, split_, False, seed=2)
        rows = run_op(case, wanted=())["out"]
        pooled = run_op(dict(case, pool=True), wanted=())["out"]
        live = case["mask"].astype(bool)
        assert np.array_equal(bits(pooled), bits(_np_pool(rows, live))), (view, shape)


@VIEW
def test_the_gpool_backward_is_the_rows_backward_fed_gpool_over_n(view, split):
    case = case_of(PROP, view, split, True, seed=2)
    live = case["mask"].astype(bool)
    n = live.sum(1)
    g = np.full(case["g"].shape, 1e30)                                     # (masked rows are never read)
    for b in range(PROP[0]):
        if n[b]:
            g[b, live[b]] = (case["gpool"][b].astype(np.float32) / np.float32(n[b])).astype(np.float64)
    pooled = run_op(case)
    rows = run_op(dict(case, pool=False, g=g))
    same_bits({k: pooled[k] for k in ref.GRADS}, rows, view)
    assert pooled["dx"].any() and pooled["dWq"].any()


@pytest.mark.parametrize("how", ["masked", "nan"])
def test_a_causal_row_reads_nothing_after_itself(how):
    case = case_of(PROP, "causal", 0, False, seed=2, mask=None)
    T = PROP[1]
    whole = run_op(case, wanted=())["out"]
    for t in (0, 3, T - 2):
        if how == "masked":
            m = np.ones(PROP[:2], np.uint8)
            m[:, t + 1:] = 0
            other = dict(case, mask=m)
        else:
            x = case["x"].copy()
            x[:, t + 1:] = np.nan
            other = dict(case, x=x)
        got = run_op(other, wanted=())["out"]
        assert np.array_equal(bits(got[:, :t + 1]), bits(whole[:, :t + 1])), t
        assert np.isfinite(got[:, :t + 1]).all()


def test_cross_view_with_one_live_history_slot_returns_its_value_row():
    """Every static row then sees one key: it returns that slot's v row exactly (the bits the full view gives a row that is alone)
    and sends no score gradient: with g on the static rows only, dWq and dWk are exactly 0."""
    B, T, K, H, D = PROP
    S = 3
    m = np.zeros((B, T), np.uint8)
    m[:, :S] = 1
    slot = [S + (2 * b) % (T - S) for b in range(B)]
    for b in range(B):
        m[b, slot[b]] = 1
    g = ref.make_case(*PROP, seed=4)["g"].copy()
    g[:, S:] = 0.0
    case = dict(ref.make_case(*PROP, seed=4, view="cross", split=S, mask=m), g=g)
    got = run_op(case)
    alone = np.zeros((B, T), np.uint8)
    for b in range(B):
        alone[b, slot[b]] = 1
    v = run_op(dict(case, view="full", split=0, mask=alone), wanted=())["out"]
    for b in range(B):
        for r in range(S):
            assert np.array_equal(bits(got["out"][b, r]), bits(v[b, slot[b]])), (b, r)
    _, bwd, _ = ref.reference(case)
    assert not bwd["dWq"].any() and not bwd["dWk"].any() and bwd["dWv"].any()
    assert not got["dWq"].any() and not got["dWk"].any()
    check_parity(got, case, label="one live history slot")


@POOL
def test_cross_view_of_a_sample_whose_history_is_all_padding_is_exactly_zero(pool):
    B, T, K, H, D = PROP
    S = 3
    m = np.ones((B, T), np.uint8)
    m[2, S:] = 0                      # static rows live, nothing to see
    m[4, :S] = 0                      # the other way round: history rows live, no static row
    m[1, S + 1:] = 0
    case = ref.make_case(*PROP, seed=5, view="cross", split=S, pool=pool, mask=m)
    got = run_op(case)
    for b in (2, 4):
        assert not got["out"][b].any() and not got["dx"][b].any(), b
    assert got["out"][0].any() and got["dx"][1].any()
    check_parity(got, case, label="empty rows")
    # ... and such a sample contributes nothing: without it the parameter gradients have the same bits
    keep = [0, 1, 3, 5]
    less = dict(case, shape=(4,) + PROP[1:], x=case["x"][keep], g=case["g"][keep], gpool=case["gpool"][keep], mask=m[keep])
    without = run_op(less)
    for k in ("dWq", "dWk", "dWv"):
        assert np.array_equal(bits(without[k]), bits(got[k])), k


@POOL
@VIEW
def test_masked_inputs_are_never_used(view, split, pool):
    case = case_of(PROP, view, split, pool, seed=2)
    live = case["mask"].astype(bool)
    assert not live.all() and live.any()
    poisoned = dict(case, x=np.where(live[:, :, None], case["x"], 1e30), g=np.where(live[:, :, None], case["g"], 1e30))
    clean, dirty = run_op(case), run_op(poisoned)
    for k, v in dirty.items():
        assert np.isfinite(v).all(), k
    same_bits(clean, dirty)
    assert not clean["dx"][~live].any() and (pool or not clean["out"][~live].any())


@POOL
@pytest.mark.parametrize("which", [(PROP, "causal", 0), (PROP, "cross", 3), ((300, 20, 16, 2, 8), "causal", 0), ((300, 28, 16, 1, 16), "cross", 8)],
                         ids=id_of)
def test_repeats_are_bit_identical(which, pool):
    shape, view, split = which
    case = case_of(shape, view, split, pool, seed=2)
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    check_parity(first, case)


@POOL
@VIEW
def test_a_sample_alone_has_the_bits_of_its_rows_in_the_batch(view, split, pool):
    one = lambda c, b: dict(c, shape=(1,) + c["shape"][1:], x=c["x"][b:b + 1], g=c["g"][b:b + 1], gpool=c["gpool"][b:b + 1], mask=c["mask"][b:b + 1])
    case = case_of(PROP, view, split, pool, seed=2)
    got = run_op(case)
    for b in range(PROP[0]):
        alone = run_op(one(case, b))
        assert np.array_equal(bits(alone["out"][0]), bits(got["out"][b])) and np.array_equal(bits(alone["dx"][0]), bits(got["dx"][b])), b
    # ... and inside a batch with a second tile and more than one workgroup
    big = case_of((300,) + PROP[1:], view, split, pool, seed=3)
    assert Fn.seq_attn_plan(300, *PROP[1:])["grid"] > 1
    whole = run_op(big)
    alone = run_op(one(big, 299))
    assert np.array_equal(bits(alone["out"][0]), bits(whole["out"][299])) and np.array_equal(bits(alone["dx"][0]), bits(whole["dx"][299]))


def test_needs_input_grad_is_honoured():
    case = case_of((9, 6, 8, 2, 4), "cross", 2, True)
    full = run_op(case)
    for wanted in (("x",), tuple(ref.PARAMS), ("Wk",), ("x", "Wv")):
        got = run_op(case, wanted=wanted)
        for k in NAMES:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["out"]), bits(full["out"]))
    assert np.array_equal(bits(run_op(case, wanted=())["out"]), bits(full["out"]))


# ---------------------------------------------------------------------------------------------------- 3. the raw entry points
EDGE = (3, 4, 1, 4)            # T, K, H, D
EDGE_VIEWS = [("causal", 0), ("cross", 1), ("cross", 2)]
EDGE_VIEW = pytest.mark.parametrize("view,split", EDGE_VIEWS, ids=["causal", "cross1", "cross2"])


def run_raw(case, subset=ref.GRADS, outputs=("out", "pooled")):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace guarded behind its
    bytes, `saved` between guard words.  The forward writes `outputs`; the backward takes g, or gpool for a pooled case."""
    lib = _lib.load()
    B, T, K, H, D = case["shape"]
    us = int(case.get("use_scale", True))
    view, split = Fn.SEQ_VIEWS[case["view"]], case["split"]
    t = {k: dev(case[k]) for k in NAMES + ("g", "gpool")}
    mask = dev_mask(case)
    shapes = dict(out=(B, T, H * D), pooled=(B, H * D), dx=(B, T, K), dWq=(K, H * D), dWk=(K, H * D), dWv=(K, H * D))
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in list(outputs) + list(subset)}
    at = lambda k: bufs[k].ptr if k in bufs else None
    nsv = lib.fil_seqattn_saved_bytes(B, T, K, H, D)
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    check(lib.fil_seqattn_fwd_v(ptr(t["x"]), ptr(mask), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), at("out"), at("pooled"), saved.ptr,
                                B, T, K, H, D, us, view, split, stream_ptr()), "fil_seqattn_fwd_v")
    nws = lib.fil_seqattn_bwd_workspace_bytes(B, T, K, H, D)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    params = any(k in bufs for k in ("dWq", "dWk", "dWv"))
    pool = case["pool"]
    check(lib.fil_seqattn_bwd_v(ptr(t["x"]), ptr(mask), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), saved.ptr, None if pool else ptr(t["g"]),
                                ptr(t["gpool"]) if pool else None, at("dx"), at("dWq"), at("dWk"), at("dWv"), ptr(ws) if params else None,
                                nws if params else 0, B, T, K, H, D, us, view, split, stream_ptr()), "fil_seqattn_bwd_v")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_seqattn_bwd_v", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64) for k, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def edge_case(B, view, split, pool):
    """Samples of three positions: the seed is the first whose sums over (b, t) are well conditioned in the fp64 reference
    (seq_view_ref.conditioned_case; the seed is printed)."""
    return ref.conditioned_case(B, *EDGE, view=view, split=split, pool=pool)


def check_raw(raw, case, label):
    """Both outputs of the forward and the gradients against the reference of the case's form."""
    form = {k: v for k, v in raw.items() if k not in ("out", "pooled")}
    form["out"] = raw["pooled" if case["pool"] else "out"]
    check_parity(form, case, label=label)
    other = dict(case, pool=not case["pool"])
    check_parity(dict(out=raw["out" if case["pool"] else "pooled"]), other, label=label)


@POOL
@EDGE_VIEW
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which, view, split, pool):
    """T = 3, K = 4, one head of 4.  tile - 1 (a partial tile) and tile: one workgroup, one partial; tile + 1: two, the second with one
    sample.  out, pooled, every gradient and `saved` sit between guard words, the workspace has guard bytes behind it."""
    tile = Fn.seq_attn_plan(1, *EDGE)["tile"]
    assert tile == 85
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    assert Fn.seq_attn_plan(B, *EDGE)["partials"] == (2 if which == "tile+1" else 1)
    case = edge_case(B, view, split, pool)
    print("seed", case["seed"])
    check_raw(run_raw(case), case, which)


@POOL
@EDGE_VIEW
def test_small_batches_with_guard_words(view, split, pool):
    for B in (1, 3):
        case = edge_case(B, view, split, pool)
        check_raw(run_raw(case), case, "B=%d seed %d" % (B, case["seed"]))


@POOL
def test_null_output_subsets_have_the_full_calls_bits(pool):
    case = edge_case(5, "cross", 2, pool)
    full = run_raw(case)
    for subset in (("dx",), ("dWq", "dWk", "dWv"), ("dWk",)):
        part = run_raw(case, subset=subset)
        assert set(part) == {"out", "pooled"} | set(subset)
        same_bits(part, full, subset)
    for outputs in (("out",), ("pooled",)):
        part = run_raw(case, outputs=outputs)
        assert set(part) == set(outputs) | set(ref.GRADS)
        same_bits(part, full, outputs)
    with pytest.raises(_lib.FilError):                                  # nothing is left to compute: FIL_ERR_ARG
        run_raw(case, subset=())
    with pytest.raises(_lib.FilError):
        run_raw(case, outputs=())
    # the inference call saves nothing and has the training call's bits
    lib = _lib.load()
    B, T, K, H, D = case["shape"]
    t = {k: dev(case[k]) for k in NAMES}
    out = guarded.GuardedOutput((B, H * D) if pool else (B, T, H * D), np.uint32, "out")
    check(lib.fil_seqattn_fwd_v(ptr(t["x"]), ptr(dev_mask(case)), ptr(t["Wq"]), ptr(t["Wk"]), ptr(t["Wv"]), None if pool else out.ptr,
                                out.ptr if pool else None, None, B, T, K, H, D, 1, _lib.FIL_SEQ_VIEW_CROSS, 2, stream_ptr()), "fil_seqattn_fwd_v")
    torch.cuda.synchronize()
    assert np.array_equal(out.read("out").view(np.int32), bits(full["pooled" if pool else "out"]))


def test_past_the_grid_cap_a_workgroup_walks_a_second_tile():
    """T = 1, one head: a tile of 256 samples, one per thread, so B = cap * 256 + 1 leaves one workgroup a second tile of one sample.
    The causal view (T = 1 has no other besides the full one); rows out and pooled from the same draws."""
    T, K, H, D = 1, 4, 1, 4
    cap = Fn.seq_attn_plan(1, T, K, H, D)["cap"]
    B = cap * 256 + 1
    plan = Fn.seq_attn_plan(B, T, K, H, D)
    assert plan["tile"] == 256 and plan["grid"] == cap and plan["partials"] == cap
    for pool in (False, True):
        case = case_of((B, T, K, H, D), "causal", 0, pool, mask=None)
        check_parity(run_op(case), case, label="cap*tile+1")


@POOL
@EDGE_VIEW
def test_empty_batch_is_a_no_op(view, split, pool):
    x = torch.empty(0, 3, 4, device="cuda", requires_grad=True)
    w = [torch.randn(4, 8, device="cuda", requires_grad=True) for _ in range(3)]
    out = Fn.seq_view_attention(x, None, *w, 2, view=view, split=split, pool=pool)
    assert out.shape == ((0, 8) if pool else (0, 3, 8))
    out.sum().backward()
    torch.cuda.synchronize()
    assert x.grad.shape == (0, 3, 4) and all(not p.grad.any() for p in w)


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
    assert out.dtype == torch.float32 and out.shape == ((B, H * D) if case["pool"] else (B, T, H * D))
    out.backward(dev(case["gpool" if case["pool"] else "g"]))
    torch.cuda.synchronize()
    Dn = lambda v: v.detach().cpu().double().numpy()
    res = dict(out=Dn(out), dx=Dn(x.grad))
    for k, name in LAYER_NAMES.items():
        res["d" + k] = Dn(getattr(layer, name).grad).reshape(K, H * D)
    return res


def _layer_of(case):
    return layers.SeqViewAttentionLayer(case["shape"][3], case["shape"][4], view=case["view"], split=case["split"], pool=case["pool"])


@POOL
@pytest.mark.parametrize("which", [((3, 5, 6, 2, 4), "causal", 0), ((3, 5, 8, 1, 68), "cross", 2), ((2, 257, 8, 1, 4), "cross", 8)],
                         ids=["K=6", "HD=68", "T=257"])
def test_layer_outside_the_menu_takes_the_composed_path(which, pool):
    shape, view, split = which
    case = case_of(shape, view, split, pool, seed=9)
    layer = _layer_of(case)
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["x"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


@POOL
@VIEW
def test_layer_inside_the_menu_is_the_op(view, split, pool):
    case = case_of((9, 6, 8, 2, 4), view, split, pool)
    layer = _layer_of(case)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["x"]))
    same_bits(got, run_op(case))


@POOL
def test_layer_computes_a_half_precision_input_in_fp32(pool):
    case = case_of((9, 6, 8, 2, 4), "causal", 0, pool, seed=6)
    r16 = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.float16).double().numpy()
    case16 = dict(case, x=r16(case["x"]))
    half = _run_layer(_layer_of(case), case16, dtype=torch.float16)        # asserts an fp32 output; the input gradient comes back in fp16
    check_parity(half, case16, keys=("out", "dWq", "dWk", "dWv"), label="fp16 in")


VOCAB, T_HIST, K_EMB, B_MODEL = [50, 30, 20], 6, 8, 64


def _seqfm(seed, **kw):
    return behaviour_model(lambda: models.SeqFM(**kw), VOCAB, T_HIST, K_EMB, seed)


def test_seqfm_against_the_model_on_the_composed_path(monkeypatch):
    """3 fields, one history of T = 6, B = 64, K = 8.  The same weights with every view forced onto the composed path
    (seq_view_attention_graph: fp32 torch ops): the logits and every gradient, the embedding table's included, agree within 1e-5,
    the floor of the bars max(1e-5, 4 E32) (no fp64 model is built here, so the term that could only widen the bar is left out)."""
    _, idx, hist = behaviour_inputs(B_MODEL, VOCAB, T_HIST, seed=1)
    y = torch.tensor(np.random.default_rng(2).integers(0, 2, B_MODEL), dtype=torch.float32, device="cuda")
    model = _seqfm(3, att_heads=2, ffn_layers=2)
    model(None, idx, hist)          # the first call builds the layers (and the score head takes its composed path once)

    def grads():
        model.zero_grad()
        p = model(None, idx, hist)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads()
    body = model.body
    assert [v.view for v in (body.static_view, body.dynamic_views[0], body.cross_views[0])] == ["full", "causal", "cross"]
    assert body.cross_views[0].split == 3 and all(v.pool and v.heads == 2 and v.head_dim == 4 for v in (body.static_view, body.dynamic_views[0], body.cross_views[0]))
    assert body.cross_views[0].fits_kernel_menu(torch.empty(B_MODEL, 3 + T_HIST, K_EMB))
    calls = []
    real = Fn.seq_view_attention
    monkeypatch.setattr(Fn, "seq_view_attention", lambda *a, **k: calls.append(k) or real(*a, **k))
    again = grads()
    assert [(k["view"], k["split"], k["pool"]) for k in calls] == [("full", 0, True), ("causal", 0, True), ("cross", 3, True)]
    same_bits(again, fused)
    monkeypatch.setattr(layers.SeqSelfAttentionLayer, "fits_kernel_menu", lambda self, x: False)
    comp = grads()
    assert len(calls) == 3                              # the composed path does not reach the op
    monkeypatch.undo()
    names = ["static_view.query_w", "dynamic_views.0.key_w", "cross_views.0.value_w", "ffn.0.ln_gamma", "ffn.1.dense.kernel", "score.dense.kernel"]
    assert set(fused) == set(comp) and all("body." + n in fused for n in names), sorted(fused)
    table = [n for n in fused if "embeddings" in n]
    assert len(table) == 1, sorted(fused)
    for k in sorted(fused):
        direct = ref.norm_rel(fused[k], comp[k])
        print("SeqFM %-45s fused vs composed %.2e   bar 1.00e-05" % (k, direct))
        assert direct <= 1e-5, k
    assert np.abs(fused["body.cross_views.0.query_w"]).max() > 0 and np.abs(fused[table[0]]).max() > 0


def test_seqfm_trains_under_captured_adam_and_replays_the_eager_bits():
    """The loss falls over 20 captured optim.Adam steps on one batch, and three captured steps on three batches leave every
    parameter with the bits of three eager steps."""
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx, hist = behaviour_inputs(B_MODEL, VOCAB, T_HIST, seed=40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B_MODEL), dtype=torch.float32, device="cuda")))

    def make():
        model = _seqfm(7)
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
    name = "body.cross_views.0.query_w"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
