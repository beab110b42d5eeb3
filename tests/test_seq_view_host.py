"""Host-only checks of the view-masked, pooled self-attention (include/fil.h fil_seqattn_*_v, functional.seq_view_attention,
layers.SeqViewAttentionLayer, models.SeqFM): the entry points in the header, the binding and the library; their argument validation
through ctypes with dummy pointers; the Python surface that needs no GPU; and self-checks of the fp64 restatement
(tests/seq_view_ref.py) the GPU tests are held to."""
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import seq_attn_ref as base
from tests import seq_view_ref as ref

NEW = ("fil_seqattn_fwd_v", "fil_seqattn_bwd_v")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
FULL, CAUSAL, CROSS = 0, 1, 2
DIMS = (3, 4, 1, 4)        # T, K, H, D of the small shape
VARIANTS = [("full", 0), ("causal", 0), ("cross", 1), ("cross", 2)]      # at T = 3
graph = layers.behavior_layer.seq_view_attention_graph


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _msg(lib):
    return lib.fil_last_error().decode()


def test_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    P, I, Z = _lib._P, _lib._I, _lib._Z
    assert _lib.SIGNATURES["fil_seqattn_fwd_v"] == (I, [P] * 8 + [I] * 8 + [P])
    assert _lib.SIGNATURES["fil_seqattn_bwd_v"] == (I, [P] * 13 + [Z] + [I] * 8 + [P])
    assert (_lib.FIL_SEQ_VIEW_FULL, _lib.FIL_SEQ_VIEW_CAUSAL, _lib.FIL_SEQ_VIEW_CROSS) == (FULL, CAUSAL, CROSS)
    header = open(_lib.HEADER_PATH).read()
    for name, value in (("FULL", FULL), ("CAUSAL", CAUSAL), ("CROSS", CROSS)):
        assert "#define FIL_SEQ_VIEW_%s %d\n" % (name, value) in header
    assert Fn.SEQ_VIEWS == dict(full=FULL, causal=CAUSAL, cross=CROSS) and tuple(Fn.SEQ_VIEWS) == ref.VIEWS


# positions:  fwd_v: x mask Wq Wk Wv out pooled saved      bwd_v: x mask Wq Wk Wv saved g gpool | dx dWq dWk dWv | workspace
def _fwd(lib, args, B=5, dims=DIMS, view=FULL, split=0):
    return lib.fil_seqattn_fwd_v(*args, B, *dims, 1, view, split, None)


def _bwd(lib, args, B=5, dims=DIMS, view=FULL, split=0, nws=1 << 20):
    return lib.fil_seqattn_bwd_v(*args, nws, B, *dims, 1, view, split, None)


def test_argument_validation(lib):
    """Every call below returns before a pointer is followed."""
    p = 4096
    fwd_ok = [p] * 8            # (both outputs given)
    bwd_ok = [p] * 7 + [None] + [p] * 5            # g given, gpool not
    # B == 0: a no-op that returns 0 before any pointer is looked at, in every view
    for view, split in ((FULL, 0), (CAUSAL, 0), (CROSS, 2)):
        assert _fwd(lib, [None] * 8, B=0, view=view, split=split) == OK
        assert _bwd(lib, [None] * 13, B=0, view=view, split=split, nws=0) == OK
    # a view outside 0 .. 2
    for view in (-1, 3, 7):
        assert _fwd(lib, fwd_ok, view=view) == ERR_ARG
        assert "fil_seqattn_fwd_v" in _msg(lib) and "view=%d" % view in _msg(lib), _msg(lib)
        assert _bwd(lib, bwd_ok, view=view) == ERR_ARG
        assert "fil_seqattn_bwd_v" in _msg(lib) and "view=%d" % view in _msg(lib), _msg(lib)
        assert _fwd(lib, [None] * 8, B=0, view=view) == ERR_ARG                      # (the dimensions are checked before B == 0)
    # split != 0 with FULL or CAUSAL
    for view in (FULL, CAUSAL):
        for split in (1, -1):
            assert _fwd(lib, fwd_ok, view=view, split=split) == ERR_ARG
            assert "fil_seqattn_fwd_v" in _msg(lib) and "split=%d" % split in _msg(lib), _msg(lib)
            assert _bwd(lib, bwd_ok, view=view, split=split) == ERR_ARG
            assert "fil_seqattn_bwd_v" in _msg(lib) and "split=%d" % split in _msg(lib), _msg(lib)
    # CROSS with split < 1 or split >= T (T = 3: 1 and 2 are the splits there are)
    for split in (0, -2, 3, 4):
        assert _fwd(lib, fwd_ok, view=CROSS, split=split) == ERR_ARG
        assert "fil_seqattn_fwd_v" in _msg(lib) and "split=%d" % split in _msg(lib), _msg(lib)
        assert _bwd(lib, bwd_ok, view=CROSS, split=split) == ERR_ARG
        assert "fil_seqattn_bwd_v" in _msg(lib) and "split=%d" % split in _msg(lib), _msg(lib)
    assert _fwd(lib, fwd_ok, dims=(1, 4, 1, 4), view=CROSS, split=1) == ERR_ARG         # T = 1 has no cross view
    # both outputs NULL
    args = list(fwd_ok)
    args[5] = args[6] = None
    assert _fwd(lib, args) == ERR_ARG
    assert "fil_seqattn_fwd_v" in _msg(lib) and "out" in _msg(lib) and "pooled" in _msg(lib) and "NULL" in _msg(lib), _msg(lib)
    # both or neither of g / gpool
    for g, gpool, word in ((p, p, "both"), (None, None, "neither")):
        args = list(bwd_ok)
        args[6], args[7] = g, gpool
        assert _bwd(lib, args, view=CAUSAL) == ERR_ARG
        assert "fil_seqattn_bwd_v" in _msg(lib) and "gpool" in _msg(lib) and word in _msg(lib), _msg(lib)
    # the required tensors, as in the first form: x, Wq, Wk, Wv; saved in the backward (mask = NULL is all live)
    for hole in (0, 2, 3, 4):
        args = list(fwd_ok)
        args[hole] = None
        assert _fwd(lib, args, view=CAUSAL) == ERR_ARG and "fil_seqattn_fwd_v" in _msg(lib), hole
    for hole in (0, 2, 3, 4, 5):
        args = list(bwd_ok)
        args[hole] = None
        assert _bwd(lib, args, view=CAUSAL) == ERR_ARG and "fil_seqattn_bwd_v" in _msg(lib), hole
    assert _bwd(lib, [p] * 7 + [None] * 5 + [p]) == ERR_ARG                            # nothing to compute
    assert _bwd(lib, [p] * 6 + [None, p] + [None] * 4 + [p]) == ERR_ARG
    # non-positive dimensions
    for dims in ((-1, 3, 4, 1, 4), (5, 0, 4, 1, 4), (5, 3, 0, 1, 4), (5, 3, 4, 0, 4), (5, 3, 4, 1, 0)):
        assert _fwd(lib, fwd_ok, B=dims[0], dims=dims[1:]) == ERR_ARG, dims
        assert _bwd(lib, bwd_ok, B=dims[0], dims=dims[1:]) == ERR_ARG, dims
    # a workspace that is too small (or NULL) when a parameter gradient is asked for: the needed size in the message
    need = lib.fil_seqattn_bwd_workspace_bytes(5, *DIMS)
    for args in (bwd_ok, [p] * 6 + [None, p] + [p] * 5):
        assert _bwd(lib, args, view=CROSS, split=2, nws=need - 1) == ERR_ARG
        assert str(need) in _msg(lib) and "workspace" in _msg(lib) and "fil_seqattn_bwd_v" in _msg(lib)
        args = list(args)
        args[12] = None
        assert _bwd(lib, args, view=CROSS, split=2, nws=need) == ERR_ARG and str(need) in _msg(lib)


def test_menu_errors_are_the_first_forms(lib):
    p = 4096
    outside = (((5, 3, 6, 1, 4), "K=6", "<= 64"), ((5, 3, 68, 1, 4), "K=68", "<= 64"), ((5, 3, 4, 1, 6), "D=6", "% 4"),
               ((5, 3, 4, 9, 4), "H=9", "<= 8"), ((5, 3, 4, 1, 68), "H*D=68", "<= 64"), ((5, 257, 4, 1, 4), "T=257", "<= 256"))
    for dims, word, limit in outside:
        assert _fwd(lib, [p] * 8, B=dims[0], dims=dims[1:], view=CAUSAL) == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and limit in _msg(lib) and "fil_seqattn_fwd_v" in _msg(lib), (_msg(lib), word)
        assert _bwd(lib, [p] * 7 + [None] + [p] * 5, B=dims[0], dims=dims[1:], view=CAUSAL) == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and limit in _msg(lib) and "fil_seqattn_bwd_v" in _msg(lib), (_msg(lib), word)
    # the LDS limit of the widest shape, from the shared plan
    K, H, D = 64, 8, 8
    t_max = max(T for T in range(1, 257) if Fn.seq_attn_plan(5, T, K, H, D)["fits"])
    assert 64 <= t_max < 256
    assert _fwd(lib, [p] * 8, dims=(t_max + 1, K, H, D), view=CROSS, split=t_max) == ERR_UNSUPPORTED and "LDS" in _msg(lib)


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_python_signatures_and_defaults():
    E = inspect.Parameter.empty
    s = _sig(Fn.seq_view_attention)
    assert list(s) == ["x", "mask", "Wq", "Wk", "Wv", "heads", "use_scale", "view", "split", "pool"]
    assert s["heads"] is E and s["use_scale"] is True and s["view"] == "full" and s["split"] == 0 and s["pool"] is False
    s = _sig(graph)
    assert list(s) == ["x", "mask", "wq", "wk", "wv", "heads", "use_scale", "view", "split", "pool"]
    assert s["heads"] is E and s["use_scale"] is True and s["view"] == "full" and s["split"] == 0 and s["pool"] is False
    assert layers.SeqViewAttentionLayer is layers.behavior_layer.SeqViewAttentionLayer and "SeqViewAttentionLayer" in layers.__all__
    assert issubclass(layers.SeqViewAttentionLayer, layers.SeqSelfAttentionLayer)
    assert _sig(layers.SeqViewAttentionLayer.__init__) == dict(heads=E, head_dim=E, use_scale=True, seed=2020, view="full", split=0, pool=False)
    assert _sig(models.SeqFM.__init__) == dict(att_heads=1, ffn_layers=1, seed=2020)
    # the first form's surface is what it was
    assert list(_sig(Fn.seq_self_attention)) == ["x", "mask", "Wq", "Wk", "Wv", "heads", "use_scale"]
    assert _sig(layers.SeqSelfAttentionLayer.__init__) == dict(heads=E, head_dim=E, use_scale=True, seed=2020)


def test_layer_and_op_value_errors():
    for kw in (dict(view="diagonal"), dict(view="full", split=1), dict(view="causal", split=2), dict(view="cross"),
               dict(view="cross", split=0), dict(view="cross", split=-1)):
        with pytest.raises(ValueError, match="view|split"):
            layers.SeqViewAttentionLayer(1, 4, **kw)
    with pytest.raises(ValueError, match="heads"):
        layers.SeqViewAttentionLayer(0, 4, view="causal")
    layer = layers.SeqViewAttentionLayer(2, 4, view="cross", split=3, pool=True)
    assert (layer.view, layer.split, layer.pool, layer.heads, layer.head_dim) == ("cross", 3, True, 2, 4)
    layer.build((2, 5, 8))
    assert list(layer.state_dict()) == ["query_w", "key_w", "value_w"]
    same = layers.SeqSelfAttentionLayer(2, 4)
    same.build((2, 5, 8))
    assert all(torch.equal(v, same.state_dict()[n]) for n, v in layer.state_dict().items())      # same weights for the same seed
    # a split the sequence has no room for is known at the call: T = 3 leaves splits 1 and 2
    x = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="split=3"):
        layer(x)
    with pytest.raises(ValueError, match="split=3"):
        Fn.seq_view_attention(x, None, *([torch.zeros(8, 8)] * 3), 2, view="cross", split=3)
    with pytest.raises(ValueError, match="view"):
        Fn.seq_view_attention(x, None, *([torch.zeros(8, 8)] * 3), 2, view="banded")
    with pytest.raises(ValueError, match=r"\[B,T,K\]"):
        layers.SeqViewAttentionLayer(2, 4)(torch.zeros(3, 8))
    with pytest.raises(ValueError, match="mask must be"):
        layers.SeqViewAttentionLayer(2, 4, view="causal")(torch.zeros(2, 3, 8), mask=torch.ones(2, 4, dtype=torch.bool))


def test_seqfm_value_errors():
    with pytest.raises(ValueError, match="att_heads"):
        models.SeqFM(att_heads=0)
    with pytest.raises(ValueError, match="ffn_layers"):
        models.SeqFM(ffn_layers=-1)
    m = models.SeqFM(att_heads=3, ffn_layers=2)
    assert m.att_heads == 3 and len(m.ffn) == 2 and isinstance(m.score, layers.MergeScoreLayer) and isinstance(m.stack, layers.StackLayer)
    emb = list(torch.zeros(2, 3, 8).split(1, dim=1))
    fea = lambda seq: models.InputFeature(denseInputs=[], sparseEmbed=emb, seqEmbedList=seq)
    with pytest.raises(ValueError, match="att_heads=3"):                       # 3 heads do not divide K = 8: known at the first call
        m(fea([[torch.zeros(2, 6, 8)], [torch.ones(2, 6, dtype=torch.bool)]]))
    for nothing in ([None, None], [[], []], None):                             # no behaviour
        with pytest.raises(ValueError, match="behaviour"):
            models.SeqFM()(fea(nothing))


def test_no_cpu_fallback():
    x, mask = torch.zeros(3, 5, 8), torch.ones(3, 5, dtype=torch.bool)
    w = [torch.zeros(8, 8)] * 3
    for kw in (dict(), dict(view="causal"), dict(view="cross", split=2, pool=True), dict(pool=True)):
        with pytest.raises(FilError, match="GPU only"):
            Fn.seq_view_attention(x, mask, *w, 2, **kw)
        with pytest.raises(FilError, match="GPU only"):
            layers.SeqViewAttentionLayer(2, 4, **kw)(x, mask=mask)
        with pytest.raises(FilError, match="GPU only"):
            layers.SeqViewAttentionLayer(1, 68, **kw)(x)                       # outside the menu: the composed path
    emb = list(torch.zeros(3, 2, 8).split(1, dim=1))
    with pytest.raises(FilError, match="GPU only"):
        models.SeqFM()(models.InputFeature(denseInputs=[], sparseEmbed=emb, seqEmbedList=[[x], [mask]]))


# ------------------------------------------------------------------------------------------------ the reference
def _cases(shape, seed, **kw):
    """Every view at `shape` (the cross view at two splits), rows out and pooled; ragged masks with sample 1 all masked and sample 0
    all live."""
    B, T = shape[:2]
    m = ref.make_mask(B, T, "ragged", np.random.default_rng(5))
    if B > 1:
        m[1] = 0
        m[0] = 1
    else:
        m[:] = 1
    splits = {"full": (0,), "causal": (0,), "cross": tuple(sorted({1, T - 1, (T + 1) // 2}))}
    for view in ref.VIEWS:
        for split in splits[view] if T > 1 or view != "cross" else ():
            for pool in (False, True):
                yield ref.make_case(*shape, seed=seed, view=view, split=split, pool=pool, mask=m, **kw)


def test_composed_graph_is_the_reference_on_the_cpu():
    n = 0
    for shape in ((4, 9, 8, 2, 4), (3, 2, 4, 1, 4), (1, 1, 4, 1, 4)):
        for use_scale in (True, False):
            for case in _cases(shape, seed=4, use_scale=use_scale):
                t = lambda k: torch.tensor(case[k], dtype=torch.float64)
                for mask in ((torch.tensor(case["mask"]),) + ((None,) if shape[0] == 1 else ())):
                    out = graph(t("x"), mask, t("Wq"), t("Wk"), t("Wv"), case["heads"], use_scale=use_scale, view=case["view"],
                                split=case["split"], pool=case["pool"])
                    want = ref.forward(case if mask is not None else dict(case, mask=None))
                    assert out.shape == want.shape and np.abs(out.numpy() - want).max() < 1e-12, (shape, case["view"], case["split"], case["pool"])
                    n += 1
    assert n >= 40


def test_reference_backward_equals_fp64_autograd():
    for shape in ((3, 3, 4, 1, 4), (4, 9, 8, 3, 4), (1, 1, 4, 1, 4)):
        for use_scale in (True, False):
            for case in _cases(shape, seed=3, use_scale=use_scale):
                what = (shape, case["view"], case["split"], case["pool"])
                out, hand = ref.forward(case), ref.backward(case)
                for g in (ref.torch_graph, graph):          # the restatement's own graph, and the composed path's
                    auto = ref.torch_run(case, torch.float64, graph=g)
                    assert np.abs(auto["out"] - out).max() < 1e-12, what
                    for k in ref.GRADS:
                        assert np.abs(auto[k] - hand[k]).max() < 1e-12 * max(1.0, np.abs(hand[k]).max()), (what, k)
                m = case["mask"]
                assert not hand["dx"][m == 0].any() and not ref.rows(case)[m == 0].any() and hand["dx"].any(), what
                if shape[0] > 1:
                    assert not out[1].any() and not hand["dx"][1].any(), what          # the all-masked sample


def test_reference_exact_facts():
    B, T, K, H, D = 3, 7, 8, 2, 4
    # view="full", pool=False is seq_attn_ref itself
    for mask in ("ragged", None):
        case = ref.make_case(B, T, K, H, D, seed=1, mask=mask)
        plain = base.make_case(B, T, K, H, D, seed=1, mask=mask)
        assert all(np.array_equal(case[k], plain[k]) for k in ("x", "g") + ref.PARAMS)
        assert np.array_equal(ref.forward(case), base.forward(plain))
        for k in ref.GRADS + ("ds", "v_rows"):
            assert np.array_equal(ref.backward(case)[k], base.backward(plain)[k]), k
    # a causal row reads nothing after itself: changing (or NaN-ing) x, the mask and g past t leaves rows <= t as they were
    case = ref.make_case(B, T, K, H, D, seed=2, view="causal", mask=None)
    out = ref.forward(case)
    for t in range(T - 1):
        x2 = case["x"].copy()
        x2[:, t + 1:] = 7.0 - x2[:, t + 1:]
        assert np.array_equal(ref.forward(dict(case, x=x2))[:, :t + 1], out[:, :t + 1]), t
        m2 = np.ones((B, T), np.uint8)
        m2[:, t + 1:] = 0
        assert np.array_equal(ref.forward(dict(case, mask=m2))[:, :t + 1], out[:, :t + 1]), t
    assert np.array_equal(out[:, 0], ref.backward(case)["v_rows"][:, 0])          # row 0 sees key 0 only
    assert not ref.backward(case)["ds"][:, :, 0].any()
    # the cross view: changing one static row's x leaves every other static row's output unchanged (static rows see only the history),
    # and changes the history rows'
    S = 3
    case = ref.make_case(B, T, K, H, D, seed=3, view="cross", split=S, mask=None)
    out = ref.forward(case)
    for r in range(S):
        x2 = case["x"].copy()
        x2[:, r] += 1.0
        out2 = ref.forward(dict(case, x=x2))
        others = [i for i in range(S) if i != r]
        assert np.array_equal(out2[:, others], out[:, others]) and not np.array_equal(out2[:, r], out[:, r]), r
        assert not np.array_equal(out2[:, S:], out[:, S:])
    # ... a sample whose history is all padding: its static rows have nothing to see, its output and gradients are exact zeros
    m = np.ones((B, T), np.uint8)
    m[1, S:] = 0
    for pool in (False, True):
        case = ref.make_case(B, T, K, H, D, seed=3, view="cross", split=S, pool=pool, mask=m)
        assert not ref.forward(case)[1].any() and not ref.backward(case)["dx"][1].any() and ref.forward(case)[0].any()
    # ... and with one live history slot every static row returns that slot's v row, with no score gradient
    m[1, S + 2] = 1
    case = ref.make_case(B, T, K, H, D, seed=3, view="cross", split=S, mask=m)
    out, bw = ref.forward(case), ref.backward(case)
    assert all(np.array_equal(out[1, r], bw["v_rows"][1, S + 2]) for r in range(S)) and not bw["ds"][1, :, :S].any() and bw["ds"][1, :, S + 2].any()
    # pooled is the mean of the live rows; gpool / n_b is the rows' gradient
    case = ref.make_case(B, T, K, H, D, seed=4, view="causal", pool=True)
    case["mask"][2] = 0
    live = case["mask"].astype(bool)
    rows_out = ref.rows(case)
    for b in range(B):
        want = rows_out[b][live[b]].mean(0) if live[b].any() else np.zeros(H * D)
        assert np.allclose(ref.forward(case)[b], want, rtol=1e-15, atol=1e-300), b
    g = ref.g_rows(case)
    assert not g[~live].any() and all(np.array_equal(g[b, t], case["gpool"][b] / live[b].sum()) for b in range(B) for t in range(T) if live[b, t])
    unpooled = ref.backward(dict(case, pool=False, g=g))
    for k in ref.GRADS:
        assert np.array_equal(ref.backward(case)[k], unpooled[k]), k
    # a masked position's x and g rows are never used
    case = ref.make_case(B, T, K, H, D, seed=2, view="cross", split=2)
    live = case["mask"].astype(bool)
    with np.errstate(invalid="ignore"):
        dirty = dict(case, x=np.where(live[:, :, None], case["x"], 1e30), g=np.where(live[:, :, None], case["g"], 1e30))
        assert np.array_equal(ref.forward(case), ref.forward(dirty))
        for k in ref.GRADS:
            assert np.array_equal(ref.backward(case)[k], ref.backward(dirty)[k]), k


def test_rows_with_one_allowed_key_send_no_score_gradient():
    """(1,1,4,1,4 | causal) and (3,2,4,1,4 | cross,1): every row has at most one key to see, so dWq and dWk are exactly 0."""
    for shape, view, split in (((1, 1, 4, 1, 4), "causal", 0), ((3, 2, 4, 1, 4), "cross", 1)):
        for pool in (False, True):
            case = ref.make_case(*shape, seed=0, view=view, split=split, pool=pool)
            bw = ref.backward(case)
            assert not bw["ds"].any() and not bw["dWq"].any() and not bw["dWk"].any(), (shape, pool)


def test_make_case_draws_what_the_bars_were_sized_on():
    c = ref.make_case(5, 28, 16, 1, 16, seed=0, view="cross", split=8, pool=True)
    for k in ("x", "g", "gpool") + ref.PARAMS:
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    assert c["gpool"].shape == (5, 16) and c["g"].shape == (5, 28, 16) and (c["view"], c["split"], c["pool"]) == ("cross", 8, True)
    # the fp32 torch restatement's own error at SeqFM's shapes: the 1e-5 floor binds (4 E32 < 1e-5); peaked rows: E32 <= 8e-6
    for shape, view, split in (((5, 20, 16, 1, 16), "causal", 0), ((5, 28, 16, 1, 16), "cross", 8), ((3, 7, 12, 3, 4), "cross", 3)):
        for pool in (False, True):
            _, _, e32 = ref.reference(ref.make_case(*shape, seed=0, view=view, split=split, pool=pool))
            assert set(e32) == {"out"} | set(ref.GRADS)
            assert set(ref.bars(e32).values()) == {1e-5}, (shape, view, pool, e32)
            if shape[2] == 16:
                _, _, e32 = ref.reference(ref.make_case(*shape, seed=0, view=view, split=split, pool=pool, w_scale=24.0))
                assert max(e32.values()) <= 8e-6, (shape, view, pool, e32)
    # the conditioned seeds of the tile-edge cases exist, and early
    for B in (1, 3, 84, 85, 86):
        for view, split in VARIANTS[1:]:
            for pool in (False, True):
                cc = ref.conditioned_case(B, *DIMS, view=view, split=split, pool=pool)
                assert max(ref.backward(cc)["cond"].values()) <= ref.MAX_COND and cc["shape"] == (B,) + DIMS and cc["seed"] <= 1, (B, view, split, pool, cc["seed"])
