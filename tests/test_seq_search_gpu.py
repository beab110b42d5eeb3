"""GPU checks of the top-k retrieval over a long behaviour history (include/fil.h N3 fil_seq_search, functional.seq_search,
models.SIMInput / SIM).  The kernel is held to EXACT equality of sel_pos, sel_idx, count and the bits of sel_score with the numpy
restatement (tests/seq_search_ref.py) and with functional.seq_search_graph; there is no tolerance anywhere.  The bits of the scores
are what catch a contracted multiply-add."""
import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, models, optim
from ml_function_amd import functional as Fn
from tests import seq_search_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel elements on either side of every output
SENT = -7777777
GRID_CAP = 4096


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _guarded(n, dtype):
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def kernel(case, scores=True):
    """fil_seq_search through ctypes on outputs that sit between sentinels -> the restatement's dict (sel_score None without scores)."""
    B, T = case["hist"].shape
    k = case["k"]
    K = 4 if case["table"] is None else case["table"].shape[1]
    t = {n: _dev(case[n]) for n in ("hist", "table", "q", "attr", "cand", "mask")}
    bufs = dict(sel_pos=_guarded(B * k, torch.int32), sel_idx=_guarded(B * k, torch.int64), count=_guarded(B, torch.int32),
                sel_score=_guarded(B * k, torch.float32) if scores else (None, None))
    oob = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    rc = _lib.load().fil_seq_search(p(t["hist"]), T, case["offset"], -1 if case["size"] is None else case["size"], case["pad"], p(t["mask"]),
                                    p(t["table"]), p(t["q"]), K, p(t["attr"]), T, p(t["cand"]), p(bufs["sel_pos"][1]),
                                    p(bufs["sel_idx"][1]), p(bufs["count"][1]), p(bufs["sel_score"][1]), p(oob), B, T, K, k,
                                    Fn.SEARCH_PREFER[case["prefer"]], _lib.stream_ptr())
    _lib.check(rc, "fil_seq_search")
    torch.cuda.synchronize()
    out = {}
    for name, (buf, view) in bufs.items():
        if buf is None:
            out[name] = None
            continue
        assert _intact(buf), name                                            # the sentinels on both sides of every output
        out[name] = view.cpu().numpy().reshape((B,) if name == "count" else (B, k))
    out["oob"] = int(oob)
    return out


def through(fn, case, scores=True, **kw):
    """functional.seq_search or seq_search_graph on the case -> the restatement's dict."""
    oob = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = {n: _dev(case[n]) for n in ("hist", "table", "q", "attr", "cand", "mask")}
    t.update(kw)
    res = fn(t["hist"], case["k"], table=t["table"], offset=case["offset"], size=case["size"], query=t["q"], attr=t["attr"], cand=t["cand"],
             mask=t["mask"], padding_id=case["pad"], prefer=case["prefer"], return_scores=scores, oob_count=oob)
    assert res[0].dtype == torch.int64 and res[1].dtype == torch.int32 and res[2].dtype == torch.int32 and len(res) == 3 + bool(scores)
    assert not any(r.requires_grad for r in res)
    return dict(sel_idx=res[0].cpu().numpy(), sel_pos=res[1].cpu().numpy(), count=res[2].cpu().numpy(),
                sel_score=res[3].cpu().numpy() if scores else None, oob=int(oob))


def same(got, want, what=""):
    for name in ("sel_pos", "sel_idx", "count"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
    if got["sel_score"] is not None:
        assert np.array_equal(got["sel_score"].view(np.int32), want["sel_score"].view(np.int32)), (what, "sel_score bits")
    assert got["oob"] == want["oob"], (what, "oob")


def held(case, what=""):
    """The kernel (raw and through functional.seq_search) and the torch graph against the restatement; -> the restatement's answer."""
    want = ref.search(case)
    same(kernel(case), want, (what, "kernel"))
    same(through(Fn.seq_search, case), want, (what, "seq_search"))
    same(through(Fn.seq_search_graph, case), want, (what, "graph"))
    return want


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("shape", [(3, 1, 4, 1), (2, 5, 4, 8), (2, 64, 16, 64), (3, 100, 64, 7)])
def test_small_and_edge_shapes(shape):
    B, T, K, k = shape
    for mode in ("soft", "hard", "both"):
        for prefer in ("first", "last"):
            held(ref.random_case(B, T, K, k, seed=T + k, mode=mode, prefer=prefer, ragged=T > 1), (shape, mode, prefer))
    held(ref.random_case(B, T, K, k, seed=1, ragged=False), (shape, "full"))


@pytest.mark.parametrize("T", [63, 64, 65, 255, 256, 257, 1000])
def test_lengths_around_the_wave_and_the_workgroup(T):
    for k in (1, 7, 50, 256):
        if k <= T:
            want = held(ref.random_case(3, T, 8, k, seed=T * 1000 + k), (T, k))
            assert want["count"][0] == k                                     # sample 0 is full: the radix select ran
            held(ref.random_case(3, T, 16, k, seed=T + k, mode="both", prefer="last", n_attr=2), (T, k, "both"))


def test_longest_history():
    case = ref.random_case(2, 16384, 4, 256, seed=5, vocab=3000)
    want = held(case, "T=16384")
    assert want["count"].tolist()[0] == 256
    held(ref.lattice_case(2, 16384, 4, 256, seed=6, prefer="last"), "T=16384 lattice")


def test_batch_past_the_grid_cap():
    B = GRID_CAP + 5
    assert Fn.seq_search_plan(B, 3, 4, 2)["grid"] == GRID_CAP
    want = held(ref.random_case(B, 3, 4, 2, seed=9, vocab=30), "past the cap")
    assert want["count"][GRID_CAP:].any()


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("prefer", ["first", "last"])
def test_integer_lattice_ties(prefer):
    for shape in ((4, 70, 4, 8), (3, 300, 8, 50), (2, 1000, 16, 256)):
        case = ref.lattice_case(*shape, seed=11, prefer=prefer)
        want = held(case, (shape, prefer))
        # a tie block does straddle the k-th place: the last selected score also occurs among the slots left out
        b = 0
        thr = want["sel_score"][b, :want["count"][b]].min()
        left_out = np.setdiff1d(np.nonzero(want["live"][b])[0], want["sel_pos"][b])
        assert (want["score"][b, left_out] == thr).any(), shape


@pytest.mark.parametrize("prefer", ["first", "last"])
def test_every_row_takes_the_same_score(prefer):
    B, T, K, k, V = 3, 300, 4, 50, 40
    rng = np.random.default_rng(3)
    table = np.tile(rng.standard_normal((1, K)).astype(np.float32), (V, 1))
    hist = rng.integers(1, V, (B, T))
    hist[1, 100:] = 0
    hist[2, ::3] = 0                                                           # padding in the middle
    case = ref.make_case(hist, k, table=table, q=rng.standard_normal((B, K)), size=V, prefer=prefer)
    want = held(case, prefer)
    live0 = np.nonzero(want["live"][2])[0]
    assert want["sel_pos"][2].tolist() == (live0[:k] if prefer == "first" else live0[-k:]).tolist()


def test_scores_that_differ_in_the_last_bit():
    B, T, K, k, V = 2, 257, 4, 50, 300
    table = np.zeros((V, K), np.float32)
    table[:, 0] = (np.float32(1.0) + np.arange(V, dtype=np.float32) * np.float32(2.0 ** -23))            # consecutive floats
    table[:, 1] = np.float32(3.0)
    rng = np.random.default_rng(4)
    hist = rng.integers(1, V, (B, T))
    q = np.array([[1, 0, 0, 0], [-1, 0.5, 0, 0]], np.float32)
    for prefer in ("first", "last"):
        want = held(ref.make_case(hist, k, table=table, q=q, size=V, prefer=prefer), prefer)
        assert len(np.unique(want["score"][0])) > 100


def test_negative_scores_zeros_and_infinities():
    special = np.array([-np.inf, -3e38, -2.5, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 2.5, 3e38, np.inf], np.float32)
    V, K = len(special) + 1, 4
    table = np.zeros((V, K), np.float32)
    table[1:, 0] = special
    rng = np.random.default_rng(5)
    hist = rng.integers(1, V, (4, 130))
    hist[3, 50:] = 0
    q = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0.5, 0, 0, 0], [-2, 0, 0, 0]], np.float32)
    for k in (3, 20, 100):
        for prefer in ("first", "last"):
            want = held(ref.make_case(hist, k, table=table, q=q, size=V, prefer=prefer), (k, prefer))
            assert not np.isnan(want["score"]).any()
    assert np.isinf(want["sel_score"]).any() and (want["sel_score"] < 0).any()
    # all scores negative: the tail's +0 must not be mistaken for a score, and the best are the least negative
    neg = ref.make_case(hist, 7, table=-np.abs(np.random.default_rng(6).standard_normal((V, K))).astype(np.float32) - 1,
                        q=np.ones((4, K), np.float32), size=V)
    want = held(neg, "negative")
    assert (want["sel_score"][0] < 0).all()


# ------------------------------------------------------------------------------------------------ the live set
def test_live_set_ragged_padding_mask_and_an_empty_sample():
    B, T, K, k = 5, 200, 8, 20
    rng = np.random.default_rng(7)
    base = ref.random_case(B, T, K, k, seed=8, mode="both", n_attr=2)
    hist = base["hist"].copy()
    hist[0, rng.random(T) < 0.3] = 0                                           # padding in the middle
    hist[2, :] = 0                                                             # no live slot by padding
    mask = (rng.random((B, T)) < 0.7).astype(np.uint8)
    mask[3, :] = 0                                                             # no live slot by the mask
    for prefer in ("first", "last"):
        for part in ("soft", "hard", "both"):
            case = dict(base, hist=hist, mask=mask, prefer=prefer)
            if part == "soft":
                case.update(attr=None, cand=None)
            if part == "hard":
                case.update(table=None, q=None)
            want = held(case, (prefer, part))
            assert want["count"][2] == 0 and want["count"][3] == 0 and want["count"].max() == k
            assert (want["sel_pos"][2] == -1).all() and (want["sel_idx"][3] == 0).all()
    bool_mask = through(Fn.seq_search, case, mask=_dev(mask).bool())
    same(bool_mask, want, "bool mask")


def test_out_of_range_ids_and_the_padding_row_never_win():
    B, T, K, k = 3, 150, 4, 12
    offset, size, V = 10, 20, 50
    rng = np.random.default_rng(9)
    table = rng.standard_normal((V, K)).astype(np.float32)
    table[:offset] = 1e30
    table[offset + size:] = 1e30                 # what an id out of range for its field would land on inside the concatenated table
    table[offset] = 1e30                         # the row of pad_id = 0
    hist = rng.integers(1, size, (B, T))
    hist[:, 5::17] = rng.integers(size, V - offset, hist[:, 5::17].shape)       # too large, but inside the table
    hist[:, 3::19] = -rng.integers(1, offset + 1, hist[:, 3::19].shape)         # negative, but inside the table
    hist[:, 7::11] = 0
    q = np.abs(rng.standard_normal((B, K))).astype(np.float32) + 1
    q[:, 1:] = 0                                 # one huge product at most: 1e30 * q stays finite
    table[:, 1:] = np.abs(table[:, 1:])
    for prefer in ("first", "last"):
        want = held(ref.make_case(hist, k, table=table, q=q, offset=offset, size=size, prefer=prefer), prefer)
        assert want["oob"] == int(((hist >= size) | (hist < 0)).sum()) > 0
        assert (np.abs(want["sel_score"]) < 1e20).all() and (want["sel_idx"] > 0).all() and (want["sel_idx"] < size).all()
    # ids that are trusted (size=None) read whatever row they name: here every id is in range, so nothing changes but the count
    inside = np.where((hist >= size) | (hist < 0), 0, hist)
    a = held(ref.make_case(inside, k, table=table, q=q, offset=offset, size=None), "trusted")
    b = ref.search(ref.make_case(inside, k, table=table, q=q, offset=offset, size=size))
    assert np.array_equal(a["sel_pos"], b["sel_pos"]) and a["oob"] == 0


def test_nan_scores_give_a_valid_selection():
    B, T, K, k, V = 3, 200, 4, 30, 60
    rng = np.random.default_rng(10)
    table = rng.standard_normal((V, K)).astype(np.float32)
    table[7] = np.nan
    table[9, 2] = np.nan
    hist = rng.integers(1, V, (B, T))
    hist[:, ::9] = 7
    hist[1, 120:] = 0
    case = ref.make_case(hist, k, table=table, q=rng.standard_normal((B, K)), size=V)
    live, _ = ref.live_slots(case)
    for got in (kernel(case), through(Fn.seq_search_graph, case)):
        for b in range(B):
            n = got["count"][b]
            assert n == min(k, live[b].sum())
            pos = got["sel_pos"][b, :n]
            assert (np.diff(pos) > 0).all() and live[b, pos].all() and (got["sel_pos"][b, n:] == -1).all()
            assert np.array_equal(got["sel_idx"][b, :n], hist[b, pos])


# ------------------------------------------------------------------------------------------------ the contract
def test_scores_are_optional_repeats_are_identical_and_a_sample_stands_alone():
    case = ref.random_case(6, 500, 16, 50, seed=12, mode="both", n_attr=2)
    want = ref.search(case)
    first = kernel(case)
    same(first, want)
    bare = kernel(case, scores=False)
    assert bare["sel_score"] is None
    same(bare, want, "sel_score = NULL")
    same(through(Fn.seq_search, case, scores=False), want, "return_scores=False")
    for _ in range(3):
        again = kernel(case)
        same(again, first, "repeat")
    for b in (0, 3, 5):
        alone = dict(case, hist=case["hist"][b:b + 1], q=case["q"][b:b + 1], attr=case["attr"][b:b + 1], cand=case["cand"][b:b + 1])
        got = kernel(alone)
        for name in ("sel_pos", "sel_idx", "count"):
            assert np.array_equal(got[name][0], first[name][b]), (b, name)
        assert np.array_equal(got["sel_score"][0].view(np.int32), first["sel_score"][b].view(np.int32))


def test_strided_history_attribute_and_query():
    case = ref.random_case(5, 130, 8, 9, seed=13, mode="both", n_attr=2)
    want = ref.search(case)
    B, T = case["hist"].shape
    wide_hist = torch.full((B, 3, T), 5, dtype=torch.int64, device="cuda")
    wide_attr = torch.full((B, 3, T), 1, dtype=torch.int64, device="cuda")
    wide_q = torch.full((B, 2, 8), 9.0, device="cuda")
    wide_hist[:, 1] = _dev(case["hist"])
    wide_attr[:, 1] = _dev(case["attr"])
    wide_q[:, 1] = _dev(case["q"])
    assert not wide_hist[:, 1].is_contiguous() and not wide_q[:, 1].is_contiguous()
    same(through(Fn.seq_search, case, hist=wide_hist[:, 1], attr=wide_attr[:, 1], q=wide_q[:, 1]), want, "row strides")
    # strides the kernel does not read in place: a transposed history, a query with a column stride, an expanded candidate
    hist_t = _dev(case["hist"]).t().contiguous().t()
    q_cols = torch.zeros((B, 16), device="cuda")
    q_cols[:, ::2] = _dev(case["q"])
    assert hist_t.stride(1) != 1
    same(through(Fn.seq_search, case, hist=hist_t, q=q_cols[:, ::2]), want, "copied")


def test_replays_from_a_hip_graph_with_changed_inputs():
    cases = [ref.random_case(7, 300, 16, 50, seed=20 + s, vocab=500, mode="both", n_attr=2) for s in range(3)]
    t = {n: _dev(cases[0][n]) for n in ("hist", "table", "q", "attr", "cand")}
    oob = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = lambda: Fn.seq_search(t["hist"], 50, table=t["table"], size=500, query=t["q"], attr=t["attr"], cand=t["cand"], return_scores=True,
                                oob_count=oob)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run()
    for case in cases[::-1]:
        for n in t:
            t[n].copy_(_dev(case[n]))
        g.replay()
        torch.cuda.synchronize()
        got = dict(sel_idx=res[0].cpu().numpy(), sel_pos=res[1].cpu().numpy(), count=res[2].cpu().numpy(), sel_score=res[3].cpu().numpy(), oob=0)
        same(got, ref.search(case), "replay")


def test_outside_the_menu_the_graph_runs_and_equals_the_restatement():
    assert Fn.seq_search_plan(4, 90, 6, 10) == dict(fits=False)
    for prefer in ("first", "last"):
        case = ref.random_case(4, 90, 6, 10, seed=14, prefer=prefer)
        same(through(Fn.seq_search, case), ref.search(case), "K=6")
    case = ref.random_case(2, 40, 4, 300, seed=15)                             # k > 256
    same(through(Fn.seq_search, case), ref.search(case), "k=300")
    empty = Fn.seq_search(torch.zeros((0, 9), dtype=torch.int64, device="cuda"), 4, table=torch.zeros((5, 4), device="cuda"),
                          query=torch.zeros((0, 4), device="cuda"), return_scores=True)
    assert [tuple(r.shape) for r in empty] == [(0, 4), (0, 4), (0,), (0, 4)]


# ------------------------------------------------------------------------------------------------ the model
VOCAB = (50, 4, 7)               # item, cate, user
B_M, TL, K_SEL, K_EMB = 33, 70, 8, 8


def _sim_batch(seed, B=B_M):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(1, v, B) for v in VOCAB], 1)
    long_idx = rng.integers(1, VOCAB[0], (B, 1, TL))
    lens = rng.integers(1, TL + 1, B)
    long_idx[np.arange(TL)[None, None, :] >= lens[:, None, None]] = 0
    long_attr = rng.integers(1, VOCAB[1], (B, 1, TL))
    return _dev(idx), _dev(long_idx), _dev(long_attr)


def _info():
    return models.make_sparse_info(list(VOCAB), embed_dim=K_EMB, names=["item", "cate", "user"])


def _sim_model(mode, seed=3):
    torch.manual_seed(seed)
    long_b = [("item", TL, K_SEL, mode, None if mode == "soft" else "cate")]
    return models.CTRModel(models.SIMInput(_info(), None, long_b), models.SIM(att_hidden_units=(8, 4), hidden_units=[16, 8])).cuda()


@pytest.mark.parametrize("mode", ["soft", "hard", "both"])
def test_sim_equals_din_on_the_restatements_selection(mode):
    idx, long_idx, long_attr = _sim_batch(31)
    sim = _sim_model(mode)
    torch.manual_seed(3)
    logits = sim(None, idx, (None, long_idx, None if mode == "soft" else long_attr))
    torch.manual_seed(3)
    din = models.CTRModel(models.DINInput(_info(), [("item", K_SEL)]),
                          models.DIN(att_hidden_units=(8, 4), att_softmax=True, hidden_units=[16, 8])).cuda()
    table = sim.feature_input.sparse_embed.embeddings.detach().cpu().numpy()
    ids = idx.cpu().numpy()
    soft, hard = mode != "hard", mode != "soft"
    case = ref.make_case(long_idx[:, 0].cpu().numpy(), K_SEL, table=table if soft else None, q=table[ids[:, 0]] if soft else None,
                         attr=long_attr[:, 0].cpu().numpy() if hard else None, cand=ids[:, 1] if hard else None, offset=0, size=VOCAB[0],
                         prefer="last")
    want = ref.search(case)
    assert want["count"].min() < K_SEL == want["count"].max()                  # retrieved sets with and without a padded tail
    hist = _dev(want["sel_idx"]).reshape(B_M, 1, K_SEL)
    torch.manual_seed(3)
    ref_logits = din(None, idx, hist)
    params_s, params_d = dict(sim.named_parameters()), dict(din.named_parameters())
    assert list(params_s) == list(params_d)
    for n in params_s:
        assert torch.equal(params_s[n], params_d[n]), n                       # the same seed built the same model
    assert torch.equal(logits, ref_logits)
    w = torch.linspace(-1, 1, logits.numel(), device="cuda").reshape(logits.shape)
    (logits * w).sum().backward()
    (ref_logits * w).sum().backward()
    for n in params_s:
        assert (params_s[n].grad is None) == (params_d[n].grad is None), n
        assert params_s[n].grad is None or torch.equal(params_s[n].grad, params_d[n].grad), n
    assert params_s["feature_input.sparse_embed.embeddings"].grad.abs().sum() > 0
    # the search in torch ops retrieves the same ids, and the same keys come out of the gather
    args = (None, idx, None, long_idx, None if mode == "soft" else long_attr)
    fused = sim.feature_input(args)
    sim.feature_input.search_fn = Fn.seq_search_graph
    composed = sim.feature_input(args)
    assert torch.equal(fused.seq_inputs[0], hist[:, 0]) and torch.equal(composed.seq_inputs[0], hist[:, 0])
    assert torch.equal(fused.seq_embed_list[0][0], composed.seq_embed_list[0][0])


def test_sim_with_a_short_history_beside_the_long_one():
    torch.manual_seed(5)
    long_b = [("item", TL, K_SEL, "both", "cate"), ("item", TL, 4, "soft", None)]
    model = models.CTRModel(models.SIMInput(_info(), [("item", 6)], long_b), models.SIM(att_hidden_units=(8, 4), hidden_units=[16, 8])).cuda()
    idx, long_idx, long_attr = _sim_batch(41)
    long_idx = torch.cat([long_idx, long_idx.flip(2)], 1).contiguous()
    long_attr = torch.cat([long_attr, long_attr], 1).contiguous()
    hist = long_idx[:, :1, :6].contiguous()
    fea = model.feature_input((None, idx, hist, long_idx, long_attr))
    keys, masks = fea.seq_embed_list
    assert [tuple(t.shape) for t in keys] == [(B_M, 6, K_EMB), (B_M, K_SEL, K_EMB), (B_M, 4, K_EMB)]
    assert fea.seq_info == [(0, 6), (0, K_SEL), (0, 4)] and len(fea.seq_inputs) == 3
    table = model.feature_input.sparse_embed.embeddings.detach()
    for m, kk in ((1, K_SEL), (2, 4)):
        assert torch.equal(masks[m], fea.seq_inputs[m] != 0) and torch.equal(keys[m], table[fea.seq_inputs[m]])
    out = model(None, idx, (hist, long_idx, long_attr))
    assert tuple(out.shape) == (B_M, 2) and len(model.body.atten) == 3     # MergeScoreLayer(use_merge=False): the two-class softmax
    out.sum().backward()
    assert model.feature_input.sparse_embed.embeddings.grad is not None
    with pytest.raises(ValueError, match="SIMInput"):
        model(None, idx, (hist, long_idx[:, :1], long_attr))
    with pytest.raises(ValueError, match="SIMInput"):
        model(None, idx, (hist, long_idx, None))


def test_sim_training_step_replays_from_capture_step():
    batches = []
    for s in range(4):
        idx, long_idx, long_attr = _sim_batch(50 + s)
        y = _dev((np.random.default_rng(60 + s).random(B_M) < 0.4).astype(np.float32))
        batches.append((idx, long_idx, long_attr, y))

    def make():
        model = _sim_model("both", seed=7)
        model(None, batches[0][0], (None, batches[0][1], batches[0][2]))
        opt = optim.Adam(model.parameters(), learning_rate=1e-2)

        def step(idx, long_idx, long_attr, y):
            opt.zero_grad()
            p = model(None, idx, (None, long_idx, long_attr))[:, 0]
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
    assert not torch.equal(model_c.feature_input.sparse_embed.embeddings, init["feature_input.sparse_embed.embeddings"])
