"""Host-only checks of the top-k retrieval over a long behaviour history (include/fil.h N3 fil_seq_search, functional.seq_search,
models.SIMInput / SIM): the entry points in the header, the binding and the library; their argument validation, the menu limits and
the plan's arithmetic through ctypes; the Python surface that needs no GPU; and self-checks of the numpy restatement
(tests/seq_search_ref.py) the GPU tests are held to."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import seq_search_ref as ref

NEW = ("fil_seq_search_plan", "fil_seq_search")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
LDS_LIMIT = 163328
GRID_CAP = 4096
P = 4096          # any non-NULL, 16-byte aligned address: every call below returns before a pointer is followed


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, k):
    plan = (ctypes.c_int * 8)()
    rc = lib.fil_seq_search_plan(B, T, K, k, plan)
    return rc, list(plan)


def _msg(lib):
    return lib.fil_last_error().decode()


def _call(lib, B=5, T=9, K=4, k=3, flags=0, hist_stride=None, q_stride=None, attr_stride=None, **ptrs):
    """fil_seq_search with every pointer at P unless named (None = NULL); the optional mask, sel_score and oob_count default to NULL."""
    a = dict(hist=P, mask=None, table=P, q=P, attr=P, cand=P, sel_pos=P, sel_idx=P, count=P, sel_score=None, oob=None)
    a.update(ptrs)
    return lib.fil_seq_search(a["hist"], T if hist_stride is None else hist_stride, 0, 100, 0, a["mask"], a["table"], a["q"],
                              K if q_stride is None else q_stride, a["attr"], T if attr_stride is None else attr_stride, a["cand"],
                              a["sel_pos"], a["sel_idx"], a["count"], a["sel_score"], a["oob"], B, T, K, k, flags, None)


def test_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    Pt, I, L = _lib._P, _lib._I, ctypes.c_int64
    assert _lib.SIGNATURES["fil_seq_search_plan"] == (I, [I] * 4 + [Pt])
    assert _lib.SIGNATURES["fil_seq_search"] == (I, [Pt, L, L, L, L, Pt, Pt, Pt, L, Pt, L] + [Pt] * 6 + [I] * 5 + [Pt])
    assert _lib.FIL_SEARCH_PREFER_LAST == 1 and "#define FIL_SEARCH_PREFER_LAST 1" in open(_lib.HEADER_PATH).read()


def test_argument_validation(lib):
    # B == 0: a no-op that returns 0 before any pointer is looked at
    assert lib.fil_seq_search(None, 9, 0, 100, 0, *([None] * 3), 4, None, 9, *([None] * 6), 0, 9, 4, 3, 0, None) == OK
    # a NULL required pointer
    for hole in ("hist", "sel_pos", "sel_idx", "count"):
        assert _call(lib, **{hole: None}) == ERR_ARG, hole
        assert "fil_seq_search" in _msg(lib)
    # neither part, half of a part
    assert _call(lib, table=None, q=None, attr=None, cand=None) == ERR_ARG
    for hole in ("table", "q", "attr", "cand"):
        assert _call(lib, **{hole: None}) == ERR_ARG, hole
    # non-positive dimensions
    for dims in (dict(B=-1), dict(T=0), dict(K=0), dict(k=0), dict(T=-3), dict(k=-1)):
        assert _call(lib, **dims) == ERR_ARG, dims
        full = dict(B=5, T=9, K=4, k=3)
        full.update(dims)
        assert _plan(lib, **full)[0] == ERR_ARG
    assert lib.fil_seq_search_plan(5, 9, 4, 3, None) == ERR_ARG
    # unknown flags
    for flags in (2, 4, 3, -1):
        assert _call(lib, flags=flags) == ERR_ARG and "flags" in _msg(lib), flags
    # rows that overlap, a table off the 16-byte grid
    assert _call(lib, hist_stride=8) == ERR_ARG and _call(lib, q_stride=3) == ERR_ARG and _call(lib, attr_stride=8) == ERR_ARG
    assert _call(lib, table=P + 4) == ERR_ARG


def test_menu_limits_from_both_sides(lib):
    outside = ((dict(K=6), "K=6", "% 4"), (dict(K=68), "K=68", "<= 64"), (dict(k=257), "k=257", "<= 256"),
               (dict(T=16385), "T=16385", "<= 16384"), (dict(B=1 << 17, T=16384), "2^31", "B*T"))
    for dims, word, limit in outside:
        full = dict(B=5, T=9, K=4, k=3)
        full.update(dims)
        assert _plan(lib, **full)[0] == ERR_UNSUPPORTED, dims
        assert word in _msg(lib) and limit in _msg(lib) and "fil_seq_search_plan" in _msg(lib), (_msg(lib), word)
        assert _call(lib, **dims) == ERR_UNSUPPORTED and "fil_seq_search" in _msg(lib)
        assert Fn.seq_search_plan(**full) == dict(fits=False)
    # the inside edges: the widest row, the longest history and the largest k at once, and B T one below 2^31; k may exceed T
    for full in (dict(B=5, T=16384, K=64, k=256), dict(B=(1 << 17) - 1, T=16384, K=4, k=1), dict(B=5, T=1, K=4, k=256)):
        rc, pl = _plan(lib, **full)
        assert rc == OK and pl[0] == 1 and 0 < pl[6] <= LDS_LIMIT, (full, _msg(lib))


def test_plan_arithmetic(lib):
    up = lambda v, m: -(-v // m) * m
    for T, K, k in ((1, 4, 1), (3, 4, 8), (63, 8, 7), (64, 16, 64), (65, 16, 50), (1000, 16, 50), (1024, 16, 50), (4096, 16, 50),
                    (16384, 64, 256)):
        lds = 4 * (K + up(T, 4)) + 8 * up(T, 64) // 64 + 4 * 256 + 4 * 16        # q | keys | live bitmap | histogram | hand-over
        for B in (0, 1, 33, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 1 << 16):
            rc, (fwd_ok, bwd_ok, tile, grid, cap, parts, lds_f, lds_b) = _plan(lib, B, T, K, k)
            assert rc == OK and fwd_ok == 1 and bwd_ok == 1 and tile == 1 and cap == GRID_CAP
            assert grid == min(B, cap) and parts == grid
            assert lds_f == lds and lds_b == 0 and lds_f <= LDS_LIMIT
    assert Fn.seq_search_plan(4096, 1024, 16, 50) == dict(fits=True, tile=1, grid=4096, cap=4096, partials=4096, lds_fwd=5376, lds_bwd=0)
    assert Fn.seq_search_plan(5000, 3, 4, 1)["grid"] == GRID_CAP            # past the cap a workgroup walks several samples
    with pytest.raises(FilError):
        Fn.seq_search_plan(8, 0, 16, 2)


# ------------------------------------------------------------------------------------------------ the restatement
def _cases():
    yield ref.random_case(4, 37, 8, 5, seed=1)
    yield ref.random_case(3, 20, 4, 30, seed=2, prefer="last")                                   # T < k
    yield ref.random_case(5, 50, 4, 7, seed=3, mode="hard")
    yield ref.random_case(5, 50, 4, 7, seed=3, mode="hard", prefer="last")
    yield ref.random_case(5, 64, 8, 9, seed=4, mode="both", prefer="last")
    yield ref.lattice_case(4, 70, 4, 8, seed=5)
    yield ref.lattice_case(4, 70, 4, 8, seed=5, prefer="last")


def test_restatement_equals_brute_force_on_tuples():
    for case in _cases():
        got = ref.search(case)
        want = ref.brute_force(case)
        for b, slots in enumerate(want):
            n = len(slots)
            assert got["count"][b] == n == min(case["k"], int(got["live"][b].sum()))
            assert list(got["sel_pos"][b, :n]) == slots, (b, case["prefer"])
            assert (got["sel_pos"][b, n:] == -1).all() and (got["sel_idx"][b, n:] == case["pad"]).all()
            assert not got["sel_score"][b, n:].any() and not np.signbit(got["sel_score"][b, n:]).any()
            assert np.array_equal(got["sel_idx"][b, :n], case["hist"][b, slots])
            assert np.array_equal(got["sel_score"][b, :n].view(np.int32), got["score"][b, slots].view(np.int32))


def test_restatement_on_the_lattice_equals_a_float64_score():
    # every product and partial sum is a small integer: fp32 is exact, so a float64 dot product orders the slots the same way --
    # except that the key tells -0 from +0 and float64 comparison does not; the lattice's sums never give -0 (they start at +0)
    for prefer in ("first", "last"):
        case = ref.lattice_case(6, 90, 8, 10, seed=7, prefer=prefer)
        t64, q64 = case["table"].astype(np.float64), case["q"].astype(np.float64)
        score64 = lambda b, t: float(t64[case["hist"][b, t] + case["offset"]] @ q64[b])
        got = ref.search(case)
        assert not np.signbit(got["score"]).any() or (got["score"][np.signbit(got["score"])] != 0).all()
        want = ref.brute_force(case, score64)
        for b, slots in enumerate(want):
            assert list(got["sel_pos"][b, :len(slots)]) == slots
        assert np.array_equal(got["score"].astype(np.float64), np.einsum("btk,bk->bt", t64[case["hist"]], q64))
        # the scores do tie: fewer distinct values than slots by far
        assert len(np.unique(got["score"][0])) < 60


def test_keys_order_like_the_scores():
    vals = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, np.inf], np.float32)
    k = ref.keys(vals)
    assert (np.diff(k) > 0).all() and k[4] == ref.KEY_ZERO and k.min() >= 0 and k.max() < 1 << 32


def test_restatement_live_set_and_counting():
    hist = np.array([[1, 0, 7, 9, -2, 3, 0, 3]])
    case = ref.make_case(hist, 4, attr=np.array([[5, 5, 5, 4, 5, 5, 5, 5]]), cand=np.array([5]), mask=np.array([[1, 1, 1, 1, 1, 0, 1, 1]]), size=8)
    live, oob = ref.live_slots(case)
    assert live.tolist() == [[True, False, True, False, False, False, False, True]] and oob == 2       # 9 and -2; padding is not counted
    got = ref.search(case)
    assert got["sel_pos"].tolist() == [[0, 2, 7, -1]] and got["sel_idx"].tolist() == [[1, 7, 3, 0]] and got["count"].tolist() == [3]
    got = ref.search(dict(case, k=2, prefer="last"))
    assert got["sel_pos"].tolist() == [[2, 7]]
    got = ref.search(dict(case, k=2))
    assert got["sel_pos"].tolist() == [[0, 2]]


def test_graph_equals_the_restatement_on_the_cpu():
    for case in _cases():
        t = lambda key: None if case[key] is None else torch.tensor(case[key])
        oob = torch.zeros((), dtype=torch.int32)
        sel_idx, sel_pos, count, score = Fn.seq_search_graph(t("hist"), case["k"], table=t("table"), offset=case["offset"], size=case["size"],
                                                             query=t("q"), attr=t("attr"), cand=t("cand"), mask=t("mask"),
                                                             padding_id=case["pad"], prefer=case["prefer"], return_scores=True, oob_count=oob)
        want = ref.search(case)
        assert np.array_equal(sel_pos.numpy(), want["sel_pos"]) and sel_pos.dtype == torch.int32
        assert np.array_equal(sel_idx.numpy(), want["sel_idx"]) and sel_idx.dtype == torch.int64
        assert np.array_equal(count.numpy(), want["count"]) and count.dtype == torch.int32
        assert np.array_equal(score.numpy().view(np.int32), want["sel_score"].view(np.int32))
        assert int(oob) == want["oob"]


# ------------------------------------------------------------------------------------------------ the Python surface
def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_surface_and_defaults():
    E = inspect.Parameter.empty
    want = dict(hist_idx=E, k=E, table=None, offset=0, size=None, query=None, attr=None, cand=None, mask=None, padding_id=0,
                prefer="first", return_scores=False, oob_count=None)
    assert _sig(Fn.seq_search) == want and _sig(Fn.seq_search_graph) == want
    assert list(_sig(Fn.seq_search_plan)) == ["B", "T", "K", "k"]
    assert _sig(models.SIMInput.__init__) == dict(sparseInfo=E, behavior=E, long_behavior=E, denseInfo=None, padding_id=0, prefer="last")
    assert _sig(models.SIM.__init__) == dict(att_hidden_units=(80, 40), att_activation="prelu", hidden_units=None)
    assert issubclass(models.SIMInput, models.DINInput) and issubclass(models.SIM, models._BehaviorModel)
    assert _sig(models.DINInput.__init__) == dict(sparseInfo=E, behavior=E, denseInfo=None, padding_id=0, tableGrad="dense")
    m = models.SIM(att_hidden_units=(8, 4))
    assert m.att_args == dict(hidden_units=(8, 4), activation="prelu", softmax=True) and len(m.atten) == 0


def test_sim_input_validation():
    info = models.make_sparse_info([50, 9, 7], embed_dim=8, names=["item", "cate", "user"])
    ok = models.SIMInput(info, [("item", 5)], [("item", 70, 8, "both", "cate"), ("item", 70, 4, "soft", None)])
    assert [e["offset"] for e in ok.long_behavior] == [0, 0] and ok.long_behavior[0]["attr_field"] == 1 and ok.behavior == [(0, 5)]
    assert models.SIMInput(info, None, [("cate", 70, 8, "hard", "user")]).long_behavior[0]["offset"] == 50
    for bad in ([("nope", 70, 8, "soft", None)], [("item", 0, 8, "soft", None)], [("item", 70, 0, "soft", None)],
                [("item", 70, 8, "fuzzy", None)], [("item", 70, 8, "hard", None)], [("item", 70, 8, "soft", "cate")],
                [("item", 70, 8, "both", "nope")], [], [("item", 70, 8, "soft", None), ("item", 60, 8, "soft", None)]):
        with pytest.raises(ValueError, match="SIMInput"):
            models.SIMInput(info, [("item", 5)], bad)
    with pytest.raises(ValueError, match="prefer"):
        models.SIMInput(info, None, [("item", 70, 8, "soft", None)], prefer="middle")


def test_argument_checks_and_no_cpu_fallback():
    hist = torch.ones(3, 9, dtype=torch.int64)
    table, q = torch.zeros(20, 4), torch.zeros(3, 4)
    with pytest.raises(FilError, match="GPU only"):
        Fn.seq_search(hist, 2, table=table, query=q)
    with pytest.raises(FilError, match="GPU only"):
        Fn.seq_search(hist, 2, attr=hist, cand=torch.ones(3, dtype=torch.int64))
    for kw in (dict(), dict(table=table), dict(query=q), dict(attr=hist), dict(table=table, query=q, cand=torch.ones(3, dtype=torch.int64))):
        with pytest.raises(FilError, match="soft search"):
            Fn.seq_search_graph(hist, 2, **kw)
    with pytest.raises(FilError, match="int64"):
        Fn.seq_search_graph(hist.to(torch.int32), 2, table=table, query=q)
    with pytest.raises(FilError, match=r"\[B,K\]"):
        Fn.seq_search_graph(hist, 2, table=table, query=torch.zeros(3, 8))
    with pytest.raises(FilError, match="not inside the table"):
        Fn.seq_search_graph(hist, 2, table=table, query=q, offset=15, size=6)
    with pytest.raises(FilError, match="positive"):
        Fn.seq_search_graph(hist, 0, table=table, query=q)
    with pytest.raises(ValueError, match="prefer"):
        Fn.seq_search_graph(hist, 2, table=table, query=q, prefer="best")
