"""The integer-lattice CIN cases (tests/cin_lattice_cases.py) have the properties tests/test_cin_lattice_gpu.py relies on.  No GPU.

For every case of the table and every seed of it: each operand family of the one-plane bf16 kernels is made of bf16 numbers; the net
evaluated on absolute values stays below 2^24 (2^23 for an even F, whose halved pair weights make multiples of 1/2) in every tensor
but the recorded head tensors of Dense(1) cases; and, over the case's seeds, no sparsity hides an index: every pair slot of W1s and of
Ts is nonzero in some column, no weight column is empty, every field is nonzero in every block of 32 rows, and at least 95 % of the
entries of every oracle gradient are nonzero.  The oracle restatement used here for speed (rows_oracle) is held equal to
oracle/closed.py, and that to oracle/graph.py, exactly, on the lattice; the table's precision column is held to the library's answer.
"""
import numpy as np
import pytest
import torch

from oracle import closed, graph
from tests import cin_lattice_cases as lc

CASE_IDS = [c.id for c in lc.CASES]


def test_is_bf16():
    assert lc.is_bf16([0.0, -0.0, 1.0, -255.0, 256.0, 258.0, 302.0, 0.5, 2.0 ** 100, 1.0 + 2.0 ** -7])
    for v in (257.0, 301.0, 1.0 + 2.0 ** -8, 0.1, 1e-300, np.float64(np.float32(0.1))):
        assert not lc.is_bf16([1.0, v]), v


def test_to_bf16_rounds_to_nearest_even():
    v = np.concatenate([np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 37,
                        np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 0.0, 257.0, 259.0], np.float32)])
    want = torch.tensor(v).to(torch.bfloat16).to(torch.float32).numpy()
    got = lc.to_bf16(v)
    assert np.array_equal(got, want) and lc.is_bf16(got)
    assert list(got[4096:4100]) == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]      # ties to even, both ways; above a tie; the sign


def test_the_table_holds_the_required_cases():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    have = {(c.group, c.B, c.F, c.K, c.H, c.output_dim) for c in lc.CASES}
    H3, WIDE = (128, 128, 128), (128, 130, 8)
    for F in (2, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 31, 32, 39, 40, 41, 42):
        assert ("F", 17, F, 8, H3, 2) in have
    for F in (42, 47, 48):
        assert ("F", 17, F, 8, WIDE, 2) in have
    for c in lc.CASES:
        if c.group == "F":
            assert 100 <= c.M <= 200
    for F in (12, 39):
        for H in ((100, 37, 9), (3, 2, 2), (128, 200, 12), (64, 48, 8)):
            assert ("width", 17, F, 8, H, 2) in have
        for B, K in ((1, 1), (31, 1), (33, 1), (127, 1), (129, 1), (7, 5), (3, 64), (17, 8), (192, 16), (193, 16)):
            assert ("rows", B, F, K, H3, 2) in have
    for K in (8, 16, 32, 5, 64):
        assert any(c.group == "head" and c.K == K and c.output_dim == 1 for c in lc.CASES)
    for L in (1, 2, 4):
        for F in (5, 13, 39):
            assert any(c.group == "depth" and c.L == L and c.F == F for c in lc.CASES)


def test_jt_and_the_dz2_b_rule():
    """cin_jt_sym's classes of the F sweep, and cin_launch_dz2_b's rule on both sides of its two edges (F = 11|12, 19|20)."""
    assert [lc.jt_sym(F) for F in (2, 7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 41, 42, 47, 48)] == [2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 12, 12, 14]
    assert [lc.dz2_b_accepts(F) for F in (2, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 31, 32, 39, 40, 41, 42, 47)] == \
        [False, False, False, False, True, True, False, False, True, True, True, True, True, True, True, True, True, True]
    by = {(c.F, c.H): c for c in lc.CASES if c.group == "F"}
    assert not by[(11, (128,) * 3)].dz2_b and by[(12, (128,) * 3)].dz2_b and not by[(19, (128,) * 3)].dz2_b and by[(20, (128,) * 3)].dz2_b
    assert not by[(42, (128,) * 3)].dz2_b and by[(47, (128, 130, 8))].dz2_b


@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_precision_column(case):
    """What the library says a bf16 call at TAIL_ALWAYS runs (a host-only call) is what the table says."""
    from ml_function_amd import functional as Fn
    assert Fn.cin_precision_used(case.B, case.F, case.K, list(case.H), mode=lc.TAIL_ALWAYS, precision="bf16") == case.prec
    if case.L != 3:
        assert case.prec == "f32"


def _peak(v):
    return float(np.max(np.abs(v), initial=0.0))


@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_case_conditions(case):
    od = case.output_dim
    assert set(case.exempt) <= set(lc.HEAD_TENSORS) and (od == 1 or not case.exempt)
    cover_w1s = cover_ts = None
    nonzero = {}
    for seed in case.seeds:
        c = lc.build(case, seed)
        # the lattice itself
        assert set(np.unique(c["x"])) <= {-1.0, 0.0, 1.0} and set(np.unique(c["dense_w"])) <= {-1.0, 1.0}
        assert set(np.unique(np.abs(c["g"]))) <= {1.0, 2.0} and c["g"].shape == ((case.B, 1) if od == 1 else (case.B, case.L * case.K))
        for W, b in zip(c["Ws"], c["bs"]):
            assert set(np.unique(W)) <= {-1.0, 0.0, 1.0} and np.all(b == np.round(b)) and _peak(b) <= 2
            assert W.any(0).all(), "an empty weight column"
        xr = lc.rows_of(c["x"])
        for lo in range(0, case.M, 32):
            assert xr[lo:lo + 32].any(0).all(), "a field that is zero in the whole row block at %d" % lo
        # operands of the one-plane kernels: bf16 numbers
        if case.L == 3:
            ops = lc.operands(c, od)
            for fam in lc.OPERAND_FAMILIES:
                assert lc.is_bf16(ops[fam]), "seed %d: %s holds values that are no bf16 numbers (max |v| = %g)" % (seed, fam, _peak(ops[fam]))
            w, t = ops["W1s"].any(2), ops["Ts"].any(2)
            cover_w1s = w if cover_w1s is None else cover_w1s | w
            cover_ts = t if cover_ts is None else cover_ts | t
        # every partial sum of every order is exact in fp32
        limit = lc.HALF_BELOW if case.F % 2 == 0 else lc.EXACT_BELOW
        over = tuple(n for n, v in lc.flat(lc.abs_bound(c, od)) if _peak(v) >= (lc.EXACT_BELOW if n in lc.HEAD_TENSORS and od == 1 else limit))
        assert set(over) <= set(case.exempt), "seed %d: %s reach the exactness bound" % (seed, over)
        if seed == case.seeds[0]:
            assert over == case.exempt, "the table exempts %s, the bound asks for %s" % (case.exempt, over)
        for n, v in lc.flat(lc.rows_oracle(c, od)):
            nz = np.asarray(v) != 0
            nonzero[n] = nz if n not in nonzero else nonzero[n] | nz
    if case.L == 3:
        assert cover_w1s.all() and cover_ts.all(), "pair slots that are zero in every column: W1s %d, Ts %d" % ((~cover_w1s).sum(), (~cover_ts).sum())
    for n, nz in nonzero.items():
        if n != "out":
            assert nz.mean() >= 0.95, "%s: only %.1f %% of the entries are nonzero" % (n, 100 * nz.mean())


def test_head_cases_exact_in_full():
    """At least one Dense(1) case per K class -- head folded into the forward's epilogue (K a power of two <= 32) or its own kernel -- and
    every pooled-output case compare every tensor bit for bit."""
    folded = lambda K: K <= 32 and K & (K - 1) == 0
    heads = [c for c in lc.CASES if c.output_dim == 1]
    assert any(folded(c.K) and not c.exempt for c in heads) and any(not folded(c.K) and not c.exempt for c in heads)
    assert all(not c.exempt for c in lc.CASES if c.output_dim == 2)


SMALL = [(5, 6, 4, (7, 5, 6), 1), (4, 9, 3, (10, 3, 4), 2), (3, 4, 2, (3, 3, 3, 3), 1)]


@pytest.mark.parametrize("B,F,K,H,od", SMALL)
def test_closed_graph_and_rows_oracles_agree_exactly(B, F, K, H, od):
    """oracle/closed.py == oracle/graph.py under autograd == rows_oracle in float64, exactly: on the lattice every fp64 sum is exact, so
    the three restatements may not differ in a single bit.  Also pins operands(): db_1 = sum_m G1 and dW_1 = Z^T G1."""
    c = lc.lattice_case(B, F, K, H, od, seed=5)
    out = closed.cin_fwd(c["x"], c["Ws"], c["bs"], c["dense_w"], c["dense_b"], od)
    dx, dWs, dbs, ddw, ddb = closed.cin_bwd(c["x"], c["Ws"], c["bs"], c["dense_w"], c["g"], od)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).requires_grad_()
    x, Ws, bs, dw, db = T(c["x"]), [T(w) for w in c["Ws"]], [T(b) for b in c["bs"]], T(c["dense_w"]), T(c["dense_b"])
    o = graph.cin(x, Ws, bs, dw, db, output_dim=od)
    o.backward(torch.tensor(c["g"], dtype=torch.float64))
    r = lc.rows_oracle(c, od)
    N = lambda t: t.detach().numpy()
    assert np.array_equal(out, N(o)) and np.array_equal(out, r["out"])
    assert np.array_equal(dx, N(x.grad)) and np.array_equal(dx, r["dx"])
    for l in range(len(H)):
        assert np.array_equal(dWs[l], N(Ws[l].grad)) and np.array_equal(dWs[l], r["dW"][l])
        assert np.array_equal(dbs[l], N(bs[l].grad)) and np.array_equal(dbs[l], r["db"][l])
    if od == 1:
        assert np.array_equal(ddw, N(dw.grad)) and np.array_equal(ddw, r["ddw"])
        assert np.array_equal(ddb, N(db.grad)) and np.array_equal(ddb, r["ddb"])
    if len(H) == 3:
        ops = lc.operands(c, od)
        Z = (ops["xe"][:, :, None] * ops["xe"][:, None, :]).reshape(B * K, F * F)
        assert np.array_equal(ops["G1"].sum(0), dbs[0]) and np.array_equal(Z.T @ ops["G1"], dWs[0])
        # the pair form of the first layer and of the quadratic form: x1 = P W1s + b_1, R = P Ts
        assert np.array_equal(np.einsum("mhd,hdn->mn", ops["P"], ops["W1s"]) + c["bs"][0], ops["x1"])
        assert np.array_equal(np.einsum("mhd,hdn->mn", ops["P"], ops["Ts"]), ops["R"])
