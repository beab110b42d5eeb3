"""Every CIN path against the fp64 oracle BIT FOR BIT, element for element, on the integer-lattice cases of tests/cin_lattice_cases.py.

On those cases every fp32 sum is exact in any order and every value the bf16 kernels round is already a bf16 number
(tests/test_cin_lattice_host.py proves both for every case), so the exact kernels, the split-bf16 kernels (FIL_CIN_BF16X3) and the
one-plane bf16 kernels (FIL_CIN_PREC_BF16) all have to return the oracle's value in every element of every output and gradient: a
dropped row, a lost weight tile, a wrong pair slot or a padded column that leaks shows as a wrong integer, however small its share
of the tensor's norm.  Equality is torch.equal(got.cpu().double(), oracle): -0 equals +0.  The only tensors held to the project's
1e-5 bar instead are the head tensors a Dense(1) case records as exempt (their sums pass 2^24).

All results being equal, bits cannot show which kernels ran: the case table says what fil_cin_precision_used must answer, and the
tests assert it (the host file checks the whole column).  What the lattice cannot see -- the rounding mode of the one-plane kernels --
is test_bf16_rounds_its_direct_operands_to_nearest_even, on ordinary inputs.

What these tests see was checked with value-only mutants of the split kernels, each built and run once (MI355X): the last row of the
last split of cin_dwq_b_kernel dropped; the last weight tile of cin_qs_pack_wz_body zeroed; cin_sym_weight without its 0.5; pass 1 of
cin_dz2_b_kernel unscaled in the last wave of a workgroup -- each fails the bf16 and the BF16X3 run of test 1 at every shape that reaches the
mutated code (28 to 56 cases each) and no run of an exact path; split_planes<1> truncating instead of rounding passes every lattice test, as it
must, and fails test 3 at 7e-3 against the 1e-5 bar.

Oracle: oracle/closed.py on the CPU for the small cases; the op-for-op graph in float64 on the GPU (tests.test_gpu_parity.
_graph_oracle_cin, exact on integers) where the closed form's einsum would take seconds (M F > 2048).
"""
import numpy as np
import pytest
import torch

from ml_function_amd import synth
from oracle import closed
from tests import cin_lattice_cases as lc

pytestmark = pytest.mark.gpu

TOL = 1e-5                 # tests/test_gpu_parity.py's bar, for the exempt head tensors only
T = lc.TAIL_ALWAYS
# (name, mode, precision, three-layer nets only, row sweep only)
PATHS = [("bf16", T, "bf16", True, False), ("bf16x3", T | 2, "f32", True, False),
         ("qtail", T, "f32", False, False), ("noqmerge", T | 512, "f32", False, False), ("noqtail", T | 256, "f32", False, False),
         ("default", 0, "f32", False, False), ("general", 1, "f32", False, False), ("nosym", 8, "f32", False, False),
         ("notail", 32, "f32", False, False),
         ("mb2", T | 4, "f32", False, True), ("noksplit", T | 128, "f32", False, True)]
RUNS = [(c, p) for c in lc.CASES for p in PATHS if (c.L == 3 or not p[3]) and (c.group == "rows" or not p[4])]


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def run(c, output_dim, mode, precision="f32", g=None):
    from ml_function_amd import functional as Fn
    x = dev(c["x"]).requires_grad_()
    Ws = [dev(w).requires_grad_() for w in c["Ws"]]
    bs = [dev(b).requires_grad_() for b in c["bs"]]
    dw, db = (dev(c["dense_w"]).requires_grad_(), dev(c["dense_b"]).requires_grad_()) if output_dim == 1 else (None, None)
    out = Fn.cin(x, Ws, bs, dw, db, output_dim=output_dim, mode=mode, precision=precision)
    out.backward(dev(c["g"] if g is None else g))
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, dW=[w.grad for w in Ws], db=[b.grad for b in bs],
                ddw=dw.grad if dw is not None else None, ddb=db.grad if db is not None else None)


_ORACLE = {}     # (case id, seed) -> oracle, for the case the tests are at (the runs are ordered by case)


def oracle(case, seed):
    key = (case.id, seed)
    if key not in _ORACLE:
        for k in [k for k in _ORACLE if k[0] != case.id]:
            del _ORACLE[k]
        c = lc.build(case, seed)
        if case.M * case.F <= 2048:
            out = closed.cin_fwd(c["x"], c["Ws"], c["bs"], c["dense_w"], c["dense_b"], case.output_dim)
            dx, dWs, dbs, ddw, ddb = closed.cin_bwd(c["x"], c["Ws"], c["bs"], c["dense_w"], c["g"], case.output_dim)
            res = dict(out=out, dx=dx, dW=dWs, db=dbs, ddw=ddw, ddb=ddb)
        else:
            from tests.test_gpu_parity import _graph_oracle_cin
            res = _graph_oracle_cin(c, case.output_dim)
        _ORACLE[key] = {n: torch.tensor(np.asarray(v, np.float64)) for n, v in lc.flat(res)}
    return _ORACLE[key]


def mismatches(got, want, exempt=()):
    """[(tensor, what)] for every tensor of a run that is not the oracle's, element for element (the exempt ones: beyond TOL)."""
    bad = []
    for n, v in lc.flat(got):
        a, b = v.detach().cpu().double().reshape(want[n].shape), want[n]
        if n in exempt:
            e = float((a - b).abs().max() / b.abs().max())
            if not e <= TOL:
                bad.append((n, "max-rel %.2e > %.0e" % (e, TOL)))
        elif not torch.equal(a, b):
            d = (a != b) | ~torch.isfinite(a)
            i = tuple(int(t) for t in d.nonzero()[0])
            bad.append((n, "%d of %d elements differ, first at %s: got %r, oracle %r" % (int(d.sum()), d.numel(), i, float(a[i]), float(b[i]))))
    return bad


def same(a, b):
    return all(torch.equal(u, v) for (_, u), (_, v) in zip(lc.flat(a), lc.flat(b)))


# ------------------------------------------------------------------------------------------------ 1. every case on every path
@pytest.mark.parametrize("case,path", RUNS, ids=["%s-%s" % (c.id, p[0]) for c, p in RUNS])
def test_path_equals_the_oracle_bit_for_bit(case, path):
    from ml_function_amd import functional as Fn
    name, mode, precision = path[:3]
    if name == "bf16":      # the predicate is the proof that the one-plane kernels ran (or, for an "f32" row of the table, did not)
        assert Fn.cin_precision_used(case.B, case.F, case.K, list(case.H), mode=mode, precision="bf16") == case.prec
    for seed in case.seeds:
        c = lc.build(case, seed)
        got = run(c, case.output_dim, mode, precision)
        bad = mismatches(got, oracle(case, seed), case.exempt)
        assert not bad, "%s seed %d mode %d precision %s: %s" % (case.id, seed, mode, precision, bad)
        if name == "bf16" and case.prec == "f32":      # the fall-back runs the same kernels as the exact call
            assert same(got, run(c, case.output_dim, mode, "f32"))


# ------------------------------------------------------------------------------------------------ 2. one plane against three
@pytest.mark.parametrize("case", [c for c in lc.CASES if c.L == 3], ids=[c.id for c in lc.CASES if c.L == 3])
def test_one_plane_equals_three_planes(case):
    """precision="bf16" against BF16X3 on the same inputs: on bf16-exact operands the split's five further MFMAs add products of zero
    pieces, so every output and gradient is the same in every bit (the exempt head tensors too: same kernels, same order)."""
    for seed in case.seeds:
        c = lc.build(case, seed)
        one, three = run(c, case.output_dim, T, "bf16"), run(c, case.output_dim, T | 2, "f32")
        diff = [n for (n, u), (_, v) in zip(lc.flat(one), lc.flat(three)) if not torch.equal(u, v)]
        assert not diff, "%s seed %d: bf16 and BF16X3 differ in %s" % (case.id, seed, diff)


# ------------------------------------------------------------------------------------------------ 3. the rounding rule
@pytest.mark.parametrize("F", [12, 20, 39, 41])
def test_bf16_rounds_its_direct_operands_to_nearest_even(F):
    """Ordinary inputs (x = 10 x synth's, glorot weights, pooled output), mode TAIL_ALWAYS, bf16: the first pooled block,
    out[:, 0:K] = sum_h x1[m,h], against a restatement that rounds exactly what the forward rounds of it -- P = fp32(x_h) fp32(x_f)
    and the pair weights W1s (cin_sym_weight's rule in fp32), each to the nearest bf16, ties to even -- and multiplies and sums in
    float64, plus the bias.  What is left is fp32 accumulation over at most 861 products, which the exact kernels do at the same
    1e-5 norm-relative bar; truncation instead of rounding is off by ~2^-9 per operand.  The unrounded oracle must be more than 1e-4
    away, so the test does tell the two references apart.  (T and G1 are fp32 results before they are rounded: a value next to a bf16
    tie would make their restatement ambiguous, so the check stops at block 0.)"""
    from ml_function_amd import functional as Fn
    B, K, H = 24, 8, [128, 128, 128]
    assert Fn.cin_precision_used(B, F, K, H, mode=T, precision="bf16") == "bf16"
    c = synth.cin_case(B, F, K, H, output_dim=2)
    c["x"] = (c["x"] * 10).astype(np.float32)
    got = run(c, 2, T, "bf16")["out"][:, :K].cpu().double().numpy()
    xr = c["x"].transpose(0, 2, 1).reshape(B * K, F)                                   # float32 rows
    W3 = c["Ws"][0].reshape(F, F, -1)
    want = np.zeros((B * K, H[0]))
    exact = np.zeros((B * K, H[0]))
    for h in range(F):
        for d in range(F // 2 + 1):
            f = (h + d) % F
            w = W3[h, h] if d == 0 else (W3[h, f] + W3[f, h]) * np.float32(0.5 if 2 * d == F else 1.0)      # float32, as the kernel
            p = xr[:, h] * xr[:, f]                                                                      # float32 product
            want += lc.to_bf16(p).astype(np.float64)[:, None] * lc.to_bf16(w).astype(np.float64)[None, :]
            exact += p.astype(np.float64)[:, None] * w.astype(np.float64)[None, :]
    want = (want + c["bs"][0].astype(np.float64)).sum(1).reshape(B, K)
    exact = (exact + c["bs"][0].astype(np.float64)).sum(1).reshape(B, K)
    nrel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    e_round, e_exact = nrel(got, want), nrel(got, exact)
    print("F=%d: pooled block 0 against the bf16-rounded restatement %.2e, against the unrounded one %.2e" % (F, e_round, e_exact))
    assert e_exact > 1e-4
    assert e_round <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. linearity in g
LINEAR = [c for c in lc.CASES if c.id in ("F-B17-F39-K8-H128x128x128-od2", "head-B6-F12-K8-H128x128x128-od1")]


@pytest.mark.parametrize("case", LINEAR, ids=[c.id for c in LINEAR])
@pytest.mark.parametrize("mode,precision", [(T, "f32"), (T, "bf16"), (0, "f32")])
def test_gradients_are_linear_in_g(case, mode, precision):
    """2 g doubles every gradient bit for bit (doubling keeps the lattice and every bound with room to spare) and leaves the output
    alone: a gradient that depended on a buffer of the call before, or on anything but g linearly, would not."""
    c = lc.build(case, case.seeds[0])
    one = run(c, case.output_dim, mode, precision)
    two = run(c, case.output_dim, mode, precision, g=2 * c["g"])
    assert torch.equal(one["out"], two["out"])
    for (n, u), (_, v) in zip(lc.flat(one)[1:], lc.flat(two)[1:]):
        assert torch.equal(2 * u, v), n
    assert not mismatches(one, oracle(case, case.seeds[0]), case.exempt)
