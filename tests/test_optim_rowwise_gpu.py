"""Keras' Adagrad and Ftrl on the GPU (include/fil.h O2, ml_function_amd/optim.py): fil_rowopt_multi against float64 restatements of
TF 2.1's ApplyAdagradV2 / ApplyFtrl(V2), the runs tables against Keras' per-field semantics (bitwise where Keras leaves a row alone),
torch's Adagrad as an independent cross-check, the data-parallel merged update, HIP-graph capture, state_dict / reset_, a whole XDeepFM
step against the float64 oracle graph, and a short training run."""
import copy
import os

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, models, optim
from ml_function_amd._lib import RowoptHyper, check, ptr, stream_ptr
from ml_function_amd.layers import SparseEmbed
from ml_function_amd.layers.base import collect_regularization_loss
from oracle import graph

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
ADAGRAD, FTRL = _lib.FIL_OPT_ADAGRAD, _lib.FIL_OPT_FTRL


def f32(x):
    """Keras' hyper-parameters are float32 variables: the float64 reference takes their float32 values."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------ float64 restatement of TF 2.1's functors
def adagrad64(p, g, acc, h):
    acc = acc + g * g
    return p - g * h["lr"] / (np.sqrt(acc) + h["eps"]), acc


def _pw(h):
    return (lambda x: np.sqrt(x)) if h["lr_power"] == -0.5 else (lambda x: np.power(x, -h["lr_power"]))


def ftrl64(p, g, n, z, h):
    """ApplyFtrl (ApplyFtrlV2 when l2_shrinkage > 0) in float64.  Returns (p, n, z)."""
    gs = g + 2 * h["shrink"] * p if h["shrink"] > 0 else g
    n1 = n + g * g
    a = _pw(h)
    z = z + gs - (a(n1) - a(n)) / h["lr"] * p
    q = a(n1) / h["lr"] + 2 * h["l2"]
    return np.where(np.abs(z) > h["l1"], (np.sign(z) * h["l1"] - z) / q, 0.0), n1, z


def hyper(rule, lr=1e-3, eps=1e-7, lr_power=-0.5, l1=0.0, l2=0.0, shrink=0.0):
    return dict(rule=rule, lr=f32(lr), eps=f32(eps), lr_power=f32(lr_power), l1=f32(l1), l2=f32(l2), shrink=f32(shrink))


def make_opt(params, h, **kw):
    if h["rule"] == ADAGRAD:
        return optim.Adagrad(params, learning_rate=h["lr"], epsilon=h["eps"], **kw)
    return optim.Ftrl(params, learning_rate=h["lr"], learning_rate_power=h["lr_power"], l1_regularization_strength=h["l1"],
                      l2_regularization_strength=h["l2"], l2_shrinkage_regularization_strength=h["shrink"], **kw)


def c_hyper(h):
    return RowoptHyper(h["lr"], h["eps"], h["lr_power"], h["l1"], h["l2"], h["shrink"])


def check_step(h, got, old, g, where="", g_err=0.0):
    """One step of the rule from the float32 state `old` (p, acc[, z]) with the float64 gradient g, element by element against the
    float64 rule, within a bound on fp32 rounding of each operation (a formula slip is orders of magnitude outside it).  g_err bounds
    the error of the gradient the kernel formed itself (an fp32 run sum, the l2 term).  Ftrl: p is compared outside the band |z| ~ l1
    (fp32 and fp64 may land on different sides there); outside it the exact zeros must match."""
    g_err = np.broadcast_to(g_err, np.shape(g))
    if h["rule"] == ADAGRAD:
        p0, a0 = old
        want_p, want_a = adagrad64(p0, g, a0, h)
        p, a = got
        tol_a = 4 * EPS32 * want_a + 2 * np.abs(g) * g_err + g_err * g_err
        assert np.all(np.abs(a - want_a) <= tol_a), (where, (np.abs(a - want_a) / tol_a).max())
        d = np.sqrt(want_a) + h["eps"]
        step = np.abs(g * h["lr"] / d)
        tol_p = 8 * EPS32 * (np.abs(p0) + step) + h["lr"] * g_err / d + step * tol_a / (2 * np.sqrt(want_a) * d)
        assert np.all(np.abs(p - want_p) <= tol_p), (where, (np.abs(p - want_p) / tol_p).max())
        return
    p0, n0, z0 = old
    want_p, want_n, want_z = ftrl64(p0, g, n0, z0, h)
    p, n, z = got
    tol_n = 4 * EPS32 * want_n + 2 * np.abs(g) * g_err + g_err * g_err
    assert np.all(np.abs(n - want_n) <= tol_n), (where, (np.abs(n - want_n) / tol_n).max())
    a = _pw(h)
    da = -h["lr_power"] * np.power(want_n, -h["lr_power"] - 1) * tol_n        # a(n') moves this much with n' inside tol_n
    gs = g + 2 * h["shrink"] * p0 if h["shrink"] > 0 else g
    tol_z = (16 * EPS32 * (np.abs(z0) + np.abs(gs) + (a(want_n) + a(n0)) / h["lr"] * np.abs(p0)) + g_err + da / h["lr"] * np.abs(p0)
             + 1e-30)
    assert np.all(np.abs(z - want_z) <= tol_z), (where, (np.abs(z - want_z) / tol_z).max())
    q = a(want_n) / h["lr"] + 2 * h["l2"]
    out = np.abs(np.abs(want_z) - h["l1"]) > tol_z
    tol_p = (tol_z + 16 * EPS32 * (h["l1"] + np.abs(want_z))) / q + (16 * EPS32 + da / h["lr"] / q) * np.abs(want_p)
    assert np.all(np.abs(p - want_p)[out] <= tol_p[out]), (where, (np.abs(p - want_p)[out] / tol_p[out]).max())
    assert np.array_equal((p == 0)[out], (np.abs(want_z) <= h["l1"])[out]), where


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def c64(t):
    return t.detach().cpu().double().numpy()


FTRL_CASES = [(pw, l1, l2, s) for pw in (-0.5, -0.3) for l1 in (0.0, 1e-3) for l2 in (0.0, 1e-2) for s in (0.0, 1e-2)]
CASES = [hyper(ADAGRAD)] + [hyper(FTRL, lr=1e-2, lr_power=pw, l1=l1, l2=l2, shrink=s) for pw, l1, l2, s in FTRL_CASES]
CASE_IDS = ["adagrad"] + ["ftrl_p%g_l1%g_l2%g_s%g" % c for c in FTRL_CASES]


# ---------------------------------------------------------------------------------------------------- 1. dense tensors, one launch
SIZES = [(1,), (3,), (4,), (1023,), (4096,), (65537,), (1521, 128)]
NONE, WITH_L2, DESC_L2 = 2, 4, 3e-2          # tensor 2 has no gradient (grad NULL); tensor 4 carries a descriptor l2


@pytest.mark.parametrize("h", CASES, ids=CASE_IDS)
def test_rowopt_multi_matches_float64(h):
    """5 steps of fil_rowopt_multi over 7 tensors of awkward sizes, one with no gradient and one with l2: every step element by element
    against the float64 rule from the same state, and the whole trajectory against a float64 one."""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    ftrl = h["rule"] == FTRL
    ps = [torch.tensor(rng.standard_normal(s) * 0.5, dtype=torch.float32, device="cuda") for s in SIZES]
    acc = [torch.full(s, f32(0.1), device="cuda") for s in SIZES]
    lin = [torch.zeros(s, device="cuda") for s in SIZES] if ftrl else [None] * len(SIZES)
    gs = [torch.empty(s, device="cuda") for s in SIZES]
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    descs = (optim._Desc * len(SIZES))(*[optim._Desc(p.data_ptr(), None if i == NONE else g.data_ptr(), a.data_ptr(), ptr(z),
                                                     p.numel(), DESC_L2 if i == WITH_L2 else 0.0, 0)
                                         for i, (p, g, a, z) in enumerate(zip(ps, gs, acc, lin))])
    d = torch.frombuffer(bytearray(descs), dtype=torch.uint8).cuda()
    total = sum(p.numel() for p in ps)
    ch = c_hyper(h)
    traj = [(c64(p), c64(a), c64(z) if ftrl else None) for p, a, z in zip(ps, acc, lin)]
    lo = -2 if ftrl else -6                 # (Ftrl's sigma is a difference of square roots: fp32 cancels for g^2 << n)
    for t in range(1, 6):
        grads = [rng.standard_normal(s) * 10.0 ** rng.integers(lo, 0) for s in SIZES]
        for g, gn in zip(gs, grads):
            g.copy_(torch.tensor(gn, dtype=torch.float32))
        before = [(c64(p), c64(a)) + ((c64(z),) if ftrl else ()) for p, a, z in zip(ps, acc, lin)]
        check(lib.fil_rowopt_multi(ptr(d), len(SIZES), total, ptr(step), h["rule"], ctypes_addr(ch), 1, stream_ptr()), "fil_rowopt_multi")
        torch.cuda.synchronize()
        assert int(step) == t
        for i in range(len(SIZES)):
            g64 = np.zeros(SIZES[i]) if i == NONE else c64(gs[i])
            if i == WITH_L2:
                g64 = g64 + 2 * f32(DESC_L2) * before[i][0]
            got = (c64(ps[i]), c64(acc[i])) + ((c64(lin[i]),) if ftrl else ())
            check_step(h, got, before[i], g64, where=(SIZES[i], t), g_err=2 * EPS32 * np.abs(g64) if i == WITH_L2 else 0.0)
            gt = np.zeros(SIZES[i]) if i == NONE else c64(gs[i])
            if i == WITH_L2:
                gt = gt + 2 * f32(DESC_L2) * traj[i][0]
            if ftrl:
                traj[i] = ftrl64(traj[i][0], gt, traj[i][1], traj[i][2], h)
                band = np.abs(np.abs(traj[i][2]) - h["l1"]) <= 1e-3 * np.maximum(np.abs(traj[i][2]), 1e-6)
                assert nrel(got[0][~band], traj[i][0][~band]) < 2e-3, (SIZES[i], t)
            else:
                traj[i] = adagrad64(traj[i][0], gt, traj[i][1], h) + (None,)
                assert nrel(got[0], traj[i][0]) < 1e-6, (SIZES[i], t)
    if not ftrl:            # Adagrad with a zero gradient leaves the tensor and its accumulator bit for bit
        assert torch.all(acc[NONE] == f32(0.1))


def ctypes_addr(s):
    import ctypes
    return ctypes.addressof(s)


# ---------------------------------------------------------------------------------------------------- 2. the tables, in place
VOCAB = [50, 200, 30, 1000, 7, 64]
L2 = {0: 1e-2, 3: 3e-3}              # two regularised fields
FROZEN = 2                           # one frozen field
K, BT = 16, 512
TABLE_CASES = [hyper(ADAGRAD, lr=1e-2), hyper(FTRL, lr=1e-2, l1=1e-3, l2=1e-3, shrink=1e-3)]
TABLE_IDS = ["adagrad", "ftrl"]


def _table_layer(out_dtype, l2=True):
    info = models.make_sparse_info(VOCAB, embed_dim=K)
    info = [i._replace(emb_reg=L2.get(f, 0.0) if l2 else 0.0, is_trainable=(f != FROZEN)) for f, i in enumerate(info)]
    torch.manual_seed(3)
    return SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs", out_dtype=out_dtype)


def _table_batches(steps, seed, B=BT):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        idx = np.stack([np.minimum(rng.zipf(1.2, B) - 1, v - 1) for v in VOCAB], 1)          # heavy duplication
        bad = rng.random(idx.shape) < 0.02                                                  # out-of-range ids (dropped)
        idx[bad] = np.array(VOCAB)[np.nonzero(bad)[1]] + 3
        idx[rng.random(idx.shape) < 0.01] = -1
        g = rng.standard_normal((B, len(VOCAB), K)) * 0.1
        out.append((idx, g))
    return out


def _dense_grad64(idx, g, offs, p64, l2=True):
    """The table gradient of the reference's autograd, float64: the rows' gradients summed, + 2 l2 p on the regularised fields.
    Also a bound on the error of the kernel's fp32 version: (terms + 1) eps times the sum of the terms' magnitudes."""
    G, A, C = np.zeros_like(p64), np.zeros_like(p64), np.zeros(p64.shape[0])
    for f, v in enumerate(VOCAB):
        if f == FROZEN:
            continue
        ok = (idx[:, f] >= 0) & (idx[:, f] < v)
        np.add.at(G, offs[f] + idx[ok, f], g[ok, f])
        np.add.at(A, offs[f] + idx[ok, f], np.abs(g[ok, f]))
        np.add.at(C, offs[f] + idx[ok, f], 1)
    if l2:
        for f, lam in L2.items():
            r = slice(offs[f], offs[f] + VOCAB[f])
            G[r] += 2 * f32(lam) * p64[r]
            A[r] += 2 * f32(lam) * np.abs(p64[r])
            C[r] += 1
    return G, (C[:, None] + 1) * EPS32 * A


def _touched(idx, offs):
    rows = set()
    for f, v in enumerate(VOCAB):
        if f != FROZEN:
            rows.update((offs[f] + i) for i in idx[:, f] if 0 <= i < v)
    return np.array(sorted(rows))


def _slots(opt, p):
    st = opt.state[p]
    return (st["accumulator"],) + ((st["linear"],) if "linear" in st else ())


def _run_table(h, out_dtype, batches, check_each, l2=True, **kw):
    emb = _table_layer(out_dtype, l2)
    emb(torch.tensor(batches[0][0], device="cuda"))                     # build
    p = emb.embeddings
    opt = make_opt([p], h, **kw)
    offs = emb.offsets.cpu().numpy()
    V = p.shape[0]
    frozen_rows = np.arange(offs[FROZEN], offs[FROZEN] + VOCAB[FROZEN])
    l2_rows = np.concatenate([np.arange(offs[f], offs[f] + VOCAB[f]) for f in L2]) if l2 else np.zeros(0, np.int64)
    for t, (idx, g) in enumerate(batches, 1):
        opt.zero_grad()
        block = emb(torch.tensor(idx, device="cuda"))
        gt = torch.tensor(g, dtype=block.dtype, device="cuda")
        block.backward(gt)
        assert p.grad is None and p._fil_pending_runs is not None
        old = (c64(p),) + (tuple(c64(s) for s in _slots(opt, p)) if p in opt.state else
                           (np.full(p.shape, f32(0.1)),) + ((np.zeros(p.shape),) if h["rule"] == FTRL else ()))
        opt.step()
        assert p._fil_pending_runs is None
        if not check_each:
            continue
        got = (c64(p),) + tuple(c64(s) for s in _slots(opt, p))
        G, Gerr = _dense_grad64(idx, c64(gt), offs, old[0], l2)
        touched = _touched(idx, offs)
        rows = np.union1d(touched, l2_rows)                 # Keras updates these (IndexedSlices rows + dense regulariser fields)
        check_step(h, tuple(x[rows] for x in got), tuple(x[rows] for x in old), G[rows], where=t, g_err=Gerr[rows])
        # everything else keeps its bits, slots included: untouched rows of unregularised fields, and the frozen field
        keep = np.setdiff1d(np.arange(V), rows)
        assert np.intersect1d(keep, frozen_rows).size == frozen_rows.size and np.setdiff1d(keep, frozen_rows).size > 0
        for a, b in zip(got, old):
            assert np.array_equal(a[keep], b[keep]), t
        untouched_l2 = np.setdiff1d(l2_rows, touched)
        if l2:
            assert untouched_l2.size > 0
            if h["rule"] == ADAGRAD or t == 1:          # the regulariser moves them (Ftrl: then they sit at ~0, often exactly)
                live_rows = untouched_l2[(old[0][untouched_l2] != 0).any(axis=1)]
                assert live_rows.size > 0 and (got[0][live_rows] != old[0][live_rows]).any(axis=1).all()
            if h["rule"] == FTRL and t == 1:
                # Keras' first-step collapse: p -> about -lr 2 emb_reg p / sqrt(n), in effect 0 (the initial weights are gone)
                lam = np.zeros(V)
                for f, v in L2.items():
                    lam[offs[f]:offs[f] + VOCAB[f]] = f32(v)
                u = untouched_l2
                bound = 1.01 * h["lr"] * 2 * lam[u, None] * np.abs(old[0][u]) / np.sqrt(f32(0.1)) + 1e-30
                assert np.all(np.abs(got[0][u]) <= bound)
                assert np.abs(got[0][u]).max() < 1e-3 * np.abs(old[0][u]).max()
    assert opt.iterations == len(batches)
    return (p.detach().clone(),) + tuple(s.clone() for s in _slots(opt, p))


@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("h", TABLE_CASES, ids=TABLE_IDS)
def test_runs_table_matches_keras_semantics(h, out_dtype):
    batches = _table_batches(3, seed=11)
    a = _run_table(h, out_dtype, batches, check_each=True)
    b = _run_table(h, out_dtype, batches, check_each=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))           # run 2 bitwise equal to run 1


@pytest.mark.parametrize("h", TABLE_CASES, ids=TABLE_IDS)
def test_runs_table_without_regularised_fields_has_no_stamps(h):
    batches = _table_batches(2, seed=13)
    emb = _table_layer(None, l2=False)
    _run_table(h, None, batches, check_each=True, l2=False)
    emb(torch.tensor(batches[0][0], device="cuda"))
    opt = make_opt([emb.embeddings], h)
    opt.zero_grad()
    emb(torch.tensor(batches[0][0], device="cuda")).sum().backward()
    opt.step()
    assert not opt._stamps                          # stamps only for tables with a regularised field


@pytest.mark.parametrize("cls", ["Adagrad", "Ftrl"])
def test_second_pending_record_raises_and_zero_grad_clears(cls):
    emb = _table_layer(None)
    idx = torch.tensor(_table_batches(1, seed=3)[0][0], device="cuda")
    emb(idx).sum().backward()
    with pytest.raises(Exception, match="pending"):
        emb(idx).sum().backward()
    opt = getattr(optim, cls)([emb.embeddings])
    opt.zero_grad()
    assert emb.embeddings._fil_pending_runs is None
    emb(idx).sum().backward()
    emb.embeddings.grad = torch.zeros_like(emb.embeddings)
    with pytest.raises(_lib.FilError, match="both a .grad and a pending"):
        opt.step()
    emb.embeddings.grad = None
    opt.step()
    assert opt.iterations == 1


@pytest.mark.parametrize("cls", ["Adagrad", "Ftrl"])
def test_refuses_sparse_gradients_and_adam_deferred_tables(cls):
    p = torch.nn.Parameter(torch.zeros(10, 4, device="cuda"))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]], device="cuda"), torch.ones(2, 4, device="cuda"), (10, 4))
    with pytest.raises(_lib.FilError, match="sparse"):
        getattr(optim, cls)([p]).step()
    emb = _table_layer(None)
    idx = torch.tensor(_table_batches(1, seed=5)[0][0], device="cuda")
    emb(idx)
    adam = optim.Adam([emb.embeddings], sweep_period=4)
    assert optim.deferred_state(emb.embeddings) is not None
    emb(idx).sum().backward()
    with pytest.raises(_lib.FilError, match="deferred"):
        getattr(optim, cls)([emb.embeddings]).step()
    del adam


# ---------------------------------------------------------------------------------------------------- 3. torch as a cross-check
def test_adagrad_agrees_with_torch_adagrad():
    """optim.Adagrad on dense parameters against torch.optim.Adagrad(lr, initial_accumulator_value=0.1, eps=1e-7), 5 steps: the
    same rule written independently, equal to rounding."""
    rng = np.random.default_rng(4)
    shapes = [(7,), (4096,), (333, 17)]
    a = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s), dtype=torch.float32, device="cuda")) for s in shapes]
    b = [torch.nn.Parameter(x.detach().clone()) for x in a]
    oa = optim.Adagrad(a, learning_rate=0.01)
    ob = torch.optim.Adagrad(b, lr=0.01, initial_accumulator_value=0.1, eps=1e-7)
    for _ in range(5):
        for x, y, s in zip(a, b, shapes):
            g = torch.tensor(rng.standard_normal(s) * 0.3, dtype=torch.float32, device="cuda")
            x.grad, y.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    for x, y in zip(a, b):
        assert nrel(c64(x), c64(y)) < 1e-6
        assert torch.allclose(oa.state[x]["accumulator"], ob.state[y]["sum"], rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------- 4. data parallelism
@pytest.mark.parametrize("l2", [True, False], ids=["l2", "nol2"])
@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("h", TABLE_CASES, ids=TABLE_IDS)
def test_w1_exchange_is_bitwise_the_one_gpu_update(h, out_dtype, l2):
    batches = [(idx, g) for s in range(3) for idx, g in _table_batches(1, seed=60 + s, B=512 - 64 * s)]
    runs = []
    for force in (False, True):
        emb = _table_layer(out_dtype, l2)
        emb(torch.tensor(batches[0][0], device="cuda"))
        opt = make_opt([emb.embeddings], h, force_exchange=force)
        traj = []
        for idx, g in batches:
            opt.zero_grad()
            block = emb(torch.tensor(idx, device="cuda"))
            block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
            opt.step()
            traj.append((emb.embeddings.detach().clone(),) + tuple(s.clone() for s in _slots(opt, emb.embeddings)))
        assert (emb.embeddings in opt._xbuf) == force
        runs.append(traj)
    for s, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


@pytest.mark.parametrize("cls", ["Adagrad", "Ftrl"])
def test_record_larger_than_the_agreed_capacity_raises(cls):
    emb = _table_layer(None)
    emb(torch.tensor(_table_batches(1, 1, B=64)[0][0], device="cuda"))
    opt = getattr(optim, cls)([emb.embeddings], force_exchange=True)
    for B in (64, 128):
        opt.zero_grad()
        idx, g = _table_batches(1, seed=B, B=B)[0]
        emb(torch.tensor(idx, device="cuda")).backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
        if B == 64:
            opt.step()
        else:
            with pytest.raises(_lib.FilError, match="capacity"):
                opt.step()


def _record(emb, idx, g):
    block = emb(torch.tensor(idx, device="cuda"))
    block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
    rec = emb.embeddings._fil_pending_runs
    emb.embeddings._fil_pending_runs = None
    return rec


def _gather(recs):
    W, cap = len(recs), max(r["R"] for r in recs)
    ids = torch.empty(W * cap, dtype=torch.int64, device="cuda")
    values = torch.empty(W * cap * K, dtype=torch.float32, device="cuda")
    counts = torch.empty(W, dtype=torch.int64, device="cuda")
    for w, rec in enumerate(recs):
        ws = torch.empty(max(1, optim.runs_compact_workspace_bytes(rec["R"])), dtype=torch.uint8, device="cuda")
        optim.runs_compact(rec, K, ids[w * cap:(w + 1) * cap], values[w * cap * K:(w + 1) * cap * K], counts[w:w + 1], cap, ws)
    return ids, values, counts, cap


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("h", TABLE_CASES, ids=TABLE_IDS)
def test_sharded_merged_update_matches_float64_full_batch(h, W):
    """W shards' compact lists gathered on one GPU, fil_embed_rowopt_merged + the sweep, against the float64 rule on the full
    batch's dense gradient (the rows Keras updates), and bitwise-unchanged rows elsewhere."""
    per = 256
    lib = _lib.load()
    emb = _table_layer(None)
    emb(torch.tensor(_table_batches(1, 0, B=8)[0][0], device="cuda"))
    offs = emb.offsets.cpu().numpy()
    p = emb.embeddings
    V = p.shape[0]
    ftrl = h["rule"] == FTRL
    acc = torch.full((V, K), f32(0.1), device="cuda")
    lin = torch.zeros((V, K), device="cuda") if ftrl else None
    stamp = torch.zeros(V, dtype=torch.int32, device="cuda")
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    ch = c_hyper(h)
    l2_rows = np.concatenate([np.arange(offs[f], offs[f] + VOCAB[f]) for f in L2])
    for step in (1, 2):
        idx, g = _table_batches(1, seed=100 * W + step, B=W * per)[0]
        shards = [_record(emb, idx[w * per:(w + 1) * per], g[w * per:(w + 1) * per]) for w in range(W)]
        ids, values, counts, cap = _gather(shards)
        old = (c64(p), c64(acc)) + ((c64(lin),) if ftrl else ())
        rec = shards[0]
        optim.rowopt_merged(h["rule"], ids, values, counts, W, cap, emb.offsets, rec["field_l2"], p, acc, lin, stamp, t, ch)
        check(lib.fil_embed_rowopt_sweep(ptr(p), ptr(acc), ptr(lin), ptr(stamp), V, K, ptr(rec["offsets"]), ptr(rec["field_l2"]),
                                         ptr(rec["frozen"]), rec["F"], ptr(t), h["rule"], ctypes_addr(ch), stream_ptr()),
              "fil_embed_rowopt_sweep")
        t += 1
        got = (c64(p), c64(acc)) + ((c64(lin),) if ftrl else ())
        G, Gerr = _dense_grad64(idx, c64(torch.tensor(g, dtype=torch.float32)), offs, old[0])
        rows = np.union1d(_touched(idx, offs), l2_rows)
        check_step(h, tuple(x[rows] for x in got), tuple(x[rows] for x in old), G[rows], where=(W, step), g_err=Gerr[rows])
        keep = np.setdiff1d(np.arange(V), rows)
        assert keep.size > 0
        for a, b in zip(got, old):
            assert np.array_equal(a[keep], b[keep])


def _ranks(n):
    from tests.test_dp_gpu import _run_ranks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return _run_ranks([os.path.join(root, "tests", "dp_rowwise_worker.py")], n, timeout=300)


def test_dp_rowwise_worker_on_one_rank():
    r = _ranks(1)
    assert r.returncode == 0 and "DP_ROWWISE_OK 1" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_dp_rowwise_worker_on_two_ranks():
    r = _ranks(2)
    assert r.returncode == 0 and "DP_ROWWISE_OK 2" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------- 5. HIP-graph capture
def _xdeepfm(vocab, K_, table_grad, emb_reg=1e-3):
    info = [i._replace(emb_reg=emb_reg) for i in models.make_sparse_info(vocab, embed_dim=K_)]
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad=table_grad)
    return fi, models.CTRModel(fi, models.XDeepFM(conv_size=[16, 12], hidden_units=[32, 16])).cuda()


def _inputs(B, n_dense, vocab, seed=0):
    rng = np.random.default_rng(seed)
    dense = torch.tensor(rng.random((B, n_dense)), dtype=torch.float32, device="cuda")
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device="cuda")
    return dense, idx


@pytest.mark.parametrize("emb_reg", [1e-3, 0.0], ids=["l2", "nol2"])
@pytest.mark.parametrize("h", [hyper(ADAGRAD, lr=1e-2), hyper(FTRL, lr=1e-2, l1=1e-3, l2=1e-3)], ids=TABLE_IDS)
def test_captured_step_replays_bitwise_like_eager(h, emb_reg):
    vocab = [7, 11, 5, 13, 3, 17]
    B, K_ = 256, 8
    batches = []
    rng = np.random.default_rng(5)
    for s in range(3):
        d, i = _inputs(B, 3, vocab, seed=40 + s)
        batches.append((d, i, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        torch.manual_seed(7)
        fi, model = _xdeepfm(vocab, K_, "runs", emb_reg)
        model(batches[0][0], batches[0][1])
        opt = make_opt(model.parameters(), h)

        def step(dense, idx, y):
            opt.zero_grad()
            p = model(dense, idx)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)
            loss.backward()
            opt.step()
            return loss.detach()
        return model, opt, step

    model_e, opt_e, step_e = make()
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
    torch.cuda.synchronize()
    assert opt_c.iterations == 0
    for s, bt in enumerate(batches, 1):
        captured(*bt)
        torch.cuda.synchronize()
        assert opt_c.iterations == s
    for (n, a), (_, b) in zip(model_e.named_parameters(), model_c.named_parameters()):
        assert torch.equal(a, b), n
        for k in opt_e.state[a]:
            assert torch.equal(opt_e.state[a][k], opt_c.state[b][k]), (n, k)


# ---------------------------------------------------------------------------------------------------- 6. state_dict, reset_
@pytest.mark.parametrize("h", TABLE_CASES, ids=TABLE_IDS)
def test_state_dict_round_trip_and_reset(h):
    emb = _table_layer(None)
    idx = torch.tensor(_table_batches(1, seed=4)[0][0], device="cuda")
    emb(idx)
    dense = torch.nn.Parameter(torch.randn(37, device="cuda"))
    opt = make_opt([emb.embeddings, dense], h)

    def one(o):
        o.zero_grad()
        (emb(idx).square().sum() + dense.square().sum()).backward()
        o.step()

    fresh = None
    for s in range(2):
        one(opt)
        if s == 0:
            fresh = {k: v.clone() for k, v in opt.state[emb.embeddings].items()}
    sd = copy.deepcopy(opt.state_dict())
    assert sd["iterations"] == 2
    assert set(sd["state"][0]) == ({"accumulator", "linear"} if h["rule"] == FTRL else {"accumulator"})
    snap = [emb.embeddings.detach().clone(), dense.detach().clone()]
    one(opt)
    after_a = [emb.embeddings.detach().clone(), dense.detach().clone()]
    with torch.no_grad():
        emb.embeddings.copy_(snap[0])
        dense.copy_(snap[1])
    opt2 = make_opt([emb.embeddings, dense], h)
    opt2.load_state_dict(sd)
    assert opt2.iterations == 2
    one(opt2)
    assert opt2.iterations == 3
    assert torch.equal(emb.embeddings, after_a[0]) and torch.equal(dense, after_a[1])
    # reset_: the never-stepped state, in place -- one step from there repeats the first step of the run above
    with torch.no_grad():
        emb.embeddings.copy_(snap[0])
    store = {k: v.data_ptr() for k, v in opt2.state[emb.embeddings].items()}
    opt2.reset_()
    assert opt2.iterations == 0
    st = opt2.state[emb.embeddings]
    assert {k: v.data_ptr() for k, v in st.items()} == store
    assert torch.all(st["accumulator"] == f32(0.1)) and ("linear" not in st or not st["linear"].any())
    assert all(not s.any() for s in opt2._stamps.values())
    assert set(fresh) == set(st)


# ---------------------------------------------------------------------------------------------------- 7. whole model
@pytest.mark.parametrize("h", [hyper(ADAGRAD, lr=1e-2), hyper(FTRL, lr=5e-2, l1=1e-4, l2=1e-3)], ids=TABLE_IDS)
def test_xdeepfm_steps_match_oracle(h):
    """XDeepFM with tableGrad="runs", 3 steps against the float64 oracle graph's gradients pushed through the float64 rule: every
    parameter within 1e-5 (relative to its largest element) under Adagrad, each update within 1e-3.  Ftrl recomputes p from z, and
    from z = 0 its first step replaces every weight by about -lr g / sqrt(n): p is a direct function of the summed gradients and
    inherits the fp32 model's gradient error, so the parameters are held to 1e-2 of their largest element -- and every dense
    parameter's step is checked element by element against the float64 rule on the gradient the model produced (check_step)."""
    torch.manual_seed(2)
    vocab = [7, 11, 5, 13, 3, 17]
    B, K_ = 48, 8
    fi, model = _xdeepfm(vocab, K_, "runs")
    dense, idx = _inputs(B, 3, vocab, seed=9)
    model(dense, idx)
    names = [n for n, _ in model.named_parameters()]
    key = {id(p): n for n, p in model.named_parameters()}
    b = model.body
    offs, loff = fi.sparse_embed.offsets.cpu(), fi.linear_embed.offsets.cpu()
    P = {n: p.detach().cpu().double().clone() for n, p in model.named_parameters()}
    S1 = {n: torch.full_like(v, f32(0.1)) for n, v in P.items()}
    Z = {n: torch.zeros_like(v) for n, v in P.items()}
    opt = make_opt(model.parameters(), h)
    rng = np.random.default_rng(10)
    for t in range(1, 4):
        dense, idx = _inputs(B, 3, vocab, seed=20 + t)
        y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")
        Q = {n: v.clone().requires_grad_() for n, v in P.items()}
        O = lambda p: Q[key[id(p)]]
        emb, lin = O(fi.sparse_embed.embeddings), O(fi.linear_embed.embeddings)
        sparse = graph.sparse_embed([emb[offs[f]:offs[f] + vocab[f]] for f in range(len(vocab))],
                                    [idx[:, f:f + 1].cpu() for f in range(len(vocab))])
        linear = sum(lin[loff[f]:loff[f] + vocab[f]][idx[:, f].cpu()] for f in range(len(vocab)))
        cin_out = graph.cin(torch.cat(sparse, 1), [O(w)[0] for w in b.cin.conv_kernels], [O(v) for v in b.cin.conv_biases],
                            O(b.cin.logit_kernel), O(b.cin.logit_bias))
        x = graph.stack_layer([dense.cpu().double()[:, i:i + 1] for i in range(3)] + sparse)
        for hl in b.dnn.hidden_list:
            yy = x @ O(hl.dense.kernel) + O(hl.dense.bias)
            x = torch.relu(x + yy) if x.shape == yy.shape else torch.relu(yy)
        p64 = torch.sigmoid(linear + cin_out + x @ O(b.dnn.logit_layer.kernel) + O(b.dnn.logit_layer.bias))[:, 0]
        y64 = y.cpu().double()
        reg64 = sum(1e-3 * emb[offs[f]:offs[f] + vocab[f]].square().sum() for f in range(len(vocab)))
        loss64 = -(y64 * torch.log(p64) + (1 - y64) * torch.log(1 - p64)).mean() + reg64
        loss64.backward()
        old = dict(P)
        for n in names:
            tab = n.endswith("embeddings")
            if Q[n].grad is None and not tab:
                continue
            g = (Q[n].grad if Q[n].grad is not None else torch.zeros_like(P[n])).numpy()
            if tab:     # Keras' IndexedSlices: an unregularised table (the linear one) changes only in its touched rows
                rows = np.nonzero(np.abs(g).sum(1) > 0)[0] if "linear" in n else np.arange(g.shape[0])
            else:
                rows = slice(None)
            pp, s1, zz = P[n].numpy().copy(), S1[n].numpy().copy(), Z[n].numpy().copy()
            if h["rule"] == ADAGRAD:
                pp[rows], s1[rows] = adagrad64(pp[rows], g[rows], s1[rows], h)
            else:
                pp[rows], s1[rows], zz[rows] = ftrl64(pp[rows], g[rows], s1[rows], zz[rows], h)
            P[n], S1[n], Z[n] = torch.tensor(pp), torch.tensor(s1), torch.tensor(zz)
        prev = {n: p.detach().cpu().double().clone() for n, p in model.named_parameters()}
        opt.zero_grad()
        out = model(dense, idx)
        loss = torch.nn.functional.binary_cross_entropy(out[:, 0], y) + collect_regularization_loss(model)
        assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
        loss.backward()
        assert fi.sparse_embed.embeddings.grad is None and fi.linear_embed.embeddings.grad is None
        ftrl = h["rule"] == FTRL
        before = {}
        for n, p in model.named_parameters():
            st = opt.state.get(p, {})
            before[n] = (c64(p), c64(st["accumulator"]) if "accumulator" in st else np.full(p.shape, f32(0.1)),
                         c64(st["linear"]) if "linear" in st else np.zeros(p.shape))
        opt.step()
        for n, p in model.named_parameters():
            got = p.detach().cpu().double()
            if P[n].abs().max() > 0:
                e = float((got - P[n]).abs().max() / P[n].abs().max())
                assert e < (1e-2 if ftrl else 1e-5), (n, t, e)
            if ftrl:
                if p.grad is not None:
                    st = opt.state[p]
                    check_step(h, (c64(p), c64(st["accumulator"]), c64(st["linear"])), before[n], c64(p.grad), where=(n, t))
                continue
            upd, upd64 = got - prev[n], P[n] - old[n]
            if upd64.abs().max() > 0:
                e = float((upd - upd64).abs().max() / upd64.abs().max())
                assert e < 1e-3, (n, t, e)
    assert opt.iterations == 3


def test_wide_deep_trains_with_ftrl_linear_and_adagrad_rest():
    """Wide_Deep on the synthetic teacher data of test_cin_bf16 (Zipf ids, labels from a per-category logit), tableGrad="runs": Ftrl
    with l1 > 0 on the linear (wide) tables, Adagrad on everything else, 150 steps at B = 4096.  Held-out BCE falls well below its
    starting value and the AUC clears a bar set from a recorded run (one MI355X: BCE 0.699 -> 0.631, AUC 0.701, 80% of the wide
    tables' weights exactly zero)."""
    from ml_function_amd import metrics
    from tests.test_cin_bf16 import _teacher_batches
    rng0 = np.random.default_rng(7)
    vocab = [int(v) for v in np.exp(rng0.uniform(np.log(10), np.log(2e4), 26))]
    B, Kd = 4096, 16
    batches = _teacher_batches(150, B, vocab, seed=1)
    held = _teacher_batches(1, 4 * B, vocab, seed=2)[0]
    torch.manual_seed(0)
    info = models.make_sparse_info(vocab, embed_dim=Kd)
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useFlattenLinear=True, tableGrad="runs")
    model = models.CTRModel(fi, models.Wide_Deep(hidden_units=[64, 32])).cuda()
    model(batches[0][0], batches[0][1])
    wide = [fi.linear_embed.embeddings]
    rest = [p for p in model.parameters() if p is not wide[0]]
    ftrl = optim.Ftrl(wide, learning_rate=0.05, l1_regularization_strength=1e-3)
    ada = optim.Adagrad(rest, learning_rate=0.05)

    def held_out():
        with torch.no_grad():
            out = model(held[0], held[1])
            p = out[:, 1] if out.shape[1] == 2 else out[:, 0]
            return float(losses.binary_crossentropy(p, held[2], eps=1e-6)), metrics.auc(held[2], p)

    bce0, _ = held_out()
    for dense, idx, y in batches:
        ftrl.zero_grad()
        ada.zero_grad()
        out = model(dense, idx)
        p = out[:, 1] if out.shape[1] == 2 else out[:, 0]
        (losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)).backward()
        ftrl.step()
        ada.step()
    bce, auc = held_out()
    zeros = float((fi.linear_embed.embeddings == 0).float().mean())
    print("held-out BCE %.5f -> %.5f, AUC %.4f, exact zeros in the wide tables %.3f" % (bce0, bce, auc, zeros))
    assert ftrl.iterations == ada.iterations == len(batches)
    assert bce < bce0 - 0.04
    assert auc > 0.68
    assert zeros > 0.0                              # Ftrl's l1 makes rows exactly zero
