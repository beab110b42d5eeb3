"""Keras' SGD and RMSprop on the GPU (include/fil.h O4, ml_function_amd/optim.py), each test over the five variants (SGD plain /
momentum / Nesterov, RMSprop with momentum == 0 / > 0): fil_momopt_multi and the runs tables BIT-EQUAL to the numpy fp32 restatement
of tests/keras_sgd_rmsprop_ref.py (which rows move included) and within tests/test_optim_rowwise_gpu.py's bars of float64, torch's SGD
as an independent cross-check, the data-parallel merged update, HIP-graph capture with a float rate and a schedule, state_dict /
reset_, and a whole XDeepFM step against the float64 oracle graph."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, models, optim, schedules
from ml_function_amd._lib import MomoptHyper, check, ptr, stream_ptr
from ml_function_amd.layers import SparseEmbed
from ml_function_amd.layers.base import collect_regularization_loss
from oracle import graph
from tests import keras_sgd_rmsprop_ref as ref

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
F = np.float32
VARIANTS = ref.VARIANTS


def make_opt(params, h, **kw):
    v = h["variant"]
    if v.startswith("sgd"):
        return optim.SGD(params, learning_rate=kw.pop("learning_rate", float(h["lr"])), momentum=float(h["momentum"]),
                         nesterov=(v == "sgd_nesterov"), **kw)
    return optim.RMSprop(params, learning_rate=kw.pop("learning_rate", float(h["lr"])), rho=float(h["rho"]),
                         momentum=float(h["momentum"]), epsilon=float(h["eps"]), **kw)


def rule_of(h):
    return _lib.FIL_OPT_SGD if h["variant"].startswith("sgd") else _lib.FIL_OPT_RMSPROP


def c_hyper(h):
    return MomoptHyper(float(h["lr"]), float(h["eps"]), float(h["rho"]), float(h["momentum"]),
                       _lib.FIL_MOMOPT_NESTEROV if h["variant"] == "sgd_nesterov" else 0, 0)


def n32(t):
    return None if t is None else t.detach().cpu().numpy()


def c64(t):
    return t.detach().cpu().double().numpy()


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def slot_tensors(opt, p, h):
    """(slot0, slot1) of p as the optimizer holds them (None where the variant has none or before the first step)."""
    st = opt.state.get(p, {})
    got = [st.get(k) for k in ref.SLOT_NAMES[h["variant"]]]
    return tuple(got + [None] * (2 - len(got)))


def check_step64(h, got, old, g, g_err, where=""):
    """One step from the float32 state `old` (p, s, z as float64 arrays or None) with the float64 gradient g against the float64 rule,
    within a bound on the fp32 rounding of each operation plus what an error g_err of the gradient the kernel formed itself (an fp32 run
    sum over several lists, the l2 term) moves the result by.  A formula slip is orders of magnitude outside it."""
    v = h["variant"]
    lr, m, rho, eps = (float(h[k]) for k in ("lr", "momentum", "rho", "eps"))
    p0, s0, z0 = old
    want_p, want_s, want_z = ref.elem64(h, p0, s0, z0, g, True)
    p, s, z = got
    ag = np.abs(g)

    def close(x, want, tol, what):
        assert np.all(np.abs(x - want) <= tol), (where, what, float((np.abs(x - want) / tol).max()))

    if v == "sgd":
        close(p, want_p, 4 * EPS32 * (np.abs(p0) + ag * lr) + lr * g_err + 1e-30, "p")
        return
    if v in ("sgd_momentum", "sgd_nesterov"):
        tol_a = 4 * EPS32 * (np.abs(s0) * m + ag * lr) + lr * g_err + 1e-30
        close(s, want_s, tol_a, "a")
        if v == "sgd_momentum":
            close(p, want_p, 4 * EPS32 * (np.abs(p0) + np.abs(want_s)) + tol_a, "p")
        else:
            close(p, want_p, 8 * EPS32 * (np.abs(p0) + np.abs(want_s) * m + ag * lr) + m * tol_a + lr * g_err, "p")
        return
    tol_s = 4 * EPS32 * (s0 + g * g) + (1 - rho) * (2 * ag * g_err + g_err * g_err) + 1e-30
    close(s, want_s, tol_s, "rms")
    if v == "rmsprop":
        root = np.maximum(np.sqrt(want_s), 1e-30)
        d = root + eps
        step = lr * ag / d
        close(p, want_p, 8 * EPS32 * (np.abs(p0) + step) + lr * g_err / d + step * tol_s / (2 * root * d) + 1e-30, "p")
        return
    d = np.sqrt(want_s + eps)
    upd = lr * ag / d
    tol_z = 8 * EPS32 * (np.abs(z0) * m + upd) + lr * g_err / d + upd * tol_s / (2 * (want_s + eps)) + 1e-30
    close(z, want_z, tol_z, "mom")
    close(p, want_p, 4 * EPS32 * (np.abs(p0) + np.abs(want_z)) + tol_z, "p")


# ---------------------------------------------------------------------------------------------------- 1. dense tensors, one launch
SIZES = [(1,), (3,), (4,), (1023,), (4096,), (65537,), (1521, 128), (517,), (2051,)]
NONE, WITH_L2, DESC_L2 = 2, 4, 3e-2          # tensor 2 has no gradient (grad NULL); tensor 4 carries a descriptor l2
MIS_P, MIS_S = 7, 8                          # tensor 7: parameter 4 bytes off a 16-byte boundary; tensor 8: its slots and gradient


def _alloc(shape, off):
    n = int(np.prod(shape))
    return torch.zeros(n + 4, device="cuda")[off:off + n].view(shape)


def _dense_state(h, rng):
    n = ref.N_SLOTS[h["variant"]]
    ps = [_alloc(s, 1 if i == MIS_P else 0) for i, s in enumerate(SIZES)]
    for p, s in zip(ps, SIZES):
        p.copy_(torch.tensor(rng.standard_normal(s) * 0.5, dtype=torch.float32))
    s0 = [_alloc(s, 1 if i == MIS_S else 0) if n >= 1 else None for i, s in enumerate(SIZES)]
    s1 = [_alloc(s, 3 if i == MIS_S else 0) if n >= 2 else None for i, s in enumerate(SIZES)]
    gs = [_alloc(s, 2 if i == MIS_S else 0) for i, s in enumerate(SIZES)]
    assert ps[MIS_P].data_ptr() % 16 == 4 and gs[MIS_S].data_ptr() % 16 == 8
    return ps, s0, s1, gs


@pytest.mark.parametrize("variant", VARIANTS)
def test_momopt_multi_is_bit_equal_to_the_restatement(variant):
    """5 steps of fil_momopt_multi over 9 tensors (awkward sizes and tails, one without gradient, one with l2, misaligned ones): every
    tensor and slot bit-equal to the numpy fp32 restatement after every step, and the trajectory within 1e-6 of a float64 one
    (tests/test_optim_rowwise_gpu.py's bar for Adagrad, at its rate 1e-3 and its parameter scale: the bar is relative to the norm of
    the tensor, so it presumes, as there, steps that are small against the parameters -- a one-element tensor that a larger rate walks
    through zero has no such norm to lean on)."""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    h = ref.hyper(variant, lr=1e-3)
    ps, s0, s1, gs = _dense_state(h, rng)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    descs = (optim._Desc * len(SIZES))(*[optim._Desc(p.data_ptr(), None if i == NONE else g.data_ptr(), ptr(a), ptr(z), p.numel(),
                                                     DESC_L2 if i == WITH_L2 else 0.0, 0)
                                         for i, (p, g, a, z) in enumerate(zip(ps, gs, s0, s1))])
    d = torch.frombuffer(bytearray(descs), dtype=torch.uint8).cuda()
    total = sum(p.numel() for p in ps)
    ch = c_hyper(h)
    state = [(n32(p).copy(), None if a is None else n32(a).copy(), None if z is None else n32(z).copy()) for p, a, z in zip(ps, s0, s1)]
    traj = [tuple(None if x is None else x.astype(np.float64) for x in st) for st in state]
    for t in range(1, 6):
        grads = [(rng.standard_normal(s) * 10.0 ** rng.integers(-3, 0)).astype(F) for s in SIZES]
        for g, gn in zip(gs, grads):
            g.copy_(torch.tensor(gn))
        check(lib.fil_momopt_multi(ptr(d), len(SIZES), total, ptr(step), rule_of(h), ctypes.addressof(ch), 1, stream_ptr()),
              "fil_momopt_multi")
        torch.cuda.synchronize()
        assert int(step) == t
        for i, shape in enumerate(SIZES):
            g = np.zeros(shape, F) if i == NONE else grads[i]
            l2 = DESC_L2 if i == WITH_L2 else 0.0
            state[i] = ref.dense_step(h, *state[i], g, l2)
            for got, want, what in zip((ps[i], s0[i], s1[i]), state[i], "psz"):
                assert (got is None) == (want is None)
                if got is not None:
                    assert same_bits(n32(got), want), (shape, t, what)
            g64 = g.astype(np.float64) + 2 * float(F(l2)) * traj[i][0]
            traj[i] = ref.elem64(h, *traj[i], g64, False)
            assert nrel(c64(ps[i]), traj[i][0]) < 1e-6, (shape, t)


@pytest.mark.parametrize("variant", VARIANTS)
def test_dense_parameters_with_decay_take_the_decayed_rate(variant):
    """optim.SGD / RMSprop(decay=) on dense parameters, one with grad None: the rate of every step is the device's word
    (current_learning_rate), and with it every step is bit-equal to the restatement."""
    rng = np.random.default_rng(1)
    h = ref.hyper(variant, lr=1e-2)
    shapes = [(7,), (4099,), (33, 17)]
    ps = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s), dtype=torch.float32, device="cuda")) for s in shapes]
    idle = torch.nn.Parameter(torch.ones(5, device="cuda"))
    opt = make_opt(ps + [idle], h, decay=0.5)
    n = ref.N_SLOTS[variant]
    state = [(n32(p).copy(), np.zeros(s, F) if n >= 1 else None, np.zeros(s, F) if n >= 2 else None) for p, s in zip(ps, shapes)]
    rates = []
    for t in range(4):
        lr_t = F(float(opt.current_learning_rate()))
        rates.append(float(lr_t))
        for i, (p, s) in enumerate(zip(ps, shapes)):
            g = (rng.standard_normal(s) * 0.3).astype(F)
            p.grad = torch.tensor(g, device="cuda")
            state[i] = ref.dense_step(ref.with_lr(h, lr_t), *state[i], g)
        opt.step()
        for i, p in enumerate(ps):
            assert same_bits(n32(p), state[i][0]), (i, t)
            for got, want in zip(slot_tensors(opt, p, h), state[i][1:]):
                assert (got is None) == (want is None) and (got is None or same_bits(n32(got), want)), (i, t)
    assert opt.iterations == 4 and torch.all(idle == 1) and idle not in opt.state
    np.testing.assert_allclose(rates, [1e-2 / (1 + 0.5 * t) for t in range(4)], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------- 2. the tables, in place
VOCAB = [50, 200, 30, 1000, 7, 64]
L2 = {0: 1e-2, 3: 3e-3}              # two regularised fields
FROZEN = 2                           # one frozen field
K, BT = 16, 512


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


def _row_maps(offs, V, l2=True):
    row_l2, frozen = np.zeros(V, F), np.zeros(V, bool)
    if l2:
        for f, lam in L2.items():
            row_l2[offs[f]:offs[f] + VOCAB[f]] = F(lam)
    frozen[offs[FROZEN]:offs[FROZEN] + VOCAB[FROZEN]] = True
    return row_l2, frozen


def _touched_rows(idx, offs, V):
    t = np.zeros(V, bool)
    for f, v in enumerate(VOCAB):
        if f != FROZEN:
            ok = (idx[:, f] >= 0) & (idx[:, f] < v)
            t[offs[f] + idx[ok, f]] = True
    return t


def _dense_grad64(idx, g, offs, V):
    """The summed row gradients in float64 and a bound on the error of an fp32 sum of them: (terms + 1) eps sum |terms|."""
    G, A, C = np.zeros((V, K)), np.zeros((V, K)), np.zeros(V)
    for f, v in enumerate(VOCAB):
        if f == FROZEN:
            continue
        ok = (idx[:, f] >= 0) & (idx[:, f] < v)
        np.add.at(G, offs[f] + idx[ok, f], g[ok, f])
        np.add.at(A, offs[f] + idx[ok, f], np.abs(g[ok, f]))
        np.add.at(C, offs[f] + idx[ok, f], 1)
    return G, (C[:, None] + 1) * EPS32 * A


def _library_run_sums(p, rec):
    """The record's run sums as the library forms them (fil_embed_run_sum_dt into a zeroed table) and the rows it holds."""
    dt = torch.zeros_like(p)
    check(_lib.load().fil_embed_run_sum_dt(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), ptr(dt), rec["R"], p.shape[1],
                                           rec["g_dtype"], stream_ptr()), "fil_embed_run_sum_dt")
    ids = rec["sorted_ids"][:rec["R"]]
    touched = np.zeros(p.shape[0], bool)
    touched[ids[ids >= 0].cpu().numpy()] = True
    return n32(dt), touched


def _run_table(h, out_dtype, batches, check_each, l2=True, **kw):
    emb = _table_layer(out_dtype, l2)
    emb(torch.tensor(batches[0][0], device="cuda"))                     # build
    p = emb.embeddings
    opt = make_opt([p], h, **kw)
    offs = emb.offsets.cpu().numpy()
    V = p.shape[0]
    n = ref.N_SLOTS[h["variant"]]
    row_l2, frozen = _row_maps(offs, V, l2)
    state = (n32(p).copy(), np.zeros((V, K), F) if n >= 1 else None, np.zeros((V, K), F) if n >= 2 else None)
    seen_decay = False
    for t, (idx, g) in enumerate(batches, 1):
        opt.zero_grad()
        block = emb(torch.tensor(idx, device="cuda"))
        gt = torch.tensor(g, dtype=block.dtype, device="cuda")
        block.backward(gt)
        assert p.grad is None and p._fil_pending_runs is not None
        if check_each:
            sums, touched = _library_run_sums(p, p._fil_pending_runs)
        opt.step()
        assert p._fil_pending_runs is None
        if not check_each:
            continue
        # the record holds exactly the rows the batch touches, and its sums are the batch's gradient
        assert np.array_equal(touched, _touched_rows(idx, offs, V)) and not touched[frozen].any()
        G64, Gerr = _dense_grad64(idx, c64(gt), offs, V)
        assert np.all(np.abs(sums[touched] - G64[touched]) <= Gerr[touched] + 1e-30)
        old = state
        state, moved, decayed = ref.table_step(h, *state, sums, touched, row_l2, frozen)
        got = (n32(p),) + tuple(n32(s) for s in slot_tensors(opt, p, h))
        for a, b, what in zip(got, state, "psz"):
            assert (a is None) == (b is None)
            if a is not None:
                assert same_bits(a, b), (t, what, int((a.view(np.int32) != b.view(np.int32)).any(axis=1).sum()))
        # spelled out: every row that Keras leaves alone has unchanged bits in p and in every slot
        keep = ~moved & ~decayed
        assert keep[frozen].all() and (keep & ~frozen).any() == (h["variant"] != "rmsprop")
        for a, b in zip(got, old):
            if a is not None:
                assert same_bits(a[keep], b[keep]), t
        untouched_l2 = ~touched & (row_l2 > 0)
        assert untouched_l2.any() == l2
        if l2:
            assert (got[0][untouched_l2] != old[0][untouched_l2]).any(axis=1).all()       # the regulariser moves them
        if h["variant"] == "rmsprop":
            # untouched rows of unregularised fields: rms *= rho, p untouched; frozen fields: rms untouched
            assert decayed.any() and same_bits(got[0][decayed], old[0][decayed])
            assert same_bits(got[1][decayed], old[1][decayed] * h["rho"])
            assert same_bits(got[1][frozen], old[1][frozen]) and not got[1][frozen].any()
            seen_decay = seen_decay or bool((old[1][decayed] != 0).any())
        else:
            assert not decayed.any()
    assert opt.iterations == len(batches)
    if check_each and h["variant"] == "rmsprop":
        assert seen_decay                               # some row was touched at one step and decayed at a later one
    return opt, (p.detach().clone(),) + tuple(s.clone() for s in slot_tensors(opt, p, h) if s is not None)


@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_runs_table_matches_keras_semantics(variant, out_dtype):
    h = ref.hyper(variant, lr=1e-2)
    batches = _table_batches(3, seed=11)
    _, a = _run_table(h, out_dtype, batches, check_each=True)
    _, b = _run_table(h, out_dtype, batches, check_each=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))           # run 2 bitwise equal to run 1


@pytest.mark.parametrize("variant", VARIANTS)
def test_runs_table_without_regularised_fields(variant):
    """No field regularised: the row-local variants run no sweep and allocate no stamps; RMSprop with momentum == 0 still sweeps (rms
    decays on every untouched row: checked bit for bit inside _run_table) and so has stamps."""
    h = ref.hyper(variant, lr=1e-2)
    opt, _ = _run_table(h, None, _table_batches(3, seed=13), check_each=True, l2=False)
    assert bool(opt._stamps) == (variant == "rmsprop")


# ---------------------------------------------------------------------------------------------------- 3. slot-less SGD
def test_plain_sgd_keeps_no_slot_tensors_and_takes_null_slots():
    lib = _lib.load()
    h = ref.hyper("sgd", lr=1e-2)
    opt, _ = _run_table(h, None, _table_batches(2, seed=17), check_each=True)
    assert all(not st for st in opt.state.values())
    dense = torch.nn.Parameter(torch.ones(1000, device="cuda"))
    opt = make_opt([dense], h)
    dense.grad = torch.ones_like(dense)
    opt.step()
    assert not opt.state and opt.state_dict()["state"] == {}
    assert same_bits(n32(dense), np.ones(1000, F) - np.ones(1000, F) * h["lr"])
    # the C entry points with NULL slots: the dense descriptor and the runs update
    p = torch.ones(1000, device="cuda")
    g = torch.full((1000,), 2.0, device="cuda")
    desc = (optim._Desc * 1)(optim._Desc(p.data_ptr(), g.data_ptr(), None, None, 1000, 0.0, 0))
    d = torch.frombuffer(bytearray(desc), dtype=torch.uint8).cuda()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ch = c_hyper(h)
    check(lib.fil_momopt_multi(ptr(d), 1, 1000, ptr(step), _lib.FIL_OPT_SGD, ctypes.addressof(ch), 1, stream_ptr()), "fil_momopt_multi")
    assert int(step) == 1 and same_bits(n32(p), np.ones(1000, F) - np.full(1000, 2, F) * h["lr"])
    emb = _table_layer(None)
    idx, gg = _table_batches(1, seed=19)[0]
    emb(torch.tensor(idx, device="cuda")).backward(torch.tensor(gg, dtype=torch.float32, device="cuda"))
    rec, tab = emb.embeddings._fil_pending_runs, emb.embeddings
    emb.embeddings._fil_pending_runs = None
    sums, touched = _library_run_sums(tab, rec)
    before = n32(tab).copy()
    check(lib.fil_embed_momopt_runs(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), rec["R"], K, rec["g_dtype"], rec["F"], None,
                                    ptr(tab), None, None, None, ptr(step), _lib.FIL_OPT_SGD, ctypes.addressof(ch), stream_ptr()),
          "fil_embed_momopt_runs")
    want = before.copy()
    want[touched] = before[touched] - sums[touched] * h["lr"]
    assert same_bits(n32(tab), want)


# ---------------------------------------------------------------------------------------------------- 4. torch as a cross-check
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_agrees_with_torch_sgd(momentum):
    """optim.SGD on dense parameters against torch.optim.SGD, 5 steps.  Plain SGD is the same rule; with momentum torch keeps
    buf = momentum buf + g and moves p -= lr buf, Keras a = momentum a - lr g and p += a: a = -lr buf at a constant rate, equal to
    rounding.  Nesterov and RMSprop are NOT compared: torch's Nesterov step is p -= lr (g + momentum buf) on the gradient-scale
    buffer, which is Keras' form only up to rounding of different intermediate sums and differs in what the slot holds under a changing
    rate; torch's RMSprop has epsilon 1e-8 outside the root in both of its forms, where Keras' fused form (momentum > 0) has it inside,
    and it moves every row of a dense table."""
    rng = np.random.default_rng(4)
    shapes = [(7,), (4096,), (333, 17)]
    a = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s), dtype=torch.float32, device="cuda")) for s in shapes]
    b = [torch.nn.Parameter(x.detach().clone()) for x in a]
    oa = optim.SGD(a, learning_rate=0.01, momentum=momentum)
    ob = torch.optim.SGD(b, lr=0.01, momentum=momentum)
    for _ in range(5):
        for x, y, s in zip(a, b, shapes):
            g = torch.tensor(rng.standard_normal(s) * 0.3, dtype=torch.float32, device="cuda")
            x.grad, y.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    for x, y in zip(a, b):
        assert nrel(c64(x), c64(y)) < 1e-6
        if momentum:
            assert torch.allclose(oa.state[x]["momentum"], -0.01 * ob.state[y]["momentum_buffer"], rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------------------------------- 5. data parallelism
@pytest.mark.parametrize("l2", [True, False], ids=["l2", "nol2"])
@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_w1_exchange_is_bitwise_the_one_gpu_update(variant, out_dtype, l2):
    h = ref.hyper(variant, lr=1e-2)
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
            traj.append((emb.embeddings.detach().clone(),) + tuple(s.clone() for s in slot_tensors(opt, emb.embeddings, h) if s is not None))
        assert (emb.embeddings in opt._xbuf) == force
        runs.append(traj)
    for s, (a, b) in enumerate(zip(*runs)):
        assert len(a) == len(b) == 1 + ref.N_SLOTS[variant]
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


@pytest.mark.parametrize("cls", ["SGD", "RMSprop"])
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
@pytest.mark.parametrize("variant", VARIANTS)
def test_sharded_merged_update_matches_float64_full_batch(variant, W):
    """W shards' compact lists gathered on one GPU, fil_embed_momopt_merged + the sweep, against the float64 rule on the full batch's
    dense gradient (the rows Keras updates), bitwise-unchanged rows elsewhere, and for RMSprop with momentum == 0 the decayed rms."""
    per = 256
    lib = _lib.load()
    h = ref.hyper(variant, lr=1e-2)
    emb = _table_layer(None)
    emb(torch.tensor(_table_batches(1, 0, B=8)[0][0], device="cuda"))
    offs = emb.offsets.cpu().numpy()
    p = emb.embeddings
    V = p.shape[0]
    n = ref.N_SLOTS[variant]
    s0 = torch.zeros((V, K), device="cuda") if n >= 1 else None
    s1 = torch.zeros((V, K), device="cuda") if n >= 2 else None
    stamp = torch.zeros(V, dtype=torch.int32, device="cuda")
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    ch = c_hyper(h)
    row_l2, frozen = _row_maps(offs, V)
    opt64 = lambda x: None if x is None else c64(x)
    for step in (1, 2):
        idx, g = _table_batches(1, seed=100 * W + step, B=W * per)[0]
        shards = [_record(emb, idx[w * per:(w + 1) * per], g[w * per:(w + 1) * per]) for w in range(W)]
        ids, values, counts, cap = _gather(shards)
        old = (c64(p), opt64(s0), opt64(s1))
        rec = shards[0]
        optim.momopt_merged(rule_of(h), ids, values, counts, W, cap, emb.offsets, rec["field_l2"], p, s0, s1, stamp, t, ch)
        check(lib.fil_embed_momopt_sweep(ptr(p), ptr(s0), ptr(s1), ptr(stamp), V, K, ptr(rec["offsets"]), ptr(rec["field_l2"]),
                                         ptr(rec["frozen"]), rec["F"], ptr(t), rule_of(h), ctypes.addressof(ch), stream_ptr()),
              "fil_embed_momopt_sweep")
        t += 1
        got = (c64(p), opt64(s0), opt64(s1))
        G, Gerr = _dense_grad64(idx, c64(torch.tensor(g, dtype=torch.float32)), offs, V)
        G = G + 2 * row_l2.astype(np.float64)[:, None] * old[0]
        Gerr = Gerr + 4 * EPS32 * np.abs(G)
        touched = _touched_rows(idx, offs, V)
        rows = (touched | (row_l2 > 0)) & ~frozen
        sub = lambda x, r: None if x is None else x[r]
        check_step64(h, tuple(sub(x, rows) for x in got), tuple(sub(x, rows) for x in old), G[rows], Gerr[rows], where=(W, step))
        keep = ~rows
        assert keep.any()
        assert np.array_equal(got[0][keep], old[0][keep])
        if variant == "rmsprop":
            dec = keep & ~frozen
            assert np.array_equal(got[1][dec], (old[1][dec].astype(F) * h["rho"]).astype(np.float64))
            assert np.array_equal(got[1][frozen], old[1][frozen])
        else:
            for a, b in zip(got[1:], old[1:]):
                assert a is None or np.array_equal(a[keep], b[keep])


def _ranks(n):
    from tests.test_dp_gpu import _run_ranks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return _run_ranks([os.path.join(root, "tests", "dp_momentum_worker.py")], n, timeout=600)


def test_dp_momentum_worker_on_one_rank():
    r = _ranks(1)
    assert r.returncode == 0 and "DP_MOMENTUM_OK 1" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_dp_momentum_worker_on_two_ranks():
    r = _ranks(2)
    assert r.returncode == 0 and "DP_MOMENTUM_OK 2" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------- 6. HIP-graph capture
def _xdeepfm(vocab, K_, table_grad, emb_reg=1e-3):
    info = [i._replace(emb_reg=emb_reg) for i in models.make_sparse_info(vocab, embed_dim=K_)]
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad=table_grad)
    return fi, models.CTRModel(fi, models.XDeepFM(conv_size=[16, 12], hidden_units=[32, 16])).cuda()


def _inputs(B, n_dense, vocab, seed=0):
    rng = np.random.default_rng(seed)
    dense = torch.tensor(rng.random((B, n_dense)), dtype=torch.float32, device="cuda")
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device="cuda")
    return dense, idx


@pytest.mark.parametrize("rate,emb_reg", [("float", 1e-3), ("float", 0.0), ("exponential", 1e-3)], ids=["float-l2", "float-nol2", "sched-l2"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_captured_step_replays_bitwise_like_eager(variant, rate, emb_reg):
    """Three replays of a captured XDeepFM step against three eager steps: every parameter and slot bit-equal, with a float rate and
    with ExponentialDecay (the rate changes from replay to replay: the graph reads it from the device)."""
    h = ref.hyper(variant, lr=1e-2)
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
        kw = {}
        if rate == "exponential":
            kw["learning_rate"] = schedules.ExponentialDecay(1e-2, decay_steps=2, decay_rate=0.5)
        opt = make_opt(model.parameters(), h, **kw)

        def step(dense, idx, y):
            opt.zero_grad()
            p = model(dense, idx)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)
            loss.backward()
            opt.step()
            return loss.detach()
        return model, opt, step

    model_e, opt_e, step_e = make()
    lrs = []
    for bt in batches:
        lrs.append(float(opt_e.current_learning_rate()))
        step_e(*bt)
    if rate == "exponential":
        assert lrs[0] > lrs[1] > lrs[2] > 0
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
        assert set(opt_e.state.get(a, {})) == set(opt_c.state.get(b, {})) == set(ref.SLOT_NAMES[variant]), n
        for k in opt_e.state.get(a, {}):
            assert torch.equal(opt_e.state[a][k], opt_c.state[b][k]), (n, k)


# ---------------------------------------------------------------------------------------------------- 7. state_dict, reset_, refusals
@pytest.mark.parametrize("variant", VARIANTS)
def test_state_dict_round_trip_and_reset(variant):
    h = ref.hyper(variant, lr=1e-2)
    emb = _table_layer(None)
    idx = torch.tensor(_table_batches(1, seed=4)[0][0], device="cuda")
    emb(idx)
    dense = torch.nn.Parameter(torch.randn(37, device="cuda"))
    opt = make_opt([emb.embeddings, dense], h)

    def one(o):
        o.zero_grad()
        (emb(idx).square().sum() + dense.square().sum()).backward()
        o.step()

    first = None
    start = [emb.embeddings.detach().clone(), dense.detach().clone()]
    for s in range(2):
        one(opt)
        if s == 0:
            first = [emb.embeddings.detach().clone(), dense.detach().clone()]
    sd = copy.deepcopy(opt.state_dict())
    assert sd["iterations"] == 2
    names = set(ref.SLOT_NAMES[variant])
    assert (set(sd["state"][0]) == names) if names else (sd["state"] == {})
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
    # reset_: the never-stepped state, in place -- one step from the initial weights repeats the first step of the run above
    with torch.no_grad():
        emb.embeddings.copy_(start[0])
        dense.copy_(start[1])
    store = {k: v.data_ptr() for k, v in opt2.state.get(emb.embeddings, {}).items()}
    opt2.reset_()
    assert opt2.iterations == 0
    st = opt2.state.get(emb.embeddings, {})
    assert {k: v.data_ptr() for k, v in st.items()} == store and set(st) == names
    assert all(not v.any() for v in st.values())
    assert all(not s.any() for s in opt2._stamps.values())
    one(opt2)
    assert torch.equal(emb.embeddings, first[0]) and torch.equal(dense, first[1])


@pytest.mark.parametrize("cls", ["SGD", "RMSprop"])
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


@pytest.mark.parametrize("cls", ["SGD", "RMSprop"])
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


# ---------------------------------------------------------------------------------------------------- 8. whole model
@pytest.mark.parametrize("variant", VARIANTS)
def test_xdeepfm_steps_match_oracle(variant):
    """XDeepFM with tableGrad="runs", 3 steps against the float64 oracle graph's gradients pushed through the float64 rule, at the
    bars tests/test_optim_rowwise_gpu.py::test_xdeepfm_steps_match_oracle holds Adagrad to: every parameter within 1e-5 (relative to
    its largest element), each update within 1e-3 (relative to the largest update of the tensor)."""
    torch.manual_seed(2)
    h = ref.hyper(variant, lr=1e-2)
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
    S1 = {n: torch.zeros_like(v) for n, v in P.items()}
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
                rows = np.abs(g).sum(1) > 0 if "linear" in n else np.ones(g.shape[0], bool)
            else:
                rows = np.ones(g.shape[0], bool)
            pp, s1, zz = P[n].numpy().copy(), S1[n].numpy().copy(), Z[n].numpy().copy()
            np_, ns, nz = ref.elem64(h, pp[rows], s1[rows], zz[rows], g[rows], True)
            pp[rows] = np_
            if ns is not None:
                s1[rows] = ns
            if nz is not None:
                zz[rows] = nz
            if variant == "rmsprop":        # ... except its rms, which Keras decays on every row
                s1[~rows] = s1[~rows] * float(h["rho"])
            P[n], S1[n], Z[n] = torch.tensor(pp), torch.tensor(s1), torch.tensor(zz)
        prev = {n: p.detach().cpu().double().clone() for n, p in model.named_parameters()}
        opt.zero_grad()
        out = model(dense, idx)
        loss = torch.nn.functional.binary_cross_entropy(out[:, 0], y) + collect_regularization_loss(model)
        assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
        loss.backward()
        assert fi.sparse_embed.embeddings.grad is None and fi.linear_embed.embeddings.grad is None
        opt.step()
        for n, p in model.named_parameters():
            got = p.detach().cpu().double()
            if P[n].abs().max() > 0:
                e = float((got - P[n]).abs().max() / P[n].abs().max())
                print("%s %s step %d: parameter error %.3e" % (variant, n, t, e))
                assert e < 1e-5, (n, t, e)
            upd, upd64 = got - prev[n], P[n] - old[n]
            if upd64.abs().max() > 0:
                e = float((upd - upd64).abs().max() / upd64.abs().max())
                print("%s %s step %d: update error %.3e" % (variant, n, t, e))
                assert e < 1e-3, (n, t, e)
    assert opt.iterations == 3
