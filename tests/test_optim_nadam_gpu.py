"""Keras' Nadam on the GPU (include/fil.h O6, ml_function_amd/optim.py) on the smallest shapes that reach every path of its kernels
(csrc/optim_rule.h with csrc/optim_nadam.hip): dense tensors of 1, 4095 and 4097 elements beside one without a gradient; the table of
tests/test_optim_adaptive_gpu.py -- three fields of 5, 1 and 40 rows (one regularised, one plain, one frozen, in two assignments), K in
{1, 3, 4, 16} (the scalar and the 16-byte sweep loop, and a slot array one dword off a 16-byte boundary), runs of 1, 2 and 70 ids, one
empty batch, f32 and bf16 gradients, the merged update at W = 1 and W = 3.

m and v involve no power: BIT-EQUAL to the numpy fp32 restatement (tests/keras_nadam_ref.py) after every step, and so are the decayed
rows (m b1, v b2, the bits of p kept) and the frozen ones (every bit kept).  The step's coefficients take the device's powf, so from
iterations 0 p is held to the float64 twin at the bars check_step applies to Adamax (ref.BARS: update 1e-4, p 1e-6, m and v 1e-5,
norm-relative, one step from the device's fp32 state and the device's fp32 cache; the twin carries its own float64 cache).  From
iterations 200 000 with cache 0 both powers have left the coefficients (tests/test_optim_nadam_host.py) and p is bit-equal too.
|p| is in [1, 1.95] and lr 1e-2: see ref.dense_inputs for why the bars hold there whatever the last bit of powf is.
Then the momentum cache over 64 advance-only steps, and the Python layer on SparseEmbed tables: the runs exchange at world size 1,
capture (one eager step + three replays == four eager steps, momentum_cache and iterations included), state_dict / reset_."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, models, optim
from ml_function_amd._lib import NadamHyper, check, ptr, stream_ptr
from ml_function_amd.layers import SparseEmbed
from tests import keras_nadam_ref as ref

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
F = np.float32
NADAM = _lib.FIL_OPT_NADAM
SENT = 12345.678          # sentinel around every array: never a value of the run
TAIL = 200000             # iterations from which the powers have left the coefficients (with cache 0)


def c_hyper(h, cache):
    return NadamHyper(float(h["lr"]), float(h["b1"]), float(h["b2"]), float(h["eps"]), float(h["sd"]), 0, cache.data_ptr())


def n32(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def guarded(shape, off=0, pad=64):
    """A zeroed array of `shape` inside a sentinel-filled buffer, `off` dwords past a 16-byte boundary -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), SENT, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[pad + off:pad + off + n].view(shape)
    view.zero_()
    return view, buf


def guards_intact(view, buf):
    b = n32(buf)
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((b[:lo] == F(SENT)).all() and (b[lo + view.numel():] == F(SENT)).all())


def advance(step, ch):
    """The launch that ends a step when nothing dense has a gradient: cache = cache mt(it), then the counter (n = 0)."""
    check(_lib.load().fil_nadam_multi(None, 0, 0, ptr(step), NADAM, ctypes.addressof(ch), 1, stream_ptr()), "fil_nadam_multi")


def check_step(h, it, cache32, cache64, got, old, g, where, exact):
    """One step from the device's fp32 state `old` = (p, m, v) and the device's fp32 cache with the fp32 gradient g (what the kernel
    forms: run sum + 2 l2 p).  m and v: bit-equal to the restatement.  p: bit-equal where `exact` (the tail), else against the float64
    twin (its own float64 cache) at ref.BARS.  Prints the measured errors."""
    want = ref.elem(h, ref.coefs(h, it, cache32), *old, g)
    assert same_bits(got[1], want[1]), (where, it, "m", int((got[1].view(np.int32) != want[1].view(np.int32)).sum()))
    assert same_bits(got[2], want[2]), (where, it, "v", int((got[2].view(np.int32) != want[2].view(np.int32)).sum()))
    if exact:
        assert same_bits(got[0], want[0]), (where, it, "p", int((got[0].view(np.int32) != want[0].view(np.int32)).sum()))
        return
    e = ref.step_errors(h, ref.coefs64(h, it, cache64), got, old, g)
    print("nadam %s it=%d: update %.2e  p %.2e  m %.2e  v %.2e" % (where, it, e["update"], e["p"], e["m"], e["v"]))
    assert ref.within_bars(e), (where, it, e)


# ---------------------------------------------------------------------------------------------------- 1. dense tensors, one launch
@pytest.mark.parametrize("start,sd", [(0, 0.004), (TAIL, 0.004), (0, 0.5)], ids=["it0", "it200000", "it0-sd0.5"])
def test_nadam_dense_tensors_in_one_launch(start, sd):
    """optim.Nadam over tensors of 1, 4095 and 4097 elements (the second with its slots one dword off a 16-byte boundary: the
    element-wise path) and one whose .grad is None, every step ONE dense launch: 12 steps from iterations 0, 3 from 200 000 with
    cache 0 on slots with history.  The parameter without a gradient keeps its bits and gets no slots; counter and cache advance.
    At Keras' schedule_decay 0.004 the momenta of neighbouring steps differ by 1.6e-4, which reaches the update damped below the
    bars: the case at schedule_decay 0.5 (2 % apart) is the one that tells mt1, the look-ahead momentum, from mt."""
    h = ref.hyper(lr=ref.DENSE_LR, schedule_decay=sd)
    rng, p0, signs = ref.dense_inputs(0)
    arrs = [[guarded((n,), off=(1 if (i == 1 and j > 0) else 0)) for j in range(3)] for i, n in enumerate(ref.DENSE_SIZES)]   # p, m, v
    params = []
    for (p, _), x in zip((a[0] for a in arrs), p0):
        p.copy_(torch.tensor(x))
        params.append(torch.nn.Parameter(p))
        assert params[-1].data_ptr() == p.data_ptr()
    idle = torch.nn.Parameter(torch.full((5,), 1.5, device="cuda"))
    opt = optim.Nadam(params + [idle], learning_rate=float(h["lr"]), schedule_decay=sd)
    for q, a in zip(params, arrs):
        if start:       # a state that has history
            a[1][0].copy_(torch.tensor(rng.standard_normal(q.shape) * 0.5, dtype=torch.float32))
            a[2][0].copy_(torch.tensor(rng.uniform(0.5, 1.5, q.shape), dtype=torch.float32))
        opt.state[q]["m"], opt.state[q]["v"] = a[1][0], a[2][0]
    dev = params[0].device
    opt._counter(dev).fill_(start)
    opt._cache_word(dev).fill_(0.0 if start else 1.0)
    launches = []
    dense = opt._launch_dense
    opt._launch_dense = lambda lib, desc, n, *a: (launches.append(n), dense(lib, desc, n, *a))[1]
    cache64 = 0.0 if start else 1.0
    for it in range(start, start + (3 if start else 12)):
        cache32 = F(opt.momentum_cache)
        old = [tuple(n32(a[j][0]).copy() for j in range(3)) for a in arrs]
        grads = ref.dense_grads(rng, signs)
        for q, g in zip(params, grads):
            q.grad = torch.tensor(g, device="cuda")
        opt.step()
        torch.cuda.synchronize()
        assert opt.iterations == it + 1 and launches == [3]         # one launch, three descriptors, and it advanced
        launches.clear()
        for i, a in enumerate(arrs):
            check_step(h, it, cache32, cache64, tuple(n32(a[j][0]) for j in range(3)), old[i], grads[i], ("dense", ref.DENSE_SIZES[i]),
                       exact=start > 0)
            assert all(guards_intact(*a[j]) for j in range(3)), (ref.DENSE_SIZES[i], it)
        # the cache took the step's momentum
        want = ref.coefs(h, it, cache32)["msn"]
        cache64 = ref.coefs64(h, it, cache64)["msn"]
        got = F(opt.momentum_cache)
        assert (got == want == 0) if start else abs(float(got) - cache64) <= 8 * (it + 1) * 2.0 ** -24 * cache64, (it, got, want, cache64)
    assert torch.all(idle == 1.5) and idle not in opt.state


# ---------------------------------------------------------------------------------------------------- 2. the momentum cache
def test_momentum_cache_over_64_advance_only_steps():
    """fil_nadam_multi(n = 0, advance = 1), 64 times: after every step the counter is t and the cache the product of mt(1) ... mt(t),
    against the float64 product within 8 t 2^-24 relative -- one product rounding per step plus mt's own (the product by beta_1, the
    subtraction from 1 at half the weight, powf at its documented 1 ulp and sd t's rounding, which the power damps): below 4 2^-24 a step.
    The cache stays a normal number (0.45^64 is about 1e-22).  Through optim.Nadam: a parameter without a gradient."""
    h = ref.hyper()
    idle = torch.nn.Parameter(torch.ones(3, device="cuda"))
    opt = optim.Nadam([idle])
    want, worst = 1.0, 0.0
    for t in range(1, 65):
        opt.step()
        want = ref.coefs64(h, t - 1, want)["msn"]
        got = opt.momentum_cache
        rel = abs(got - want) / want
        worst = max(worst, rel / (t * 2.0 ** -24))
        assert opt.iterations == t and rel <= 8 * t * 2.0 ** -24, (t, got, want, rel / 2.0 ** -24)
    print("momentum cache after 64 steps: %.9e against %.9e; worst error %.2f t 2^-24" % (got, want, worst))
    assert 1e-23 < got < 1e-21 and torch.all(idle == 1) and idle not in opt.state
    # the C entry point alone gives the same word
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    cache = torch.ones(1, device="cuda")
    ch = c_hyper(h, cache)
    for _ in range(64):
        advance(step, ch)
    assert int(step) == 64 and float(cache) == got


# ---------------------------------------------------------------------------------------------------- 3. the tables, in place (C ABI)
ROWS = [5, 1, 40]
OFFS = [0, 5, 6]
V = 46
B = 80
L2 = 1e-2
# field roles: (regularised, plain, frozen) -- the two layouts of tests/test_optim_adaptive_gpu.py
LAYOUTS = {"A": (2, 0, 1),       # the 40-row field regularised, the 5-row field plain, the 1-row field frozen
           "B": (0, 1, 2)}       # the 5-row field regularised, the 1-row field plain (one run of 80: longer than a wave), the 40-row frozen
BATCHES = [0, 1, None, 2]        # the steps of a run: _batch_ids(0), (1), an EMPTY batch, (2)


def _batch_ids(step):
    """[B, 3] ids.  Field 0: runs of 1, 2 and 70 on rows that rotate with the step (so a row touched at one step is untouched at a
    later one; row 4 only at the last), 3 ids of -1 and 4 out of range.  Field 1: its one row, 80 times (at step 1 not at all, so
    where it is the plain field it is once an untouched row).  Field 2: runs of 70, 2, 1 on rows 10 + step ..., a few other rows, two
    invalid ids; most of its 40 rows stay untouched."""
    rng = np.random.default_rng(100 + step)
    a, b, c = [(0, 1, 2), (3, 0, 1), (2, 4, 0)][step]
    f0 = [a] * 1 + [b] * 2 + [c] * 70 + [-1] * 3 + [7] * 4
    f1 = [0 if step != 1 else -1] * B
    f2 = [10 + step] * 70 + [20 + step] * 2 + [30 + step] * 1 + list(rng.integers(0, 40, 5)) + [40, -3]
    idx = np.stack([np.array(f0), np.array(f1), np.array(f2)], 1).astype(np.int64)
    assert idx.shape == (B, 3)
    return idx[rng.permutation(B)]


def _record(idx, frozen_field, K, bf16, seed, empty=False):
    """The runs record of a batch, built by hand: row ids (-1: invalid or frozen), stably sorted, and the permutation."""
    rng = np.random.default_rng(seed)
    rows = np.full(idx.shape, -1, np.int64)
    for f in range(3):
        ok = (idx[:, f] >= 0) & (idx[:, f] < ROWS[f]) & (f != frozen_field) & (not empty)
        rows[ok, f] = OFFS[f] + idx[ok, f]
    flat = rows.reshape(-1)
    order = np.argsort(flat, kind="stable")
    g = torch.tensor(rng.standard_normal((idx.size, K)) * 0.1, dtype=torch.float32, device="cuda")
    if bf16:
        g = g.to(torch.bfloat16)
    touched = np.zeros(V, bool)
    touched[flat[flat >= 0]] = True
    return dict(g=g, perm=torch.tensor(order, device="cuda"), sorted_ids=torch.tensor(flat[order], device="cuda"), R=idx.size,
                g_dtype=_lib.FIL_BF16 if bf16 else _lib.FIL_F32), touched, rows


def _library_run_sums(rec, K):
    """The record's run sums as the library forms them (fil_embed_run_sum_dt into a zeroed table)."""
    dt = torch.zeros((V, K), device="cuda")
    check(_lib.load().fil_embed_run_sum_dt(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), ptr(dt), rec["R"], K, rec["g_dtype"],
                                           stream_ptr()), "fil_embed_run_sum_dt")
    return n32(dt)


def _sums64(rec, rows, K):
    """The same sums in float64 and the bound of an fp32 sum in any order: (terms + 1) eps sum |terms|."""
    g = rec["g"].detach().cpu().double().numpy()
    G, A, C = np.zeros((V, K)), np.zeros((V, K)), np.zeros(V)
    flat = rows.reshape(-1)
    ok = flat >= 0
    np.add.at(G, flat[ok], g[ok])
    np.add.at(A, flat[ok], np.abs(g[ok]))
    np.add.at(C, flat[ok], 1)
    return G, (C[:, None] + 1) * EPS32 * A


def _field_maps(layout):
    reg, plain, frozen = LAYOUTS[layout]
    field_l2 = np.zeros(3, F)
    field_l2[reg] = F(L2)
    row_l2, row_frozen = np.zeros(V, F), np.zeros(V, bool)
    row_l2[OFFS[reg]:OFFS[reg] + ROWS[reg]] = F(L2)
    row_frozen[OFFS[frozen]:OFFS[frozen] + ROWS[frozen]] = True
    fz = np.zeros(3, np.uint8)
    fz[frozen] = 1
    return (torch.tensor(field_l2, device="cuda"), torch.tensor(fz, device="cuda"), torch.tensor(OFFS, dtype=torch.int64, device="cuda"),
            row_l2, row_frozen, frozen)


def _table_state(K, mis, start, seed):
    """Table and slots [V, K], each inside sentinels; `mis`: m one dword off a 16-byte boundary.  |p| in [1, 1.95] (ref.dense_inputs
    says why); start > 0: slots with history."""
    rng = np.random.default_rng(seed)
    p, m, v = guarded((V, K)), guarded((V, K), off=1 if mis else 0), guarded((V, K))
    if mis:
        assert m[0].data_ptr() % 16 == 4 and p[0].data_ptr() % 16 == 0
    p[0].copy_(torch.tensor(np.sign(rng.standard_normal((V, K))) * rng.uniform(1.0, 1.95, (V, K)), dtype=torch.float32))
    if start:
        m[0].copy_(torch.tensor(rng.standard_normal((V, K)) * 0.05, dtype=torch.float32))
        v[0].copy_(torch.tensor(np.abs(rng.standard_normal((V, K))) * 0.05 + 1e-3, dtype=torch.float32))
    return p, m, v


def _run_table_steps(h, K, mis, bf16, layout, start, W):
    """Four steps on the table through the C ABI, the third on an empty batch: W == 0: fil_embed_nadam_runs + sweep; W >= 1: the batch
    split over W lists (fil_embed_runs_compact each; for W == 3 the middle list empty), fil_embed_nadam_merged + sweep; then the
    advancing launch.  Every step checked from the device's previous state, every row by its kind.  Returns the final (p, m, v, cache)."""
    lib = _lib.load()
    field_l2, fz, offs, row_l2, row_frozen, frozen_field = _field_maps(layout)
    P, M, Vv = _table_state(K, mis, start, K)
    stamp = torch.zeros(V, dtype=torch.int32, device="cuda")
    step = torch.full((1,), start, dtype=torch.int64, device="cuda")
    cache = torch.full((1,), 0.0 if start else 1.0, device="cuda")
    cache64 = 0.0 if start else 1.0
    ch = c_hyper(h, cache)
    exact = start > 0
    live_decay = False
    for n_step, which in enumerate(BATCHES):
        it = start + n_step
        empty = which is None
        idx = _batch_ids(0 if empty else which)
        old = tuple(n32(x[0]).copy() for x in (P, M, Vv))
        cache32 = F(float(cache))
        if W == 0:
            rec, touched, rows = _record(idx, frozen_field, K, bf16, seed=7 * n_step + 1, empty=empty)
            sums = _library_run_sums(rec, K)
            G64, Gerr = _sums64(rec, rows, K)
            assert np.all(np.abs(sums[touched] - G64[touched]) <= Gerr[touched] + 1e-30)
            check(lib.fil_embed_nadam_runs(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), rec["R"], K, rec["g_dtype"], 3,
                                           ptr(field_l2), ptr(P[0]), ptr(M[0]), ptr(Vv[0]), ptr(stamp), ptr(step), NADAM,
                                           ctypes.addressof(ch), stream_ptr()), "fil_embed_nadam_runs")
        else:
            # shard w takes the samples b with b % W' == w (W == 3: the middle list is empty, the other two split the batch)
            parts = [idx] if W == 1 else [idx[0::2], idx[:0], idx[1::2]]
            recs = [_record(part if len(part) else idx, frozen_field, K, bf16, seed=7 * n_step + 1 + w, empty=empty or len(part) == 0)
                    for w, part in enumerate(parts)]
            cap = max(r[0]["R"] for r in recs) + 3           # greater than every count
            ids = torch.full((W * cap,), -7, dtype=torch.int64, device="cuda")
            values = torch.full((W * cap * K,), SENT, device="cuda")
            counts = torch.full((W,), -1, dtype=torch.int64, device="cuda")
            sums, touched = np.zeros((V, K), F), np.zeros(V, bool)
            for w, (rec, tw, _) in enumerate(recs):
                ws = torch.empty(max(1, optim.runs_compact_workspace_bytes(rec["R"])), dtype=torch.uint8, device="cuda")
                optim.runs_compact(rec, K, ids[w * cap:(w + 1) * cap], values[w * cap * K:(w + 1) * cap * K], counts[w:w + 1], cap, ws)
                sw = _library_run_sums(rec, K)
                first = tw & ~touched                                   # the lowest list holding a row owns it; the others are added
                sums[first] = sw[first]                                 # in list order, fp32
                sums[tw & touched] = sums[tw & touched] + sw[tw & touched]
                touched |= tw
            cnt = counts.cpu().numpy()
            assert (cnt < cap).all() and (W == 1 or cnt[1] == 0) and (cnt[0] > 0) != empty
            optim.nadam_merged(ids, values, counts, W, cap, offs, field_l2, P[0], M[0], Vv[0], stamp, step, ch)
        check(lib.fil_embed_nadam_sweep(ptr(P[0]), ptr(M[0]), ptr(Vv[0]), ptr(stamp), V, K, ptr(offs), ptr(field_l2), ptr(fz), 3, ptr(step),
                                        NADAM, ctypes.addressof(ch), stream_ptr()), "fil_embed_nadam_sweep")
        advance(step, ch)
        torch.cuda.synchronize()
        assert int(step) == it + 1
        got = tuple(n32(x[0]) for x in (P, M, Vv))
        assert not touched[row_frozen].any() and touched.any() != empty
        moved_t = touched & ~row_frozen
        moved_u = ~touched & ~row_frozen & (row_l2 > 0)
        decayed = ~touched & ~row_frozen & ~(row_l2 > 0)
        assert moved_u.any() and (moved_t.any() or empty)
        l2x2 = (F(2) * row_l2)[:, None]
        for rows_, is_touched in ((moved_t, True), (moved_u, False)):
            if not rows_.any():
                continue
            acc = sums[rows_] if is_touched else np.zeros((int(rows_.sum()), K), F)
            g = acc + l2x2[rows_] * old[0][rows_]
            check_step(h, it, cache32, cache64, tuple(x[rows_] for x in got), tuple(x[rows_] for x in old), g,
                       (layout, K, "touched" if is_touched else "swept"), exact)
        # decayed rows -- the untouched rows of the plain field: m b1 and v b2 bit for bit, the bits of p kept
        assert same_bits(got[0][decayed], old[0][decayed]), (layout, K, n_step)
        assert same_bits(got[1][decayed], old[1][decayed] * h["b1"]) and same_bits(got[2][decayed], old[2][decayed] * h["b2"])
        live_decay = live_decay or bool(decayed.any() and (old[1][decayed] != 0).any() and (got[1][decayed] != old[1][decayed]).any()
                                        and (got[2][decayed] != old[2][decayed]).any())
        # the frozen field: every bit kept
        for a, b in zip(got, old):
            assert same_bits(a[row_frozen], b[row_frozen]), (layout, K, n_step)
        assert (moved_t | moved_u | decayed | row_frozen).all()
        assert (got[0][moved_t | moved_u] != old[0][moved_t | moved_u]).any(axis=1).all()
        assert all(guards_intact(*x) for x in (P, M, Vv)), (layout, K, n_step)
        # the restatement's table step says the same (one definition of the row kinds for the host tests and these)
        (_, m_ref, v_ref), moved, dec = ref.table_step(h, ref.coefs(h, it, cache32), *old, sums, touched, row_l2, row_frozen)
        assert np.array_equal(moved, moved_t | moved_u) and np.array_equal(dec, decayed)
        assert same_bits(got[1], m_ref) and same_bits(got[2], v_ref)
        # the cache after the step
        cache64 = ref.coefs64(h, it, cache64)["msn"]
        assert (float(cache) == 0.0) if start else abs(float(cache) - cache64) <= 8 * (it + 1) * 2.0 ** -24 * cache64
    assert live_decay                   # a row with history in m and v was among the decayed ones (also on the empty batch)
    return tuple(n32(x[0]).copy() for x in (P, M, Vv)) + (n32(cache).copy(),)


TABLE_CASES = [(1, False), (3, False), (4, False), (16, False), (4, True), (16, True)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,mis", TABLE_CASES, ids=["K%d%s" % (k, "-slot+4B" if m else "") for k, m in TABLE_CASES])
def test_runs_and_sweep_match_keras_semantics(K, mis, bf16):
    h = ref.hyper(lr=1e-2)
    a = _run_table_steps(h, K, mis, bf16, "A", 0, 0)
    if K in (3, 4):                     # the other assignment of the fields: the swept field first, the frozen one last
        _run_table_steps(h, K, mis, bf16, "B", 0, 0)
    if mis:                             # the element-wise sweep loop gives the bits of the 16-byte one
        b = _run_table_steps(h, K, False, bf16, "A", 0, 0)
        assert all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("K,mis", [(3, False), (16, False), (16, True)], ids=["K3", "K16", "K16-slot+4B"])
def test_nadam_from_iterations_200000_is_bit_equal(K, mis, layout):
    """From iterations 200 000 with cache 0 the coefficients hold no power: p, m and v are all held to the fp32 restatement bit for
    bit, on slots with history -- touched, swept and decayed rows, runs and the merged update of three lists."""
    h = ref.hyper(lr=1e-2)
    c = ref.coefs(h, TAIL, F(0))
    assert c["mt"] == c["mt1"] == h["b1"] and c["omsn"] == c["omsx"] == c["vden"] == F(1)
    _run_table_steps(h, K, mis, False, layout, TAIL, 0)
    _run_table_steps(h, K, mis, False, layout, TAIL, 3)


def test_sweep_without_a_regularised_field_still_decays():
    """field_l2 NULL: fil_embed_nadam_sweep launches all the same, and every row of the non-frozen fields that the (empty) batch did not
    touch gets m b1, v b2; p and the frozen field keep their bits."""
    lib = _lib.load()
    h = ref.hyper(lr=1e-2)
    _, fz, offs, _, row_frozen, _ = _field_maps("A")
    for K, mis in ((4, False), (3, False), (16, True)):
        P, M, Vv = _table_state(K, mis, TAIL, 11)
        old = tuple(n32(x[0]).copy() for x in (P, M, Vv))
        stamp = torch.zeros(V, dtype=torch.int32, device="cuda")
        step = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        cache = torch.full((1,), 0.3, device="cuda")
        ch = c_hyper(h, cache)
        check(lib.fil_embed_nadam_sweep(ptr(P[0]), ptr(M[0]), ptr(Vv[0]), ptr(stamp), V, K, ptr(offs), None, ptr(fz), 3, ptr(step), NADAM,
                                        ctypes.addressof(ch), stream_ptr()), "fil_embed_nadam_sweep")
        torch.cuda.synchronize()
        got = tuple(n32(x[0]) for x in (P, M, Vv))
        live = ~row_frozen
        assert same_bits(got[0], old[0]) and same_bits(got[1][row_frozen], old[1][row_frozen])
        assert same_bits(got[2][row_frozen], old[2][row_frozen])
        assert same_bits(got[1][live], old[1][live] * h["b1"]) and same_bits(got[2][live], old[2][live] * h["b2"])
        assert int(step) == 5 and float(cache) == float(F(0.3)) and all(guards_intact(*x) for x in (P, M, Vv))


# ---------------------------------------------------------------------------------------------------- 4. merged against runs
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [3, 16])
def test_merged_update_w1_is_runs_and_w3_sums_in_list_order(K, bf16):
    """W = 1 merged (cap greater than the count) gives the bits of the runs update on the same records; W = 3 with an empty middle list
    is checked against the lists' sums added in list order."""
    h = ref.hyper(lr=1e-2)
    runs = _run_table_steps(h, K, False, bf16, "A", 0, 0)
    w1 = _run_table_steps(h, K, False, bf16, "A", 0, 1)
    assert all(same_bits(x, y) for x, y in zip(runs, w1))
    _run_table_steps(h, K, False, bf16, "A", 0, 3)


# ---------------------------------------------------------------------------------------------------- the Python layer on SparseEmbed
VOCAB = [5, 1, 40]
KE = 4


def _layer(out_dtype=None):
    info = models.make_sparse_info(VOCAB, embed_dim=KE)
    info = [i._replace(emb_reg=(L2 if f == 2 else 0.0), is_trainable=(f != 1)) for f, i in enumerate(info)]
    torch.manual_seed(3)
    return SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs", out_dtype=out_dtype)


def _slots(opt, p):
    return tuple(opt.state[p][k] for k in ref.SLOT_NAMES)


# ---------------------------------------------------------------------------------------------------- 5. the exchange
@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_w1_exchange_is_bitwise_the_one_gpu_update(out_dtype):
    """force_exchange=True at world size 1 (compact + merged) against the one-GPU path (runs), three steps, the first batch the
    largest: table, slots and cache bit-equal after every step."""
    rng = np.random.default_rng(5)
    batches = [(_batch_ids(s)[:B - 16 * s], rng.standard_normal((B - 16 * s, 3, KE)) * 0.1) for s in range(3)]
    runs = []
    for force in (False, True):
        emb = _layer(out_dtype)
        emb(torch.tensor(batches[0][0], device="cuda"))
        opt = optim.Nadam([emb.embeddings], learning_rate=1e-2, force_exchange=force)
        traj = []
        for idx, g in batches:
            opt.zero_grad()
            block = emb(torch.tensor(idx, device="cuda"))
            block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
            assert emb.embeddings.grad is None and emb.embeddings._fil_pending_runs is not None
            opt.step()
            traj.append((emb.embeddings.detach().clone(),) + tuple(s.clone() for s in _slots(opt, emb.embeddings))
                        + (torch.tensor(opt.momentum_cache),))
        assert (emb.embeddings in opt._xbuf) == force and opt.iterations == 3 and bool(opt._stamps)
        runs.append(traj)
    for s, (a, b) in enumerate(zip(*runs)):
        assert len(a) == len(b) == 4
        for x, y in zip(a, b):
            assert torch.equal(x, y), s
    assert not torch.equal(runs[0][0][0], runs[0][2][0]) and 0 < float(runs[0][2][3]) < 0.1


# ---------------------------------------------------------------------------------------------------- 6. capture
def test_one_eager_step_plus_three_replays_equal_four_eager_steps():
    """A step over a runs table (regularised, plain and frozen fields) and two dense parameters: one eager step and three replays of
    the captured step against four eager steps, every parameter and slot bit-equal, momentum_cache and iterations too (device against
    device: the coefficients change from replay to replay and are formed from the device's counter and cache)."""
    rng = np.random.default_rng(6)
    batches = [(torch.tensor(_batch_ids(s % 3), device="cuda"), torch.tensor(rng.standard_normal(B), dtype=torch.float32, device="cuda"))
               for s in range(4)]

    def make():
        emb = _layer()
        emb(batches[0][0])
        torch.manual_seed(9)
        w = torch.nn.Parameter(torch.randn(3, KE, device="cuda") * 0.3)
        b = torch.nn.Parameter(torch.zeros(1, device="cuda"))
        opt = optim.Nadam([emb.embeddings, w, b], learning_rate=1e-2)

        def step(idx, y):
            opt.zero_grad()
            pred = (emb(idx) * w).sum((1, 2)) + b
            loss = (pred - y).square().mean()
            loss.backward()
            opt.step()
            return loss.detach()
        return (emb.embeddings, w, b), opt, step

    pe, opt_e, step_e = make()
    caches = []
    for bt in batches:
        step_e(*bt)
        caches.append(opt_e.momentum_cache)
    assert 1 > caches[0] > caches[1] > caches[2] > caches[3] > 0
    pc, opt_c, step_c = make()
    init = [p.detach().clone() for p in pc]

    def restore():
        with torch.no_grad():
            for p, v in zip(pc, init):
                p.copy_(v)
        opt_c.reset_()

    captured = capture.capture_step(step_c, *batches[0], restore=restore)
    torch.cuda.synchronize()
    assert opt_c.iterations == 0 and opt_c.momentum_cache == 1.0
    step_c(*batches[0])                                     # one eager step
    assert opt_c.momentum_cache == caches[0]
    for s, bt in enumerate(batches[1:], 2):                 # three replays
        captured(*bt)
        torch.cuda.synchronize()
        assert opt_c.iterations == s and opt_c.momentum_cache == caches[s - 1]
    assert opt_e.iterations == opt_c.iterations == 4 and opt_e.momentum_cache == opt_c.momentum_cache
    for i, (a, b) in enumerate(zip(pe, pc)):
        assert torch.equal(a, b), i
        assert set(opt_e.state[a]) == set(opt_c.state[b]) == set(ref.SLOT_NAMES)
        for k in opt_e.state[a]:
            assert torch.equal(opt_e.state[a][k], opt_c.state[b][k]), (i, k)
    assert not torch.equal(pe[0], init[0])


# ---------------------------------------------------------------------------------------------------- 7. state
def test_state_dict_round_trip_and_reset():
    emb = _layer()
    idx = torch.tensor(_batch_ids(0), device="cuda")
    emb(idx)
    dense = torch.nn.Parameter(torch.randn(37, device="cuda"))
    opt = optim.Nadam([emb.embeddings, dense], learning_rate=1e-2)

    def one(o):
        o.zero_grad()
        (emb(idx).square().sum() + dense.square().sum()).backward()
        o.step()

    start = [emb.embeddings.detach().clone(), dense.detach().clone()]
    one(opt)
    first = [emb.embeddings.detach().clone(), dense.detach().clone()]
    cache1 = opt.momentum_cache
    one(opt)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["iterations"] == 2 and set(sd["state"][0]) == set(ref.SLOT_NAMES)
    assert sd["momentum_cache"] == opt.momentum_cache and 0 < sd["momentum_cache"] < cache1 < 1
    h = ref.hyper(lr=1e-2)
    np.testing.assert_allclose(sd["momentum_cache"], ref.coefs64(h, 1, ref.coefs64(h, 0, 1.0)["msn"])["msn"], rtol=16 * 2.0 ** -24)
    snap = [emb.embeddings.detach().clone(), dense.detach().clone()]
    one(opt)
    after = [emb.embeddings.detach().clone(), dense.detach().clone()]
    with torch.no_grad():
        emb.embeddings.copy_(snap[0])
        dense.copy_(snap[1])
    opt2 = optim.Nadam([emb.embeddings, dense], learning_rate=1e-2)
    opt2.load_state_dict(sd)
    assert opt2.iterations == 2 and opt2.momentum_cache == sd["momentum_cache"]
    one(opt2)                                               # the third step's coefficients, from the loaded counter and cache
    assert opt2.iterations == 3 and torch.equal(emb.embeddings, after[0]) and torch.equal(dense, after[1])
    assert opt2.momentum_cache == opt.momentum_cache
    # a state_dict without the cache (another optimizer's): 1.0
    sd0 = copy.deepcopy(sd)
    del sd0["momentum_cache"]
    opt3 = optim.Nadam([emb.embeddings, dense], learning_rate=1e-2)
    opt3.load_state_dict(sd0)
    assert opt3.momentum_cache == 1.0 and opt3.iterations == 2
    # reset_: the never-stepped state, in place -- one step from the initial weights repeats the first step of the run above
    with torch.no_grad():
        emb.embeddings.copy_(start[0])
        dense.copy_(start[1])
    store = {k: v.data_ptr() for k, v in opt2.state[emb.embeddings].items()}
    word = next(iter(opt2._cache.values())).data_ptr()
    opt2.reset_()
    st = opt2.state[emb.embeddings]
    assert opt2.iterations == 0 and opt2.momentum_cache == 1.0 and {k: v.data_ptr() for k, v in st.items()} == store
    assert next(iter(opt2._cache.values())).data_ptr() == word
    assert all(not v.any() for v in st.values()) and all(not s.any() for s in opt2._stamps.values())
    one(opt2)
    assert torch.equal(emb.embeddings, first[0]) and torch.equal(dense, first[1]) and opt2.momentum_cache == cache1


def test_a_table_in_adams_deferred_mode_is_refused():
    emb = _layer()
    idx = torch.tensor(_batch_ids(0), device="cuda")
    emb(idx)
    adam = optim.Adam([emb.embeddings], sweep_period=4)
    opt = optim.Nadam([emb.embeddings])
    emb(idx).square().sum().backward()
    with pytest.raises(_lib.FilError, match="deferred mode"):
        opt.step()
    del adam
