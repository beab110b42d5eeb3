"""The data-parallel runs exchange of Keras' Adam on the GPU (include/fil.h O1: fil_embed_runs_compact, fil_embed_adam_merged;
ml_function_amd/optim.py, dp.exchange_runs): the compaction against numpy and bitwise against the dense run sums, W = 1 bitwise
equal to the one-GPU update, W simulated shards against the float64 Keras Adam of the full batch, HIP-graph replay, no host sync
after the first step, and real process groups (tests/dp_adam_worker.py)."""
import os

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, models, optim
from ml_function_amd._lib import check, ptr, stream_ptr
from ml_function_amd.layers import SparseEmbed

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))
I64MAX = np.iinfo(np.int64).max
VOCAB = [50, 200, 30, 1000, 7, 64]
L2 = {0: 1e-2, 3: 3e-3}
FROZEN = 2


def keras_adam64(p, g, m, v, t):
    """TensorFlow's ApplyAdam (Keras 'adam') in float64 on float32 hyper-parameters (as in test_optim_gpu.py)."""
    alpha = LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    m = m + (g - m) * (1 - B1)
    v = v + (g * g - v) * (1 - B2)
    return p - m * alpha / (np.sqrt(v) + EPS), m, v


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def c64(t):
    return t.detach().cpu().double().numpy()


def _layer(K, out_dtype=None, l2=True, vocab=VOCAB, seed=3):
    info = models.make_sparse_info(vocab, embed_dim=K)
    info = [i._replace(emb_reg=L2.get(f, 0.0) if l2 else 0.0, is_trainable=(f != FROZEN)) for f, i in enumerate(info)]
    torch.manual_seed(seed)
    return SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs", out_dtype=out_dtype)


def _batch(B, K, seed, vocab=VOCAB):
    rng = np.random.default_rng(seed)
    idx = np.stack([np.minimum(rng.zipf(1.2, B) - 1, v - 1) for v in vocab], 1)     # heavy duplication: long and short runs
    bad = rng.random(idx.shape) < 0.02                                                # out-of-range ids (dropped)
    idx[bad] = np.array(vocab)[np.nonzero(bad)[1]] + 3
    idx[rng.random(idx.shape) < 0.01] = -1
    return idx, rng.standard_normal((B, len(vocab), K)) * 1e-3


def _record(emb, idx, g):
    """The runs record of one backward (taken off the table, so several shards' records can coexist)."""
    block = emb(torch.tensor(idx, device="cuda"))
    block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
    rec = emb.embeddings._fil_pending_runs
    emb.embeddings._fil_pending_runs = None
    return rec


def _compact(rec, K, cap):
    ids = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
    values = torch.full((cap * K,), float("nan"), dtype=torch.float32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(1, optim.runs_compact_workspace_bytes(rec["R"])), dtype=torch.uint8, device="cuda")
    optim.runs_compact(rec, K, ids, values, count, cap, ws)
    return ids, values, count


# ---------------------------------------------------------------------------------------------------- 1. compaction
@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,K", [(512, 16), (300, 1), (2048, 8), (37, 5), (4096, 32)])
def test_compaction_matches_numpy_and_dense_run_sums(out_dtype, B, K):
    emb = _layer(K, out_dtype)
    idx, g = _batch(B, K, seed=B + K)
    rec = _record(emb, idx, g)
    R = rec["R"]
    cap = R + 37
    ids, values, count = _compact(rec, K, cap)
    sid = rec["sorted_ids"].cpu().numpy()
    want = np.unique(sid[sid >= 0])
    n = int(count.item())
    assert n == want.size > 0
    got = ids.cpu().numpy()
    assert np.array_equal(got[:n], want) and (got[n:] == I64MAX).all()
    # the numpy view of the same rows: the table's ids of every live, in-range entry
    offs = emb.offsets.cpu().numpy()
    rows = set()
    for f, v in enumerate(VOCAB):
        if f != FROZEN:
            rows.update(int(offs[f] + i) for i in idx[:, f] if 0 <= i < v)
    assert np.array_equal(want, np.array(sorted(rows)))
    # every compact row bitwise equal to the dense gradient's row (fil_embed_run_sum_dt)
    V = emb.embeddings.shape[0]
    dense = torch.zeros((V, K), dtype=torch.float32, device="cuda")
    check(_lib.load().fil_embed_run_sum_dt(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), ptr(dense), R, K, rec["g_dtype"],
                                           stream_ptr()), "fil_embed_run_sum_dt")
    vals = values.view(cap, K)[:n]
    assert torch.equal(vals, dense[torch.tensor(want, device="cuda")])
    # deterministic: a second compaction gives the same bits
    ids2, values2, count2 = _compact(rec, K, cap)
    assert torch.equal(ids2, ids) and torch.equal(values2.view(cap, K)[:n], vals) and torch.equal(count2, count)


def test_compaction_of_an_all_skipped_record():
    """Every entry -1 (ids out of range): count 0, every slot padding."""
    emb = _layer(4)
    idx = np.full((16, len(VOCAB)), -1, dtype=np.int64)
    rec = _record(emb, idx, np.ones((16, len(VOCAB), 4)))
    ids, _, count = _compact(rec, 4, rec["R"])
    assert int(count.item()) == 0 and (ids.cpu().numpy() == I64MAX).all()


# ---------------------------------------------------------------------------------------------------- 2. W = 1 == today's update
@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("l2", [True, False], ids=["l2", "nol2"])
@pytest.mark.parametrize("lazy", [False, True], ids=["keras", "lazy"])
def test_w1_exchange_is_bitwise_the_one_gpu_update(lazy, l2, out_dtype):
    K = 16
    batches = [_batch(512 - 64 * s, K, seed=60 + s) for s in range(3)]       # (later batches shorter: they fit the first cap)
    runs = []
    for force in (False, True):
        emb = _layer(K, out_dtype, l2=l2)
        emb(torch.tensor(batches[0][0], device="cuda"))
        opt = optim.Adam([emb.embeddings], lazy_tables=lazy, force_exchange=force)
        traj = []
        for idx, g in batches:
            opt.zero_grad()
            block = emb(torch.tensor(idx, device="cuda"))
            block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
            opt.step()
            st = opt.state[emb.embeddings]
            traj.append((emb.embeddings.detach().clone(), st["m"].clone(), st["v"].clone()))
        assert (emb.embeddings in opt._xbuf) == force
        runs.append(traj)
    for s, (a, b) in enumerate(zip(*runs)):
        for x, y, what in zip(a, b, ("table", "m", "v")):
            assert torch.equal(x, y), (s, what)


def test_record_larger_than_the_agreed_capacity_raises():
    K = 8
    emb = _layer(K)
    emb(torch.tensor(_batch(64, K, 1)[0], device="cuda"))
    opt = optim.Adam([emb.embeddings], force_exchange=True)
    for B in (64, 128):
        opt.zero_grad()
        idx, g = _batch(B, K, seed=B)
        emb(torch.tensor(idx, device="cuda")).backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
        if B == 64:
            opt.step()
        else:
            with pytest.raises(_lib.FilError, match="capacity"):
                opt.step()


# ---------------------------------------------------------------------------------------------------- 3. W shards vs float64
def _dense_grad64(idx, g, offs, p64):
    G = np.zeros_like(p64)
    for f, v in enumerate(VOCAB):
        if f == FROZEN:
            continue
        ok = (idx[:, f] >= 0) & (idx[:, f] < v)
        np.add.at(G, offs[f] + idx[ok, f], g[ok, f])
    for f, lam in L2.items():
        G[offs[f]:offs[f] + VOCAB[f]] += 2 * lam * p64[offs[f]:offs[f] + VOCAB[f]]
    return G


def _gather(recs, K):
    """Every shard compacted into its slot of one gathered buffer (what the all-gather builds on every rank)."""
    W, cap = len(recs), max(r["R"] for r in recs)
    ids = torch.empty(W * cap, dtype=torch.int64, device="cuda")
    values = torch.empty(W * cap * K, dtype=torch.float32, device="cuda")
    counts = torch.empty(W, dtype=torch.int64, device="cuda")
    for w, rec in enumerate(recs):
        ws = torch.empty(max(1, optim.runs_compact_workspace_bytes(rec["R"])), dtype=torch.uint8, device="cuda")
        optim.runs_compact(rec, K, ids[w * cap:(w + 1) * cap], values[w * cap * K:(w + 1) * cap * K], counts[w:w + 1], cap, ws)
    return ids, values, counts, cap


def _sweep(lib, emb, m, v, stamp, t, rec):
    V, K = emb.embeddings.shape
    check(lib.fil_embed_adam_sweep(ptr(emb.embeddings), ptr(m), ptr(v), ptr(stamp), V, K, ptr(rec["offsets"]), ptr(rec["field_l2"]),
                                   ptr(rec["frozen"]), rec["F"], ptr(t), LR, B1, B2, EPS, stream_ptr()), "fil_embed_adam_sweep")


@pytest.mark.parametrize("lazy", [False, True], ids=["keras", "lazy"])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_sharded_merged_update_matches_float64_full_batch(W, lazy):
    K, per = 16, 256
    lib = _lib.load()
    emb = _layer(K)
    ref = _layer(K)                                   # the same table, updated from the FULL batch's record (one-GPU path)
    for layer in (emb, ref):                          # build (no backward: no record)
        layer(torch.tensor(_batch(8, K, seed=0)[0], device="cuda"))
    offs = emb.offsets.cpu().numpy()
    V = emb.embeddings.shape[0]
    frozen_rows = np.arange(offs[FROZEN], offs[FROZEN] + VOCAB[FROZEN])
    live = np.setdiff1d(np.arange(V), frozen_rows)
    state = [torch.zeros((V, K), device="cuda") for _ in range(4)]
    m, v, rm, rv = state
    stamp, rstamp = (torch.zeros(V, dtype=torch.int32, device="cuda") for _ in range(2))
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    for step in (1, 2):
        idx, g = _batch(W * per, K, seed=100 * W + step)
        shards = [_record(emb, idx[w * per:(w + 1) * per], g[w * per:(w + 1) * per]) for w in range(W)]
        full = _record(ref, idx, g)
        ids, values, counts, cap = _gather(shards, K)
        lists = [set(ids[w * cap:w * cap + int(counts[w])].tolist()) for w in range(W)]
        union = np.array(sorted(set.union(*lists)))
        shared = set.intersection(*lists[:2])
        assert shared and (lists[0] - set().union(*lists[1:]))          # rows shared between shards and rows of one shard only
        p_old, m_old, v_old = c64(emb.embeddings), c64(m), c64(v)
        optim.adam_merged(ids, values, counts, W, cap, emb.offsets, shards[0]["field_l2"], emb.embeddings, m, v, stamp, t, LR, B1, B2,
                          EPS, lazy=lazy)
        check(lib.fil_embed_adam_runs(ptr(full["g"]), ptr(full["perm"]), ptr(full["sorted_ids"]), full["R"], K, full["g_dtype"],
                                      full["F"], ptr(full["field_l2"]), ptr(ref.embeddings), ptr(rm), ptr(rv), ptr(rstamp), ptr(t),
                                      LR, B1, B2, EPS, _lib.FIL_ADAM_LAZY if lazy else _lib.FIL_ADAM_KERAS, stream_ptr()),
              "fil_embed_adam_runs")
        if not lazy:
            _sweep(lib, emb, m, v, stamp, t, shards[0])
            _sweep(lib, ref, rm, rv, rstamp, t, full)
        t += 1
        p_new, m_new, v_new = c64(emb.embeddings), c64(m), c64(v)
        G = _dense_grad64(idx, c64(torch.tensor(g, dtype=torch.float32)), offs, p_old)
        want_p, want_m, want_v = keras_adam64(p_old, G, m_old, v_old, step)
        rows = union if lazy else live
        assert nrel(p_new[rows], want_p[rows]) < 1e-6, step
        assert nrel(p_new[rows] - p_old[rows], want_p[rows] - p_old[rows]) < 1e-4, step
        assert nrel(m_new[rows], want_m[rows]) < 1e-5 and nrel(v_new[rows], want_v[rows]) < 1e-5, step
        assert np.array_equal(p_new[frozen_rows], p_old[frozen_rows]) and not m_new[frozen_rows].any()
        outside = np.setdiff1d(live, union)
        assert outside.size > 0
        if lazy:        # rows outside the union: bit-untouched
            assert np.array_equal(p_new[outside], p_old[outside])
            assert np.array_equal(m_new[outside], m_old[outside]) and np.array_equal(v_new[outside], v_old[outside])
        else:           # rows outside the union: exactly what the sweep does on the one-GPU path from the same state
            o = torch.tensor(outside, device="cuda")
            assert torch.equal(emb.embeddings[o], ref.embeddings[o]) and torch.equal(m[o], rm[o]) and torch.equal(v[o], rv[o])
            moved = p_new != p_old
            l2_rows = np.concatenate([np.arange(offs[f], offs[f] + VOCAB[f]) for f in L2])
            assert moved[np.intersect1d(outside, l2_rows)].any(axis=1).all()
        with torch.no_grad():       # the reference follows the sharded run (outside rows compared from the same state next step)
            ref.embeddings.copy_(emb.embeddings)
            rm.copy_(m)
            rv.copy_(v)


# ---------------------------------------------------------------------------------------------------- 4. capture, no host sync
@pytest.mark.parametrize("lazy", [False, True], ids=["keras", "lazy"])
def test_captured_compaction_and_merge_replay_bitwise(lazy):
    K, W, per = 16, 3, 512
    emb = _layer(K)
    idx, g = _batch(W * per, K, seed=77)
    shards = [_record(emb, idx[w * per:(w + 1) * per], g[w * per:(w + 1) * per]) for w in range(W)]
    V = emb.embeddings.shape[0]
    cap = max(r["R"] for r in shards)
    ids = torch.empty(W * cap, dtype=torch.int64, device="cuda")
    values = torch.empty(W * cap * K, dtype=torch.float32, device="cuda")
    counts = torch.empty(W, dtype=torch.int64, device="cuda")
    wss = [torch.empty(max(1, optim.runs_compact_workspace_bytes(r["R"])), dtype=torch.uint8, device="cuda") for r in shards]
    m, v = torch.rand((V, K), device="cuda") * 1e-3, torch.rand((V, K), device="cuda") * 1e-6
    stamp = torch.zeros(V, dtype=torch.int32, device="cuda")
    t = torch.full((1,), 4, dtype=torch.int64, device="cuda")
    init = [x.clone() for x in (emb.embeddings.detach(), m, v, stamp)]

    def body():
        for w, rec in enumerate(shards):
            optim.runs_compact(rec, K, ids[w * cap:(w + 1) * cap], values[w * cap * K:(w + 1) * cap * K], counts[w:w + 1], cap, wss[w])
        optim.adam_merged(ids, values, counts, W, cap, emb.offsets, shards[0]["field_l2"], emb.embeddings, m, v, stamp, t, LR, B1, B2,
                          EPS, lazy=lazy)

    def restore():
        with torch.no_grad():
            for x, x0 in zip((emb.embeddings, m, v, stamp), init):
                x.copy_(x0)
        ids.fill_(-1)
        values.fill_(float("nan"))
        counts.fill_(-1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in (emb.embeddings.detach(), m, v, stamp)]
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    restore()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (emb.embeddings.detach(), m, v, stamp)):
        assert torch.equal(a, b)
    assert not torch.equal(eager[0], init[0])


def test_exchange_step_after_the_first_never_synchronises():
    K = 16
    emb = _layer(K)
    dense = torch.nn.Parameter(torch.randn(33, device="cuda"))
    emb(torch.tensor(_batch(256, K, 1)[0], device="cuda"))
    opt = optim.Adam([emb.embeddings, dense], force_exchange=True)
    dense.grad = torch.ones_like(dense)
    for s in range(3):
        opt.zero_grad(set_to_none=False)        # (the dense gradient keeps its storage: its descriptor is reused)
        idx, g = _batch(256, K, seed=90 + s)
        emb(torch.tensor(idx, device="cuda")).backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
        dense.grad.fill_(1.0)
        torch.cuda.synchronize()
        if s == 0:
            opt.step()              # the first step agrees on the capacity and allocates
            continue
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert opt.iterations == 3


# ---------------------------------------------------------------------------------------------------- 5. real process groups
def _ranks(n):
    from tests.test_dp_gpu import _run_ranks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return _run_ranks([os.path.join(root, "tests", "dp_adam_worker.py")], n, timeout=240)


def test_dp_adam_worker_on_one_rank():
    r = _ranks(1)
    assert r.returncode == 0 and "DP_ADAM_OK 1" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_dp_adam_worker_on_two_ranks():
    r = _ranks(2)
    assert r.returncode == 0 and "DP_ADAM_OK 2" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
