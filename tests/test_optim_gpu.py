"""Keras' Adam on the GPU (include/fil.h O1, ml_function_amd/optim.py): fil_adam_multi against a float64 ApplyAdam, the fused table
update (fil_embed_adam_runs + fil_embed_adam_sweep) against a float64 dense Keras Adam on the dense table gradient, the lazy mode,
a whole XDeepFM step against the float64 oracle graph, HIP-graph capture, and a 200-step training run against torch's Adam."""
import copy

import numpy as np
import pytest
import torch

from ml_function_amd import capture, losses, models, optim
from ml_function_amd.layers import SparseEmbed
from ml_function_amd.layers.base import collect_regularization_loss
from oracle import graph

pytestmark = pytest.mark.gpu

# Keras' hyper-parameters are float32 variables: the float64 reference takes their float32 values (1 - beta_2 of the float32 0.999 is
# 1.3e-5 away from 0.001 -- every v carries that)
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))


def keras_adam64(p, g, m, v, t):
    """TensorFlow's ApplyAdam (Keras 'adam', TF 2.1) in float64 on float32 hyper-parameters; t = the 1-based step.  Returns (p, m, v)."""
    alpha = LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    m = m + (g - m) * (1 - B1)
    v = v + (g * g - v) * (1 - B2)
    return p - m * alpha / (np.sqrt(v) + EPS), m, v


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def c64(t):
    return t.detach().cpu().double().numpy()


# ---------------------------------------------------------------------------------------------------- 1. dense tensors, one launch
SIZES = [(1,), (3,), (4,), (1023,), (4096,), (65537,), (1521, 128)]


def test_adam_multi_matches_keras_apply_adam():
    """5 steps over 7 tensors of awkward sizes (one with no gradient): every step against ApplyAdam in float64 from the same state
    (updates within 1e-4 norm-relative), and the whole trajectory against a float64 one (parameters within 1e-6)."""
    rng = np.random.default_rng(0)
    ps = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s) * 0.5, dtype=torch.float32, device="cuda")) for s in SIZES]
    none = 2                                                    # this one never has a gradient
    opt = optim.Adam(ps)
    traj = [(c64(p), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    start = [c64(p) for p in ps]
    for t in range(1, 6):
        grads = [None if i == none else rng.standard_normal(s) * 10.0 ** rng.integers(-6, 0) for i, s in enumerate(SIZES)]
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float32, device="cuda")
        before = [(c64(p), c64(opt.state[p]["m"]) if "m" in opt.state[p] else np.zeros(p.shape),
                   c64(opt.state[p]["v"]) if "v" in opt.state[p] else np.zeros(p.shape)) for p in ps]
        opt.step()
        assert opt.iterations == t
        for i, (p, g) in enumerate(zip(ps, grads)):
            if g is None:
                continue
            g32 = c64(p.grad)
            want, wm, wv = keras_adam64(*before[i][:1], g32, before[i][1], before[i][2], t)
            assert nrel(c64(p) - before[i][0], want - before[i][0]) < 1e-4, (SIZES[i], t)
            assert nrel(c64(opt.state[p]["m"]), wm) < 1e-6 and nrel(c64(opt.state[p]["v"]), wv) < 1e-5, (SIZES[i], t)
            traj[i] = keras_adam64(traj[i][0], g32, traj[i][1], traj[i][2], t)
            assert nrel(c64(p), traj[i][0]) < 1e-6, (SIZES[i], t)
    assert np.array_equal(c64(ps[none]), start[none]) and "m" not in opt.state[ps[none]]


def test_adam_multi_is_not_torch_adam_for_tiny_gradients():
    """|g| ~ 1e-6 is the order of epsilon: Keras' placement (eps on the uncorrected sqrt(v)) moves the parameter far less than
    torch's on the first step -- proof that it is Keras' form that runs."""
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(4096).astype(np.float32)
    g = (rng.standard_normal(4096) * 1e-6).astype(np.float32)
    a = torch.nn.Parameter(torch.tensor(p0, device="cuda"))
    b = torch.nn.Parameter(torch.tensor(p0, device="cuda"))
    a.grad, b.grad = torch.tensor(g, device="cuda"), torch.tensor(g, device="cuda")
    optim.Adam([a]).step()
    torch.optim.Adam([b], lr=LR, betas=(B1, B2), eps=EPS).step()
    ua, ub = c64(a) - p0, c64(b) - p0
    want, _, _ = keras_adam64(p0.astype(np.float64), g.astype(np.float64), 0.0, 0.0, 1)
    assert nrel(ua, want - p0) < 1e-3
    assert nrel(ua, ub) > 0.5, nrel(ua, ub)


# ---------------------------------------------------------------------------------------------------- 2. the tables, in place
VOCAB = [50, 200, 30, 1000, 7, 64]
L2 = {0: 1e-2, 3: 3e-3}              # two regularised fields
FROZEN = 2                           # one frozen field
K, BT = 16, 512


def _table_layer(out_dtype):
    info = models.make_sparse_info(VOCAB, embed_dim=K)
    info = [i._replace(emb_reg=L2.get(f, 0.0), is_trainable=(f != FROZEN)) for f, i in enumerate(info)]
    torch.manual_seed(3)
    emb = SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs", out_dtype=out_dtype)
    return emb


def _table_batches(steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        idx = np.stack([np.minimum(rng.zipf(1.2, BT) - 1, v - 1) for v in VOCAB], 1)          # heavy duplication
        bad = rng.random(idx.shape) < 0.02                                                   # out-of-range ids (dropped)
        idx[bad] = np.array(VOCAB)[np.nonzero(bad)[1]] + 3
        idx[rng.random(idx.shape) < 0.01] = -1
        g = rng.standard_normal((BT, len(VOCAB), K)) * 1e-3
        out.append((torch.tensor(idx, device="cuda"), g))
    return out


def _dense_grad64(idx, g, offs, p64):
    """The dense table gradient the reference's autograd would build, float64: sum of the rows' gradients + 2 l2 p on the
    regularised fields; frozen fields and out-of-range ids contribute nothing."""
    G = np.zeros_like(p64)
    for f, v in enumerate(VOCAB):
        if f == FROZEN:
            continue
        ok = (idx[:, f] >= 0) & (idx[:, f] < v)
        np.add.at(G, offs[f] + idx[ok, f], g[ok, f])
    for f, lam in L2.items():
        G[offs[f]:offs[f] + VOCAB[f]] += 2 * lam * p64[offs[f]:offs[f] + VOCAB[f]]
    return G


def _touched(idx, offs):
    rows = set()
    for f, v in enumerate(VOCAB):
        if f != FROZEN:
            rows.update((offs[f] + i) for i in idx[:, f] if 0 <= i < v)
    return np.array(sorted(rows))


def _run_table(out_dtype, lazy, batches, check):
    emb = _table_layer(out_dtype)
    emb(batches[0][0])                                                   # build
    opt = optim.Adam([emb.embeddings], lazy_tables=lazy)
    offs = emb.offsets.cpu().numpy()
    frozen_rows = np.arange(offs[FROZEN], offs[FROZEN] + VOCAB[FROZEN])
    m64 = np.zeros(emb.embeddings.shape)
    v64 = np.zeros(emb.embeddings.shape)
    for t, (idx, g) in enumerate(batches, 1):
        opt.zero_grad()
        block = emb(idx)
        gt = torch.tensor(g, dtype=block.dtype, device="cuda")
        block.backward(gt)
        assert emb.embeddings.grad is None and emb.embeddings._fil_pending_runs is not None
        p_old = c64(emb.embeddings)
        st = opt.state[emb.embeddings]
        m_old = c64(st["m"]) if "m" in st else m64
        v_old = c64(st["v"]) if "v" in st else v64
        opt.step()
        assert emb.embeddings._fil_pending_runs is None
        if not check:
            continue
        p_new, m_new, v_new = c64(emb.embeddings), c64(st["m"]), c64(st["v"])
        G = _dense_grad64(idx.cpu().numpy(), c64(gt), offs, p_old)
        want_p, want_m, want_v = keras_adam64(p_old, G, m_old, v_old, t)
        live = np.setdiff1d(np.arange(p_old.shape[0]), frozen_rows)
        touched = _touched(idx.cpu().numpy(), offs)
        rows = touched if lazy else live
        assert nrel(p_new[rows], want_p[rows]) < 1e-6, t
        assert nrel(p_new[rows] - p_old[rows], want_p[rows] - p_old[rows]) < 1e-4, t
        assert nrel(m_new[rows], want_m[rows]) < 1e-5 and nrel(v_new[rows], want_v[rows]) < 1e-5, t
        # frozen field: never touched by anything
        assert np.array_equal(p_new[frozen_rows], p_old[frozen_rows]) and not m_new[frozen_rows].any()
        untouched = np.setdiff1d(live, touched)
        assert untouched.size > 0
        if lazy:        # LazyAdam: untouched rows and their moments bitwise as they were
            assert np.array_equal(p_new[untouched], p_old[untouched])
            assert np.array_equal(m_new[untouched], m_old[untouched]) and np.array_equal(v_new[untouched], v_old[untouched])
        else:           # Keras: untouched rows of the l2 fields move (l2), and after step 1 the others do too (momentum)
            l2_rows = np.concatenate([np.arange(offs[f], offs[f] + VOCAB[f]) for f in L2])
            moved = p_new != p_old
            assert moved[np.intersect1d(untouched, l2_rows)].any(axis=1).all()
            if t > 1:
                had_m = untouched[np.abs(m_old[untouched]).max(1) > 0]
                assert had_m.size > 0 and moved[had_m].any(axis=1).all()
    assert opt.iterations == len(batches)
    return emb.embeddings.detach().clone(), opt.state[emb.embeddings]["m"].clone(), opt.state[emb.embeddings]["v"].clone()


@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_table_keras_mode_matches_dense_keras_adam(out_dtype):
    batches = _table_batches(3, seed=11)
    a = _run_table(out_dtype, False, batches, check=True)
    b = _run_table(out_dtype, False, batches, check=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))          # run 2 bitwise equal to run 1


@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_table_lazy_mode_matches_lazy_adam(out_dtype):
    batches = _table_batches(3, seed=12)
    a = _run_table(out_dtype, True, batches, check=True)
    b = _run_table(out_dtype, True, batches, check=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_second_pending_record_raises_and_zero_grad_clears():
    emb = _table_layer(None)
    idx = _table_batches(1, seed=3)[0][0]
    emb(idx).sum().backward()
    with pytest.raises(Exception, match="pending"):
        emb(idx).sum().backward()
    opt = optim.Adam([emb.embeddings])
    opt.zero_grad()
    assert emb.embeddings._fil_pending_runs is None
    emb(idx).sum().backward()
    opt.step()
    assert opt.iterations == 1


def test_state_dict_round_trip():
    emb = _table_layer(None)
    idx = _table_batches(1, seed=4)[0][0]
    emb(idx)
    dense = torch.nn.Parameter(torch.randn(37, device="cuda"))
    opt = optim.Adam([emb.embeddings, dense])
    for _ in range(2):
        opt.zero_grad()
        (emb(idx).square().sum() + dense.square().sum()).backward()
        opt.step()
    sd = copy.deepcopy(opt.state_dict())      # (torch hands out the live moment tensors)
    assert sd["iterations"] == 2
    snap = [emb.embeddings.detach().clone(), dense.detach().clone()]
    opt.zero_grad()
    (emb(idx).square().sum() + dense.square().sum()).backward()
    opt.step()
    after_a = [emb.embeddings.detach().clone(), dense.detach().clone()]
    with torch.no_grad():
        emb.embeddings.copy_(snap[0])
        dense.copy_(snap[1])
    opt2 = optim.Adam([emb.embeddings, dense])
    opt2.load_state_dict(sd)
    assert opt2.iterations == 2
    opt2.zero_grad()
    (emb(idx).square().sum() + dense.square().sum()).backward()
    opt2.step()
    assert opt2.iterations == 3
    assert torch.equal(emb.embeddings, after_a[0]) and torch.equal(dense, after_a[1])


# ---------------------------------------------------------------------------------------------------- 3. a whole model step
def _xdeepfm(vocab, K, table_grad):
    info = [i._replace(emb_reg=1e-3) for i in models.make_sparse_info(vocab, embed_dim=K)]
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad=table_grad)
    return fi, models.CTRModel(fi, models.XDeepFM(conv_size=[16, 12], hidden_units=[32, 16])).cuda()


def _inputs(B, n_dense, vocab, seed=0):
    rng = np.random.default_rng(seed)
    dense = torch.tensor(rng.random((B, n_dense)), dtype=torch.float32, device="cuda")
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device="cuda")
    return dense, idx


def test_xdeepfm_keras_adam_steps_match_oracle():
    """The model of test_xdeepfm_adam_step_matches_oracle with tableGrad="runs" and optim.Adam, 3 steps against the float64 oracle
    graph with Keras' Adam: every parameter after each step within 1e-5, each step's update within 1e-3."""
    torch.manual_seed(2)
    vocab = [7, 11, 5, 13, 3, 17]
    B, K = 48, 8
    fi, model = _xdeepfm(vocab, K, "runs")
    dense, idx = _inputs(B, 3, vocab, seed=9)
    model(dense, idx)
    names = [n for n, _ in model.named_parameters()]
    key = {id(p): n for n, p in model.named_parameters()}
    b = model.body
    offs, loff = fi.sparse_embed.offsets.cpu(), fi.linear_embed.offsets.cpu()
    P = {n: p.detach().cpu().double().clone() for n, p in model.named_parameters()}
    M = {n: torch.zeros_like(v) for n, v in P.items()}
    V = {n: torch.zeros_like(v) for n, v in P.items()}
    opt = optim.Adam(model.parameters())
    rng = np.random.default_rng(10)
    for t in range(1, 4):
        dense, idx = _inputs(B, 3, vocab, seed=20 + t)
        y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")
        # ---- oracle, float64
        Q = {n: v.clone().requires_grad_() for n, v in P.items()}
        O = lambda p: Q[key[id(p)]]
        emb, lin = O(fi.sparse_embed.embeddings), O(fi.linear_embed.embeddings)
        sparse = graph.sparse_embed([emb[offs[f]:offs[f] + vocab[f]] for f in range(len(vocab))],
                                    [idx[:, f:f + 1].cpu() for f in range(len(vocab))])
        linear = sum(lin[loff[f]:loff[f] + vocab[f]][idx[:, f].cpu()] for f in range(len(vocab)))
        cin_out = graph.cin(torch.cat(sparse, 1), [O(w)[0] for w in b.cin.conv_kernels], [O(v) for v in b.cin.conv_biases],
                            O(b.cin.logit_kernel), O(b.cin.logit_bias))
        x = graph.stack_layer([dense.cpu().double()[:, i:i + 1] for i in range(3)] + sparse)
        for h in b.dnn.hidden_list:
            yy = x @ O(h.dense.kernel) + O(h.dense.bias)
            x = torch.relu(x + yy) if x.shape == yy.shape else torch.relu(yy)
        p64 = torch.sigmoid(linear + cin_out + x @ O(b.dnn.logit_layer.kernel) + O(b.dnn.logit_layer.bias))[:, 0]
        y64 = y.cpu().double()
        reg64 = sum(1e-3 * emb[offs[f]:offs[f] + vocab[f]].square().sum() for f in range(len(vocab)))
        loss64 = -(y64 * torch.log(p64) + (1 - y64) * torch.log(1 - p64)).mean() + reg64
        loss64.backward()
        old = dict(P)
        for n in names:
            g = Q[n].grad if Q[n].grad is not None else torch.zeros_like(P[n])
            p_, m_, v_ = keras_adam64(P[n].numpy(), g.numpy(), M[n].numpy(), V[n].numpy(), t)
            P[n], M[n], V[n] = torch.tensor(p_), torch.tensor(m_), torch.tensor(v_)
        # ---- HIP path
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
                assert float((got - P[n]).abs().max() / P[n].abs().max()) < 1e-5, (n, t)
            upd, upd64 = got - prev[n], P[n] - old[n]
            if upd64.abs().max() > 0:
                assert float((upd - upd64).abs().max() / upd64.abs().max()) < 1e-3, (n, t)
    assert opt.iterations == 3


# ---------------------------------------------------------------------------------------------------- 4. HIP-graph capture
@pytest.mark.parametrize("lazy", [False, True], ids=["keras", "lazy"])
def test_captured_step_replays_bitwise_like_eager(lazy):
    vocab = [7, 11, 5, 13, 3, 17]
    B, K = 256, 8
    batches = []
    rng = np.random.default_rng(5)
    for s in range(3):
        d, i = _inputs(B, 3, vocab, seed=40 + s)
        batches.append((d, i, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        torch.manual_seed(7)
        fi, model = _xdeepfm(vocab, K, "runs")
        model(batches[0][0], batches[0][1])
        opt = optim.Adam(model.parameters(), lazy_tables=lazy)

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


# ---------------------------------------------------------------------------------------------------- 5. training sanity
def test_xdeepfm_trains_with_keras_adam_like_torch_adam():
    """XDeepFM 3x128 at B = 4096 for 200 steps on the data of test_bf16_xdeepfm_trains_like_f32: optim.Adam (Keras mode, tables
    in place) ends within 0.005 held-out BCE of torch's Adam."""
    from ml_function_amd import metrics
    from tests.test_cin_bf16 import _teacher_batches, _train
    rng0 = np.random.default_rng(7)
    vocab = [int(v) for v in np.exp(rng0.uniform(np.log(10), np.log(2e4), 26))]
    B, Kd = 4096, 16
    batches = _teacher_batches(200, B, vocab, seed=1)
    held = _teacher_batches(1, 4 * B, vocab, seed=2)[0]
    bce_t, auc_t = _train("f32", batches, held, vocab, Kd)
    torch.manual_seed(0)
    info = models.make_sparse_info(vocab, embed_dim=Kd)
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad="runs")
    model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128], hidden_units=[64, 32], precision="f32")).cuda()
    model(batches[0][0], batches[0][1])
    opt = optim.Adam(model.parameters())
    for dense, idx, y in batches:
        opt.zero_grad()
        p = model(dense, idx)[:, 0]
        losses.binary_crossentropy(p, y, eps=1e-6).backward()
        opt.step()
    with torch.no_grad():
        p = model(held[0], held[1])[:, 0]
        bce_k, auc_k = float(losses.binary_crossentropy(p, held[2], eps=1e-6)), metrics.auc(held[2], p)
    print("held-out BCE / AUC after 200 steps: torch Adam %.5f / %.4f, Keras Adam %.5f / %.4f" % (bce_t, auc_t, bce_k, auc_k))
    assert auc_k > 0.6
    assert abs(bce_k - bce_t) <= 0.005
