"""Pooled multi-valued fields on the GPU (include/fil.h N3: fil_embed_bag_fwd / _row_ids / _bwd_prep, functional.embed_bag,
layers.BagEmbed, models.FeatureInput(seqInfo=...)) against the numpy restatement tests/embed_bag_ref.py.

Nothing below the model test has a tolerance.  The forward adds in fp32 in slot order and divides once, as the restatement does, so
the two agree bit for bit.  The gradient is a record (g / d, perm = bag of every sorted slot, sorted row ids) handed to the run sums
and the fused optimizers that the one-id gather already uses: with integer-valued rows the sums are exact and must equal int64
sums; with any rows they must equal, bit for bit, what the one-id gather computes on the expanded one-hot form (F T virtual fields
over the same tables, padding as id -1) -- both sort the same slots stably, so runs and their order coincide."""
import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FIL_F32, FilError, check, ptr, stream_ptr
from tests import embed_bag_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0x7FC12345                      # a quiet NaN with a payload: compared as bits
VOCAB = [50, 47, 53, 41, 59]               # V ~ 50 per field
SHAPES = [(5, 1), (32, 2), (13, 5), (257, 3)]          # (B, F): B F = 5, 64, 65, 3 * 257 bags
KS = [3, 4, 16, 36, 256]
TS = [1, 2, 7, 8, 9, 19, 50]


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def layout(F):
    sizes = np.array(VOCAB[:F], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return offsets, sizes


def make_ids(B, F, T, sizes, rng, pad_share=0.3):
    """Random bags (ids in [1, V), a share of the slots padding, anywhere in the row) with the constructed ones written over them:
    bag 0 all padding; bag 1 full; bag 2 padding in the middle; bag 3 one id repeated; bag 4 a negative id and ids >= V beside
    padding (min(T, 3) out-of-range slots, the only ones of the batch).  Id V - 1 of the last field (the table's last row) goes into
    the last bag, or with five bags in all into the full one.  B F >= 5 everywhere."""
    idx = np.stack([rng.integers(1, sizes[f], (B, T)) for f in range(F)], 1)
    idx[rng.random((B, F, T)) < pad_share] = 0
    flat = idx.reshape(B * F, T)
    v = lambda bag: int(sizes[bag % F])
    flat[0] = 0
    flat[1] = rng.integers(1, v(1), T)
    flat[2] = rng.integers(1, v(2), T)
    flat[2, 1:T - 1] = 0
    flat[3] = int(rng.integers(1, v(3)))
    flat[4] = 0
    flat[4, 0] = -int(rng.integers(1, 5))
    if T >= 2:
        flat[4, T - 1] = v(4)
    if T >= 3:
        flat[4, 1] = v(4) + 7
    last = B * F - 1 if B * F > 5 else 1
    assert last % F == F - 1
    flat[last, T // 2] = sizes[F - 1] - 1
    return idx


def bag_forward(table, offsets, sizes, idx, combiner, padding_id):
    """Fn.embed_bag through the C ABI: (out, count, oob) as numpy; the guard floats around `out` are checked here."""
    B, F, T = idx.shape
    K = table.shape[1]
    buf = torch.full((B * F * K + 2 * K,), SENTINEL, dtype=torch.int32, device="cuda")
    out = buf[K:K + B * F * K].view(torch.float32)
    count = torch.full((B * F + 2,), -7, dtype=torch.int32, device="cuda")
    oob = torch.zeros((), dtype=torch.int32, device="cuda")
    pad = _lib.FIL_BAG_NO_PAD if padding_id is None else padding_id
    check(_lib.load().fil_embed_bag_fwd(ptr(table), ptr(offsets), ptr(sizes), ptr(idx), pad, out.data_ptr(), count[1:].data_ptr(), ptr(oob),
                                        B, F, T, K, Fn.BAG_COMBINERS[combiner], stream_ptr()), "fil_embed_bag_fwd")
    bits = buf.cpu().numpy()
    assert (bits[:K] == SENTINEL).all() and (bits[-K:] == SENTINEL).all(), "a store outside the output block"
    c = count.cpu().numpy()
    assert c[0] == -7 and c[-1] == -7, "a store outside count"
    return bits[K:-K].view(f32).reshape(B, F, K), c[1:-1].reshape(B, F), int(oob)


@pytest.fixture(scope="module")
def tables():
    """One random table per (F, K), made once and never modified: the forward cases only read it."""
    made = {}

    def get(F, K):
        if (F, K) not in made:
            _, sizes = layout(F)
            t = np.random.default_rng(100 * F + K).standard_normal((int(sizes.sum()), K)).astype(f32)
            made[(F, K)] = (t, dev(t))
        return made[(F, K)]
    return get


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
def test_forward_is_bit_equal_to_the_sequential_restatement(K, T, tables):
    """Every bag count and combiner at this (K, T), with padding id 0 and without a padding id: output bits, count = n and the exact
    number of out-of-range slots (padding not among them)."""
    rng = np.random.default_rng(1000 * K + T)
    for B, F in SHAPES:
        offsets, sizes = layout(F)
        table, table_d = tables(F, K)
        idx = make_ids(B, F, T, sizes, rng)
        live, bad = ref.masks(idx, sizes, 0)
        n = live.reshape(B * F, T).sum(1)
        assert n[0] == 0 and n[1] == T and bad.reshape(B * F, T)[4].sum() == min(T, 3) and bad.sum() == min(T, 3)
        assert (idx[:, F - 1] == sizes[-1] - 1).any() and (T < 3 or (idx.reshape(B * F, T)[2, 1] == 0 and n[2] == 2))
        off_d, sizes_d, idx_d = dev(offsets), dev(sizes), dev(idx)
        for padding_id in (0, None):
            for combiner in ref.COMBINERS:
                want, want_n, want_oob = ref.forward(table, offsets, sizes, idx, combiner, padding_id)
                got, got_n, got_oob = bag_forward(table_d, off_d, sizes_d, idx_d, combiner, padding_id)
                what = (B, F, combiner, padding_id)
                assert np.array_equal(got_n, want_n), what
                assert got_oob == want_oob == min(T, 3), what
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (what, np.argwhere(got != want)[:4])
            if padding_id is None:      # id 0 was read as a row: the all-"padding" bag is T times row 0 of its field
                assert want_n[0, 0] == T and np.array_equal(got[0, 0], want[0, 0]) and np.abs(got[0, 0]).max() > 0


def test_forward_grid_loop_takes_a_second_trip():
    """More (bag, lane-group) items than the launch's grid cap has threads: the grid-stride loop runs again for the tail."""
    K, T, F = 256, 2, 3
    threads = _lib.FIL_BAG_MAX_BLOCKS * 256
    KQ = (K + 3) // 4
    B = threads // KQ // F + 1                  # the first batch size whose items do not fit one trip
    assert B * F * KQ > threads >= (B - 1) * F * KQ and B * F * KQ < 2 * threads
    offsets, sizes = layout(F)
    rng = np.random.default_rng(7)
    table = rng.standard_normal((int(sizes.sum()), K)).astype(f32)
    idx = make_ids(B, F, T, sizes, rng)
    want, want_n, want_oob = ref.forward(table, offsets, sizes, idx, "mean", 0)
    got, got_n, got_oob = bag_forward(dev(table), dev(offsets), dev(sizes), dev(idx), "mean", 0)
    assert np.array_equal(got_n, want_n) and got_oob == want_oob
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    tail = (threads // KQ) // F                 # the bags of the second trip are really there
    assert np.abs(want[tail:]).max() > 0


@pytest.mark.parametrize("K", [3, 16])
def test_single_slot_bags_equal_the_one_id_gather(K):
    """T = 1 without a padding id: output and dense table gradient torch.equal to embed_gather's."""
    B, F = 65, 3
    offsets, sizes = layout(F)
    rng = np.random.default_rng(K)
    idx = np.stack([rng.integers(0, v, B) for v in sizes], 1)
    g = dev(rng.standard_normal((B, F, K)), torch.float32)
    t0 = torch.randn(int(sizes.sum()), K, device="cuda")
    for combiner in ref.COMBINERS:
        a, b = t0.clone().requires_grad_(), t0.clone().requires_grad_()
        out = Fn.embed_bag(a, dev(offsets), dev(idx[:, :, None]), sizes=dev(sizes), combiner=combiner, padding_id=None)
        want = Fn.embed_gather(b, dev(offsets), dev(idx), sizes=dev(sizes))
        assert torch.equal(out, want)
        out.backward(g)
        want.backward(g)
        assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0


def int_grad(rng, shape):
    """Integers in [-64, 64] without 0 (tests/test_embed_runs_gpu.py): fp32 sums of them are exact in any order."""
    return (rng.integers(1, 65, size=shape) * rng.choice(np.array([-1, 1]), size=shape)).astype(np.int64)


def bag_record(offsets, sizes, frozen, idx, g, count, combiner, padding_id=0):
    """The gradient record through the C ABI, as functional.embed_bag's backward builds it: (gs, perm, sorted_ids)."""
    lib = _lib.load()
    B, F, T = idx.shape
    K = g.shape[-1]
    pad = _lib.FIL_BAG_NO_PAD if padding_id is None else padding_id
    row_ids = torch.empty(B * F * T, dtype=torch.int64, device="cuda")
    check(lib.fil_embed_bag_row_ids(ptr(offsets), ptr(sizes), ptr(frozen), ptr(idx), pad, ptr(row_ids), B, F, T, stream_ptr()), "row_ids")
    sorted_ids, slot_perm = torch.sort(row_ids, stable=True)
    gs = None if combiner == "sum" else torch.full_like(g, float("nan"))
    perm = torch.full_like(slot_perm, -1)
    check(lib.fil_embed_bag_bwd_prep(ptr(g), ptr(count), ptr(slot_perm), ptr(gs), ptr(perm), B, F, T, K, Fn.BAG_COMBINERS[combiner],
                                     stream_ptr()), "bwd_prep")
    assert torch.equal(perm, slot_perm // T)
    return row_ids, (g if gs is None else gs), perm, sorted_ids


@pytest.mark.parametrize("K,T", [(3, 7), (16, 50), (36, 9), (256, 2)])
def test_dense_gradient_of_the_sum_equals_int64_sums(K, T):
    """Integer-valued g and combiner sum: every touched row equals the int64 sum exactly; a frozen field's rows, every field's row 0
    (the padding id) and the sentinel rows before and after the table are never written.  The slots' row ids and the record are
    checked on the way, and the autograd path gives the same table with zeros in place of the untouched sentinels."""
    B, F = 257, 3
    offsets, sizes = layout(F)
    V = int(sizes.sum())
    frozen = np.array([0, 1, 0], np.uint8)
    rng = np.random.default_rng(K * 100 + T)
    idx = make_ids(B, F, T, sizes, rng)
    g = int_grad(rng, (B, F, K))
    want, touched = ref.table_grad(V, offsets, sizes, idx, g, frozen=frozen, dtype=np.int64)
    assert not touched[offsets].any() and not touched[offsets[1]:offsets[2]].any() and touched[V - 1] and touched.sum() > 60
    off_d, sizes_d, frozen_d, idx_d, g_d = dev(offsets), dev(sizes), dev(frozen), dev(idx), dev(g, torch.float32)
    live, _ = ref.masks(idx, sizes, 0)
    count = dev(live.sum(2), torch.int32)
    row_ids, gs, perm, sorted_ids = bag_record(off_d, sizes_d, frozen_d, idx_d, g_d, count, "sum")
    want_ids = np.where(live & (frozen == 0).reshape(1, F, 1), idx + offsets.reshape(1, F, 1), -1)
    assert np.array_equal(row_ids.cpu().numpy(), want_ids.reshape(-1))
    buf = torch.full((V + 2, K), SENTINEL, dtype=torch.int32, device="cuda")
    check(_lib.load().fil_embed_run_sum_dt(ptr(gs), ptr(perm), ptr(sorted_ids), buf[1:].data_ptr(), B * F * T, K, FIL_F32, stream_ptr()),
          "fil_embed_run_sum_dt")
    bits = buf.cpu().numpy()
    assert (bits[0] == SENTINEL).all() and (bits[-1] == SENTINEL).all(), "a store outside the table"
    assert (bits[1:-1][~touched] == SENTINEL).all(), "a row that no live slot names was written"
    assert np.array_equal(bits[1:-1].view(f32)[touched].astype(np.int64), want[touched])
    table = torch.zeros(V, K, device="cuda", requires_grad=True)
    Fn.embed_bag(table, off_d, idx_d, sizes=sizes_d, combiner="sum", frozen=frozen_d).backward(g_d)
    assert np.array_equal(table.grad.cpu().numpy().astype(np.int64), want)


def onehot_gradient(V, K, e):
    """Dense table gradient of the one-id gather on the expanded form."""
    table = torch.zeros(V, K, device="cuda", requires_grad=True)
    out = Fn.embed_gather(table, dev(e["offsets"]), dev(e["ids"]), sizes=dev(e["sizes"]), frozen=None if e["frozen"] is None else dev(e["frozen"]))
    out.backward(dev(e["g"]))
    return table.grad


@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
@pytest.mark.parametrize("K,T", [(3, 7), (16, 19), (36, 8), (256, 2)])
def test_dense_gradient_equals_the_one_id_gather_on_the_expanded_form(K, T, combiner):
    """Any n: the bag's dense gradient is torch.equal to embed_gather's on the expanded one-hot form fed g_exp[b, f T + t] = g[b,f] / d
    (the restatement's fp32 division).  A frozen field's rows and every row 0 stay zero."""
    B, F = 65, 3
    offsets, sizes = layout(F)
    V = int(sizes.sum())
    frozen = np.array([0, 0, 1], np.uint8)
    rng = np.random.default_rng(K + T)
    idx = make_ids(B, F, T, sizes, rng)
    g = rng.standard_normal((B, F, K)).astype(f32)
    _, count, _ = ref.forward(np.zeros((V, K), f32), offsets, sizes, idx, combiner)
    assert count.min() == 0 and count.max() == T and len(np.unique(count)) >= 3
    e = ref.expanded(offsets, sizes, idx, ref.scaled_grad(g, count, combiner), frozen=frozen)
    want = onehot_gradient(V, K, e)
    table = torch.zeros(V, K, device="cuda", requires_grad=True)
    Fn.embed_bag(table, dev(offsets), dev(idx), sizes=dev(sizes), combiner=combiner, frozen=dev(frozen)).backward(dev(g))
    assert torch.equal(table.grad, want)
    got = table.grad.cpu().numpy()
    assert not got[offsets].any() and not got[offsets[2]:].any() and np.abs(got[:offsets[2]]).max() > 0
    # against float64 sums, at the textbook bound of a fp32 sum of the at most B T terms of a row: gamma(n - 1) sum |terms|
    w64, _ = ref.table_grad(V, offsets, sizes, idx, e["g"][:, ::T], frozen=frozen)
    a64, _ = ref.table_grad(V, offsets, sizes, idx, np.abs(e["g"][:, ::T]), frozen=frozen)
    assert (np.abs(got - w64) <= B * T * np.finfo(f32).eps * a64).all()


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_sparse_gradient(combiner):
    """sparse_grad=True: rows sorted, unique and without the -1 bucket; densified, the dense gradient bit for bit."""
    B, F, T, K = 65, 3, 9, 16
    offsets, sizes = layout(F)
    V = int(sizes.sum())
    rng = np.random.default_rng(3)
    idx = make_ids(B, F, T, sizes, rng)
    g = dev(rng.standard_normal((B, F, K)), torch.float32)
    grads = []
    for sparse in (False, True):
        table = torch.zeros(V, K, device="cuda", requires_grad=True)
        Fn.embed_bag(table, dev(offsets), dev(idx), sizes=dev(sizes), combiner=combiner, sparse_grad=sparse).backward(g)
        grads.append(table.grad)
    dense, sp = grads
    assert sp.is_sparse and not dense.is_sparse
    rows = sp._indices()[0].cpu().numpy()
    _, touched = ref.table_grad(V, offsets, sizes, idx, np.zeros((B, F, K)))
    assert rows.min() >= 0 and (np.diff(rows) > 0).all() and np.array_equal(rows, np.nonzero(touched)[0])
    assert torch.equal(sp.to_dense(), dense)


# ------------------------------------------------------------------------------------------------------------ runs mode
RB, RF, RT, RK = 33, 3, 5, 8
OPTIMIZERS = {
    "adam": lambda p, **kw: optim.Adam(p, learning_rate=1e-2, **kw),
    "amsgrad": lambda p, **kw: optim.Adam(p, learning_rate=1e-2, amsgrad=True, **kw),
    "adagrad": lambda p, **kw: optim.Adagrad(p, learning_rate=1e-2, **kw),
    "sgd-momentum": lambda p, **kw: optim.SGD(p, learning_rate=1e-2, momentum=0.9, **kw),
    "adamax": lambda p, **kw: optim.Adamax(p, learning_rate=1e-2, **kw),
    "nadam": lambda p, **kw: optim.Nadam(p, learning_rate=1e-2, **kw),
}


def seq_info(K=RK, F=RF, T=RT):
    """F pooled fields; field 1 alone is regularised."""
    return [i._replace(emb_reg=0.01 if n == 1 else 0.0) for n, i in enumerate(models.make_seq_info(VOCAB[:F], T, embed_dim=K))]


def built(layer):
    layer._build_device = torch.device("cuda")
    layer.build(None)
    layer.built = True
    return layer


def expanded_onehot(bag, T):
    """The one-hot SparseEmbed(grad_mode="runs") over the expanded form of a built BagEmbed: the same table values, and F T virtual
    fields (offsets, sizes, field_l2 repeated T times) that share the F tables."""
    emb = built(layers.SparseEmbed(bag.sparse_info, use_flatten=False, packed=True, grad_mode="runs"))
    with torch.no_grad():
        emb.embeddings.copy_(bag.embeddings)
    emb.offsets = bag.offsets.repeat_interleave(T)
    emb.sizes = bag.sizes.repeat_interleave(T)
    emb.field_l2 = bag.field_l2.repeat_interleave(T)
    emb._layout_key = (tuple(emb.sizes.tolist()), None)
    return emb


def slots(opt, p):
    return [opt.state[p][k] for k in opt._SLOTS]


def two_steps(name, combiner, force_exchange=False):
    """Two steps of optimizer `name` on a BagEmbed(grad_mode="runs") table and on the one-hot table over the expanded form: table
    and every slot torch.equal after each step."""
    rng = np.random.default_rng(11)
    _, sizes = layout(RF)
    bag = built(layers.BagEmbed(seq_info(), combiner=combiner, packed=True, grad_mode="runs"))
    assert bag.field_l2.tolist() == [0.0, f32(0.01), 0.0] and bag.embeddings._fil_runs_table
    hot = expanded_onehot(bag, RT)
    opts = [OPTIMIZERS[name]([emb.embeddings], force_exchange=force_exchange) for emb in (bag, hot)]
    start = bag.embeddings.detach().clone()
    for step in range(2):
        idx = make_ids(RB, RF, RT, sizes, rng)
        g = rng.standard_normal((RB, RF, RK)).astype(f32)
        count = ref.masks(idx, sizes, 0)[0].sum(2)
        e = ref.expanded(None, None, idx, ref.scaled_grad(g, count, combiner))
        bag(dev(idx)).backward(dev(g))
        hot(dev(e["ids"])).backward(dev(e["g"]))
        for emb in (bag, hot):
            assert emb.embeddings.grad is None and emb.embeddings._fil_pending_runs["R"] == RB * RF * RT
        for o in opts:
            o.step()
        assert bag.embeddings._fil_pending_runs is None
        assert torch.equal(bag.embeddings, hot.embeddings), (combiner, step)
        for a, b in zip(slots(opts[0], bag.embeddings), slots(opts[1], hot.embeddings)):
            assert torch.equal(a, b), (combiner, step)
    assert not torch.equal(bag.embeddings, start)


@pytest.mark.parametrize("combiner", ref.COMBINERS)
@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_runs_mode_equals_the_one_hot_table_under_every_optimizer(name, combiner):
    two_steps(name, combiner)


def test_runs_mode_through_the_exchange_path_at_world_size_one():
    """force_exchange=True: the record goes through fil_embed_runs_compact and the merged update instead of the runs update."""
    two_steps("adam", "mean", force_exchange=True)


def test_captured_step_equals_the_eager_one():
    """Forward + backward + optim.Adagrad.step captured with capture_step and replayed on three id batches that differ in their
    bags' lengths: the table after every replay equals the eager run's bit for bit."""
    rng = np.random.default_rng(21)
    _, sizes = layout(RF)
    batches = [(dev(make_ids(RB, RF, RT, sizes, rng, pad_share=share)), dev(rng.standard_normal((RB, RF, RK)), torch.float32))
               for share in (0.3, 0.0, 0.7)]

    def make():
        bag = built(layers.BagEmbed(seq_info(), combiner="mean", packed=True, grad_mode="runs"))
        opt = optim.Adagrad([bag.embeddings], learning_rate=1e-2)

        def step(idx, g):
            bag(idx).backward(g)
            opt.step()
        return bag, opt, step

    eager, _, step_e = make()
    init = eager.embeddings.detach().clone()
    traj = []
    for bt in batches:
        step_e(*bt)
        traj.append(eager.embeddings.detach().clone())
    bag, opt, step_c = make()
    assert torch.equal(bag.embeddings, init)            # (the layers' seeded initialisation)

    def restore():              # the warm-up runs are real steps
        with torch.no_grad():
            bag.embeddings.copy_(init)
        opt.reset_()

    captured = capture.capture_step(step_c, *batches[0], restore=restore)
    for bt, want in zip(batches, traj):
        captured(*bt)
        torch.cuda.synchronize()
        assert torch.equal(bag.embeddings, want)
    assert not torch.equal(traj[0], traj[1]) and not torch.equal(traj[1], traj[2])


def test_repeats_are_bit_identical():
    B, F, T, K = 257, 3, 19, 36
    offsets, sizes = layout(F)
    rng = np.random.default_rng(5)
    idx, g = dev(make_ids(B, F, T, sizes, rng)), dev(rng.standard_normal((B, F, K)), torch.float32)
    t0 = torch.randn(int(sizes.sum()), K, device="cuda")
    runs = []
    for _ in range(2):
        table = t0.clone().requires_grad_()
        out = Fn.embed_bag(table, dev(offsets), idx, sizes=dev(sizes), combiner="sqrtn")
        out.backward(g)
        runs.append((out.detach().clone(), table.grad.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


def test_deferred_table_is_refused():
    bag = built(layers.BagEmbed(seq_info(), grad_mode="runs"))
    opt = optim.Adam([bag.embeddings], sweep_period=4)
    assert optim.deferred_state(bag.embeddings) is not None
    with pytest.raises(FilError, match="deferred"):
        bag(torch.zeros(4, RF, RT, dtype=torch.int64, device="cuda"))
    del opt


# ------------------------------------------------------------------------------------------------------------ the model
def rel(a, b):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def pooled64(table, offsets, sizes, idx, combiner="mean"):
    """The torch restatement in float64: gather of the padded block, mask, sum, divide."""
    live = (idx != 0) & (idx >= 0) & (idx < sizes.view(1, -1, 1))
    rows = table[(idx.clamp(min=0) + offsets.view(1, -1, 1)) * live]
    s = (rows * live.unsqueeze(-1)).sum(2)
    n = live.sum(2, keepdim=True).clamp(min=1).double()
    return s / (n if combiner == "mean" else n.sqrt() if combiner == "sqrtn" else 1.0)


@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
def test_model_with_pooled_fields_matches_the_torch_restatement(combiner):
    """CTRModel(FeatureInput(one-id fields, dense columns, two pooled fields, linear terms), DeepFM()) at B = 64, T = 5: output and both
    bag tables' gradients against the same body fed an InputFeature whose pooled embeddings come from the float64 torch restatement,
    at the project's 1e-5 relative bar (fp32 against float64)."""
    torch.manual_seed(3)
    B, T, K = 64, 5, 8
    rng = np.random.default_rng(9)
    vocab, seq_vocab = [7, 11, 5], [50, 47]
    fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), denseInfo=[models.denseFea("I1", None), models.denseFea("I2", None)],
                             seqInfo=models.make_seq_info(seq_vocab, T, embed_dim=K), seqCombiner=combiner, useLinear=True)
    model = models.CTRModel(fi, models.DeepFM(hidden_units=[32, 16])).cuda()
    dense = dev(rng.random((B, 2)), torch.float32)
    sparse = dev(np.stack([rng.integers(0, v, B) for v in vocab], 1))
    seq_np = make_ids(B, 2, T, np.array(seq_vocab), rng)
    seq_np[ref.masks(seq_np, seq_vocab, 0)[1]] = 1                  # (every id in range: check_ids comes last)
    seq = dev(seq_np)
    w = dev(rng.standard_normal((B, 2)), torch.float32)
    out = model(dense, sparse, seq)
    assert out.shape == (B, 2)
    feats = fi((dense, sparse, seq))
    assert len(feats.sparse_embed) == 5 and len(feats.linear_embed) == 5 and feats.seq_info is fi.seq_info and len(feats.seq_inputs) == 2
    assert feats.sparse_embed[4].shape == (B, 1, K) and feats.linear_embed[4].shape == (B, 1, 1) and tuple(feats.seq_inputs[1].shape) == (B, T)
    (out * w).sum().backward()
    got = [fi.seq_embed.embeddings.grad.clone(), fi.seq_linear_embed.embeddings.grad.clone()]
    # the same body on an InputFeature whose pooled fields are the restatement's
    t64 = [fi.seq_embed.embeddings.detach().double().requires_grad_(), fi.seq_linear_embed.embeddings.detach().double().requires_grad_()]
    emb = pooled64(t64[0], fi.seq_embed.offsets, fi.seq_embed.sizes, seq, combiner)
    lin = pooled64(t64[1], fi.seq_linear_embed.offsets, fi.seq_linear_embed.sizes, seq, combiner)
    plain = models.InputFeature(fi.dense_info, fi.sparse_info, fi.seq_info, [dense[:, i:i + 1] for i in range(2)], [], [],
                                fi.linear_embed(sparse) + [lin[:, f:f + 1].float() for f in range(2)],
                                fi.sparse_embed(sparse) + [emb[:, f:f + 1].float() for f in range(2)], [None, None])
    want = model.body(plain)
    assert rel(out, want) < 1e-5, rel(out, want)
    (want * w).sum().backward()
    for a, b in zip(got, t64):
        assert float(b.grad.abs().max()) > 0 and rel(a, b.grad) < 1e-5, rel(a, b.grad)
        assert float(a[0].abs().max()) == 0.0                       # row 0 is the padding id: never updated
    # check_ids=True raises like SparseEmbed, naming the sample and the field
    strict = layers.BagEmbed(fi.seq_info, check_ids=True)
    strict(seq)
    seq[9, 1, 2] = seq_vocab[1]
    with pytest.raises(IndexError, match=r"sample 9, field S2, slot 2 \(id 47, word_size 47\)"):
        strict(seq)
