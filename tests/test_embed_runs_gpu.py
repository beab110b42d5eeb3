"""The embedding run sums (csrc/embed_runs.h: one walk behind fil_embed_run_sum(_dt), fil_embed_adam_runs, fil_embed_runs_compact,
the deferred Adam runs kernel and fil_embed_rowopt_runs), the per-field sort and the gathers at CONSTRUCTED records: run lengths placed
at every switch of the walk (8 | 9, C, 4C, 64 ids per ballot), every run moved through every lane group and window boundary by a
skipped prefix, and row widths of every KQ = ceil(K/4) class (C = 64 / KQ not a power of two, dead lanes).

The run sums need no tolerance: the gradient rows are integers in [-64, 64] \\ {0}, exact in bf16 and fp32, and every partial sum of
up to 200 000 of them stays below 2^24, so fp32 addition is exact in any order and the kernel must equal the int64 sum bit for bit.
The only inexact comparison of the module is the textbook gamma(n - 1) bound of fp32 summation in section 3."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, models, optim
from ml_function_amd._lib import FIL_BF16, FIL_F32, check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIL_ERR_UNSUPPORTED = -4
I64MAX = np.iinfo(np.int64).max
SENTINEL = 0x7FC12345                      # a quiet NaN with a payload: compared as bits
DTYPES = [FIL_F32, FIL_BF16]
DT_IDS = ["f32", "bf16"]

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 28, 32, 33, 36, 48, 64, 65, 84, 85, 100, 128, 129, 252, 253, 256]
EVERY_PREFIX = (16, 20, 100, 256)          # these widths run every prefix 0 .. C, the others s in {0, 1, C-1, C}


def lanes(K):
    """C of embed_runs.h: rows (sorted positions) a wave takes per iteration."""
    return 64 // ((K + 3) // 4)


def run_lengths(K):
    C = lanes(K)
    raw = [1, 2, 7, 8, 9, C - 1, C, C + 1, 4 * C - 1, 4 * C, 4 * C + 1, 8 * C, 8 * C + 1, 63, 64, 65, 66, 127, 128, 129, 130, 1000, 4097]
    return sorted({n for n in raw if n > 0})


def prefixes(K):
    C = lanes(K)
    return list(range(C + 1)) if K in EVERY_PREFIX else sorted({0, 1, C - 1, C})


def with_separators(lengths, rng):
    """The lengths in a shuffled order, every two of them separated by one or two runs of 1-3 elements (as Criteo-like batches are)."""
    out = []
    for n in rng.permutation(np.asarray(lengths, np.int64)):
        out.extend(int(x) for x in rng.integers(1, 4, size=int(rng.integers(1, 3))))
        out.append(int(n))
    return out


class Record:
    """A sorted runs record built from run lengths.  Run r owns the gradient rows rows[r] (a random partition of range(R0)), in that
    order; `order` places the runs, `s` puts a prefix of s skipped (-1) entries in front whose permutation entries point at the rows
    R0 .. R0 + s - 1, so perm is a permutation of range(R) and one gradient block [R0 + max s, K] serves every prefix."""

    def __init__(self, lengths, rng):
        self.lengths = [int(n) for n in lengths]
        assert self.lengths and min(self.lengths) > 0
        self.R0 = int(sum(self.lengths))
        p = rng.permutation(self.R0)
        cuts = np.cumsum([0] + self.lengths)
        self.rows = [p[cuts[r]:cuts[r + 1]] for r in range(len(self.lengths))]
        self.rng = rng

    def layout(self, s=0, order=None, first_id=2):
        """-> sorted_ids [R], perm [R], ids [runs] (the table row of run r), V (table rows: a few that nobody touches among them --
        rows 0 and 1, holes between the runs, the two rows after the last touched one)."""
        order = list(range(len(self.lengths))) if order is None else [int(r) for r in order]
        gaps = self.rng.integers(1, 4, size=len(order))
        placed = first_id + np.cumsum(gaps) - gaps[0]
        ids = np.zeros(len(self.lengths), np.int64)
        ids[order] = placed
        sorted_ids = np.concatenate([np.full(s, -1, np.int64)] + [np.full(self.lengths[r], ids[r], np.int64) for r in order])
        perm = np.concatenate([np.arange(self.R0, self.R0 + s, dtype=np.int64)] + [self.rows[r] for r in order]).astype(np.int64)
        return sorted_ids, perm, ids, int(placed.max()) + 3


def int_grad(rng, rows, K):
    """Integers in [-64, 64] without 0: a dropped, doubled or misattributed element moves the sum by at least 1."""
    g = rng.integers(1, 65, size=(rows, K)) * rng.choice(np.array([-1, 1]), size=(rows, K))
    return g.astype(np.int64)


def int_reference(sorted_ids, perm, g, V, cache=None):
    """np.add.at on int64 over the record as the kernel sees it (sorted_ids, perm): want [V, K] and the mask of touched rows.  cache:
    the run sums of the previous call are kept while the live part of the record (run structure and permutation) is the same one --
    a skipped prefix or other ids do not change them."""
    live = sorted_ids >= 0
    rows, inv = np.unique(sorted_ids[live], return_inverse=True)
    pl = perm[live]
    if cache is not None and "sums" in cache and np.array_equal(cache["inv"], inv) and np.array_equal(cache["perm"], pl):
        sums = cache["sums"]
    else:
        sums = np.zeros((rows.size, g.shape[1]), np.int64)
        np.add.at(sums, inv, g[pl])
        if cache is not None:
            cache.update(inv=inv, perm=pl, sums=sums)
    want = np.zeros((V, g.shape[1]), np.int64)
    want[rows] = sums
    touched = np.zeros(V, bool)
    touched[rows] = True
    return want, touched


def g_tensor(g, dt):
    t = torch.tensor(np.asarray(g, np.float32), device="cuda")
    return t.bfloat16() if dt == FIL_BF16 else t


def sentinel_table(V, K):
    """[V + 2, K] of sentinel bits; rows 1 .. V are the table, rows 0 and V + 1 guards (row -1 is where a skipped entry would land)."""
    return torch.full((V + 2, K), SENTINEL, dtype=torch.int32, device="cuda")


def run_sum(sorted_ids, perm, g_t, V, K, dt, expect=0):
    """fil_embed_run_sum_dt into a sentinel-filled table -> (table as float32 [V, K], its bits [V, K]); the guard rows are checked here."""
    buf = sentinel_table(V, K)
    sid, pm = torch.tensor(sorted_ids, device="cuda"), torch.tensor(perm, device="cuda")
    rc = _lib.load().fil_embed_run_sum_dt(ptr(g_t), ptr(pm), ptr(sid), buf[1:].data_ptr(), len(sorted_ids), K, dt, stream_ptr())
    assert rc == expect, (rc, _lib.load().fil_last_error())
    bits = buf.cpu().numpy()
    assert (bits[0] == SENTINEL).all() and (bits[-1] == SENTINEL).all(), "a store outside the table (row -1 / row V)"
    return bits[1:-1].view(np.float32), bits[1:-1]


def assert_exact(got, bits, want, touched, what=""):
    stray = np.nonzero((bits != SENTINEL).any(1) & ~touched)[0]
    assert stray.size == 0, "%s: rows %s were written and belong to no run" % (what, stray[:8])
    g, w = got[touched].astype(np.float64), want[touched].astype(np.float64)
    bad = np.nonzero((g != w).any(1))[0]          # (a sentinel left in a touched row is a NaN: != everything)
    assert bad.size == 0, "%s: %d touched rows differ, first rows %s: got %s want %s" % (
        what, bad.size, np.nonzero(touched)[0][bad[:4]], g[bad[0]][:8], w[bad[0]][:8])


def check_record(K, dt, lengths, prefix_list, rng):
    rec = Record(lengths, rng)
    g = int_grad(rng, rec.R0 + max(prefix_list), K)
    g_t = g_tensor(g, dt)
    cache = {}
    for s in prefix_list:
        sorted_ids, perm, _, V = rec.layout(s)
        want, touched = int_reference(sorted_ids, perm, g, V, cache)
        assert touched.sum() == len(lengths) and not touched[V - 1] and not touched[0]
        got, bits = run_sum(sorted_ids, perm, g_t, V, K, dt)
        assert_exact(got, bits, want, touched, "K=%d s=%d R=%d" % (K, s, len(sorted_ids)))


# ------------------------------------------------------------------------------------------------ 1. run sums, exact reference
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", WIDTHS)
def test_run_sums_equal_the_int64_sums_at_every_length_and_prefix(K, dt):
    """Every run length of the list at least once in one record, shuffled, separated by runs of 1-3, behind a skipped prefix of s
    entries: touched rows equal np.add.at on int64, everything else keeps the sentinel's bits."""
    rng = np.random.default_rng(1000 + K)
    check_record(K, dt, with_separators(run_lengths(K), rng), prefixes(K), rng)


PLACE_WIDTHS = [1, 7, 12, 16, 20, 33, 100, 256]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", PLACE_WIDTHS)
def test_run_sums_at_the_ends_of_the_record(K, dt):
    """A long last run that ends at R; a run of 1 at R - 1 behind a long run; R = 1, C, C + 1 (as one run and as runs of 1); a record
    that is one run; each behind prefixes 0, 1, C - 1, C."""
    C = lanes(K)
    rng = np.random.default_rng(2000 + K)
    ss = sorted({0, 1, C - 1, C})
    for n in (8 * C + 5, 4 * C + 1, 131, 9):
        check_record(K, dt, [3, 1, 2, n], ss, rng)                  # the long run ends at R
        check_record(K, dt, [2, n, 1], ss, rng)                     # a run of 1 behind it is the last entry
        check_record(K, dt, [n], ss, rng)                           # the record is one run
    for R in sorted({1, C, C + 1}):
        check_record(K, dt, [R], ss, rng)
        check_record(K, dt, [1] * R, ss, rng)
    check_record(K, dt, [1000 + C], [0, C], rng)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", [1, 16, 20, 256])
def test_run_sums_of_an_all_skipped_record_store_nothing(K, dt):
    C = lanes(K)
    rng = np.random.default_rng(K)
    for R in (1, C, 2 * C + 3, 700):
        g_t = g_tensor(int_grad(rng, R, K), dt)
        _, bits = run_sum(np.full(R, -1, np.int64), rng.permutation(R).astype(np.int64), g_t, 6, K, dt)
        assert (bits == SENTINEL).all()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_run_sums_refuse_k_257_and_leave_the_table_alone(dt):
    rng = np.random.default_rng(257)
    rec = Record([1, 9, 3, 70], rng)
    sorted_ids, perm, _, V = rec.layout()
    _, bits = run_sum(sorted_ids, perm, g_tensor(int_grad(rng, rec.R0, 257), dt), V, 257, dt, expect=FIL_ERR_UNSUPPORTED)
    assert (bits == SENTINEL).all()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,R", [(256, 40000), (64, 140000)])
def test_run_sums_second_trip_of_the_grid_loop(K, R, dt):
    """The grid is capped at 8192 workgroups of 4 waves: positions from 32768 C on belong to a workgroup's SECOND trip of the outer
    loop.  Short runs up to there, a long run lying across position 32768 C, short and long runs behind it, the last one ending at R."""
    C = lanes(K)
    edge = 32768 * C
    assert R > edge + 4000
    rng = np.random.default_rng(K)
    lengths = []

    def filler():
        lengths.extend(int(x) for x in rng.integers(1, 4, size=64))
        lengths.append(int(rng.choice([8, 9, 4 * C + 1, 65, 130])))

    while sum(lengths) < edge - 700:
        filler()
    before = sum(lengths)
    lengths.append(1500)
    assert before < edge < before + 1500
    lengths.extend([1, 2, 9, 4 * C, 4 * C + 1, 64, 65, 129, 1000, 3, 1])
    while sum(lengths) < R - 700:
        filler()
    lengths.append(R - sum(lengths))
    assert lengths[-1] > 300 and sum(lengths) == R
    check_record(K, dt, lengths, [0, 1], rng)


# ------------------------------------------------------------------------------------------------ 2. the other consumers
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", [1, 5, 12, 16, 20, 33, 100, 256])
def test_compaction_equals_the_int64_sums(K, dt):
    """fil_embed_runs_compact on the records of section 1: ids ascending and unique, the count, values equal to the int64 reference
    (not to fil_embed_run_sum_dt, which shares the walk), slots past the count untouched."""
    C = lanes(K)
    rng = np.random.default_rng(3000 + K)
    rec = Record(with_separators(run_lengths(K), rng), rng)
    g = int_grad(rng, rec.R0 + C, K)
    g_t = g_tensor(g, dt)
    cache = {}
    for s in sorted({0, 1, C}):
        sorted_ids, perm, _, V = rec.layout(s)
        R = len(sorted_ids)
        want, touched = int_reference(sorted_ids, perm, g, V, cache)
        cap = R + 37
        ids = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
        values = torch.full((cap * K,), SENTINEL, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        ws = torch.empty(max(1, optim.runs_compact_workspace_bytes(R)), dtype=torch.uint8, device="cuda")
        r = dict(g=g_t, perm=torch.tensor(perm, device="cuda"), sorted_ids=torch.tensor(sorted_ids, device="cuda"), R=R, g_dtype=dt)
        optim.runs_compact(r, K, ids, values, count, cap, ws)
        n = int(count.item())
        rows = np.nonzero(touched)[0]
        assert n == rows.size == len(rec.lengths)
        got_ids = ids.cpu().numpy()
        assert np.array_equal(got_ids[:n], rows) and (got_ids[n:] == I64MAX).all()
        bits = values.cpu().numpy().reshape(cap, K)
        assert (bits[n:] == SENTINEL).all()
        assert np.array_equal(bits[:n].view(np.float32).astype(np.float64), want[rows].astype(np.float64)), (K, s)


SEG_WIDTHS = [1, 3, 4, 8, 12, 20, 28, 64, 129, 253, 256]        # KQ = 1, 1, 1, 2, 3, 5, 7, 16, 33, 64, 64


@pytest.mark.parametrize("outputs", ["values", "dtable", "both"])
@pytest.mark.parametrize("K", SEG_WIDTHS)
def test_segment_sum_equals_the_int64_sums(K, outputs):
    """fil_embed_segment_sum (the sparse_grad=True path): starts / rows from np.unique of the sorted ids, the skipped bucket included
    (its value row and row -1 of the table stay untouched)."""
    C = lanes(K)
    rng = np.random.default_rng(4000 + K)
    rec = Record(with_separators(run_lengths(K), rng), rng)
    g = int_grad(rng, rec.R0 + C, K)
    g_t = g_tensor(g, FIL_F32)
    cache = {}
    for s in (0, C):
        sorted_ids, perm, _, V = rec.layout(s)
        want, touched = int_reference(sorted_ids, perm, g, V, cache)
        rows, starts = np.unique(sorted_ids, return_index=True)
        starts = np.concatenate([starts, [len(sorted_ids)]]).astype(np.int64)
        U = rows.size
        values = torch.full((U, K), SENTINEL, dtype=torch.int32, device="cuda")
        buf = sentinel_table(V, K)
        pm, st, rw = (torch.tensor(a, device="cuda") for a in (perm, starts, rows))
        check(_lib.load().fil_embed_segment_sum(ptr(g_t), ptr(pm), ptr(st), ptr(rw), ptr(values) if outputs != "dtable" else None,
                                                buf[1:].data_ptr() if outputs != "values" else None, U, K, stream_ptr()),
              "fil_embed_segment_sum")
        live = rows >= 0
        assert (~live).sum() == (1 if s else 0)
        vb, tb = values.cpu().numpy(), buf.cpu().numpy()
        if outputs != "dtable":
            assert (vb[~live] == SENTINEL).all()
            assert np.array_equal(vb[live].view(np.float32).astype(np.float64), want[rows[live]].astype(np.float64)), (K, s)
        else:
            assert (vb == SENTINEL).all()
        if outputs != "values":
            assert (tb[0] == SENTINEL).all() and (tb[-1] == SENTINEL).all()
            assert_exact(tb[1:-1].view(np.float32), tb[1:-1], want, touched, "segment K=%d s=%d" % (K, s))
        else:
            assert (tb == SENTINEL).all()


@pytest.mark.parametrize("K", SEG_WIDTHS)
def test_atomic_scatter_add_equals_the_int64_sums(K):
    """fil_embed_scatter_add through embed_gather(atomic=True): integer gradients make the unordered fp32 atomics exact."""
    from ml_function_amd import functional as Fn
    rng = np.random.default_rng(5000 + K)
    vocab = [5, 300, 37, 2]
    B, F = 1031, len(vocab)
    idx = np.stack([np.minimum(rng.zipf(1.2, B) - 1, v - 1) for v in vocab], 1).astype(np.int64)
    idx[3, 0], idx[7, 3], idx[9, 1], idx[B - 1, 2] = 5, -1, 10 ** 9, 37
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    table_np = rng.integers(-99, 100, size=(sum(vocab), K)).astype(np.float32)
    table = torch.tensor(table_np, device="cuda").requires_grad_()
    cnt = torch.zeros((), dtype=torch.int32, device="cuda")
    out = Fn.embed_gather(table, torch.tensor(offs, device="cuda"), torch.tensor(idx, device="cuda"), sizes=torch.tensor(vocab, device="cuda"),
                          atomic=True, oob_count=cnt)
    ok = (idx >= 0) & (idx < np.array(vocab))
    want_out = np.where(ok[..., None], table_np[offs + np.where(ok, idx, 0)], np.float32(0)).astype(np.float32)
    assert int(cnt) == 4 and np.array_equal(out.detach().cpu().numpy(), want_out)
    g = int_grad(rng, B * F, K).reshape(B, F, K)
    out.backward(torch.tensor(g.astype(np.float32), device="cuda"))
    want = np.zeros((sum(vocab), K), np.int64)
    np.add.at(want, (offs + idx)[ok], g[ok])
    assert np.array_equal(table.grad.cpu().numpy().astype(np.float64), want.astype(np.float64))


# Run-structure invariance of the fused optimizers: one step from a record with duplicates == one step from the record in which every
# run is a single entry carrying the run's exact integer sum.  No optimizer reference needed (tests/test_optim_gpu.py and
# test_optim_rowwise_gpu.py hold those): this isolates the walk from the epilogue.
INV_VOCAB = [400, 60, 9, 700]
INV_L2 = {0: 1e-2, 3: 3e-3}
INV_FROZEN = 2


def _inv_layer(K):
    from ml_function_amd.layers import SparseEmbed
    info = models.make_sparse_info(INV_VOCAB, embed_dim=K)
    info = [i._replace(emb_reg=INV_L2.get(f, 0.0), is_trainable=(f != INV_FROZEN)) for f, i in enumerate(info)]
    torch.manual_seed(7)
    return SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs")


def _inv_batches(K, rng):
    """(idx, g) with duplicates, and the same batch collapsed: per field the distinct ids once each, carrying the integer sum of their
    rows (same field: per-field l2 and the frozen flag are unchanged); the fields' columns are padded with skipped ids to one batch size."""
    C = lanes(K)
    B, F = 900, len(INV_VOCAB)
    runs = {0: [1, 1, 2, 8, 9, 4 * C + 1, 65, 70, 130, 300, 3], 1: [9, 8, 1, 100, 500, 4 * C + 2, 66], 3: [1] * 40 + [2] * 10 + [8, 9, 129, 17]}
    idx = np.full((B, F), -1, np.int64)
    for f, lens in runs.items():
        assert sum(lens) <= B and len(lens) <= INV_VOCAB[f]
        ids = np.sort(rng.choice(INV_VOCAB[f], size=len(lens), replace=False))
        col = np.concatenate([np.repeat(ids, lens), np.full(B - sum(lens), -1 if f != 1 else INV_VOCAB[f] + 5, np.int64)])
        idx[:, f] = rng.permutation(col)
    idx[:, INV_FROZEN] = rng.integers(0, INV_VOCAB[INV_FROZEN], B)
    g = int_grad(rng, B * F, K).reshape(B, F, K)
    uniq = {f: np.unique(idx[(idx[:, f] >= 0) & (idx[:, f] < INV_VOCAB[f]), f]) for f in runs}
    assert all(uniq[f].size == len(runs[f]) for f in runs)
    B2 = max(u.size for u in uniq.values())
    idx2 = np.full((B2, F), -1, np.int64)
    g2 = int_grad(rng, B2 * F, K).reshape(B2, F, K)
    for f, u in uniq.items():
        for slot, i in zip(rng.permutation(B2)[:u.size], u):
            idx2[slot, f] = i
            g2[slot, f] = g[idx[:, f] == i, f].sum(0)
    idx2[:, INV_FROZEN] = rng.integers(0, INV_VOCAB[INV_FROZEN], B2)
    assert np.abs(g2).max() < 2 ** 24
    return (idx, g), (idx2, g2)


def _inv_make(name, p):
    if name in ("adam_keras", "adam_lazy"):
        return optim.Adam([p], lazy_tables=(name == "adam_lazy")), ("m", "v")
    if name == "adagrad":
        return optim.Adagrad([p], learning_rate=1e-2), ("accumulator",)
    return optim.Ftrl([p], learning_rate=1e-2, l1_regularization_strength=1e-3, l2_regularization_strength=1e-2,
                      l2_shrinkage_regularization_strength=1e-2), ("accumulator", "linear")


@pytest.mark.parametrize("K", [16, 13, 20])
@pytest.mark.parametrize("name", ["adam_keras", "adam_lazy", "adagrad", "ftrl"])
def test_fused_optimizers_see_a_run_as_its_sum(name, K):
    rng = np.random.default_rng(6000 + K)
    res = []
    for idx, g in _inv_batches(K, rng):
        emb = _inv_layer(K)
        emb(torch.tensor(idx, device="cuda"))                         # build
        p = emb.embeddings
        opt, slots = _inv_make(name, p)
        opt.zero_grad()
        block = emb(torch.tensor(idx, device="cuda"))
        block.backward(torch.tensor(g.astype(np.float32), device="cuda"))
        assert p.grad is None and p._fil_pending_runs is not None and p._fil_pending_runs["g_dtype"] == FIL_F32
        before = p.detach().clone()
        opt.step()
        assert not torch.equal(before, p.detach())
        res.append([p.detach().clone()] + [opt.state[p][k].clone() for k in slots])
    for what, a, b in zip(("table",) + slots, *res):                  # bitwise: table and every slot
        assert a.shape == b.shape and torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ 3. real-valued sums
U24 = 2.0 ** -24


def gamma(m):
    return m * U24 / (1.0 - m * U24)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", [7, 16, 20, 100, 256])
def test_real_sums_stay_inside_the_fp32_bound_and_do_not_depend_on_position(K, dt):
    """Standard normal rows (and the same rounded to bf16).  Against the fp64 sum of the STORED inputs every element of every run of
    n <= 130 elements satisfies |got - want| <= gamma(n - 1) sum|g_i|, gamma(m) = m u / (1 - m u), u = 2^-24: the bound of fp32
    summation in any order (so a run of 1 equals its input bit for bit), which anything narrower than fp32 accumulation breaks.  The
    sum of a run -- same elements, same order -- is bitwise the same behind every prefix 0 .. C, with other neighbours (the runs in
    another order, under other ids) and in a second call."""
    C = lanes(K)
    rng = np.random.default_rng(7000 + K)
    lengths = with_separators(run_lengths(K), rng)
    rec = Record(lengths, rng)
    g_t = g_tensor(rng.standard_normal((rec.R0 + C, K)).astype(np.float32), dt)
    g64 = g_t.float().cpu().numpy().astype(np.float64)               # what the kernel reads
    want = np.stack([g64[r].sum(0) for r in rec.rows])
    mag = np.stack([np.abs(g64[r]).sum(0) for r in rec.rows])
    n = np.array(rec.lengths)
    checked = n <= 130
    assert {x for x in run_lengths(K) if x <= 130} <= set(n[checked].tolist())
    bound = gamma(n - 1.0)[:, None] * mag
    first = None
    layouts = [(s, None) for s in range(C + 1)] + [(0, None)] + [(s, rng.permutation(len(lengths))) for s in (0, 1, C)]
    for s, order in layouts:
        sorted_ids, perm, ids_of, V = rec.layout(s, order)
        got, bits = run_sum(sorted_ids, perm, g_t, V, K, dt)
        touched = np.zeros(V, bool)
        touched[ids_of] = True
        assert (bits[~touched] == SENTINEL).all()
        if first is None:
            first = bits[ids_of]
            sums = got[ids_of]
            assert np.isfinite(sums).all()
            err = np.abs(sums.astype(np.float64) - want)
            print("K=%d %s: max (err / bound) over runs of 2..130 = %.3f" % (K, DT_IDS[dt], (err[checked & (n > 1)] / bound[checked & (n > 1)]).max()))
            assert (err[checked] <= bound[checked]).all(), "K=%d: runs of lengths %s exceed gamma(n-1) sum|g|" % (
                K, n[checked][(err[checked] > bound[checked]).any(1)][:8])
            ones = np.nonzero(n == 1)[0]
            assert ones.size > 0 and np.array_equal(sums[ones], g64[[rec.rows[r][0] for r in ones]].astype(np.float32))
        else:
            diff = np.nonzero((bits[ids_of] != first).any(1))[0]
            assert diff.size == 0, "K=%d s=%d reordered=%s: runs of lengths %s changed bits" % (K, s, order is not None, n[diff][:8])


# ------------------------------------------------------------------------------------------------ 4. the per-field sort at its key edges
SORT_B = [2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 8191]


def _top_bit_case(B, rng):
    """A layout whose fields 0 and 3 have the largest vocabulary V that still takes 32-bit composites at this B; field 0's ids sit at
    both ends of it, at every power of two and just outside."""
    bits = max(1, int(np.ceil(np.log2(B))))
    V = (0xFFFFFFFF >> bits) - 1
    top = int(np.floor(np.log2(V)))
    pool = [0, 1, V - 2, V - 1] * 4 + [V, V + 1, -1]
    for k in range(1, top + 1):
        pool += [x for x in ((1 << k) - 1, 1 << k) if x < V]
    pool = np.array(pool, np.int64)
    head = np.array([V - 1, 0, V - 2, 1, V - 1, 0, V, 1, V - 2, -1, V + 1], np.int64)
    col0 = np.concatenate([head, rng.permutation(pool), pool[rng.integers(0, pool.size, size=B)]])[:B]
    if B > head.size:
        col0 = rng.permutation(col0)
    vocab = [V, 3, 50, V]
    col3 = rng.integers(0, V, size=B)
    col3[rng.integers(0, B, size=max(1, B // 8))] = V - 1                 # duplicates of the largest id
    idx = np.stack([col0, rng.integers(0, 3, size=B), rng.integers(0, 50, size=B), col3], 1).astype(np.int64)
    return vocab, idx, V


def _check_sort(B, seed):
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    vocab, idx, V = _top_bit_case(B, rng)
    F = len(vocab)
    off = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    offsets, sizes = torch.tensor(off, device="cuda"), torch.tensor(vocab, dtype=torch.int64, device="cuda")
    frozen = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
    ids = torch.tensor(idx, device="cuda")
    want_ids, want_perm = [], []
    for f in range(F):
        ok = (idx[:, f] >= 0) & (idx[:, f] < vocab[f]) & (f != 2)
        row = np.where(ok, off[f] + idx[:, f], -1)
        order = np.argsort(row, kind="stable")
        want_ids.append(row[order])
        want_perm.append(order * F + f)
    want_ids, want_perm = np.concatenate(want_ids), np.concatenate(want_perm)
    if B >= 63:
        assert (want_ids[:B] == V - 1).sum() >= 2 and (want_ids[:B] == 0).sum() >= 2 and (want_ids[:B] == -1).sum() >= 3
    for max_vocab in (V, V + 2, 0):           # 32-bit composites at their largest vocabulary, 64-bit ones just above it, bound unknown
        s_ids = torch.full((B * F,), -99, dtype=torch.int64, device="cuda")
        perm = torch.full((B * F,), -99, dtype=torch.int64, device="cuda")
        assert lib.fil_embed_sort_fields(ptr(offsets), ptr(sizes), ptr(frozen), ptr(ids), ptr(s_ids), ptr(perm), B, F, max_vocab, stream_ptr()) == 0
        got_ids, got_perm = s_ids.cpu().numpy(), perm.cpu().numpy()
        assert np.array_equal(got_ids, want_ids), (B, max_vocab, np.nonzero(got_ids != want_ids)[0][:8])
        assert np.array_equal(got_perm, want_perm), (B, max_vocab, np.nonzero(got_perm != want_perm)[0][:8])


@pytest.mark.parametrize("B", SORT_B)
def test_sort_fields_with_the_top_key_bits_set(B):
    """fil_embed_sort_fields against np.argsort(kind="stable") of the row ids (skipped entries first) where the 32-bit composite
    (id + 1) << bits | position uses every bit: V = (0xffffffff >> bits) - 1 is the largest vocabulary the host gives 32-bit keys.  The
    same ids with max_vocab = V + 2 (64-bit composites) and 0 (unknown) must give the same arrays."""
    _check_sort(B, B)


@pytest.mark.parametrize("B", [4096, 8191])
def test_sort_fields_top_key_bits_at_the_largest_networks(B):
    _check_sort(B, 10 * B)


def test_sort_fields_all_lds_network_with_the_top_key_bits_set():
    """FIL_EMBED_SORT_LDS=1 (read once per process: a fresh child) keeps the all-LDS bitonic network at N >= 1024: B = 4096 and 8191 at
    the top-bit vocabulary, same reference."""
    env = dict(os.environ)
    env["FIL_EMBED_SORT_LDS"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_embed_runs_gpu.py::test_sort_fields_top_key_bits_at_the_largest_networks",
                        "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).strip().splitlines()[-15:])
    assert r.returncode == 0, "FIL_EMBED_SORT_LDS=1:\n%s" % tail
    assert "2 passed" in r.stdout and "no tests ran" not in r.stdout, tail


# ------------------------------------------------------------------------------------------------ 5. gather
def _gather_case(rng, B, F, K, lo, hi):
    vocab = [int(v) for v in rng.integers(lo, hi, size=F)]
    off = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    table_np = rng.standard_normal((sum(vocab), K)).astype(np.float32)
    idx = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int64)
    return vocab, off, table_np, idx


def _gather_want(vocab, off, table_np, idx):
    ok = (idx >= 0) & (idx < np.array(vocab))
    return np.where(ok[..., None], table_np[off + np.where(ok, idx, 0)], np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,B,F", [(1, 333, 5), (3, 333, 5), (4, 333, 5), (5, 4096, 26), (20, 4096, 26), (100, 333, 5), (256, 333, 5)])
def test_gather_dt_is_numpy_indexing(K, B, F, dt):
    """fil_embed_gather_dt bit-exact against NumPy indexing (bf16: the fp32 block rounded by torch), out-of-range ids counted and
    zeroed.  B F = 106 496 rows at K = 20 (5 lanes per row) and at K = 5 (a lane per element) are more than the grid cap of 2048 x 256
    threads: the second trip of the kernel's loop."""
    rng = np.random.default_rng(8000 + K)
    if B == 4096:
        assert B * F * (K // 4 if K % 4 == 0 else K) > 2048 * 256
    vocab, off, table_np, idx = _gather_case(rng, B, F, K, 2, 400)
    bad = [(3, 0, vocab[0]), (7, F - 1, -1), (9, 1, 10 ** 9), (B - 1, F - 1, vocab[F - 1] + 1)]
    for b, f, v in bad:
        idx[b, f] = v
    want = _gather_want(vocab, off, table_np, idx)
    tdt, ibits = (torch.float32, torch.int32) if dt == FIL_F32 else (torch.bfloat16, torch.int16)
    n = B * F * K
    out = torch.full((n + K,), -1, dtype=ibits, device="cuda")
    cnt = torch.zeros((), dtype=torch.int32, device="cuda")
    table, offsets, sizes, ids = (torch.tensor(a, device="cuda") for a in (table_np, off, np.array(vocab, np.int64), idx))
    check(_lib.load().fil_embed_gather_dt(ptr(table), ptr(offsets), ptr(sizes), ptr(ids), ptr(out), ptr(cnt), B, F, K, dt, stream_ptr()),
          "fil_embed_gather_dt")
    assert int(cnt) == len(bad)
    got = out.cpu()
    assert torch.equal(got[:n], torch.tensor(want).to(tdt).reshape(-1).view(ibits))
    assert (got[n:] == -1).all()                                       # nothing behind the block


@pytest.mark.parametrize("B,F,K,ok", [(37, 7, 5, True), (37, 39, 16, True), (5, 1, 3, True), (9, 200, 64, True), (9, 200, 84, False)])
def test_gather_xt_both_layouts(B, F, K, ok):
    """fil_embed_gather_xt: F K not a multiple of the 256 threads; F (K + 1) 4 bytes of LDS just above 48 KiB (F = 200, K = 64: the
    raised dynamic LDS limit); above 64 KiB (F = 200, K = 84) FIL_ERR_UNSUPPORTED with both outputs untouched."""
    rng = np.random.default_rng(9000 + F + K)
    if F == 200:
        assert F * (K + 1) * 4 > 48 * 1024 and (F * (K + 1) * 4 <= 64 * 1024) == ok
    else:
        assert (F * K) % 256 != 0
    vocab, off, table_np, idx = _gather_case(rng, B, F, K, 2, 60)
    idx[2, 0], idx[B - 1, F - 1] = vocab[0], -1
    want = _gather_want(vocab, off, table_np, idx)
    n = B * F * K
    out = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    xt = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((), dtype=torch.int32, device="cuda")
    table, offsets, sizes, ids = (torch.tensor(a, device="cuda") for a in (table_np, off, np.array(vocab, np.int64), idx))
    rc = _lib.load().fil_embed_gather_xt(ptr(table), ptr(offsets), ptr(sizes), ptr(ids), ptr(out), ptr(xt), ptr(cnt), B, F, K, stream_ptr())
    ob, xb = out.cpu().numpy(), xt.cpu().numpy()
    if not ok:
        assert rc == FIL_ERR_UNSUPPORTED and int(cnt) == 0 and (ob == SENTINEL).all() and (xb == SENTINEL).all()
        return
    assert rc == 0, _lib.load().fil_last_error()
    assert int(cnt) == 2 and (ob[n:] == SENTINEL).all() and (xb[n:] == SENTINEL).all()
    assert np.array_equal(ob[:n], want.view(np.int32).reshape(-1))
    assert np.array_equal(xb[:n], np.ascontiguousarray(want.transpose(0, 2, 1)).view(np.int32).reshape(-1))      # xt[(b K + k) F + f]
