"""The device walks the fused table optimizers share (ml_function_amd/csrc/optim_rows.h, optim_rule.h, optim_adam.h) at the edges the
per-optimizer tests never reach, on the constructed cases of tests/optim_walk_cases.py (properties checked without a GPU by
tests/test_optim_walk_cases_host.py): field tables of 1 ... 1024 fields with zero-row, frozen and unregularised fields on every side
of the lane and wave boundaries of the sweep's workgroup scan; hand-built gathered lists with K past one, two and sixteen chunks of the
merged walk, clipped and negative counts and ids outside the table; tables, lists and dense tensors one step past the 2048-workgroup
grid cap; more dense descriptors than workgroups.  SGD with momentum and RMSprop carry the bit-for-bit comparisons (their table kernels
are held to tests/keras_sgd_rmsprop_ref.py elsewhere; every gradient sum here is exact in fp32), the other families are compared
with themselves: W lists against one list of the same sums, one description of a table against a finer one.  Every table, slot and
stamp array sits between sentinel guards (tests/guarded.py), checked after every call."""
import ctypes
import types

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, optim
from ml_function_amd._lib import AdaoptHyper, MomoptHyper, NadamHyper, RowoptHyper, ptr, stream_ptr
from tests import guarded, keras_amsgrad_ref as aref, keras_sgd_rmsprop_ref as ref, optim_walk_cases as wc

pytestmark = pytest.mark.gpu

F = np.float32
UNSUPPORTED = -4


def ok(rc, what):
    _lib.check(rc, what)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_differ(a, b):
    return (bits(a) != bits(b)).reshape(a.shape[0], -1).any(axis=1)


class Buf:
    """A device array between sentinel guards, set from a float32 / int32 host array; f32() / i32() check the guards and read it."""

    def __init__(self, a, name):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize == 4
        self.g = guarded.GuardedOutput(a.shape, np.uint32, name)
        if a.size:
            self.g.t[self.g.guard:self.g.guard + a.size] = torch.from_numpy(a.reshape(-1).view(np.int32).copy()).cuda()
        self.ptr = self.g.ptr

    def f32(self, what=""):
        return self.g.read(what).view(F)

    def i32(self, what=""):
        return self.g.read(what).view(np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_f32(a):
    """A float32 input with poisoned words behind it."""
    return guarded.poisoned_input(guarded.f32_words(a))


class Fields:
    def __init__(self, lay):
        self.F, self.V = lay["F"], lay["V"]
        self.offsets, self.l2, self.frozen = dev(lay["offsets"]), dev_f32(lay["l2"]), dev(lay["frozen"])


def tag_of(step):
    return int(np.array([step + 1], np.int64).astype(np.uint32).view(np.int32)[0])


def momopt(variant):
    h = ref.hyper(variant, lr=1e-2)
    ch = MomoptHyper(float(h["lr"]), float(h["eps"]), float(h["rho"]), float(h["momentum"]),
                     _lib.FIL_MOMOPT_NESTEROV if variant == "sgd_nesterov" else 0, 0)
    return h, ch, (_lib.FIL_OPT_SGD if variant.startswith("sgd") else _lib.FIL_OPT_RMSPROP)


def table_state(V, K, seed, slots=1):
    """p and `slots` positive slot arrays (an rms, a v must not be negative)."""
    rng = np.random.default_rng([V, K, seed])
    return [(rng.standard_normal((V, K)) * 0.5).astype(F)] + [(np.abs(rng.standard_normal((V, K))) * 0.1 + 0.01).astype(F)
                                                              for _ in range(slots)]


def lists_dev(c):
    return dev(c["ids"]), dev_f32(c["values"]), dev(c["counts"])


# ---------------------------------------------------------------------------------------------------- 1. the rule sweep's field table
def rule_steps(variant, lay, K, via="runs", steps=3, step0=0, n_random=12):
    """`steps` steps of (runs update | merged update of one list) + sweep from step count step0: after every step p and the slot
    bit-equal to ref.table_step on the batch's exact sums, the rows outside its moved / decayed sets with unchanged bits, the stamps
    the step's tag on exactly the touched rows."""
    lib = _lib.load()
    h, ch, rule = momopt(variant)
    V, fl = lay["V"], Fields(lay)
    row_l2, frozen = wc.row_maps(lay)
    p0, s0 = table_state(V, K, 1)
    P, S, ST = Buf(p0, "table"), Buf(s0, "slot"), Buf(np.zeros(V, np.int32), "stamp")
    step = torch.tensor([step0], dtype=torch.int64, device="cuda")
    state, stamps = (p0, s0, None), np.zeros(V, np.int32)
    hp = ctypes.addressof(ch)
    for t in range(steps):
        b = wc.touch_batch(lay, K, t, n_random)
        if via == "runs":
            g, perm, ids = dev_f32(b["g"]), dev(b["perm"]), dev(b["sorted_ids"])
            ok(lib.fil_embed_momopt_runs(ptr(g), ptr(perm), ptr(ids), b["R"], K, _lib.FIL_F32, fl.F, ptr(fl.l2), P.ptr, S.ptr, None, ST.ptr,
                                         ptr(step), rule, hp, stream_ptr()), "runs")
        else:
            one = wc.one_list(b["sums"], b["touched"])
            ids, values, counts = lists_dev(one)
            ok(lib.fil_embed_momopt_merged(ptr(ids), ptr(values), ptr(counts), 1, one["cap"], K, ptr(fl.offsets), ptr(fl.l2), fl.F, P.ptr,
                                           S.ptr, None, ST.ptr, V, ptr(step), rule, hp, stream_ptr()), "merged")
        ok(lib.fil_embed_momopt_sweep(P.ptr, S.ptr, None, ST.ptr, V, K, ptr(fl.offsets), ptr(fl.l2), ptr(fl.frozen), fl.F, ptr(step), rule,
                                      hp, stream_ptr()), "sweep")
        torch.cuda.synchronize()
        where = (variant, lay["F"], K, via, t)
        stamps = np.where(b["touched"], np.int32(tag_of(step0 + t)), stamps)
        assert np.array_equal(ST.i32(where), stamps), where
        old = state
        state, moved, decayed = ref.table_step(h, *old, b["sums"], b["touched"], row_l2, frozen)
        got = (P.f32(where), S.f32(where))
        for a, w, o, what in zip(got, state, old, "ps"):
            bad = np.nonzero(rows_differ(a, w))[0]
            assert bad.size == 0, (where, what, bad[:8], wc.field_of_row(lay)[bad[:8]])
        took = moved | decayed
        assert np.array_equal(rows_differ(got[0], old[0]) | rows_differ(got[1], old[1]), took), where
        assert np.array_equal(rows_differ(got[0], old[0]), moved), where
        step += 1
    return state


@pytest.mark.parametrize("variant", ["sgd_momentum", "rmsprop"])
@pytest.mark.parametrize("kind", wc.LAYOUT_KINDS)
@pytest.mark.parametrize("F_", wc.FIELD_SIZES)
def test_rule_sweep_field_table(F_, kind, variant):
    """K = 4: the 16-byte path.  Every layout kind at every table size: the compacted table of load_reg_tab with entries from every
    lane and wave (roles, all), from the last lane alone, from the first alone, and empty."""
    rule_steps(variant, wc.field_layout(F_, kind), 4)


@pytest.mark.parametrize("variant", ["sgd_momentum", "rmsprop"])
@pytest.mark.parametrize("F_", wc.FIELD_SIZES)
def test_rule_sweep_field_table_element_path(F_, variant):
    rule_steps(variant, wc.field_layout(F_), 3)


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("F_", wc.FIELD_SIZES)
def test_merged_field_search_at_every_table_size(F_, K):
    """The touched rows arrive as one gathered list: sweep_field over F_ offsets in the merged update, RegTab in the sweep behind it."""
    rule_steps("sgd_momentum", wc.field_layout(F_), K, via="merged")


@pytest.mark.parametrize("F_", wc.FIELD_SIZES)
def test_sweep_without_a_walked_field_changes_nothing(F_):
    """field_l2 non-NULL and all zero: the sweep of a rule that is not kSweepAll launches, compacts an empty table and leaves."""
    lib = _lib.load()
    h, ch, rule = momopt("sgd_momentum")
    lay = wc.field_layout(F_, "none")
    fl, (p0, s0) = Fields(lay), table_state(lay["V"], 4, 2)
    P, S, ST = Buf(p0, "table"), Buf(s0, "slot"), Buf(np.zeros(lay["V"], np.int32), "stamp")
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    ok(lib.fil_embed_momopt_sweep(P.ptr, S.ptr, None, ST.ptr, fl.V, 4, ptr(fl.offsets), ptr(fl.l2), ptr(fl.frozen), fl.F, ptr(step), rule,
                                  ctypes.addressof(ch), stream_ptr()), "sweep")
    assert same_bits(P.f32(), p0) and same_bits(S.f32(), s0) and not ST.i32().any()


def test_step_tag_crosses_the_int32_sign():
    """Steps 2^31 - 1, 2^31, 2^31 + 1: the tag goes from INT32_MAX to INT32_MIN; stamped rows are still the ones the sweep skips."""
    assert tag_of(2 ** 31 - 2) == 2 ** 31 - 1 and tag_of(2 ** 31 - 1) == -2 ** 31
    rule_steps("sgd_momentum", wc.field_layout(257), 4, step0=2 ** 31 - 2)


# ---------------------------------------------------------------------------------------------------- 2. one table, two descriptions
ADAM = aref.hyper()


def sweep_call(entry, bufs, ST, fl, K, step):
    lib = _lib.load()
    a = [b.ptr for b in bufs]
    tail = (fl.V, K, ptr(fl.offsets), ptr(fl.l2), ptr(fl.frozen), fl.F, ptr(step))
    if entry == "adam":
        return lib.fil_embed_adam_sweep(a[0], a[1], a[2], ST.ptr, *tail, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], stream_ptr())
    if entry == "amsgrad":
        return lib.fil_embed_amsgrad_sweep(a[0], a[1], a[2], a[3], ST.ptr, *tail, ADAM["lr"], None, ADAM["b1"], ADAM["b2"], ADAM["eps"],
                                           stream_ptr())
    h, ch, rule = momopt(entry)
    return lib.fil_embed_momopt_sweep(a[0], a[1], None, ST.ptr, *tail, rule, ctypes.addressof(ch), stream_ptr())


N_SLOTS = dict(adam=2, amsgrad=3, sgd_momentum=1, rmsprop=1)


def split_equality(entry, lay, K, stamped):
    """One sweep from the same state under the table's own description and under wc.split_layout's 1024 sub-fields: bit-identical
    arrays.  The state is not a fresh one and some rows carry the step's tag (next to field boundaries too)."""
    V = lay["V"]
    arrays = table_state(V, K, 3, N_SLOTS[entry])
    stamp0 = np.zeros(V, np.int32)
    stamp0[stamped] = tag_of(6)
    out = []
    for d in (lay, wc.split_layout(lay)):
        bufs, ST = [Buf(x, "array %d" % i) for i, x in enumerate(arrays)], Buf(stamp0, "stamp")
        step = torch.tensor([6], dtype=torch.int64, device="cuda")
        ok(sweep_call(entry, bufs, ST, Fields(d), K, step), entry)
        out.append([b.f32((entry, d["F"])) for b in bufs])
        assert np.array_equal(ST.i32(), stamp0)
    for i, (a, b) in enumerate(zip(*out)):
        bad = np.nonzero(rows_differ(a, b))[0]
        assert bad.size == 0, (entry, i, bad[:8])
    # what both did: stamped and frozen rows keep every bit, every other row of a regularised field moved
    row_l2, frozen = wc.row_maps(lay)
    hold = frozen.copy()
    hold[stamped] = True
    for a, x in zip(out[0], arrays):
        assert same_bits(a[hold], x[hold])
    assert rows_differ(out[0][0], arrays[0])[~hold & (row_l2 > 0)].all() and (~hold & (row_l2 > 0)).any()


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("F_", [5, 257])
@pytest.mark.parametrize("entry", ["adam", "amsgrad", "sgd_momentum", "rmsprop"])
def test_sweep_is_the_same_under_a_finer_description(entry, F_, K):
    lay = wc.field_layout(F_)
    b = wc.touch_batch(lay, K, 0)
    split_equality(entry, lay, K, np.nonzero(b["touched"])[0][::3])          # (the six rows of F = 5 are all touched)


def test_rows_in_front_of_the_first_offset_are_pinned():
    """offsets[0] > 0 (SparseEmbed never builds it: its first field starts at row 0).  The entry points DISAGREE about the rows in front,
    and this pins what each does today so that a change is a decision: the Adam / AMSGrad sweeps give them field -1, unregularised
    and not frozen, so they take the g = 0 step exactly as under a description with one more plain field in front (bit-identical);
    the rule sweeps walk the rows of fields only, so not even RMSprop's rms decays there, while under the longer description it
    does."""
    V, K = 9, 4
    short = dict(F=2, V=V, offsets=np.array([2, 5], np.int64), l2=np.array([wc.l2_of_field(1), wc.l2_of_field(2)], F),
                 frozen=np.zeros(2, np.uint8))
    full = dict(F=3, V=V, offsets=np.array([0, 2, 5], np.int64), l2=np.array([0, wc.l2_of_field(1), wc.l2_of_field(2)], F),
                frozen=np.zeros(3, np.uint8))
    front = np.arange(V) < 2
    for entry in ("adam", "amsgrad", "sgd_momentum", "rmsprop"):
        arrays = table_state(V, K, 8, N_SLOTS[entry])
        out = []
        for d in (short, full):
            bufs, ST = [Buf(x, "array") for x in arrays], Buf(np.zeros(V, np.int32), "stamp")
            step = torch.tensor([2], dtype=torch.int64, device="cuda")
            ok(sweep_call(entry, bufs, ST, Fields(d), K, step), entry)
            out.append([b.f32(entry) for b in bufs])
        for a, b in zip(*out):
            assert same_bits(a[~front], b[~front]), entry
        if entry in ("adam", "amsgrad"):
            assert all(same_bits(a, b) for a, b in zip(*out)) and rows_differ(out[0][0], arrays[0])[front].all(), entry
        else:
            assert all(same_bits(a[front], x[front]) for a, x in zip(out[0], arrays)), entry
            assert rows_differ(out[1][1], arrays[1])[front].all() == (entry == "rmsprop"), entry


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_more_than_1024_fields_are_refused_and_nothing_is_touched():
    lib = _lib.load()
    V, K, F_ = 8, 4, 1025
    arrays = table_state(V, K, 4, 3)
    bufs, ST = [Buf(x, "array") for x in arrays], Buf(np.zeros(V, np.int32), "stamp")
    a = [b.ptr for b in bufs]
    offsets, l2, frozen = dev(np.minimum(np.arange(F_), V).astype(np.int64)), dev_f32(np.full(F_, 0.01, F)), dev(np.zeros(F_, np.uint8))
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ids, values, counts = dev(np.arange(4, dtype=np.int64)), dev_f32(np.ones((4, K), F)), dev(np.array([4], np.int64))
    ring = torch.zeros(8 * 4, device="cuda")
    h, ch, rule = momopt("sgd_momentum")
    hp, s = ctypes.addressof(ch), stream_ptr()
    A = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"])
    sweep_tail = (V, K, ptr(offsets), ptr(l2), ptr(frozen), F_, ptr(step))
    lists = (ptr(ids), ptr(values), ptr(counts), 1, 4, K, ptr(offsets), ptr(l2))
    calls = dict(
        momopt_sweep=lambda: lib.fil_embed_momopt_sweep(a[0], a[1], None, ST.ptr, *sweep_tail, rule, hp, s),
        adam_sweep=lambda: lib.fil_embed_adam_sweep(a[0], a[1], a[2], ST.ptr, *sweep_tail, *A, s),
        amsgrad_sweep=lambda: lib.fil_embed_amsgrad_sweep(a[0], a[1], a[2], a[3], ST.ptr, *sweep_tail, A[0], None, *A[1:], s),
        momopt_merged=lambda: lib.fil_embed_momopt_merged(*lists, F_, a[0], a[1], None, ST.ptr, V, ptr(step), rule, hp, s),
        adam_merged=lambda: lib.fil_embed_adam_merged(*lists, F_, a[0], a[1], a[2], ST.ptr, V, ptr(step), *A, _lib.FIL_ADAM_KERAS, s),
        amsgrad_merged=lambda: lib.fil_embed_amsgrad_merged(*lists, F_, a[0], a[1], a[2], a[3], ST.ptr, V, ptr(step), A[0], None, *A[1:], s),
        adam_merged_deferred=lambda: lib.fil_embed_adam_merged_deferred(*lists, ptr(frozen), F_, a[0], a[1], a[2], ST.ptr, ptr(ring), 4, V,
                                                                        ptr(step), *A, s))
    wide = types.SimpleNamespace(F=F_, offsets=offsets, l2=l2, frozen=frozen)
    fams = families()                                                       # the merged entry point of every family
    for name, (_, merged, _keep) in fams.items():
        calls[name + " merged"] = lambda merged=merged: merged(lib, lists[:6], wide, a, ST, V, step)
    for name, call in calls.items():
        assert call() == UNSUPPORTED, name
        assert b"F=1025" in lib.fil_last_error(), (name, lib.fil_last_error())
    torch.cuda.synchronize()
    for b, x in zip(bufs, arrays):
        assert same_bits(b.f32(), x)
    assert not ST.i32().any() and int(step) == 0


# ---------------------------------------------------------------------------------------------------- 4. the merged walk
def check_stamps(ST, before, touched, tag, where):
    want = np.where(touched, np.int32(tag), before)
    got = ST.i32(where)
    assert np.array_equal(got, want), (where, np.nonzero(got != want)[0][:8])


def merged_sgd(case, step0=3):
    """fil_embed_momopt_merged (SGD with momentum) on the case's lists, bit-equal to the restatement on the exact sums of the rows the
    reference says are touched (no sweep: the other rows keep their bits), and stamped on exactly those."""
    lib = _lib.load()
    h, ch, rule = momopt("sgd_momentum")
    lay, K = case["lay"], case["K"]
    V, fl = lay["V"], Fields(lay)
    row_l2, _ = wc.row_maps(lay)
    sums, touched = wc.merged_reference(case)
    p0, s0 = table_state(V, K, 5)
    stamp0 = np.full(V, 77, np.int32)
    P, S, ST = Buf(p0, "table"), Buf(s0, "slot"), Buf(stamp0, "stamp")
    step = torch.tensor([step0], dtype=torch.int64, device="cuda")
    ids, values, counts = lists_dev(case)
    ok(lib.fil_embed_momopt_merged(ptr(ids), ptr(values), ptr(counts), case["W"], case["cap"], K, ptr(fl.offsets), ptr(fl.l2), fl.F, P.ptr,
                                   S.ptr, None, ST.ptr, V, ptr(step), rule, ctypes.addressof(ch), stream_ptr()), "merged")
    torch.cuda.synchronize()
    where = (K, case["W"])
    (wp, ws, _), moved, _ = ref.table_step(h, p0, s0, None, sums, touched, row_l2, ~touched)
    assert np.array_equal(moved, touched)
    for a, w, what in ((P.f32(where), wp, "p"), (S.f32(where), ws, "slot")):
        bad = np.nonzero(rows_differ(a, w))[0]
        assert bad.size == 0, (where, what, bad[:8], (bits(a) != bits(w))[bad[0]].nonzero()[0][:8])
    check_stamps(ST, stamp0, touched, tag_of(step0), where)
    assert int(step) == step0


@pytest.mark.parametrize("W", wc.MERGED_W)
@pytest.mark.parametrize("K", wc.MERGED_K)
def test_merged_walk_of_hand_built_lists(K, W):
    merged_sgd(wc.merged_case(K, W))


def test_merged_walk_compound_case():
    merged_sgd(wc.merged_case(33, 3, wc.field_layout(257), n_rows=60))


def _rule_family(name, rule, hyper, keep=()):
    def call(lib, lists, fl, a, ST, V, step):
        fn = getattr(lib, "fil_embed_%s_merged" % name)
        return fn(*lists, ptr(fl.offsets), ptr(fl.l2), fl.F, a[0], a[1], a[2], ST.ptr, V, ptr(step), rule, ctypes.addressof(hyper), stream_ptr())
    return 2, call, (hyper,) + tuple(keep)


def families():
    """name -> (slots, call, objects to keep alive): every entry point that sits on merged_row_sums."""
    A = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"])
    out = {}
    for mode, name in ((_lib.FIL_ADAM_KERAS, "adam_keras"), (_lib.FIL_ADAM_LAZY, "adam_lazy")):
        out[name] = (2, lambda lib, lists, fl, a, ST, V, step, mode=mode: lib.fil_embed_adam_merged(
            *lists, ptr(fl.offsets), ptr(fl.l2), fl.F, a[0], a[1], a[2], ST.ptr, V, ptr(step), *A, mode, stream_ptr()), ())
    out["amsgrad"] = (3, lambda lib, lists, fl, a, ST, V, step: lib.fil_embed_amsgrad_merged(
        *lists, ptr(fl.offsets), ptr(fl.l2), fl.F, a[0], a[1], a[2], a[3], ST.ptr, V, ptr(step), A[0], None, *A[1:], stream_ptr()), ())
    ring = torch.zeros(_lib.load().fil_embed_adam_ring_len(4) * 4, device="cuda")
    out["adam_deferred"] = (2, lambda lib, lists, fl, a, ST, V, step: lib.fil_embed_adam_merged_deferred(
        *lists, ptr(fl.offsets), ptr(fl.l2), ptr(fl.frozen), fl.F, a[0], a[1], a[2], ST.ptr, ptr(ring), 4, V, ptr(step), *A, stream_ptr()),
        (ring,))
    out["adagrad"] = _rule_family("rowopt", _lib.FIL_OPT_ADAGRAD, RowoptHyper(1e-2, 1e-7, -0.5, 0.0, 0.0, 0.0))
    out["ftrl"] = _rule_family("rowopt", _lib.FIL_OPT_FTRL, RowoptHyper(1e-2, 1e-7, -0.5, 1e-3, 1e-3, 0.0))
    for v in ref.VARIANTS:
        h, ch, rule = momopt(v)
        out[v] = _rule_family("momopt", rule, ch)
    out["adadelta"] = _rule_family("adaopt", _lib.FIL_OPT_ADADELTA, AdaoptHyper(1.0, 0.95, 0.9, 0.999, 1e-7))
    out["adamax"] = _rule_family("adaopt", _lib.FIL_OPT_ADAMAX, AdaoptHyper(1e-2, 0.95, 0.9, 0.999, 1e-7))
    cache = torch.ones(1, device="cuda")
    out["nadam"] = _rule_family("nadam", _lib.FIL_OPT_NADAM, NadamHyper(1e-2, 0.9, 0.999, 1e-7, 0.004, 0, cache.data_ptr()), keep=(cache,))
    return out


FAMILIES = ("adam_keras", "adam_lazy", "amsgrad", "adam_deferred", "adagrad", "ftrl") + ref.VARIANTS + ("adadelta", "adamax", "nadam")


def lists_equal_one_list(family, case):
    """The merged update over the case's W lists and the same entry point on ONE list holding the exact sums, from the same state:
    every array and the stamps bit-identical; untouched rows keep their bits, touched rows moved."""
    lib = _lib.load()
    slots, call, keep = families()[family]
    lay, K = case["lay"], case["K"]
    V, fl = lay["V"], Fields(lay)
    sums, touched = wc.merged_reference(case)
    arrays = table_state(V, K, 6, 3)
    out = []
    for c in (case, wc.one_list(sums, touched)):
        bufs, ST = [Buf(x, "array %d" % i) for i, x in enumerate(arrays)], Buf(np.zeros(V, np.int32), "stamp")
        step = torch.zeros(1, dtype=torch.int64, device="cuda")
        ids, values, counts = lists_dev(c)
        lists = (ptr(ids), ptr(values), ptr(counts), c["W"], c["cap"], K)
        ok(call(lib, lists, fl, [b.ptr for b in bufs], ST, V, step), family)
        torch.cuda.synchronize()
        out.append([b.f32((family, c["W"])) for b in bufs] + [ST.i32()])
    for i, (a, b) in enumerate(zip(*out)):
        bad = np.nonzero(rows_differ(a, b))[0]
        assert bad.size == 0, (family, K, i, bad[:8])
    got = out[0]
    for a, x in zip(got[:4], arrays):
        assert same_bits(a[~touched], x[~touched]), family
    assert rows_differ(got[0], arrays[0])[touched].all(), family
    stamped = family not in ("adam_lazy",)
    assert np.array_equal(got[4] != 0, touched if stamped else np.zeros(V, bool)), family


@pytest.mark.parametrize("family", FAMILIES)
def test_every_merged_family_sums_w_lists_like_one(family):
    lists_equal_one_list(family, wc.merged_case(33, 3, wc.field_layout(257), n_rows=60))


@pytest.mark.parametrize("K", wc.MERGED_K)
@pytest.mark.parametrize("family", ["adam_keras", "amsgrad"])
def test_adam_merged_sums_w_lists_like_one_at_every_k(family, K):
    lists_equal_one_list(family, wc.merged_case(K, 5))


def row_nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


@pytest.mark.parametrize("K", [17, 33, 256])
@pytest.mark.parametrize("family", ["adam_keras", "amsgrad"])
def test_adam_merged_rows_against_float64(family, K):
    """W = 1, K past one, two and sixteen chunks, two steps (the second with gradients 1/8 the size, so vhat > v): every touched row
    against keras_amsgrad_ref.adam64 / amsgrad64 from the device's fp32 state at tests/test_optim_gpu.py's bars, applied PER ROW (a
    row's norm has K terms, the table's V K): 1e-6 on p, 1e-4 on the update, 1e-5 on m and v.  The project's bars hold per row as they
    stand, so none was measured anew (worst rows on an MI355X: p 3.5e-8, update 3.2e-5, m 5.2e-8, v 1.0e-7; each step prints its own)."""
    lib = _lib.load()
    ams = family == "amsgrad"
    slots, call, _ = families()[family]
    lay = wc.merged_layout()
    V, fl = lay["V"], Fields(lay)
    row_l2, _ = wc.row_maps(lay)
    p0 = table_state(V, K, 7, 0)[0]
    arrays = [p0] + [np.zeros((V, K), F)] * 3
    bufs, ST = [Buf(x, "array %d" % i) for i, x in enumerate(arrays)], Buf(np.zeros(V, np.int32), "stamp")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    old = [x.astype(np.float64) for x in arrays]
    worst = dict(p=0.0, update=0.0, m=0.0, v=0.0)
    for t in (1, 2):
        case = wc.merged_case(K, 1, seed=t)
        if t == 2:
            case["values"] = case["values"] * F(0.125)
        sums, touched = wc.merged_reference(case)
        ids, values, counts = lists_dev(case)
        ok(call(lib, (ptr(ids), ptr(values), ptr(counts), 1, case["cap"], K), fl, [b.ptr for b in bufs], ST, V, step), family)
        step += 1
        new = [b.f32((family, K, t)).astype(np.float64) for b in bufs]
        g = sums.astype(np.float64) + 2.0 * row_l2.astype(np.float64)[:, None] * old[0]
        if ams:
            want = aref.amsgrad64(ADAM, old[0], g, old[1], old[2], old[3], t)
        else:
            want = aref.adam64(ADAM, old[0], g, old[1], old[2], t) + (old[3],)
        r = touched
        e = dict(p=row_nrel(new[0][r], want[0][r]), update=row_nrel(new[0][r] - old[0][r], want[0][r] - old[0][r]),
                 m=row_nrel(new[1][r], want[1][r]), v=row_nrel(new[2][r], want[2][r]))
        for k in e:
            worst[k] = max(worst[k], float(e[k].max()))
        print("%s K=%d step %d worst row: %s" % (family, K, t, {k: "%.2e" % float(v.max()) for k, v in e.items()}))
        assert (e["p"] < 1e-6).all() and (e["update"] < 1e-4).all() and (e["m"] < 1e-5).all() and (e["v"] < 1e-5).all(), (t, worst)
        if ams:
            assert same_bits(new[3].astype(F), aref.vhat_next32(old[3], new[2]))
        for a, b in zip(new, old):
            assert np.array_equal(a[~r], b[~r])
        old = new


# ---------------------------------------------------------------------------------------------------- 5. past the grid cap
BIG = {4: wc.two_field_layout(524288 + 2051, 1000), 3: wc.two_field_layout(174763 + 517, 100)}


@pytest.mark.parametrize("variant", ["sgd_momentum", "rmsprop"])
@pytest.mark.parametrize("K", [4, 3])
def test_rule_sweep_past_the_grid_cap(K, variant):
    """The walked rows are more than 2048 workgroups' lanes: the sweep's grid-stride loop makes a second trip."""
    rule_steps(variant, BIG[K], K, steps=1, n_random=300)


@pytest.mark.parametrize("entry", ["adam", "amsgrad"])
@pytest.mark.parametrize("K", [4, 3])
def test_adam_sweep_past_the_grid_cap(K, entry):
    lay = BIG[K]
    split_equality(entry, lay, K, np.nonzero(wc.touch_batch(lay, K, 0, n_random=300)["touched"])[0])


@pytest.mark.parametrize("fill_last", [False, True], ids=["thirds", "filled"])
def test_merged_walk_past_the_grid_cap(fill_last):
    merged_sgd(wc.big_merged_case(fill_last))


def descriptors(c, base, slots):
    """fil_adam_tensor descriptors of the dense case's tensors inside the flat device arrays at base = (p, g, slot, slot2)."""
    at = lambda b, i: b + 4 * int(c["starts"][i])
    ds = [optim._Desc(at(base[0], i), None if i in c["none"] else at(base[1], i), at(base[2], i), at(base[3], i) if slots == 2 else None,
                      n, c["l2"][i], 0) for i, n in enumerate(c["sizes"])]
    return torch.frombuffer(bytearray((optim._Desc * len(ds))(*ds)), dtype=torch.uint8).cuda()


def dense_momopt(c, total_numel, what):
    lib = _lib.load()
    h, ch, rule = momopt("sgd_momentum")
    P, S, g = Buf(c["p"], "p"), Buf(c["s"], "slot"), dev_f32(c["g"])
    d = descriptors(c, (P.ptr, g.data_ptr(), S.ptr, 0), 1)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ok(lib.fil_momopt_multi(ptr(d), len(c["sizes"]), total_numel, ptr(step), rule, ctypes.addressof(ch), 1, stream_ptr()), what)
    torch.cuda.synchronize()
    assert int(step) == 1
    got_p, got_s = P.f32(what), S.f32(what)
    for i, n in enumerate(c["sizes"]):
        sl = slice(int(c["starts"][i]), int(c["starts"][i]) + n)
        gi = np.zeros(n, F) if i in c["none"] else c["g"][sl]
        wp, ws, _ = ref.dense_step(h, c["p"][sl], c["s"][sl], None, gi, c["l2"][i])
        assert same_bits(got_p[sl], wp) and same_bits(got_s[sl], ws), (what, i, n)
    return got_p, got_s


def dense_adam(c, total_numel, what):
    lib = _lib.load()
    n_all = len(c["p"])
    P, M, V_, g = Buf(c["p"], "p"), Buf(np.zeros(n_all, F), "m"), Buf(np.zeros(n_all, F), "v"), dev_f32(c["g"])
    d = descriptors(c, (P.ptr, g.data_ptr(), M.ptr, V_.ptr), 2)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ok(lib.fil_adam_multi(ptr(d), len(c["sizes"]), total_numel, ptr(step), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 1, stream_ptr()),
       what)
    torch.cuda.synchronize()
    assert int(step) == 1
    return P.f32(what), M.f32(what), V_.f32(what)


def test_dense_walk_past_the_grid_cap():
    """2051 chunks on 2048 workgroups: fil_momopt_multi bit-equal to the restatement; fil_adam_multi against adam64 at
    test_adam_multi_matches_keras_apply_adam's bars per tensor (update 1e-4, m 1e-6, v 1e-5, p 1e-6, norm-relative)."""
    c = wc.dense_case(wc.BIG_DENSE, 1, none=(4,))
    total = sum(c["sizes"])
    dense_momopt(c, total, "momopt")
    p, m, v = dense_adam(c, total, "adam")
    for i, n in enumerate(c["sizes"]):
        if n == 0:
            continue
        sl = slice(int(c["starts"][i]), int(c["starts"][i]) + n)
        p0 = c["p"][sl].astype(np.float64)
        g = (0.0 if i in c["none"] else c["g"][sl].astype(np.float64)) + 2.0 * float(F(c["l2"][i])) * p0
        wp, wm, wv = aref.adam64(ADAM, p0, g, np.zeros(n), np.zeros(n), 1)
        assert aref.nrel(p[sl], wp) < 1e-6 and aref.nrel(p[sl].astype(np.float64) - p0, wp - p0) < 1e-4, (i, n)
        assert aref.nrel(m[sl], wm) < 1e-6 and aref.nrel(v[sl], wv) < 1e-5, (i, n)


def test_dense_rotation_with_more_descriptors_than_workgroups():
    """300 descriptors: the grid comes from the caller's total_numel (91 workgroups for the true one, ONE for total_numel = 0), the
    chunks from the descriptors (330): both launches bit-equal to the restatement, Adam's two launches to each other."""
    c = wc.dense_case(wc.ROTATION_SIZES, 2)
    total = sum(c["sizes"])
    a = dense_momopt(c, total, "true total")
    b = dense_momopt(c, 0, "one workgroup")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    x, y = dense_adam(c, total, "adam true total"), dense_adam(c, 0, "adam one workgroup")
    assert all(same_bits(u, w) for u, w in zip(x, y)) and not same_bits(x[0], c["p"])


def test_no_descriptors_only_advance_the_step():
    lib = _lib.load()
    h, ch, rule = momopt("sgd_momentum")
    step = torch.tensor([41], dtype=torch.int64, device="cuda")
    ok(lib.fil_momopt_multi(None, 0, 0, ptr(step), rule, ctypes.addressof(ch), 1, stream_ptr()), "momopt")
    ok(lib.fil_adam_multi(None, 0, 0, ptr(step), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 1, stream_ptr()), "adam")
    ok(lib.fil_adam_multi(None, 0, 0, ptr(step), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 0, stream_ptr()), "adam")
    assert int(step) == 43
