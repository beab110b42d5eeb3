"""Keras' Mean, BinaryCrossentropy, BinaryAccuracy, Precision and Recall on the GPU (include/fil.h M2, ml_function_amd.metrics) against
the numpy restatement of TensorFlow 2.1's metrics (tests/keras_mean_metrics_ref.py).

Bars.  Accuracy, Precision and Recall count in integers: total, count, tp / fp / fn and their quotients are bit-equal.  For Mean
and BinaryCrossentropy neither Keras nor the kernel fixes the order of the float32 sum inside one update, so `total` (from a zero
state) is held to the float64 sum of the restatement's float32 per-sample values within (ceil(log2 n) + 8) 2^-24 sum|v|: a tree
summation's bound plus a few ulp per sample for the device's logf against numpy's.  `result` is bit-equal to float32(total) /
float32(count) of the state's own bits."""
import math
import socket

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, metrics, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd.layers.base import collect_regularization_loss
from tests import keras_mean_metrics_ref as ref

pytestmark = pytest.mark.gpu

ONE = _lib.FIL_MEAN_ONE_LAUNCH_N
f32 = np.float32
U = 2.0 ** -24


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _case(n, seed):
    """Skewed CTR scores with the decisions' special values mixed in, binary labels, and signed values for Mean."""
    rng = np.random.default_rng(seed)
    p = (1.0 / (1.0 + np.exp(-rng.normal(-1.5, 2.0, n)))).astype(f32)
    sp = np.asarray([0.0, 1.0, 0.5, 1e-7, 1 - 1e-7, np.nextafter(f32(0.5), f32(1)), 1e-45, 1.1754942e-38], f32)
    k = min(n // 2, len(sp))
    p[rng.permutation(n)[:k]] = sp[rng.permutation(len(sp))[:k]]
    y = (rng.random(n) < np.maximum(p, 0.05)).astype(f32)
    v = (rng.normal(0.3, 1.0, n) * np.exp(rng.normal(0, 2.0, n))).astype(f32)
    return y, p, v


def _bar(v):
    """(ceil(log2 n) + 8) 2^-24 sum|v| for the float32 values v of one update."""
    v = np.asarray(v, np.float64)
    return (math.ceil(math.log2(len(v))) + 8) * U * np.abs(v).sum()


def _state():
    return torch.zeros(3, device="cuda")


def _check_result_bits(st):
    """result = float32(total) / float32(count) of the state's own bits (the correctly rounded quotient; 0 for a zero count)."""
    total, count, result = (f32(x) for x in st)
    want = ref.div_no_nan(total, count)[()]
    assert result.tobytes() == want.tobytes() or (np.isnan(result) and np.isnan(want)), (total, count, result, want)


def _check_all_kinds(y, p, v, Y, P, V, tag, lines=None):
    """One update of each kind from a zero state against the restatement; Y, P, V are the device tensors (views allowed)."""
    n = len(p)
    # values
    st = Fn.mean_update("values", V, None, _state()).cpu().numpy()
    want = v.astype(np.float64).sum()
    err, bar = abs(float(st[0]) - want), _bar(v)
    if lines is not None:
        lines.append("%-22s values  total %.9g  off %.3e  bar %.3e" % (tag, st[0], err, bar))
        print(lines[-1])
    assert err <= bar and st[1] == n, (tag, "values", st, want, err, bar)
    _check_result_bits(st)
    # binary cross-entropy, with and without label smoothing
    for ls in (0.0, 0.1):
        vals = ref.values_bce(y, p, ls)
        st = Fn.mean_update("binary_crossentropy", P, Y, _state(), 1e-7, ls).cpu().numpy()
        want = vals.astype(np.float64).sum()
        err, bar = abs(float(st[0]) - want), _bar(vals)
        if lines is not None:
            lines.append("%-22s bce %.1f total %.9g  off %.3e  bar %.3e" % (tag, ls, st[0], err, bar))
            print(lines[-1])
        assert err <= bar and st[1] == n, (tag, "bce", ls, st, want, err, bar)
        _check_result_bits(st)
    # accuracy: bit-equal
    for thr in (0.5, 0.25):
        st = Fn.mean_update("binary_accuracy", P, Y, _state(), thr).cpu().numpy()
        r = ref.MeanState().update_accuracy(y, p, thr)
        assert st[0] == r.total and st[1] == r.count == n and st[2].tobytes() == r.result().tobytes(), (tag, "accuracy", thr, st, r.total)


# ------------------------------------------------------------------------------------------------ 1. sizes and alignments
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 1023, 1024, 1025, 4096, 4097, ONE, ONE + 1, 100003, (1 << 20) + 1])
def test_all_kinds_equal_the_restatement(n, capsys):
    y, p, v = _case(n, seed=n)
    with capsys.disabled():
        _check_all_kinds(y, p, v, _dev(y), _dev(p), _dev(v), "n=%d" % n, lines=[])
    assert (_lib.load().fil_mean_workspace_bytes(n) == 0) == (n <= ONE)                # the sizes cover both launch paths


@pytest.mark.parametrize("n", [1, 5, 4099, 70001])
def test_views_that_are_not_16_byte_aligned(n):
    y, p, v = _case(n + 8, seed=n + 1)
    Y, P, V = _dev(y), _dev(p), _dev(v)
    for ao, yo in ((1, 0), (0, 3), (1, 3), (2, 2), (3, 1)):
        pv, vv, yv = P[ao:ao + n], V[ao:ao + n], Y[yo:yo + n]
        assert pv.data_ptr() % 16 == 4 * ao and yv.data_ptr() % 16 == 4 * yo
        _check_all_kinds(y[yo:yo + n], p[ao:ao + n], v[ao:ao + n], yv, pv, vv, "n=%d a[%d:] y[%d:]" % (n, ao, yo))


# ------------------------------------------------------------------------------------------------ 2. values at the edges
def _ulps(a, b):
    """Distance of two finite float32 in units in the last place."""
    ia, ib = (int(np.asarray(x, f32).view(np.int32)) for x in (a, b))
    ia, ib = (x if x >= 0 else -(x & 0x7FFFFFFF) for x in (ia, ib))
    return abs(ia - ib)


def test_bce_per_sample_values_at_the_edges():
    """n = 1 updates from a zero state leave the sample's value in `total`: within 4 ulp of the restatement (two logf results, each
    within an ulp or two of numpy's, multiplied and added in the same float32 operations)."""
    ps = np.asarray([0.0, 1.0, 1e-7, 1 - 1e-7, 1e-41, -0.5, 1.5], f32)
    ys = np.asarray([0.0, 1.0, 0.3], f32)
    cases = [(pv, yv, ls) for ls in (0.0, 0.1) for pv in ps for yv in ys]
    states = torch.zeros(len(cases), 3, device="cuda")
    P, Y = _dev([c[0] for c in cases]), _dev([c[1] for c in cases])
    for i, (pv, yv, ls) in enumerate(cases):
        Fn.mean_update("binary_crossentropy", P[i:i + 1], Y[i:i + 1], states[i], 1e-7, ls)
    got = states.cpu().numpy()
    for i, (pv, yv, ls) in enumerate(cases):
        want = ref.values_bce([yv], [pv], ls)[0]
        assert np.isfinite(want) and _ulps(got[i, 0], want) <= 4, (pv, yv, ls, got[i], want)
        assert got[i, 1] == 1.0 and got[i, 2] == got[i, 0]
    # through the class: the same values, and epsilon is Keras' 1e-7
    m = metrics.BinaryCrossentropy(label_smoothing=0.1)
    m.update_state(Y[:21], P[:21])
    vals = ref.values_bce(Y[:21].cpu().numpy(), P[:21].cpu().numpy(), 0.1)
    assert abs(float(m.total) - vals.astype(np.float64).sum()) <= _bar(vals) and float(m.count) == 21.0


def test_nan_and_infinity_are_kept():
    y, p, v = _case(4096, seed=5)
    Y = _dev(y)
    # binary cross-entropy: a NaN score is a NaN loss (the clip keeps it), an infinite score is clipped like any other
    for n in (4096, ONE + 5):
        yy, pp, _ = _case(n, seed=n)
        bad = pp.copy()
        bad[n // 3] = np.nan
        m = metrics.BinaryCrossentropy()
        m.update_state(_dev(yy), _dev(bad))
        assert math.isnan(float(m.total)) and math.isnan(float(m.result())) and float(m.count) == n
        m.update_state(_dev(yy), _dev(pp))                                            # a clean batch afterwards: still NaN
        assert math.isnan(float(m.total)) and math.isnan(float(m.result())) and float(m.count) == 2 * n
        m.reset_states()
        m.update_state(_dev(yy), _dev(pp))
        assert math.isfinite(float(m.result()))
    inf = p.copy()
    inf[7], inf[8] = np.inf, -np.inf
    m = metrics.BinaryCrossentropy()
    m.update_state(Y, _dev(inf))
    vals = ref.values_bce(y, inf)
    assert np.isfinite(vals).all() and abs(float(m.total) - vals.astype(np.float64).sum()) <= _bar(vals)
    lab = y.copy()
    lab[9] = np.inf                                                                   # an infinite label: inf * log, an infinite loss
    m.reset_states()
    m.update_state(_dev(lab), _dev(p))
    assert not math.isfinite(float(m.total)) and not math.isfinite(float(m.result()))
    # Mean: inf stays inf, inf - inf and NaN are NaN, and they stay
    for special, check in ((np.inf, lambda x: x == math.inf), (-np.inf, lambda x: x == -math.inf), (np.nan, math.isnan)):
        w = v.copy()
        w[100] = special
        m = metrics.Mean()
        m.update_state(_dev(w))
        assert check(float(m.total)) and check(float(m.result()))
        m.update_state(_dev(v))
        assert check(float(m.total)) and check(float(m.result())) and float(m.count) == 8192
    w = v.copy()
    w[1], w[4000] = np.inf, -np.inf
    m = metrics.Mean()
    m.update_state(_dev(w))
    assert math.isnan(float(m.total)) and math.isnan(float(m.result()))
    # accuracy: a NaN score is not above any threshold -- a predicted 0; nothing becomes NaN
    q = p.copy()
    q[::7] = np.nan
    a = metrics.BinaryAccuracy()
    a.update_state(Y, _dev(q))
    r = ref.MeanState().update_accuracy(y, q)
    assert float(a.total) == r.total and float(a.result()) == r.result()


def test_accuracy_threshold_edges():
    below, above = np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1))
    p = np.asarray([0.5, 0.5, below, below, above, above, 0.0, 0.0, 1.0, 1.0, 0.9, 0.9, 0.9, 0.1, 0.1, -0.0, 1e-45], f32)
    y = np.asarray([0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.7, 2.0, 1.0, 0.7, 2.0, 0.0, 1.0], f32)
    P, Y = _dev(p), _dev(y)
    for thr, want in ((0.5, 7), (0.0, 8), (1.0, 6)):
        m = metrics.BinaryAccuracy(threshold=thr)
        m.update_state(Y, P)
        r = ref.MeanState().update_accuracy(y, p, thr)
        assert r.total == want, (thr, r.total)                                        # by hand: a strict >, and 0.7 / 2 never match
        assert (float(m.total), float(m.count)) == (want, len(p)) and float(m.result()) == float(r.result())
        for i in range(len(p)):                                                       # sample by sample
            st = Fn.mean_update("binary_accuracy", P[i:i + 1], Y[i:i + 1], _state(), thr).cpu().numpy()
            assert st[0] == float(ref.matches(y[i:i + 1], p[i:i + 1], thr)[0]) and st[1] == 1, (thr, i)
    # labels of another dtype are cast to float32 (Keras' cast to y_pred.dtype), scores in float64 too
    m = metrics.BinaryAccuracy()
    m.update_state(torch.tensor(y.astype(np.int64), device="cuda").reshape(-1, 1), _dev(p, torch.float64).reshape(-1, 1))
    r = ref.MeanState().update_accuracy(y.astype(np.int64).astype(f32), p)
    assert float(m.total) == r.total and float(m.count) == len(p)
    with pytest.raises(ValueError, match="y_true has 3 elements, y_pred 4"):
        m.update_state(Y[:3], P[:4])


# ------------------------------------------------------------------------------------------------ 3. accumulation
def test_count_past_2_pow_24_rounds_like_keras_fp32_assign_add():
    m = metrics.Mean().build("cuda")
    sd = dict(state=torch.tensor([5.0, 2.0 ** 24, 0.0]))
    m.load_state_dict(sd)
    one = _dev([1.0])
    m.update_state(one)
    assert float(m.count) == 2.0 ** 24 and float(m.total) == 6.0                       # 2^24 + 1 is not a float32: the count stays
    _check_result_bits(m.state.cpu().numpy())
    m.load_state_dict(sd)
    m.update_state(_dev([1.0, 1.0]))
    assert float(m.count) == 2.0 ** 24 + 2 and float(m.total) == 7.0
    a = metrics.BinaryAccuracy().build("cuda")
    a.load_state_dict(dict(state=torch.tensor([2.0 ** 24, 2.0 ** 24, 1.0])))
    a.update_state(_dev([1.0]), _dev([0.9]))
    assert float(a.total) == 2.0 ** 24 and float(a.count) == 2.0 ** 24
    a.update_state(_dev([1.0, 1.0, 0.0]), _dev([0.9, 0.8, 0.7]))
    assert float(a.total) == 2.0 ** 24 + 2 and float(a.count) == f32(f32(2.0 ** 24) + f32(3))


def test_fifty_updates_equal_the_restatement():
    """Accuracy is bit-equal.  Mean is fed multiples of 1/8 of at most 2, whose float32 sums (below 2^21 eighths in all) are exact in any order: bit-equal too.
    Binary cross-entropy: every update adds its own bar, and each of the state's fifty additions rounds once, by at most 2^-24 of
    the (positive, growing) total."""
    rng = np.random.default_rng(50)
    mean, bce, acc = metrics.Mean(), metrics.BinaryCrossentropy(), metrics.BinaryAccuracy()
    r_mean, r_bce, r_acc = ref.MeanState(), ref.MeanState(), ref.MeanState()
    exact, bar = 0.0, 0.0
    for s in range(50):
        n = (4096, 1000, ONE + 3)[s % 3]
        y, p, _ = _case(n, seed=500 + s)
        v = (rng.integers(-16, 16, n) / 8.0).astype(f32)
        shape = (-1, 8) if n % 8 == 0 else (-1,)
        mean.update_state(_dev(v).reshape(shape))                                     # any shape, flattened
        bce.update_state(_dev(y).reshape(shape), _dev(p).reshape(shape))
        acc.update_state(_dev(y), _dev(p))
        r_mean.update_values(v)
        r_bce.update_bce(y, p)
        r_acc.update_accuracy(y, p)
        vals = ref.values_bce(y, p)
        exact += vals.astype(np.float64).sum()
        bar += _bar(vals)
    assert mean.state.cpu().numpy()[:2].tobytes() == np.asarray([r_mean.total, r_mean.count], f32).tobytes()
    assert acc.state.cpu().numpy().tobytes() == np.asarray([r_acc.total, r_acc.count, r_acc.result()], f32).tobytes()
    st = bce.state.cpu().numpy()
    assert st[1] == r_bce.count and abs(float(st[0]) - exact) <= bar + 50 * U * exact, (st, exact, bar)
    assert abs(float(st[0]) - float(r_bce.total)) <= bar + 100 * U * exact
    for m in (mean, bce, acc):
        _check_result_bits(m.state.cpu().numpy())
        assert m.total.data_ptr() == m.state.data_ptr() and m.count.data_ptr() == m.state[1].data_ptr()


def test_repeats_give_the_same_bits_reset_keeps_pointers_and_state_dict_round_trips():
    for cls in (metrics.Mean, metrics.BinaryCrossentropy, metrics.BinaryAccuracy):
        m = cls().build("cuda")
        ptrs = (m.state.data_ptr(), m.result().data_ptr())
        for n in (4096, 300001):                                                      # both launch paths
            y, p, v = _case(n, seed=n)
            args = (_dev(v),) if cls is metrics.Mean else (_dev(y), _dev(p))
            outs = []
            for _ in range(3):
                m.reset_states()
                m.state[:2].copy_(torch.tensor([123.25, 77.0]))
                m.update_state(*args)
                outs.append(m.state.clone())
            assert all(torch.equal(o, outs[0]) for o in outs) and float(outs[0][1]) == 77.0 + n
            _check_result_bits(outs[0].cpu().numpy())
        m.reset_states()
        assert (m.state.data_ptr(), m.result().data_ptr()) == ptrs and float(m.state.abs().sum()) == 0 and float(m.result()) == 0
        m.update_state(*args)
        sd = m.state_dict()
        m2 = cls()
        m2.load_state_dict(sd)
        assert torch.equal(m2.state, m.state) and m2.state.data_ptr() != m.state.data_ptr()
        m.reset_states()
        m.load_state_dict(sd)
        assert torch.equal(m2.state, m.state) and m.state.data_ptr() == ptrs[0]
        m.load_state_dict(cls().state_dict())                                         # an empty checkpoint: back to nothing seen
        assert float(m.state.abs().sum()) == 0


def test_layer_equals_the_raw_entry_point_with_a_garbage_workspace():
    import ctypes
    lib = _lib.load()
    for n in (ONE, ONE + 1, 250001):
        y, p, _ = _case(n, seed=n)
        Y, P = _dev(y), _dev(p)
        m = metrics.BinaryCrossentropy()
        m.update_state(Y, P)
        need = lib.fil_mean_workspace_bytes(n)
        ws = torch.full((max(need, 1),), 0xAB, dtype=torch.uint8, device="cuda")      # garbage: needs no initialisation
        st = torch.zeros(3, device="cuda")
        rc = lib.fil_mean_update(_lib.FIL_MEAN_BCE, P.data_ptr(), Y.data_ptr(), n, 1e-7, 0.0, st.data_ptr(), ws.data_ptr() if need else None,
                                 need, ctypes.c_void_p(_lib.stream_ptr()))
        assert rc == 0, lib.fil_last_error()
        torch.cuda.synchronize()
        assert torch.equal(st, m.state), n


# ------------------------------------------------------------------------------------------------ 4. Precision and Recall
def _check_confusion(m_p, m_r, c):
    for m in (m_p, m_r):
        for name, want in (("true_positives", c.tp), ("false_positives", c.fp), ("true_negatives", c.tn), ("false_negatives", c.fn)):
            assert np.array_equal(getattr(m, name).cpu().numpy(), want), (type(m).__name__, name)
        assert int(m.invalid) == c.invalid
    for m, want in ((m_p, c.precision()), (m_r, c.recall())):
        got = m.result()
        assert got.dtype == torch.float32 and tuple(got.shape) == (() if len(c.thr) == 1 else (len(c.thr),))
        assert got.cpu().numpy().tobytes() == (want[0] if len(c.thr) == 1 else want).tobytes(), (type(m).__name__, got, want)


@pytest.mark.parametrize("thresholds", [None, 0.3, [0.5, 0.0, 1.0, 0.25], [0.7, 0.7, 0.1]])
def test_precision_and_recall_equal_the_restatement(thresholds):
    m_p, m_r = metrics.Precision(thresholds), metrics.Recall(thresholds=thresholds)
    c = ref.ConfusionState(thresholds)
    _check_confusion(m_p.build("cuda"), m_r.build("cuda"), c)                         # the empty state: 0, not NaN
    for n in (300, 4097, 50001):
        y, p, _ = _case(n, seed=n + 3)
        p[:len(c.thr)] = c.thr                                                        # scores exactly on the thresholds (strict >)
        y[::5] = 2.0                                                                  # any non-zero label is a positive
        for m in (m_p, m_r):
            m.update_state(_dev(y).reshape(-1, 1), _dev(p).reshape(-1, 1))
        c.update(y, p)
        _check_confusion(m_p, m_r, c)
    want_p, want_r = c.precision(), c.recall()
    if len(c.thr) == 1:
        assert m_p.result_value() == float(want_p[0]) and m_r.result_value() == float(want_r[0])
    else:
        assert m_p.result_value() == [float(x) for x in want_p] and m_r.result_value() == [float(x) for x in want_r]
    # reset in place, checkpoint round trip
    ptr_, res = m_p.confusion.data_ptr(), m_p.result()
    sd = m_p.state_dict()
    m_p.reset_states()
    assert m_p.confusion.data_ptr() == ptr_ and float(m_p.confusion.abs().sum()) == 0 and float(m_p.result().abs().sum()) == 0
    m_p.load_state_dict(sd)
    assert m_p.result() is res and res.cpu().numpy().tobytes() == (want_p[0] if len(c.thr) == 1 else want_p).tobytes()
    m2 = metrics.Precision(thresholds)
    m2.load_state_dict(sd)
    assert torch.equal(m2.confusion, m_p.confusion)


def test_precision_and_recall_one_class_batches_and_scores_outside_the_unit_interval():
    y, p, _ = _case(5000, seed=9)
    for lab in (np.ones(5000, f32), np.zeros(5000, f32)):
        m_p, m_r = metrics.Precision(), metrics.Recall()
        m_p.update_state(_dev(lab), _dev(p))
        m_r.update_state(_dev(lab), _dev(p))
        _check_confusion(m_p, m_r, ref.ConfusionState().update(lab, p))
        assert m_r.result_value() == (0.0 if lab[0] == 0 else float(m_r.result())) and m_p.result_value() in (0.0, 1.0)
    low = np.minimum(p, f32(0.4))                                                     # nothing predicted positive: precision 0 / 0 = 0
    m_p = metrics.Precision()
    m_p.update_state(_dev(y), _dev(low))
    assert m_p.result_value() == 0.0
    bad = p.copy()
    bad[:6] = [np.nan, np.inf, -0.25, 1.5, -np.inf, np.nextafter(f32(1), f32(2))]
    for cls in (metrics.Precision, metrics.Recall):
        m = cls(thresholds=[0.9, 0.2])
        m.update_state(_dev(y), _dev(bad))
        m.update_state(_dev(y[6:]), _dev(p[6:]))                                      # a clean batch afterwards does not clear the counter
        c = ref.ConfusionState([0.9, 0.2]).update(y, bad).update(y[6:], p[6:])
        assert c.invalid == 6 and int(m.invalid) == 6
        assert np.array_equal(m.true_positives.cpu().numpy(), c.tp) and np.array_equal(m.false_negatives.cpu().numpy(), c.fn)
        m.result()                                                                    # result() does not check ...
        with pytest.raises(ValueError, match="%s: 6 predictions" % cls.__name__):
            m.result_value()                                                          # ... result_value() does
        m.reset_states()
        assert m.result_value() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 5. capture
def _five():
    return [metrics.Mean().build("cuda"), metrics.BinaryCrossentropy(label_smoothing=0.1).build("cuda"),
            metrics.BinaryAccuracy().build("cuda"), metrics.Precision(thresholds=[0.5, 0.1]).build("cuda"), metrics.Recall().build("cuda")]


def _update_five(ms, y, p, v):
    ms[0].update_state(v)
    for m in ms[1:]:
        m.update_state(y, p)
    return [m.result() for m in ms]


def _states(ms):
    return [(m.state if hasattr(m, "state") else m.confusion).clone() for m in ms] + [m.result().clone() for m in ms]


def _eager_reference(batches):
    ms = _five()
    want = []
    for y, p, v in batches:
        _update_five(ms, _dev(y), _dev(p), _dev(v))
        want.append(_states(ms))
    return want


def test_all_five_inside_a_hip_graph():
    batches = [_case(4096, seed=700 + s) for s in range(6)]
    want = _eager_reference(batches)
    ms = _five()
    Y, P, V = (_dev(a) for a in batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _update_five(ms, Y, P, V)
    torch.cuda.current_stream().wait_stream(side)
    for m in ms:
        m.reset_states()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = _update_five(ms, Y, P, V)
    for m in ms:
        m.reset_states()
    for k, (y, p, v) in enumerate(batches):
        Y.copy_(_dev(y))
        P.copy_(_dev(p))
        V.copy_(_dev(v))
        g.replay()
        got = _states(ms)
        assert all(torch.equal(a, b) for a, b in zip(got, want[k])), k                # k replays = k eager updates, bit for bit
        for m, r in zip(ms[:3], res[:3]):
            assert m.result() is r and torch.equal(r, m.state[2])                     # the same object, current after the replay
        for r, w in zip(res, want[k][5:]):
            assert torch.equal(r, w), k


def test_all_five_through_capture_step():
    batches = [_case(4096, seed=800 + s) for s in range(6)]
    want = _eager_reference(batches)
    ms = _five()

    def step(y, p, v):
        return tuple(_update_five(ms, y, p, v))

    def restore():
        for m in ms:
            m.reset_states()

    captured = capture.capture_step(step, *(_dev(a) for a in batches[0]), restore=restore)
    first = None
    for k, (y, p, v) in enumerate(batches):
        out = captured(_dev(y), _dev(p), _dev(v))
        first = out if first is None else first
        assert all(a is b for a, b in zip(out, first))                                # the same static tensors after every replay
        assert all(torch.equal(a, b) for a, b in zip(out, want[k][5:])), k
        assert all(torch.equal(a, b) for a, b in zip(_states(ms), want[k])), k        # the warm-up runs were undone by restore
    assert all(m.result() is r for m, r in zip(ms, out))


# ------------------------------------------------------------------------------------------------ 6. the metrics do not perturb training
def test_metrics_inside_the_captured_training_step_change_no_parameter_bit():
    vocab = [7, 11, 5, 13]
    B, K = 256, 8
    rng = np.random.default_rng(5)
    batches = []
    for s in range(8):
        r = np.random.default_rng(40 + s)
        dense = torch.tensor(r.random((B, 3)), dtype=torch.float32, device="cuda")
        idx = torch.tensor(np.stack([r.integers(0, v, B) for v in vocab], 1), device="cuda")
        batches.append((dense, idx, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def run(with_metrics):
        torch.manual_seed(7)
        info = [i._replace(emb_reg=1e-3) for i in models.make_sparse_info(vocab, embed_dim=K)]
        fi = models.FeatureInput(sparseInfo=info, useLinear=True, useFlattenLinear=True, tableGrad="runs")
        model = models.CTRModel(fi, models.DeepFM(hidden_units=[32, 16])).cuda()
        model(batches[0][0], batches[0][1])
        opt = optim.Adam(model.parameters())
        ms = ([metrics.Mean(name="loss").build("cuda"), metrics.BinaryCrossentropy().build("cuda"), metrics.BinaryAccuracy().build("cuda"),
               metrics.Precision().build("cuda"), metrics.Recall().build("cuda")] if with_metrics else [])

        def step(dense, idx, y):
            opt.zero_grad()
            p = model(dense, idx)[:, 1]
            bce = losses.binary_crossentropy(p, y, eps=1e-7)
            (bce + collect_regularization_loss(model)).backward()
            opt.step()
            if ms:
                ms[0].update_state(bce)
                for m in ms[1:]:
                    m.update_state(y, p)
            return (p.detach(), bce.detach()) + tuple(m.result() for m in ms)

        init = {k: v.clone() for k, v in model.state_dict().items()}

        def restore():
            with torch.no_grad():
                for k, v in model.state_dict().items():
                    v.copy_(init[k])
            opt.reset_()
            for m in ms:
                m.reset_states()

        captured = capture.capture_step(step, *batches[0], restore=restore)
        ps, ls = [], []
        for bt in batches:
            out = captured(*bt)
            ps.append(out[0].clone())
            ls.append(out[1].clone())
        torch.cuda.synchronize()
        slots = [v.clone() for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]
        return model, slots, ps, ls, ms, out

    model_a, slots_a, ps_a, ls_a, ms, out = run(True)
    model_b, slots_b, ps_b, ls_b, _, _ = run(False)
    for (n, a), (_, b) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert torch.equal(a, b), n
    assert len(slots_a) == len(slots_b) > 0 and all(torch.equal(a, b) for a, b in zip(slots_a, slots_b))
    assert all(torch.equal(a, b) for a, b in zip(ps_a + ls_a, ps_b + ls_b))
    # and what the metrics saw is what the step computed
    y = np.concatenate([bt[2].cpu().numpy() for bt in batches])
    p = np.concatenate([q.cpu().numpy() for q in ps_a])
    r_loss, r_bce, r_acc, conf = ref.MeanState(), ref.MeanState(), ref.MeanState(), ref.ConfusionState()
    bar = 0.0
    for k in range(len(batches)):
        sl = slice(k * B, (k + 1) * B)
        r_loss.update_values([float(ls_a[k])])
        r_bce.update_bce(y[sl], p[sl])
        r_acc.update_accuracy(y[sl], p[sl])
        conf.update(y[sl], p[sl])
        bar += _bar(ref.values_bce(y[sl], p[sl]))
    assert (float(ms[0].total), float(ms[0].count)) == (float(r_loss.total), len(batches))
    assert abs(float(ms[1].total) - float(r_bce.total)) <= bar + 2 * len(batches) * U * float(r_bce.total) and float(ms[1].count) == len(y)
    assert ms[2].state.cpu().numpy().tobytes() == np.asarray([r_acc.total, r_acc.count, r_acc.result()], f32).tobytes()
    assert float(ms[3].result()) == float(conf.precision()[0]) and float(ms[4].result()) == float(conf.recall()[0])
    assert all(torch.equal(o, m.result()) for o, m in zip(out[2:], ms))


# ------------------------------------------------------------------------------------------------ 7. data parallel
def test_result_through_a_one_rank_rccl_group():
    import torch.distributed as dist
    import bench
    device = torch.device("cuda", 0)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with bench.stdout_to_stderr():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=device)
    try:
        y, p, v = _case(30000, seed=1)
        ms = _five()
        _update_five(ms, _dev(y), _dev(p), _dev(v))
        before = _states(ms)
        for _ in range(2):                                                            # mid-epoch, repeatedly
            for m in ms:
                got = m.result(process_group=dist.group.WORLD)
                assert got.shape == m.result().shape and got.data_ptr() != m.result().data_ptr()
                assert torch.equal(got, m.result())
        assert ms[4].result_value(process_group=dist.group.WORLD) == float(ms[4].result())
        assert all(torch.equal(a, b) for a, b in zip(_states(ms), before))            # the local state is not touched
        ms[3].update_state(_dev(y[:10]), _dev(p[:10] + 2.0))
        with pytest.raises(ValueError, match="10 predictions"):
            ms[3].result_value(process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
