"""Host-only checks of Keras' Mean, BinaryCrossentropy, BinaryAccuracy, Precision and Recall (include/fil.h M2,
ml_function_amd/metrics.py): the entry points in the header, the binding and the library; their argument validation through ctypes;
the Python surface that needs no GPU; and self-checks of the numpy restatement (tests/keras_mean_metrics_ref.py) the GPU tests are
held to."""
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, metrics
from ml_function_amd import functional as Fn
from tests import keras_mean_metrics_ref as ref

NEW = ("fil_mean_workspace_bytes", "fil_mean_update")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_mean_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    for macro in ("FIL_MEAN_VALUES", "FIL_MEAN_BCE", "FIL_MEAN_BINARY_ACC", "FIL_MEAN_ONE_LAUNCH_N"):
        assert "#define %s %d\n" % (macro, getattr(_lib, macro)) in header, macro
    assert (_lib.FIL_MEAN_VALUES, _lib.FIL_MEAN_BCE, _lib.FIL_MEAN_BINARY_ACC) == (0, 1, 2)
    assert 4096 <= _lib.FIL_MEAN_ONE_LAUNCH_N < 1 << 20
    assert Fn.MEAN_KINDS == {"values": 0, "binary_crossentropy": 1, "binary_accuracy": 2}


def test_mean_entry_points_validate(lib):
    from tests import host_calls_metrics_mean
    assert host_calls_metrics_mean.run(lib) >= 50


def test_constructor_defaults_and_names():
    m = metrics.Mean()
    assert (m.name, m.dtype, m.state, m.total, m.count) == ("mean", torch.float32, None, None, None)
    assert metrics.Mean(name="loss").name == "loss"
    b = metrics.BinaryCrossentropy()
    assert (b.name, b.from_logits, b.label_smoothing, b._constants()) == ("binary_crossentropy", False, 0.0, (1e-7, 0.0))
    assert metrics.BinaryCrossentropy(label_smoothing=0.1, name="logloss")._constants() == (1e-7, 0.1)
    a = metrics.BinaryAccuracy()
    assert (a.name, a.threshold) == ("binary_accuracy", 0.5) and metrics.BinaryAccuracy(threshold=0.25).threshold == 0.25
    for cls, name in ((metrics.Precision, "precision"), (metrics.Recall, "recall")):
        m = cls()
        assert (m.name, m.thresholds, m.top_k, m.class_id, m.dtype) == (name, [0.5], None, None, torch.float32)
        assert m.confusion is None and m.true_positives is None and m.false_negatives is None
        assert cls(thresholds=0.3).thresholds == [0.3] and cls(0.3, name="x").name == "x"
        assert cls(thresholds=[0.5, 0.0, 1.0, 0.25]).thresholds == [0.5, 0.0, 1.0, 0.25]           # used as given, in the given order
        assert cls(thresholds=[0.5, 0.0, 1.0, 0.25])._sorted == [0.0, 0.25, 0.5, 1.0] and cls()._sorted == [0.5, 0.5]
    # Keras' argument names, in Keras' order
    assert list(inspect.signature(metrics.Mean).parameters) == ["name", "dtype"]
    assert list(inspect.signature(metrics.BinaryCrossentropy).parameters) == ["name", "dtype", "from_logits", "label_smoothing"]
    assert list(inspect.signature(metrics.BinaryAccuracy).parameters) == ["name", "dtype", "threshold"]
    assert list(inspect.signature(metrics.Precision).parameters) == ["thresholds", "top_k", "class_id", "name", "dtype"]


def test_constructor_errors():
    with pytest.raises(NotImplementedError, match="from_logits"):
        metrics.BinaryCrossentropy(from_logits=True)
    for cls in (metrics.Precision, metrics.Recall):
        with pytest.raises(NotImplementedError, match="top_k"):
            cls(top_k=3)
        with pytest.raises(NotImplementedError, match="class_id"):
            cls(class_id=0)
        for bad in ([0.5, 1.5], [-0.1], -0.1, 1.0000001, [0.2, float("nan")], [None]):
            with pytest.raises(ValueError, match=r"Threshold values must be in \[0, 1\]. Invalid values: "):
                cls(thresholds=bad)
        with pytest.raises(ValueError, match="FIL_CONFUSION_MAX_T"):
            cls(thresholds=[0.5] * (_lib.FIL_CONFUSION_MAX_T + 1))
    for cls in (metrics.Mean, metrics.BinaryCrossentropy, metrics.BinaryAccuracy, metrics.Precision, metrics.Recall):
        with pytest.raises(ValueError, match="dtype"):
            cls(dtype=torch.float64)
        assert cls(dtype="float32").dtype == torch.float32


def test_nothing_seen_gives_zero_and_no_state():
    for m in (metrics.Mean(), metrics.BinaryCrossentropy(), metrics.BinaryAccuracy(), metrics.Precision(), metrics.Recall()):
        r = m.result()
        assert r.dim() == 0 and r.dtype == torch.float32 and float(r) == 0.0             # Keras: 0.0 before any update
        m.reset_states()                                                              # a no-op, not an error
        with pytest.raises(_lib.FilError, match="no state yet"):
            m.result(process_group=object())
    assert metrics.Mean().state_dict() == {} and metrics.Precision().state_dict() == dict(thresholds=[0.5])
    p = metrics.Precision(thresholds=[0.9, 0.1])
    assert p.result().tolist() == [0.0, 0.0] and p.result_value() == [0.0, 0.0] and metrics.Recall().result_value() == 0.0
    with pytest.raises(ValueError, match="other thresholds"):
        p.load_state_dict(metrics.Precision().state_dict())


def test_sample_weight_cpu_tensors_and_non_tensors_are_refused():
    y, p = torch.zeros(4), torch.full((4,), 0.5)
    pairs = (metrics.BinaryCrossentropy(), metrics.BinaryAccuracy(), metrics.Precision(), metrics.Recall())
    for m in pairs:
        with pytest.raises(NotImplementedError, match="sample_weight is not supported .*order-independent"):
            m.update_state(y, p, sample_weight=torch.ones(4))
        with pytest.raises(_lib.FilError, match="GPU"):
            m.update_state(y, p)
        with pytest.raises(_lib.FilError, match="GPU"):
            m.build("cpu")
        with pytest.raises(TypeError, match="torch tensors"):
            m.update_state([0.0], [0.5])
    m = metrics.Mean()
    with pytest.raises(NotImplementedError, match="sample_weight is not supported .*order-independent"):
        m.update_state(p, sample_weight=torch.ones(4))
    with pytest.raises(_lib.FilError, match="GPU"):
        m.update_state(p)
    with pytest.raises(_lib.FilError, match="GPU"):
        m.build("cpu")
    with pytest.raises(TypeError, match="torch tensor"):
        m.update_state(0.5)
    for kind in Fn.MEAN_KINDS:
        with pytest.raises(_lib.FilError, match="GPU"):
            Fn.mean_update(kind, p, y, torch.zeros(3))
    with pytest.raises(_lib.FilError, match="kind"):
        Fn.mean_update("sum", p, y, torch.zeros(3))
    assert all(getattr(x, "state", None) is None and getattr(x, "confusion", None) is None for x in pairs + (m,))


# ---- the restatement checked against itself and by hand (these guard the yardstick)
def test_restatement_by_hand():
    s = ref.MeanState()
    assert s.result() == 0 and s.result().dtype == f32                                # an empty state gives 0, not NaN
    s.update_values([1.0, 2.0, 6.0])
    assert (s.total, s.count, s.result()) == (9.0, 3.0, 3.0)
    s.update_values([[1.0], [0.0]])
    assert (s.total, s.count, s.result()) == (10.0, 5.0, 2.0)
    # binary cross-entropy: the clip at epsilon and the epsilon inside the log, in float32
    eps = f32(1e-7)
    v = ref.values_bce([1, 0, 1, 0, 1], [0.5, 0.5, 1.0, 0.0, 0.0])
    assert v.dtype == f32
    assert v[0] == -np.log(f32(0.5) + eps) and v[1] == -np.log(f32(1) - f32(0.5) + eps)
    assert v[2] == -np.log(f32(1) - eps + eps) and v[3] == -np.log(f32(1) - eps + eps) and abs(v[2]) < 2e-7
    assert v[4] == -np.log(eps + eps) and 15.4 < v[4] < 15.5                         # a confident miss costs -log(2e-7), not infinity
    assert np.isnan(ref.values_bce([1], [np.nan])[0]) and np.isfinite(ref.values_bce([1], [np.inf])[0])      # the clip keeps a NaN only
    # label smoothing: y (1 - s) + 0.5 s
    ls = f32(0.1)
    ys = f32(1) * (f32(1) - ls) + f32(0.5) * ls
    assert ref.values_bce([1], [0.25], 0.1)[0] == -(ys * np.log(f32(0.25) + eps) + (f32(1) - ys) * np.log(f32(1) - f32(0.25) + eps))
    assert ref.values_bce([0.3], [0.25], 0.0)[0] != ref.values_bce([0.3], [0.25], 0.1)[0]
    # accuracy: a strict >, labels that are neither 0 nor 1 never match
    assert ref.matches([0, 1, 1, 0, 0.7, 2, 0], [0.5, 0.5, 0.6, 0.6, 0.9, 0.9, np.nan]).tolist() == [True, False, True, False, False, False, True]
    assert ref.matches([1, 0], [0.0, 0.0], threshold=0.0).tolist() == [False, True]
    a = ref.MeanState().update_accuracy([0, 1, 1, 0], [0.5, 0.5, 0.6, 0.6])
    assert (a.total, a.count, a.result()) == (2.0, 4.0, 0.5)


def test_restatement_state_is_float32_with_one_addition_per_update():
    s = ref.MeanState(count=2.0 ** 24)
    s.update_values([1.0])
    assert s.count == 2.0 ** 24 and s.total == 1.0                                    # fp32 assign_add: 2^24 + 1 rounds back
    s.update_values([1.0, 1.0])
    assert s.count == 2.0 ** 24 + 2
    t = ref.MeanState().update_values([np.nan]).update_values([1.0])
    assert np.isnan(t.total) and np.isnan(t.result()) and t.count == 2.0             # a NaN stays
    assert ref.MeanState().update_values([np.inf]).result() == np.inf


def test_restatement_shards_add_up():
    rng = np.random.default_rng(0)
    p = rng.random(3000, dtype=f32)
    y = (rng.random(3000) < p).astype(f32)
    whole, parts = ref.MeanState().update_accuracy(y, p), ref.MeanState()
    cw, cp = ref.ConfusionState([0.0, 0.25, 0.5, 1.0]).update(y, p), ref.ConfusionState([0.0, 0.25, 0.5, 1.0])
    for lo in range(0, 3000, 700):
        parts.update_accuracy(y[lo:lo + 700], p[lo:lo + 700])
        cp.update(y[lo:lo + 700], p[lo:lo + 700])
    assert (whole.total, whole.count) == (parts.total, parts.count) and whole.count == 3000
    for k in ("tp", "fp", "tn", "fn"):
        assert np.array_equal(getattr(cw, k), getattr(cp, k))
    assert (cw.tp + cw.fn == y.sum()).all() and (cw.fp + cw.tn == 3000 - y.sum()).all()
    # the float32 values of shards sum (in float64) to the whole's float64 sum
    v = ref.values_bce(y, p).astype(np.float64)
    assert abs(sum(v[lo:lo + 700].sum() for lo in range(0, 3000, 700)) - v.sum()) <= 1e-9 * v.sum()


def test_restatement_precision_and_recall_by_hand():
    y = [1, 1, 0, 0, 1, 2]
    p = [0.9, 0.4, 0.6, 0.1, 0.5, 0.7]
    c = ref.ConfusionState().update(y, p)                                             # 0.5, strict: p = 0.5 is a predicted negative
    assert (c.tp[0], c.fp[0], c.tn[0], c.fn[0]) == (2, 1, 1, 2)
    assert c.precision()[0] == f32(2) / f32(3) and c.recall()[0] == f32(0.5)
    c = ref.ConfusionState([1.0, 0.0]).update(y, p)
    assert c.precision().tolist() == [0.0, f32(4) / f32(6)] and c.recall().tolist() == [0.0, 1.0]     # nothing is above 1: 0 / 0 = 0
    e = ref.ConfusionState()
    assert e.precision()[0] == 0 and e.recall()[0] == 0
    assert ref.ConfusionState().update([0, 0], [0.9, 0.2]).recall()[0] == 0           # no positives
    assert ref.ConfusionState().update([1, 1], [0.1, 0.2]).precision()[0] == 0        # nothing predicted positive
    bad = ref.ConfusionState().update([1, 0, 1], [1.5, -0.1, np.nan])
    assert bad.invalid == 3 and bad.tp[0] == bad.fn[0] == 0
