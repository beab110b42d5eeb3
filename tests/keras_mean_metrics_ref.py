"""A numpy restatement of TensorFlow 2.1's Mean, BinaryCrossentropy, BinaryAccuracy, Precision and Recall metrics (keras/metrics.py:
Reduce / Mean / MeanMetricWrapper, Precision, Recall; keras/losses.py and keras/backend.py: binary_crossentropy;
keras/utils/metrics_utils.py: update_confusion_matrix_variables), single label, no sample weights -- the yardstick of
tests/test_metrics_mean_gpu.py.

Per-sample values are float32, operation by operation in Keras' order.  The state is float32 and takes ONE addition per update
(assign_add).  What Keras leaves open is the order of the float32 reduce_sum inside one update; `MeanState` sums in float64 and
rounds once, and `values_*` are there for tests that bound a kernel's own order against the float64 sum."""
import numpy as np

EPSILON = 1e-7          # K.epsilon()
f32 = np.float32


def values_bce(y, p, label_smoothing=0.0, eps=EPSILON):
    """Keras' per-sample binary_crossentropy on probabilities, float32 [n]."""
    y, p = np.asarray(y, f32), np.asarray(p, f32)
    eps, ls = f32(eps), f32(label_smoothing)
    with np.errstate(all="ignore"):
        if ls != 0:
            y = y * (f32(1) - ls) + f32(0.5) * ls
        pc = np.where(np.isnan(p), p, np.minimum(np.maximum(p, eps), f32(1) - eps)).astype(f32)      # clip_by_value keeps a NaN
        v = -(y * np.log(pc + eps) + (f32(1) - y) * np.log(f32(1) - pc + eps))
    assert v.dtype == f32
    return v


def matches(y, p, threshold=0.5):
    """equal(y_true, cast(y_pred > threshold, float32)), bool [n]."""
    y, p = np.asarray(y, f32), np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        return y == (p > f32(threshold)).astype(f32)


def div_no_nan(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        return np.where(b == 0, f32(0), a / np.where(b == 0, f32(1), b)).astype(f32)


class MeanState:
    """total, count: float32 scalars with one addition per update."""

    def __init__(self, total=0.0, count=0.0):
        self.total, self.count = f32(total), f32(count)

    def add(self, batch_sum, n):
        with np.errstate(all="ignore"):
            self.total = f32(self.total + f32(batch_sum))
            self.count = f32(self.count + f32(n))
        return self

    def update_values(self, v):
        v = np.asarray(v, f32).reshape(-1)
        with np.errstate(all="ignore"):
            return self.add(v.astype(np.float64).sum(), v.size)

    def update_bce(self, y, p, label_smoothing=0.0):
        return self.update_values(values_bce(np.asarray(y).reshape(-1), np.asarray(p).reshape(-1), label_smoothing))

    def update_accuracy(self, y, p, threshold=0.5):
        m = matches(np.asarray(y).reshape(-1), np.asarray(p).reshape(-1), threshold)
        return self.add(int(m.sum()), m.size)                  # an integer count, exact in float32 up to 2^24

    def result(self):
        return div_no_nan(self.total, self.count)[()]


class ConfusionState:
    """true_positives, false_positives, true_negatives, false_negatives at the given thresholds, in the given order: direct comparison
    `p > float32(threshold)`, any non-zero label positive, float32 state with one addition per update.  Scores outside [0, 1] (and
    NaN), where TensorFlow fails an assertion, are left out and counted in `invalid`."""

    def __init__(self, thresholds=None):
        thresholds = [0.5] if thresholds is None else list(np.atleast_1d(thresholds))
        self.thr = np.asarray(thresholds, np.float64).astype(f32)
        self.tp, self.fp, self.tn, self.fn = (np.zeros(len(self.thr), f32) for _ in range(4))
        self.invalid = 0

    def update(self, y, p):
        y, p = np.asarray(y).reshape(-1), np.asarray(p, f32).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok = (p >= 0) & (p <= 1)
        self.invalid += int((~ok).sum())
        pos, p = (y != 0)[ok], p[ok]
        above = p[None, :] > self.thr[:, None]
        self.tp = self.tp + (above & pos).sum(1).astype(f32)
        self.fp = self.fp + (above & ~pos).sum(1).astype(f32)
        self.tn = self.tn + (~above & ~pos).sum(1).astype(f32)
        self.fn = self.fn + (~above & pos).sum(1).astype(f32)
        return self

    def precision(self):
        return div_no_nan(self.tp, self.tp + self.fp)

    def recall(self):
        return div_no_nan(self.tp, self.tp + self.fn)
