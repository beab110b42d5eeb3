"""numpy restatement of tf.keras.metrics.AUC as TensorFlow 2.1 computes it (keras/metrics.py: AUC, keras/utils/metrics_utils.py:
update_confusion_matrix_variables): the yardstick of tests/test_metrics_host.py and tests/test_metrics_gpu.py.  Test infrastructure
only -- the product path is ml_function_amd.metrics.AUC on the GPU."""
import numpy as np

CURVES = ("ROC", "PR")
METHODS = ("interpolation", "minoring", "majoring")


def thresholds(num_thresholds=200, user=None):
    """float32 [T], T = num_thresholds (or len(user) + 2): K.epsilon() end points; python floats -> ONE rounding to fp32."""
    t = sorted(user) if user is not None else [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
    return np.asarray([0.0 - 1e-7] + t + [1.0 + 1e-7], np.float32)


def counts(y, p, thr):
    """Exact integers, int64 [T] each: TP, FP, TN, FN."""
    y = np.asarray(y) != 0                                # tf.cast(y_true, bool): ANY non-zero label is positive
    pos = np.asarray(p, np.float32)[None, :] > thr[:, None]          # strict >, compared in fp32
    return (pos & y).sum(1), (pos & ~y).sum(1), (~pos & ~y).sum(1), (~pos & y).sum(1)


def counts_chunked(y, p, thr, chunk=1 << 18):
    """counts() over slices of the samples, added up (the [T, N] comparison of a large N does not fit in memory)."""
    y, p = np.asarray(y), np.asarray(p, np.float32)
    tot = [np.zeros(len(thr), np.int64) for _ in range(4)]
    for lo in range(0, len(p), chunk):
        for a, c in zip(tot, counts(y[lo:lo + chunk], p[lo:lo + chunk], thr)):
            a += c
    return tuple(tot)


def bucket_counts(y, p, thr):
    """The same integers by bucket: b(p) = #{i : thr[i] < p}, TP[i] = #{y != 0, b > i}."""
    y = np.asarray(y) != 0
    b = np.searchsorted(thr, np.asarray(p, np.float32), side="left")
    T = len(thr)
    hp = np.bincount(b[y], minlength=T + 1).astype(np.int64)
    hn = np.bincount(b[~y], minlength=T + 1).astype(np.int64)
    sp, sn = np.cumsum(hp[::-1])[::-1], np.cumsum(hn[::-1])[::-1]          # #{b >= j}
    tp, fp = sp[1:], sn[1:]
    return tp, fp, sn[0] - fp, sp[0] - tp


def dnn(a, b):
    """tf.math.div_no_nan"""
    return np.where(b == 0, 0, a / np.where(b == 0, 1, b))


def result(tp, fp, tn, fn, curve="ROC", method="interpolation", dt=np.float32):
    tp, fp, tn, fn = [np.asarray(a, dt) for a in (tp, fp, tn, fn)]
    n = len(tp)
    if curve == "PR" and method == "interpolation":       # AUC.interpolate_pr_auc
        dtp = tp[:n - 1] - tp[1:]
        p = tp + fp
        dp = p[:n - 1] - p[1:]
        slope = dnn(dtp, np.maximum(dp, 0))
        inter = tp[1:] - slope * p[1:]
        ratio = np.where((p[:n - 1] > 0) & (p[1:] > 0), dnn(p[:n - 1], np.maximum(p[1:], 0)), np.ones_like(p[1:]))
        return np.sum(dnn(slope * (dtp + inter * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0)))
    rec = dnn(tp, tp + fn)
    x, yv = (dnn(fp, fp + tn), rec) if curve == "ROC" else (rec, dnn(tp, tp + fp))
    h = {"interpolation": (yv[:n - 1] + yv[1:]) / 2, "minoring": np.minimum(yv[:n - 1], yv[1:]),
         "majoring": np.maximum(yv[:n - 1], yv[1:])}[method]
    return np.sum((x[:n - 1] - x[1:]) * h)


def uniform_scores(rng, n):
    return rng.random(n, dtype=np.float32)


def skewed_scores(rng, n):
    """sigmoid of N(-3.5, 1): about 3 % mean, a CTR model's scores"""
    return (1.0 / (1.0 + np.exp(-rng.normal(-3.5, 1.0, n)))).astype(np.float32)
