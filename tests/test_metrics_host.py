"""Host-only checks of Keras' streaming AUC (include/fil.h M1, ml_function_amd/metrics.py: AUC): the entry points in the header,
the binding and the library; their argument validation through ctypes, in-process and under the ASan/UBSan build; the Python
surface that needs no GPU; and self-checks of the numpy restatement (tests/keras_auc_ref.py) the GPU tests are held to."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, metrics
from tests import keras_auc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_confusion_workspace_bytes", "fil_confusion_update", "fil_auc_result")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_metrics_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    assert "#define FIL_CONFUSION_MAX_T %d\n" % _lib.FIL_CONFUSION_MAX_T in header
    assert "#define FIL_CONFUSION_ONE_LAUNCH_N %d\n" % _lib.FIL_CONFUSION_ONE_LAUNCH_N in header
    assert _lib.FIL_CONFUSION_ONE_LAUNCH_N >= 4096 and _lib.FIL_CONFUSION_MAX_T >= 1000


def test_metrics_entry_points_validate(lib):
    from tests import host_calls_metrics
    assert host_calls_metrics.run(lib) >= 30


def test_metrics_entry_points_under_asan_ubsan():
    """host_calls_metrics.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_metrics.py"), asan_lib], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "metrics host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]


def test_auc_constructor_defaults_names_and_errors():
    m = metrics.AUC()
    assert (m.num_thresholds, m.curve, m.summation_method, m.name, m.dtype) == (200, "ROC", "interpolation", "auc", torch.float32)
    assert isinstance(m.thresholds, list) and len(m.thresholds) == 200 and all(type(t) is float for t in m.thresholds)
    assert m.thresholds[0] == -1e-7 and m.thresholds[1] == 1.0 / 199 and m.thresholds[-1] == 1.0 + 1e-7
    assert m.true_positives is None and m.confusion is None                       # the state appears on the first update's device
    assert metrics.AUC(curve="PR", summation_method="majoring", name="pr").name == "pr"
    assert metrics.AUC(curve="pr").curve == "PR"
    for bad in (dict(num_thresholds=1), dict(num_thresholds=0), dict(num_thresholds=-5)):
        with pytest.raises(ValueError, match="num_thresholds"):
            metrics.AUC(**bad)
    with pytest.raises(ValueError, match="curve"):
        metrics.AUC(curve="DET")
    with pytest.raises(ValueError, match="summation"):
        metrics.AUC(summation_method="trapezoid")
    for bad in ([0.5, 1.5], [-0.1], [0.2, float("nan")]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            metrics.AUC(thresholds=bad)
    with pytest.raises(ValueError, match="FIL_CONFUSION_MAX_T"):
        metrics.AUC(num_thresholds=_lib.FIL_CONFUSION_MAX_T + 1)
    assert float(m.result()) == 0.0 and m.result_value() == 0.0                    # Keras: 0.0 before any update, no error


def test_auc_thresholds_equal_the_restatement_bit_for_bit():
    for T in (2, 3, 7, 200, 201, 1000, _lib.FIL_CONFUSION_MAX_T):
        got = np.asarray(metrics.AUC(num_thresholds=T).thresholds, np.float32)
        assert got.tobytes() == ref.thresholds(T).tobytes(), T
    user = [0.7, 0.1, 0.5, 0.5, 1.0, 0.0, 1e-40]
    m = metrics.AUC(num_thresholds=17, thresholds=user)                            # a list wins over num_thresholds
    assert m.num_thresholds == len(user) + 2 and m.thresholds[1:-1] == sorted(user)
    assert np.asarray(m.thresholds, np.float32).tobytes() == ref.thresholds(user=user).tobytes()
    t = ref.thresholds()
    assert t[0] == np.float32(-1e-7) and t[-1] == np.float32(1) + np.float32(2.0 ** -23)
    assert np.float32(0.0) > t[0] and not np.float32(1.0) > t[-1]


def test_auc_refuses_sample_weight_and_cpu_tensors():
    m = metrics.AUC()
    y, p = torch.zeros(4), torch.full((4,), 0.5)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        m.update_state(y, p, sample_weight=torch.ones(4))
    with pytest.raises(_lib.FilError, match="GPU"):
        m.update_state(y, p)
    with pytest.raises(_lib.FilError, match="GPU"):
        m.build("cpu")
    from ml_function_amd import functional as Fn
    with pytest.raises(_lib.FilError, match="GPU"):
        Fn.confusion_update(p, y, torch.zeros(200), torch.zeros(4, 200), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(_lib.FilError, match="GPU"):
        Fn.auc_result(torch.zeros(4, 200))
    assert m.confusion is None


# ---- the restatement checked against itself (these hold on any commit: they guard the yardstick)
def _case(seed, n, skewed):
    rng = np.random.default_rng(seed)
    logit = rng.normal(-3.5 if skewed else 0.0, 1.0, n)
    p = (1.0 / (1.0 + np.exp(-(logit + rng.normal(0, 1.0, n))))).astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    return y, p


@pytest.mark.parametrize("skewed", [False, True])
def test_restatement_bucket_counting_equals_the_comparison(skewed):
    y, p = _case(1, 20000, skewed)
    for thr in (ref.thresholds(), ref.thresholds(2), ref.thresholds(3), ref.thresholds(1000), ref.thresholds(user=[0.5, 0.25, 0.5, 0.0, 1.0])):
        q = p.copy()
        q[:len(thr)] = thr.clip(0, 1)                                             # scores exactly on the stored thresholds
        q[len(thr):len(thr) + 4] = [0.0, 1.0, -0.0, 1e-45]
        a, b, c = ref.counts(y, q, thr), ref.bucket_counts(y, q, thr), ref.counts_chunked(y, q, thr, chunk=777)
        for x, z, w in zip(a, b, c):
            assert np.array_equal(x, z) and np.array_equal(x, w)
        tp, fp, tn, fn = a
        assert (tp + fn == (y != 0).sum()).all() and (fp + tn == (y == 0).sum()).all()
        assert tp[0] == (y != 0).sum() and tp[-1] == 0                            # every score is above -1e-7, none above 1 + 2^-23


@pytest.mark.parametrize("skewed", [False, True])
def test_restatement_brackets_the_exact_auc(skewed):
    y, p = _case(2, 65536, skewed)
    c = ref.counts(y, p, ref.thresholds())
    lo, mid, hi = (float(ref.result(*c, "ROC", m, np.float64)) for m in ("minoring", "interpolation", "majoring"))
    exact = metrics.auc(torch.tensor(y), torch.tensor(p))
    assert lo <= exact <= hi and lo <= mid <= hi, (lo, mid, exact, hi)


def test_restatement_counts_of_shards_add_up_and_degenerate_states_give_zero():
    y, p = _case(3, 30000, True)
    thr = ref.thresholds()
    whole = ref.counts(y, p, thr)
    parts = [ref.counts(y[lo:lo + 7000], p[lo:lo + 7000], thr) for lo in range(0, 30000, 7000)]
    for k in range(4):
        assert np.array_equal(whole[k], sum(part[k] for part in parts))
    zero = [np.zeros(200)] * 4
    one_class = ref.counts(np.ones(100), p[:100], thr)
    for curve in ref.CURVES:
        for method in ref.METHODS:
            assert ref.result(*zero, curve, method) == 0.0
            if curve == "ROC":
                assert ref.result(*one_class, curve, method) == 0.0
