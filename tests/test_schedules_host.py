"""Host-only checks of Keras' learning-rate schedules (include/fil.h O3, ml_function_amd/schedules.py): known answers of the numpy
restatement (tests/keras_schedules_ref.py) computed by hand, the package's own host evaluation against it, config round trips,
constructor errors, the entry points in the header, the binding and the library, and their argument validation through ctypes,
in-process and under the ASan/UBSan build."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from ml_function_amd import _lib, optim, schedules
from tests import keras_schedules_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the restatement's known answers (by hand: every value below is exact in float32 arithmetic or spelled as its float32 ops)
def test_exponential_known_answers():
    for staircase in (False, True):                     # at multiples of decay_steps the staircase changes nothing
        assert ref.exponential(0, 0.1, 10, 0.5, staircase) == f32(0.1)
        assert ref.exponential(10, 0.1, 10, 0.5, staircase) == f32(0.1) * f32(0.5)
        assert ref.exponential(20, 0.1, 10, 0.5, staircase) == f32(0.1) * f32(0.25)
    assert ref.exponential(15, 0.1, 10, 0.5, True) == f32(0.1) * f32(0.5)                   # floor(1.5) = 1
    assert ref.exponential(15, 0.1, 10, 0.5, False) == f32(0.1) * f32(np.float64(0.5) ** 1.5)
    assert ref.exponential(5, 1.0, 10, 0.25) == f32(0.5)                                   # 0.25 ** 0.5


def test_inverse_time_known_answers():
    assert ref.inverse_time(0, 0.5, 10, 1.0) == f32(0.5)
    assert ref.inverse_time(10, 0.5, 10, 1.0) == f32(0.25)                                 # 0.5 / (1 + 1)
    assert ref.inverse_time(30, 0.5, 10, 1.0) == f32(0.125)
    assert ref.inverse_time(5, 0.5, 10, 2.0) == f32(0.25)                                  # 0.5 / (1 + 2 * 0.5)
    assert ref.inverse_time(5, 0.5, 10, 2.0, staircase=True) == f32(0.5)                   # floor(0.5) = 0
    assert ref.inverse_time(19, 0.5, 10, 1.0, staircase=True) == f32(0.25)


def test_polynomial_known_answers():
    assert ref.polynomial(0, 1.0, 10, end=0.0) == f32(1)
    assert ref.polynomial(5, 1.0, 10, end=0.0) == f32(0.5)
    assert ref.polynomial(10, 1.0, 10, end=0.0) == f32(0)
    assert ref.polynomial(1000, 1.0, 10, end=0.25) == f32(0.25)                            # clipped at decay_steps: the end rate
    assert ref.polynomial(5, 1.0, 10, end=0.0, power=2.0) == f32(0.25)
    assert ref.polynomial(5, 1.0, 10, end=0.5, power=2.0) == f32(0.625)                    # 0.5 * 0.25 + 0.5
    # cycle: decay_steps stretches to the next multiple at or beyond the step; step 0 keeps it (multiplier 1, not ceil(0) = 0)
    assert ref.polynomial(0, 1.0, 10, end=0.0, cycle=True) == f32(1)
    assert ref.polynomial(10, 1.0, 10, end=0.0, cycle=True) == f32(0)                      # step == decay_steps: multiplier 1, p = 1
    assert ref.polynomial(15, 1.0, 10, end=0.0, cycle=True) == f32(0.25)                   # 1 - 15 / 20
    assert ref.polynomial(20, 1.0, 10, end=0.0, cycle=True) == f32(0)
    assert ref.polynomial(25, 1.0, 10, end=0.0, cycle=True) == f32(1) - f32(25) / f32(30)
    assert ref.polynomial(3, 0.1, 10) == (f32(0.1) - f32(0.0001)) * (f32(1) - f32(3) / f32(10)) + f32(0.0001)


def test_piecewise_known_answers():
    b, v = [10, 20], [1.0, 0.5, 0.25]
    assert [float(ref.piecewise(s, b, v)) for s in (0, 9, 10, 11, 19, 20, 21, 10 ** 9)] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25]
    assert ref.piecewise(7, [7], [0.3, 0.2]) == f32(0.3) and ref.piecewise(8, [7], [0.3, 0.2]) == f32(0.2)
    # integer comparisons: 2^24 + 1 is beyond a boundary at 2^24 although its float32 cast equals it
    assert ref.piecewise(2 ** 24 + 1, [2 ** 24], [1.0, 0.5]) == f32(0.5) and f32(2 ** 24 + 1) == f32(2 ** 24)


def test_decay_known_answers():
    assert ref.decayed(0.5, 0, 0.5) == f32(0.5)
    assert ref.decayed(0.5, 2, 0.5) == f32(0.25)
    assert ref.decayed(0.5, 6, 0.5) == f32(0.125)
    assert ref.decayed(0.5, 100, 0.0) == f32(0.5)
    # after the schedule
    s = schedules.InverseTimeDecay(0.5, 10, 1.0)
    assert ref.rate(s, 10, decay=0.1) == f32(0.25) / (f32(1) + f32(0.1) * f32(10))
    assert ref.rate(0.5, 2, decay=0.5) == f32(0.25)


def test_ulps():
    one = f32(1)
    assert ref.ulps(one, one) == 0 and ref.ulps(one, np.nextafter(one, f32(2))) == 1 and ref.ulps(np.nextafter(one, f32(0)), one) == 1
    assert ref.ulps(f32("nan"), f32("nan")) == 0 and ref.ulps(f32("nan"), one) > 1 and ref.ulps(f32(-0.0), f32(0.0)) == 0


# ---- the package's host evaluation (schedule(step)) is the same function
CASES = [schedules.ExponentialDecay(0.1, 10, 0.5), schedules.ExponentialDecay(1e-3, 1000, 0.96, staircase=True),
         schedules.InverseTimeDecay(0.01, 7, 0.3), schedules.InverseTimeDecay(0.01, 7, 0.3, staircase=True),
         schedules.PolynomialDecay(0.1, 100), schedules.PolynomialDecay(0.1, 100, cycle=True),
         schedules.PolynomialDecay(0.1, 100, end_learning_rate=1e-3, power=2.5), schedules.PolynomialDecay(0.1, 100, 1e-3, 0.5, True),
         schedules.PiecewiseConstantDecay([5, 50, 500], [1e-2, 5e-3, 1e-3, 1e-4])]
STEPS = [0, 1, 4, 5, 6, 7, 9, 10, 11, 49, 50, 51, 99, 100, 101, 999, 1000, 1001, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 5]


@pytest.mark.parametrize("sched", CASES, ids=lambda s: type(s).__name__)
def test_schedule_call_equals_the_restatement(sched):
    for step in STEPS:
        assert f32(sched(step)).tobytes() == ref.rate(sched, step).tobytes(), step
        for decay in (1e-3, 0.5):
            got = schedules.evaluate(sched.descriptor(decay), step)
            assert got.tobytes() == ref.rate(sched, step, decay).tobytes(), (step, decay)
    assert schedules.evaluate(schedules.constant_descriptor(0.01, 0.5), 6).tobytes() == ref.rate(0.01, 6, 0.5).tobytes()


# ---- configs
@pytest.mark.parametrize("sched", CASES, ids=lambda s: type(s).__name__)
def test_config_round_trips(sched):
    cfg = sched.get_config()
    again = type(sched).from_config(cfg)
    assert again.get_config() == cfg and again == sched
    ser = schedules.serialize(sched)
    assert ser == {"class_name": type(sched).__name__, "config": cfg}
    assert schedules.deserialize(ser) == sched
    assert pickle.loads(pickle.dumps(sched)) == sched
    assert bytes(sched.descriptor(0.25)) == bytes(schedules.deserialize(ser).descriptor(0.25))


def test_constructor_names_and_defaults():
    e = schedules.ExponentialDecay(initial_learning_rate=0.1, decay_steps=10, decay_rate=0.5)
    assert e.staircase is False and e.name is None
    i = schedules.InverseTimeDecay(initial_learning_rate=0.1, decay_steps=10, decay_rate=0.5)
    assert i.staircase is False
    p = schedules.PolynomialDecay(initial_learning_rate=0.1, decay_steps=10)
    assert (p.end_learning_rate, p.power, p.cycle) == (0.0001, 1.0, False)
    w = schedules.PiecewiseConstantDecay(boundaries=[1, 2], values=[0.3, 0.2, 0.1])
    assert w.boundaries == [1, 2] and w.values == [0.3, 0.2, 0.1]
    assert all(issubclass(c, schedules.LearningRateSchedule) for c in (type(e), type(i), type(p), type(w)))


def test_constructor_errors():
    with pytest.raises(ValueError, match="1 less"):
        schedules.PiecewiseConstantDecay([1, 2], [0.1, 0.2])
    with pytest.raises(ValueError, match="at most 32 boundaries"):
        schedules.PiecewiseConstantDecay(list(range(33)), [0.1] * 34)
    schedules.PiecewiseConstantDecay(list(range(32)), [0.1] * 33)
    with pytest.raises(ValueError, match="sorted"):
        schedules.PiecewiseConstantDecay([5, 3], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="integers"):
        schedules.PiecewiseConstantDecay([1.5], [0.1, 0.2])
    with pytest.raises(ValueError, match="1 ... 32"):
        schedules.PiecewiseConstantDecay([], [0.1])
    for cls in (schedules.ExponentialDecay, schedules.InverseTimeDecay):
        with pytest.raises(ValueError, match="decay_steps"):
            cls(0.1, 0, 0.5)
    with pytest.raises(ValueError, match="decay_steps"):
        schedules.PolynomialDecay(0.1, -4)
    with pytest.raises(ValueError, match="unknown learning-rate schedule"):
        schedules.deserialize({"class_name": "CosineDecay", "config": {}})
    with pytest.raises(TypeError):
        schedules.serialize(0.1)


def test_optimizers_take_a_schedule_and_decay_and_refuse_a_negative_decay():
    import torch
    p = [torch.nn.Parameter(torch.zeros(3))]
    s = schedules.ExponentialDecay(0.1, 10, 0.5)
    for cls in (optim.Adam, optim.Adagrad, optim.Ftrl):
        o = cls(p, learning_rate=s, decay=0.25)
        assert o.param_groups[0]["learning_rate"] is s and o.param_groups[0]["decay"] == 0.25
        assert "decay" not in cls(p).defaults and isinstance(cls(p).param_groups[0]["learning_rate"], float)     # unused: as before
        with pytest.raises(ValueError, match="decay cannot be less than 0"):
            cls(p, decay=-0.1)
        with pytest.raises(ValueError, match="learning_rate"):
            cls(p, learning_rate=-1.0)
        sd = o.state_dict()
        assert sd["param_groups"][0]["learning_rate"] == schedules.serialize(s) and sd["param_groups"][0]["decay"] == 0.25
        pickle.dumps(sd)
        fresh = cls(p)
        fresh.load_state_dict(sd)
        assert fresh.param_groups[0]["learning_rate"] == s and fresh.param_groups[0]["decay"] == 0.25
        assert o.param_groups[0]["learning_rate"] is s                                    # state_dict() left the live group alone


# ---- the library
def test_schedule_entry_points_are_in_header_signatures_and_library(lib):
    from tests import host_calls_schedules
    assert len(host_calls_schedules.NEW) == 13
    for name in host_calls_schedules.NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.fil_version() == _lib.header_abi_version() == 216                          # entry points added only
    header = open(_lib.HEADER_PATH).read()
    assert "#define FIL_LR_MAX_BOUNDARIES %d\n" % _lib.FIL_LR_MAX_BOUNDARIES in header
    assert ("enum { FIL_LR_CONSTANT = %d, FIL_LR_EXPONENTIAL = %d, FIL_LR_INVERSE_TIME = %d, FIL_LR_POLYNOMIAL = %d, FIL_LR_PIECEWISE = %d };"
            % (_lib.FIL_LR_CONSTANT, _lib.FIL_LR_EXPONENTIAL, _lib.FIL_LR_INVERSE_TIME, _lib.FIL_LR_POLYNOMIAL, _lib.FIL_LR_PIECEWISE)) in header
    assert "/* 432 bytes */" in header and __import__("ctypes").sizeof(_lib.LrSchedule) == 432
    # every by-value update entry point step() can reach has its device-rate twin, with one pointer in place of / beside the rate
    for name in host_calls_schedules.LR_POS:
        twin = _lib.SIGNATURES[name[:-len("_lrdev")]][1]
        mine = _lib.SIGNATURES[name][1]
        assert len(mine) - len(twin) == (1 if "rowopt" in name else 0), name
        assert mine[host_calls_schedules.LR_POS[name]] is __import__("ctypes").c_void_p, name


def test_every_descriptor_of_the_package_passes_the_library_check(lib):
    import ctypes
    for sched in CASES:
        for decay in (0.0, 0.5):
            d = sched.descriptor(decay)
            assert lib.fil_lr_schedule_check(ctypes.addressof(d)) == 0, (sched, lib.fil_last_error())
    d = schedules.constant_descriptor(0.01, 0.5)
    assert lib.fil_lr_schedule_check(ctypes.addressof(d)) == 0


def test_schedule_entry_points_validate(lib):
    from tests import host_calls_schedules
    assert host_calls_schedules.run(lib) >= 40


def test_schedule_entry_points_under_asan_ubsan():
    """host_calls_schedules.py against the AddressSanitizer + UBSan build, in a child that sees no GPU."""
    from ml_function_amd import build as _build
    asan_lib = _build.build_asan()
    rt = _build.asan_runtime()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_calls_schedules.py"), asan_lib], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "schedules host calls ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
