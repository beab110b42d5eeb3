"""Keras' learning-rate schedules (TF 2.1: keras/optimizer_v2/learning_rate_schedule.py) and OptimizerV2._decayed_lr, restated in
numpy float32: the reference the schedule tests are held to.  Written from the formulas of the TF 2.1 sources (TensorFlow is not a
dependency of this repository); parity with a TensorFlow run is unpinned, as for every other Keras restatement here.

`step` is Keras' `iterations` (completed steps, 0 at the first step).  Keras casts the step and every constant to float32 and every
op rounds to float32; `exact_pow=True` takes the two powers in float64 and rounds them once to float32 (what the device computes;
tf.pow in float32 is whatever its libm returns), `exact_pow=False` takes numpy's float32 power.

    exponential(step, initial, decay_steps, decay_rate, staircase)
    inverse_time(step, initial, decay_steps, decay_rate, staircase)
    polynomial(step, initial, decay_steps, end, power, cycle)
    piecewise(step, boundaries, values)                      integer comparisons
    decayed(lr, step, decay)                                 the legacy `decay`, applied after the schedule
    rate(schedule_or_float, step, decay)                     _decayed_lr for a schedules.* object or a float
"""
import numpy as np

f32 = np.float32


def _pow(base, p, exact_pow):
    if exact_pow:
        return f32(np.float64(base) ** np.float64(p))
    return np.power(f32(base), f32(p), dtype=np.float32)


def _ratio(step, decay_steps, staircase):
    p = f32(int(step)) / f32(decay_steps)
    return np.floor(p) if staircase else p


def exponential(step, initial, decay_steps, decay_rate, staircase=False, exact_pow=True):
    with np.errstate(all="ignore"):
        return f32(f32(initial) * _pow(f32(decay_rate), _ratio(step, decay_steps, staircase), exact_pow))


def inverse_time(step, initial, decay_steps, decay_rate, staircase=False):
    with np.errstate(all="ignore"):
        denom = f32(1) + f32(decay_rate) * _ratio(step, decay_steps, staircase)
        return f32(f32(initial) / denom)


def polynomial(step, initial, decay_steps, end=0.0001, power=1.0, cycle=False, exact_pow=True):
    with np.errstate(all="ignore"):
        s, d = f32(int(step)), f32(decay_steps)
        if cycle:
            d = d * (f32(1) if s == 0 else np.ceil(s / f32(decay_steps)))
        else:
            s = np.minimum(s, d)
        p = s / d
        base = f32(1) - p
        # x ** 1.0 == x for every float x (NaN included), so the power-1 case involves no pow at all
        pw = base if f32(power) == 1 else _pow(base, f32(power), exact_pow)
        return f32((f32(initial) - f32(end)) * pw + f32(end))


def piecewise(step, boundaries, values):
    step = int(step)
    assert len(values) == len(boundaries) + 1
    if step <= boundaries[0]:
        return f32(values[0])
    for i in range(1, len(boundaries)):
        if boundaries[i - 1] < step <= boundaries[i]:
            return f32(values[i])
    return f32(values[-1])


def decayed(lr, step, decay):
    if not decay > 0:
        return f32(lr)
    with np.errstate(all="ignore"):
        return f32(f32(lr) / (f32(1) + f32(decay) * f32(int(step))))


def rate(schedule, step, decay=0.0, exact_pow=True):
    """OptimizerV2._decayed_lr: the schedule (an ml_function_amd.schedules object, dispatched on its class name and config, or a
    float) at `step`, then the legacy decay."""
    if isinstance(schedule, (int, float, np.floating)):
        lr = f32(schedule)
    else:
        c = schedule.get_config()
        kind = type(schedule).__name__
        if kind == "ExponentialDecay":
            lr = exponential(step, c["initial_learning_rate"], c["decay_steps"], c["decay_rate"], c["staircase"], exact_pow)
        elif kind == "InverseTimeDecay":
            lr = inverse_time(step, c["initial_learning_rate"], c["decay_steps"], c["decay_rate"], c["staircase"])
        elif kind == "PolynomialDecay":
            lr = polynomial(step, c["initial_learning_rate"], c["decay_steps"], c["end_learning_rate"], c["power"], c["cycle"], exact_pow)
        elif kind == "PiecewiseConstantDecay":
            lr = piecewise(step, c["boundaries"], c["values"])
        else:
            raise ValueError(kind)
    return decayed(lr, step, decay)


def ulps(a, b):
    """Distance of two float32 in units in the last place (0 for equal bits or two NaNs; a large number across NaN / non-NaN)."""
    a, b = f32(a), f32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if (np.isnan(a) and np.isnan(b)) else 1 << 31
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    ia = ia if ia >= 0 else -(ia & 0x7FFFFFFF)
    ib = ib if ib >= 0 else -(ib & 0x7FFFFFFF)
    return abs(ia - ib)
