"""Keras' learning-rate schedules (tf.keras.optimizers.schedules, TF 2.1) as plain picklable Python objects, with Keras' constructor
names and defaults, get_config() / from_config() and the module-level serialize() / deserialize().

    opt = optim.Adam(model.parameters(), learning_rate=schedules.ExponentialDecay(1e-3, decay_steps=10000, decay_rate=0.96))

A schedule holds no tensors.  optim.Adam / Adagrad / Ftrl turn it into a fil_lr_schedule descriptor (include/fil.h O3) on the device,
and fil_lr_schedule_eval computes the rate of every step there, from the device step counter: a step captured into a HIP graph
changes its rate on every replay.  `step` is Keras' `iterations`: the number of completed steps, 0 at the first step.  Keras casts the
step and every constant to float32 and computes in float32; schedule(step) below returns that float32 value as a Python float,
computed on the host by the same formulas (the two powers in float64, rounded once -- as the device takes them).
"""
import numpy as np

from ._lib import (FIL_LR_CONSTANT, FIL_LR_EXPONENTIAL, FIL_LR_INVERSE_TIME, FIL_LR_MAX_BOUNDARIES, FIL_LR_PIECEWISE,
                   FIL_LR_POLYNOMIAL, LrSchedule)

_f32 = np.float32


def _pow_once(base, p):
    return _f32(np.float64(base) ** np.float64(p))


class LearningRateSchedule:
    """Base class: a subclass supplies get_config() and _fill(descriptor)."""

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def _fill(self, d):
        raise NotImplementedError

    def descriptor(self, decay=0.0):
        """The schedule as an _lib.LrSchedule (fil_lr_schedule) in host memory, with the legacy `decay` folded in."""
        d = LrSchedule()
        self._fill(d)
        d.decay = float(decay)
        return d

    def __call__(self, step):
        return float(evaluate(self.descriptor(), step))

    def __eq__(self, other):
        return type(other) is type(self) and other.get_config() == self.get_config()

    def __hash__(self):
        return hash((type(self).__name__, repr(sorted(self.get_config().items()))))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % kv for kv in self.get_config().items()))


def _check_decay_steps(name, decay_steps):
    if not decay_steps > 0:
        raise ValueError("%s: decay_steps must be positive, got %r" % (name, decay_steps))


class ExponentialDecay(LearningRateSchedule):
    """lr = initial_learning_rate * decay_rate ** (step / decay_steps); staircase: the exponent floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        _check_decay_steps("ExponentialDecay", decay_steps)
        self.initial_learning_rate = initial_learning_rate
        self.decay_steps = decay_steps
        self.decay_rate = decay_rate
        self.staircase = bool(staircase)
        self.name = name

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}

    def _fill(self, d):
        d.kind, d.flag = FIL_LR_EXPONENTIAL, int(self.staircase)
        d.initial_lr, d.decay_steps, d.decay_rate = self.initial_learning_rate, self.decay_steps, self.decay_rate


class InverseTimeDecay(LearningRateSchedule):
    """lr = initial_learning_rate / (1 + decay_rate * step / decay_steps); staircase: step / decay_steps floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        _check_decay_steps("InverseTimeDecay", decay_steps)
        self.initial_learning_rate = initial_learning_rate
        self.decay_steps = decay_steps
        self.decay_rate = decay_rate
        self.staircase = bool(staircase)
        self.name = name

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}

    def _fill(self, d):
        d.kind, d.flag = FIL_LR_INVERSE_TIME, int(self.staircase)
        d.initial_lr, d.decay_steps, d.decay_rate = self.initial_learning_rate, self.decay_steps, self.decay_rate


class PolynomialDecay(LearningRateSchedule):
    """lr = (initial_learning_rate - end_learning_rate) * (1 - step / decay_steps) ** power + end_learning_rate, the step clipped to
    decay_steps; cycle: decay_steps is instead stretched to the next multiple of itself at or beyond the step."""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False, name=None):
        _check_decay_steps("PolynomialDecay", decay_steps)
        self.initial_learning_rate = initial_learning_rate
        self.decay_steps = decay_steps
        self.end_learning_rate = end_learning_rate
        self.power = power
        self.cycle = bool(cycle)
        self.name = name

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "end_learning_rate": self.end_learning_rate, "power": self.power, "cycle": self.cycle, "name": self.name}

    def _fill(self, d):
        d.kind, d.flag = FIL_LR_POLYNOMIAL, int(self.cycle)
        d.initial_lr, d.decay_steps, d.end_lr, d.power = self.initial_learning_rate, self.decay_steps, self.end_learning_rate, self.power


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] for step <= boundaries[0], values[i] for boundaries[i-1] < step <= boundaries[i], values[-1] beyond the last
    boundary; integer comparisons.  At most 32 boundaries (the descriptor's size), in non-decreasing order."""

    def __init__(self, boundaries, values, name=None):
        boundaries, values = list(boundaries), list(values)
        if len(boundaries) != len(values) - 1:
            raise ValueError("The length of boundaries should be 1 less than the length of values")
        if not 1 <= len(boundaries) <= FIL_LR_MAX_BOUNDARIES:
            raise ValueError("PiecewiseConstantDecay: %d boundaries (1 ... %d: the device descriptor holds at most %d boundaries)"
                             % (len(boundaries), FIL_LR_MAX_BOUNDARIES, FIL_LR_MAX_BOUNDARIES))
        if any(int(b) != b for b in boundaries):
            raise ValueError("PiecewiseConstantDecay: boundaries are step counts (integers), got %r" % (boundaries,))
        if any(b < a for a, b in zip(boundaries, boundaries[1:])):
            raise ValueError("PiecewiseConstantDecay: boundaries must be sorted, got %r" % (boundaries,))
        self.boundaries = [int(b) for b in boundaries]
        self.values = values
        self.name = name

    def get_config(self):
        return {"boundaries": self.boundaries, "values": self.values, "name": self.name}

    def _fill(self, d):
        d.kind, d.n_boundaries = FIL_LR_PIECEWISE, len(self.boundaries)
        for i, b in enumerate(self.boundaries):
            d.boundaries[i] = b
        for i, v in enumerate(self.values):
            d.values[i] = v


def constant_descriptor(learning_rate, decay):
    """A float rate with the legacy `decay` as a descriptor (FIL_LR_CONSTANT)."""
    d = LrSchedule()
    d.kind, d.initial_lr, d.decay = FIL_LR_CONSTANT, float(learning_rate), float(decay)
    return d


def evaluate(d, step):
    """What fil_lr_schedule_eval computes for descriptor d (an _lib.LrSchedule) at `step` completed steps, on the host: the same
    float32 operations in the same order, as a numpy float32 (Keras' OptimizerV2._decayed_lr)."""
    it = int(step)
    s = _f32(it)
    lr = _f32(d.initial_lr)
    ds = _f32(d.decay_steps)
    with np.errstate(all="ignore"):
        if d.kind == FIL_LR_EXPONENTIAL:
            p = s / ds
            if d.flag:
                p = np.floor(p)
            lr = lr * _pow_once(_f32(d.decay_rate), p)
        elif d.kind == FIL_LR_INVERSE_TIME:
            p = s / ds
            if d.flag:
                p = np.floor(p)
            lr = lr / (_f32(1) + _f32(d.decay_rate) * p)
        elif d.kind == FIL_LR_POLYNOMIAL:
            if d.flag:
                ds = ds * (_f32(1) if s == 0 else np.ceil(s / ds))
            else:
                s = min(s, ds)
            p = s / ds
            base = _f32(1) - p
            pw = base if d.power == 1.0 else _pow_once(base, _f32(d.power))
            lr = (lr - _f32(d.end_lr)) * pw + _f32(d.end_lr)
        elif d.kind == FIL_LR_PIECEWISE:
            i = 0
            while i < d.n_boundaries and it > d.boundaries[i]:
                i += 1
            lr = _f32(d.values[i])
        if d.decay > 0:
            lr = lr / (_f32(1) + _f32(d.decay) * _f32(it))
    return _f32(lr)


_CLASSES = {c.__name__: c for c in (ExponentialDecay, InverseTimeDecay, PolynomialDecay, PiecewiseConstantDecay)}


def serialize(learning_rate_schedule):
    """{"class_name": ..., "config": ...} of a schedule (Keras' schedules.serialize)."""
    if not isinstance(learning_rate_schedule, LearningRateSchedule):
        raise TypeError("serialize: not a LearningRateSchedule: %r" % (learning_rate_schedule,))
    return {"class_name": type(learning_rate_schedule).__name__, "config": learning_rate_schedule.get_config()}


def deserialize(config, custom_objects=None):
    """The schedule of a serialize() dict (Keras' schedules.deserialize)."""
    classes = dict(_CLASSES, **(custom_objects or {}))
    try:
        cls = classes[config["class_name"]]
    except (KeyError, TypeError):
        raise ValueError("deserialize: unknown learning-rate schedule %r (known: %s)" % (config, ", ".join(sorted(classes))))
    return cls.from_config(config["config"])
