"""Evaluation metrics of the reference's training scripts: binary cross-entropy is torch's; AUC
(example/ctr_example/un_seq.py:61 compiles the model with tf.keras.metrics.AUC) is computed exactly here, as the
Mann-Whitney statistic with average ranks for ties -- the quantity sklearn.metrics.roc_auc_score returns (Keras' AUC is
a 200-threshold approximation of the same number).  `AUC` is that Keras metric itself: stateful, with Keras' thresholds, counts and
result formulas, updated on the GPU without a host synchronisation, so it can live inside a captured training step.  `Mean`,
`BinaryCrossentropy`, `BinaryAccuracy`, `Precision` and `Recall` are the rest of what a compiled Keras model reports per batch, kept
the same way."""
import torch

from . import _lib


def auc(y_true, y_score):
    """y_true [N] in {0,1}, y_score [N] -> ROC AUC (float).  Runs on the tensors' device."""
    y_true = y_true.reshape(-1).to(torch.float64)
    y_score = y_score.reshape(-1).to(torch.float64)
    n_pos = float(y_true.sum())
    n_neg = float(y_true.numel()) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("auc: only one class present")
    order = torch.argsort(y_score)
    s = y_score[order]
    # average 1-based ranks over runs of equal scores
    uniq, inverse, counts = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    ends = torch.cumsum(counts, 0).to(torch.float64)
    avg_rank = ends - (counts.to(torch.float64) - 1.0) / 2.0
    ranks = avg_rank[inverse]
    pos_rank_sum = float((ranks * y_true[order]).sum())
    return (pos_rank_sum - n_pos * (n_pos + 1.0) / 2.0) / (n_pos * n_neg)


_SLICE = 1 << 24        # fil_confusion_update's limit: one call's counts are exact in fp32


class AUC:
    """tf.keras.metrics.AUC of TensorFlow 2.1 (single label, no sample weights), state on the GPU.

        m = AUC()                                   # 200 thresholds, ROC, interpolation
        m.update_state(y, p)                        # inside or outside a captured step; no host synchronisation
        m.result()                                  # 0-dim device tensor, no synchronisation; float(m.result()) is the caller's sync
        m.result_value()                            # python float; THE call that checks the scores were all in [0, 1]

    State, as in Keras: four float32 vectors of num_thresholds counts (true_positives, false_positives, true_negatives,
    false_negatives; views of one [4, T] block, `confusion`), each taking ONE fp32 addition per update_state (integer-exact below
    2^24, rounding like Keras' assign_add past it).  thresholds[i] = i / (num_thresholds - 1) with the end points moved out by
    K.epsilon() = 1e-7, compared as float32 with a strict `y_pred > threshold`; any non-zero label is positive.
    The one deviation: TensorFlow fails an assertion on a y_pred outside [0, 1]; a captured step cannot raise, so such scores (and
    NaN) are left out of the counts and counted in `invalid` (one int64 on the device), and result_value() raises ValueError with the
    count -- result() and float(result()) do NOT check.  The state is created on the device of the first update_state (or build()),
    before any capture, and never re-allocated: reset_states() and load_state_dict() write in place."""

    def __init__(self, num_thresholds=200, curve="ROC", summation_method="interpolation", name=None, dtype=None, thresholds=None):
        from .functional import AUC_CURVES, AUC_SUMMATIONS
        if isinstance(curve, str) and curve.upper() in AUC_CURVES:          # Keras' AUCCurve.from_str takes 'pr' and 'PR' alike
            curve = curve.upper()
        if curve not in AUC_CURVES:
            raise ValueError('Invalid AUC curve value "%s". Valid values are: %s' % (curve, sorted(AUC_CURVES)))
        if summation_method not in AUC_SUMMATIONS:
            raise ValueError('Invalid AUC summation method value "%s". Valid values are: %s' % (summation_method, sorted(AUC_SUMMATIONS)))
        if dtype not in (None, torch.float32, "float32"):
            raise ValueError("AUC: dtype %r (the state is float32, as Keras' default)" % (dtype,))
        if thresholds is not None:
            thresholds = sorted(float(t) for t in thresholds)
            if any(not (0.0 <= t <= 1.0) for t in thresholds):
                raise ValueError("Threshold values must be in [0, 1]. Invalid values: %s" % [t for t in thresholds if not (0.0 <= t <= 1.0)])
            self.num_thresholds = len(thresholds) + 2
        else:
            if num_thresholds <= 1:
                raise ValueError("`num_thresholds` must be > 1.")
            self.num_thresholds = int(num_thresholds)
            thresholds = [(i + 1) * 1.0 / (self.num_thresholds - 1) for i in range(self.num_thresholds - 2)]
        if self.num_thresholds > _lib.FIL_CONFUSION_MAX_T:
            raise ValueError("AUC: %d thresholds (at most FIL_CONFUSION_MAX_T = %d)" % (self.num_thresholds, _lib.FIL_CONFUSION_MAX_T))
        # python floats, as in Keras (K.epsilon() end points); ONE rounding to float32 when they go to the device
        self.thresholds = [0.0 - 1e-7] + thresholds + [1.0 + 1e-7]
        self.curve, self.summation_method = curve, summation_method
        self.name = "auc" if name is None else name
        self.dtype = torch.float32
        self.confusion = self.invalid = self._thr = self._out = None

    # ---- state
    def build(self, device):
        """Create the state on `device` (update_state does it on its first call).  Do this before capturing a step."""
        if self.confusion is not None:
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FilError("ml_function_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % device.type)
        self._thr = torch.tensor(self.thresholds, dtype=torch.float64).to(torch.float32).to(device)
        self.confusion = torch.zeros((4, self.num_thresholds), dtype=torch.float32, device=device)
        self.invalid = torch.zeros((1,), dtype=torch.int64, device=device)
        self._out = torch.zeros((1,), dtype=torch.float32, device=device)
        return self

    true_positives = property(lambda self: None if self.confusion is None else self.confusion[0])
    false_positives = property(lambda self: None if self.confusion is None else self.confusion[1])
    true_negatives = property(lambda self: None if self.confusion is None else self.confusion[2])
    false_negatives = property(lambda self: None if self.confusion is None else self.confusion[3])

    def update_state(self, y_true, y_pred, sample_weight=None):
        """Add one batch (any shape, flattened; labels of any dtype, non-zero = positive).  Capturable once the state exists."""
        from . import functional as Fn
        if sample_weight is not None:
            raise NotImplementedError("AUC.update_state: sample_weight is not supported (a weighted float32 sum has no order-independent "
                                      "value, and this library's results repeat bit for bit); pass sample_weight=None")
        if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred)):
            raise TypeError("AUC.update_state takes torch tensors")
        Fn._require_cuda(y_pred, y_true)
        if y_true.numel() != y_pred.numel():
            raise ValueError("AUC.update_state: y_true has %d elements, y_pred %d" % (y_true.numel(), y_pred.numel()))
        self.build(y_pred.device)
        p = y_pred.detach().reshape(-1)
        y = y_true.detach().reshape(-1)
        p = p if p.dtype == torch.float32 else p.to(torch.float32)
        y = y if y.dtype == torch.float32 else (y != 0).to(torch.float32)          # tf.cast(y_true, bool)
        for lo in range(0, p.numel(), _SLICE):
            Fn.confusion_update(p[lo:lo + _SLICE], y[lo:lo + _SLICE], self._thr, self.confusion, self.invalid)

    def reset_states(self):
        """Zero the state in place (a captured graph keeps its pointers)."""
        if self.confusion is not None:
            self.confusion.zero_()
            self.invalid.zero_()

    def state_dict(self):
        """The counts for a checkpoint (clones; an AUC that has seen nothing has an empty state)."""
        d = dict(num_thresholds=self.num_thresholds, thresholds=list(self.thresholds), curve=self.curve, summation_method=self.summation_method)
        if self.confusion is not None:
            d.update(confusion=self.confusion.clone(), invalid=self.invalid.clone())
        return d

    def load_state_dict(self, state, device=None):
        """Copy a state_dict()'s counts into this metric's state IN PLACE (created first, on `device` or the saved tensors' device, when
        this metric has none yet).  The thresholds must be the same."""
        if list(state["thresholds"]) != list(self.thresholds):
            raise ValueError("AUC.load_state_dict: the checkpoint was taken with other thresholds")
        if "confusion" not in state:
            self.reset_states()
            return
        if self.confusion is None:
            self.build(device if device is not None else state["confusion"].device)
        self.confusion.copy_(state["confusion"])
        self.invalid.copy_(state["invalid"].reshape(1))

    # ---- reading
    def _reduced(self, process_group):
        """SUM over the group of COPIES of the counts and of the invalid counter; the local state is not touched."""
        import torch.distributed as dist
        cm, bad = self.confusion.clone(), self.invalid.clone()
        dist.all_reduce(cm, op=dist.ReduceOp.SUM, group=process_group)
        dist.all_reduce(bad, op=dist.ReduceOp.SUM, group=process_group)
        return cm, bad

    def result(self, process_group=None):
        """Keras' AUC.result() as a 0-dim float32 device tensor; no host synchronisation and NO check of `invalid` (result_value()
        checks).  Without a group the same static tensor is returned every time (an output of a captured step stays valid across
        replays).  process_group: the whole group's AUC -- the counts of every rank summed into a copy (all ranks must call; the
        local state is left as it is, so this can be read mid-epoch, repeatedly)."""
        from . import functional as Fn
        if self.confusion is None:
            if process_group is not None:
                raise _lib.FilError("AUC.result(process_group=...): this rank has no state yet (call build(device) or update_state first)")
            return torch.zeros((), dtype=torch.float32)         # Keras: 0.0 before any update
        if process_group is None:
            return Fn.auc_result(self.confusion, self.curve, self.summation_method, out=self._out)
        return Fn.auc_result(self._reduced(process_group)[0], self.curve, self.summation_method)

    def result_value(self, process_group=None):
        """float(result()) after checking, on the host, that no score was outside [0, 1] (or NaN): raises ValueError with the count
        otherwise -- where TensorFlow's assertion would have failed in update_state.  Synchronises."""
        from . import functional as Fn
        if self.confusion is None:
            return float(self.result(process_group))
        cm, bad = (self.confusion, self.invalid) if process_group is None else self._reduced(process_group)
        out = Fn.auc_result(cm, self.curve, self.summation_method)
        bad = int(bad.item())
        if bad:
            raise ValueError("AUC: %d predictions were outside [0, 1] (or NaN); they were left out of the counts" % bad)
        return float(out)


# ------------------------------------------------------------------------------------------------ Keras' Mean metrics (include/fil.h M2)
_NO_WEIGHTS = ("sample_weight is not supported (a weighted float32 sum has no order-independent value, and this library's results "
               "repeat bit for bit); pass sample_weight=None")


def _div_no_nan(a, b):
    """tf.math.div_no_nan on tensors."""
    return torch.where(b == 0, torch.zeros_like(a), a / b)


class _MeanState:
    """The state of tf.keras.metrics.Mean of TensorFlow 2.1 (Reduce with Reduction.WEIGHTED_MEAN, no sample weights) on the GPU:
    `total` and `count`, two float32 scalars that take ONE fp32 addition each per update (Keras' assign_add; the count is
    integer-exact below 2^24 and rounds past it), and result = div_no_nan(total, count), which the update's own launch writes.  The
    three are views of one [3] block, `state`, created on the device of the first update_state (or build()), before any capture,
    and never re-allocated: reset_states() and load_state_dict() write in place.  NaN and infinity are not filtered, as in Keras: a
    NaN value makes total and result NaN until reset_states()."""
    _kind = "values"

    def _init(self, name, dtype):
        if dtype not in (None, torch.float32, "float32"):
            raise ValueError("%s: dtype %r (the state is float32, as Keras' default)" % (type(self).__name__, dtype))
        self.name = name
        self.dtype = torch.float32
        self.state = self._total = self._count = self._result = None

    def _constants(self):
        return 0.0, 0.0

    # ---- state
    def build(self, device):
        """Create the state on `device` (update_state does it on its first call).  Do this before capturing a step."""
        if self.state is not None:
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FilError("ml_function_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % device.type)
        self.state = torch.zeros((3,), dtype=torch.float32, device=device)
        self._total, self._count, self._result = self.state[0], self.state[1], self.state[2]
        return self

    total = property(lambda self: self._total)
    count = property(lambda self: self._count)

    def _update(self, a, y):
        from . import functional as Fn
        self.build(a.device)
        c0, c1 = self._constants()
        for lo in range(0, a.numel(), _SLICE):
            Fn.mean_update(self._kind, a[lo:lo + _SLICE], None if y is None else y[lo:lo + _SLICE], self.state, c0, c1)

    def _update_pair(self, y_true, y_pred, sample_weight):
        """update_state(y_true, y_pred) of the metrics that wrap a per-sample function: any shape, flattened, every element a sample."""
        from . import functional as Fn
        who = type(self).__name__
        if sample_weight is not None:
            raise NotImplementedError("%s.update_state: %s" % (who, _NO_WEIGHTS))
        if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred)):
            raise TypeError("%s.update_state takes torch tensors" % who)
        Fn._require_cuda(y_pred, y_true)
        if y_true.numel() != y_pred.numel():
            raise ValueError("%s.update_state: y_true has %d elements, y_pred %d" % (who, y_true.numel(), y_pred.numel()))
        p = y_pred.detach().reshape(-1)
        y = y_true.detach().reshape(-1)
        p = p if p.dtype == torch.float32 else p.to(torch.float32)
        y = y if y.dtype == torch.float32 else y.to(torch.float32)                 # tf.cast(y_true, y_pred.dtype)
        self._update(p, y)

    def reset_states(self):
        """Zero the state in place (a captured graph keeps its pointers)."""
        if self.state is not None:
            self.state.zero_()

    def state_dict(self):
        """total | count | result for a checkpoint (a clone; a metric that has seen nothing has an empty state)."""
        return {} if self.state is None else dict(state=self.state.clone())

    def load_state_dict(self, state, device=None):
        """Copy a state_dict()'s values into this metric's state IN PLACE (created first, on `device` or the saved tensor's device,
        when this metric has none yet)."""
        if "state" not in state:
            self.reset_states()
            return
        if self.state is None:
            self.build(device if device is not None else state["state"].device)
        self.state.copy_(state["state"])

    # ---- reading
    def _reduced(self, process_group):
        """SUM over the group of a COPY of total and count; the local state is not touched."""
        import torch.distributed as dist
        st = self.state[:2].clone()
        dist.all_reduce(st, op=dist.ReduceOp.SUM, group=process_group)
        return st

    def result(self, process_group=None):
        """Keras' result(), div_no_nan(total, count), as a 0-dim float32 device tensor; no host synchronisation.  Without a group this
        is the state's own third word -- written by the update's launch, so reading costs no launch, and the same static tensor every
        time (it stays valid and current across replays of a captured step).  process_group: the whole group's mean -- total and count
        of every rank summed into a copy (all ranks must call; the local state is left as it is)."""
        if self.state is None:
            if process_group is not None:
                raise _lib.FilError("%s.result(process_group=...): this rank has no state yet (call build(device) or update_state first)"
                                    % type(self).__name__)
            return torch.zeros((), dtype=torch.float32)         # Keras: 0.0 before any update
        if process_group is None:
            return self._result
        st = self._reduced(process_group)
        return _div_no_nan(st[0], st[1])


class Mean(_MeanState):
    """tf.keras.metrics.Mean: the running mean of everything update_state was given.

        loss_avg = Mean(name="loss").build(device)   # Keras' progress-bar loss: the mean of the batch losses so far
        loss_avg.update_state(loss)                  # inside or outside a captured step; one launch, no host synchronisation
        loss_avg.result()                            # 0-dim device tensor, no launch"""

    def __init__(self, name="mean", dtype=None):
        self._init(name, dtype)

    def update_state(self, values, sample_weight=None):
        """Add values (any shape, flattened: total += sum, count += numel).  Capturable once the state exists."""
        from . import functional as Fn
        if sample_weight is not None:
            raise NotImplementedError("Mean.update_state: %s" % _NO_WEIGHTS)
        if not torch.is_tensor(values):
            raise TypeError("Mean.update_state takes a torch tensor")
        Fn._require_cuda(values)
        v = values.detach().reshape(-1)
        self._update(v if v.dtype == torch.float32 else v.to(torch.float32), None)


class BinaryCrossentropy(_MeanState):
    """tf.keras.metrics.BinaryCrossentropy on probabilities: the running mean of Keras' per-sample binary_crossentropy (epsilon 1e-7;
    label_smoothing moves the labels to y (1 - s) + 0.5 s) -- the LogLoss the CTR papers report.  Labels that are not float32 are cast
    to it, as Keras casts y_true to y_pred's dtype."""
    _kind = "binary_crossentropy"

    def __init__(self, name="binary_crossentropy", dtype=None, from_logits=False, label_smoothing=0):
        if from_logits:
            raise NotImplementedError("BinaryCrossentropy: from_logits=True is not supported (this library's models end in a sigmoid or "
                                      "a softmax: pass probabilities)")
        self._init(name, dtype)
        self.from_logits = False
        self.label_smoothing = float(label_smoothing)

    def _constants(self):
        return 1e-7, self.label_smoothing

    def update_state(self, y_true, y_pred, sample_weight=None):
        self._update_pair(y_true, y_pred, sample_weight)


class BinaryAccuracy(_MeanState):
    """tf.keras.metrics.BinaryAccuracy: the running mean of (y_true == (y_pred > threshold)), a strict >; a label that is neither 0 nor
    1 never matches.  Matches are counted in integers.  Labels that are not float32 are cast to it, as Keras casts y_true to y_pred's
    dtype."""
    _kind = "binary_accuracy"

    def __init__(self, name="binary_accuracy", dtype=None, threshold=0.5):
        self._init(name, dtype)
        self.threshold = float(threshold)

    def _constants(self):
        return self.threshold, 0.0

    def update_state(self, y_true, y_pred, sample_weight=None):
        self._update_pair(y_true, y_pred, sample_weight)


class _AtThresholds:
    """What tf.keras.metrics.Precision and Recall share (TF 2.1, single label, no sample weights): update_confusion_matrix_variables
    at the user's thresholds -- fil_confusion_update, the AUC's kernel -- and a div_no_nan of two of its vectors.  thresholds: None
    (0.5), a float or a list, each in [0, 1], compared as float32 with a strict `y_pred > threshold` and used as given (no
    epsilon-moved end points).  The kernel wants its thresholds ascending and at least two: they are kept sorted on the device (a
    single one twice) and every reading is put back into the caller's order.  As for AUC, scores outside [0, 1] (and NaN) are left
    out and counted in `invalid`, and result_value() raises for them."""
    _den = None     # row of `confusion` added to the true positives: 1 (false positives) or 3 (false negatives)

    def __init__(self, thresholds=None, top_k=None, class_id=None, name=None, dtype=None):
        who = type(self).__name__
        if top_k is not None or class_id is not None:
            raise NotImplementedError("%s: top_k / class_id are not supported (single-label scores only)" % who)
        if dtype not in (None, torch.float32, "float32"):
            raise ValueError("%s: dtype %r (the state is float32, as Keras' default)" % (who, dtype))
        self.init_thresholds = thresholds
        if thresholds is None:
            thresholds = [0.5]
        elif isinstance(thresholds, (list, tuple)):
            thresholds = [None if t is None else float(t) for t in thresholds]
        else:
            thresholds = [float(thresholds)]
        bad = [t for t in thresholds if t is None or not (0.0 <= t <= 1.0)]
        if bad:
            raise ValueError("Threshold values must be in [0, 1]. Invalid values: %s" % bad)
        if not thresholds:
            raise ValueError("%s: an empty list of thresholds" % who)
        self.thresholds = thresholds
        order = sorted(range(len(thresholds)), key=thresholds.__getitem__)
        self._sorted = [thresholds[i] for i in order] * (2 if len(thresholds) == 1 else 1)
        if len(self._sorted) > _lib.FIL_CONFUSION_MAX_T:
            raise ValueError("%s: %d thresholds (at most FIL_CONFUSION_MAX_T = %d)" % (who, len(thresholds), _lib.FIL_CONFUSION_MAX_T))
        pos = [0] * len(thresholds)
        for k, i in enumerate(order):
            pos[i] = k
        self._pos = pos                                      # thresholds[i] is column pos[i] of `confusion`
        self._in_order = pos == list(range(len(pos)))
        self.top_k, self.class_id = None, None
        self.name = who.lower() if name is None else name
        self.dtype = torch.float32
        self.confusion = self.invalid = self._thr = self._idx = self._out = self._res = None

    # ---- state
    def build(self, device):
        """Create the state on `device` (update_state does it on its first call).  Do this before capturing a step."""
        if self.confusion is not None:
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FilError("ml_function_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % device.type)
        self._thr = torch.tensor(self._sorted, dtype=torch.float64).to(torch.float32).to(device)
        self._idx = torch.tensor(self._pos, dtype=torch.int64, device=device)
        self.confusion = torch.zeros((4, len(self._sorted)), dtype=torch.float32, device=device)
        self.invalid = torch.zeros((1,), dtype=torch.int64, device=device)
        self._out = torch.zeros((len(self.thresholds),), dtype=torch.float32, device=device)
        self._res = self._out[0] if len(self.thresholds) == 1 else self._out
        return self

    def _row(self, cm, r):
        """Row r of a [4, T] block in the caller's threshold order (a view where that is the stored order)."""
        if self._in_order:
            return cm[r, :len(self.thresholds)]
        return cm[r].index_select(0, self._idx)

    true_positives = property(lambda self: None if self.confusion is None else self._row(self.confusion, 0))
    false_positives = property(lambda self: None if self.confusion is None else self._row(self.confusion, 1))
    true_negatives = property(lambda self: None if self.confusion is None else self._row(self.confusion, 2))
    false_negatives = property(lambda self: None if self.confusion is None else self._row(self.confusion, 3))

    def update_state(self, y_true, y_pred, sample_weight=None):
        """Add one batch (any shape, flattened; labels of any dtype, non-zero = positive).  Capturable once the state exists."""
        from . import functional as Fn
        who = type(self).__name__
        if sample_weight is not None:
            raise NotImplementedError("%s.update_state: %s" % (who, _NO_WEIGHTS))
        if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred)):
            raise TypeError("%s.update_state takes torch tensors" % who)
        Fn._require_cuda(y_pred, y_true)
        if y_true.numel() != y_pred.numel():
            raise ValueError("%s.update_state: y_true has %d elements, y_pred %d" % (who, y_true.numel(), y_pred.numel()))
        self.build(y_pred.device)
        p = y_pred.detach().reshape(-1)
        y = y_true.detach().reshape(-1)
        p = p if p.dtype == torch.float32 else p.to(torch.float32)
        y = y if y.dtype == torch.float32 else (y != 0).to(torch.float32)          # tf.cast(y_true, bool)
        for lo in range(0, p.numel(), _SLICE):
            Fn.confusion_update(p[lo:lo + _SLICE], y[lo:lo + _SLICE], self._thr, self.confusion, self.invalid)

    def reset_states(self):
        """Zero the state in place (a captured graph keeps its pointers)."""
        if self.confusion is not None:
            self.confusion.zero_()
            self.invalid.zero_()

    def state_dict(self):
        """The counts for a checkpoint (clones, columns in ascending threshold order; empty before the first update)."""
        d = dict(thresholds=list(self.thresholds))
        if self.confusion is not None:
            d.update(confusion=self.confusion.clone(), invalid=self.invalid.clone())
        return d

    def load_state_dict(self, state, device=None):
        """Copy a state_dict()'s counts into this metric's state IN PLACE (created first, on `device` or the saved tensors' device, when
        this metric has none yet).  The thresholds must be the same."""
        if list(state["thresholds"]) != list(self.thresholds):
            raise ValueError("%s.load_state_dict: the checkpoint was taken with other thresholds" % type(self).__name__)
        if "confusion" not in state:
            self.reset_states()
            return
        if self.confusion is None:
            self.build(device if device is not None else state["confusion"].device)
        self.confusion.copy_(state["confusion"])
        self.invalid.copy_(state["invalid"].reshape(1))

    # ---- reading
    def _reduced(self, process_group):
        """SUM over the group of COPIES of the counts and of the invalid counter; the local state is not touched."""
        import torch.distributed as dist
        cm, bad = self.confusion.clone(), self.invalid.clone()
        dist.all_reduce(cm, op=dist.ReduceOp.SUM, group=process_group)
        dist.all_reduce(bad, op=dist.ReduceOp.SUM, group=process_group)
        return cm, bad

    def _quotient(self, cm):
        tp = self._row(cm, 0)
        return _div_no_nan(tp, tp + self._row(cm, self._den))

    def result(self, process_group=None):
        """Keras' result(): div_no_nan(tp, tp + fp) for Precision, div_no_nan(tp, tp + fn) for Recall, in float32 on the device -- a
        0-dim tensor for one threshold, a vector in the caller's threshold order otherwise; no host synchronisation and NO check of
        `invalid` (result_value() checks).  Without a group the same static tensor is rewritten and returned every time.
        process_group: the whole group's value, from the counts of every rank summed into a copy (all ranks must call)."""
        n = len(self.thresholds)
        if self.confusion is None:
            if process_group is not None:
                raise _lib.FilError("%s.result(process_group=...): this rank has no state yet (call build(device) or update_state first)"
                                    % type(self).__name__)
            return torch.zeros(() if n == 1 else (n,), dtype=torch.float32)
        if process_group is None:
            self._out.copy_(self._quotient(self.confusion))
            return self._res
        q = self._quotient(self._reduced(process_group)[0])
        return q[0] if n == 1 else q

    def result_value(self, process_group=None):
        """result() on the host (a float for one threshold, a list otherwise) after checking that no score was outside [0, 1] (or NaN):
        raises ValueError with the count otherwise -- where TensorFlow's assertion would have failed in update_state.  Synchronises."""
        n = len(self.thresholds)
        if self.confusion is None:
            return 0.0 if n == 1 else [0.0] * n
        cm, bad = (self.confusion, self.invalid) if process_group is None else self._reduced(process_group)
        q = self._quotient(cm)
        bad = int(bad.item())
        if bad:
            raise ValueError("%s: %d predictions were outside [0, 1] (or NaN); they were left out of the counts" % (type(self).__name__, bad))
        return float(q[0]) if n == 1 else [float(v) for v in q.tolist()]


class Precision(_AtThresholds):
    """tf.keras.metrics.Precision: true positives / predicted positives at each threshold (default 0.5)."""
    _den = 1


class Recall(_AtThresholds):
    """tf.keras.metrics.Recall: true positives / actual positives at each threshold (default 0.5)."""
    _den = 3
