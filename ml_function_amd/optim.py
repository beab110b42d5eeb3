"""Keras' Adam, Adagrad, Ftrl, SGD, RMSprop, Adadelta, Adamax and Nadam on the HIP path (include/fil.h O1, O2, O4, O5, O6, O7): the optimizer the reference compiles (optimizer='adam', example/ctr_example/
un_seq.py:61; TF 2.1), with Keras' names, defaults and numerics.

    opt = optim.Adam(model.parameters())                    # learning_rate 1e-3, beta_1 0.9, beta_2 0.999, epsilon 1e-7
    loss.backward(); opt.step(); opt.zero_grad()

Keras adds epsilon to the UNCORRECTED sqrt(v) and folds the bias correction into the step size (alpha = lr sqrt(1 - b2^t) /
(1 - b1^t); p -= alpha m / (sqrt(v) + eps)); torch.optim.Adam adds it to the corrected sqrt(v / (1 - b2^t)), which at t = 1 is an
epsilon 1/sqrt(1 - beta_2) ~ 31.6 times larger -- of the order of an embedding row's gradient.

* Dense parameters with a gradient: ONE fil_adam_multi launch per (parameter group, device) over all of them.  A parameter whose
  .grad is None is skipped (Keras filters None gradients); the step counter advances anyway.
* Embedding tables of SparseEmbed(grad_mode="runs") / FeatureInput(tableGrad="runs"): the backward leaves the batch's sorted
  gradient runs on the table and step() applies them IN PLACE -- fil_embed_adam_runs, plus fil_embed_adam_sweep over every row the
  batch did not touch (Keras' dense Adam: their m and v decay and they move; l2(emb_reg) of table_l2_ranges() is added inside the
  update).  No [V,K] gradient is ever built.  lazy_tables=True is the LABELLED deviation from the reference (TF-Addons LazyAdam):
  only the touched rows change, no sweep.  A table in "dense" mode is an ordinary dense parameter here.
* Data parallelism (process_group, or the default group once torch.distributed is initialised, with more than one rank; or
  force_exchange=True at any world size): every runs table's record is compacted (fil_embed_runs_compact: distinct row ids + their
  summed rows), the ranks all-gather the fixed-size lists (dp.exchange_runs) and every rank applies the same merged update
  (fil_embed_adam_merged: the union's rows, summed in rank order, so the replicas stay bit-identical), then the sweep.  The list
  capacity `cap` is agreed once per table on the first step (an all-reduce MAX of R, one host read); later steps neither synchronise
  nor allocate, and a record with R > cap raises.  Without a group of > 1 ranks (and without force_exchange) step() takes the
  one-GPU path above, unchanged.
* Deferred mode (sweep_period=N, opt-in): the untouched rows are not swept at every step.  Their update (g = 2 l2 p)
  depends only on the row's own p, m, v, its field's l2 and the step's coefficients, so the steps a row misses are replayed later
  with the same fp32 operations in the same order -- the same bits.  Per deferred table: int32 [V] row stamps (row r is current
  through completed step stamp[r]) and a device ring of D >= N + 1 per-step coefficients.  A forward that gathers from the table first
  catches up the batch's rows (fil_embed_adam_catchup_runs); step() catches up and updates the batch's rows
  (fil_embed_adam_runs_deferred / fil_embed_adam_merged_deferred), writes the step's ring entry and catches up one slice of ceil(V/N)
  rows (fil_embed_adam_roll), so no row is ever more than N steps behind.  Everything that leaves the library is bit-identical to
  Keras mode: gathered rows, losses, and the table, m and v after flush() -- which state_dict(), SparseEmbed's state-dict hook and
  SparseEmbed.regularization_losses() call, and the optimizer's finaliser (a table never outlives its optimizer lagging).  Only
  the table in memory between steps lags, for rows nobody has read.  Runs tables attach at construction, through
  add_param_group, or at their first record.
* The step counter t (Keras' `iterations`) is an int64 on the device, read by every launch and advanced by the last one: a step
  captured into a HIP graph (capture.capture_step) advances it on every replay.  Betas and a float learning rate are baked into a
  capture.
* learning_rate may be a schedules.LearningRateSchedule (Keras' ExponentialDecay, InverseTimeDecay, PolynomialDecay,
  PiecewiseConstantDecay), and decay= is Keras' legacy keyword (lr / (1 + decay * iterations), applied after the schedule;
  OptimizerV2._decayed_lr): with either, step() first enqueues one fil_lr_schedule_eval per (group, device) -- the rate of step t
  computed on the device from the counter, one fp32 word -- and every update launch of the step reads that word (the *_lrdev entry
  points, include/fil.h O3), so a captured step changes its rate on every replay, and the deferred ring holds each step's own rate.
  The rate uses iterations (0 at the first step), Adam's bias correction iterations + 1.  current_learning_rate() reads it without a
  synchronisation; state_dict() carries the schedule's config.  With a float rate and no decay, step() makes exactly the calls it
  always made.  Adagrad and Ftrl take both too.

Adagrad and Ftrl (Keras' tf.keras.optimizers.Adagrad / Ftrl, TF 2.1; O2) follow the same contract -- iterations, one dense launch per
(group, device), runs tables consumed in place, the same data-parallel route, capture after one eager step -- with row-local rules:
an untouched row has no state that decays, so only the regularised fields (l2(emb_reg) > 0) are swept, over their rows alone, and
an untouched row of any other field keeps its bits (Keras' IndexedSlices semantics).  No deferred or lazy mode.

SGD and RMSprop (tf.keras.optimizers.SGD / RMSprop, TF 2.1; O4) take that contract too.  SGD (plain, momentum, Nesterov) and RMSprop
with momentum > 0 are row-local like Adagrad.  RMSprop with momentum == 0 -- what model.compile(optimizer='rmsprop') builds -- is not:
Keras decays the `rms` slot of EVERY row of an embedding (rms = rms * rho over the whole variable) and moves the batch's rows only, so
its sweep walks every non-frozen field of every runs table (rms alone on the unregularised ones) and every such table has row stamps.
SGD with momentum == 0 has no slot at all: its state holds no tensors and its launches carry NULL slots.  RMSprop(centered=True)
raises NotImplementedError (a third slot, which the descriptors and the runs entry points do not carry).

Adadelta and Adamax (tf.keras.optimizers.Adadelta / Adamax, TF 2.1; O5) take that contract as well, both row-local with two slots
(accum_grad / accum_var; m / v).  Adadelta reads no step and is bit-exact.  Adamax' step size c = lr / (1 - beta_1^t), t = iterations
+ 1, is formed on the device at the top of every launch from the step counter and the step's rate (a float, a schedule's word, or
decay=), so a captured step takes each replay's own coefficient; beta_1^t is the device's powf, as in Adam, so it is Keras-exact
within Adam's bars rather than bit-exact.

Nadam (tf.keras.optimizers.Nadam, TF 2.1; O6) takes the contract too, although it is not row-local: its sparse apply decays m and v
over the whole variable, so -- like RMSprop with momentum == 0 -- its sweep walks every non-frozen field of every runs table (m and v
alone on the unregularised ones) and every such table has row stamps.  Its running momentum-cache product is one fp32 word per
device beside the step counter (`momentum_cache`), read by every launch and multiplied by the step's momentum in the launch that
advances the counter, so a captured step moves both on every replay.  The step's coefficients are formed on the device from the two
words; its powers are the device's powf, so it is Keras-exact within Adam's bars, bit-exact in m and v.  Keras' Nadam takes neither a
schedule nor decay=, and neither does this one.

Adam(amsgrad=True) (Keras' Adam with amsgrad, TF 2.1 ApplyAdamWithAmsgrad; O7) keeps a third slot `vhat` (Keras' name, zeros): vhat =
(vhat < v) ? v : vhat after m and v, and p -= alpha m / (sqrt(vhat) + epsilon).  Same contract as Adam's Keras mode -- one dense launch
per (group, device) over a five-array descriptor (fil_amsgrad_multi), runs tables in place (fil_embed_amsgrad_runs, or with an exchange
fil_embed_amsgrad_merged, then fil_embed_amsgrad_sweep over every other row of every non-frozen field), schedules and decay=, capture,
the data-parallel route.  Whole-variable semantics: an untouched row's m and v decay, its vhat holds, and it keeps moving on the old,
larger denominator.  The table m and v are formed by Adam's own helpers: bit-equal to an optim.Adam run on the same gradients.  Not
with sweep_period (the deferred ring and replays carry no third slot) and not with lazy_tables (ValueError); state_dict() carries vhat
and a top-level "amsgrad": True only when it is on, and loading across the flag raises.  An Adam built without amsgrad makes exactly the
calls it made before.  The sweep writes a lane's vhat only where its bits change (never on an untouched row of an unregularised
field: 28 bytes per element there, 32 elsewhere, against Adam's 24).  Measured (profiles/r21_optim_amsgrad_bench.txt, 33.8 M rows x
K=16, replayed): 3.45 ms with no field regularised and 3.90 ms with every one, against Adam's 3.13 ms in the same run -- 1.10 and 1.24
of Adam's step for 1.17 and 1.33 of its bytes, 0.70 / 0.71 of 6.3 TB/s against Adam's 0.67.

Only fp32 parameters on a GPU are supported: anything else raises (there is no CPU / eager fallback).
"""
import ctypes
import weakref

import torch
import torch.distributed as dist
from torch.utils.weak import WeakIdKeyDictionary

from . import _lib, schedules
from ._lib import (FIL_ADAM_KERAS, FIL_ADAM_LAZY, FIL_ADAM_ROLL_FLUSH, FIL_ADAM_ROLL_SKIP, FIL_ADAM_ROLL_STEP, FIL_MOMOPT_NESTEROV,
                   FIL_OPT_ADADELTA, FIL_OPT_ADAGRAD, FIL_OPT_ADAMAX, FIL_OPT_FTRL, FIL_OPT_NADAM, FIL_OPT_RMSPROP, FIL_OPT_SGD, AdaoptHyper,
                   AmsgradTensor, FilError, MomoptHyper, NadamHyper, RowoptHyper, check, ptr, stream_ptr)


class _Desc(ctypes.Structure):
    """fil_adam_tensor (include/fil.h)"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("l2", ctypes.c_float), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(_Desc) == 48


def _rated(lib, name, lr):
    """The entry point `name` for a rate that is a float (by value) or a device tensor (its _lrdev variant, include/fil.h O3):
    (function, rate argument, name for messages)."""
    if isinstance(lr, torch.Tensor):
        return getattr(lib, name + "_lrdev"), lr.data_ptr(), name + "_lrdev"
    return getattr(lib, name), lr, name


def _rate_pair(lr):
    """The (lr, lr_dev) of an entry point that takes both (include/fil.h O7): a float by value, or a device tensor's address."""
    if isinstance(lr, torch.Tensor):
        return 0.0, lr.data_ptr()
    return lr, None


def _check_rate(who, learning_rate, decay):
    if isinstance(learning_rate, schedules.LearningRateSchedule):
        pass
    elif not learning_rate >= 0.0:
        raise ValueError("%s: learning_rate=%r (>= 0, or a schedules.LearningRateSchedule)" % (who, learning_rate))
    if decay < 0.0:
        raise ValueError("decay cannot be less than 0: {}".format(decay))
    return learning_rate if isinstance(learning_rate, schedules.LearningRateSchedule) else float(learning_rate), float(decay)


def _decay_entry(decay):
    """The `decay` entry of an optimizer's defaults: present only when it is used, so an optimizer built without it has the defaults
    (and the param groups, and the state_dict) it always had."""
    return {"decay": decay} if decay > 0.0 else {}


def _float_rate(group):
    """The group's by-value rate (0 for a schedule: the launches that take it read no rate)."""
    lr = group["learning_rate"]
    return 0.0 if isinstance(lr, schedules.LearningRateSchedule) else lr


MAX_SWEEP_PERIOD = 1023     # the ring (D >= N + 1 entries, a power of two) sits in LDS in fil_embed_adam_roll: D <= 1024


# runs table -> its _Deferred state.  Keyed by identity and weakly: nothing is stored on the Parameter (a pickled module stays
# picklable) and the registry keeps no table alive.  The state outlives its optimizer until that optimizer is finalised, which
# flushes the table and removes the entry: a table is never left lagging with nobody to bring it current.
_DEFERRED = WeakIdKeyDictionary()


class _Deferred:
    """One table's deferred state, shared by its optimizer and the table's readers (the forward's catch-up, SparseEmbed's
    state-dict hook and regulariser).  Holds the table and the optimizer weakly and everything a catch-up or a flush needs
    strongly: moments, step counter, stamps, ring, the fields of the last record."""

    def __init__(self, opt, p, m, v, t, N):
        self.opt = weakref.ref(opt)
        self.table = weakref.ref(p)
        self.m, self.v, self.t, self.N = m, v, t, N
        D = int(_lib.load().fil_embed_adam_ring_len(N))
        self.stamp = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
        self.stamp.copy_(t.expand(p.shape[0]))             # current through the completed steps
        self.ring = torch.zeros((D, 4), dtype=torch.float32, device=p.device)
        self.fields = None
        # (for flush(), which reads no rate)
        self.hyper = (_float_rate(opt.defaults), opt.defaults["beta_1"], opt.defaults["beta_2"], opt.defaults["epsilon"])

    def field_args(self, p, rec=None):
        """(offsets, field_l2, frozen, F) for the replays: the record's, else the last one seen.  Before any record or forward every
        step of this table was a skip step, and a replay of those changes nothing: one field without l2 is then exact."""
        if rec is not None:
            self.fields = (rec["offsets"], rec.get("field_l2"), rec.get("frozen"))
        if self.fields is None:
            self.fields = (torch.zeros(1, dtype=torch.int64, device=p.device), None, None)
        offsets, field_l2, frozen = self.fields
        return offsets, field_l2, frozen, int(offsets.numel())

    def catch_up(self, p, sorted_ids, rec):
        """The forward's launch: the record's rows current through the completed steps, in place (fil_embed_adam_catchup_runs)."""
        V, K = p.shape
        offsets, field_l2, frozen, F = self.field_args(p, rec)
        with torch.cuda.device(p.device):
            check(_lib.load().fil_embed_adam_catchup_runs(ptr(sorted_ids), sorted_ids.numel(), K, ptr(p), ptr(self.m), ptr(self.v),
                                                          ptr(self.stamp), ptr(self.ring), self.N, ptr(offsets), ptr(field_l2),
                                                          ptr(frozen), F, V, ptr(self.t), stream_ptr()), "fil_embed_adam_catchup_runs")

    def roll(self, p, hyper, flags, rec=None):
        V, K = p.shape
        offsets, field_l2, frozen, F = self.field_args(p, rec)
        fn, lr, name = _rated(_lib.load(), "fil_embed_adam_roll", hyper[0])
        with torch.cuda.device(p.device):
            check(fn(ptr(p), ptr(self.m), ptr(self.v), ptr(self.stamp), ptr(self.ring), self.N, V, K, ptr(offsets), ptr(field_l2),
                     ptr(frozen), F, ptr(self.t), lr, *hyper[1:], flags, stream_ptr()), name)

    @torch.no_grad()
    def flush(self):
        p = self.table()
        if p is not None:
            self.roll(p, self.hyper, FIL_ADAM_ROLL_FLUSH)


def _release(states):
    """An optimizer with deferred tables is finalised: flush every table it still owns and detach it (the table is then current and
    an ordinary runs table again)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return      # (never launch into someone's capture: the states stay registered, and the readers still catch up through them)
    for st in states:
        p = st.table()
        if p is not None and _DEFERRED.get(p) is st:
            st.flush()
            del _DEFERRED[p]


def deferred_state(table):
    """The _Deferred state of a table in deferred Keras mode (optim.Adam(sweep_period)), or None."""
    return _DEFERRED.get(table)


def deferred_optimizer(table):
    """The live deferred optim.Adam a table is attached to (sweep_period), or None."""
    st = _DEFERRED.get(table)
    return st.opt() if st is not None else None


class _RunsOptimizer(torch.optim.Optimizer):
    """What the fused optimizers of this module share: the device step counter (Keras' iterations), the staged descriptor arrays of
    the one dense launch per (group, device), the pending runs records, the row stamps, the data-parallel exchange of the runs
    tables, the step loop and the state.  A subclass sets _NAME (its name in messages) and _SLOTS (the state keys of its per-element
    slots: up to three, none for a rule without state; an instance may set its own) and supplies _slot_init (their initial values), _hyper, _launch_dense and _apply_runs; Adam's deferred mode hooks in
    through _skip and _admit."""
    _NAME = None
    _SLOTS = ()

    def __init__(self, params, defaults, process_group, force_exchange):
        if process_group is not None and not isinstance(process_group, dist.ProcessGroup):
            raise TypeError("%s: process_group must be a torch.distributed.ProcessGroup or None, not %r" % (self._NAME, process_group))
        if not isinstance(force_exchange, bool):
            raise TypeError("%s: force_exchange must be a bool, not %r" % (self._NAME, force_exchange))
        self._t = {}            # device -> int64 [1] step counter (Keras' iterations)
        self._stamps = {}       # runs table -> int32 [V] row stamps of the sweep (valid within one step only: not state)
        self._descs = {}        # descriptor key -> (device descriptors, pinned host copy)
        self._pinned = []       # descriptor arrays built during a stream capture: a graph replays them, they are never dropped
        # pinned staging for descriptors built DURING a capture: a host allocation there would invalidate it, so it is reserved by
        # the first eager step; a captured copy reads its slice at every replay, so a slice is never handed out twice
        self._arena, self._arena_off = None, 0
        self._rates = {}        # (group index, device) -> (key, device fil_lr_schedule, fp32 [1] rate of the step): schedules / decay only
        self._xbuf = {}         # runs table -> buffers of the data-parallel exchange (cap fixed on the first step, reused after)
        self.process_group = process_group
        self.force_exchange = force_exchange
        super().__init__(params, defaults)

    def _counter(self, dev):
        t = self._t.get(dev)
        if t is None:
            t = self._t[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
        return t

    def _stamp(self, p):
        s = self._stamps.get(p)
        if s is None:
            s = self._stamps[p] = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
        return s

    @property
    def iterations(self):
        """Completed steps (Keras' optimizer.iterations), as a host int (synchronises)."""
        return int(next(iter(self._t.values()))[0]) if self._t else 0

    # -- the rate (include/fil.h O3) ---------------------------------------------------------------------------------
    @staticmethod
    def _on_device(group):
        """Is the group's rate computed on the device: a schedule, or the legacy decay."""
        return isinstance(group["learning_rate"], schedules.LearningRateSchedule) or group.get("decay", 0.0) > 0.0

    def _rate_state(self, gi, group, dev):
        """The group's descriptor and rate word on `dev`, built on first use (and again when the group's rate was replaced)."""
        lr, decay = group["learning_rate"], group.get("decay", 0.0)
        if decay < 0.0:
            raise ValueError("decay cannot be less than 0: {}".format(decay))
        key = (schedules.serialize(lr) if isinstance(lr, schedules.LearningRateSchedule) else float(lr), float(decay))
        hit = self._rates.get((gi, dev))
        if hit is not None and hit[0] == key:
            return hit
        if torch.cuda.is_current_stream_capturing():
            raise FilError("%s: the learning-rate schedule of a captured step has no descriptor on %s yet -- run one eager step before "
                           "capturing (capture.capture_step's warm-up does)" % (self._NAME, dev))
        d = (lr.descriptor(decay) if isinstance(lr, schedules.LearningRateSchedule) else schedules.constant_descriptor(lr, decay))
        check(_lib.load().fil_lr_schedule_check(ctypes.addressof(d)), "fil_lr_schedule_check")
        host = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8)
        hit = self._rates[(gi, dev)] = (key, host.to(dev), torch.zeros(1, dtype=torch.float32, device=dev))
        return hit

    def _eval_rate(self, gi, group, dev, out=None):
        """Enqueues fil_lr_schedule_eval of the group on `dev`: the rate of the step about to run, into the group's rate word (or
        `out`); returns the tensor written."""
        _, desc, word = self._rate_state(gi, group, dev)
        out = word if out is None else out
        with torch.cuda.device(dev):
            check(_lib.load().fil_lr_schedule_eval(ptr(desc), ptr(self._counter(dev)), ptr(out), stream_ptr()), "fil_lr_schedule_eval")
        return out

    def _step_rates(self):
        """Per parameter group: None (a float rate, by value) or {device: the rate word}, with one fil_lr_schedule_eval per (group,
        device) enqueued -- before any update launch of the step, so every one of them reads the same bits."""
        out = []
        for gi, group in enumerate(self.param_groups):
            if not self._on_device(group):
                out.append(None)
                continue
            devs = []
            for p in group["params"]:
                if p.device.type == "cuda" and p.device not in devs:
                    devs.append(p.device)
            out.append({dev: self._eval_rate(gi, group, dev) for dev in devs})
        return out

    def current_learning_rate(self, group=0):
        """Keras' _decayed_lr of parameter group `group` for the step about to run: a 0-dim fp32 device tensor, computed on the
        device from the step counter without synchronising (float() of it is the caller's synchronisation)."""
        g = self.param_groups[group]
        dev = next((p.device for p in g["params"] if p.device.type == "cuda"), None)
        if dev is None:
            raise FilError("%s: parameter group %d has no GPU parameter" % (self._NAME, group))
        if not self._on_device(g):
            return torch.full((), g["learning_rate"], dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        return self._eval_rate(group, g, dev, out).reshape(())

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none=set_to_none)
        for g in self.param_groups:
            for p in g["params"]:
                if getattr(p, "_fil_pending_runs", None) is not None:
                    p._fil_pending_runs = None

    # -- what a subclass supplies ----------------------------------------------------------------------------------
    def _slot_init(self, group):
        """The initial values of the _SLOTS of a parameter in `group`."""
        raise NotImplementedError

    def _hyper(self, group, lr_dev=None, dev=None):
        """The group's hyper-parameters; lr_dev: the device word holding the step's rate (a schedule / decay), else by value; dev: the
        device of the launches that will take them (for a rule that keeps a device word of its own there; the others ignore it)."""
        raise NotImplementedError

    def _launch_dense(self, lib, desc, n, numel, t, hyper, advance):
        """The dense launch of one (group, device): n descriptors of numel elements in all; advance: the step counter t too."""
        raise NotImplementedError

    def _apply_runs(self, lib, p, pend, s0, s1, t, hyper):
        raise NotImplementedError

    def _skip(self, p, hyper):
        """A parameter without a gradient or a record at this step."""

    def _admit(self, p, pend):
        """Checks a parameter with a gradient or a record before anything else."""

    # -- state ---------------------------------------------------------------------------------------------------
    def _slots(self, p, group):
        """The parameter's slot tensors, made on first use: two of them (None for a slot the rule does not have), three for a rule
        with a third."""
        if not self._SLOTS:
            return None, None
        st = self.state[p]
        if self._SLOTS[0] not in st:
            for k, x in zip(self._SLOTS, self._slot_init(group)):
                st[k] = torch.full_like(p, x, memory_format=torch.contiguous_format)
        slots = tuple(st[k] for k in self._SLOTS)
        return slots if len(slots) > 1 else slots + (None,)

    def state_dict(self):
        sd = super().state_dict()
        sd["iterations"] = self.iterations
        # a schedule travels as its config ({"class_name", "config"}), not as an object
        sd["param_groups"] = [dict(g, learning_rate=schedules.serialize(g["learning_rate"]))
                              if isinstance(g.get("learning_rate"), schedules.LearningRateSchedule) else g for g in sd["param_groups"]]
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        it = int(state_dict.pop("iterations", 0))
        state_dict["param_groups"] = [dict(g, learning_rate=schedules.deserialize(g["learning_rate"]))
                                      if isinstance(g.get("learning_rate"), dict) else g for g in state_dict["param_groups"]]
        super().load_state_dict(state_dict)
        for st in self.state.values():          # (torch's loader may hand non-contiguous copies back)
            for k in self._SLOTS:
                if k in st:
                    st[k] = st[k].contiguous()
        for g in self.param_groups:
            for p in g["params"]:
                self._counter(p.device)
        for t in self._t.values():
            t.fill_(it)
        for s in self._stamps.values():         # t may go backwards: a stale stamp must never look current
            s.zero_()

    def reset_(self):
        """Back to "never stepped" IN PLACE (slots, stamps and counter keep their storage): what a capture's restore needs after
        warm-up steps (capture.capture_step(..., restore=...))."""
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p, {})
                for k, x in zip(self._SLOTS, self._slot_init(group)):
                    if k in st:
                        st[k].fill_(x)
        for s in self._stamps.values():
            s.zero_()
        for t in self._t.values():
            t.zero_()

    # -- the step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        rates = self._step_rates()
        calls = []      # (device, hyper, entries) of the dense launches, in group order
        for group, rate in zip(self.param_groups, rates):
            hypers = {}     # device -> the group's hyper-parameters there (they differ by device only in the rate word)
            per_dev = {}
            for p in group["params"]:
                hyper = hypers.get(p.device)
                if hyper is None:
                    hyper = hypers[p.device] = self._hyper(group, rate.get(p.device) if rate else None, p.device)
                pend = getattr(p, "_fil_pending_runs", None)
                if pend is None and p.grad is None:
                    self._skip(p, hyper)        # (Keras filters None gradients)
                    continue
                self._admit(p, pend)
                if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                    raise FilError("%s: parameter %s %s on %s -- contiguous fp32 GPU tensors only" % (self._NAME, tuple(p.shape), p.dtype,
                                                                                                   p.device))
                slots = self._slots(p, group)
                t = self._counter(p.device)
                if pend is not None:
                    if p.grad is not None:
                        raise FilError("%s: table %s has both a .grad and a pending runs record (a gradient reached the table "
                                       "outside its gather -- e.g. a regulariser not detached)" % (self._NAME, tuple(p.shape)))
                    self._apply_runs(lib, p, pend, *slots, t, hyper)
                    p._fil_pending_runs = None
                    continue
                g = p.grad
                if g.is_sparse:
                    raise FilError("%s: sparse gradient of %s -- use SparseEmbed(grad_mode='runs') for the tables" % (self._NAME,
                                                                                                                    tuple(p.shape)))
                if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                    raise FilError("%s: gradient of %s must be a dense contiguous fp32 tensor of its shape" % (self._NAME, tuple(p.shape)))
                per_dev.setdefault(p.device, []).append((p.data_ptr(), g.data_ptr(), *[ptr(x) for x in slots], p.numel(), 0.0))
            for dev, entries in per_dev.items():
                calls.append((dev, hypers[dev], entries))
        # the last launch on every device advances its counter -- one with no tensors where nothing dense had a gradient
        devs = set(self._t)
        for g in self.param_groups:
            for p in g["params"]:
                if p.device.type == "cuda":
                    devs.add(p.device)
        last = {}
        for i, (dev, _, _) in enumerate(calls):
            last[dev] = i
        for dev in devs:
            if dev not in last:
                calls.append((dev, self._hyper(dict(self.defaults, learning_rate=_float_rate(self.defaults)), None, dev), []))  # (reads no rate)
                last[dev] = len(calls) - 1
        for i, (dev, hyper, entries) in enumerate(calls):
            with torch.cuda.device(dev):
                desc = self._desc_array(dev, entries) if entries else None
                self._launch_dense(lib, desc, len(entries), sum(e[-2] for e in entries), self._counter(dev), hyper,
                                   1 if last[dev] == i else 0)
        return loss

    def _desc_array(self, dev, entries):
        key = (dev, tuple(entries))
        hit = self._descs.get(key)
        if hit is not None:
            return hit[0]
        # an entry: (param, grad, the slots, numel, l2) -- fil_adam_tensor, or with a third slot fil_amsgrad_tensor
        cls = _Desc if len(entries[0]) == 6 else AmsgradTensor
        host = (cls * len(entries))(*[cls(*e, 0) for e in entries])
        size = ctypes.sizeof(host)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            if self._arena is None or self._arena_off + size > self._arena.numel():
                raise FilError("%s: no room for the descriptors of a captured step -- run one eager step before capturing "
                               "(capture.capture_step's warm-up does)" % self._NAME)
            pinned = self._arena[self._arena_off:self._arena_off + size]
            self._arena_off += (size + 255) // 256 * 256
        else:
            if self._arena is None:
                self._arena = torch.empty(max(1 << 16, 8 * size), dtype=torch.uint8, pin_memory=True)
            pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        ctypes.memmove(pinned.data_ptr(), ctypes.addressof(host), size)
        d = torch.empty(size, dtype=torch.uint8, device=dev)
        d.copy_(pinned, non_blocking=True)
        if capturing:
            self._pinned.append((d, pinned))
        else:
            if len(self._descs) >= 16:
                self._descs.clear()
            self._descs[key] = (d, pinned)
        return d

    def _exchange_world(self):
        """The world size of the runs exchange, or 0 for the one-GPU path (no group of > 1 ranks and no force_exchange)."""
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(self.process_group)
            if world > 1 or self.force_exchange:
                return world
            return 0
        if self.process_group is not None:
            raise FilError("%s: a process_group was given but torch.distributed is not initialised" % self._NAME)
        return 1 if self.force_exchange else 0

    def _exchange_buffers(self, p, pend, world):
        V, K = p.shape
        R = int(pend["R"])
        buf = self._xbuf.get(p)
        if buf is None:
            dev = p.device
            if world > 1 or dist.is_initialized():      # one all-reduce MAX of R: every rank's lists get the same capacity
                r = torch.tensor([R], dtype=torch.int64, device=dev)
                dist.all_reduce(r, op=dist.ReduceOp.MAX, group=self.process_group)
                cap = int(r.item())
            else:
                cap = R
            cap = max(cap, 1)
            lib = _lib.load()
            ids = torch.empty(cap, dtype=torch.int64, device=dev)
            values = torch.empty(cap * K, dtype=torch.float32, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = torch.empty(max(1, int(lib.fil_embed_runs_compact_workspace_bytes(cap))), dtype=torch.uint8, device=dev)
            if world > 1 or dist.is_initialized():
                gathered = (torch.empty(world * cap, dtype=torch.int64, device=dev),
                            torch.empty(world * cap * K, dtype=torch.float32, device=dev),
                            torch.empty(world, dtype=torch.int64, device=dev))
            else:
                gathered = (ids, values, count)        # no process group (force_exchange): the local list IS the gathered one
            buf = self._xbuf[p] = dict(cap=cap, ids=ids, values=values, count=count, ws=ws, gathered=gathered)
        if R > buf["cap"]:
            raise FilError("%s: runs record of %d entries > the exchange capacity %d agreed on the first step (the first "
                           "batch must be the largest)" % (self._NAME, R, buf["cap"]))
        return buf

    def _compact_and_exchange(self, lib, p, pend, world, st):
        """fil_embed_runs_compact of the record, then dp.exchange_runs (nothing to exchange without a process group): the W
        gathered lists (ids, values, counts) and their capacity."""
        from . import dp
        K = p.shape[1]
        buf = self._exchange_buffers(p, pend, world)
        cap = buf["cap"]
        check(lib.fil_embed_runs_compact(ptr(pend["g"]), ptr(pend["perm"]), ptr(pend["sorted_ids"]), pend["R"], K, pend["g_dtype"],
                                         ptr(buf["ids"]), ptr(buf["values"]), ptr(buf["count"]), cap, ptr(buf["ws"]), buf["ws"].numel(),
                                         st), "fil_embed_runs_compact")
        ids, values, counts = buf["gathered"]
        if ids is not buf["ids"]:
            dp.exchange_runs(buf["ids"], buf["values"], buf["count"], ids, values, counts, group=self.process_group)
        return ids, values, counts, cap


class Adam(_RunsOptimizer):
    _NAME = "optim.Adam"
    _SLOTS = ("m", "v")

    def __init__(self, params, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, lazy_tables=False, process_group=None,
                 force_exchange=False, sweep_period=None, decay=0.0, amsgrad=False):
        if not isinstance(amsgrad, bool):
            raise TypeError("Adam: amsgrad must be a bool, not %r" % (amsgrad,))
        learning_rate, decay = _check_rate("Adam", learning_rate, decay)
        if not 0.0 <= beta_1 < 1.0 or not 0.0 <= beta_2 < 1.0 or not epsilon >= 0.0:
            raise ValueError("Adam: learning_rate=%r beta_1=%r beta_2=%r epsilon=%r (rate, epsilon >= 0; betas in [0, 1))"
                             % (learning_rate, beta_1, beta_2, epsilon))
        if sweep_period is not None:
            if isinstance(sweep_period, bool) or not isinstance(sweep_period, int):
                raise TypeError("Adam: sweep_period must be an int or None, not %r" % (sweep_period,))
            if not 1 <= sweep_period <= MAX_SWEEP_PERIOD:
                raise ValueError("Adam: sweep_period %d (1 ... %d)" % (sweep_period, MAX_SWEEP_PERIOD))
            if lazy_tables:
                raise ValueError("Adam: sweep_period (deferred Keras mode) and lazy_tables exclude each other")
        if amsgrad and sweep_period is not None:
            raise ValueError("Adam: amsgrad and sweep_period exclude each other (the deferred ring and replays carry no third slot)")
        if amsgrad and lazy_tables:
            raise ValueError("Adam: amsgrad and lazy_tables exclude each other (the lazy mode is a labelled deviation with nothing to "
                             "pin an AMSGrad form against)")
        self.amsgrad = amsgrad
        if amsgrad:
            self._SLOTS = ("m", "v", "vhat")        # Keras' slot name; zeros
        # (set before the base class adds the parameter groups: add_param_group attaches their runs tables)
        self.sweep_period = sweep_period
        self.lazy_tables = bool(lazy_tables)
        self._defer = {}        # deferred runs table -> its _Deferred state (also in _DEFERRED, for the table's readers)
        self._released = []     # the same states, for the finaliser (which must not hold the optimizer)
        if sweep_period is not None:
            fin = weakref.finalize(self, _release, self._released)
            fin.atexit = False
        super().__init__(params, dict(learning_rate=learning_rate, beta_1=float(beta_1), beta_2=float(beta_2),
                                      epsilon=float(epsilon), **_decay_entry(decay)), process_group, force_exchange)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if self.sweep_period is not None:           # deferred mode: the group's runs tables join it now
            for p in self.param_groups[-1]["params"]:
                if getattr(p, "_fil_runs_table", False):
                    self._attach(p)

    def _slot_init(self, group):
        return (0.0,) * len(self._SLOTS)

    def _hyper(self, group, lr_dev=None, dev=None):
        return group["learning_rate"] if lr_dev is None else lr_dev, group["beta_1"], group["beta_2"], group["epsilon"]

    def _launch_dense(self, lib, desc, n, numel, t, hyper, advance):
        if self.amsgrad:
            check(lib.fil_amsgrad_multi(ptr(desc), n, numel, ptr(t), *_rate_pair(hyper[0]), *hyper[1:], advance, stream_ptr()),
                  "fil_amsgrad_multi")
            return
        fn, lr, name = _rated(lib, "fil_adam_multi", hyper[0])
        check(fn(ptr(desc), n, numel, ptr(t), lr, *hyper[1:], advance, stream_ptr()), name)

    def state_dict(self):
        self.flush()
        sd = super().state_dict()
        if self.amsgrad:
            sd["amsgrad"] = True
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        flag = bool(state_dict.pop("amsgrad", False))
        if flag != self.amsgrad:
            raise FilError("optim.Adam: the checkpoint was taken with amsgrad=%r, this optimizer has amsgrad=%r" % (flag, self.amsgrad))
        if self.amsgrad:
            for k, st in state_dict.get("state", {}).items():
                if "m" in st and "vhat" not in st:
                    raise FilError("optim.Adam: parameter %r of the checkpoint has m but no vhat (amsgrad=True)" % (k,))
        super().load_state_dict(state_dict)
        it = int(state_dict.get("iterations", 0))
        for p, d in self._defer.items():        # deferred: a checkpoint is taken flushed -- every row is current through `it`
            d.m, d.v = self._slots(p, None)    # (the loader replaced the moments)
            d.stamp.fill_(it)

    def reset_(self):
        super().reset_()
        for d in self._defer.values():
            d.stamp.zero_()

    # -- deferred mode hooks of the step -----------------------------------------------------------------------------
    def _skip(self, p, hyper):
        if p in self._defer:                    # Keras mode leaves the table alone at this step: the ring says so
            self._defer[p].roll(p, hyper, FIL_ADAM_ROLL_SKIP)

    def _admit(self, p, pend):
        if self.amsgrad and deferred_state(p) is not None:
            raise FilError("optim.Adam: table %s is in another optim.Adam's deferred mode (sweep_period) -- drop that optimizer first"
                           % (tuple(p.shape),))
        if pend is not None and self.sweep_period is not None and p not in self._defer:
            # a runs table that was not one when it joined (swept every step so far, so current): deferred from now on
            self._attach(p)
        if pend is None and p in self._defer:
            raise FilError("optim.Adam: deferred table %s has a .grad -- with sweep_period its gradient must arrive as runs "
                           "(SparseEmbed(grad_mode='runs'))" % (tuple(p.shape),))

    def _apply_runs_amsgrad(self, lib, p, pend, m, v, vhat, t, hyper):
        """amsgrad=True: fil_embed_amsgrad_runs, or with an exchange fil_embed_amsgrad_merged of the gathered lists; then
        fil_embed_amsgrad_sweep over every row the update did not stamp (include/fil.h O7)."""
        r, b1, b2, eps = hyper
        lr, lr_dev = _rate_pair(r)
        V, K = p.shape
        stamp = self._stamp(p)
        with torch.cuda.device(p.device):
            st = stream_ptr()
            world = self._exchange_world()
            if world:
                ids, values, counts, cap = self._compact_and_exchange(lib, p, pend, world, st)
                check(lib.fil_embed_amsgrad_merged(ptr(ids), ptr(values), ptr(counts), world, cap, K, ptr(pend["offsets"]),
                                                   ptr(pend["field_l2"]), pend["F"], ptr(p), ptr(m), ptr(v), ptr(vhat), ptr(stamp), V,
                                                   ptr(t), lr, lr_dev, b1, b2, eps, st), "fil_embed_amsgrad_merged")
            else:
                check(lib.fil_embed_amsgrad_runs(ptr(pend["g"]), ptr(pend["perm"]), ptr(pend["sorted_ids"]), pend["R"], K,
                                                 pend["g_dtype"], pend["F"], ptr(pend["field_l2"]), ptr(p), ptr(m), ptr(v), ptr(vhat),
                                                 ptr(stamp), ptr(t), lr, lr_dev, b1, b2, eps, st), "fil_embed_amsgrad_runs")
            check(lib.fil_embed_amsgrad_sweep(ptr(p), ptr(m), ptr(v), ptr(vhat), ptr(stamp), V, K, ptr(pend["offsets"]),
                                              ptr(pend["field_l2"]), ptr(pend["frozen"]), pend["F"], ptr(t), lr, lr_dev, b1, b2, eps, st),
                  "fil_embed_amsgrad_sweep")

    def _apply_runs(self, lib, p, pend, m, v, *rest):
        """One table's step from its runs record.  The update: fil_embed_adam_runs, or with an exchange (data parallel,
        force_exchange) fil_embed_adam_merged of the gathered lists; either in its _deferred form for a deferred table.  Then the rows
        the batch did not touch: a deferred table's roll, Keras mode's sweep, nothing in lazy mode."""
        if self.amsgrad:
            return self._apply_runs_amsgrad(lib, p, pend, m, v, *rest)
        t, hyper = rest
        lr, b1, b2, eps = hyper
        V, K = p.shape
        d = self._defer.get(p)
        if d is not None:
            offsets, field_l2, frozen, F = d.field_args(p, pend)
            stamp = d.stamp
        else:
            mode = FIL_ADAM_LAZY if self.lazy_tables else FIL_ADAM_KERAS
            stamp = self._stamp(p) if mode == FIL_ADAM_KERAS else None
        with torch.cuda.device(p.device):
            st = stream_ptr()
            world = self._exchange_world()
            if world:
                ids, values, counts, cap = self._compact_and_exchange(lib, p, pend, world, st)
                if d is not None:
                    fn, r, name = _rated(lib, "fil_embed_adam_merged_deferred", lr)
                    check(fn(ptr(ids), ptr(values), ptr(counts), world, cap, K, ptr(offsets), ptr(field_l2), ptr(frozen), F, ptr(p),
                             ptr(m), ptr(v), ptr(stamp), ptr(d.ring), self.sweep_period, V, ptr(t), r, b1, b2, eps, st), name)
                else:
                    fn, r, name = _rated(lib, "fil_embed_adam_merged", lr)
                    check(fn(ptr(ids), ptr(values), ptr(counts), world, cap, K, ptr(pend["offsets"]), ptr(pend["field_l2"]), pend["F"],
                             ptr(p), ptr(m), ptr(v), ptr(stamp), V, ptr(t), r, b1, b2, eps, mode, st), name)
            elif d is not None:
                fn, r, name = _rated(lib, "fil_embed_adam_runs_deferred", lr)
                check(fn(ptr(pend["g"]), ptr(pend["perm"]), ptr(pend["sorted_ids"]), pend["R"], K, pend["g_dtype"], F, ptr(offsets),
                         ptr(field_l2), ptr(frozen), ptr(p), ptr(m), ptr(v), ptr(stamp), ptr(d.ring), self.sweep_period, V, ptr(t), r,
                         b1, b2, eps, st), name)
            else:
                fn, r, name = _rated(lib, "fil_embed_adam_runs", lr)
                check(fn(ptr(pend["g"]), ptr(pend["perm"]), ptr(pend["sorted_ids"]), pend["R"], K, pend["g_dtype"], pend["F"],
                         ptr(pend["field_l2"]), ptr(p), ptr(m), ptr(v), ptr(stamp), ptr(t), r, b1, b2, eps, mode, st), name)
            if d is not None:
                d.roll(p, hyper, FIL_ADAM_ROLL_STEP)
            elif mode == FIL_ADAM_KERAS:
                fn, r, name = _rated(lib, "fil_embed_adam_sweep", lr)
                check(fn(ptr(p), ptr(m), ptr(v), ptr(stamp), V, K, ptr(pend["offsets"]), ptr(pend["field_l2"]), ptr(pend["frozen"]),
                         pend["F"], ptr(t), r, b1, b2, eps, st), name)

    # -- deferred mode -----------------------------------------------------------------------------------------------
    def _attach(self, p):
        """A runs table joins deferred mode: moments now (the forward's catch-up may run before the first step), stamps at the
        current count, the ring, and its entry in the registry that the forward and SparseEmbed follow."""
        if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous() or p.dim() != 2:
            raise FilError("optim.Adam: deferred table %s %s on %s -- a contiguous fp32 [V, K] GPU tensor" % (tuple(p.shape), p.dtype,
                                                                                                               p.device))
        if p in self._defer:
            return
        old = _DEFERRED.get(p)
        if old is not None:
            if old.opt() is not None:
                raise FilError("optim.Adam: table %s already belongs to another deferred optimizer" % (tuple(p.shape),))
            _release([old])                 # its optimizer is gone but not yet finalised: bring the table current first
        m, v = self._slots(p, None)
        d = self._defer[p] = _Deferred(self, p, m, v, self._counter(p.device), self.sweep_period)
        self._released.append(d)
        _DEFERRED[p] = d

    @torch.no_grad()
    def flush(self):
        """Deferred mode: bring every row of every deferred table current (table, m and v then hold exactly what Keras mode holds).
        A no-op without sweep_period.  Also done when the optimizer is finalised."""
        for d in self._defer.values():
            d.flush()


class _Rowwise(_RunsOptimizer):
    """Keras' Adagrad and Ftrl (include/fil.h O2): optim.Adam's contract with a row-local rule.  Slots: `accumulator` (filled with
    initial_accumulator_value) and, for Ftrl, `linear` (zeros).  Dense parameters: one fil_rowopt_multi launch per (group, device);
    runs tables: fil_embed_rowopt_runs (or, data parallel, fil_embed_runs_compact + dp.exchange_runs + fil_embed_rowopt_merged),
    then fil_embed_rowopt_sweep over the untouched rows of the regularised fields only.  Row stamps exist only for tables with a
    regularised field.  SGD and RMSprop (O4) take the same calls at their own entry points (_ENTRY: the O4 argument lists are O2's),
    RMSprop with momentum == 0 with a sweep, hence stamps, for every table (_sweeps); Adadelta and Adamax (O5) likewise, and Nadam
    (O6), which always sweeps."""
    _RULE = None
    _ENTRY = ("fil_rowopt_multi", "fil_embed_rowopt_runs", "fil_embed_rowopt_sweep", "fil_embed_rowopt_merged")

    def _slot_init(self, group):
        return group["initial_accumulator_value"], 0.0

    @staticmethod
    def _rate_args(lib, name, hyper):
        """(entry point, the arguments from the hyper-parameters on, name): hyper = (RowoptHyper, the rate word or None)."""
        h, lr_dev = hyper
        if lr_dev is None:
            return getattr(lib, name), (ctypes.addressof(h),), name
        return getattr(lib, name + "_lrdev"), (ctypes.addressof(h), lr_dev.data_ptr()), name + "_lrdev"

    def _launch_dense(self, lib, desc, n, numel, t, hyper, advance):
        fn, h, name = self._rate_args(lib, self._ENTRY[0], hyper)
        check(fn(ptr(desc), n, numel, ptr(t), self._RULE, *h, advance, stream_ptr()), name)

    def _admit(self, p, pend):
        if deferred_state(p) is not None:
            raise FilError("%s: table %s is in optim.Adam's deferred mode (sweep_period) -- drop that optimizer first"
                           % (self._NAME, tuple(p.shape)))

    def _sweeps(self, field_l2):
        """Does a sweep follow the runs update of a table with these per-field l2 (None: no regularised field)."""
        return field_l2 is not None

    def _apply_runs(self, lib, p, pend, acc, lin, t, hyper):
        V, K = p.shape
        field_l2 = pend["field_l2"]
        # a regularised field: its untouched rows move too (the sweep), stamps tell them apart
        sweeps = self._sweeps(field_l2)
        stamp = self._stamp(p) if sweeps else None
        with torch.cuda.device(p.device):
            st = stream_ptr()
            world = self._exchange_world()
            if world:
                ids, values, counts, cap = self._compact_and_exchange(lib, p, pend, world, st)
                fn, h, name = self._rate_args(lib, self._ENTRY[3], hyper)
                check(fn(ptr(ids), ptr(values), ptr(counts), world, cap, K, ptr(pend["offsets"]), ptr(field_l2), pend["F"], ptr(p),
                         ptr(acc), ptr(lin), ptr(stamp), V, ptr(t), self._RULE, *h, st), name)
            else:
                fn, h, name = self._rate_args(lib, self._ENTRY[1], hyper)
                check(fn(ptr(pend["g"]), ptr(pend["perm"]), ptr(pend["sorted_ids"]), pend["R"], K, pend["g_dtype"], pend["F"],
                         ptr(field_l2), ptr(p), ptr(acc), ptr(lin), ptr(stamp), ptr(t), self._RULE, *h, st), name)
            if sweeps:
                fn, h, name = self._rate_args(lib, self._ENTRY[2], hyper)
                check(fn(ptr(p), ptr(acc), ptr(lin), ptr(stamp), V, K, ptr(pend["offsets"]), ptr(field_l2), ptr(pend["frozen"]),
                         pend["F"], ptr(t), self._RULE, *h, st), name)


class Adagrad(_Rowwise):
    """tf.keras.optimizers.Adagrad (TF 2.1; ApplyAdagradV2): acc += g^2;  p -= lr g / (sqrt(acc) + epsilon), with Keras' defaults
    (initial_accumulator_value 0.1 and epsilon 1e-7, where torch.optim.Adagrad has 0 and 1e-10).  Dense parameters take the rule
    on every element; runs tables (SparseEmbed(grad_mode="runs")) take Keras' per-field semantics in place: the batch's rows, plus
    every other row of a field with l2(emb_reg) > 0 (g = 2 emb_reg p); an untouched row of an unregularised field keeps its bits.
    A table in "dense" mode is an ordinary dense parameter.  process_group / force_exchange: as optim.Adam's."""
    _NAME = "optim.Adagrad"
    _RULE = FIL_OPT_ADAGRAD
    _SLOTS = ("accumulator",)

    def __init__(self, params, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, process_group=None,
                 force_exchange=False, decay=0.0):
        if epsilon is None:
            epsilon = 1e-7              # Keras: backend.epsilon()
        if initial_accumulator_value < 0.0:
            raise ValueError("initial_accumulator_value must be non-negative: %s" % initial_accumulator_value)
        learning_rate, decay = _check_rate("Adagrad", learning_rate, decay)
        if not epsilon >= 0.0:
            raise ValueError("Adagrad: learning_rate=%r epsilon=%r (both >= 0)" % (learning_rate, epsilon))
        super().__init__(params, dict(learning_rate=learning_rate, initial_accumulator_value=float(initial_accumulator_value),
                                      epsilon=float(epsilon), **_decay_entry(decay)), process_group, force_exchange)

    def _hyper(self, group, lr_dev=None, dev=None):
        return RowoptHyper(_float_rate(group), group["epsilon"], 0.0, 0.0, 0.0, 0.0), lr_dev


class Ftrl(_Rowwise):
    """tf.keras.optimizers.Ftrl (TF 2.1; ApplyFtrl, or ApplyFtrlV2 when l2_shrinkage_regularization_strength > 0), with Keras' names,
    defaults and checks (TF 2.1 has no `beta`).  Slots: accumulator n (initial_accumulator_value) and linear z (0); the rule is in
    include/fil.h O2.  Runs tables (SparseEmbed(grad_mode="runs")) take Keras' per-field semantics: the batch's rows, plus every other
    row of a field with l2(emb_reg) > 0 (g = 2 emb_reg p); every other row and its slots keep their bits -- NOT a dense apply with
    g = 0, which would recompute p from z and zero every untouched row.  Keras' quirk, reproduced: the first step takes the untouched
    rows of a regularised field to about -lr 2 emb_reg p / sqrt(n), in effect 0 (make_sparse_info's default emb_reg is 1e-8).
    Everything with a dense .grad -- a tableGrad="dense" table included -- takes the rule on every element: for such a table that is
    Keras' dense semantics, not its IndexedSlices ones; the exact Keras behaviour of unregularised fields needs tableGrad="runs".
    process_group / force_exchange: as optim.Adam's."""
    _NAME = "optim.Ftrl"
    _RULE = FIL_OPT_FTRL
    _SLOTS = ("accumulator", "linear")

    def __init__(self, params, learning_rate=0.001, learning_rate_power=-0.5, initial_accumulator_value=0.1,
                 l1_regularization_strength=0.0, l2_regularization_strength=0.0, l2_shrinkage_regularization_strength=0.0,
                 process_group=None, force_exchange=False, decay=0.0):
        if initial_accumulator_value < 0.0:
            raise ValueError("initial_accumulator_value %f needs to be positive or zero" % initial_accumulator_value)
        if learning_rate_power > 0.0:
            raise ValueError("learning_rate_power %f needs to be negative or zero" % learning_rate_power)
        if l1_regularization_strength < 0.0:
            raise ValueError("l1_regularization_strength %f needs to be positive or zero" % l1_regularization_strength)
        if l2_regularization_strength < 0.0:
            raise ValueError("l2_regularization_strength %f needs to be positive or zero" % l2_regularization_strength)
        if l2_shrinkage_regularization_strength < 0.0:
            raise ValueError("l2_shrinkage_regularization_strength %f needs to be positive or zero"
                             % l2_shrinkage_regularization_strength)
        learning_rate, decay = _check_rate("Ftrl", learning_rate, decay)
        super().__init__(params, dict(learning_rate=learning_rate, learning_rate_power=float(learning_rate_power),
                                      initial_accumulator_value=float(initial_accumulator_value),
                                      l1_regularization_strength=float(l1_regularization_strength),
                                      l2_regularization_strength=float(l2_regularization_strength),
                                      l2_shrinkage_regularization_strength=float(l2_shrinkage_regularization_strength),
                                      **_decay_entry(decay)),
                         process_group, force_exchange)

    def _hyper(self, group, lr_dev=None, dev=None):
        return RowoptHyper(_float_rate(group), 0.0, group["learning_rate_power"], group["l1_regularization_strength"],
                           group["l2_regularization_strength"], group["l2_shrinkage_regularization_strength"]), lr_dev


_MOMOPT_ENTRY = ("fil_momopt_multi", "fil_embed_momopt_runs", "fil_embed_momopt_sweep", "fil_embed_momopt_merged")


def _check_momentum(momentum):
    if isinstance(momentum, (int, float)) and (momentum < 0 or momentum > 1):
        raise ValueError("`momentum` must be between [0, 1].")
    return float(momentum)


class SGD(_Rowwise):
    """tf.keras.optimizers.SGD (TF 2.1): momentum == 0: p -= g lr; momentum > 0 (ApplyKerasMomentum): a = a momentum - g lr; p += a,
    or with nesterov p += a momentum - g lr.  The slot `momentum` (zeros) exists only when momentum > 0: plain SGD keeps no state
    tensors and its launches carry NULL slots.  Runs tables (SparseEmbed(grad_mode="runs")) take Keras' per-field semantics in place:
    the batch's rows, plus every other row of a field with l2(emb_reg) > 0 (g = 2 emb_reg p: its momentum decays and it moves); an
    untouched row of an unregularised field keeps its bits, its slot's too.  With momentum == 0 Keras scatter-adds each duplicate id of
    a batch separately, in an order it does not specify, so there are no bits to match: here the run is summed first, in
    fil_embed_run_sum's order, like every other rule.  Whether momentum is 0 is fixed at construction (a parameter group may change its
    value, not that).  process_group / force_exchange / decay / schedules: as optim.Adam's."""
    _NAME = "optim.SGD"
    _RULE = FIL_OPT_SGD
    _ENTRY = _MOMOPT_ENTRY

    def __init__(self, params, learning_rate=0.01, momentum=0.0, nesterov=False, process_group=None, force_exchange=False, decay=0.0):
        momentum = _check_momentum(momentum)
        learning_rate, decay = _check_rate("SGD", learning_rate, decay)
        self._SLOTS = ("momentum",) if momentum > 0.0 else ()
        super().__init__(params, dict(learning_rate=learning_rate, momentum=momentum, nesterov=bool(nesterov), **_decay_entry(decay)),
                         process_group, force_exchange)

    def _slot_init(self, group):
        return (0.0,) * len(self._SLOTS)

    def _hyper(self, group, lr_dev=None, dev=None):
        momentum = _check_momentum(group["momentum"])
        if (momentum > 0.0) != bool(self._SLOTS):
            raise ValueError("optim.SGD: a parameter group's momentum=%r -- whether momentum is 0 is fixed at construction" % momentum)
        return MomoptHyper(_float_rate(group), 0.0, 0.0, momentum, FIL_MOMOPT_NESTEROV if group["nesterov"] else 0, 0), lr_dev


class RMSprop(_Rowwise):
    """tf.keras.optimizers.RMSprop (TF 2.1), centered=False.  Slots: `rms` (zeros) and, only when momentum > 0, `momentum` (zeros).
    momentum == 0 (Keras' Python ops, epsilon outside the root): rms = rho rms + (1 - rho) g^2; p -= lr g / (sqrt(rms) + epsilon).
    momentum > 0 (ApplyRMSProp / SparseApplyRMSProp, epsilon inside the root): rms, then mom = mom momentum + lr g / sqrt(rms +
    epsilon); p -= mom (include/fil.h O4 has the two roundings).  Runs tables take Keras' per-field semantics in place.  With
    momentum > 0 the rule is row-local: the batch's rows, plus the other rows of the fields with l2(emb_reg) > 0.  With momentum == 0
    Keras decays rms over the whole variable (rms = rms * rho) and moves the batch's rows only: an untouched row of an unregularised
    field gets rms *= rho and keeps p, an untouched row of a regularised field takes the rule with g = 2 emb_reg p, a frozen field
    changes nothing -- one sweep per table and step, over every non-frozen field.  centered=True raises NotImplementedError: it needs
    a third slot (mg), which the dense descriptors (fil_adam_tensor) and the runs entry points do not carry."""
    _NAME = "optim.RMSprop"
    _RULE = FIL_OPT_RMSPROP
    _ENTRY = _MOMOPT_ENTRY

    def __init__(self, params, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, process_group=None,
                 force_exchange=False, decay=0.0):
        momentum = _check_momentum(momentum)
        if centered:
            raise NotImplementedError("optim.RMSprop: centered=True needs a third slot (mg); the dense descriptors (fil_adam_tensor) and "
                                      "the runs entry points carry two")
        if epsilon is None:
            epsilon = 1e-7              # Keras: backend.epsilon()
        learning_rate, decay = _check_rate("RMSprop", learning_rate, decay)
        if not 0.0 <= rho <= 1.0 or not epsilon >= 0.0:
            raise ValueError("RMSprop: rho=%r epsilon=%r (rho in [0, 1], epsilon >= 0)" % (rho, epsilon))
        self._SLOTS = ("rms", "momentum") if momentum > 0.0 else ("rms",)
        super().__init__(params, dict(learning_rate=learning_rate, rho=float(rho), momentum=momentum, epsilon=float(epsilon),
                                      centered=False, **_decay_entry(decay)), process_group, force_exchange)

    def _slot_init(self, group):
        return (0.0,) * len(self._SLOTS)

    def _sweeps(self, field_l2):
        return len(self._SLOTS) == 1 or field_l2 is not None         # momentum == 0: rms decays on every row

    def _hyper(self, group, lr_dev=None, dev=None):
        momentum = _check_momentum(group["momentum"])
        if (momentum > 0.0) != (len(self._SLOTS) == 2):
            raise ValueError("optim.RMSprop: a parameter group's momentum=%r -- whether momentum is 0 is fixed at construction" % momentum)
        return MomoptHyper(_float_rate(group), group["epsilon"], group["rho"], momentum, 0, 0), lr_dev


_ADAOPT_ENTRY = ("fil_adaopt_multi", "fil_embed_adaopt_runs", "fil_embed_adaopt_sweep", "fil_embed_adaopt_merged")


class Adadelta(_Rowwise):
    """tf.keras.optimizers.Adadelta (TF 2.1; ApplyAdadelta / SparseApplyAdadelta, one rule for both): accum_grad = accum_grad rho +
    g^2 (1 - rho); upd = sqrt(accum_var + epsilon) / sqrt(accum_grad + epsilon) g; p -= lr upd; accum_var = accum_var rho + upd^2
    (1 - rho) (include/fil.h O5 has the rounding), with Keras' defaults (learning_rate 1e-3 and epsilon 1e-7, where
    torch.optim.Adadelta has 1.0 and 1e-6).  Slots: `accum_grad` and `accum_var` (zeros).  Runs tables (SparseEmbed(grad_mode="runs"))
    take Keras' per-field semantics in place: the batch's rows, plus every other row of a field with l2(emb_reg) > 0 (g = 2 emb_reg p);
    an untouched row of an unregularised field keeps its bits, its slots' too.  Reads no step: bit-exact.  process_group /
    force_exchange / decay / schedules: as optim.Adam's."""
    _NAME = "optim.Adadelta"
    _RULE = FIL_OPT_ADADELTA
    _ENTRY = _ADAOPT_ENTRY
    _SLOTS = ("accum_grad", "accum_var")

    def __init__(self, params, learning_rate=0.001, rho=0.95, epsilon=1e-7, process_group=None, force_exchange=False, decay=0.0):
        if epsilon is None:
            epsilon = 1e-7              # Keras: backend.epsilon()
        learning_rate, decay = _check_rate("Adadelta", learning_rate, decay)
        if not 0.0 <= rho <= 1.0 or not epsilon >= 0.0:
            raise ValueError("Adadelta: rho=%r epsilon=%r (rho in [0, 1], epsilon >= 0)" % (rho, epsilon))
        super().__init__(params, dict(learning_rate=learning_rate, rho=float(rho), epsilon=float(epsilon), **_decay_entry(decay)),
                         process_group, force_exchange)

    def _slot_init(self, group):
        return 0.0, 0.0

    def _hyper(self, group, lr_dev=None, dev=None):
        return AdaoptHyper(_float_rate(group), group["rho"], 0.0, 0.0, group["epsilon"]), lr_dev


class Adamax(_Rowwise):
    """tf.keras.optimizers.Adamax (TF 2.1; ApplyAdaMax, and adamax.py's Python for IndexedSlices): m = beta_1 m + (1 - beta_1) g;
    v = max(beta_2 v, |g|); p -= c m / (v + epsilon) with c = lr / (1 - beta_1^t), t = iterations + 1 (include/fil.h O5 has the two
    roundings).  Slots: `m` and `v` (zeros).  Row-local, unlike Keras' Adam: runs tables take the batch's rows, plus every other row of
    a field with l2(emb_reg) > 0 (g = 2 emb_reg p); an untouched row of an unregularised field keeps its bits, its slots' too.  c is
    formed on the device in every launch, from the step counter and the step's rate, so schedules, decay= and captured steps work as
    for the other optimizers; beta_1^t is the device's powf: Keras-exact within optim.Adam's bars.  process_group / force_exchange /
    decay / schedules: as optim.Adam's."""
    _NAME = "optim.Adamax"
    _RULE = FIL_OPT_ADAMAX
    _ENTRY = _ADAOPT_ENTRY
    _SLOTS = ("m", "v")

    def __init__(self, params, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, process_group=None, force_exchange=False,
                 decay=0.0):
        if epsilon is None:
            epsilon = 1e-7              # Keras: backend.epsilon()
        learning_rate, decay = _check_rate("Adamax", learning_rate, decay)
        if not 0.0 <= beta_1 < 1.0 or not 0.0 <= beta_2 < 1.0 or not epsilon >= 0.0:
            raise ValueError("Adamax: beta_1=%r beta_2=%r epsilon=%r (betas in [0, 1), epsilon >= 0)" % (beta_1, beta_2, epsilon))
        super().__init__(params, dict(learning_rate=learning_rate, beta_1=float(beta_1), beta_2=float(beta_2), epsilon=float(epsilon),
                                      **_decay_entry(decay)), process_group, force_exchange)

    def _slot_init(self, group):
        return 0.0, 0.0

    def _hyper(self, group, lr_dev=None, dev=None):
        return AdaoptHyper(_float_rate(group), 0.0, group["beta_1"], group["beta_2"], group["epsilon"]), lr_dev


_NADAM_ENTRY = ("fil_nadam_multi", "fil_embed_nadam_runs", "fil_embed_nadam_sweep", "fil_embed_nadam_merged")


class Nadam(_Rowwise):
    """tf.keras.optimizers.Nadam (TF 2.1; keras/optimizer_v2/nadam.py): with t = iterations + 1, mt = beta_1 (1 - 0.5 0.96^(schedule_decay
    t)), mt1 the same at t + 1, and the momentum cache msn = (the product of mt over the steps so far, this one included), msx = msn mt1:
    gp = g / (1 - msn); m = beta_1 m + (1 - beta_1) g; mp = m / (1 - msx); v = beta_2 v + (1 - beta_2) g^2; vp = v / (1 - beta_2^t);
    p -= lr ((1 - mt) gp + mt1 mp) / (sqrt(vp) + epsilon) (include/fil.h O6 has the rounding; the dense and the IndexedSlices form are
    the same bits).  Slots: `m` and `v` (zeros).  `momentum_cache` is the product of the completed steps' mt (1.0 before the first):
    one fp32 word per device beside the step counter, advanced with it by the step's last launch, carried by state_dict() and put back
    to 1.0 by reset_().  Runs tables take Keras' per-field semantics in place, and Keras decays m and v over the whole variable: an
    untouched row of an unregularised field gets m *= beta_1, v *= beta_2 and keeps p, an untouched row of a regularised field takes
    the rule with g = 2 emb_reg p, a frozen field changes nothing -- one sweep per table and step, over every non-frozen field.
    learning_rate is a number: Keras' Nadam refuses a LearningRateSchedule and overwrites `decay` with schedule_decay, so there is no
    decay= here.  beta_1 and schedule_decay are optimizer-wide (the cache has one recurrence); learning_rate, beta_2 and epsilon may
    differ by parameter group.  The powers are the device's powf: Keras-exact within optim.Adam's bars, bit-exact in m and v.
    process_group / force_exchange: as optim.Adam's."""
    _NAME = "optim.Nadam"
    _RULE = FIL_OPT_NADAM
    _ENTRY = _NADAM_ENTRY
    _SLOTS = ("m", "v")

    def __init__(self, params, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004, process_group=None,
                 force_exchange=False):
        if epsilon is None:
            epsilon = 1e-7              # Keras: backend.epsilon()
        if isinstance(learning_rate, schedules.LearningRateSchedule):
            raise ValueError("The Nadam optimizer does not support tf.keras.optimizers.LearningRateSchedules as the learning rate.")
        if not learning_rate >= 0.0:
            raise ValueError("Nadam: learning_rate=%r (>= 0)" % (learning_rate,))
        if not 0.0 <= beta_1 < 1.0 or not 0.0 <= beta_2 < 1.0 or not epsilon >= 0.0 or not schedule_decay >= 0.0:
            raise ValueError("Nadam: beta_1=%r beta_2=%r epsilon=%r schedule_decay=%r (betas in [0, 1); epsilon, schedule_decay >= 0)"
                             % (beta_1, beta_2, epsilon, schedule_decay))
        self._cache = {}        # device -> fp32 [1] momentum cache (Keras' _m_cache), beside the step counter
        super().__init__(params, dict(learning_rate=float(learning_rate), beta_1=float(beta_1), beta_2=float(beta_2),
                                      epsilon=float(epsilon), schedule_decay=float(schedule_decay)), process_group, force_exchange)

    def _cache_word(self, dev):
        c = self._cache.get(dev)
        if c is None:
            c = self._cache[dev] = torch.ones(1, dtype=torch.float32, device=dev)
        return c

    @property
    def momentum_cache(self):
        """The product of the completed steps' momenta (Keras' _m_cache), as a host float (synchronises)."""
        return float(next(iter(self._cache.values()))[0]) if self._cache else 1.0

    def _slot_init(self, group):
        return 0.0, 0.0

    def _sweeps(self, field_l2):
        return True                     # m and v decay on every row

    def _hyper(self, group, lr_dev=None, dev=None):
        if isinstance(group["learning_rate"], schedules.LearningRateSchedule):
            raise ValueError("The Nadam optimizer does not support tf.keras.optimizers.LearningRateSchedules as the learning rate.")
        for k in ("beta_1", "schedule_decay"):
            if group[k] != self.defaults[k]:
                raise ValueError("optim.Nadam: a parameter group's %s=%r -- %s is optimizer-wide (%r): the momentum cache has one "
                                 "recurrence" % (k, group[k], k, self.defaults[k]))
        if dev is None and len(self._cache) == 1:
            dev = next(iter(self._cache))
        cache = self._cache_word(dev) if dev is not None and dev.type == "cuda" else None
        return NadamHyper(group["learning_rate"], group["beta_1"], group["beta_2"], group["epsilon"], group["schedule_decay"], 0,
                          ptr(cache)), None

    def state_dict(self):
        sd = super().state_dict()
        sd["momentum_cache"] = self.momentum_cache
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        cache = float(state_dict.pop("momentum_cache", 1.0))
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for p in g["params"]:
                if p.device.type == "cuda":
                    self._cache_word(p.device)
        for c in self._cache.values():
            c.fill_(cache)

    def reset_(self):
        super().reset_()
        for c in self._cache.values():
            c.fill_(1.0)


def _rule_merged(entry, rule, ids, values, counts, W, cap, offsets, field_l2, table, slot0, slot1, stamp, step, hyper):
    V, K = table.shape
    check(getattr(_lib.load(), entry)(ptr(ids), ptr(values), ptr(counts), int(W), int(cap), K, ptr(offsets), ptr(field_l2),
                                      offsets.numel(), ptr(table), ptr(slot0), ptr(slot1), ptr(stamp), V, ptr(step), int(rule),
                                      ctypes.addressof(hyper), stream_ptr()), entry)


def momopt_merged(rule, ids, values, counts, W, cap, offsets, field_l2, table, slot0, slot1, stamp, step, hyper):
    """fil_embed_momopt_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / slot0 / slot1 [V, K] in place
    (a slot the variant lacks: None); rule FIL_OPT_SGD or FIL_OPT_RMSPROP, hyper an _lib.MomoptHyper."""
    _rule_merged("fil_embed_momopt_merged", rule, ids, values, counts, W, cap, offsets, field_l2, table, slot0, slot1, stamp, step, hyper)


def adaopt_merged(rule, ids, values, counts, W, cap, offsets, field_l2, table, slot0, slot1, stamp, step, hyper):
    """fil_embed_adaopt_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / slot0 / slot1 [V, K] in place;
    rule FIL_OPT_ADADELTA or FIL_OPT_ADAMAX, hyper an _lib.AdaoptHyper."""
    _rule_merged("fil_embed_adaopt_merged", rule, ids, values, counts, W, cap, offsets, field_l2, table, slot0, slot1, stamp, step, hyper)


def nadam_merged(ids, values, counts, W, cap, offsets, field_l2, table, m, v, stamp, step, hyper):
    """fil_embed_nadam_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / m / v [V, K] in place; hyper
    an _lib.NadamHyper (its m_cache the device address of the momentum cache word)."""
    _rule_merged("fil_embed_nadam_merged", FIL_OPT_NADAM, ids, values, counts, W, cap, offsets, field_l2, table, m, v, stamp, step, hyper)


def rowopt_merged(rule, ids, values, counts, W, cap, offsets, field_l2, table, accum, linear, stamp, step, hyper):
    """fil_embed_rowopt_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / accum / linear [V, K] in
    place; rule FIL_OPT_ADAGRAD or FIL_OPT_FTRL, hyper an _lib.RowoptHyper."""
    _rule_merged("fil_embed_rowopt_merged", rule, ids, values, counts, W, cap, offsets, field_l2, table, accum, linear, stamp, step, hyper)


def runs_compact_workspace_bytes(R):
    """Workspace bytes of runs_compact for a record of R entries."""
    return int(_lib.load().fil_embed_runs_compact_workspace_bytes(int(R)))


def runs_compact(rec, K, ids, values, count, cap, workspace):
    """fil_embed_runs_compact on a runs record (the dict SparseEmbed(grad_mode="runs") leaves as table._fil_pending_runs, or any
    dict with g, perm, sorted_ids, R, g_dtype): ids [cap] int64, values [cap*K] fp32, count [1] int64 are written on the device."""
    check(_lib.load().fil_embed_runs_compact(ptr(rec["g"]), ptr(rec["perm"]), ptr(rec["sorted_ids"]), int(rec["R"]), int(K),
                                             int(rec["g_dtype"]), ptr(ids), ptr(values), ptr(count), int(cap), ptr(workspace),
                                             workspace.numel() * workspace.element_size(), stream_ptr()), "fil_embed_runs_compact")


def amsgrad_merged(ids, values, counts, W, cap, offsets, field_l2, table, m, v, vhat, stamp, step, lr=1e-3, beta_1=0.9, beta_2=0.999,
                   epsilon=1e-7):
    """fil_embed_amsgrad_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / m / v / vhat [V, K] in
    place; stamp [V] int32 is required."""
    V, K = table.shape
    check(_lib.load().fil_embed_amsgrad_merged(ptr(ids), ptr(values), ptr(counts), int(W), int(cap), K, ptr(offsets), ptr(field_l2),
                                               offsets.numel(), ptr(table), ptr(m), ptr(v), ptr(vhat), ptr(stamp), V, ptr(step),
                                               *_rate_pair(lr), beta_1, beta_2, epsilon, stream_ptr()), "fil_embed_amsgrad_merged")


def adam_merged(ids, values, counts, W, cap, offsets, field_l2, table, m, v, stamp, step, lr=1e-3, beta_1=0.9, beta_2=0.999,
                epsilon=1e-7, lazy=False):
    """fil_embed_adam_merged on W gathered lists (ids [W*cap], values [W*cap*K], counts [W]); table / m / v [V, K] in place."""
    V, K = table.shape
    check(_lib.load().fil_embed_adam_merged(ptr(ids), ptr(values), ptr(counts), int(W), int(cap), K, ptr(offsets), ptr(field_l2),
                                            offsets.numel(), ptr(table), ptr(m), ptr(v), ptr(stamp), V, ptr(step), lr, beta_1, beta_2,
                                            epsilon, FIL_ADAM_LAZY if lazy else FIL_ADAM_KERAS, stream_ptr()), "fil_embed_adam_merged")
