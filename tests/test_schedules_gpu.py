"""Keras' learning-rate schedules and the legacy `decay` on the GPU (include/fil.h O3, ml_function_amd/schedules.py, optim.py):
fil_lr_schedule_eval against the numpy restatement (tests/keras_schedules_ref.py), whole optimizer trajectories against the by-value
route with the host setting the reference rate before every step, dense Adam against the float64 ApplyAdam fed the reference rate,
HIP-graph capture (alone and with metrics.AUC in the same graph), resume from a state_dict, and no effect when unused."""
import collections
import copy
import ctypes
import gc

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, metrics, models, optim, schedules
from ml_function_amd._lib import check, ptr, stream_ptr
from ml_function_amd.layers import SparseEmbed
from ml_function_amd.layers.base import collect_regularization_loss
from tests import keras_schedules_ref as ref

pytestmark = pytest.mark.gpu


def c64(t):
    return t.detach().cpu().double().numpy()


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------------------------------------------- 1. the rate itself
DS = 1000
BOUNDS = [5, 1000, 2 ** 24]
# 0 and 1; decay_steps and each boundary with their neighbours; where Keras' float32 cast of the step starts to round; near 2^31
STEPS = sorted({0, 1, DS - 1, DS, DS + 1, 2 * DS - 1, 2 * DS, 2 * DS + 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 7}
               | {b + d for b in BOUNDS for d in (-1, 0, 1)})
EXACT = [schedules.InverseTimeDecay(0.01, DS, 0.5), schedules.InverseTimeDecay(0.01, DS, 0.5, staircase=True),
         schedules.PiecewiseConstantDecay(BOUNDS, [1e-2, 3e-3, 1e-3, 1e-4]),
         schedules.PolynomialDecay(0.01, DS), schedules.PolynomialDecay(0.01, DS, cycle=True), 0.01]
POW = [schedules.ExponentialDecay(0.01, DS, 0.96), schedules.ExponentialDecay(0.01, DS, 0.96, staircase=True),
       schedules.PolynomialDecay(0.01, DS, 1e-4, power=2.5), schedules.PolynomialDecay(0.01, DS, 1e-4, power=2.5, cycle=True),
       schedules.PolynomialDecay(0.01, DS, 1e-4, power=0.5), schedules.PolynomialDecay(0.01, DS, 1e-4, power=0.5, cycle=True)]
DECAYS = [0.0, 1e-3]


def _device_rates(sched, decay, steps):
    """fil_lr_schedule_eval with the counter set to each step in turn: float32 [len(steps)]."""
    d = sched.descriptor(decay) if isinstance(sched, schedules.LearningRateSchedule) else schedules.constant_descriptor(sched, decay)
    lib = _lib.load()
    check(lib.fil_lr_schedule_check(ctypes.addressof(d)), "fil_lr_schedule_check")
    desc = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((len(steps),), -1.0, dtype=torch.float32, device="cuda")
    for i, s in enumerate(steps):
        counter.fill_(s)
        check(lib.fil_lr_schedule_eval(ptr(desc), ptr(counter), ptr(out[i:]), stream_ptr()), "fil_lr_schedule_eval")
    return out.cpu().numpy()


def _id(s):
    if not isinstance(s, schedules.LearningRateSchedule):
        return "float"
    c = s.get_config()
    return type(s).__name__ + "".join("_%s" % k for k in ("staircase", "cycle") if c.get(k)) + ("_p%g" % c["power"] if "power" in c else "")


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("sched", EXACT, ids=_id)
def test_rate_without_a_power_is_bit_equal_to_the_restatement(sched, decay):
    """Inverse time, piecewise, polynomial with power 1 and the legacy decay are built from + - * / floor ceil min and comparisons:
    every step of STEPS bit for bit."""
    if not isinstance(sched, schedules.LearningRateSchedule) and decay == 0.0:
        decay = 0.5                                     # (a float without decay never reaches the device: a second decay instead)
    got = _device_rates(sched, decay, STEPS)
    for s, g in zip(STEPS, got):
        want = ref.rate(sched, s, decay)
        assert np.float32(g).tobytes() == want.tobytes(), (s, float(g), float(want))


def test_rate_with_a_power_is_within_one_ulp_of_the_restatement():
    """The pow kinds against the same formula with the power taken in float64 and rounded once to float32, on both sides.  The bar
    is 1 float32 ulp, derived, not measured: a float64 pow is within 1 float64 ulp of the exact power, and a single rounding of two
    such values to float32 can differ only across a rounding boundary, by one ulp.  The number of cases that are not bit-equal is
    printed (a finding, kept in profiles/r12_optim_schedule_bench.txt); no case is left out."""
    worst, off, total = 0, 0, 0
    for sched in POW:
        for decay in DECAYS:
            got = _device_rates(sched, decay, STEPS)
            for s, g in zip(STEPS, got):
                u = ref.ulps(g, ref.rate(sched, s, decay))
                total += 1
                off += u != 0
                worst = max(worst, u)
                if u > 1:
                    print("pow case beyond 1 ulp:", _id(sched), decay, s, float(g), float(ref.rate(sched, s, decay)), u)
    print("pow kinds: %d of %d cases not bit-equal to the float64-pow restatement, worst %d ulp" % (off, total, worst))
    assert worst <= 1


# ---------------------------------------------------------------------------------------------------- 2. trajectories
# (the table sizes and batches of tests/test_optim_gpu.py / test_optim_rowwise_gpu.py: their helpers, copied)
VOCAB = [50, 200, 30, 1000, 7, 64]
L2 = {0: 1e-2, 3: 3e-3}              # two regularised fields
FROZEN = 2                           # one frozen field
K, BT = 16, 512
DENSE = [(3,), (1023,), (65537,), (5,)]         # the last one never has a gradient
CHANGING = schedules.ExponentialDecay(1e-2, 5, 0.7)     # a different rate at every step
CHANGING_DECAY = 0.05


def _table_layer(out_dtype):
    info = models.make_sparse_info(VOCAB, embed_dim=K)
    info = [i._replace(emb_reg=L2.get(f, 0.0), is_trainable=(f != FROZEN)) for f, i in enumerate(info)]
    torch.manual_seed(3)
    emb = SparseEmbed(info, packed=True, check_ids=False, grad_mode="runs", out_dtype=out_dtype)
    return emb


def _table_batches(steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        idx = np.stack([np.minimum(rng.zipf(1.2, BT) - 1, v - 1) for v in VOCAB], 1)          # heavy duplication
        bad = rng.random(idx.shape) < 0.02                                                   # out-of-range ids (dropped)
        idx[bad] = np.array(VOCAB)[np.nonzero(bad)[1]] + 3
        idx[rng.random(idx.shape) < 0.01] = -1
        g = rng.standard_normal((BT, len(VOCAB), K)) * 1e-3
        out.append((torch.tensor(idx, device="cuda"), g))
    return out


def _trajectory(cls, kw, device_rate, batches, dense_grads, resume=None):
    """`len(batches)` steps of cls(**kw) on the runs table and the dense tensors.  device_rate: the optimizer holds the schedule and
    the decay; else it is built with a float and the host sets param_group["learning_rate"] to the reference's float32 rate before
    every step (the by-value route).  Returns every parameter and slot, cloned."""
    emb = _table_layer(None)
    emb(batches[0][0])                                                   # build
    rng = np.random.default_rng(0)
    dense = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s) * 0.5, dtype=torch.float32, device="cuda")) for s in DENSE]
    params = [emb.embeddings] + dense
    if device_rate:
        opt = cls(params, learning_rate=CHANGING, decay=CHANGING_DECAY, **kw)
    else:
        opt = cls(params, learning_rate=1.0, **kw)
    for t, ((idx, g), dg) in enumerate(zip(batches, dense_grads)):
        if resume is not None and t == resume:                           # a fresh optimizer picks the run up from a state_dict
            sd = copy.deepcopy(opt.state_dict())
            del opt                                                      # (a deferred table leaves its optimizer when that one goes)
            gc.collect()
            opt = cls(params, learning_rate=0.5, **kw)
            opt.load_state_dict(sd)
        opt.zero_grad()
        block = emb(idx)
        block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
        for p, x in zip(dense[:-1], dg):
            p.grad = x.clone()
        if not device_rate:
            opt.param_groups[0]["learning_rate"] = float(ref.rate(CHANGING, t, CHANGING_DECAY))
        opt.step()
    if hasattr(opt, "flush"):
        opt.flush()
    assert opt.iterations == len(batches)
    out = [p.detach().clone() for p in params]
    for p in params:
        out += [opt.state[p][k].clone() for k in opt._SLOTS if k in opt.state[p]]
    return out


def _dense_grads(steps, seed):
    rng = np.random.default_rng(seed)
    return [[torch.tensor(rng.standard_normal(s) * 10.0 ** rng.integers(-4, 0), dtype=torch.float32, device="cuda") for s in DENSE[:-1]]
            for _ in range(steps)]


FTRL_KW = dict(l1_regularization_strength=1e-3, l2_regularization_strength=1e-3, l2_shrinkage_regularization_strength=1e-3)
TRAJ = [(optim.Adam, {}), (optim.Adam, dict(lazy_tables=True)), (optim.Adam, dict(sweep_period=1)), (optim.Adam, dict(sweep_period=4)),
        (optim.Adam, dict(force_exchange=True)), (optim.Adam, dict(force_exchange=True, sweep_period=4)),
        (optim.Adagrad, {}), (optim.Adagrad, dict(force_exchange=True)),
        (optim.Ftrl, dict(FTRL_KW)), (optim.Ftrl, dict(FTRL_KW, force_exchange=True))]
TRAJ_IDS = ["adam", "adam_lazy", "adam_deferred1", "adam_deferred4", "adam_exchange", "adam_exchange_deferred4", "adagrad",
            "adagrad_exchange", "ftrl", "ftrl_exchange"]


@pytest.mark.parametrize("cls,kw", TRAJ, ids=TRAJ_IDS)
def test_schedule_trajectory_is_bitwise_the_by_value_route_fed_the_reference_rate(cls, kw):
    """12 steps with a rate that changes at every step (a schedule and the decay together), on dense tensors and a runs table with
    l2 on two fields: the device-rate route against the existing by-value route, which the optimizer tests hold to the float64
    oracle -- so the dense launch, the runs update, the sweep, the merged update and the deferred ring all took the rate the
    restatement gives, to the bit."""
    batches, dg = _table_batches(12, seed=21), _dense_grads(12, seed=22)
    rates = [ref.rate(CHANGING, t, CHANGING_DECAY) for t in range(12)]
    assert len({r.tobytes() for r in rates}) == 12
    a = _trajectory(cls, kw, True, batches, dg)
    b = _trajectory(cls, kw, False, batches, dg)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    fresh = _table_layer(None)
    fresh(batches[0][0])
    assert not torch.equal(a[0], fresh.embeddings.detach())             # (the table did move)


# ---------------------------------------------------------------------------------------------------- 3. against float64
LR0, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))
SIZES = [(1,), (3,), (4,), (1023,), (4096,), (65537,), (1521, 128)]


def keras_adam64(p, g, m, v, t, lr):
    """TensorFlow's ApplyAdam (Keras 'adam', TF 2.1) in float64 on float32 hyper-parameters; t = the 1-based step, lr = the step's
    float32 rate (tests/test_optim_gpu.py's, with the rate an argument).  Returns (p, m, v)."""
    alpha = lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    m = m + (g - m) * (1 - B1)
    v = v + (g * g - v) * (1 - B2)
    return p - m * alpha / (np.sqrt(v) + EPS), m, v


def test_adam_multi_with_schedule_and_decay_matches_keras_apply_adam():
    """The dense case of test_adam_multi_matches_keras_apply_adam with a schedule and the decay together, against ApplyAdam in
    float64 fed the reference rate of each step (the rate uses iterations = t - 1, the bias correction t): that test's bars."""
    sched, decay = schedules.ExponentialDecay(1e-3, 2, 0.8), 0.1
    rng = np.random.default_rng(0)
    ps = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s) * 0.5, dtype=torch.float32, device="cuda")) for s in SIZES]
    none = 2                                                    # this one never has a gradient
    opt = optim.Adam(ps, learning_rate=sched, decay=decay)
    traj = [(c64(p), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    start = [c64(p) for p in ps]
    for t in range(1, 6):
        lr = float(ref.rate(sched, t - 1, decay))
        assert float(opt.current_learning_rate()) == lr
        grads = [None if i == none else rng.standard_normal(s) * 10.0 ** rng.integers(-6, 0) for i, s in enumerate(SIZES)]
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float32, device="cuda")
        before = [(c64(p), c64(opt.state[p]["m"]) if "m" in opt.state[p] else np.zeros(p.shape),
                   c64(opt.state[p]["v"]) if "v" in opt.state[p] else np.zeros(p.shape)) for p in ps]
        opt.step()
        assert opt.iterations == t
        for i, (p, g) in enumerate(zip(ps, grads)):
            if g is None:
                continue
            g32 = c64(p.grad)
            want, wm, wv = keras_adam64(*before[i][:1], g32, before[i][1], before[i][2], t, lr)
            assert nrel(c64(p) - before[i][0], want - before[i][0]) < 1e-4, (SIZES[i], t)
            assert nrel(c64(opt.state[p]["m"]), wm) < 1e-6 and nrel(c64(opt.state[p]["v"]), wv) < 1e-5, (SIZES[i], t)
            traj[i] = keras_adam64(traj[i][0], g32, traj[i][1], traj[i][2], t, lr)
            assert nrel(c64(p), traj[i][0]) < 1e-6, (SIZES[i], t)
    assert np.array_equal(c64(ps[none]), start[none]) and "m" not in opt.state[ps[none]]


# ---------------------------------------------------------------------------------------------------- 4. capture
def _xdeepfm(vocab, K_, table_grad):
    info = [i._replace(emb_reg=1e-3) for i in models.make_sparse_info(vocab, embed_dim=K_)]
    fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad=table_grad)
    return fi, models.CTRModel(fi, models.XDeepFM(conv_size=[16, 12], hidden_units=[32, 16])).cuda()


def _inputs(B, n_dense, vocab, seed=0):
    rng = np.random.default_rng(seed)
    dense = torch.tensor(rng.random((B, n_dense)), dtype=torch.float32, device="cuda")
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device="cuda")
    return dense, idx


def _snapshot(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        out += [opt.state[p][k].clone() for k in opt._SLOTS if k in opt.state.get(p, {})]
    return out


CAPTURE = [(optim.Adam, {}), (optim.Adam, dict(sweep_period=4)), (optim.Adagrad, {}), (optim.Ftrl, dict(FTRL_KW))]


@pytest.mark.parametrize("with_auc", [False, True], ids=["alone", "with_auc"])
@pytest.mark.parametrize("cls,kw", CAPTURE, ids=["adam", "adam_deferred4", "adagrad", "ftrl"])
def test_captured_step_with_schedule_replays_bitwise_like_eager(cls, kw, with_auc):
    """An XDeepFM step with a schedule and the decay, captured after warm-up and reset_(), replayed 10 times: after EVERY replay
    the parameters, slots and tables are bitwise the eager run's, and current_learning_rate() is the reference's rate of the next
    step -- a different one at every replay.  with_auc: metrics.AUC updated inside the same graph."""
    vocab = [7, 11, 5, 13, 3, 17]
    B, K_ = 256, 8
    sched, decay = schedules.PolynomialDecay(5e-3, 8, 1e-4, power=2.0, cycle=True), 0.02
    batches = []
    rng = np.random.default_rng(5)
    for s in range(3):
        d, i = _inputs(B, 3, vocab, seed=40 + s)
        batches.append((d, i, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        torch.manual_seed(7)
        fi, model = _xdeepfm(vocab, K_, "runs")
        model(batches[0][0], batches[0][1])
        opt = cls(model.parameters(), learning_rate=sched, decay=decay, **kw)
        auc = metrics.AUC().build("cuda") if with_auc else None

        def step(dense, idx, y):
            opt.zero_grad()
            p = model(dense, idx)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model, skip_tables="sweep_period" in kw)
            loss.backward()
            opt.step()
            if auc is not None:
                auc.update_state(y, p.detach())
            return loss.detach()
        return model, opt, auc, step

    def current(model, opt):
        if hasattr(opt, "flush"):
            opt.flush()
        return _snapshot(model, opt)

    model_e, opt_e, auc_e, step_e = make()
    eager = []
    for s in range(10):
        step_e(*batches[s % 3])
        eager.append((current(model_e, opt_e), None if auc_e is None else auc_e.confusion.clone()))
    model_c, opt_c, auc_c, step_c = make()
    init = {k: v.clone() for k, v in model_c.state_dict().items()}

    def restore():
        with torch.no_grad():
            for k, v in model_c.state_dict().items():
                v.copy_(init[k])
        opt_c.reset_()
        if auc_c is not None:
            auc_c.reset_states()

    captured = capture.capture_step(step_c, *batches[0], restore=restore)
    torch.cuda.synchronize()
    assert opt_c.iterations == 0
    seen = set()
    for s in range(10):
        assert float(opt_c.current_learning_rate()) == float(ref.rate(sched, s, decay))
        seen.add(float(opt_c.current_learning_rate()))
        captured(*batches[s % 3])
        torch.cuda.synchronize()
        assert opt_c.iterations == s + 1
        got = current(model_c, opt_c)
        assert len(got) == len(eager[s][0])
        bad = [i for i, (a, b) in enumerate(zip(got, eager[s][0])) if not torch.equal(a, b)]
        assert not bad, (s, bad)
        if with_auc:
            assert torch.equal(auc_c.confusion, eager[s][1]), s
    assert len(seen) == 10


# ---------------------------------------------------------------------------------------------------- 5. resume
@pytest.mark.parametrize("cls,kw", [(optim.Adam, {}), (optim.Adam, dict(sweep_period=4)), (optim.Adagrad, {}), (optim.Ftrl, dict(FTRL_KW))],
                         ids=["adam", "adam_deferred4", "adagrad", "ftrl"])
def test_resume_from_state_dict_continues_at_the_right_rate(cls, kw):
    """state_dict() after 5 steps loaded into a fresh optimizer (built with another, float rate), then 5 more steps: bitwise the 10
    uninterrupted steps -- the schedule, the decay and iterations all travelled."""
    batches, dg = _table_batches(10, seed=31), _dense_grads(10, seed=32)
    whole = _trajectory(cls, kw, True, batches, dg)
    resumed = _trajectory(cls, kw, True, batches, dg, resume=5)
    assert all(torch.equal(x, y) for x, y in zip(whole, resumed))


def test_reset_puts_the_rate_back_to_step_zero():
    p = torch.nn.Parameter(torch.ones(8, device="cuda"))
    opt = optim.Adam([p], learning_rate=CHANGING, decay=CHANGING_DECAY)
    for _ in range(3):
        p.grad = torch.ones_like(p)
        opt.step()
    assert float(opt.current_learning_rate()) == float(ref.rate(CHANGING, 3, CHANGING_DECAY))
    opt.reset_()
    assert float(opt.current_learning_rate()) == float(ref.rate(CHANGING, 0, CHANGING_DECAY))


# ---------------------------------------------------------------------------------------------------- 6. no effect when unused
class _Counting:
    """The library handle with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("cls", [optim.Adam, optim.Adagrad, optim.Ftrl], ids=["adam", "adagrad", "ftrl"])
def test_float_rate_without_decay_makes_no_schedule_call_and_no_descriptor(cls, monkeypatch):
    counting = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counting)
    batches, dg = _table_batches(2, seed=41), _dense_grads(2, seed=42)

    def run(**kw):
        emb = _table_layer(None)
        emb(batches[0][0])
        dense = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in DENSE[:-1]]
        opt = cls([emb.embeddings] + dense, **kw)
        for (idx, g), d in zip(batches, dg):
            opt.zero_grad()
            block = emb(idx)
            block.backward(torch.tensor(g, dtype=block.dtype, device="cuda"))
            for p, x in zip(dense, d):
                p.grad = x.clone()
            opt.step()
        return opt

    counting.calls.clear()
    opt = run(learning_rate=1e-3)
    assert counting.calls["fil_lr_schedule_eval"] == 0 and counting.calls["fil_lr_schedule_check"] == 0
    assert not [n for n in counting.calls if n.endswith("_lrdev")] and opt._rates == {}
    assert sum(counting.calls.values()) > 0                              # (the wrapper does see the step's calls)
    assert float(opt.current_learning_rate()) == float(np.float32(1e-3)) and opt._rates == {}
    counting.calls.clear()
    opt = run(learning_rate=1e-3, decay=0.5)                             # the decay alone takes the device route
    assert counting.calls["fil_lr_schedule_eval"] == 2 and counting.calls["fil_lr_schedule_check"] == 1 and len(opt._rates) == 1
    by_value = {"fil_adam_multi", "fil_embed_adam_runs", "fil_embed_adam_sweep", "fil_rowopt_multi", "fil_embed_rowopt_runs",
                "fil_embed_rowopt_sweep"}
    assert not by_value & set(counting.calls), counting.calls
    assert float(opt.current_learning_rate()) == float(ref.rate(1e-3, 2, 0.5))
