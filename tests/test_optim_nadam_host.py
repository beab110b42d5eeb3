"""Host-only checks of the Keras Nadam (include/fil.h O6, ml_function_amd/optim.py): the new entry points in the header, the binding
and the library; their argument validation through ctypes; the Python surface that needs no GPU (Keras' names, defaults and errors);
and the numpy restatement of the rule (tests/keras_nadam_ref.py) against hand-computed two-step values, against Keras' row semantics
on a tiny table, in its tail, and against its own float64 twin on the inputs and at the bars of the GPU tests."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from tests import keras_nadam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fil_nadam_multi", "fil_embed_nadam_runs", "fil_embed_nadam_sweep", "fil_embed_nadam_merged")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_nadam_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
        # the O6 entry points take the argument lists of their O4 counterparts, and have no _lrdev twins
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("nadam", "momopt")]
        assert name + "_lrdev" not in _lib.SIGNATURES and name + "_lrdev" not in _lib.header_symbols()
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.FIL_OPT_NADAM == 7
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"enum\s*\{\s*FIL_OPT_NADAM\s*=\s*7\s*\}", header)
    # the O6 section follows the O5 prototypes and precedes the metrics
    assert (header.index(" * O5 ") < header.index("int fil_embed_adaopt_merged_lrdev(") < header.index(" * O6 ")
            < header.index("fil_nadam_multi(") < header.index(" * M1 "))


def test_nadam_hyper_field_order_and_size():
    assert ctypes.sizeof(_lib.NadamHyper) == 32
    assert [f for f, _ in _lib.NadamHyper._fields_] == ["lr", "beta_1", "beta_2", "epsilon", "schedule_decay", "reserved", "m_cache"]
    assert [t for _, t in _lib.NadamHyper._fields_] == [ctypes.c_float] * 5 + [ctypes.c_int32, ctypes.c_void_p]
    assert _lib.NadamHyper.m_cache.offset == 24 and _lib.NadamHyper.reserved.offset == 20
    header = open(_lib.HEADER_PATH).read()
    body = header[:header.index("} fil_nadam_hyper;")]
    body = body[body.rindex("typedef struct {"):]
    assert re.findall(r"^\s*(float\*?|int32_t) (\w+);", body, flags=re.M) == [
        ("float", "lr"), ("float", "beta_1"), ("float", "beta_2"), ("float", "epsilon"), ("float", "schedule_decay"),
        ("int32_t", "reserved"), ("float*", "m_cache")]
    assert "fil_nadam_hyper;      /* 32 bytes */" in header


def test_abi_version_and_the_other_hypers_are_unchanged(lib):
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216
    assert ctypes.sizeof(_lib.RowoptHyper) == 24 and ctypes.sizeof(_lib.MomoptHyper) == 24 and ctypes.sizeof(_lib.AdaoptHyper) == 20
    assert (_lib.FIL_OPT_ADAGRAD, _lib.FIL_OPT_FTRL, _lib.FIL_OPT_SGD, _lib.FIL_OPT_RMSPROP, _lib.FIL_OPT_ADADELTA,
            _lib.FIL_OPT_ADAMAX) == (1, 2, 3, 4, 5, 6)


def test_nadam_entry_points_validate(lib):
    from tests import host_calls_optim_nadam
    assert host_calls_optim_nadam.run(lib) >= 250


def test_nadam_keras_names_defaults_and_errors():
    from ml_function_amd import optim, schedules
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Nadam([p])
    assert isinstance(opt, torch.optim.Optimizer) and isinstance(opt, optim._Rowwise)
    assert opt.defaults == dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004)
    assert opt.iterations == 0 and opt.momentum_cache == 1.0 and opt.force_exchange is False and opt.process_group is None
    assert opt._SLOTS == ("m", "v") and opt._RULE == 7 and opt._slot_init(opt.param_groups[0]) == (0.0, 0.0)
    assert opt._sweeps(None) is True and opt._sweeps(object()) is True          # every table is swept at every step
    assert optim.Nadam([p], epsilon=None).defaults["epsilon"] == 1e-7            # Keras: backend.epsilon()
    optim.Nadam([p], beta_1=0.0, beta_2=0.0, schedule_decay=0.0, learning_rate=0.0, epsilon=0.0)
    for kw in (dict(beta_1=-0.1), dict(beta_1=1.0), dict(beta_2=1.0), dict(beta_2=-1.0), dict(epsilon=-1.0), dict(learning_rate=-1.0),
               dict(schedule_decay=-0.004), dict(beta_1=float("nan")), dict(learning_rate=float("nan"))):
        with pytest.raises(ValueError):
            optim.Nadam([p], **kw)
    with pytest.raises(ValueError) as e:
        optim.Nadam([p], learning_rate=schedules.ExponentialDecay(1e-2, decay_steps=2, decay_rate=0.5))
    assert str(e.value) == "The Nadam optimizer does not support tf.keras.optimizers.LearningRateSchedules as the learning rate."
    for kw in (dict(decay=0.5), dict(decay=0.0), dict(lazy_tables=True), dict(sweep_period=4)):
        with pytest.raises(TypeError):
            optim.Nadam([p], **kw)
    with pytest.raises(TypeError):
        optim.Nadam([p], force_exchange=1)
    with pytest.raises(TypeError):
        optim.Nadam([p], process_group="world")
    h, lr_dev = opt._hyper(opt.param_groups[0])
    assert lr_dev is None and isinstance(h, _lib.NadamHyper)
    assert (h.lr, h.beta_1, h.beta_2, h.epsilon, h.schedule_decay, h.reserved) == (F(1e-3), F(0.9), F(0.999), F(1e-7), F(0.004), 0)
    assert h.m_cache is None                        # no GPU parameter: no cache word (the library refuses a NULL one)
    assert "Nadam" in optim.__doc__ and "Nadam is not offered" not in optim.__doc__


def test_nadam_beta_1_and_schedule_decay_are_optimizer_wide():
    from ml_function_amd import optim
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = optim.Nadam([dict(params=[p]), dict(params=[q], learning_rate=0.5, beta_2=0.99, epsilon=1e-3)], beta_1=0.8)
    h = opt._hyper(opt.param_groups[1])[0]
    assert (h.lr, h.beta_1, h.beta_2, h.epsilon) == (F(0.5), F(0.8), F(0.99), F(1e-3))
    for k, x in (("beta_1", 0.8), ("schedule_decay", 0.01)):
        bad = optim.Nadam([dict(params=[p]), dict(params=[q], **{k: x})])
        bad._hyper(bad.param_groups[0])
        with pytest.raises(ValueError, match=k):
            bad._hyper(bad.param_groups[1])


def test_the_other_optimizers_ignore_the_device_argument():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    for cls in (optim.Adam, optim.Adagrad, optim.Ftrl, optim.SGD, optim.RMSprop, optim.Adadelta, optim.Adamax):
        opt = cls([p])
        a, b = opt._hyper(opt.param_groups[0]), opt._hyper(opt.param_groups[0], None, torch.device("cpu"))
        if cls is optim.Adam:
            assert a == b
        else:
            assert bytes(a[0]) == bytes(b[0]) and a[1] is b[1] is None


def test_nadam_refuses_cpu_parameters():
    from ml_function_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.FilError, match="GPU"):
        optim.Nadam([p]).step()


# ---- the restatement against two steps computed by hand: p0 = 1, g = 0.5 at both steps; lr 0.1, beta_1 = beta_2 = 0.5, epsilon 0,
# schedule_decay 0, so that 0.96^0 = 1 and mt = mt1 = 0.5 (1 - 0.5) = 0.25 at every step:
#   step 1: cache 1   -> msn 1/4, msx 1/16; gp = 0.5 / (3/4); m = 1/4; mp = (1/4) / (15/16); v = 1/8; vp = (1/8) / (1/2), sqrt 1/2
#   step 2: cache 1/4 -> msn 1/16, msx 1/64; gp = 0.5 / (15/16); m = 3/8; mp = (3/8) / (63/64); v = 3/16; vp = (3/16) / (3/4), sqrt 1/2
MB1 = 0.75 * (0.5 / 0.75) + 0.25 * (0.25 / (15 / 16))
MB2 = 0.75 * (0.5 / (15 / 16)) + 0.25 * (0.375 / (63 / 64))
HAND = [(1 - 0.1 * MB1 / 0.5, 0.25, 0.125, 0.25), (1 - 0.1 * MB1 / 0.5 - 0.1 * MB2 / 0.5, 0.375, 0.1875, 0.0625)]     # p, m, v, cache
RTOL = 2e-6         # float32(0.1) against the decimal, plus a dozen roundings


def test_restatement_matches_hand_computed_two_steps():
    assert abs(MB1 - 0.5666667) < 1e-6 and abs(MB2 - 0.4952381) < 1e-6 and abs(HAND[1][0] - 0.7876190) < 1e-6        # the decimals
    h = ref.hyper(lr=0.1, beta_1=0.5, beta_2=0.5, epsilon=0.0, schedule_decay=0.0)
    p, g, m, v = np.ones(5, F), np.full(5, 0.5, F), np.zeros(5, F), np.zeros(5, F)
    s64 = (1.0, 0.0, 0.0)
    cache, cache64 = F(1), 1.0
    for it, want in enumerate(HAND):
        c, c64 = ref.coefs(h, it, cache), ref.coefs64(h, it, cache64)
        assert c["mt"] == c["mt1"] == F(0.25) and c["vden"] == F(1 - 0.5 ** (it + 1))
        p, m, v = ref.elem(h, c, p, m, v, g)
        s64 = ref.elem64(h, c64, *s64, 0.5)
        cache, cache64 = c["msn"], c64["msn"]
        for got, got64, w in zip((p, m, v, cache), s64 + (cache64,), want):
            np.testing.assert_allclose(got, w, rtol=RTOL, atol=0)
            np.testing.assert_allclose(got64, w, rtol=RTOL, atol=0)
    # dense_step is elem on g + 2 l2 p
    a = ref.dense_step(h, c, p, m, v, g, l2=0.25)
    b = ref.elem(h, c, p, m, v, g + F(0.5) * p)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_restatement_schedule_and_cache():
    """Keras' defaults: mt(1) = 0.9 (1 - 0.5 0.96^0.004), and the cache is the running product of mt."""
    h = ref.hyper()
    c = ref.coefs(h, 0, F(1))
    np.testing.assert_allclose(c["mt"], 0.9 * (1 - 0.5 * 0.96 ** 0.004), rtol=1e-6)
    np.testing.assert_allclose(c["mt1"], 0.9 * (1 - 0.5 * 0.96 ** 0.008), rtol=1e-6)
    assert c["msn"] == c["mt"] and c["msx"] == F(c["mt"] * c["mt1"]) and c["mt1"] > c["mt"]
    np.testing.assert_allclose(c["vden"], 1e-3, rtol=1e-4)
    cache, want = F(1), 1.0
    for it in range(5):
        c = ref.coefs(h, it, cache)
        cache = c["msn"]
        want *= 0.9 * (1 - 0.5 * 0.96 ** (0.004 * (it + 1)))
    np.testing.assert_allclose(cache, want, rtol=1e-6)
    np.testing.assert_allclose(ref.coefs64(h, 4, want / ref.coefs64(h, 4, 1.0)["mt"])["msn"], want, rtol=1e-12)


def test_restatement_tail_is_free_of_the_powers():
    """At it = 200 000 with cache 0: 0.96^800 is far below half an ulp of 1, 0.999^200001 underflows, and a zero cache stays zero --
    whatever the last bits of the power are, the coefficients are mt == mt1 == b1 and omsn == omsx == vden == 1 exactly."""
    h = ref.hyper(lr=1e-2)
    for pw in (ref.powf, lambda a, b: np.nextafter(np.nextafter(ref.powf(a, b), F(np.inf)), F(np.inf)),
               lambda a, b: np.nextafter(ref.powf(a, b), F(-np.inf))):
        for it in (200000, 200001, 200002):
            c = ref.coefs(h, it, F(0), pw)
            assert c["mt"] == c["mt1"] == h["b1"] and c["omsn"] == c["omsx"] == c["vden"] == F(1) and c["msn"] == c["msx"] == F(0)
            assert c["omm"] == F(1) - h["b1"]
    assert float(ref.powf(0.96, F(0.004) * F(200001))) < 2.0 ** -40 and float(ref.powf(0.999, 200001)) == 0.0


def test_restatement_moves_the_rows_keras_moves():
    """A table of three fields of 3 rows: regularised, plain, frozen; one touched row in each (a real record never holds a frozen row:
    the restatement ignores it)."""
    V, K = 9, 4
    rng = np.random.default_rng(1)
    p = rng.standard_normal((V, K)).astype(F)
    m = rng.standard_normal((V, K)).astype(F)
    v = np.abs(rng.standard_normal((V, K))).astype(F)
    row_l2 = np.repeat(np.array([1e-2, 0, 0], F), 3)
    frozen = np.repeat(np.array([False, False, True]), 3)
    touched = np.zeros(V, bool)
    touched[[1, 4, 7]] = True
    G = rng.standard_normal((V, K)).astype(F)
    h = ref.hyper(lr=1e-2)
    c = ref.coefs(h, 1, F(0.45))
    (p1, m1, v1), moved, decayed = ref.table_step(h, c, p, m, v, G, touched, row_l2, frozen)
    assert moved.tolist() == [True] * 3 + [False, True, False] + [False] * 3
    assert decayed.tolist() == [False] * 3 + [True, False, True] + [False] * 3
    assert (p1[moved] != p[moved]).all()
    # decayed rows: m b1, v b2, p's bits kept
    assert np.array_equal(p1[decayed], p[decayed])
    assert np.array_equal(m1[decayed], m[decayed] * h["b1"]) and np.array_equal(v1[decayed], v[decayed] * h["b2"])
    assert (m1[decayed] != m[decayed]).all() and (v1[decayed] != v[decayed]).all()
    # the frozen field: nothing changes
    for a, b in ((p1, p), (m1, m), (v1, v)):
        assert np.array_equal(a[frozen], b[frozen])
    # a touched row of the plain field: the rule on the run sum alone; of the regularised one: run sum + 2 l2 p
    assert all(np.array_equal(x[4], y) for x, y in zip((p1, m1, v1), ref.elem(h, c, p[4], m[4], v[4], G[4])))
    assert all(np.array_equal(x[1], y) for x, y in zip((p1, m1, v1), ref.elem(h, c, p[1], m[1], v[1], G[1] + (F(2) * F(1e-2)) * p[1])))
    # an untouched row of the regularised field: the rule on 2 l2 p
    assert all(np.array_equal(x[0], y) for x, y in zip((p1, m1, v1), ref.elem(h, c, p[0], m[0], v[0], (F(2) * F(1e-2)) * p[0])))


@pytest.mark.parametrize("sd", [0.004, 0.5], ids=["sd0.004", "sd0.5"])
@pytest.mark.parametrize("ulps", [0, 2], ids=["powf", "powf+2ulp"])
def test_restatement_passes_the_gpu_bars_against_its_float64_twin(ulps, sd):
    """The GPU tests' dense inputs (12 steps from iterations 0, lr 1e-2, tensors of 1, 4095 and 4097 elements), the fp32 restatement in
    place of the device: every step from the fp32 state against the float64 twin (which carries its own float64 cache) is inside the
    GPU tests' bars -- also with every power pushed 2 ulp up, twice the error a 1-ulp device powf may have, and at the GPU tests'
    second schedule_decay.  The look-ahead momentum taken at the step itself (mt1 = mt) is outside them at schedule_decay 0.5."""
    def pw(a, b):
        x = ref.powf(a, b)
        for _ in range(ulps):
            x = np.nextafter(x, F(np.inf))
        return x

    h = ref.hyper(lr=ref.DENSE_LR, schedule_decay=sd)
    rng, ps, signs = ref.dense_inputs(0)
    state = [(p, np.zeros_like(p), np.zeros_like(p)) for p in ps]
    cache, cache64 = F(1), 1.0
    worst = dict.fromkeys(ref.BARS, 0.0)
    if sd == 0.5:
        c, g = ref.coefs(h, 0, cache), ref.dense_grads(np.random.default_rng(1), signs)[2]
        wrong = dict(c, mt1=c["mt"], msx=F(c["msn"] * c["mt"]), omsx=F(F(1) - F(c["msn"] * c["mt"])))
        assert not ref.within_bars(ref.step_errors(h, ref.coefs64(h, 0, 1.0), ref.elem(h, wrong, *state[2], g), state[2], g))
    for it in range(12):
        c, c64 = ref.coefs(h, it, cache, pw), ref.coefs64(h, it, cache64)
        grads = ref.dense_grads(rng, signs)
        for i, g in enumerate(grads):
            new = ref.elem(h, c, *state[i], g)
            e = ref.step_errors(h, c64, new, state[i], g)
            assert ref.within_bars(e), (it, len(g), e)
            worst = {k: max(worst[k], e[k]) for k in worst}
            state[i] = new
        cache, cache64 = c["msn"], c64["msn"]
    print("restatement (+%d ulp) against float64 over 12 steps: %s" % (ulps, worst))
    assert all(1.0 <= np.abs(p).min() and np.abs(p).max() < 1.95 for p in ps)


def test_train_ctr_offers_nadam():
    src = open(os.path.join(ROOT, "examples", "train_ctr.py")).read()
    for word in ('"keras-nadam"', '"--schedule-decay"', "optim.Nadam("):
        assert word in src, word
