"""Keras' streaming AUC on the GPU (include/fil.h M1, ml_function_amd.metrics.AUC) against the numpy restatement of TensorFlow 2.1's
AUC (tests/keras_auc_ref.py): counts bit for bit, accumulation with Keras' fp32 state, the six result forms, the layer against the
raw C ABI, HIP-graph capture, a training step that the metric does not perturb, and the data-parallel read."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, losses, metrics, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd.layers.base import collect_regularization_loss
from tests import keras_auc_ref as ref

pytestmark = pytest.mark.gpu

MAX_T = _lib.FIL_CONFUSION_MAX_T
DISTS = {"uniform": ref.uniform_scores, "skewed": ref.skewed_scores}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _specials(thr, rng):
    """Scores that sit on and around the decisions: 0, 1, every stored threshold inside [0, 1], the fp32 neighbours on both sides of a
    sample of thresholds, denormals and -0.0."""
    inside = thr[(thr >= 0) & (thr <= 1)]
    some = inside[rng.permutation(len(inside))[:64]]
    around = np.concatenate([np.nextafter(some, np.float32(2)), np.nextafter(some, np.float32(-1))]).astype(np.float32)
    around = around[(around >= 0) & (around <= 1)]
    fixed = np.asarray([0.0, 1.0, -0.0, 1e-45, 1e-39, 1.1754942e-38, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    return np.concatenate([fixed, inside, around]).astype(np.float32)


def _scores(dist, n, thr, seed):
    rng = np.random.default_rng(seed)
    p = DISTS[dist](rng, n)
    sp = _specials(thr, rng)
    sp = sp[rng.permutation(len(sp))][:min(n, len(sp))]
    p[rng.permutation(n)[:len(sp)]] = sp
    return p, rng


def _labels(kind, rng, p):
    if kind == "binary":
        return (rng.random(len(p)) < np.maximum(p, 0.05)).astype(np.float32)
    return rng.choice(np.asarray([0, 1, 2, -1, 0.5], np.float32), len(p))


def _update(p, y, thr, cm=None, invalid=None):
    T = len(thr)
    cm = torch.zeros(4, T, device="cuda") if cm is None else cm
    invalid = torch.zeros(1, dtype=torch.int64, device="cuda") if invalid is None else invalid
    Fn.confusion_update(p if torch.is_tensor(p) else _dev(p), y if torch.is_tensor(y) else _dev(y), _dev(thr), cm, invalid)
    return cm, invalid


def _want(y, p, thr):
    return np.stack(ref.counts_chunked(y, p, thr, chunk=max(1024, (1 << 25) // len(thr)))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. counts, bit for bit
@pytest.mark.parametrize("T", [2, 3, 200, 201, 1000, MAX_T])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 4096, 4097, 100003])
def test_counts_equal_the_restatement(n, T):
    thr = ref.thresholds(T)
    for dist in DISTS:
        for kind in ("binary", "mixed"):
            p, rng = _scores(dist, n, thr, seed=n * 7 + T)
            y = _labels(kind, rng, p)
            cm, invalid = _update(p, y, thr)
            assert np.array_equal(cm.cpu().numpy(), _want(y, p, thr)), (n, T, dist, kind)
            assert int(invalid) == 0


@pytest.mark.parametrize("dist,kind", [("uniform", "binary"), ("skewed", "mixed")])
@pytest.mark.parametrize("n", [(1 << 20) + 1, 1 << 24])
def test_counts_equal_the_restatement_large(n, dist, kind):
    thr = ref.thresholds(200)
    p, rng = _scores(dist, n, thr, seed=11)
    y = _labels(kind, rng, p)
    cm, invalid = _update(p, y, thr)
    got = cm.cpu().numpy()
    assert int(invalid) == 0
    assert np.array_equal(got, _want(y, p, thr)), (n, dist)
    # the same call from the same state: the same bits (the workspace needs no initialisation and the counts no luck)
    cm2, _ = _update(p, y, thr)
    assert torch.equal(cm, cm2)


@pytest.mark.parametrize("n", [1, 65, 4096, 40000])
def test_one_class_batches(n):
    thr = ref.thresholds(200)
    p, _ = _scores("skewed", n, thr, seed=3)
    for y in (np.ones(n, np.float32), np.zeros(n, np.float32)):
        cm, invalid = _update(p, y, thr)
        assert np.array_equal(cm.cpu().numpy(), _want(y, p, thr)) and int(invalid) == 0
        m = metrics.AUC()
        m.update_state(_dev(y), _dev(p))
        assert m.result_value() == 0.0                                  # div_no_nan: Keras does not raise, neither do we


def test_user_thresholds_unsorted_with_duplicates():
    user = [0.9, 0.1, 0.5, 0.5, 0.5, 0.0, 1.0, 0.25, 1e-40, 0.1]
    m = metrics.AUC(thresholds=user)
    thr = ref.thresholds(user=user)
    assert m.num_thresholds == len(thr) == 12
    for n in (300, 4096, 50000):
        p, rng = _scores("uniform", n, thr, seed=n)
        y = _labels("mixed", rng, p)
        m.reset_states()
        m.update_state(_dev(y), _dev(p))
        assert np.array_equal(m.confusion.cpu().numpy(), _want(y, p, thr)), n
        got = m.result_value()
        assert abs(got - float(ref.result(*_want(y, p, thr), dt=np.float64))) <= 4 * 12 * 2.0 ** -24


@pytest.mark.parametrize("n", [1, 5, 4096, 4099, 70001])
def test_views_that_are_not_16_byte_aligned(n):
    thr = ref.thresholds(200)
    p, rng = _scores("skewed", n + 8, thr, seed=n)
    y = _labels("binary", rng, p)
    P, Y = _dev(p), _dev(y)
    for po, yo in ((1, 3), (1, 1), (2, 0), (0, 3), (3, 2)):
        pv, yv = P[po:po + n], Y[yo:yo + n]
        assert pv.data_ptr() % 16 == 4 * po and yv.data_ptr() % 16 == 4 * yo
        cm, invalid = _update(pv, yv, thr)
        assert np.array_equal(cm.cpu().numpy(), _want(y[yo:yo + n], p[po:po + n], thr)), (n, po, yo)
        assert int(invalid) == 0


@pytest.mark.parametrize("n", [64, 4096, 100003])
def test_scores_outside_the_unit_interval_are_left_out_and_counted(n):
    thr = ref.thresholds(200)
    p, rng = _scores("uniform", n, thr, seed=n)
    y = _labels("binary", rng, p)
    bad_vals = np.asarray([np.nan, np.inf, -np.inf, -1e-45, thr[0], thr[-1], 1.5, -0.25, 7.0, -np.nan], np.float32)
    where = rng.permutation(n)[:min(n // 2, 37)]
    p[where] = bad_vals[np.arange(len(where)) % len(bad_vals)]
    ok = (p >= 0) & (p <= 1)
    assert (~ok).sum() == len(where)
    m = metrics.AUC()
    m.update_state(_dev(y), _dev(p))
    m.update_state(_dev(y[ok]), _dev(p[ok]))                             # a clean batch afterwards does not clear the counter
    want = 2 * _want(y[ok], p[ok], thr)
    assert np.array_equal(m.confusion.cpu().numpy(), want)
    assert int(m.invalid) == len(where)
    float(m.result())                                                    # result() does not check ...
    with pytest.raises(ValueError, match="%d predictions" % len(where)):
        m.result_value()                                                 # ... result_value() does
    m.reset_states()
    assert m.result_value() == 0.0


# ------------------------------------------------------------------------------------------------ 2. accumulation
def test_fifty_updates_equal_the_restatement_on_the_concatenation():
    thr = ref.thresholds(200)
    m = metrics.AUC()
    ys, ps = [], []
    for s in range(50):
        p, rng = _scores("skewed" if s % 2 else "uniform", 4096, thr, seed=100 + s)
        y = _labels("binary", rng, p)
        m.update_state(_dev(y).reshape(64, 64), _dev(p).reshape(64, 64))          # any shape, flattened
        ys.append(y)
        ps.append(p)
    assert np.array_equal(m.confusion.cpu().numpy(), _want(np.concatenate(ys), np.concatenate(ps), thr))
    assert m.true_positives.data_ptr() == m.confusion.data_ptr() and m.false_negatives.data_ptr() == m.confusion[3].data_ptr()
    # labels of another dtype, scores in float64
    m2 = metrics.AUC()
    m2.update_state(torch.tensor(np.concatenate(ys)[:5000] != 0, device="cuda"), _dev(np.concatenate(ps)[:5000], torch.float64))
    assert np.array_equal(m2.confusion.cpu().numpy(), _want(np.concatenate(ys)[:5000], np.concatenate(ps)[:5000], thr))


def test_state_past_2_pow_24_rounds_like_keras_fp32_assign_add():
    """A state preset just under 2^24 follows np.float32 addition call by call -- one fp32 add of the batch's count per entry --
    and not the integer sum."""
    thr = ref.thresholds(200)
    m = metrics.AUC().build("cuda")
    start = np.float32(2 ** 24 - 3000)
    m.confusion.fill_(float(start))
    state = np.full((4, 200), start, np.float32)
    exact = np.full((4, 200), int(start), np.int64)
    for s in range(6):
        p, rng = _scores("uniform", 4097, thr, seed=200 + s)
        y = _labels("binary", rng, p)
        c = np.stack(ref.counts(y, p, thr))
        state = state + c.astype(np.float32)                             # fp32 + fp32 -> fp32, once per call
        exact += c
        m.update_state(_dev(y), _dev(p))
        assert np.array_equal(m.confusion.cpu().numpy(), state), s
    assert (state != exact.astype(np.float64)).any()                     # the quirk was exercised: odd sums past 2^24 were rounded


def test_repeat_from_the_same_state_gives_the_same_bits_and_reset_keeps_pointers():
    thr = ref.thresholds(200)
    m = metrics.AUC().build("cuda")
    ptrs = (m.confusion.data_ptr(), m.invalid.data_ptr())
    for n in (4096, 300000):
        p, rng = _scores("skewed", n, thr, seed=n)
        p[::101] = 2.0
        y = _labels("mixed", rng, p)
        P, Y = _dev(p), _dev(y)
        outs = []
        for _ in range(3):
            m.reset_states()
            m.confusion.fill_(12345.0)
            m.update_state(Y, P)
            outs.append((m.confusion.clone(), int(m.invalid)))
        assert all(torch.equal(o[0], outs[0][0]) and o[1] == outs[0][1] == len(p[::101]) for o in outs)
    m.reset_states()
    assert (m.confusion.data_ptr(), m.invalid.data_ptr()) == ptrs and float(m.confusion.abs().sum()) == 0 and int(m.invalid) == 0
    # checkpoint round trip, in place
    m.update_state(Y, P)
    sd = m.state_dict()
    m2 = metrics.AUC()
    m2.load_state_dict(sd)
    assert torch.equal(m2.confusion, m.confusion) and int(m2.invalid) == int(m.invalid)
    m.reset_states()
    m.load_state_dict(sd)
    assert torch.equal(m2.confusion, m.confusion) and m.confusion.data_ptr() == ptrs[0]


# ------------------------------------------------------------------------------------------------ 3. result
def _result_states():
    thr = ref.thresholds(200)
    states = {}
    for dist in DISTS:
        p, rng = _scores(dist, 65536, thr, seed=5)
        y = (rng.random(len(p)) < p).astype(np.float32)
        states[dist] = np.stack(ref.counts(y, p, thr)).astype(np.float32)
    p, _ = _scores("skewed", 5000, thr, seed=6)
    states["positives only"] = np.stack(ref.counts(np.ones(5000), p, thr)).astype(np.float32)
    states["negatives only"] = np.stack(ref.counts(np.zeros(5000), p, thr)).astype(np.float32)
    states["empty"] = np.zeros((4, 200), np.float32)
    return states


def test_result_all_six_forms_against_the_float64_restatement(capsys):
    """Bars.  The five Riemann forms sum at most T - 1 non-negative terms to at most 1, each term a product of quantities with at
    most three roundings: 4 T 2^-24 absolute (4.8e-5 at T = 200).  PR-interpolation has a log and a cancellation and no such bound:
    the kernel is allowed the larger of 4 T 2^-24 and 8x the distance of the fp32 numpy restatement from the fp64 one on the same
    counts.  Measured on these counts on an MI355X (fp32 numpy restatement vs fp64 ; kernel vs fp64), PR-interpolation:
        uniform 8.07e-08 ; 2.11e-08     skewed 4.24e-09 ; 1.91e-08     positives only 1.19e-07 ; 0     negatives only, empty 0 ; 0
    so the derived 4.8e-5 is the bar that applies.  Largest kernel distance over the five Riemann forms: 8.92e-08."""
    bar = 4 * 200 * 2.0 ** -24
    lines = []
    for name, st in _result_states().items():
        cm = _dev(st)
        for curve in ref.CURVES:
            for method in ref.METHODS:
                want = float(ref.result(*st, curve, method, np.float64))
                ref32 = abs(float(ref.result(*st, curve, method, np.float32)) - want)
                got = float(Fn.auc_result(cm, curve, method))
                lines.append("%-15s %-3s %-13s want %.9f  numpy-fp32 off %.2e  kernel off %.2e" % (name, curve, method, want, ref32, abs(got - want)))
                allowed = max(bar, 8 * ref32) if (curve, method) == ("PR", "interpolation") else bar
                with capsys.disabled():
                    print(lines[-1])
                assert abs(got - want) <= allowed, lines[-1]
                if name == "empty" or (curve == "ROC" and name.endswith("only")) or name == "negatives only":
                    assert got == 0.0 and want == 0.0, lines[-1]
                m = metrics.AUC(curve=curve, summation_method=method).build("cuda")
                m.confusion.copy_(cm)
                assert float(m.result()) == got == m.result_value()


def test_default_auc_sits_between_minoring_and_majoring_of_the_exact_auc():
    thr = ref.thresholds(200)
    p, rng = _scores("skewed", 65536, thr, seed=9)
    y = (rng.random(len(p)) < p).astype(np.float32)
    vals = {}
    for method in ref.METHODS:
        m = metrics.AUC(summation_method=method)
        m.update_state(_dev(y), _dev(p))
        vals[method] = m.result_value()
    exact = metrics.auc(_dev(y), _dev(p))
    slack = 4 * 200 * 2.0 ** -24
    assert vals["minoring"] - slack <= exact <= vals["majoring"] + slack
    assert vals["minoring"] - slack <= vals["interpolation"] <= vals["majoring"] + slack


# ------------------------------------------------------------------------------------------------ 4. layer against the raw C ABI
def test_layer_equals_the_raw_entry_points():
    lib = _lib.load()
    T = 200
    thr = ref.thresholds(T)
    m = metrics.AUC(curve="PR")
    cm = torch.zeros(4, T, device="cuda")
    invalid = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(1, device="cuda")
    thr_d = _dev(thr)
    for n in (4096, 16384, 16385, 250001):
        p, rng = _scores("skewed", n, thr, seed=n)
        p[5] = -3.0
        y = _labels("mixed", rng, p)
        P, Y = _dev(p), _dev(y)
        m.update_state(Y, P)
        need = lib.fil_confusion_workspace_bytes(n, T)
        assert (need == 0) == (n <= _lib.FIL_CONFUSION_ONE_LAUNCH_N)
        ws = torch.full((max(need, 1),), 0xAB, dtype=torch.uint8, device="cuda")      # garbage: needs no initialisation
        rc = lib.fil_confusion_update(P.data_ptr(), Y.data_ptr(), n, thr_d.data_ptr(), T, cm.data_ptr(), invalid.data_ptr(),
                                      ws.data_ptr() if need else None, need, ctypes.c_void_p(_lib.stream_ptr()))
        assert rc == 0, lib.fil_last_error()
    assert lib.fil_auc_result(cm.data_ptr(), T, 1, 0, out.data_ptr(), ctypes.c_void_p(_lib.stream_ptr())) == 0
    torch.cuda.synchronize()
    assert torch.equal(cm, m.confusion) and int(invalid) == int(m.invalid) == 4
    assert float(out) == float(m.result())


# ------------------------------------------------------------------------------------------------ 5. capture
def _batches(k, n, seed):
    thr = ref.thresholds(200)
    out = []
    for s in range(k):
        p, rng = _scores("skewed" if s % 2 else "uniform", n, thr, seed=seed + s)
        out.append((_labels("binary", rng, p), p))
    return out


def test_update_and_result_inside_a_hip_graph():
    thr = ref.thresholds(200)
    batches = _batches(20, 4096, 300)
    m = metrics.AUC().build("cuda")
    Y, P = _dev(batches[0][0]), _dev(batches[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update_state(Y, P)
        m.result()
    torch.cuda.current_stream().wait_stream(side)
    m.reset_states()
    ptrs = (m.confusion.data_ptr(), m.invalid.data_ptr())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.update_state(Y, P)
        res = m.result()
    m.reset_states()                                                     # (the capture itself ran nothing; be explicit anyway)
    for k, (y, p) in enumerate(batches, 1):
        Y.copy_(_dev(y))
        P.copy_(_dev(p))
        g.replay()
        assert m.result().data_ptr() == res.data_ptr()                   # the same static tensor (this eager call rewrites the same value)
        if k in (1, 7, 20):
            c = ref.counts(np.concatenate([b[0] for b in batches[:k]]), np.concatenate([b[1] for b in batches[:k]]), thr)
            assert np.array_equal(m.confusion.cpu().numpy(), np.stack(c).astype(np.float32)), k
            assert abs(float(res) - float(ref.result(*c, dt=np.float64))) <= 4 * 200 * 2.0 ** -24
    assert (m.confusion.data_ptr(), m.invalid.data_ptr()) == ptrs and int(m.invalid) == 0


def test_update_and_result_through_capture_step():
    thr = ref.thresholds(200)
    batches = _batches(20, 4096, 400)
    m = metrics.AUC(curve="PR", summation_method="minoring").build("cuda")

    def step(y, p):
        m.update_state(y, p)
        return m.result()

    captured = capture.capture_step(step, _dev(batches[0][0]), _dev(batches[0][1]), restore=m.reset_states)
    first = captured(_dev(batches[0][0]), _dev(batches[0][1]))
    for y, p in batches[1:]:
        out = captured(_dev(y), _dev(p))
        assert out is first or out.data_ptr() == first.data_ptr()
    c = ref.counts(np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches]), thr)
    assert np.array_equal(m.confusion.cpu().numpy(), np.stack(c).astype(np.float32))     # the warm-up runs were undone by restore
    assert abs(float(out) - float(ref.result(*c, "PR", "minoring", np.float64))) <= 4 * 200 * 2.0 ** -24
    assert m.result_value() == float(out)


# ------------------------------------------------------------------------------------------------ 6. the metric does not perturb training
def test_metric_inside_the_captured_training_step_changes_no_parameter_bit():
    vocab = [7, 11, 5, 13, 3, 17]
    B, K = 256, 8
    rng = np.random.default_rng(5)
    batches = []
    for s in range(10):
        r = np.random.default_rng(40 + s)
        dense = torch.tensor(r.random((B, 3)), dtype=torch.float32, device="cuda")
        idx = torch.tensor(np.stack([r.integers(0, v, B) for v in vocab], 1), device="cuda")
        batches.append((dense, idx, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def run(with_metric):
        torch.manual_seed(7)
        info = [i._replace(emb_reg=1e-3) for i in models.make_sparse_info(vocab, embed_dim=K)]
        fi = models.FeatureInput(sparseInfo=info, useLinear=True, useAddLinear=True, useFlattenLinear=True, tableGrad="runs")
        model = models.CTRModel(fi, models.XDeepFM(conv_size=[16, 12], hidden_units=[32, 16])).cuda()
        model(batches[0][0], batches[0][1])
        opt = optim.Adam(model.parameters())
        m = metrics.AUC().build("cuda") if with_metric else None

        def step(dense, idx, y):
            opt.zero_grad()
            p = model(dense, idx)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)
            loss.backward()
            opt.step()
            if m is not None:
                m.update_state(y, p)
                return p.detach(), m.result()
            return p.detach(), loss.detach()

        init = {k: v.clone() for k, v in model.state_dict().items()}

        def restore():
            with torch.no_grad():
                for k, v in model.state_dict().items():
                    v.copy_(init[k])
            opt.reset_()
            if m is not None:
                m.reset_states()

        captured = capture.capture_step(step, *batches[0], restore=restore)
        ps = []
        for bt in batches:
            p, _ = captured(*bt)
            ps.append(p.clone())
        torch.cuda.synchronize()
        slots = [v.clone() for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]
        return model, slots, ps, m

    model_a, slots_a, ps_a, m = run(True)
    model_b, slots_b, ps_b, _ = run(False)
    for (n, a), (_, b) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert torch.equal(a, b), n
    assert len(slots_a) == len(slots_b) > 0 and all(torch.equal(a, b) for a, b in zip(slots_a, slots_b))
    assert all(torch.equal(a, b) for a, b in zip(ps_a, ps_b))
    thr = ref.thresholds(200)
    c = ref.counts(np.concatenate([bt[2].cpu().numpy() for bt in batches]), np.concatenate([p.cpu().numpy() for p in ps_a]), thr)
    assert np.array_equal(m.confusion.cpu().numpy(), np.stack(c).astype(np.float32))
    assert abs(m.result_value() - float(ref.result(*c, dt=np.float64))) <= 4 * 200 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 7. data parallel
def test_result_through_a_one_rank_rccl_group():
    import torch.distributed as dist
    import bench
    device = torch.device("cuda", 0)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with bench.stdout_to_stderr():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=device)
    try:
        thr = ref.thresholds(200)
        p, rng = _scores("skewed", 30000, thr, seed=1)
        y = _labels("binary", rng, p)
        m = metrics.AUC()
        m.update_state(_dev(y), _dev(p))
        before = (m.confusion.clone(), m.invalid.clone())
        for _ in range(2):                                               # mid-epoch, repeatedly
            got = m.result(process_group=dist.group.WORLD)
            assert got.dim() == 0 and got.data_ptr() != m.result().data_ptr()
            assert float(got) == float(m.result()) == m.result_value(process_group=dist.group.WORLD)
        assert torch.equal(m.confusion, before[0]) and torch.equal(m.invalid, before[1])
        m.update_state(_dev(y[:10]), _dev(p[:10] + 2.0))
        with pytest.raises(ValueError, match="10 predictions"):
            m.result_value(process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (a one-GPU box runs the one-rank group above)")
def test_two_ranks_read_the_whole_auc():
    """tests/dp_metrics_worker.py at world size 2: each rank updates with its shard, both read the AUC of the whole."""
    from tests.test_dp_gpu import _run_ranks
    r = _run_ranks([os.path.join(ROOT, "tests", "dp_metrics_worker.py")], 2)
    assert r.returncode == 0 and "DP_METRICS_OK 2" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
