"""The Neural Turing Machine memory read / write over a sequence on the GPU (include/fil.h N4 fil_ntm_*, functional.ntm_memory,
layers.NTMMemoryLayer, models.MIMN) against the fp64 restatement of tests/ntm_ref.py.

Error measure: norm-relative per tensor against the fp64 reference.  Bar per tensor: max(1e-5, 4 E32), E32 = the error of the fp32
torch restatement of the same graph on the same inputs, computed here on the CPU (ntm_ref.bars).  The measured errors are printed.
Every shape is (B, T, H, m, D)."""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, capture, layers, losses, models, optim
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from tests import guarded
from tests import ntm_ref as ref
from tests.seq_common import behaviour_inputs, behaviour_model, bits, dev, dev_mask, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("h",) + ref.PARAMS
ids_of = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def case_of(shape, seed=0, mask="ragged", grads="both", scale=1.0, zero_row=False):
    return ref.make_case(*shape, seed, mask=mask, grads=grads, scale=scale, zero_row=zero_row)


def run_op(case, wanted=NAMES):
    """functional.ntm_memory forward + backward on the case -> dict of float64 numpy arrays (rs or last, MT and the gradients asked
    for).  A case with g_last runs return_sequences=False; an output without an upstream gradient gets none (NULL in the backward)."""
    t = {k: dev(case[k]).requires_grad_(k in wanted) for k in NAMES}
    seq = case.get("g_last") is None
    out, MT = Fn.ntm_memory(t["h"], dev_mask(case), t["Wp"], t["bp"], t["M0"], return_sequences=seq)
    g_out = case["g_rs"] if seq else case["g_last"]
    pairs = [(o, dev(g)) for o, g in ((out, g_out), (MT, case.get("g_M"))) if g is not None]
    if any(v.requires_grad for v in t.values()):
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()
    D = lambda v: v.detach().cpu().double().numpy()
    res = {"rs" if seq else "last": D(out), "MT": D(MT)}
    for k, v in t.items():
        res["d" + k] = None if v.grad is None else D(v.grad)
    return res


def check_parity(got, case, keys=None, label=""):
    fwd, bwd, e32 = ref.reference(case)
    got = {k: v for k, v in got.items() if v is not None and (keys is None or k in keys)}
    if "last" in got:
        got = dict(got)
        last = got.pop("last")
        e_last = ref.norm_rel(last, fwd["rs"][:, -1])
        print("%s last %.2e" % (label, e_last))
        assert e_last <= max(1e-5, 4 * e32["rs"])
    err, bar = ref.errors(got, fwd, bwd), ref.bars(e32)
    print("%s %s  " % (label, case["shape"]) + "  ".join("%s %.2e (E32 %.2e, bar %.2e)" % (k, err[k], e32[k], bar[k]) for k in err))
    for k in err:
        assert np.isfinite(got[k]).all(), k
        assert err[k] <= bar[k], (k, err[k], bar[k])
    return err


# ---------------------------------------------------------------------------------------------------- 1. parity
PARITY_SHAPES = [(1, 1, 4, 1, 4),           # the minimum
                 (3, 5, 8, 2, 4),
                 (5, 7, 16, 4, 16),         # the benchmark's widths
                 (9, 13, 32, 8, 32),
                 (3, 6, 64, 16, 64),        # the menu's corner
                 (2, 3, 4, 16, 64),         # narrow controller, the widest memory
                 (2, 3, 64, 1, 4),          # wide controller, one narrow slot: more pieces of h_t than lanes of a sample
                 (4, 6, 12, 3, 20)]         # H / 4, m and D / 4 odd


@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=ids_of)
def test_parity_with_the_fp64_reference(shape):
    case = case_of(shape, mask="ragged" if shape[1] > 1 else "prefix")          # (a single step is live)
    check_parity(run_op(case), case)


def test_parity_at_saturated_activations():
    """h and Wp times 8: tanh and sigmoid sit at their ends, the betas grow, the softmaxes peak.  Against the case's own E32 bars."""
    case = case_of((5, 7, 16, 4, 16), scale=8.0)
    check_parity(run_op(case), case, label="x8")


def test_last_read_only():
    case = case_of((5, 9, 8, 3, 12), grads="last+M")
    check_parity(run_op(case), case, label="last+M")


@pytest.mark.parametrize("grads", ["M", "rs", "last"])
def test_one_upstream_gradient_alone(grads):
    case = case_of((5, 9, 8, 3, 12), grads=grads)
    check_parity(run_op(case), case, label=grads)


# ---------------------------------------------------------------------------------------------------- 2. batch, tile and grid edges
EDGE = (3, 8, 2, 4)            # T, H, m, D


def run_raw(case, subset=ref.GRADS):
    """The two entry points called directly: every output inside a sentinel-guarded allocation, the workspace guarded behind its
    bytes, `saved` NaN-filled before the forward (masked steps are never written and never used)."""
    lib = _lib.load()
    B, T, H, m, D = case["shape"]
    t = {k: (None if case.get(k) is None else dev(case[k])) for k in NAMES + ("g_rs", "g_last", "g_M")}
    mask = dev_mask(case)
    shapes = dict(rs=(B, T, D), MT=(B, m, D), dh=(B, T, H), dWp=(H, 4 * D + 2), dbp=(4 * D + 2,), dM0=(m, D))
    bufs = {k: guarded.GuardedOutput(shapes[k], np.uint32, k) for k in ["rs", "MT"] + list(subset)}
    nsv = lib.fil_ntm_saved_bytes(B, T, H, m, D)
    assert nsv >= B * T * (m * D + 4 * D + 6 + 5 * m) * 4
    saved = guarded.GuardedOutput((nsv // 4,), np.uint32, "saved")
    check(lib.fil_ntm_fwd(ptr(t["h"]), ptr(mask), ptr(t["Wp"]), ptr(t["bp"]), ptr(t["M0"]), bufs["rs"].ptr, None, bufs["MT"].ptr, saved.ptr,
                          B, T, H, m, D, stream_ptr()), "fil_ntm_fwd")
    nws = lib.fil_ntm_bwd_workspace_bytes(B, T, H, m, D)
    ws = guarded.workspace(nws, fill=guarded.WS_NAN_FILL)
    out = lambda k: bufs[k].ptr if k in bufs else None
    params = any(k in bufs for k in ("dWp", "dbp", "dM0"))
    check(lib.fil_ntm_bwd(ptr(t["h"]), ptr(mask), ptr(t["Wp"]), saved.ptr, ptr(t["g_rs"]), ptr(t["g_last"]), ptr(t["g_M"]), out("dh"), out("dWp"),
                          out("dbp"), out("dM0"), ptr(ws) if params else None, nws if params else 0, B, T, H, m, D, stream_ptr()), "fil_ntm_bwd")
    torch.cuda.synchronize()
    guarded.assert_workspace_guard(ws, nws, "fil_ntm_bwd", fill=guarded.WS_NAN_FILL)
    saved.read("saved")
    return {k: guarded.words_f32(b.read(k)).astype(np.float64) for k, b in bufs.items()}


@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_tile_edges_with_guard_words(which):
    """T = 3, H = 8, m = 2, D = 4.  tile - 1 (a partial tile) and tile: one workgroup, one partial; tile + 1: two, the second with one
    sample.  Every output and `saved` sit between guard words, the workspace has guard bytes behind it."""
    tile = Fn.ntm_plan(1, *EDGE)["tile"]
    B = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    plan = Fn.ntm_plan(B, *EDGE)
    assert plan["tile"] == tile and plan["partials"] == (2 if which == "tile+1" else 1)
    case = case_of((B,) + EDGE)
    check_parity(run_raw(case), case, label=which)


def test_past_the_grid_cap_a_workgroup_walks_a_second_tile():
    """H = 4, m = 1, D = 4: one lane per sample, so the tile stops at 256 samples and B = cap * 256 + 1 leaves one workgroup a second
    tile of one sample.  T = 2 keeps the fp64 reference cheap."""
    T, H, m, D = 2, 4, 1, 4
    cap = Fn.ntm_plan(1, T, H, m, D)["cap"]
    B = cap * 256 + 1
    plan = Fn.ntm_plan(B, T, H, m, D)
    assert plan["tile"] == 256 and plan["grid"] == cap and plan["partials"] == cap
    case = case_of((B, T, H, m, D), mask=None)
    check_parity(run_op(case), case, label="cap*tile+1")


def test_empty_batch_is_a_no_op():
    h = torch.empty(0, 3, 8, device="cuda", requires_grad=True)
    w = [torch.randn(s, device="cuda", requires_grad=True) for s in ((8, 18), (18,), (2, 4))]
    rs, MT = Fn.ntm_memory(h, None, *w)
    assert rs.shape == (0, 3, 4) and MT.shape == (0, 2, 4)
    last, MT = Fn.ntm_memory(h, None, *w, return_sequences=False)
    assert last.shape == (0, 4)
    (last.sum() + MT.sum()).backward()
    assert h.grad.shape == (0, 3, 8) and all(not p.grad.any() for p in w)


@pytest.mark.parametrize("subset", [("dh",), ("dWp", "dbp", "dM0"), ("dM0",), ("dh", "dbp")], ids=["dh", "params", "dM0", "dh+dbp"])
def test_null_output_subsets_have_the_full_backwards_bits(subset):
    case = case_of((5,) + EDGE)
    full = run_raw(case)
    part = run_raw(case, subset=subset)
    assert set(part) == {"rs", "MT"} | set(subset)
    same_bits(part, full, subset)
    with pytest.raises(_lib.FilError):              # nothing is left to compute: FIL_ERR_ARG
        run_raw(case, subset=())


# ---------------------------------------------------------------------------------------------------- 3. exact properties
PROP = (6, 10, 8, 3, 12)


def test_no_mask_is_the_all_ones_mask_bit_for_bit():
    case = case_of(PROP, seed=2, mask=None)
    same_bits(run_op(case), run_op(dict(case, mask=np.ones(PROP[:2], np.uint8))))


def test_masked_steps_carry_the_read_and_get_no_gradient():
    B, T = PROP[:2]
    m = np.ones((B, T), np.uint8)
    m[:, :2] = 0           # leading padding
    m[:, 5] = 0
    m[1, 7:] = 0           # trailing padding
    m[4] = 0               # an all-masked sample
    case = ref.make_case(*PROP, 2, mask=m)
    got = run_op(case)
    rs = got["rs"]
    assert not rs[:, :2].any() and np.array_equal(bits(rs[:, 5]), bits(rs[:, 4])) and rs[0, 2].any()
    for t in range(7, T):
        assert np.array_equal(bits(rs[1, t]), bits(rs[1, 6]))
    assert not rs[4].any() and not got["dh"][4].any()
    assert np.array_equal(bits(got["MT"][4]), bits(case["M0"]))            # the all-masked sample keeps M0 bit for bit
    assert not got["dh"][m == 0].any() and got["dh"][m != 0].any()
    check_parity(got, case, label="masked")


def test_masked_inputs_are_never_used():
    case = case_of(PROP, seed=2)
    live = case["mask"].astype(bool)
    clean, dirty = run_op(case), run_op(dict(case, h=np.where(live[:, :, None], case["h"], np.nan)))
    for k, v in dirty.items():
        assert np.isfinite(v).all(), k
    same_bits(clean, dirty)


def test_one_slot_reads_the_previous_row_and_writes_erase_then_add():
    """m = 1: wr = ww = 1 exactly, so r_t is the previous memory row bit for bit and M_t = M (1 - e) + a."""
    case = case_of((4, 5, 8, 1, 8), seed=1, mask=None)
    got = run_op(case)
    fwd = ref.forward(case)
    assert np.array_equal(bits(got["rs"][:, 0]), bits(np.broadcast_to(case["M0"][0], (4, 8))))       # the first read is M0's row
    assert ref.norm_rel(got["rs"], fwd["rs"]) < 1e-5 and ref.norm_rel(got["MT"], fwd["MT"]) < 1e-5
    one = run_op(dict(case, shape=(4, 1, 8, 1, 8), h=case["h"][:, :1], g_rs=case["g_rs"][:, :1]))
    p = case["h"][:, 0] @ case["Wp"] + case["bp"]
    e, a = 1 / (1 + np.exp(-p[:, 16:24])), np.tanh(p[:, 24:32])
    assert np.abs(one["MT"][:, 0] - (case["M0"][0] * (1 - e) + a)).max() < 1e-6


def test_identical_rows_stay_identical_bit_for_bit():
    """Every row of M0 the same: every slot's sums run in the same order, so the weights are 1 / m and the rows of M_T and of dM0 hold
    the same bits across the slots."""
    base = case_of((5, 7, 16, 4, 16), seed=3)
    M0 = np.tile(base["M0"][:1], (4, 1))
    got = run_op(dict(base, M0=M0, g_M=np.tile(base["g_M"][:, :1], (1, 4, 1))))
    for i in range(1, 4):
        assert np.array_equal(bits(got["MT"][:, i]), bits(got["MT"][:, 0])), i
        assert np.array_equal(bits(got["dM0"][i]), bits(got["dM0"][0])), i
    check_parity(got, dict(base, M0=M0, g_M=np.tile(base["g_M"][:, :1], (1, 4, 1))), label="identical rows")


def test_repeats_are_bit_identical():
    case = case_of((300, 20, 16, 4, 16))
    first, second = run_op(case), run_op(case)
    same_bits(first, second)
    check_parity(first, case)


def test_a_samples_bits_do_not_depend_on_its_place_or_on_the_batch():
    case = case_of((37, 6, 8, 3, 12), seed=4)
    full = run_op(case)
    pick = lambda c, idx: dict(c, shape=(len(idx),) + c["shape"][1:], **{k: c[k][idx] for k in ("h", "mask", "g_rs", "g_M")})
    alone = run_op(pick(case, [20]))
    moved = run_op(pick(case, [5, 20, 36, 0]))
    for k in ("rs", "MT", "dh"):
        assert np.array_equal(bits(alone[k][0]), bits(full[k][20])), k
        assert np.array_equal(bits(moved[k][1]), bits(full[k][20])), k


def test_needs_input_grad_is_honoured():
    case = case_of((9, 6, 8, 3, 12))
    full = run_op(case)
    for wanted in (("h",), tuple(ref.PARAMS), ("M0",), ("h", "bp")):
        got = run_op(case, wanted=wanted)
        for k in NAMES:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["rs"]), bits(full["rs"])) and np.array_equal(bits(got["MT"]), bits(full["MT"]))


# ---------------------------------------------------------------------------------------------------- 4. layer and model
LAYER_NAMES = dict(Wp="read_write_kernel", bp="read_write_bias", M0="initial_memory")


def _run_layer(layer, case, dtype=torch.float32):
    h = dev(case["h"]).to(dtype).requires_grad_()
    mask = None if case.get("mask") is None else dev(case["mask"], torch.uint8).bool()
    with torch.no_grad():
        layer(h, mask=mask)        # lazy build
        for k, name in LAYER_NAMES.items():
            getattr(layer, name).copy_(dev(case[k]))
    layer.zero_grad()
    out, MT = layer(h, mask=mask)
    B, T, H, m, D = case["shape"]
    assert out.dtype == torch.float32 and out.shape == (B, T, D) and MT.shape == (B, m, D)
    torch.autograd.backward([out, MT], [dev(case["g_rs"]), dev(case["g_M"])])
    torch.cuda.synchronize()
    Dn = lambda v: v.detach().cpu().double().numpy()
    res = dict(rs=Dn(out), MT=Dn(MT), dh=Dn(h.grad))
    for k, name in LAYER_NAMES.items():
        res["d" + k] = Dn(getattr(layer, name).grad)
    return res


@pytest.mark.parametrize("shape", [(3, 5, 68, 2, 8), (3, 5, 8, 2, 6), (3, 5, 8, 17, 8)], ids=["H=68", "D=6", "m=17"])
def test_layer_outside_the_menu_takes_the_composed_path(shape):
    case = case_of(shape, seed=9)
    layer = layers.NTMMemoryLayer(shape[3], shape[4], return_sequences=True)
    got = _run_layer(layer, case)
    assert not layer.fits_kernel_menu(dev(case["h"]))
    with pytest.raises(_lib.FilError):              # the op itself does not fall back
        run_op(case)
    check_parity(got, case, label="composed")


def test_layer_inside_the_menu_is_the_op():
    case = case_of((9, 6, 8, 3, 12))
    layer = layers.NTMMemoryLayer(3, 12, return_sequences=True)
    got = _run_layer(layer, case)
    assert layer.fits_kernel_menu(dev(case["h"]))
    same_bits(got, run_op(case))


def test_layer_computes_a_half_precision_input_in_fp32():
    case = case_of((9, 6, 8, 3, 12), seed=6)
    case16 = dict(case, h=torch.tensor(case["h"], dtype=torch.float32).to(torch.bfloat16).double().numpy())
    layer = layers.NTMMemoryLayer(3, 12, return_sequences=True)
    half = _run_layer(layer, case16, dtype=torch.bfloat16)          # asserts an fp32 output; the input gradient comes back in bf16
    check_parity(half, case16, keys=("rs", "MT", "dWp", "dbp", "dM0"), label="bf16 in")


def _mimn_model(vocab, T, K, seed, **kw):
    return behaviour_model(lambda: models.MIMN(hidden_units=[32, 16], **kw), vocab, T, K, seed)


@pytest.mark.parametrize("kw", [dict(), dict(memory_slots=3, memory_dim=12)], ids=["default", "m=3,D=12"])
def test_mimn_against_the_model_with_the_composed_path_forced(kw, monkeypatch):
    """3 fields, one history of T = 6, B = 5.  The same weights with the memory on the composed path (ntm_memory_graph: fp32 torch
    ops): the output and every parameter gradient agree within 1e-5, the floor of the bars max(1e-5, 4 E32) (no fp64 model is built
    here, so the term that could only widen the bar is left out)."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    _, idx, hist = behaviour_inputs(B, vocab, T, seed=1)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], device="cuda")
    model = _mimn_model(vocab, T, K, 3, **kw)

    def grads():
        model.zero_grad()
        p = model(None, idx, hist)[:, 0]
        torch.nn.functional.binary_cross_entropy(p.clamp(1e-6, 1 - 1e-6), y).backward()
        torch.cuda.synchronize()
        return dict(out=p.detach().double().cpu().numpy(), **{n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None})

    fused = grads()
    beh = model.body.behaviors[0]
    assert beh.memory.fits_kernel_menu(torch.empty(B, T, K)) and ("query_kernel" in dict(beh.named_parameters())) == bool(kw)
    monkeypatch.setattr(layers.NTMMemoryLayer, "fits_kernel_menu", lambda self, h: False)
    comp = grads()
    monkeypatch.undo()
    assert set(fused) == set(comp)
    for name in ("memory.read_write_kernel", "memory.read_write_bias", "memory.initial_memory", "controller.recurrent_kernel", "read_beta"):
        assert "body.behaviors.0." + name in fused, name
    for k in sorted(fused):
        direct = ref.norm_rel(fused[k], comp[k])
        print("MIMN %-45s fused vs composed %.2e   bar 1.00e-05" % (k, direct))
        assert direct <= 1e-5, k
    assert np.abs(fused["body.behaviors.0.memory.initial_memory"]).max() > 0


def test_mimn_trains_under_captured_adam_and_replays_the_eager_bits():
    """The loss falls over 20 captured optim.Adam steps on one batch, and three captured steps on three batches leave every
    parameter with the bits of three eager steps."""
    vocab, T, K, B = [12, 5, 7], 6, 8, 5
    rng = np.random.default_rng(5)
    batches = []
    for s in range(3):
        _, idx, hist = behaviour_inputs(B, vocab, T, seed=40 + s)
        batches.append((idx, hist, torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device="cuda")))

    def make():
        model = _mimn_model(vocab, T, K, 7)
        model(None, batches[0][0], batches[0][1])
        opt = optim.Adam(model.parameters(), learning_rate=1e-2)

        def step(idx, hist, y):
            opt.zero_grad()
            p = model(None, idx, hist)[:, 0]
            loss = losses.binary_crossentropy(p, y, eps=1e-6)
            loss.backward()
            opt.step()
            return loss.detach()
        return model, opt, step

    model_e, _, step_e = make()
    for bt in batches:
        step_e(*bt)
    model_c, opt_c, step_c = make()
    init = {k: v.clone() for k, v in model_c.state_dict().items()}

    def restore():
        with torch.no_grad():
            for k, v in model_c.state_dict().items():
                v.copy_(init[k])
        opt_c.reset_()

    captured = capture.capture_step(step_c, *batches[0], restore=restore)
    for bt in batches:
        captured(*bt)
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(model_e.named_parameters(), model_c.named_parameters()):
        assert torch.equal(a, b), n
    name = "body.behaviors.0.memory.initial_memory"
    assert not torch.equal(dict(model_c.named_parameters())[name], init[name])
    history = [float(captured(*batches[0])) for _ in range(20)]      # (the captured step returns its static output: read at once)
    assert np.isfinite(history).all() and history[-1] < history[0], history[::5]
