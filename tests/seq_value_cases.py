"""Value-edge cases of the GRU and the LSTM (tests/test_seq_value_edges_host.py, tests/test_seq_value_edges_gpu.py): gates driven to
exactly 0 or 1 through a bias of +-100 (saturated_case) or through large inputs (driven_case), a long LSTM whose cell state leaves
tanh's range (long_lstm_case), and a measure per unit and per sample instead of per tensor.  numpy and the references of
tests/gru_ref.py / tests/lstm_ref.py only: no GPU, no library.

Why +-100: for v >= 90 expf(-v) vanishes next to 1 and 1 / (1 + expf(-v)) is exactly 1 in fp32; for v <= -90 expf(-v) overflows to inf
and 1 / (1 + inf) is exactly 0; tanhf(+-100) is exactly +-1.  In fp64, sigmoid(100) rounds to 1.0 and sigmoid(-100) is 3.7e-44.

Slices.  A per-unit slice is one tensor's part that belongs to one hidden unit j (in "bidirectional": to one unit of one direction):
hs[:, :, j] (or last[:, j]), and the unit's gate columns {g H + j} of dW, dU and db.  A per-sample slice is hs[b] (or last[b]), dx[b]
and, in the modes "augru" and "agru", da[b].  A slice is DEAD when its fp64 reference norm is at most DEAD_NORM, else LIVE.

The dead set follows from the construction (predicted_dead; the host test asserts that the fp64 reference gives exactly this set):
    LSTM, saturated   every slice of the units i- (c stays 0) and o- (h is 0 and passes no gradient on);
    GRU, saturated    "gru", "augru": every slice of the unit z+ (u = 1 - z = 0: the state stays 0 and no gradient passes);
                      "agru" (the score replaces the update gate, and tanh'(+-100) = 0): dW, dU, db of the units h+ and h-, and dU of
                      the unit r- (its recurrent pre-activation reaches nothing: dhp = (0, dc hp r (1 - r), dc r));
                      "augru", "agru": hs and dx of sample 0, whose scores are all 0;
    every case        hs, dx and da of a sample whose mask has no live slot;
    driven, long      nothing beyond the line above (the driven cases have no mask).
As printed by the host test (pytest -s), the dead per-unit slices of the saturated cases are, per (tensor, unit): LSTM hs / dW / dU / db
of i- and o- in each direction; GRU "gru" / "augru" hs / dW / dU / db of z+; GRU "agru" dW / dU / db of h+ and h-, dU of r-."""
import functools

import numpy as np
import torch

from tests import gru_ref, lstm_ref

SHAPE = (5, 6, 4, 8)            # B = one full sample quad plus one sample
LONG_SHAPE = (2, 300, 4, 8)
SAT = 100.0
DRIVE = 64.0                    # (at 256 the E32 of dW rises to 2.8e-6 and starts moving the bar)
DEAD_NORM = 1e-30
MAX_E32 = 2.5e-6                # a live slice's bar max(1e-5, 4 E32) is then the 1e-5 floor
MIN_NORM = 1e-2                 # of a live per-unit slice
LONG_MIN_C = 20.0               # |c| of the f+ unit in the long case: tanh(c) is exactly +-1 in fp32 there and 1 - tanh^2 is 0

LSTM_UNITS = ("plain", "i+", "i-", "f+", "f-", "o+", "o-", "c+")        # unit j of every direction
GRU_UNITS = ("plain", "z+", "z-", "r+", "r-", "h+", "h-", "plain")      # unit j (the input-bias row b[0])
GATES = dict(lstm="ifco", gru="zrh")
REF = dict(lstm=lstm_ref, gru=gru_ref)
MODES = dict(lstm=lstm_ref.DIRECTIONS, gru=gru_ref.MODES)


def units_of(op):
    return LSTM_UNITS if op == "lstm" else GRU_UNITS


def _saturate(op, case):
    """The bias of the chosen units at +-SAT (in place)."""
    H = case["shape"][3]
    gates = GATES[op]
    b = case["b"]
    rows = [b[0], b[1]] if (op == "lstm" and b.ndim == 2) else ([b[0]] if op == "gru" else [b])
    for row in rows:
        for j, u in enumerate(units_of(op)):
            if u != "plain":
                row[gates.index(u[0]) * H + j] = SAT if u[1] == "+" else -SAT
    return case


def _scores(case):
    """The scores of "augru" / "agru": sample 0 all 0, sample 1 all 1, sample 2 1.5 at even steps, sample 3 -0.5 at even steps, sample
    4 (and the odd steps of 2 and 3) uniform in (0, 1) as drawn."""
    a = case["a"]
    a[0], a[1] = 0.0, 1.0
    a[2, ::2], a[3, ::2] = 1.5, -0.5
    return case


def _make(op, mode, seed, shape, mask, grads):
    key = "direction" if op == "lstm" else "mode"
    case = REF[op].make_case(*shape, mode, seed, mask=mask, grads=grads)
    case.update(op=op, seed=seed, which=case[key])
    return case


def saturated_case(op, mode, seed, grads="both", shape=SHAPE):
    """make_case at SHAPE with a ragged mask, the bias of the units of LSTM_UNITS / GRU_UNITS at +-100 and, for "augru" / "agru", the
    scores of _scores."""
    case = _saturate(op, _make(op, mode, seed, shape, "ragged", grads))
    if case.get("a") is not None:
        _scores(case)
    case["kind"] = "saturated"
    return case


def driven_case(op, mode, seed, grads="both"):
    """make_case at SHAPE without a mask, saturated through the inputs: sample 0 has x * 64, sample 1 x = 0 (live, zero), sample 2
    x * 64 at even steps."""
    case = _make(op, mode, seed, SHAPE, None, grads)
    x = case["x"]
    x[0] *= DRIVE
    x[1] = 0.0
    x[2, ::2] *= DRIVE
    case["kind"] = "driven"
    return case


def long_lstm_case(direction, seed):
    """(2, 300, 4, 8) with the saturated bias pattern and a ragged mask."""
    case = saturated_case("lstm", direction, seed, shape=LONG_SHAPE)
    case["kind"] = "long"
    return case


def ndir(case):
    return 2 if case["which"] == "bidirectional" else 1


def last_of(case, hs):
    return lstm_ref.last_of(hs, case["which"]) if case["op"] == "lstm" else hs[:, -1]


def unit_names(case):
    """The per-unit slices' unit labels, in slice order: "3:f+" or, with two directions, "fwd 3:f+" / "rev 3:f+" (a driven case has no
    bias pattern: every unit is "plain")."""
    us = units_of(case["op"]) if case["kind"] != "driven" else ("plain",) * case["shape"][3]
    tag = lambda j, u: "%d:%s" % (j, u)
    if ndir(case) == 1:
        return [tag(j, u) for j, u in enumerate(us)]
    return ["%s %s" % (d, tag(j, u)) for d in ("fwd", "rev") for j, u in enumerate(us)]


def slices(case, t):
    """t: dict with hs [B,T,nH] or last [B,nH], and any of dx, da, dW, dU, db (None = absent) -> {(tensor, "unit" | "sample", label):
    the slice as a float64 array}.  da is left out in mode "gru" (it has none)."""
    op = case["op"]
    B, T, K, H = case["shape"]
    n, ng = ndir(case), len(GATES[op])
    names = unit_names(case)
    out = {}
    A = lambda v: np.asarray(v, np.float64)
    for key in ("hs", "last"):
        if t.get(key) is not None:
            v = A(t[key])
            for u, name in enumerate(names):
                out[(key, "unit", name)] = v[..., u]
            for b in range(B):
                out[(key, "sample", b)] = v[b]
    for key in ("dx", "da"):
        if t.get(key) is not None and not (key == "da" and case["which"] == "gru"):
            v = A(t[key])
            for b in range(B):
                out[(key, "sample", b)] = v[b]
    for key in ("dW", "dU", "db"):
        if t.get(key) is not None:
            v = A(t[key])
            full = dict(dW=(K, ng * H), dU=(H, ng * H), db=((2, ng * H) if op == "gru" else (ng * H,)))[key]
            v = v.reshape(((n,) if n == 2 else ()) + full)
            for u, name in enumerate(names):
                d, j = divmod(u, H)
                cols = [g * H + j for g in range(ng)]
                out[(key, "unit", name)] = (v[d] if n == 2 else v)[..., cols]
    return out


_CACHE = {}


def value_reference(case):
    """-> dict(ref: the fp64 tensors (hs, last, the gradients), f32: the fp32 torch restatement's, norm / e32: per slice key), computed
    once per case object."""
    hit = _CACHE.get(id(case))
    if hit is None or hit[0] is not case:
        R = REF[case["op"]]
        hs, bwd, _ = R.reference(case)
        f32 = R.torch_run(case, torch.float32)
        ref = dict(hs=hs, last=last_of(case, hs), **{k: bwd[k] for k in R.GRADS})
        f32 = dict(f32, last=last_of(case, f32["hs"]))
        rs, fs = slices(case, ref), slices(case, f32)
        norm = {k: float(np.linalg.norm(v)) for k, v in rs.items()}
        e32 = {k: float(np.linalg.norm(fs[k] - v) / norm[k]) for k, v in rs.items() if norm[k] > DEAD_NORM}
        hit = _CACHE[id(case)] = (case, dict(ref=ref, f32=f32, norm=norm, e32=e32))
    return hit[1]


def dead_set(case):
    """The slice keys whose fp64 reference norm is at most DEAD_NORM (of hs, not of last)."""
    return {k for k, v in value_reference(case)["norm"].items() if v <= DEAD_NORM and k[0] != "last"}


def predicted_dead(case):
    """The dead set the construction predicts (the module docstring says why); reads the case's inputs only."""
    op, kind, which = case["op"], case["kind"], case["which"]
    B = case["shape"][0]
    dead = set()
    per_sample = ("hs", "dx") + (("da",) if op == "gru" and which != "gru" else ())
    if case.get("mask") is not None:
        for b in np.nonzero(np.asarray(case["mask"]).sum(1) == 0)[0]:
            dead |= {(k, "sample", int(b)) for k in per_sample}
    if kind == "driven":
        return dead
    for name in unit_names(case):
        u = name.split(":")[1]
        if op == "lstm" and u in ("i-", "o-"):
            dead |= {(k, "unit", name) for k in ("hs", "dW", "dU", "db")}
        if op == "gru" and which in ("gru", "augru") and u == "z+":
            dead |= {(k, "unit", name) for k in ("hs", "dW", "dU", "db")}
        if op == "gru" and which == "agru" and u in ("h+", "h-"):
            dead |= {(k, "unit", name) for k in ("dW", "dU", "db")}
        if op == "gru" and which == "agru" and u == "r-":
            dead.add(("dU", "unit", name))
    if op == "gru" and which in ("augru", "agru"):
        dead |= {("hs", "sample", 0), ("dx", "sample", 0)}
    return dead


def conditions(case):
    """-> (worst E32 of a live slice, smallest norm of a live per-unit slice), over the slices a GPU run of the case returns (hs with a
    g_hs, else last)."""
    v = value_reference(case)
    skip = "last" if case.get("g_hs") is not None else "hs"
    live = [k for k in v["e32"] if k[0] != skip]
    return max(v["e32"][k] for k in live), min(v["norm"][k] for k in live if k[1] == "unit")


def long_max_c(case):
    """max |c| of the f+ unit in the fp64 reference, per direction."""
    x, live, W, U, b, revs = lstm_ref._inputs(case)
    j = LSTM_UNITS.index("f+")
    return [max(float(np.abs(s["cn"][:, j]).max()) for s in lstm_ref._steps(x, live, W[d], U[d], b[d], rev)[1]) for d, rev in enumerate(revs)]


@functools.lru_cache(maxsize=None)
def find_case(kind, op, mode, grads="both"):
    """The case of `kind` ("saturated", "driven", "long") with the first seed in 0 .. 99 whose live slices all have E32 <= MAX_E32,
    whose live per-unit slices all have a reference norm >= MIN_NORM and whose dead set is the predicted one ("long": and whose f+
    cell state reaches LONG_MIN_C in every direction), in the style of conditioned_case: the choice reads the fp64 reference and the
    CPU's fp32 restatement only."""
    for seed in range(100):
        if kind == "long":
            case = long_lstm_case(mode, seed)
            if min(long_max_c(case)) < LONG_MIN_C:
                continue
        else:
            case = (saturated_case if kind == "saturated" else driven_case)(op, mode, seed, grads=grads)
        e32, norm = conditions(case)
        if e32 <= MAX_E32 and norm >= MIN_NORM and dead_set(case) == predicted_dead(case):
            return case
    raise AssertionError("find_case: no seed in 0 .. 99 meets the conditions for %s" % ((kind, op, mode, grads),))


def bar_of(case, key):
    """max(1e-5, 4 E32_slice): the project's bar formula with E32 taken on the same slice."""
    return max(1e-5, 4.0 * value_reference(case)["e32"][key])


def check_slices(case, got, label=""):
    """The rules, on what a run returned (got: hs or last, and the gradients; None = absent).  A live slice: norm-relative error
    against that slice of the fp64 reference <= bar_of.  A dead slice: every element finite and at most DEAD_NORM in magnitude (not
    exactly zero: torch's fp32 sigmoid(-100) is a denormal, the kernel's is 0, and both are right).  Every slice is printed with its
    bar.  -> the worst error / bar ratio's (error, bar, key) among the live slices."""
    v = value_reference(case)
    gs = slices(case, got)
    rs = slices(case, {k: v["ref"][k] for k in got if got[k] is not None and k in v["ref"]})
    assert set(gs) == set(rs) and gs
    worst, fails = (0.0, 1.0, None), []
    for k in sorted(gs, key=str):
        g, r = gs[k], rs[k]
        if not np.isfinite(g).all():
            fails.append((k, "not finite"))
            continue
        if v["norm"][k] <= DEAD_NORM:
            top = float(np.abs(g).max())
            print("%s %-28s dead   max |value| %.2e   bar %.0e" % (label, k, top, DEAD_NORM))
            if top > DEAD_NORM:
                fails.append((k, "dead slice", top))
            continue
        err, bar = float(np.linalg.norm(g - r) / v["norm"][k]), bar_of(case, k)
        print("%s %-28s live   error %.2e   bar %.2e (E32 %.2e, norm %.2e)" % (label, k, err, bar, v["e32"][k], v["norm"][k]))
        if err / bar > worst[0] / worst[1]:
            worst = (err, bar, k)
        if err > bar:
            fails.append((k, err, bar))
    print("%s worst live slice: %s error %.2e bar %.2e" % (label, worst[2], worst[0], worst[1]))
    assert not fails, fails
    return worst


# (kind, op, mode or direction, grads): "both" runs return_sequences=True (g_hs + g_last), "last" return_sequences=False
CASES = ([(kind, op, mode, grads) for kind in ("saturated", "driven") for op in ("gru", "lstm") for mode in MODES[op] for grads in ("both", "last")]
         + [("long", "lstm", d, "both") for d in ("forward", "bidirectional")])
case_id = lambda c: "-".join(c)
