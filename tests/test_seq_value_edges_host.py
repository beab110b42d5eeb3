"""The value-edge cases of tests/seq_value_cases.py on the CPU: every condition the GPU test (tests/test_seq_value_edges_gpu.py) leans
on is asserted here against the fp64 references -- the seed that was chosen, the dead set and that it is the predicted one, the cap
on the live slices' E32 (so that every bar is the 1e-5 floor), the live per-unit slices' norms, that the gates meant to saturate do,
and |c| >= 20 in the long case.  pytest -s prints them."""
import numpy as np
import pytest

from tests import gru_ref, lstm_ref
from tests import seq_value_cases as vc

cases = pytest.mark.parametrize("spec", vc.CASES, ids=vc.case_id)


@cases
def test_the_case_meets_its_conditions(spec):
    case = vc.find_case(*spec)
    v = vc.value_reference(case)
    e32, norm = vc.conditions(case)
    dead = vc.dead_set(case)
    print("%s: seed %d, worst live E32 %.2e (cap %.1e), smallest live per-unit norm %.2e (at least %.0e)"
          % (vc.case_id(spec), case["seed"], e32, vc.MAX_E32, norm, vc.MIN_NORM))
    print("  dead:", sorted(dead, key=str))
    assert e32 <= vc.MAX_E32 and norm >= vc.MIN_NORM
    assert dead == vc.predicted_dead(case)
    for k in v["e32"]:
        assert vc.bar_of(case, k) == 1e-5, k
    for k in dead:        # far below the line between dead and live, and gone in the fp32 restatement too
        assert v["norm"][k] < 1e-40 and np.abs(vc.slices(case, v["f32"])[k]).max() <= vc.DEAD_NORM, k
    live_units = [k for k in v["e32"] if k[1] == "unit"]
    assert len(live_units) + len([k for k in v["norm"] if k[1] == "unit" and k not in v["e32"]]) == 5 * 8 * vc.ndir(case)
    if spec[0] != "driven":
        assert case["mask"] is not None and 0 < case["mask"].sum() < case["mask"].size
        if spec[1] == "lstm":
            assert {k[2].split(":")[1] for k in dead if k[1] == "unit"} == {"i-", "o-"}
    else:
        assert case["mask"] is None and not case["x"][1].any() and np.abs(case["x"][0]).max() > 32


def _gate_values(case):
    """{unit label: the values its saturated gate takes over the live steps} from the fp64 reference's kept steps."""
    out = {}
    if case["op"] == "lstm":
        x, live, W, U, b, revs = lstm_ref._inputs(case)
        for d, rev in enumerate(revs):
            keep = lstm_ref._steps(x, live, W[d], U[d], b[d], rev)[1]
            for j, u in enumerate(vc.LSTM_UNITS):
                if u != "plain":
                    out[(d, u)] = np.concatenate([s[dict(i="i", f="f", o="o", c="g")[u[0]]][live[:, t], j] for t, s in enumerate(keep)])
    else:
        p = gru_ref._steps(case)
        for j, u in enumerate(vc.GRU_UNITS):
            if u != "plain":
                out[(0, u)] = np.concatenate([s[dict(z="z", r="r", h="c")[u[0]]][p["live"][:, t], j] for t, s in enumerate(p["keep"])])
    return out


@pytest.mark.parametrize("spec", [c for c in vc.CASES if c[0] != "driven" and c[3] == "both"], ids=vc.case_id)
def test_the_saturated_gates_are_exactly_at_their_ends(spec):
    """sigmoid(+100) and tanh(+100) round to 1.0 in fp64, tanh(-100) to -1.0, sigmoid(-100) is 3.7e-44: the pre-activation stays past
    +-90 whatever x W + h U adds."""
    case = vc.find_case(*spec)
    for (d, u), vals in _gate_values(case).items():
        assert vals.size
        if u[1] == "+":
            assert (vals == 1.0).all(), (d, u)
        elif u[0] in "ch":
            assert (vals == -1.0).all(), (d, u)
        else:
            assert (vals > 0).all() and (vals < 1e-39).all(), (d, u)


@pytest.mark.parametrize("direction", ["forward", "bidirectional"])
def test_the_long_cases_cell_state_leaves_tanhs_range(direction):
    case = vc.find_case("long", "lstm", direction)
    top = vc.long_max_c(case)
    print("long %s: seed %d, max |c| of the f+ unit per direction %s" % (direction, case["seed"], ["%.1f" % c for c in top]))
    assert case["shape"] == vc.LONG_SHAPE and min(top) >= vc.LONG_MIN_C
    assert np.float32(np.tanh(np.float32(vc.LONG_MIN_C))) == 1.0


def test_the_driven_scale_saturates_without_a_bias():
    """x * 64 pushes gates of sample 0 past |z| = 16, where 1 - sigmoid is below fp32's half ulp of 1."""
    case = vc.find_case("driven", "lstm", "forward")
    z = np.abs(case["x"][0] @ case["W"] + case["b"])
    assert (z > 16).any() and vc.DRIVE == 64.0


@pytest.mark.parametrize("spec", [("saturated", "gru", "augru", "both"), ("saturated", "lstm", "bidirectional", "both"),
                                  ("driven", "lstm", "forward", "last")], ids=vc.case_id)
def test_the_rules_pass_the_fp32_restatement_and_catch_one_wrong_unit(spec):
    """check_slices on the CPU's fp32 restatement passes; with one small-valued unit of hs off by 1e-4 of itself -- far inside the
    whole tensor's bar -- or one dead column at 1e-20, or a NaN, it fails."""
    case = vc.find_case(*spec)
    v = vc.value_reference(case)
    out = "hs" if spec[3] == "both" else "last"
    got = {k: np.array(v["f32"][k]) for k in (out,) + tuple(vc.REF[spec[1]].GRADS) if not (k == "da" and spec[2] == "gru")}
    vc.check_slices(case, got)
    live = [k for k in v["e32"] if k[:2] == (out, "unit")]
    name = min(live, key=lambda k: v["norm"][k])[2]
    u = vc.unit_names(case).index(name)
    wrong = dict(got, **{out: got[out].copy()})
    wrong[out][..., u] *= 1.0 + 1e-4
    whole = np.linalg.norm(wrong[out] - v["ref"][out]) / np.linalg.norm(v["ref"][out])
    print("one unit off by 1e-4: whole-tensor error %.2e" % whole)
    with pytest.raises(AssertionError):
        vc.check_slices(case, wrong)
    dead = sorted((k for k in vc.dead_set(case) if k[0] == "dW"), key=str)
    if dead:
        wrong = dict(got, dW=got["dW"].copy())
        H = case["shape"][3]
        d, j = divmod(vc.unit_names(case).index(dead[0][2]), H)
        (wrong["dW"][d] if vc.ndir(case) == 2 else wrong["dW"])[0, j] = 1e-20
        with pytest.raises(AssertionError):
            vc.check_slices(case, wrong)
    wrong = dict(got, dx=got["dx"].copy())
    wrong["dx"][0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        vc.check_slices(case, wrong)
