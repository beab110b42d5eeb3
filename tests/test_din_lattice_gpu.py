"""Every dispatch path of the DIN attention kernels (csrc/din.hip: H2T in {16, 32, 48, 64} x NT in {1, 2}, NS = 1 .. 4 samples per
workgroup) against the fp64 reference BIT FOR BIT, element for element, on the integer-lattice cases of tests/din_lattice_cases.py.

On those cases every fp32 sum of raw-mode PReLU DIN is exact in any order (tests/test_din_lattice_host.py proves it for every case),
so out and all ten gradients have to be the reference's value in every element: a dW1 tile that misses a sample, a partial the
reduction skips, a padded unit that leaks or a tie (u = 0: a fifth of layer 1) taken the other way shows as a wrong multiple of 1/64,
however small its share of the tensor's norm.  The softmax mode of the same inputs, whose pre-activations are the same and still
exact, is held to the standing bars of tests/test_din_attn_gpu.py (max(1e-5, 4 E32) = 1e-5 on every case, host test), and the sigmoid
instantiations of the paths no other test reaches to the same bars on din_attn_ref.make_case inputs.

What these tests see was checked with value-only mutants of csrc/din.hip, each built and run once (MI355X), counted in the raw-mode
test: `u >= 0.f` in the backward's du1 fails all 90 cases (and no test of tests/test_din_attn_gpu.py); the second tile of an NT = 2
thread zeroed fails the 36 NT = 2 cases and no other; param_reduce_kernel without slice 15 the 25 cases with 16 or more partials;
dalpha1 of the last unit zeroed where H1 % 8 != 0 43 of those 47 cases (in four small ones the reference's value is 0); the layer-2
accumulator m = 16 dropped in the H2T = 32 forward 30 of the 31 H2T = 32 cases.  The softmax test found that the backward lost
2^-24 / eps of ds where one weight was 1 - eps (dq off by up to 14 %); din_bwd_kernel's gc is the fix.

All results being equal, bits cannot show which kernel ran: the host test holds fil_din_plan and the restated launch rule to the
table's (H2T, NT, NS) for every case; each case prints them."""
import functools

import numpy as np
import pytest
import torch

from tests import din_attn_ref as ref
from tests import din_lattice_cases as lc
from tests.test_din_attn_gpu import bits, check_parity, run_op, run_raw

pytestmark = pytest.mark.gpu

IDS = [c.id for c in lc.CASES]
by_id = {c.id: c for c in lc.CASES}


@functools.lru_cache(maxsize=None)
def oracle(case):
    return lc.reference(lc.build(case))


@functools.lru_cache(maxsize=None)
def softmax_case(case):
    """The same inputs in softmax mode: one object per case, so that din_attn_ref.reference computes its oracle once."""
    return dict(lc.build(case), softmax=True)


def where(name, idx, case):
    """The place of a wrong element in the backward's work split: the 4 x 16 tile of dW1 / dW2, its thread and which of the thread's NT
    tiles it is."""
    n_c1, n_c2 = -(-case.H1 // 16), -(-case.H2 // 16)
    if name == "dW1":
        tile = (idx[0] // 4) * n_c1 + idx[1] // 16
    elif name == "dW2":
        tile = case.K * n_c1 + (idx[0] // 4) * n_c2 + idx[1] // 16
    else:
        return ""
    return ", tile %d (rows %d.., columns %d..) = thread %d's tile %d" % (tile, idx[0] // 4 * 4, idx[1] // 16 * 16, tile % 256, tile // 256)


def mismatches(got, want, case):
    """[text] for every tensor of a run that is not the oracle's in every element."""
    bad = []
    for name in lc.TENSORS:
        a, b = np.asarray(got[name], np.float64).reshape(want[name].shape), want[name]
        if not np.array_equal(a, b):
            d = a != b          # (a NaN differs from everything)
            i = tuple(int(v) for v in np.argwhere(d)[0])
            bad.append("%s: %d of %d elements differ, first at %s: got %r, reference %r%s"
                       % (name, int(d.sum()), d.size, i, float(a[i]), float(b[i]), where(name, i, case)))
    return bad


def plus_zero(a):
    return not np.asarray(a).any() and not np.signbit(np.asarray(a)).any()


def check_exact(got, case, label):
    c, L = lc.build(case), case.plan
    bad = mismatches(got, oracle(case), case)
    print("%s %s H2T %d NT %d NS %d grid %d: %s" % (label, case.id, L["H2T"], L["NT"], L["NS"], lc.grid(case.B, L["NS"]),
                                                   "bit-equal in out and 10 gradients" if not bad else "; ".join(bad)))
    assert not bad, "%s: %s" % (case.id, "; ".join(bad))
    live = ref._live(c["mask"], case.B, case.T)
    assert plus_zero(got["dkeys"][~live])                                       # every masked slot: exactly +0
    assert not got["out"][~live.any(1)].any() and not got["dq"][~live.any(1)].any()


# ---------------------------------------------------------------------------------------------------- 1. raw mode, bit for bit
@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_raw_mode_equals_the_reference_bit_for_bit(case):
    check_exact(run_op(lc.build(case)), case, "op")


# ---------------------------------------------------------------------------------------------------- 2. the entry points under guards
RAW = ["batch-3x3x36x100x10","path-2x3x32x112x18", "path-3x3x4x128x17"]       # NT = 2 (NS = 2); NT = 2 and H2T = 32 (NS = 1); H2T = 32 (NS = 2)


@pytest.mark.parametrize("name", RAW)
def test_raw_entry_points_under_guards(name):
    """B = NS + 1: the last workgroup holds fewer than NS samples.  The outputs lie between sentinels, the workspace is NaN before the
    call (run_raw asserts the guards): a partial that a short workgroup left unwritten would reach a gradient as NaN."""
    case = by_id[name]
    assert case.B == case.plan["NS"] + 1 and (case.plan["NT"] == 2 or case.plan["H2T"] == 32)
    got = run_raw(lc.build(case))
    assert all(np.isfinite(v).all() for v in got.values())
    check_exact(got, case, "entry points")


# ---------------------------------------------------------------------------------------------------- 3. softmax on the same cases
@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_softmax_mode_of_the_same_cases(case):
    c = softmax_case(case)
    got = run_op(c)
    check_parity(got, c, label=case.id)
    live = ref._live(c["mask"], case.B, case.T)
    assert plus_zero(got["dkeys"][~live])
    assert not got["out"][~live.any(1)].any() and not got["dq"][~live.any(1)].any()
    # live keys that are all the same row (one live slot among them): equal scores, weights that are exactly 1 / n, that row exactly
    n_same = 0
    for b in range(case.B):
        rows = c["keys"][b][live[b]]
        if len(rows) and (rows == rows[0]).all():
            n_same += 1
            assert np.array_equal(bits(got["out"][b]), bits(rows[0] + 0.0)), (b, got["out"][b], rows[0])
    assert n_same >= 3 or case.mask != "edges"


# ---------------------------------------------------------------------------------------------------- 4. sigmoid on the new paths
# one shape per (H2T, NT) that no test of tests/test_din_attn_gpu.py launches: (32, 1), (16, 2), (32, 2), (48, 2), (64, 2)
SIGMOID_DIMS = [(3, 8, 20, 32), (3, 36, 100, 10), (3, 32, 112, 18), (3, 64, 56, 33), (3, 20, 113, 49)]


@functools.lru_cache(maxsize=None)
def sigmoid_case(dims, softmax):
    """B = 32 NS + 1: 33 partials, the last workgroup short, and B T >= 64 slots (below that din_attn_ref.conditioned_case would have to
    pick the draw; it finds none at these widths, where h2 hardly varies and softmax's sum_t ds_t h2_t nearly cancels)."""
    B = 32 * lc.PATHS[dims][2] + 1
    assert B * dims[0] >= 64
    return ref.make_case(B, *dims, "sigmoid", softmax, seed=0)


@pytest.mark.parametrize("softmax", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("dims", SIGMOID_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_sigmoid_on_the_paths_no_other_test_reaches(dims, softmax):
    H2T, NT, _ = lc.PATHS[dims]
    assert (H2T, NT) in ((32, 1), (16, 2), (32, 2), (48, 2), (64, 2))
    case = sigmoid_case(dims, softmax)
    check_parity(run_op(case), case, label="H2T %d NT %d" % (H2T, NT))


# ---------------------------------------------------------------------------------------------------- 5. gradient subsets
def test_gradient_subsets_have_the_bits_of_the_full_backward():
    """NT = 2.  q and keys alone: no parameter pass, no workspace, the tiles idle; the parameters alone: no dq / dkeys stores."""
    case = by_id["path-5x3x64x56x33"]
    assert case.plan["NT"] == 2
    c = lc.build(case)
    full = run_op(c)
    check_exact(full, case, "full")
    for wanted in (("q", "keys"), tuple(ref.PARAMS)):
        got = run_op(c, wanted=wanted)
        for k in ("q", "keys") + ref.PARAMS:
            if k in wanted:
                assert np.array_equal(bits(got["d" + k]), bits(full["d" + k])), (wanted, k)
            else:
                assert got["d" + k] is None, (wanted, k)
        assert np.array_equal(bits(got["out"]), bits(full["out"]))


# ---------------------------------------------------------------------------------------------------- 6. repeats
def test_repeats_are_bit_identical_with_two_tiles_per_thread():
    case = lc.REPEAT
    assert (case.plan["NT"], case.plan["NS"], case.B) == (2, 1, 513)
    c = lc.build(case)
    first, second = run_op(c), run_op(c)
    for k, v in first.items():
        assert np.array_equal(bits(v), bits(second[k])), k
