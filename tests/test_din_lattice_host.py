"""The conditions tests/din_lattice_cases.py states, checked for every case of its table (no GPU): the inputs are on the lattice, every
sum of the raw-mode PReLU graph is exact in fp32 in any order (abs_bound below 2^18 = 2^24 quanta), the fp32 torch graph equals the
fp64 reference bit for bit, the launchers pick the (H2T, NT, NS) the table says, the ties and the gradients are dense enough for a
dropped term to show, and the softmax run of the same inputs is well conditioned (so that a failing bar of
tests/test_din_lattice_gpu.py is the kernel's)."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from tests import din_attn_ref as ref
from tests import din_lattice_cases as lc

IDS = [c.id for c in lc.CASES]
E32_MAX = 5e-7           # of the softmax run: at most 5e-7 was measured on the CPU; the GPU tests' bars are max(1e-5, 4 E32)
BY_DIMS = collections.OrderedDict()
for _c in lc.CASES:
    BY_DIMS.setdefault(_c.dims[1:], []).append(_c)
del _c


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, B, T, K, H1, H2):
    plan = (ctypes.c_int * 8)()
    return lib.fil_din_plan(B, T, K, H1, H2, plan), list(plan)


# ---------------------------------------------------------------------------------------------------- the table
def test_paths_cover_every_template_instantiation():
    reached = collections.Counter()
    for dims, want in lc.PATHS.items():
        L = lc.layout(*dims)
        assert lc.on_the_menu(*dims), dims
        assert (L["H2T"], L["NT"], L["NS"]) == want, (dims, L)
        reached[want[:2]] += 1
    # NT = 2 at H2T = 64 is on the menu (K = 20, H1 = 113, H2 = 49: 14577 parameters, 276 tiles), so all eight pairs are asked for
    assert lc.on_the_menu(3, 20, 113, 49) and 4 * 20 * 113 + 113 * 49 <= lc.MAX_PARAMS
    assert set(reached) == {(h, n) for h in (16, 32, 48, 64) for n in (1, 2)}
    assert {w[2] for w in lc.PATHS.values()} == {1, 2, 3, 4}
    # the notes of the table
    assert lc.layout(3, 16, 128, 64)["tiles"] == 256 and lc.layout(3, 32, 112, 18)["tiles"] == 280 and lc.layout(3, 64, 56, 33)["tiles"] == 298
    assert lc.layout(3, 36, 100, 10)["lds_bwd"] == 161008 and lc.layout(3, 16, 80, 40)["lds_bwd"] == 162320 <= lc.LDS_LIMIT
    assert 4 * 16 * 128 + 128 * 32 == 12288
    # the backward's footprint, and so NS and NT, does not depend on T
    for (T, K, H1, H2), want in lc.PATHS.items():
        for T2 in (1, 64, 256):
            L = lc.layout(T2, K, H1, H2)
            assert L["lds_bwd"] == lc.layout(T, K, H1, H2)["lds_bwd"] and (L["H2T"], L["NT"]) == want[:2]


def test_case_table():
    assert len(set(IDS)) == len(IDS)
    runs = {(c.dims, c.B) for c in lc.CASES}
    for ns, dims in lc.EDGE_SHAPES.items():
        assert lc.PATHS[dims][2] == ns
        assert lc.B_EDGES(ns) == tuple(b for b in (ns - 1, ns, ns + 1, 15 * ns, 16 * ns, 16 * ns + 1, 512 * ns + 1) if b >= 1)
        for B in lc.B_EDGES(ns):
            assert (dims, B) in runs
        # one partial, one, two; 15, 16 and 17 partials; the whole grid, whose workgroup 0 makes a second trip with one sample
        assert [lc.grid(B, ns) for B in lc.B_EDGES(ns)][-6:] == [1, 2, 15, 16, 17, 512]
    for dims, (_, _, ns) in lc.PATHS.items():
        assert (dims, ns + 1) in runs and (dims, 2 * ns + 3) in runs or dims in lc.EDGE_SHAPES.values()
    for K, H1, H2 in lc.SLOT_SHAPES:
        for T in lc.SLOT_TRIPS:
            assert any(c.dims == (T, K, H1, H2) for c in lc.CASES)
    assert lc.SLOT_TRIPS == (63, 64, 65, 128, 129, 192, 193, 255, 256)
    assert {c.mask for c in lc.CASES} == {"ragged", None, "edges"}
    # every (H2T, NT) pair and every NS is among the cases that run
    assert {(c.plan["H2T"], c.plan["NT"]) for c in lc.CASES} == {(h, n) for h in (16, 32, 48, 64) for n in (1, 2)}
    assert {c.plan["NS"] for c in lc.CASES} == {1, 2, 3, 4}


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_the_library_plans_what_the_table_says(lib, case):
    L = case.plan
    rc, pl = _plan(lib, *case.shape)
    assert rc == 0, lib.fil_last_error().decode()
    want_grid = lc.grid(case.B, L["NS"])
    assert pl[:6] == [1, 1, L["NS"], want_grid, lc.GRID_CAP, want_grid], (pl, L)
    assert pl[6:] == [L["lds_fwd"], L["lds_bwd"]]
    if (case.T, case.K, case.H1, case.H2) in lc.PATHS:
        assert (L["H2T"], L["NT"], L["NS"]) == lc.PATHS[case.dims]


# ---------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_inputs_are_on_the_lattice(case):
    c = lc.build(case)
    B, T, K, H1, H2 = case.shape
    assert c["activation"] == "prelu" and c["shape"] == case.shape and c["quantum"] == 2.0 ** -6
    for name, quantum in lc.INPUT_QUANTA.items():
        v = np.asarray(c[name], np.float64)
        assert np.array_equal(v, np.round(v / quantum) * quantum), name
    assert set(np.unique(c["q"])) <= {-1, 0, 1} and set(np.unique(c["keys"])) <= {-1, 0, 1} and set(np.unique(c["g"])) <= {-2, -1, 0, 1, 2}
    assert set(np.unique(c["b1"])) <= {-1, 0, 1} and set(np.unique(c["b2"])) <= {-1, 0, 1}
    assert set(np.unique(c["alpha1"])) <= {0, 0.25, 0.5} and set(np.unique(c["alpha2"])) <= {0, 0.25, 0.5}
    assert set(np.unique(c["w3"])) <= {-1, 1} and c["b3"].tolist() == [1.0]
    W1, W2 = c["W1"], c["W2"]
    assert W1.shape == (4 * K, H1) and W2.shape == (H1, H2) and set(np.unique(W1)) <= {-1, 0, 1} and set(np.unique(W2)) <= {-1, 0, 1}
    assert ((W1 != 0).sum(0) == min(4, 4 * K)).all()
    assert ((W2 != 0).sum(0) >= min(4, H1)).all() and W2.any(1).all()           # (more than four where a row would be empty)
    if 4 * H2 >= H1:
        assert ((W2 != 0).sum(0) == min(4, H1)).all()
    if 4 * H1 >= 4 * K:
        assert W1.any(1).all()
    if case.mask is None:
        assert c["mask"] is None
    else:
        assert c["mask"].shape == (B, T) and c["mask"].dtype == np.uint8
    if case.mask == "edges":
        m = c["mask"]
        assert not m[0].any() and m[1].all() and m[2].tolist() == [1] + [0] * (T - 1) and m[3].tolist() == [0] * (T - 1) + [1]
        assert B >= 5 and m[4].sum() >= 2 and (c["keys"][4] == c["keys"][4, 0]).all()


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_every_sum_is_exact_and_the_fp32_graph_is_the_reference(case):
    c = lc.build(case)
    want = lc.reference(c)
    assert lc.EXACT_BELOW == 2.0 ** 18 == 2.0 ** 24 * c["quantum"]
    assert set(c["bound"]) >= set(lc.TENSORS)
    for name, bound in c["bound"].items():
        assert float(np.max(bound, initial=0.0)) < lc.EXACT_BELOW, name
        if name in want:       # the bound is one: proved on the case
            assert (np.abs(want[name]).reshape(bound.shape) <= bound).all(), name
    for name, v in want.items():
        assert np.array_equal(v, np.round(v / c["quantum"]) * c["quantum"]), name
    got = ref.torch_run(c, torch.float32)
    for name in lc.TENSORS:
        assert np.array_equal(got[name].reshape(want[name].shape), want[name]), name
    # ties, and gradients dense enough to show a dropped term
    z1, z2 = lc.zero_fractions(c)
    assert z1 >= 0.05 and z2 >= 0.01, (z1, z2)
    assert (want["dW1"] != 0).mean() >= 0.75
    live = ref._live(c["mask"], case.B, case.T)
    assert not want["dkeys"][~live].any() and not want["out"][~live.any(1)].any() and not want["dq"][~live.any(1)].any()


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_the_softmax_run_is_well_conditioned(case):
    c = dict(lc.build(case), softmax=True)
    out, bwd, e32 = ref.reference(c)
    assert max(bwd["cond"].values()) <= ref.MAX_COND, bwd["cond"]
    assert max(e32.values()) <= E32_MAX, e32
    assert all(v == 1e-5 for v in ref.bars(e32).values())          # 4 E32 < 1e-5: the bar is the standing one
    # one live slot, or live keys that are all the same row: the output is that row
    live = ref._live(c["mask"], case.B, case.T)
    for b in range(case.B):
        rows = c["keys"][b][live[b]]
        if len(rows) and (rows == rows[0]).all():
            assert np.abs(out[b] - rows[0]).max() < 1e-15


@pytest.mark.parametrize("dims", list(BY_DIMS), ids=lambda d: "x".join(map(str, d)))
def test_every_parameter_gradient_element_is_nonzero_in_some_case(dims):
    """Per (K, H1, H2), the shape of the parameters, over its cases: a tile, a column or a unit that no case moves could be dropped
    unseen.  (The rows of dq are samples: every one of its K columns is nonzero in some sample.)"""
    seen = {}
    for case in BY_DIMS[dims]:
        want = lc.reference(lc.build(case))
        for name in ("dW1", "dW2", "db1", "db2", "dalpha1", "dw3"):
            seen[name] = seen.get(name, False) | (want[name] != 0)
        seen["dq"] = seen.get("dq", False) | (want["dq"] != 0).any(0)
    for name, s in seen.items():
        assert s.all(), (name, np.argwhere(~s)[:4].tolist(), int((~s).sum()))
