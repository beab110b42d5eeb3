"""The DCN cross network (csrc/dcn.hip: fil_dcn_fwd / fil_dcn_bwd) at CONSTRUCTED menu, path and grid edges, called through the C ABI
with poisoned words behind every input, guarded outputs and a workspace of exactly fil_dcn_bwd_workspace_bytes in front of a guard.

Reference: oracle.closed.dcn_fwd / dcn_bwd in float64 on synth.dcn_case(dist="uniform").  Bar: the project's own norm-relative
max|a - b| / max|b| <= 1e-5 (TOL of tests/test_gpu_parity.py) for y, s, dx, dw and db.  s is the kernel's saved state: the backward is
fed the s that the forward wrote, so the cases whose two directions take different paths hand one path's s to the other.

The dispatch rule is restated in tests/dcn_edge_cases.py (dcn_paths(D, L), the grids, the workspace formula); every case asserts the path
it was built for, and the workspace size -- the observable that tells the two backward paths apart -- against the formula of that path.

    kernel                                           case
    dcn_fwd_kernel<8, 4> / dcn_bwd_kernel<8, 4, 6>   (9, 512, 6); the grid cases (B, 8, 2) and (B, 68, 2) (<8, 4, 2>)
    dcn_fwd_kernel<20, 4> / dcn_bwd_kernel<20, 4, 4> (9, 516, 4) almost every lane masked, (9, 1280, 4) none
    dcn_fwd_kernel<20, 4> + generic backward         (9, 516, 5)
    dcn_fwd_kernel<20, 1> / dcn_bwd_kernel<20, 1, 1> (9, 513, 1)
    dcn_fwd_kernel<32, 1>, <32, 4> + generic bwd     (7, 1281, 1), (7, 1284, 2), (7, 2048, 5)
    dcn_fwd_kernel<64, 4> + generic backward         (5, 2052, 2), (5, 4096, 5) (dynamic LDS = kDcnLdsLimit exactly)
    dcn_fwd_kernel<8, 1> / dcn_bwd_kernel<8, 1, 3>   (5, 1, 3), (5, 2, 3), (5, 3, 3)
    dcn_{fwd,bwd}_scalars_kernel<16>, bwd_cols<16>   (6, 5, 7), (6, 3, 16); the grid cases (B, 5, 7)
    dcn_{fwd,bwd}_scalars_kernel<6>, bwd_cols<6>     the generic backward of the crossing cases above (forward <6> is reached only at
                                                     D > 4096 or w, b beyond the LDS: test_gpu_parity.py::test_dcn)
    dcn_reduce_closed_kernel                         1, 1, 1, 2, 4, 31, 32, 33, 256, 256 partials (stride 32, four waves), D = 8 and 68
    dcn_reduce_kernel                                1, 2, 5, 9, 64 (ragged last chunk), 64 partials
    grid-stride loops                                B = 2053: 5 of 2048 backward waves take a second sample; B = 4101: 5 of 4096 forward
                                                     waves do; B = 2100 / 8200: the generic forward / backward scalars kernels stride
    prefetch chain of dcn_bwd_kernel,                (37, D, L) for the 13 (D, L) above with a register-resident direction, in the child
    loop of dcn_fwd_kernel, per instantiation        of tests/test_gpu_knobs.py::test_dcn_edges_with_a_two_workgroup_grid (FIL_DCN_GRID=2):
                                                     16 backward waves take 3, 3, 3, 3, 3, 2, ... samples, 8 forward waves 5, ..., 5, 4, 4, 4.
                                                     Without the knob the same cases run one sample per wave.
    That child also runs the path cases and the grid cases with B <= 257 (ids ending in `le257`).  Its path cases keep B <= 9 and so at
    most one sample per backward wave (one forward wave takes two at B = 9); its grid cases walk up to 17 samples per wave at <8, 4, 2>.
"""
import functools

import numpy as np
import pytest

from ml_function_amd import _lib, synth
from ml_function_amd._lib import check, stream_ptr
from oracle import closed
from tests import dcn_edge_cases as dc
from tests import guarded as G

pytestmark = pytest.mark.gpu

TOL = 1e-5                                 # tests/test_gpu_parity.py TOL


def rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def poisoned_input(a):
    return G.poisoned_input(G.f32_words(a))


def guarded(shape, name):
    return G.GuardedOutput(shape, np.uint32, name)


def run_dcn(x, w, b, g):
    """fil_dcn_fwd, then fil_dcn_bwd on the s it saved -> dict of the bits of y, s, dx, dw, db.  Checked here: the return codes, the
    guards of all five outputs, the workspace's size against the predicted path's formula and the guard behind the workspace."""
    lib = _lib.load()
    (B, D), L = x.shape, w.shape[0]
    what = "B=%d D=%d L=%d" % (B, D, L)
    xt, wt, bt, gt = (poisoned_input(a) for a in (x, w, b, g))
    y, s = guarded((B, D), "y"), guarded((B, L), "s")
    check(lib.fil_dcn_fwd(xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y.ptr, s.ptr, B, D, L, stream_ptr()), "fil_dcn_fwd")
    out = dict(y=y.read(what), s=s.read(what))
    st = poisoned_input(out["s"].view(np.float32))
    nws = lib.fil_dcn_bwd_workspace_bytes(B, D, L)
    assert nws == dc.workspace_bytes(B, D, L), "%s: workspace %d bytes, the %s path's formula gives %d" % (
        what, nws, dc.dcn_paths(D, L).bwd, dc.workspace_bytes(B, D, L))
    ws = G.workspace(nws)
    dx, dw, db = guarded((B, D), "dx"), guarded((L, D), "dw"), guarded((L, D), "db")
    check(lib.fil_dcn_bwd(xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), st.data_ptr(), gt.data_ptr(), dx.ptr, dw.ptr, db.ptr, B, D, L,
                          ws.data_ptr(), nws, stream_ptr()), "fil_dcn_bwd")
    out.update(dx=dx.read(what), dw=dw.read(what), db=db.read(what))
    G.assert_workspace_guard(ws, nws, what)
    return out


@functools.lru_cache(maxsize=None)
def dcn_case(B, D, L):
    """synth.dcn_case(dist="uniform") and its float64 results; read-only, shared by the tests of a shape."""
    c = synth.dcn_case(B, D, L, dist="uniform")
    y, s = closed.dcn_fwd(c["x"], c["w"], c["b"])
    dx, dw, db = closed.dcn_bwd(c["x"], c["w"], c["b"], c["g"])
    c.update(want=dict(y=y, s=s, dx=dx, dw=dw, db=db))
    for a in list(c["want"].values()) + [c[k] for k in "xwbg"]:
        a.setflags(write=False)
    return c


def check_case(B, D, L):
    c = dcn_case(B, D, L)
    got = run_dcn(c["x"], c["w"], c["b"], c["g"])
    errs = {k: rel(got[k].view(np.float32), c["want"][k]) for k in ("y", "s", "dx", "dw", "db")}
    print("B=%d D=%d L=%d (%s / %s): " % (B, D, L, *dc.dcn_paths(D, L)[:2]) + ", ".join("%s %.2e" % kv for kv in errs.items()))
    bad = {k: e for k, e in errs.items() if not (np.isfinite(e) and e <= TOL)}
    assert not bad, "B=%d D=%d L=%d: norm-relative error above %.0e: %s" % (B, D, L, TOL, bad)
    return got


# ------------------------------------------------------------------------------------------------ 1. menu and path cases
@pytest.mark.parametrize("B,D,L", list(dc.PATH_CASES), ids=["%d-%d-%d" % c for c in dc.PATH_CASES])
def test_dcn_path_and_menu_cases(B, D, L):
    fwd, bwd, npl, vec = dc.PATH_CASES[(B, D, L)]
    p = dc.dcn_paths(D, L)
    assert (p.fwd, p.bwd, p.npl, p.vec) == (fwd, bwd, npl, vec), p
    assert p.lm == (16 if L > 6 else 6)
    if (D, L) == (512, 6):
        assert 64 * npl == D and L == dc.DCN_MAX_L                                         # no masked lane, the deepest register backward
    if (D, L) == (516, 4):
        assert (L + 7) * npl == 220 and (L + 8) * npl > 230 and D // 4 == 129                # the limit for npl 20; 129 of 320 chunks live
    if (D, L) == (516, 5):
        assert (L + 7) * npl == 240
    if D in (1280, 2048, 4096):
        assert 64 * npl == D
    if D in (513, 516, 1281, 1284, 2052):
        below = {513: 512, 516: 512, 1281: 1280, 1284: 1280, 2052: 2048}[D]               # just past the previous menu entry
        assert dc.pick_npl(below, True) < npl and D - below <= 4
    if (D, L) == (4096, 5):
        assert 2 * L * D * 4 == dc.DCN_LDS_LIMIT and dc.dcn_paths(D, L + 1).fwd == "generic"
    if D < 4:
        assert not vec
    # at most one sample per wave whatever FIL_DCN_GRID is (B = 9 at two workgroups: one forward wave takes two); the loops of these
    # instantiations are test_dcn_menu_cases_with_a_ragged_batch's
    assert B <= 8 * dc.grid_bwd(B) and B <= 4 * dc.grid_fwd(B) + 1
    check_case(B, D, L)                              # (run_dcn holds the workspace size to the formula of p.bwd)


def walk_id(D, L):
    return "37-%d-%d-walk" % (D, L)


@pytest.mark.parametrize("D,L", dc.MENU_WALK_DL, ids=[walk_id(*c) for c in dc.MENU_WALK_DL])
def test_dcn_menu_cases_with_a_ragged_batch(D, L):
    """Every (D, L) of the path cases that has a register-resident direction, at B = 37.  Under FIL_DCN_GRID=2 (the child of
    tests/test_gpu_knobs.py) the register backward has 16 waves for 37 samples: five waves walk three samples and eleven walk two
    through the prefetch chain (`more` true, then the empty descriptors), and the forward's 8 waves loop five or four times -- at every
    menu instantiation.  Without the knob every wave has at most one sample."""
    B = dc.MENU_WALK_B
    p = dc.dcn_paths(D, L)
    assert "register" in (p.fwd, p.bwd) and (B, D, L) not in dc.PATH_CASES
    waves_b, waves_f = 8 * dc.grid_bwd(B), 4 * dc.grid_fwd(B)
    if dc.forced_grid() == 2:
        assert (waves_b, waves_f) == (16, 8)
        assert B > 2 * waves_b and B % waves_b == 5                  # backward: 5 waves take 3 samples, 11 take 2
        assert B > 4 * waves_f and B % waves_f == 5                  # forward: 5 waves take 5 samples, 3 take 4
    elif not dc.forced_grid():
        assert waves_b >= B and waves_f >= B
    check_case(B, D, L)


# ------------------------------------------------------------------------------------------------ 2. grid and reduction cases
def knob_id(B):
    return "-le257" if B <= dc.KNOB_MAX_B else ""


@pytest.mark.parametrize("B", list(dc.REG_GRID_B), ids=["B%d%s" % (B, knob_id(B)) for B in dc.REG_GRID_B])
@pytest.mark.parametrize("D", dc.REG_GRID_D, ids=["D%d" % D for D in dc.REG_GRID_D])
def test_dcn_register_grid_cases(D, B):
    """Register-resident both ways, L = 2: the partials of dcn_reduce_closed_kernel around its stride of 32 and its four waves, and the
    two grid-stride loops with waves of unequal trip counts."""
    L = dc.REG_GRID_L
    p = dc.dcn_paths(D, L)
    assert (p.fwd, p.bwd, p.npl, p.vec) == ("register", "register", 8, True)
    forced = dc.forced_grid()
    parts = dc.REG_GRID_B[B]
    assert dc.grid_bwd(B) == (min(parts, forced) if forced else parts)
    if not forced:
        waves_b, waves_f = 8 * dc.grid_bwd(B), 4 * dc.grid_fwd(B)
        if B == 2053:
            assert waves_b == 2048 and B - waves_b == 5 and waves_f >= B        # 5 backward waves take two samples, 2043 take one
        if B == 4101:
            assert waves_f == 4096 and B - waves_f == 5                          # 5 forward waves take two samples
            assert dc.cdiv(B, waves_b) == 3 and B - 2 * waves_b == 5             # backward: 5 waves take three, the others two
        if B <= 2048:
            assert waves_b >= B and waves_f >= B
    if D == 68:
        assert dc.cdiv(D, 64) == 2 and D % 64 == 4
    check_case(B, D, L)


@pytest.mark.parametrize("B", list(dc.GEN_GRID_B), ids=["B%d%s" % (B, knob_id(B)) for B in dc.GEN_GRID_B])
def test_dcn_generic_grid_cases(B):
    """Generic both ways (L = 7): the partials of dcn_reduce_kernel (pairs of four waves' strides and one tail), a ragged last chunk, and
    the grid-stride loops of the two scalars kernels."""
    D, L = dc.GEN_GRID_D, dc.GEN_GRID_L
    p = dc.dcn_paths(D, L)
    assert (p.fwd, p.bwd, p.lm) == ("generic", "generic", 16)
    parts, last = dc.generic_parts(B)
    assert parts == dc.GEN_GRID_B[B]
    if B == 2100:
        assert (parts, last) == (64, 21) and dc.cdiv(B, dc.generic_chunks(B)) == 33        # ragged last chunk
        assert dc.cdiv(B, 4) > 512                                                        # the forward scalars kernel strides
        assert dc.cdiv(B, 4) <= 2048
    if B == 8200:
        assert dc.cdiv(B, 4) > 2048                                                       # the backward scalars kernel strides
    check_case(B, D, L)


# ------------------------------------------------------------------------------------------------ 3. containment
@pytest.mark.parametrize("B,D,L", dc.CONTAIN_CASES)
def test_dcn_rows_do_not_depend_on_their_position_or_neighbours(B, D, L):
    """y, s and dx of the first n rows are bit-equal whether the call saw B rows or only those n (other grids, other waves, other trip
    counts), and a sample whose x holds NaN, +Inf and -Inf leaves every other row of y, s and dx bit-equal to the clean run while its own
    rows are non-finite.  (dw and db sum over the samples: not asserted for the poisoned run.)"""
    c = dcn_case(B, D, L)
    full = check_case(B, D, L)
    n = B // 2 + 3
    assert n % 8 and n % 32 and n % dc.cdiv(B, dc.generic_chunks(B))                      # cuts a workgroup's samples and a chunk
    part = run_dcn(c["x"][:n], c["w"], c["b"], c["g"][:n])
    for k in ("y", "s", "dx"):
        assert np.array_equal(part[k], full[k][:n]), "%s of the first %d rows depends on the batch size" % (k, n)
    bad = B - 3                                                                           # (2053: one of the second samples of a wave)
    x = c["x"].copy()
    x[bad, 0], x[bad, D // 2], x[bad, D - 1] = np.nan, np.inf, -np.inf
    got = run_dcn(x, c["w"], c["b"], c["g"])
    others = np.arange(B) != bad
    for k in ("y", "s", "dx"):
        assert np.array_equal(got[k][others], full[k][others]), "%s: the non-finite sample %d reached rows %s" % (
            k, bad, np.nonzero((got[k] != full[k]).any(1) & others)[0][:8])
        assert not np.isfinite(got[k].view(np.float32)[bad]).any(), k
