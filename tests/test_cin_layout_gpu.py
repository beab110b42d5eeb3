"""The sizes fil_cin_saved_bytes / fil_cin_fwd_workspace_bytes / fil_cin_bwd_workspace_bytes report are the bytes fil_cin_fwd[_p] /
fil_cin_bwd[_p] touch: `saved` and both workspaces at EXACTLY the reported byte counts inside sentinel-filled allocations (a guard
behind each, one in front of `saved` as well; every base 256-byte aligned), every output a tests/guarded.py GuardedOutput.  After
forward + backward every guard holds its bits, and the outputs equal, bit for bit, those of the same call made through
functional.cin_forward_raw / cin_backward_raw on ordinary allocations (the library is deterministic:
tests/test_gpu_parity.py::test_cin_repeatable_and_batch_independent).  One small case per layout variant of csrc/cin.hip
(plain, fused tail, quadratic tail) and per path through the two launchers."""
import ctypes

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, synth
from ml_function_amd._lib import check, int_array, stream_ptr
from tests import guarded as G

pytestmark = pytest.mark.gpu

X_TRANSPOSED = 16                          # fil.h FIL_CIN_X_TRANSPOSED
PREC_F32, PREC_BF16 = 0, 1
NORTH = (64, 39, 16, [128, 128, 128])

CASES = [
    ((5, 3, 4, [5]), 0, "f32"),                      # one layer: the last-layer shortcut on x itself
    ((9, 5, 8, [6, 7]), 0, "f32"),                   # pair-symmetric first layer + shortcut
    ((9, 5, 8, [6, 7]), 1, "f32"),                   # general kernels throughout
    ((16, 26, 16, [200, 200]), 0, "f32"),            # two column chunks
    ((9, 5, 8, [6, 7, 5]), 64, "f32"),               # merged quadratic tail
    ((9, 5, 8, [6, 7, 5]), 64 | 512, "f32"),         # quadratic tail, two launches per direction
    ((9, 5, 8, [6, 7, 5]), 64 | 256, "f32"),         # fused tail
    ((9, 5, 8, [6, 7, 5]), 64 | 8, "f32"),           # fused tail above a general first layer
    ((3, 4, 2, [3, 3, 3, 3]), 64, "f32"),            # general layers under the fused tail
    ((4, 64, 2, [3, 3, 3]), 64, "f32"),              # tail unsupported: plain layout
    (NORTH, 64, "f32"),                              # merged quadratic tail on its 256-column / two-pass kernels
    (NORTH, 64 | 2, "f32"),                          # ... on split-bf16 operands
    (NORTH, 64, "bf16"),                             # ... on one bf16 plane per operand
    ((9, 5, 8, [6, 7, 5]), 64 | X_TRANSPOSED, "f32"),
]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def guarded(shape, name):
    return G.GuardedOutput(shape, np.uint32, name)


class GuardedBytes:
    """nbytes of a uint8 allocation filled with G.WS_FILL, G.GUARD_BYTES of guard in front and behind."""

    def __init__(self, nbytes, name):
        self.n, self.name = int(nbytes), name
        self.t = torch.full((2 * G.GUARD_BYTES + self.n,), G.WS_FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + G.GUARD_BYTES
        assert self.ptr % 256 == 0

    def assert_guards(self, what):
        w = self.t.cpu().numpy()
        stray = np.nonzero(np.concatenate([w[:G.GUARD_BYTES], w[G.GUARD_BYTES + self.n:]]) != G.WS_FILL)[0]
        assert stray.size == 0, "%s: %d guard bytes around the %d bytes of %s were written (guard byte indices %s; %d = first byte behind)" % (
            what, stray.size, self.n, self.name, stray[:8], G.GUARD_BYTES)


def words(t):
    return None if t is None else G.f32_words(t.detach().cpu().numpy())


def _case_id(v):
    return "B%d-F%d-K%d-H%s" % (v[0], v[1], v[2], "x".join(map(str, v[3]))) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape,mode,precision", CASES, ids=_case_id)
def test_reported_sizes_are_the_touched_bytes(shape, mode, precision):
    from ml_function_amd import functional as Fn
    B, F, K, H = shape
    L, M = len(H), B * K
    what = "B=%d F=%d K=%d H=%s mode=%d %s" % (B, F, K, H, mode, precision)
    lib = _lib.load()
    Harr = int_array(H)
    prec = PREC_BF16 if precision == "bf16" else PREC_F32
    if prec == PREC_BF16:
        assert lib.fil_cin_precision_used(B, F, K, L, Harr, mode, PREC_BF16) == PREC_BF16, what
    c = synth.cin_case(B, F, K, H, dist="uniform")
    c["x"] = (c["x"] * 10).astype(np.float32)
    x, Ws, bs, dw, db, g = dev(c["x"]), [dev(w) for w in c["Ws"]], [dev(b) for b in c["bs"]], dev(c["dense_w"]), dev(c["dense_b"]), dev(c["g"])
    xt = x.permute(0, 2, 1).reshape(M, F).contiguous() if mode & X_TRANSPOSED else None
    xin = xt if xt is not None else x
    Wp, bp = _lib.ptr_array(Ws), _lib.ptr_array(bs)

    # the same call on ordinary allocations
    ref_out, ref_pooled, ref_saved = Fn.cin_forward_raw(x, Ws, bs, dw, db, 1, mode & ~X_TRANSPOSED, xt=xt, precision=precision)
    ref = Fn.cin_backward_raw(x, Ws, bs, dw, ref_pooled, ref_saved, g, 1, mode & ~X_TRANSPOSED, xt=xt, precision=precision)
    want = dict(out=words(ref_out), pooled=words(ref_pooled), dx=words(ref["dx"]), ddw=words(ref["ddw"]), ddb=words(ref["ddb"]))
    for l in range(L):
        want["dW%d" % l], want["db%d" % l] = words(ref["dW"][l]), words(ref["db"][l])

    nsv, nfw, nbw = (fn(B, F, K, L, Harr) for fn in (lib.fil_cin_saved_bytes, lib.fil_cin_fwd_workspace_bytes, lib.fil_cin_bwd_workspace_bytes))
    assert nsv > 0 and nfw > 0 and nbw > 0, what
    saved, fws, bws = GuardedBytes(nsv, "saved"), GuardedBytes(nfw, "the forward workspace"), GuardedBytes(nbw, "the backward workspace")
    out, pooled = guarded((B, 1), "out"), guarded((B, L * K), "pooled")
    if prec == PREC_F32:
        check(lib.fil_cin_fwd(xin.data_ptr(), Wp, bp, dw.data_ptr(), db.data_ptr(), out.ptr, pooled.ptr, saved.ptr, B, F, K, L, Harr, 1, mode,
                              fws.ptr, nfw, stream_ptr()), "fil_cin_fwd")
    else:
        check(lib.fil_cin_fwd_p(xin.data_ptr(), Wp, bp, dw.data_ptr(), db.data_ptr(), out.ptr, pooled.ptr, saved.ptr, B, F, K, L, Harr, 1, mode, prec,
                                fws.ptr, nfw, stream_ptr()), "fil_cin_fwd_p")
    got = dict(out=out.read(what), pooled=pooled.read(what))
    saved.assert_guards(what + " (forward)")
    fws.assert_guards(what)

    dx, ddw, ddb = guarded((B, F, K), "dx"), guarded((L * K, 1), "ddense_w"), guarded((1,), "ddense_b")
    dWs = [guarded(tuple(w.shape), "dW[%d]" % l) for l, w in enumerate(Ws)]
    dbs = [guarded((H[l],), "dbias[%d]" % l) for l in range(L)]
    dWp = (ctypes.c_void_p * L)(*[o.ptr for o in dWs])
    dbp = (ctypes.c_void_p * L)(*[o.ptr for o in dbs])
    pooled_in = torch.from_numpy(got["pooled"].view(np.float32)).cuda()
    if prec == PREC_F32:
        check(lib.fil_cin_bwd(xin.data_ptr(), Wp, bp, dw.data_ptr(), pooled_in.data_ptr(), saved.ptr, g.data_ptr(), dx.ptr, dWp, dbp, ddw.ptr, ddb.ptr,
                              B, F, K, L, Harr, 1, mode, None, bws.ptr, nbw, stream_ptr()), "fil_cin_bwd")
    else:
        check(lib.fil_cin_bwd_p(xin.data_ptr(), Wp, bp, dw.data_ptr(), pooled_in.data_ptr(), saved.ptr, g.data_ptr(), dx.ptr, dWp, dbp, ddw.ptr, ddb.ptr,
                                B, F, K, L, Harr, 1, mode, prec, None, bws.ptr, nbw, stream_ptr()), "fil_cin_bwd_p")
    got.update(dx=dx.read(what), ddw=ddw.read(what), ddb=ddb.read(what))
    for l in range(L):
        got["dW%d" % l], got["db%d" % l] = dWs[l].read(what), dbs[l].read(what)
    saved.assert_guards(what + " (backward)")
    bws.assert_guards(what)

    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %s differs from the call on ordinary allocations in %d of %d words" % (
            what, k, int((got[k] != want[k]).sum()), want[k].size)
