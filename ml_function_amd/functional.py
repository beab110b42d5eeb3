"""torch.autograd.Function wrappers over the C ABI (include/fil.h).

Every function requires CUDA tensors and the HIP library; there is no eager/CPU fallback (the oracle lives
in oracle/ and is test infrastructure only).  Tensors are made contiguous; dtypes are fp32 unless noted.
"""
import ctypes

import os

import time
import weakref

import torch

from . import _lib
from ._lib import FIL_BF16, FIL_F32, FilError, check, int_array, ptr, ptr_array, stream_ptr
from .optim import deferred_state


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FilError("ml_function_amd runs on the GPU only (got a %s tensor); there is no CPU fallback"
                           % t.device.type)


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise FilError("expected float32, got %s" % t.dtype)
    return t.contiguous()


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# Scratch workspaces (NOT the `saved` buffers, which live until the backward) are kept per (device, stream, call site) and only ever
# grow: consecutive calls on one stream are ordered by the stream, so they can share the bytes, and a layer call no longer pays an
# allocator round trip per direction.  Under stream capture the cache is left alone (a block allocated there belongs to the graph's
# private pool): the call allocates as before.
_WS_CACHE = {}
_WS_LAST_USE = {}      # (device, stream) -> monotonic time of the last _scratch() call on that stream
_WS_IDLE_S = 2.0       # another stream's workspaces are dropped once that stream has not asked for scratch for this long


def _scratch(nbytes, device, tag):
    nbytes = max(int(nbytes), 256)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    cur = stream_ptr()
    key = (device, cur, tag)
    now = time.monotonic()
    _WS_LAST_USE[(device, cur)] = now
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        # a (re)allocation is also the moment to let go of what IDLE streams of this device left behind: warm-up side streams
        # (capture_step, bench.py) would otherwise keep hundreds of MB at headline shapes alive for good, invisible to
        # torch.cuda.empty_cache().  A stream that is still in use (two model replicas on two streams, a side-stream warm-up
        # followed by main-stream eager steps) keeps its workspaces: only streams that have not asked for scratch for _WS_IDLE_S
        # are evicted, so two live streams no longer free each other's hot buffers on every call.  Work still queued on an
        # evicted stream keeps its bytes: the caching allocator does not hand a block out again before the stream it was
        # allocated on has passed the free.
        for k in [k for k in _WS_CACHE if k[0] == device and k[1] != cur and now - _WS_LAST_USE.get((k[0], k[1]), 0.0) > _WS_IDLE_S]:
            del _WS_CACHE[k]
        ws = _WS_CACHE[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def release_scratch():
    """Drop every cached scratch workspace (they are re-created on demand)."""
    _WS_CACHE.clear()
    _WS_LAST_USE.clear()


def _partials_scratch(entry, tag, wanted, device, *dims):
    """(workspace, bytes) for the parameter-gradient partials of a tiled backward: what the library's `entry`
    (fil_*_bwd_workspace_bytes) asks for at `dims`, from _scratch under `tag` -- or (None, 0) when no parameter gradient is wanted
    (the kernel then skips the partials and the library is not asked)."""
    if not wanted:
        return None, 0
    nws = getattr(_lib.load(), entry)(*dims)
    return _scratch(nws, device, tag), nws


def _saved_floats(nbytes, device):
    """The fp32 `saved` buffer a forward hands to its backward, for the byte count the library's fil_*_saved_bytes gave."""
    return torch.empty(max(int(nbytes), 256) // 4, dtype=torch.float32, device=device)


def _grad(want, shape, device):
    """An uninitialised fp32 gradient of `shape`, or None when it is not wanted (the kernels skip a null output)."""
    return torch.empty(shape, dtype=torch.float32, device=device) if want else None


def _no_samples(B, *param_grads):
    """True for the backward of an empty batch.  The library answers B == 0 with a no-op that writes nothing, so the parameter
    gradients -- sums over no sample -- are zeroed here (they came uninitialised from _grad) and the library is not called; the input
    gradients are empty as they are."""
    if B > 0:
        return False
    for t in param_grads:
        if t is not None:
            t.zero_()
    return True


def _save(ctx, *tensors):
    """ctx.save_for_backward of the tensors that are there (so autograd's version check covers every one of them); which places
    were None is kept on ctx for _saved."""
    ctx.saved_places = tuple(t is not None for t in tensors)
    ctx.save_for_backward(*[t for t in tensors if t is not None])


def _saved(ctx):
    """What _save was given, in its order: the saved tensors with None back in the places that were None."""
    it = iter(ctx.saved_tensors)
    return tuple(next(it) if there else None for there in ctx.saved_places)


# --------------------------------------------------------------------------------------------- A1  FM
class _FmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, lin):
        _require_cuda(emb, lin)
        if emb.dtype not in (torch.float32, torch.bfloat16):
            raise FilError("fm: emb must be float32 or bfloat16, got %s" % emb.dtype)
        emb = emb.contiguous()
        lin = None if lin is None else _f32c(lin.float() if lin.dtype != torch.float32 else lin)
        B, F, K = emb.shape
        if lin is not None and tuple(lin.shape) != (B, lin.shape[1]):
            raise FilError("fm: lin must be [B, n_linear]")
        out = torch.empty((B, K), dtype=emb.dtype, device=emb.device)
        dt = FIL_F32 if emb.dtype == torch.float32 else FIL_BF16
        lib = _lib.load()
        if lin is not None and lin.shape[1] != F:
            # the reference's Add takes any number of [B,1,1] linear terms; the kernel sums F columns
            lin_k = torch.zeros((B, F), dtype=torch.float32, device=emb.device)
            lin_k[:, 0] = lin.sum(1)
        else:
            lin_k = lin
        check(lib.fil_fm_fwd(ptr(emb), ptr(lin_k), ptr(out), B, F, K, dt, stream_ptr()), "fil_fm_fwd")
        ctx.save_for_backward(emb)
        ctx.lin_shape = None if lin is None else tuple(lin.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (emb,) = ctx.saved_tensors
        B, F, K = emb.shape
        g = g.to(emb.dtype).contiguous()
        demb = torch.empty_like(emb)
        dlin_k = None
        if ctx.lin_shape is not None and ctx.needs_input_grad[1]:
            dlin_k = torch.empty((B, F), dtype=torch.float32, device=emb.device)
        dt = FIL_F32 if emb.dtype == torch.float32 else FIL_BF16
        check(_lib.load().fil_fm_bwd(ptr(emb), ptr(g), ptr(demb), ptr(dlin_k), B, F, K, dt, stream_ptr()), "fil_fm_bwd")
        dlin = None
        if dlin_k is not None:
            n = ctx.lin_shape[1]
            dlin = dlin_k if n == F else dlin_k[:, :1].expand(B, n).contiguous()
        return demb, dlin


def fm(emb, lin=None):
    """emb [B,F,K] (fp32/bf16), lin [B,n] fp32 or None -> [B,K]: sum_{i<j} e_i*e_j + sum of linear terms."""
    return _FmFn.apply(emb, lin)


class _FmPairsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb):
        _require_cuda(emb)
        emb = _f32c(emb)
        B, F, K = emb.shape
        pairs = torch.empty((B, F * (F - 1) // 2, K), dtype=torch.float32, device=emb.device)
        check(_lib.load().fil_fm_pairs_fwd(ptr(emb), ptr(pairs), B, F, K, stream_ptr()), "fil_fm_pairs_fwd")
        ctx.save_for_backward(emb)
        return pairs

    @staticmethod
    def backward(ctx, gp):
        (emb,) = ctx.saved_tensors
        B, F, K = emb.shape
        demb = torch.empty_like(emb)
        check(_lib.load().fil_fm_pairs_bwd(ptr(emb), ptr(_f32c(gp)), ptr(demb), B, F, K, stream_ptr()), "fil_fm_pairs_bwd")
        return demb


def fm_pairs(emb):
    """emb [B,F,K] -> [B, F(F-1)/2, K] pair products in itertools.combinations order."""
    return _FmPairsFn.apply(emb)


def _tiled_plan(name, *dims):
    """The answer of the fil_*_plan entry point `name` for `dims`, as the dict of afm_plan / din_plan / gru_plan / seq_attn_plan."""
    plan = (ctypes.c_int * 8)()
    rc = getattr(_lib.load(), name)(*dims, plan)
    if rc == _lib.FIL_ERR_UNSUPPORTED:
        return dict(fits=False)
    check(rc, name)
    return dict(fits=bool(plan[0]) and bool(plan[1]), tile=plan[2], grid=plan[3], cap=plan[4], partials=plan[5], lds_fwd=plan[6],
                lds_bwd=plan[7])


def _seq_mask(who, mask, B, T):
    """The [B,T] bool / uint8 mask of a behaviour-sequence op as the contiguous uint8 tensor the kernels read (None stays None)."""
    if mask is None:
        return None
    if tuple(mask.shape) != (B, T) or mask.dtype not in (torch.bool, torch.uint8):
        raise FilError("%s: mask must be a [B,T] bool or uint8 tensor, got %s %s" % (who, tuple(mask.shape), mask.dtype))
    return (mask.to(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()


class _AfmPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, w, b, h, hidden_relu):
        _require_cuda(emb, w, b, h)
        emb, w, b, h = _f32c(emb), _f32c(w), _f32c(b), _f32c(h)
        if emb.dim() != 3 or w.dim() != 2 or w.shape[0] != emb.shape[2]:
            raise FilError("afm_pool: emb must be [B,F,K] and w [K,A], got %s and %s" % (tuple(emb.shape), tuple(w.shape)))
        B, F, K = emb.shape
        A = w.shape[1]
        if b.numel() != A or h.numel() != A:
            raise FilError("afm_pool: b must be [A] and h [A,1] with A = %d, got %s and %s" % (A, tuple(b.shape), tuple(h.shape)))
        flags = _lib.FIL_AFM_HIDDEN_RELU if hidden_relu else 0
        pooled = torch.empty((B, K), dtype=torch.float32, device=emb.device)
        stats = torch.empty((B, 2), dtype=torch.float32, device=emb.device)
        check(_lib.load().fil_afm_fwd(ptr(emb), ptr(w), ptr(b), ptr(h), ptr(pooled), ptr(stats), B, F, K, A, flags, stream_ptr()),
              "fil_afm_fwd")
        ctx.save_for_backward(emb, w, b, h, pooled, stats)
        ctx.flags = flags
        ctx.shapes = (tuple(b.shape), tuple(h.shape))
        return pooled

    @staticmethod
    def backward(ctx, g):
        emb, w, b, h, pooled, stats = ctx.saved_tensors
        B, F, K = emb.shape
        A = w.shape[1]
        need = ctx.needs_input_grad
        if not any(need[:4]):
            return None, None, None, None, None
        lib = _lib.load()
        dev = emb.device
        demb = _grad(need[0], emb.shape, dev)
        dw = _grad(need[1], w.shape, dev)
        db = _grad(need[2], ctx.shapes[0], dev)
        dh = _grad(need[3], ctx.shapes[1], dev)
        if _no_samples(B, dw, db, dh):
            return demb, dw, db, dh, None
        ws, nws = _partials_scratch("fil_afm_bwd_workspace_bytes", "afm_bwd", need[1] or need[2] or need[3], dev, B, F, K, A)
        check(lib.fil_afm_bwd(ptr(emb), ptr(w), ptr(b), ptr(h), ptr(pooled), ptr(stats), ptr(_f32c(g)), ptr(demb), ptr(dw), ptr(db),
                              ptr(dh), ptr(ws), nws, B, F, K, A, ctx.flags, stream_ptr()), "fil_afm_bwd")
        return demb, dw, db, dh, None


def afm_pool(emb, w, b, h, hidden_relu=False):
    """AFM's attention pooling with the softmax over the PAIRS (extension; include/fil.h fil_afm_*): emb [B,F,K], w [K,A], b [A],
    h [A,1] (or [A]) -> [B,K] = sum_p softmax_p(s)_p e_i * e_j over the pairs p = (i, j), i < j, with s_p = relu((x_p w + b) . h)
    (the reference's op order) or, hidden_relu=True, relu(x_p w + b) . h (the paper's form).  One launch per direction (plus the small
    fixed-order sum of the parameter-gradient partials); no [B,P,K] tensor exists.  Shapes outside the kernel menu raise FilError
    (layers.AFMLayer takes its composed path there)."""
    return _AfmPoolFn.apply(emb, w, b, h, bool(hidden_relu))


def afm_plan(B, F, K, A):
    """fil_afm_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a shape
    outside the kernel menu."""
    return _tiled_plan("fil_afm_plan", int(B), int(F), int(K), int(A))


DIN_ACTIVATIONS = ("prelu", "sigmoid")


def _din_flags(softmax, activation):
    if activation not in DIN_ACTIVATIONS:
        raise ValueError("din_attention: activation %r (%s)" % (activation, ", ".join(DIN_ACTIVATIONS)))
    return (_lib.FIL_DIN_SOFTMAX if softmax else 0) | (_lib.FIL_DIN_SIGMOID if activation == "sigmoid" else 0)


class _DinAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, keys, mask, w1, b1, alpha1, w2, b2, alpha2, w3, b3, flags):
        _require_cuda(q, keys, mask, w1, b1, alpha1, w2, b2, alpha2, w3, b3)
        q, keys, w1, b1, alpha1, w2, b2, alpha2, w3, b3 = (_f32c(t) for t in (q, keys, w1, b1, alpha1, w2, b2, alpha2, w3, b3))
        if q.dim() != 2 or keys.dim() != 3 or keys.shape[0] != q.shape[0] or keys.shape[2] != q.shape[1]:
            raise FilError("din_attention: q must be [B,K] and keys [B,T,K], got %s and %s" % (tuple(q.shape), tuple(keys.shape)))
        B, T, K = keys.shape
        if w1.dim() != 2 or w1.shape[0] != 4 * K or w2.dim() != 2 or w2.shape[0] != w1.shape[1]:
            raise FilError("din_attention: w1 must be [4K,H1] and w2 [H1,H2] with K = %d, got %s and %s" % (K, tuple(w1.shape), tuple(w2.shape)))
        H1, H2 = w1.shape[1], w2.shape[1]
        sig = bool(flags & _lib.FIL_DIN_SIGMOID)
        for name, t, n in (("b1", b1, H1), ("alpha1", alpha1, H1), ("b2", b2, H2), ("alpha2", alpha2, H2), ("w3", w3, H2), ("b3", b3, 1)):
            if t is None:
                if not (sig and name.startswith("alpha")):
                    raise FilError("din_attention: %s is None (only alpha1 / alpha2 may be, with the sigmoid)" % name)
            elif t.numel() != n:
                raise FilError("din_attention: %s must hold %d values, got %s" % (name, n, tuple(t.shape)))
        mask = _seq_mask("din_attention", mask, B, T)
        out = torch.empty((B, K), dtype=torch.float32, device=q.device)
        stats = torch.empty((B, T + 2), dtype=torch.float32, device=q.device)
        check(_lib.load().fil_din_fwd(ptr(q), ptr(keys), ptr(mask), ptr(w1), ptr(b1), ptr(alpha1), ptr(w2), ptr(b2), ptr(alpha2), ptr(w3),
                                      ptr(b3), ptr(out), ptr(stats), B, T, K, H1, H2, flags, stream_ptr()), "fil_din_fwd")
        _save(ctx, q, keys, mask, w1, b1, alpha1, w2, b2, alpha2, w3, b3, out, stats)
        ctx.flags = flags
        ctx.shapes = {n: tuple(t.shape) for n, t in (("b1", b1), ("alpha1", alpha1), ("b2", b2), ("alpha2", alpha2), ("w3", w3), ("b3", b3))
                      if t is not None}
        return out

    @staticmethod
    def backward(ctx, g):
        q, keys, mask, w1, b1, alpha1, w2, b2, alpha2, w3, b3, out, stats = _saved(ctx)
        B, T, K = keys.shape
        H1, H2 = w1.shape[1], w2.shape[1]
        need = ctx.needs_input_grad
        none = (None,) * 12
        if not any(need):
            return none
        dev, shapes = q.device, ctx.shapes
        dq = _grad(need[0], q.shape, dev)
        dkeys = _grad(need[1], keys.shape, dev)
        dw1 = _grad(need[3], w1.shape, dev)
        db1 = _grad(need[4], shapes["b1"], dev)
        da1 = _grad(need[5] and alpha1 is not None, shapes.get("alpha1"), dev)      # a slope that was None gets no gradient
        dw2 = _grad(need[6], w2.shape, dev)
        db2 = _grad(need[7], shapes["b2"], dev)
        da2 = _grad(need[8] and alpha2 is not None, shapes.get("alpha2"), dev)
        dw3 = _grad(need[9], shapes["w3"], dev)
        db3 = _grad(need[10], shapes["b3"], dev)
        if _no_samples(B, dw1, db1, da1, dw2, db2, da2, dw3, db3):
            return dq, dkeys, None, dw1, db1, da1, dw2, db2, da2, dw3, db3, None
        lib = _lib.load()
        ws, nws = _partials_scratch("fil_din_bwd_workspace_bytes", "din_bwd",
                                    any(t is not None for t in (dw1, db1, da1, dw2, db2, da2, dw3, db3)), dev, B, T, K, H1, H2)
        check(lib.fil_din_bwd(ptr(q), ptr(keys), ptr(mask), ptr(w1), ptr(b1), ptr(alpha1), ptr(w2), ptr(b2), ptr(alpha2), ptr(w3), ptr(b3),
                              ptr(out), ptr(stats), ptr(_f32c(g)), ptr(dq), ptr(dkeys), ptr(dw1), ptr(db1), ptr(da1), ptr(dw2), ptr(db2),
                              ptr(da2), ptr(dw3), ptr(db3), ptr(ws), nws, B, T, K, H1, H2, ctx.flags, stream_ptr()), "fil_din_bwd")
        return dq, dkeys, None, dw1, db1, da1, dw2, db2, da2, dw3, db3, None


def din_attention(q, keys, mask, W1, b1, alpha1, W2, b2, alpha2, w3, b3, softmax=False, activation="prelu"):
    """The Deep Interest Network's attention pooling of a behaviour sequence (extension: the paper's activation unit; the reference's
    AttentionUnitLayer / ActivationUnitLayer are not restated, their source was not available; include/fil.h fil_din_*):
    q [B,K] the candidate, keys [B,T,K] the history, mask [B,T] bool / uint8 (non-zero = live; None = all live), W1 [4K,H1], b1, alpha1
    [H1], W2 [H1,H2], b2, alpha2 [H2], w3 [H2] (or [H2,1]), b3 [1] -> [B,K] = sum_t a_t k_t with s_t = act(act([q, k_t, q - k_t, q * k_t]
    W1 + b1) W2 + b2) . w3 + b3 and a_t = s_t on the live slots (the paper) or, softmax=True, the softmax of s over the live slots.
    activation "prelu" (a slope per unit; alpha = 0 without a gradient is ReLU) or "sigmoid" (alpha1 / alpha2 are ignored and may be
    None).  One launch per direction (plus the small fixed-order sum of the parameter-gradient partials); no [B,T,4K] or [B,T,H1]
    tensor exists; only the gradients that are asked for are computed.  GPU only; shapes outside the kernel menu raise FilError
    (layers.DinAttentionLayer takes its composed path there)."""
    return _DinAttentionFn.apply(q, keys, mask, W1, b1, alpha1, W2, b2, alpha2, w3, b3, _din_flags(softmax, activation))


def din_plan(B, T, K, H1, H2):
    """fil_din_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a shape
    outside the kernel menu."""
    return _tiled_plan("fil_din_plan", int(B), int(T), int(K), int(H1), int(H2))


GRU_MODES = {"gru": _lib.FIL_GRU_GRU, "augru": _lib.FIL_GRU_AUGRU, "agru": _lib.FIL_GRU_AGRU}


class _GruFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, mask, w, u, b, mode, return_sequences):
        _require_cuda(x, a, mask, w, u, b)
        x, a, w, u, b = (_f32c(t) for t in (x, a, w, u, b))
        if x.dim() != 3 or w.dim() != 2 or u.dim() != 2 or w.shape[0] != x.shape[2] or u.shape[1] != 3 * u.shape[0] or w.shape[1] != u.shape[1]:
            raise FilError("gru: x must be [B,T,K], W [K,3H] and U [H,3H], got %s, %s and %s" % (tuple(x.shape), tuple(w.shape), tuple(u.shape)))
        B, T, K = x.shape
        H = u.shape[0]
        if tuple(b.shape) != (2, 3 * H):
            raise FilError("gru: b must be [2,3H] with H = %d (input bias, recurrent bias), got %s" % (H, tuple(b.shape)))
        if (mode == _lib.FIL_GRU_GRU) != (a is None):
            raise FilError("gru: the scores a are given in the modes 'augru' and 'agru' and only there")
        if a is not None and tuple(a.shape) != (B, T):
            raise FilError("gru: a must be [B,T], got %s" % (tuple(a.shape),))
        mask = _seq_mask("gru", mask, B, T)
        lib = _lib.load()
        hs = torch.empty((B, T, H), dtype=torch.float32, device=x.device)
        need = ctx.needs_input_grad
        saved = None
        if any(need[i] for i in (0, 1, 3, 4, 5)):
            saved = _saved_floats(lib.fil_gru_saved_bytes(B, T, K, H), x.device)
        check(lib.fil_gru_fwd(ptr(x), ptr(a), ptr(mask), ptr(w), ptr(u), ptr(b), ptr(hs), ptr(saved), B, T, K, H, mode, stream_ptr()),
              "fil_gru_fwd")
        _save(ctx, x, a, mask, w, u, hs, saved)
        ctx.mode, ctx.return_sequences = mode, return_sequences
        if return_sequences:
            return hs
        return hs[:, T - 1].clone() if B > 0 else hs.new_zeros((0, H))

    @staticmethod
    def backward(ctx, g):
        x, a, mask, w, u, hs, saved = _saved(ctx)
        B, T, K = x.shape
        H = u.shape[0]
        need = ctx.needs_input_grad
        none = (None,) * 8
        want_da = need[1] and a is not None      # scores that were None get no gradient
        if not (need[0] or want_da or need[3] or need[4] or need[5]):
            return none
        dev = x.device
        dx = _grad(need[0], x.shape, dev)
        da = _grad(want_da, (B, T), dev)
        dw = _grad(need[3], w.shape, dev)
        du = _grad(need[4], u.shape, dev)
        db = _grad(need[5], (2, 3 * H), dev)
        if _no_samples(B, dw, du, db):
            return dx, da, None, dw, du, db, None, None
        g = _f32c(g)
        g_hs, g_last = (g, None) if ctx.return_sequences else (None, g)
        lib = _lib.load()
        ws, nws = _partials_scratch("fil_gru_bwd_workspace_bytes", "gru_bwd", need[3] or need[4] or need[5], dev, B, T, K, H)
        check(lib.fil_gru_bwd(ptr(x), ptr(a), ptr(mask), ptr(w), ptr(u), ptr(hs), ptr(saved), ptr(g_hs), ptr(g_last), ptr(dx), ptr(da),
                              ptr(dw), ptr(du), ptr(db), ptr(ws), nws, B, T, K, H, ctx.mode, stream_ptr()), "fil_gru_bwd")
        return dx, da, None, dw, du, db, None, None


def gru(x, a, mask, W, U, b, mode="gru", return_sequences=True):
    """A GRU over a behaviour sequence, or the Deep Interest Evolution Network's attention-gated variants (extension; include/fil.h
    fil_gru_*): x [B,T,K], a [B,T] attention scores (None with mode "gru"), mask [B,T] bool / uint8 (non-zero = live; None = all
    live), W [K,3H], U [H,3H] (Keras' column order z | r | h), b [2,3H] (input bias, recurrent bias: Keras' reset_after=True) ->
    hs [B,T,H], or hs[:, -1] [B,H] with return_sequences=False (its gradient then enters the backward as [B,H]: no zero [B,T,H] block
    is made).  mode "gru": Keras' GRU; "augru": the score scales the update gate, u' = a_t (1 - z); "agru": the score replaces it.
    A masked step repeats the state (Keras' masking).  One launch per direction (plus the small fixed-order sum of the
    parameter-gradient partials); only the gradients that are asked for are computed.  GPU only; shapes outside the kernel menu raise
    FilError (layers.GRULayer takes its composed path there)."""
    if mode not in GRU_MODES:
        raise ValueError("gru: mode %r (%s)" % (mode, ", ".join(GRU_MODES)))
    return _GruFn.apply(x, a, mask, W, U, b, GRU_MODES[mode], bool(return_sequences))


def gru_plan(B, T, K, H, mode="gru"):
    """fil_gru_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a shape
    outside the kernel menu."""
    return _tiled_plan("fil_gru_plan", int(B), int(T), int(K), int(H), GRU_MODES[mode])


class _TsGruFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dt, dt_out, mask, w, u, b, wf, bf, steps, return_sequences):
        _require_cuda(x, dt, dt_out, mask, w, u, b, wf, bf)
        x, dt, dt_out, w, u, b, wf, bf = (_f32c(t) for t in (x, dt, dt_out, w, u, b, wf, bf))
        if x.dim() != 3 or w.dim() != 2 or u.dim() != 2 or w.shape[0] != x.shape[2] or u.shape[1] != 3 * u.shape[0] or w.shape[1] != u.shape[1]:
            raise FilError("ts_gru: x must be [B,T,K], W [K,3H] and U [H,3H], got %s, %s and %s" % (tuple(x.shape), tuple(w.shape), tuple(u.shape)))
        B, T, K = x.shape
        H = u.shape[0]
        if tuple(b.shape) != (2, 3 * H):
            raise FilError("ts_gru: b must be [2,3H] with H = %d (input bias, recurrent bias), got %s" % (H, tuple(b.shape)))
        if tuple(wf.shape) != (H, H) or tuple(bf.shape) != (H,):
            raise FilError("ts_gru: Wf and bf must be [H,H] and [H] with H = %d, got %s and %s" % (H, tuple(wf.shape), tuple(bf.shape)))
        if tuple(dt.shape) != (B, T) or (dt_out is not None and tuple(dt_out.shape) != (B,)):
            raise FilError("ts_gru: dt must be [B,T] and dt_out [B] or None, got %s and %s"
                           % (tuple(dt.shape), None if dt_out is None else tuple(dt_out.shape)))
        mask = _seq_mask("ts_gru", mask, B, T)
        lib = _lib.load()
        dev = x.device
        hs = torch.empty((B, T, H), dtype=torch.float32, device=dev)
        z = None if dt_out is None else torch.empty((B, H), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        saved = None
        if any(need[i] for i in (0, 4, 5, 6, 7, 8)):
            saved = _saved_floats(lib.fil_tsgru_saved_bytes(B, T, K, H, steps), dev)
        check(lib.fil_tsgru_fwd(ptr(x), ptr(dt), ptr(dt_out), ptr(mask), ptr(w), ptr(u), ptr(b), ptr(wf), ptr(bf), ptr(hs), ptr(z), ptr(saved),
                                B, T, K, H, steps, stream_ptr()), "fil_tsgru_fwd")
        _save(ctx, x, dt, dt_out, mask, w, u, wf, saved)
        ctx.steps, ctx.return_sequences = steps, return_sequences
        ctx.set_materialize_grads(False)
        out = hs if return_sequences else (hs[:, T - 1].clone() if B > 0 else hs.new_zeros((0, H)))
        return out if z is None else (out, z)

    @staticmethod
    def backward(ctx, g, g_z=None):
        need = ctx.needs_input_grad
        none = (None,) * 11
        if not any(need[i] for i in (0, 4, 5, 6, 7, 8)) or (g is None and g_z is None):
            return none
        x, dt, dt_out, mask, w, u, wf, saved = _saved(ctx)
        B, T, K = x.shape
        H = u.shape[0]
        dev = x.device
        dx = _grad(need[0], x.shape, dev)
        dw = _grad(need[4], w.shape, dev)
        du = _grad(need[5], u.shape, dev)
        db = _grad(need[6], (2, 3 * H), dev)
        dwf = _grad(need[7], (H, H), dev)
        dbf = _grad(need[8], (H,), dev)
        if _no_samples(B, dw, du, db, dwf, dbf):
            return dx, None, None, None, dw, du, db, dwf, dbf, None, None
        g, g_z = _f32c(g), _f32c(g_z)
        g_hs, g_last = (g, None) if ctx.return_sequences else (None, g)
        ws, nws = _partials_scratch("fil_tsgru_bwd_workspace_bytes", "tsgru_bwd", any(need[i] for i in (4, 5, 6, 7, 8)), dev, B, T, K, H,
                                    ctx.steps)
        check(_lib.load().fil_tsgru_bwd(ptr(x), ptr(dt), ptr(dt_out), ptr(mask), ptr(w), ptr(u), ptr(wf), ptr(saved), ptr(g_hs), ptr(g_last),
                                        ptr(g_z), ptr(dx), ptr(dw), ptr(du), ptr(db), ptr(dwf), ptr(dbf), ptr(ws), nws, B, T, K, H, ctx.steps,
                                        stream_ptr()), "fil_tsgru_bwd")
        return dx, None, None, None, dw, du, db, dwf, dbf, None, None


def _ts_steps(who, steps):
    if int(steps) != steps or int(steps) < 1:
        raise ValueError("%s: steps must be a positive integer, got %r" % (who, steps))
    return int(steps)


def ts_gru(x, dt, dt_out, mask, W, U, b, Wf, bf, steps=2, return_sequences=True):
    """A time-stream GRU over a behaviour sequence with event gaps (extension: the core of the Deep Time-Stream model; include/fil.h
    fil_tsgru_*): x [B,T,K], dt [B,T] the time from the previous live event to this one (>= 0, the caller's units), dt_out [B] the
    time from the last event to the prediction or None, mask [B,T] bool / uint8 (non-zero = live; None = all live), W [K,3H], U [H,3H],
    b [2,3H] (Fn.gru's in the mode "gru"), Wf [H,H], bf [H] -> hs [B,T,H] (hs[:, -1] [B,H] with return_sequences=False), and with
    dt_out (hs or last, z [B,H]).  Before each live step the state moves under dh/dt = tanh(h Wf + bf) by `steps` explicit Euler
    substeps of dt / steps, then the GRU step runs on it; z is the last state moved by dt_out in the same way.  A masked step repeats
    the state.  dt and dt_out are data: they get no gradient, and one that requires it raises.  One launch per direction for all
    steps and substeps (plus the small fixed-order sum of the parameter-gradient partials); an output that received no gradient enters
    the backward as NULL and only the gradients that are asked for are computed.  GPU only; shapes outside the kernel menu raise
    FilError (layers.TimeStreamGRULayer takes its composed path there)."""
    steps = _ts_steps("ts_gru", steps)
    for name, t in (("dt", dt), ("dt_out", dt_out)):
        if t is not None and t.requires_grad:
            raise ValueError("ts_gru: %s requires grad -- the gaps are data, there is no gradient to them" % name)
    return _TsGruFn.apply(x, dt, dt_out, mask, W, U, b, Wf, bf, steps, bool(return_sequences))


def ts_gru_plan(B, T, K, H, steps=2):
    """fil_tsgru_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a shape
    outside the kernel menu (more than 8 substeps are outside it too)."""
    return _tiled_plan("fil_tsgru_plan", int(B), int(T), int(K), int(H), _ts_steps("ts_gru_plan", steps))


def ts_gru_graph(x, dt, dt_out, mask, W, U, b, Wf, bf, steps=2, return_sequences=True):
    """ts_gru's math as torch ops on the tensors given (their dtype and device; autograd for the backward), one substep and one step at
    a time: the composed path of TimeStreamGRULayer and the comparator of its benchmark -- about 10 + 4 steps launches per step.
    mask: [B,T] bool or None.  x_t and dt of a masked step are replaced by zero before anything reads them."""
    steps = _ts_steps("ts_gru_graph", steps)
    B, T, K = x.shape
    H = U.shape[0]
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    live = None if mask is None else mask.to(torch.bool)
    if live is not None:
        x = torch.where(live.unsqueeze(-1), x, zero)
        dt = torch.where(live, dt, zero)

    def evolve(h, gap):
        delta = (gap / steps).unsqueeze(-1)
        for _ in range(steps):
            h = h + delta * torch.tanh(torch.matmul(h, Wf) + bf)
        return h

    h = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    out = []
    for t in range(T):
        he = evolve(h, dt[:, t])
        xp = torch.matmul(x[:, t], W) + b[0]
        hp = torch.matmul(he, U) + b[1]
        z = torch.sigmoid(xp[:, :H] + hp[:, :H])
        r = torch.sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
        c = torch.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
        hn = z * he + (1 - z) * c
        h = hn if live is None else torch.where(live[:, t:t + 1], hn, h)
        if return_sequences:
            out.append(h)
    res = torch.stack(out, dim=1) if return_sequences else h
    return res if dt_out is None else (res, evolve(h, dt_out))


LSTM_DIRECTIONS = {"forward": _lib.FIL_LSTM_FORWARD, "reverse": _lib.FIL_LSTM_REVERSE, "bidirectional": _lib.FIL_LSTM_BIDIR}


def _lstm_last(hs, dirs, H):
    """The directions' last states [B, ndir H] from hs [B,T,ndir H]: the forward direction's sits at T - 1, the reverse one's at 0."""
    if dirs == _lib.FIL_LSTM_FORWARD:
        return hs[:, -1].clone()
    if dirs == _lib.FIL_LSTM_REVERSE:
        return hs[:, 0].clone()
    return torch.cat([hs[:, -1, :H], hs[:, 0, H:]], dim=1)


class _LstmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, w, u, b, dirs, return_sequences):
        _require_cuda(x, mask, w, u, b)
        x, w, u, b = (_f32c(t) for t in (x, w, u, b))
        ndir = 2 if dirs == _lib.FIL_LSTM_BIDIR else 1
        lead = (2,) if ndir == 2 else ()
        if x.dim() != 3 or u.dim() != len(lead) + 2:
            raise FilError("lstm: x must be [B,T,K] and U %s, got %s and %s"
                           % ("[2,H,4H]" if lead else "[H,4H]", tuple(x.shape), tuple(u.shape)))
        B, T, K = x.shape
        H = u.shape[-2]
        if tuple(w.shape) != lead + (K, 4 * H) or tuple(u.shape) != lead + (H, 4 * H) or tuple(b.shape) != lead + (4 * H,):
            raise FilError("lstm: W, U and b must be %s with K = %d and H = %d, got %s, %s and %s"
                           % ("[2,K,4H], [2,H,4H] and [2,4H]" if lead else "[K,4H], [H,4H] and [4H]", K, H, tuple(w.shape), tuple(u.shape),
                              tuple(b.shape)))
        mask = _seq_mask("lstm", mask, B, T)
        lib = _lib.load()
        hs = torch.empty((B, T, ndir * H), dtype=torch.float32, device=x.device)
        need = ctx.needs_input_grad
        saved = None
        if any(need[i] for i in (0, 2, 3, 4)):
            saved = _saved_floats(lib.fil_lstm_saved_bytes(B, T, K, H, dirs), x.device)
        check(lib.fil_lstm_fwd(ptr(x), ptr(mask), ptr(w), ptr(u), ptr(b), ptr(hs), ptr(saved), B, T, K, H, dirs, stream_ptr()), "fil_lstm_fwd")
        _save(ctx, x, mask, w, u, hs, saved)
        ctx.dirs, ctx.return_sequences = dirs, return_sequences
        if return_sequences:
            return hs
        return _lstm_last(hs, dirs, H) if B > 0 else hs.new_zeros((0, ndir * H))

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        if not (need[0] or need[2] or need[3] or need[4]):
            return (None,) * 7
        x, mask, w, u, hs, saved = _saved(ctx)
        B, T, K = x.shape
        H = u.shape[-2]
        dev = x.device
        dx = _grad(need[0], x.shape, dev)
        dw = _grad(need[2], w.shape, dev)
        du = _grad(need[3], u.shape, dev)
        db = _grad(need[4], u.shape[:-2] + (4 * H,), dev)
        if _no_samples(B, dw, du, db):
            return dx, None, dw, du, db, None, None
        g = _f32c(g)
        g_hs, g_last = (g, None) if ctx.return_sequences else (None, g)
        # the partials of the parameter gradients, and with both directions in one launch the second direction's dx
        uses_ws = need[2] or need[3] or need[4] or (ctx.dirs == _lib.FIL_LSTM_BIDIR and need[0])
        ws, nws = _partials_scratch("fil_lstm_bwd_workspace_bytes", "lstm_bwd", uses_ws, dev, B, T, K, H, ctx.dirs)
        check(_lib.load().fil_lstm_bwd(ptr(x), ptr(mask), ptr(w), ptr(u), ptr(hs), ptr(saved), ptr(g_hs), ptr(g_last), ptr(dx), ptr(dw),
                                       ptr(du), ptr(db), ptr(ws), nws, B, T, K, H, ctx.dirs, stream_ptr()), "fil_lstm_bwd")
        return dx, None, dw, du, db, None, None


def lstm(x, mask, W, U, b, direction="forward", return_sequences=True):
    """An LSTM over a sequence, in one direction or in both (extension; include/fil.h fil_lstm_*): x [B,T,K], mask [B,T] bool / uint8
    (non-zero = live; None = all live), W [K,4H], U [H,4H] (Keras' column order i | f | c | o), b [4H] -> hs [B,T,H].  direction
    "reverse" walks t = T-1 .. 0 and leaves the state reached after step t at position t (Keras' go_backwards with the output turned
    back); "bidirectional" takes W [2,K,4H], U [2,H,4H], b [2,4H] (forward, reverse) and returns [B,T,2H], the forward direction in
    the first H columns -- both directions run in ONE launch per pass.  With return_sequences=False the result is the directions' last
    states [B, ndir H] (the forward hs[:,T-1], the reverse hs[:,0]); their gradient enters the backward as [B, ndir H]: no zero
    [B,T,.] block is made.  A masked step repeats both states (Keras' masking).  Only the gradients that are asked for are computed.
    GPU only; shapes outside the kernel menu raise FilError (layers.LSTMLayer / BiLSTMLayer take their composed path there)."""
    if direction not in LSTM_DIRECTIONS:
        raise ValueError("lstm: direction %r (%s)" % (direction, ", ".join(LSTM_DIRECTIONS)))
    return _LstmFn.apply(x, mask, W, U, b, LSTM_DIRECTIONS[direction], bool(return_sequences))


def lstm_plan(B, T, K, H, direction="forward"):
    """fil_lstm_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd; grid and cap count the workgroups of one
    direction); fits=False (and nothing else) for a shape outside the kernel menu."""
    return _tiled_plan("fil_lstm_plan", int(B), int(T), int(K), int(H), LSTM_DIRECTIONS[direction])


class _NtmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, mask, wp, bp, m0, return_sequences):
        _require_cuda(h, mask, wp, bp, m0)
        h, wp, bp, m0 = (_f32c(t) for t in (h, wp, bp, m0))
        if h.dim() != 3 or m0.dim() != 2:
            raise FilError("ntm_memory: h must be [B,T,H] and M0 [m,D], got %s and %s" % (tuple(h.shape), tuple(m0.shape)))
        B, T, H = h.shape
        m, D = m0.shape
        if tuple(wp.shape) != (H, 4 * D + 2) or tuple(bp.shape) != (4 * D + 2,):
            raise FilError("ntm_memory: Wp and bp must be [H,4D+2] and [4D+2] with H = %d and D = %d, got %s and %s"
                           % (H, D, tuple(wp.shape), tuple(bp.shape)))
        mask = _seq_mask("ntm_memory", mask, B, T)
        lib = _lib.load()
        dev = h.device
        rs = torch.empty((B, T, D), dtype=torch.float32, device=dev) if return_sequences else None
        r_last = None if return_sequences else torch.empty((B, D), dtype=torch.float32, device=dev)
        mt = torch.empty((B, m, D), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        saved = None
        if any(need[i] for i in (0, 2, 3, 4)):
            saved = _saved_floats(lib.fil_ntm_saved_bytes(B, T, H, m, D), dev)
        check(lib.fil_ntm_fwd(ptr(h), ptr(mask), ptr(wp), ptr(bp), ptr(m0), ptr(rs), ptr(r_last), ptr(mt), ptr(saved), B, T, H, m, D,
                              stream_ptr()), "fil_ntm_fwd")
        _save(ctx, h, mask, wp, saved)
        ctx.return_sequences, ctx.dims = return_sequences, (B, T, H, m, D)
        ctx.set_materialize_grads(False)
        return (rs if return_sequences else r_last), mt

    @staticmethod
    def backward(ctx, g, g_m):
        need = ctx.needs_input_grad
        none = (None,) * 6
        if not (need[0] or need[2] or need[3] or need[4]) or (g is None and g_m is None):
            return none
        h, mask, wp, saved = _saved(ctx)
        B, T, H, m, D = ctx.dims
        dev = h.device
        dh = _grad(need[0], h.shape, dev)
        dwp = _grad(need[2], wp.shape, dev)
        dbp = _grad(need[3], (4 * D + 2,), dev)
        dm0 = _grad(need[4], (m, D), dev)
        if _no_samples(B, dwp, dbp, dm0):
            return dh, None, dwp, dbp, dm0, None
        g, g_m = _f32c(g), _f32c(g_m)
        g_rs, g_last = (g, None) if ctx.return_sequences else (None, g)
        ws, nws = _partials_scratch("fil_ntm_bwd_workspace_bytes", "ntm_bwd", need[2] or need[3] or need[4], dev, B, T, H, m, D)
        check(_lib.load().fil_ntm_bwd(ptr(h), ptr(mask), ptr(wp), ptr(saved), ptr(g_rs), ptr(g_last), ptr(g_m), ptr(dh), ptr(dwp), ptr(dbp),
                                      ptr(dm0), ptr(ws), nws, B, T, H, m, D, stream_ptr()), "fil_ntm_bwd")
        return dh, None, dwp, dbp, dm0, None


def ntm_memory(h, mask, Wp, bp, M0, return_sequences=True):
    """A Neural Turing Machine memory read and written over a sequence (extension: the memory of the Multi-channel user Interest
    Memory Network; include/fil.h fil_ntm_*): h [B,T,H] the controller's states, mask [B,T] bool / uint8 (non-zero = live; None = all
    live), Wp [H,4D+2] and bp [4D+2] (columns kr | kw | e | a | beta_r | beta_w), M0 [m,D] the initial memory shared by all samples ->
    (rs [B,T,D], M_T [B,m,D]), or (rs[:, -1] [B,D], M_T) with return_sequences=False (its gradient then enters the backward as [B,D]:
    no zero [B,T,D] block is made).  Per live step the slots are addressed by cosine similarity (two softmaxes with learned
    sharpness), read, then erased and added to; a masked step carries the memory and the read.  One launch per direction (plus the
    small fixed-order sum of the parameter-gradient partials); an output that received no gradient enters the backward as NULL and
    only the gradients that are asked for are computed.  GPU only; shapes outside the kernel menu raise FilError
    (layers.NTMMemoryLayer takes its composed path there)."""
    return _NtmFn.apply(h, mask, Wp, bp, M0, bool(return_sequences))


def ntm_plan(B, T, H, m, D):
    """fil_ntm_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a shape
    outside the kernel menu."""
    return _tiled_plan("fil_ntm_plan", int(B), int(T), int(H), int(m), int(D))


SEQ_VIEWS = {"full": _lib.FIL_SEQ_VIEW_FULL, "causal": _lib.FIL_SEQ_VIEW_CAUSAL, "cross": _lib.FIL_SEQ_VIEW_CROSS}


def seq_view_check(who, view, split, T=None):
    """ValueError for a view that is not one of SEQ_VIEWS or a split that contradicts it (full / causal: 0; cross: 1 .. T-1, the
    upper end only once T is known) -- the rule of fil_seqattn_*_v, for the callers that want it before a tensor exists."""
    if view not in SEQ_VIEWS:
        raise ValueError("%s: view %r (%s)" % (who, view, ", ".join(SEQ_VIEWS)))
    split = int(split)
    if view != "cross" and split != 0:
        raise ValueError("%s: split=%d needs view='cross' (view=%r takes split=0)" % (who, split, view))
    if view == "cross" and (split < 1 or (T is not None and split >= T)):
        raise ValueError("%s: view='cross' needs 1 <= split <= T-1, got split=%d%s" % (who, split, "" if T is None else " at T=%d" % T))
    return SEQ_VIEWS[view], split


class _SeqAttnFn(torch.autograd.Function):
    """seq_self_attention and seq_view_attention: fil_seqattn_fwd_v / _bwd_v (the first is the full view with rows out)."""

    @staticmethod
    def forward(ctx, x, mask, wq, wk, wv, who, heads, use_scale, view, split, pool):
        _require_cuda(x, mask, wq, wk, wv)
        x, wq, wk, wv = (_f32c(t) for t in (x, wq, wk, wv))
        if (x.dim() != 3 or wq.dim() != 2 or wq.shape[0] != x.shape[2] or tuple(wk.shape) != tuple(wq.shape)
                or tuple(wv.shape) != tuple(wq.shape)):
            raise FilError("%s: x must be [B,T,K] and Wq, Wk, Wv [K,H*D], got %s, %s, %s and %s"
                           % (who, tuple(x.shape), tuple(wq.shape), tuple(wk.shape), tuple(wv.shape)))
        B, T, K = x.shape
        HD = wq.shape[1]
        if heads < 1 or HD % heads != 0:
            raise FilError("%s: %d heads do not divide the %d projection columns" % (who, heads, HD))
        H, D = heads, HD // heads
        mask = _seq_mask(who, mask, B, T)
        lib = _lib.load()
        res = torch.empty((B, HD) if pool else (B, T, HD), dtype=torch.float32, device=x.device)
        need = ctx.needs_input_grad
        saved = None
        if any(need[i] for i in (0, 2, 3, 4)):
            saved = _saved_floats(lib.fil_seqattn_saved_bytes(B, T, K, H, D), x.device)
        check(lib.fil_seqattn_fwd_v(ptr(x), ptr(mask), ptr(wq), ptr(wk), ptr(wv), None if pool else ptr(res), ptr(res) if pool else None,
                                    ptr(saved), B, T, K, H, D, int(use_scale), view, split, stream_ptr()), "fil_seqattn_fwd_v")
        _save(ctx, x, mask, wq, wk, wv, saved)
        ctx.dims = (H, D, int(use_scale), view, split, pool)
        return res

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        if not (need[0] or need[2] or need[3] or need[4]):
            return (None,) * 11
        x, mask, wq, wk, wv, saved = _saved(ctx)
        B, T, K = x.shape
        H, D, use_scale, view, split, pool = ctx.dims
        dev = x.device
        dx = _grad(need[0], x.shape, dev)
        dwq = _grad(need[2], wq.shape, dev)
        dwk = _grad(need[3], wk.shape, dev)
        dwv = _grad(need[4], wv.shape, dev)
        grads = (dx, None, dwq, dwk, dwv) + (None,) * 6
        if _no_samples(B, dwq, dwk, dwv):
            return grads
        g = _f32c(g)
        lib = _lib.load()
        ws, nws = _partials_scratch("fil_seqattn_bwd_workspace_bytes", "seqattn_bwd", need[2] or need[3] or need[4], dev, B, T, K, H, D)
        check(lib.fil_seqattn_bwd_v(ptr(x), ptr(mask), ptr(wq), ptr(wk), ptr(wv), ptr(saved), None if pool else ptr(g), ptr(g) if pool else None,
                                    ptr(dx), ptr(dwq), ptr(dwk), ptr(dwv), ptr(ws), nws, B, T, K, H, D, use_scale, view, split,
                                    stream_ptr()), "fil_seqattn_bwd_v")
        return grads


def seq_self_attention(x, mask, Wq, Wk, Wv, heads, use_scale=True):
    """Masked multi-head scaled dot-product self-attention over a behaviour sequence (extension; include/fil.h fil_seqattn_*):
    x [B,T,K], mask [B,T] bool / uint8 (non-zero = live; None = all live), Wq, Wk, Wv [K,H*D] with H = heads -> [B,T,H*D], heads
    concatenated.  The softmax runs over the live keys; a masked position's row is 0 and its x row is never read.  No biases, no
    output projection, no dropout; seq_view_attention adds a structure mask and a pooled output.  One launch per direction (plus the
    small fixed-order sum of the parameter-gradient partials); only the gradients that are asked for are written.  GPU only; shapes
    outside the kernel menu raise FilError (layers.SeqSelfAttentionLayer takes its composed path there)."""
    return _SeqAttnFn.apply(x, mask, Wq, Wk, Wv, "seq_self_attention", int(heads), bool(use_scale), _lib.FIL_SEQ_VIEW_FULL, 0, False)


def seq_view_attention(x, mask, Wq, Wk, Wv, heads, use_scale=True, view="full", split=0, pool=False):
    """seq_self_attention under a structure mask, with an optional mean over the rows (extension; include/fil.h fil_seqattn_*_v: the
    views of the Sequence-Aware Factorization Machine).  view: "full" (every live key), "causal" (row i sees the live keys j <= i) or
    "cross" (the first `split` rows see only the live keys of the others and the others only theirs; 1 <= split <= T-1).  A live row
    with no key to see is 0 and sends no gradient.  pool=False -> [B,T,H*D]; pool=True -> [B,H*D], the mean of the live rows (0 for a
    sample without one), summed inside the kernel: no [B,T,H*D] tensor exists in either direction.  The same kernels as
    seq_self_attention, which is view="full", pool=False bit for bit.  A bad view / split raises ValueError; GPU only; shapes outside the
    kernel menu raise FilError (layers.SeqViewAttentionLayer takes its composed path there)."""
    T = x.shape[1] if torch.is_tensor(x) and x.dim() == 3 else None
    v, s = seq_view_check("seq_view_attention", view, split, T)
    return _SeqAttnFn.apply(x, mask, Wq, Wk, Wv, "seq_view_attention", int(heads), bool(use_scale), v, s, bool(pool))


def seq_attn_plan(B, T, K, H, D):
    """fil_seqattn_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a
    shape outside the kernel menu."""
    return _tiled_plan("fil_seqattn_plan", int(B), int(T), int(K), int(H), int(D))


# --------------------------------------------------------------------------------------------- N3  top-k retrieval over a long history
SEARCH_PREFER = {"first": 0, "last": _lib.FIL_SEARCH_PREFER_LAST}


def _search_args(who, hist_idx, k, table, offset, size, query, attr, cand, mask, prefer):
    """The checks seq_search and seq_search_graph share -> (B, T, K, soft, hard, the mask as uint8); K = 4 without the soft part
    (unused there)."""
    if prefer not in SEARCH_PREFER:
        raise ValueError("%s: prefer %r (%s)" % (who, prefer, ", ".join(SEARCH_PREFER)))
    if hist_idx.dim() != 2 or hist_idx.dtype != torch.int64:
        raise FilError("%s: hist_idx must be a [B,T] int64 tensor, got %s %s" % (who, tuple(hist_idx.shape), hist_idx.dtype))
    B, T = hist_idx.shape
    if int(k) < 1 or T < 1:
        raise FilError("%s: k and T must be positive, got k=%d, T=%d" % (who, k, T))
    if (table is None) != (query is None) or (attr is None) != (cand is None) or (table is None and attr is None):
        raise FilError("%s: give table and query (the soft search), attr and cand (the hard search), or both pairs" % who)
    K = 4
    if table is not None:
        if table.dim() != 2 or query.dim() != 2 or tuple(query.shape) != (B, table.shape[1]) or table.dtype != torch.float32 or \
                query.dtype != torch.float32:
            raise FilError("%s: table must be [V,K] and query [B,K], float32, got %s %s and %s %s"
                           % (who, tuple(table.shape), table.dtype, tuple(query.shape), query.dtype))
        K = table.shape[1]
        rows = int(offset) + (table.shape[0] - int(offset) if size is None else int(size))
        if int(offset) < 0 or rows > table.shape[0]:
            raise FilError("%s: the field's rows [%d, %d) are not inside the table of %d rows" % (who, offset, rows, table.shape[0]))
    if attr is not None and (tuple(attr.shape) != (B, T) or attr.dtype != torch.int64 or tuple(cand.shape) != (B,) or cand.dtype != torch.int64):
        raise FilError("%s: attr must be [B,T] and cand [B], int64, got %s %s and %s %s"
                       % (who, tuple(attr.shape), attr.dtype, tuple(cand.shape), cand.dtype))
    return B, T, K, table is not None, attr is not None, _seq_mask(who, mask, B, T)


def seq_search_graph(hist_idx, k, table=None, offset=0, size=None, query=None, attr=None, cand=None, mask=None, padding_id=0,
                     prefer="first", return_scores=False, oob_count=None):
    """seq_search's definition in torch ops (include/fil.h fil_seq_search), bit-equal to the kernel: what seq_search runs outside the
    kernel menu, and the second reference of its tests.  The score is K elementwise multiply and add steps in ascending j (separate
    ops: nothing is contracted), the selection a stable sort on integers, the output order a second one.  It gathers the [B,T,K]
    rows the kernel never materialises.  No host synchronisation, no data-dependent shape."""
    B, T, K, soft, hard, mask = _search_args("seq_search_graph", hist_idx, k, table, offset, size, query, attr, cand, mask, prefer)
    k = int(k)
    dev = hist_idx.device
    slot = hist_idx != padding_id
    ok = torch.ones_like(slot) if size is None else (hist_idx >= 0) & (hist_idx < int(size))
    live = slot & ok
    if oob_count is not None:
        oob_count += (slot & ~ok).sum().to(oob_count.dtype)
    if mask is not None:
        live = live & (mask != 0)
    if hard:
        live = live & (attr == cand[:, None])
    if soft:
        rows = table.detach()[torch.where(live, hist_idx + int(offset), torch.zeros_like(hist_idx))]          # [B,T,K]
        q = query.detach()
        score = torch.zeros((B, T), dtype=torch.float32, device=dev)
        for j in range(K):
            p = rows[:, :, j] * q[:, j:j + 1]
            score = score + p
        score = torch.where(live, score, torch.zeros_like(score))
    else:
        score = torch.zeros((B, T), dtype=torch.float32, device=dev)
    bits = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = bits ^ torch.where(bits >> 31 != 0, torch.full_like(bits, 0xFFFFFFFF), torch.full_like(bits, 0x80000000))
    pos = torch.arange(T, dtype=torch.int64, device=dev).expand(B, T)
    # ascending in (dead last, key descending, position ascending -- descending for prefer="last")
    rank = torch.where(live, 0xFFFFFFFF - key, torch.full_like(key, 1 << 32)) * T + (pos if prefer == "first" else T - 1 - pos)
    order = torch.sort(rank, dim=1, stable=True)[1]
    n = live.sum(1).clamp(max=k)
    kk = min(k, T)
    taken = torch.arange(kk, dtype=torch.int64, device=dev)[None, :] < n[:, None]
    chosen = torch.where(taken, order[:, :kk], torch.full_like(order[:, :kk], T))
    chosen = torch.sort(chosen, dim=1, stable=True)[0]                                              # back to time order
    safe = chosen.clamp(max=T - 1)
    sel_pos = torch.where(taken, chosen, torch.full_like(chosen, -1)).to(torch.int32)
    sel_idx = torch.where(taken, hist_idx.gather(1, safe), torch.full_like(chosen, padding_id))
    sel_score = torch.where(taken, score.gather(1, safe), torch.zeros((B, kk), dtype=torch.float32, device=dev))
    if kk < k:
        sel_pos = torch.nn.functional.pad(sel_pos, (0, k - kk), value=-1)
        sel_idx = torch.nn.functional.pad(sel_idx, (0, k - kk), value=padding_id)
        sel_score = torch.nn.functional.pad(sel_score, (0, k - kk), value=0.0)
    out = (sel_idx, sel_pos, n.to(torch.int32))
    return out + (sel_score,) if return_scores else out


def _row_strided(t):
    """A 2-D tensor as (tensor, row stride in elements) the search kernel can read in place -- rows contiguous, any row stride -- or its
    contiguous copy."""
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, max(t.stride(0), t.shape[1])


def seq_search(hist_idx, k, table=None, offset=0, size=None, query=None, attr=None, cand=None, mask=None, padding_id=0, prefer="first",
               return_scores=False, oob_count=None):
    """Top-k retrieval over a long behaviour history (extension; include/fil.h fil_seq_search): hist_idx [B,T] int64 field-local ids of
    the field whose rows start at `offset` of `table` [V,K] and number `size` (None: ids are trusted) -> (sel_idx [B,k] int64,
    sel_pos [B,k] int32, count [B] int32[, scores [B,k] fp32]).  Soft search: table and query [B,K], the score of a slot is the fp32
    inner product of its row with the query, summed sequentially; hard search: attr [B,T] and cand [B] int64, a slot takes part only
    where attr == cand; both may be given.  A slot also drops out where its id is padding_id, out of range (counted in oob_count, an
    int32 device scalar) or mask [B,T] is zero.  The min(k, live) best slots -- ties to the earlier position, to the later with
    prefer="last" -- come back in time order; the tail is padding_id / -1 / +0.  Integer results: there is no autograd node, query and
    table are read as data.  One launch, no host synchronisation; rows of hist_idx, attr and query may be strided.  GPU only; a shape
    outside the kernel menu runs seq_search_graph, the same definition in torch ops."""
    _require_cuda(hist_idx, table, query, attr, cand, mask, oob_count)
    B, T, K, soft, hard, mask = _search_args("seq_search", hist_idx, k, table, offset, size, query, attr, cand, mask, prefer)
    k = int(k)
    if not seq_search_plan(B, T, K, k)["fits"]:
        return seq_search_graph(hist_idx, k, table, offset, size, query, attr, cand, mask, padding_id, prefer, return_scores, oob_count)
    dev = hist_idx.device
    hist_idx, hs = _row_strided(hist_idx)
    qs = as_ = 0
    if soft:
        table = _f32c(table.detach())
        query, qs = _row_strided(query.detach())
    if hard:
        attr, as_ = _row_strided(attr)
        cand = cand.contiguous()
    sel_idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    sel_pos = torch.empty((B, k), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    scores = torch.empty((B, k), dtype=torch.float32, device=dev) if return_scores else None
    check(_lib.load().fil_seq_search(ptr(hist_idx), hs, int(offset), -1 if size is None else int(size), int(padding_id), ptr(mask),
                                     ptr(table), ptr(query), qs, ptr(attr), as_, ptr(cand), ptr(sel_pos), ptr(sel_idx), ptr(count),
                                     ptr(scores), ptr(oob_count), B, T, K, k, SEARCH_PREFER[prefer], stream_ptr()), "fil_seq_search")
    out = (sel_idx, sel_pos, count)
    return out + (scores,) if return_scores else out


def seq_search_plan(B, T, K, k):
    """fil_seq_search_plan's answer as a dict (fits, tile, grid, cap, partials, lds_fwd, lds_bwd); fits=False (and nothing else) for a
    shape outside the kernel menu."""
    return _tiled_plan("fil_seq_search_plan", int(B), int(T), int(K), int(k))


def attn_plan(F, K, H, A, precision="f32"):
    """fil_attn_plan's answer for AutoInt's fused interacting layer (the plan does not depend on the batch) as a dict: fits = the
    dynamic LDS of BOTH the forward and the backward within the launchers' limit in this precision, fwd_ok, bwd_ok; fits=False (and
    nothing else) for a shape outside the kernel menu."""
    plan = (ctypes.c_int * 10)()
    rc = _lib.load().fil_attn_plan(int(F), int(K), int(H), int(A), _precision(precision), plan)
    if rc == _lib.FIL_ERR_UNSUPPORTED:
        return dict(fits=False)
    check(rc, "fil_attn_plan")
    return dict(fits=bool(plan[0]) and bool(plan[4]), fwd_ok=bool(plan[0]), bwd_ok=bool(plan[4]))


# --------------------------------------------------------------------------------------------- A2  DCN
class _DcnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        _require_cuda(x, w, b)
        x, w, b = _f32c(x), _f32c(w), _f32c(b)
        B, D = x.shape
        L = w.shape[0]
        y = torch.empty_like(x)
        s = torch.empty((B, L), dtype=torch.float32, device=x.device)
        check(_lib.load().fil_dcn_fwd(ptr(x), ptr(w), ptr(b), ptr(y), ptr(s), B, D, L, stream_ptr()), "fil_dcn_fwd")
        ctx.save_for_backward(x, w, b, s)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, b, s = ctx.saved_tensors
        B, D = x.shape
        L = w.shape[0]
        lib = _lib.load()
        g = _f32c(g)
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        db = torch.empty_like(b)
        nws = lib.fil_dcn_bwd_workspace_bytes(B, D, L)
        ws = _scratch(nws, x.device, "dcn_bwd")
        check(lib.fil_dcn_bwd(ptr(x), ptr(w), ptr(b), ptr(s), ptr(g), ptr(dx), ptr(dw), ptr(db), B, D, L, ptr(ws), nws,
                              stream_ptr()), "fil_dcn_bwd")
        return dx, dw, db


def dcn_cross(x, w, b):
    """x [B,D], w,b [L,D] -> x_L [B,D] with x_{l+1} = x0*(x_l.w_l) + x_l + b_l."""
    return _DcnFn.apply(x, w, b)


# --------------------------------------------------------------------------------------------- A3  CIN
CIN_BF16X3 = 2          # fil.h FIL_CIN_BF16X3: the labelled split-bf16 mode of the merged quadratic tail's GEMMs (csrc/cin_qsplit.h)
CIN_X_TRANSPOSED = 16   # fil.h FIL_CIN_X_TRANSPOSED: x handed over as [B*K, F] (embed_gather(emit_xt=True))
CIN_TAIL_ALWAYS = 64    # fil.h FIL_CIN_TAIL_ALWAYS: the tails wherever they are defined, whatever the batch size (tests, smoke)
CIN_NOQTAIL = 256       # fil.h FIL_CIN_NOQTAIL: three-layer nets on the F+1-column fused tail instead of the quadratic tail
CIN_NOQMERGE = 512      # fil.h FIL_CIN_NOQMERGE: round 3's two launches per direction for the quadratic tail (no 256-column forward with the pools and the head in its epilogue, no 256-column dW, no two-pass dZ)
CIN_PREC_DEFAULT = 0    # fil.h FIL_CIN_PREC_DEFAULT: what `mode` selects
CIN_PREC_BF16 = 1       # fil.h FIL_CIN_PREC_BF16: the labelled bf16 training mode of the merged quadratic tail's GEMMs (one bf16 MFMA per product)
_CIN_PRECISIONS = {"f32": CIN_PREC_DEFAULT, "bf16": CIN_PREC_BF16}


def _cin_precision_code(precision):
    if precision not in _CIN_PRECISIONS:
        raise FilError("cin: precision must be one of %s, got %r" % (sorted(_CIN_PRECISIONS), precision))
    return _CIN_PRECISIONS[precision]


def cin_precision_used(B, F, K, H, mode=0, precision="bf16"):
    """The precision a CIN call with this shape, mode and precision actually runs (fil_cin_precision_used): "bf16" where the one-plane
    bf16 kernels of the merged quadratic tail run, else "f32" (the exact kernels)."""
    lib = _lib.load()
    code = _cin_precision_code(precision)
    rc = lib.fil_cin_precision_used(int(B), int(F), int(K), len(H), int_array(list(H)), int(mode), code)
    if rc < 0:
        raise FilError("fil_cin_precision_used: %s" % lib.fil_last_error().decode())
    return "bf16" if rc == CIN_PREC_BF16 else "f32"


def cin_shortdx_used(B, F, K, H, output_dim=1, mode=0, precision="f32"):
    """True where a CIN backward with this shape, head, mode and precision runs cin_shortcut_dx_kernel for the shortcut's data gradient
    (fil_cin_shortdx_used)."""
    lib = _lib.load()
    rc = lib.fil_cin_shortdx_used(int(B), int(F), int(K), len(H), int_array(list(H)), int(output_dim), int(mode), _cin_precision_code(precision))
    if rc < 0:
        raise FilError("fil_cin_shortdx_used: %s" % lib.fil_last_error().decode())
    return rc == 1


def cin_grad_ready_points(B, F, K, H, mode=0):
    """Where in fil_cin_bwd each grad_ready slot is recorded (fil.h): list of L+1 ordinals, [l] for layer l and [L] for the dense
    head; slots with equal ordinals become final together, so a data-parallel caller reduces them with one collective."""
    lib = _lib.load()
    L = len(H)
    pts = (ctypes.c_int * (L + 1))()
    n = lib.fil_cin_grad_ready_points(int(B), int(F), int(K), L, int_array(list(H)), int(mode), pts)
    if n < 0:
        raise FilError("fil_cin_grad_ready_points: %s" % lib.fil_last_error().decode())
    return [int(v) for v in pts]


def cin_forward_raw(x, Ws, bs, dense_w, dense_b, output_dim=1, mode=0, xt=None, precision="f32"):
    """Raw forward through the C ABI.  Returns (out [B,1] or None, pooled [B,L*K], saved uint8 buffer).
    xt (optional): x already transposed to [B*K, F] by the gather that produced it; the kernels then read it in place.
    precision: "f32" (fil_cin_fwd) or "bf16" (fil_cin_fwd_p with FIL_CIN_PREC_BF16: the labelled bf16 mode where its kernels run)."""
    lib = _lib.load()
    prec = _cin_precision_code(precision)
    B, F, K = x.shape
    if xt is not None:
        if tuple(xt.shape) != (B * K, F) or xt.dtype != torch.float32 or not xt.is_contiguous() or xt.device != x.device:
            raise FilError("cin: xt must be a contiguous float32 [B*K, F] = [%d, %d] tensor on %s" % (B * K, F, x.device))
        mode |= CIN_X_TRANSPOSED
    L = len(Ws)
    H = [int(w.shape[1]) for w in Ws]
    hp = F
    for l, w in enumerate(Ws):
        if tuple(w.shape) != (hp * F, H[l]) or tuple(bs[l].shape) != (H[l],):
            raise FilError("cin: W[%d] must be [%d,%d] and bias[%d] [%d]" % (l, hp * F, H[l], l, H[l]))
        hp = H[l]
    Harr = int_array(H)
    saved = _workspace(lib.fil_cin_saved_bytes(B, F, K, L, Harr), x.device)
    nws = lib.fil_cin_fwd_workspace_bytes(B, F, K, L, Harr)
    if nws == 0 and B > 0:
        raise FilError("cin: %s" % lib.fil_last_error().decode())
    ws = _scratch(nws, x.device, "cin_fwd")
    pooled = torch.empty((B, L * K), dtype=torch.float32, device=x.device)
    out = torch.empty((B, 1), dtype=torch.float32, device=x.device) if output_dim == 1 else None
    if prec == CIN_PREC_DEFAULT:
        check(lib.fil_cin_fwd(ptr(xt if xt is not None else x), ptr_array(Ws), ptr_array(bs), ptr(dense_w), ptr(dense_b), ptr(out),
                              ptr(pooled), ptr(saved), B, F, K, L, Harr, output_dim, mode, ptr(ws), nws, stream_ptr()), "fil_cin_fwd")
    else:
        check(lib.fil_cin_fwd_p(ptr(xt if xt is not None else x), ptr_array(Ws), ptr_array(bs), ptr(dense_w), ptr(dense_b), ptr(out),
                                ptr(pooled), ptr(saved), B, F, K, L, Harr, output_dim, mode, prec, ptr(ws), nws, stream_ptr()), "fil_cin_fwd_p")
    return out, pooled, saved


def cin_backward_raw(x, Ws, bs, dense_w, pooled, saved, g, output_dim=1, mode=0, grads=None, ready_events=None, xt=None, precision="f32"):
    """Raw backward.  grads (optional): dict with preallocated 'dx','dW'(list),'db'(list),'ddw','ddb' tensors
    (e.g. views into one flat all-reduce bucket).  ready_events (optional): L+1 torch.cuda.Event objects (or None
    entries), recorded as each layer's / the head's parameter gradients become final (fil.h: grad_ready_events; the same points
    for either precision).  precision: as cin_forward_raw's (fil_cin_bwd_p for "bf16").  Returns the dict."""
    lib = _lib.load()
    prec = _cin_precision_code(precision)
    B, F, K = x.shape
    L = len(Ws)
    H = [int(w.shape[1]) for w in Ws]
    Harr = int_array(H)
    if grads is None:
        grads = dict(dx=torch.empty_like(x), dW=[torch.empty_like(w) for w in Ws], db=[torch.empty_like(b) for b in bs],
                     ddw=torch.empty((L * K, 1), dtype=torch.float32, device=x.device) if output_dim == 1 else None,
                     ddb=torch.empty((1,), dtype=torch.float32, device=x.device) if output_dim == 1 else None)
    nws = lib.fil_cin_bwd_workspace_bytes(B, F, K, L, Harr)
    ws = _scratch(nws, x.device, "cin_bwd")
    evs = None
    if ready_events is not None:
        if len(ready_events) != L + 1:
            raise FilError("cin: ready_events must have L+1 = %d entries" % (L + 1))
        for e in ready_events:      # a torch event only owns a hipEvent_t once it has been recorded
            if e is not None and not e.cuda_event:
                e.record()
        evs = (ctypes.c_void_p * (L + 1))(*[None if e is None else e.cuda_event for e in ready_events])
    if xt is not None:
        mode |= CIN_X_TRANSPOSED
    if prec == CIN_PREC_DEFAULT:
        check(lib.fil_cin_bwd(ptr(xt if xt is not None else x), ptr_array(Ws), ptr_array(bs), ptr(dense_w), ptr(pooled), ptr(saved), ptr(g),
                              ptr(grads["dx"]), ptr_array(grads["dW"]), ptr_array(grads["db"]), ptr(grads["ddw"]),
                              ptr(grads["ddb"]), B, F, K, L, Harr, output_dim, mode, evs, ptr(ws), nws, stream_ptr()), "fil_cin_bwd")
    else:
        check(lib.fil_cin_bwd_p(ptr(xt if xt is not None else x), ptr_array(Ws), ptr_array(bs), ptr(dense_w), ptr(pooled), ptr(saved), ptr(g),
                                ptr(grads["dx"]), ptr_array(grads["dW"]), ptr_array(grads["db"]), ptr(grads["ddw"]),
                                ptr(grads["ddb"]), B, F, K, L, Harr, output_dim, mode, prec, evs, ptr(ws), nws, stream_ptr()), "fil_cin_bwd_p")
    return grads


class _CinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dense_w, dense_b, output_dim, mode, xt, precision, *params):
        L = len(params) // 2
        Ws = [_f32c(p) for p in params[:L]]
        bs = [_f32c(p) for p in params[L:]]
        _require_cuda(x, *Ws, *bs)
        x = _f32c(x)
        dense_w = _f32c(dense_w)
        dense_b = _f32c(dense_b)
        out, pooled, saved = cin_forward_raw(x, Ws, bs, dense_w, dense_b, output_dim, mode, xt=xt, precision=precision)
        # xt (the gather's second output, same values as x) goes through save_for_backward too: an in-place edit between the
        # forward and the backward then trips autograd's version check instead of silently feeding stale rows to the kernels
        _save(ctx, x, dense_w, pooled, saved, xt, *Ws, *bs)
        ctx.cfg = (L, output_dim, mode, precision)
        return out if output_dim == 1 else pooled

    @staticmethod
    def backward(ctx, g):
        L, output_dim, mode, precision = ctx.cfg
        x, dense_w, pooled, saved, xt, *params = _saved(ctx)
        gr = cin_backward_raw(x, params[:L], params[L:], dense_w, pooled, saved, _f32c(g), output_dim, mode, xt=xt, precision=precision)
        return (gr["dx"], gr["ddw"], gr["ddb"], None, None, None, None, *gr["dW"], *gr["db"])


def cin(x, Ws, bs, dense_w=None, dense_b=None, output_dim=1, mode=0, xt=None, precision="f32"):
    """x [B,F,K]; Ws[l] [H_{l-1}*F, H_l]; bs[l] [H_l]; dense_w [L*K,1]; dense_b [1] -> [B,1] (or pooled [B,L*K]).
    xt (optional) = x transposed to [B*K, F] by the gather that produced x (embed_gather(emit_xt=True) attaches it to its
    result as `_fil_xt`): the kernels read it in place instead of transposing x again.  Gradients still flow to x.
    precision: "f32" (exact, the default) or "bf16" -- the labelled bf16 training mode (include/fil.h fil_cin_fwd_p): the merged
    quadratic tail's GEMMs on one bf16 value per operand, ~1e-3 relative error; shapes without those kernels run exact
    (cin_precision_used says which)."""
    _cin_precision_code(precision)
    return _CinFn.apply(x, dense_w, dense_b, output_dim, mode, xt, precision, *Ws, *bs)


# --------------------------------------------------------------------------------------------- A4  AutoInt
class _AttnFn(torch.autograd.Function):
    """fuse_relu=True: returns y = relu(res + LN(av)); fuse_relu=False: returns (LN(av), res).
    head_major=True: x is the [H',B,F,A'] output of a previous interacting layer, read in place as its head-concat
    [B,F,H'*A'] (fil.h: x_chunk = A'); the gradient comes back in the same layout."""

    @staticmethod
    def forward(ctx, x, Wq, Wk, Wr, gamma, beta, scale, eps, fuse_relu, precision=0, head_major=False):
        _require_cuda(x, Wq, Wk, Wr, gamma, beta)
        x, Wq, Wk, Wr, gamma, beta = [_f32c(t) for t in (x, Wq, Wk, Wr, gamma, beta)]
        if head_major:
            Hp, B, F, Ap = x.shape
            K, x_chunk = Hp * Ap, Ap
        else:
            B, F, K = x.shape
            x_chunk = 0
        Kw, H, A = Wq.shape
        if Kw != K:
            raise FilError("attention: weights are [%d,H,A] but the input has %d features" % (Kw, K))
        lib = _lib.load()
        y = torch.empty((H, B, F, A), dtype=torch.float32, device=x.device)
        res = None
        if not fuse_relu and Wr is not None:
            res = torch.empty((H, B, F, A), dtype=torch.float32, device=x.device)
        # the LayerNorm input is kept for the backward's LayerNorm gradient, normalised, with the rows' 1/sigma beside it
        # (H*B*F*(A+1) floats: the backward does not derive the statistics again); FIL_ATTN_SAVE_AV=0 drops both and makes the
        # backward re-run the forward into its workspace instead
        av = rstd = None
        if gamma is not None and _SAVE_AV:
            av = torch.empty((H, B, F, A), dtype=torch.float32, device=x.device)
            rstd = torch.empty((H, B, F), dtype=torch.float32, device=x.device)
        check(lib.fil_attn_fwd(ptr(x), ptr(Wq), ptr(Wk), ptr(Wr), ptr(gamma), ptr(beta), ptr(y), ptr(res), ptr(av), ptr(rstd),
                               B, F, K, H, A,
                               float(scale), float(eps), int(bool(fuse_relu)), int(precision), x_chunk, None, 0, stream_ptr()),
              "fil_attn_fwd")
        keep_y = bool(fuse_relu) and (av is not None or gamma is None)   # the fused ReLU mask is y > 0
        _save(ctx, x, Wq, Wk, Wr, gamma, beta, av, rstd, y if keep_y else None)
        ctx.cfg = (float(scale), float(eps), bool(fuse_relu), int(precision), x_chunk, (B, F, K))
        if fuse_relu:
            return y
        if res is None:
            return y, None
        return y, res

    @staticmethod
    def backward(ctx, dy, dres=None):
        scale, eps, fuse_relu, precision, x_chunk, (B, F, K) = ctx.cfg
        x, Wq, Wk, Wr, gamma, beta, av_saved, rstd_saved, y_saved = _saved(ctx)
        has_res, has_ln = Wr is not None, gamma is not None
        _, H, A = Wq.shape
        lib = _lib.load()
        dy = _f32c(dy) if dy is not None else torch.zeros((H, B, F, A), dtype=torch.float32, device=x.device)
        dres_in = None
        if not fuse_relu and has_res:
            dres_in = _f32c(dres) if dres is not None else torch.zeros((H, B, F, A), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        dWq, dWk = torch.empty_like(Wq), torch.empty_like(Wk)
        dWr = torch.empty_like(Wr) if has_res else None
        dgamma = torch.empty_like(gamma) if has_ln else None
        dbeta = torch.empty_like(beta) if has_ln else None
        have_saved = int((not has_ln or av_saved is not None) and (not fuse_relu or y_saved is not None))
        nws = lib.fil_attn_bwd_workspace_bytes(B, F, K, H, A, have_saved)
        ws = _scratch(nws, x.device, "attn_bwd")
        check(lib.fil_attn_bwd(ptr(x), ptr(Wq), ptr(Wk), ptr(Wr), ptr(gamma), ptr(beta), ptr(dy), ptr(dres_in), ptr(y_saved),
                               ptr(av_saved), ptr(rstd_saved), ptr(dx),
                               ptr(dWq), ptr(dWk), ptr(dWr), ptr(dgamma), ptr(dbeta), B, F, K, H, A, scale, eps,
                               int(fuse_relu), precision, x_chunk, ptr(ws), nws, stream_ptr()), "fil_attn_bwd")
        return dx, dWq, dWk, dWr, dgamma, dbeta, None, None, None, None, None


_SAVE_AV = os.environ.get("FIL_ATTN_SAVE_AV", "1") != "0"   # read once at import


def _attn_scale(Wq, use_scale):
    return (1.0 / (Wq.shape[-1] ** 0.5)) if use_scale else 1.0


PRECISIONS = {"f32": 0, "f16_mfma": 1}


def _precision(p):
    if p not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (sorted(PRECISIONS), p))
    return PRECISIONS[p]


def autoint_interact(x, Wq, Wk, Wr=None, gamma=None, beta=None, use_scale=True, eps=1e-3, precision="f32", head_major=False):
    """x [B,F,K], W* [K,H,A] -> y [H,B,F,A] = relu(x Wr + LN(sigmoid(scale q k^T) k))  (V == K projection).
    precision "f16_mfma": matrix products on the fp16 MFMA with fp32 accumulation (include/fil.h, fil_precision).
    head_major=True: x is a previous layer's [H',B,F,A'] output, consumed as its head-concat [B,F,H'*A'] without a copy."""
    return _AttnFn.apply(x, Wq, Wk, Wr, gamma, beta, _attn_scale(Wq, use_scale), eps, True, _precision(precision),
                         bool(head_major))


def autoint_stack(x, layers, use_scale=True, eps=1e-3, precision="f32"):
    """A stack of interacting layers (BASELINE config 5: 3 layers).  layers: list of (Wq, Wk, Wr, gamma, beta); layer l > 0
    takes the head-concat [B,F,H*A] of layer l-1 (ESULayer's convention, reference behavior_layer.py:973) -- read in
    place from the head-major output.  Returns the last layer's [H,B,F,A]."""
    y = x
    for l, (Wq, Wk, Wr, gamma, beta) in enumerate(layers):
        y = autoint_interact(y, Wq, Wk, Wr, gamma, beta, use_scale=use_scale, eps=eps, precision=precision, head_major=l > 0)
    return y


def mult_head_attention(x, Wq, Wk, Wr=None, gamma=None, beta=None, use_scale=True, eps=1e-3, precision="f32"):
    """Stand-alone MultHeadAttentionLayer: returns (atten_v [H,B,F,A] = LN(sigmoid(scale q k^T) k), res = x Wr or None)."""
    return _AttnFn.apply(x, Wq, Wk, Wr, gamma, beta, _attn_scale(Wq, use_scale), eps, False, _precision(precision))


class _PAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, scale, mask_period):
        _require_cuda(q, k, v, mask)
        q, k, v, mask = _f32c(q), _f32c(k), _f32c(v), _f32c(mask)
        N, Fq, A = q.shape
        _, Fk, Av = v.shape
        out = torch.empty((N, Fq, Av), dtype=torch.float32, device=q.device)
        check(_lib.load().fil_pattn_fwd(ptr(q), ptr(k), ptr(v), ptr(mask), ptr(out), N, Fq, Fk, A, Av, float(scale), int(mask_period),
                                        stream_ptr()), "fil_pattn_fwd")
        _save(ctx, q, k, v, mask)
        ctx.cfg = (float(scale), int(mask_period))
        return out

    @staticmethod
    def backward(ctx, dout):
        scale, mask_period = ctx.cfg
        q, k, v, mask = _saved(ctx)
        N, Fq, A = q.shape
        _, Fk, Av = v.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        check(_lib.load().fil_pattn_bwd(ptr(q), ptr(k), ptr(v), ptr(mask), ptr(_f32c(dout)), ptr(dq), ptr(dk), ptr(dv), N, Fq, Fk, A, Av,
                                        scale, mask_period, stream_ptr()), "fil_pattn_bwd")
        return dq, dk, dv, None, None, None


def product_attention(q, k, v, use_scale=False, mask=None, mask_mod=1):
    """ProductAttentionLayer.call([q, k, v], mask) (reference behavior_layer.py:292-311): q [..., Fq, A], k [..., Fk, A],
    v [..., Fk, Av] -> sigmoid(scale q k^T (masked)) v, leading axes flattened into the kernel's item axis.
    mask_mod 1: scores @ mask (mask [..., Fk, Fk'] broadcast over the leading axes; v must have Fk' rows) -- computed as
    q (mask^T k)^T, so only k is touched; mask_mod 2: scores + mask * (-100000), mask broadcastable to [..., Fq, Fk]."""
    lead = tuple(q.shape[:-2])
    Fq, A = q.shape[-2:]
    scale = 1.0 / (A ** 0.5) if use_scale else 1.0
    kmask, period = None, 0
    if mask is not None:
        m = mask.to(torch.float32)
        if mask_mod == 1:
            k = torch.matmul(m.transpose(-1, -2), k)            # (q k^T) M == q (M^T k)^T; autograd carries dk through
        elif mask_mod == 2:
            Fk = k.shape[-2]
            if m.dim() < 2:
                m = m.reshape((1,) * (2 - m.dim()) + tuple(m.shape))
            mlead = tuple(m.shape[:-2])
            # a mask whose leading axes are a suffix of q's (e.g. [B,Fq,Fk] against [H,B,...]) is indexed n % period in the kernel
            if len(mlead) <= len(lead) and mlead == lead[len(lead) - len(mlead):]:
                period = 1
                for s_ in mlead:
                    period *= s_
                kmask = m.expand(*mlead, Fq, Fk).reshape(max(period, 1), Fq, Fk).contiguous()
                period = max(period, 1)
            else:
                kmask = m.expand(*lead, Fq, Fk).reshape(-1, Fq, Fk).contiguous()
                period = kmask.shape[0]
    if v.shape[-2] != k.shape[-2]:
        raise FilError("product_attention: k has %d rows but v has %d" % (k.shape[-2], v.shape[-2]))
    out = _PAttnFn.apply(q.reshape(-1, Fq, A), k.expand(*lead, *k.shape[-2:]).reshape(-1, k.shape[-2], A),
                         v.reshape(-1, v.shape[-2], v.shape[-1]), kmask, scale, period)
    return out.reshape(*lead, Fq, v.shape[-1])


# --------------------------------------------------------------------------------------------- N1  embeddings
# (sorted row ids, permutation) of the most recent index tensors.  A model usually looks the SAME ids up in two tables (the
# embeddings and the linear weights): their gradients need the same sort.  An entry keeps its idx tensor alive, so an equal
# (data_ptr, _version) really is the same contents; in-place updates bump the version and miss -- and every gather (forward)
# empties the cache, so that an entry only ever serves the backward passes that follow the forwards which saw these ids
# (an update of idx that bypasses the version counter, e.g. through `.data`, cannot meet a stale entry).  The one exception is a
# gather from a table in deferred Keras mode, which sorts in the forward: it keeps only the entry that the gather immediately
# before it, from another table, made for the SAME idx tensor object (the other table of its layout, same forward), so no sort
# outlives its forward pair either.  An entry records the number of the gather it was made under (_SORT_GEN);
# _SORT_PREV_TABLE is (a weak reference to) the runs table of the latest gather.
_SORT_CACHE = []
_SORT_GEN = [0]
_SORT_PREV_TABLE = [None]


class _ScoreAddSigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *parts):
        _require_cuda(*parts)
        shape = parts[0].shape
        parts = [_f32c(t) for t in parts]
        n = parts[0].numel()
        out = torch.empty(shape, dtype=torch.float32, device=parts[0].device)
        pp = [ptr(t) for t in parts] + [None] * (4 - len(parts))
        check(_lib.load().fil_score_add_sigmoid_fwd(*pp, ptr(out), n, stream_ptr()), "fil_score_add_sigmoid_fwd")
        ctx.save_for_backward(out)
        ctx.n_parts = len(parts)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        g = _f32c(g)
        dsum = torch.empty_like(out)
        check(_lib.load().fil_score_add_sigmoid_bwd(ptr(out), ptr(g), ptr(dsum), out.numel(), stream_ptr()),
              "fil_score_add_sigmoid_bwd")
        return (dsum,) * ctx.n_parts


def score_add_sigmoid(parts):
    """sigmoid(((p0 + p1) + p2) + p3) over 1..4 fp32 tensors of ONE shape (ScoreLayer(use_add=True), core_layer.py:58-84): one launch
    forward, one backward (every part receives the same gradient tensor)."""
    parts = list(parts)
    if not 1 <= len(parts) <= 4:
        raise FilError("score_add_sigmoid takes 1..4 parts, got %d" % len(parts))
    if any(t.shape != parts[0].shape for t in parts):
        raise FilError("score_add_sigmoid: the parts must have one shape, got %s" % [tuple(t.shape) for t in parts])
    return _ScoreAddSigmoidFn.apply(*parts)


def gemm_f32(a, b, trans_a=False, trans_b=False, bias=None, relu=False):
    """op(a) @ op(b) (+ bias, ReLU) in fp32 through the library's own MFMA GEMM (fil_gemm_f32, csrc/gemm.hip): a, b contiguous 2-D CUDA
    fp32 tensors; trans_a: a is [K, M]; trans_b: b is [N, K].  No autograd (the dense layers' Functions call it in both directions)."""
    _require_cuda(a, b)
    a, b = _f32c(a), _f32c(b)
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N = b.shape[0] if trans_b else b.shape[1]
    if (b.shape[1] if trans_b else b.shape[0]) != K:
        raise FilError("gemm_f32: %s x %s (trans_a=%s, trans_b=%s)" % (tuple(a.shape), tuple(b.shape), trans_a, trans_b))
    lib = _lib.load()
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    nws = lib.fil_gemm_f32_workspace_bytes(M, N, K)
    ws = _scratch(nws, a.device, "gemm_f32") if nws else None
    epi = 0 if bias is None else (2 if relu else 1)
    check(lib.fil_gemm_f32(ptr(a), ptr(b), ptr(c), ptr(_f32c(bias)) if bias is not None else None, M, N, K, a.shape[1], b.shape[1], N,
                           int(bool(trans_a)), int(bool(trans_b)), epi, ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0,
                           stream_ptr()), "fil_gemm_f32")
    return c


class _DenseReluFn(torch.autograd.Function):
    """y = relu(x @ kernel + bias) -- a hidden layer of the zoo's MLPs (DnnLayer, core_layer.py:102-118,201-226) -- as a library GEMM
    with the bias + ReLU in its epilogue forward, and backward as ONE HIP pass (ReLU mask + bias gradient, fil_relu_bias_bwd) plus the
    layer's two library GEMMs.  torch composes the same layer from 3 launches forward and 5 backward.  Under autocast the GEMMs run in
    the autocast dtype (bf16), as torch.matmul would."""

    @staticmethod
    def forward(ctx, x, kernel, bias):
        _require_cuda(x, kernel, bias)
        cd = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
        if cd not in (torch.float32, torch.bfloat16):
            raise FilError("dense_relu: autocast dtype %s (float32 or bfloat16)" % cd)
        with torch.autocast("cuda", enabled=False):
            xc, wc = x.to(cd).contiguous(), kernel.to(cd)
            if cd == torch.float32:      # the library's own fp32 MFMA GEMM, bias + ReLU in its epilogue (csrc/gemm.hip)
                y = gemm_f32(xc, wc, bias=bias, relu=True)
            else:                        # bf16 autocast: the framework's GEMM with the same epilogue
                y = torch._addmm_activation(bias.to(cd), xc, wc, use_gelu=False)
        ctx.save_for_backward(xc, wc, y)
        ctx.cfg = (x.dtype, kernel.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, wc, y = ctx.saved_tensors
        xdt, wdt, bdt = ctx.cfg
        lib = _lib.load()
        B, N = y.shape
        dy = dy.to(y.dtype).contiguous()
        dz = torch.empty_like(y)
        db = torch.empty((N,), dtype=torch.float32, device=y.device)
        ws = _scratch(lib.fil_relu_bias_bwd_workspace_bytes(B, N), y.device, "relu_bias_bwd")
        check(lib.fil_relu_bias_bwd(ptr(y), ptr(dy), ptr(dz), ptr(db), B, N, FIL_F32 if y.dtype == torch.float32 else FIL_BF16, ptr(ws),
                                    ws.numel(), stream_ptr()), "fil_relu_bias_bwd")
        with torch.autocast("cuda", enabled=False):
            if y.dtype == torch.float32:
                dx = gemm_f32(dz, wc, trans_b=True).to(xdt) if ctx.needs_input_grad[0] else None      # dz W^T
                dw = gemm_f32(xc, dz, trans_a=True).to(wdt) if ctx.needs_input_grad[1] else None      # x^T dz (split over the batch)
            else:
                dx = torch.matmul(dz, wc.t()).to(xdt) if ctx.needs_input_grad[0] else None
                dw = _batch_split_xt_dz(xc, dz).to(wdt) if ctx.needs_input_grad[1] else None
        return dx, dw, db.to(bdt)


def _batch_split_xt_dz(x, dz, splits=16):
    """x^T dz for bf16 x [B, I], dz [B, O] with the reduction over the batch cut into `splits` slices: one batched library GEMM + an
    fp32 sum of the slices in slice order.  As ONE GEMM the library runs the (I x O)-tile grid of this shape -- 8...40 workgroups for a
    4096-row batch -- at 27-31 us (MLP 637-256-128, B = 4096); cut in 16 it is 15-16 us including the sum (tools/mm_forms.py), and the
    result is fp32 without a separate cast.  Small or ragged batches take the plain product."""
    B = x.shape[0]
    if B < 1024 or B % splits != 0:
        return torch.matmul(x.t(), dz)
    parts = torch.bmm(x.view(splits, B // splits, x.shape[1]).transpose(1, 2), dz.view(splits, B // splits, dz.shape[1]))
    return parts.sum(0, dtype=torch.float32)


class _DenseFn(torch.autograd.Function):
    """y = x @ kernel + bias in fp32 through the library's own GEMM, forward and backward (dx = dy W^T, dW = x^T dy split over the batch and
    summed in order, db = the column sums).  The logit heads of the zoo's MLPs are Dense(1) / Dense(2) on a [B, 64...144] input: as library
    calls the framework runs dW = x^T dy of such a layer -- 64 x 1 outputs, reduction 4096 -- in 35 us (one 16 x 64 tile walking the batch)."""

    @staticmethod
    def forward(ctx, x, kernel, bias):
        _require_cuda(x, kernel, bias)
        xc, wc = _f32c(x), _f32c(kernel)
        ctx.save_for_backward(xc, wc)
        return gemm_f32(xc, wc, bias=bias)

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        dy = _f32c(dy)
        dx = gemm_f32(dy, wc, trans_b=True) if ctx.needs_input_grad[0] else None
        dw = gemm_f32(xc, dy, trans_a=True) if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db


def dense(x, kernel, bias):
    """x @ kernel + bias, x [B, in] fp32, kernel [in, units], bias [units] (csrc/gemm.hip both ways)."""
    if x.dim() != 2 or kernel.dim() != 2 or x.shape[1] != kernel.shape[0] or tuple(bias.shape) != (kernel.shape[1],):
        raise FilError("dense: x %s, kernel %s, bias %s" % (tuple(x.shape), tuple(kernel.shape), tuple(bias.shape)))
    return _DenseFn.apply(x, kernel, bias)


def dense_relu(x, kernel, bias):
    """relu(x @ kernel + bias), x [B, in] (fp32 or bf16), kernel [in, units], bias [units]."""
    if x.dim() != 2 or kernel.dim() != 2 or x.shape[1] != kernel.shape[0] or tuple(bias.shape) != (kernel.shape[1],):
        raise FilError("dense_relu: x %s, kernel %s, bias %s" % (tuple(x.shape), tuple(kernel.shape), tuple(bias.shape)))
    return _DenseReluFn.apply(x, kernel, bias)


class _MergeSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kernel, bias, *parts):
        _require_cuda(kernel, bias, *parts)
        dts = [FIL_F32 if t.dtype == torch.float32 else FIL_BF16 for t in parts]
        parts = [t.contiguous() for t in parts]
        kernel, bias = _f32c(kernel), _f32c(bias)
        B, O = parts[0].shape[0], kernel.shape[1]
        widths = [int(t.shape[1]) for t in parts]
        out = torch.empty((B, O), dtype=torch.float32, device=kernel.device)
        check(_lib.load().fil_merge_softmax_fwd(ptr_array(parts), int_array(widths), int_array(dts), len(parts), ptr(kernel), ptr(bias),
                                                ptr(out), B, O, stream_ptr()), "fil_merge_softmax_fwd")
        ctx.save_for_backward(kernel, out, *parts)
        ctx.cfg = (widths, dts)
        return out

    @staticmethod
    def backward(ctx, g):
        kernel, out, *parts = ctx.saved_tensors
        widths, dts = ctx.cfg
        lib = _lib.load()
        B, O, D = out.shape[0], out.shape[1], sum(widths)
        g = _f32c(g)
        need = ctx.needs_input_grad[2:]
        dparts = [torch.empty_like(t) if n else None for t, n in zip(parts, need)]
        dW = torch.empty_like(kernel)
        db = torch.empty((O,), dtype=torch.float32, device=kernel.device)
        ws = _scratch(lib.fil_merge_softmax_bwd_workspace_bytes(B, D, O), kernel.device, "merge_softmax_bwd")
        dp = (ctypes.c_void_p * len(parts))(*[None if t is None else t.data_ptr() for t in dparts])
        check(lib.fil_merge_softmax_bwd(ptr_array(parts), int_array(widths), int_array(dts), len(parts), ptr(kernel), ptr(out), ptr(g), dp,
                                        ptr(dW), ptr(db), B, O, ptr(ws), ws.numel(), stream_ptr()), "fil_merge_softmax_bwd")
        return (dW, db) + tuple(dparts)


def merge_softmax(parts, kernel, bias):
    """softmax(concat(parts, -1) @ kernel + bias): MergeScoreLayer.call (core_layer.py:86-100) as one launch forward and one backward.
    parts: 1..4 tensors [B, w_i], each fp32 or bf16 (under bf16 autocast a model hands a bf16 FM output next to an fp32 MLP output);
    kernel [sum w_i, O <= 8], bias [O] fp32; returns fp32 [B, O]."""
    parts = list(parts)
    if not 1 <= len(parts) <= 4:
        raise FilError("merge_softmax takes 1..4 parts, got %d" % len(parts))
    if any(t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 2 or t.shape[0] != parts[0].shape[0] for t in parts):
        raise FilError("merge_softmax: the parts must be [B, w] float32 / bfloat16 tensors, got %s" %
                       [(tuple(t.shape), t.dtype) for t in parts])
    if kernel.dim() != 2 or kernel.shape[0] != sum(t.shape[1] for t in parts) or tuple(bias.shape) != (kernel.shape[1],):
        raise FilError("merge_softmax: kernel %s / bias %s do not fit %d concatenated columns" %
                       (tuple(kernel.shape), tuple(bias.shape), sum(t.shape[1] for t in parts)))
    return _MergeSoftmaxFn.apply(kernel, bias, *parts)


class _BceMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, y, eps):
        _require_cuda(p, y)
        if p.shape != y.shape:
            raise FilError("binary_crossentropy: p is %s, y is %s" % (tuple(p.shape), tuple(y.shape)))
        p, y = _f32c(p), _f32c(y)
        if p.numel() == 0:
            raise FilError("binary_crossentropy of an empty batch")
        loss = torch.empty((1,), dtype=torch.float32, device=p.device)
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        check(_lib.load().fil_bce_mean_fwd(ptr(p), ptr(y), float(eps), ptr(loss), ptr(dp), p.numel(), stream_ptr()), "fil_bce_mean_fwd")
        if dp is not None:
            ctx.save_for_backward(dp)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None, None


def binary_crossentropy(p, y, eps=1e-7):
    """mean(-(y log(pc + eps) + (1 - y) log(1 - pc + eps))), pc = clip(p, eps, 1 - eps): tf.losses.binary_crossentropy on
    probabilities as TensorFlow 2.1 computes it (the reference compiles its CTR models with it, example/ctr_example/un_seq.py:61;
    eps = the Keras backend epsilon), as one launch that also leaves d loss / d p; deterministic."""
    return _BceMeanFn.apply(p, y, eps)


# --------------------------------------------------------------------------------------------- M1  Keras' streaming AUC
AUC_CURVES = {"ROC": 0, "PR": 1}
AUC_SUMMATIONS = {"interpolation": 0, "minoring": 1, "majoring": 2}


def confusion_update(p, y, thr, cm, invalid, workspace=None):
    """Keras' update_confusion_matrix_variables for one batch (fil_confusion_update): p, y [n] fp32 (n <= 2^24; y != 0 is a positive),
    thr [T] fp32 ascending, cm [4, T] fp32 = TP | FP | TN | FN and invalid (one int64) updated IN PLACE.  Integer counting, then one
    fp32 add per state entry; samples with p outside [0, 1] or NaN only count in `invalid`.  No host synchronisation: capturable.
    workspace: a uint8 tensor of fil_confusion_workspace_bytes(n, T) bytes (none is needed up to _lib.FIL_CONFUSION_ONE_LAUNCH_N
    samples); allocated here when missing."""
    _require_cuda(p, y, thr, cm, invalid)
    if p.dim() != 1 or p.shape != y.shape:
        raise FilError("confusion_update: p is %s, y is %s (two vectors of one length)" % (tuple(p.shape), tuple(y.shape)))
    p, y, thr = _f32c(p), _f32c(y), _f32c(thr)
    T = thr.numel()
    if cm.dtype != torch.float32 or tuple(cm.shape) != (4, T) or not cm.is_contiguous():
        raise FilError("confusion_update: cm must be a contiguous float32 [4, %d] tensor, got %s %s" % (T, cm.dtype, tuple(cm.shape)))
    if invalid.dtype != torch.int64 or invalid.numel() != 1:
        raise FilError("confusion_update: invalid must be one int64, got %s %s" % (invalid.dtype, tuple(invalid.shape)))
    n = p.numel()
    if n == 0:
        return cm
    lib = _lib.load()
    need = lib.fil_confusion_workspace_bytes(n, T) if n <= (1 << 24) else 0
    if need and workspace is None:
        workspace = _scratch(need, p.device, "confusion")
    check(lib.fil_confusion_update(ptr(p), ptr(y), n, ptr(thr), T, ptr(cm), ptr(invalid), ptr(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), stream_ptr()),
          "fil_confusion_update")
    return cm


def auc_result(cm, curve="ROC", summation="interpolation", out=None):
    """Keras' AUC.result() of cm [4, T] (fil_auc_result) as a 0-dim fp32 device tensor (a view of `out`, one float32, when given):
    one small launch, no host synchronisation."""
    _require_cuda(cm, out)
    if curve not in AUC_CURVES or summation not in AUC_SUMMATIONS:
        raise FilError("auc_result: curve %r (ROC, PR), summation %r (interpolation, minoring, majoring)" % (curve, summation))
    if cm.dtype != torch.float32 or cm.dim() != 2 or cm.shape[0] != 4 or not cm.is_contiguous():
        raise FilError("auc_result: cm must be a contiguous float32 [4, T] tensor, got %s %s" % (cm.dtype, tuple(cm.shape)))
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=cm.device)
    elif out.dtype != torch.float32 or out.numel() != 1:
        raise FilError("auc_result: out must be one float32, got %s %s" % (out.dtype, tuple(out.shape)))
    check(_lib.load().fil_auc_result(ptr(cm), cm.shape[1], AUC_CURVES[curve], AUC_SUMMATIONS[summation], ptr(out), stream_ptr()),
          "fil_auc_result")
    return out.reshape(())


# --------------------------------------------------------------------------------------------- M2  Keras' Mean metrics
MEAN_KINDS = {"values": _lib.FIL_MEAN_VALUES, "binary_crossentropy": _lib.FIL_MEAN_BCE, "binary_accuracy": _lib.FIL_MEAN_BINARY_ACC}


def mean_update(kind, a, y, state, c0=0.0, c1=0.0, workspace=None):
    """One update of a Keras Mean state (fil_mean_update): a [n] fp32 (n <= 2^24) and, except for kind "values", y [n] fp32; state
    [3] fp32 = total | count | result updated IN PLACE: total += sum v, count += n (one fp32 addition each) and result =
    div_no_nan(total, count), all by the same launch.  kind "values": v = a; "binary_crossentropy": Keras' per-sample loss, c0 =
    epsilon, c1 = label_smoothing; "binary_accuracy": v = (y == (a > c0)), c0 = threshold.  No host synchronisation: capturable.
    workspace: a uint8 tensor of fil_mean_workspace_bytes(n) bytes (none is needed up to _lib.FIL_MEAN_ONE_LAUNCH_N samples);
    allocated here when missing."""
    if kind not in MEAN_KINDS:
        raise FilError("mean_update: kind %r (%s)" % (kind, ", ".join(MEAN_KINDS)))
    _require_cuda(a, y, state)
    if kind == "values":
        y = None
    elif y is None:
        raise FilError("mean_update: kind %r needs y" % kind)
    if a.dim() != 1 or (y is not None and a.shape != y.shape):
        raise FilError("mean_update: a is %s, y is %s (vectors of one length)" % (tuple(a.shape), None if y is None else tuple(y.shape)))
    a, y = _f32c(a), _f32c(y)
    if state.dtype != torch.float32 or tuple(state.shape) != (3,) or not state.is_contiguous():
        raise FilError("mean_update: state must be a contiguous float32 [3] tensor, got %s %s" % (state.dtype, tuple(state.shape)))
    n = a.numel()
    if n == 0:
        return state
    lib = _lib.load()
    need = lib.fil_mean_workspace_bytes(n)
    if need and workspace is None:
        workspace = _scratch(need, a.device, "mean")
    check(lib.fil_mean_update(MEAN_KINDS[kind], ptr(a), ptr(y), n, float(c0), float(c1), ptr(state), ptr(workspace),
                              0 if workspace is None else workspace.numel() * workspace.element_size(), stream_ptr()),
          "fil_mean_update")
    return state


_DISJOINT_CACHE = {}


def _fields_disjoint(offsets, sizes, layout_key):
    """True when every field owns its own row range of the concatenated table: offsets ascending and offsets[f] + sizes[f] <=
    offsets[f + 1].  Only then are equal row ids adjacent after a PER-FIELD sort; two fields that share or overlap a table
    (offsets[f] == offsets[g], or no `sizes` to bound the ids) put one row into two runs, and fil_embed_run_sum STORES each run's sum
    -- one would overwrite the other.  Such layouts keep the global sort.  Checked once per layout (one small device -> host copy),
    never during a stream capture (an unchecked layout then takes the global sort)."""
    if sizes is None:
        return False
    key = layout_key if layout_key is not None else (offsets.data_ptr(), offsets._version, sizes.data_ptr(), sizes._version,
                                                     int(offsets.numel()))
    hit = _DISJOINT_CACHE.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            return False
        o, z = offsets.detach().cpu().to(torch.int64), sizes.detach().cpu().to(torch.int64)
        hit = bool(o.numel() == z.numel() and (o.numel() < 2 or bool(((o[:-1] + z[:-1]) <= o[1:]).all())) and bool((z >= 0).all()))
        if len(_DISJOINT_CACHE) > 64:
            _DISJOINT_CACHE.clear()
        _DISJOINT_CACHE[key] = hit
    return hit


def _sorted_row_ids(offsets, sizes, frozen, idx, layout_key=None, n_rows=None, per_field=False):
    """layout_key: a hashable description of (offsets, sizes, frozen) -- two tables with the same field layout (SparseEmbed
    passes its word sizes / frozen flags) share the sort even though their offset tensors are different objects."""
    lib = _lib.load()
    layout = layout_key if layout_key is not None else (
        offsets.data_ptr(), offsets._version, sizes.data_ptr() if sizes is not None else 0,
        frozen.data_ptr() if frozen is not None else 0)
    per_field = per_field and _fields_disjoint(offsets, sizes, layout_key)
    key = (idx.data_ptr(), idx._version, tuple(idx.shape), layout, torch.cuda.current_stream().cuda_stream, bool(per_field))
    for k, _, out in _SORT_CACHE:
        if k == key:
            return out
    B, F = idx.shape
    if per_field and 0 < B <= 8192 and (n_rows is None or n_rows < 2 ** 31):
        # the dense (run-sum) gradient only needs equal row ids adjacent and in a fixed order, and ids of fields with disjoint row
        # ranges (checked above) never collide: one launch sorts every field's (id, position) pairs in LDS (fil.h fil_embed_sort_fields) -- no library sort
        sorted_ids = torch.empty(B * F, dtype=torch.int64, device=idx.device)
        perm = torch.empty(B * F, dtype=torch.int64, device=idx.device)
        check(lib.fil_embed_sort_fields(ptr(offsets), ptr(sizes), ptr(frozen), ptr(idx), ptr(sorted_ids), ptr(perm), B, F,
                                        int(n_rows) if n_rows is not None else 0, stream_ptr()), "fil_embed_sort_fields")
        out = (sorted_ids, perm)
        _SORT_CACHE.insert(0, (key, (idx, offsets, sizes, frozen, _SORT_GEN[0]), out))
        del _SORT_CACHE[2:]
        return out
    row_ids = torch.empty(B * F, dtype=torch.int64, device=idx.device)
    check(lib.fil_embed_row_ids(ptr(offsets), ptr(sizes), ptr(frozen), ptr(idx), ptr(row_ids), B, F, stream_ptr()), "fil_embed_row_ids")
    # (n_rows = rows of the concatenated table: when the global row ids fit 31 bits, 32-bit keys halve the radix passes of the sort)
    # -- only with a range check: `sizes` guarantees every id in [-1, n_rows); unchecked ids could fall outside 32 bits, wrap in the
    # cast, sort out of place and merge with valid rows)
    if sizes is not None and n_rows is not None and n_rows < 2 ** 31 and row_ids.numel() > 0:
        s32, perm = torch.sort(row_ids.to(torch.int32), stable=True)
        out = (s32.to(torch.int64), perm)
    else:
        out = torch.sort(row_ids, stable=True)
    _SORT_CACHE.insert(0, (key, (idx, offsets, sizes, frozen, _SORT_GEN[0]), out))
    del _SORT_CACHE[2:]
    return out


def embed_grad_rows(offsets, sizes, idx, g, frozen=None, layout_key=None, n_rows=None):
    """Deterministic embedding-table gradient as (rows [U] int64, values [U,K]): the unique global table rows the batch
    touched (sorted) and the sum of their gradient rows, contributions added in a fixed order (no atomics).  Out-of-range
    ids and frozen fields (frozen [F] uint8) contribute nothing.  The sort is torch's (plumbing); the sums are the HIP
    segment kernel (fil.h: fil_embed_row_ids / fil_embed_segment_sum)."""
    lib = _lib.load()
    B, F = idx.shape
    K = g.shape[-1]
    g = _f32c(g)
    sorted_ids, perm = _sorted_row_ids(offsets, sizes, frozen, idx, layout_key, n_rows)
    rows, counts = torch.unique_consecutive(sorted_ids, return_counts=True)
    starts = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=g.device)
    torch.cumsum(counts, 0, out=starts[1:])
    values = torch.zeros((rows.numel(), K), dtype=torch.float32, device=g.device)
    check(lib.fil_embed_segment_sum(ptr(g), ptr(perm), ptr(starts), ptr(rows), ptr(values), None, rows.numel(), K, stream_ptr()),
          "fil_embed_segment_sum")
    # the skipped bucket (id -1: out-of-range ids / frozen fields) sorts first and its value row is never written: drop it, so
    # that `rows` really are the unique touched rows (a lazy / sparse optimizer must not see a spurious row 0 every step).
    # Only possible with a range check or frozen fields; unique_consecutive above has synchronised already.
    if (sizes is not None or frozen is not None) and rows.numel() > 0 and bool(rows[0] < 0):
        rows, values = rows[1:], values[1:]
    return rows, values


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, offsets, sizes, idx, frozen, sparse_grad, atomic, oob_count, layout_key=None, xt_out=None, out_dtype=None,
                runs_grad=None):
        _require_cuda(table, offsets, idx)
        ctx.runs_grad = runs_grad
        ctx.sorted = None
        deferred = None
        if runs_grad is not None:
            if sparse_grad or atomic:
                raise FilError("embed_gather: grad_mode='runs' excludes sparse_grad / atomic")
            ctx.table_param = table
            deferred = deferred_state(table)
        table = _f32c(table)
        idx = idx.to(torch.int64).contiguous()
        offsets = offsets.to(torch.int64).contiguous()
        B, F = idx.shape
        K = table.shape[1]
        _SORT_GEN[0] += 1
        prev = _SORT_PREV_TABLE[0]() if _SORT_PREV_TABLE[0] is not None else None
        _SORT_PREV_TABLE[0] = weakref.ref(ctx.table_param) if runs_grad is not None else None
        if deferred is not None:
            # deferred Keras mode (optim.Adam(sweep_period=N)): the batch's rows may lag the completed steps in memory -- sort the
            # batch here and bring its rows current in place before the unchanged gather reads them; the backward reuses the sort.
            # The cache keeps only what the gather just before this one, from ANOTHER table, sorted for this very idx tensor: the
            # other table of the same layout in the same forward shares it, and nothing older is ever reused
            shared = prev is not None and prev is not ctx.table_param
            _SORT_CACHE[:] = [e for e in _SORT_CACHE if shared and e[1][0] is idx and e[1][4] == _SORT_GEN[0] - 1]
            ctx.sorted = _sorted_row_ids(offsets, sizes, frozen, idx, layout_key, table.shape[0], per_field=True)
            deferred.catch_up(ctx.table_param, ctx.sorted[0], runs_grad)
        else:
            del _SORT_CACHE[:]
        out_dtype = out_dtype or torch.float32
        if out_dtype not in (torch.float32, torch.bfloat16) or (xt_out is not None and out_dtype != torch.float32):
            raise FilError("embed_gather: out_dtype %s (float32, or bfloat16 without emit_xt)" % out_dtype)
        out = torch.empty((B, F, K), dtype=out_dtype, device=table.device)
        if xt_out is not None:     # both layouts in one pass: the packed block and its [B*K, F] transpose (fil.h)
            check(_lib.load().fil_embed_gather_xt(ptr(table), ptr(offsets), ptr(sizes), ptr(idx), ptr(out), ptr(xt_out), ptr(oob_count),
                                                  B, F, K, stream_ptr()), "fil_embed_gather_xt")
        else:
            check(_lib.load().fil_embed_gather_dt(ptr(table), ptr(offsets), ptr(sizes), ptr(idx), ptr(out), ptr(oob_count), B, F, K,
                                                  FIL_F32 if out_dtype == torch.float32 else FIL_BF16, stream_ptr()), "fil_embed_gather_dt")
        _save(ctx, offsets, idx, sizes, frozen)
        ctx.cfg = (tuple(table.shape), bool(sparse_grad), bool(atomic), layout_key)
        return out

    @staticmethod
    def backward(ctx, g):
        table_shape, sparse_grad, atomic, layout_key = ctx.cfg
        offsets, idx, sizes, frozen = _saved(ctx)
        B, F = idx.shape
        K = table_shape[1]
        # (a bf16 block's gradient arrives as bf16: the dense deterministic path reads it as it is, the others take fp32)
        g_bf16 = g.dtype == torch.bfloat16 and not atomic and not sparse_grad
        g = g.contiguous() if g_bf16 else _f32c(g)
        if ctx.runs_grad is not None:   # deferred: the optimizer applies the runs in place (optim.Adam / Adagrad / Ftrl)
            table = ctx.table_param
            if getattr(table, "_fil_pending_runs", None) is not None:
                raise FilError("embed_gather(grad_mode='runs'): the table already holds a pending gradient record -- one backward per "
                               "table per optimizer step (call optimizer.step() or zero_grad() in between)")
            sorted_ids, perm = ctx.sorted if ctx.sorted is not None else _sorted_row_ids(offsets, sizes, frozen, idx, layout_key,
                                                                                         table_shape[0], per_field=True)
            table._fil_pending_runs = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=FIL_BF16 if g_bf16 else FIL_F32,
                                           **ctx.runs_grad)
            dtable = None
        elif atomic:      # opt-in: fp32 atomics into a zeroed dense table (order of additions not fixed)
            dtable = torch.zeros(table_shape, dtype=torch.float32, device=g.device)
            check(_lib.load().fil_embed_scatter_add(ptr(offsets), ptr(sizes), ptr(idx), ptr(g), ptr(dtable), B, F, K, stream_ptr()),
                  "fil_embed_scatter_add")
            if frozen is not None:
                raise FilError("embed_gather: frozen fields are not supported by the atomic scatter-add")
        elif sparse_grad:   # what Keras hands its optimizers (IndexedSlices): only the touched rows exist
            rows, values = embed_grad_rows(offsets, sizes, idx, g, frozen, layout_key, table_shape[0])
            dtable = torch.sparse_coo_tensor(rows.unsqueeze(0), values, table_shape)
        else:               # dense table, deterministic, no data-dependent shapes (HIP-graph capturable)
            lib = _lib.load()
            sorted_ids, perm = _sorted_row_ids(offsets, sizes, frozen, idx, layout_key, table_shape[0], per_field=True)
            dtable = torch.zeros(table_shape, dtype=torch.float32, device=g.device)
            check(lib.fil_embed_run_sum_dt(ptr(g), ptr(perm), ptr(sorted_ids), ptr(dtable), B * F, K, FIL_BF16 if g_bf16 else FIL_F32,
                                           stream_ptr()), "fil_embed_run_sum_dt")
        return dtable, None, None, None, None, None, None, None, None, None, None, None


def embed_gather(table, offsets, idx, sizes=None, frozen=None, sparse_grad=False, atomic=False, oob_count=None, layout_key=None,
                 emit_xt=False, out_dtype=None, runs_grad=None):
    """table [sum V_f, K] (all fields concatenated), offsets [F], idx [B,F] -> packed [B,F,K].
    sizes [F] int64: ids outside [0, V_f) give zero rows (counted in oob_count, an int32 device scalar) and no gradient.
    The gradient is deterministic (sorted segment sums); sparse_grad=True returns it as a sparse COO tensor over the touched
    rows instead of a dense table; atomic=True selects the fp32-atomic scatter-add instead.
    runs_grad (a dict: offsets, frozen, field_l2 [F] fp32 or None): the table gets NO gradient; the backward leaves the sorted runs
    (g, perm, sorted_ids) on the table as `table._fil_pending_runs` for optim.Adam, Adagrad, Ftrl, SGD or RMSprop to apply in place
    (fil_embed_adam_runs / fil_embed_rowopt_runs / fil_embed_momopt_runs)."""
    if not emit_xt:   # (out_dtype=torch.bfloat16: the block leaves the gather rounded to bf16 and its gradient is read as bf16 -- no cast launches)
        return _EmbedFn.apply(table, offsets, sizes, idx, frozen, sparse_grad, atomic, oob_count, layout_key, None, out_dtype, runs_grad)
    # emit_xt: the same launch also writes the block transposed to [B*K, F], the layout the CIN kernels read; it rides on the
    # result as `_fil_xt` (the CIN layer picks it up: no second pass over the block)
    B, F = idx.shape
    xt = torch.empty((B * table.shape[1], F), dtype=torch.float32, device=table.device)
    out = _EmbedFn.apply(table, offsets, sizes, idx, frozen, sparse_grad, atomic, oob_count, layout_key, xt, None, runs_grad)
    out._fil_xt = xt
    out._fil_xt_version = out._version      # a consumer ignores xt once the block has been modified in place
    return out


# --------------------------------------------------------------------------------------------- N3  pooled multi-valued fields
BAG_COMBINERS = {"sum": _lib.FIL_BAG_SUM, "mean": _lib.FIL_BAG_MEAN, "sqrtn": _lib.FIL_BAG_SQRTN}


def _bag_combiner(combiner):
    if combiner not in BAG_COMBINERS:
        raise ValueError("embed_bag: combiner %r (%s)" % (combiner, ", ".join(BAG_COMBINERS)))
    return BAG_COMBINERS[combiner]


class _EmbedBagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, offsets, sizes, idx, combiner, pad_id, frozen, sparse_grad, oob_count, runs_grad):
        _require_cuda(table, offsets, idx, sizes, frozen, oob_count)
        if idx.dim() != 3:
            raise FilError("embed_bag: idx must be [B, F, T], got %s" % (tuple(idx.shape),))
        if deferred_state(table) is not None:
            raise FilError("embed_bag: the table is in deferred Keras mode (optim.Adam(sweep_period=N)); a pooled field's rows are not "
                           "brought current by its forward -- deferred Adam on bag tables is not supported")
        if runs_grad is not None and sparse_grad:
            raise FilError("embed_bag: grad_mode='runs' excludes sparse_grad")
        ctx.runs_grad = runs_grad
        ctx.table_param = table if runs_grad is not None else None
        table = _f32c(table)
        idx = idx.to(torch.int64).contiguous()
        offsets = offsets.to(torch.int64).contiguous()
        B, F, T = idx.shape
        K = table.shape[1]
        if offsets.numel() != F:
            raise FilError("embed_bag: idx has %d fields, offsets %d" % (F, offsets.numel()))
        out = torch.empty((B, F, K), dtype=torch.float32, device=table.device)
        count = torch.empty((B, F), dtype=torch.int32, device=table.device)
        check(_lib.load().fil_embed_bag_fwd(ptr(table), ptr(offsets), ptr(sizes), ptr(idx), pad_id, ptr(out), ptr(count), ptr(oob_count),
                                            B, F, T, K, combiner, stream_ptr()), "fil_embed_bag_fwd")
        _save(ctx, offsets, idx, count, sizes, frozen)
        ctx.cfg = (tuple(table.shape), bool(sparse_grad), combiner, pad_id)
        return out

    @staticmethod
    def backward(ctx, g):
        table_shape, sparse_grad, combiner, pad_id = ctx.cfg
        offsets, idx, count, sizes, frozen = _saved(ctx)
        B, F, T = idx.shape
        K = table_shape[1]
        R = B * F * T
        lib = _lib.load()
        g = _f32c(g)
        table = ctx.table_param
        if table is not None and getattr(table, "_fil_pending_runs", None) is not None:
            raise FilError("embed_bag(grad_mode='runs'): the table already holds a pending gradient record -- one backward per "
                           "table per optimizer step (call optimizer.step() or zero_grad() in between)")
        # the slots' global row ids, their stable sort (plumbing: torch's; 32-bit keys when the row ids fit, as the one-id gradient's
        # global sort), then one launch: the rows divided by the forward's divisor and every sorted slot mapped back to its bag
        row_ids = torch.empty(R, dtype=torch.int64, device=g.device)
        check(lib.fil_embed_bag_row_ids(ptr(offsets), ptr(sizes), ptr(frozen), ptr(idx), pad_id, ptr(row_ids), B, F, T, stream_ptr()),
              "fil_embed_bag_row_ids")
        if sizes is not None and table_shape[0] < 2 ** 31 and R > 0:
            s32, perm = torch.sort(row_ids.to(torch.int32), stable=True)
            sorted_ids = s32.to(torch.int64)
        else:
            sorted_ids, perm = torch.sort(row_ids, stable=True)
        gs = g if combiner == _lib.FIL_BAG_SUM else torch.empty_like(g)
        check(lib.fil_embed_bag_bwd_prep(ptr(g), ptr(count), ptr(perm), None if gs is g else ptr(gs), ptr(perm), B, F, T, K, combiner,
                                         stream_ptr()), "fil_embed_bag_bwd_prep")
        if table is not None:     # the optimizer applies the runs in place: a record of the form embed_gather's backward leaves
            table._fil_pending_runs = dict(g=gs, perm=perm, sorted_ids=sorted_ids, R=R, K=K, F=F, g_dtype=FIL_F32, **ctx.runs_grad)
            dtable = None
        elif sparse_grad:         # the touched rows only: the record compacted by the dense gradient's own walk (the same bits)
            cap = max(R, 1)
            rows = torch.empty(cap, dtype=torch.int64, device=g.device)
            values = torch.empty((cap, K), dtype=torch.float32, device=g.device)
            n_rows = torch.zeros(1, dtype=torch.int64, device=g.device)
            if R > 0:
                ws = _scratch(lib.fil_embed_runs_compact_workspace_bytes(R), g.device, "embed_bag_compact")
                check(lib.fil_embed_runs_compact(ptr(gs), ptr(perm), ptr(sorted_ids), R, K, FIL_F32, ptr(rows), ptr(values), ptr(n_rows), cap,
                                                 ptr(ws), ws.numel(), stream_ptr()), "fil_embed_runs_compact")
            u = int(n_rows)       # (a sparse tensor has a data-dependent shape: this path synchronises, as embed_gather's does)
            dtable = torch.sparse_coo_tensor(rows[:u].unsqueeze(0), values[:u], table_shape)
        else:                     # dense table, deterministic, no data-dependent shapes (HIP-graph capturable)
            dtable = torch.zeros(table_shape, dtype=torch.float32, device=g.device)
            check(lib.fil_embed_run_sum_dt(ptr(gs), ptr(perm), ptr(sorted_ids), ptr(dtable), R, K, FIL_F32, stream_ptr()),
                  "fil_embed_run_sum_dt")
        return dtable, None, None, None, None, None, None, None, None, None


def embed_bag(table, offsets, idx, sizes=None, combiner="mean", padding_id=0, frozen=None, sparse_grad=False, oob_count=None,
              runs_grad=None):
    """Pooled multi-valued fields (tf.nn.safe_embedding_lookup_sparse without weights): table [sum V_f, K], offsets [F], idx [B,F,T]
    (T padded slots per sample and field) -> [B,F,K] = combiner over each bag's live rows, in one launch (fil_embed_bag_fwd).
    A slot is padding iff its id == padding_id (default 0, Keras' mask_zero: row 0 of a field is never read or updated; None: no
    id is padding).  With sizes [F] int64, a non-padding id outside [0, V_f) contributes nothing, is counted in oob_count (an int32
    device scalar) and gets no gradient.  combiner: "sum"; "mean" = the sum divided by the number n of live slots; "sqrtn" = divided
    by sqrt(n); n = 0 gives a zero row.  fp32 additions in slot order and one division: bit-equal to the sequential restatement.
    The gradient is deterministic (the slots' sorted run sums, no atomics): a dense table by default, a sparse COO tensor over the
    touched rows with sparse_grad=True; runs_grad (embed_gather's dict) leaves the record on the table as `_fil_pending_runs` for
    the fused optimizers of ml_function_amd.optim instead.  frozen [F] uint8: fields whose rows get no gradient."""
    pad = _lib.FIL_BAG_NO_PAD if padding_id is None else int(padding_id)
    return _EmbedBagFn.apply(table, offsets, sizes, idx, _bag_combiner(combiner), pad, frozen, sparse_grad, oob_count, runs_grad)
