"""fp64 restatement of the view-masked, pooled self-attention (include/fil.h fil_seqattn_*_v, functional.seq_view_attention): the
forward and the hand-derived backward, the torch graph of the same math (fp64: the autograd check of the backward; fp32: the
restatement whose own error E32 sets the tests' bars), and make_case().  tests/seq_attn_ref.py (the operator without views) lends its
masks, its error measures, its bars and the idea of the conditioned seed.

    x [B,T,K], mask [B,T] (non-zero = live; None = all live), Wq, Wk, Wv [K,H D], view in VIEWS, split S.  q = x Wq, k = x Wk,
    v = x Wv; per head: s_ij = q_i . k_j (/ sqrt(D) when use_scale).  The keys row i may see: A_i = {j live and allowed(i, j)},
        full: every j;   causal: j <= i;   cross: (i < S) != (j < S), 1 <= S <= T-1.
    p_ij = softmax of s_ij over A_i;  out_i = sum over A_i of p_ij v_j for a live i with a non-empty A_i, else 0 (and such a row sends
    no gradient).  pooled[b] = (sum of out_i over the live i) / n_b, n_b = the live rows of b; zeros for n_b = 0.
    The upstream gradient is g [B,T,H D], or for the pooled form gpool [B,H D]: every live row then takes g_i = gpool[b] / n_b."""
import numpy as np
import torch

from tests.seq_attn_ref import GRADS, MAX_COND, PARAMS, PARAMS_GRADS, bars, make_mask, norm_rel      # noqa: F401 (re-exported)
from tests import seq_attn_ref as base

VIEWS = ("full", "causal", "cross")


def allowed(view, split, T):
    """[T,T] bool: allowed[i, j] = row i may see key j."""
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    if view == "full":
        assert split == 0
        return np.ones((T, T), bool)
    if view == "causal":
        assert split == 0
        return j <= i
    assert view == "cross" and 1 <= split <= T - 1, (view, split, T)
    return (i < split) != (j < split)


def _live(case):
    B, T, _ = np.shape(case["x"])
    return np.ones((B, T), bool) if case.get("mask") is None else np.asarray(case["mask"]).astype(bool)


def _parts(case):
    f = lambda k: np.asarray(case[k], np.float64)
    x, Wq, Wk, Wv = (f(k) for k in ("x",) + PARAMS)
    B, T, K = x.shape
    H = case["heads"]
    D = Wq.shape[1] // H
    live = _live(case)
    x = np.where(live[:, :, None], x, 0.0)
    heads = lambda w: (x @ w).reshape(B, T, H, D).transpose(0, 2, 1, 3)          # [B,H,T,D]
    q, k, v = heads(Wq), heads(Wk), heads(Wv)
    scale = 1.0 / np.sqrt(D) if case.get("use_scale", True) else 1.0
    s = np.einsum("bhid,bhjd->bhij", q, k) * scale
    see = live[:, None, None, :] & allowed(case.get("view", "full"), case.get("split", 0), T)[None, None]      # [B,1,T,T]
    s = np.where(see, s, -np.inf)
    m = np.where(see.any(-1, keepdims=True), s.max(-1, keepdims=True), 0.0)
    e = np.where(see, np.exp(s - m), 0.0)
    den = e.sum(-1, keepdims=True)
    p = np.where(den > 0, e / np.where(den > 0, den, 1.0), 0.0)
    p = p * live[:, None, :, None]                                               # a masked row gives nothing and takes no gradient
    return dict(x=x, Wq=Wq, Wk=Wk, Wv=Wv, q=q, k=k, v=v, p=p, live=live, see=see, scale=scale, H=H, D=D)


def rows(case):
    """-> out [B,T,H D] float64, whatever case["pool"] says."""
    P = _parts(case)
    B, T, _ = P["x"].shape
    return np.einsum("bhij,bhjd->bhid", P["p"], P["v"]).transpose(0, 2, 1, 3).reshape(B, T, P["H"] * P["D"])


def pool_rows(out, live):
    """The mean over the live rows, [B,T,C] -> [B,C]; zeros for a sample without one."""
    n = live.sum(1)
    total = np.where(live[:, :, None], out, 0.0).sum(1)
    return np.where(n[:, None] > 0, total / np.maximum(n, 1)[:, None], 0.0)


def forward(case):
    """-> what the op returns: pooled [B,H D] for case["pool"], else out [B,T,H D]; float64."""
    out = rows(case)
    return pool_rows(out, _live(case)) if case.get("pool") else out


def g_rows(case):
    """The upstream gradient of the rows, [B,T,H D] float64, zero at masked rows: case["g"], or gpool[b] / n_b for the pooled form."""
    live = _live(case)
    if case.get("pool"):
        gp = np.asarray(case["gpool"], np.float64)
        g = gp[:, None, :] / np.maximum(live.sum(1), 1)[:, None, None] * np.ones(live.shape)[:, :, None]
    else:
        g = np.asarray(case["g"], np.float64)
    return np.where(live[:, :, None], g, 0.0)


def backward(case):
    """-> dict of GRADS, float64, by the chain rule written out; v_rows: v [B,T,H D]; ds: the score gradients [B,H,T,T]; cond: the
    conditioning (sum of |terms| / |sum|, in norms) of the sums over (b, t) behind dWq, dWk and dWv."""
    P = _parts(case)
    x, p, q, k, v, live = P["x"], P["p"], P["q"], P["k"], P["v"], P["live"]
    B, T, K = x.shape
    H, D = P["H"], P["D"]
    g = g_rows(case).reshape(B, T, H, D).transpose(0, 2, 1, 3)
    dv = np.einsum("bhij,bhid->bhjd", p, g)
    dp = np.einsum("bhid,bhjd->bhij", g, v)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    dq = np.einsum("bhij,bhjd->bhid", ds, k) * P["scale"]
    dk = np.einsum("bhij,bhid->bhjd", ds, q) * P["scale"]
    flat = lambda t: t.transpose(0, 2, 1, 3).reshape(B, T, H * D)
    dq, dk, dv = flat(dq), flat(dk), flat(dv)
    dx = dq @ P["Wq"].T + dk @ P["Wk"].T + dv @ P["Wv"].T
    dx = np.where(live[:, :, None], dx, 0.0)
    res = dict(dx=dx, v_rows=flat(v), ds=ds, cond={})
    for name, d in (("dWq", dq), ("dWk", dk), ("dWv", dv)):
        res[name] = np.einsum("btk,btc->kc", x, d)
        res["cond"][name] = float(np.linalg.norm(np.einsum("btk,btc->kc", np.abs(x), np.abs(d))) / max(np.linalg.norm(res[name]), 1e-300))
    return res


def torch_graph(x, mask, Wq, Wk, Wv, heads, use_scale=True, view="full", split=0, pool=False):
    """The same math as torch ops on the tensors given (their dtype; autograd for the backward) -> out [B,T,H D] or pooled [B,H D]."""
    B, T, K = x.shape
    H = heads
    D = Wq.shape[1] // H
    zero = torch.zeros((), dtype=x.dtype)
    live = torch.ones((B, T), dtype=torch.bool) if mask is None else mask
    x = torch.where(live.unsqueeze(-1), x, zero)
    q, k, v = (torch.matmul(x, w).reshape(B, T, H, D).permute(0, 2, 1, 3) for w in (Wq, Wk, Wv))
    s = torch.matmul(q, k.transpose(-1, -2))
    if use_scale:
        s = s * (1.0 / float(D) ** 0.5)
    see = live.reshape(B, 1, 1, T) & torch.tensor(allowed(view, split, T)).reshape(1, 1, T, T)
    s = torch.where(see, s, torch.full((), -float("inf"), dtype=s.dtype))
    m = torch.where(see.any(dim=-1, keepdim=True), s.detach().max(dim=-1, keepdim=True).values, zero)
    e = torch.where(see, torch.exp(s - m), zero)
    p = e / e.sum(dim=-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)
    out = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, H * D)
    out = torch.where(live.unsqueeze(-1), out, zero)
    if not pool:
        return out
    n = live.sum(dim=1, keepdim=True).to(out.dtype)
    return torch.where(n > 0, out.sum(dim=1) / n.clamp_min(1.0), zero)


def torch_run(case, dtype, graph=torch_graph):
    """out and the gradients of `graph` on the CPU in `dtype`, as float64 numpy arrays (out + the keys of GRADS)."""
    names = ("x",) + PARAMS
    t = {k: torch.tensor(np.asarray(case[k]), dtype=dtype, requires_grad=True) for k in names}
    mask = None if case.get("mask") is None else torch.tensor(np.asarray(case["mask"]).astype(bool))
    pool = bool(case.get("pool"))
    out = graph(t["x"], mask, t["Wq"], t["Wk"], t["Wv"], case["heads"], case.get("use_scale", True), case.get("view", "full"),
                case.get("split", 0), pool)
    g = torch.tensor(np.asarray(case["gpool" if pool else "g"]), dtype=dtype)
    if mask is not None and not pool:
        g = torch.where(mask.unsqueeze(-1), g, torch.zeros((), dtype=dtype))
    (out * g).sum().backward()
    D = lambda v: v.detach().double().numpy()
    res = dict(out=D(out))
    for k in names:
        res["d" + k] = D(t[k].grad) if t[k].grad is not None else np.zeros(t[k].shape)
    return res


def make_case(B, T, K, H, D, seed, view="full", split=0, pool=False, mask="ragged", w_scale=1.0, use_scale=True):
    """seq_attn_ref.make_case's draws (the same x, weights, mask and g for the same seed) plus gpool ~ N(0,1) [B,H D], the view, the
    split and the form."""
    case = base.make_case(B, T, K, H, D, seed, mask=mask, w_scale=w_scale, use_scale=use_scale)
    rng = np.random.default_rng([seed, 77])
    case["gpool"] = np.asarray(rng.standard_normal((B, H * D)), np.float32).astype(np.float64)
    case.update(view=view, split=int(split), pool=bool(pool))
    return case


def conditioned_case(B, T, K, H, D, **kw):
    """make_case with the first seed in 0 .. 99 whose sums over (b, t) (backward()'s cond) have a conditioning of at most MAX_COND and
    are not zero (seq_attn_ref.conditioned_case says why).  The choice reads the fp64 reference only."""
    for seed in range(100):
        case = make_case(B, T, K, H, D, seed, **kw)
        bw = backward(case)
        if all(np.any(bw[k]) for k in PARAMS_GRADS) and max(bw["cond"].values()) <= MAX_COND:
            case["seed"] = seed
            return case
    raise AssertionError("conditioned_case: no seed in 0 .. 99 gives conditioning <= %g for %s %s" % (MAX_COND, (B, T, K, H, D), kw))


def errors(got, out_ref, bwd_ref):
    """got: dict(out, GRADS...) -> the same keys (those present in got and not None): norm-relative error against the fp64 reference."""
    res = {}
    for k, v in got.items():
        if v is None:
            continue
        if k == "out":
            res[k] = norm_rel(np.asarray(v).reshape(out_ref.shape), out_ref)
        elif k in GRADS:
            res[k] = norm_rel(np.asarray(v).reshape(bwd_ref[k].shape), bwd_ref[k])
    return res


_REF_CACHE = {}


def reference(case):
    """(out, backward dict, E32 dict) of a case, computed once per case object."""
    key = id(case)
    hit = _REF_CACHE.get(key)
    if hit is None or hit[0] is not case:
        out, bwd = forward(case), backward(case)
        e32 = errors(torch_run(case, torch.float32), out, bwd)
        hit = _REF_CACHE[key] = (case, out, bwd, e32)
    return hit[1], hit[2], hit[3]
