"""fp64 restatement of the masked multi-head self-attention over a behaviour sequence (include/fil.h N3 fil_seqattn_*,
ml_function_amd.functional.seq_self_attention): the forward and the hand-derived backward, the torch graph of the same math (fp64: the
autograd check of the backward; fp32: the restatement whose own error E32 sets the tests' bars), the error measures and make_case().

    x [B,T,K], mask [B,T] (non-zero = live; None = all live), Wq, Wk, Wv [K,H D].  q = x Wq, k = x Wk, v = x Wv; per head h:
        s_ij = q_i . k_j (/ sqrt(D) when use_scale);  p_ij = softmax of s_ij over the live j;  out_i = sum_j p_ij v_j for a live i,
        0 for a masked i.  The upstream gradient is g [B,T,H D]; a masked position's x and g rows are never used."""
import numpy as np
import torch

PARAMS = ("Wq", "Wk", "Wv")
GRADS = ("dx", "dWq", "dWk", "dWv")


def _live(mask, B, T):
    return np.ones((B, T), bool) if mask is None else np.asarray(mask).astype(bool)


def _parts(case):
    f = lambda k: np.asarray(case[k], np.float64)
    x, Wq, Wk, Wv = (f(k) for k in ("x",) + PARAMS)
    B, T, K = x.shape
    H = case["heads"]
    D = Wq.shape[1] // H
    live = _live(case.get("mask"), B, T)
    x = np.where(live[:, :, None], x, 0.0)
    heads = lambda w: (x @ w).reshape(B, T, H, D).transpose(0, 2, 1, 3)          # [B,H,T,D]
    q, k, v = heads(Wq), heads(Wk), heads(Wv)
    scale = 1.0 / np.sqrt(D) if case.get("use_scale", True) else 1.0
    s = np.einsum("bhid,bhjd->bhij", q, k) * scale
    s = np.where(live[:, None, None, :], s, -np.inf)
    m = np.where(live.any(1)[:, None, None, None], s.max(-1, keepdims=True), 0.0)
    e = np.where(live[:, None, None, :], np.exp(s - m), 0.0)
    den = e.sum(-1, keepdims=True)
    p = np.where(den > 0, e / np.where(den > 0, den, 1.0), 0.0)
    p = p * live[:, None, :, None]                                               # a masked row gives nothing and takes no gradient
    return dict(x=x, Wq=Wq, Wk=Wk, Wv=Wv, q=q, k=k, v=v, p=p, live=live, scale=scale, H=H, D=D)


def forward(case):
    """-> out [B,T,H D] float64."""
    P = _parts(case)
    B, T, _ = P["x"].shape
    return np.einsum("bhij,bhjd->bhid", P["p"], P["v"]).transpose(0, 2, 1, 3).reshape(B, T, P["H"] * P["D"])


def backward(case):
    """g [B,T,H D] -> dict of GRADS, float64, by the chain rule written out; v_rows: v [B,T,H D] (what a sample with one live slot
    returns); ds: the score gradients [B,H,T,T]; cond: the conditioning (sum of |terms| / |sum|, in norms) of the sums over (b, t)
    behind dWq, dWk and dWv."""
    P = _parts(case)
    x, p, q, k, v, live = P["x"], P["p"], P["q"], P["k"], P["v"], P["live"]
    B, T, K = x.shape
    H, D = P["H"], P["D"]
    g = np.where(live[:, :, None], np.asarray(case["g"], np.float64), 0.0).reshape(B, T, H, D).transpose(0, 2, 1, 3)
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


def torch_graph(x, mask, Wq, Wk, Wv, heads, use_scale=True):
    """The same math as torch ops on the tensors given (their dtype; autograd for the backward) -> out [B,T,H D]."""
    B, T, K = x.shape
    H = heads
    D = Wq.shape[1] // H
    zero = torch.zeros((), dtype=x.dtype)
    if mask is not None:
        x = torch.where(mask.unsqueeze(-1), x, zero)
    q, k, v = (torch.matmul(x, w).reshape(B, T, H, D).permute(0, 2, 1, 3) for w in (Wq, Wk, Wv))
    s = torch.matmul(q, k.transpose(-1, -2))
    if use_scale:
        s = s * (1.0 / float(D) ** 0.5)
    if mask is None:
        p = torch.softmax(s, dim=-1)
    else:
        key_live = mask.reshape(B, 1, 1, T)
        s = torch.where(key_live, s, torch.full((), -float("inf"), dtype=s.dtype))
        m = torch.where(mask.any(dim=1).reshape(B, 1, 1, 1), s.detach().max(dim=-1, keepdim=True).values, zero)
        e = torch.where(key_live, torch.exp(s - m), zero)
        p = e / e.sum(dim=-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)
    out = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, H * D)
    return out if mask is None else torch.where(mask.unsqueeze(-1), out, zero)


def torch_run(case, dtype):
    """out and the gradients of torch_graph on the CPU in `dtype`, as float64 numpy arrays (the keys of backward())."""
    names = ("x",) + PARAMS
    t = {k: torch.tensor(np.asarray(case[k]), dtype=dtype, requires_grad=True) for k in names}
    mask = None if case.get("mask") is None else torch.tensor(np.asarray(case["mask"]).astype(bool))
    out = torch_graph(t["x"], mask, t["Wq"], t["Wk"], t["Wv"], case["heads"], case.get("use_scale", True))
    g = torch.tensor(np.asarray(case["g"]), dtype=dtype)
    if mask is not None:
        g = torch.where(mask.unsqueeze(-1), g, torch.zeros((), dtype=dtype))
    (out * g).sum().backward()
    D = lambda v: v.detach().double().numpy()
    res = dict(out=D(out))
    for k in names:
        res["d" + k] = D(t[k].grad) if t[k].grad is not None else np.zeros(t[k].shape)
    return res


def make_mask(B, T, kind, rng):
    """None (all live), "ragged" (0 .. T live slots per sample at random positions), "prefix" (the first 1 .. T slots), or an array."""
    if kind is None or not isinstance(kind, str):
        return None if kind is None else np.asarray(kind).astype(np.uint8)
    m = np.zeros((B, T), np.uint8)
    for b in range(B):
        if kind == "ragged":
            m[b, rng.permutation(T)[:rng.integers(0, T + 1)]] = 1
        else:
            assert kind == "prefix", kind
            m[b, :rng.integers(1, T + 1)] = 1
    return m


def make_case(B, T, K, H, D, seed, mask="ragged", w_scale=1.0, use_scale=True):
    """x ~ 0.5 N(0,1), Wq / Wk / Wv glorot-scaled normal (Wq, Wk times w_scale: 24 makes every row peaked), g ~ N(0,1), ragged lengths
    0 .. T; all fp32-representable (returned as float64 arrays)."""
    rng = np.random.default_rng(seed)
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    std = np.sqrt(2.0 / (K + H * D))
    return dict(shape=(B, T, K, H, D), heads=H, use_scale=use_scale,
                Wq=r32(rng.standard_normal((K, H * D)) * std * w_scale),
                Wk=r32(rng.standard_normal((K, H * D)) * std * w_scale),
                Wv=r32(rng.standard_normal((K, H * D)) * std),
                x=r32(rng.standard_normal((B, T, K)) * 0.5),
                mask=make_mask(B, T, mask, rng),
                g=r32(rng.standard_normal((B, T, H * D))))


MAX_COND = 64.0


def conditioned_case(B, T, K, H, D, **kw):
    """make_case with the first seed in 0 .. 99 whose sums over (b, t) (backward()'s cond: dWq, dWk, dWv) have a conditioning of at
    most MAX_COND and are not zero: for the cases of a handful of positions, where a single draw decides how many digits a cancelling
    sum keeps.  The choice reads the fp64 reference only."""
    for seed in range(100):
        case = make_case(B, T, K, H, D, seed, **kw)
        bw = backward(case)
        if all(np.any(bw[k]) for k in PARAMS_GRADS) and max(bw["cond"].values()) <= MAX_COND:
            case["seed"] = seed
            return case
    raise AssertionError("conditioned_case: no seed in 0 .. 99 gives conditioning <= %g for %s" % (MAX_COND, (B, T, K, H, D)))


PARAMS_GRADS = ("dWq", "dWk", "dWv")


def norm_rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def errors(got, out_ref, bwd_ref):
    """got: dict(out, GRADS...) -> the same keys (those present in got and not None): norm-relative error against the fp64 reference."""
    res = {}
    for k, v in got.items():
        if v is None:
            continue
        if k == "out":
            res[k] = norm_rel(v, out_ref)
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


def bars(e32):
    """max(1e-5, 4 E32) per tensor: 1e-5 is the standing bar of the fp32 kernels against the fp64 oracle, E32 the error of the fp32
    torch restatement of the same graph on the same inputs; the factor 4 covers another summation order and the device's expf."""
    return {k: max(1e-5, 4.0 * v) for k, v in e32.items()}
