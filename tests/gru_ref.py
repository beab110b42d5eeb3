"""fp64 restatement of the GRU / AUGRU / AGRU over a behaviour sequence (include/fil.h N3 fil_gru_*, ml_function_amd.functional.gru):
the forward and the hand-derived backward written out step by step, the torch graph of the same math (fp64: the autograd check of the
backward; fp32: the restatement whose own error E32 sets the tests' bars), the error measures and make_case().

    x [B,T,K], a [B,T] (None in mode "gru"), mask [B,T] (non-zero = live; None = all live), W [K,3H], U [H,3H] (columns z | r | h),
    b [2,3H] (input bias, recurrent bias).  One live step, h = the previous state, h_0 = 0:
        xp = x_t W + b[0];  hp = h U + b[1];  z = sigmoid(xp_z + hp_z);  r = sigmoid(xp_r + hp_r);  c = tanh(xp_h + r hp_h);
        u = 1 - z;  u' = u (gru) | a_t u (augru) | a_t (agru);  h_new = (1 - u') h + u' c.
    A masked step carries the state.  The upstream gradients are g_hs [B,T,H] and / or g_last [B,H] (of hs[:, T-1])."""
import numpy as np
import torch

MODES = ("gru", "augru", "agru")
PARAMS = ("W", "U", "b")
GRADS = ("dx", "da", "dW", "dU", "db")


def _live(mask, B, T):
    return np.ones((B, T), bool) if mask is None else np.asarray(mask).astype(bool)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _steps(case):
    """The forward, keeping what the backward needs of every step."""
    f = lambda k: None if case.get(k) is None else np.asarray(case[k], np.float64)
    x, a, W, U, b = (f(k) for k in ("x", "a", "W", "U", "b"))
    B, T, K = x.shape
    H = U.shape[0]
    mode = case["mode"]
    live = _live(case.get("mask"), B, T)
    x = np.where(live[:, :, None], x, 0.0)                   # a masked step's x and a are never used
    a = np.ones((B, T)) if a is None else np.where(live, a, 0.0)
    h = np.zeros((B, H))
    hs = np.zeros((B, T, H))
    keep = []
    for t in range(T):
        xp = x[:, t] @ W + b[0]
        hp = h @ U + b[1]
        z = _sig(xp[:, :H] + hp[:, :H])
        r = _sig(xp[:, H:2 * H] + hp[:, H:2 * H])
        c = np.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
        u = 1.0 - z
        at = a[:, t:t + 1]
        up = u if mode == "gru" else (at * u if mode == "augru" else np.broadcast_to(at, u.shape))
        hn = (1.0 - up) * h + up * c
        keep.append(dict(h=h, z=z, r=r, c=c, u=u, up=up, hph=hp[:, 2 * H:], at=at))
        h = np.where(live[:, t:t + 1], hn, h)
        hs[:, t] = h
    return dict(x=x, a=a, W=W, U=U, live=live, hs=hs, keep=keep, H=H)


def forward(case):
    """-> hs [B,T,H] float64."""
    return _steps(case)["hs"]


def backward(case):
    """g_hs [B,T,H] and / or g_last [B,H] -> dict of GRADS (da: zeros in mode "gru"), float64, by the chain rule written out, and
    cond: the conditioning (sum of |terms| / |sum|, in norms) of the sums over (b, t) behind dW, dU and db."""
    p = _steps(case)
    x, W, U, live, H, mode = p["x"], p["W"], p["U"], p["live"], p["H"], case["mode"]
    B, T, K = x.shape
    g_hs = None if case.get("g_hs") is None else np.asarray(case["g_hs"], np.float64)
    dh = np.zeros((B, H)) if case.get("g_last") is None else np.asarray(case["g_last"], np.float64).copy()
    dx, da = np.zeros((B, T, K)), np.zeros((B, T))
    dW, dU, db = np.zeros_like(W), np.zeros_like(U), np.zeros((2, 3 * H))
    aW, aU, ab = np.zeros_like(W), np.zeros_like(U), np.zeros((2, 3 * H))
    for t in range(T - 1, -1, -1):
        s = p["keep"][t]
        lv = live[:, t:t + 1]
        if g_hs is not None:
            dh = dh + g_hs[:, t]
        dup = dh * (s["c"] - s["h"])                          # d h_new / d u'
        if mode == "gru":
            du = dup
        elif mode == "augru":
            du = s["at"] * dup
            da[:, t] = np.where(lv[:, 0], (dup * s["u"]).sum(1), 0.0)
        else:
            du = np.zeros_like(dup)
            da[:, t] = np.where(lv[:, 0], dup.sum(1), 0.0)
        dzp = np.where(lv, -du * s["z"] * (1.0 - s["z"]), 0.0)                 # u = 1 - z
        dcp = np.where(lv, dh * s["up"] * (1.0 - s["c"] ** 2), 0.0)
        drp = dcp * s["hph"] * s["r"] * (1.0 - s["r"])
        dxp = np.concatenate([dzp, drp, dcp], 1)
        dhp = np.concatenate([dzp, drp, dcp * s["r"]], 1)
        dx[:, t] = dxp @ W.T
        dW += x[:, t].T @ dxp
        dU += s["h"].T @ dhp
        db[0] += dxp.sum(0)
        db[1] += dhp.sum(0)
        aW += np.abs(x[:, t]).T @ np.abs(dxp)
        aU += np.abs(s["h"]).T @ np.abs(dhp)
        ab[0] += np.abs(dxp).sum(0)
        ab[1] += np.abs(dhp).sum(0)
        dh = np.where(lv, dh * (1.0 - s["up"]) + dhp @ U.T, dh)
    cond_of = lambda ab_, v: float(np.linalg.norm(ab_) / max(np.linalg.norm(v), 1e-300))
    return dict(dx=dx, da=da, dW=dW, dU=dU, db=db, cond=dict(dW=cond_of(aW, dW), dU=cond_of(aU, dU), db=cond_of(ab, db)))


def torch_graph(x, a, mask, W, U, b, mode="gru"):
    """The same math as torch ops on the tensors given (their dtype; autograd for the backward) -> hs [B,T,H]."""
    B, T, K = x.shape
    H = U.shape[0]
    zero = torch.zeros((), dtype=x.dtype)
    if mask is not None:
        x = torch.where(mask.unsqueeze(-1), x, zero)
        if a is not None:
            a = torch.where(mask, a, zero)
    h = torch.zeros((B, H), dtype=x.dtype)
    out = []
    for t in range(T):
        xp = torch.matmul(x[:, t], W) + b[0]
        hp = torch.matmul(h, U) + b[1]
        z = torch.sigmoid(xp[:, :H] + hp[:, :H])
        r = torch.sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
        c = torch.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
        up = 1 - z
        if mode == "augru":
            up = a[:, t:t + 1] * up
        elif mode == "agru":
            up = a[:, t:t + 1].expand(B, H)
        hn = (1 - up) * h + up * c
        h = hn if mask is None else torch.where(mask[:, t:t + 1], hn, h)
        out.append(h)
    return torch.stack(out, 1)


def torch_run(case, dtype):
    """hs and the gradients of torch_graph on the CPU in `dtype`, as float64 numpy arrays (the keys of backward())."""
    names = ("x",) + (("a",) if case.get("a") is not None else ()) + PARAMS
    t = {k: torch.tensor(np.asarray(case[k]), dtype=dtype, requires_grad=True) for k in names}
    mask = None if case.get("mask") is None else torch.tensor(np.asarray(case["mask"]).astype(bool))
    hs = torch_graph(t["x"], t.get("a"), mask, t["W"], t["U"], t["b"], mode=case["mode"])
    loss = torch.zeros((), dtype=dtype)
    if case.get("g_hs") is not None:
        loss = loss + (hs * torch.tensor(np.asarray(case["g_hs"]), dtype=dtype)).sum()
    if case.get("g_last") is not None:
        loss = loss + (hs[:, -1] * torch.tensor(np.asarray(case["g_last"]), dtype=dtype)).sum()
    loss.backward()
    D = lambda v: v.detach().double().numpy()
    res = dict(hs=D(hs))
    for k in names:
        res["d" + k] = D(t[k].grad) if t[k].grad is not None else np.zeros(t[k].shape)
    if "da" not in res:
        res["da"] = np.zeros(case["x"].shape[:2])
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


def make_case(B, T, K, H, mode, seed, mask="ragged", grads="both", u_scale=1.5):
    """x ~ 0.5 N(0,1), a ~ U(0,1) (None in mode "gru"), W glorot-scaled normal, U u_scale x glorot, b ~ 0.1 N(0,1), g ~ N(0,1), ragged
    lengths 0 .. T; all fp32-representable (returned as float64 arrays).  grads: "both" (g_hs and g_last), "hs" or "last"."""
    rng = np.random.default_rng(seed)
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return dict(mode=mode, shape=(B, T, K, H),
                W=r32(rng.standard_normal((K, 3 * H)) * np.sqrt(2.0 / (K + 3 * H))),
                U=r32(rng.standard_normal((H, 3 * H)) * np.sqrt(2.0 / (4 * H)) * u_scale),
                b=r32(rng.standard_normal((2, 3 * H)) * 0.1),
                x=r32(rng.standard_normal((B, T, K)) * 0.5),
                a=None if mode == "gru" else r32(rng.uniform(0, 1, (B, T))),
                mask=make_mask(B, T, mask, rng),
                g_hs=r32(rng.standard_normal((B, T, H))) if grads in ("both", "hs") else None,
                g_last=r32(rng.standard_normal((B, H))) if grads in ("both", "last") else None)


MAX_COND = 64.0


def conditioned_case(B, T, K, H, mode, **kw):
    """make_case with the first seed in 0 .. 99 whose sums over (b, t) (backward()'s cond: dW, dU, db) have a conditioning of at most
    MAX_COND: for the cases of a handful of steps, where a single draw decides how many digits a cancelling sum keeps.  The choice
    reads the fp64 reference only."""
    for seed in range(100):
        case = make_case(B, T, K, H, mode, seed, **kw)
        if max(backward(case)["cond"].values()) <= MAX_COND:
            case["seed"] = seed
            return case
    raise AssertionError("conditioned_case: no seed in 0 .. 99 gives conditioning <= %g for %s" % (MAX_COND, (B, T, K, H)))


def norm_rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def errors(got, hs_ref, bwd_ref):
    """got: dict(hs, GRADS...) -> the same keys (those present in got and not None): norm-relative error against the fp64 reference."""
    res = {}
    for k, v in got.items():
        if v is None:
            continue
        if k == "hs":
            res[k] = norm_rel(v, hs_ref)
        elif k in GRADS:
            res[k] = norm_rel(np.asarray(v).reshape(bwd_ref[k].shape), bwd_ref[k])
    return res


_REF_CACHE = {}


def reference(case):
    """(hs, backward dict, E32 dict) of a case, computed once per case object."""
    key = id(case)
    hit = _REF_CACHE.get(key)
    if hit is None or hit[0] is not case:
        hs, bwd = forward(case), backward(case)
        e32 = errors(torch_run(case, torch.float32), hs, bwd)
        hit = _REF_CACHE[key] = (case, hs, bwd, e32)
    return hit[1], hit[2], hit[3]


def bars(e32):
    """max(1e-5, 4 E32) per tensor: 1e-5 is the standing bar of the fp32 kernels against the fp64 oracle, E32 the error of the fp32
    torch restatement of the same graph on the same inputs; the factor 4 covers another summation order and the device's expf / tanhf."""
    return {k: max(1e-5, 4.0 * v) for k, v in e32.items()}
