"""fp64 restatement of the LSTM over a sequence, one direction or both (include/fil.h N3 fil_lstm_*, ml_function_amd.functional.lstm):
the forward and the hand-derived backward written out step by step, the torch graph of the same math (fp64: the autograd check of the
backward; fp32: the restatement whose own error E32 sets the tests' bars), the error measures and make_case().

    x [B,T,K], mask [B,T] (non-zero = live; None = all live), per direction W [K,4H], U [H,4H] (columns i | f | c | o), b [4H].
    One live step, h and c = the previous states, h_0 = c_0 = 0:
        z = x_t W + h U + b;  i = sigmoid(z_i);  f = sigmoid(z_f);  g = tanh(z_c);  o = sigmoid(z_o);  c_new = f c + i g;
        h_new = o tanh(c_new).
    A masked step carries both states.  "forward" walks t = 0 .. T-1, "reverse" t = T-1 .. 0 and leaves the state reached after step
    t at position t; "bidirectional" has W [2,K,4H], U [2,H,4H], b [2,4H] (forward, reverse) and hs [B,T,2H], the forward direction in
    the first H columns.  The upstream gradients are g_hs [B,T,nH] and / or g_last [B,nH] (of the directions' last states: the
    forward hs[:,T-1,:H], the reverse hs[:,0,H:])."""
import numpy as np
import torch

DIRECTIONS = ("forward", "reverse", "bidirectional")
PARAMS = ("W", "U", "b")
GRADS = ("dx", "dW", "dU", "db")


def ndir(direction):
    return 2 if direction == "bidirectional" else 1


def _live(mask, B, T):
    return np.ones((B, T), bool) if mask is None else np.asarray(mask).astype(bool)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _order(T, rev):
    return range(T - 1, -1, -1) if rev else range(T)


def _steps(x, live, W, U, b, rev):
    """One direction's forward, keeping what the backward needs of every step (keep[t] belongs to time position t)."""
    B, T, K = x.shape
    H = U.shape[0]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    hs = np.zeros((B, T, H))
    keep = [None] * T
    for t in _order(T, rev):
        z = x[:, t] @ W + h @ U + b
        i, f, g, o = _sig(z[:, :H]), _sig(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sig(z[:, 3 * H:])
        cn = f * c + i * g
        hn = o * np.tanh(cn)
        keep[t] = dict(h=h, c=c, i=i, f=f, g=g, o=o, cn=cn)
        lv = live[:, t:t + 1]
        h, c = np.where(lv, hn, h), np.where(lv, cn, c)
        hs[:, t] = h
    return hs, keep


def _inputs(case):
    f = lambda k: np.asarray(case[k], np.float64)
    x, W, U, b = (f(k) for k in ("x", "W", "U", "b"))
    B, T, K = x.shape
    live = _live(case.get("mask"), B, T)
    x = np.where(live[:, :, None], x, 0.0)                    # a masked step's x is never used
    n = ndir(case["direction"])
    if n == 1:
        W, U, b = W[None], U[None], b[None]
    revs = (False, True) if n == 2 else (case["direction"] == "reverse",)
    return x, live, W, U, b, revs


def forward(case):
    """-> hs [B,T,nH] float64."""
    x, live, W, U, b, revs = _inputs(case)
    return np.concatenate([_steps(x, live, W[d], U[d], b[d], rev)[0] for d, rev in enumerate(revs)], axis=-1)


def last_of(hs, direction):
    """The directions' last states [B,nH] of hs [B,T,nH]."""
    if direction == "forward":
        return hs[:, -1]
    if direction == "reverse":
        return hs[:, 0]
    H = hs.shape[-1] // 2
    return np.concatenate([hs[:, -1, :H], hs[:, 0, H:]], axis=-1)


def backward(case):
    """g_hs [B,T,nH] and / or g_last [B,nH] -> dict of GRADS (in the shapes of x, W, U, b), float64, by the chain rule written out,
    and cond: the conditioning (sum of |terms| / |sum|, in norms) of the sums over (b, t) behind dW, dU and db."""
    x, live, W, U, b, revs = _inputs(case)
    B, T, K = x.shape
    H = U.shape[1]
    g_hs = None if case.get("g_hs") is None else np.asarray(case["g_hs"], np.float64)
    g_last = None if case.get("g_last") is None else np.asarray(case["g_last"], np.float64)
    dx = np.zeros((B, T, K))
    dW, dU, db = np.zeros_like(W), np.zeros_like(U), np.zeros_like(b)
    aW, aU, ab = np.zeros_like(W), np.zeros_like(U), np.zeros_like(b)
    for d, rev in enumerate(revs):
        _, keep = _steps(x, live, W[d], U[d], b[d], rev)
        cols = slice(d * H, (d + 1) * H)
        dh = np.zeros((B, H)) if g_last is None else g_last[:, cols].copy()
        dc = np.zeros((B, H))
        for t in reversed(list(_order(T, rev))):
            s = keep[t]
            lv = live[:, t:t + 1]
            if g_hs is not None:
                dh = dh + g_hs[:, t, cols]
            tc = np.tanh(s["cn"])
            do = dh * tc
            dcn = dc + dh * s["o"] * (1.0 - tc ** 2)
            dz = np.concatenate([dcn * s["g"] * s["i"] * (1.0 - s["i"]), dcn * s["c"] * s["f"] * (1.0 - s["f"]),
                                 dcn * s["i"] * (1.0 - s["g"] ** 2), do * s["o"] * (1.0 - s["o"])], 1)
            dz = np.where(lv, dz, 0.0)
            dx[:, t] += dz @ W[d].T
            dW[d] += x[:, t].T @ dz
            dU[d] += s["h"].T @ dz
            db[d] += dz.sum(0)
            aW[d] += np.abs(x[:, t]).T @ np.abs(dz)
            aU[d] += np.abs(s["h"]).T @ np.abs(dz)
            ab[d] += np.abs(dz).sum(0)
            dh = np.where(lv, dz @ U[d].T, dh)
            dc = np.where(lv, dcn * s["f"], dc)
    cond_of = lambda ab_, v: float(np.linalg.norm(ab_) / max(np.linalg.norm(v), 1e-300))
    cond = dict(dW=cond_of(aW, dW), dU=cond_of(aU, dU), db=cond_of(ab, db))
    if len(revs) == 1:
        dW, dU, db = dW[0], dU[0], db[0]
    return dict(dx=dx, dW=dW, dU=dU, db=db, cond=cond)


def _torch_direction(x, mask, W, U, b, rev):
    B, T, K = x.shape
    H = U.shape[0]
    h = torch.zeros((B, H), dtype=x.dtype)
    c = torch.zeros((B, H), dtype=x.dtype)
    out = [None] * T
    for t in _order(T, rev):
        z = torch.matmul(x[:, t], W) + torch.matmul(h, U) + b
        i, f, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 3 * H:])
        cn = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
        hn = o * torch.tanh(cn)
        if mask is not None:
            cn, hn = torch.where(mask[:, t:t + 1], cn, c), torch.where(mask[:, t:t + 1], hn, h)
        h, c = hn, cn
        out[t] = h
    return torch.stack(out, 1)


def torch_graph(x, mask, W, U, b, direction="forward"):
    """The same math as torch ops on the tensors given (their dtype; autograd for the backward) -> hs [B,T,nH]."""
    if mask is not None:
        x = torch.where(mask.unsqueeze(-1), x, torch.zeros((), dtype=x.dtype))
    if direction == "bidirectional":
        return torch.cat([_torch_direction(x, mask, W[d], U[d], b[d], d == 1) for d in range(2)], dim=-1)
    return _torch_direction(x, mask, W, U, b, direction == "reverse")


def torch_last(hs, direction):
    if direction == "forward":
        return hs[:, -1]
    if direction == "reverse":
        return hs[:, 0]
    H = hs.shape[-1] // 2
    return torch.cat([hs[:, -1, :H], hs[:, 0, H:]], dim=-1)


def torch_run(case, dtype):
    """hs and the gradients of torch_graph on the CPU in `dtype`, as float64 numpy arrays (the keys of backward())."""
    names = ("x",) + PARAMS
    t = {k: torch.tensor(np.asarray(case[k]), dtype=dtype, requires_grad=True) for k in names}
    mask = None if case.get("mask") is None else torch.tensor(np.asarray(case["mask"]).astype(bool))
    hs = torch_graph(t["x"], mask, t["W"], t["U"], t["b"], direction=case["direction"])
    loss = torch.zeros((), dtype=dtype)
    if case.get("g_hs") is not None:
        loss = loss + (hs * torch.tensor(np.asarray(case["g_hs"]), dtype=dtype)).sum()
    if case.get("g_last") is not None:
        loss = loss + (torch_last(hs, case["direction"]) * torch.tensor(np.asarray(case["g_last"]), dtype=dtype)).sum()
    loss.backward()
    D = lambda v: v.detach().double().numpy()
    res = dict(hs=D(hs))
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


def make_case(B, T, K, H, direction, seed, mask="ragged", grads="both", u_scale=1.5):
    """x ~ 0.5 N(0,1), W glorot-scaled normal, U u_scale x glorot, b ~ 0.1 N(0,1), g ~ N(0,1), ragged lengths 0 .. T; all
    fp32-representable (returned as float64 arrays).  grads: "both" (g_hs and g_last), "hs" or "last"."""
    rng = np.random.default_rng(seed)
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    n = ndir(direction)
    lead = (2,) if n == 2 else ()
    return dict(direction=direction, shape=(B, T, K, H),
                W=r32(rng.standard_normal(lead + (K, 4 * H)) * np.sqrt(2.0 / (K + 4 * H))),
                U=r32(rng.standard_normal(lead + (H, 4 * H)) * np.sqrt(2.0 / (5 * H)) * u_scale),
                b=r32(rng.standard_normal(lead + (4 * H,)) * 0.1),
                x=r32(rng.standard_normal((B, T, K)) * 0.5),
                mask=make_mask(B, T, mask, rng),
                g_hs=r32(rng.standard_normal((B, T, n * H))) if grads in ("both", "hs") else None,
                g_last=r32(rng.standard_normal((B, n * H))) if grads in ("both", "last") else None)


MAX_COND = 64.0


def conditioned_case(B, T, K, H, direction, **kw):
    """make_case with the first seed in 0 .. 99 whose sums over (b, t) (backward()'s cond: dW, dU, db) have a conditioning of at most
    MAX_COND: for the cases of a handful of steps, where a single draw decides how many digits a cancelling sum keeps.  The choice
    reads the fp64 reference only."""
    for seed in range(100):
        case = make_case(B, T, K, H, direction, seed, **kw)
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
