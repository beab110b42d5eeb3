"""fp64 restatement of the Neural Turing Machine memory read / write over a sequence (include/fil.h N4 fil_ntm_*,
ml_function_amd.functional.ntm_memory): the forward and the hand-derived backward written out step by step, the torch graph of the
same math (fp64: the autograd check of the backward; fp32: the restatement whose own error E32 sets the tests' bars), the error
measures and make_case().  Plain seeds need no selection: backward()'s cond stays far below gru_ref.MAX_COND on every shape the tests
use (tests/test_ntm_host.py asserts it from this reference alone).

    h [B,T,H], mask [B,T] (non-zero = live; None = all live), Wp [H,4D+2] and bp [4D+2] (columns kr | kw | e | a | beta_r | beta_w),
    M0 [m,D].  The state is M (M0 before the first live step) and r (zeros).  One live step, M = the previous memory:
        p = h_t Wp + bp;  kr = tanh(p_kr);  kw = tanh(p_kw);  e = sigmoid(p_e);  a = tanh(p_a);  beta = softplus(p_beta) + 1;
        c_i(k) = (M_i . k) / sqrt((|M_i|^2 + eps)(|k|^2 + eps)), eps = 1e-6;
        wr = softmax_i(beta_r c_i(kr));  ww = softmax_i(beta_w c_i(kw));  r_t = sum_i wr_i M_i;  M_t[i] = M_i (1 - ww_i e) + ww_i a.
    A masked step carries M and r.  The upstream gradients are g_rs [B,T,D] or g_last [B,D] (of rs[:, T-1]) and / or g_M [B,m,D]."""
import numpy as np
import torch

from tests.gru_ref import make_mask, norm_rel

EPS = 1e-6
PARAMS = ("Wp", "bp", "M0")
GRADS = ("dh", "dWp", "dbp", "dM0")
OUTS = ("rs", "MT")


def _live(mask, B, T):
    return np.ones((B, T), bool) if mask is None else np.asarray(mask).astype(bool)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def _address(M, k, beta):
    """-> (w [B,m], c [B,m], nM2 [B,m], nk2 [B,1])."""
    nM2 = (M * M).sum(-1) + EPS
    nk2 = (k * k).sum(-1, keepdims=True) + EPS
    c = (M * k[:, None, :]).sum(-1) / np.sqrt(nM2 * nk2)
    s = beta * c
    w = np.exp(s - s.max(1, keepdims=True))
    return w / w.sum(1, keepdims=True), c, nM2, nk2


def _steps(case):
    """The forward, keeping what the backward needs of every step."""
    h, Wp, bp, M0 = (np.asarray(case[k], np.float64) for k in ("h", "Wp", "bp", "M0"))
    B, T, H = h.shape
    m, D = M0.shape
    live = _live(case.get("mask"), B, T)
    h = np.where(live[:, :, None], h, 0.0)                   # a masked step's h is never used
    M = np.broadcast_to(M0, (B, m, D)).copy()
    r = np.zeros((B, D))
    rs = np.zeros((B, T, D))
    keep = []
    for t in range(T):
        p = h[:, t] @ Wp + bp
        kr, kw, e, a = np.tanh(p[:, :D]), np.tanh(p[:, D:2 * D]), _sig(p[:, 2 * D:3 * D]), np.tanh(p[:, 3 * D:4 * D])
        pb = p[:, 4 * D:]
        beta = _softplus(pb) + 1.0
        wr, cr, nM2, nkr2 = _address(M, kr, beta[:, 0:1])
        ww, cw, _, nkw2 = _address(M, kw, beta[:, 1:2])
        rn = (wr[:, :, None] * M).sum(1)
        Mn = M * (1.0 - ww[:, :, None] * e[:, None, :]) + ww[:, :, None] * a[:, None, :]
        keep.append(dict(M=M, kr=kr, kw=kw, e=e, a=a, pb=pb, beta=beta, wr=wr, ww=ww, cr=cr, cw=cw, nM2=nM2, nkr2=nkr2, nkw2=nkw2))
        lv = live[:, t]
        r = np.where(lv[:, None], rn, r)
        M = np.where(lv[:, None, None], Mn, M)
        rs[:, t] = r
    return dict(h=h, Wp=Wp, live=live, rs=rs, MT=M, keep=keep, dims=(B, T, H, m, D))


def forward(case):
    """-> dict(rs [B,T,D], MT [B,m,D]) float64."""
    p = _steps(case)
    return dict(rs=p["rs"], MT=p["MT"])


def _head_backward(dw, w, c, beta, M, k, nM2, nk2):
    """One addressing head: the gradient of its weights -> (dM [B,m,D], dk [B,D], dbeta [B,1])."""
    ds = w * (dw - (w * dw).sum(1, keepdims=True))
    dbeta = (ds * c).sum(1, keepdims=True)
    dc = beta * ds
    inv = 1.0 / np.sqrt(nM2 * nk2)                          # 1 / (nM_i nk)
    dM = dc[:, :, None] * (k[:, None, :] * inv[:, :, None] - (c / nM2)[:, :, None] * M)
    dk = (dc[:, :, None] * (M * inv[:, :, None] - (c / nk2)[:, :, None] * k[:, None, :])).sum(1)
    return dM, dk, dbeta


def backward(case):
    """g_rs [B,T,D] or g_last [B,D] and / or g_M [B,m,D] -> dict of GRADS, float64, by the chain rule written out, and cond: the
    conditioning (sum of |terms| / |sum|, in norms) of the sums over (b, t) behind dWp and dbp and of the sum over b behind dM0."""
    p = _steps(case)
    h, Wp, live = p["h"], p["Wp"], p["live"]
    B, T, H, m, D = p["dims"]
    g = lambda k: None if case.get(k) is None else np.asarray(case[k], np.float64)
    g_rs, g_last, g_M = g("g_rs"), g("g_last"), g("g_M")
    dM = np.zeros((B, m, D)) if g_M is None else g_M.copy()
    dr = np.zeros((B, D)) if g_last is None else g_last.copy()
    dh = np.zeros((B, T, H))
    dWp, dbp = np.zeros_like(Wp), np.zeros(4 * D + 2)
    aW, ab = np.zeros_like(Wp), np.zeros(4 * D + 2)
    for t in range(T - 1, -1, -1):
        s = p["keep"][t]
        lv = live[:, t]
        if g_rs is not None:
            dr = dr + g_rs[:, t]
        M, e, a, ww, wr = s["M"], s["e"], s["a"], s["ww"], s["wr"]
        # write
        dMp = dM * (1.0 - ww[:, :, None] * e[:, None, :])
        dww = (dM * (a[:, None, :] - M * e[:, None, :])).sum(-1)
        de = -(dM * M * ww[:, :, None]).sum(1)
        da = (dM * ww[:, :, None]).sum(1)
        # read
        dMp = dMp + wr[:, :, None] * dr[:, None, :]
        dwr = (M * dr[:, None, :]).sum(-1)
        dMr, dkr, dbr = _head_backward(dwr, wr, s["cr"], s["beta"][:, 0:1], M, s["kr"], s["nM2"], s["nkr2"])
        dMw, dkw, dbw = _head_backward(dww, ww, s["cw"], s["beta"][:, 1:2], M, s["kw"], s["nM2"], s["nkw2"])
        dMp = dMp + dMr + dMw
        dp = np.concatenate([dkr * (1.0 - s["kr"] ** 2), dkw * (1.0 - s["kw"] ** 2), de * e * (1.0 - e), da * (1.0 - a ** 2),
                             np.concatenate([dbr, dbw], 1) * _sig(s["pb"])], 1)
        dp = np.where(lv[:, None], dp, 0.0)
        dh[:, t] = dp @ Wp.T
        dWp += h[:, t].T @ dp
        dbp += dp.sum(0)
        aW += np.abs(h[:, t]).T @ np.abs(dp)
        ab += np.abs(dp).sum(0)
        dM = np.where(lv[:, None, None], dMp, dM)
        dr = np.where(lv[:, None], 0.0, dr)                  # the read is replaced at a live step
    cond_of = lambda ab_, v: float(np.linalg.norm(ab_) / max(np.linalg.norm(v), 1e-300))
    return dict(dh=dh, dWp=dWp, dbp=dbp, dM0=dM.sum(0),
                cond=dict(dWp=cond_of(aW, dWp), dbp=cond_of(ab, dbp), dM0=cond_of(np.abs(dM).sum(0), dM.sum(0))))


def torch_graph(h, mask, Wp, bp, M0):
    """The same math as torch ops on the tensors given (their dtype; autograd for the backward) -> (rs [B,T,D], M_T [B,m,D])."""
    B, T, H = h.shape
    m, D = M0.shape

    def address(M, k, pb):
        beta = torch.clamp_min(pb, 0) + torch.log1p(torch.exp(-torch.abs(pb))) + 1
        c = (M * k.unsqueeze(1)).sum(-1) / torch.sqrt(((M * M).sum(-1) + EPS) * ((k * k).sum(-1, keepdim=True) + EPS))
        s = beta * c
        w = torch.exp(s - s.max(dim=1, keepdim=True).values)
        return w / w.sum(dim=1, keepdim=True)

    if mask is not None:
        h = torch.where(mask.unsqueeze(-1), h, torch.zeros((), dtype=h.dtype))
    M = M0.unsqueeze(0).expand(B, m, D)
    r = torch.zeros((B, D), dtype=h.dtype)
    out = []
    for t in range(T):
        p = torch.matmul(h[:, t], Wp) + bp
        kr, kw = torch.tanh(p[:, :D]), torch.tanh(p[:, D:2 * D])
        e, a = torch.sigmoid(p[:, 2 * D:3 * D]), torch.tanh(p[:, 3 * D:4 * D])
        wr = address(M, kr, p[:, 4 * D:4 * D + 1])
        ww = address(M, kw, p[:, 4 * D + 1:4 * D + 2]).unsqueeze(-1)
        rn = (wr.unsqueeze(-1) * M).sum(1)
        Mn = M * (1 - ww * e.unsqueeze(1)) + ww * a.unsqueeze(1)
        if mask is not None:
            lt = mask[:, t:t + 1]
            rn, Mn = torch.where(lt, rn, r), torch.where(lt.unsqueeze(-1), Mn, M)
        r, M = rn, Mn
        out.append(r)
    return torch.stack(out, 1), M


def torch_run(case, dtype):
    """rs, MT and the gradients of torch_graph on the CPU in `dtype`, as float64 numpy arrays (the keys of forward() and backward())."""
    names = ("h",) + PARAMS
    t = {k: torch.tensor(np.asarray(case[k]), dtype=dtype, requires_grad=True) for k in names}
    mask = None if case.get("mask") is None else torch.tensor(np.asarray(case["mask"]).astype(bool))
    rs, MT = torch_graph(t["h"], mask, t["Wp"], t["bp"], t["M0"])
    loss = torch.zeros((), dtype=dtype)
    G = lambda k: torch.tensor(np.asarray(case[k]), dtype=dtype)
    if case.get("g_rs") is not None:
        loss = loss + (rs * G("g_rs")).sum()
    if case.get("g_last") is not None:
        loss = loss + (rs[:, -1] * G("g_last")).sum()
    if case.get("g_M") is not None:
        loss = loss + (MT * G("g_M")).sum()
    loss.backward()
    D = lambda v: v.detach().double().numpy()
    res = dict(rs=D(rs), MT=D(MT))
    for k in names:
        res["d" + k] = D(t[k].grad) if t[k].grad is not None else np.zeros(t[k].shape)
    return res


def make_case(B, T, H, m, D, seed, mask="ragged", grads="both", scale=1.0, zero_row=False):
    """h ~ 0.5 N(0,1), Wp glorot-scaled normal, bp ~ 0.1 N(0,1), M0 ~ 0.1 N(0,1), g ~ N(0,1), ragged lengths 0 .. T; all
    fp32-representable (returned as float64 arrays).  grads: "both" (g_rs and g_M), "rs", "last" (g_last alone), "last+M" or "M".
    scale multiplies h and Wp (a saturated case); zero_row zeroes the first row of M0."""
    rng = np.random.default_rng(seed)
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    M0 = rng.standard_normal((m, D)) * 0.1
    if zero_row:
        M0[0] = 0.0
    return dict(shape=(B, T, H, m, D),
                Wp=r32(rng.standard_normal((H, 4 * D + 2)) * np.sqrt(2.0 / (H + 4 * D + 2)) * scale),
                bp=r32(rng.standard_normal(4 * D + 2) * 0.1),
                M0=r32(M0),
                h=r32(rng.standard_normal((B, T, H)) * 0.5 * scale),
                mask=make_mask(B, T, mask, rng),
                g_rs=r32(rng.standard_normal((B, T, D))) if grads in ("both", "rs") else None,
                g_last=r32(rng.standard_normal((B, D))) if grads in ("last", "last+M") else None,
                g_M=r32(rng.standard_normal((B, m, D))) if grads in ("both", "M", "last+M") else None)


def errors(got, fwd_ref, bwd_ref):
    """got: dict(rs, MT, GRADS...) -> the same keys (those present in got and not None): norm-relative error against the fp64 reference."""
    res = {}
    for k, v in got.items():
        if v is None:
            continue
        if k in OUTS:
            res[k] = norm_rel(v, fwd_ref[k])
        elif k in GRADS:
            res[k] = norm_rel(np.asarray(v).reshape(bwd_ref[k].shape), bwd_ref[k])
    return res


_REF_CACHE = {}


def reference(case):
    """(forward dict, backward dict, E32 dict) of a case, computed once per case object."""
    key = id(case)
    hit = _REF_CACHE.get(key)
    if hit is None or hit[0] is not case:
        fwd, bwd = forward(case), backward(case)
        e32 = errors(torch_run(case, torch.float32), fwd, bwd)
        hit = _REF_CACHE[key] = (case, fwd, bwd, e32)
    return hit[1], hit[2], hit[3]


def bars(e32):
    """max(1e-5, 4 E32) per tensor: 1e-5 is the standing bar of the fp32 kernels against the fp64 oracle, E32 the error of the fp32
    torch restatement of the same graph on the same inputs; the factor 4 covers another summation order and the device's expf / tanhf."""
    return {k: max(1e-5, 4.0 * v) for k, v in e32.items()}
