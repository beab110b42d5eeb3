"""The numpy fp32 restatement of Keras' Adadelta and Adamax (TF 2.1: keras/optimizer_v2/adadelta.py, adamax.py, core/kernels/
training_ops.cc; restated from memory -- TF is not installed where these tests run, so parity with TF itself is unpinned, as for
oracle/) that the tests of optim.Adadelta / optim.Adamax compare against: every operation on float32 arrays and float32 scalars, in the
order written (numpy rounds each one to fp32; its division and square root are correctly rounded), and which rows of an embedding
table move.  TEST INFRASTRUCTURE: no GPU, no library.

    variant    slots                   dense form                                          touched (IndexedSlices) form
    adadelta   accum_grad, accum_var   ag  = (ag rho) + ((g g) (1 - rho))                  the same (ApplyAdadelta and SparseApplyAdadelta
                                       upd = (sqrt(av + eps) (1 / sqrt(ag + eps))) g       are one rule)
                                       p   = p - (upd lr)
                                       av  = (av rho) + ((upd upd) (1 - rho))
    adamax     m, v                    m = m + ((g - m) (1 - b1))                          m = (m b1) + (g (1 - b1))
                                       v = max(b2 v, |g|)                                  v = max(v b2, |g|)
                                       p = p - (c (m / (v + eps)))                         p = p + ((-c) (m / (v + eps)))
               c = lr / (1 - b1^t), t = iterations + 1 as float32.  1 - rho and 1 - b1 are formed once in fp32.  b1^t here is numpy's
               float32 power; the library takes the device's powf, which may differ in the last bits: Adamax is therefore compared
               against the float64 twin (elem64) within bars, and bit for bit only in WHICH rows move; `coef` exposes c so that a test
               can check its tail (at large t, 1 - b1^t rounds to 1 and c == lr exactly).
"""
import numpy as np

F = np.float32
VARIANTS = ("adadelta", "adamax")
N_SLOTS = dict(adadelta=2, adamax=2)
SLOT_NAMES = dict(adadelta=("accum_grad", "accum_var"), adamax=("m", "v"))


def hyper(variant, lr, rho=0.95, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """The variant's hyper-parameters as float32 (Keras keeps them in float32 variables)."""
    assert variant in VARIANTS
    rho, b1 = F(rho), F(beta_1)
    return dict(variant=variant, lr=F(lr), rho=rho, omr=F(1) - rho, b1=b1, omb1=F(1) - b1, b2=F(beta_2), eps=F(epsilon))


def with_lr(h, lr):
    return dict(h, lr=F(lr))


def _f(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def coef(h, t):
    """Adamax' step size of step t (= iterations + 1) in float32: lr / (1 - b1^t)."""
    return F(h["lr"] / (F(1) - np.power(h["b1"], F(t), dtype=F)))


def coef64(h, t):
    return float(h["lr"]) / (1.0 - float(h["b1"]) ** float(t))


def elem(h, p, s, z, g, touched, t=None):
    """One step of the rule on float32 arrays p, g and the slots s, z -> (p, s, z).  t (Adamax): the step, iterations + 1."""
    p, s, z, g = _f(p), _f(s), _f(z), _f(g)
    eps = h["eps"]
    if h["variant"] == "adadelta":
        rho, omr = h["rho"], h["omr"]
        s = s * rho + (g * g) * omr
        upd = (np.sqrt(z + eps) * (F(1) / np.sqrt(s + eps))) * g
        p = p - upd * h["lr"]
        z = z * rho + (upd * upd) * omr
        return p, s, z
    c = coef(h, t)
    if touched:
        s = s * h["b1"] + g * h["omb1"]
        z = np.maximum(z * h["b2"], np.abs(g))
        return p + (-c) * (s / (z + eps)), s, z
    s = s + (g - s) * h["omb1"]
    z = np.maximum(h["b2"] * z, np.abs(g))
    return p - c * (s / (z + eps)), s, z


def dense_step(h, p, s, z, g, l2=0.0, t=None):
    """A dense variable: g (zeros for a variable without gradient) + 2 l2 p, the dense form."""
    p = _f(p)
    return elem(h, p, s, z, _f(g) + (F(2) * F(l2)) * p, touched=False, t=t)


def table_step(h, p, s, z, run_sums, touched, row_l2, frozen, t=None):
    """One step of an embedding table [V, K].  run_sums [V, K] float32: the summed gradient of every touched row (anything elsewhere);
    touched [V] bool; row_l2 [V] float32: the l2(emb_reg) of the row's field (0: none); frozen [V] bool.  Returns (p, s, z) and the
    boolean row mask `moved`: the rows that took the rule -- the touched rows (touched form, g = run sum + 2 l2 p) and the untouched
    rows of the regularised fields (dense form, g = 2 l2 p); every other row keeps p and both slots."""
    p, s, z = _f(p).copy(), _f(s).copy(), _f(z).copy()
    row_l2 = _f(row_l2)
    l2x2 = (F(2) * row_l2)[:, None]
    tr = touched & ~frozen
    u = ~touched & ~frozen & (row_l2 > 0)
    for rows, is_touched in ((tr, True), (u, False)):
        if not rows.any():
            continue
        acc = _f(run_sums)[rows] if is_touched else np.zeros_like(p[rows])
        g = acc + l2x2[rows] * p[rows]
        p[rows], s[rows], z[rows] = elem(h, p[rows], s[rows], z[rows], g, touched=is_touched, t=t)
    return (p, s, z), (tr | u)


def elem64(h, p, s, z, g, touched, t=None):
    """The same rules in float64 from the float32 hyper-parameters (the twin the tolerance comparisons use; the two Adamax forms are
    one in exact arithmetic)."""
    eps = float(h["eps"])
    if h["variant"] == "adadelta":
        rho = float(h["rho"])
        s = s * rho + g * g * (1.0 - rho)
        upd = np.sqrt(z + eps) / np.sqrt(s + eps) * g
        return p - upd * float(h["lr"]), s, z * rho + upd * upd * (1.0 - rho)
    b1, b2 = float(h["b1"]), float(h["b2"])
    s = s * b1 + g * (1.0 - b1)
    z = np.maximum(z * b2, np.abs(g))
    return p - coef64(h, t) * (s / (z + eps)), s, z
