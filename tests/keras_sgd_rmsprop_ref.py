"""The numpy fp32 restatement of Keras' SGD and RMSprop (TF 2.1: keras/optimizer_v2/gradient_descent.py, rmsprop.py, core/kernels/
training_ops.cc) that the tests of optim.SGD / optim.RMSprop compare against, bit for bit: every operation on float32 arrays and
float32 scalars, in the order written (numpy rounds each one to fp32; its division and square root are correctly rounded), and which
rows of an embedding table move.  TEST INFRASTRUCTURE: no GPU, no library.

    variant            slots             dense form                                              touched (IndexedSlices) form
    sgd                -                 p -= g lr                                               the same
    sgd_momentum       a                 a = a m - g lr;  p += a                                 the same
    sgd_nesterov       a                 a = a m - g lr;  p += a m - g lr                        the same
    rmsprop            rms               rms = rho rms + (1 - rho)(g g)                          rms = (rms rho) + (g g)(1 - rho)
                                         p = p - lr g / (sqrt(rms) + eps)                        the same
    rmsprop_momentum   rms, mom          rms = rms + (g g - rms)(1 - rho)                        rms = rms rho + (g g)(1 - rho)
                                         mom = mom m + (g lr) / sqrt(rms + eps);  p -= mom       mom = mom m + ((1 / sqrt(rms + eps)) lr) g
"""
import numpy as np

F = np.float32
VARIANTS = ("sgd", "sgd_momentum", "sgd_nesterov", "rmsprop", "rmsprop_momentum")
N_SLOTS = dict(sgd=0, sgd_momentum=1, sgd_nesterov=1, rmsprop=1, rmsprop_momentum=2)
SLOT_NAMES = dict(sgd=(), sgd_momentum=("momentum",), sgd_nesterov=("momentum",), rmsprop=("rms",), rmsprop_momentum=("rms", "momentum"))


def hyper(variant, lr, momentum=0.9, rho=0.9, epsilon=1e-7):
    """The variant's hyper-parameters as float32 (Keras keeps them in float32 variables); momentum is forced to 0 where the variant
    has none."""
    assert variant in VARIANTS
    if variant in ("sgd", "rmsprop"):
        momentum = 0.0
    assert momentum > 0 or variant in ("sgd", "rmsprop")
    rho = F(rho)
    return dict(variant=variant, lr=F(lr), momentum=F(momentum), rho=rho, omr=F(1) - rho, eps=F(epsilon))


def with_lr(h, lr):
    return dict(h, lr=F(lr))


def _f(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def elem(h, p, s, z, g, touched):
    """One step of the rule on float32 arrays p, g and the slots s, z (None where the variant has none) -> (p, s, z)."""
    v, lr, m, rho, omr, eps = h["variant"], h["lr"], h["momentum"], h["rho"], h["omr"], h["eps"]
    p, g = _f(p), _f(g)
    if v == "sgd":
        return p - g * lr, None, None
    s = _f(s)
    if v == "sgd_momentum":
        s = s * m - g * lr
        return p + s, s, None
    if v == "sgd_nesterov":
        s = s * m - g * lr
        return p + (s * m - g * lr), s, None
    if v == "rmsprop":
        s = (s * rho) + (g * g) * omr if touched else rho * s + omr * (g * g)
        return p - lr * g / (np.sqrt(s) + eps), s, None
    z = _f(z)
    if touched:
        s = s * rho + (g * g) * omr
        z = z * m + ((F(1) / np.sqrt(s + eps)) * lr) * g
    else:
        s = s + (g * g - s) * omr
        z = z * m + (g * lr) / np.sqrt(s + eps)
    return p - z, s, z


def dense_step(h, p, s, z, g, l2=0.0):
    """A dense variable: g (zeros for a variable without gradient) + 2 l2 p, the dense form."""
    p = _f(p)
    return elem(h, p, s, z, _f(g) + (F(2) * F(l2)) * p, touched=False)


def table_step(h, p, s, z, run_sums, touched, row_l2, frozen):
    """One step of an embedding table [V, K].  run_sums [V, K] float32: the summed gradient of every touched row (anything elsewhere);
    touched [V] bool; row_l2 [V] float32: the l2(emb_reg) of the row's field (0: none); frozen [V] bool.  Returns (p, s, z) and the
    boolean row masks (moved, decayed): rows that took the rule, and rows whose rms alone changed (rmsprop only)."""
    p = _f(p).copy()
    s = None if s is None else _f(s).copy()
    z = None if z is None else _f(z).copy()
    row_l2 = _f(row_l2)
    l2x2 = (F(2) * row_l2)[:, None]
    t = touched & ~frozen
    u = ~touched & ~frozen & (row_l2 > 0)
    sub = lambda a, r: None if a is None else a[r]
    for rows, is_touched in ((t, True), (u, False)):
        if not rows.any():
            continue
        acc = _f(run_sums)[rows] if is_touched else np.zeros_like(p[rows])
        g = acc + l2x2[rows] * p[rows]
        pp, ss, zz = elem(h, p[rows], sub(s, rows), sub(z, rows), g, touched=is_touched)
        p[rows] = pp
        if s is not None:
            s[rows] = ss
        if z is not None:
            z[rows] = zz
    d = np.zeros_like(t)
    if h["variant"] == "rmsprop":
        d = ~touched & ~frozen & ~(row_l2 > 0)
        s[d] = s[d] * h["rho"]
    return (p, s, z), (t | u), d


def elem64(h, p, s, z, g, touched):
    """The same rules in float64 from float32 hyper-parameters (for the tolerance comparisons)."""
    v = h["variant"]
    lr, m, rho, eps = (float(h[k]) for k in ("lr", "momentum", "rho", "eps"))
    omr = 1.0 - rho
    if v == "sgd":
        return p - g * lr, None, None
    if v == "sgd_momentum":
        s = s * m - g * lr
        return p + s, s, None
    if v == "sgd_nesterov":
        s = s * m - g * lr
        return p + (s * m - g * lr), s, None
    s = rho * s + omr * g * g
    if v == "rmsprop":
        return p - lr * g / (np.sqrt(s) + eps), s, None
    z = z * m + lr * g / np.sqrt(s + eps)
    return p - z, s, z
