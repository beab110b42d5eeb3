"""The numpy fp32 restatement of Keras' Nadam (TF 2.1: keras/optimizer_v2/nadam.py; restated from memory -- TF is not installed where
these tests run, so parity with TF itself is unpinned, as for oracle/) that the tests of optim.Nadam compare against: every operation
on float32 arrays and float32 scalars, in the order written (numpy rounds each one to fp32; its division and square root are
correctly rounded), and which rows of an embedding table move.  TEST INFRASTRUCTURE: no GPU, no library.

Per step, with it = iterations (completed steps), t = float32(it + 1), n = float32(it + 2), sd = schedule_decay and cache = the
momentum cache (1.0 before the first step):

    mt   = b1 (1 - 0.5 0.96^(sd t))         mt1 = b1 (1 - 0.5 0.96^(sd n))         msn = cache mt        msx = msn mt1
    omm  = 1 - mt    omsn = 1 - msn    omsx = 1 - msx    vden = 1 - b2^t    omb1 = 1 - b1    omb2 = 1 - b2
    after the step: cache = msn, iterations = it + 1

Per element, with gradient g (Keras' dense and IndexedSlices forms round to the same bits: one form):

    gp = g / omsn;  m = b1 m + omb1 g;  mp = m / omsx;  v = b2 v + omb2 (g g);  vp = v / vden
    mbar = omm gp + mt1 mp;  p = p - (lr mbar) / (sqrt(vp) + eps)

The powers here are numpy's float32 power; the library takes the device's powf, which may differ in the last bits, so p is compared
against the float64 twin (coefs64 / elem64, which carries its own float64 cache) within bars; m and v involve no power and are
compared bit for bit; at large `it` with cache 0 the powers leave the coefficients and everything is bit for bit.
"""
import numpy as np

F = np.float32
SLOT_NAMES = ("m", "v")
COEFS = ("mt", "mt1", "msn", "msx", "omm", "omsn", "omsx", "vden", "omb1", "omb2")


def hyper(lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004):
    """The hyper-parameters as float32 (Keras keeps them in float32 variables)."""
    return dict(lr=F(lr), b1=F(beta_1), b2=F(beta_2), eps=F(epsilon), sd=F(schedule_decay))


def _f(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def powf(a, b):
    return np.power(F(a), F(b), dtype=F)


def coefs(h, it, cache, pow_=powf):
    """The step's coefficients in float32 from the completed steps `it` and the float32 cache; c["msn"] is the cache after the step.
    pow_: the float32 power (a test may perturb it)."""
    b1, b2, sd, one, half = h["b1"], h["b2"], h["sd"], F(1), F(0.5)
    t, n = F(it + 1), F(it + 2)
    c = {}
    c["mt"] = F(b1 * F(one - F(half * pow_(F(0.96), F(sd * t)))))
    c["mt1"] = F(b1 * F(one - F(half * pow_(F(0.96), F(sd * n)))))
    c["msn"] = F(F(cache) * c["mt"])
    c["msx"] = F(c["msn"] * c["mt1"])
    c["omm"], c["omsn"], c["omsx"] = F(one - c["mt"]), F(one - c["msn"]), F(one - c["msx"])
    c["vden"] = F(one - pow_(b2, t))
    c["omb1"], c["omb2"] = F(one - b1), F(one - b2)
    assert all(isinstance(c[k], np.float32) for k in COEFS)
    return c


def coefs64(h, it, cache):
    """The same in float64 from the float32 hyper-parameters and a float64 cache."""
    b1, b2, sd = float(h["b1"]), float(h["b2"]), float(h["sd"])
    t, n = float(it + 1), float(it + 2)
    c = {}
    c["mt"] = b1 * (1.0 - 0.5 * 0.96 ** (sd * t))
    c["mt1"] = b1 * (1.0 - 0.5 * 0.96 ** (sd * n))
    c["msn"] = float(cache) * c["mt"]
    c["msx"] = c["msn"] * c["mt1"]
    c["omm"], c["omsn"], c["omsx"] = 1.0 - c["mt"], 1.0 - c["msn"], 1.0 - c["msx"]
    c["vden"] = 1.0 - b2 ** t
    c["omb1"], c["omb2"] = 1.0 - b1, 1.0 - b2
    return c


def elem(h, c, p, m, v, g):
    """One step of the rule on float32 arrays with the coefficients c -> (p, m, v)."""
    p, m, v, g = _f(p), _f(m), _f(v), _f(g)
    gp = g / c["omsn"]
    m = h["b1"] * m + c["omb1"] * g
    mp = m / c["omsx"]
    v = h["b2"] * v + c["omb2"] * (g * g)
    vp = v / c["vden"]
    mbar = c["omm"] * gp + c["mt1"] * mp
    p = p - (h["lr"] * mbar) / (np.sqrt(vp) + h["eps"])
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def elem64(h, c, p, m, v, g):
    """The same in float64 (c from coefs64)."""
    b1, b2 = float(h["b1"]), float(h["b2"])
    gp = g / c["omsn"]
    m = b1 * m + (1.0 - b1) * g
    mp = m / c["omsx"]
    v = b2 * v + (1.0 - b2) * (g * g)
    vp = v / c["vden"]
    mbar = c["omm"] * gp + c["mt1"] * mp
    return p - (float(h["lr"]) * mbar) / (np.sqrt(vp) + float(h["eps"])), m, v


def dense_step(h, c, p, m, v, g, l2=0.0):
    """A dense variable: g + 2 l2 p."""
    p = _f(p)
    return elem(h, c, p, m, v, _f(g) + (F(2) * F(l2)) * p)


def table_step(h, c, p, m, v, run_sums, touched, row_l2, frozen):
    """One step of an embedding table [V, K].  run_sums [V, K] float32: the summed gradient of every touched row (anything elsewhere);
    touched [V] bool; row_l2 [V] float32: the l2(emb_reg) of the row's field (0: none); frozen [V] bool.  Returns (p, m, v) and two
    boolean row masks: `moved`, the rows that took the rule -- the touched rows (g = run sum + 2 l2 p) and the untouched rows of the
    regularised fields (g = 2 l2 p) -- and `decayed`, the untouched rows of the unregularised, non-frozen fields: m = m b1, v = v b2, p
    kept.  A frozen row keeps everything."""
    p, m, v = _f(p).copy(), _f(m).copy(), _f(v).copy()
    row_l2 = _f(row_l2)
    l2x2 = (F(2) * row_l2)[:, None]
    tr = touched & ~frozen
    u = ~touched & ~frozen & (row_l2 > 0)
    d = ~touched & ~frozen & ~(row_l2 > 0)
    for rows, is_touched in ((tr, True), (u, False)):
        if not rows.any():
            continue
        acc = _f(run_sums)[rows] if is_touched else np.zeros_like(p[rows])
        g = acc + l2x2[rows] * p[rows]
        p[rows], m[rows], v[rows] = elem(h, c, p[rows], m[rows], v[rows], g)
    m[d] = m[d] * h["b1"]
    v[d] = v[d] * h["b2"]
    return (p, m, v), (tr | u), d


# ---- what the host tests and the GPU tests share: the dense inputs and the bars
BARS = dict(update=1e-4, p=1e-6, m=1e-5, v=1e-5)     # optim.Adam's, as check_step applies them to Adamax: norm-relative, one step
DENSE_SIZES = (1, 4095, 4097)
DENSE_LR = 1e-2


def dense_inputs(seed, sizes=DENSE_SIZES):
    """Per tensor: the initial p (|p| in [1, 1.95], random sign) and the persistent sign of its gradient.  With |p| >= 1 and an update of
    at most a few lr = 1e-2, the update's own relative error (the coefficients', of the order of 1e-6 with a 1-ulp powf) reaches p
    scaled by |update| / |p| <= a few 1e-2; p's final rounding (half an ulp, 6e-8 relative) is 1e-5 of an update of lr / 3 or more."""
    rng = np.random.default_rng(seed)
    ps = [(np.sign(rng.standard_normal(n)) * rng.uniform(1.0, 1.95, n)).astype(F) for n in sizes]
    signs = [np.sign(rng.standard_normal(n)) for n in sizes]
    return rng, ps, signs


def dense_grads(rng, signs):
    """One step's gradients: the persistent sign, |g| in [0.5, 1.5]."""
    return [(sg * rng.uniform(0.5, 1.5, sg.shape)).astype(F) for sg in signs]


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def step_errors(h, c64, got, old, g):
    """One step from the fp32 state `old` = (p, m, v) with the fp32 gradient g: the norm-relative errors of `got` = (p, m, v) against
    the float64 twin with coefficients c64 -> dict(update, p, m, v)."""
    o64 = tuple(np.asarray(x, np.float64) for x in old)
    w64 = elem64(h, c64, *o64, np.asarray(g, np.float64))
    return dict(update=nrel(np.asarray(got[0], np.float64) - o64[0], w64[0] - o64[0]), p=nrel(got[0], w64[0]), m=nrel(got[1], w64[1]),
                v=nrel(got[2], w64[2]))


def within_bars(e):
    return all(e[k] < BARS[k] for k in BARS)
