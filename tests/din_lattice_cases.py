"""DIN attention inputs on an integer lattice, the conditions they guarantee and the table of cases (TEST INFRASTRUCTURE: numpy only,
no GPU, no library).  tests/test_din_lattice_host.py checks every condition stated here for every case of the table;
tests/test_din_lattice_gpu.py relies on them to hold every dispatch path of csrc/din.hip to the fp64 reference (tests/din_attn_ref.py)
bit for bit, element for element, PReLU ties included.

The construction (lattice_case).  q and keys are in {-1, 0, 1}, g in {-2 .. 2}, every column of W1 and W2 has min(4, rows) entries of
+-1 and zeros elsewhere, b1 and b2 are in {-1, 0, 1}, the slopes in {0, 1/4, 1/2}, w3 is +-1 and b3 = 1.  Then in raw mode with PReLU
  * every input x_t = [q, k, q - k, q k] and every layer-1 pre-activation is an integer, h1 a multiple of 1/4, u2, h2, the score and
    out multiples of 1/16; backwards ds is an integer, du2 and dh1 multiples of 1/4, du1, dx, dq, dkeys, dW1, db1 and dW2 of 1/16 and
    none of the ten gradients is finer than 1/64 = QUANTUM;
  * an fp32 sum of multiples of QUANTUM whose terms' absolute values add up to less than 2^24 QUANTUM = EXACT_BELOW is exact in ANY
    order: abs_bound() forms every sum of the reference with the absolute value of every term in place of the term, which bounds
    every partial sum of every order of that sum, and the proof goes from sum to sum in evaluation order;
  * integer pre-activations are exactly zero often (a fifth of layer 1), so the kernel's convention at u = 0 (slope alpha) decides bits.
Every output and every gradient of a correct fp32 evaluation is then the fp64 reference's value in every element.

Where the rows outnumber a matrix's entries (W2 of a wide first layer and a narrow second one) the columns' entries are first spread
over distinct rows and every row still empty then gets one entry more: a unit whose row of W2 is zero has no gradient at all, and its
columns of dW1, db1 and dalpha1 could not show a dropped term.  The rows of W1 are covered by moving entries only (4 H1 >= 4 K).
"""
import collections
import functools

import numpy as np

from tests import din_attn_ref as ref

QUANTUM = 2.0 ** -6
EXACT_BELOW = 2.0 ** 24 * QUANTUM      # 2^18
INPUT_QUANTA = dict(q=1.0, keys=1.0, g=1.0, W1=1.0, b1=1.0, alpha1=0.25, W2=1.0, b2=1.0, alpha2=0.25, w3=1.0, b3=1.0)
TENSORS = ("out",) + ref.GRADS

# ---------------------------------------------------------------------------------------------------- the launchers' arithmetic
LDS_LIMIT, GRID_CAP, MAX_SAMPLES, BWD_THREADS, MAX_PARAMS = 163328, 512, 4, 256, 16384
_up = lambda v, m: -(-v // m) * m


def layout(T, K, H1, H2):
    """din_layout / din_pick / din_launch_bwd of csrc/din.hip restated: dict(H2T, NT, NS, tiles, lds_fwd, lds_bwd); NS = 0 where not
    even one sample fits."""
    H1C, H2T, KQ = _up(H1, 8), _up(H2, 16), K // 4
    KP = K + 4 if KQ % 2 == 0 else K
    shared = 4 * K * H1C + 2 * H1C + H1C * H2T + 3 * H2T + 4 + MAX_SAMPLES * (3 * 64 + 4)
    samp_fwd = 64 * KP + K + _up(T, 4) + (64 // KQ) * K
    samp_bwd = 64 * KP + 3 * K + 64 + H1C + 64 * (_up(H1, 16) + 4) + 64 * (H2T + 4)
    tiles = K * -(-H1 // 16) + -(-H1 // 4) * -(-H2 // 16)
    res = dict(H2T=H2T, NT=1 if tiles <= BWD_THREADS else 2, tiles=tiles, NS=0, lds_fwd=0, lds_bwd=0)
    for ns in range(MAX_SAMPLES, 0, -1):
        fwd, bwd = 4 * (shared + ns * samp_fwd), 4 * (shared + ns * samp_bwd)
        if fwd <= LDS_LIMIT and bwd <= LDS_LIMIT:
            res.update(NS=ns, lds_fwd=fwd, lds_bwd=bwd)
            break
    return res


def on_the_menu(T, K, H1, H2):
    return (K % 4 == 0 and 4 <= K <= 64 and 1 <= T <= 256 and 1 <= H1 <= 128 and 1 <= H2 <= 64 and 4 * K * H1 + H1 * H2 <= MAX_PARAMS
            and layout(T, K, H1, H2)["NS"] > 0)


def grid(B, NS):
    return min(-(-B // NS), GRID_CAP)


# ---------------------------------------------------------------------------------------------------- the builder
def _sparse_columns(rng, rows, cols, add):
    """[rows, cols] with min(4, rows) entries of +-1 per column at random rows.  Entries of rows that hold several then move, inside
    their column, to rows that hold none, while there are both; add: every row still empty gets one entry in a random column."""
    W = np.zeros((rows, cols))
    n = min(4, rows)
    for j in range(cols):
        W[rng.permutation(rows)[:n], j] = rng.choice([-1.0, 1.0], n)
    for i in np.flatnonzero(~W.any(1)):
        count = (W != 0).sum(1)
        donors = np.argwhere((W != 0) & (count[:, None] >= 2))
        if len(donors) == 0:
            break
        r, j = donors[rng.integers(len(donors))]
        W[i, j], W[r, j] = W[r, j], 0.0
    if add:
        for i in np.flatnonzero(~W.any(1)):
            W[i, rng.integers(cols)] = rng.choice([-1.0, 1.0])
    return W


def edge_mask(B, T, rng):
    """Ragged, but sample 0 has no live slot, sample 1 all, sample 2 only slot 0 and sample 3 only slot T - 1 (B >= 4)."""
    assert B >= 4
    m = ref.make_mask(B, T, "ragged", rng)
    m[0] = 0
    m[1] = 1
    m[2] = 0
    m[2, 0] = 1
    m[3] = 0
    m[3, T - 1] = 1
    return m


def lattice_case(B, T, K, H1, H2, seed=0, mask="ragged"):
    """A PReLU case on the lattice in the format of din_attn_ref.make_case (float64 arrays; softmax=False: the harness sets it), with
    quantum = QUANTUM and bound = abs_bound(case).  mask: "ragged", None, "edges" (edge_mask; with B >= 5 the live keys of sample 4
    are all the same row) or an array."""
    rng = np.random.default_rng([seed, B, T, K, H1, H2])
    draw = lambda vals, shape, p=None: rng.choice(np.asarray(vals, np.float64), shape, p=p)
    case = dict(activation="prelu", softmax=False, shape=(B, T, K, H1, H2), seed=seed,
                W1=_sparse_columns(rng, 4 * K, H1, add=False), b1=draw([-1, 0, 1], H1), alpha1=draw([0, 0.25, 0.5], H1),
                W2=_sparse_columns(rng, H1, H2, add=True), b2=draw([-1, 0, 1], H2), alpha2=draw([0, 0.25, 0.5], H2),
                w3=draw([-1, 1], H2), b3=np.array([1.0]),
                g=draw([-2, -1, 0, 1, 2], (B, K), p=[0.1, 0.35, 0.1, 0.35, 0.1]),
                q=draw([-1, 0, 1], (B, K), p=[0.4, 0.2, 0.4]), keys=draw([-1, 0, 1], (B, T, K), p=[0.4, 0.2, 0.4]))
    if isinstance(mask, str) and mask == "edges":
        case["mask"] = edge_mask(B, T, rng)
        if B >= 5:
            case["mask"][4, :min(2, T)] = 1
            case["keys"][4] = case["keys"][4, 0]
    else:
        case["mask"] = ref.make_mask(B, T, mask, rng)
    case["quantum"] = QUANTUM
    case["bound"] = abs_bound(case)
    return case


def abs_bound(case):
    """dict over TENSORS and the intermediate sums (u1, u2, s, ds, dh1, dx): every sum the raw-mode PReLU reference forms, with |term|
    in place of every term -- elementwise upper bounds of the absolute value of every partial sum in any order.  The terms are products
    of the reference's own intermediate values, so the proof goes in evaluation order: a sum whose bound is below EXACT_BELOW is exact
    in fp32 in any order, its value is then the reference's, and the products that the next sum adds are the reference's too.  (It
    covers every evaluation that forms these sums, whatever their order and grouping: csrc/din.hip's header lists the same ones.)"""
    p = ref._parts(dict(case, softmax=False))
    A = np.abs
    live, k, q, W1, W2, w3 = p["live"], A(p["keys"]), A(p["qe"]), A(p["W1"]), A(p["W2"]), A(p["w3"])
    g = np.asarray(case["g"], np.float64)
    b1, b2, b3 = (A(np.asarray(case[n], np.float64)).reshape(-1) for n in ("b1", "b2", "b3"))
    K = k.shape[2]
    dact = lambda u, al: np.where(u > 0, 1.0, al)
    ds = np.einsum("bk,btk->bt", g, p["keys"]) * live
    dh2 = ds[:, :, None] * p["w3"]
    du2 = dh2 * dact(p["u2"], p["a2"])
    dh1 = du2 @ p["W2"].T
    du1 = dh1 * dact(p["u1"], p["a1"])
    dx = A(du1 @ p["W1"].T)
    dxa, dxb, dxc, dxd = dx[..., :K], dx[..., K:2 * K], dx[..., 2 * K:3 * K], dx[..., 3 * K:]
    neg = lambda u: np.where(u > 0, 0.0, u)
    return dict(u1=A(p["x"]) @ W1 + b1, u2=A(p["h1"]) @ W2 + b2, s=(A(p["h2"]) @ w3 + b3[0]) * live,
                ds=np.einsum("bk,btk->bt", A(g), k) * live, dh1=A(du2) @ W2.T, dx=A(du1) @ W1.T,
                out=(A(p["a"])[:, :, None] * k).sum(1), dq=(dxa + dxc + k * dxd).sum(1),
                dkeys=(A(p["a"])[:, :, None] * A(g)[:, None, :] + dxb + dxc + q * dxd) * live[:, :, None],
                dW1=np.einsum("bti,btj->ij", A(p["x"]), A(du1)), db1=A(du1).sum((0, 1)), dalpha1=A(dh1 * neg(p["u1"])).sum((0, 1)),
                dW2=np.einsum("btj,btm->jm", A(p["h1"]), A(du2)), db2=A(du2).sum((0, 1)), dalpha2=A(dh2 * neg(p["u2"])).sum((0, 1)),
                dw3=np.einsum("bt,btm->m", A(ds), A(p["h2"])), db3=np.array([A(ds).sum()]))


def reference(case, softmax=False):
    """dict over TENSORS of the fp64 reference in the given mode."""
    c = dict(case, softmax=softmax)
    bwd = ref.backward(c)
    return dict(out=ref.forward(c), **{k: bwd[k] for k in ref.GRADS})


def zero_fractions(case):
    """(layer 1, layer 2): the fraction of the live slots' pre-activations that are exactly 0."""
    p = ref._parts(case)
    return float((p["u1"][p["live"]] == 0).mean()), float((p["u2"][p["live"]] == 0).mean())


# ---------------------------------------------------------------------------------------------------- the case table
# (T, K, H1, H2) -> the (H2T, NT, NS) the launchers must pick
PATHS = collections.OrderedDict([
    ((3, 8, 20, 32), (32, 1, 4)),
    ((5, 4, 8, 17), (32, 1, 4)),        # H2 just past a 16 boundary
    ((3, 4, 128, 17), (32, 1, 2)),
    ((3, 16, 128, 32), (32, 1, 2)),     # 4 K H1 + H1 H2 = 12288
    ((3, 32, 112, 18), (32, 2, 1)),     # 280 tiles
    ((3, 36, 100, 10), (16, 2, 2)),     # K / 4 odd, so KP = K; backward LDS 161 008 of 163 328
    ((3, 64, 63, 1), (16, 2, 2)),       # H1 = 8 n - 1, H2 = 1
    ((3, 64, 56, 33), (48, 2, 1)),      # 298 tiles
    ((3, 60, 60, 33), (48, 2, 1)),      # K / 4 odd
    ((3, 16, 80, 40), (48, 1, 3)),      # backward LDS 162 320, the closest fit
    ((5, 48, 64, 48), (48, 1, 2)),
    ((3, 64, 36, 16), (16, 1, 3)),
    ((3, 16, 128, 64), (64, 1, 1)),     # exactly 256 tiles, the NT boundary
    ((64, 28, 9, 64), (64, 1, 4)),      # H1 = 9: one real unit in the second chunk of 8
    ((65, 20, 63, 49), (64, 1, 2)),
    ((3, 20, 113, 49), (64, 2, 1)),     # 276 tiles: the menu does reach NT = 2 at H2T = 64; H1 = 16 n + 1, H2 = 48 + 1, K / 4 odd
])
SLOT_TRIPS = (63, 64, 65, 128, 129, 192, 193, 255, 256)
SLOT_SHAPES = ((8, 20, 32), (64, 56, 33))
# the shape of each NS that runs all of B_EDGES
EDGE_SHAPES = {1: (3, 16, 128, 64), 2: (3, 36, 100, 10), 3: (3, 16, 80, 40), 4: (3, 8, 20, 32)}
# the shapes that also run without a mask and with edge_mask
MASK_SHAPES = ((3, 8, 20, 32), (3, 36, 100, 10), (3, 64, 56, 33), (64, 28, 9, 64))


def B_EDGES(NS):
    """NS - 1, NS, NS + 1: one partial, then two, the last one short; 15 NS, 16 NS, 16 NS + 1: the partial count on both sides of one
    round of param_reduce_kernel's 16 slices; 512 NS + 1: a second grid-stride trip that one workgroup makes with one sample."""
    return tuple(b for b in (NS - 1, NS, NS + 1, 15 * NS, 16 * NS, 16 * NS + 1, GRID_CAP * NS + 1) if b >= 1)


Case = collections.namedtuple("Case", "group B T K H1 H2 mask")
Case.dims = property(lambda c: (c.T, c.K, c.H1, c.H2))
Case.shape = property(lambda c: (c.B, c.T, c.K, c.H1, c.H2))
Case.id = property(lambda c: "%s-%s%s" % (c.group, "x".join(map(str, c.shape)), {"ragged": "", None: "-nomask", "edges": "-edgemask"}[c.mask]))
Case.plan = property(lambda c: layout(*c.dims))


REPEAT = Case("repeat", 513, 3, 32, 112, 18, "ragged")      # NT = 2, NS = 1 and a second grid-stride trip: run twice


def _cases():
    out = []
    for ns, dims in sorted(EDGE_SHAPES.items()):
        out += [Case("batch", b, *dims, "ragged") for b in B_EDGES(ns)]
    for dims, (_, _, ns) in PATHS.items():
        if dims not in EDGE_SHAPES.values():
            # (16 NS + 1: 17 partials once more, and enough slots for every unit to be active in one of them)
            out += [Case("path", b, *dims, "ragged") for b in (ns + 1, 2 * ns + 3, 16 * ns + 1)]
    for khh in SLOT_SHAPES:
        for T in SLOT_TRIPS:
            out.append(Case("slots", layout(T, *khh)["NS"] + 1, T, *khh, "ragged"))
    for dims in MASK_SHAPES:
        ns = PATHS[dims][2]
        out += [Case("mask", 2 * ns + 3, *dims, None), Case("mask", 2 * ns + 3, *dims, "edges")]
    out.append(REPEAT)
    return out


CASES = _cases()
# The seed of a case is the first of 0, 1, 2, ... at which the inputs meet every condition of tests/test_din_lattice_host.py (bound,
# ties, dense dW1, conditioning and E32 of the softmax run); the cases that need another seed than 0 are listed.  The reference alone
# decides.
SEEDS = {"batch-1x3x16x128x64": 127, "batch-1x3x36x100x10": 17, "path-3x3x4x128x17": 2, "path-2x3x32x112x18": 3, "path-3x3x64x63x1": 21,
         "path-7x3x64x63x1": 102, "path-2x3x60x60x33": 2, "path-2x3x20x113x49": 1,
         "path-33x3x4x128x17": 1, "path-33x3x16x128x32": 5, "path-17x3x60x60x33": 1, "path-65x64x28x9x64": 10, "path-17x3x20x113x49": 2,"slots-5x193x8x20x32": 1, "slots-5x256x8x20x32": 3}


@functools.lru_cache(maxsize=None)
def build(case):
    """The inputs of one case, built once (shared by the raw and the softmax run; never written)."""
    return lattice_case(*case.shape, seed=SEEDS.get(case.id, 0), mask=case.mask)
