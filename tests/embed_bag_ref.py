"""numpy restatement of the pooled multi-valued fields (include/fil.h N3, ml_function_amd.functional.embed_bag): what
tf.nn.safe_embedding_lookup_sparse computes without weights, with the arithmetic order the kernel is held to.

Forward: fp32, sequential in the slot index t -- acc starts at +0 and takes one fp32 addition per live slot in ascending t (a dead slot
adds the constant +0, which changes no bit of a sum that started at +0), then ONE fp32 division by float32(n) (mean) or
sqrt(float32(n)) (sqrtn).  numpy's float32 add, divide and sqrt are correctly rounded, so a kernel that follows the same order must
agree bit for bit.  Gradient: the rows g / d (the same fp32 division) summed per table row in int64 (integer-valued g) or float64.
The expanded one-hot form restates a [B,F,T] bag batch as a [B, F T] one-id batch over F T virtual fields that share the F tables."""
import numpy as np

f32 = np.float32
COMBINERS = ("sum", "mean", "sqrtn")


def masks(idx, sizes, padding_id):
    """(live, oob) [B,F,T] bool: a slot is padding iff id == padding_id (None: never), out of range iff it is not padding and its id
    lies outside [0, sizes[f]); every other slot is live."""
    idx = np.asarray(idx, np.int64)
    sizes = np.asarray(sizes, np.int64).reshape(1, -1, 1)
    pad = np.zeros(idx.shape, bool) if padding_id is None else idx == padding_id
    inside = (idx >= 0) & (idx < sizes)
    return ~pad & inside, ~pad & ~inside


def divisor(count, combiner):
    """fp32 divisor of every bag ([B,F]); 1 where the bag is empty or the combiner is the sum (x / 1 == x)."""
    n = np.asarray(count).astype(f32)
    d = n if combiner == "mean" else np.sqrt(n) if combiner == "sqrtn" else np.ones_like(n)
    assert combiner in COMBINERS and d.dtype == f32
    return np.where(n > 0, d, f32(1))


def forward(table, offsets, sizes, idx, combiner="mean", padding_id=0):
    """-> out [B,F,K] fp32, count [B,F] int32 (= n), oob (number of out-of-range slots)."""
    table = np.asarray(table, f32)
    idx = np.asarray(idx, np.int64)
    B, F, T = idx.shape
    live, oob = masks(idx, sizes, padding_id)
    rows = np.where(live, idx + np.asarray(offsets, np.int64).reshape(1, F, 1), 0)
    acc = np.zeros((B, F, table.shape[1]), f32)
    for t in range(T):                                   # ascending t, one fp32 addition per slot
        acc = acc + np.where(live[:, :, t, None], table[rows[:, :, t]], f32(0))
        assert acc.dtype == f32
    count = live.sum(2).astype(np.int32)
    out = acc / divisor(count, combiner)[:, :, None]
    assert out.dtype == f32
    return out, count, int(oob.sum())


def scaled_grad(g, count, combiner):
    """gs [B,F,K] fp32 = g / d with the forward's divisor (zeros for an empty bag: nothing reads them); the sum takes g as it is."""
    g = np.asarray(g, f32)
    if combiner == "sum":
        return g
    gs = g / divisor(count, combiner)[:, :, None]
    assert gs.dtype == f32
    return np.where(np.asarray(count)[:, :, None] > 0, gs, f32(0))


def table_grad(n_rows, offsets, sizes, idx, gs, padding_id=0, frozen=None, dtype=np.float64):
    """[n_rows, K] sums of gs[b,f] over every live slot of (b,f) (once per occurrence), in `dtype` (int64 for integer-valued gs,
    float64 otherwise), and the mask of touched rows.  frozen [F]: fields whose rows get nothing."""
    idx = np.asarray(idx, np.int64)
    B, F, T = idx.shape
    live, _ = masks(idx, sizes, padding_id)
    if frozen is not None:
        live = live & ~np.asarray(frozen, bool).reshape(1, F, 1)
    rows = idx + np.asarray(offsets, np.int64).reshape(1, F, 1)
    b, f, t = np.nonzero(live)
    out = np.zeros((n_rows, gs.shape[-1]), dtype)
    np.add.at(out, rows[b, f, t], np.asarray(gs)[b, f].astype(dtype))
    touched = np.zeros(n_rows, bool)
    touched[rows[b, f, t]] = True
    return out, touched


def expanded(offsets, sizes, idx, gs, padding_id=0, frozen=None, field_l2=None):
    """The one-hot form: ids [B, F T] (padding -> -1, which every range check drops), offsets / sizes / frozen / field_l2 [F T] (field
    f repeated T times) and g_exp [B, F T, K] with g_exp[b, f T + t] = gs[b, f].  Slot (b, f, t) sits at flat position
    (b F + f) T + t in both forms."""
    idx = np.asarray(idx, np.int64)
    B, F, T = idx.shape
    ids = idx.copy()
    if padding_id is not None:
        ids[idx == padding_id] = -1
    rep = lambda a, dt: None if a is None else np.repeat(np.asarray(a, dt), T)
    g_exp = None if gs is None else np.repeat(np.asarray(gs, f32), T, axis=1)
    return dict(ids=ids.reshape(B, F * T), offsets=rep(offsets, np.int64), sizes=rep(sizes, np.int64), frozen=rep(frozen, np.uint8),
                field_l2=rep(field_l2, f32), g=g_exp)
