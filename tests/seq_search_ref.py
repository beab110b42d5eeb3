"""The numpy restatement of the top-k retrieval over a long behaviour history (include/fil.h N3 fil_seq_search) that
tests/test_seq_search_host.py checks against brute force and tests/test_seq_search_gpu.py holds the kernel to, bit for bit: the fp32
sequential score, the integer keys, the selection and the output order.  A case is a dict of numpy arrays (None where a part is
absent): hist [B,T] int64, table [V,K] fp32, q [B,K] fp32, attr [B,T] int64, cand [B] int64, mask [B,T] uint8, and the scalars
offset, size (None: ids are trusted), pad, k, prefer ("first" / "last")."""
import numpy as np

KEY_ZERO = 0x80000000            # the key of +0


def make_case(hist, k, table=None, q=None, attr=None, cand=None, mask=None, offset=0, size=None, pad=0, prefer="first"):
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    i64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64)
    return dict(hist=i64(hist), k=int(k), table=f32(table), q=f32(q), attr=i64(attr), cand=i64(cand),
                mask=None if mask is None else np.ascontiguousarray(mask, np.uint8), offset=int(offset), size=size, pad=int(pad),
                prefer=prefer)


def live_slots(case):
    """-> (live [B,T] bool, the number of ids that are not padding and out of range)."""
    hist = case["hist"]
    slot = hist != case["pad"]
    ok = np.ones_like(slot) if case["size"] is None else (hist >= 0) & (hist < case["size"])
    live = slot & ok
    if case["mask"] is not None:
        live &= case["mask"] != 0
    if case["attr"] is not None:
        live &= case["attr"] == case["cand"][:, None]
    return live, int((slot & ~ok).sum())


def scores(case, live):
    """s = +0; for j ascending: s = fp32(s + fp32(row[j] * q[j])) at the live slots, +0 elsewhere and without the soft part."""
    B, T = case["hist"].shape
    s = np.zeros((B, T), np.float32)
    if case["table"] is None:
        return s
    rows = case["table"][np.where(live, case["hist"] + case["offset"], 0)]                       # [B,T,K]; dead slots are overwritten below
    with np.errstate(all="ignore"):
        for j in range(case["table"].shape[1]):
            p = (rows[:, :, j] * case["q"][:, j:j + 1]).astype(np.float32)
            s = (s + p).astype(np.float32)
    return np.where(live, s, np.float32(0.0)).astype(np.float32)


def keys(s):
    """The order-preserving unsigned key of fp32 bits, as int64."""
    bits = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.int64)
    return bits ^ np.where(bits >> 31 != 0, 0xFFFFFFFF, KEY_ZERO)


def search(case):
    """-> dict(sel_pos [B,k] int32, sel_idx [B,k] int64, sel_score [B,k] fp32, count [B] int32, oob int)."""
    hist, k = case["hist"], case["k"]
    B, T = hist.shape
    live, oob = live_slots(case)
    s = scores(case, live)
    key = keys(s)
    sel_pos = np.full((B, k), -1, np.int32)
    sel_idx = np.full((B, k), case["pad"], np.int64)
    sel_score = np.zeros((B, k), np.float32)
    count = np.zeros(B, np.int32)
    pos = np.arange(T)
    second = pos if case["prefer"] == "first" else -pos
    for b in range(B):
        cand = pos[live[b]]
        order = cand[np.lexsort((second[cand], -key[b, cand]))]                # key descending, then the preferred position
        chosen = np.sort(order[:k])
        n = len(chosen)
        count[b] = n
        sel_pos[b, :n] = chosen
        sel_idx[b, :n] = hist[b, chosen]
        sel_score[b, :n] = s[b, chosen]
    return dict(sel_pos=sel_pos, sel_idx=sel_idx, sel_score=sel_score, count=count, oob=oob, live=live, score=s)


def brute_force(case, score_fn=None):
    """The same selection by sorted() on tuples; score_fn(b, t) -> a Python float replaces the fp32 score (the float64 check)."""
    hist, k = case["hist"], case["k"]
    B, T = hist.shape
    live, _ = live_slots(case)
    s = scores(case, live)
    key = keys(s)
    sign = 1 if case["prefer"] == "first" else -1
    out = []
    for b in range(B):
        slots = [t for t in range(T) if live[b, t]]
        rank = (lambda t: (-score_fn(b, t), sign * t)) if score_fn is not None else (lambda t: (-int(key[b, t]), sign * t))
        out.append(sorted(sorted(slots, key=rank)[:k]))
    return out


def lattice_case(B, T, K, k, seed, vocab=40, prefer="first", **kw):
    """table and q in {-2..2}: every product and sum is an exact small integer, so the scores tie massively."""
    rng = np.random.default_rng(seed)
    table = rng.integers(-2, 3, (vocab, K)).astype(np.float32)
    q = rng.integers(-2, 3, (B, K)).astype(np.float32)
    hist = rng.integers(1, vocab, (B, T))
    return make_case(hist, k, table=table, q=q, size=vocab, prefer=prefer, **kw)


def random_case(B, T, K, k, seed, vocab=None, mode="soft", ragged=True, prefer="first", n_attr=3):
    """Random fp32 table and queries; ragged lengths padded with id 0; mode soft / hard / both."""
    rng = np.random.default_rng(seed)
    vocab = vocab or max(8, min(4 * T, 5000))
    hist = rng.integers(1, vocab, (B, T))
    if ragged:
        lens = rng.integers(0, T + 1, B)
        lens[0] = T
        hist[np.arange(T)[None, :] >= lens[:, None]] = 0
    table = q = attr = cand = None
    if mode != "hard":
        table = rng.standard_normal((vocab, K)).astype(np.float32)
        q = rng.standard_normal((B, K)).astype(np.float32)
    if mode != "soft":
        attr = rng.integers(0, n_attr, (B, T))
        cand = rng.integers(0, n_attr, B)
    return make_case(hist, k, table=table, q=q, attr=attr, cand=cand, size=vocab, prefer=prefer)
