"""Constructed inputs and a plain numpy reference for the device walks every fused table optimizer shares (ml_function_amd/csrc/
optim_rows.h, optim_rule.h, optim_adam.h): the sweep's compacted field table (load_reg_tab / reg_field), the field search of the Adam
sweep and of every merged update (sweep_field), the merged walk of W gathered lists (merged_row_sums), the grid-stride loops behind
the 2048-workgroup cap, and the dense descriptor walk (multi_tensor_walk_desc).  TEST INFRASTRUCTURE: numpy only, no GPU, no library.
tests/test_optim_walk_cases_host.py checks that every case has the properties tests/test_optim_walk_edges_gpu.py relies on.

Every gradient value is an integer in [-8, 8] times a power of two (2^-6 unless said otherwise), so a sum of a row's copies is exact
in fp32 in any order: "the row's summed gradient" is one value and the comparisons with the fp32 restatement need no tolerance for it.
A field f that is regularised has l2 = 1e-2 (1 + f % 7): neighbouring fields differ, a row given its neighbour's field has wrong bits.
"""
import numpy as np

F32 = np.float32
SENT_BITS = 0x7FC12345                     # tests/guarded.py's sentinel: a quiet NaN with a payload
INT64_MAX = np.iinfo(np.int64).max
MAX_F = 1024                               # kSweepMaxF
LANE_FIELDS, WAVE_FIELDS = 4, 256          # load_reg_tab: fields per lane, fields per wave of 64 lanes
MERGE_CHUNK = 16                           # kMergeChunk
GRID_LANES = 2048 * 256                    # stride_grid's cap: 2048 workgroups of 256 lanes
DENSE_CHUNK, GRID_CHUNKS = 1024, 2048      # kMultiChunk and the dense launch's grid cap


def sentinel_f32(shape):
    return np.full(shape, SENT_BITS, np.uint32).view(F32)


def grad_values(rng, shape, shift=6):
    """Integers in [-8, 8] times 2^-shift, as float32."""
    return (rng.integers(-8, 9, size=shape).astype(np.float64) * 2.0 ** -shift).astype(F32)


def l2_of_field(f):
    return F32(1e-2 * (1 + f % 7))


# ------------------------------------------------------------------------------------------------------------------ field layouts
FIELD_SIZES = (1, 4, 5, 255, 256, 257, 1023, 1024)
LAYOUT_KINDS = ("roles", "only_last", "only_first", "none", "all")


def _layout(rows, l2, frozen):
    rows = np.asarray(rows, np.int64)
    offsets = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
    return dict(F=len(rows), V=int(rows.sum()), rows=rows, offsets=offsets, l2=np.asarray(l2, F32), frozen=np.asarray(frozen, np.uint8))


def field_layout(F, kind="roles", seed=0):
    """F fields of 0 to 3 rows each -> dict(F, V, rows, offsets [F], l2 [F] (0: not regularised), frozen [F]).
    roles       from the seed: regularised, plain, frozen and zero-row fields; the fields on both sides of every multiple of 4 (a lane of
                load_reg_tab holds 4 fields; 256, 512, 768: a wave's) are regularised and have rows, the others take any role, so the
                compacted table has gaps of every length up to 2 inside a lane; from F = 4 on field 1 has no rows
    only_last   only field F - 1 regularised      only_first   only field 0      none   no field (l2 all zero)      all   every field
    A zero-row field of "roles" keeps an l2 of its own, and some are frozen: neither may reach a row."""
    assert kind in LAYOUT_KINDS and 1 <= F <= MAX_F
    rng = np.random.default_rng([F, seed, LAYOUT_KINDS.index(kind)])
    rows = rng.integers(0, 4, F)
    role = rng.choice(4, F, p=[0.3, 0.25, 0.2, 0.25])                      # 0 regularised, 1 plain, 2 frozen, 3 zero-row
    f = np.arange(F)
    if kind == "roles":
        edge = (f % LANE_FIELDS == 0) | (f % LANE_FIELDS == LANE_FIELDS - 1)
        role[edge] = 0
        rows[edge] = rng.integers(1, 3, F)[edge]
        if F >= 4:
            role[1] = 3
            role[2] = 1 if F == 4 else 2
    elif kind == "all":
        role[:] = 0
        rows = np.minimum(rows, 2)
    else:
        role[role == 0] = 1
        if kind == "only_last":
            role[F - 1] = 0
        if kind == "only_first":
            role[0] = 0
    rows[role == 3] = 0
    rows[(role != 3) & (rows == 0)] = 1
    if rows.sum() == 0:
        rows[0], role[0] = 1, 1
    l2 = np.where(role == 0, [l2_of_field(x) for x in f], F32(0)).astype(F32)
    frozen = role == 2
    if kind == "roles":
        zero = np.nonzero(role == 3)[0]
        l2[zero[::2]] = [l2_of_field(x) for x in zero[::2]]
        frozen[zero[1::3]] = True
    return _layout(rows, l2, frozen)


def walked_fields(lay, sweep_all):
    """The fields whose untouched rows a rule's sweep walks: non-frozen with rows, and regularised unless the rule is kSweepAll."""
    return (lay["rows"] > 0) & (lay["frozen"] == 0) & (sweep_all | (lay["l2"] > 0))


def field_of_row(lay):
    f = np.searchsorted(lay["offsets"], np.arange(lay["V"]), side="right") - 1
    assert (f >= 0).all()
    return f


def row_maps(lay):
    """-> (row_l2 [V] float32, row_frozen [V] bool)."""
    f = field_of_row(lay)
    return lay["l2"][f].astype(F32), lay["frozen"][f].astype(bool)


def row_maps_slow(lay):
    row_l2, frozen = np.zeros(lay["V"], F32), np.zeros(lay["V"], bool)
    for r in range(lay["V"]):
        f = max(x for x in range(lay["F"]) if lay["offsets"][x] <= r)
        row_l2[r], frozen[r] = lay["l2"][f], bool(lay["frozen"][f])
    return row_l2, frozen


def two_field_layout(V, first, l2_first=False):
    """The grid-cap tables: a short first field and a regularised second one holding the rest."""
    return _layout([first, V - first], [l2_of_field(0) if l2_first else 0, l2_of_field(1)], [0, 0])


def split_layout(lay, seed=0, target=MAX_F):
    """The same table described with `target` fields: every field cut into sub-fields of its own role, and zero-row sub-fields (of the
    role of the field they sit in) in between.  Every row keeps its l2 and its frozen flag."""
    rng = np.random.default_rng([lay["F"], seed, 77])
    F, rows = lay["F"], lay["rows"]
    budget = target - F
    assert budget > 0
    room = np.maximum(rows - 1, 0)
    real = int(min(room.sum(), budget * 3 // 4))
    extra = np.minimum(room, real // max(1, int((room > 0).sum())))          # an even share, then the remainder one by one
    left = real - int(extra.sum())
    for f in np.nonzero(room > extra)[0]:
        if left == 0:
            break
        add = int(min(left, room[f] - extra[f]))
        extra[f] += add
        left -= add
    empty = np.bincount(rng.integers(0, F, budget - int(extra.sum())), minlength=F)      # zero-row sub-fields per field
    sub_rows, sub_l2, sub_frozen = [], [], []
    for f in range(F):
        cuts = np.sort(rng.choice(np.arange(1, rows[f]), extra[f], replace=False)) if extra[f] else np.zeros(0, np.int64)
        parts = list(np.diff(np.concatenate([[0], cuts, [rows[f]]]))) + [0] * int(empty[f])
        parts = [parts[i] for i in rng.permutation(len(parts))]
        sub_rows += parts
        sub_l2 += [lay["l2"][f]] * len(parts)
        sub_frozen += [lay["frozen"][f]] * len(parts)
    out = _layout(sub_rows, sub_l2, sub_frozen)
    assert out["F"] == target and out["V"] == lay["V"]
    return out


# ------------------------------------------------------------------------------------------------------------------ the runs batch
def touch_batch(lay, K, seed, n_random=12):
    """One batch's record for a runs update (g, perm, sorted_ids as SparseEmbed leaves them): it touches the first row of a field, the
    last row of a field, row 0 and row V - 1 and a few others, some twice or three times; a row of a frozen field arrives as id -1,
    as the layer sends it.  perm = position * F + field, so perm % F is the row's field; g is the sentinel NaN wherever no entry
    points.  -> dict(g [R * F, K], perm [R], sorted_ids [R], R, rows (the touched rows), sums [V, K] float32, touched [V])."""
    rng = np.random.default_rng([lay["F"], K, seed, 5])
    F, V, off, rows = lay["F"], lay["V"], lay["offsets"], lay["rows"]
    fld, (_, frozen) = field_of_row(lay), row_maps(lay)
    have = np.nonzero(rows > 0)[0]
    pick = have[rng.integers(0, len(have), 6)]
    want = [0, V - 1] + [int(off[f]) for f in pick[:3]] + [int(off[f] + rows[f] - 1) for f in pick[3:]]
    want += [int(r) for r in rng.integers(0, V, n_random)]
    entries = []
    for r in sorted(set(want)):
        entries += [r] * int(rng.integers(1, 4))
    ids = np.array([-1 if frozen[r] else r for r in entries] + [-1, -1], np.int64)
    fields = np.array([fld[r] for r in entries] + [0, F - 1], np.int64)
    order = np.argsort(ids, kind="stable")
    ids, fields = ids[order], fields[order]
    R = len(ids)
    perm = rng.permutation(R).astype(np.int64) * F + fields                # batch positions in any order, perm % F the entry's field
    g = sentinel_f32((R * F, K))
    g[perm] = grad_values(rng, (R, K))
    live = ids >= 0
    sums = np.zeros((V, K), F32)
    np.add.at(sums, ids[live], g[perm[live]])
    touched = np.zeros(V, bool)
    touched[ids[live]] = True
    return dict(g=g, perm=perm, sorted_ids=ids, R=R, sums=sums, touched=touched, interest=want[:8])


def runs_sums_slow(b, V):
    """The batch's summed gradients row by row, in float64."""
    sums, touched = np.zeros((V, b["g"].shape[1])), np.zeros(V, bool)
    for j in range(b["R"]):
        r = int(b["sorted_ids"][j])
        if r >= 0:
            sums[r] += b["g"][b["perm"][j]].astype(np.float64)
            touched[r] = True
    return sums, touched


# ------------------------------------------------------------------------------------------------------------------ merged lists
MERGED_K = (1, 15, 16, 17, 32, 33, 100, 256)
MERGED_W = (1, 2, 5, 8)
MERGED_ROWS = (13, 1, 0, 29, 17, 5, 32)                                    # F = 7, V = 97, field 2 without rows
PATTERNS = ("only_first", "only_last", "all", "first_and_last", "one_middle")


def merged_layout():
    return _layout(MERGED_ROWS, [l2_of_field(f) if f in (0, 1, 3, 6) else 0 for f in range(7)], [0] * 7)


def patterns_of(W):
    """The membership patterns W lists can show (the others coincide with one of these)."""
    return PATTERNS if W >= 3 else (PATTERNS[:3] if W == 2 else PATTERNS[:1])


def merged_roles(W):
    """-> dict: which list is clipped (count > cap, the list full), empty (count 0), negative (count -1), and the middle list that
    holds the one_middle rows.  W >= 5: a list of each kind, the middle list also the clipped one; below that list 0 is clipped."""
    if W >= 5:
        return dict(clipped=1, empty=2, negative=3, middle=1)
    return dict(clipped=0, empty=None, negative=None, middle=1 if W == 3 else None)


def merged_case(K, W, lay=None, seed=0, n_rows=30):
    """W ascending, distinct lists of cap entries each, side by side, built by hand.
    -> dict(ids [W * cap], values [W * cap, K], counts [W], cap, W, K, lay, member {pattern: rows}, roles, oob).
    Rows at the starts and ends of fields take the patterns in turn; the clipped list is filled up to cap with rows of its own and its
    count says more; the negative list holds in-range ids and the sentinel NaN throughout.  List 0 holds the ids -2^40, -1, V and V + 5,
    the last list -1 and V (W >= 2), a middle list V + 5 (W >= 3): skipped, never stamped.  Behind its count a list holds INT64_MAX (even
    lists) or in-range ids (odd lists), and the sentinel NaN as values."""
    lay = merged_layout() if lay is None else lay
    rng = np.random.default_rng([K, W, lay["F"], seed])
    V, off, rows = lay["V"], lay["offsets"], lay["rows"]
    have = np.nonzero(rows > 0)[0]
    if len(have) > 12:
        have = have[np.sort(rng.choice(len(have), 12, replace=False))]
    interest = sorted(set([0, V - 1] + [int(off[f]) for f in have] + [int(off[f] + rows[f] - 1) for f in have]))
    pool = np.setdiff1d(np.arange(V), interest)
    chosen = interest + [int(r) for r in rng.choice(pool, max(0, n_rows - len(interest)), replace=False)]
    pats, roles = patterns_of(W), merged_roles(W)
    live = [w for w in range(W) if w not in (roles["empty"], roles["negative"])]
    member = {p: [] for p in pats}
    lists = [set() for _ in range(W)]
    for i, r in enumerate(chosen):
        p = pats[i % len(pats)]
        member[p].append(r)
        on = dict(only_first=[0], only_last=[W - 1], all=live, first_and_last=[0, W - 1], one_middle=[roles["middle"]])[p]
        for w in on:
            lists[w].add(r)
    cap = max(len(s) for s in lists) + 7
    spare = list(rng.permutation(np.setdiff1d(np.arange(V), chosen)))
    oob = {0: [-(1 << 40), -1, V, V + 5]}
    if W >= 2:
        oob[W - 1] = [-1, V]
    if W >= 3:
        oob[1] = oob.get(1, []) + [V + 5]
    c = roles["clipped"]
    fill = cap - len(lists[c]) - len(oob.get(c, []))
    assert 0 < fill <= len(spare)
    own = [int(r) for r in spare[:fill]]
    lists[c] |= set(own)
    member["only_first" if c == 0 else "one_middle"] += own
    ids = np.full((W, cap), INT64_MAX, np.int64)
    values = sentinel_f32((W, cap, K))
    counts = np.zeros(W, np.int64)
    for w in range(W):
        if w == roles["negative"]:
            ids[w] = np.sort(rng.choice(V, cap, replace=False))
            counts[w] = -1
            continue
        full = np.array(sorted(lists[w] | set(oob.get(w, []))), np.int64)
        n = len(full)
        assert n <= cap and (w != roles["empty"] or n == 0)
        ids[w, :n] = full
        values[w, :n] = grad_values(rng, (n, K))
        counts[w] = n
        if w % 2 == 1:
            ids[w, n:] = rng.integers(0, V, cap - n)
    assert counts[c] == cap
    counts[c] = cap + 3
    return dict(ids=ids.reshape(-1), values=values.reshape(W * cap, K), counts=counts, cap=cap, W=W, K=K, lay=lay, member=member,
                roles=roles, oob=oob)


def valid_prefixes(case):
    """[(w, ids, values)] of every list's valid prefix: its count clipped to [0, cap]."""
    W, cap, K = case["W"], case["cap"], case["K"]
    ids, values = case["ids"].reshape(W, cap), case["values"].reshape(W, cap, K)
    out = []
    for w in range(W):
        n = int(min(max(case["counts"][w], 0), cap))
        out.append((w, ids[w, :n], values[w, :n]))
    return out


def merged_reference(case):
    """-> (sums [V, K] float32, touched [V] bool): the concatenation of the valid prefixes, ids outside [0, V) dropped, summed."""
    V, K = case["lay"]["V"], case["K"]
    ids = np.concatenate([i for _, i, _ in valid_prefixes(case)])
    values = np.concatenate([v for _, _, v in valid_prefixes(case)])
    ok = (ids >= 0) & (ids < V)
    sums = np.zeros((V, K), F32)
    np.add.at(sums, ids[ok], values[ok])
    touched = np.zeros(V, bool)
    touched[ids[ok]] = True
    return sums, touched


def merged_reference_slow(case):
    """The same row by row in float64, lists in order."""
    V, K = case["lay"]["V"], case["K"]
    sums, touched = np.zeros((V, K)), np.zeros(V, bool)
    for r in range(V):
        for _, ids, values in valid_prefixes(case):
            for j in range(len(ids)):
                if int(ids[j]) == r:
                    sums[r] += values[j].astype(np.float64)
                    touched[r] = True
    return sums, touched


def one_list(sums, touched, pad=3, seed=0):
    """The summed rows as ONE gathered list (W = 1): what the merged update of the W lists must equal bit for bit."""
    rng = np.random.default_rng([int(touched.sum()), seed])
    rows = np.nonzero(touched)[0].astype(np.int64)
    n, K = len(rows), sums.shape[1]
    ids = np.concatenate([rows, np.full(pad, INT64_MAX, np.int64)])
    values = np.concatenate([sums[rows], sentinel_f32((pad, K))])
    return dict(ids=ids, values=values, counts=np.array([n], np.int64), cap=n + pad, W=1, K=K)


def big_merged_case(fill_last):
    """The merged grid-cap case: W = 2, cap = 262 144 + 333, K = 1, V = 400 000, one field; list 0 the even rows, list 1 every third
    row.  W cap is past the cap's 524 288 lanes, but list 1 ends long before the lanes of the second trip (q >= 524 288 is entry
    261 811 ... of list 1); fill_last: list 1 holds the rows r with r % 3 != 1 instead, more than cap of them, so its count is clipped
    and the second trip's lanes hold valid entries."""
    V, cap, W, K = 400000, 262144 + 333, 2, 1
    rng = np.random.default_rng(9)
    r = np.arange(V, dtype=np.int64)
    l0, l1 = r[r % 2 == 0], (r[r % 3 != 1] if fill_last else r[r % 3 == 0])
    ids = np.full((W, cap), INT64_MAX, np.int64)
    values = sentinel_f32((W, cap, K))
    counts = np.array([len(l0), len(l1)], np.int64)
    for w, l in enumerate((l0, l1)):
        n = min(len(l), cap)
        ids[w, :n] = l[:n]
        values[w, :n] = grad_values(rng, (n, K))
    lay = _layout([V], [l2_of_field(3)], [0])
    return dict(ids=ids.reshape(-1), values=values.reshape(W * cap, K), counts=counts, cap=cap, W=W, K=K, lay=lay)


# ------------------------------------------------------------------------------------------------------------------ dense descriptors
BIG_DENSE = (2048 * 1024 + 1024 + 3, 5, 0, 1025, 1)                        # the last one has no gradient (grad NULL)
ROTATION_SIZES = tuple((1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025)[i % 10] for i in range(300))


def dense_chunks(sizes):
    return sum((n + DENSE_CHUNK - 1) // DENSE_CHUNK for n in sizes)


def dense_grid(total_numel):
    """The workgroups of the dense launch for a caller's total_numel."""
    return min(max(1, (total_numel + DENSE_CHUNK - 1) // DENSE_CHUNK), GRID_CHUNKS)


def dense_case(sizes, seed, none=()):
    """Flat p, slot and gradient arrays holding the tensors back to back (so most start off a 16-byte boundary and a store past a
    tensor's end lands in its neighbour), each tensor's start, and the descriptors' l2 (every third tensor has one)."""
    rng = np.random.default_rng([len(sizes), seed])
    n = int(sum(sizes))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    l2 = [float(l2_of_field(i)) if i % 3 == 1 else 0.0 for i in range(len(sizes))]
    return dict(sizes=tuple(sizes), starts=starts, none=tuple(none), l2=l2, p=(rng.standard_normal(n) * 0.5).astype(F32),
                s=(rng.standard_normal(n) * 0.1).astype(F32), g=grad_values(rng, n))


# ------------------------------------------------------------------------------------------------------------------ exactness
def sums_exact(values_by_row):
    """Is the fp32 sum of every group of addends its float64 sum?  values_by_row: [n, terms, K] float32 (zeros where a row has fewer)."""
    a = np.asarray(values_by_row, F32)
    s32 = np.zeros(a.shape[::2], F32)
    for t in range(a.shape[1]):
        s32 = s32 + a[:, t]
    return bool(np.array_equal(s32.astype(np.float64), a.astype(np.float64).sum(1)))
