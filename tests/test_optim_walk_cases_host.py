"""The constructed cases of tests/optim_walk_cases.py have the properties tests/test_optim_walk_edges_gpu.py relies on (no GPU): exact
fp32 sums, ascending distinct lists, every membership pattern, walked fields on both sides of the lane and wave boundaries of the
sweep's field table, work past the grid caps, and a numpy reference that agrees with a per-row Python loop."""
import numpy as np
import pytest

from tests import optim_walk_cases as wc

SMALL_MERGED = [(K, W) for K in (1, 17, 33) for W in wc.MERGED_W]


def _addends(case):
    """[V, W, K]: every row's copies, list by list (zeros where a list does not hold it)."""
    V, K = case["lay"]["V"], case["K"]
    a = np.zeros((V, case["W"], K), np.float32)
    for w, ids, values in wc.valid_prefixes(case):
        ok = (ids >= 0) & (ids < V)
        a[ids[ok], w] = values[ok]
    return a


# ------------------------------------------------------------------------------------------------------------------ field layouts
@pytest.mark.parametrize("kind", wc.LAYOUT_KINDS)
@pytest.mark.parametrize("F", wc.FIELD_SIZES)
def test_field_layouts(F, kind):
    lay = wc.field_layout(F, kind)
    assert lay["F"] == F and 1 <= lay["V"] <= 1600 and lay["rows"].max() <= 3 and lay["offsets"][0] == 0
    assert np.array_equal(np.diff(np.append(lay["offsets"], lay["V"])), lay["rows"])
    reg = wc.walked_fields(lay, False)
    want = dict(only_last=[F - 1], only_first=[0], none=[], all=list(range(F))).get(kind)
    if want is not None:
        assert list(np.nonzero(reg)[0]) == want
        assert kind != "none" or (lay["l2"] == 0).all()
        return
    # regularised fields differ from their neighbours, and every role is there from the first size that has room for it
    on = np.nonzero(lay["l2"] > 0)[0]
    assert all(lay["l2"][a] != lay["l2"][a + 1] for a in on[:-1] if lay["l2"][a + 1] > 0)
    for b in range(wc.LANE_FIELDS, F, wc.LANE_FIELDS):                    # every lane boundary, the wave boundaries among them
        assert reg[b - 1] and reg[b], b
    assert all(b >= F or (reg[b - 1] and reg[b]) for b in range(wc.WAVE_FIELDS, wc.MAX_F, wc.WAVE_FIELDS))
    if F >= 4:
        assert ((lay["rows"] == 0) & (lay["l2"] > 0)).any()               # a zero-row field with an l2 of its own
    if F >= 255:
        plain = (lay["rows"] > 0) & (lay["l2"] == 0) & (lay["frozen"] == 0)
        assert plain.any() and ((lay["rows"] > 0) & (lay["frozen"] == 1)).any()
        assert ((lay["rows"] == 0) & (lay["frozen"] == 1)).any()
        # the compacted table differs from the field table in every wave: a lane's count of walked fields takes 2, 3 and 4
        per_lane = np.add.reduceat(reg.astype(int), np.arange(0, F, 4))
        assert set(per_lane[:F // 4]) == {2, 3, 4}
        all_lane = np.add.reduceat(wc.walked_fields(lay, True).astype(int), np.arange(0, F, 4))
        assert (all_lane >= per_lane).all() and (all_lane > per_lane).any()


@pytest.mark.parametrize("F", [1, 4, 5, 255, 257])
def test_row_maps_agree_with_a_loop_over_rows(F):
    for kind in wc.LAYOUT_KINDS:
        lay = wc.field_layout(F, kind)
        a, b = wc.row_maps(lay), wc.row_maps_slow(lay)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("lay", [wc.field_layout(5), wc.field_layout(257), wc.two_field_layout(524288 + 2051, 1000),
                                 wc.two_field_layout(174763 + 517, 100)], ids=["F5", "F257", "big4", "big3"])
def test_split_description_keeps_every_rows_role(lay):
    sub = wc.split_layout(lay)
    assert sub["F"] == wc.MAX_F and sub["V"] == lay["V"] and (sub["rows"] == 0).sum() >= 100
    assert (np.diff(sub["offsets"]) >= 0).all()
    a, b = wc.row_maps(lay), wc.row_maps(sub)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len(set(sub["offsets"])) > lay["F"] or lay["V"] <= lay["F"]      # real cuts, not only empty sub-fields


# ------------------------------------------------------------------------------------------------------------------ the runs batch
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("F", wc.FIELD_SIZES)
def test_touch_batches(F, K):
    lay = wc.field_layout(F)
    fld, (_, frozen) = wc.field_of_row(lay), wc.row_maps(lay)
    starts, ends = set(lay["offsets"][lay["rows"] > 0]), set((lay["offsets"] + lay["rows"] - 1)[lay["rows"] > 0])
    for step in range(3):
        b = wc.touch_batch(lay, K, step)
        ids, perm = b["sorted_ids"], b["perm"]
        assert (np.diff(ids) >= 0).all() and (ids == -1).sum() >= 2 and ids.max() < lay["V"] and len(set(perm)) == b["R"]
        live = ids >= 0
        assert np.array_equal(perm[live] % F, fld[ids[live]]) and not frozen[ids[live]].any()
        want = [r for r in b["interest"] if not frozen[r]]
        assert b["touched"][want].all() and {0, lay["V"] - 1} <= set(b["interest"])
        assert set(b["interest"]) & starts and set(b["interest"]) & ends
        assert np.isnan(b["g"]).all(axis=1).sum() == b["g"].shape[0] - b["R"]        # poisoned wherever no entry points
        slow, touched = wc.runs_sums_slow(b, lay["V"])
        assert np.array_equal(b["sums"].astype(np.float64), slow) and np.array_equal(b["touched"], touched)
        assert np.bincount(ids[live]).max() >= 2


# ------------------------------------------------------------------------------------------------------------------ merged lists
def _check_merged_lists(case):
    W, cap, V = case["W"], case["cap"], case["lay"]["V"]
    roles = case["roles"]
    held = []
    for w, ids, values in wc.valid_prefixes(case):
        assert (np.diff(ids) > 0).all() and not np.isnan(values).any()
        held.append(set(int(i) for i in ids if 0 <= i < V))
    union = set().union(*held)
    on = lambda r: [w for w in range(W) if r in held[w]]
    for p in wc.patterns_of(W):
        rows = case["member"][p]
        assert len(rows) >= 2, p
        live = [w for w in range(W) if w not in (roles["empty"], roles["negative"])]
        want = dict(only_first=[0], only_last=[W - 1], all=live, first_and_last=[0, W - 1], one_middle=[roles["middle"]])[p]
        assert all(on(r) == want for r in rows), p
    lay = case["lay"]
    starts, ends = set(lay["offsets"][lay["rows"] > 0]), set((lay["offsets"] + lay["rows"] - 1)[lay["rows"] > 0])
    assert len(union & starts) >= 4 and len(union & ends) >= 4 and {0, V - 1} <= union
    assert 0 < len(union) < V                                               # some rows stay untouched
    # counts: one clipped (the list full), and from W = 5 on one empty middle list and one -1; the tails are poisoned
    counts = case["counts"]
    assert counts[roles["clipped"]] > cap
    ids, values = case["ids"].reshape(W, cap), case["values"].reshape(W, cap, -1)
    if W >= 5:
        assert counts[roles["empty"]] == 0 and counts[roles["negative"]] == -1 and 0 < roles["empty"] < W - 1
        neg = ids[roles["negative"]]
        assert ((neg >= 0) & (neg < V)).all() and (np.diff(neg) > 0).all() and not set(neg) <= union
    for w in range(W):
        n = int(min(max(counts[w], 0), cap))
        assert np.isnan(values[w, n:]).all()
        if n < cap and w != roles["negative"]:
            tail = ids[w, n:]
            assert (tail == wc.INT64_MAX).all() if w % 2 == 0 else ((tail >= 0) & (tail < V)).all()
    if W >= 2:
        assert any(c < cap and w % 2 == 1 for w, c in enumerate(counts))     # a tail of in-range ids
    # the ids outside [0, V): all four in one list, two of them in several
    flat = [int(i) for _, l, _ in wc.valid_prefixes(case) for i in l]
    for bad in (-1, -(1 << 40), V, V + 5):
        assert bad in flat
    assert W == 1 or (flat.count(-1) >= 2 and flat.count(V) >= 2)
    assert wc.sums_exact(_addends(case))
    sums, touched = wc.merged_reference(case)
    assert set(np.nonzero(touched)[0]) == union
    return sums, touched


@pytest.mark.parametrize("W", wc.MERGED_W)
@pytest.mark.parametrize("K", wc.MERGED_K)
def test_merged_cases(K, W):
    case = wc.merged_case(K, W)
    assert case["lay"]["F"] == 7 and case["lay"]["V"] == 97 and case["values"].shape == (W * case["cap"], K)
    sums, touched = _check_merged_lists(case)
    if (K, W) in SMALL_MERGED:
        slow, t2 = wc.merged_reference_slow(case)
        assert np.array_equal(sums.astype(np.float64), slow) and np.array_equal(touched, t2)
    one = wc.one_list(sums, touched)
    assert one["counts"][0] == touched.sum() and np.array_equal(one["values"][:one["counts"][0]], sums[touched])


def test_merged_widths_sit_on_both_sides_of_the_chunk():
    c = wc.MERGE_CHUNK
    assert {1, c - 1, c, c + 1, 2 * c, 2 * c + 1} <= set(wc.MERGED_K) and max(wc.MERGED_K) == 256 == 16 * c
    assert any(K % c not in (0, 1, c - 1) and K > 2 * c for K in wc.MERGED_K)          # a last chunk that is partly filled


def test_compound_merged_case():
    lay = wc.field_layout(257)
    case = wc.merged_case(33, 3, lay, n_rows=60)
    sums, touched = _check_merged_lists(case)
    row_l2, _ = wc.row_maps(lay)
    assert len(set(row_l2[touched])) >= 6                                   # rows of many differently regularised fields
    slow, t2 = wc.merged_reference_slow(case)
    assert np.array_equal(sums.astype(np.float64), slow) and np.array_equal(touched, t2)


# ------------------------------------------------------------------------------------------------------------------ the grid caps
def test_grid_cap_cases_are_past_the_cap():
    for V, K, first in ((524288 + 2051, 4, 1000), (174763 + 517, 3, 100)):
        lay = wc.two_field_layout(V, first)
        for sweep_all in (False, True):
            rows = int(lay["rows"][wc.walked_fields(lay, sweep_all)].sum())
            lanes = rows * K // 4 if K % 4 == 0 else rows * K
            assert lanes > wc.GRID_LANES, (V, K, sweep_all)                  # the rule sweeps stride over the walked rows only
        assert (V * K // 4 if K % 4 == 0 else V * K) > wc.GRID_LANES         # the Adam sweeps over the table
        b = wc.touch_batch(lay, K, 0, n_random=300)
        beyond = (wc.GRID_LANES * 4 // K if K % 4 == 0 else wc.GRID_LANES // K) + first
        assert 200 <= b["touched"].sum() <= 400 and b["touched"][beyond:].any() and b["touched"][V - 1]
    for fill in (False, True):
        case = wc.big_merged_case(fill)
        W, cap = case["W"], case["cap"]
        assert W * cap > wc.GRID_LANES and case["lay"]["V"] == 400000 and case["K"] == 1
        second = [(q // cap, q % cap) for q in (wc.GRID_LANES, W * cap - 1)]
        live = [i < min(max(case["counts"][w], 0), cap) for w, i in second]
        assert live == [fill, fill]                                          # only the filled case has entries in the second trip
        assert (case["counts"][1] > cap) == fill
        for w, ids, values in wc.valid_prefixes(case):
            assert (np.diff(ids) > 0).all() and not np.isnan(values).any()
        a = _addends(case)
        assert wc.sums_exact(a) and (np.abs(a).sum(2) > 0).all(1).any()      # some rows are held by both lists
    assert wc.dense_chunks(wc.BIG_DENSE) > wc.GRID_CHUNKS and wc.dense_grid(sum(wc.BIG_DENSE)) == wc.GRID_CHUNKS
    assert wc.BIG_DENSE[1:] == (5, 0, 1025, 1)
    n = sum(wc.ROTATION_SIZES)
    assert len(wc.ROTATION_SIZES) == 300 > wc.dense_grid(n) > 1 and wc.dense_chunks(wc.ROTATION_SIZES) > wc.dense_grid(n)
    assert wc.dense_grid(0) == 1


def test_dense_cases():
    for sizes, none in ((wc.BIG_DENSE, (4,)), (wc.ROTATION_SIZES, ())):
        c = wc.dense_case(sizes, 1, none)
        assert len(c["p"]) == sum(sizes) and (c["starts"] % 4 != 0).any()
        assert np.array_equal(c["g"], np.round(c["g"] * 64) / 64) and np.abs(c["g"]).max() <= 0.125
