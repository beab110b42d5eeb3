"""Host-only checks of the pooled multi-valued fields (include/fil.h N3, functional.embed_bag, layers.BagEmbed,
models.FeatureInput(seqInfo=...)): the entry points in the header, the binding and the library; their argument validation through
ctypes; the Python surface that needs no GPU; and self-checks of the numpy restatement (tests/embed_bag_ref.py) the GPU tests are
held to."""
import inspect

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, layers, models
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FilError
from tests import embed_bag_ref as ref

NEW = ("fil_embed_bag_fwd", "fil_embed_bag_row_ids", "fil_embed_bag_bwd_prep")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_bag_entry_points_are_in_header_signatures_and_library(lib):
    for name in NEW:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert _lib.header_abi_version() == 216 and lib.fil_version() == 216            # entry points added only
    header = open(_lib.HEADER_PATH).read()
    for macro in ("FIL_BAG_SUM", "FIL_BAG_MEAN", "FIL_BAG_SQRTN"):
        assert "#define %s %d\n" % (macro, getattr(_lib, macro)) in header, macro
    assert "#define FIL_BAG_NO_PAD INT64_MIN\n" in header and _lib.FIL_BAG_NO_PAD == np.iinfo(np.int64).min
    assert "#define FIL_BAG_MAX_BLOCKS %d\n" % _lib.FIL_BAG_MAX_BLOCKS in header
    assert (_lib.FIL_BAG_SUM, _lib.FIL_BAG_MEAN, _lib.FIL_BAG_SQRTN) == (0, 1, 2)
    assert Fn.BAG_COMBINERS == {"sum": 0, "mean": 1, "sqrtn": 2} and tuple(Fn.BAG_COMBINERS) == ref.COMBINERS
    # fil_embed_bag_fwd's arguments in the documented order: the four N1 tensors, pad_id, out, count, oob_count, B F T K, combiner, stream
    P, I, L = _lib._P, _lib._I, _lib._c.c_int64
    assert _lib.SIGNATURES["fil_embed_bag_fwd"] == (I, [P, P, P, P, L, P, P, P, I, I, I, I, I, P])


def test_bag_entry_points_validate(lib):
    from tests import host_calls_embed_bag
    assert host_calls_embed_bag.run(lib) >= 25


def _sig(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_constructor_surface_and_defaults():
    assert layers.BagEmbed is layers.interactive_layer.BagEmbed and "BagEmbed" in layers.__all__
    assert issubclass(layers.BagEmbed, layers.SparseEmbed) and layers.BagEmbed.build is layers.SparseEmbed.build
    s = _sig(layers.BagEmbed.__init__)
    assert list(s) == ["sparse_info", "combiner", "padding_id", "is_linear", "use_flatten", "seed", "packed", "check_ids", "sparse_grad",
                       "grad_mode"]
    assert {k: v for k, v in s.items() if k != "sparse_info"} == dict(
        combiner="mean", padding_id=0, is_linear=False, use_flatten=False, seed=2020, packed=False, check_ids=None, sparse_grad=False,
        grad_mode="dense")
    e = _sig(Fn.embed_bag)
    assert list(e) == ["table", "offsets", "idx", "sizes", "combiner", "padding_id", "frozen", "sparse_grad", "oob_count", "runs_grad"]
    assert (e["sizes"], e["combiner"], e["padding_id"], e["frozen"], e["sparse_grad"], e["oob_count"], e["runs_grad"]) == (
        None, "mean", 0, None, False, None, None)
    f = _sig(models.FeatureInput.__init__)
    assert f["seqInfo"] is None and f["seqCombiner"] == "mean" and f["tableGrad"] == "dense"
    assert list(inspect.signature(models.CTRModel.forward).parameters) == ["self", "dense", "sparse_idx", "seq_idx"]
    assert _sig(models.CTRModel.forward)["seq_idx"] is None

    info = models.make_seq_info([5, 7], 4, embed_dim=6)
    assert [(i.fea_name, i.word_size, i.cross_unit, i.linear_unit, i.mask_zero, i.input_length) for i in info] == [
        ("S1", 5, 6, 1, True, 4), ("S2", 7, 6, 1, True, 4)]
    one = models.make_sparse_info([5, 7], embed_dim=6)
    assert [(i.mask_zero, i.input_length) for i in one] == [(False, 1)] * 2          # make_sparse_info is as it was
    assert info[0]._replace(fea_name="C1", mask_zero=False, input_length=1) == one[0]

    bag = layers.BagEmbed(info)
    assert (bag.combiner, bag.padding_id, bag.grad_mode, bag.use_add, bag.emit_xt, bag.out_dtype) == ("mean", 0, "dense", False, False, None)
    assert layers.BagEmbed(info, combiner="sqrtn", padding_id=None, grad_mode="runs").padding_id is None

    # the defaults keep the one-id FeatureInput exactly; seqInfo adds the two bag layers (the linear one only with useLinear)
    fi = models.FeatureInput(sparseInfo=one, useLinear=True)
    assert fi.seq_embed is None and fi.seq_linear_embed is None and fi.seq_info == []
    fs = models.FeatureInput(sparseInfo=one, seqInfo=info, seqCombiner="sum", useLinear=True, tableGrad="runs")
    assert isinstance(fs.seq_embed, layers.BagEmbed) and (fs.seq_embed.combiner, fs.seq_embed.grad_mode) == ("sum", "runs")
    assert fs.seq_linear_embed.is_linear and fs.seq_linear_embed.grad_mode == "runs" and not fs.seq_embed.is_linear
    assert models.FeatureInput(sparseInfo=one, seqInfo=info).seq_linear_embed is None


def test_constructor_errors():
    info = models.make_seq_info([5, 7], 4)
    with pytest.raises(ValueError, match="combiner"):
        layers.BagEmbed(info, combiner="max")
    with pytest.raises(ValueError, match="grad_mode"):
        layers.BagEmbed(info, grad_mode="atomic")
    with pytest.raises(ValueError, match="exclude"):
        layers.BagEmbed(info, grad_mode="runs", sparse_grad=True)
    with pytest.raises(ValueError, match="padding_id"):
        layers.BagEmbed(info, padding_id=0.5)
    with pytest.raises(ValueError, match="emitXT"):
        models.FeatureInput(sparseInfo=models.make_sparse_info([5]), seqInfo=info, emitXT=True)
    with pytest.raises(ValueError, match="combiner"):
        models.FeatureInput(seqInfo=info, seqCombiner="max")
    with pytest.raises(ValueError, match="combiner"):
        Fn.embed_bag(torch.zeros(12, 4), torch.tensor([0, 5]), torch.zeros(2, 2, 3, dtype=torch.int64), combiner="max")


def test_no_cpu_fallback():
    info = models.make_seq_info([5, 7], 3, embed_dim=4)
    idx = torch.zeros(2, 2, 3, dtype=torch.int64)
    with pytest.raises(FilError, match="GPU only"):
        Fn.embed_bag(torch.zeros(12, 4), torch.tensor([0, 5]), idx)
    with pytest.raises(FilError, match="GPU only"):
        layers.BagEmbed(info)(idx)
    with pytest.raises(FilError, match="GPU only"):
        layers.BagEmbed(info)([idx[:, 0], idx[:, 1]])
    with pytest.raises(ValueError, match=r"\[B, 2, T\]"):
        layers.BagEmbed(info)(idx[:, :1])
    fi = models.FeatureInput(sparseInfo=models.make_sparse_info([5], embed_dim=4), seqInfo=info)
    with pytest.raises(ValueError, match="seq_idx"):
        fi((None, torch.zeros(2, 1, dtype=torch.int64)))
    with pytest.raises(FilError, match="GPU only"):
        models.CTRModel(fi, models.FM())(None, torch.zeros(2, 1, dtype=torch.int64), idx)


# ------------------------------------------------------------------------------------------- the reference, checked by hand
def _table():
    """Two fields of 4 and 3 rows, K = 2: row r of the concatenated table is (r, 10 r) -- sums are read off at sight."""
    t = np.stack([np.arange(7), 10 * np.arange(7)], 1).astype(f32)
    return t, np.array([0, 4]), np.array([4, 3])


def test_reference_hand_computed_bags():
    table, offsets, sizes = _table()
    idx = np.array([[[1, 0, 3, 3], [0, 0, 0, 0]],          # padding in the middle, a repeated id | an all-padding bag
                    [[2, 1, 3, 1], [2, -1, 3, 0]]])        # a full bag | the table's last row, a negative id, an id == V, padding
    out, count, oob = ref.forward(table, offsets, sizes, idx, "sum")
    assert count.tolist() == [[3, 0], [4, 1]] and oob == 2
    assert out.tolist() == [[[7, 70], [0, 0]], [[7, 70], [6, 60]]]
    mean, _, _ = ref.forward(table, offsets, sizes, idx, "mean")
    assert np.array_equal(mean, np.array([[[7, 70], [0, 0]], [[7, 70], [6, 60]]], f32) / np.array([[3, 1], [4, 1]], f32)[:, :, None])
    sq, _, _ = ref.forward(table, offsets, sizes, idx, "sqrtn")
    assert np.array_equal(sq[1, 0], np.array([3.5, 35], f32)) and np.array_equal(sq[0, 0], np.array([7, 70], f32) / np.sqrt(f32(3)))
    # without a padding id, id 0 is row 0 of its field
    out0, count0, oob0 = ref.forward(table, offsets, sizes, idx, "sum", padding_id=None)
    assert count0.tolist() == [[4, 4], [4, 2]] and oob0 == 2
    assert out0.tolist() == [[[7, 70], [16, 160]], [[7, 70], [10, 100]]]
    # the gradient: every live slot receives its bag's row, once per occurrence; padding, bad ids and frozen fields nothing
    g = np.array([[[1, 2], [4, 8]], [[16, 32], [64, 128]]], np.int64)
    want, touched = ref.table_grad(7, offsets, sizes, idx, g, dtype=np.int64)
    assert want.tolist() == [[0, 0], [1 + 32, 2 + 64], [16, 32], [2 + 16, 4 + 32], [0, 0], [0, 0], [64, 128]]
    assert touched.tolist() == [False, True, True, True, False, False, True]
    frz, t2 = ref.table_grad(7, offsets, sizes, idx, g, frozen=[0, 1], dtype=np.int64)
    assert np.array_equal(frz[:4], want[:4]) and not frz[4:].any() and not t2[4:].any()
    gs = ref.scaled_grad(g, count, "mean")
    assert gs.dtype == f32 and np.array_equal(gs[0, 0], np.array([1, 2], f32) / f32(3)) and not gs[0, 1].any()
    assert np.array_equal(ref.scaled_grad(g, count, "sum"), g.astype(f32))


def test_reference_single_slot_bag_is_a_plain_lookup():
    rng = np.random.default_rng(0)
    sizes = np.array([9, 5, 7])
    offsets = np.array([0, 9, 14])
    table = rng.standard_normal((21, 5)).astype(f32)
    idx = np.stack([rng.integers(0, v, 11) for v in sizes], 1)[:, :, None]
    for combiner in ref.COMBINERS:
        out, count, oob = ref.forward(table, offsets, sizes, idx, combiner, padding_id=None)
        assert np.array_equal(out, table[idx[:, :, 0] + offsets]) and (count == 1).all() and oob == 0


def test_reference_mean_of_equal_rows_is_that_row():
    rng = np.random.default_rng(1)
    # rows of eighths in [-8, 8): every partial sum j x (j <= 19) is exact in fp32, and (n x) / n is then exactly x
    table = (rng.integers(-64, 64, (6, 8)) / 8).astype(f32)
    for n in (1, 2, 3, 7, 16, 19):
        idx = np.full((1, 1, 19), 0, np.int64)
        idx[0, 0, 19 - n:] = 5
        out, count, _ = ref.forward(table, [0], [6], idx, "mean")
        assert count[0, 0] == n and np.array_equal(out[0, 0], table[5])
    table = rng.standard_normal((6, 8)).astype(f32)          # any rows: within one rounding per addition and one for the division
    out, _, _ = ref.forward(table, [0], [6], np.full((1, 1, 7), 2, np.int64), "mean")
    assert np.allclose(out[0, 0], table[2], rtol=8 * np.finfo(f32).eps, atol=0)


def test_reference_expanded_form():
    table, offsets, sizes = _table()
    idx = np.array([[[1, 0, 3], [2, 0, 0]]])
    gs = np.array([[[1, 2], [3, 4]]], f32)
    e = ref.expanded(offsets, sizes, idx, gs, frozen=[0, 1], field_l2=[0.5, 0.0])
    assert e["ids"].tolist() == [[1, -1, 3, 2, -1, -1]]
    assert e["offsets"].tolist() == [0, 0, 0, 4, 4, 4] and e["sizes"].tolist() == [4, 4, 4, 3, 3, 3]
    assert e["frozen"].tolist() == [0, 0, 0, 1, 1, 1] and e["field_l2"].tolist() == [0.5, 0.5, 0.5, 0, 0, 0]
    assert e["g"].shape == (1, 6, 2) and e["g"][0].tolist() == [[1, 2]] * 3 + [[3, 4]] * 3
    assert ref.expanded(offsets, sizes, idx, None, padding_id=None)["ids"].tolist() == [[1, 0, 3, 2, 0, 0]]
