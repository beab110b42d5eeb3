"""The host plumbing that every autograd Function of functional.py shares (_save / _saved, _grad, _partials_scratch), on CPU tensors:
no GPU and no library load."""
import pytest
import torch

from ml_function_amd import _lib
from ml_function_amd import functional as Fn

SEEN = []


class _Toy(torch.autograd.Function):
    """x is always there; a (first place), b (a middle place) and c (the last place) may be None."""

    @staticmethod
    def forward(ctx, x, a, b, c):
        Fn._save(ctx, a, x, b, c)
        return x * 2.0

    @staticmethod
    def backward(ctx, g):
        SEEN.append(Fn._saved(ctx))
        return g * 2.0, None, None, None


PATTERNS = {"first": (0,), "middle": (1,), "last": (2,), "all": (0, 1, 2), "none": ()}


def _inputs(missing):
    x = torch.arange(4.0, requires_grad=True)
    abc = [None if i in missing else torch.full((3,), float(i + 1)) for i in range(3)]
    return x, abc


@pytest.mark.parametrize("missing", PATTERNS.values(), ids=PATTERNS.keys())
def test_saved_restores_the_places_of_the_missing_tensors(missing):
    x, (a, b, c) = _inputs(missing)
    del SEEN[:]
    _Toy.apply(x, a, b, c).sum().backward()
    (got,) = SEEN
    assert len(got) == 4
    for g, want in zip(got, (a, x, b, c)):
        assert g is want
    assert torch.equal(x.grad, torch.full((4,), 2.0))


@pytest.mark.parametrize("missing", PATTERNS.values(), ids=PATTERNS.keys())
def test_an_in_place_edit_of_a_saved_tensor_still_trips_the_version_check(missing):
    x, (a, b, c) = _inputs(missing)
    out = _Toy.apply(x, a, b, c).sum()
    edited = next((t for t in (c, b, a) if t is not None), None)
    if edited is None:
        with torch.no_grad():
            x.add_(1.0)
    else:
        edited.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward()


def test_an_unwanted_gradient_is_none_and_a_wanted_one_is_fp32_of_the_shape():
    assert Fn._grad(False, (2, 3), "cpu") is None
    g = Fn._grad(True, (2, 3), "cpu")
    assert g.shape == (2, 3) and g.dtype == torch.float32 and g.device.type == "cpu"


def test_an_empty_batch_zeroes_the_parameter_gradients_and_a_batch_leaves_them():
    nan = lambda: torch.full((2, 3), float("nan"))
    a, b = nan(), nan()
    assert Fn._no_samples(0, a, None, b) is True
    assert not a.view(torch.int32).any() and not b.view(torch.int32).any()
    c = nan()
    assert Fn._no_samples(1, c, None) is False and bool(torch.isnan(c).all())
    assert Fn._no_samples(0) is True and Fn._no_samples(0, None) is True


def test_no_partials_workspace_without_a_wanted_parameter_gradient(monkeypatch):
    def load():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(Fn, "_scratch", lambda *a: load())
    assert Fn._partials_scratch("fil_gru_bwd_workspace_bytes", "gru_bwd", False, "cpu", 4, 5, 8, 8) == (None, 0)
    with pytest.raises(AssertionError):
        Fn._partials_scratch("fil_gru_bwd_workspace_bytes", "gru_bwd", True, "cpu", 4, 5, 8, 8)


def test_saved_floats_holds_the_bytes_asked_for_and_at_least_256():
    assert Fn._saved_floats(0, "cpu").numel() == 64
    t = Fn._saved_floats(4096, "cpu")
    assert t.numel() == 1024 and t.dtype == torch.float32
