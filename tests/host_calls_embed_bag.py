"""The pooled-field entry points (include/fil.h N3: fil_embed_bag_fwd / _row_ids / _bwd_prep) driven through their argument
validation WITHOUT a GPU: every call returns before the first launch.  Run in-process by tests/test_embed_bag_host.py."""
import ctypes

from ml_function_amd import _lib

ARG, UNSUPPORTED = -1, -4


def run(lib):
    n = 0

    def expect(rc, want, needle=None):
        nonlocal n
        n += 1
        assert rc == want, (n, rc, want, lib.fil_last_error())
        if needle is not None:
            assert needle in lib.fil_last_error(), (n, lib.fil_last_error())

    one = ctypes.c_void_p(8)   # (never dereferenced: every check below fails, or the batch is empty, before a launch)
    fwd = lambda B, F, T, K, comb, p=None, pad=0: lib.fil_embed_bag_fwd(p, p, None, p, pad, p, p, None, B, F, T, K, comb, None)
    ids = lambda B, F, T, p=None: lib.fil_embed_bag_row_ids(p, None, None, p, 0, p, B, F, T, None)
    prep = lambda B, F, T, K, comb, g=None, gs=None, pm=None: lib.fil_embed_bag_bwd_prep(g, g, pm, gs, pm, B, F, T, K, comb, None)

    # forward
    expect(fwd(4, 3, 5, 8, _lib.FIL_BAG_MEAN), ARG, b"bad argument")            # NULL tensors
    expect(fwd(0, 3, 5, 8, _lib.FIL_BAG_MEAN), 0)                               # empty batch: nothing is looked at
    expect(fwd(0, 3, 5, 8, _lib.FIL_BAG_SUM, pad=_lib.FIL_BAG_NO_PAD), 0)
    for B, F, T, K in ((-1, 3, 5, 8), (4, 0, 5, 8), (4, 3, 0, 8), (4, 3, 5, 0), (4, -3, 5, 8)):
        expect(fwd(B, F, T, K, _lib.FIL_BAG_SUM, one), ARG, b"bad argument")
    expect(fwd(4, 3, 5, 257, _lib.FIL_BAG_SQRTN, one), UNSUPPORTED, b"256")
    expect(fwd(4, 3, 5, 256, _lib.FIL_BAG_SQRTN), ARG)                          # K = 256 is in: the NULL check is next
    expect(fwd(1 << 20, 64, 32, 8, _lib.FIL_BAG_MEAN, one), UNSUPPORTED, b"2^31")   # B F T = 2^31
    expect(fwd(4, 3, 5, 8, 3, one), ARG, b"combiner")
    expect(fwd(4, 3, 5, 8, -1, one), ARG, b"combiner")
    expect(lib.fil_embed_bag_fwd(one, one, None, one, 0, one, None, None, 4, 3, 5, 8, 1, None), ARG)   # count is not optional
    # row ids
    expect(ids(4, 3, 5), ARG, b"bad argument")
    expect(ids(0, 3, 5), 0)
    expect(ids(4, 3, 0, one), ARG)
    expect(ids(4, 0, 5, one), ARG)
    expect(ids(1 << 20, 64, 32, one), UNSUPPORTED, b"2^31")
    # backward preparation
    expect(prep(4, 3, 5, 8, _lib.FIL_BAG_MEAN), ARG, b"bad argument")
    expect(prep(0, 3, 5, 8, _lib.FIL_BAG_MEAN), 0)
    expect(prep(4, 3, 5, 257, _lib.FIL_BAG_MEAN, one, one, one), UNSUPPORTED, b"256")
    expect(prep(4, 3, 5, 8, 7, one, one, one), ARG, b"combiner")
    expect(prep(4, 3, 5, 8, _lib.FIL_BAG_MEAN, None, one, one), ARG)            # mean needs g and count
    expect(prep(4, 3, 5, 8, _lib.FIL_BAG_SQRTN, one, None, one), ARG)           # ... and somewhere to put the divided rows
    expect(prep(4, 3, 5, 8, _lib.FIL_BAG_SUM, one, one, one), ARG, b"gs")       # sum: no divided copy
    expect(prep(4, 3, 0, 8, _lib.FIL_BAG_SUM, None, None, one), ARG)
    expect(prep(1 << 20, 64, 32, 8, _lib.FIL_BAG_SUM, None, None, one), UNSUPPORTED, b"2^31")
    assert len(lib.fil_last_error()) < 512
    return n
