"""The Keras Adagrad / Ftrl entry points (fil_rowopt_multi / fil_embed_rowopt_runs / fil_embed_rowopt_sweep / fil_embed_rowopt_merged)
driven through their argument checks WITHOUT a GPU (every call returns before its first launch).  Run in-process by
tests/test_optim_rowwise_host.py and, as a script, against the AddressSanitizer + UBSan build of the same sources:

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_optim_rowwise.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

ADAGRAD, FTRL = _lib.FIL_OPT_ADAGRAD, _lib.FIL_OPT_FTRL
ARG, UNSUPPORTED = -1, -4
FAKE = 1 << 20      # a non-NULL "device" pointer: only ever looked at by a launch, and no call below gets that far


def bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def run(lib):
    n = 0

    def expect(rc, want, needle=None):
        nonlocal n
        n += 1
        assert rc == want, (n, rc, want, lib.fil_last_error())
        if needle is not None:
            assert needle in lib.fil_last_error(), (n, lib.fil_last_error())

    good = _lib.RowoptHyper(1e-3, 1e-7, -0.5, 0.0, 0.0, 0.0)
    H = ctypes.addressof(good)
    keep = []

    def hyper(**kw):
        vals = dict(lr=1e-3, epsilon=1e-7, lr_power=-0.5, l1=0.0, l2=0.0, l2_shrinkage=0.0)
        vals.update(kw)
        h = _lib.RowoptHyper(**vals)
        keep.append(h)
        return ctypes.addressof(h)

    bad_common = [(ADAGRAD, hyper(lr=-1.0), b"Adagrad hyper-parameters"), (ADAGRAD, hyper(epsilon=-1e-7), b"Adagrad hyper-parameters"),
                  (ADAGRAD, hyper(lr=float("nan")), b"Adagrad hyper-parameters"), (FTRL, hyper(lr_power=0.5), b"Ftrl hyper-parameters"),
                  (FTRL, hyper(l1=-1.0), b"Ftrl hyper-parameters"), (FTRL, hyper(l2=-1.0), b"Ftrl hyper-parameters"),
                  (FTRL, hyper(l2_shrinkage=-1.0), b"Ftrl hyper-parameters"), (FTRL, hyper(lr=-1.0), b"Ftrl hyper-parameters"),
                  (0, H, b"rule 0"), (3, H, b"rule 3"), (ADAGRAD, None, b"hyper is NULL")]

    def multi(tensors=FAKE, n_=1, total=1, step=FAKE, rule=ADAGRAD, h=H, advance=1):
        return lib.fil_rowopt_multi(tensors, n_, total, step, rule, h, advance, None)

    # fil_rowopt_multi
    expect(multi(n_=-1), ARG, b"bad argument")
    expect(multi(total=-5), ARG, b"bad argument")
    expect(multi(step=None), ARG, b"bad argument")
    expect(multi(tensors=None), ARG, b"bad argument")
    expect(multi(advance=2), ARG, b"advance 2")
    for rule, h, needle in bad_common:
        expect(multi(rule=rule, h=h), ARG, needle)
    expect(multi(tensors=None, n_=0, total=0, advance=0), 0)          # nothing to update, nothing to advance: no launch
    expect(multi(tensors=None, n_=0, total=0, advance=0, rule=FTRL, h=hyper(lr_power=-0.3, l1=1e-3)), 0)

    def runs(g=FAKE, R=8, K=16, g_dtype=_lib.FIL_F32, F=2, table=FAKE, accum=FAKE, linear=FAKE, step=FAKE, rule=ADAGRAD, h=H):
        return lib.fil_embed_rowopt_runs(g, FAKE, FAKE, R, K, g_dtype, F, None, table, accum, linear, None, step, rule, h, None)

    # fil_embed_rowopt_runs
    expect(runs(R=-1), ARG, b"bad argument")
    expect(runs(K=0), ARG, b"bad argument")
    expect(runs(F=0), ARG, b"bad argument")
    expect(runs(g_dtype=7), ARG, b"g_dtype 7")
    expect(runs(K=257), UNSUPPORTED, b"K=257")
    for rule, h, needle in bad_common:
        expect(runs(rule=rule, h=h), ARG, needle)
    expect(runs(R=0), 0)
    expect(runs(g=None), ARG, b"bad argument")
    expect(runs(table=None), ARG, b"bad argument")
    expect(runs(accum=None), ARG, b"bad argument")
    expect(runs(step=None), ARG, b"bad argument")
    expect(runs(rule=FTRL, linear=None), ARG, b"linear slot")
    expect(runs(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")

    def sweep(V=100, K=16, F=2, table=FAKE, accum=FAKE, linear=FAKE, stamp=FAKE, offsets=FAKE, field_l2=FAKE, step=FAKE, rule=ADAGRAD,
              h=H):
        return lib.fil_embed_rowopt_sweep(table, accum, linear, stamp, V, K, offsets, field_l2, None, F, step, rule, h, None)

    # fil_embed_rowopt_sweep
    expect(sweep(V=-1), ARG, b"bad argument")
    expect(sweep(K=0), ARG, b"bad argument")
    expect(sweep(F=0), ARG, b"bad argument")
    expect(sweep(F=1025), UNSUPPORTED, b"F=1025")
    for rule, h, needle in bad_common:
        expect(sweep(rule=rule, h=h), ARG, needle)
    expect(sweep(V=0), 0)
    expect(sweep(field_l2=None, stamp=None, table=None), 0)            # no regularised field: nothing moves, no launch
    expect(sweep(table=None), ARG, b"bad argument")
    expect(sweep(stamp=None), ARG, b"bad argument")
    expect(sweep(offsets=None), ARG, b"bad argument")
    expect(sweep(step=None), ARG, b"bad argument")
    expect(sweep(rule=FTRL, linear=None), ARG, b"linear slot")

    def merged(ids=FAKE, W=2, cap=64, K=16, F=2, V=100, table=FAKE, accum=FAKE, linear=FAKE, step=FAKE, rule=FTRL, h=H):
        return lib.fil_embed_rowopt_merged(ids, FAKE, FAKE, W, cap, K, FAKE, None, F, table, accum, linear, None, V, step, rule, h, None)

    # fil_embed_rowopt_merged
    expect(merged(W=0), ARG, b"bad argument")
    expect(merged(cap=-1), ARG, b"bad argument")
    expect(merged(K=0), ARG, b"bad argument")
    expect(merged(V=-1), ARG, b"bad argument")
    expect(merged(K=257), UNSUPPORTED, b"K=257")
    expect(merged(F=1025), UNSUPPORTED, b"F=1025")
    for rule, h, needle in bad_common:
        expect(merged(rule=rule, h=h), ARG, needle)
    expect(merged(cap=0), 0)
    expect(merged(V=0), 0)
    expect(merged(ids=None), ARG, b"bad argument")
    expect(merged(table=None), ARG, b"bad argument")
    expect(merged(step=None), ARG, b"bad argument")
    expect(merged(linear=None), ARG, b"linear slot")
    expect(merged(linear=None, rule=ADAGRAD, cap=0), 0)
    return n


if __name__ == "__main__":
    print("optim rowwise host calls ok:", run(bind(sys.argv[1])))
