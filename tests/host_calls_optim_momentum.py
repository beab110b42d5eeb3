"""The Keras SGD / RMSprop entry points (fil_momopt_multi / fil_embed_momopt_runs / fil_embed_momopt_sweep / fil_embed_momopt_merged and
their _lrdev twins) driven through their argument checks WITHOUT a GPU (every call returns before its first launch).  Run in-process
by tests/test_optim_momentum_host.py and, as a script, against the AddressSanitizer + UBSan build of the same sources:

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_optim_momentum.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

SGD, RMSPROP = _lib.FIL_OPT_SGD, _lib.FIL_OPT_RMSPROP
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

    keep = []

    def hyper(**kw):
        vals = dict(lr=1e-3, epsilon=1e-7, rho=0.9, momentum=0.0, flags=0, reserved=0)
        vals.update(kw)
        h = _lib.MomoptHyper(**vals)
        keep.append(h)
        return ctypes.addressof(h)

    H = hyper()                     # plain SGD / Keras' default RMSprop
    HM = hyper(momentum=0.9)        # the momentum variants
    nan = float("nan")
    bad_common = [(SGD, hyper(lr=-1.0), b"SGD hyper-parameters"), (SGD, hyper(lr=nan), b"SGD hyper-parameters"),
                  (SGD, hyper(momentum=-0.1), b"SGD hyper-parameters"), (SGD, hyper(momentum=1.5), b"SGD hyper-parameters"),
                  (SGD, hyper(momentum=nan), b"SGD hyper-parameters"), (SGD, hyper(flags=2), b"flags 2"),
                  (SGD, hyper(reserved=1), b"reserved 1"),
                  (RMSPROP, hyper(lr=-1.0), b"RMSprop hyper-parameters"), (RMSPROP, hyper(epsilon=-1e-7), b"RMSprop hyper-parameters"),
                  (RMSPROP, hyper(rho=-0.1), b"RMSprop hyper-parameters"), (RMSPROP, hyper(rho=1.5), b"RMSprop hyper-parameters"),
                  (RMSPROP, hyper(rho=nan), b"RMSprop hyper-parameters"), (RMSPROP, hyper(momentum=2.0), b"RMSprop hyper-parameters"),
                  (RMSPROP, hyper(flags=_lib.FIL_MOMOPT_NESTEROV), b"RMSprop hyper-parameters"),
                  (0, H, b"rule 0"), (1, H, b"rule 1"), (2, H, b"rule 2"), (5, H, b"rule 5"), (SGD, None, b"hyper is NULL"),
                  (RMSPROP, None, b"hyper is NULL")]

    def twins(name, call):
        """call(fn, extra) for the by-value entry point and its _lrdev twin (extra: the lr_dev argument, a tuple); the twin with a
        NULL lr_dev is an argument error of its own."""
        call(getattr(lib, name), ())
        call(getattr(lib, name + "_lrdev"), (FAKE,))

    # ---- fil_momopt_multi
    def multi_cases(fn, lr_dev):
        def multi(tensors=FAKE, n_=1, total=1, step=FAKE, rule=SGD, h=H, advance=1):
            return fn(tensors, n_, total, step, rule, h, *lr_dev, advance, None)
        expect(multi(n_=-1), ARG, b"bad argument")
        expect(multi(total=-5), ARG, b"bad argument")
        expect(multi(step=None), ARG, b"bad argument")
        expect(multi(tensors=None), ARG, b"bad argument")
        expect(multi(advance=2), ARG, b"advance 2")
        for rule, h, needle in bad_common:
            expect(multi(rule=rule, h=h), ARG, needle)
        expect(multi(tensors=None, n_=0, total=0, advance=0), 0)          # nothing to update, nothing to advance: no launch
        expect(multi(tensors=None, n_=0, total=0, advance=0, rule=RMSPROP, h=HM), 0)
        expect(multi(tensors=None, n_=0, total=0, advance=0, rule=SGD, h=hyper(momentum=1.0, flags=_lib.FIL_MOMOPT_NESTEROV)), 0)
    twins("fil_momopt_multi", multi_cases)
    expect(lib.fil_momopt_multi_lrdev(FAKE, 1, 1, FAKE, SGD, H, None, 1, None), ARG, b"lr_dev is NULL")

    # ---- fil_embed_momopt_runs
    def runs_cases(fn, lr_dev):
        def runs(g=FAKE, R=8, K=16, g_dtype=_lib.FIL_F32, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, step=FAKE, rule=RMSPROP, h=HM):
            return fn(g, FAKE, FAKE, R, K, g_dtype, F, None, table, slot0, slot1, None, step, rule, h, *lr_dev, None)
        expect(runs(R=-1), ARG, b"bad argument")
        expect(runs(K=0), ARG, b"bad argument")
        expect(runs(F=0), ARG, b"bad argument")
        expect(runs(g_dtype=7), ARG, b"g_dtype 7")
        expect(runs(K=257), UNSUPPORTED, b"K=257")
        for rule, h, needle in bad_common:
            expect(runs(rule=rule, h=h), ARG, needle)
        expect(runs(R=0), 0)
        expect(runs(R=0, rule=SGD, h=H, slot0=None, slot1=None), 0)
        expect(runs(g=None), ARG, b"bad argument")
        expect(runs(table=None), ARG, b"bad argument")
        expect(runs(step=None), ARG, b"bad argument")
        expect(runs(slot0=None), ARG, b"first slot")
        expect(runs(slot1=None), ARG, b"momentum slot")
        expect(runs(rule=SGD, h=HM, slot0=None), ARG, b"first slot")
        expect(runs(rule=RMSPROP, h=H, slot0=None), ARG, b"first slot")
        expect(runs(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")
    twins("fil_embed_momopt_runs", runs_cases)
    expect(lib.fil_embed_momopt_runs_lrdev(FAKE, FAKE, FAKE, 8, 16, 0, 2, None, FAKE, FAKE, FAKE, None, FAKE, SGD, H, None, None), ARG,
           b"lr_dev is NULL")

    # ---- fil_embed_momopt_sweep
    def sweep_cases(fn, lr_dev):
        def sweep(V=100, K=16, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, stamp=FAKE, offsets=FAKE, field_l2=FAKE, step=FAKE, rule=RMSPROP,
                  h=HM):
            return fn(table, slot0, slot1, stamp, V, K, offsets, field_l2, None, F, step, rule, h, *lr_dev, None)
        expect(sweep(V=-1), ARG, b"bad argument")
        expect(sweep(K=0), ARG, b"bad argument")
        expect(sweep(F=0), ARG, b"bad argument")
        expect(sweep(F=1025), UNSUPPORTED, b"F=1025")
        for rule, h, needle in bad_common:
            expect(sweep(rule=rule, h=h), ARG, needle)
        expect(sweep(V=0), 0)
        # a row-local variant without a regularised field: nothing moves, no launch, no pointer looked at
        expect(sweep(field_l2=None, stamp=None, table=None), 0)
        expect(sweep(field_l2=None, stamp=None, table=None, rule=SGD, h=H), 0)
        expect(sweep(field_l2=None, stamp=None, table=None, rule=SGD, h=HM), 0)
        # RMSprop with momentum == 0 sweeps every table: without field_l2 it still needs its arrays
        expect(sweep(field_l2=None, rule=RMSPROP, h=H, table=None), ARG, b"bad argument")
        expect(sweep(field_l2=None, rule=RMSPROP, h=H, stamp=None), ARG, b"bad argument")
        expect(sweep(field_l2=None, rule=RMSPROP, h=H, slot0=None), ARG, b"first slot")
        expect(sweep(table=None), ARG, b"bad argument")
        expect(sweep(stamp=None), ARG, b"bad argument")
        expect(sweep(offsets=None), ARG, b"bad argument")
        expect(sweep(step=None), ARG, b"bad argument")
        expect(sweep(slot0=None), ARG, b"first slot")
        expect(sweep(slot1=None), ARG, b"momentum slot")
    twins("fil_embed_momopt_sweep", sweep_cases)
    expect(lib.fil_embed_momopt_sweep_lrdev(FAKE, FAKE, FAKE, FAKE, 100, 16, FAKE, FAKE, None, 2, FAKE, SGD, H, None, None), ARG,
           b"lr_dev is NULL")

    # ---- fil_embed_momopt_merged
    def merged_cases(fn, lr_dev):
        def merged(ids=FAKE, W=2, cap=64, K=16, F=2, V=100, table=FAKE, slot0=FAKE, slot1=FAKE, step=FAKE, rule=RMSPROP, h=HM):
            return fn(ids, FAKE, FAKE, W, cap, K, FAKE, None, F, table, slot0, slot1, None, V, step, rule, h, *lr_dev, None)
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
        expect(merged(slot0=None), ARG, b"first slot")
        expect(merged(slot1=None), ARG, b"momentum slot")
        expect(merged(slot0=None, slot1=None, rule=SGD, h=H, cap=0), 0)
    twins("fil_embed_momopt_merged", merged_cases)
    expect(lib.fil_embed_momopt_merged_lrdev(FAKE, FAKE, FAKE, 2, 64, 16, FAKE, None, 2, FAKE, FAKE, FAKE, None, 100, FAKE, SGD, H, None,
                                             None), ARG, b"lr_dev is NULL")
    return n


if __name__ == "__main__":
    print("optim momentum host calls ok:", run(bind(sys.argv[1])))
