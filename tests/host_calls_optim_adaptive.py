"""The Keras Adadelta / Adamax entry points (fil_adaopt_multi / fil_embed_adaopt_runs / fil_embed_adaopt_sweep / fil_embed_adaopt_merged
and their _lrdev twins) driven through their argument checks WITHOUT a GPU (every call returns before its first launch).  Run
in-process by tests/test_optim_adaptive_host.py; as a script it takes the path of a build of the library:

    python tests/host_calls_optim_adaptive.py ml_function_amd/libfil_hip.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

ADADELTA, ADAMAX = _lib.FIL_OPT_ADADELTA, _lib.FIL_OPT_ADAMAX
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
        vals = dict(lr=1e-3, rho=0.95, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
        vals.update(kw)
        h = _lib.AdaoptHyper(**vals)
        keep.append(h)
        return ctypes.addressof(h)

    H = hyper()
    nan = float("nan")
    DD, MX = b"Adadelta hyper-parameters", b"Adamax hyper-parameters"
    bad_common = [(ADADELTA, hyper(lr=-1.0), DD), (ADADELTA, hyper(lr=nan), DD), (ADADELTA, hyper(rho=-0.1), DD),
                  (ADADELTA, hyper(rho=1.5), DD), (ADADELTA, hyper(rho=nan), DD), (ADADELTA, hyper(epsilon=-1e-7), DD),
                  (ADAMAX, hyper(lr=-1.0), MX), (ADAMAX, hyper(lr=nan), MX), (ADAMAX, hyper(beta_1=-0.1), MX),
                  (ADAMAX, hyper(beta_1=1.0), MX), (ADAMAX, hyper(beta_1=nan), MX), (ADAMAX, hyper(beta_2=1.0), MX),
                  (ADAMAX, hyper(beta_2=-0.5), MX), (ADAMAX, hyper(epsilon=-1.0), MX), (ADAMAX, hyper(epsilon=nan), MX),
                  # an unknown rule: the other families' and the next free number
                  (0, H, b"rule 0"), (1, H, b"rule 1"), (2, H, b"rule 2"), (3, H, b"rule 3"), (4, H, b"rule 4"), (7, H, b"rule 7"),
                  (-1, H, b"rule -1"), (ADADELTA, None, b"hyper is NULL"), (ADAMAX, None, b"hyper is NULL")]
    # a hyper-parameter of the OTHER rule is not looked at
    ok_other = [(ADADELTA, hyper(beta_1=5.0, beta_2=-1.0)), (ADAMAX, hyper(rho=7.0)), (ADADELTA, hyper(rho=0.0)), (ADADELTA, hyper(rho=1.0)),
                (ADAMAX, hyper(beta_1=0.0, beta_2=0.0, epsilon=0.0, lr=0.0))]

    def twins(name, call):
        """call(fn, extra) for the by-value entry point and its _lrdev twin (extra: the lr_dev argument, a tuple)."""
        call(getattr(lib, name), ())
        call(getattr(lib, name + "_lrdev"), (FAKE,))

    # ---- fil_adaopt_multi
    def multi_cases(fn, lr_dev):
        def multi(tensors=FAKE, n_=1, total=1, step=FAKE, rule=ADADELTA, h=H, advance=1):
            return fn(tensors, n_, total, step, rule, h, *lr_dev, advance, None)
        expect(multi(n_=-1), ARG, b"bad argument")
        expect(multi(total=-5), ARG, b"bad argument")
        expect(multi(step=None), ARG, b"bad argument")
        expect(multi(tensors=None), ARG, b"bad argument")
        expect(multi(advance=2), ARG, b"advance 2")
        expect(multi(advance=-1, rule=ADAMAX), ARG, b"advance -1")
        for rule, h, needle in bad_common:
            expect(multi(rule=rule, h=h), ARG, needle)
        for rule, h in ok_other + [(ADADELTA, H), (ADAMAX, H)]:
            expect(multi(tensors=None, n_=0, total=0, advance=0, rule=rule, h=h), 0)    # nothing to update or advance: no launch
    twins("fil_adaopt_multi", multi_cases)
    expect(lib.fil_adaopt_multi_lrdev(FAKE, 1, 1, FAKE, ADAMAX, H, None, 1, None), ARG, b"lr_dev is NULL")

    # ---- fil_embed_adaopt_runs
    def runs_cases(fn, lr_dev):
        def runs(g=FAKE, R=8, K=16, g_dtype=_lib.FIL_F32, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, step=FAKE, rule=ADAMAX, h=H,
                 perm=FAKE, ids=FAKE):
            return fn(g, perm, ids, R, K, g_dtype, F, None, table, slot0, slot1, None, step, rule, h, *lr_dev, None)
        expect(runs(R=-1), ARG, b"bad argument")
        expect(runs(K=0), ARG, b"bad argument")
        expect(runs(F=0), ARG, b"bad argument")
        expect(runs(g_dtype=7), ARG, b"g_dtype 7")
        expect(runs(K=257), UNSUPPORTED, b"K=257")
        expect(runs(K=256, R=0), 0)
        for rule, h, needle in bad_common:
            expect(runs(rule=rule, h=h), ARG, needle)
        for rule in (ADADELTA, ADAMAX):
            # R = 0: FIL_OK without a pointer looked at
            expect(runs(R=0, rule=rule, g=None, perm=None, ids=None, table=None, slot0=None, slot1=None, step=None), 0)
            expect(runs(rule=rule, g=None), ARG, b"bad argument")
            expect(runs(rule=rule, table=None), ARG, b"bad argument")
            expect(runs(rule=rule, step=None), ARG, b"bad argument")
            expect(runs(rule=rule, slot0=None), ARG, b"first slot")
            expect(runs(rule=rule, slot1=None), ARG, b"second slot")
            expect(runs(rule=rule, slot0=None, slot1=None), ARG, b"first slot")
        expect(runs(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")
    twins("fil_embed_adaopt_runs", runs_cases)
    expect(lib.fil_embed_adaopt_runs_lrdev(FAKE, FAKE, FAKE, 8, 16, 0, 2, None, FAKE, FAKE, FAKE, None, FAKE, ADAMAX, H, None, None), ARG,
           b"lr_dev is NULL")

    # ---- fil_embed_adaopt_sweep
    def sweep_cases(fn, lr_dev):
        def sweep(V=100, K=16, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, stamp=FAKE, offsets=FAKE, field_l2=FAKE, step=FAKE, rule=ADAMAX,
                  h=H):
            return fn(table, slot0, slot1, stamp, V, K, offsets, field_l2, None, F, step, rule, h, *lr_dev, None)
        expect(sweep(V=-1), ARG, b"bad argument")
        expect(sweep(K=0), ARG, b"bad argument")
        expect(sweep(F=0), ARG, b"bad argument")
        expect(sweep(F=1025), UNSUPPORTED, b"F=1025")
        for rule, h, needle in bad_common:
            expect(sweep(rule=rule, h=h), ARG, needle)
        for rule in (ADADELTA, ADAMAX):
            # V = 0, or no regularised field (both rules are row-local): FIL_OK, no launch, no pointer looked at
            expect(sweep(rule=rule, V=0, table=None, slot0=None, slot1=None, stamp=None, offsets=None, step=None), 0)
            expect(sweep(rule=rule, field_l2=None, table=None, slot0=None, slot1=None, stamp=None, offsets=None, step=None), 0)
            expect(sweep(rule=rule, table=None), ARG, b"bad argument")
            expect(sweep(rule=rule, stamp=None), ARG, b"bad argument")
            expect(sweep(rule=rule, offsets=None), ARG, b"bad argument")
            expect(sweep(rule=rule, step=None), ARG, b"bad argument")
            expect(sweep(rule=rule, slot0=None), ARG, b"first slot")
            expect(sweep(rule=rule, slot1=None), ARG, b"second slot")
    twins("fil_embed_adaopt_sweep", sweep_cases)
    expect(lib.fil_embed_adaopt_sweep_lrdev(FAKE, FAKE, FAKE, FAKE, 100, 16, FAKE, FAKE, None, 2, FAKE, ADADELTA, H, None, None), ARG,
           b"lr_dev is NULL")

    # ---- fil_embed_adaopt_merged
    def merged_cases(fn, lr_dev):
        def merged(ids=FAKE, values=FAKE, counts=FAKE, W=2, cap=64, K=16, F=2, V=100, offsets=FAKE, table=FAKE, slot0=FAKE, slot1=FAKE,
                   step=FAKE, rule=ADADELTA, h=H):
            return fn(ids, values, counts, W, cap, K, offsets, None, F, table, slot0, slot1, None, V, step, rule, h, *lr_dev, None)
        expect(merged(W=0), ARG, b"bad argument")
        expect(merged(cap=-1), ARG, b"bad argument")
        expect(merged(K=0), ARG, b"bad argument")
        expect(merged(V=-1), ARG, b"bad argument")
        expect(merged(K=257), UNSUPPORTED, b"K=257")
        expect(merged(F=1025), UNSUPPORTED, b"F=1025")
        for rule, h, needle in bad_common:
            expect(merged(rule=rule, h=h), ARG, needle)
        for rule in (ADADELTA, ADAMAX):
            none = dict(ids=None, values=None, counts=None, offsets=None, table=None, slot0=None, slot1=None, step=None)
            expect(merged(rule=rule, cap=0, **none), 0)
            expect(merged(rule=rule, V=0, **none), 0)
            expect(merged(rule=rule, ids=None), ARG, b"bad argument")
            expect(merged(rule=rule, table=None), ARG, b"bad argument")
            expect(merged(rule=rule, step=None), ARG, b"bad argument")
            expect(merged(rule=rule, slot0=None), ARG, b"first slot")
            expect(merged(rule=rule, slot1=None), ARG, b"second slot")
    twins("fil_embed_adaopt_merged", merged_cases)
    expect(lib.fil_embed_adaopt_merged_lrdev(FAKE, FAKE, FAKE, 2, 64, 16, FAKE, None, 2, FAKE, FAKE, FAKE, None, 100, FAKE, ADAMAX, H, None,
                                             None), ARG, b"lr_dev is NULL")
    return n


if __name__ == "__main__":
    print("optim adaptive host calls ok:", run(bind(sys.argv[1])))
