"""The Keras-Adam entry points (fil_adam_multi / fil_embed_adam_runs / fil_embed_adam_sweep) driven through their argument checks
WITHOUT a GPU (every call returns before its first launch).  Run in-process by tests/test_optim_host.py and, as a script, against the
AddressSanitizer + UBSan build of the same sources (as tests/host_calls.py):

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_optim.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

KERAS, LAZY = _lib.FIL_ADAM_KERAS, _lib.FIL_ADAM_LAZY
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

    H = (1e-3, 0.9, 0.999, 1e-7)

    def multi(tensors=FAKE, n_=1, total=1, step=FAKE, hyper=H, advance=1):
        return lib.fil_adam_multi(tensors, n_, total, step, *hyper, advance, None)

    # fil_adam_multi
    expect(multi(n_=-1), ARG, b"bad argument")
    expect(multi(total=-5), ARG, b"bad argument")
    expect(multi(step=None), ARG, b"bad argument")
    expect(multi(tensors=None), ARG, b"bad argument")
    expect(multi(advance=2), ARG, b"advance 2")
    expect(multi(advance=-1), ARG, b"advance")
    for bad in ((-1e-3, 0.9, 0.999, 1e-7), (1e-3, 1.0, 0.999, 1e-7), (1e-3, 0.9, -0.5, 1e-7), (1e-3, 0.9, 0.999, -1.0),
                (float("nan"), 0.9, 0.999, 1e-7)):
        expect(multi(hyper=bad), ARG, b"hyper-parameters")
    expect(multi(tensors=None, n_=0, total=0, advance=0), 0)        # nothing to update, nothing to advance: no launch

    def runs(g=FAKE, R=8, K=16, g_dtype=_lib.FIL_F32, F=2, table=FAKE, stamp=FAKE, step=FAKE, hyper=H, mode=KERAS):
        return lib.fil_embed_adam_runs(g, FAKE, FAKE, R, K, g_dtype, F, None, table, FAKE, FAKE, stamp, step, *hyper, mode, None)

    # fil_embed_adam_runs
    expect(runs(R=-1), ARG, b"bad argument")
    expect(runs(K=0), ARG, b"bad argument")
    expect(runs(F=0), ARG, b"bad argument")
    expect(runs(g_dtype=7), ARG, b"g_dtype 7")
    expect(runs(mode=2), ARG, b"mode 2")
    expect(runs(stamp=None), ARG, b"row stamps")                      # Keras mode needs them ...
    expect(runs(stamp=None, mode=LAZY, R=0), 0)                       # ... lazy mode does not (R = 0: nothing to do)
    expect(runs(K=257), UNSUPPORTED, b"K=257")
    expect(runs(hyper=(1e-3, 0.9, 1.5, 1e-7)), ARG, b"hyper-parameters")
    expect(runs(R=0), 0)
    expect(runs(g=None), ARG, b"bad argument")
    expect(runs(table=None, mode=LAZY), ARG, b"bad argument")
    expect(runs(step=None), ARG, b"bad argument")
    expect(runs(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")

    def sweep(V=100, K=16, F=2, table=FAKE, stamp=FAKE, offsets=FAKE, step=FAKE, hyper=H):
        return lib.fil_embed_adam_sweep(table, FAKE, FAKE, stamp, V, K, offsets, None, None, F, step, *hyper, None)

    # fil_embed_adam_sweep
    expect(sweep(V=-1), ARG, b"bad argument")
    expect(sweep(K=0), ARG, b"bad argument")
    expect(sweep(F=0), ARG, b"bad argument")
    expect(sweep(F=1025), UNSUPPORTED, b"F=1025")
    expect(sweep(hyper=(1e-3, -0.1, 0.999, 1e-7)), ARG, b"hyper-parameters")
    expect(sweep(V=0), 0)
    expect(sweep(table=None), ARG, b"bad argument")
    expect(sweep(stamp=None), ARG, b"bad argument")
    expect(sweep(offsets=None), ARG, b"bad argument")
    expect(sweep(step=None), ARG, b"bad argument")
    return n


if __name__ == "__main__":
    print("optim host calls ok:", run(bind(sys.argv[1])))
