"""The deferred Keras-Adam entry points (fil_embed_adam_ring_len / fil_embed_adam_catchup_runs / fil_embed_adam_runs_deferred /
fil_embed_adam_merged_deferred / fil_embed_adam_roll) driven through their argument checks WITHOUT a GPU (every call returns before
its first launch).  Run in-process by tests/test_optim_deferred_host.py and, as a script, against the AddressSanitizer + UBSan build
of the same sources (as tests/host_calls_optim.py):

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_optim_deferred.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

ARG, UNSUPPORTED = -1, -4
FAKE = 1 << 20      # a non-NULL, 16-byte aligned "device" pointer: only ever looked at by a launch, and no call below gets that far
STEP, SKIP, FLUSH = _lib.FIL_ADAM_ROLL_STEP, _lib.FIL_ADAM_ROLL_SKIP, _lib.FIL_ADAM_ROLL_FLUSH


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
    # the ring: the power of two >= N + 1, for N in 1 ... 1023
    for N, D in ((1, 2), (2, 4), (3, 4), (4, 8), (5, 8), (7, 8), (8, 16), (16, 32), (512, 1024), (1023, 1024)):
        assert lib.fil_embed_adam_ring_len(N) == D, (N, D)
    for N in (0, -1, 1024, 1 << 20):
        assert lib.fil_embed_adam_ring_len(N) == 0, N

    def catchup(ids=FAKE, R=64, K=16, table=FAKE, stamp=FAKE, ring=FAKE, N=8, offsets=FAKE, F=3, V=100, step=FAKE):
        return lib.fil_embed_adam_catchup_runs(ids, R, K, table, FAKE, FAKE, stamp, ring, N, offsets, None, None, F, V, step, None)

    expect(catchup(R=-1), ARG, b"bad argument")
    expect(catchup(K=0), ARG, b"bad argument")
    expect(catchup(F=0), ARG, b"bad argument")
    expect(catchup(V=-1), ARG, b"bad argument")
    expect(catchup(K=257), UNSUPPORTED, b"K=257")
    expect(catchup(F=1025), UNSUPPORTED, b"F=1025")
    expect(catchup(N=0), ARG, b"sweep_period 0")
    expect(catchup(N=1024), ARG, b"sweep_period 1024")
    expect(catchup(ring=FAKE + 4), ARG, b"16-byte aligned")
    expect(catchup(R=0), 0)
    expect(catchup(V=0), 0)
    expect(catchup(ids=None), ARG, b"bad argument")
    expect(catchup(table=None), ARG, b"bad argument")
    expect(catchup(stamp=None), ARG, b"bad argument")
    expect(catchup(ring=None), ARG, b"bad argument")
    expect(catchup(offsets=None), ARG, b"bad argument")
    expect(catchup(step=None), ARG, b"bad argument")

    def runs(g=FAKE, R=64, K=16, g_dtype=_lib.FIL_F32, F=3, offsets=FAKE, table=FAKE, stamp=FAKE, ring=FAKE, N=8, V=100, step=FAKE,
             hyper=H):
        return lib.fil_embed_adam_runs_deferred(g, FAKE, FAKE, R, K, g_dtype, F, offsets, None, None, table, FAKE, FAKE, stamp, ring, N,
                                                V, step, *hyper, None)

    expect(runs(R=-1), ARG, b"bad argument")
    expect(runs(K=0), ARG, b"bad argument")
    expect(runs(F=0), ARG, b"bad argument")
    expect(runs(g_dtype=7), ARG, b"g_dtype 7")
    expect(runs(K=300), UNSUPPORTED, b"K=300")
    expect(runs(N=-3), ARG, b"sweep_period -3")
    expect(runs(ring=FAKE + 8), ARG, b"16-byte aligned")
    expect(runs(hyper=(-1.0, 0.9, 0.999, 1e-7)), ARG, b"hyper-parameters")
    expect(runs(hyper=(1e-3, 0.9, 0.999, -1.0)), ARG, b"hyper-parameters")
    expect(runs(R=0), 0)
    expect(runs(V=0), 0)
    expect(runs(g=None), ARG, b"bad argument")
    expect(runs(offsets=None), ARG, b"bad argument")
    expect(runs(stamp=None), ARG, b"bad argument")
    expect(runs(ring=None), ARG, b"bad argument")
    expect(runs(step=None), ARG, b"bad argument")

    def merged(ids=FAKE, W=2, cap=64, K=16, offsets=FAKE, F=3, table=FAKE, stamp=FAKE, ring=FAKE, N=8, V=100, step=FAKE, hyper=H):
        return lib.fil_embed_adam_merged_deferred(ids, FAKE, FAKE, W, cap, K, offsets, None, None, F, table, FAKE, FAKE, stamp, ring, N,
                                                  V, step, *hyper, None)

    expect(merged(W=0), ARG, b"bad argument")
    expect(merged(cap=-1), ARG, b"bad argument")
    expect(merged(K=0), ARG, b"bad argument")
    expect(merged(F=0), ARG, b"bad argument")
    expect(merged(V=-1), ARG, b"bad argument")
    expect(merged(K=257), UNSUPPORTED, b"K=257")
    expect(merged(F=2000), UNSUPPORTED, b"F=2000")
    expect(merged(N=5000), ARG, b"sweep_period 5000")
    expect(merged(hyper=(1e-3, 1.0, 0.999, 1e-7)), ARG, b"hyper-parameters")
    expect(merged(cap=0), 0)
    expect(merged(V=0), 0)
    expect(merged(ids=None), ARG, b"bad argument")
    expect(merged(stamp=None), ARG, b"bad argument")
    expect(merged(ring=None), ARG, b"bad argument")
    expect(merged(table=None), ARG, b"bad argument")

    def roll(table=FAKE, stamp=FAKE, ring=FAKE, N=8, V=100, K=16, offsets=FAKE, F=3, step=FAKE, hyper=H, flags=STEP):
        return lib.fil_embed_adam_roll(table, FAKE, FAKE, stamp, ring, N, V, K, offsets, None, None, F, step, *hyper, flags, None)

    expect(roll(V=-1), ARG, b"bad argument")
    expect(roll(K=0), ARG, b"bad argument")
    expect(roll(F=0), ARG, b"bad argument")
    expect(roll(flags=3), ARG, b"flags 3")
    expect(roll(flags=-1), ARG, b"flags -1")
    expect(roll(K=257), UNSUPPORTED, b"K=257")
    expect(roll(F=1025), UNSUPPORTED, b"F=1025")
    expect(roll(N=0), ARG, b"sweep_period 0")
    expect(roll(ring=FAKE + 12), ARG, b"16-byte aligned")
    expect(roll(hyper=(1e-3, 0.9, float("nan"), 1e-7)), ARG, b"hyper-parameters")
    for fl in (STEP, SKIP, FLUSH):
        expect(roll(V=0, flags=fl), 0)
        expect(roll(table=None, flags=fl), ARG, b"bad argument")
    expect(roll(stamp=None), ARG, b"bad argument")
    expect(roll(ring=None), ARG, b"bad argument")
    expect(roll(offsets=None), ARG, b"bad argument")
    expect(roll(step=None), ARG, b"bad argument")
    return n


if __name__ == "__main__":
    print("optim deferred host calls ok:", run(bind(sys.argv[1])))
