"""The streaming-AUC entry points (fil_confusion_workspace_bytes / fil_confusion_update / fil_auc_result, include/fil.h M1) driven
through their argument checks WITHOUT a GPU (every call returns before its first launch).  Run in-process by
tests/test_metrics_host.py and, as a script, against the AddressSanitizer + UBSan build of the same sources:

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_metrics.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

ARG, WORKSPACE, UNSUPPORTED = -1, -3, -4
FAKE = 1 << 20      # a non-NULL, 16-byte aligned "device" pointer: only ever looked at by a launch, and no call below gets that far
MAX_T, ONE = _lib.FIL_CONFUSION_MAX_T, _lib.FIL_CONFUSION_ONE_LAUNCH_N


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

    # fil_confusion_workspace_bytes: nothing up to the one-launch size, one integer slab per workgroup (a multiple of 256 bytes) above
    ws = lib.fil_confusion_workspace_bytes
    for T in (2, 200, MAX_T):
        assert ws(1, T) == 0 and ws(4096, T) == 0 and ws(ONE, T) == 0, T
        prev = 0
        for m in (ONE + 1, 100003, 1 << 20, 1 << 24):
            b = ws(m, T)
            assert b >= 2 * (T + 1) * 4 and b % 256 == 0 and b >= prev, (m, T, b)
            prev = b
        assert ws(1 << 24, T) <= 256 * (2 * (T + 1) * 4 + 4) + 512, T           # at most one slab per CU
        n += 1
    assert ws(1 << 20, 1) == 0 and ws(1 << 20, MAX_T + 1) == 0                 # outside the menu: nothing to size

    def update(p=FAKE, y=FAKE, m=4096, thr=FAKE, T=200, cm=FAKE, invalid=FAKE, w=None, wb=0):
        return lib.fil_confusion_update(p, y, m, thr, T, cm, invalid, w, wb, None)

    expect(update(m=0), ARG, b"bad argument")
    expect(update(m=-3), ARG, b"bad argument")
    expect(update(m=(1 << 24) + 1), ARG, b"2^24")
    expect(update(T=1), UNSUPPORTED, b"FIL_CONFUSION_MAX_T = %d" % MAX_T)
    expect(update(T=0), UNSUPPORTED, b"T=0")
    expect(update(T=-1), UNSUPPORTED, b"T=-1")
    expect(update(T=MAX_T + 1), UNSUPPORTED, b"T=%d" % (MAX_T + 1))
    expect(update(p=None), ARG, b"bad argument")
    expect(update(y=None), ARG, b"bad argument")
    expect(update(thr=None), ARG, b"bad argument")
    expect(update(cm=None), ARG, b"bad argument")
    expect(update(invalid=None), ARG, b"bad argument")
    expect(update(p=FAKE + 2), ARG, b"bad argument")                           # not even 4-byte aligned
    expect(update(y=FAKE + 1), ARG, b"bad argument")
    for m in (ONE + 1, 1 << 20, 1 << 24):
        need = ws(m, 200)
        expect(update(m=m), WORKSPACE, b"workspace 0 <")
        expect(update(m=m, w=FAKE, wb=need - 1), WORKSPACE, b"< %d bytes" % need)
        expect(update(m=m, w=None, wb=need), WORKSPACE, b"workspace")
    expect(update(m=1 << 24, T=MAX_T, w=FAKE, wb=ws(1 << 24, MAX_T) - 256), WORKSPACE, b"workspace")

    def result(cm=FAKE, T=200, curve=0, summation=0, out=FAKE):
        return lib.fil_auc_result(cm, T, curve, summation, out, None)

    expect(result(T=1), UNSUPPORTED, b"FIL_CONFUSION_MAX_T = %d" % MAX_T)
    expect(result(T=MAX_T + 1), UNSUPPORTED, b"T=%d" % (MAX_T + 1))
    expect(result(cm=None), ARG, b"bad argument")
    expect(result(out=None), ARG, b"bad argument")
    expect(result(curve=2), ARG, b"curve 2")
    expect(result(curve=-1), ARG, b"curve -1")
    expect(result(summation=3), ARG, b"summation 3")
    expect(result(summation=-1), ARG, b"summation -1")
    return n


if __name__ == "__main__":
    print("metrics host calls ok:", run(bind(sys.argv[1])))
