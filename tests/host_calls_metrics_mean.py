"""The Mean-metric entry points (fil_mean_workspace_bytes / fil_mean_update, include/fil.h M2) driven through their argument checks
WITHOUT a GPU (every call returns before its first launch).  Run in-process by tests/test_metrics_mean_host.py against the ordinary
library."""
from ml_function_amd import _lib

ARG, WORKSPACE = -1, -3
FAKE = 1 << 20      # a non-NULL, 16-byte aligned "device" pointer: only ever looked at by a launch, and no call below gets that far
ONE = _lib.FIL_MEAN_ONE_LAUNCH_N
VALUES, BCE, ACC = _lib.FIL_MEAN_VALUES, _lib.FIL_MEAN_BCE, _lib.FIL_MEAN_BINARY_ACC


def run(lib):
    n = 0

    def expect(rc, want, needle=None):
        nonlocal n
        n += 1
        assert rc == want, (n, rc, want, lib.fil_last_error())
        if needle is not None:
            assert needle in lib.fil_last_error(), (n, lib.fil_last_error())

    # fil_mean_workspace_bytes: nothing up to the one-launch size, one 4-byte partial per workgroup (a multiple of 256 bytes) above
    ws = lib.fil_mean_workspace_bytes
    assert ws(1) == 0 and ws(4096) == 0 and ws(ONE) == 0
    prev = 0
    for m in (ONE + 1, 100003, 1 << 20, 1 << 24):
        b = ws(m)
        assert b >= 4 and b % 256 == 0 and b >= prev, (m, b)
        prev = b
    assert ws(1 << 24) <= 256 * 4                                             # at most one partial per CU
    assert ws(0) == 0 and ws(-7) == 0 and ws((1 << 24) + 1) == 0              # outside the limits: nothing to size
    n += 1

    def update(kind=BCE, a=FAKE, y=FAKE, m=4096, c0=1e-7, c1=0.0, state=FAKE, w=None, wb=0):
        return lib.fil_mean_update(kind, a, y, m, c0, c1, state, w, wb, None)

    for kind in (VALUES, BCE, ACC):
        expect(update(kind, m=0), ARG, b"bad argument")
        expect(update(kind, m=-3), ARG, b"bad argument")
        expect(update(kind, m=(1 << 24) + 1), ARG, b"2^24")
        expect(update(kind, a=None), ARG, b"bad argument")
        expect(update(kind, state=None), ARG, b"bad argument")
        expect(update(kind, a=FAKE + 2), ARG, b"bad argument")                # not even 4-byte aligned
        expect(update(kind, a=FAKE + 1), ARG, b"bad argument")
        expect(update(kind, state=FAKE + 3), ARG, b"bad argument")
        for m in (ONE + 1, 1 << 20, 1 << 24):
            need = ws(m)
            expect(update(kind, m=m), WORKSPACE, b"workspace 0 <")
            expect(update(kind, m=m, w=FAKE, wb=need - 1), WORKSPACE, b"< %d bytes" % need)
            expect(update(kind, m=m, w=None, wb=need), WORKSPACE, b"workspace")
        expect(update(kind, m=1 << 20, w=FAKE + 2, wb=ws(1 << 20)), ARG, b"bad argument")
    expect(update(BCE, y=None), ARG, b"bad argument")                         # only FIL_MEAN_VALUES reads no y
    expect(update(ACC, y=None), ARG, b"bad argument")
    expect(update(BCE, y=FAKE + 1), ARG, b"bad argument")
    expect(update(ACC, y=FAKE + 2), ARG, b"bad argument")
    for kind in (-1, 3, 7):
        expect(update(kind), ARG, b"kind %d" % kind)
    return n
