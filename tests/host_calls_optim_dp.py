"""The data-parallel runs entry points (fil_embed_runs_compact / fil_embed_adam_merged) driven through their argument checks WITHOUT a
GPU (every call returns before its first launch).  Run in-process by tests/test_optim_dp_host.py and, as a script, against the
AddressSanitizer + UBSan build of the same sources (as tests/host_calls_optim.py):

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_optim_dp.py ml_function_amd/build/asan/libfil_hip_asan.so
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
    # workspace: a tile count per 2048 positions + one int32 slot per position, each rounded to 256 bytes; nothing for R = 0
    assert lib.fil_embed_runs_compact_workspace_bytes(0) == 0 and lib.fil_embed_runs_compact_workspace_bytes(-3) == 0
    assert lib.fil_embed_runs_compact_workspace_bytes(1) == 512
    assert lib.fil_embed_runs_compact_workspace_bytes(4096) == 256 + 16384
    WS = lib.fil_embed_runs_compact_workspace_bytes(64)

    def compact(g=FAKE, R=64, K=16, g_dtype=_lib.FIL_F32, ids=FAKE, values=FAKE, count=FAKE, cap=64, ws=FAKE, ws_bytes=WS):
        return lib.fil_embed_runs_compact(g, FAKE, FAKE, R, K, g_dtype, ids, values, count, cap, ws, ws_bytes, None)

    # fil_embed_runs_compact
    expect(compact(R=-1), ARG, b"bad argument")
    expect(compact(K=0), ARG, b"bad argument")
    expect(compact(cap=-1), ARG, b"bad argument")
    expect(compact(g_dtype=5), ARG, b"g_dtype 5")
    expect(compact(K=257), UNSUPPORTED, b"K=257")
    expect(compact(cap=63), ARG, b"cap 63 < R 64")
    expect(compact(R=1 << 31, cap=1 << 31, ws_bytes=1 << 40), UNSUPPORTED, b"R=2147483648")
    expect(compact(ids=None), ARG, b"bad argument")
    expect(compact(count=None), ARG, b"bad argument")
    expect(compact(ws_bytes=WS - 1), ARG, b"workspace")
    expect(compact(g=None), ARG, b"bad argument")
    expect(compact(values=None), ARG, b"bad argument")
    expect(compact(ws=None), ARG, b"bad argument")
    expect(compact(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")

    def merged(ids=FAKE, W=2, cap=64, K=16, offsets=FAKE, F=3, table=FAKE, stamp=FAKE, V=100, step=FAKE, hyper=H, mode=KERAS):
        return lib.fil_embed_adam_merged(ids, FAKE, FAKE, W, cap, K, offsets, None, F, table, FAKE, FAKE, stamp, V, step, *hyper, mode,
                                         None)

    # fil_embed_adam_merged
    expect(merged(W=0), ARG, b"bad argument")
    expect(merged(W=-2), ARG, b"bad argument")
    expect(merged(cap=-1), ARG, b"bad argument")
    expect(merged(K=0), ARG, b"bad argument")
    expect(merged(F=0), ARG, b"bad argument")
    expect(merged(V=-1), ARG, b"bad argument")
    expect(merged(mode=3), ARG, b"mode 3")
    expect(merged(stamp=None), ARG, b"row stamps")                   # Keras mode needs them ...
    expect(merged(stamp=None, mode=LAZY, cap=0), 0)                  # ... lazy mode does not (cap = 0: nothing to do)
    expect(merged(K=257), UNSUPPORTED, b"K=257")
    expect(merged(F=1025), UNSUPPORTED, b"F=1025")
    expect(merged(hyper=(1e-3, 0.9, 1.0, 1e-7)), ARG, b"hyper-parameters")
    expect(merged(hyper=(float("nan"), 0.9, 0.999, 1e-7)), ARG, b"hyper-parameters")
    expect(merged(cap=0), 0)
    expect(merged(V=0), 0)
    expect(merged(ids=None), ARG, b"bad argument")
    expect(merged(offsets=None), ARG, b"bad argument")
    expect(merged(table=None, mode=LAZY), ARG, b"bad argument")
    expect(merged(step=None), ARG, b"bad argument")
    return n


if __name__ == "__main__":
    print("optim dp host calls ok:", run(bind(sys.argv[1])))
