"""The CIN precision entry points (fil_cin_fwd_p / fil_cin_bwd_p / fil_cin_precision_used, ABI 216) driven through their argument
checks WITHOUT a GPU (every call returns before the first launch).  Run in-process by tests/test_cin_bf16.py and, as a script, against
the AddressSanitizer + UBSan build of the same sources (as tests/host_calls.py):

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_bf16.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

PREC_DEFAULT, PREC_BF16 = 0, 1
BF16X3, TAIL_ALWAYS, NOQMERGE = 2, 64, 512


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

    assert lib.fil_version() == _lib.header_abi_version() == 216
    H3 = _lib.int_array([128, 128, 128])
    H200 = _lib.int_array([200, 200, 200])
    nul8 = [None] * 8
    nul12 = [None] * 12

    def fwd(B, F, mode, prec, H=H3, L=3):
        return lib.fil_cin_fwd_p(*nul8, B, F, 16, L, H, 1, mode, prec, None, 0, None)

    def bwd(B, F, mode, prec, H=H3, L=3):
        return lib.fil_cin_bwd_p(*nul12, B, F, 16, L, H, 1, mode, prec, None, None, 0, None)

    # the existing entry points are unchanged: mode 1024 is still beyond the mode bits
    expect(lib.fil_cin_fwd(*nul8, 4, 39, 16, 3, H3, 1, 1024, None, 0, None), -4, b"mode 1024")
    expect(lib.fil_cin_bwd(*nul12, 4, 39, 16, 3, H3, 1, 1024, None, None, 0, None), -4, b"mode 1024")
    expect(lib.fil_cin_fwd(*nul8, 4, 39, 16, 3, H3, 1, 1 << 20, None, 0, None), -4, b"mode")   # no internal bit gets through
    # ... nor do the _p ones accept it
    expect(fwd(4, 39, 1024, PREC_DEFAULT), -4, b"mode 1024")
    expect(fwd(4, 39, 1 << 20, PREC_BF16), -4, b"mode")
    expect(bwd(4, 39, 1024, PREC_BF16), -4, b"mode 1024")
    # precision codes
    for bad in (2, -1, 7, 1 << 20):
        expect(fwd(4, 39, 0, bad), -1, b"precision")
        expect(bwd(4, 39, 0, bad), -1, b"precision")
    # BF16 with the split mode: two operand precisions
    expect(fwd(4096, 39, BF16X3, PREC_BF16), -1, b"BF16X3")
    expect(bwd(4096, 39, BF16X3 | TAIL_ALWAYS, PREC_BF16), -1, b"BF16X3")
    # NULL tensors / workspace: the argument check of the existing entry points
    expect(fwd(4, 39, 0, PREC_BF16), -1, b"bad argument")
    expect(bwd(4, 39, 0, PREC_BF16), -1, b"bad argument")
    expect(fwd(4, 39, BF16X3, PREC_DEFAULT), -1, b"bad argument")
    # B = 0: nothing to do (the forward returns before its pointers are looked at; the backward zero-fills dW, so it needs them)
    expect(fwd(0, 39, 0, PREC_BF16), 0)
    expect(bwd(0, 39, 0, PREC_BF16), -1, b"bad argument")
    # shape limits come first, as in fil_cin_fwd
    expect(fwd(4, 70, 0, PREC_BF16), -4, b"64 fields")
    expect(fwd(4, 39, 0, PREC_BF16, L=9), -4)
    # what runs
    P = lib.fil_cin_precision_used
    expect(P(4096, 39, 16, 3, H3, 0, PREC_BF16), PREC_BF16)
    expect(P(4096, 20, 16, 3, H3, 0, PREC_BF16), PREC_BF16)
    expect(P(4096, 41, 16, 3, H3, 0, PREC_BF16), PREC_BF16)
    expect(P(4096, 39, 16, 3, H3, 0, PREC_DEFAULT), PREC_DEFAULT)
    expect(P(4096, 39, 16, 3, H200, 0, PREC_BF16), PREC_DEFAULT)               # H_1 != 128
    expect(P(64, 39, 16, 3, H3, 0, PREC_BF16), PREC_DEFAULT)                    # below the 16 K-row rule ...
    expect(P(64, 39, 16, 3, H3, TAIL_ALWAYS, PREC_BF16), PREC_BF16)             # ... which TAIL_ALWAYS lifts
    expect(P(4096, 39, 16, 3, H3, NOQMERGE, PREC_BF16), PREC_DEFAULT)           # not on the merged tail
    expect(P(4096, 39, 16, 2, H3, 0, PREC_BF16), PREC_DEFAULT)                  # two layers
    expect(P(0, 39, 16, 3, H3, 0, PREC_BF16), PREC_DEFAULT)                     # nothing runs
    expect(P(4096, 39, 16, 3, H3, BF16X3, PREC_BF16), -1, b"BF16X3")
    expect(P(4096, 39, 16, 3, H3, 0, 5), -1, b"precision")
    expect(P(4096, 39, 16, 3, H3, 1024, PREC_BF16), -4, b"mode")
    expect(P(4096, 70, 16, 3, H3, 0, PREC_BF16), -4)
    expect(P(4096, 39, 16, 3, None, 0, PREC_BF16), -1)
    # the sizes of saved / workspaces are the existing functions' and cover every precision (they take none)
    for B in (1, 4096, 150000):
        assert lib.fil_cin_saved_bytes(B, 39, 16, 3, H3) > 0 and lib.fil_cin_fwd_workspace_bytes(B, 39, 16, 3, H3) > 0
    # the bf16 path's ready points are the merged tail's, whatever the precision (fil_cin_grad_ready_points takes none)
    pts = (ctypes.c_int * 4)()
    assert lib.fil_cin_grad_ready_points(4096, 39, 16, 3, H3, 0, pts) == 2 and list(pts) == [0, 1, 1, 0]
    return n


if __name__ == "__main__":
    print("bf16 host calls ok:", run(bind(sys.argv[1])))
