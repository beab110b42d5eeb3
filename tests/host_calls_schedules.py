"""The schedule entry points (fil_lr_schedule_check / fil_lr_schedule_eval and the *_lrdev update variants, include/fil.h O3) driven
through their argument checks WITHOUT a GPU (every call returns before its first launch).  Run in-process by
tests/test_schedules_host.py and, as a script, against the AddressSanitizer + UBSan build of the same sources:

    LD_PRELOAD=<libclang_rt.asan> python tests/host_calls_schedules.py ml_function_amd/build/asan/libfil_hip_asan.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

ARG, UNSUPPORTED = -1, -4
FAKE = 1 << 20      # a non-NULL, 16-byte aligned "device" pointer: only ever looked at by a launch, and no call below gets that far

# the update variants and the position of lr_dev in their argument lists
LR_POS = {"fil_adam_multi_lrdev": 4, "fil_embed_adam_runs_lrdev": 13, "fil_embed_adam_sweep_lrdev": 11, "fil_embed_adam_merged_lrdev": 15,
          "fil_embed_adam_runs_deferred_lrdev": 18, "fil_embed_adam_merged_deferred_lrdev": 18, "fil_embed_adam_roll_lrdev": 13,
          "fil_rowopt_multi_lrdev": 6, "fil_embed_rowopt_runs_lrdev": 15, "fil_embed_rowopt_sweep_lrdev": 13,
          "fil_embed_rowopt_merged_lrdev": 17}
NEW = ("fil_lr_schedule_check", "fil_lr_schedule_eval") + tuple(LR_POS)


def bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def descriptor(kind=_lib.FIL_LR_EXPONENTIAL, flag=0, initial=0.1, decay_steps=10.0, decay_rate=0.5, end=1e-4, power=1.0, decay=0.0,
               boundaries=(), values=()):
    d = _lib.LrSchedule()
    d.kind, d.flag, d.initial_lr, d.decay_steps, d.decay_rate, d.end_lr, d.power, d.decay = (kind, flag, initial, decay_steps, decay_rate,
                                                                                             end, power, decay)
    d.n_boundaries = len(boundaries)
    for i, b in enumerate(boundaries[:_lib.FIL_LR_MAX_BOUNDARIES]):
        d.boundaries[i] = b
    for i, v in enumerate(values[:_lib.FIL_LR_MAX_BOUNDARIES + 1]):
        d.values[i] = v
    return d


def plain_args(name, lr_dev=FAKE):
    """An argument list that passes every check of the variant's by-value twin up to the first launch guard: pointers FAKE, sizes
    small, hyper-parameters Keras' defaults."""
    out = []
    for i, t in enumerate(_lib.SIGNATURES[name][1]):
        if i == LR_POS[name]:
            out.append(lr_dev)
        elif t is ctypes.c_void_p:
            out.append(FAKE)
        elif t is ctypes.c_float:
            out.append(0.5)
        else:
            out.append(1)
    return out


def run(lib):
    n = 0

    def expect(rc, want, needle=None):
        nonlocal n
        n += 1
        assert rc == want, (n, rc, want, lib.fil_last_error())
        if needle is not None:
            assert needle in lib.fil_last_error(), (n, lib.fil_last_error())

    def checked(d):
        return lib.fil_lr_schedule_check(None if d is None else ctypes.addressof(d))

    K = _lib
    expect(checked(None), ARG, b"host_sched is NULL")
    expect(checked(descriptor(kind=5)), ARG, b"kind 5")
    expect(checked(descriptor(kind=-1)), ARG, b"kind -1")
    for kind in (K.FIL_LR_EXPONENTIAL, K.FIL_LR_INVERSE_TIME, K.FIL_LR_POLYNOMIAL):
        expect(checked(descriptor(kind=kind, decay_steps=0.0)), ARG, b"decay_steps 0")
        expect(checked(descriptor(kind=kind, decay_steps=-3.0)), ARG, b"decay_steps -3")
        expect(checked(descriptor(kind=kind, decay_steps=float("nan"))), ARG, b"decay_steps")
        expect(checked(descriptor(kind=kind, flag=1)), 0)
    expect(checked(descriptor(kind=K.FIL_LR_CONSTANT, decay_steps=0.0, decay=0.5)), 0)         # (a constant has no decay_steps)
    expect(checked(descriptor(decay=-0.5)), ARG, b"decay -0.5")
    expect(checked(descriptor(decay=float("nan"))), ARG, b"decay")
    many = list(range(33))
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=many, values=[0.1] * 34)), ARG, b"33 boundaries")
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE)), ARG, b"0 boundaries")
    bad = descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=[1], values=[0.1, 0.2])
    bad.n_boundaries = -2
    expect(checked(bad), ARG, b"-2 boundaries")
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=[10, 5, 20], values=[0.1] * 4)), ARG, b"not sorted")
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=[10, 20, 19], values=[0.1] * 4)), ARG, b"boundaries[2] = 19")
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=[10, 10, 20], values=[0.1] * 4)), 0)     # equal boundaries: an empty piece
    expect(checked(descriptor(kind=K.FIL_LR_PIECEWISE, boundaries=list(range(32)), values=[0.1] * 33)), 0)

    ev = lib.fil_lr_schedule_eval
    expect(ev(None, FAKE, FAKE, None), ARG, b"bad argument")
    expect(ev(FAKE, None, FAKE, None), ARG, b"bad argument")
    expect(ev(FAKE, FAKE, None, None), ARG, b"bad argument")

    for name in LR_POS:
        fn = getattr(lib, name)
        expect(fn(*plain_args(name, lr_dev=None)), ARG, b"%s: no device rate (lr_dev is NULL)" % name.encode())
    # the shared bodies report under the variant's own name
    a = plain_args("fil_adam_multi_lrdev")
    a[1] = -1
    expect(lib.fil_adam_multi_lrdev(*a), ARG, b"fil_adam_multi_lrdev: bad argument")
    a = plain_args("fil_adam_multi_lrdev")
    a[5] = 1.5                                                                                 # beta_1
    expect(lib.fil_adam_multi_lrdev(*a), ARG, b"fil_adam_multi_lrdev: hyper-parameters")
    a = plain_args("fil_embed_adam_runs_lrdev")
    a[17] = 7                                                                                  # mode
    expect(lib.fil_embed_adam_runs_lrdev(*a), ARG, b"fil_embed_adam_runs_lrdev: mode 7")
    a = plain_args("fil_embed_adam_sweep_lrdev")
    a[9] = 5000                                                                                # F
    expect(lib.fil_embed_adam_sweep_lrdev(*a), UNSUPPORTED, b"fil_embed_adam_sweep_lrdev: F=5000")
    a = plain_args("fil_embed_adam_roll_lrdev")
    a[17] = 9                                                                                  # flags
    expect(lib.fil_embed_adam_roll_lrdev(*a), ARG, b"fil_embed_adam_roll_lrdev: flags 9")
    h = _lib.RowoptHyper(0.0, 1e-7, -0.5, 0.0, 0.0, 0.0)
    a = plain_args("fil_rowopt_multi_lrdev")
    a[4], a[5] = 3, ctypes.addressof(h)                                                        # rule
    expect(lib.fil_rowopt_multi_lrdev(*a), ARG, b"fil_rowopt_multi_lrdev: rule 3")
    a = plain_args("fil_embed_rowopt_runs_lrdev")
    a[13], a[14] = _lib.FIL_OPT_ADAGRAD, None                                                  # no hyper-parameters
    expect(lib.fil_embed_rowopt_runs_lrdev(*a), ARG, b"fil_embed_rowopt_runs_lrdev: no hyper-parameters")
    return n


if __name__ == "__main__":
    print("schedules host calls ok:", run(bind(sys.argv[1])))
