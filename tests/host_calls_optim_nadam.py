"""The Keras Nadam entry points (fil_nadam_multi / fil_embed_nadam_runs / fil_embed_nadam_sweep / fil_embed_nadam_merged) driven through
their argument checks WITHOUT a GPU (every call returns before its first launch).  Run in-process by tests/test_optim_nadam_host.py; as
a script it takes the path of a build of the library:

    python tests/host_calls_optim_nadam.py ml_function_amd/libfil_hip.so
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib  # noqa: E402

NADAM = _lib.FIL_OPT_NADAM
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
        vals = dict(lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004, reserved=0, m_cache=FAKE)
        vals.update(kw)
        h = _lib.NadamHyper(**vals)
        keep.append(h)
        return ctypes.addressof(h)

    H = hyper()
    nan = float("nan")
    NH = b"Nadam hyper-parameters"
    bad = [(NADAM, hyper(lr=-1.0), NH), (NADAM, hyper(lr=nan), NH), (NADAM, hyper(epsilon=-1e-7), NH), (NADAM, hyper(epsilon=nan), NH),
           (NADAM, hyper(schedule_decay=-0.004), NH), (NADAM, hyper(schedule_decay=nan), NH), (NADAM, hyper(beta_1=-0.1), NH),
           (NADAM, hyper(beta_1=1.0), NH), (NADAM, hyper(beta_1=nan), NH), (NADAM, hyper(beta_2=1.0), NH), (NADAM, hyper(beta_2=-0.5), NH),
           (NADAM, hyper(beta_2=nan), NH), (NADAM, hyper(m_cache=None), b"m_cache is NULL"), (NADAM, hyper(reserved=1), b"reserved 1"),
           (NADAM, hyper(reserved=-1), b"reserved -1"),
           # an unknown rule: the other families' and the next free number
           (0, H, b"rule 0"), (1, H, b"rule 1"), (2, H, b"rule 2"), (3, H, b"rule 3"), (4, H, b"rule 4"), (5, H, b"rule 5"),
           (6, H, b"rule 6"), (8, H, b"rule 8"), (-1, H, b"rule -1"), (NADAM, None, b"hyper is NULL")]
    ok = [H, hyper(beta_1=0.0, beta_2=0.0, epsilon=0.0, lr=0.0, schedule_decay=0.0), hyper(beta_1=0.999, beta_2=0.5, schedule_decay=10.0)]

    # ---- fil_nadam_multi
    def multi(tensors=FAKE, n_=1, total=1, step=FAKE, rule=NADAM, h=H, advance=1):
        return lib.fil_nadam_multi(tensors, n_, total, step, rule, h, advance, None)
    expect(multi(n_=-1), ARG, b"bad argument")
    expect(multi(total=-5), ARG, b"bad argument")
    expect(multi(step=None), ARG, b"bad argument")
    expect(multi(tensors=None), ARG, b"bad argument")
    expect(multi(advance=2), ARG, b"advance 2")
    expect(multi(advance=-1), ARG, b"advance -1")
    for rule, h, needle in bad:
        expect(multi(rule=rule, h=h), ARG, needle)
        expect(multi(rule=rule, h=h, tensors=None, n_=0, total=0, advance=0), ARG, needle)      # checked even with nothing to do
    for h in ok:
        expect(multi(tensors=None, n_=0, total=0, advance=0, h=h), 0)    # nothing to update or advance: no launch

    # ---- fil_embed_nadam_runs
    def runs(g=FAKE, R=8, K=16, g_dtype=_lib.FIL_F32, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, step=FAKE, rule=NADAM, h=H, perm=FAKE,
             ids=FAKE):
        return lib.fil_embed_nadam_runs(g, perm, ids, R, K, g_dtype, F, None, table, slot0, slot1, None, step, rule, h, None)
    expect(runs(R=-1), ARG, b"bad argument")
    expect(runs(K=0), ARG, b"bad argument")
    expect(runs(F=0), ARG, b"bad argument")
    expect(runs(g_dtype=7), ARG, b"g_dtype 7")
    expect(runs(K=257), UNSUPPORTED, b"K=257")
    expect(runs(K=256, R=0), 0)
    for rule, h, needle in bad:
        expect(runs(rule=rule, h=h), ARG, needle)
        expect(runs(rule=rule, h=h, R=0), ARG, needle)
    # R = 0: FIL_OK without a pointer looked at
    expect(runs(R=0, g=None, perm=None, ids=None, table=None, slot0=None, slot1=None, step=None), 0)
    expect(runs(g=None), ARG, b"bad argument")
    expect(runs(perm=None), ARG, b"bad argument")
    expect(runs(ids=None), ARG, b"bad argument")
    expect(runs(table=None), ARG, b"bad argument")
    expect(runs(step=None), ARG, b"bad argument")
    expect(runs(slot0=None), ARG, b"first slot")
    expect(runs(slot1=None), ARG, b"second slot")
    expect(runs(slot0=None, slot1=None), ARG, b"first slot")
    expect(runs(g_dtype=_lib.FIL_BF16, g=None), ARG, b"bad argument")

    # ---- fil_embed_nadam_sweep
    def sweep(V=100, K=16, F=2, table=FAKE, slot0=FAKE, slot1=FAKE, stamp=FAKE, offsets=FAKE, field_l2=FAKE, step=FAKE, rule=NADAM, h=H):
        return lib.fil_embed_nadam_sweep(table, slot0, slot1, stamp, V, K, offsets, field_l2, None, F, step, rule, h, None)
    expect(sweep(V=-1), ARG, b"bad argument")
    expect(sweep(K=0), ARG, b"bad argument")
    expect(sweep(F=0), ARG, b"bad argument")
    expect(sweep(F=1025), UNSUPPORTED, b"F=1025")
    for rule, h, needle in bad:
        expect(sweep(rule=rule, h=h), ARG, needle)
        expect(sweep(rule=rule, h=h, V=0), ARG, needle)
    # V = 0: FIL_OK, no launch, no pointer looked at
    expect(sweep(V=0, table=None, slot0=None, slot1=None, stamp=None, offsets=None, step=None), 0)
    # the sweep decays m and v on every row: it launches without a regularised field too, so its pointers are looked at
    for l2 in (FAKE, None):
        expect(sweep(field_l2=l2, table=None), ARG, b"bad argument")
        expect(sweep(field_l2=l2, stamp=None), ARG, b"bad argument")
        expect(sweep(field_l2=l2, offsets=None), ARG, b"bad argument")
        expect(sweep(field_l2=l2, step=None), ARG, b"bad argument")
        expect(sweep(field_l2=l2, slot0=None), ARG, b"first slot")
        expect(sweep(field_l2=l2, slot1=None), ARG, b"second slot")

    # ---- fil_embed_nadam_merged
    def merged(ids=FAKE, values=FAKE, counts=FAKE, W=2, cap=64, K=16, F=2, V=100, offsets=FAKE, table=FAKE, slot0=FAKE, slot1=FAKE,
               step=FAKE, rule=NADAM, h=H):
        return lib.fil_embed_nadam_merged(ids, values, counts, W, cap, K, offsets, None, F, table, slot0, slot1, None, V, step, rule, h, None)
    expect(merged(W=0), ARG, b"bad argument")
    expect(merged(cap=-1), ARG, b"bad argument")
    expect(merged(K=0), ARG, b"bad argument")
    expect(merged(V=-1), ARG, b"bad argument")
    expect(merged(K=257), UNSUPPORTED, b"K=257")
    expect(merged(F=1025), UNSUPPORTED, b"F=1025")
    for rule, h, needle in bad:
        expect(merged(rule=rule, h=h), ARG, needle)
        expect(merged(rule=rule, h=h, cap=0), ARG, needle)
    none = dict(ids=None, values=None, counts=None, offsets=None, table=None, slot0=None, slot1=None, step=None)
    expect(merged(cap=0, **none), 0)
    expect(merged(V=0, **none), 0)
    expect(merged(ids=None), ARG, b"bad argument")
    expect(merged(values=None), ARG, b"bad argument")
    expect(merged(counts=None), ARG, b"bad argument")
    expect(merged(offsets=None), ARG, b"bad argument")
    expect(merged(table=None), ARG, b"bad argument")
    expect(merged(step=None), ARG, b"bad argument")
    expect(merged(slot0=None), ARG, b"first slot")
    expect(merged(slot1=None), ARG, b"second slot")
    return n


if __name__ == "__main__":
    print("optim nadam host calls ok:", run(bind(sys.argv[1])))
