"""The FM kernels (csrc/fm.hip: fil_fm_fwd / fil_fm_bwd, 10 instantiations, and fil_fm_pairs_fwd / fil_fm_pairs_bwd) at CONSTRUCTED tile,
path and grid edges, called through the C ABI with poisoned words behind every input and guarded outputs.

No tolerance anywhere.  emb holds integers in [-4, 4] \\ {0}, lin and g integers in [-8, 8] \\ {0}, F <= 64 (pair list: F <= 200): the
prefix sums and S stay <= 256, the outputs <= 2016 * 16 + 512, g (S - e) <= 8 * 63 * 4 = 2016 (S - e is the sum of the OTHER F - 1 fields),
dlin <= 8 K, the pair list's demb <= 199 * 32 -- every fp32 intermediate of forward and backward is an integer below 2^24 in ANY
summation order, so the fp32 results must equal the integer results
bit for bit (oracle.closed.fm_* on the same integers in float64, where they are exact as well; max |reference| < 2^24 is asserted).  All
inputs are exact in bf16; with bf16 storage out and demb must equal the exact value rounded ONCE to bf16, dlin (fp32) stays exact.  A
dropped, doubled or misplaced term, sample, field or column moves an element by at least 1.

Every operand starts 16-byte aligned (the kernels' contract; functional.py guarantees it) inside a larger allocation: 64 words of the
payload NaN 0x7FC12345 behind each input, 256 bytes of it in front of and behind out, demb and dlin, which must hold those bits after the
call.  (tests/guarded.py)

Which path a case reaches (restated from launch_fm / fm_tile, esz = bytes per element):
    lds     <=>  K % 4 == 0 and K esz % 16 == 0 and K / 4 <= 64 and F K esz <= 32768    fm_{fwd,bwd}_lds_kernel<T>
    vec4    <=>  not lds and K % 4 == 0                                                 fm_{fwd,bwd}_kernel<T, 4>
    scalar  <=>  K % 4 != 0                                                             fm_{fwd,bwd}_kernel<T, 1>
    lds:  slab = F K esz;  TS = clamp(12288 // slab, 1, 64) samples per tile;  a wave's LDS = al16(TS slab) + 1024
          + al16(TS (F 4 forward | K esz backward)) + 1024 (+ al16(TS K 4) + al16(TS (K / 4) 4) backward);  sh = 4 waves of it;
          per_cu = clamp(163840 // sh, 1, 8);  grid = min(cdiv(ntiles, 4), 256 per_cu) workgroups of 4 waves;  wave w of workgroup g takes
          tiles 4 g + w, 4 g + w + 4 grid, ...;  lane -> (sample lane // KQ of a step of bstep = 64 // KQ samples, column quad lane % KQ),
          KQ = K / 4, the 64 - KQ bstep last lanes idle;  the backward stores fpi = 64 // KQ field rows per instruction

    kernel                             case (B, F, K)
    fm_*_lds_kernel<float>             (103, 5, 12) KQ = 3, lane 63 idle, tiles 51, 51, 1;  (45, 7, 20) KQ = 5, four idle lanes, 21, 21, 3;
                                       (9, 3, 256) KQ = 64, fpi = 1, tiles 4, 4, 1;  (6, 32, 256) slab = 32768 = the limit, TS = 1, dynamic
                                       LDS > 48 KiB;  (130, 3, 4) TS capped at 64: 64, 64, 2;  (3, 1, 4) one field;  (1030, 40, 128) TS = 1,
                                       per_cu = 1, 256 workgroups = 1024 waves, waves 0..5 take a SECOND tile (the LDS image is reused)
    fm_*_kernel<float, 4>              (5, 2, 260) KQ = 65;  (5, 33, 256) slab = 33792
    fm_*_kernel<float, 1>              (17, 5, 6), (1, 1, 1)
    fm_*_lds_kernel<__hip_bfloat16>    (67, 9, 8) KQ = 2, tiles 64, 3;  (50, 5, 24) KQ = 6, four idle lanes
    fm_*_kernel<__hip_bfloat16, 4>     (33, 6, 4) rows of 8 bytes;  (33, 6, 12) rows of 24 bytes
    fm_*_kernel<__hip_bfloat16, 1>     (17, 5, 6)
    fm_pairs_fwd_kernel                (6, 200, 9): 1,074,600 elements > 4096 x 256 threads (grid stride), F = 200;  (4, 64, 3);  (66000, 2, 8)
    fm_pairs_bwd_kernel                (66000, 2, 8): 1,056,000 elements (grid stride), one pair;  the other two
"""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from ml_function_amd._lib import FIL_BF16, FIL_F32, check, stream_ptr
from oracle import closed
from tests.guarded import GuardedOutput, poisoned_input

pytestmark = pytest.mark.gpu

DT_IDS = {FIL_F32: "f32", FIL_BF16: "bf16"}
ESZ = {FIL_F32: 4, FIL_BF16: 2}
NPW = {FIL_F32: np.uint32, FIL_BF16: np.uint16}


def cdiv(a, b):
    return (a + b - 1) // b


def fm_path(F, K, esz):
    if K % 4 == 0 and (K * esz) % 16 == 0 and K // 4 <= 64 and F * K * esz <= 32768:
        return "lds"
    return "vec4" if K % 4 == 0 else "scalar"


def fm_geometry(B, F, K, esz, bwd):
    """fm_tile and the launch of launch_fm for an lds shape."""
    al = lambda v: (v + 15) // 16 * 16
    slab = F * K * esz
    TS = max(1, min(64, 12288 // slab))
    wave = al(TS * slab) + 1024 + al(TS * (K * esz if bwd else F * 4)) + 1024 + (al(TS * K * 4) + al(TS * (K // 4) * 4) if bwd else 0)
    sh = 4 * wave
    ntiles = cdiv(B, TS)
    per_cu = max(1, min(8, 163840 // sh))
    grid = max(1, min(cdiv(ntiles, 4), 256 * per_cu))
    KQ = K // 4
    return dict(slab=slab, TS=TS, sh=sh, ntiles=ntiles, per_cu=per_cu, grid=grid, KQ=KQ, bstep=64 // KQ, fpi=64 // KQ, idle=64 - KQ * (64 // KQ),
                tiles=tuple(min(TS, B - t * TS) for t in range(ntiles)))


# (B, F, K, dtype) -> (path, geometry the case was built for: asserted for the forward's and the backward's launch)
CASES = {
    (103, 5, 12, FIL_F32): ("lds", dict(KQ=3, bstep=21, idle=1, TS=51, tiles=(51, 51, 1))),
    (45, 7, 20, FIL_F32): ("lds", dict(KQ=5, bstep=12, idle=4, TS=21, tiles=(21, 21, 3))),
    (9, 3, 256, FIL_F32): ("lds", dict(KQ=64, bstep=1, fpi=1, idle=0, TS=4, tiles=(4, 4, 1))),
    (5, 2, 260, FIL_F32): ("vec4", None),
    (6, 32, 256, FIL_F32): ("lds", dict(slab=32768, TS=1, per_cu=1)),
    (5, 33, 256, FIL_F32): ("vec4", None),
    (130, 3, 4, FIL_F32): ("lds", dict(KQ=1, TS=64, tiles=(64, 64, 2))),
    (1030, 40, 128, FIL_F32): ("lds", dict(TS=1, per_cu=1, grid=256, ntiles=1030)),
    (67, 9, 8, FIL_BF16): ("lds", dict(KQ=2, TS=64, tiles=(64, 3))),
    (50, 5, 24, FIL_BF16): ("lds", dict(KQ=6, bstep=10, idle=4, TS=51, tiles=(50,))),
    (33, 6, 4, FIL_BF16): ("vec4", None),
    (33, 6, 12, FIL_BF16): ("vec4", None),
    (17, 5, 6, FIL_BF16): ("scalar", None),
    (17, 5, 6, FIL_F32): ("scalar", None),
    (1, 1, 1, FIL_F32): ("scalar", None),
    (3, 1, 4, FIL_F32): ("lds", dict(KQ=1, TS=64, tiles=(3,))),      # K = 4 in fp32 is a 16-byte row: the LDS kernels with a single field
}
CASE_IDS = ["%d-%d-%d-%s" % (B, F, K, DT_IDS[dt]) for B, F, K, dt in CASES]


def nonzero_ints(rng, shape, hi):
    return (rng.integers(1, hi + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_case(B, F, K):
    """emb [B, F, K], lin [B, F], g [B, K] (integers held in fp32) and the exact results (float64); read-only, shared by every test of the
    shape."""
    rng = np.random.default_rng(1000003 * B + 1009 * F + K)
    c = dict(emb=nonzero_ints(rng, (B, F, K), 4), lin=nonzero_ints(rng, (B, F), 8), g=nonzero_ints(rng, (B, K), 8))
    c["out"], c["out_nolin"] = closed.fm_fwd(c["emb"], c["lin"]), closed.fm_fwd(c["emb"], None)
    c["demb"], c["dlin"] = closed.fm_bwd(c["emb"], c["g"])
    for k in ("out", "out_nolin", "demb", "dlin"):
        assert np.abs(c[k]).max() < 2 ** 24 and np.array_equal(c[k], np.rint(c[k]))
    for a in c.values():
        a.setflags(write=False)
    return c


def to_words(values, dt):
    """Values that are exact in fp32 (float32 or float64 array) -> the words of the storage type; bf16: rounded once, to nearest even."""
    t = torch.tensor(np.ascontiguousarray(values), dtype=torch.float32)
    if dt == FIL_F32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.bfloat16().view(torch.int16).numpy().view(np.uint16)


def to_f32(words):
    return words.view(np.float32) if words.dtype == np.uint32 else (words.astype(np.uint32) << 16).view(np.float32)


def run_fm(emb, lin, g, dt, with_dlin=True):
    """fil_fm_fwd and fil_fm_bwd on fp32-held values that are exact in the storage type (lin = None: NULL) -> dict of the words of out,
    demb and dlin (None without).  The return codes and every guard are checked here."""
    lib = _lib.load()
    B, F, K = emb.shape
    what = "B=%d F=%d K=%d %s" % (B, F, K, DT_IDS[dt])
    for a in (emb, g):
        assert np.array_equal(to_f32(to_words(a, dt)), a) or not np.isfinite(a).all()        # exact in the storage type
    et, gt = poisoned_input(to_words(emb, dt)), poisoned_input(to_words(g, dt))
    lt = None if lin is None else poisoned_input(to_words(lin, FIL_F32))
    out, demb = GuardedOutput((B, K), NPW[dt], "out"), GuardedOutput((B, F, K), NPW[dt], "demb")
    dlin = GuardedOutput((B, F), np.uint32, "dlin") if with_dlin else None
    check(lib.fil_fm_fwd(et.data_ptr(), None if lt is None else lt.data_ptr(), out.ptr, B, F, K, dt, stream_ptr()), "fil_fm_fwd")
    check(lib.fil_fm_bwd(et.data_ptr(), gt.data_ptr(), demb.ptr, dlin.ptr if with_dlin else None, B, F, K, dt, stream_ptr()), "fil_fm_bwd")
    return dict(out=out.read(what), demb=demb.read(what), dlin=dlin.read(what) if with_dlin else None)


def assert_words(got, want, dt, what):
    want_w = to_words(want, dt)
    bad = np.argwhere(got != want_w)
    assert bad.size == 0, "%s: %d of %d elements differ, first index %s: got %s want %s" % (
        what, len(bad), got.size, bad[:6].tolist(), to_f32(got)[tuple(bad[:6].T)], np.asarray(want)[tuple(bad[:6].T)])


@functools.lru_cache(maxsize=None)
def clean_run(B, F, K, dt):
    c = int_case(B, F, K)
    r = run_fm(c["emb"], c["lin"], c["g"], dt)
    for a in r.values():
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ 1. fil_fm_fwd / fil_fm_bwd, exact
@pytest.mark.parametrize("B,F,K,dt", list(CASES), ids=CASE_IDS)
def test_fm_equals_the_integer_results(B, F, K, dt):
    path, want_geo = CASES[(B, F, K, dt)]
    assert fm_path(F, K, ESZ[dt]) == path
    if path == "lds":
        for bwd in (False, True):
            geo = fm_geometry(B, F, K, ESZ[dt], bwd)
            assert {k: geo[k] for k in want_geo} == want_geo, (bwd, geo)
            assert geo["sh"] <= 160 * 1024
            if (F, K) == (32, 256):
                assert geo["sh"] > 48 * 1024 and fm_path(F + 1, K, ESZ[dt]) == "vec4"            # the LDS limit; dynamic LDS above 48 KiB
            if B == 1030:
                assert geo["ntiles"] - 4 * geo["grid"] == 6 and geo["sh"] > 80 * 1024           # waves 0..5 take a second tile
            else:
                assert geo["ntiles"] <= 4 * geo["grid"]
    elif K % 4 == 0:
        assert K // 4 > 64 or F * K * ESZ[dt] > 32768 or (K * ESZ[dt]) % 16 != 0
    c = int_case(B, F, K)
    what = "B=%d F=%d K=%d %s (%s)" % (B, F, K, DT_IDS[dt], path)
    got = clean_run(B, F, K, dt)
    assert_words(got["out"], c["out"], dt, what + ": out")
    assert_words(got["demb"], c["demb"], dt, what + ": demb")
    assert_words(got["dlin"], c["dlin"], FIL_F32, what + ": dlin")
    if F == 1:
        assert not c["demb"].any() and np.array_equal(c["out"], np.repeat(c["lin"].astype(np.float64), K, axis=1))      # no pair at all


@pytest.mark.parametrize("B,F,K,dt", [(103, 5, 12, FIL_F32), (17, 5, 6, FIL_F32), (50, 5, 24, FIL_BF16), (17, 5, 6, FIL_BF16)],
                         ids=["lds-f32", "scalar-f32", "lds-bf16", "scalar-bf16"])
def test_fm_without_linear_terms(B, F, K, dt):
    """lin = NULL and dlin = NULL at an LDS shape and a fallback shape of each type: out is the pair sum alone, demb is unchanged."""
    c = int_case(B, F, K)
    got = run_fm(c["emb"], None, c["g"], dt, with_dlin=False)
    what = "B=%d F=%d K=%d %s, lin = dlin = NULL" % (B, F, K, DT_IDS[dt])
    assert_words(got["out"], c["out_nolin"], dt, what + ": out")
    assert_words(got["demb"], c["demb"], dt, what + ": demb")


# ------------------------------------------------------------------------------------------------ 2. containment
@pytest.mark.parametrize("B,F,K,n,bad", [(103, 5, 12, 77, 75), (1030, 40, 128, 1027, 1027 - 1)], ids=["103-5-12", "1030-40-128"])
def test_fm_samples_do_not_depend_on_their_position_or_neighbours(B, F, K, n, bad):
    """fm(emb[:n]) == fm(emb)[:n] bit for bit (out, demb, dlin) for an n that cuts a tile (103: tile 51..101; 1030: 1027 tiles of one sample,
    of which three are a wave's second), and NaN, +Inf and -Inf in one sample's embedding -- in the middle of a tile; at 1030 a tile that is
    its wave's second -- leave every other sample and that sample's other columns bit-equal to the clean run, while the columns they sit in
    are non-finite.  (dlin depends on g alone: it stays bit-equal everywhere.)"""
    c = int_case(B, F, K)
    geo = fm_geometry(B, F, K, 4, False)
    if B == 1030:
        assert geo["TS"] == 1 and bad >= 4 * geo["grid"] and n > 4 * fm_geometry(n, F, K, 4, True)["grid"]
    else:
        assert 0 < n % geo["TS"] and 0 < bad % geo["TS"] < geo["TS"] - 1 and bad // geo["TS"] == 1
    full = clean_run(B, F, K, FIL_F32)
    part = run_fm(c["emb"][:n], c["lin"][:n], c["g"][:n], FIL_F32)
    for k in ("out", "demb", "dlin"):
        assert np.array_equal(part[k], full[k][:n]), "%s of the first %d samples depends on the batch size" % (k, n)
    emb = c["emb"].copy()
    cols = [0, K // 2, K - 1]
    emb[bad, 0, cols[0]], emb[bad, F // 2, cols[1]], emb[bad, F - 1, cols[2]] = np.nan, np.inf, -np.inf
    got = run_fm(emb, c["lin"], c["g"], FIL_F32)
    clean = np.ones((B, K), bool)
    clean[bad, cols] = False
    assert np.array_equal(got["out"][clean], full["out"][clean]), "out: the non-finite sample %d reached (sample, column) %s" % (
        bad, np.argwhere((got["out"] != full["out"]) & clean)[:8].tolist())
    cleand = np.broadcast_to(clean[:, None, :], (B, F, K))
    assert np.array_equal(got["demb"][cleand], full["demb"][cleand]), "demb: the non-finite sample %d reached (sample, field, column) %s" % (
        bad, np.argwhere((got["demb"] != full["demb"]) & cleand)[:8].tolist())
    assert np.array_equal(got["dlin"], full["dlin"])
    assert not np.isfinite(to_f32(got["out"])[bad, cols]).any() and not np.isfinite(to_f32(got["demb"])[bad][:, cols]).any()


# ------------------------------------------------------------------------------------------------ 3. the pair list
PAIR_THREADS = 4096 * 256                  # the cap of both launches: more elements than that and the kernels stride


@functools.lru_cache(maxsize=None)
def pair_case(B, F, K):
    rng = np.random.default_rng(7 * B + 11 * F + K)
    emb = nonzero_ints(rng, (B, F, K), 4)
    gp = nonzero_ints(rng, (B, F * (F - 1) // 2, K), 8)
    out = (emb, gp, closed.fm_pairs_fwd(emb), closed.fm_pairs_bwd(emb, gp))
    assert np.abs(out[3]).max() < 2 ** 24
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("B,F,K", [(6, 200, 9), (66000, 2, 8), (4, 64, 3)])
def test_fm_pairs_equal_the_integer_results(B, F, K):
    lib = _lib.load()
    P = F * (F - 1) // 2
    if F == 200:
        assert B * P * K > PAIR_THREADS                                         # the forward strides
    if F == 2:
        assert P == 1 and B * F * K > PAIR_THREADS >= B * P * K                 # the backward strides
    if F == 64:
        assert B * P * K <= PAIR_THREADS
    emb, gp, want_pairs, want_demb = pair_case(B, F, K)
    what = "pairs B=%d F=%d K=%d" % (B, F, K)
    et, gt = poisoned_input(to_words(emb, FIL_F32)), poisoned_input(to_words(gp, FIL_F32))
    pairs, demb = GuardedOutput((B, P, K), np.uint32, "pairs"), GuardedOutput((B, F, K), np.uint32, "demb")
    check(lib.fil_fm_pairs_fwd(et.data_ptr(), pairs.ptr, B, F, K, stream_ptr()), "fil_fm_pairs_fwd")
    check(lib.fil_fm_pairs_bwd(et.data_ptr(), gt.data_ptr(), demb.ptr, B, F, K, stream_ptr()), "fil_fm_pairs_bwd")
    assert_words(pairs.read(what), want_pairs, FIL_F32, what + ": pairs")
    assert_words(demb.read(what), want_demb, FIL_F32, what + ": demb")
