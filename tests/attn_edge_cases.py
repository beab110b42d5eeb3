"""The AutoInt interacting layer's dispatch (csrc/attn_impl.h: make_dims, fwd_lds, bwd_lds, plan_fwd, plan_bwd) restated in Python, and the case
tables built on it.  Shared by tests/test_attn_edges_gpu.py (which runs every case on the GPU and asserts, against fil_attn_plan, the
instantiation it was built for) and tests/test_host.py (which holds this restatement to fil_attn_plan over the whole menu without a GPU).
Needs neither torch nor the library.

    nblk = cdiv(F, 16), FP = 16 nblk, NC = cdiv(K, 16);  menu: K <= 64, A <= 16, H <= 8, F <= 512, else FIL_ERR_UNSUPPORTED
    LDS_CAP = 160 KiB - 512 = 163,328 bytes of dynamic LDS;  a direction whose footprint exceeds it is refused (FIL_ERR_UNSUPPORTED)
    forward   kreg (k fragments in registers) <=> f16 and nblk <= 13 and FIL_ATTN_KREG != 0:  sh = 32 NC FP
              otherwise  f16: sh = 32 FP (NC + H),  f32: sh = 80 H FP;   A == 16 form <=> A == 16
    backward  NB = the first of 4, 8, 13, 32 with NB >= nblk;  A == 16 form <=> A == 16 and NB >= 13
              sh(wph, dx) = f16: 2 (16 NC FP + 16 H (FP + 16) + 256 (6 H wph + 3 H NC)) + dx 64 NC FP
                            f32: 4 (20 H (FP + 16) + 1920 H wph)                        + dx 64 NC FP
              refused if sh(1, 0) > LDS_CAP.  wph = 2 if nblk > 8 and 2 sh(1, 0) > LDS_CAP;  also if nblk > 8, H <= 4, the dx image
              does not come free with one wave per head (sh(1, 1) > LDS_CAP or it costs the second resident workgroup) and
              sh(2, 1) <= LDS_CAP;  FIL_ATTN_WPH = 1 / 2 replaces that choice where nblk > 8;  back to 1 if H > 4 or sh(2, 0) > LDS_CAP.
              dx image in LDS <=> FIL_ATTN_DX_LDS != 0 and sh(wph, 1) <= LDS_CAP and LDS_CAP // sh(wph, 1) >= min(LDS_CAP // sh(wph, 0), 2)
    grid      persistent backward workgroups: at most 1024 / wph, each reduces into its own wph partial sets (attn_reduce_kernel sums
              grid * wph sets of dW* and grid * wph * H of dgamma / dbeta);  with B <= 256 every sample has a workgroup of its own
"""
import collections
import os

LDS_CAP = 160 * 1024 - 512
MAX_K, MAX_A, MAX_H, MAX_F = 64, 16, 8, 512
F32, F16 = 0, 1
PRECISIONS = {"f32": F32, "f16_mfma": F16}
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4

# the ten words of fil_attn_plan, in its order
Plan = collections.namedtuple("Plan", "fwd_ok fwd_kreg fwd_a16 fwd_lds bwd_ok bwd_nb bwd_wph bwd_dx_lds bwd_a16 bwd_lds")


def cdiv(a, b):
    return (a + b - 1) // b


def _knob(name, default):
    """An integer knob as the library reads it (atoi of the variable; unset = default)."""
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        return int(v.strip() or 0)
    except ValueError:
        return 0


def fwd_lds(F, K, H, f16):
    FP, NC = 16 * cdiv(F, 16), cdiv(K, 16)
    return (NC * FP * 16 + H * FP * 16) * 2 if f16 else H * FP * 20 * 4


def bwd_lds(F, K, H, f16, wph=1, dx=False):
    FP, NC = 16 * cdiv(F, 16), cdiv(K, 16)
    dxb = NC * FP * 16 * 4 if dx else 0
    if f16:
        tiles = H * wph * 6 + 3 * H * NC
        return (NC * FP * 16 + H * (FP + 16) * 16 + tiles * 256) * 2 + dxb
    return (H * (FP + 16) * 20 + H * wph * 6 * 320) * 4 + dxb


def plan_rc(F, K, H, A, precision):
    """The return code of fil_attn_plan (make_dims' order of checks)."""
    if F < 1 or K < 1 or H < 1 or A < 1:
        return ERR_ARG
    if K > MAX_K or A > MAX_A or H > MAX_H or F > MAX_F:
        return ERR_UNSUPPORTED
    return OK if precision in (F32, F16) else ERR_ARG


def plan(F, K, H, A, precision):
    """-> Plan, what fil_attn_plan writes for a shape inside the menu (the knobs are read from the environment at every call)."""
    assert plan_rc(F, K, H, A, precision) == OK
    f16 = precision == F16
    nblk, NC = cdiv(F, 16), cdiv(K, 16)
    FP = 16 * nblk
    kreg = f16 and nblk <= 13 and _knob("FIL_ATTN_KREG", 1) != 0
    fsh = NC * FP * 16 * 2 if kreg else fwd_lds(F, K, H, f16)
    nb = 4 if nblk <= 4 else 8 if nblk <= 8 else 13 if nblk <= 13 else 32
    a16 = nb >= 13 and A == 16
    sh = bwd_lds(F, K, H, f16)
    if sh > LDS_CAP:
        return Plan(int(fsh <= LDS_CAP), int(kreg), int(A == 16), fsh, 0, nb, 1, 0, int(a16), sh)
    wph = 2 if (2 * sh > LDS_CAP and nblk > 8) else 1
    if wph == 1 and nblk > 8 and H <= 4:
        sh1d, sh2d = bwd_lds(F, K, H, f16, 1, True), bwd_lds(F, K, H, f16, 2, True)
        dx_with_1 = sh1d <= LDS_CAP and LDS_CAP // sh1d >= min(LDS_CAP // sh, 2)
        if not dx_with_1 and sh2d <= LDS_CAP:
            wph = 2
    wk = _knob("FIL_ATTN_WPH", 0)
    if wk in (1, 2):
        wph = wk if nblk > 8 else 1
    if wph == 2 and (H > 4 or bwd_lds(F, K, H, f16, 2) > LDS_CAP or nblk < 2):
        wph = 1
    sh = bwd_lds(F, K, H, f16, wph)
    dx = 0
    if _knob("FIL_ATTN_DX_LDS", 1) != 0:
        sh2 = bwd_lds(F, K, H, f16, wph, True)
        if sh2 <= LDS_CAP and LDS_CAP // sh2 >= min(LDS_CAP // sh, 2):
            dx, sh = 1, sh2
    return Plan(int(fsh <= LDS_CAP), int(kreg), int(A == 16), fsh, 1, nb, wph, dx, int(a16), sh)


def knobs_set():
    return [k for k in ("FIL_ATTN_KREG", "FIL_ATTN_WPH", "FIL_ATTN_DX_LDS") if k in os.environ]


# the host sweep of tests/test_host.py: the whole menu
SWEEP_F = range(1, MAX_F + 1)
SWEEP_K = (1, 16, 17, 32, 33, 48, 49, 64)
SWEEP_H = range(1, MAX_H + 1)
SWEEP_A = (1, 7, 16)

# ---------------------------------------------------------------------------------------------------------------- shape cases
# (F, K, H, A) -> {precision: (NB, wph, dx_lds) of the backward the case was built for without knobs, or None = as the plan says}, the edge
# the case is built for.  "f16 only": the f32 twin is one of REFUSED below.
SHAPE_CASES = collections.OrderedDict([
    ((1, 1, 1, 1), ({}, "smallest legal shape")),
    ((16, 16, 1, 16), ({}, "one full tile, no masks")),
    ((17, 17, 1, 16), ({}, "one row into block 2, one column into chunk 2")),
    ((64, 16, 2, 16), ({}, "top of NB=4")),
    ((65, 33, 2, 8), ({F32: (8, 1, 1), F16: (8, 1, 1)}, "bottom of NB=8, NC=3 with one live column, A=8")),
    ((112, 33, 5, 3), ({F32: (8, 1, 1), F16: (8, 1, 0)}, "H=5, A=3")),
    ((128, 48, 8, 16), ({F32: (8, 1, 0), F16: (8, 1, 1)}, "top of NB=8, H=8")),
    ((129, 48, 4, 7), ({F32: (13, 2, 1), F16: (13, 2, 0)}, "bottom of NB=13 in the general (A != 16) form")),
    ((208, 64, 4, 16), ({}, "top of NB=13; f16 forward k still in registers")),
    ((209, 64, 4, 16), ({}, "first NB=32 shape; f16 forward k out of registers")),
    ((300, 48, 4, 16), ({F32: (32, 1, 0), F16: (32, 2, 0)}, "NC=3 at NB=32")),
    ((384, 32, 4, 16), ({F32: (32, 1, 0), F16: (32, 2, 1)}, "last f32-supported F at H=4 (158,720 B); f16 at 161,792 B")),
    ((512, 16, 1, 16), ({F32: (32, 2, 0), F16: (32, 1, 1)}, "menu end, one head")),
    ((512, 16, 2, 16), ({F32: (32, 2, 1), F16: (32, 2, 0)}, "menu end, two heads")),
    # the (NB, NC) pairs of the backward menu that no edge above lands on
    ((40, 40, 2, 16), ({}, "NB=4 x NC=3")),
    ((33, 64, 2, 4), ({}, "NB=4 x NC=4")),
    ((80, 16, 3, 16), ({}, "NB=8 x NC=1")),
    ((100, 32, 2, 5), ({}, "NB=8 x NC=2")),
    ((97, 64, 1, 16), ({}, "NB=8 x NC=4")),
    ((130, 16, 2, 9), ({}, "NB=13 x NC=1, general form")),
    ((150, 32, 3, 16), ({}, "NB=13 x NC=2")),
])
F16_ONLY_CASES = collections.OrderedDict([
    ((400, 48, 2, 16), ({}, "f16: dynamic LDS equal to LDS_CAP exactly (163,328 B); the launch must succeed")),
    ((208, 64, 8, 16), ({F16: (13, 1, 0)}, "f16: last supported F at H=8, K=64")),
    ((400, 16, 8, 1), ({F16: (32, 1, 0)}, "f16: H=8, A=1 at NB=32")),
])
# exact LDS bytes of the backward the table above promises (without knobs)
BWD_LDS_BYTES = {((384, 32, 4, 16), F32): 158720, ((384, 32, 4, 16), F16): 161792, ((400, 48, 2, 16), F16): LDS_CAP}

# past the LDS limit: (F, K, H, A), precision -> (forward refused, backward refused)
REFUSED = collections.OrderedDict([
    (((129, 16, 8, 16), F32), (False, True)),
    (((209, 64, 8, 16), F16), (False, True)),
    (((400, 16, 8, 1), F32), (True, True)),
    (((512, 64, 4, 16), F32), (True, True)),
])

# first F at which a direction is refused: (K, H, precision, direction) -> F  (the figures of include/fil.h and of the layer's docstring)
FIRST_REFUSED_F = {(16, 8, F32, "fwd"): 241, (16, 8, F32, "bwd"): 129, (16, 6, F32, "bwd"): 225, (16, 5, F32, "bwd"): 289,
                   (16, 4, F32, "bwd"): 385, (16, 4, F32, "fwd"): 497, (64, 8, F16, "bwd"): 209, (64, 4, F16, "bwd"): 481}


def shape_case_list():
    """[((F, K, H, A), precision name)] of every pair that runs (REFUSED pairs are the others)."""
    out = [(s, p) for s in SHAPE_CASES for p in PRECISIONS]
    return out + [(s, "f16_mfma") for s in F16_ONLY_CASES]


def expected_tuple(shape, precision):
    table = SHAPE_CASES.get(shape) or F16_ONLY_CASES.get(shape)
    return None if table is None else table[0].get(PRECISIONS[precision] if isinstance(precision, str) else precision)


# option subset, value edges
OPTION_SHAPES = [(65, 33, 2, 8), (129, 48, 4, 7)]
VALUE_SHAPES = [(39, 16, 3, 8), (129, 48, 4, 7)]

# head-major input: (x_chunk, K)
HEAD_MAJOR = [(1, 8), (3, 12), (5, 10), (16, 48)]

# several samples per workgroup: B = MULTI_B = MULTI_PERIOD distinct samples repeated; one case per NB, and one with more than 1024
# dgamma / dbeta partial blocks (grid * wph * H)
MULTI_B, MULTI_PERIOD = 1025, 5
MULTI_CASES = collections.OrderedDict([((17, 17, 1, 16), 4), ((65, 33, 2, 8), 8), ((129, 48, 4, 7), 13), ((209, 16, 2, 16), 32), ((17, 8, 8, 4), 4)])

# attn_reduce_kernel: partial sets = B at (5, 4, 2, 4) (one workgroup per sample, one wave per head): the four-way unrolled loop takes
# wave w's sets w, w + 16, w + 32, w + 48 while p + 48 < parts, then single steps
REDUCE_SHAPE = (5, 4, 2, 4)
REDUCE_B = [1, 2, 15, 16, 17, 48, 49, 50, 63, 64, 65, 113]
REDUCE_N = collections.OrderedDict([((4, 1, 8), 32), ((4, 1, 16), 64), ((13, 5, 1), 65)])      # (K, H, A) -> n = K H A, 64 columns per block

NAN_B = 1030          # value edge 4: a periodic batch in which every workgroup takes two samples (some three)
KNOB_MIN_F = 129      # the knob children run the shape cases with F >= this


def bwd_grid_bounds(B, wph):
    """(fewest, most) persistent workgroups a backward of B samples can have -- the occupancy query decides inside this range."""
    cap_hi = 1024 // wph
    lo_cap = min(cap_hi, 256)
    def grid(cap):
        rounds = cdiv(B, cap)
        return max(1, cdiv(B, max(rounds, 1)))
    return grid(lo_cap), grid(cap_hi)
