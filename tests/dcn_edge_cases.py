"""The DCN dispatch of csrc/dcn.hip restated in Python, and the (B, D, L) tables built on it.  Shared by tests/test_dcn_edges_gpu.py (which
runs every case on the GPU and asserts the path it was built for) and tests/test_host.py (which holds fil_dcn_bwd_workspace_bytes to the
prediction without a GPU).  Needs neither torch nor the library.

    vec = D % 4 == 0;  npl = the first of 8, 20, 32, 64 with 64 npl >= D (and npl % 4 == 0 if vec), none for D > 4096
    forward   register-resident  <=>  L <= 6 and D <= 4096 and 2 L D 4 <= 163840 (w and b in LDS), else the generic pair (any D, L <= 16)
    backward  register-resident  <=>  L <= 6 and D <= 4096 and (L + 7) npl <= 230 and 4 max(L D, 8 (D + 8)) <= 163840, else generic
    generic kernels: instantiation LM = 6 for L <= 6, LM = 16 above
    grids     forward min(cdiv(B, 4), 1024) workgroups of 4 waves, backward min(cdiv(B, 8), 256) of 8 waves, one partial each;
              FIL_DCN_GRID = n > 0 (read once per process) replaces both caps
    generic   chunks = min(cdiv(B, 32), 64) sized in the workspace, nchunk = cdiv(B, chunks), cdiv(B, nchunk) partials reduced;
              scalars kernels: min(cdiv(B, 4), 512) workgroups forward, min(cdiv(B, 4), 2048) backward, 4 waves = 4 samples per trip
    workspace register: align256(grid ((L + 1) D + 8) 4);   generic: align256(4 B L) + align256(chunks 2 L D 4)
"""
import collections
import os

DCN_LDS_LIMIT = 160 * 1024
DCN_MAX_L = 6
DCN_GEN_MAX_L = 16

DcnPaths = collections.namedtuple("DcnPaths", "fwd bwd npl vec lm")      # fwd, bwd: "register" or "generic"; lm: the generic pair's LM


def cdiv(a, b):
    return (a + b - 1) // b


def align256(n):
    return cdiv(n, 256) * 256


def pick_npl(D, vec):
    for npl in (8, 20, 32, 64):
        if npl * 64 >= D and (not vec or npl % 4 == 0):
            return npl
    return -1


def dcn_paths(D, L):
    vec = D % 4 == 0
    npl = pick_npl(D, vec)
    fits = L <= DCN_MAX_L and D <= 4096 and npl > 0
    fwd = fits and 2 * L * D * 4 <= DCN_LDS_LIMIT
    bwd = fits and (L + 7) * npl <= 230 and max(L * D, 8 * (D + 8)) * 4 <= DCN_LDS_LIMIT
    return DcnPaths("register" if fwd else "generic", "register" if bwd else "generic", npl, vec, DCN_MAX_L if L <= DCN_MAX_L else DCN_GEN_MAX_L)


def forced_grid():
    """FIL_DCN_GRID as the library reads it (atoi; <= 0 or unset = no override)."""
    try:
        return max(int(os.environ.get("FIL_DCN_GRID", "0")), 0)
    except ValueError:
        return 0


def grid_bwd(B):
    return max(1, min(cdiv(B, 8), forced_grid() or 256))


def grid_fwd(B):
    return max(1, min(cdiv(B, 4), forced_grid() or 1024))


def generic_chunks(B):
    return max(1, min(cdiv(B, 32), 64))


def generic_parts(B):
    """(partials that dcn_reduce_kernel sums, samples in the last one)"""
    nchunk = cdiv(B, generic_chunks(B))
    parts = cdiv(B, nchunk)
    return parts, B - (parts - 1) * nchunk


def workspace_bytes(B, D, L):
    if dcn_paths(D, L).bwd == "register":
        return align256(grid_bwd(B) * ((L + 1) * D + 8) * 4)
    return align256(4 * B * L) + align256(generic_chunks(B) * 2 * L * D * 4)


# (B, D, L) -> (forward path, backward path, npl, vec) the case was built for
PATH_CASES = collections.OrderedDict([
    ((9, 512, 6), ("register", "register", 8, True)),       # npl 8 vector, no masked lane; the register backward at its deepest L
    ((9, 516, 4), ("register", "register", 20, True)),      # npl 20 vector, 129 of 320 chunks live; (4 + 7) 20 = 220 <= 230
    ((9, 516, 5), ("register", "generic", 20, True)),       # (5 + 7) 20 = 240: the generic backward consumes the register forward's s
    ((9, 513, 1), ("register", "register", 20, False)),     # npl 20 scalar
    ((9, 1280, 4), ("register", "register", 20, True)),     # npl 20 full
    ((7, 1281, 1), ("register", "generic", 32, False)),     # npl 32 scalar: (1 + 7) 32 = 256
    ((7, 1284, 2), ("register", "generic", 32, True)),      # npl 32 vector
    ((7, 2048, 5), ("register", "generic", 32, True)),      # npl 32 full
    ((5, 2052, 2), ("register", "generic", 64, True)),      # npl 64
    ((5, 4096, 5), ("register", "generic", 64, True)),      # npl 64 full; the forward's dynamic LDS = 163840 bytes exactly
    ((6, 5, 7), ("generic", "generic", 8, False)),          # L > 6: the LM = 16 instantiations
    ((6, 3, 16), ("generic", "generic", 8, False)),         # the deepest L
    ((5, 1, 3), ("register", "register", 8, False)),        # D below one vector
    ((5, 2, 3), ("register", "register", 8, False)),
    ((5, 3, 3), ("register", "register", 8, False)),
])

# register-resident grid cases: (B, D, 2) for D in REG_GRID_D; B -> partials of the backward = workgroups (without FIL_DCN_GRID)
REG_GRID_D = [8, 68]                                         # 68: two ragged 64-column blocks of dcn_reduce_closed_kernel
REG_GRID_L = 2
REG_GRID_B = collections.OrderedDict([(1, 1), (7, 1), (8, 1), (9, 2), (25, 4), (248, 31), (256, 32), (257, 33), (2053, 256), (4101, 256)])

# generic grid cases: (B, 5, 7); B -> partials of dcn_reduce_kernel
GEN_GRID_D, GEN_GRID_L = 5, 7
GEN_GRID_B = collections.OrderedDict([(20, 1), (64, 2), (160, 5), (288, 9), (2100, 64), (8200, 64)])

# the menu shapes with a register-resident direction once more at a ragged B: with FIL_DCN_GRID=2 every wave of the register kernels
# walks several samples, unequally (16 backward waves: 3 or 2 each; 8 forward waves: 5 or 4 each)
MENU_WALK_B = 37
MENU_WALK_DL = [(D, L) for (_, D, L), (fwd, bwd, _, _) in PATH_CASES.items() if "register" in (fwd, bwd)]

KNOB_MAX_B = 257                                             # the grid cases that the FIL_DCN_GRID=2 child runs as well

CONTAIN_CASES = [(2053, 8, 2), (2100, 5, 7)]


def all_cases():
    """Every (B, D, L) of the tables."""
    out = list(PATH_CASES)
    out += [(B, D, REG_GRID_L) for D in REG_GRID_D for B in REG_GRID_B]
    out += [(B, GEN_GRID_D, GEN_GRID_L) for B in GEN_GRID_B]
    out += [(MENU_WALK_B, D, L) for D, L in MENU_WALK_DL]
    return out + [c for c in CONTAIN_CASES if c not in out]
