"""The cases of tests/test_ts_gru_gpu.py, kept apart from it so that tests/test_ts_gru_host.py can check on the CPU what they are a
condition for: every case's E32 (the fp32 torch restatement's own error) is finite and every bar max(1e-5, 4 E32) is below 1e-3, so
that a bar cannot hide a wrong kernel.  A shape that fails that check gets another seed here, never another bar."""
import functools

import numpy as np

from tests import ts_gru_ref as ref

# (B, T, K, H, S)
PARITY_SHAPES = [(1, 1, 4, 4, 1),          # the minimum
                 (3, 2, 4, 8, 2),          # small
                 (5, 50, 16, 16, 2),       # the benchmark's
                 (3, 5, 24, 24, 3),        # NR = 16
                 (3, 7, 12, 20, 1),        # K / 4 and H / 4 odd, K != H
                 (2, 40, 8, 4, 8)]         # many substeps, narrow state
CORNERS = [(2, 5, 64, 4, 2), (2, 5, 4, 64, 2)]
EDGE = (3, 4, 8, 2)                        # T, K, H, S of the tile-edge cases
LARGE = (4, 6, 8, 12, 2)
SEEDS = {}                                 # shape -> the seed in place of 0, where seed 0 fails the check above


def largest_square():
    """The largest K = H the plan admits at B = 3, T = 6, S = 2 (the LDS edge of the menu)."""
    from ml_function_amd import functional as Fn
    return max(kh for kh in range(4, 65, 4) if Fn.ts_gru_plan(3, 6, kh, kh, 2)["fits"])


@functools.lru_cache(maxsize=None)
def case_of(shape, seed=None, mask="ragged", out=True, seq=True):
    """seq: the op runs return_sequences=True and every upstream gradient is given; else g_last and g_z."""
    seed = SEEDS.get(shape, 0) if seed is None else seed
    return ref.make_case(*shape, seed, mask=mask, out=out, grads=("hs", "last", "z") if seq else ("last", "z"))


@functools.lru_cache(maxsize=None)
def edge_case(B):
    """A few samples of three steps: the seed is the first whose sums are well conditioned in the fp64 reference
    (ts_gru_ref.conditioned_case; the seed is printed by the tests)."""
    return ref.conditioned_case(B, *EDGE)


@functools.lru_cache(maxsize=None)
def large_case(seed=0):
    """x, W, U times 8 (saturated gates, as tests/seq_value_cases.py does for the GRU) and every gap 1e3."""
    case = ref.make_case(*LARGE, seed, mask="prefix")
    B, T = LARGE[:2]
    return dict(case, x=case["x"] * 8, W=case["W"] * 8, U=case["U"] * 8, dt=np.full((B, T), 1e3), dt_out=np.full(B, 1e3))


def parity_cases(kh):
    """Every case of the parity test, with kh = largest_square()."""
    for shape in PARITY_SHAPES + CORNERS + [(3, 6, kh, kh, 2)]:
        for out in (True, False):
            for seq in (True, False):
                yield case_of(shape, out=out, seq=seq)
