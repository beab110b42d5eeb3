"""What the CIN launcher tells its callers, as a table: fil_cin_saved_bytes, fil_cin_fwd_workspace_bytes, fil_cin_bwd_workspace_bytes,
fil_cin_grad_ready_points (modes 0, 32, 64, 64|256, 64|512, 1) and fil_cin_precision_used (both precisions) for every shape of
tests/test_gpu_parity.py's CIN_SHAPES and TAIL_SHAPES, each also at B = 0, 1024 and 4096, and the two benchmark shapes.  No GPU needed.

    python tools/cin_layout_table.py > a.txt;  FIL_LIB_PATH=tools/abl/libfil_<name>.so python tools/cin_layout_table.py > b.txt;  diff a.txt b.txt

(a host-side refactor of csrc/cin.hip must leave every row as it is: profiles/r17_cin_layout_sizes.txt)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ml_function_amd import _lib  # noqa: E402
from tests.test_gpu_parity import CIN_SHAPES, TAIL_SHAPES  # noqa: E402

MODES = (0, 32, 64, 64 | 256, 64 | 512, 1)


def main():
    lib = _lib.load()
    shapes = []
    for B, F, K, H in CIN_SHAPES + TAIL_SHAPES:
        for b in (B, 0, 1024, 4096):
            if (b, F, K, H) not in shapes:
                shapes.append((b, F, K, H))
    shapes += [(4096, 39, 16, [200] * 3), (8192, 39, 16, [128] * 3)]
    print("%-34s %14s %14s %14s  %s" % ("B F K H", "saved", "fwd_ws", "bwd_ws", "per mode %s: ready points / precision_used(DEFAULT, BF16)" % (MODES,)))
    for B, F, K, H in shapes:
        L, Harr = len(H), _lib.int_array(H)
        cells = []
        for mode in MODES:
            pts = (ctypes.c_int * (L + 1))()
            n = lib.fil_cin_grad_ready_points(B, F, K, L, Harr, mode, pts)
            cells.append("%d:%s/%d%d" % (n, ",".join(str(v) for v in pts), lib.fil_cin_precision_used(B, F, K, L, Harr, mode, 0),
                                         lib.fil_cin_precision_used(B, F, K, L, Harr, mode, 1)))
        print("%-34s %14d %14d %14d  %s" % ("%d %d %d %s" % (B, F, K, "x".join(map(str, H))), lib.fil_cin_saved_bytes(B, F, K, L, Harr),
                                            lib.fil_cin_fwd_workspace_bytes(B, F, K, L, Harr), lib.fil_cin_bwd_workspace_bytes(B, F, K, L, Harr), "  ".join(cells)))


if __name__ == "__main__":
    main()
