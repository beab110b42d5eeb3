"""Poisoned inputs and guarded outputs for tests that call the C ABI directly on flat tensors (tests/test_fm_edges_gpu.py,
tests/test_dcn_edges_gpu.py, tests/test_head_edges_gpu.py, tests/test_pattn_edges_gpu.py, tests/test_attn_edges_gpu.py).  Every payload starts 16-byte aligned: an input at
the start of its allocation with TAIL words of the payload NaN behind it (a read past the end turns up in the results), an output GUARD_BYTES into a sentinel-filled allocation whose words in front
of and behind the payload must hold the sentinel's bits after the call.  Words are uint32 (fp32) or uint16 (bf16)."""
import numpy as np
import torch

SENTINEL = 0x7FC12345                      # a quiet NaN with a payload: compared as bits; its upper half 0x7FC1 is the bf16 sentinel
GUARD_BYTES = 256                          # in front of and behind every output
TAIL = 64                                  # poisoned words behind every input
WS_GUARD = 256                             # bytes behind a workspace
WS_FILL = 0xA5
WS_NAN_FILL = 0xFF                         # all-ones words: a NaN in fp32 and in bf16, so a partial read past the written ones shows in the sum

_SIGNED = {np.dtype(np.uint32): (np.int32, torch.int32), np.dtype(np.uint16): (np.int16, torch.int16)}


def sentinel(npw):
    return SENTINEL if np.dtype(npw) == np.uint32 else SENTINEL >> 16


def f32_words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poisoned_input(words):
    """words (uint32 / uint16 array) -> device tensor: the payload at the start of the allocation, TAIL poisoned words behind it."""
    buf = np.concatenate([words.ravel(), np.full(TAIL, sentinel(words.dtype), words.dtype)])
    return torch.from_numpy(buf.view(_SIGNED[words.dtype][0])).cuda()


class GuardedOutput:
    def __init__(self, shape, npw, name):
        self.shape, self.name, self.n, self.npw = shape, name, int(np.prod(shape)), np.dtype(npw)
        self.guard = GUARD_BYTES // self.npw.itemsize
        self.t = torch.full((2 * self.guard + self.n,), sentinel(npw), dtype=_SIGNED[self.npw][1], device="cuda")
        self.ptr = self.t.data_ptr() + GUARD_BYTES

    def read(self, what):
        """-> the payload's words; both guards must still hold the sentinel."""
        w = self.t.cpu().numpy().view(self.npw)
        stray = np.nonzero(np.concatenate([w[:self.guard], w[self.guard + self.n:]]) != sentinel(self.npw))[0]
        assert stray.size == 0, "%s: %d guard words of %s were written (guard word indices %s)" % (what, stray.size, self.name, stray[:8])
        return w[self.guard:self.guard + self.n].reshape(self.shape).copy()


def workspace(nbytes, fill=WS_FILL):
    """nbytes of workspace and WS_GUARD bytes behind them, every byte `fill` (WS_FILL: -2.9e-16 as an fp32 word; WS_NAN_FILL: a NaN)."""
    return torch.full((nbytes + WS_GUARD,), fill, dtype=torch.uint8, device="cuda")


def assert_workspace_guard(ws, nbytes, what, fill=WS_FILL):
    assert (ws[nbytes:].cpu().numpy() == fill).all(), "%s: a store behind the workspace's %d bytes" % (what, nbytes)


def bf16_words(a):
    """fp32 values -> their bf16 words, rounded to nearest even (exact where the values are bf16 values already)."""
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16).copy()


def words_f32(words):
    """The fp32 values that uint32 (fp32) or uint16 (bf16) words stand for."""
    return words.view(np.float32) if words.dtype == np.uint32 else (words.astype(np.uint32) << 16).view(np.float32)
