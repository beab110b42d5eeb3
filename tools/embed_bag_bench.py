"""Pooled multi-valued fields (fil_embed_bag_fwd and its gradient record) beside the ways to get the same numbers without them.

    python tools/embed_bag_bench.py [--iters 50] [--windows 5]          (GPU box; output: profiles/r23_embed_bag_bench.txt)

Shape: B = 4096 samples, F = 4 pooled fields of T = 50 slots, K = 16, 2 M rows per field (one concatenated 8 M-row table, 512 MB:
larger than the 256 MB Infinity Cache), ids uniform over each field's rows 1 .. V-1 (0 is the padding id).  Two batches: FULL bags
(every slot live) and RAGGED bags (a uniform length 1 .. T per bag, the rest padding at the end).
  1. forward       fil_embed_bag_fwd (mean) beside fil_embed_gather_dt on the same ids viewed as [B, F T]: the gather reads the same
                   rows (for ragged bags also row 0 for every padding slot) and writes T times the bytes.
  2. fwd + bwd     functional.embed_bag(mean) with its dense table gradient, beside
                     restated       embed_gather of [B, F T] + mask + sum + divide in torch, dense table gradient through autograd;
                     embedding_bag  torch.nn.functional.embedding_bag(mode="mean", padding_idx=0), one call and one table per field
                                    (its backward is not deterministic and is not captured: that pair is timed as eager calls).
  3. DeepFM step   a whole captured training step (13 dense columns + the four pooled fields with linear terms, MLP 256-128-64,
                   binary cross-entropy, optim.Adam in Keras mode): the bag tables in runs mode (updated in place from the record)
                   beside the restated pooling with a dense table gradient.
Every other timing is a replay of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window by
window; reported: the median window's time per replay and the spread (min .. max) over the windows."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, layers, losses, models, optim  # noqa: E402
from ml_function_amd._lib import check, ptr, stream_ptr  # noqa: E402

B, F, T, K, V = 4096, 4, 50, 16, 2_000_000


def batches(rng, dev):
    full = np.stack([rng.integers(1, V, (B, T)) for _ in range(F)], 1)
    ragged = full.copy()
    lengths = rng.integers(1, T + 1, (B, F))
    ragged[np.arange(T).reshape(1, 1, T) >= lengths[:, :, None]] = 0
    return {"full": torch.tensor(full, device=dev), "ragged": torch.tensor(ragged, device=dev)}, float(lengths.mean())


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


class Eager:
    """A variant that cannot be captured: timed as eager calls (launch and Python overhead included), and labelled so."""

    def __init__(self, fn):
        self.replay = fn


def compare(variants, iters, windows):
    """variants: [(name, fn or Eager(fn))] -> [(name, median ms, min ms, max ms)]; the graphs take turns window by window."""
    graphs = [(name, fn if isinstance(fn, Eager) else graph_of(fn)) for name, fn in variants]
    for _, g in graphs:
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in graphs}
    for _ in range(windows):
        for name, g in graphs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
    return [(name, float(np.median(t)), min(t), max(t)) for name, t in times.items()]


def report(out, rows):
    for name, med, lo, hi in rows:
        out.append("  %-34s %9.4f ms   (windows %.4f .. %.4f)" % (name, med, lo, hi))


def restated(table, offsets_x, sizes_x, idx):
    """embed_gather of the [B, F T] ids + mask + sum + divide: the pooling as torch ops (T times the bytes materialised)."""
    block = Fn.embed_gather(table, offsets_x, idx.view(B, F * T), sizes=sizes_x).view(B, F, T, K)
    live = idx != 0
    n = live.sum(2, keepdim=True).clamp(min=1).to(torch.float32)
    return (block * live.unsqueeze(-1)).sum(2) / n


def forward_rows(out, data, iters, windows, dev):
    lib = _lib.load()
    table = torch.randn(F * V, K, device=dev) * 0.05
    offsets = torch.arange(F, device=dev, dtype=torch.int64) * V
    sizes = torch.full((F,), V, device=dev, dtype=torch.int64)
    offsets_x, sizes_x = offsets.repeat_interleave(T), sizes.repeat_interleave(T)
    pooled = torch.empty(B, F, K, device=dev)
    count = torch.empty(B, F, dtype=torch.int32, device=dev)
    block = torch.empty(B, F * T, K, device=dev)
    for name, idx in data.items():
        def bag():
            check(lib.fil_embed_bag_fwd(ptr(table), ptr(offsets), ptr(sizes), ptr(idx), 0, ptr(pooled), ptr(count), None, B, F, T, K,
                                        _lib.FIL_BAG_MEAN, stream_ptr()), "fil_embed_bag_fwd")

        def gather():
            check(lib.fil_embed_gather_dt(ptr(table), ptr(offsets_x), ptr(sizes_x), ptr(idx), ptr(block), None, B, F * T, K, _lib.FIL_F32,
                                          stream_ptr()), "fil_embed_gather_dt")
        out.append("1. forward, %s bags:" % name)
        report(out, compare([("fil_embed_bag_fwd (mean)", bag), ("fil_embed_gather_dt [B, F T]", gather)], iters, windows))
    del table, block
    torch.cuda.empty_cache()


def train_rows(out, data, iters, windows, dev):
    offsets = torch.arange(F, device=dev, dtype=torch.int64) * V
    sizes = torch.full((F,), V, device=dev, dtype=torch.int64)
    offsets_x, sizes_x = offsets.repeat_interleave(T), sizes.repeat_interleave(T)
    g = torch.randn(B, F, K, device=dev) * 1e-3
    for name, idx in data.items():
        table = torch.nn.Parameter(torch.randn(F * V, K, device=dev) * 0.05)
        per_field = [torch.nn.Parameter(table.detach()[f * V:(f + 1) * V].clone()) for f in range(F)]
        cols = [idx[:, f].contiguous() for f in range(F)]

        def bag():
            table.grad = None
            Fn.embed_bag(table, offsets, idx, sizes=sizes, combiner="mean").backward(g)

        def torch_restated():
            table.grad = None
            restated(table, offsets_x, sizes_x, idx).backward(g)

        def torch_embedding_bag():
            for f in range(F):
                per_field[f].grad = None
                torch.nn.functional.embedding_bag(cols[f], per_field[f], mode="mean", padding_idx=0).backward(g[:, f])
        out.append("2. forward + dense table gradient, %s bags:" % name)
        # (embedding_bag's backward is kept out of a capture here: it runs eager, and embed_bag runs eager beside it for a
        # like-for-like pair)
        report(out, compare([("embed_bag (mean)", bag), ("restated (gather+mask+sum+div)", torch_restated),
                             ("embed_bag (mean), eager", Eager(bag)), ("F.embedding_bag per field, eager", Eager(torch_embedding_bag))],
                            iters, windows))
        del table, per_field
        torch.cuda.empty_cache()


class RestatedBagEmbed(layers.BagEmbed):
    """BagEmbed's table and interface with the pooling restated in torch (mean, padding id 0) and a dense table gradient."""

    def call(self, idx, **kwargs):
        k = self.embeddings.shape[1]
        block = Fn.embed_gather(self.embeddings, self.offsets.repeat_interleave(T), idx.view(B, F * T),
                                sizes=self.sizes.repeat_interleave(T)).view(B, F, T, k)
        live = idx != 0
        n = live.sum(2, keepdim=True).clamp(min=1).to(torch.float32)
        pooled = (block * live.unsqueeze(-1)).sum(2) / n
        return list(pooled.split(1, dim=1))


def model_rows(out, data, iters, windows, dev):
    rng = np.random.default_rng(2021)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = models.make_seq_info([V] * F, T, embed_dim=K)
    info = [i._replace(emb_reg=0.0) for i in info]
    for name, idx in data.items():
        steps, keep = [], []
        for variant in ("bag, runs mode", "restated, dense gradient"):
            torch.manual_seed(0)
            runs = variant.startswith("bag")
            fi = models.FeatureInput(denseInfo=[models.denseFea("I%d" % i, None) for i in range(13)], seqInfo=info, useLinear=True,
                                     tableGrad="runs" if runs else "dense")
            if not runs:
                fi.seq_embed = RestatedBagEmbed(info)
                fi.seq_linear_embed = RestatedBagEmbed(info, is_linear=True)
            model = models.CTRModel(fi, models.DeepFM()).to(dev)
            model(dense, None, idx)
            opt = optim.Adam(model.parameters())

            def step(model=model, opt=opt):
                opt.zero_grad(set_to_none=True)
                p = model(dense, None, idx)[:, 0]
                losses.binary_crossentropy(p, y, eps=1e-6).backward()
                opt.step()
            steps.append(("DeepFM step: " + variant, step))
            keep.append((model, opt))
        out.append("3. captured DeepFM training step (optim.Adam, Keras mode), %s bags:" % name)
        report(out, compare(steps, iters, windows))
        del steps, keep
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="1,2,3")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, mean_len = batches(np.random.default_rng(2020), dev)
    out = ["embed_bag_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d F=%d T=%d K=%d, %s rows per field (table %.0f MB), uniform ids; ragged bags: uniform length 1..T, mean %.1f live slots"
           % (B, F, T, K, format(V, ","), F * V * K * 4 / 1e6, mean_len),
           "HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters)]
    for part, fn in (("1", forward_rows), ("2", train_rows), ("3", model_rows)):
        if part in args.parts.split(","):
            out.append("")
            n = len(out)
            fn(out, data, args.iters, args.windows, dev)
            print("\n".join(out[n:]), flush=True)
    print("\n" + "\n".join(out))


if __name__ == "__main__":
    main()
