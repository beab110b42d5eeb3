"""The data-parallel runs exchange of optim.Adam on one GPU: its kernels, against today's data-parallel route and the one-GPU update.

    python tools/optim_dp_bench.py [--iters 20] [--out profiles/r08_optim_dp_bench.txt]     (GPU box)

One Criteo-shaped setting: F = 26 fields, K = 16, the 33.8 M-row table of tools/optim_bench.py (its criteo-like vocabulary draw,
26 fields, scaled to 33.8 M rows), zipf(1.1) ids, B = 4096 per rank.  For W simulated ranks a batch of W x 4096 rows is drawn and
cut into W shards of 4096; every shard leaves its own runs record (fil_embed_sort_fields).  Timed (CUDA-event means over --iters):
  compact            fil_embed_runs_compact of one shard (3 launches)
  merged W           fil_embed_adam_merged over the W shards' lists, gathered into one buffer on this GPU (Keras mode, with stamps)
  sweep              fil_embed_adam_sweep (the pass over the whole table that dominates the Keras step)
  exchange step W=1  optim.Adam(force_exchange=True).step(): compact + merged + sweep + the counter launch
  runs step          optim.Adam.step() on one GPU: fil_embed_adam_runs + sweep + the counter launch
  dense DP route     today's data-parallel route at world size 1: dense [V,K] zero fill + fil_embed_run_sum_dt + dp.exchange_sparse_rows
                     (torch.unique; no collective at one rank) + fil_adam_multi over the whole table
RCCL at W > 1 is NOT measured here (no multi-GPU hardware): the all-gather moves W x cap x (8 + 4 K) bytes + W x 8 per table."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, dp, functional as Fn, optim  # noqa: E402
from ml_function_amd._lib import check, ptr, stream_ptr  # noqa: E402

HBM = 6.3e12
B, F, K = 4096, 26, 16
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


def criteo_size_vocab():
    rng = np.random.default_rng(2020)
    w = np.exp(rng.uniform(np.log(10), np.log(1e6), F))
    return [max(10, int(v)) for v in w / w.sum() * 33.8e6]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r08_optim_dp_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    vocab = criteo_size_vocab()
    V = sum(vocab)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(vocab)[:-1]]), dtype=torch.int64, device=dev)
    sizes = torch.tensor(vocab, dtype=torch.int64, device=dev)
    worlds = [int(w) for w in args.worlds.split(",")]
    Wmax = max(worlds)
    rng = np.random.default_rng(2020)
    idx_all = torch.tensor(np.stack([np.minimum(rng.zipf(1.1, Wmax * B) - 1, v - 1) for v in vocab], 1), device=dev)
    g_all = torch.randn(Wmax * B, F, K, device=dev) * 1e-4
    recs = []
    for w in range(Wmax):
        idx, g = idx_all[w * B:(w + 1) * B].contiguous(), g_all[w * B:(w + 1) * B].contiguous()
        sorted_ids, perm = Fn._sorted_row_ids(offs, sizes, None, idx, ("dpbench", w), V, per_field=True)
        recs.append(dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None, field_l2=None,
                         idx=idx))
    R = B * F
    cap = R
    table = torch.randn(V, K, device=dev) * 0.05
    m, v = torch.zeros_like(table), torch.zeros_like(table)
    stamp = torch.zeros(V, dtype=torch.int32, device=dev)
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    ids = torch.empty(Wmax * cap, dtype=torch.int64, device=dev)
    values = torch.empty(Wmax * cap * K, dtype=torch.float32, device=dev)
    counts = torch.empty(Wmax, dtype=torch.int64, device=dev)
    ws = torch.empty(optim.runs_compact_workspace_bytes(R), dtype=torch.uint8, device=dev)

    def compact(w):
        optim.runs_compact(recs[w], K, ids[w * cap:(w + 1) * cap], values[w * cap * K:(w + 1) * cap * K], counts[w:w + 1], cap, ws)

    for w in range(Wmax):
        compact(w)
    torch.cuda.synchronize()
    n_unique = counts.cpu().tolist()
    out = ["optim_dp_bench: %s" % torch.cuda.get_device_name(0),
           "table %s rows x K=%d (%.2f GB per array), F=%d, B=%d per rank, zipf(1.1); distinct rows per shard: %s"
           % (format(V, ","), K, 4.0 * V * K / 1e9, F, B, ", ".join(str(c) for c in n_unique)),
           "times: CUDA-event means over %d iterations, eager launches" % args.iters, ""]
    t_compact = timed(lambda: compact(0), args.iters)
    by = R * K * 4.0 + R * 8 * 3 + n_unique[0] * (8 + 4 * K)
    out.append("  %-26s %9.3f ms   (reads g, perm, ids: %.1f MB; %.2f of 6.3 TB/s)" % ("compact (one shard)", t_compact, by / 1e6,
                                                                                       by / (t_compact * 1e-3) / HBM))

    def merged(W):
        optim.adam_merged(ids, values, counts, W, cap, offs, None, table, m, v, stamp, t, LR, B1, B2, EPS)
    t_merged = {}
    for W in worlds:
        t_merged[W] = timed(lambda: merged(W) if W > 1 else optim.adam_merged(ids[:cap], values[:cap * K], counts[:1], 1, cap, offs, None,
                                                                                table, m, v, stamp, t, LR, B1, B2, EPS), args.iters)
        union = int(torch.unique(torch.cat([ids[w * cap:w * cap + n_unique[w]] for w in range(W)])).numel())
        by = W * cap * 8.0 + sum(n_unique[:W]) * 4.0 * K + union * 24.0 * K + union * 4.0
        out.append("  %-26s %9.3f ms   (union %d rows; gathered lists + rows: %.1f MB)" % ("merged W=%d" % W, t_merged[W], union,
                                                                                          by / 1e6))
    t_sweep = timed(lambda: check(lib.fil_embed_adam_sweep(ptr(table), ptr(m), ptr(v), ptr(stamp), V, K, ptr(offs), None, None, F, ptr(t),
                                                           LR, B1, B2, EPS, stream_ptr()), "sweep"), args.iters)
    out.append("  %-26s %9.3f ms   (%.2f of 6.3 TB/s)" % ("sweep", t_sweep, (24.0 * V * K + 4.0 * V) / (t_sweep * 1e-3) / HBM))
    del table, m, v, stamp
    torch.cuda.empty_cache()
    out.append("")

    # whole optimizer steps (one table parameter)
    rec0 = {k: val for k, val in recs[0].items() if k != "idx"}

    def opt_step(force):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        opt = optim.Adam([p], force_exchange=force)

        def step():
            p._fil_pending_runs = rec0
            opt.step()
        return timed(step, args.iters), (p, opt)
    t_x, keep = opt_step(True)
    del keep
    torch.cuda.empty_cache()
    t_r, keep = opt_step(False)
    del keep
    torch.cuda.empty_cache()

    p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
    mm, vv = torch.zeros_like(p), torch.zeros_like(p)
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)
    rows = (recs[0]["idx"] + offs).reshape(-1)

    dt = torch.empty_like(p)
    desc = optim._Desc(p.data_ptr(), dt.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), 0.0, 0)
    d_desc = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)

    def dense_route():
        dt.zero_()
        check(lib.fil_embed_run_sum_dt(ptr(rec0["g"]), ptr(rec0["perm"]), ptr(rec0["sorted_ids"]), ptr(dt), R, K, 0, stream_ptr()), "rs")
        dp.exchange_sparse_rows(dt, rows)
        check(lib.fil_adam_multi(ptr(d_desc), 1, p.numel(), ptr(step_t), LR, B1, B2, EPS, 1, stream_ptr()), "adam_multi")
    t_d = timed(dense_route, args.iters)
    out.append("  %-26s %9.3f ms" % ("exchange step W=1", t_x))
    out.append("  %-26s %9.3f ms" % ("runs step (one GPU)", t_r))
    out.append("  %-26s %9.3f ms   (%.1fx the exchange step)" % ("dense DP route W=1", t_d, t_d / t_x))
    out.append("")
    out.append("  exchange overhead over the one-GPU step: %+.3f ms (%+.1f %%); compact + merged W=1 = %.3f ms = %.1f %% of the one-GPU step"
               % (t_x - t_r, 100.0 * (t_x - t_r) / t_r, t_compact + t_merged.get(1, float("nan")),
                  100.0 * (t_compact + t_merged.get(1, float("nan"))) / t_r))
    out.append("  NOT measured: the RCCL all-gather at W > 1 (no multi-GPU hardware); per table and step it moves W x %d x %d bytes"
               % (cap, 8 + 4 * K))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
