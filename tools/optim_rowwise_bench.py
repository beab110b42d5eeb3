"""The Keras Adagrad / Ftrl table step alone (include/fil.h O2), per table size, against what a user would write otherwise.

    python tools/optim_rowwise_bench.py [--iters 20]          (GPU box; output: profiles/r10_optim_rowwise_bench.txt)
    rocprofv3 --kernel-trace --stats -- python tools/optim_rowwise_bench.py --sizes criteo-size --iters 10
                                                          (per-kernel totals: profiles/r10_optim_rowwise_kernel_stats.csv)

Tables as tools/optim_bench.py builds them (K = 16, B = 4096, F = 39, zipf ids, one concatenated table): 0.6 M, 4.85 M and 33.8 M rows.
Paths per rule:
  all-l2        optim.Adagrad / optim.Ftrl, every field regularised (emb_reg 1e-8, make_sparse_info's default): fil_embed_rowopt_runs
                + fil_embed_rowopt_sweep over every untouched row (+ the counter launch)
  no-l2         the same with no field regularised: fil_embed_rowopt_runs only (Keras' IndexedSlices rows; no sweep, no stamps)
  torch         the table's dense gradient (zeros + fil_embed_run_sum_dt) and then
                  Adagrad: torch.optim.Adagrad(initial_accumulator_value=0.1, eps=1e-7) (foreach; not capturable: eager only) and the
                           same arithmetic as captured torch element-wise ops ("torch-ops")
                  Ftrl:    an element-wise torch restatement of ApplyFtrl on the dense gradient (torch has no Ftrl)
  sweep         fil_embed_rowopt_sweep alone over the whole table (no row stamped)
Times are CUDA-event means over --iters steps, eager and replayed from a HIP graph.  "bytes" = the DRAM traffic the path must move at
least: the sweep reads and writes p and the accumulator (Adagrad, 4 passes) or p, n and z (Ftrl, 6 passes) and reads the int32 stamps;
no-l2 moves the touched rows' arrays and the gradient block; torch writes the zero gradient and then reads p, g and the slots and
writes p and the slots (Adagrad 6 passes, Ftrl 8).  "of 6.3 TB/s" = bytes / replay time / 6.3e12."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, optim  # noqa: E402
from ml_function_amd._lib import FIL_OPT_ADAGRAD, FIL_OPT_FTRL, RowoptHyper, check, ptr, stream_ptr  # noqa: E402
from optim_bench import B, F, HBM, K, replayed, timed, vocab_of  # noqa: E402

LR, L1, L2 = 1e-3, 1e-3, 0.0


def table_paths(vocab, iters, out):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2020)
    V = sum(vocab)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(vocab)[:-1]]), dtype=torch.int64, device=dev)
    sizes = torch.tensor(vocab, dtype=torch.int64, device=dev)
    idx = torch.tensor(np.stack([np.minimum(rng.zipf(1.1, B) - 1, v - 1) for v in vocab], 1), device=dev)
    g = torch.randn(B, F, K, device=dev) * 1e-2
    sorted_ids, perm = Fn._sorted_row_ids(offs, sizes, None, idx, ("bench", tuple(vocab)), V, per_field=True)
    touched = int(torch.unique(sorted_ids[sorted_ids >= 0]).numel())
    field_l2 = torch.full((F,), 1e-8, dtype=torch.float32, device=dev)
    lib = _lib.load()
    table_bytes = 4.0 * V * K
    res = []

    def ours(rule, l2):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        p._fil_runs_table = True
        opt = (optim.Adagrad([p]) if rule == FIL_OPT_ADAGRAD
               else optim.Ftrl([p], learning_rate=LR, l1_regularization_strength=L1, l2_regularization_strength=L2))
        rec = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None,
                   field_l2=field_l2 if l2 else None)

        def step():
            p._fil_pending_runs = rec
            opt.step()
        arrays = 2 if rule == FIL_OPT_ADAGRAD else 3
        by = (2 * arrays * table_bytes + 4.0 * V) if l2 else (touched * K * 4.0 * 2 * arrays + B * F * K * 4.0)
        return step, by, (p, opt)

    def sweep_only(rule):
        p = torch.randn(V, K, device=dev) * 0.05
        acc = torch.full((V, K), 0.1, device=dev)
        lin = torch.zeros((V, K), device=dev) if rule == FIL_OPT_FTRL else None
        stamp = torch.zeros(V, dtype=torch.int32, device=dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        h = RowoptHyper(LR, 1e-7, -0.5, L1, L2, 0.0)
        import ctypes

        def step():
            check(lib.fil_embed_rowopt_sweep(ptr(p), ptr(acc), ptr(lin), ptr(stamp), V, K, ptr(offs), ptr(field_l2), None, F, ptr(t),
                                             rule, ctypes.addressof(h), stream_ptr()), "fil_embed_rowopt_sweep")
        arrays = 2 if rule == FIL_OPT_ADAGRAD else 3
        return step, 2 * arrays * table_bytes + 4.0 * V, (p, acc, lin, stamp, t, h)

    def dense_grad(p):
        dt = torch.zeros_like(p)
        check(lib.fil_embed_run_sum_dt(ptr(g), ptr(perm), ptr(sorted_ids), ptr(dt), B * F, K, 0, stream_ptr()), "run_sum")
        return dt

    def torch_adagrad():
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        opt = torch.optim.Adagrad([p], lr=LR, initial_accumulator_value=0.1, eps=1e-7, foreach=True)

        def step():
            p.grad = dense_grad(p)
            opt.step()
            p.grad = None
        return step, 6 * table_bytes, (p, opt)

    def torch_adagrad_ops():
        p = torch.randn(V, K, device=dev) * 0.05
        acc = torch.full((V, K), 0.1, device=dev)

        def step():
            dt = dense_grad(p)
            acc.addcmul_(dt, dt)
            p.addcdiv_(dt, acc.sqrt().add_(1e-7), value=-LR)
        return step, 6 * table_bytes, (p, acc)

    def torch_ftrl():
        p = torch.randn(V, K, device=dev) * 0.05
        n = torch.full((V, K), 0.1, device=dev)
        z = torch.zeros((V, K), device=dev)

        def step():
            dt = dense_grad(p)
            n1 = n + dt * dt
            s1 = n1.sqrt()
            z.add_(dt - (s1 - n.sqrt()) / LR * p)
            q = s1 / LR + 2 * L2
            p.copy_(torch.where(z.abs() > L1, (torch.sign(z) * L1 - z) / q, torch.zeros_like(z)))
            n.copy_(n1)
        return step, 8 * table_bytes, (p, n, z)

    makers = [("adagrad all-l2", lambda: ours(FIL_OPT_ADAGRAD, True), True),
              ("adagrad no-l2", lambda: ours(FIL_OPT_ADAGRAD, False), True),
              ("adagrad sweep", lambda: sweep_only(FIL_OPT_ADAGRAD), True),
              ("torch Adagrad", torch_adagrad, False),
              ("torch-ops Adagrad", torch_adagrad_ops, True),
              ("ftrl all-l2", lambda: ours(FIL_OPT_FTRL, True), True),
              ("ftrl no-l2", lambda: ours(FIL_OPT_FTRL, False), True),
              ("ftrl sweep", lambda: sweep_only(FIL_OPT_FTRL), True),
              ("torch-ops Ftrl", torch_ftrl, True)]
    for name, make, capturable in makers:
        step, by, keep = make()
        te = timed(step, iters)
        tr = replayed(step, iters) if capturable else None
        res.append((name, te, tr, by))
        del keep, step
        torch.cuda.empty_cache()
    out.append("table %s rows x K=%d (%.2f GB per array), B=%d F=%d, %d touched rows" % (format(V, ","), K, table_bytes / 1e9, B, F,
                                                                                         touched))
    out.append("  %-20s %10s %10s %12s %14s" % ("path", "eager ms", "replay ms", "bytes (GB)", "of 6.3 TB/s"))
    for name, te, tr, by in res:
        if tr is None:
            out.append("  %-20s %10.3f %10s %12.3f %14s" % (name, te, "n/a", by / 1e9, "(eager) %.2f" % (by / (te * 1e-3) / HBM)))
        else:
            out.append("  %-20s %10.3f %10.3f %12.3f %14.2f" % (name, te, tr, by / 1e9, by / (tr * 1e-3) / HBM))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="bench,criteo-like,criteo-size")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = ["Keras Adagrad / Ftrl table step (tools/optim_rowwise_bench.py, --iters %d); %s" % (args.iters, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for name in args.sizes.split(","):
        out = []
        table_paths(vocab_of(name), args.iters, out)
        print("\n".join(out), flush=True)
        lines += out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

if __name__ == "__main__":
    main()
