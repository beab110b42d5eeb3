"""The Keras SGD / RMSprop table step alone (include/fil.h O4), against optim.Adagrad's step and against what a user writes today.

    python tools/optim_momentum_bench.py [--iters 10 --windows 5]      (GPU box; output: profiles/r13_optim_momentum_bench.txt)
    rocprofv3 --kernel-trace --stats -- python tools/optim_momentum_bench.py --iters 5 --windows 1

One concatenated table as tools/optim_rowwise_bench.py builds it (K = 16, B = 4096, F = 39, zipf ids; default: 33.8 M rows).  Paths:
  <variant> all-l2   optim.SGD / optim.RMSprop, every field regularised (emb_reg 1e-8): fil_embed_momopt_runs + fil_embed_momopt_sweep
                     over every untouched row with the full rule
  <variant> no-l2    no field regularised: fil_embed_momopt_runs only for the row-local variants; for RMSprop with momentum == 0 also
                     the decay-only sweep (rms *= rho on every untouched row: one read and one write of rms)
  adagrad ...        optim.Adagrad, the reference point of the same run
  torch SGD/RMSprop  the table's dense gradient (zeros + fil_embed_run_sum_dt), then torch.optim.SGD / RMSprop (foreach; eager) and the
                     same arithmetic as captured torch element-wise ops ("torch-ops")
Every path is captured into a HIP graph and replayed: --windows windows of --iters replays each, the median window and the spread
(min - max) are printed; "eager" is one window of eager steps.  "bytes" = the DRAM traffic the path must move at least: a full-rule
sweep reads and writes p and the variant's slots and reads the int32 stamps; the decay-only sweep reads and writes rms and reads the
stamps; a runs-only step moves the touched rows' arrays and the gradient block; torch writes the zero gradient, then reads p, g and
the slots and writes p and the slots.  "of 6.3 TB/s" = bytes / median replay time / 6.3e12."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, optim  # noqa: E402
from ml_function_amd._lib import check, ptr, stream_ptr  # noqa: E402
from optim_bench import B, F, HBM, K, timed, vocab_of  # noqa: E402

LR = 1e-3
VARIANTS = [("sgd", lambda ps: optim.SGD(ps, learning_rate=LR), 0),
            ("sgd-momentum", lambda ps: optim.SGD(ps, learning_rate=LR, momentum=0.9), 1),
            ("sgd-nesterov", lambda ps: optim.SGD(ps, learning_rate=LR, momentum=0.9, nesterov=True), 1),
            ("rmsprop", lambda ps: optim.RMSprop(ps, learning_rate=LR), 1),
            ("rmsprop-momentum", lambda ps: optim.RMSprop(ps, learning_rate=LR, momentum=0.9), 2),
            ("adagrad", lambda ps: optim.Adagrad(ps, learning_rate=LR), 1)]


def windows(fn, iters, n):
    """n windows of iters calls each: (median, min, max) ms per call."""
    ts = [timed(fn, iters) for _ in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def replay_windows(fn, iters, n):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return windows(g.replay, iters, n)


def table_paths(vocab, iters, nwin, out):
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

    def ours(make, slots, l2, decay_only):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        p._fil_runs_table = True
        opt = make([p])
        rec = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None,
                   field_l2=field_l2 if l2 else None)

        def step():
            p._fil_pending_runs = rec
            opt.step()
        arrays = 1 + slots
        runs_bytes = touched * K * 4.0 * 2 * arrays + B * F * K * 4.0
        if l2:
            by = 2 * arrays * table_bytes + 4.0 * V
        elif decay_only:
            by = 2 * table_bytes + 4.0 * V + runs_bytes
        else:
            by = runs_bytes
        return step, by, (p, opt)

    def dense_grad(p):
        dt = torch.zeros_like(p)
        check(lib.fil_embed_run_sum_dt(ptr(g), ptr(perm), ptr(sorted_ids), ptr(dt), B * F, K, 0, stream_ptr()), "run_sum")
        return dt

    def torch_opt(kind):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        opt = (torch.optim.SGD([p], lr=LR, momentum=0.9, foreach=True) if kind == "sgd"
               else torch.optim.RMSprop([p], lr=LR, alpha=0.9, eps=1e-7, foreach=True))

        def step():
            p.grad = dense_grad(p)
            opt.step()
            p.grad = None
        return step, 6 * table_bytes, (p, opt)

    def torch_ops(kind):
        p = torch.randn(V, K, device=dev) * 0.05
        s = torch.zeros((V, K), device=dev)

        def step():
            dt = dense_grad(p)
            if kind == "sgd":
                s.mul_(0.9).add_(dt, alpha=-LR)
                p.add_(s)
            else:
                s.mul_(0.9).addcmul_(dt, dt, value=0.1)
                p.addcdiv_(dt, s.sqrt().add_(1e-7), value=-LR)
        return step, 6 * table_bytes, (p, s)

    makers = []
    for name, make, slots in VARIANTS:
        makers.append((name + " all-l2", lambda make=make, slots=slots: ours(make, slots, True, False), True))
        makers.append((name + " no-l2", lambda make=make, slots=slots, name=name: ours(make, slots, False, name == "rmsprop"), True))
    makers += [("torch SGD(0.9)", lambda: torch_opt("sgd"), False), ("torch-ops SGD(0.9)", lambda: torch_ops("sgd"), True),
               ("torch RMSprop", lambda: torch_opt("rms"), False), ("torch-ops RMSprop", lambda: torch_ops("rms"), True)]
    for name, make, capturable in makers:
        step, by, keep = make()
        te = timed(step, iters)
        tr = replay_windows(step, iters, nwin) if capturable else None
        res.append((name, te, tr, by))
        del keep, step
        torch.cuda.empty_cache()
    out.append("table %s rows x K=%d (%.2f GB per array), B=%d F=%d, %d touched rows" % (format(V, ","), K, table_bytes / 1e9, B, F,
                                                                                         touched))
    out.append("  %-26s %9s %10s %19s %11s %12s" % ("path", "eager ms", "replay ms", "spread (min - max)", "bytes (GB)", "of 6.3 TB/s"))
    for name, te, tr, by in res:
        if tr is None:
            out.append("  %-26s %9.3f %10s %19s %11.3f %12s" % (name, te, "n/a", "", by / 1e9, "(eager) %.2f" % (by / (te * 1e-3) / HBM)))
        else:
            out.append("  %-26s %9.3f %10.3f %19s %11.3f %12.2f" % (name, te, tr[0], "%.3f - %.3f" % (tr[1], tr[2]), by / 1e9,
                                                                    by / (tr[0] * 1e-3) / HBM))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sizes", default="criteo-size")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = ["Keras SGD / RMSprop table step (tools/optim_momentum_bench.py, --iters %d --windows %d); %s"
             % (args.iters, args.windows, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for name in args.sizes.split(","):
        out = []
        table_paths(vocab_of(name), args.iters, args.windows, out)
        print("\n".join(out), flush=True)
        lines += out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
