"""The Keras Adam(amsgrad=True) table step alone (include/fil.h O7), beside optim.Adam's of the same run -- the step it is by bytes 4/3
of: a sweep that reads and writes p, m, v and vhat of every row, 32 B per element, against Adam's 24 (28 where the vhat store is
skipped because vhat holds: every untouched row of an unregularised field) -- and against what a user writes otherwise.

    python tools/optim_amsgrad_bench.py [--iters 10 --windows 5]      (GPU box; output: profiles/r21_optim_amsgrad_bench.txt)
    rocprofv3 --kernel-trace --stats -- python tools/optim_amsgrad_bench.py --iters 5 --windows 1

One concatenated table as tools/optim_rowwise_bench.py builds it (K = 16, B = 4096, F = 39, zipf ids; default: 33.8 M rows).  Paths:
  amsgrad            optim.Adam(amsgrad=True), no field regularised: the runs update + the sweep of p, m, v and vhat (vhat read only)
  amsgrad all-l2     the same with every field regularised (emb_reg 1e-8): g = 2 l2 p in the sweep, counted with every vhat written
  adam keras         optim.Adam, no field regularised: the runs update + Keras' dense sweep of p, m and v
  torch Adam amsgrad the table's dense gradient (zeros + fil_embed_run_sum_dt), then torch.optim.Adam(amsgrad=True) (foreach; NOT
                     Keras' rule: epsilon on the corrected root, the maximum taken of the uncorrected v), eager and, with
                     capturable=True, captured ("n/a": refused)
Every path is captured into a HIP graph and replayed: --windows windows of --iters replays each, the median window and the spread
(min - max) are printed; "eager" is one window of eager steps.  "bytes" = the DRAM traffic the path must move at least: a sweep reads
and writes the arrays it walks and reads the int32 stamps; torch writes the zero gradient, then reads p, g and three slots and writes
p and the slots.  "of 6.3 TB/s" = bytes / median replay time / 6.3e12.  Then the ratio of the amsgrad step to Adam's against the
byte ratios (28/24 and 32/24), with the spread of that run's windows, and a whole captured XDeepFM training step with either Keras optimizer
(--no-model skips them)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, optim  # noqa: E402
from ml_function_amd._lib import check, ptr, stream_ptr  # noqa: E402
from optim_bench import B, F, HBM, K, timed, vocab_of  # noqa: E402
from optim_nadam_bench import replay_windows  # noqa: E402

LR = 1e-3
# (name, optimizer, regularised fields, array passes of the sweep: reads + writes; an unregularised amsgrad sweep writes no vhat)
VARIANTS = [("amsgrad", lambda ps: optim.Adam(ps, learning_rate=LR, amsgrad=True), False, 7),
            ("adam keras", lambda ps: optim.Adam(ps, learning_rate=LR), False, 6),
            ("amsgrad all-l2", lambda ps: optim.Adam(ps, learning_rate=LR, amsgrad=True), True, 8),
            ("adam keras (again)", lambda ps: optim.Adam(ps, learning_rate=LR), False, 6)]
MODEL_STEPS = [("adam", lambda ps: optim.Adam(ps, learning_rate=LR)), ("adam amsgrad", lambda ps: optim.Adam(ps, learning_rate=LR, amsgrad=True))]


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

    def ours(make, l2, passes):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        p._fil_runs_table = True
        opt = make([p])
        rec = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None,
                   field_l2=field_l2 if l2 else None)

        def step():
            p._fil_pending_runs = rec
            opt.step()
        return step, passes * table_bytes + 4.0 * V + B * F * K * 4.0, (p, opt)

    def dense_grad(p):
        dt = torch.zeros_like(p)
        check(lib.fil_embed_run_sum_dt(ptr(g), ptr(perm), ptr(sorted_ids), ptr(dt), B * F, K, 0, stream_ptr()), "run_sum")
        return dt

    def torch_opt(capturable):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        opt = torch.optim.Adam([p], lr=LR, betas=(0.9, 0.999), eps=1e-7, amsgrad=True, foreach=True, capturable=capturable)

        def step():
            p.grad = dense_grad(p)
            opt.step()
            p.grad = None
        return step, 10 * table_bytes, (p, opt)

    makers = []
    for name, make, l2, passes in VARIANTS:
        makers.append((name, lambda make=make, l2=l2, passes=passes: ours(make, l2, passes), True))
    # (the captured torch paths last: a refused capture then costs no other line)
    makers += [("torch Adam amsgrad", lambda: torch_opt(False), False), ("torch Adam amsgrad capt.", lambda: torch_opt(True), True)]
    for name, make, capturable in makers:
        step, by, keep = make()
        te = timed(step, iters)
        try:
            tr = replay_windows(step, iters, nwin) if capturable else None
        except RuntimeError as e:           # (only torch's own optimizers can get here: ours raise FilError before any capture)
            if not name.startswith("torch"):
                raise
            print("  %s: capture refused: %s" % (name, str(e).splitlines()[0]), flush=True)
            tr = None
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
        if name.startswith("torch"):
            out[-1] += "   not Keras' rule"
    by_name = {name: (tr, by) for name, te, tr, by in res}
    (ta, ba), (td, bd) = by_name["amsgrad"], by_name["adam keras"]
    fa, fd = ba / (ta[0] * 1e-3) / HBM, bd / (td[0] * 1e-3) / HBM
    out.append("  amsgrad / adam keras: %.3f of the step time (median windows; bytes %.3f: the sweeps alone 28/24 = 1.167 with the vhat store "
               "skipped where vhat holds, 32/24 = 1.333 where every array is written, as in all-l2); windows' spread: "
               "amsgrad %.1f %%, adam %.1f %% of the median" % (ta[0] / td[0], ba / bd, 100 * (ta[2] - ta[1]) / ta[0],
                                                                100 * (td[2] - td[1]) / td[0]))
    out.append("  fraction of 6.3 TB/s: amsgrad %.3f, adam keras %.3f (gap %.3f; adam measured again at the end of the run: %.3f)"
               % (fa, fd, fd - fa, by_name["adam keras (again)"][1] / (by_name["adam keras (again)"][0][0] * 1e-3) / HBM))


def model_steps(iters, nwin, out, vocab_name="bench"):
    """A whole captured XDeepFM training step (tools/optim_bench.py's model, tables in "runs" mode) per optimizer."""
    from ml_function_amd import losses, models
    from ml_function_amd.layers.base import collect_regularization_loss
    dev = torch.device("cuda", 0)
    vocab = vocab_of(vocab_name)
    rng = np.random.default_rng(2020)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    out.append("captured XDeepFM training step (CIN 3x128, MLP 256-128-64, B=%d, F=%d, K=%d, %s vocab, %s rows), replay ms "
               "(median window, min - max):" % (B, F, K, vocab_name, format(sum(vocab), ",")))
    for name, make in MODEL_STEPS:
        torch.manual_seed(0)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useAddLinear=True,
                                 useFlattenLinear=True, emitXT=True, tableGrad="runs")
        model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128])).to(dev)
        model(dense, idx)
        opt = make(list(model.parameters()))

        def step():
            opt.zero_grad(set_to_none=True)
            p = model(dense, idx)[:, 0]
            (losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)).backward()
            opt.step()
        tr = replay_windows(step, iters, nwin)
        out.append("  %-18s %10.3f   %.3f - %.3f" % (name, tr[0], tr[1], tr[2]))
        del model, opt, step
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sizes", default="criteo-size", help="table sizes of optim_bench.vocab_of, comma-separated (empty: none)")
    ap.add_argument("--no-model", action="store_true", help="skip the captured XDeepFM steps")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = ["Keras Adam(amsgrad=True) table step (tools/optim_amsgrad_bench.py, --iters %d --windows %d); %s"
             % (args.iters, args.windows, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for name in filter(None, args.sizes.split(",")):
        out = []
        table_paths(vocab_of(name), args.iters, args.windows, out)
        print("\n".join(out), flush=True)
        lines += out
    if not args.no_model:
        out = []
        model_steps(args.iters, args.windows, out)
        print("\n".join(out), flush=True)
        lines += out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
