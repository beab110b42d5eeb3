"""Keras' Mean / BinaryCrossentropy / BinaryAccuracy (include/fil.h M2, ml_function_amd.metrics): what an update costs, against what a
user would write otherwise.  The sibling of tools/metrics_bench.py (the AUC), with the same yardsticks.

    python tools/metrics_mean_bench.py [--iters 200]      (GPU box; output: profiles/r22_metrics_mean_bench.txt)

1. one update of each kind at n = 4,096, replayed from a one-node HIP graph: fil_mean_update, the torch restatement a user would
   write captured the same way, and an empty-ish graph (one 4-byte copy: what a replay costs by itself).  Precision and Recall (one
   fil_confusion_update each, result() as torch ops) beside them.
2. the whole captured XDeepFM step of tools/metrics_bench.py (keras Adam, bench vocabulary) with and without Mean(loss) +
   BinaryCrossentropy + BinaryAccuracy inside the graph: A/B alternating in one process, medians of --windows windows.  The plain
   step launches exactly what the parent commit's step launches (this library only gained kernels).  Expectation: (added graph
   nodes: the three updates and one copy that makes the strided score column contiguous) x (the cost of a further node from 1),
   give or take the windows' spread.
3. one update at n = 2^20 and 2^24 (evaluation sizes), eager launches in a stream: GB/s of the bytes the update must read (8 n; 4 n
   for Mean) against the 6.3 TB/s a streaming read reaches on this part."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import losses, metrics, models, optim  # noqa: E402
from metrics_bench import graph_of, median_us, scores  # noqa: E402
from optim_bench import B, F, HBM, K, timed, vocab_of  # noqa: E402

EPS = 1e-7


def torch_mean(v, st):
    st[0].add_(v.sum())
    st[1].add_(float(v.numel()))
    st[2].copy_(st[0] / st[1])


def torch_bce(p, y, st):
    pc = p.clamp(EPS, 1 - EPS)
    torch_mean(-(y * torch.log(pc + EPS) + (1 - y) * torch.log(1 - pc + EPS)), st)


def torch_acc(p, y, st):
    torch_mean((y == (p > 0.5).to(torch.float32)).to(torch.float32), st)


def small_update(iters, out):
    out.append("1. one update at n = 4096, replayed from a one-node HIP graph, us per replay (median of 5 windows of %d):" % iters)
    p, y = scores("skewed", 4096)
    ms = [metrics.Mean().build("cuda"), metrics.BinaryCrossentropy().build("cuda"), metrics.BinaryAccuracy().build("cuda")]
    st = [torch.zeros(3, device="cuda") for _ in range(3)]
    a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    none = median_us(graph_of(lambda: a.copy_(b)).replay, iters)
    rows = (("Mean", lambda: ms[0].update_state(p), lambda: torch_mean(p, st[0])),
            ("BinaryCrossentropy", lambda: ms[1].update_state(y, p), lambda: torch_bce(p, y, st[1])),
            ("BinaryAccuracy", lambda: ms[2].update_state(y, p), lambda: torch_acc(p, y, st[2])))
    node = []
    for name, ours, theirs in rows:
        t_ours, t_torch = median_us(graph_of(ours).replay, iters), median_us(graph_of(theirs).replay, iters)
        node.append(t_ours)
        out.append("  %-19s fil_mean_update (result included) %7.2f   torch restatement %7.2f   one 4-byte copy %7.2f"
                   % (name, t_ours, t_torch, none))
    all3 = median_us(graph_of(lambda: [r[1]() for r in rows]).replay, iters)
    out.append("  all three in one graph (three nodes) %7.2f   = one 4-byte copy + %.2f per added node" % (all3, (all3 - none) / 3))
    for cls in (metrics.Precision, metrics.Recall):
        m = cls().build("cuda")
        t_upd = median_us(graph_of(lambda: m.update_state(y, p)).replay, iters)
        t_both = median_us(graph_of(lambda: (m.update_state(y, p), m.result())).replay, iters)
        out.append("  %-19s fil_confusion_update (T = 2)        %7.2f   + result() as torch ops %7.2f" % (cls.__name__, t_upd, t_both))
    return none, node, all3


def model_step(iters, windows, out, none, all3):
    from ml_function_amd.layers.base import collect_regularization_loss
    dev = torch.device("cuda", 0)
    vocab = vocab_of("bench")
    rng = np.random.default_rng(2020)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    graphs, keep = {}, []
    for name in ("plain", "with metrics"):
        torch.manual_seed(0)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useAddLinear=True,
                                 useFlattenLinear=True, emitXT=True, tableGrad="runs")
        model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128])).to(dev)
        model(dense, idx)
        opt = optim.Adam(model.parameters())
        ms = ([metrics.Mean(name="loss").build(dev), metrics.BinaryCrossentropy().build(dev), metrics.BinaryAccuracy().build(dev)]
              if name == "with metrics" else None)

        def step(model=model, opt=opt, ms=ms):
            opt.zero_grad(set_to_none=True)
            p = model(dense, idx)[:, 0]
            bce = losses.binary_crossentropy(p, y, eps=1e-6)
            (bce + collect_regularization_loss(model)).backward()
            opt.step()
            if ms is not None:
                pc = p.detach().contiguous()                   # model(...)[:, 0] is a strided view: one copy for both readers
                ms[0].update_state(bce)
                ms[1].update_state(y, pc)
                ms[2].update_state(y, pc)
        graphs[name] = graph_of(step)
        keep.append((model, opt, ms))
    times = {k: [] for k in graphs}
    for _ in range(windows):                                   # A/B alternating in one process
        for name, g in graphs.items():
            times[name].append(timed(g.replay, iters))
    a, b = statistics.median(times["plain"]), statistics.median(times["with metrics"])
    spread = max(max(t) - min(t) for t in times.values()) * 1e3
    per_node = (all3 - none) / 3
    expect = 4 * per_node                                      # the three updates and the copy of the strided score column
    out.append("2. captured XDeepFM training step (CIN 3x128, MLP 256-128-64, B=%d, F=%d, K=%d, bench vocab, keras Adam), replay ms, "
               "A/B alternating, median of %d windows of %d:" % (B, F, K, windows, iters))
    out.append("  plain %.4f   with Mean(loss) + BinaryCrossentropy + BinaryAccuracy in the graph %.4f   difference %+.2f us (%+.2f %%)"
               % (a, b, (b - a) * 1e3, 100 * (b - a) / a))
    out.append("  windows plain        %s" % " ".join("%.4f" % t for t in times["plain"]))
    out.append("  windows with metrics %s" % " ".join("%.4f" % t for t in times["with metrics"]))
    out.append("  expectation: 4 added nodes (three updates + one copy of the strided score column) x %.2f us (section 1) = %.2f us; "
               "windows' spread %.2f us; the step %s it" % (per_node, expect, spread, "meets" if (b - a) * 1e3 <= expect + spread else "does NOT meet"))


def large_update(iters, out):
    out.append("3. one update at large n, eager launches (event time per call, median of 5 windows of %d):" % iters)
    for n in (1 << 20, 1 << 24):
        p, y = scores("skewed", n)
        for name, m, call, nbytes in (("Mean", metrics.Mean().build("cuda"), lambda m: m.update_state(p), 4.0 * n),
                                      ("BinaryCrossentropy", metrics.BinaryCrossentropy().build("cuda"), lambda m: m.update_state(y, p), 8.0 * n),
                                      ("BinaryAccuracy", metrics.BinaryAccuracy().build("cuda"), lambda m: m.update_state(y, p), 8.0 * n)):
            us = median_us(lambda: call(m), iters)
            gbs = nbytes / (us * 1e-6) / 1e9
            out.append("  n = 2^%d %-19s %9.2f us   %2d n bytes   %8.1f GB/s   %5.1f %% of 6.3 TB/s"
                       % (n.bit_length() - 1, name, us, nbytes / n, gbs, 100 * gbs * 1e9 / HBM))
        del p, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default="update,model,large")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_mean_bench needs a GPU (there is nothing to time on a CPU)")
    out = ["metrics_mean_bench: %s" % torch.cuda.get_device_name(0)]
    only = args.only.split(",")
    none, _, all3 = small_update(args.iters * 10, out) if "update" in only or "model" in only else (0.0, [], 0.0)
    if "model" in only:
        model_step(args.iters, args.windows, out, none, all3)
    if "large" in only:
        large_update(max(10, args.iters // 4), out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
