"""Keras' streaming AUC (include/fil.h M1, metrics.AUC): what the update costs, against what a user would write otherwise.

    python tools/metrics_bench.py [--iters 200]           (GPU box; output: profiles/r11_metrics_bench.txt)
    rocprofv3 --kernel-trace --stats -- python tools/metrics_bench.py --only update --iters 20
                                                          (per-kernel totals and the launch count of one update)

1. update at n = 4,096, T = 200, replayed from a HIP graph: fil_confusion_update (one launch), the torch restatement a user would
   write ((p[None] > thr[:, None]), masks, four sums, four add_), captured the same way, and an empty-ish graph (one 4-byte copy:
   what a replay costs by itself).  Scores uniform on [0, 1] and skewed (sigmoid of N(-3.5, 1)).
2. update at n = 2^20 and 2^24, eager launches in a stream (event time over --iters calls): GB/s of the 8 n bytes the update must
   read, against the 6.3 TB/s a streaming read reaches on this part.
3. the whole captured XDeepFM step of tools/optim_bench.py (keras Adam, bench vocabulary) with and without update_state + result()
   inside the graph: A/B alternating in one process, medians of --windows windows.
4. metrics.auc (exact Mann-Whitney: a sort, host synchronisations) beside AUC().update_state + result() at 2^20 scores, for scale.
   DIFFERENT quantities: the first is the exact AUC of the scores, the second Keras' 200-threshold approximation of it."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import functional as Fn, losses, metrics, models, optim  # noqa: E402
from optim_bench import B, F, HBM, K, timed, vocab_of  # noqa: E402

T = 200


def scores(dist, n, seed=0):
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        p = rng.random(n, dtype=np.float32)
    else:
        p = (1.0 / (1.0 + np.exp(-rng.normal(-3.5, 1.0, n)))).astype(np.float32)
    y = (rng.random(n) < p).astype(np.float32)
    return torch.tensor(p, device="cuda"), torch.tensor(y, device="cuda")


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


def median_us(fn, iters, windows=5):
    return statistics.median(timed(fn, iters) for _ in range(windows)) * 1e3


def torch_update(p, y, thr, tp, fp, tn, fn_):
    """The restatement a user would write in torch."""
    pos = p[None, :] > thr[:, None]
    lab = (y != 0)[None, :]
    tp.add_((pos & lab).sum(1))
    fp.add_((pos & ~lab).sum(1))
    tn.add_((~pos & ~lab).sum(1))
    fn_.add_((~pos & lab).sum(1))


def small_update(iters, out):
    out.append("1. update at n = 4096, T = 200, replayed from a HIP graph, us per replay (median of 5 windows of %d):" % iters)
    per = {}
    for dist in ("uniform", "skewed"):
        p, y = scores(dist, 4096)
        m = metrics.AUC().build("cuda")
        g_ours = graph_of(lambda: m.update_state(y, p))
        g_both = graph_of(lambda: (m.update_state(y, p), m.result()))
        state = [torch.zeros(T, device="cuda") for _ in range(4)]
        g_torch = graph_of(lambda: torch_update(p, y, m._thr, *state))
        a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        g_none = graph_of(lambda: a.copy_(b))
        per[dist] = [median_us(g.replay, iters) for g in (g_ours, g_both, g_torch, g_none)]
        out.append("  %-8s fil_confusion_update %7.2f   + fil_auc_result %7.2f   torch restatement %7.2f   one 4-byte copy %7.2f"
                   % ((dist,) + tuple(per[dist])))
    out.append("  skewed / uniform, fil_confusion_update: %.2fx" % (per["skewed"][0] / per["uniform"][0]))


def large_update(iters, out):
    out.append("2. update at large n, T = 200, eager launches (event time per call, median of 5 windows of %d); bytes = 8 n:" % iters)
    for n in (1 << 20, 1 << 24):
        for dist in ("uniform", "skewed"):
            p, y = scores(dist, n)
            m = metrics.AUC().build("cuda")
            us = median_us(lambda: m.update_state(y, p), iters)
            gbs = 8.0 * n / (us * 1e-6) / 1e9
            out.append("  n = 2^%d %-8s %9.2f us   %8.1f GB/s   %5.1f %% of 6.3 TB/s" % (n.bit_length() - 1, dist, us, gbs, 100 * gbs * 1e9 / HBM))
            del p, y


def model_step(iters, windows, out):
    from ml_function_amd.layers.base import collect_regularization_loss
    dev = torch.device("cuda", 0)
    vocab = vocab_of("bench")
    rng = np.random.default_rng(2020)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    graphs = {}
    keep = []
    for name in ("plain", "with AUC"):
        torch.manual_seed(0)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useAddLinear=True,
                                 useFlattenLinear=True, emitXT=True, tableGrad="runs")
        model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128])).to(dev)
        model(dense, idx)
        opt = optim.Adam(model.parameters())
        m = metrics.AUC().build(dev) if name == "with AUC" else None

        def step(model=model, opt=opt, m=m):
            opt.zero_grad(set_to_none=True)
            p = model(dense, idx)[:, 0]
            (losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)).backward()
            opt.step()
            if m is not None:
                m.update_state(y, p)
                m.result()
        graphs[name] = graph_of(step)
        keep.append((model, opt, m))
    times = {k: [] for k in graphs}
    for _ in range(windows):                                   # A/B alternating in one process
        for name, g in graphs.items():
            times[name].append(timed(g.replay, iters))
    a, b = statistics.median(times["plain"]), statistics.median(times["with AUC"])
    out.append("3. captured XDeepFM training step (CIN 3x128, MLP 256-128-64, B=%d, F=%d, K=%d, bench vocab, keras Adam), replay ms, "
               "A/B alternating, median of %d windows of %d:" % (B, F, K, windows, iters))
    out.append("  plain %.4f   with update_state + result() in the graph %.4f   difference %+.2f us (%+.2f %%)"
               % (a, b, (b - a) * 1e3, 100 * (b - a) / a))
    out.append("  windows plain    %s" % " ".join("%.4f" % t for t in times["plain"]))
    out.append("  windows with AUC %s" % " ".join("%.4f" % t for t in times["with AUC"]))


def for_scale(out):
    n = 1 << 20
    p, y = scores("skewed", n)
    m = metrics.AUC().build("cuda")

    def ours():
        m.reset_states()
        m.update_state(y, p)
        return float(m.result())

    def exact():
        return metrics.auc(y, p)
    t_ours = statistics.median(timed(ours, 10) for _ in range(5))
    t_exact = statistics.median(timed(exact, 10) for _ in range(5))
    out.append("4. for scale, 2^20 skewed scores, eager, ms per call including the host read (DIFFERENT quantities):")
    out.append("  metrics.auc (exact Mann-Whitney)                          %8.3f ms   value %.6f" % (t_exact, exact()))
    out.append("  AUC(): reset + update_state + float(result()) (Keras 200) %8.3f ms   value %.6f" % (t_ours, ours()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default="update,large,model,scale")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU (there is nothing to time on a CPU)")
    out = ["metrics_bench: %s" % torch.cuda.get_device_name(0)]
    only = args.only.split(",")
    if "update" in only:
        small_update(args.iters * 10, out)
    if "large" in only:
        large_update(max(10, args.iters // 4), out)
    if "model" in only:
        model_step(args.iters, args.windows, out)
    if "scale" in only:
        for_scale(out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
