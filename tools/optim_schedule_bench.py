"""What a learning-rate schedule costs inside a captured step: one more one-thread node (fil_lr_schedule_eval) and one more
wave-uniform load per update kernel.

    python tools/optim_schedule_bench.py [--iters 20] [--windows 7] [--float-only]      (GPU box; output: profiles/r12_optim_schedule_bench.txt)
    rocprofv3 --kernel-trace --stats -- python tools/optim_schedule_bench.py --only a --kinds ExponentialDecay --windows 2

In one process, replayed from HIP graphs, in the windows of tools/optim_bench.py (3 warm-up replays, then the CUDA-event mean of
--iters replays), --windows windows per figure (median reported, the spread is max - min over the windows):
  (a) the optimizer step alone on the Criteo-size table (33.8 M rows x K = 16, optim_bench's "keras" path: fil_embed_adam_runs +
      fil_embed_adam_sweep + the counter launch)
  (b) the captured XDeepFM training step of profiles/r07_optim_bench.txt (bench vocabulary, optim.Adam in Keras mode)
each on ONE set of tensors (parameters, slots and stamps shared by the optimizers of a step), with a float rate (the by-value entry
points) and with schedules.ExponentialDecay (the *_lrdev ones behind the evaluation) -- and, as a control, "float+node": the
float-rate step behind one extra one-thread launch, i.e. the graph shape of the schedule step with the by-value kernels -- and
  (c) what one more one-thread kernel node costs a replay: graphs of 1 and of 17 launches of the counter's advance kernel (one thread,
      one 8-byte read-modify-write), the difference over 16.
--float-only measures the float-rate rows alone and imports nothing of the schedules: it is how the same tool times the parent
commit, whose float-rate figures are the yardstick (same box, same session)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, losses, models, optim  # noqa: E402
from ml_function_amd._lib import check  # noqa: E402
from optim_bench import B, F, K, timed, vocab_of  # noqa: E402


def windows(fn, iters, n):
    """n windows of one captured fn: (median, min, max) ms."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    ts = sorted(timed(g.replay, iters) for _ in range(n))
    return ts[len(ts) // 2], ts[0], ts[-1]


def rate(name):
    if name.startswith("float"):
        return 1e-3
    from ml_function_amd import schedules
    return schedules.ExponentialDecay(1e-3, decay_steps=10000, decay_rate=0.96)


def with_node(step):
    """`step` behind one launch of the counter's advance kernel on a counter of its own (the "float+node" control)."""
    lib = _lib.load()
    scratch = torch.zeros(1, dtype=torch.int64, device="cuda")

    def fn():
        check(lib.fil_adam_multi(None, 0, 0, scratch.data_ptr(), 1e-3, 0.9, 0.999, 1e-7, 1, _lib.stream_ptr()), "fil_adam_multi")
        step()
    return fn


def optimizers(params, kinds, run_once):
    """One optim.Adam per rate among `kinds` over the SAME parameters, slots and row stamps: the rows of one step differ in the rate
    route alone, not in where their tensors lie (two fresh 2 GB allocations of the same step differ by up to 0.6 ms at (a): the
    float+node control rows showed it).  run_once(opt): one eager step, which creates the slots of the first optimizer."""
    opts = {}
    for kind in kinds:
        key = "float" if kind.startswith("float") else kind
        if key in opts:
            continue
        opt = optim.Adam(params, learning_rate=rate(key))
        if opts:
            first = next(iter(opts.values()))
            for q, st in first.state.items():
                opt.state[q] = st
            opt._stamps = first._stamps
        opts[key] = opt
        run_once(opt)
    return opts


def table_step(kinds):
    dev = torch.device("cuda", 0)
    vocab = vocab_of("criteo-size")
    rng = np.random.default_rng(2020)
    V = sum(vocab)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(vocab)[:-1]]), dtype=torch.int64, device=dev)
    sizes = torch.tensor(vocab, dtype=torch.int64, device=dev)
    idx = torch.tensor(np.stack([np.minimum(rng.zipf(1.1, B) - 1, v - 1) for v in vocab], 1), device=dev)
    g = torch.randn(B, F, K, device=dev) * 1e-4
    sorted_ids, perm = Fn._sorted_row_ids(offs, sizes, None, idx, ("bench", tuple(vocab)), V, per_field=True)
    p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
    p._fil_runs_table = True
    rec = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None, field_l2=None)

    def stepper(opt):
        def step():
            p._fil_pending_runs = rec
            opt.step()
        return step
    opts = optimizers([p], kinds, lambda opt: stepper(opt)())
    return {k: stepper(o) for k, o in opts.items()}, (p, opts)


def model_step(kinds):
    dev = torch.device("cuda", 0)
    from ml_function_amd.layers.base import collect_regularization_loss
    vocab = vocab_of("bench")
    rng = np.random.default_rng(2020)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    torch.manual_seed(0)
    fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useAddLinear=True,
                             useFlattenLinear=True, emitXT=True, tableGrad="runs")
    model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128])).to(dev)
    model(dense, idx)

    def stepper(opt):
        def step():
            opt.zero_grad(set_to_none=True)
            p = model(dense, idx)[:, 0]
            (losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model)).backward()
            opt.step()
        return step
    opts = optimizers(list(model.parameters()), kinds, lambda opt: stepper(opt)())
    return {k: stepper(o) for k, o in opts.items()}, (model, opts)


def node_cost(iters, n):
    """Graphs of 1 and of 17 one-thread launches (fil_adam_multi with no tensors and advance = 1: the counter's advance kernel)."""
    lib = _lib.load()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")

    def launches(k):
        def fn():
            for _ in range(k):
                check(lib.fil_adam_multi(None, 0, 0, counter.data_ptr(), 1e-3, 0.9, 0.999, 1e-7, 1, _lib.stream_ptr()), "fil_adam_multi")
        return fn
    one = windows(launches(1), iters, n)
    many = windows(launches(17), iters, n)
    return one, many, (many[0] - one[0]) / 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--float-only", action="store_true")
    ap.add_argument("--only", default="a,b,c", help="which of (a), (b), (c) to run")
    ap.add_argument("--kinds", default=None, help="comma-separated rows per step: float, float+node, ExponentialDecay")
    args = ap.parse_args()
    kinds = ["float"] if args.float_only else ["float", "ExponentialDecay", "float+node", "float", "ExponentialDecay"]
    if args.kinds:
        kinds = args.kinds.split(",")
    only = args.only.split(",")
    out = ["optim_schedule_bench: %s, %d windows of %d replays%s" % (torch.cuda.get_device_name(0), args.windows, args.iters,
                                                                     " (float rate only)" if args.float_only else "")]
    out.append("  %-46s %-18s %10s %10s %10s %10s" % ("step", "rate", "median ms", "min ms", "max ms", "spread us"))
    for title, make in (("(a) Adam step, 33.8 M x 16 table", table_step), ("(b) captured XDeepFM step, bench vocabulary", model_step)):
        if title[1] not in only:
            continue
        steps, keep = make(kinds)
        for kind in kinds:
            step = with_node(steps["float"]) if kind == "float+node" else steps[kind]
            med, lo, hi = windows(step, args.iters, args.windows)
            out.append("  %-46s %-18s %10.4f %10.4f %10.4f %10.1f" % (title, kind, med, lo, hi, (hi - lo) * 1e3))
            print(out[-1], flush=True)
        del steps, keep
        torch.cuda.empty_cache()
    if "c" not in only:
        print("\n".join(out))
        return
    one, many, per = node_cost(args.iters, args.windows)
    out.append("  (c) graph of 1 one-thread node: %.2f us (min %.2f, max %.2f); of 17: %.2f us (min %.2f, max %.2f); per added node %.2f us"
               % (one[0] * 1e3, one[1] * 1e3, one[2] * 1e3, many[0] * 1e3, many[1] * 1e3, many[2] * 1e3, per * 1e3))
    print("\n".join(out))


if __name__ == "__main__":
    main()
