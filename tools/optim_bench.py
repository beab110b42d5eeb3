"""The optimizer step alone, per embedding-table size, and a whole captured XDeepFM training step per optimizer.

    python tools/optim_bench.py [--iters 20]          (GPU box; output: profiles/r07_optim_bench.txt, r09_optim_deferred_bench.txt)

Table sizes (K = 16, B = 4096, F = 39, one concatenated table): the bench's vocabulary (39 fields log-uniform in [10, 1e5], ~0.4 M
rows: fits the MALL), SURVEY D1's Criteo-like draw (log-uniform in [10, 1e6], ~3.4 M rows) and a Criteo-size 33.8 M rows.  Paths:
  torch / torch-fused  the table's dense gradient (zeros + fil_embed_run_sum_dt) + torch.optim.Adam(capturable, foreach / fused)
  keras                optim.Adam, Keras mode: fil_embed_adam_runs + fil_embed_adam_sweep (+ the counter launch)
  keras-lazy           optim.Adam(lazy_tables=True): fil_embed_adam_runs only (LazyAdam semantics, a labelled deviation)
  keras-deferred/N     optim.Adam(sweep_period=N): the forward's catch-up (fil_embed_adam_catchup_runs) + fil_embed_adam_runs_deferred
                       + fil_embed_adam_roll (+ the counter launch); four different batches in turn (a replay captures four steps and
                       is reported per step), so the catch-up has stale rows to bring current
Times are CUDA-event means over --iters steps, eager and replayed from a HIP graph.  "bytes" = the DRAM traffic the path must move
at least (table-sized arrays: torch 8 passes -- zero fill, then read p g m v, write p m v; keras 6 passes + the int32 stamps; lazy:
the touched rows' p m v read + written + the gradient block; deferred: 6 passes over ceil(V/N) rows + the lazy bytes); "of 6.3
TB/s" = bytes / time / 6.3e12.  Deferred rows also give "VALU bound": the element-updates of one step (V K: every row once per step
on average) at ~38 VALU instructions each (64 per wave instruction), over 1024 SIMDs issuing one wave64 instruction per 2 cycles at
2.4 GHz."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import _lib, functional as Fn, losses, models, optim  # noqa: E402
from ml_function_amd._lib import check, ptr, stream_ptr  # noqa: E402

HBM = 6.3e12
B, F, K = 4096, 39, 16


def vocab_of(name):
    if name == "bench":
        rng = np.random.default_rng(2020)
        return [int(v) for v in np.exp(rng.uniform(np.log(10), np.log(1e5), F))]
    if name == "criteo-like":
        rng = np.random.default_rng(2020)
        return [int(v) for v in np.exp(rng.uniform(np.log(10), np.log(1e6), F))]
    rng = np.random.default_rng(2020)                     # criteo-size: the criteo-like draw scaled to 33.8 M rows
    w = np.exp(rng.uniform(np.log(10), np.log(1e6), F))
    return [max(10, int(v)) for v in w / w.sum() * 33.8e6]


def timed(fn, iters, per=1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters / per


def valu_bound_ms(V):
    """V K element-updates per step at ~38 VALU instructions each, 64 lanes per wave instruction, every one of the 1024 SIMDs issuing
    one wave64 instruction per 2 cycles at 2.4 GHz."""
    return V * K * 38 / 64 * 2 / (1024 * 2.4e9) * 1e3


def replayed(fn, iters, per=1):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return timed(g.replay, iters, per)


def table_paths(vocab, iters, out, paths, periods):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2020)
    V = sum(vocab)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(vocab)[:-1]]), dtype=torch.int64, device=dev)
    sizes = torch.tensor(vocab, dtype=torch.int64, device=dev)
    idx = torch.tensor(np.stack([np.minimum(rng.zipf(1.1, B) - 1, v - 1) for v in vocab], 1), device=dev)
    g = torch.randn(B, F, K, device=dev) * 1e-4
    sorted_ids, perm = Fn._sorted_row_ids(offs, sizes, None, idx, ("bench", tuple(vocab)), V, per_field=True)
    touched = int(torch.unique(sorted_ids[sorted_ids >= 0]).numel())
    lib = _lib.load()
    table_bytes = 4.0 * V * K
    res = []

    def torch_path(fused):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        opt = torch.optim.Adam([p], lr=1e-3, eps=1e-7, capturable=True, **({"fused": True} if fused else {"foreach": True}))

        def step():
            dt = torch.zeros_like(p)
            check(lib.fil_embed_run_sum_dt(ptr(g), ptr(perm), ptr(sorted_ids), ptr(dt), B * F, K, 0, stream_ptr()), "run_sum")
            p.grad = dt
            opt.step()
            p.grad = None
        return step, 8 * table_bytes, (p, opt)

    def keras_path(lazy):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        p._fil_runs_table = True
        opt = optim.Adam([p], lazy_tables=lazy)
        rec = dict(g=g, perm=perm, sorted_ids=sorted_ids, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None, field_l2=None)

        def step():
            p._fil_pending_runs = rec
            opt.step()
        by = (touched * K * 4.0 * 6 + B * F * K * 4.0) if lazy else 6 * table_bytes + 4.0 * V
        return step, by, (p, opt)

    # four batches for the deferred rows: a batch's rows are stale when its forward catches them up
    recs = []
    for i in range(4):
        ix = torch.tensor(np.stack([np.minimum(rng.zipf(1.1, B) - 1, v - 1) for v in vocab], 1), device=dev)
        si, pe = Fn._sorted_row_ids(offs, sizes, None, ix, ("bench%d" % i, tuple(vocab)), V, per_field=True)
        recs.append(dict(g=g, perm=pe, sorted_ids=si, R=B * F, K=K, F=F, g_dtype=0, offsets=offs, frozen=None, field_l2=None))

    def deferred_path(N):
        p = torch.nn.Parameter(torch.randn(V, K, device=dev) * 0.05)
        p._fil_runs_table = True
        opt = optim.Adam([p], sweep_period=N)

        def step():
            for rec in recs:
                optim.deferred_state(p).catch_up(p, rec["sorted_ids"], rec)     # the forward's launch
                p._fil_pending_runs = rec
                opt.step()
        by = 6 * table_bytes / N + 4.0 * V / N + touched * K * 4.0 * 6 + B * F * K * 4.0
        return step, by, (p, opt)

    makers = [("torch", lambda: torch_path(False)), ("torch-fused", lambda: torch_path(True)), ("keras", lambda: keras_path(False)),
              ("keras-lazy", lambda: keras_path(True))]
    makers += [("keras-deferred/%d" % n, (lambda n=n: deferred_path(n))) for n in periods]
    for name, make in makers:
        if name.split("/")[0] not in paths:
            continue
        per = len(recs) if name.startswith("keras-deferred") else 1
        step, by, keep = make()
        te = timed(step, iters, per)
        tr = replayed(step, iters, per)
        res.append((name, te, tr, by))
        del keep, step
        torch.cuda.empty_cache()
    out.append("table %s rows x K=%d (%.2f GB per array), B=%d F=%d, %d touched rows" % (format(V, ","), K, table_bytes / 1e9, B, F,
                                                                                         touched))
    out.append("  %-18s %10s %10s %12s %14s %12s" % ("path", "eager ms", "replay ms", "bytes (GB)", "of 6.3 TB/s", "VALU bound"))
    for name, te, tr, by in res:
        vb = "%.3f ms" % valu_bound_ms(V) if name.startswith("keras-deferred") else ""
        out.append("  %-18s %10.3f %10.3f %12.3f %14.2f %12s" % (name, te, tr, by / 1e9, by / (tr * 1e-3) / HBM, vb))


def model_steps(iters, out, vocab_name="bench", names=("torch", "keras", "keras-lazy"), period=8):
    dev = torch.device("cuda", 0)
    from ml_function_amd.layers.base import collect_regularization_loss
    vocab = vocab_of(vocab_name)
    rng = np.random.default_rng(2020)
    dense = torch.tensor(rng.random((B, 13), dtype=np.float32), device=dev)
    idx = torch.tensor(np.stack([rng.integers(0, v, B) for v in vocab], 1), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    out.append("captured XDeepFM training step (CIN 3x128, MLP 256-128-64, B=%d, F=%d, K=%d, %s vocab, %s rows), replay ms:"
               % (B, F, K, vocab_name, format(sum(vocab), ",")))
    for name in names:
        torch.manual_seed(0)
        fi = models.FeatureInput(sparseInfo=models.make_sparse_info(vocab, embed_dim=K), useLinear=True, useAddLinear=True,
                                 useFlattenLinear=True, emitXT=True, tableGrad="dense" if name == "torch" else "runs")
        model = models.CTRModel(fi, models.XDeepFM(conv_size=[128, 128, 128])).to(dev)
        model(dense, idx)
        opt = (torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7, capturable=True) if name == "torch"
               else optim.Adam(model.parameters(), lazy_tables=name == "keras-lazy",
                               sweep_period=period if name == "keras-deferred" else None))
        # (the table regulariser's value flushes a deferred table: these steps leave it out, as train_ctr.py does)
        skip = vocab_name != "bench"

        def step():
            opt.zero_grad(set_to_none=True)
            p = model(dense, idx)[:, 0]
            (losses.binary_crossentropy(p, y, eps=1e-6) + collect_regularization_loss(model, skip_tables=skip)).backward()
            opt.step()
        out.append("  %-18s %10.3f" % (name + ("/%d" % period if name == "keras-deferred" else ""), replayed(step, iters)))
        del model, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="bench,criteo-like,criteo-size")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--paths", default="torch,torch-fused,keras,keras-lazy,keras-deferred")
    ap.add_argument("--periods", default="4,8,16,32", help="sweep periods of the keras-deferred rows")
    ap.add_argument("--model-sizes", default="bench,criteo-size", help="vocabularies of the captured XDeepFM steps")
    ap.add_argument("--model-period", type=int, default=8, help="sweep period of the keras-deferred XDeepFM step")
    args = ap.parse_args()
    paths = args.paths.split(",")
    periods = [int(x) for x in args.periods.split(",") if x]
    out = ["optim_bench: %s" % torch.cuda.get_device_name(0)]
    for s in args.sizes.split(","):
        if not s:
            continue
        out.append("")
        out.append("[%s]" % s)
        table_paths(vocab_of(s), args.iters, out, paths, periods)
        print("\n".join(out[-12:]), flush=True)
    if not args.no_model:
        for vs in args.model_sizes.split(","):
            out.append("")
            names = ("torch", "keras", "keras-lazy", "keras-deferred") if vs == "bench" else ("keras", "keras-deferred")
            model_steps(args.iters, out, vs, names, args.model_period)
            print("\n".join(out[-6:]), flush=True)
    print("\n".join(out))


if __name__ == "__main__":
    main()
