"""Top-k retrieval over a long behaviour history: the fused kernel (fil_seq_search behind functional.seq_search) beside the route a user
would compose from torch ops and this library's gather.

    python tools/seq_search_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r29_seq_search_bench.txt)

Shape: B = 4096 samples, K = 16, k = 50, histories of T = 1024 and T = 4096 slots (lengths uniform in 1..T, id 0 = padding) over a
table of 2 M rows; the hard search matches one of 20 categories.
  a. fused       functional.seq_search: one launch, reads the ids and the live rows, writes [B,k].
  b. composed    embed_gather of the [B,T,K] rows + bmm with the query + masked_fill + topk + sort (back to time order) + gather of the
                 ids; the hard search alone ranks the matching slots by position instead of a score.  The reference of the direction check.
  c. SIM step    a whole captured training step of models.SIM under optim.Adam (T = 1024, mode "both"): the fused search beside the
                 same model with SIMInput.search_fn = functional.seq_search_graph.
Timings are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window by
window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the end
(exit status 1 if it fails): in every variant of a / b and in c, the slowest fused window is below the fastest composed window.
Reported, not gated: the fused time over its byte floor -- the ids (and the attributes where they are read) 8 B T each, the live rows
4 K bytes each, the queries and the outputs -- at 8 TB/s, and at the 2.1 TB/s that embed_bag measured for random 64-byte rows."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pool_bench import compare, report  # noqa: E402
from ml_function_amd import functional as Fn, losses, models, optim  # noqa: E402

B, K, SEL, V, CATES = 4096, 16, 50, 2_000_000, 20
LENGTHS = (1024, 4096)
HBM_PEAK, ROW_RATE = 8.0e12, 2.1e12


def make_inputs(T, dev, seed=2021):
    rng = np.random.default_rng(seed)
    hist = rng.integers(1, V, (B, T))
    lens = rng.integers(1, T + 1, B)
    hist[np.arange(T)[None, :] >= lens[:, None]] = 0
    attr = rng.integers(0, CATES, (B, T))
    cand = rng.integers(0, CATES, B)
    t = lambda a: torch.tensor(a, device=dev)
    return t(hist), t(attr), t(cand), torch.randn(B, K, device=dev)


def composed(hist, table, q, attr, cand, offsets, sizes):
    """The search from torch ops: soft when table is given, hard when attr is given."""
    T = hist.shape[1]
    live = hist != 0
    if attr is not None:
        live = live & (attr == cand[:, None])
    if table is not None:
        rows = Fn.embed_gather(table, offsets, hist, sizes=sizes)                        # [B,T,K]
        score = torch.bmm(rows, q.unsqueeze(2)).squeeze(2)
    else:
        score = torch.arange(T, dtype=torch.float32, device=hist.device).expand(hist.shape)   # the most recent matches
    score = score.masked_fill(~live, float("-inf"))
    top = score.topk(SEL, dim=1)
    pos = torch.where(top.values > float("-inf"), top.indices, torch.full_like(top.indices, T)).sort(dim=1).values
    return torch.where(pos < T, hist.gather(1, pos.clamp(max=T - 1)), torch.zeros_like(pos))


def search_rows(out, iters, windows, dev, verdicts):
    table = torch.randn(V, K, device=dev) * 0.1
    for T in LENGTHS:
        hist, attr, cand, q = make_inputs(T, dev)
        offsets = torch.zeros(T, dtype=torch.int64, device=dev)
        sizes = torch.full((T,), V, dtype=torch.int64, device=dev)
        for mode in ("soft", "hard", "both"):
            soft, hard = mode != "hard", mode != "soft"
            kw = dict(size=V, prefer="last" if mode == "hard" else "first")
            if soft:
                kw.update(table=table, query=q)
            if hard:
                kw.update(attr=attr, cand=cand)
            c_args = (hist, table if soft else None, q, attr if hard else None, cand, offsets, sizes)
            with torch.no_grad():
                sel_f, _, count = Fn.seq_search(hist, SEL, **kw)
                sel_c = composed(*c_args)
                agree = float((sel_f == sel_c).all(1).float().mean())
                live = (hist != 0) & ((attr == cand[:, None]) if hard else True)
                n_live = int(live.sum())

            def fused():
                with torch.no_grad():
                    Fn.seq_search(hist, SEL, **kw)

            def comp():
                with torch.no_grad():
                    composed(*c_args)
            floor = 8.0 * B * T * (2 if hard else 1) + (4.0 * K * n_live + 4.0 * B * K if soft else 0.0) + B * SEL * 12.0 + B * 4.0
            out.append("a/b. T = %d, %s search: %d live slots of %d, %.1f selected per sample; fused and composed retrieve the same ids in %.1f %% "
                       "of the samples (the composed score is a bmm: another rounding)" % (T, mode, n_live, B * T, float(count.float().mean()), 100 * agree))
            rows = compare([("a. fused", fused), ("b. composed", comp)], iters, windows)
            report(out, rows)
            fa, co = rows[0], rows[1]
            good = fa[3] < co[2]
            out.append("  composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
                       % (co[1] / fa[1], fa[3], co[2], "below" if good else "NOT below"))
            out.append("  byte floor %.1f MB: %.4f ms at 8 TB/s (fused = %.1fx of it), %.4f ms at 2.1 TB/s (fused = %.1fx of it)"
                       % (floor / 1e6, floor / HBM_PEAK * 1e3, fa[1] / (floor / HBM_PEAK * 1e3), floor / ROW_RATE * 1e3,
                          fa[1] / (floor / ROW_RATE * 1e3)))
            verdicts.append(("T = %d, %s" % (T, mode), good, co[1] / fa[1]))
        del hist, attr, cand, q
        torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev, verdicts):
    rng = np.random.default_rng(2021)
    T, small = LENGTHS[0], 10_000
    vocab = [V, CATES + 1] + [small] * 6
    idx = torch.tensor(np.stack([rng.integers(1, v, B) for v in vocab], 1), device=dev)
    long_idx = rng.integers(1, V, (B, 1, T))
    long_idx[np.arange(T)[None, None, :] >= rng.integers(1, T + 1, B)[:, None, None]] = 0
    long_idx = torch.tensor(long_idx, device=dev)
    long_attr = torch.tensor(rng.integers(1, CATES + 1, (B, 1, T)), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info(vocab, embed_dim=K)]
    steps, keep = [], []
    for variant in ("fused", "search in torch ops"):
        torch.manual_seed(0)
        fi = models.SIMInput(info, None, [(info[0].fea_name, T, SEL, "both", info[1].fea_name)])
        model = models.CTRModel(fi, models.SIM()).to(dev)
        model(None, idx, (None, long_idx, long_attr))
        if variant != "fused":
            fi.search_fn = Fn.seq_search_graph
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, (None, long_idx, long_attr))[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("SIM step: " + variant, step))
        keep.append((model, opt))
    out.append("c. captured models.SIM training step (optim.Adam, %d one-id fields, the first of %d rows, one long history of %d, k = %d, "
               "mode both, K = %d):" % (len(vocab), V, T, SEL, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    verdicts.append(("SIM step", good, rows[1][1] / rows[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,c")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["seq_search_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d, K=%d, k=%d, T in %s (lengths uniform in 1..T), a table of %d rows; the [B,T,K] block the composed route gathers is %.0f MB at T = %d"
           % (B, K, SEL, list(LENGTHS), V, B * LENGTHS[0] * K * 4 / 1e6, LENGTHS[0])]
    for T in LENGTHS:
        plan = Fn.seq_search_plan(B, T, K, SEL)
        out.append("fil_seq_search_plan T = %d: one sample per workgroup, grid %d of at most %d, LDS %d bytes"
                   % (T, plan["grid"], plan["cap"], plan["lds_fwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", search_rows), ("c", model_rows)):
        if part in args.parts.split(","):
            out.append("")
            n = len(out)
            fn(out, args.iters, args.windows, dev, verdicts)
            print("\n".join(out[n:]), flush=True)
    out.append("")
    for label, ok, ratio in verdicts:
        out.append("direction check, %s: %s (fused %.1fx faster than composed at the medians; every fused window below every composed window: %s)"
                   % (label, "PASS" if ok else "FAIL", ratio, "yes" if ok else "no"))
    print("\n" + "\n".join(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0 if all(ok for _, ok, _ in verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
