"""The three views of the Sequence-Aware Factorization Machine: the fused, pooled kernels (fil_seqattn_fwd_v / fil_seqattn_bwd_v behind
layers.SeqViewAttentionLayer) beside the layer's own composed path (seq_view_attention_graph: the same math in torch ops) and beside
the fused kernels with rows out followed by torch's masked mean.

    python tools/seqfm_bench.py [--iters 30] [--windows 5] [--out profiles/r30_seqfm_bench.txt]          (GPU box)

Shapes: B = 4096 samples, K = 16, one head of 16, F = 8 static fields, a history of T = 20 and of T = 50 (lengths uniform in 1..T).
  static view   [B,8,16], no mask, view "full";   dynamic view   [B,T,16] under the history's mask, view "causal";
  cross view    [B,8+T,16] under [ones ; mask], view "cross", split 8;   all three: the three calls in one graph.
  a. fused pooled    layers.SeqViewAttentionLayer(pool=True): forward alone (no_grad), and forward + backward with the gradients of x
                     and the weights.
  b. composed        the same layer's _composed path (seq_view_attention_graph), the same weights.
  c. rows + mean     the fused kernels with pool=False, then (out * w).sum(1) / w.sum(1).clamp_min(1) in torch ops.  Reported, not gated.
  d. SeqFM step      a whole captured training step of models.SeqFM under optim.Adam: the fused layers beside the same model with
                     every view forced onto the composed path.
Every timing is a replay of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window
by window; reported: the median window's time per replay and the spread (min .. max) over the windows.  Each part (one history length
of a / b / c, one of d) runs in a child process of its own under a time limit; the first part that does not end normally ends the
run.  The direction check at the end (exit status 1 if it fails): in every variant of a / b and of d, the slowest fused window is
below the fastest composed window."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, V, K, H, F = 4096, 10_000, 16, 1, 8
HISTORIES = (20, 50)
PARTS = ["views%d" % T for T in HISTORIES] + ["model%d" % T for T in HISTORIES]
PART_LIMIT_S = 240
VERDICT = "direction check, "


def view_rows(out, T, iters, windows, dev):
    from afm_pool_bench import compare, report
    from ml_function_amd import layers
    rng = np.random.default_rng(2021)
    lens = rng.integers(1, T + 1, B)
    hist_mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    cross_mask = torch.cat([torch.ones((B, F), dtype=torch.bool, device=dev), hist_mask], dim=1)
    leaf = lambda n: (torch.randn(B, n, K, device=dev) * 0.5).requires_grad_()
    views = [("static view (full, T = %d)" % F, dict(view="full"), leaf(F), None),
             ("dynamic view (causal, T = %d)" % T, dict(view="causal"), leaf(T), hist_mask),
             ("cross view (cross, T = %d + %d, split %d)" % (F, T, F), dict(view="cross", split=F), leaf(F + T), cross_mask)]
    made = []
    for label, kw, x, mask in views:
        pooled = layers.SeqViewAttentionLayer(H, K // H, pool=True, **kw)
        rows = layers.SeqViewAttentionLayer(H, K // H, pool=False, **kw)
        with torch.no_grad():
            pooled(x.detach(), mask=mask)
            rows(x.detach(), mask=mask)
        rows.load_state_dict(pooled.state_dict())
        assert pooled.fits_kernel_menu(x)
        w = (torch.ones(x.shape[:2], device=dev) if mask is None else mask.to(torch.float32)).unsqueeze(-1)
        made.append(dict(label=label, x=x, mask=mask, pooled=pooled, rows=rows, w=w, dy=torch.randn(B, K, device=dev)))

    def fused(v):
        return v["pooled"](v["x"], mask=v["mask"])

    def comp(v):
        return v["pooled"]._composed(v["x"], v["mask"])

    def rows_mean(v):
        o = v["rows"](v["x"], mask=v["mask"])
        return (o * v["w"]).sum(dim=1) / v["w"].sum(dim=1).clamp_min(1.0)

    def forward(fn, group):
        def run():
            with torch.no_grad():
                for v in group:
                    fn(v)
        return run

    def both(fn, group):
        def run():
            for v in group:
                v["x"].grad = None
                v["pooled"].zero_grad(set_to_none=True)
                v["rows"].zero_grad(set_to_none=True)
                fn(v).backward(v["dy"])
        return run

    for label, group in [(v["label"], [v]) for v in made] + [("the three views together", made)]:
        with torch.no_grad():
            d = max(float((fused(v) - comp(v)).abs().max() / comp(v).abs().max()) for v in group)
            d2 = max(float((fused(v) - rows_mean(v)).abs().max() / comp(v).abs().max()) for v in group)
        out.append("a/b/c. history T = %d, %s (fused vs composed output: max difference %.1e of the largest value; vs rows + mean: %.1e):"
                   % (T, label, d, d2))
        rows = compare([("a. fused pooled, forward", forward(fused, group)), ("b. composed, forward", forward(comp, group)),
                        ("c. fused rows + torch mean, forward", forward(rows_mean, group)),
                        ("a. fused pooled, forward + backward", both(fused, group)), ("b. composed, forward + backward", both(comp, group)),
                        ("c. fused rows + torch mean, forward + backward", both(rows_mean, group))], iters, windows)
        report(out, rows)
        t = {name: (med, lo, hi) for name, med, lo, hi in rows}
        ok = True
        for what in ("forward", "forward + backward"):
            fa, co, rm = t["a. fused pooled, " + what], t["b. composed, " + what], t["c. fused rows + torch mean, " + what]
            good = fa[2] < co[1]
            ok = ok and good
            out.append("  %-19s composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
                       % (what + ":", co[0] / fa[0], fa[2], co[1], "below" if good else "NOT below"))
            out.append("  %-19s (rows + mean) / pooled = %.2fx (medians); slowest pooled window %.4f ms, fastest rows + mean window %.4f ms: %s"
                       % ("", rm[0] / fa[0], fa[2], rm[1], "pooling in the kernel is faster in every window" if fa[2] < rm[1]
                          else "pooling in the kernel is NOT faster in every window"))
        ratio = t["b. composed, forward + backward"][0] / t["a. fused pooled, forward + backward"][0]
        out.append("%sT = %d, %s: %s (fused %.1fx faster than composed at the medians, forward + backward)"
                   % (VERDICT, T, label, "PASS" if ok else "FAIL", ratio))


def model_rows(out, T, iters, windows, dev):
    from afm_pool_bench import compare, report
    from ml_function_amd import layers, losses, models, optim
    rng = np.random.default_rng(2021)
    idx = torch.tensor(rng.integers(1, V, (B, F)), device=dev)
    hist = rng.integers(1, V, (B, T))
    hist[np.arange(T)[None, :] >= rng.integers(1, T + 1, B)[:, None]] = 0
    hist = torch.tensor(hist.reshape(B, 1, T), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info([V] * F, embed_dim=K)]
    steps, keep = [], []
    for variant in ("fused", "composed path forced"):
        torch.manual_seed(0)
        fi = models.DINInput(info, behavior=[(info[0].fea_name, T)])
        model = models.CTRModel(fi, models.SeqFM()).to(dev)
        model(None, idx, hist)
        if variant != "fused":
            for m in model.modules():
                if isinstance(m, layers.SeqViewAttentionLayer):
                    m.fits_kernel_menu = lambda x: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, hist)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("SeqFM step: " + variant, step))
        keep.append((model, opt))
    out.append("d. captured models.SeqFM training step (optim.Adam, %d one-id fields of %d rows, one history of %d, K = %d, 1 head, 1 FFN layer):"
               % (F, V, T, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    out.append("%sSeqFM step, T = %d: %s (fused %.2fx faster than composed at the medians)"
               % (VERDICT, T, "PASS" if good else "FAIL", rows[1][1] / rows[0][1]))


def run_part(part, iters, windows):
    """In the child process: one part's report lines on stdout."""
    dev = torch.device("cuda", 0)
    out = []
    (view_rows if part.startswith("views") else model_rows)(out, int("".join(c for c in part if c.isdigit())), iters, windows, dev)
    print("\n".join(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--part", default=None, help="(internal) run this one part in this process")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.part:
        return run_part(args.part, args.iters, args.windows)
    out = ["seqfm_bench: B=%d, K=%d, %d head, F=%d static fields, histories of %s, lengths uniform in 1..T" % (B, K, H, F, list(HISTORIES)),
           "HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters)]
    print("\n".join(out), flush=True)
    ended = True
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--iters", str(args.iters), "--windows", str(args.windows)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=PART_LIMIT_S)
        except subprocess.TimeoutExpired:
            out += ["", "%s: not measured (no end within %d s); nothing after it was started" % (part, PART_LIMIT_S)]
            ended = False
            break
        if r.returncode != 0:
            out += ["", "%s: not measured (exit status %d); nothing after it was started" % (part, r.returncode)] + r.stderr.splitlines()[-15:]
            ended = False
            break
        out += [""] + r.stdout.splitlines()
        print("\n" + r.stdout, flush=True)
    verdicts = [line for line in out if line.startswith(VERDICT)]
    out += ["", "direction checks: %d of %d PASS%s" % (sum(": PASS" in v for v in verdicts), len(verdicts), "" if ended else " (the run did not end)")]
    print("\n".join(out[-2:]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0 if ended and verdicts and all(": PASS" in v for v in verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
