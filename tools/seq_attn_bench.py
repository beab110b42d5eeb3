"""Masked multi-head self-attention over a behaviour sequence: the fused kernels (fil_seqattn_fwd / fil_seqattn_bwd behind
layers.SeqSelfAttentionLayer) beside the layer's own composed path (the same math in torch ops) and torch's
scaled_dot_product_attention.

    python tools/seq_attn_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r27_seq_attn_bench.txt)

Shapes: B = 4096 samples; T = 50 positions (lengths uniform in 1..50) at (K, H, D) = (16, 2, 8) and (32, 4, 8); T = 20 at (16, 2, 8).
  a. fused        layers.SeqSelfAttentionLayer: forward alone (no_grad), and forward + backward with the gradients of x and the weights.
  b. composed     the same layer's _composed path (seq_self_attention_graph), the same weights, captured.
  c. SDPA         torch.nn.functional.scaled_dot_product_attention on PRE-PROJECTED q, k, v [B,H,T,D] with the same key mask, EAGER
                  timing (not a graph replay): it leaves out the three projections and the masked rows' zeroing; listed for scale,
                  not gated.
  d. bare op      functional.seq_self_attention forward and forward + backward against the bytes it cannot avoid (x, out and `saved`
                  once each way, at the 8 TB/s HBM peak) and against its fp32 FLOP count at the fp32 matrix peak.  Reported, not gated.
  e. BST step     a whole captured training step of models.BST under optim.Adam: the fused layer beside the same model with its
                  attention layer forced onto the composed path.  Reported, not gated.
Timings a, b, d, e are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns
window by window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check
at the end (exit status 1 if it fails): at every shape of a / b, forward and forward + backward, the slowest fused window is below
the fastest composed window."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pool_bench import compare, report  # noqa: E402
from ml_function_amd import functional as Fn, layers, losses, models, optim  # noqa: E402

B, V = 4096, 10_000
SHAPES = ((50, 16, 2, 8), (50, 32, 4, 8), (20, 16, 2, 8))      # T, K, H, D
HBM_PEAK = 8.0e12
FP32_MATRIX_PEAK = 157.3e12


def make_inputs(T, K, dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    x = (torch.randn(B, T, K, device=dev) * 0.5).requires_grad_()
    return x, mask, lens


def make_layer(H, D, x, mask):
    layer = layers.SeqSelfAttentionLayer(H, D)
    with torch.no_grad():
        layer(x.detach(), mask=mask)
    assert layer.fits_kernel_menu(x)
    return layer


def layer_rows(out, iters, windows, dev, verdicts):
    for T, K, H, D in SHAPES:
        x, mask, _ = make_inputs(T, K, dev)
        layer = make_layer(H, D, x, mask)
        dy = torch.randn(B, T, H * D, device=dev)
        fused = lambda: layer(x, mask=mask)
        comp = lambda: layer._composed(x, mask)
        with torch.no_grad():
            d = float((fused() - comp()).abs().max() / comp().abs().max())

        def fused_fwd():
            with torch.no_grad():
                fused()

        def comp_fwd():
            with torch.no_grad():
                comp()

        def step(fn):
            x.grad = None
            layer.zero_grad(set_to_none=True)
            fn().backward(dy)
        label = "T = %d, K = %d, %d heads of %d" % (T, K, H, D)
        out.append("a/b. layer, %s (fused vs composed output: max difference %.1e of the largest value):" % (label, d))
        rows = compare([("a. fused forward", fused_fwd), ("b. composed forward", comp_fwd),
                        ("a. fused forward + backward", lambda: step(fused)), ("b. composed forward + backward", lambda: step(comp))],
                       iters, windows)
        report(out, rows)
        t = {name: (med, lo, hi) for name, med, lo, hi in rows}
        ok = True
        for what in ("forward", "forward + backward"):
            fa, co = t["a. fused " + what], t["b. composed " + what]
            good = fa[2] < co[1]
            ok = ok and good
            out.append("  %-19s composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
                       % (what + ":", co[0] / fa[0], fa[2], co[1], "below" if good else "NOT below"))
        verdicts.append((label, ok, t["b. composed forward + backward"][0] / t["a. fused forward + backward"][0]))
        sdpa_rows(out, layer, x, mask, dy, T, H, D, iters, windows)
        del layer
        torch.cuda.empty_cache()


def sdpa_rows(out, layer, x, mask, dy, T, H, D, iters, windows):
    """torch's scaled_dot_product_attention on pre-projected q, k, v, eager: events around `iters` calls, `windows` times."""
    try:
        with torch.no_grad():
            q, k, v = (torch.matmul(x.detach(), w).reshape(B, T, H, D).permute(0, 2, 1, 3).contiguous() for w in layer._flat())
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        key_mask = mask.reshape(B, 1, 1, T)
        g = dy.reshape(B, T, H, D).permute(0, 2, 1, 3).contiguous()
        sdpa = torch.nn.functional.scaled_dot_product_attention

        def fwd():
            with torch.no_grad():
                sdpa(q, k, v, attn_mask=key_mask)

        def both():
            q.grad = k.grad = v.grad = None
            sdpa(q, k, v, attn_mask=key_mask).backward(g)
        for name, fn in (("c. SDPA on projected q, k, v, forward (eager)", fwd), ("c. SDPA ..., forward + backward (eager)", both)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / iters)
            report(out, [(name, float(np.median(times)), min(times), max(times))])
        out.append("  (SDPA: no projections, masked rows not zeroed; a smaller computation, listed for scale)")
    except Exception as e:      # a build without a kernel for the shape or the mask: say so and go on
        out.append("  c. scaled_dot_product_attention: not measured (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:120]))


def floor_rows(out, iters, windows, dev):
    for T, K, H, D in SHAPES:
        HD = H * D
        x, mask, lens = make_inputs(T, K, dev)
        layer = make_layer(H, D, x, mask)
        w = [p.detach().clone().requires_grad_() for p in layer._flat()]
        g = torch.randn(B, T, HD, device=dev)

        def fwd():
            with torch.no_grad():
                Fn.seq_self_attention(x, mask, *w, H)

        def both():
            x.grad = None
            for p in w:
                p.grad = None
            Fn.seq_self_attention(x, mask, *w, H).backward(g)
        live = int(lens.sum())
        pairs = int((lens.astype(np.int64) ** 2).sum())
        # forward: x in, out out (no_grad: nothing is saved); with the backward: x in twice, out out, saved (q, k, v) out and in, g in, dx out
        fwd_bytes = 4 * B * T * (K + HD)
        both_bytes = 4 * B * T * (2 * K + HD + 6 * HD + HD + K)
        # forward: three projections, q k^T and p v; backward: dp = g v^T, dv, dq, dk and the four products with the weights
        fwd_flops = 6.0 * K * HD * live + 4.0 * HD * pairs
        bwd_flops = 12.0 * K * HD * live + 8.0 * HD * pairs
        out.append("d. the bare op (functional.seq_self_attention), T = %d, K = %d, %d heads of %d, %d live positions of %d, %d live (row, key) pairs:"
                   % (T, K, H, D, live, B * T, pairs))
        rows = compare([("forward", fwd), ("forward + backward", both)], iters, windows)
        report(out, rows)
        for (name, med, _, _), nbytes, flops in zip(rows, (fwd_bytes, both_bytes), (fwd_flops, fwd_flops + bwd_flops)):
            out.append("  %-20s byte floor %.2f MB = %.4f ms at 8 TB/s: %.1f %% of it;  %.2f GFLOP = %.4f ms at %.1f TFLOP/s fp32 matrix: %.2f %% of it"
                       % (name, nbytes / 1e6, nbytes / HBM_PEAK * 1e3, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), flops / 1e9,
                          flops / FP32_MATRIX_PEAK * 1e3, FP32_MATRIX_PEAK / 1e12, 100.0 * flops / FP32_MATRIX_PEAK / (med * 1e-3)))
        del layer
        torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev):
    rng = np.random.default_rng(2021)
    F, K, T = 8, 16, 50
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
        model = models.CTRModel(fi, models.BST()).to(dev)
        model(None, idx, hist)
        if variant != "fused":
            model.body.behaviors[0].atten.fits_kernel_menu = lambda x: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, hist)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("BST step: " + variant, step))
        keep.append((model, opt))
    out.append("e. captured models.BST training step (optim.Adam, %d one-id fields of %d rows, one history of %d + the candidate, K = %d, 2 heads):"
               % (F, V, T, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s (reported, not gated)"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,d,e")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["seq_attn_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d, lengths uniform in 1..T; (T, K, H, D) in %s" % (B, list(SHAPES))]
    for T, K, H, D in SHAPES:
        plan = Fn.seq_attn_plan(B, T, K, H, D)
        out.append("fil_seqattn_plan T = %d K = %d H = %d D = %d: %d samples per workgroup, grid %d of at most %d, %d parameter-gradient partials, "
                   "LDS %d / %d bytes fwd / bwd" % (T, K, H, D, plan["tile"], plan["grid"], plan["cap"], plan["partials"], plan["lds_fwd"], plan["lds_bwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", lambda *a: layer_rows(*a, verdicts)), ("d", floor_rows), ("e", model_rows)):
        if part in args.parts.split(","):
            out.append("")
            n = len(out)
            fn(out, args.iters, args.windows, dev)
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
