"""AFM pair-attention pooling with the softmax over the pairs: the fused kernels (fil_afm_fwd / fil_afm_bwd behind layers.AFMLayer)
beside the composed form (InnerLayer's pair tensor + AttentionBaseLayer(softmax_axis=1) in torch).

    python tools/afm_pool_bench.py [--iters 50] [--windows 5]          (GPU box; output: profiles/r24_afm_pool_bench.txt)

Shape: B = 4096 samples, F = 39 fields, K = 16, attention_dim A = 4 (P = 741 pairs), both score forms (reference op order
relu(u . h), and hidden_relu = the paper's relu(u) . h).  The composed form materialises [B,P,K] (194 MB) forward and backward.
  a. fused        layers.AFMLayer on the packed field embeddings: forward alone (no_grad), and forward + backward with the
                  gradients of the embeddings and of every weight.
  b. composed     the same through layers.InnerLayer pairs + layers.AttentionBaseLayer(softmax_axis=1), the same weights.
  c. byte floor   the bare op (functional.afm_pool, no Dense), forward + backward, against the bytes it cannot avoid:
                  B (2 F K + 2 K) 4 -- the embeddings in, their gradient out, pooled out, its gradient in -- at the 8 TB/s HBM peak.
  d. AFM step     a whole captured training step of models.AFM under optim.Adam (39 fields of 10,000 rows, tables in runs mode,
                  binary cross-entropy): pair_softmax=True on the fused path beside the same model with the composed layers wired in.
Every timing is a replay of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window
by window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the
end (exit status 1 if it fails): fused forward + backward is faster than composed, and the slowest fused window is below the fastest
composed window, for both score forms."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_function_amd import functional as Fn, layers, losses, models, optim  # noqa: E402

B, F, K, A, V = 4096, 39, 16, 4, 10_000
P = F * (F - 1) // 2
HBM_PEAK = 8.0e12
FORMS = (("reference form", False), ("paper form (hidden_relu)", True))


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


def compare(variants, iters, windows):
    """variants: [(name, fn)] -> [(name, median ms, min ms, max ms)]; the graphs take turns window by window."""
    graphs = [(name, graph_of(fn)) for name, fn in variants]
    for _, g in graphs:
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in graphs}
    for _ in range(windows):
        for name, g in graphs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
    return [(name, float(np.median(t)), min(t), max(t)) for name, t in times.items()]


def report(out, rows):
    for name, med, lo, hi in rows:
        out.append("  %-44s %9.4f ms   (windows %.4f .. %.4f)" % (name, med, lo, hi))


def layer_pair(hidden_relu, emb):
    """(fused AFMLayer, InnerLayer, composed AttentionBaseLayer) with the same weights, built on `emb`."""
    fused = layers.AFMLayer(attention_dim=A, hidden_relu=hidden_relu)
    inner = layers.InnerLayer()
    comp = layers.AttentionBaseLayer(attention_dim=A, softmax_axis=1, hidden_relu=hidden_relu)
    with torch.no_grad():
        fused(emb)
        comp(inner(emb))
    comp.load_state_dict(fused.state_dict())
    assert fused.fits_kernel_menu(emb)
    return fused, inner, comp


def layer_rows(out, iters, windows, dev, verdicts):
    emb = (torch.randn(B, F, K, device=dev) * 0.5).requires_grad_()
    dy = torch.randn(B, 1, device=dev)
    for label, hidden_relu in FORMS:
        fused, inner, comp = layer_pair(hidden_relu, emb.detach())
        with torch.no_grad():
            d = float((fused(emb) - comp(inner(emb))).abs().max() / comp(inner(emb)).abs().max())

        def fused_fwd():
            with torch.no_grad():
                fused(emb)

        def comp_fwd():
            with torch.no_grad():
                comp(inner(emb))

        def fused_step():
            emb.grad = None
            fused.zero_grad(set_to_none=True)
            fused(emb).backward(dy)

        def comp_step():
            emb.grad = None
            comp.zero_grad(set_to_none=True)
            comp(inner(emb)).backward(dy)
        out.append("a/b. layer, %s (fused vs composed output: max difference %.1e of the largest value):" % (label, d))
        rows = compare([("a. fused forward", fused_fwd), ("b. composed forward", comp_fwd),
                        ("a. fused forward + backward", fused_step), ("b. composed forward + backward", comp_step)], iters, windows)
        report(out, rows)
        t = {name: (med, lo, hi) for name, med, lo, hi in rows}
        fa, co = t["a. fused forward + backward"], t["b. composed forward + backward"]
        out.append("  forward + backward: composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms"
                   % (co[0] / fa[0], fa[2], co[1]))
        out.append("  forward alone:      composed / fused = %.1fx (medians)" % (t["b. composed forward"][0] / t["a. fused forward"][0]))
        verdicts.append((label, fa[0] < co[0] and fa[2] < co[1], co[0] / fa[0]))
        del fused, inner, comp
        torch.cuda.empty_cache()


def floor_rows(out, iters, windows, dev):
    emb = (torch.randn(B, F, K, device=dev) * 0.5).requires_grad_()
    w = (torch.randn(K, A, device=dev) * 0.5).requires_grad_()
    b = (torch.randn(A, device=dev) * 0.1).requires_grad_()
    h = torch.randn(A, 1, device=dev).requires_grad_()
    g = torch.randn(B, K, device=dev)
    fwd_bytes = B * (F * K + K) * 4
    both_bytes = B * (2 * F * K + 2 * K) * 4
    for label, hidden_relu in FORMS:
        def fwd():
            with torch.no_grad():
                Fn.afm_pool(emb, w, b, h, hidden_relu=hidden_relu)

        def both():
            emb.grad = w.grad = b.grad = h.grad = None
            Fn.afm_pool(emb, w, b, h, hidden_relu=hidden_relu).backward(g)
        out.append("c. the bare op (functional.afm_pool), %s:" % label)
        rows = compare([("forward", fwd), ("forward + backward", both)], iters, windows)
        report(out, rows)
        for (name, med, _, _), nbytes in zip(rows, (fwd_bytes, both_bytes)):
            out.append("  %-20s byte floor %.2f MB = %.4f ms at 8 TB/s: the op runs at %.1f %% of it (%.2f TB/s of floor bytes)"
                       % (name, nbytes / 1e6, nbytes / HBM_PEAK * 1e3, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), nbytes / (med * 1e-3) / 1e12))


class ComposedAFM(torch.nn.Module):
    """models.AFM(pair_softmax=True) with the comparator wired in by hand: InnerLayer pairs + AttentionBaseLayer(softmax_axis=1)."""

    def __init__(self, hidden_relu):
        super().__init__()
        self.inner = layers.InnerLayer()
        self.atten = layers.AttentionBaseLayer(softmax_axis=1, hidden_relu=hidden_relu)
        self.score = layers.ScoreLayer(use_add=True)

    def forward(self, inputFea):
        return self.score(list(inputFea.linear_embed) + [self.atten(self.inner(inputFea.sparse_embed))])


def model_rows(out, iters, windows, dev):
    rng = np.random.default_rng(2021)
    idx = torch.tensor(rng.integers(0, V, (B, F)), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info([V] * F, embed_dim=K)]
    for label, hidden_relu in FORMS:
        steps, keep = [], []
        for variant in ("fused (pair_softmax=True)", "composed layers wired in"):
            torch.manual_seed(0)
            fi = models.FeatureInput(sparseInfo=info, useLinear=True, useFlattenLinear=True, tableGrad="runs")
            body = models.AFM(pair_softmax=True, hidden_relu=hidden_relu) if variant.startswith("fused") else ComposedAFM(hidden_relu)
            model = models.CTRModel(fi, body).to(dev)
            model(None, idx)
            opt = optim.Adam(model.parameters())

            def step(model=model, opt=opt):
                opt.zero_grad(set_to_none=True)
                p = model(None, idx)[:, 0]
                losses.binary_crossentropy(p, y, eps=1e-6).backward()
                opt.step()
            steps.append(("AFM step: " + variant, step))
            keep.append((model, opt))
        out.append("d. captured models.AFM training step (optim.Adam, tables in runs mode), %s:" % label)
        rows = compare(steps, iters, windows)
        report(out, rows)
        out.append("  composed / fused = %.1fx (medians)" % (rows[1][1] / rows[0][1]))
        del steps, keep
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,c,d")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    plan = Fn.afm_plan(B, F, K, A)
    out = ["afm_pool_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d F=%d K=%d A=%d, P=%d pairs; the pair tensor [B,P,K] is %.0f MB; inputs %.1f MB, pooled %.2f MB"
           % (B, F, K, A, P, B * P * K * 4 / 1e6, B * F * K * 4 / 1e6, B * K * 4 / 1e6),
           "fil_afm_plan: %d samples (waves) per workgroup, grid %d of at most %d, %d parameter-gradient partials, LDS %d / %d bytes fwd / bwd"
           % (plan["tile"], plan["grid"], plan["cap"], plan["partials"], plan["lds_fwd"], plan["lds_bwd"]),
           "HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters)]
    verdicts = []
    for part, fn in (("ab", lambda *a: layer_rows(*a, verdicts)), ("c", floor_rows), ("d", model_rows)):
        if part in args.parts.split(","):
            out.append("")
            n = len(out)
            fn(out, args.iters, args.windows, dev)
            print("\n".join(out[n:]), flush=True)
    out.append("")
    for label, ok, ratio in verdicts:
        out.append("direction check, %s: %s (fused forward + backward %.1fx faster than composed; every fused window below every composed window: %s)"
                   % (label, "PASS" if ok else "FAIL", ratio, "yes" if ok else "no"))
    print("\n" + "\n".join(out))
    return 0 if all(ok for _, ok, _ in verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
