"""DIN attention pooling over a behaviour sequence: the fused kernels (fil_din_fwd / fil_din_bwd behind layers.DinAttentionLayer)
beside the layer's own composed path (the same graph in torch ops, which materialises [B,T,4K] and [B,T,H1]).

    python tools/din_attn_bench.py [--iters 50] [--windows 5]          (GPU box; output: profiles/r25_din_attn_bench.txt)

Shape: B = 4096 samples, T = 50 history slots (lengths uniform in 1..50), K = 16, hidden units (80, 40); both activations (PReLU,
sigmoid) and both modes (raw scores, softmax over the live slots).
  a. fused        layers.DinAttentionLayer: forward alone (no_grad), and forward + backward with the gradients of the query, the
                  keys and every weight.
  b. composed     the same layer's _composed path, the same weights.
  c. byte floor   the bare op (functional.din_attention), forward + backward, against the bytes it cannot avoid:
                  4 B (2 T K + 3 K + T) -- the keys in, their gradient out, the [B,K] rows, the mask -- at the 8 TB/s HBM peak.
  d. DIN step     a whole captured training step of models.DIN under optim.Adam (binary cross-entropy): the fused layer beside
                  the same model with the layer forced onto its composed path.
Every timing is a replay of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window
by window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the
end (exit status 1 if it fails): for every activation and mode fused forward + backward is faster than composed, and the slowest
fused window is below the fastest composed window."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pool_bench import compare, graph_of, report  # noqa: E402,F401
from ml_function_amd import functional as Fn, layers, losses, models, optim  # noqa: E402

B, T, K, HIDDEN, V = 4096, 50, 16, (80, 40), 10_000
HBM_PEAK = 8.0e12
VARIANTS = [(act, sm) for act in ("prelu", "sigmoid") for sm in (False, True)]


def label_of(act, sm):
    return "%s, %s" % (act, "softmax" if sm else "raw")


def make_inputs(dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    q = (torch.randn(B, K, device=dev) * 0.5).requires_grad_()
    keys = (torch.randn(B, T, K, device=dev) * 0.5).requires_grad_()
    return q, keys, mask, float(lens.mean())


def make_layer(act, sm, q, keys, mask):
    layer = layers.DinAttentionLayer(hidden_units=HIDDEN, activation=act, softmax=sm)
    with torch.no_grad():
        layer([q.detach(), keys.detach()], mask=mask)
        for name, p in layer.named_parameters():          # Keras' zero biases and slopes would hide half of the backward
            if name.endswith(("b1", "b2", "b3")):
                p.normal_(0.0, 0.1)
            elif "alpha" in name:
                p.uniform_(0.0, 0.3)
    assert layer.fits_kernel_menu(q, keys)
    return layer


def layer_rows(out, iters, windows, dev, verdicts):
    q, keys, mask, _ = make_inputs(dev)
    dy = torch.randn(B, 1, K, device=dev)
    for act, sm in VARIANTS:
        layer = make_layer(act, sm, q, keys, mask)
        fused = lambda: layer([q, keys], mask=mask)
        comp = lambda: layer._composed(q, keys, mask).unsqueeze(1)
        with torch.no_grad():
            d = float((fused() - comp()).abs().max() / comp().abs().max())

        def fused_fwd():
            with torch.no_grad():
                fused()

        def comp_fwd():
            with torch.no_grad():
                comp()

        def step(fn):
            q.grad = keys.grad = None
            layer.zero_grad(set_to_none=True)
            fn().backward(dy)
        out.append("a/b. layer, %s (fused vs composed output: max difference %.1e of the largest value):" % (label_of(act, sm), d))
        rows = compare([("a. fused forward", fused_fwd), ("b. composed forward", comp_fwd),
                        ("a. fused forward + backward", lambda: step(fused)), ("b. composed forward + backward", lambda: step(comp))],
                       iters, windows)
        report(out, rows)
        t = {name: (med, lo, hi) for name, med, lo, hi in rows}
        fa, co = t["a. fused forward + backward"], t["b. composed forward + backward"]
        out.append("  forward + backward: composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms"
                   % (co[0] / fa[0], fa[2], co[1]))
        out.append("  forward alone:      composed / fused = %.1fx (medians)" % (t["b. composed forward"][0] / t["a. fused forward"][0]))
        verdicts.append((label_of(act, sm), fa[0] < co[0] and fa[2] < co[1], co[0] / fa[0]))
        del layer
        torch.cuda.empty_cache()


def floor_rows(out, iters, windows, dev):
    q, keys, mask, _ = make_inputs(dev)
    g = torch.randn(B, K, device=dev)
    fwd_bytes = 4 * B * (T * K + 2 * K) + B * T
    both_bytes = 4 * B * (2 * T * K + 3 * K + T)
    for act, sm in VARIANTS:
        layer = make_layer(act, sm, q, keys, mask)
        w = [None if p is None else p.detach().clone().requires_grad_() for p in layer._weights()]      # (the slopes: None with the sigmoid)

        def fwd():
            with torch.no_grad():
                Fn.din_attention(q, keys, mask, *w, softmax=sm, activation=act)

        def both():
            q.grad = keys.grad = None
            for p in w:
                if p is not None:
                    p.grad = None
            Fn.din_attention(q, keys, mask, *w, softmax=sm, activation=act).backward(g)
        out.append("c. the bare op (functional.din_attention), %s:" % label_of(act, sm))
        rows = compare([("forward", fwd), ("forward + backward", both)], iters, windows)
        report(out, rows)
        for (name, med, _, _), nbytes in zip(rows, (fwd_bytes, both_bytes)):
            out.append("  %-20s byte floor %.2f MB = %.4f ms at 8 TB/s: the op runs at %.1f %% of it (%.2f TB/s of floor bytes)"
                       % (name, nbytes / 1e6, nbytes / HBM_PEAK * 1e3, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), nbytes / (med * 1e-3) / 1e12))
        del layer
        torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev):
    rng = np.random.default_rng(2021)
    F = 8
    idx = torch.tensor(rng.integers(1, V, (B, F)), device=dev)
    hist = rng.integers(1, V, (B, T))
    hist[np.arange(T)[None, :] >= rng.integers(1, T + 1, B)[:, None]] = 0
    hist = torch.tensor(hist.reshape(B, 1, T), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info([V] * F, embed_dim=K)]
    for act, sm in VARIANTS:
        steps, keep = [], []
        for variant in ("fused", "composed path forced"):
            torch.manual_seed(0)
            fi = models.DINInput(info, behavior=[(info[0].fea_name, T)])
            model = models.CTRModel(fi, models.DIN(att_hidden_units=HIDDEN, att_activation=act, att_softmax=sm)).to(dev)
            model(None, idx, hist)
            if variant != "fused":
                model.body.atten[0].fits_kernel_menu = lambda q, k: False
            opt = optim.Adam(model.parameters())

            def step(model=model, opt=opt):
                opt.zero_grad(set_to_none=True)
                p = model(None, idx, hist)[:, 0]
                losses.binary_crossentropy(p, y, eps=1e-6).backward()
                opt.step()
            steps.append(("DIN step: " + variant, step))
            keep.append((model, opt))
        out.append("d. captured models.DIN training step (optim.Adam, %d one-id fields of %d rows, one history of %d), %s:" % (F, V, T, label_of(act, sm)))
        rows = compare(steps, iters, windows)
        report(out, rows)
        out.append("  composed / fused = %.2fx (medians)" % (rows[1][1] / rows[0][1]))
        del steps, keep
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,c,d")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    plan = Fn.din_plan(B, T, K, *HIDDEN)
    out = ["din_attn_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d T=%d K=%d hidden=%s; the composed path's [B,T,4K] block is %.0f MB and its [B,T,H1] block %.0f MB; keys %.1f MB, out %.2f MB"
           % (B, T, K, HIDDEN, B * T * 4 * K * 4 / 1e6, B * T * HIDDEN[0] * 4 / 1e6, B * T * K * 4 / 1e6, B * K * 4 / 1e6),
           "fil_din_plan: %d samples per workgroup, grid %d of at most %d, %d parameter-gradient partials, LDS %d / %d bytes fwd / bwd"
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
