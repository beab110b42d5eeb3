"""Time-stream GRU over a behaviour sequence with event gaps: the fused kernels (fil_tsgru_fwd / fil_tsgru_bwd behind
layers.TimeStreamGRULayer) beside the layer's own composed path (functional.ts_gru_graph: the same math in torch ops, one substep at
a time) and beside the plain fused GRU of the same shape.

    python tools/ts_gru_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r32_ts_gru_bench.txt)

Shape: B = 4096 samples, lengths uniform in 1..T, gaps uniform in [0, 2].  Configurations: T = 50 with K = H = 16 and 32 at S = 2
substeps, and T = 20, K = H = 16 at S = 1 and 4.  The layer runs as models.DTS uses it: the last state and z out.
  a. fused        layers.TimeStreamGRULayer: forward alone (no_grad), and forward + backward with the gradients of x and all weights.
  b. composed     the same layer's _composed path (ts_gru_graph), the same weights, captured: about 10 + 4 S launches per step.
  c. bare op      functional.ts_gru forward and forward + backward against the bytes it cannot avoid (x, dt, hs and `saved` read and
                  written once, at the 8 TB/s HBM peak), and functional.gru at the same shape beside it: the price of the substeps
                  over the plain fused GRU.  Reported, not gated.
  d. DTS step     a whole captured training step of models.DTS under optim.Adam: the fused layer beside the same model with the layer
                  forced onto the composed path.
Timings are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window by
window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the end
(exit status 1 if it fails): in every configuration, forward and forward + backward, and for the DTS step, the slowest fused window
is below the fastest composed window."""
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
CONFIGS = [(50, 16, 2), (50, 32, 2), (20, 16, 1), (20, 16, 4)]      # T, K = H, S
HBM_PEAK = 8.0e12


def make_inputs(T, K, dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    x = (torch.randn(B, T, K, device=dev) * 0.5).requires_grad_()
    dt = torch.tensor(rng.uniform(0, 2, (B, T)), dtype=torch.float32, device=dev)
    dt_out = torch.tensor(rng.uniform(0, 2, B), dtype=torch.float32, device=dev)
    return x, dt, dt_out, mask, int(lens.sum())


def make_layer(H, S, x, dt, dt_out, mask):
    layer = layers.TimeStreamGRULayer(H, steps=S, return_sequences=False)
    with torch.no_grad():
        layer([x.detach(), dt, dt_out], mask=mask)
        layer.bias.normal_(0.0, 0.1)          # (Keras' biases start at zero)
        layer.ode_bias.normal_(0.0, 0.1)
    assert layer.fits_kernel_menu(x)
    return layer


def layer_rows(out, iters, windows, dev, verdicts):
    for T, K, S in CONFIGS:
        H = K
        x, dt, dt_out, mask, _ = make_inputs(T, K, dev)
        layer = make_layer(H, S, x, dt, dt_out, mask)
        dy, dz = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
        fused = lambda: layer([x, dt, dt_out], mask=mask)
        comp = lambda: layer._composed(x, dt, dt_out, mask)
        with torch.no_grad():
            d = max(float((f - c).abs().max() / c.abs().max()) for f, c in zip(fused(), comp()))

        def fused_fwd():
            with torch.no_grad():
                fused()

        def comp_fwd():
            with torch.no_grad():
                comp()

        def step(fn):
            x.grad = None
            layer.zero_grad(set_to_none=True)
            torch.autograd.backward(list(fn()), [dy, dz])
        label = "T = %d, K = H = %d, S = %d" % (T, K, S)
        out.append("a/b. layer, %s (fused vs composed outputs: max difference %.1e of the largest value):" % (label, d))
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
        del layer
        torch.cuda.empty_cache()


def floor_rows(out, iters, windows, dev):
    for T, K, S in CONFIGS:
        H = K
        x, dt, dt_out, mask, live = make_inputs(T, K, dev)
        layer = make_layer(H, S, x, dt, dt_out, mask)
        w = [p.detach().clone().requires_grad_() for p in layer._weights()]
        g, gz = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)

        def fwd():
            with torch.no_grad():
                Fn.ts_gru(x, dt, dt_out, mask, *w, steps=S, return_sequences=False)

        def both():
            x.grad = None
            for p in w:
                p.grad = None
            torch.autograd.backward(list(Fn.ts_gru(x, dt, dt_out, mask, *w, steps=S, return_sequences=False)), [g, gz])

        def gru_fwd():
            with torch.no_grad():
                Fn.gru(x, None, mask, *w[:3], return_sequences=False)

        def gru_both():
            x.grad = None
            for p in w:
                p.grad = None
            Fn.gru(x, None, mask, *w[:3], return_sequences=False).backward(g)
        # forward: x and dt in, hs out (no_grad: nothing is saved); with the backward: x and dt in twice, hs out, `saved` out and in
        # ((4 + 2 S) H floats per step), dx out
        planes = 4 + 2 * S
        fwd_bytes = 4 * B * T * (K + 1 + H)
        both_bytes = 4 * B * T * (2 * K + 2 + H + 2 * planes * H + K)
        out.append("c. the bare op (functional.ts_gru), T = %d, K = H = %d, S = %d, %d live steps of %d:" % (T, K, S, live, B * T))
        rows = compare([("ts_gru forward", fwd), ("gru forward", gru_fwd), ("ts_gru forward + backward", both),
                        ("gru forward + backward", gru_both)], iters, windows)
        report(out, rows)
        t = {name: med for name, med, _, _ in rows}
        for what, nbytes in (("forward", fwd_bytes), ("forward + backward", both_bytes)):
            med = t["ts_gru " + what]
            out.append("  %-20s byte floor %.2f MB = %.4f ms at 8 TB/s: %.1f %% of it;  %.2f us per step;  %.2fx the plain fused GRU"
                       % (what, nbytes / 1e6, nbytes / HBM_PEAK * 1e3, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), med * 1e3 / T,
                          med / t["gru " + what]))
        del layer
        torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev, verdicts):
    rng = np.random.default_rng(2021)
    F, K, T = 8, 16, 50
    idx = torch.tensor(rng.integers(1, V, (B, F)), device=dev)
    hist = rng.integers(1, V, (B, T))
    hist[np.arange(T)[None, :] >= rng.integers(1, T + 1, B)[:, None]] = 0
    hist = torch.tensor(hist.reshape(B, 1, T), device=dev)
    seq = (hist, torch.tensor(rng.uniform(0, 2, (B, 1, T)), dtype=torch.float32, device=dev),
           torch.tensor(rng.uniform(0, 2, (B, 1)), dtype=torch.float32, device=dev))
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info([V] * F, embed_dim=K)]
    steps, keep = [], []
    for variant in ("fused", "composed path forced"):
        torch.manual_seed(0)
        fi = models.DTSInput(info, behavior=[(info[0].fea_name, T)])
        model = models.CTRModel(fi, models.DTS()).to(dev)
        model(None, idx, seq)
        if variant != "fused":
            model.body.behaviors[0].fits_kernel_menu = lambda x: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, seq)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("DTS step: " + variant, step))
        keep.append((model, opt))
    out.append("d. captured models.DTS training step (optim.Adam, %d one-id fields of %d rows, one history of %d, K = %d, S = 2):" % (F, V, T, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    verdicts.append(("DTS step", good, rows[1][1] / rows[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,c,d")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["ts_gru_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d, lengths uniform in 1..T, gaps uniform in [0, 2]; configurations (T, K = H, S): %s" % (B, CONFIGS)]
    for T, K, S in CONFIGS:
        plan = Fn.ts_gru_plan(B, T, K, K, S)
        out.append("fil_tsgru_plan T = %d, K = H = %d, S = %d: %d samples per workgroup, grid %d of at most %d, %d parameter-gradient partials, LDS %d / %d bytes fwd / bwd"
                   % (T, K, S, plan["tile"], plan["grid"], plan["cap"], plan["partials"], plan["lds_fwd"], plan["lds_bwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", lambda *a: layer_rows(*a, verdicts)), ("c", floor_rows), ("d", lambda *a: model_rows(*a, verdicts))):
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
