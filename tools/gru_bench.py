"""GRU / AUGRU over a behaviour sequence: the fused kernels (fil_gru_fwd / fil_gru_bwd behind layers.GRULayer) beside the layer's own
composed path (the same math in torch ops, one step at a time) and, for the plain GRU, torch.nn.GRU (MIOpen).

    python tools/gru_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r26_gru_bench.txt)

Shape: B = 4096 samples, T = 50 steps (lengths uniform in 1..50), K = H = 16; also K = H = 32.  Variants: the GRU with the sequence
out, and the AUGRU with the last state out.
  a. fused        layers.GRULayer: forward alone (no_grad), and forward + backward with the gradients of x, the scores and the weights.
  b. composed     the same layer's _composed path (gru_graph), the same weights, captured.
  c. torch.nn.GRU plain GRU only, EAGER timing (not a graph replay): MIOpen's gate order is r | z | n and its masking differs (none:
                  all T steps run), so it is a different computation of the same size and NOT bit-comparable; listed for scale.
  d. bare op      functional.gru forward and forward + backward against the bytes it cannot avoid (x, hs and `saved` read and written
                  once, at the 8 TB/s HBM peak) and against its fp32 FLOP count (6 (K + H) H per live step forward, three times that
                  with the backward) at the fp32 matrix peak.  Reported, not gated.
  e. DIEN step    a whole captured training step of models.DIEN under optim.Adam: the fused layers beside the same model with its
                  GRU layers forced onto the composed path.
Timings a, b, d, e are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns
window by window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check
at the end (exit status 1 if it fails): in every variant and at both widths, forward and forward + backward, the slowest fused
window is below the fastest composed window."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pool_bench import compare, report  # noqa: E402
from ml_function_amd import functional as Fn, layers, losses, models, optim  # noqa: E402

B, T, V = 4096, 50, 10_000
WIDTHS = (16, 32)
HBM_PEAK = 8.0e12
FP32_MATRIX_PEAK = 157.3e12
VARIANTS = [("gru", True, "GRU, sequence out"), ("augru", False, "AUGRU, last state out")]


def make_inputs(K, dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    x = (torch.randn(B, T, K, device=dev) * 0.5).requires_grad_()
    a = torch.rand(B, T, device=dev).requires_grad_()
    return x, a, mask, int(lens.sum())


def make_layer(mode, seq, H, x, a, mask):
    layer = layers.GRULayer(H, mode=mode, return_sequences=seq)
    with torch.no_grad():
        layer(x.detach() if mode == "gru" else [x.detach(), a.detach()], mask=mask)
        layer.bias.normal_(0.0, 0.1)          # (Keras' biases start at zero)
    assert layer.fits_kernel_menu(x)
    return layer


def layer_rows(out, iters, windows, dev, verdicts):
    for K in WIDTHS:
        H = K
        x, a, mask, _ = make_inputs(K, dev)
        for mode, seq, label in VARIANTS:
            layer = make_layer(mode, seq, H, x, a, mask)
            inputs = x if mode == "gru" else [x, a]
            dy = torch.randn((B, T, H) if seq else (B, H), device=dev)
            fused = lambda: layer(inputs, mask=mask)
            comp = lambda: layer._composed(x, None if mode == "gru" else a, mask)
            with torch.no_grad():
                d = float((fused() - comp()).abs().max() / comp().abs().max())

            def fused_fwd():
                with torch.no_grad():
                    fused()

            def comp_fwd():
                with torch.no_grad():
                    comp()

            def step(fn):
                x.grad = a.grad = None
                layer.zero_grad(set_to_none=True)
                fn().backward(dy)
            out.append("a/b. layer, %s, K = H = %d (fused vs composed output: max difference %.1e of the largest value):" % (label, K, d))
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
            verdicts.append(("%s, K = H = %d" % (label, K), ok, t["b. composed forward + backward"][0] / t["a. fused forward + backward"][0]))
            if mode == "gru":
                miopen_rows(out, K, H, x, dy, iters, windows)
            del layer
            torch.cuda.empty_cache()


def miopen_rows(out, K, H, x, dy, iters, windows):
    """torch.nn.GRU, eager: events around `iters` calls, `windows` times."""
    try:
        rnn = torch.nn.GRU(K, H, batch_first=True).to(x.device)
        xd = x.detach().clone().requires_grad_()

        def fwd():
            with torch.no_grad():
                rnn(xd)

        def both():
            xd.grad = None
            rnn.zero_grad(set_to_none=True)
            rnn(xd)[0].backward(dy)
        for name, fn in (("c. torch.nn.GRU forward (eager)", fwd), ("c. torch.nn.GRU forward + backward (eager)", both)):
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
        out.append("  (MIOpen: gate order r | z | n, no masking -- all %d steps of every sample run; a different computation, not bit-comparable)" % T)
    except Exception as e:      # MIOpen without a kernel for the shape: say so and go on
        out.append("  c. torch.nn.GRU: not measured (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:120]))


def floor_rows(out, iters, windows, dev):
    for K in WIDTHS:
        H = K
        x, a, mask, live = make_inputs(K, dev)
        for mode, seq, label in VARIANTS:
            layer = make_layer(mode, seq, H, x, a, mask)
            w = [p.detach().clone().requires_grad_() for p in (layer.kernel, layer.recurrent_kernel, layer.bias)]
            sc = None if mode == "gru" else a
            g = torch.randn((B, T, H) if seq else (B, H), device=dev)

            def fwd():
                with torch.no_grad():
                    Fn.gru(x, sc, mask, *w, mode=mode, return_sequences=seq)

            def both():
                x.grad = a.grad = None
                for p in w:
                    p.grad = None
                Fn.gru(x, sc, mask, *w, mode=mode, return_sequences=seq).backward(g)
            # forward: x in, hs out (no_grad: nothing is saved); with the backward: x in twice, hs out and in, saved out and in, dx out
            fwd_bytes = 4 * B * T * (K + H)
            both_bytes = 4 * B * T * (2 * K + 2 * H + 8 * H + K)
            fwd_flops = 6.0 * (K + H) * H * live
            out.append("d. the bare op (functional.gru), %s, K = H = %d, %d live steps of %d:" % (label, K, live, B * T))
            rows = compare([("forward", fwd), ("forward + backward", both)], iters, windows)
            report(out, rows)
            for (name, med, _, _), nbytes, flops in zip(rows, (fwd_bytes, both_bytes), (fwd_flops, 3 * fwd_flops)):
                out.append("  %-20s byte floor %.2f MB = %.4f ms at 8 TB/s: %.1f %% of it;  %.2f GFLOP = %.4f ms at %.1f TFLOP/s fp32 matrix: %.2f %% of it"
                           % (name, nbytes / 1e6, nbytes / HBM_PEAK * 1e3, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), flops / 1e9,
                              flops / FP32_MATRIX_PEAK * 1e3, FP32_MATRIX_PEAK / 1e12, 100.0 * flops / FP32_MATRIX_PEAK / (med * 1e-3)))
            del layer
            torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev, verdicts):
    rng = np.random.default_rng(2021)
    F, K = 8, 16
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
        model = models.CTRModel(fi, models.DIEN()).to(dev)
        model(None, idx, hist)
        if variant != "fused":
            for layer in (model.body.behaviors[0].extract, model.body.behaviors[0].evolve):
                layer.fits_kernel_menu = lambda x: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, hist)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("DIEN step: " + variant, step))
        keep.append((model, opt))
    out.append("e. captured models.DIEN training step (optim.Adam, %d one-id fields of %d rows, one history of %d, K = %d, AUGRU):" % (F, V, T, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    verdicts.append(("DIEN step", good, rows[1][1] / rows[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,d,e")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["gru_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d T=%d (lengths uniform in 1..%d), K = H in %s; hs is %.1f MB at H = 16, saved four times that"
           % (B, T, T, list(WIDTHS), B * T * 16 * 4 / 1e6)]
    for K in WIDTHS:
        plan = Fn.gru_plan(B, T, K, K)
        out.append("fil_gru_plan K = H = %d: %d samples per workgroup, grid %d of at most %d, %d parameter-gradient partials, LDS %d / %d bytes fwd / bwd"
                   % (K, plan["tile"], plan["grid"], plan["cap"], plan["partials"], plan["lds_fwd"], plan["lds_bwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", lambda *a: layer_rows(*a, verdicts)), ("d", floor_rows), ("e", lambda *a: model_rows(*a, verdicts))):
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
