"""LSTM over a sequence, one direction and both in one launch: the fused kernels (fil_lstm_fwd / fil_lstm_bwd behind layers.LSTMLayer
and layers.BiLSTMLayer) beside the layers' own composed path (the same math in torch ops, one step at a time).

    python tools/lstm_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r28_lstm_bench.txt)

Shapes: B = 4096 samples, K = H = 16 and 32; T = 50 steps (lengths uniform in 1..50), one direction and bidirectional, and T = 5 (the
session count of models.DSIN; 1..5 live sessions), bidirectional.  Sequence out everywhere.
  a. fused        the layer: forward alone (no_grad), and forward + backward with the gradients of x and of every weight.
  b. composed     the same layer's _composed path (lstm_graph), the same weights, captured.  The reference of the direction check.
  c. one launch   functional.lstm "bidirectional" beside a "forward" and a "reverse" call of this same library on one stream, their
                  outputs concatenated (and their dx added by autograd).  Reported, not gated.
  d. scale        functional.gru (fil_gru_*) at the same shape beside functional.lstm in one direction: an LSTM step has 4/3 of the
                  GRU's products.  Reported, not gated.
  e. DSIN step    a whole captured training step of models.DSIN under optim.Adam: the fused layers beside the same model with its
                  BiLSTMLayer forced onto the composed path.
Timings are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window by
window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the end
(exit status 1 if it fails): in every variant of a / b and at both widths, forward and forward + backward, and in e, the slowest
fused window is below the fastest composed window."""
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
WIDTHS = (16, 32)
VARIANTS = [(50, "forward", "T = 50, one direction"), (50, "bidirectional", "T = 50, bidirectional"), (5, "bidirectional", "T = 5, bidirectional")]


def make_inputs(T, K, dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    x = (torch.randn(B, T, K, device=dev) * 0.5).requires_grad_()
    return x, mask, int(lens.sum())


def make_layer(direction, H, x, mask):
    layer = layers.BiLSTMLayer(H) if direction == "bidirectional" else layers.LSTMLayer(H, go_backwards=direction == "reverse")
    with torch.no_grad():
        layer(x.detach(), mask=mask)
        for name, p in layer.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)          # (Keras' biases start at zero and one)
    assert layer.fits_kernel_menu(x)
    return layer


def layer_rows(out, iters, windows, dev, verdicts):
    for K in WIDTHS:
        H = K
        for T, direction, label in VARIANTS:
            x, mask, _ = make_inputs(T, K, dev)
            layer = make_layer(direction, H, x, mask)
            dy = torch.randn((B, T, (2 if direction == "bidirectional" else 1) * H), device=dev)
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
            del layer
            torch.cuda.empty_cache()


def launch_rows(out, iters, windows, dev):
    """c: both directions in one launch beside two one-direction calls; d: the GRU at the same shape."""
    for K in WIDTHS:
        H = K
        for T in (50, 5):
            x, mask, live = make_inputs(T, K, dev)
            bi = make_layer("bidirectional", H, x, mask)
            w = [p.detach().clone().requires_grad_() for p in bi._weights()]
            halves = [[p[d].detach().clone().requires_grad_() for p in w] for d in range(2)]
            g = torch.randn(B, T, 2 * H, device=dev)
            gru = layers.GRULayer(H)
            with torch.no_grad():
                gru(x.detach(), mask=mask)
            wg = [p.detach().clone().requires_grad_() for p in (gru.kernel, gru.recurrent_kernel, gru.bias)]
            every = w + halves[0] + halves[1] + wg

            def clear():
                x.grad = None
                for p in every:
                    p.grad = None

            one = lambda: Fn.lstm(x, mask, *w, direction="bidirectional")
            two = lambda: torch.cat([Fn.lstm(x, mask, *halves[0], direction="forward"), Fn.lstm(x, mask, *halves[1], direction="reverse")], dim=-1)
            lstm1 = lambda: Fn.lstm(x, mask, *halves[0], direction="forward")
            gru1 = lambda: Fn.gru(x, None, mask, *wg)
            with torch.no_grad():
                assert torch.equal(one(), two())

            def fwd(fn):
                def run():
                    with torch.no_grad():
                        fn()
                return run

            def both(fn, dy):
                def run():
                    clear()
                    fn().backward(dy)
                return run
            out.append("c. functional.lstm, both directions, T = %d, K = H = %d, %d live steps of %d (the two forms return the same bits):"
                       % (T, K, live, B * T))
            rows = compare([("one bidirectional launch: forward", fwd(one)), ("a forward and a reverse call: forward", fwd(two)),
                            ("one bidirectional launch: forward + backward", both(one, g)),
                            ("a forward and a reverse call: forward + backward", both(two, g))], iters, windows)
            report(out, rows)
            out.append("  two calls / one launch = %.2fx forward, %.2fx forward + backward (medians)"
                       % (rows[1][1] / rows[0][1], rows[3][1] / rows[2][1]))
            out.append("d. one direction beside functional.gru, T = %d, K = H = %d:" % (T, K))
            rows = compare([("lstm forward", fwd(lstm1)), ("gru forward", fwd(gru1)), ("lstm forward + backward", both(lstm1, g[..., :H].contiguous())),
                            ("gru forward + backward", both(gru1, g[..., :H].contiguous()))], iters, windows)
            report(out, rows)
            out.append("  lstm / gru = %.2fx forward, %.2fx forward + backward (medians; 4/3 = 1.33x by the products)"
                       % (rows[0][1] / rows[1][1], rows[2][1] / rows[3][1]))
            del bi, gru
            torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev, verdicts):
    rng = np.random.default_rng(2021)
    F, K, T, S = 8, 16, 50, 5
    idx = torch.tensor(rng.integers(1, V, (B, F)), device=dev)
    hist = rng.integers(1, V, (B, T))
    hist[np.arange(T)[None, :] >= rng.integers(1, T + 1, B)[:, None]] = 0
    hist = torch.tensor(hist.reshape(B, 1, T), device=dev)
    y = torch.tensor(rng.integers(0, 2, B), dtype=torch.float32, device=dev)
    info = [i._replace(emb_reg=0.0) for i in models.make_sparse_info([V] * F, embed_dim=K)]
    steps, keep = [], []
    for variant in ("fused", "LSTM on the composed path"):
        torch.manual_seed(0)
        fi = models.DINInput(info, behavior=[(info[0].fea_name, T)])
        model = models.CTRModel(fi, models.DSIN(S)).to(dev)
        model(None, idx, hist)
        if variant != "fused":
            model.body.behaviors[0].interact.fits_kernel_menu = lambda x: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, hist)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("DSIN step: " + variant, step))
        keep.append((model, opt))
    out.append("e. captured models.DSIN training step (optim.Adam, %d one-id fields of %d rows, one history of %d in %d sessions, K = %d):"
               % (F, V, T, S, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    verdicts.append(("DSIN step", good, rows[1][1] / rows[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,cd,e")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["lstm_bench: %s" % torch.cuda.get_device_name(0),
           "B=%d, T = 50 (lengths uniform in 1..50) and T = 5 (1..5), K = H in %s; at T = 50, H = 16 one direction's hs is %.1f MB, its saved five times that"
           % (B, list(WIDTHS), B * 50 * 16 * 4 / 1e6)]
    for K in WIDTHS:
        for T in (50, 5):
            for direction in ("forward", "bidirectional"):
                plan = Fn.lstm_plan(B, T, K, K, direction)
                out.append("fil_lstm_plan %s T = %d K = H = %d: %d samples per workgroup, grid %d per direction of at most %d, %d parameter-gradient "
                           "partials, LDS %d / %d bytes fwd / bwd" % (direction, T, K, plan["tile"], plan["grid"], plan["cap"], plan["partials"],
                                                                      plan["lds_fwd"], plan["lds_bwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", lambda *a: layer_rows(*a, verdicts)), ("cd", launch_rows), ("e", lambda *a: model_rows(*a, verdicts))):
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
