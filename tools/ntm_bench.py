"""Neural Turing Machine memory read / write over a sequence: the fused kernels (fil_ntm_fwd / fil_ntm_bwd behind
functional.ntm_memory) beside the same math in torch ops, one step at a time (layers.behavior_layer.ntm_memory_graph, the composed
path of layers.NTMMemoryLayer).

    python tools/ntm_bench.py [--iters 30] [--windows 5]          (GPU box; output: profiles/r31_ntm_bench.txt)

Shape: B = 4096 samples, lengths uniform in 1..T.  Variants: T = 50 with H = D = 16, m = 4; T = 50 with H = D = 32, m = 8; T = 20
with H = D = 16, m = 4.  Sequence of reads and the final memory out, both with an upstream gradient.
  a. fused        functional.ntm_memory: forward alone (no_grad), and forward + backward with the gradients of h, Wp, bp and M0;
                  beside the bytes it cannot avoid (h, rs and `saved` read and written once, at the 8 TB/s HBM peak) and per step.
                  Reported, not gated.
  b. composed     ntm_memory_graph on the same tensors, captured.
  c. MIMN step    a whole captured training step of models.MIMN under optim.Adam: the fused layers beside the same model with its
                  memory layer forced onto the composed path.
Timings are replays of a HIP graph: --windows windows of --iters replays each, the variants of a comparison taking turns window by
window; reported: the median window's time per replay and the spread (min .. max) over the windows.  The direction check at the end
(exit status 1 if it fails): in every variant, forward and forward + backward, the slowest fused window is below the fastest
composed window."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pool_bench import compare, report  # noqa: E402
from ml_function_amd import functional as Fn, layers, losses, models, optim  # noqa: E402
from ml_function_amd.layers.behavior_layer import ntm_memory_graph  # noqa: E402

B, V = 4096, 10_000
SHAPES = ((50, 16, 4, 16), (50, 32, 8, 32), (20, 16, 4, 16))          # T, H, m, D
HBM_PEAK = 8.0e12


def make_inputs(T, H, m, D, dev, seed=2021):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    mask = torch.tensor(np.arange(T)[None, :] < lens[:, None], device=dev)
    torch.manual_seed(seed)
    h = (torch.randn(B, T, H, device=dev) * 0.5).requires_grad_()
    w = [(torch.randn(H, 4 * D + 2, device=dev) * np.sqrt(2.0 / (H + 4 * D + 2))).requires_grad_(),
         (torch.randn(4 * D + 2, device=dev) * 0.1).requires_grad_(), (torch.randn(m, D, device=dev) * 0.1).requires_grad_()]
    return h, w, mask, int(lens.sum())


def op_rows(out, iters, windows, dev, verdicts):
    for T, H, m, D in SHAPES:
        h, w, mask, live = make_inputs(T, H, m, D, dev)
        g = [torch.randn(B, T, D, device=dev), torch.randn(B, m, D, device=dev)]
        fused = lambda: Fn.ntm_memory(h, mask, *w)
        comp = lambda: ntm_memory_graph(h, mask, *w)
        with torch.no_grad():
            d = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused(), comp()))

        def fwd(fn):
            with torch.no_grad():
                fn()

        def step(fn):
            h.grad = None
            for p in w:
                p.grad = None
            torch.autograd.backward(list(fn()), g)
        label = "T = %d, H = D = %d, m = %d" % (T, H, m)
        out.append("a/b. the op, %s, %d live steps of %d (fused vs composed outputs: max difference %.1e of the largest value):"
                   % (label, live, B * T, d))
        rows = compare([("a. fused forward", lambda: fwd(fused)), ("b. composed forward", lambda: fwd(comp)),
                        ("a. fused forward + backward", lambda: step(fused)), ("b. composed forward + backward", lambda: step(comp))],
                       iters, windows)
        report(out, rows)
        t = {name: (med, lo, hi) for name, med, lo, hi in rows}
        S = m * D + 4 * D + (6 + 5 * m + 3) // 4 * 4                  # floats of `saved` per live step
        # forward: h in, rs and M_T out (no_grad: nothing is saved); with the backward: h in twice, rs out, saved out and in (live
        # steps), g_rs in, dh out, M_T and g_M once each
        nbytes = {"forward": 4 * (B * T * (H + D) + B * m * D), "forward + backward": 4 * (B * T * (3 * H + 2 * D) + 2 * live * S + 2 * B * m * D)}
        ok = True
        for what in ("forward", "forward + backward"):
            fa, co = t["a. fused " + what], t["b. composed " + what]
            good = fa[2] < co[1]
            ok = ok and good
            out.append("  %-19s composed / fused = %.1fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
                       % (what + ":", co[0] / fa[0], fa[2], co[1], "below" if good else "NOT below"))
            out.append("  %-19s byte floor %.2f MB = %.4f ms at 8 TB/s: %.1f %% of it;  %.2f us per step of the recurrence"
                       % ("", nbytes[what] / 1e6, nbytes[what] / HBM_PEAK * 1e3, 100.0 * nbytes[what] / HBM_PEAK / (fa[0] * 1e-3),
                          fa[0] * 1e3 / T))
        verdicts.append((label, ok, t["b. composed forward + backward"][0] / t["a. fused forward + backward"][0]))
        torch.cuda.empty_cache()


def model_rows(out, iters, windows, dev, verdicts):
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
        model = models.CTRModel(fi, models.MIMN()).to(dev)
        model(None, idx, hist)
        if variant != "fused":
            model.body.behaviors[0].memory.fits_kernel_menu = lambda h: False
        opt = optim.Adam(model.parameters())

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            p = model(None, idx, hist)[:, 0]
            losses.binary_crossentropy(p, y, eps=1e-6).backward()
            opt.step()
        steps.append(("MIMN step: " + variant, step))
        keep.append((model, opt))
    out.append("c. captured models.MIMN training step (optim.Adam, %d one-id fields of %d rows, one history of %d, K = %d, m = 4):" % (F, V, T, K))
    rows = compare(steps, iters, windows)
    report(out, rows)
    good = rows[0][3] < rows[1][2]
    out.append("  composed / fused = %.2fx (medians); slowest fused window %.4f ms, fastest composed window %.4f ms: %s"
               % (rows[1][1] / rows[0][1], rows[0][3], rows[1][2], "below" if good else "NOT below"))
    verdicts.append(("MIMN step", good, rows[1][1] / rows[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parts", default="ab,c")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = ["ntm_bench: %s" % torch.cuda.get_device_name(0), "B=%d, lengths uniform in 1..T" % B]
    for T, H, m, D in SHAPES:
        plan = Fn.ntm_plan(B, T, H, m, D)
        out.append("fil_ntm_plan T = %d, H = D = %d, m = %d: %d samples per workgroup, grid %d of at most %d, %d parameter-gradient partials, LDS %d / %d bytes fwd / bwd"
                   % (T, H, m, plan["tile"], plan["grid"], plan["cap"], plan["partials"], plan["lds_fwd"], plan["lds_bwd"]))
    out.append("HIP-graph replays, %d windows of %d replays, variants alternating; median window (min .. max)" % (args.windows, args.iters))
    verdicts = []
    for part, fn in (("ab", op_rows), ("c", model_rows)):
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
