"""The c4 step (xDeepFM CIN fwd+bwd, B=4096, F=39, K=16, 3x128, bench.py's seeded inputs) in its three operand precisions, in ONE
process on one device: exact fp32 (mode 0, the headline), split bf16 (mode 2, FIL_CIN_BF16X3) and bf16 (fil_cin_fwd_p / fil_cin_bwd_p
with FIL_CIN_PREC_BF16).  bench.py's protocol: W warm-up steps in front of every window of K steps, a device synchronisation as the
fence, --windows windows per precision (taken round-robin, so that clock drift hits all three alike), then the step replayed from a
HIP graph.  Prints one JSON line; then (unless --no-error-table) the bf16 rows of tests/cin_error_table.py's table against the fp64
oracle graph.  The exact chain stays the headline: the other two are labelled modes.

    python tools/cin_precision_bench.py --steps 20 --warmup 5     (needs a GPU)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (make_inputs, timed_steps: the headline's inputs and timing)
from ml_function_amd import functional as Fn  # noqa: E402

VARIANTS = (("f32", 0, "f32"), ("bf16x3", Fn.CIN_BF16X3, "f32"), ("bf16", 0, "bf16"))


def error_table(B):
    """norm-relative / max-relative error of every output and gradient against the fp64 oracle graph (tests/cin_error_table.py's
    columns), for bf16 beside the exact chain, uniform (x10) and normal inputs."""
    from ml_function_amd import synth
    from oracle import graph

    def rel(a, b):
        a = a.detach().double().cpu().numpy().ravel()
        b = b.detach().double().cpu().numpy().ravel()
        return float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max())

    lines = ["CIN error table at B=%d, F=39, K=16, 3x128: norm-relative / max-relative error against the fp64 oracle graph" % B]
    for dist in ("uniform", "normal"):
        c = synth.cin_case(B, 39, 16, [128, 128, 128], dist=dist)
        if dist == "uniform":
            c["x"] = (c["x"] * 10).astype(np.float32)
        T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
        Ws, bs = [T(w).requires_grad_() for w in c["Ws"]], [T(b).requires_grad_() for b in c["bs"]]
        dw, db = T(c["dense_w"]).requires_grad_(), T(c["dense_b"]).requires_grad_()
        outs, dxs = [], []
        for lo in range(0, B, 512):
            x = T(c["x"][lo:lo + 512]).requires_grad_()
            out = graph.cin(x, Ws, bs, dw, db, output_dim=1)
            out.backward(T(c["g"][lo:lo + 512]))
            outs.append(out.detach())
            dxs.append(x.grad)
        want, wdx = torch.cat(outs), torch.cat(dxs)
        for prec, name in (("f32", "exact fp32 (mode 0)"), ("bf16", "bf16 (PREC_BF16)")):
            dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
            x = dev(c["x"]).requires_grad_()
            W2 = [dev(w).requires_grad_() for w in c["Ws"]]
            b2 = [dev(b).requires_grad_() for b in c["bs"]]
            dw2, db2 = dev(c["dense_w"]).requires_grad_(), dev(c["dense_b"]).requires_grad_()
            out = Fn.cin(x, W2, b2, dw2, db2, output_dim=1, precision=prec)
            out.backward(dev(c["g"]))
            lines.append("%-8s %-22s out %.2e/%.2e  dx %.2e/%.2e  " % ((dist, name) + rel(out, want) + rel(x.grad, wdx)) +
                         "  ".join("dW%d %.2e/%.2e" % ((l + 1,) + rel(W2[l].grad, Ws[l].grad)) for l in range(3)) + "  " +
                         "  ".join("db%d %.2e/%.2e" % ((l + 1,) + rel(b2[l].grad, bs[l].grad)) for l in range(3)) +
                         "  ddense_w %.2e/%.2e" % rel(dw2.grad, dw.grad))
        del Ws, bs, dw, db, outs, dxs
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-error-table", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cin_precision_bench.py needs a GPU"
    device = torch.device("cuda", 0)
    inp = bench.make_inputs(0, device)
    B, F, K = inp["x"].shape
    H = [int(w.shape[1]) for w in inp["Ws"]]
    used = {name: Fn.cin_precision_used(B, F, K, H, mode=mode, precision=prec) for name, mode, prec in VARIANTS}
    if used["bf16"] != "bf16":
        raise SystemExit("cin_precision_bench.py: the bf16 kernels do not run at this shape (%s)" % used)

    def compute(mode, prec):
        out, pooled, saved = Fn.cin_forward_raw(inp["x"], inp["Ws"], inp["bs"], inp["dense_w"], inp["dense_b"], 1, mode, precision=prec)
        Fn.cin_backward_raw(inp["x"], inp["Ws"], inp["bs"], inp["dense_w"], pooled, saved, inp["g"], 1, mode, precision=prec)
        return out

    fence = torch.cuda.synchronize
    windows = {name: [] for name, _, _ in VARIANTS}
    for _ in range(max(1, args.windows)):
        for name, mode, prec in VARIANTS:
            for _ in range(args.warmup):
                compute(mode, prec)
            windows[name].append(bench.timed_steps(lambda: compute(mode, prec), fence, args.steps) / args.steps * 1e3)

    def replay_ms(mode, prec):   # bench.py's replay_ms
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                compute(mode, prec)
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            compute(mode, prec)
        for _ in range(max(2, args.warmup)):
            gr.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            gr.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) / args.steps * 1e3

    res = {"metric": "ms/step fwd+bwd xDeepFM-CIN B=%d,F=%d,K=%d,%s by operand precision (f32 = the exact headline chain; bf16x3, bf16: "
                     "labelled modes)" % (B, F, K, "x".join(map(str, H))),
           "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, mode, prec in VARIANTS:
        w = windows[name]
        res[name] = {"mode": mode, "precision": prec, "precision_used": used[name], "ms_per_step_windows": [round(v, 4) for v in w],
                     "ms_per_step_median": round(sorted(w)[len(w) // 2], 4), "ms_per_step_min": round(min(w), 4),
                     "samples_per_s_median": round(B / (sorted(w)[len(w) // 2] * 1e-3)),
                     "hipgraph_replay_ms_per_step": round(replay_ms(mode, prec), 4)}
    med = lambda n: res[n]["ms_per_step_median"]
    res["speedup_bf16_over_f32"] = round(med("f32") / med("bf16"), 3)
    res["speedup_bf16_over_bf16x3"] = round(med("bf16x3") / med("bf16"), 3)
    print(json.dumps(res), flush=True)
    if not args.no_error_table:
        for line in error_table(B):
            print(line, flush=True)


if __name__ == "__main__":
    main()
