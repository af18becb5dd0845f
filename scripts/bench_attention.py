#!/usr/bin/env python
"""The softmax-attention core of TransformerMIL, from the packed to_qkv output to the merged heads
and back: (a) ``ops.attention`` (the HIP kernels of csrc/attention.hip) against (b) the path the
model ran before them (reshape, transpose, cast, torch's scaled_dot_product_attention, cast back,
transpose, reshape), H = 8 heads of 64, at (b, n) = (1, 1025), (1, 8193), (8, 1001) in both
compute dtypes.

One process; per point a warm-up, then ``--iters`` timed iterations in which the two paths
alternate; each iteration is forward then backward between device events, so one pass gives the
forward and the forward+backward time.  Reported per path: the median (and minimum) milliseconds,
TF/s from 4 b H n^2 64 forward FLOPs (x 3.5 with the backward: five n x n x 64 products after the
forward's two) over the median, and that rate's share of the dtype's dense matrix peak (bf16
2500 TF/s, fp32 157.3 TF/s); per point the ratio a / b.  A whole-call rate (casts and copies of
path (b) included), not a kernel's share of peak.  Needs a GPU (there is no fallback).  Writes
profiles/attention_bench.json and prints the same JSON line.

    python scripts/bench_attention.py [--iters 200] [--warmup 10] [--out profiles/attention_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, DH = 8, 64
POINTS = [(1, 1025), (1, 8193), (8, 1001)]
PEAK_TF = {"fp32": 157.3, "bf16": 2500.0}


def sdpa_path(qkv, heads, scale, dt):
    """TransformerMIL.Attention.forward's core before the HIP kernels."""
    import torch.nn.functional as F
    b, n, _ = qkv.shape
    q, k, v = (t.reshape(b, n, heads, -1).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(q.to(dt), k.to(dt), v.to(dt), scale=scale).float()
    return o.transpose(1, 2).reshape(b, n, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each path per point (>= 200)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention: needs a GPU")
    from transmil_deepgraft_amd import ops

    dev = "cuda:0"
    scale = DH ** -0.5
    paths = {"hip": lambda x, dt: ops.attention(x, HEADS, scale, dt),
             "sdpa": lambda x, dt: sdpa_path(x, HEADS, scale, dt)}
    results = []
    for b, n in POINTS:
        g = torch.Generator().manual_seed(1000 * b + n)
        qkv = torch.randn(b, n, 3 * HEADS * DH, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(b, n, HEADS * DH, generator=g).to(dev)
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            def once(fn):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                out = fn(qkv, dt)
                e1.record()
                out.backward(dout)
                e2.record()
                qkv.grad = None
                return e0, e1, e2
            for _ in range(args.warmup):
                for fn in paths.values():
                    once(fn)
            torch.cuda.synchronize()
            evs = {p: [] for p in paths}
            for _ in range(args.iters):
                for p, fn in paths.items():
                    evs[p].append(once(fn))
            torch.cuda.synchronize()
            flops_f = 4.0 * b * HEADS * n * n * DH
            row = {"b": b, "n": n, "heads": HEADS, "dtype": name, "iters": args.iters}
            for p, lst in evs.items():
                fwd = [e0.elapsed_time(e1) for e0, e1, _ in lst]
                fb = [e0.elapsed_time(e2) for e0, _, e2 in lst]
                mf, mfb = statistics.median(fwd), statistics.median(fb)
                tf_f, tf_fb = flops_f / (mf * 1e-3) / 1e12, 3.5 * flops_f / (mfb * 1e-3) / 1e12
                row[p] = {"fwd_ms": round(mf, 4), "fwd_min_ms": round(min(fwd), 4),
                          "fwd_bwd_ms": round(mfb, 4), "fwd_bwd_min_ms": round(min(fb), 4),
                          "fwd_tflops": round(tf_f, 2), "fwd_bwd_tflops": round(tf_fb, 2),
                          "fwd_peak_share": round(tf_f / PEAK_TF[name], 4),
                          "fwd_bwd_peak_share": round(tf_fb / PEAK_TF[name], 4)}
            row["ratio_fwd"] = round(row["hip"]["fwd_ms"] / row["sdpa"]["fwd_ms"], 4)
            row["ratio_fwd_bwd"] = round(row["hip"]["fwd_bwd_ms"] / row["sdpa"]["fwd_bwd_ms"], 4)
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    doc = {"bench": "attention_core", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "peak_tflops": PEAK_TF, "flops": "forward 4 b H n^2 64; forward+backward x 3.5",
           "timing": "device events, median over iters, paths alternating in one process", "points": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
