#!/usr/bin/env python
"""Chowder, from the bag to the logits and back: (a) ``models.Chowder`` (the fused score + top-R +
head kernels of csrc/chowder.hip) against (b) the reference's op sequence in eager torch on the same
GPU (``x.float()``, transpose, ``Conv1d(L, 1, 1)``, two ``topk``, ``cat``, three ``Linear``,
code/models/Chowder.py:37-50), at (B, N, L) = (1, 1000, 512), (1, 8192, 512), (1, 32768, 512) and
(4, 8192, 2048) on an fp32 and on a bf16 bag, r = 5, two classes.

One process; per point a warm-up, then ``--iters`` timed iterations in which the two paths
alternate; each iteration is forward then backward (parameter gradients; the bag needs none)
between device events, so one pass gives the forward and the forward+backward time.  Reported per
path: the median (and minimum) milliseconds; per point the ratio a / b and, for path (a), the
forward's share of the HBM roof: B N L elemsize bytes over the median against the 8 TB/s peak.
Needs a GPU (there is no fallback).  Writes profiles/chowder_bench.json and prints the same JSON line.

    python scripts/bench_chowder.py [--iters 200] [--warmup 10] [--out profiles/chowder_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [(1, 1000, 512), (1, 8192, 512), (1, 32768, 512), (4, 8192, 2048)]
R, CLASSES = 5, 2
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each path per point (>= 200)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chowder_bench.json"))
    args = ap.parse_args()

    import torch
    import torch.nn as nn
    if not torch.cuda.is_available():
        raise SystemExit("bench_chowder: needs a GPU")
    from transmil_deepgraft_amd.models import Chowder

    class EagerChowder(nn.Module):
        """The reference's module, op for op."""

        def __init__(self, n_classes, features, r):
            super().__init__()
            self.R = r
            self.f1 = nn.Sequential(nn.Conv1d(features, 1, 1))
            self.f2 = nn.Sequential(nn.Linear(r * 2, 200), nn.Linear(200, 100), nn.Linear(100, n_classes))

        def forward(self, x):
            x = x.float()
            x = torch.transpose(x, 1, 2)
            x = self.f1(x)
            max_indices = torch.topk(x, self.R).values
            min_indices = torch.topk(x, self.R, largest=False).values
            cat_minmax = torch.cat((min_indices, max_indices), dim=2)
            return self.f2(cat_minmax).squeeze(0), None

    dev = "cuda:0"
    results = []
    for B, N, L in POINTS:
        torch.manual_seed(0)
        hip = Chowder(CLASSES, L, R).to(dev)
        eager = EagerChowder(CLASSES, L, R).to(dev)
        eager.load_state_dict(hip.state_dict(), strict=True)
        paths = {"hip": hip, "eager": eager}
        g = torch.Generator().manual_seed(1000 * B + N)
        x32 = torch.rand(B, N, L, generator=g).to(dev)
        for name, x in (("fp32", x32), ("bf16", x32.to(torch.bfloat16))):
            dout = torch.ones_like(hip(x)[0])

            def once(model):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                out = model(x)[0]
                e1.record()
                out.backward(dout)
                e2.record()
                model.zero_grad(set_to_none=True)
                return e0, e1, e2
            for _ in range(args.warmup):
                for m in paths.values():
                    once(m)
            torch.cuda.synchronize()
            evs = {p: [] for p in paths}
            for _ in range(args.iters):
                for p, m in paths.items():
                    evs[p].append(once(m))
            torch.cuda.synchronize()
            nbytes = B * N * L * x.element_size()
            row = {"B": B, "N": N, "L": L, "r": R, "dtype": name, "iters": args.iters, "bag_bytes": nbytes}
            for p, lst in evs.items():
                fwd = [e0.elapsed_time(e1) for e0, e1, _ in lst]
                fb = [e0.elapsed_time(e2) for e0, _, e2 in lst]
                row[p] = {"fwd_ms": round(statistics.median(fwd), 4), "fwd_min_ms": round(min(fwd), 4),
                          "fwd_bwd_ms": round(statistics.median(fb), 4), "fwd_bwd_min_ms": round(min(fb), 4)}
            row["hip"]["fwd_hbm_roof_share"] = round(nbytes / (row["hip"]["fwd_ms"] * 1e-3) / HBM_PEAK, 4)
            row["ratio_fwd"] = round(row["hip"]["fwd_ms"] / row["eager"]["fwd_ms"], 4)
            row["ratio_fwd_bwd"] = round(row["hip"]["fwd_bwd_ms"] / row["eager"]["fwd_bwd_ms"], 4)
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    doc = {"bench": "chowder", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hbm_peak_bytes_per_s": HBM_PEAK, "roof": "B N L elemsize bytes / median forward time / peak",
           "timing": "device events, median over iters, paths alternating in one process; whole calls "
                     "(host launch time included)", "points": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
