#!/usr/bin/env python
"""AttMIL, from the bag to the logits and back: (a) ``models.AttMIL`` in its fp32 compute mode (f32
MFMA GEMMs, ``tm_attmil_fwd`` / ``_bwd``), (b) the same model in its bf16 compute mode (bf16 MFMA
GEMMs with fp32 accumulation, ``H`` / ``Z`` in bf16, the typed pooling ``tm_attmil_pool_fwd`` /
``_bwd``) and (c) the reference's op sequence in eager fp32 torch on the same GPU (``_fc1``, the two
gate Linears, ``softmax`` over the instances, ``mm``, the classifier; code/models/AttMIL.py:88-110),
at N = 1000, 8192 and 32768 instances x in_features 1024 and 2048, out_features 512, two classes,
eval mode.

One process; per point a warm-up, then ``--iters`` timed iterations in which the three paths
alternate; each iteration is forward then backward (parameter gradients; the bag needs none) of
``logits.sum()`` between device events, so one pass gives the forward and the forward+backward time.
Reported per path: the median (and minimum) milliseconds; per point the ratios b / a and b / c and the
pooling row pass's algorithmic bytes N (2D + L) sizeof(T) + 4 N for both storage types.  A share of the
HBM roof is not derived from these whole-call times (they include the GEMMs and host launch time): it
is stated only from a kernel-trace run of its own, so the field reads "not measured".
Needs a GPU (there is no fallback).  Writes profiles/attmil_bench.json and prints the same JSON line.

    python scripts/bench_attmil.py [--iters 200] [--warmup 10] [--out profiles/attmil_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [(n, f) for f in (1024, 2048) for n in (1000, 8192, 32768)]
CLASSES, L, D = 2, 512, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each path per point (>= 200)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attmil_bench.json"))
    args = ap.parse_args()

    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_attmil: needs a GPU")
    from transmil_deepgraft_amd.models import AttMIL

    class EagerAttMIL(nn.Module):
        """The reference's forward as eager torch ops (same parameter names)."""

        def __init__(self, in_features):
            super().__init__()
            if in_features == 2048:
                self._fc1 = nn.Sequential(nn.Linear(2048, 1024), nn.GELU(), nn.Dropout(0.6), nn.LayerNorm(1024),
                                          nn.Linear(1024, L), nn.GELU())
            else:
                self._fc1 = nn.Sequential(nn.Linear(1024, L), nn.GELU(), nn.Dropout(0.6), nn.LayerNorm(L))
            self.feature_extractor_part2 = nn.Sequential(nn.Linear(in_features, L), nn.ReLU())
            self.attention_V = nn.Sequential(nn.Linear(L, D), nn.Tanh())
            self.attention_U = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
            self.attention_weights = nn.Linear(D, 1)
            self.classifier = nn.Sequential(nn.Linear(L, CLASSES))

        def forward(self, x):
            h = self._fc1(x.squeeze())
            a = self.attention_weights(self.attention_V(h) * self.attention_U(h))
            a = F.softmax(torch.transpose(a, 1, 0), dim=1)
            return self.classifier(torch.mm(a, h))

    dev = "cuda:0"
    results = []
    for N, feat in POINTS:
        torch.manual_seed(0)
        fp32 = AttMIL(CLASSES, feat, L).to(dev).eval()
        bf16 = AttMIL(CLASSES, feat, L).to(dev).eval().set_compute_dtype(torch.bfloat16)
        eager = EagerAttMIL(feat).to(dev).eval()
        bf16.load_state_dict(fp32.state_dict(), strict=True)
        eager.load_state_dict(fp32.state_dict(), strict=True)
        paths = {"fp32": fp32, "bf16": bf16, "eager": eager}
        x = torch.rand(1, N, feat, generator=torch.Generator().manual_seed(N)).to(dev)

        def once(model):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            loss = model(x).sum()
            e1.record()
            loss.backward()
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
        row = {"N": N, "in_features": feat, "out_features": L, "classes": CLASSES, "iters": args.iters,
               "row_pass_bytes": {"fp32": N * (2 * D + L) * 4 + 4 * N, "bf16": N * (2 * D + L) * 2 + 4 * N},
               "row_pass_hbm_roof_share": "not measured"}
        for p, lst in evs.items():
            fwd = [e0.elapsed_time(e1) for e0, e1, _ in lst]
            fb = [e0.elapsed_time(e2) for e0, _, e2 in lst]
            row[p] = {"fwd_ms": round(statistics.median(fwd), 4), "fwd_min_ms": round(min(fwd), 4),
                      "fwd_bwd_ms": round(statistics.median(fb), 4), "fwd_bwd_min_ms": round(min(fb), 4)}
        for num, den in (("bf16", "fp32"), ("bf16", "eager")):
            row[f"ratio_fwd_{num}_over_{den}"] = round(row[num]["fwd_ms"] / row[den]["fwd_ms"], 4)
            row[f"ratio_fwd_bwd_{num}_over_{den}"] = round(row[num]["fwd_bwd_ms"] / row[den]["fwd_bwd_ms"], 4)
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    accept = {f"N{r['N']}_in2048": r["bf16"]["fwd_bwd_ms"] <= r["fp32"]["fwd_bwd_ms"]
              for r in results if r["in_features"] == 2048 and r["N"] in (8192, 32768)}
    doc = {"bench": "attmil", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "row_pass_bytes": "N (2D + L) sizeof(T) + 4 N: one read of Z and H, one write of the scores",
           "timing": "device events, median over iters, paths alternating in one process; whole calls "
                     "(the GEMMs and host launch time included)",
           "acceptance": {"rule": "bf16 fwd+bwd median <= fp32 fwd+bwd median at N = 8192 and 32768, in_features 2048",
                          "met": accept},
           "points": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
