#!/usr/bin/env python
"""DTFD-MIL, from the bag to ``total = (sub_loss + slide_loss) / 2`` and back: (a) ``dtfd.DTFDMIL`` (the
row gather, the HIP GEMMs and the fused double-tier pooling kernels of csrc/dtfd.hip) against (b) the
reference's op sequence in eager fp32 torch on the same GPU (``DimReduction`` over all N rows, then per
pseudo-bag the index by the permutation's slice, the gated attention, ``softmax``, the ``einsum``
weighting, the sum, ``Classifier_1fc`` and ``get_cam_1d``; ``Attention_with_Classifier``; ``argmax`` and
``softmax``; the two cross entropies on the one-hot label; code/models/model_interface_dtfd.py:174-241,
268).  Both paths draw ``torch.randperm(N)`` on the host inside the timed forward, as the reference does.

Point 1 is the reference's largest case (N = 960, bag_size = 120, G = 8, two classes); point 2 is
N = 8192, bag_size = 128, max_pseudo_bags = 64.

One process; per point a warm-up, then ``--iters`` timed iterations in which the two paths alternate;
each iteration is forward then backward (all parameter gradients; the bag needs none) of ``total``
between device events, so one pass gives the forward and the forward+backward time.  Reported per path:
the median (and minimum) milliseconds; per point the ratio a / b.  Kernel times and a share of the HBM
roof are not derived from these whole-call times (they include the GEMMs and host launch time): the
fields read "not measured".
Needs a GPU (there is no fallback).  Writes profiles/dtfd_bench.json and prints the same JSON line.

    python scripts/bench_dtfd.py [--iters 200] [--warmup 10] [--out profiles/dtfd_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, bag_size, max_pseudo_bags)
POINTS = [(960, 120, 8), (8192, 128, 64)]
CLASSES, L, D = 2, 512, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each path per point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtfd_bench.json"))
    args = ap.parse_args()

    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_dtfd: needs a GPU")
    from transmil_deepgraft_amd.dtfd import DTFDMIL

    class Gated(nn.Module):
        def __init__(self):
            super().__init__()
            self.attention_V = nn.Sequential(nn.Linear(L, D), nn.Tanh())
            self.attention_U = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
            self.attention_weights = nn.Linear(D, 1)

        def forward(self, x):
            A = self.attention_weights(self.attention_V(x) * self.attention_U(x))
            return F.softmax(torch.transpose(A, 1, 0), dim=1)

    class Classifier(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(L, CLASSES)

        def forward(self, x):
            return self.fc(x)

    class DimReduction(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = nn.Linear(1024, L, bias=False)
            self.relu1 = nn.ReLU(inplace=True)

        def forward(self, x):
            return self.relu1(self.fc1(x))

    class AttCls(nn.Module):
        def __init__(self):
            super().__init__()
            self.attention = Gated()
            self.classifier = Classifier()

        def forward(self, x):
            return self.classifier(torch.mm(self.attention(x), x))

    class EagerDTFD(nn.Module):
        """The reference's forward and losses as eager torch ops (same parameter names)."""

        def __init__(self, bag_size, cap):
            super().__init__()
            self.classifier = Classifier()
            self.attention = Gated()
            self.dimreduction = DimReduction()
            self.attCls = AttCls()
            self.bag_size, self.cap = bag_size, cap

        def forward(self, x, hot):
            x = x.float()
            S = self.bag_size
            G = min(self.cap, x.squeeze(0).shape[0] // S)
            features = self.dimreduction(x.squeeze(0))
            perm = torch.randperm(features.shape[0])
            feats, subs = [], []
            for n in range(G):
                bag = features[perm[S * n:S * (n + 1)]]
                AA = self.attention(bag).squeeze(0)
                att = torch.einsum("ns, n->ns", bag, AA)
                pooled = torch.sum(att, dim=0).unsqueeze(0)
                subs.append(self.classifier(pooled))
                cam = torch.einsum("bgf,cf->bcg", [att.unsqueeze(0), self.classifier.fc.weight]).squeeze(0)
                cam = torch.transpose(cam, 0, 1)
                feats.append(pooled)
            feats, sub = torch.cat(feats, dim=0), torch.cat(subs, dim=0)
            slide = self.attCls(feats)
            Y_hat, Y_prob = torch.argmax(slide, dim=1), F.softmax(slide, dim=1)
            sub_loss = F.cross_entropy(sub, torch.cat([hot] * sub.size(0), dim=0))
            slide_loss = F.cross_entropy(slide, hot)
            return (sub_loss + slide_loss) / 2, Y_prob, Y_hat

    dev = "cuda:0"
    results = []
    for N, S, cap in POINTS:
        torch.manual_seed(0)
        hip = DTFDMIL(CLASSES, bag_size=S, max_pseudo_bags=cap).to(dev)
        eager = EagerDTFD(S, cap).to(dev)
        eager.load_state_dict(hip.state_dict(), strict=True)
        x = torch.rand(1, N, 1024, generator=torch.Generator().manual_seed(N)).to(dev)
        label = torch.tensor([1], device=dev)
        hot = F.one_hot(label, CLASSES).float()

        def run_hip():
            out = hip(x, label=label)
            return (out[4]["sub_loss"] + out[4]["slide_loss"]) / 2

        def run_eager():
            return eager(x, hot)[0]

        paths = {"hip": (hip, run_hip), "eager": (eager, run_eager)}

        def once(model, fn):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            total = fn()
            e1.record()
            total.backward()
            e2.record()
            model.zero_grad(set_to_none=True)
            return e0, e1, e2

        for _ in range(args.warmup):
            for m, fn in paths.values():
                once(m, fn)
        torch.cuda.synchronize()
        evs = {p: [] for p in paths}
        for _ in range(args.iters):
            for p, (m, fn) in paths.items():
                evs[p].append(once(m, fn))
        torch.cuda.synchronize()
        G = min(cap, N // S)
        row = {"N": N, "bag_size": S, "pseudo_bags": G, "classes": CLASSES, "iters": args.iters,
               "tier1_bytes": 4 * G * S * (2 * D + L), "kernel_ms": "not measured", "hbm_roof_share": "not measured"}
        for p, lst in evs.items():
            fwd = [e0.elapsed_time(e1) for e0, e1, _ in lst]
            fb = [e0.elapsed_time(e2) for e0, _, e2 in lst]
            row[p] = {"fwd_ms": round(statistics.median(fwd), 4), "fwd_min_ms": round(min(fwd), 4),
                      "fwd_bwd_ms": round(statistics.median(fb), 4), "fwd_bwd_min_ms": round(min(fb), 4)}
        row["ratio_fwd"] = round(row["hip"]["fwd_ms"] / row["eager"]["fwd_ms"], 4)
        row["ratio_fwd_bwd"] = round(row["hip"]["fwd_bwd_ms"] / row["eager"]["fwd_bwd_ms"], 4)
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    doc = {"bench": "dtfd", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "tier1_bytes": "4 G S (2D + L): one read of the selected rows of Z and h",
           "timing": "device events, median over iters, paths alternating in one process; whole calls "
                     "(the host randperm, the gather, the GEMMs and host launch time included)", "points": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
