#!/usr/bin/env python
"""CLAM_MB, from the bag to the logits (and the instance loss) and back: (a) ``models.CLAM_MB`` (the
HIP GEMMs and the fused pooling / selection / instance-loss kernels of csrc/clam.hip) against (b) the
reference's op sequence in eager fp32 torch on the same GPU (``Linear`` + ``ReLU``, the gated
attention branch, ``softmax`` over the instances, per evaluated class ``topk`` / ``index_select`` /
the instance classifier / cross entropy with the label read through ``.item()`` and the predictions
copied to the host, ``mm``, one ``Linear(L, 1)`` per class; code/models/model_clam.py:222-268), at
N = 1000, 8192 and 32768 instances, two classes, size "small", k_sample = 8, with and without the
instance evaluation.

One process; per point a warm-up, then ``--iters`` timed iterations in which the two paths
alternate; each iteration is forward then backward (parameter gradients; the bag needs none) of
``logits.sum() + instance_loss`` between device events, so one pass gives the forward and the
forward+backward time.  Reported per path: the median (and minimum) milliseconds; per point the
ratio a / b and the row pass's algorithmic bytes 4 N (2D + L + K).  A share of the HBM roof is not
derived from these whole-call times (they include the GEMMs and host launch time): it is stated only
from a kernel-trace run of its own, so the field reads "not measured".
Needs a GPU (there is no fallback).  Writes profiles/clam_bench.json and prints the same JSON line.

    python scripts/bench_clam.py [--iters 200] [--warmup 10] [--out profiles/clam_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [1000, 8192, 32768]
CLASSES, K_SAMPLE, L, D = 2, 8, 512, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each path per point (>= 200)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clam_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_clam: needs a GPU")
    from transmil_deepgraft_amd.models import CLAM_MB

    class Gated(nn.Module):
        def __init__(self):
            super().__init__()
            self.attention_a = nn.Sequential(nn.Linear(L, D), nn.Tanh())
            self.attention_b = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
            self.attention_c = nn.Linear(D, CLASSES)

        def forward(self, x):
            return self.attention_c(self.attention_a(x).mul(self.attention_b(x))), x

    class EagerClam(nn.Module):
        """The reference's forward as eager torch ops (same parameter names)."""

        def __init__(self):
            super().__init__()
            self.attention_net = nn.Sequential(nn.Linear(1024, L), nn.ReLU(), Gated())
            self.classifiers = nn.ModuleList([nn.Linear(L, 1) for _ in range(CLASSES)])
            self.instance_classifiers = nn.ModuleList([nn.Linear(L, 2) for _ in range(CLASSES)])

        def forward(self, h, label=None, instance_eval=False):
            A, h = self.attention_net(h)
            A_raw = torch.transpose(A, 1, 0)
            A = F.softmax(A_raw, dim=1)
            results = {}
            if instance_eval:
                total, preds_all, targets_all = 0.0, [], []
                hot = F.one_hot(label, num_classes=CLASSES).squeeze()
                for c in range(CLASSES):
                    if hot[c].item() != 1:
                        continue
                    top = torch.index_select(h, 0, torch.topk(A[c], K_SAMPLE)[1])
                    bottom = torch.index_select(h, 0, torch.topk(-A[c], K_SAMPLE)[1])
                    targets = torch.cat([torch.full((K_SAMPLE,), 1, device=h.device).long(),
                                         torch.full((K_SAMPLE,), 0, device=h.device).long()])
                    il = self.instance_classifiers[c](torch.cat([top, bottom]))
                    preds_all.extend(torch.topk(il, 1, dim=1)[1].squeeze(1).cpu().numpy())
                    targets_all.extend(targets.cpu().numpy())
                    total = total + F.cross_entropy(il, targets)
                results = {"instance_loss": total, "inst_labels": np.array(targets_all),
                           "inst_preds": np.array(preds_all)}
            M = torch.mm(A, h)
            logits = torch.empty(1, CLASSES, device=h.device)
            for c in range(CLASSES):
                logits[0, c] = self.classifiers[c](M[c])
            return logits, F.softmax(logits, dim=1), torch.topk(logits, 1, dim=1)[1], A_raw, results

    dev = "cuda:0"
    results = []
    for N in POINTS:
        torch.manual_seed(0)
        hip = CLAM_MB(k_sample=K_SAMPLE, n_classes=CLASSES).to(dev)
        eager = EagerClam().to(dev)
        eager.load_state_dict(hip.state_dict(), strict=True)
        paths = {"hip": hip, "eager": eager}
        x = torch.rand(N, 1024, generator=torch.Generator().manual_seed(N)).to(dev)
        label = torch.tensor([1], device=dev)
        for inst in (False, True):
            def once(model):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                out = model(x, label=label, instance_eval=inst)
                loss = out[0].sum() + out[4]["instance_loss"] if inst else out[0].sum()
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
            row = {"N": N, "classes": CLASSES, "k_sample": K_SAMPLE, "instance_eval": inst, "iters": args.iters,
                   "row_pass_bytes": 4 * N * (2 * D + L + CLASSES), "row_pass_hbm_roof_share": "not measured"}
            for p, lst in evs.items():
                fwd = [e0.elapsed_time(e1) for e0, e1, _ in lst]
                fb = [e0.elapsed_time(e2) for e0, _, e2 in lst]
                row[p] = {"fwd_ms": round(statistics.median(fwd), 4), "fwd_min_ms": round(min(fwd), 4),
                          "fwd_bwd_ms": round(statistics.median(fb), 4), "fwd_bwd_min_ms": round(min(fb), 4)}
            row["ratio_fwd"] = round(row["hip"]["fwd_ms"] / row["eager"]["fwd_ms"], 4)
            row["ratio_fwd_bwd"] = round(row["hip"]["fwd_bwd_ms"] / row["eager"]["fwd_bwd_ms"], 4)
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    doc = {"bench": "clam", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "row_pass_bytes": "4 N (2D + L + K): one read of Z and h, one write of the scores",
           "timing": "device events, median over iters, paths alternating in one process; whole calls "
                     "(the GEMMs and host launch time included)", "points": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
