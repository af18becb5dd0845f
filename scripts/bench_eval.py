#!/usr/bin/env python
"""One validation epoch, eager against graph-replayed (TransMILTask.validation_step /
GraphedEvaluation): 64 synthetic bags, N drawn uniformly from 50..1500, F = 512, bf16 mode, B = 1.

Reports the median over epochs of the milliseconds per slide (host clock around the epoch's steps,
ending in a device synchronise; the epoch end's reductions and its one copy are timed on their
own).  Eager and replayed epochs alternate in one process so both see the same machine state.
Needs a GPU (there is no fallback).  Writes profiles/eval_epoch.json and prints the same JSON line.

    python scripts/bench_eval.py [--epochs 10] [--out profiles/eval_epoch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10, help="timed epochs of each kind")
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_epoch.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: needs a GPU")
    from transmil_deepgraft_amd.interface import GraphedEvaluation, TransMILTask
    from transmil_deepgraft_amd.models import TransMIL

    dev = "cuda:0"
    torch.manual_seed(1234)
    model = TransMIL(2, 512).to(dev).eval().set_compute_dtype(torch.bfloat16)
    rng = np.random.default_rng(2021)
    sizes = [int(n) for n in rng.integers(50, 1501, args.slides)]
    g = torch.Generator().manual_seed(2021)
    bags = [torch.rand(1, n, 512, generator=g).to(dev) for n in sizes]
    labels = [torch.tensor([(i // 2) % 2], device=dev) for i in range(args.slides)]
    meta = [(f"slide{i}", None, f"patient{i // 2}") for i in range(args.slides)]

    eager, graphed = TransMILTask(model), TransMILTask(model)
    ge = GraphedEvaluation(graphed, "val", capacity=max(args.slides, 1), max_graphs=len(set(sizes)))

    def epoch(task, step):
        task.on_validation_epoch_start()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.slides):
            step((bags[i], labels[i], meta[i]), i)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = task.on_validation_epoch_end()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3 / args.slides, (t2 - t1) * 1e3, out

    # warm-up: every shape eager (both tasks), then every shape captured and replayed once
    ref = epoch(eager, eager.validation_step)[2]
    epoch(graphed, ge)
    epoch(graphed, ge)
    assert ge.live_graphs() == len(set(sizes))
    ms = {"eager": [], "replayed": []}
    end_ms = []
    for _ in range(args.epochs):
        a, e1, out_e = epoch(eager, eager.validation_step)
        b, e2, out_g = epoch(graphed, ge)
        ms["eager"].append(a)
        ms["replayed"].append(b)
        end_ms += [e1, e2]
        for k, v in ref.items():        # replayed epochs compute what eager ones do
            if isinstance(v, float):
                assert out_e[k] == v and out_g[k] == v, (k, v, out_e[k], out_g[k])
    ge.close()

    res = {"metric": "validation_ms_per_slide", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "slides": args.slides, "n_min": min(sizes), "n_max": max(sizes), "n_mean": sum(sizes) / len(sizes),
           "epochs": args.epochs, "graphs": len(set(sizes)),
           "eager_ms_per_slide": statistics.median(ms["eager"]),
           "replayed_ms_per_slide": statistics.median(ms["replayed"]),
           "eager_ms_per_slide_min_max": [min(ms["eager"]), max(ms["eager"])],
           "replayed_ms_per_slide_min_max": [min(ms["replayed"]), max(ms["replayed"])],
           "epoch_end_ms": statistics.median(end_ms), "val_loss": ref["val_loss"]}
    res["speedup"] = res["eager_ms_per_slide"] / res["replayed_ms_per_slide"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
