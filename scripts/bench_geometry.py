"""Train-step time of a TransMIL width other than 512 (the fp32 tm_nysg_* attention core), against
the same step with the oracle's torch-op NystromAttention substituted and against the 512-wide
model at the same B and N; plus the per-kernel times of the new core (engine.probe: HIP events
around the named call sites, summed over both layers).

    python scripts/bench_geometry.py --batch 100 --n 1024 --out 384 --classes 3 --feat 2048 \
        --json profiles/geometry_b100_n1024_d384.json

Default shape: DeepGraft/TransMIL_feat_norm_rej_rest.yaml (batch 100, bag_size 1024, RetCCL 2048
features, out_features 384, 3 classes), bf16 compute mode, train mode (dropout on), step = forward +
CrossEntropy + backward, eager (no graph capture at these widths).  Recorded, not gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transmil_deepgraft_amd import engine as E  # noqa: E402
from transmil_deepgraft_amd.models import TransMIL  # noqa: E402

CORE_SITES = ("landmarks", "a3_fwd", "pinv_fwd", "a1_fwd", "conv_bwd", "a1_bwd", "a3_bwd", "pinv_bwd")


class _TorchAttn(torch.nn.Module):
    """The oracle's torch-op NystromAttention behind our module's call form (the unused n x n
    return_attn product is not computed: it reaches neither the logits nor a gradient)."""

    def __init__(self, ref):
        super().__init__()
        self.ref = ref

    def forward(self, x, mask=None, return_attn=False):
        out = self.ref(x)
        return (out, None) if return_attn else out


def build(ncls, feat, out, dtype, torch_attn=False):
    torch.manual_seed(0)
    m = TransMIL(ncls, feat, out).to("cuda").train().set_compute_dtype(dtype)
    if torch_attn:
        from oracle.nystrom_ref import NystromAttention as Ref
        for layer in (m.layer1, m.layer2):
            ref = Ref(dim=out, dim_head=out // 8, heads=8, num_landmarks=out // 2, pinv_iterations=6, residual=True,
                      dropout=0.7).to("cuda").train()
            ref.load_state_dict(layer.attn.state_dict())
            layer.attn = _TorchAttn(ref)
    return m


def step(m, x, target):
    m.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(m(x), target)
    loss.backward()
    return loss


def timed(m, x, target, steps, warmup):
    for _ in range(warmup):
        step(m, x, target)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        step(m, x, target)
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "steps": steps}


def core_sites(m, x, target, steps):
    """Per call site, the median over `steps` of the site's HIP-event time summed over the layers."""
    E.probe.target = set(CORE_SITES)
    per_step = []
    try:
        for _ in range(steps):
            E.probe.events, E.probe.names = [], []
            step(m, x, target)
            torch.cuda.synchronize()
            tot = {}
            for name, ev in zip(E.probe.names, E.probe.events):
                tot[name] = tot.get(name, 0.0) + ev[0].elapsed_time(ev[1])
            per_step.append(tot)
    finally:
        E.probe.target = None
        E.probe.events, E.probe.names = [], []
    return {k: sorted(t[k] for t in per_step)[len(per_step) // 2] for k in per_step[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--feat", type=int, default=2048)
    ap.add_argument("--out", type=int, default=384)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(a.batch, a.n, a.feat, generator=g).to("cuda")
    target = torch.nn.functional.one_hot(torch.arange(a.batch) % a.classes, a.classes).float().to("cuda")
    res = {"shape": {"B": a.batch, "N": a.n, "feat": a.feat, "out": a.out, "classes": a.classes}, "dtype": a.dtype,
           "device": torch.cuda.get_device_name(0), "commit": a.commit, "command": " ".join(sys.argv)}
    m = build(a.classes, a.feat, a.out, dtype)
    res["hip_step"] = timed(m, x, target, a.steps, a.warmup)
    res["hip_core_sites_ms"] = core_sites(m, x, target, max(3, a.steps // 2))
    res["hip_core_total_ms"] = sum(res["hip_core_sites_ms"].values())
    del m
    m = build(a.classes, a.feat, a.out, dtype, torch_attn=True)
    res["torch_attention_step"] = timed(m, x, target, a.steps, a.warmup)
    del m
    m = build(a.classes, a.feat, 512, dtype)
    res["wide512_step"] = timed(m, x, target, a.steps, a.warmup)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
