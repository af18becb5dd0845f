"""Image tile-bag ingest on one MI355X: seeded synthetic uint8 tiles resident in HBM.

(a) ``tm_gather_tiles_u8`` (gather + ToTensor + Normalize + cast, one pass) against the torch-op
    route on the same device in the same process (index_select -> permute -> .float() -> div ->
    sub -> div -> cast), N x 224 x 224 tiles into bf16 and fp32 NCHW: the two alternate, each timing
    is one call between device events, the median of ``--reps`` (>= 20) after warm-up.  Achieved
    bytes/s from the algorithmic byte count (3 B read + 3 x elem B written per pixel) and its share
    of the 8 TB/s spec and of the 6.29 TB/s achievable copy rate.
(b) one ``simple`` + AttMIL(2, 1024) evaluation step on N tiles: from a resident bf16 tensor
    (through ``TransMILTask.validation_step``, which hands the model an fp32 copy, and through the
    model directly on the bf16 tensor) and from a lazy ``TileBag`` over the uint8 store.
(c) a pinned-host -> device copy of one N-tile slide as uint8 and as fp32.

    python scripts/bench_ingest.py [--n 4096] [--reps 25] [--out profiles/image_ingest_bench.json]

Needs a GPU (fails without one).  ONE gate: in (a) the kernel is not slower than the torch-op route
in either dtype (exit status 1 otherwise); everything else is recorded.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 224
HBM_SPEC_BPS = 8.0e12
HBM_COPY_BPS = 6.29e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=3):
    """name -> list of per-call ms, the routes alternating call by call."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return ts


def torch_route(slab, idx, mean, std, dtype):
    x = slab.index_select(0, idx).permute(0, 3, 1, 2).float()
    return x.div_(255).sub_(mean).div_(std).to(dtype).contiguous()


def bench_kernel(store, lut, n, reps):
    from transmil_deepgraft_amd.data import TILE_MEAN, TILE_STD, gather_tiles
    dev = store.slab.device
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(dev)
    mean = torch.tensor(TILE_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(TILE_STD, device=dev).view(1, 3, 1, 1)
    out = {}
    for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        head = idx[:8]
        diff = (gather_tiles(store, head, lut, dtype).float() - torch_route(store.slab, head, mean, std, dtype).float())
        ts = alternate({"kernel": lambda: gather_tiles(store, idx, lut, dtype),
                        "torch_ops": lambda: torch_route(store.slab, idx, mean, std, dtype)}, reps)
        k, t = statistics.median(ts["kernel"]), statistics.median(ts["torch_ops"])
        nbytes = n * H * W * 3 * (1 + (2 if dtype == torch.bfloat16 else 4))
        bps = nbytes / (k * 1e-3)
        out[name] = {"kernel_ms_median": round(k, 4), "torch_ops_ms_median": round(t, 4),
                     "kernel_ms_min_max": [round(min(ts["kernel"]), 4), round(max(ts["kernel"]), 4)],
                     "torch_ops_ms_min_max": [round(min(ts["torch_ops"]), 4), round(max(ts["torch_ops"]), 4)],
                     "speedup": round(t / k, 2), "algorithmic_bytes": nbytes,
                     "kernel_tb_per_s": round(bps / 1e12, 3), "share_of_8_tb_s_spec": round(bps / HBM_SPEC_BPS, 3),
                     "share_of_6_29_tb_s_copy_rate": round(bps / HBM_COPY_BPS, 3),
                     "max_abs_diff_vs_torch_ops_8_tiles": float(diff.abs().max()),
                     "gate_kernel_not_slower": bool(k <= t)}
    return out


def bench_eval_step(store, lut, n, reps):
    from transmil_deepgraft_amd.data import TileBag
    from transmil_deepgraft_amd.encoder import ImageBagModel, simple_cnn
    from transmil_deepgraft_amd.interface import TransMILTask
    from transmil_deepgraft_amd.models import AttMIL
    dev = store.slab.device
    torch.manual_seed(1234)
    model = ImageBagModel(simple_cnn(), AttMIL(2, 1024)).to(dev).eval()
    task = TransMILTask(model)
    idx = torch.arange(n, device=dev).view(1, n)
    bag = TileBag(store, idx, lut)
    resident = TileBag(store, idx, lut).materialize(torch.bfloat16)
    label = torch.tensor([1], device=dev)
    meta = (["slide0"], None, ["patient0"])

    def step(x):
        task.on_validation_epoch_start()
        return task.validation_step((x, label, meta))

    def direct():
        with torch.no_grad():
            return model(resident)

    same = bool(torch.equal(step(bag), step(resident)))
    ts = alternate({"lazy_tile_bag": lambda: step(bag), "resident_bf16_through_task": lambda: step(resident),
                    "resident_bf16_model_only": direct}, reps, warmup=2)
    return {"tiles": n, "chunk": model.model_ft.chunk, "logits_bitwise_equal": same,
            "ms_median": {k: round(statistics.median(v), 3) for k, v in ts.items()},
            "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()},
            "largest_single_gather_tiles": bag.max_launch_tiles,
            "note": "validation_step hands the model bags.float().contiguous() of a tensor batch (an fp32 copy of the "
                    "bag); model_only calls the model on the bf16 tensor as scripts/bench_c5.py does"}


def bench_host_copy(n, reps=5):
    out = {}
    for name, dtype in (("uint8", torch.uint8), ("f32", torch.float32)):
        try:
            host = torch.empty(n, H, W, 3, dtype=dtype).pin_memory()
            host.view(-1)[::4096] = 1                                   # touch the pages
            devt = torch.empty(n, H, W, 3, dtype=dtype, device="cuda")
            devt.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
            ts = [event_ms(lambda: devt.copy_(host, non_blocking=True)) for _ in range(reps)]
            nbytes = host.numel() * host.element_size()
            ms = statistics.median(ts)
            out[name] = {"bytes": nbytes, "ms_median": round(ms, 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                         "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 2)}
            del host, devt
        except RuntimeError as e:                                        # e.g. no pinned memory for this user
            out[name] = {"not_measured": str(e).split("\n")[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_ingest_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("bench_ingest.py measures on the GPU; none is available")
    from transmil_deepgraft_amd.data import ImageBagStore, tile_lut
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    store = ImageBagStore.__new__(ImageBagStore)
    store._alloc([a.n], H, W, dev)
    store._set_coords(None)
    store.slab.copy_(torch.randint(0, 256, store.slab.shape, dtype=torch.uint8, device=dev, generator=g))
    lut = tile_lut().to(dev)
    res = {"device": torch.cuda.get_device_name(0), "tiles": a.n, "tile": [H, W], "reps": a.reps,
           "data": "synthetic (seeded uniform uint8 tiles resident in HBM, random-init weights)",
           "timing": "device events around one call, routes alternating, median"}
    res["kernel_vs_torch_ops"] = bench_kernel(store, lut, a.n, a.reps)
    res["simple_attmil_eval_step"] = bench_eval_step(store, lut, a.n, a.reps)
    res["host_to_device_copy"] = bench_host_copy(a.n)
    ok = all(v["gate_kernel_not_slower"] for v in res["kernel_vs_torch_ops"].values())
    res["gate"] = {"kernel_not_slower_than_torch_ops": ok}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
