"""BASELINE config C5 on one MI355X: on-GPU RetCCL ResNet-50 tile encoder + TransMIL(2048).

One step = tiles [1, N, 3, 224, 224] (bf16, resident in HBM) -> frozen encoder (train-mode
BatchNorm as the reference runs it under Lightning, or --encoder-mode eval: BN folded into the
convolutions) -> features [1, N, 2048] on the device -> TransMIL(2, 2048) fwd (RCC _fc1 branch,
dropout on) -> CE -> bwd -> Lookahead(RAdam).  Prints one JSON line: slides/sec, ms/step, the
encoder alone (ms, tiles/s, achieved TFLOP/s against the dense bf16 peak), the MIL part alone,
a ``roofline`` object for the encoder (the step's dominant part: library convolutions + the HIP
1x1 / BatchNorm passes) and a ``cpu_baseline``: the fp32 CPU oracle of the same step on a stated
sample (oracle/encoder_ref.py on ``--cpu-tiles`` tiles, extrapolated per tile to N, plus the
TransMIL(2048) oracle fwd + CE + bwd + RAdam step at N measured whole).

    python scripts/bench_c5.py [--n 4096] [--steps 20] [--warmup 3] [--encoder-mode train|eval] [--graph]

``--backbone resnet18`` runs the reference's default image configuration instead: the frozen
ResNet-18 (3x3 convolutions on the hand-written tm_conv3x3 kernel) with its 512 -> 512 fc ->
TransMIL(2, 512).  ``--compare-library R`` then also times the same encoder with its 3x3
convolutions routed through the library (MIOpen convolution + tm_bias_act, residual add + ReLU as
torch passes), R rounds alternating with the hand-written kernel; the route exists in this script
only.

``--backbone simple`` runs the MIL-AB tile CNN of the ``AttMIL_simple_*`` configs (two fused 5x5
convolution + ReLU + max-pool launches on tm_conv5x5_relu_pool, Linear(140450, 1024) + ReLU on
tm_gemm) -> AttMIL(2, 1024).  ``--compare-library R`` times the library route beside it: MIOpen
convolutions, torch ReLU / max-pool, the same GEMM over the NCHW-flattened rows.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK_TFS = 2500.0
R50_GFLOP_PER_TILE = 4.09   # ResNet-50 forward at 224x224, multiply-adds x 2 (conv + fc-free)
R18_GFLOP_PER_TILE = 3.63   # ResNet-18 forward at 224x224, multiply-adds x 2 (3.35 of them 3x3 convolutions)
SIMPLE_GFLOP_PER_TILE = 0.995   # 0.145 (3 -> 20 at 220 x 220) + 0.562 (20 -> 50 at 106 x 106) + 0.288 (Linear 140450 -> 1024)


def library_conv3x3(x, w, b, stride, relu, residual=None):
    """encoder._conv3x3's contract on the library route: MIOpen convolution, then the bias / ReLU
    pass (tm_bias_act) and, for a block's second convolution, the residual add + ReLU."""
    from transmil_deepgraft_amd import encoder as E
    y = E._cl(E._lib_conv2d(x, w, None, stride=stride, padding=1))
    if residual is not None:
        if b is not None:
            E._bias_act_(y, b, relu=False)
        y.add_(residual)
        return y.relu_() if relu else y
    if b is not None:
        E._bias_act_(y, b, relu=relu)
    elif relu:
        y.relu_()
    return y


class LibrarySimple:
    """encoder.SimpleCNN's forward on the library route: MIOpen convolutions (channels-last bf16), torch
    ReLU / max-pool, then the same split-K tm_gemm + tm_bias_act over the NCHW-flattened, K-padded rows
    (the weight zero-padded in the reference's own column order)."""

    def __init__(self, enc):
        from transmil_deepgraft_amd.encoder import SIMPLE_K, SIMPLE_KP
        m, dt = dict(enc.named_children()), enc.compute_dtype
        self.enc, self.k, self.kp = enc, SIMPLE_K, SIMPLE_KP
        cl = torch.channels_last
        self.w1, self.b1 = m["0"].weight.detach().to(dt).contiguous(memory_format=cl), m["0"].bias.detach().to(dt)
        self.w2, self.b2 = m["3"].weight.detach().to(dt).contiguous(memory_format=cl), m["3"].bias.detach().to(dt)
        self.wfc = torch.zeros(enc.width, SIMPLE_KP, dtype=dt, device=m["7"].weight.device)
        self.wfc[:, :SIMPLE_K] = m["7"].weight.detach()
        self.bfc = m["7"].bias.detach().float().contiguous()

    def __call__(self, x):
        import torch.nn.functional as F
        from transmil_deepgraft_amd.encoder import simple_fc
        enc = self.enc
        out = torch.empty(x.shape[0], enc.width, dtype=torch.float32, device=x.device)
        with torch.no_grad():
            for s in range(0, x.shape[0], enc.chunk):
                xc = x[s:s + enc.chunk].to(enc.compute_dtype).contiguous(memory_format=torch.channels_last)
                y = F.max_pool2d(F.relu_(F.conv2d(xc, self.w1, self.b1)), 2, 2)
                y = F.max_pool2d(F.relu_(F.conv2d(y, self.w2, self.b2)), 2, 2)
                a = torch.empty(y.shape[0], self.kp, dtype=y.dtype, device=y.device)
                a[:, :self.k].view(y.shape[0], 50, 53, 53).copy_(y)
                a[:, self.k:].zero_()
                simple_fc(a, self.wfc, self.bfc, out[s:s + y.shape[0]])
        return out


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-tiles", type=int, default=64, help="tiles of the CPU encoder sample (0: no cpu_baseline)")
    ap.add_argument("--encoder-mode", default="train", choices=["train", "eval"])
    # tiles per encoder piece: 1024 measured faster than 512 (eval 84.5 vs 89.0 ms per 4096 tiles;
    # smaller pieces slower: profiles/r04u_c5_chunks.txt); every piece tensor stays < 2 GiB (bf16: the
    # encoder clamps pieces to max_tiles_per_call() = 1337 tiles)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--graph", action="store_true", help="capture the step in a hipGraph")
    ap.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"])
    # MIOpen find (torch.backends.cudnn.benchmark) picks the 3x3 / stem convolution kernels by timing
    # them once per shape before the timed region: eval encoder 98.9 -> 89.1 ms per 4096 tiles
    # (profiles/r04p_c5_find.jsonl); --no-benchmark keeps MIOpen's immediate-mode heuristics
    ap.add_argument("--benchmark", action=argparse.BooleanOptionalAction, default=True,
                    help="torch.backends.cudnn.benchmark (MIOpen find)")
    ap.add_argument("--backbone", default="retccl", choices=["retccl", "resnet18", "simple"])
    ap.add_argument("--compare-library", type=int, default=0, metavar="ROUNDS",
                    help="resnet18 / simple: also time the encoder with library convolutions, alternating ROUNDS times")
    a = ap.parse_args()
    torch.backends.cudnn.benchmark = a.benchmark
    from transmil_deepgraft_amd import encoder as encoder_module
    from transmil_deepgraft_amd.encoder import ImageBagModel, resnet18, retccl_resnet50, simple_cnn
    from transmil_deepgraft_amd.interface import GradAllReduce, TransMILTask
    from transmil_deepgraft_amd.models import AttMIL, TransMIL
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    r18 = a.backbone == "resnet18"
    simple = a.backbone == "simple"
    width, gflop = (512, R18_GFLOP_PER_TILE) if r18 else (1024, SIMPLE_GFLOP_PER_TILE) if simple \
        else (2048, R50_GFLOP_PER_TILE)
    make = {"retccl": retccl_resnet50, "resnet18": resnet18, "simple": simple_cnn}[a.backbone]
    enc = make(chunk=a.chunk).to(dev).set_compute_dtype(torch.bfloat16)
    enc.channels_last = a.layout == "nhwc"
    enc.train(a.encoder_mode == "train")
    mil = (AttMIL(2, width, 512) if simple else TransMIL(2, width, 512)).to(dev).train()
    model = ImageBagModel(enc, mil)
    task = TransMILTask(mil)
    opt = task.configure_optimizers()[0][0]
    GradAllReduce(mil.parameters(), model=mil)        # gradient bucket (no-op collective at N = 1)
    g = torch.Generator(device=dev).manual_seed(7)
    tiles = torch.randn(1, a.n, 3, 224, 224, device=dev, generator=g).to(torch.bfloat16)
    label = torch.tensor([1], device=dev)

    def step():
        logits = model(tiles)
        loss = task.loss(logits, torch.nn.functional.one_hot(label, 2).float())
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    for _ in range(a.warmup):
        step()
    run = step
    if a.graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        run = graph.replay
    t_step = timed(run, a.steps)
    with torch.no_grad():
        t_enc = timed(lambda: enc(tiles[0]), a.steps)
        feats = enc(tiles[0])[None]

    def mil_step():
        loss = task.loss(mil(feats), torch.nn.functional.one_hot(label, 2).float())
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    t_mil = timed(mil_step, a.steps)
    enc_tfs = gflop * a.n / t_enc / 1e3
    # the CPU oracle of the encoder is the ResNet-50's (oracle/encoder_ref.py): none for resnet18
    cpu = cpu_baseline(a, enc, mil) if a.cpu_tiles > 0 and not r18 and not simple else None
    library = None
    if simple and a.compare_library > 0:
        lib_enc = LibrarySimple(enc)
        ts = {"hand": [], "library": []}
        with torch.no_grad():
            err = (lib_enc(tiles[0][:64]) - enc(tiles[0][:64])).norm() / enc(tiles[0][:64]).norm()
            lib_enc(tiles[0])                                                    # warm (MIOpen find)
            for _ in range(a.compare_library):
                for route, fn in (("hand", enc), ("library", lib_enc)):
                    ts[route].append(timed(lambda: fn(tiles[0]), a.steps) * 1e3)
        library = {"rounds": a.compare_library, "steps_per_round": a.steps,
                   "encoder_ms_hand": [round(t, 3) for t in ts["hand"]],
                   "encoder_ms_library": [round(t, 3) for t in ts["library"]],
                   "rel_l2_library_vs_hand_64_tiles": float(err),
                   "note": "same process, alternating; library = MIOpen 5x5 convolutions + torch ReLU / max-pool + "
                           "the same split-K tm_gemm"}
    if r18 and a.compare_library > 0:
        hand = encoder_module._conv3x3
        ts = {"hand": [], "library": []}
        with torch.no_grad():
            for route, fn in (("library", library_conv3x3), ("hand", hand)):     # warm both (MIOpen find)
                encoder_module._conv3x3 = fn
                enc(tiles[0])
            for _ in range(a.compare_library):
                for route, fn in (("hand", hand), ("library", library_conv3x3)):
                    encoder_module._conv3x3 = fn
                    ts[route].append(timed(lambda: enc(tiles[0]), a.steps) * 1e3)
        encoder_module._conv3x3 = hand
        library = {"rounds": a.compare_library, "steps_per_round": a.steps,
                   "encoder_ms_hand": [round(t, 3) for t in ts["hand"]],
                   "encoder_ms_library": [round(t, 3) for t in ts["library"]],
                   "note": "same process, alternating; library = MIOpen 3x3 + tm_bias_act (+ torch add / ReLU)"}
    name = "ResNet-18 encoder (fc 512) + TransMIL(512)" if r18 else "simple CNN encoder + AttMIL(1024)" if simple \
        else "RetCCL ResNet-50 encoder + TransMIL(2048)"
    net = "ResNet-18" if r18 else "simple CNN" if simple else "ResNet-50"
    print(json.dumps({
        "metric": f"slides/sec (fwd+bwd) end-to-end, {name}, N={a.n} tiles",
        "value": round(1.0 / t_step, 3), "unit": "slides/sec", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(t_step * 1e3, 3), "higher_is_better": True, "dtype": "bf16",
        "data": "synthetic (randn tiles resident in HBM, random-init weights)",
        "config": {"workload": f"C5: 1 slide x {a.n} tiles 3x224x224 -> {net} (frozen, BN "
                               f"{'none' if simple else 'batch stats' if a.encoder_mode == 'train' else 'folded'}) -> "
                               f"{'AttMIL' if simple else 'TransMIL'} 2-class",
                   "execution": "hipGraph" if a.graph else "eager", "chunk": a.chunk, "layout": a.layout,
                   "miopen_find": a.benchmark, "backbone": a.backbone},
        "encoder": {"ms": round(t_enc * 1e3, 3), "tiles_per_s": round(a.n / t_enc, 1),
                    "achieved_tfs": round(enc_tfs, 1), "peak_tfs": BF16_PEAK_TFS,
                    "frac": round(enc_tfs / BF16_PEAK_TFS, 4), "mode": a.encoder_mode,
                    "flops_note": f"{gflop} GFLOP per 224x224 tile ({net} forward)"},
        "mil_ms": round(t_mil * 1e3, 3),
        "roofline": {"bound": "mfma", "achieved": round(enc_tfs, 1), "peak": BF16_PEAK_TFS, "unit": "TFLOP/s",
                     "frac": round(enc_tfs / BF16_PEAK_TFS, 4), "traffic": None,
                     "kernel": "encoder: two fused conv5x5 + ReLU + max-pool launches (tm_conv5x5_relu_pool), split-K "
                               "tm_gemm + tm_bias_act Linear" if simple else
                               f"encoder ({a.encoder_mode} BN): hand-written stem (conv + BN + ReLU + pool, "
                               "tm_stem_*), " + ("hand-written 3x3 implicit-GEMM convolutions (tm_conv3x3), " if r18
                                                 else "MIOpen / CK 3x3 convolutions, ") +
                               "hipBLASLt 1x1 GEMMs (tm_conv1x1), HIP BatchNorm / bias passes",
                     "algorithmic_flops": int(gflop * 1e9 * a.n), "ms": round(t_enc * 1e3, 3)},
        "cpu_baseline": cpu, "library_comparison": library,
    }), flush=True)


def cpu_baseline(a, enc, mil):
    """The same step on the host's cores through the fp32 oracles: the encoder on a --cpu-tiles sample
    (oracle/encoder_ref.py, the mode's BatchNorm: train = that sample's batch statistics), median of 3,
    scaled per tile to N; the TransMIL(2048) oracle (oracle/transmil_ref.py) fwd + CE + bwd + RAdam at
    N features, median of 3 after one warm-up.  Slides/s = 1 / (extrapolated encoder + MIL step)."""
    import statistics
    from oracle.encoder_ref import features
    from oracle.transmil_ref import TransMIL as RefTransMIL
    threads = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
    torch.set_num_threads(threads)
    sd = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = torch.randn(a.cpu_tiles, 3, 224, 224, generator=g)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        features(x, sd, dtype=torch.float32, train=a.encoder_mode == "train")
        ts.append(time.perf_counter() - t0)
    t_tile = statistics.median(ts) / a.cpu_tiles
    torch.manual_seed(0)
    ref = RefTransMIL(2, 2048, 512).train()
    opt = torch.optim.RAdam(ref.parameters(), lr=2e-4)
    feats = torch.rand(1, a.n, 2048)
    y = torch.nn.functional.one_hot(torch.tensor([1]), 2).float()

    def step():
        loss = torch.nn.functional.cross_entropy(ref(feats), y)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    step()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        step()
        ms.append(time.perf_counter() - t0)
    t_mil = statistics.median(ms)
    t_slide = t_tile * a.n + t_mil
    return {"value": round(1.0 / t_slide, 5), "unit": "slides/sec", "cores": threads, "kind": "port",
            "sample": f"encoder: oracle/encoder_ref.py fp32 on {a.cpu_tiles} tiles ({a.encoder_mode} BN), median of 3, "
                      f"{t_tile * 1e3:.1f} ms per tile extrapolated x {a.n} tiles (EXTRAPOLATED); TransMIL(2048) oracle "
                      f"fwd+CE+bwd+RAdam at N={a.n} measured, median of 3: {t_mil:.3f} s",
            "encoder_s_per_tile": round(t_tile, 5), "mil_step_s": round(t_mil, 4)}


if __name__ == "__main__":
    main()
