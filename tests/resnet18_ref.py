"""torchvision's ``resnet18`` restated functionally in fp64 (F.conv2d, eval or batch-statistics
BatchNorm, ReLU, max-pool, mean, fc) over a name -> tensor dict, and a deterministic parameter /
BN-statistics generator for it -- the reference of the ResNet-18 encoder tests (torchvision is not a
dependency of the project)."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

STAGES = [(64, 1), (128, 2), (256, 2), (512, 2)]     # planes, stride of the stage's first block
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def state_dict_layout(fc_out=512):
    """(name, shape) of every state_dict entry in torchvision's order."""
    out = [("conv1.weight", (64, 3, 7, 7))]

    def bn(pre, c):
        return [(f"{pre}.{k}", () if k == "num_batches_tracked" else (c,)) for k in BN_KEYS]

    out += bn("bn1", 64)
    inp = 64
    for si, (planes, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            pre = f"layer{si}.{bi}"
            cin = inp if bi == 0 else planes
            out += [(f"{pre}.conv1.weight", (planes, cin, 3, 3))] + bn(f"{pre}.bn1", planes)
            out += [(f"{pre}.conv2.weight", (planes, planes, 3, 3))] + bn(f"{pre}.bn2", planes)
            if bi == 0 and (stride != 1 or inp != planes):
                out += [(f"{pre}.downsample.0.weight", (planes, inp, 1, 1))] + bn(f"{pre}.downsample.1", planes)
        inp = planes
    return out + [("fc.weight", (fc_out, 512)), ("fc.bias", (fc_out,))]


def deterministic_resnet18_params_(model, seed=2021):
    """Fill a ResNet-18's parameters and BN running statistics by name, each tensor from
    PCG64(seed ^ crc32(name)): conv / fc weights ~ U(+-sqrt(3 / fan_in)); BN weight ~ U(0.5, 1)
    (bn2 of each block ~ U(0.1, 0.5), which keeps the 8 residual additions bounded); biases and
    running_mean ~ U(-0.1, 0.1); running_var ~ U(0.5, 1.5)."""
    with torch.no_grad():
        for name, t in list(model.named_parameters()) + list(model.named_buffers()):
            if name.endswith("num_batches_tracked"):
                continue
            rng = np.random.default_rng(seed ^ zlib.crc32(name.encode()))
            shape = tuple(t.shape)
            if t.dim() in (2, 4):
                a = float(np.sqrt(3.0 / (t.numel() // shape[0])))
                val = rng.uniform(-a, a, shape)
            elif name.endswith("running_var"):
                val = rng.uniform(0.5, 1.5, shape)
            elif name.endswith(("running_mean", ".bias")):
                val = rng.uniform(-0.1, 0.1, shape)
            elif name.endswith("bn2.weight"):
                val = rng.uniform(0.1, 0.5, shape)
            elif name.endswith(".weight"):
                val = rng.uniform(0.5, 1.0, shape)
            else:
                raise ValueError(f"unexpected encoder tensor {name}")
            t.copy_(torch.from_numpy(np.asarray(val)).to(t.dtype))
    return model


def tiles(n, h=224, w=224, seed=77):
    """Synthetic RGB tiles in the ImageNet-normalised range: PCG64(seed).standard_normal."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3, h, w)).astype(np.float32))


def resnet18_fp64(sd, x, train=False, eps=1e-5, momentum=0.1):
    """fp64 forward over a state_dict ``sd``: returns (body features [n, 512], fc output, the
    BatchNorm running statistics after the call -- updated in train mode as nn.BatchNorm2d does,
    with the batch statistics over all n tiles)."""
    p = {k: v.detach().double().cpu() for k, v in sd.items()}
    stats = {}

    def bn(t, pre):
        if train:
            mean = t.mean((0, 2, 3))
            var = t.var((0, 2, 3), unbiased=False)
            cnt = t.numel() // t.shape[1]
            stats[pre + ".running_mean"] = (1 - momentum) * p[pre + ".running_mean"] + momentum * mean
            stats[pre + ".running_var"] = (1 - momentum) * p[pre + ".running_var"] + momentum * var * cnt / (cnt - 1)
        else:
            mean, var = p[pre + ".running_mean"], p[pre + ".running_var"]
        s = p[pre + ".weight"] / torch.sqrt(var + eps)
        return t * s[None, :, None, None] + (p[pre + ".bias"] - mean * s)[None, :, None, None]

    t = F.conv2d(x.double(), p["conv1.weight"], stride=2, padding=3)
    t = F.max_pool2d(F.relu(bn(t, "bn1")), 3, 2, 1)
    for si, (_, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            pre = f"layer{si}.{bi}"
            y = F.relu(bn(F.conv2d(t, p[pre + ".conv1.weight"], stride=stride if bi == 0 else 1, padding=1), pre + ".bn1"))
            y = bn(F.conv2d(y, p[pre + ".conv2.weight"], padding=1), pre + ".bn2")
            idt = t
            if pre + ".downsample.0.weight" in p:
                idt = bn(F.conv2d(t, p[pre + ".downsample.0.weight"], stride=stride), pre + ".downsample.1")
            t = F.relu(y + idt)
    body = t.mean((2, 3))
    return body, body @ p["fc.weight"].T + p["fc.bias"], stats
