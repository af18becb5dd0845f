"""The ``simple`` tile backbone restated from torch layers -- ``Sequential(Conv2d(3, 20, 5), ReLU,
MaxPool2d(2, 2), Conv2d(20, 50, 5), ReLU, MaxPool2d(2, 2), Flatten, Linear(50 * 53 * 53, width), ReLU)``
-- which runs in fp64 on the CPU, a deterministic parameter generator for it, and the fused
conv + ReLU + pool stage as torch ops: the reference of the SimpleCNN / tm_conv5x5_relu_pool tests."""
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

FEATURES = 50 * 53 * 53


def simple_cnn_ref(width=1024, dtype=torch.float64):
    """The nine-layer Sequential (parameterised layers at indices 0, 3 and 7)."""
    return nn.Sequential(nn.Conv2d(3, 20, 5), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Conv2d(20, 50, 5), nn.ReLU(),
                         nn.MaxPool2d(2, 2), nn.Flatten(1), nn.Linear(FEATURES, width), nn.ReLU()).to(dtype)


def deterministic_simple_params_(model, seed=2021):
    """Fill the six tensors by name, each from PCG64(seed ^ crc32(name)): weights ~ U(+-sqrt(3 / fan_in))
    (unit gain, so the activations keep their scale through the three layers), biases ~ U(-0.1, 0.1)."""
    with torch.no_grad():
        for name, t in model.named_parameters():
            rng = np.random.default_rng(seed ^ zlib.crc32(name.encode()))
            shape = tuple(t.shape)
            a = float(np.sqrt(3.0 / (t.numel() // shape[0]))) if t.dim() > 1 else 0.1
            t.copy_(torch.from_numpy(rng.uniform(-a, a, shape)).to(t.dtype))
    return model


def tiles(n, h=224, w=224, seed=77):
    """Synthetic RGB tiles in the ImageNet-normalised range: PCG64(seed).standard_normal."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3, h, w)).astype(np.float32))


def stage(x, w, b):
    """One conv stage in x's dtype: max_pool2d(relu(conv2d(x, w, b)), 2, 2), NCHW."""
    return F.max_pool2d(F.relu(F.conv2d(x, w, b)), 2, 2)


def forward_fp64(sd, x):
    """fp64 forward of the restatement over a SimpleCNN state_dict: [n, 3, 224, 224] -> [n, width]."""
    width = sd["7.weight"].shape[0]
    ref = simple_cnn_ref(width)
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in sd.items()})
    with torch.no_grad():
        return ref(x.double())
