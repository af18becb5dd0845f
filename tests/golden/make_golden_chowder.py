"""Golden fixtures for Chowder, made by importing the REFERENCE model file
``code/models/Chowder.py`` (its top-level ``pytorch_lightning``, ``pl_bolts`` and
``torchvision.models`` imports are bound to empty stand-in modules: the class uses none of them).

Weights come from ``deterministic_params_(seed=2021)``, inputs from numpy PCG64
(``chowder_ref.case_input``); the bf16 cases feed the reference the bf16-rounded values as fp32.
Stored per case, data only: the reference's fp32 and fp64 logits, ``idx`` (the contract's selection
of the fp64 scores), ``gap`` (the smallest fp64 gap between neighbouring scores among the R + 1
extreme scores at either end), ``max_E`` (the largest per-row fp32 rounding bound,
``chowder_ref.rounding_bound``) and the input seed.  A seed is kept only if ``gap >= 2 max_E``: then
every fp32 evaluation of the scores, whatever its summation order, selects the same instances in
the same order, so ``idx`` is forced.  Otherwise the next seed is tried.

    python tests/golden/make_golden_chowder.py
"""
from __future__ import annotations

import contextlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for p in (REPO, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

REFERENCE_FILE = "/root/reference/code/models/Chowder.py"
FIRST_SEED = 100        # case i starts at FIRST_SEED + 16 i and walks up until the gap condition holds

# name -> (B, N, L, R, classes, bf16 input)
CASES = {
    "chowder_n5": (1, 5, 512, 5, 2, False),                 # N = R: every instance in both selections
    "chowder_n9": (1, 9, 512, 5, 2, False),                 # overlap
    "chowder_n10": (1, 10, 512, 5, 2, False),               # exact cover
    "chowder_b2_n64": (2, 64, 512, 5, 2, False),
    "chowder_n257_c3": (1, 257, 512, 5, 3, False),          # one row past a chunk
    "chowder_b3_n300": (3, 300, 512, 5, 2, False),
    "chowder_n300_l2048": (1, 300, 2048, 5, 2, False),      # retccl-wide features
    "chowder_n33_l8_r3": (1, 33, 8, 3, 2, False),           # smallest L
    "chowder_n64_l64_r32": (1, 64, 64, 32, 2, False),       # N = 2R at the largest R
    "chowder_n300_r1": (1, 300, 512, 1, 2, False),
    "chowder_n8192": (1, 8192, 512, 5, 2, False),
    "chowder_n32768_c3": (1, 32768, 512, 5, 3, False),
    "chowder_b3_n300_bf16": (3, 300, 512, 5, 2, True),
    "chowder_n8192_bf16": (1, 8192, 512, 5, 2, True),
}


def load_reference_class():
    for name in ("torchvision", "torchvision.models", "pytorch_lightning", "pl_bolts", "pl_bolts.optimizers",
                 "pl_bolts.optimizers.lr_scheduler"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["pl_bolts.optimizers.lr_scheduler"].LinearWarmupCosineAnnealingLR = None
    spec = importlib.util.spec_from_file_location("reference_chowder", REFERENCE_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Chowder


@contextlib.contextmanager
def float_is_identity(on):
    """The reference's ``x = x.float()`` kept out of the way of an fp64 run."""
    orig = torch.Tensor.float
    if on:
        torch.Tensor.float = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.float = orig


def main():
    from chowder_ref import ChowderRef, bf16_round, case_input, extreme_gap, rounding_bound, select
    from oracle.transmil_ref import deterministic_params_
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    Reference = load_reference_class()
    for ci, (name, (B, N, L, R, C, bf16)) in enumerate(CASES.items()):
        ref = deterministic_params_(Reference(C, L, R), 2021).eval()
        sd = ref.state_dict()
        mine = ChowderRef(C, L, R).double().eval()
        mine.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        w = sd["f1.0.weight"].double().numpy().reshape(-1)
        bias = float(sd["f1.0.bias"].double())
        for seed in range(FIRST_SEED + 16 * ci, FIRST_SEED + 16 * ci + 16):
            x = case_input((B, N, L), seed)
            if bf16:
                x = bf16_round(x)
            xt = torch.from_numpy(x)
            with torch.no_grad():
                s64 = mine.scores(xt.double())[:, 0, :].numpy()
            gap, max_e = extreme_gap(s64, R), float(rounding_bound(x, w, bias).max())
            if gap >= 2.0 * max_e:
                break
            print(f"  {name}: seed {seed} gap {gap:.3e} < 2 E = {2 * max_e:.3e}, next seed", flush=True)
        else:
            raise SystemExit(f"{name}: no seed met gap >= 2 max_E")
        assert gap >= 2.0 * max_e
        with torch.no_grad():
            logits32 = ref(xt)[0].numpy()
            ref64 = ref.double()
            with float_is_identity(True):
                logits64 = ref64(xt.double())[0].numpy()
            assert np.array_equal(logits64, mine(xt.double())[0].numpy()), "restatement != reference"
        idx = select(s64, R)
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **{
            "logits": logits32, "logits.f64": logits64, "idx": idx, "gap": np.float64(gap),
            "max_E": np.float64(max_e), "seed": np.int64(seed)})
        print(f"{name}: seed {seed} gap {gap:.3e} 2E {2 * max_e:.3e} logits {logits32.reshape(-1)[:3].tolist()}",
              flush=True)


if __name__ == "__main__":
    main()
