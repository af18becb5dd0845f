"""Golden fixtures for DTFD-MIL, made by running the REFERENCE blocks of ``code/models/DTFDMIL.py``
(loaded at run time from ``--reference-root``, never at import time) composed exactly as
``ModelInterface_DTFD.forward`` composes them (code/models/model_interface_dtfd.py:174-224, with
``model_ft`` the identity on feature bags) and the training step's two losses (:235-241, 268).

That file imports ``pytorch_lightning``, ``pl_bolts`` and ``torchvision.models`` without using them in
the five classes; where they are absent, empty stand-in modules are put into ``sys.modules`` for the
import.

Weights come from ``dtfd_ref.case_params_``, bags from numpy PCG64 (``dtfd_ref.case_input``), the
permutation from ``torch.randperm(N)`` right after ``torch.manual_seed(seed)`` (the reference's own
draw, :186).  Stored per case, data only: ``perm`` and ``seed``; the reference's fp32 and fp64 ``sub``,
``slide``, ``sub_loss``, ``slide_loss``; ``err32`` (the reference's own max |fp32 - fp64| over the two
logit tensors); the state dict's key names and shapes.  The restatement (tests/dtfd_ref.py) must equal
the reference in fp64 to 1e-12.  ``index.json`` is not touched.

    python tests/golden/make_golden_dtfd.py --reference-root <checkout of the reference>
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for p in (REPO, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

_STAND_INS = ("torchvision", "torchvision.models", "pytorch_lightning", "pl_bolts", "pl_bolts.optimizers",
              "pl_bolts.optimizers.lr_scheduler")


def load_reference_module(root):
    for name in _STAND_INS:
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
            if "." in name:
                setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)
    sched = sys.modules["pl_bolts.optimizers.lr_scheduler"]
    if not hasattr(sched, "LinearWarmupCosineAnnealingLR"):
        sched.LinearWarmupCosineAnnealingLR = None
    path = os.path.join(root, "code", "models", "DTFDMIL.py")
    spec = importlib.util.spec_from_file_location("reference_dtfdmil", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class ReferenceComposition(torch.nn.Module):
    """The four modules of :162-165 under the reference's attribute names."""

    def __init__(self, ref, n_classes):
        super().__init__()
        self.classifier = ref.Classifier_1fc(n_channels=512, n_classes=n_classes)
        self.attention = ref.Attention_Gated(features=512)
        self.dimreduction = ref.DimReduction(n_channels=1024, m_dim=512)
        self.attCls = ref.Attention_with_Classifier(L=512, num_cls=n_classes)

    def forward(self, x, perm, bag_size, cap):
        """:174-224 line by line, the permutation given."""
        max_pseudo_bags = min(cap, x.squeeze(0).shape[0] // bag_size)
        slide_pseudo_feat, sub_predictions = [], []
        features = self.dimreduction(x.squeeze(0))
        for n in range(max_pseudo_bags):
            bag_idxs = perm[bag_size * n:bag_size * (n + 1)]
            # the reference writes features.squeeze(0)[bag_idxs]: the identity on [N, 512] for N > 1; at
            # N = 1 it would drop the instance axis and the reference's Linear fails, so it is left out
            bag_features = features[bag_idxs]
            t1AA = self.attention(bag_features).squeeze(0)
            t1attFeats = torch.einsum("ns, n->ns", bag_features, t1AA)
            t1attFeats_tensor = torch.sum(t1attFeats, dim=0).unsqueeze(0)
            sub_predictions.append(self.classifier(t1attFeats_tensor))
            slide_pseudo_feat.append(t1attFeats_tensor)
        slide_pseudo_feat = torch.cat(slide_pseudo_feat, dim=0)
        sub_predictions = torch.cat(sub_predictions, dim=0)
        slide_prediction = self.attCls(slide_pseudo_feat)
        return sub_predictions, slide_prediction


def losses(sub, slide, label, C):
    """:235-241: CrossEntropyLoss on the one-hot float label repeated G times."""
    hot = F.one_hot(torch.tensor([label]), num_classes=C).to(sub.dtype)
    sub_labels = torch.cat([hot] * sub.size(0), dim=0)
    loss = torch.nn.CrossEntropyLoss()
    return loss(sub, sub_labels), loss(slide, hot)


def main():
    from dtfd_ref import CASES, case_input, case_params_, case_perm, ref_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-root", default=os.environ.get("TRANSMIL_REFERENCE_ROOT"), required=False)
    args = ap.parse_args()
    if not args.reference_root:
        raise SystemExit("give --reference-root (the directory that holds code/models/DTFDMIL.py)")
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    ref = load_reference_module(args.reference_root)
    for seed, (name, (C, N, S, cap, label)) in enumerate(CASES.items()):
        ref32 = case_params_(ReferenceComposition(ref, C), name).eval()
        sd = ref32.state_dict()
        ref64 = ReferenceComposition(ref, C).double().eval()
        ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        mine = ref_model(name)
        assert list(mine.state_dict()) == list(sd)
        assert all(torch.equal(v, sd[k].double()) for k, v in mine.state_dict().items())
        x = torch.from_numpy(case_input(N, seed))
        perm = case_perm(N, seed)
        with torch.no_grad():
            sub32, slide32 = ref32(x[None], perm, S, cap)
            sub64, slide64 = ref64(x[None].double(), perm, S, cap)
            l32, l64 = losses(sub32, slide32, label, C), losses(sub64, slide64, label, C)
            r = mine(x.double(), perm, S, cap, label)
        assert (r["sub"] - sub64).abs().max() < 1e-12 and (r["slide"] - slide64).abs().max() < 1e-12, name
        assert abs(r["sub_loss"] - l64[0]) < 1e-12 and abs(r["slide_loss"] - l64[1]) < 1e-12, name
        top = max(float(sub64.abs().max()), float(slide64.abs().max()))
        assert top >= 1.0, (name, top)
        err32 = max(float((sub32.double() - sub64).abs().max()), float((slide32.double() - slide64).abs().max()))
        out = {"perm": perm.numpy().astype(np.int64), "seed": np.int64(seed),
               "sub": sub32.numpy(), "sub.f64": sub64.numpy(), "slide": slide32.numpy(), "slide.f64": slide64.numpy(),
               "sub_loss": np.float32(l32[0]), "sub_loss.f64": np.float64(l64[0]),
               "slide_loss": np.float32(l32[1]), "slide_loss.f64": np.float64(l64[1]),
               "err32": np.float64(err32), "keys": np.array(list(sd)),
               "shapes": np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])}
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
        a1 = r["a1"]
        print(f"{name}: seed {seed} G {sub64.shape[0]} max |logits| {top:.3f} err32 {err32:.3e} tier-1 scores "
              f"[{float(a1.min()):.2f}, {float(a1.max()):.2f}] max p1 {float(r['p1'].max()):.3f} "
              f"sub_loss {float(l64[0]):.6f} slide_loss {float(l64[1]):.6f}", flush=True)


if __name__ == "__main__":
    main()
