"""The reference's YAML configuration for this path, without Lightning.

Reads the same files (`Camelyon/TransMIL.yaml`, `DeepGraft/TransMIL_*.yaml`; read_yaml at
code/utils/utils.py:63-66, but with yaml.SafeLoader) and maps the keys `train.py` hands to
`ModelInterface` / the Trainer (code/train.py:118-160, 178-217, 392-397) onto this framework:

* ``Model.name / n_classes / in_features / out_features`` -> ``models.{name}(...)``
  (ModelInterface.load_model, code/models/model_interface.py:1256-1293); ``in_features``
  follows ``Data.feature_extractor`` as train.py:392-397 sets it (retccl 2048, histoencoder 384,
  ctranspath 784), default 1024 as ModelInterface's default.
* ``Model.backbone`` -> ``features`` runs on bags of features; ``retccl`` wraps the model in the
  on-GPU RetCCL encoder (``encoder.ImageBagModel``, model_interface.py:237-247, 300-316) and
  ``resnet18`` in the frozen ResNet-18 with its trainable 512 -> 512 ``fc`` (:226-234; the MIL
  model then takes 512 features); ``simple`` in the MIL-AB tile CNN (``encoder.SimpleCNN``,
  :270-281; 1024 features).
* ``General.precision`` -> ``compute_dtype``: the reference's 16 / '16-mixed' (fp16 autocast)
  and 'bf16' / 'bf16-mixed' run the bf16 MFMA mode, 32 / '32-true' the fp32 parity mode.
* ``Optimizer.opt / lr / weight_decay``, ``Loss.base_loss`` -> ``TransMILTask``;
  ``General.grad_acc`` -> ``accumulate_grad_batches`` (multi-GPU runs use 10,
  code/train.py:199; single-GPU runs ``grad_acc``, :217).
"""
from __future__ import annotations

import torch
import yaml


class AttrDict(dict):
    """``addict.Dict``-style attribute access (missing keys read as None, as the reference's
    ``cfg.Data.mixup`` etc. do when absent)."""

    def __getattr__(self, key):
        v = self.get(key)
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            v = self[key] = AttrDict(v)      # nested sections stay the same object (writable)
        return v

    def __setattr__(self, key, value):
        self[key] = value


def read_yaml(path) -> AttrDict:
    with open(path) as f:
        return AttrDict(yaml.load(f, Loader=yaml.SafeLoader) or {})


_FEATURE_WIDTH = {"retccl": 2048, "histoencoder": 384, "ctranspath": 784}
_RESNET18_WIDTH = 512      # model_ft.fc = nn.Linear(512, 512) (model_interface.py:159, 234)
_SIMPLE_WIDTH = 1024       # model_ft ends in Linear(53 * 53 * 50, 1024) + ReLU (model_interface.py:270-281)


def _image_backbone(cfg):
    """The on-GPU tile encoder the config asks for (None: bags of features)."""
    if (cfg.Data or {}).get("feature_extractor") is not None:
        return None
    return cfg.Model.backbone if cfg.Model.backbone in ("retccl", "resnet18", "simple") else None


def compute_dtype_for(precision) -> torch.dtype:
    """Lightning precision flag -> the engine's compute dtype."""
    p = str(precision).lower() if precision is not None else "32"
    if p in ("16", "16-mixed", "bf16", "bf16-mixed", "16-true", "bf16-true"):
        return torch.bfloat16
    if p in ("32", "32-true"):
        return torch.float32
    raise ValueError(f"General.precision {precision!r} has no MI355X mode (16 / bf16 / 32)")


def in_features_of(cfg) -> int:
    fe = (cfg.Data or {}).get("feature_extractor") if cfg.Data else None
    if fe in _FEATURE_WIDTH:                                   # code/train.py:392-397
        return _FEATURE_WIDTH[fe]
    if _image_backbone(cfg) == "resnet18":
        given = cfg.Model.in_features
        if given is not None and int(given) != _RESNET18_WIDTH:
            raise ValueError(f"Model.in_features {given} does not match backbone resnet18, whose output "
                             f"(fc = Linear(512, 512)) is {_RESNET18_WIDTH} wide")
        return _RESNET18_WIDTH
    if _image_backbone(cfg) == "simple":
        given = cfg.Model.in_features
        if given is not None and int(given) != _SIMPLE_WIDTH:
            raise ValueError(f"Model.in_features {given} does not match backbone simple, whose output "
                             f"(Linear(140450, 1024) + ReLU) is {_SIMPLE_WIDTH} wide")
        return _SIMPLE_WIDTH
    return int(cfg.Model.in_features or 1024)


def build_model(cfg, device="cuda"):
    """``models.{Model.name}(n_classes, in_features, out_features)`` on the device, in the compute
    dtype of ``General.precision``; wrapped in the RetCCL encoder for ``backbone: retccl``, in the
    ResNet-18 encoder for ``backbone: resnet18`` and in the MIL-AB tile CNN for ``backbone: simple``
    on images (``Model.backbone == 'features'`` keeps feature bags).  The compute dtype is set on every
    model that has ``set_compute_dtype``: TransMIL and its subclasses MDMIL / CTMIL, TransformerMIL and
    AttMIL, whose ``precision: 16`` configs thereby run its bf16 mode (``models/AttMIL.py``)."""
    from . import models
    name = cfg.Model.name
    if not hasattr(models, name):
        raise ValueError(f"Model.name {name!r} is not on the MI355X path "
                         "(TransMIL, MDMIL, CTMIL, TransformerMIL, AttMIL, Chowder, CLAM_MB)")
    klass = getattr(models, name)
    n_classes = int(cfg.Model.n_classes)
    if name == "MDMIL":
        model = klass(n_classes)
    elif name == "Chowder":
        # instancialize's rule (model_interface.py:1278-1293): only the constructor arguments that
        # cfg.Model names are passed, and in_features / out_features are not among Chowder's
        kw = {k: int(cfg.Model[k]) for k in ("features", "r") if cfg.Model.get(k) is not None}
        model = klass(n_classes, **kw)
        # Where the config fixes the bags' width (Data.feature_extractor as code/train.py:392-397 reads
        # it, or an on-GPU tile encoder), it must be Chowder's `features`: nothing maps one width to
        # the other in this model, and the reference's Conv1d(features, 1, 1) cannot take such bags either
        fe = (cfg.Data or {}).get("feature_extractor")
        backbone = _image_backbone(cfg)
        source, width = None, None
        if fe in _FEATURE_WIDTH:
            source, width = f"Data.feature_extractor {fe}", _FEATURE_WIDTH[fe]
        elif backbone is not None:
            source = f"backbone {backbone}"
            width = {"retccl": _FEATURE_WIDTH["retccl"], "resnet18": _RESNET18_WIDTH, "simple": _SIMPLE_WIDTH}[backbone]
        if width is not None and width != model.L:
            raise ValueError(f"Model.name 'Chowder' with features = {model.L} is not on the MI355X path for "
                             f"{source}, whose bags are {width} wide: set Model.features: {width}")
    elif name == "CLAM_MB":
        # instancialize's rule again: only the constructor arguments that cfg.Model names are passed
        # (n_classes among them); in_features / out_features are not CLAM_MB's
        kinds = {"gate": bool, "size_arg": str, "dropout": bool, "k_sample": int, "subtyping": bool}
        kw = {k: kind(cfg.Model[k]) for k, kind in kinds.items() if cfg.Model.get(k) is not None}
        model = klass(n_classes=n_classes, **kw)
        # CLAM_MB's first layer is Linear(1024, 512) for both sizes: where the config fixes the bags'
        # width, it must be 1024 (the reference's size_dict cannot take other bags either)
        fe = (cfg.Data or {}).get("feature_extractor")
        backbone = _image_backbone(cfg)
        source, width = None, None
        if fe in _FEATURE_WIDTH:
            source, width = f"Data.feature_extractor {fe}", _FEATURE_WIDTH[fe]
        elif backbone is not None:
            source = f"backbone {backbone}"
            width = {"retccl": _FEATURE_WIDTH["retccl"], "resnet18": _RESNET18_WIDTH, "simple": _SIMPLE_WIDTH}[backbone]
        if width is not None and width != 1024:
            raise ValueError(f"Model.name 'CLAM_MB' (bags of 1024 features) is not on the MI355X path for "
                             f"{source}, whose bags are {width} wide")
    else:
        model = klass(n_classes, in_features_of(cfg), int(cfg.Model.out_features or 512))
    model = model.to(device)
    dtype = compute_dtype_for(cfg.General.precision if cfg.General else None)
    if hasattr(model, "set_compute_dtype"):
        model.set_compute_dtype(dtype)
    backbone = _image_backbone(cfg)
    if backbone is not None:
        from .encoder import ImageBagModel, resnet18, retccl_resnet50, simple_cnn
        make = {"retccl": retccl_resnet50, "resnet18": resnet18, "simple": simple_cnn}[backbone]
        enc = make().to(device).set_compute_dtype(dtype)
        model = ImageBagModel(enc, model)
    return model


def build_task(cfg, model, n_gpus: int = 1):
    """``TransMILTask`` with the config's optimizer, loss and gradient accumulation."""
    from .interface import TransMILTask
    opt = cfg.Optimizer or AttrDict()
    acc = 10 if n_gpus > 1 else int((cfg.General or {}).get("grad_acc") or 1)
    task = TransMILTask(model, lr=float(opt.lr or 2e-4), opt=opt.opt or "lookahead_radam",
                        weight_decay=float(opt.weight_decay if opt.weight_decay is not None else 0.01),
                        loss=(cfg.Loss or {}).get("base_loss") or "CrossEntropyLoss", accumulate_grad_batches=acc)
    return task


def build_dtfd_task(cfg, device="cuda"):
    """``dtfd.DTFDTask`` for ``DeepGraft/DTFDMIL_*.yaml``.  ``ModelInterface_DTFD`` owns the parameters
    and ``models.DTFDMIL`` is no model class (model_interface_dtfd.py:162-165), so this model does not go
    through ``build_model``.  Read: ``Model.n_classes`` and, where given, ``Model.bag_size`` and
    ``Model.max_pseudo_bags``; the bags are 1024 wide (``self.out_features``, :110) whatever
    ``Model.in_features`` says, and the optimizers are the module's own two Adam (:594-601), not
    ``Optimizer.*``."""
    from .dtfd import DTFDMIL, DTFDTask
    kw = {k: int(cfg.Model[k]) for k in ("bag_size", "max_pseudo_bags") if cfg.Model.get(k) is not None}
    return DTFDTask(DTFDMIL(int(cfg.Model.n_classes), **kw).to(device))
