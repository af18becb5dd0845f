"""Feature-bag ingest and train-time sampling with the bags resident in HBM.

Mirrors ``FeatureBagLoader`` (code/datasets/feature_dataloader.py:26-431) for the feature-bag
path of the hot loop and ``DataInterface.simple_collate`` (code/datasets/data_interface.py:238-246):

* ``FeatureBagStore``   every bag of a split in ONE device slab ``[total_rows, F]`` (fp32, or
                        bf16 to halve it) plus row offsets: 288 GB of HBM holds whole cohorts
                        (a 40k-tile RetCCL bag is 328 MB fp32), so ingest happens once and the
                        per-step work is a gather, not an HDF5 read + host->device copy.  Loads
                        ``.npy`` / ``.pt`` (``weights_only=True``) / ``.safetensors`` files; the
                        reference's HDF5 reader (h5py, :228-276) is not available in this image.
* ``FeatureBagLoader``  ``__getitem__`` with the reference's sampling, drawing its indices with
                        the SAME RNG calls in the same order (torch.randperm / torch.rand /
                        torch.randint on torch's default CPU generator for train / fine_tune,
                        :346-362 and mixup :305-330; numpy ``seed(0)`` + ``choice`` with
                        replacement for val / test, :421-431), then ONE ``tm_gather_rows``
                        launch builds the sampled, zero-padded, reshuffled bag on the device.
* ``collate``           a whole batch of train bags in one launch -> ``simple_collate``'s
                        ``(bags [B, max_bag_size, F], labels, (names, patients))``.

The image path's twin (``JPGMILDataloader``, code/datasets/jpg_dataloader.py; restated below):

* ``ImageBagStore``     every tile bag of a split as 8-bit RGB in ONE device slab ``[total, H, W, 3]``.
* ``ImageBagLoader``    the reference's ``randperm`` draw on the host, then ONE
                        ``tm_gather_tiles_u8`` launch gathers, normalises (ToTensor + Normalize as a
                        [3][256] table) and zero-pads the tiles into bf16 / fp32.
* ``TileBag``           the lazy form: the encoders pull tiles chunk by chunk in their compute dtype.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F32
from .engine import _p, _stream


def _load_array(path):
    ext = os.path.splitext(path)[1]
    if ext == ".npy":
        return torch.from_numpy(np.load(path, allow_pickle=False))
    if ext == ".pt":
        obj = torch.load(path, map_location="cpu", weights_only=True)
        return obj if torch.is_tensor(obj) else obj["features"]
    if ext == ".safetensors":
        from safetensors.torch import load_file
        return load_file(path)["features"]
    raise ValueError(f"unsupported feature file {path} (.npy / .pt / .safetensors)")


class FeatureBagStore:
    """All bags of one split as rows of one HBM slab."""

    def __init__(self, bags, device="cuda", dtype=torch.float32):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("feature store dtype must be float32 or bfloat16")
        bags = [torch.as_tensor(b) for b in bags]
        if not bags or any(b.dim() != 2 for b in bags):
            raise ValueError("bags must be a non-empty list of [n_i, F] arrays")
        F = bags[0].shape[1]
        if any(b.shape[1] != F for b in bags):
            raise ValueError("every bag must have the same feature width")
        self.F, self.dtype = F, dtype
        self.sizes = [int(b.shape[0]) for b in bags]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.slab = torch.empty(int(self.offsets[-1]), F, dtype=dtype, device=device)
        for b, o, n in zip(bags, self.offsets, self.sizes):
            self.slab[o:o + n].copy_(b.to(dtype), non_blocking=False)

    @classmethod
    def from_files(cls, paths, device="cuda", dtype=torch.float32):
        return cls([_load_array(p) for p in paths], device=device, dtype=dtype)

    def __len__(self):
        return len(self.sizes)

    def bag(self, i):
        o = int(self.offsets[i])
        return self.slab[o:o + self.sizes[i]]


class _Rows:
    """Host description of one sampled bag: row ids (global, -1 = zero row) and blend rows."""

    def __init__(self, i0, i1=None, wa=None, wb=None):
        self.i0 = i0
        self.i1, self.wa, self.wb = i1, wa, wb


class FeatureBagLoader:
    """``FeatureBagLoader.__getitem__`` (feature_dataloader.py:335-431) over a FeatureBagStore.

    ``labels``, ``wsi_names``, ``patients``, ``coords`` are per bag, as the reference caches
    them (:338-344).  Train / fine_tune return ``(bag [max_bag_size, F], label, (wsi_name,
    patient))``; other modes ``(bag [ceil(0.1 n), F], label, (wsi_name, coords, patient))``."""

    def __init__(self, store: FeatureBagStore, labels, mode, n_classes, max_bag_size=1000, mixup=False,
                 wsi_names=None, patients=None, coords=None):
        self.store, self.labels, self.mode, self.n_classes = store, list(labels), mode, n_classes
        self.max_bag_size, self.mixup = max_bag_size, mixup
        n = len(store)
        self.wsi_names = list(wsi_names) if wsi_names is not None else [f"bag{i}" for i in range(n)]
        self.patients = list(patients) if patients is not None else list(self.wsi_names)
        self.coords = list(coords) if coords is not None else [None] * n

    def __len__(self):
        return len(self.store)

    # ---------------------------------------------------------------- host-side index draws
    def _mixup_rows(self, idx):
        """get_mixup_bag (:305-330) on the drawn rows ``idx`` (global row ids)."""
        m = idx.numel()
        a = torch.rand([m])
        rand_x = torch.randint(0, m, [m])
        rand_y = torch.randint(0, m, [m])
        if m < self.max_bag_size:
            sel = torch.randperm(m)[:self.max_bag_size - m]
            i0 = torch.cat([idx, idx[rand_x[sel]]])
            i1 = torch.cat([torch.full([m], -1, dtype=torch.int64), idx[rand_y[sel]]])
            wa = torch.cat([torch.ones(m), a[sel]])
            wb = torch.cat([torch.zeros(m), (1.0 - a)[sel]])
            return _Rows(i0, i1, wa, wb)
        keep = torch.rand(m)
        if not bool((keep != 0).all()):
            # the reference builds a bool row there and torch.stack fails (:327-328)
            raise RuntimeError("mixup: a zero draw makes the reference's stack fail")
        return _Rows(idx)

    def _train_rows(self, index):
        base = int(self.store.offsets[index])
        n = self.store.sizes[index]
        idx = torch.randperm(n)[:self.max_bag_size] + base          # :349-351
        rows = self._mixup_rows(idx) if self.mixup else _Rows(idx)  # :353-354
        k = rows.i0.numel()
        if k < self.max_bag_size:                                   # :356-357 zero padding
            pad = self.max_bag_size - k
            rows.i0 = torch.cat([rows.i0, torch.full([pad], -1, dtype=torch.int64)])
            if rows.i1 is not None:
                rows.i1 = torch.cat([rows.i1, torch.full([pad], -1, dtype=torch.int64)])
                rows.wa = torch.cat([rows.wa, torch.zeros(pad)])
                rows.wb = torch.cat([rows.wb, torch.zeros(pad)])
        perm = torch.randperm(rows.i0.numel())                      # :360-361 shuffle again
        rows.i0 = rows.i0[perm]
        if rows.i1 is not None:
            rows.i1, rows.wa, rows.wb = rows.i1[perm], rows.wa[perm], rows.wb[perm]
        return rows

    def _eval_rows(self, index):
        n = self.store.sizes[index]
        draw = np.random.RandomState(0).choice(n, math.ceil(n * 0.1))    # :421-427 (seed(0) + choice)
        return _Rows(torch.from_numpy(draw.astype(np.int64)) + int(self.store.offsets[index]))

    # ---------------------------------------------------------------- device gather
    def _gather(self, rows_list):
        i0 = torch.cat([r.i0 for r in rows_list])
        blend = any(r.i1 is not None for r in rows_list)
        dev = self.store.slab.device
        out = torch.empty(i0.numel(), self.store.F, dtype=self.store.dtype, device=dev)
        if i0.numel() == 0:
            return out
        i0d = i0.to(dev)
        i1d = wad = wbd = None
        if blend:
            i1 = torch.cat([r.i1 if r.i1 is not None else torch.full_like(r.i0, -1) for r in rows_list])
            wa = torch.cat([r.wa if r.wa is not None else torch.ones(r.i0.numel()) for r in rows_list])
            wb = torch.cat([r.wb if r.wb is not None else torch.zeros(r.i0.numel()) for r in rows_list])
            i1d, wad, wbd = i1.to(dev), wa.float().to(dev), wb.float().to(dev)
        for s in range(0, i0.numel(), 65535):
            e = min(i0.numel(), s + 65535)
            _lib.call("tm_gather_rows", BF16 if self.store.dtype == torch.bfloat16 else F32, _p(self.store.slab),
                      self.store.F, _p(i0d[s:e]), _p(i1d[s:e] if blend else None),
                      _p(wad[s:e] if blend else None), _p(wbd[s:e] if blend else None), e - s, _p(out[s:e]),
                      _stream())
        return out

    def __getitem__(self, index):
        label = self.labels[index]
        name, patient, coords = self.wsi_names[index], self.patients[index], self.coords[index]
        if self.mode in ("train", "fine_tune"):
            return self._gather([self._train_rows(index)]), label, (name, patient)
        return self._gather([self._eval_rows(index)]), label, (name, coords, patient)

    def collate(self, indices):
        """The items ``indices`` (train / fine_tune mode) drawn in order, as
        ``simple_collate`` returns them (data_interface.py:238-246), gathered in one launch."""
        if self.mode not in ("train", "fine_tune"):
            raise ValueError("collate stacks fixed-size bags: train / fine_tune mode only")
        rows = [self._train_rows(i) for i in indices]
        bags = self._gather(rows).view(len(indices), self.max_bag_size, self.store.F)
        labels = torch.tensor(np.stack([self.labels[i] for i in indices], axis=0)).long()
        return bags, labels, ([self.wsi_names[i] for i in indices], [self.patients[i] for i in indices])


# ---------------------------------------------------------------------------------- image path
# ``JPGMILDataloader`` (code/datasets/jpg_dataloader.py), the loader of every backbone other than
# ``features`` (code/datasets/data_interface.py:169-170), restated here: torchvision, cv2, imgaug and
# monai are not installed, so the reference file cannot be imported and this parity is pinned by
# restatement, not by a reference run.
#
# * ``get_data`` (:229-276) reads a slide directory's tiles in ``Path(dir).iterdir()`` order (not
#   sorted), each through ``ToTensor()`` + ``Normalize(mean, std)`` (:164-171), and parses
#   ``coords`` from the last ``(x-y)`` group of the file stem (:246-248).
# * ``to_fixed_size_bag`` (:284-293) draws ``torch.randperm(n)[:bag_size]`` (one call on the default
#   CPU generator) and appends ``bag_size - k`` all-zero tiles AFTER normalisation (a pad tile is
#   0.0, not pixel value 0); the coords are indexed, not padded.
# * ``__getitem__`` (:306-361): modes ``train`` and ``val`` sample, every other mode returns the
#   whole bag in directory order and draws nothing; the item is ``(tiles, label, (wsi_name, coords,
#   patient))``.  Batches come from a plain DataLoader: default collate, no sampler, no shuffle
#   (data_interface.py:220-221).
#
# ToTensor + Normalize is a function of (channel, byte value): HWC uint8 -> CHW,
# ``.to(float32).div(255)``, then ``sub_(mean).div_(std)`` with float32 mean / std tensors.
# ``tile_lut`` evaluates exactly those torch CPU ops on the 256 byte values; the kernel
# (csrc/tiles.hip) only looks values up.

TILE_MEAN = (0.485, 0.456, 0.406)     # jpg_dataloader.py:168
TILE_STD = (0.229, 0.224, 0.225)      # jpg_dataloader.py:169


def tile_lut(mean=TILE_MEAN, std=TILE_STD):
    """[3, 256] fp32 on the CPU: ``lut[c][v]`` = ToTensor + Normalize of byte value v in channel c,
    with torchvision's own arithmetic (see above)."""
    v = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    x = v.view(1, 256, 1).expand(3, 256, 1).contiguous()              # CHW, one "pixel" per byte value
    x = x.to(dtype=torch.float32).div(255)                            # ToTensor
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
    if m.numel() != 3 or s.numel() != 3 or bool((s == 0).any()):
        raise ValueError("tile_lut: three means and three non-zero stds expected")
    return x.sub_(m).div_(s).view(3, 256).contiguous()                # Normalize


def parse_tile_coords(stem):
    """``[int(x), int(y)]`` from the last ``(x-y)`` group of a tile's file stem (:246-248)."""
    import re
    pos = re.findall(r"\((.*?)\)", stem)
    x, y = pos[-1].split("-")
    return [int(x), int(y)]


def _load_tiles(path):
    """``(tiles uint8 [n, H, W, 3], coords or None)`` of one bag file (``_load_array``'s formats)."""
    ext = os.path.splitext(path)[1]
    if ext == ".npy":
        return torch.from_numpy(np.load(path, allow_pickle=False)), None
    if ext == ".pt":
        obj = torch.load(path, map_location="cpu", weights_only=True)
    elif ext == ".safetensors":
        from safetensors.torch import load_file
        obj = load_file(path)
    else:
        raise ValueError(f"unsupported tile file {path} (.npy / .pt / .safetensors)")
    if torch.is_tensor(obj):
        return obj, None
    return obj["tiles"], obj.get("coords")


def _decode_tile(path):
    """One tile file as an HWC uint8 array; like the reference, nothing is converted: a file that is
    not 8-bit 3-channel is an error."""
    from PIL import Image
    with Image.open(path) as img:
        if img.mode != "RGB":
            raise ValueError(f"{path}: an 8-bit 3-channel (RGB) tile expected, got PIL mode {img.mode}")
        return np.array(img)


class ImageBagStore:
    """All tile bags of one split as 8-bit RGB tiles ``[total, H, W, 3]`` in ONE HBM slab (150 528 B
    per 224 x 224 tile, a quarter of fp32), plus tile offsets, bag sizes and the per-bag tile
    coordinates (int64 ``[n_i, 2]``, host; zeros where none are given)."""

    def __init__(self, bags, coords=None, device="cuda"):
        bags = [torch.as_tensor(b) for b in bags]
        if not bags:
            raise ValueError("bags must be a non-empty list of uint8 [n_i, H, W, 3] arrays")
        for i, b in enumerate(bags):
            if b.dtype != torch.uint8 or b.dim() != 4 or b.shape[3] != 3:
                raise ValueError(f"bag {i}: a uint8 [n, H, W, 3] array expected, got {b.dtype} {tuple(b.shape)}")
            if tuple(b.shape[1:3]) != tuple(bags[0].shape[1:3]):
                raise ValueError(f"bag {i}: tiles are {b.shape[1]} x {b.shape[2]}, bag 0's are "
                                 f"{bags[0].shape[1]} x {bags[0].shape[2]}")
        self._alloc([int(b.shape[0]) for b in bags], int(bags[0].shape[1]), int(bags[0].shape[2]), device)
        for i, b in enumerate(bags):               # bag by bag: no second host copy of the cohort
            self.bag(i).copy_(b)
        self._set_coords(coords)

    def _alloc(self, sizes, H, W, device):
        if H <= 0 or W <= 0:
            raise ValueError("tiles must have a positive height and width")
        self.H, self.W = H, W
        self.sizes = list(sizes)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.slab = torch.empty(int(self.offsets[-1]), H, W, 3, dtype=torch.uint8, device=device)
        self.names = None

    def _set_coords(self, coords):
        if coords is None:
            coords = [None] * len(self.sizes)
        if len(coords) != len(self.sizes):
            raise ValueError(f"{len(coords)} coords arrays for {len(self.sizes)} bags")
        self.coords = []
        for i, (c, n) in enumerate(zip(coords, self.sizes)):
            c = torch.zeros(n, 2, dtype=torch.int64) if c is None else torch.as_tensor(c).to(torch.int64).cpu()
            if tuple(c.shape) != (n, 2):
                raise ValueError(f"bag {i}: coords must be [{n}, 2], got {tuple(c.shape)}")
            self.coords.append(c)

    @classmethod
    def from_files(cls, paths, device="cuda"):
        loaded = [_load_tiles(p) for p in paths]
        return cls([t for t, _ in loaded], [c for _, c in loaded], device=device)

    @classmethod
    def from_directories(cls, dirs, device="cuda"):
        """One bag per directory of tile images, decoded with PIL in ``Path(dir).iterdir()`` order
        (``get_data``, :234-252); ``names`` holds the directories' stems (the reference's wsi_name,
        :262)."""
        from pathlib import Path
        files = [list(Path(d).iterdir()) for d in dirs]
        first = next((f[0] for f in files if f), None)
        if first is None:
            raise ValueError("from_directories: no tile files")
        H, W = _decode_tile(first).shape[:2]
        self = cls.__new__(cls)
        self._alloc([len(f) for f in files], H, W, device)
        coords = []
        for i, fs in enumerate(files):
            host = torch.empty(len(fs), H, W, 3, dtype=torch.uint8)
            for j, p in enumerate(fs):
                a = _decode_tile(p)
                if a.dtype != np.uint8 or a.shape != (H, W, 3):
                    raise ValueError(f"{p}: a uint8 {H} x {W} x 3 tile expected, got {a.dtype} {a.shape}")
                host[j] = torch.from_numpy(a)
            self.bag(i).copy_(host)
            coords.append(torch.tensor([parse_tile_coords(p.stem) for p in fs], dtype=torch.int64).view(-1, 2))
        self._set_coords(coords)
        self.names = [Path(d).stem for d in dirs]
        return self

    def __len__(self):
        return len(self.sizes)

    def bag(self, i):
        o = int(self.offsets[i])
        return self.slab[o:o + self.sizes[i]]


def gather_tiles(store, idx, lut, dtype=torch.bfloat16, layout="nchw"):
    """ONE ``tm_gather_tiles_u8`` launch: tiles ``idx`` (device int64, global tile ids; outside the
    store = an all-zero tile) of the store, normalised through ``lut`` (device fp32 [3, 256]) into
    a new ``[n, 3, H, W]`` tensor of ``dtype`` -- contiguous (``"nchw"``) or in channels-last
    strides (``"nhwc"``)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("tile dtype must be float32 or bfloat16")
    if layout not in ("nchw", "nhwc"):
        raise ValueError("tile layout must be 'nchw' or 'nhwc'")
    dev = store.slab.device
    if idx.dtype != torch.int64 or idx.device != dev or lut.device != dev or lut.dtype != torch.float32 or \
            tuple(lut.shape) != (3, 256):
        raise ValueError("gather_tiles: int64 indices and an fp32 [3, 256] table on the store's device expected")
    idx = idx.reshape(-1).contiguous()
    n, H, W = idx.numel(), store.H, store.W
    out = torch.empty(n, 3, H, W, dtype=dtype, device=dev,
                      memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format)
    if n:
        sn, sc, sh, sw = (H * W * 3, 1, W * 3, 3) if layout == "nhwc" else (3 * H * W, H * W, W, 1)
        _lib.call("tm_gather_tiles_u8", BF16 if dtype == torch.bfloat16 else F32, _p(store.slab),
                  store.slab.shape[0], H, W, _p(idx), n, _p(lut.contiguous()), _p(out), sn, sc, sh, sw, _stream())
    return out


class TileBag:
    """A batch of tile bags ``[B, bag, 3, H, W]`` that is not held: the store, a device int64
    index tensor ``[B, bag]`` (global tile ids, -1 = a zero pad tile) and the normalisation table.
    The encoders pull tiles ``[s:e]`` of the flattened ``[B * bag]`` bag chunk by chunk in their
    compute dtype, so in eval mode the float bag never exists.  ``launches`` counts the gathers
    and ``max_launch_tiles`` records the largest tile count of any single one."""

    def __init__(self, store, idx, lut):
        if idx.dim() != 2 or idx.dtype != torch.int64 or idx.device != store.slab.device:
            raise ValueError("TileBag: a device int64 [B, bag] index tensor expected")
        self.store, self.idx, self.lut = store, idx.contiguous(), lut
        self.launches = 0
        self.max_launch_tiles = 0

    @property
    def shape(self):
        return torch.Size((self.idx.shape[0], self.idx.shape[1], 3, self.store.H, self.store.W))

    @property
    def device(self):
        return self.idx.device

    @property
    def is_cuda(self):
        return self.idx.is_cuda

    @property
    def n_tiles(self):
        return self.idx.numel()

    def tiles(self, s, e, dtype=torch.bfloat16, layout="nchw"):
        """Tiles ``[s:e]`` of the flattened bag as ``[e - s, 3, H, W]`` in ``dtype``: one launch."""
        part = self.idx.view(-1)[s:e]
        if part.numel():
            self.launches += 1
            self.max_launch_tiles = max(self.max_launch_tiles, part.numel())
        return gather_tiles(self.store, part, self.lut, dtype, layout)

    def materialize(self, dtype=torch.bfloat16, layout="nchw"):
        """The whole ``[B, bag, 3, H, W]`` tensor in ``dtype``: one launch."""
        return self.tiles(0, self.n_tiles, dtype, layout).view(*self.shape)


class ImageBagLoader:
    """``JPGMILDataloader.__getitem__`` (jpg_dataloader.py:306-361) over an ImageBagStore: the
    reference's index draw on the host with the same RNG call, then ONE ``tm_gather_tiles_u8``
    launch gathers, normalises and zero-pads the bag on the device in ``dtype``.

    ``train`` / ``val``: ``torch.randperm(n)[:max_bag_size]`` followed by pad tiles up to
    ``max_bag_size`` (:288-292); any other mode: the whole bag in store order, no RNG call.  Items
    are ``(tiles [bag, 3, H, W], label, (wsi_name, coords[idx] int64 [k, 2], patient))``.
    ``layout="nhwc"`` returns the same logical tensor in channels-last strides.  With
    ``lazy=True`` the tiles are a ``TileBag`` (one bag: ``[1, bag, 3, H, W]``; ``collate``:
    ``[B, bag, 3, H, W]``) instead of a tensor, and nothing is launched here."""

    def __init__(self, store: ImageBagStore, labels, mode, n_classes, max_bag_size=500, dtype=torch.bfloat16,
                 layout="nchw", wsi_names=None, patients=None, lazy=False, *, mean=TILE_MEAN, std=TILE_STD):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("tile dtype must be float32 or bfloat16")
        if layout not in ("nchw", "nhwc"):
            raise ValueError("tile layout must be 'nchw' or 'nhwc'")
        self.store, self.labels, self.mode, self.n_classes = store, list(labels), mode, n_classes
        self.max_bag_size, self.dtype, self.layout, self.lazy = max_bag_size, dtype, layout, lazy
        n = len(store)
        if wsi_names is None:
            wsi_names = store.names if store.names is not None else [f"bag{i}" for i in range(n)]
        self.wsi_names = list(wsi_names)
        self.patients = list(patients) if patients is not None else list(self.wsi_names)
        self.lut = tile_lut(mean, std).to(store.slab.device)          # once per loader

    def __len__(self):
        return len(self.store)

    @property
    def sampling(self):
        return self.mode in ("train", "val")                          # :319

    def draw(self, index):
        """The host side of one item: ``(idx, coords)`` -- int64 tile ids within bag ``index``
        with -1 for every pad tile, and ``coords[idx]`` of the real tiles (not padded)."""
        n = self.store.sizes[index]
        if self.sampling:
            idx = torch.randperm(n)[:self.max_bag_size]                # :288
            pad = self.max_bag_size - idx.numel()                      # :291-292
        else:
            idx, pad = torch.arange(n), 0                              # :355-358
        coords = self.store.coords[index][idx]                         # :290
        return torch.cat([idx, torch.full([pad], -1, dtype=torch.int64)]), coords

    def _global(self, index, idx):
        """Bag-local ids -> tile ids of the slab (pads stay -1), checked against the store here on
        the host: the kernel's out-of-range rule only guards foreign callers."""
        n = self.store.sizes[index]
        if idx.numel() and (int(idx.max()) >= n or int(idx.min()) < -1):
            raise IndexError(f"bag {index}: tile index outside [0, {n})")
        return torch.where(idx >= 0, idx + int(self.store.offsets[index]), idx)

    def _tiles(self, g):
        """[B, bag] host ids -> the loader's output for them (one launch, or a lazy TileBag)."""
        gd = g.to(self.store.slab.device)
        if self.lazy:
            return TileBag(self.store, gd, self.lut)
        return gather_tiles(self.store, gd, self.lut, self.dtype, self.layout).view(
            g.shape[0], g.shape[1], 3, self.store.H, self.store.W)

    def __getitem__(self, index):
        idx, coords = self.draw(index)
        tiles = self._tiles(self._global(index, idx).view(1, -1))
        if not self.lazy:
            tiles = tiles[0]
        return tiles, self.labels[index], (self.wsi_names[index], coords, self.patients[index])

    def collate(self, indices):
        """The items ``indices`` (train / val mode) drawn in order and stacked as the default collate
        stacks them: ``(tiles [B, bag, 3, H, W], labels long [B], (names, [coords...], patients))``,
        gathered in one launch."""
        if not self.sampling:
            raise ValueError("collate stacks fixed-size bags: train / val mode only")
        draws = [self.draw(i) for i in indices]
        g = torch.stack([self._global(i, d[0]) for i, d in zip(indices, draws)])
        labels = torch.tensor(np.stack([self.labels[i] for i in indices], axis=0)).long()
        return self._tiles(g), labels, ([self.wsi_names[i] for i in indices], [d[1] for d in draws],
                                        [self.patients[i] for i in indices])


def simple_collate(data):
    """``DataInterface.simple_collate`` (data_interface.py:238-246) for items already on the device."""
    bags = torch.stack([d[0] for d in data])
    labels = torch.Tensor(np.stack([d[1] for d in data], axis=0)).long()
    return bags, labels, ([d[2][0] for d in data], [d[2][1] for d in data])
