"""Image tile-bag ingest on the MI355X: tm_gather_tiles_u8 against ``lut[c][src[idx]]`` evaluated
with torch on the device (every comparison exact, destinations poisoned with NaN first), the
loader against the restated reference pipeline on the CPU, and the encoders / the task on a lazy
TileBag against the materialised tensor."""
import copy
import functools

import pytest
import torch

from image_ingest_ref import getitem, random_bags

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 224 * 224 * 3
DTYPES = [torch.bfloat16, torch.float32]
IDX = [4, -1, 0, 0, 2, 7, -5]            # repeats, pads, an index past the 5-tile store


@functools.lru_cache(maxsize=None)
def _lut():
    from transmil_deepgraft_amd.data import tile_lut
    return tile_lut().to(DEV)


def _launch(src, ntiles, H, W, idx, out, n=None):
    """tm_gather_tiles_u8 into ``out`` ([n, 3, H, W] at any strides)."""
    from transmil_deepgraft_amd import _lib
    from transmil_deepgraft_amd.engine import _p, _stream
    sn, sc, sh, sw = out.stride()
    _lib.call("tm_gather_tiles_u8", _lib.BF16 if out.dtype == torch.bfloat16 else _lib.F32, _p(src), ntiles, H, W,
              _p(idx), idx.numel() if n is None else n, _p(_lut()), _p(out), sn, sc, sh, sw, _stream())


def _poisoned(n, H, W, dtype, layout="nchw", shift=0):
    """A NaN-filled [n, 3, H, W] destination: contiguous or channels-last strides, optionally
    ``shift`` elements into its allocation (a base no vector store may touch)."""
    buf = torch.full((n * 3 * H * W + shift,), float("nan"), dtype=dtype, device=DEV)[shift:]
    return buf.view(n, 3, H, W) if layout == "nchw" else buf.view(n, H, W, 3).permute(0, 3, 1, 2)


def _expected(src, idx, dtype):
    """lut[c][src[idx]] in ``dtype`` with torch ops on the device; an index outside the store = zeros."""
    lut = _lut().to(dtype)
    idx = torch.as_tensor(idx, device=src.device)
    ok = (idx >= 0) & (idx < src.shape[0])
    t = src[idx.clamp(0, src.shape[0] - 1)].long()                    # [n, H, W, 3]
    val = torch.stack([lut[c][t[..., c]] for c in range(3)], dim=1)   # [n, 3, H, W]
    return torch.where(ok.view(-1, 1, 1, 1), val, torch.zeros((), dtype=dtype, device=src.device))


def _store_tiles(H, W, offset, seed=0):
    """A 5-tile slab, at the allocation's base or one tile into it (then the base itself is
    misaligned whenever H * W * 3 is no multiple of 16)."""
    g = torch.Generator().manual_seed(seed + H * 1000 + W)
    return torch.randint(0, 256, (5 + offset, H, W, 3), dtype=torch.uint8, generator=g).to(DEV)[offset:]


SHAPES = [(1, 1), (5, 7), (6, 6), (3, 16), (4, 40), (224, 224)]       # 3, 105, 108, 144, 480, 150528 B tiles


@pytest.mark.parametrize("offset", [0, 1], ids=["base", "one_tile_in"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_kernel_matches_the_table_lookup(H, W, dtype, layout, offset):
    src = _store_tiles(H, W, offset)
    assert src.data_ptr() % 16 == (offset * H * W * 3) % 16
    idx = torch.tensor(IDX, device=DEV)
    out = _poisoned(len(IDX), H, W, dtype, layout)
    _launch(src, 5, H, W, idx, out)
    want = _expected(src, IDX, dtype)
    assert torch.equal(out, want)
    assert not bool(out[1].any()) and not bool(out[5].any()) and not bool(out[6].any())   # exactly 0.0
    assert bool(out[0].all())                                          # no real pixel maps to 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("H,W", [(3, 16), (224, 224)], ids=["3x16", "224x224"])
def test_unaligned_bases_give_the_same_bits(H, W, dtype):
    """A destination one element into its allocation, and one whose rows are padded to an odd
    pitch, cannot take 16-B stores; a slab one byte into its allocation cannot be read as dwords:
    the element-wise path writes the same bits."""
    src = _store_tiles(H, W, 0)
    idx = torch.tensor(IDX, device=DEV)
    want = _expected(src, IDX, dtype)
    odd = torch.empty(src.numel() + 1, dtype=torch.uint8, device=DEV)[1:]
    odd.copy_(src.view(-1))
    assert odd.data_ptr() % 4 == 1
    out = _poisoned(len(IDX), H, W, dtype)
    _launch(odd, 5, H, W, idx, out)
    assert torch.equal(out, want)
    out = _poisoned(len(IDX), H, W, dtype, shift=1)
    _launch(src, 5, H, W, idx, out)
    assert torch.equal(out, want)
    wide = torch.full((len(IDX), 3, H, W + 3), float("nan"), dtype=dtype, device=DEV)
    _launch(src, 5, H, W, idx, wide[..., :W])
    assert torch.equal(wide[..., :W], want) and bool(torch.isnan(wide[..., W:]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_no_tiles_launches_nothing_and_one_tile_works(dtype):
    src = _store_tiles(3, 16, 0)
    idx = torch.tensor([3], device=DEV)
    out = _poisoned(1, 3, 16, dtype)
    _launch(src, 5, 3, 16, idx, out, n=0)
    assert bool(torch.isnan(out).all())
    _launch(src, 5, 3, 16, idx, out, n=1)
    assert torch.equal(out, _expected(src, [3], dtype))


def test_source_addressing_is_64_bit():
    """A slab past 2^31 bytes; only its first and last three tiles are filled, idx hits both ends."""
    nt = -(-(2 ** 31 + 3 * TILE) // TILE)                               # 14270 tiles, 2.15 GB
    assert (nt - 3) * TILE > 2 ** 31
    slab = torch.empty(nt, 224, 224, 3, dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(1)
    ends = torch.randint(0, 256, (6, 224, 224, 3), dtype=torch.uint8, generator=g).to(DEV)
    slab[:3] = ends[:3]
    slab[nt - 3:] = ends[3:]
    pick = [0, nt - 1, 2, nt - 3, 1, nt - 2, nt]                        # nt itself: outside, zeros
    small = [0, 5, 2, 3, 1, 4, 6]
    out = _poisoned(len(pick), 224, 224, torch.bfloat16)
    _launch(slab, nt, 224, 224, torch.tensor(pick, device=DEV), out)
    assert torch.equal(out, _expected(ends, small, torch.bfloat16))


def test_destination_addressing_is_64_bit():
    """3600 fp32 tiles out of a 4-tile store: 2.17 GB of output; first, middle and last 3 tiles."""
    n = 3600
    src = _store_tiles(224, 224, 0)[:4]
    idx = (torch.arange(n) * 7 % 5 - 1).to(DEV)                        # -1 (pad), 0 .. 3
    out = _poisoned(n, 224, 224, torch.float32)
    assert out.numel() * 4 > 2 ** 31
    _launch(src, 4, 224, 224, idx, out)
    for s in (0, n // 2 - 1, n - 3):
        assert torch.equal(out[s:s + 3], _expected(src, idx[s:s + 3], torch.float32)), s
    assert not bool(torch.isnan(out[-1]).any())


def test_two_launches_are_bitwise_equal():
    src = _store_tiles(224, 224, 0)
    idx = torch.tensor(IDX, device=DEV)
    a = _poisoned(len(IDX), 224, 224, torch.bfloat16)
    b = _poisoned(len(IDX), 224, 224, torch.bfloat16)
    _launch(src, 5, 224, 224, idx, a)
    _launch(src, 5, 224, 224, idx, b)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


SIZES = [3, 8, 20]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("H,W", [(5, 7), (4, 16)], ids=["5x7", "4x16"])
def test_loader_matches_the_restated_reference(H, W, dtype, layout):
    """__getitem__ (train: sampled + zero-padded; test: the whole bag) and collate([0, 2, 1]) against
    the restated JPGMILDataloader on the CPU over the same uint8 tiles, under the same seed."""
    from transmil_deepgraft_amd.data import ImageBagLoader, ImageBagStore
    bags, coords = random_bags(SIZES, H, W, seed=21)
    store = ImageBagStore(bags, coords, device=DEV)
    labels = [2, 0, 1]
    cl = torch.channels_last
    for mode in ("train", "test"):
        loader = ImageBagLoader(store, labels, mode, 3, max_bag_size=8, dtype=dtype, layout=layout,
                                wsi_names=["a", "b", "c"], patients=["pa", "pb", "pc"])
        for i, n in enumerate(SIZES):
            torch.manual_seed(40 + i)
            want, want_coords = getitem(bags[i], coords[i], mode, 8)
            torch.manual_seed(40 + i)
            tiles, label, (name, got_coords, patient) = loader[i]
            assert tiles.shape == want.shape and tiles.dtype == dtype and tiles.is_cuda
            assert tiles.is_contiguous(memory_format=cl) if layout == "nhwc" and n else tiles.is_contiguous()
            assert torch.equal(tiles.cpu(), want.to(dtype))
            if mode == "train" and n < 8:
                assert not bool(tiles[n:].any())                       # pad tiles are exactly 0
            assert torch.equal(got_coords, want_coords) and got_coords.dtype == torch.int64
            assert (label, name, patient) == (labels[i], "abc"[i], "p" + "abc"[i])
    loader = ImageBagLoader(store, labels, "val", 3, max_bag_size=8, dtype=dtype, layout=layout)
    order = [0, 2, 1]
    torch.manual_seed(9)
    ref = [getitem(bags[i], coords[i], "val", 8) for i in order]
    torch.manual_seed(9)
    tiles, lab, (names, got_coords, patients) = loader.collate(order)
    assert tiles.shape == (3, 8, 3, H, W)
    assert torch.equal(tiles.cpu(), torch.stack([r[0] for r in ref]).to(dtype))
    assert lab.dtype == torch.int64 and lab.tolist() == [2, 1, 0]
    assert all(torch.equal(a, r[1]) for a, r in zip(got_coords, ref))
    assert names == ["bag0", "bag2", "bag1"] and patients == names


def _lazy_bag(n, H, W, seed=5):
    """A lazy [1, n, 3, H, W] TileBag over a one-bag store (test mode: the whole bag, in order)."""
    from transmil_deepgraft_amd.data import ImageBagLoader, ImageBagStore
    bags, coords = random_bags([n], H, W, seed=seed)
    loader = ImageBagLoader(ImageBagStore(bags, coords, device=DEV), [1], "test", 2, lazy=True)
    return loader[0][0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_simple_cnn_on_a_lazy_bag(dtype):
    from simple_cnn_ref import deterministic_simple_params_
    from transmil_deepgraft_amd.encoder import simple_cnn
    enc = deterministic_simple_params_(simple_cnn(width=64, chunk=2), 3).set_compute_dtype(dtype).eval().cuda()
    bag = _lazy_bag(5, 224, 224)
    assert bag.shape == (1, 5, 3, 224, 224)
    lazy = enc(bag)
    assert (bag.launches, bag.max_launch_tiles) == (3, 2)             # chunks of 2, 2, 1 tiles
    resident = bag.materialize(dtype)
    assert resident.shape == (1, 5, 3, 224, 224) and resident.dtype == dtype
    assert (bag.launches, bag.max_launch_tiles) == (4, 5)
    assert torch.equal(lazy, enc(resident[0]))
    assert torch.equal(lazy, enc(bag.materialize(torch.float32)[0]))  # the fp32 batch the task hands over


def _resnet18(chunk):
    from resnet18_ref import deterministic_resnet18_params_
    from transmil_deepgraft_amd.encoder import resnet18
    return deterministic_resnet18_params_(resnet18(chunk=chunk), 2021).set_compute_dtype(torch.bfloat16).cuda()


def test_resnet18_eval_on_a_lazy_bag():
    enc = _resnet18(2).eval()
    bag = _lazy_bag(5, 72, 88)
    with torch.no_grad():
        lazy = enc(bag)
        assert (bag.launches, bag.max_launch_tiles) == (3, 2)
        assert torch.equal(lazy, enc(bag.materialize(torch.bfloat16)[0]))


def test_resnet18_train_on_a_lazy_bag():
    """Train mode needs every tile for the whole-bag statistics: ONE gather of all 4 tiles in the
    compute dtype; features and updated running statistics equal the resident run's."""
    a = _resnet18(2).train()
    b = copy.deepcopy(a)
    bag = _lazy_bag(4, 72, 88)
    with torch.no_grad():
        lazy = a(bag)
        assert (bag.launches, bag.max_launch_tiles) == (1, 4)
        assert torch.equal(lazy, b(bag.materialize(torch.bfloat16)[0]))
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert int(sa["bn1.num_batches_tracked"]) == 1


def test_task_steps_on_a_lazy_batch():
    """TransMILTask(ImageBagModel(simple_cnn(), AttMIL(2, 1024))): validation_step on a lazy batch
    records what it records for the materialised tensor batch; training_step returns a finite loss
    and backward fills the MIL model's gradients."""
    from transmil_deepgraft_amd.data import ImageBagLoader, ImageBagStore
    from transmil_deepgraft_amd.encoder import ImageBagModel, simple_cnn
    from transmil_deepgraft_amd.interface import TransMILTask
    from transmil_deepgraft_amd.models import AttMIL
    torch.manual_seed(0)
    model = ImageBagModel(simple_cnn(chunk=2), AttMIL(2, 1024)).cuda().eval()
    bags, coords = random_bags([3], 224, 224, seed=8)
    loader = ImageBagLoader(ImageBagStore(bags, coords, device=DEV), [1], "val", 2, max_bag_size=4, lazy=True,
                            wsi_names=["slide0"], patients=["patient0"])
    torch.manual_seed(1)
    bag, label, meta = loader.collate([0])                              # 3 tiles + 1 pad tile
    assert bag.shape == (1, 4, 3, 224, 224) and int(bag.idx[0, 3]) == -1
    lazy_task, tensor_task = TransMILTask(model), TransMILTask(model)
    got = lazy_task.validation_step((bag, label, meta))
    assert bag.max_launch_tiles == 2                                    # never the whole bag
    want = tensor_task.validation_step((bag.materialize(torch.float32), label, meta))
    assert got.shape == (1, 2) and torch.equal(got, want)
    a, b = lazy_task.eval_state("val"), tensor_task.eval_state("val")
    assert a.record.n == b.record.n == 1 and a.names == b.names == ["slide0"] and a.patients == b.patients == ["patient0"]
    for f in ("logits", "prob", "y_hat", "label", "nll", "class_stats", "cursor"):
        x, y = getattr(a.record, f), getattr(b.record, f)
        assert torch.equal(x[:1], y[:1]) if f not in ("class_stats", "cursor") else torch.equal(x, y), f

    model.train()
    loss = lazy_task.training_step((bag, label.cuda(), None))
    assert torch.isfinite(loss).all()
    lazy_task.backward(loss)
    grads = [p.grad for n, p in model.model.named_parameters() if not n.startswith("feature_extractor_part2.")]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    assert all(p.grad is None for p in model.model_ft.parameters())
