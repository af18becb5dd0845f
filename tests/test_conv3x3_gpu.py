"""The hand-written 3x3 implicit-GEMM convolution (csrc/conv3x3.hip, tm_conv3x3) on the MI355X:
exact placement (one-hot weights, integer operands), fp64 references with derived bounds in both
compute modes, bitwise reproducibility and 64-bit addressing.

Shapes: every (n, h, wd) x (cin, cout) x stride of the grid below -- a single pixel, extents below
the patch width, odd extents under stride 2 (the (h - 1) / 2 + 1 edge), more than one patch per row
(56 = 7 patches of 8 columns), every patch width the kernel picks (8, 16, 32) and 1 / 2 / 8 channel
tiles with 1 / 2 / 4 k slices per tap row."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 2, 3), (3, 7, 7), (2, 9, 13), (1, 14, 14), (1, 56, 56)]
CHANNELS = [(64, 64), (64, 128), (128, 64), (256, 512)]
STRIDES = [1, 2]
EPILOGUES = ["none", "bias", "bias_relu", "bias_res_relu"]
MODES = [torch.float32, torch.bfloat16]
GRID = [(s, c, st) for s in SHAPES for c in CHANNELS for st in STRIDES]
IDS = [f"n{s[0]}_{s[1]}x{s[2]}_c{c[0]}to{c[1]}_s{st}" for s, c, st in GRID]


def _seed(shape, ch, stride):
    return hash((shape, ch, stride)) % (2 ** 31)


def _run(x, w, bias, res, stride, relu):
    """x [n, cin, h, wd], w [cout, cin, 3, 3], res [n, cout, ho, wo] CPU tensors of one dtype ->
    the kernel's output [n, cout, ho, wo] on the CPU."""
    from transmil_deepgraft_amd.encoder import _conv3x3
    cl = torch.channels_last
    y = _conv3x3(x.cuda().contiguous(memory_format=cl), w.cuda().contiguous(memory_format=cl),
                 bias.cuda() if bias is not None else None, stride, relu,
                 res.cuda().contiguous(memory_format=cl) if res is not None else None)
    torch.cuda.synchronize()
    return y.cpu()


def _out_hw(h, wd, stride):
    return (h - 1) // stride + 1, (wd - 1) // stride + 1


# ----------------------------------------------------------------------------- exact placement
def _one_hot(cin, cout):
    """w[co, tap = co mod 9, ci = (7 co + 3) mod cin] = 1: an asymmetric map, so a swapped tap,
    row / column or channel index cannot pass."""
    w = torch.zeros(cout, cin, 3, 3)
    co = torch.arange(cout)
    tap = co % 9
    w[co, (7 * co + 3) % cin, tap // 3, tap % 3] = 1.0
    return w


def _gather(x, cin, cout, stride):
    """The shifted, strided, zero-padded gather the one-hot convolution must equal."""
    n, _, h, wd = x.shape
    ho, wo = _out_hw(h, wd, stride)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(n, cout, ho, wo, dtype=x.dtype)
    for co in range(cout):
        ky, kx = (co % 9) // 3, (co % 9) % 3
        out[:, co] = xp[:, (7 * co + 3) % cin, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
    return out


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,ch,stride", GRID, ids=IDS)
def test_one_hot_placement_is_bitwise(shape, ch, stride, dtype):
    g = torch.Generator().manual_seed(_seed(shape, ch, stride))
    n, h, wd = shape
    x = torch.randn(n, ch[0], h, wd, generator=g).bfloat16().float()   # bf16-representable
    got = _run(x.to(dtype), _one_hot(*ch).to(dtype), None, None, stride, False)
    assert torch.equal(got.float(), _gather(x, ch[0], ch[1], stride))


@pytest.mark.parametrize("shape,ch,stride", GRID, ids=IDS)
def test_f32_small_integers_are_bitwise(shape, ch, stride):
    """x in [-3, 3], dense w in [-2, 2]: every partial sum is an integer below 2^24 (at most
    3 * 2 * 9 * 256 = 13824), so any summation order gives the integer convolution exactly."""
    g = torch.Generator().manual_seed(_seed(shape, ch, stride) + 1)
    n, h, wd = shape
    x = torch.randint(-3, 4, (n, ch[0], h, wd), generator=g).float()
    w = torch.randint(-2, 3, (ch[1], ch[0], 3, 3), generator=g).float()
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    got = _run(x, w, None, None, stride, False)
    assert torch.equal(got.double(), ref)


# ----------------------------------------------------------------------------- random operands
@functools.lru_cache(maxsize=2)
def _operands(shape, ch, stride):
    """fp32 random operands of one grid point (shared by both modes and the four epilogues)."""
    g = torch.Generator().manual_seed(_seed(shape, ch, stride) + 2)
    n, h, wd = shape
    ho, wo = _out_hw(h, wd, stride)
    x = torch.randn(n, ch[0], h, wd, generator=g)
    w = torch.randn(ch[1], ch[0], 3, 3, generator=g) * (9 * ch[0]) ** -0.5
    b = torch.randn(ch[1], generator=g)
    r = torch.randn(n, ch[1], ho, wo, generator=g)
    return x, w, b, r


def _epilogue(conv, b, r, epi):
    out = conv
    if epi != "none":
        out = out + b[None, :, None, None]
    if epi == "bias_res_relu":
        out = out + r
    return out.relu() if epi.endswith("relu") else out


@pytest.mark.parametrize("shape,ch,stride", GRID, ids=IDS)
def test_f32_random_against_fp64(shape, ch, stride):
    """TM_F32: the error against the fp64 convolution of the same fp32 operands, relative to the
    largest output magnitude, within 4 x the error of torch's own fp32 F.conv2d on the CPU against
    the same fp64 reference (the rule for kernels without a prior bound)."""
    x, w, b, r = _operands(shape, ch, stride)
    conv64 = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    conv32 = F.conv2d(x, w, stride=stride, padding=1)
    for epi in EPILOGUES:
        ref = _epilogue(conv64, b.double(), r.double(), epi)
        cpu = _epilogue(conv32, b, r, epi)
        got = _run(x, w, b if epi != "none" else None, r if epi == "bias_res_relu" else None, stride,
                   epi.endswith("relu"))
        scale = ref.abs().max()
        bound = 4 * (cpu.double() - ref).abs().max() / scale
        err = (got.double() - ref).abs().max() / scale
        print(f"conv3x3 f32 {shape} {ch} s{stride} {epi}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (epi, float(err), float(bound))


@pytest.mark.parametrize("shape,ch,stride", GRID, ids=IDS)
def test_bf16_random_against_fp64(shape, ch, stride):
    """TM_BF16 against the fp64 convolution of the bf16-rounded operands, elementwise:
    |err| <= 2^-8 |ref| + (9 cin + 2) 2^-24 A,  A = conv(|x|, |w|) + |bias| + |residual|
    (one bf16 output rounding with a 2 x margin + fp32 accumulation in any order)."""
    x, w, b, r = (t.bfloat16() for t in _operands(shape, ch, stride))
    xd, wd_, bd, rd = x.double(), w.double(), b.double(), r.double()
    conv64 = F.conv2d(xd, wd_, stride=stride, padding=1)
    conva = F.conv2d(xd.abs(), wd_.abs(), stride=stride, padding=1)
    for epi in EPILOGUES:
        ref = _epilogue(conv64, bd, rd, epi)
        A = conva + (bd.abs()[None, :, None, None] if epi != "none" else 0) + (rd.abs() if epi == "bias_res_relu" else 0)
        got = _run(x, w, b if epi != "none" else None, r if epi == "bias_res_relu" else None, stride,
                   epi.endswith("relu"))
        err = (got.double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + (9 * ch[0] + 2) * 2.0 ** -24 * A
        print(f"conv3x3 bf16 {shape} {ch} s{stride} {epi}: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (epi, float((err - bound).max()))


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16"])
def test_two_launches_are_bitwise_equal(dtype):
    x, w, b, r = (t.to(dtype) for t in _operands((2, 9, 13), (128, 64), 1))
    a = _run(x, w, b, r, 1, True)
    c = _run(x, w, b, r, 1, True)
    assert torch.equal(a, c)


# ----------------------------------------------------------------------------- large offsets
def _tile_pair():
    g = torch.Generator().manual_seed(9)
    tiles = torch.randn(2, 56, 56, 64, generator=g)                 # [n, h, w, c]: channels-last memory
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).contiguous(memory_format=torch.channels_last)
    return tiles, w


def _call(x, w, y, n):
    from transmil_deepgraft_amd import _lib
    from transmil_deepgraft_amd.engine import _p, _stream
    _lib.call("tm_conv3x3", _lib.F32, _p(x), _p(w), None, None, _p(y), n, 56, 56, 64, 64, 1, 0, _stream())
    torch.cuda.synchronize()


def test_operands_placed_more_than_2_31_bytes_apart():
    """n = 40, 56 x 56, 64 -> 64, x and y views of one slab with y's last tile more than 2^31 bytes
    past x's first: first and last tile equal the 1-tile result."""
    tiles, w = _tile_pair()
    w = w.cuda()
    tile = 56 * 56 * 64
    slab = torch.empty(2 ** 29 + 80 * tile, dtype=torch.float32, device="cuda")   # 2 GiB + both operands
    x = slab[:40 * tile].view(40, 56, 56, 64)
    y = slab[2 ** 29 + 40 * tile:].view(40, 56, 56, 64)
    assert y[39].data_ptr() - x[0].data_ptr() > 2 ** 31
    x.zero_()
    x[0].copy_(tiles[0])
    x[39].copy_(tiles[1])
    small = torch.empty(2, 56, 56, 64, device="cuda")
    _call(tiles.cuda(), w, small, 2)
    _call(x, w, y, 40)
    assert torch.equal(y[0], small[0]) and torch.equal(y[39], small[1])
    assert not bool(y[1:39].any())


def test_offsets_past_2_31_bytes_inside_one_tensor():
    """n = 2688 tiles of 56 x 56 x 64 fp32 are 2.16 GB per tensor: the last tile's elements lie
    more than 2^31 bytes past the tensor's base (the 64-bit addressing the n = 40 case cannot reach:
    40 tiles are 32 MB).  First and last tile equal the 1-tile result."""
    tiles, w = _tile_pair()
    w = w.cuda()
    n = 2688
    assert (n - 1) * 56 * 56 * 64 * 4 > 2 ** 31
    x = torch.zeros(n, 56, 56, 64, device="cuda")
    y = torch.empty(n, 56, 56, 64, device="cuda")
    x[0].copy_(tiles[0])
    x[n - 1].copy_(tiles[1])
    small = torch.empty(2, 56, 56, 64, device="cuda")
    _call(tiles.cuda(), w, small, 2)
    _call(x, w, y, n)
    assert torch.equal(y[0], small[0]) and torch.equal(y[n - 1], small[1])
    assert not bool(y[n // 2].any())
