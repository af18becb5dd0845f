"""The model-independent fp32 row passes on the MI355X, through the C ABI: ``tm_relu`` / ``tm_relu_bwd``
(glue.hip) and ``tm_scatter_rows`` (bags.hip), each bit for bit against torch on the same tensors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.5


def _call(name, *args):
    from transmil_deepgraft_amd import _lib
    from transmil_deepgraft_amd.engine import _p, _stream
    _lib.call(name, *(_p(a) if isinstance(a, torch.Tensor) else a for a in args), _stream())
    torch.cuda.synchronize()


def _values(count, seed):
    """Both signs and exact zeros, the zeros at both ends and inside."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.randn(count, generator=g)
    v[::3] = 0.0
    v[-1] = 0.0
    v[1], v[2] = 1.5, -0.25
    return v.to(DEV)


@pytest.mark.parametrize("count", [4, 1028])      # 1028: one element group past the 1024-element block
def test_relu(count):
    h = _values(count, 1)
    ref = torch.relu(h)
    _call("tm_relu", h, count)
    assert torch.equal(h, ref)


@pytest.mark.parametrize("count", [4, 1028])
def test_relu_bwd(count):
    h, dh = _values(count, 2), _values(count, 3).flip(0)     # h > 0 meets non-zero dh, also at count 4
    ref = torch.where(h > 0, dh, torch.zeros_like(dh))
    h0 = h.clone()
    _call("tm_relu_bwd", dh, h, count)
    assert torch.equal(dh, ref)
    assert torch.equal(h, h0)


def test_relu_count_zero_is_a_noop():
    h, dh = _values(4, 4), _values(4, 5)
    h0, dh0 = h.clone(), dh.clone()
    _call("tm_relu", h, 0)
    _call("tm_relu_bwd", dh, h, 0)
    assert torch.equal(h, h0) and torch.equal(dh, dh0)


def test_relu_refuses_a_count_that_is_no_multiple_of_4():
    h, dh = _values(8, 6), _values(8, 7)
    h0, dh0 = h.clone(), dh.clone()
    with pytest.raises(RuntimeError, match=r"relu: count must be a multiple of 4"):
        _call("tm_relu", h, 6)
    with pytest.raises(RuntimeError, match=r"relu_bwd: count must be a multiple of 4"):
        _call("tm_relu_bwd", dh, h, 6)
    assert torch.equal(h, h0) and torch.equal(dh, dh0)


@pytest.mark.parametrize("F", [8, 6])             # 8: the 16-byte path, 6: the scalar path
def test_scatter_rows(F):
    nrows, N = 4, 5
    idx = torch.tensor([3, -1, 0, 5], dtype=torch.int64, device=DEV)      # -1 and 5 (= N) are skipped
    g = torch.Generator(device="cpu").manual_seed(8)
    src = torch.randn(nrows, F, generator=g).to(DEV)
    dst = torch.full((N, F), SENTINEL, device=DEV)
    ref = dst.clone()
    keep = (idx >= 0) & (idx < N)
    ref[idx[keep]] = src[keep]
    _call("tm_scatter_rows", src, idx, nrows, F, N, dst)
    assert torch.equal(dst, ref)
    assert torch.equal(dst[[1, 2, 4]], torch.full((3, F), SENTINEL, device=DEV))      # untouched rows
    assert torch.equal(dst[3], src[0]) and torch.equal(dst[0], src[2])


def test_scatter_rows_zero_rows_is_a_noop():
    idx = torch.tensor([3, -1, 0, 5], dtype=torch.int64, device=DEV)
    src = torch.ones(4, 8, device=DEV)
    dst = torch.full((5, 8), SENTINEL, device=DEV)
    _call("tm_scatter_rows", src, idx, 0, 8, 5, dst)
    assert torch.equal(dst, torch.full((5, 8), SENTINEL, device=DEV))
