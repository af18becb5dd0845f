"""Plain fp64 PyTorch restatements of the folded PPEG stencil, forward and backward, as ppeg.hip
receives its operands (helpers of test_ppeg_kernels_gpu.py; test_ppeg_refs_cpu.py checks them against
the oracle PPEG under fp64 autograd).  Each returns, next to its values, the MAGNITUDE TWIN: the same
sums over the absolute values of the operands, which the element-wise rounding bounds of the GPU
tests are multiples of.  No library code is imported.  Not a conftest: imported by name."""
import torch
import torch.nn.functional as F


def _padded_grid(t, G):
    """Rows 1.. of t [B, 1 + G*G, D] as the zero-padded grid [B, G + 6, G + 6, D] (token 1 + r*G + c
    at cell (r + 3, c + 3))."""
    B, S, D = t.shape
    assert S == 1 + G * G
    return F.pad(t[:, 1:].reshape(B, G, G, D), (0, 0, 3, 3, 3, 3))


def _stencil(gp, w, G):
    """out[b][r][c][ch] = sum_{i,j} w[i*7 + j][ch] gp[b][r + i][c + j][ch]: the 7x7 depthwise
    cross-correlation of the zero-padded grid gp with the tap-major taps w [49, D]."""
    out = torch.zeros(gp.shape[0], G, G, gp.shape[3], dtype=torch.float64)
    for i in range(7):
        for j in range(7):
            out += w[i * 7 + j] * gp[:, i:i + G, j:j + G]
    return out


def _fwd(x, wf, bf, G):
    B, S, D = x.shape
    y = torch.empty_like(x)
    y[:, 0] = x[:, 0]
    y[:, 1:] = (_stencil(_padded_grid(x, G), wf, G) + bf).reshape(B, G * G, D)
    return y


def ppeg_fwd_ref(x, wf, bf, G):
    """tm_ppeg_fwd in fp64: x [B, 1 + G*G, D], wf [49, D] tap-major, bf [D] -> (y, mag).  Row 0 is
    copied; token 1 + r*G + c gets sum_{i,j} wf[i*7+j] x[r+i-3][c+j-3] + bf, cells outside the grid
    reading zero.  mag is the same over absolute values, sum |wf| |x| + |bf| (row 0: |x|)."""
    x, wf, bf = x.double(), wf.double(), bf.double()
    return _fwd(x, wf, bf, G), _fwd(x.abs(), wf.abs(), bf.abs(), G)


def _bwd(x, dy, wf, G):
    B, S, D = x.shape
    dx = torch.empty_like(dy)
    dx[:, 0] = dy[:, 0]
    dx[:, 1:] = _stencil(_padded_grid(dy, G), wf.flip(0), G).reshape(B, G * G, D)
    xp, g = _padded_grid(x, G), dy[:, 1:].reshape(B, G, G, D)
    dw7 = torch.stack([(g * xp[:, i:i + G, j:j + G]).sum((0, 1, 2)) for i in range(7) for j in range(7)], 1)
    k = dw7.view(D, 7, 7)
    return (dx, dw7, k[:, 1:6, 1:6].reshape(D, 25).clone(), k[:, 2:5, 2:5].reshape(D, 9).clone(),
            g.sum((0, 1, 2)))


def ppeg_bwd_ref(x, dy, wf, G):
    """tm_ppeg_bwd in fp64 -> ((dx, dw7 [D, 49], dw5 [D, 25], dw3 [D, 9], db [D]), mags).
    dx: row 0 copied, token 1 + r*G + c gets sum_{i,j} wf[48 - (i*7+j)] dy[r+i-3][c+j-3] (the flipped
    taps, no bias); dw7[ch][i*7+j] = sum_{b,r,c} dy[b][r][c] x[b][r+i-3][c+j-3] (the gradient of the
    folded 7x7 kernel, which is also that of proj.weight); dw5 / dw3 its centre 5x5 / 3x3 (the fold
    is a sum); db = sum of dy over the grid cells (the gradient of each of the three biases).  mags:
    the same five over absolute values, sum |wf| |dy|, sum |dy| |x| (and its centres), sum |dy|."""
    x, dy, wf = x.double(), dy.double(), wf.double()
    return _bwd(x, dy, wf, G), _bwd(x.abs(), dy.abs(), wf.abs(), G)
