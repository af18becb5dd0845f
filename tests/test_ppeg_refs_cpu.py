"""tests/ppeg_refs.py against the oracle PPEG under fp64 autograd, and the status path of
tm_ppeg_fwd / tm_ppeg_bwd / tm_dropout_bwd_pad / tm_pad_rows (no GPU: every call is refused before
anything is launched)."""
import ctypes as C

import pytest
import torch

import ppeg_refs as P
import tail_refs as T

BOUND = 1e-12          # absolute


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _worst(a, b):
    return (a.double() - b.double()).abs().max().item()


@pytest.mark.parametrize("B,G,D", [(2, 1, 32), (3, 9, 96), (2, 25, 32)])
def test_ppeg_refs_are_the_oracle_ppeg_and_its_autograd(B, G, D):
    """Random proj / proj1 / proj2 weights folded with tail_refs.ppeg_fold_ref: ppeg_fwd_ref is the
    oracle module's output, ppeg_bwd_ref its fp64 autograd (dx, the three weight gradients, the three
    bias gradients), all within 1e-12 absolute (a probe of this comparison gave at most 1.8e-13).  The
    magnitude twins are the references themselves on the absolute values of the operands and bound
    the values element by element."""
    from oracle.transmil_ref import PPEG
    g = _gen(B * 1000 + G * 10 + D)
    ref = PPEG(D).double()
    with torch.no_grad():
        for conv in (ref.proj, ref.proj1, ref.proj2):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64) * 0.2)
            conv.bias.copy_(torch.randn(D, generator=g, dtype=torch.float64) * 0.1)
    x = torch.randn(B, 1 + G * G, D, generator=g, dtype=torch.float64)
    dy = torch.randn(B, 1 + G * G, D, generator=g, dtype=torch.float64)
    wf, bf = T.ppeg_fold_ref(ref.proj.weight.detach(), ref.proj.bias.detach(), ref.proj1.weight.detach(),
                             ref.proj1.bias.detach(), ref.proj2.weight.detach(), ref.proj2.bias.detach())
    xr = x.clone().requires_grad_()
    want = ref(xr, G, G)
    params = [ref.proj.weight, ref.proj1.weight, ref.proj2.weight, ref.proj.bias, ref.proj1.bias, ref.proj2.bias]
    gx, g7, g5, g3, gb7, gb5, gb3 = torch.autograd.grad(want, [xr] + params, dy)
    y, ymag = P.ppeg_fwd_ref(x, wf, bf, G)
    (dx, dw7, dw5, dw3, db), mags = P.ppeg_bwd_ref(x, dy, wf, G)
    assert y.shape == x.shape and dx.shape == x.shape
    assert dw7.shape == (D, 49) and dw5.shape == (D, 25) and dw3.shape == (D, 9) and db.shape == (D,)
    errs = {"y": _worst(y, want.detach()), "dx": _worst(dx, gx), "dw7": _worst(dw7, g7.reshape(D, 49)),
            "dw5": _worst(dw5, g5.reshape(D, 25)), "dw3": _worst(dw3, g3.reshape(D, 9)),
            "db7": _worst(db, gb7), "db5": _worst(db, gb5), "db3": _worst(db, gb3)}
    print(f"[measured] ppeg refs against the oracle {B, G, D}: {errs}")
    assert all(e <= BOUND for e in errs.values()), errs
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(dx[:, 0], dy[:, 0])
    # the twins: the same functions of the magnitudes, never below the values
    assert torch.equal(ymag, P.ppeg_fwd_ref(x.abs(), wf.abs(), bf.abs(), G)[0])
    for m, v, m2 in zip(mags, (dx, dw7, dw5, dw3, db), P.ppeg_bwd_ref(x.abs(), dy.abs(), wf.abs(), G)[0]):
        assert torch.equal(m, m2) and (m >= v.abs() - 1e-12).all()
    assert (ymag >= y.abs() - 1e-12).all()
    if G == 1:      # one cell: only the centre tap meets data
        off = torch.ones(49, dtype=torch.bool)
        off[24] = False
        assert (mags[1][:, off] == 0).all() and (mags[1][:, 24] > 0).all()


def test_ppeg_refs_on_a_hand_computed_grid():
    """G = 2, D = 1, taps w[i*7+j] = i*7+j: token (r, c) reads x[r'][c'] through tap
    (r' - r + 3, c' - c + 3), the backward through the mirrored tap."""
    G = 2
    x = torch.tensor([5.0, 1.0, 2.0, 3.0, 4.0]).view(1, 5, 1)
    wf = torch.arange(49, dtype=torch.float64).view(49, 1)
    bf = torch.tensor([0.5])
    y, _ = P.ppeg_fwd_ref(x, wf, bf, G)
    # token (0, 0): x00 w[3][3] + x01 w[3][4] + x10 w[4][3] + x11 w[4][4]
    assert y[0, 1, 0].item() == 1 * 24 + 2 * 25 + 3 * 31 + 4 * 32 + 0.5
    # token (1, 1): x00 w[2][2] + x01 w[2][3] + x10 w[3][2] + x11 w[3][3]
    assert y[0, 4, 0].item() == 1 * 16 + 2 * 17 + 3 * 23 + 4 * 24 + 0.5
    assert y[0, 0, 0].item() == 5.0
    (dx, dw7, dw5, dw3, db), _ = P.ppeg_bwd_ref(x, x, wf, G)
    # dx(0, 0) = sum over outputs (r, c) of dy[r][c] w[3 - r][3 - c]
    assert dx[0, 1, 0].item() == 1 * 24 + 2 * 23 + 3 * 17 + 4 * 16
    assert dx[0, 0, 0].item() == 5.0
    # dw[3][4] = sum_{r,c} dy[r][c] x[r][c + 1] = 1*2 + 3*4
    assert dw7[0, 25].item() == 14.0 and dw5[0, 2 * 5 + 3].item() == 14.0 and dw3[0, 1 * 3 + 2].item() == 14.0
    assert dw7[0, 24].item() == 30.0 and dw7[0, 0].item() == 0.0
    assert db[0].item() == 10.0


def test_ppeg_entry_points_refuse_bad_arguments():
    """A status path: every call below is refused by a guard, so nothing is launched (the pointers are
    made-up addresses that are never dereferenced).  The shape checks come before the pointer checks."""
    from transmil_deepgraft_amd import _lib
    lib = _lib.lib()
    N = None
    A = {k: 0x100000 + 0x1000 * i for i, k in enumerate(
        ("x", "y", "wfold", "bfold", "dy", "dx", "work", "dw7", "db7", "dw5", "db5", "dw3", "db3", "dout"))}

    def fwd(B=2, G=9, D=96, **over):
        a = {**A, **over}
        return lib.tm_ppeg_fwd(a["x"], B, G, D, a["wfold"], a["bfold"], a["y"], N)

    def bwd(B=2, G=9, D=96, dtype=0, n_pad=0, pad=0, **over):
        a = {**A, "dout": N, **over}
        return lib.tm_ppeg_bwd(a["x"], a["dy"], B, G, D, a["wfold"], a["dx"], a["work"], a["dw7"], a["db7"], a["dw5"],
                               a["db5"], a["dw3"], a["db3"], dtype, a["dout"], n_pad, pad, C.c_float(0.7), 5, N, N, N)

    f_align = "ppeg_fwd: x, y, wfold, bfold must be 16-byte aligned"
    b_align = "ppeg_bwd: x, dy, dx, wfold, work, dout must be 16-byte aligned"
    big = "(1+G*G)*D*4 must be < 2^32 bytes per bag"
    cases = [
        # shapes, with and without pointers
        (lambda: fwd(D=48), "ppeg_fwd: bad shape"), (lambda: fwd(D=0), "ppeg_fwd: bad shape"),
        (lambda: fwd(D=-32), "ppeg_fwd: bad shape"), (lambda: fwd(G=0), "ppeg_fwd: bad shape"),
        (lambda: fwd(G=-3), "ppeg_fwd: bad shape"), (lambda: fwd(B=0), "ppeg_fwd: bad shape"),
        (lambda: fwd(D=48, x=N, y=N, wfold=N, bfold=N), "ppeg_fwd: bad shape"),
        (lambda: bwd(D=48), "ppeg_bwd: bad shape"), (lambda: bwd(D=0), "ppeg_bwd: bad shape"),
        (lambda: bwd(G=0), "ppeg_bwd: bad shape"), (lambda: bwd(G=-3), "ppeg_bwd: bad shape"),
        (lambda: bwd(B=0), "ppeg_bwd: bad shape"), (lambda: bwd(B=-1, x=N, dy=N, dx=N), "ppeg_bwd: bad shape"),
        # a bag past the 32-bit byte offsets of the buffer loads
        (lambda: fwd(G=1024, D=1024), "ppeg_fwd: " + big), (lambda: bwd(G=1024, D=1024), "ppeg_bwd: " + big),
        (lambda: fwd(G=5793, D=32), "ppeg_fwd: " + big),
        # the fused dropout-pad output
        (lambda: bwd(dout=A["dout"], n_pad=81, pad=0), "ppeg_bwd: bad dropout-pad output"),
        (lambda: bwd(dout=A["dout"], n_pad=90, pad=9), "ppeg_bwd: bad dropout-pad output"),
        (lambda: bwd(dout=A["dout"], n_pad=90, pad=-1), "ppeg_bwd: bad dropout-pad output"),
        (lambda: bwd(dout=A["dout"], n_pad=90, pad=3, dtype=2), "ppeg_bwd: bad dropout-pad output"),
        # null pointers
        (lambda: fwd(x=N), "ppeg_fwd: null arg"), (lambda: fwd(y=N), "ppeg_fwd: null arg"),
        (lambda: fwd(wfold=N), "ppeg_fwd: null arg"), (lambda: fwd(bfold=N), "ppeg_fwd: null arg"),
        (lambda: bwd(x=N), "ppeg_bwd: null arg"), (lambda: bwd(dy=N), "ppeg_bwd: null arg"),
        (lambda: bwd(dx=N), "ppeg_bwd: null arg"), (lambda: bwd(wfold=N), "ppeg_bwd: null arg"),
        (lambda: bwd(work=N), "ppeg_bwd: null arg"),
        (lambda: bwd(dw7=N), "ppeg_bwd: null gradient"), (lambda: bwd(db7=N), "ppeg_bwd: null gradient"),
        (lambda: bwd(dw5=N), "ppeg_bwd: null gradient"), (lambda: bwd(db5=N), "ppeg_bwd: null gradient"),
        (lambda: bwd(dw3=N), "ppeg_bwd: null gradient"), (lambda: bwd(db3=N), "ppeg_bwd: null gradient"),
        # aliasing
        (lambda: fwd(y=A["x"]), "ppeg_fwd: y must not alias x"),
        (lambda: bwd(dx=A["x"]), "ppeg_bwd: dx must alias neither dy nor x"),
        (lambda: bwd(dx=A["dy"]), "ppeg_bwd: dx must alias neither dy nor x"),
        # 16-byte alignment of everything moved in 16-byte pieces
        (lambda: fwd(x=A["x"] + 4), f_align), (lambda: fwd(y=A["y"] + 8), f_align),
        (lambda: fwd(wfold=A["wfold"] + 4), f_align), (lambda: fwd(bfold=A["bfold"] + 12), f_align),
        (lambda: bwd(x=A["x"] + 4), b_align), (lambda: bwd(dy=A["dy"] + 8), b_align),
        (lambda: bwd(dx=A["dx"] + 4), b_align), (lambda: bwd(wfold=A["wfold"] + 4), b_align),
        (lambda: bwd(work=A["work"] + 4), b_align),
        (lambda: bwd(dout=A["dout"] + 8, n_pad=90, pad=3, dtype=1), b_align),
        # the padded layouts of glue.hip
        (lambda: lib.tm_dropout_bwd_pad(0, N, 2, 7, 11, 5, 64, C.c_float(0.7), 5, N, N, N),
         "dropout_bwd_pad: n_pad < S + pad"),
        (lambda: lib.tm_pad_rows(0, N, 2, 7, 11, 5, 64, N, N), "pad_rows: n_pad < S + pad"),
    ]
    for i, (fn, text) in enumerate(cases):
        rc = fn()
        assert rc != 0 and _lib.last_error() == text, (i, rc, text, _lib.last_error())
