"""Kernel-level checks on the MI355X of ppeg.hip: tm_ppeg_fwd and tm_ppeg_bwd (the dx stencil, the
weight gradient and the fused dropout-pad store of one launch), called through the C ABI as engine.py
calls them and compared with the fp64 restatements of tests/ppeg_refs.py on the same, already-rounded
operands -- exactly on small-integer data, within a-priori rounding bounds on normal data -- or bit
for bit with a second call / tm_dropout_bwd_pad.  Every output buffer is one row (or D floats) longer
than needed and prefilled with a NaN or 7.0 sentinel; every test prints the figures it then asserts
on (pytest -s shows them)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

import kernel_refs as R
import ppeg_refs as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = 7.0
U = 2.0 ** -24                                      # the unit roundoff of fp32
F32T, BF16T = torch.float32, torch.bfloat16
SEED, COUNTER = 0x5DEECE66D1234567, 3
GUARD = 256                                         # floats past the workspace

# (B, G, D): tiles are 8 x 8 cells x 32 channels, a weight-gradient workgroup walks WT = 3 tile columns
SHAPES = [
    (1, 1, 32),      # the 14 x 14 window is almost all halo; a single tile
    (3, 2, 96),      # G below the stencil radius: taps fall outside on both sides
    (2, 7, 64),      # one cell short of a tile
    (1, 8, 32),      # exactly one tile
    (3, 9, 96),      # a one-cell-wide second tile
    (2, 16, 32),     # two full tiles
    (1, 17, 64),     # three tile columns: exactly one weight-gradient group
    (2, 25, 32),     # four tile columns: the second group holds a single tile
    (3, 33, 96),     # 5 x 5 tiles, groups of 3 + 2, ragged last row and column
]                    # D = 32: one channel chunk; D = 96: three, so bx % nchunk is not a mask
GRADS = ("dw7", "db7", "dw5", "db5", "dw3", "db3")


def _lib():
    from transmil_deepgraft_amd import _lib
    return _lib


def _eng():
    from transmil_deepgraft_amd.engine import _p, _stream
    return _p, _stream


def _report(name, value):
    print(f"[measured] {name} = {value:.3e}" if isinstance(value, float) else f"[measured] {name} = {value}")


def _tt(dtype):
    from transmil_deepgraft_amd._lib import BF16, F32
    return BF16 if dtype == BF16T else F32


def _dev(*ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16T else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Queue:
    """A caller-owned tm_reduce_queue for one call (the engine's deferred form)."""

    def __enter__(self):
        self.h = C.c_void_p(_lib().lib().tm_reduce_queue_create())
        assert self.h
        return self

    def pending(self):
        return _lib().lib().tm_reduce_queue_pending(self.h)

    def flush(self):
        _, _stream = _eng()
        _lib().call("tm_reduce_flush", self.h, _stream())

    def __exit__(self, *exc):
        _lib().lib().tm_reduce_queue_destroy(self.h)
        return False


def _seed_args(use_ptr):
    """(seed_ptr tensor or None, the counter value dropout_keep takes)."""
    if use_ptr:
        return torch.tensor([COUNTER], dtype=torch.int64, device=DEV), COUNTER
    return None, 0


# ----------------------------------------------------------------------------- operands, references
@functools.lru_cache(maxsize=None)
def _case(B, G, D, integer):
    """Operands of one shape -- small integers (every product and partial sum exact in fp32) or
    normal data already rounded to fp32 -- and the fp64 references with their magnitude twins,
    computed once and shared (nothing below writes to them)."""
    g = _gen(B * 10000 + G * 100 + D + (1 if integer else 0))
    S = 1 + G * G
    if integer:
        x, dy = (torch.randint(-4, 5, (B, S, D), generator=g).float() for _ in range(2))
        wf = torch.randint(-4, 5, (49, D), generator=g).float()
        bf = torch.randint(-4, 5, (D,), generator=g).float()
    else:
        x, dy = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
        wf, bf = 0.3 * torch.randn(49, D, generator=g), 0.2 * torch.randn(D, generator=g)
    y, ymag = P.ppeg_fwd_ref(x, wf, bf, G)
    bwd, bmag = P.ppeg_bwd_ref(x, dy, wf, G)
    names = ("dx", "dw7", "dw5", "dw3", "db")
    return SimpleNamespace(B=B, G=G, D=D, S=S, x=x, dy=dy, wf=wf, bf=bf, y=y, ymag=ymag,
                           ref=dict(zip(names, bwd)), mag=dict(zip(names, bmag)))


# ----------------------------------------------------------------------------- launches
def _fwd(c):
    """tm_ppeg_fwd -> y [B, S, D] on the CPU; the extra row keeps the sentinel."""
    L = _lib()
    _p, _stream = _eng()
    xd, wfd, bfd = _dev(c.x, c.wf, c.bf)
    y = torch.full((c.B * c.S + 1, c.D), SENTINEL, device=DEV)
    L.call("tm_ppeg_fwd", _p(xd), c.B, c.G, c.D, _p(wfd), _p(bfd), _p(y), _stream())
    torch.cuda.synchronize()
    out = y.cpu()
    assert (out[-1] == SENTINEL).all()
    return out[:-1].view(c.B, c.S, c.D)


def _bwd_launch(c, drop=None, rq=None):
    """tm_ppeg_bwd with dx prefilled with 7 (one extra row), the six gradients with NaN (D extra
    floats each), the workspace with NaN and a guard tail of 7s.  drop = (dtype, n_pad, pad, p,
    use_ptr): the fused dropout-pad output [B, n_pad, D] plus one row, prefilled with 7.  Returns the
    device buffers; _bwd_collect checks the sentinels."""
    L = _lib()
    _p, _stream = _eng()
    B, G, D, S = c.B, c.G, c.D, c.S
    xd, dyd, wfd = _dev(c.x, c.dy, c.wf)
    nwork = L.query("tm_ppeg_bwd_workspace", B, G, D) // 4
    o = SimpleNamespace(c=c, nwork=nwork, keep=(xd, dyd, wfd), dout=None, drop=drop)
    o.work = torch.full((nwork + GUARD,), NAN, device=DEV)
    o.work[nwork:] = SENTINEL
    o.dx = torch.full((B * S + 1, D), SENTINEL, device=DEV)
    for name, k in (("dw7", 49), ("dw5", 25), ("dw3", 9), ("db7", 1), ("db5", 1), ("db3", 1)):
        setattr(o, name, torch.full((D * k + D,), NAN, device=DEV))
    dtype, n_pad, pad, p, sp = F32T, 0, 0, 0.0, None
    if drop is not None:
        dtype, n_pad, pad, p, use_ptr = drop
        sp, _ = _seed_args(use_ptr)
        o.dout = torch.full((B * n_pad + 1, D), SENTINEL, dtype=dtype, device=DEV)
        o.keep += (sp,)
    L.call("tm_ppeg_bwd", _p(xd), _p(dyd), B, G, D, _p(wfd), _p(o.dx), _p(o.work), _p(o.dw7), _p(o.db7), _p(o.dw5),
           _p(o.db5), _p(o.dw3), _p(o.db3), _tt(dtype), _p(o.dout), n_pad, pad, C.c_float(p), C.c_uint64(SEED), _p(sp),
           rq, _stream())
    return o


def _bwd_collect(o):
    """Synchronise; the guard tail of the workspace, the extra row of dx and the D extra floats of
    every gradient keep their sentinel, the workspace and the gradients themselves are finite
    (written, not accumulated into the NaN they held).  -> CPU tensors."""
    torch.cuda.synchronize()
    c = o.c
    D = c.D
    work = o.work.cpu()
    assert (work[o.nwork:] == SENTINEL).all() and torch.isfinite(work[:o.nwork]).all()
    dx = o.dx.cpu()
    assert (dx[-1] == SENTINEL).all()
    r = SimpleNamespace(dx=dx[:-1].view(c.B, c.S, D), dout=None if o.dout is None else o.dout.cpu())
    for name, k in (("dw7", 49), ("dw5", 25), ("dw3", 9), ("db7", 1), ("db5", 1), ("db3", 1)):
        t = getattr(o, name).cpu()
        assert torch.isnan(t[D * k:]).all() and torch.isfinite(t[:D * k]).all(), name
        setattr(r, name, t[:D * k].view(D, k) if k > 1 else t[:D])
    return r


def _bwd(c, drop=None):
    return _bwd_collect(_bwd_launch(c, drop))


def _centres(dw7, D):
    k = dw7.view(D, 7, 7)
    return k[:, 1:6, 1:6].reshape(D, 25), k[:, 2:5, 2:5].reshape(D, 9)


# ============================================================================= a. exact indexing
@pytest.mark.parametrize("B,G,D", SHAPES)
def test_ppeg_fwd_bwd_exact_on_small_integers(B, G, D):
    """x, dy, wf and bf are integers drawn from [-4, 4]: every product is an integer of magnitude at
    most 16 and every partial sum, in any order, is an integer no larger than the magnitude twin of
    its output, which the test first checks to be below 2^24 (the largest, a weight-gradient sum at
    (3, 33, 96), is 16703).  fp32 arithmetic is then exact whatever the summation order, so y, dx,
    dw7, dw5, dw3 and db7 = db5 = db3 must EQUAL the fp64 reference: no tolerance.  A dropped,
    duplicated or misplaced cell, tap, tile, weight-gradient group or channel chunk moves some output
    by at least 1.
    Measured on the MI355X: no entry differs at any of the nine shapes."""
    c = _case(B, G, D, True)
    largest = max(c.ymag.max().item(), *(m.max().item() for m in c.mag.values()))
    _report(f"exact: largest magnitude sum {B, G, D}", largest)
    assert largest < 2 ** 24
    y = _fwd(c)
    r = _bwd(c)
    got = {"y": y, "dx": r.dx, "dw7": r.dw7, "dw5": r.dw5, "dw3": r.dw3, "db7": r.db7, "db5": r.db5, "db3": r.db3}
    want = {"y": c.y, **c.ref, "db7": c.ref["db"], "db5": c.ref["db"], "db3": c.ref["db"]}
    wrong = {k: int((got[k].double() != want[k]).sum().item()) for k in got}
    _report(f"exact: entries that differ from fp64 {B, G, D}", wrong)
    for k in got:
        bad = (got[k].double() != want[k]).nonzero()
        assert bad.numel() == 0, (k, "first wrong index", bad[0].tolist(), "of", wrong[k])


# ============================================================================= b. rounding
def _ratio(got, ref, bound):
    """max |got - ref| / bound over the entries with a non-zero bound; where the bound (a multiple of
    the magnitude twin) is zero, every term of the sum is zero and the output must be exactly 0."""
    got = got.double()
    zero = bound == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    return ((got - ref).abs()[~zero] / bound[~zero]).max().item()


@pytest.mark.parametrize("B,G,D", SHAPES)
def test_ppeg_fwd_bwd_within_rounding_bounds_of_fp64(B, G, D):
    """x, dy = randn, wf = 0.3 randn, bf = 0.2 randn, rounded to fp32 before the reference sees them.
    Element by element, with u = 2^-24 and the magnitude twins of ppeg_refs:
      - |y - ref| <= 50 u (sum |wf||x| + |bf|) and |dx - ref| <= 49 u sum |wf||dy|: a chain of 49 FMAs
        (plus the bias) rounds once per step, each time by at most u times a partial sum that the
        magnitude sum bounds; row 0 of y is x row 0 and row 0 of dx is dy row 0, bitwise;
      - |dw7 - ref| <= B G^2 u sum |dy||x| and |db7 - ref| <= B G^2 u sum |dy|: a sum of n = B G^2 terms
        in any order; where the magnitude is 0 (no cell pair meets that tap: every off-centre tap at
        G = 1) the output is exactly 0;
      - dw5 / dw3 are bitwise the centre 5x5 / 3x3 of dw7, db5 and db3 bitwise db7.
    The bounds are derived, not measured: they hold for any summation order.  On the CPU, with torch's
    fp32 sums standing in for the kernel, the error was at most 0.13 of the forward bound and 0.005 of
    the weight-gradient bound, and one dropped centre term exceeded the weight-gradient bound 13-fold
    at (3, 33, 96) and 77-fold at (2, 25, 32).
    Measured on the MI355X, the worst error / bound per shape in the order of SHAPES:
      y    0.018 0.035 0.052 0.058 0.081 0.080 0.080 0.068 0.082
      dx   0.014 0.044 0.069 0.047 0.078 0.066 0.092 0.081 0.093
      dw7  0.88  0.15  0.014 0.023 0.0042 0.0011 0.0039 0.00036 0.000087
      db7  0     0.059 0.0051 0.011 0.0017 0.00042 0.0017 0.00016 0.000063
    (dw7 at (1, 1, 32) is ONE rounded product against u times its magnitude, so close to 1 by
    construction; db7 there is a single term, copied.)"""
    c = _case(B, G, D, False)
    y = _fwd(c)
    r = _bwd(c)
    n = B * G * G
    assert _same(y[:, 0], c.x[:, 0]) and _same(r.dx[:, 0], c.dy[:, 0])
    ratios = {"y": _ratio(y, c.y, 50 * U * c.ymag), "dx": _ratio(r.dx, c.ref["dx"], 49 * U * c.mag["dx"]),
              "dw7": _ratio(r.dw7, c.ref["dw7"], n * U * c.mag["dw7"]),
              "db7": _ratio(r.db7, c.ref["db"], n * U * c.mag["db"])}
    _report(f"rounding: worst error / bound {B, G, D}", ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if G == 1:
        off = torch.ones(49, dtype=torch.bool)
        off[24] = False
        assert (c.mag["dw7"][:, off] == 0).all() and (_bits(r.dw7[:, off]) == 0).all()
    c5, c3 = _centres(r.dw7, D)
    assert _same(r.dw5, c5) and _same(r.dw3, c3)
    assert _same(r.db5, r.db7) and _same(r.db3, r.db7)


# ============================================================================= c. written, repeatable
@pytest.mark.parametrize("B,G,D", SHAPES)
def test_ppeg_outputs_are_written_once_and_repeat_bitwise(B, G, D):
    """tm_ppeg_bwd_workspace(B, G, D) = 4 B ceil(G/8) ceil(ceil(G/8)/3) D 84 bytes; with the gradients
    and the workspace prefilled with NaN everything comes back finite (written, not accumulated), the
    guard tail past the workspace, the extra row of y / dx and the D extra floats of every gradient
    keep their sentinel (checked in _fwd / _bwd_collect), and a second identical call gives the same
    bits in every output: fixed-order sums, no atomics."""
    c = _case(B, G, D, False)
    nt = (G + 7) // 8
    want = 4 * B * nt * ((nt + 2) // 3) * D * 84
    got = _lib().query("tm_ppeg_bwd_workspace", B, G, D)
    _report(f"workspace bytes {B, G, D}", (got, want))
    assert got == want
    y1, y2 = _fwd(c), _fwd(c)
    assert torch.isfinite(y1).all() and _same(y1, y2)
    r1, r2 = _bwd(c), _bwd(c)
    assert torch.isfinite(r1.dx).all()
    for name in ("dx",) + GRADS:
        assert _same(getattr(r1, name), getattr(r2, name)), name


# ============================================================================= d. fused dropout-pad store
DROP_LAYOUTS = [(0, 0), (11, 0), (3, 4)]     # (pad, tail rows); pad = 11: the zeroing loop (8 rows a pass) runs twice


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("pad,tail", DROP_LAYOUTS)
@pytest.mark.parametrize("B,G,D", [(3, 9, 96), (2, 25, 32)])
def test_ppeg_bwd_fused_dropout_pad_store(B, G, D, pad, tail, dtype):
    """dout [B, n_pad = pad + S + tail, D] in fp32 / bf16, p in {0, 0.7}, seed_ptr NULL or a device
    counter (the mask is kernel_refs.dropout_keep(seed, row b*S + t, column), the one function of
    test_dropout_mask_is_one_function_of_seed_row_column, which keeps about 0.3 of the entries):
      - dx and the six weight gradients are bitwise those of the call with dout = NULL;
      - dout[b][pad + t] is bitwise T(where(keep(b*S + t, c), dx fp32(1/0.3), 0)) of the kernel's own dx
        (at p = 0, T(dx)), the class token t = 0 included;
      - pad rows are exactly zero; tail rows and the extra row keep the sentinel;
      - tm_dropout_bwd_pad, fed that dx with the same arguments, writes the same bits (and leaves the
        same tail rows alone)."""
    L = _lib()
    _p, _stream = _eng()
    c = _case(B, G, D, False)
    S = c.S
    n_pad = pad + S + tail
    base = _bwd(c)
    for p in (0.0, 0.7):
        for use_ptr in (False, True):
            r = _bwd(c, (dtype, n_pad, pad, p, use_ptr))
            for name in ("dx",) + GRADS:
                assert _same(getattr(r, name), getattr(base, name)), (name, p, use_ptr)
            sp, ctr = _seed_args(use_ptr)
            want = r.dx.reshape(B * S, D)
            kept = 1.0
            if p > 0:
                keep = torch.from_numpy(R.dropout_keep(ctr, SEED, B * S, D, p))
                kept = keep.double().mean().item()
                assert abs(kept - 0.3) < 0.01
                want = torch.where(keep, want * torch.tensor(float(R.drop_scale_f32(p))), torch.zeros(()))
            want = want.to(dtype).view(B, S, D)
            assert (r.dout[-1].float() == SENTINEL).all()
            out = r.dout[:-1].view(B, n_pad, D)
            wrong = int((_bits(out[:, pad:pad + S]) != _bits(want)).sum().item())
            _report(f"fused store: kept fraction, wrong entries {B, G, D, pad, tail, dtype, p, use_ptr}", (kept, wrong))
            assert wrong == 0
            assert (_bits(out[:, :pad]) == 0).all()
            assert (out[:, pad + S:].float() == SENTINEL).all()
            # the stand-alone kernel on the same dx
            twin = torch.full((B * n_pad + 1, D), SENTINEL, dtype=dtype, device=DEV)
            dxd = r.dx.to(DEV).contiguous()
            L.call("tm_dropout_bwd_pad", _tt(dtype), _p(dxd), B, S, n_pad, pad, D, C.c_float(p), C.c_uint64(SEED), _p(sp),
                   _p(twin), _stream())
            torch.cuda.synchronize()
            assert _same(twin.cpu(), r.dout)


# ============================================================================= e. deferred reductions
def test_ppeg_bwd_deferred_reductions_match_the_immediate_form():
    """(2, 25, 32) with a caller-owned tm_reduce_queue: after tm_ppeg_bwd six reductions are pending,
    the six gradient buffers still hold their NaN sentinel and dx is already final; after the flush
    the gradients are bitwise those of the immediate form (rq = NULL)."""
    c = _case(2, 25, 32, False)
    base = _bwd(c)
    with _Queue() as q:
        o = _bwd_launch(c, rq=q.h)
        torch.cuda.synchronize()
        pending = q.pending()
        _report("deferred: pending reductions", pending)
        assert pending == 6
        for name in GRADS:
            assert torch.isnan(getattr(o, name).cpu()).all(), name
        dx = o.dx.cpu()[:-1].view(c.B, c.S, c.D)
        assert _same(dx, base.dx)
        q.flush()
        r = _bwd_collect(o)
        assert q.pending() == 0
    for name in ("dx",) + GRADS:
        assert _same(getattr(r, name), getattr(base, name)), name
