"""The stage kernel's preloaded leading arguments (pinv_split.hip: `meta` and term 0's operand
pointers of every job, from which a producer wave issues its first LDS-DMA chunk before the job
descriptor has arrived) under graph replay, where the kernel arguments are frozen at capture: the
other pinv tests run the chain eagerly, the bench replays it.

tm_pinv_fwd_split_a3 + tm_pinv_bwd_split are captured once in one graph on fixed buffers and
replayed twice, the inputs overwritten in place between the replays.  Every output of a replay (the
whole saved buffer: Z fp32 and every saved split plane; W, lse3; the softmax-side gradient) equals,
byte for byte, an eager call on the same inputs in buffers of its own, and the eager result is
within the bounds test_pinv_stage_descriptor_gpu.py uses (5e-4 for Z, 4e-3 for the gradient) of the
exact-fp32 chain (tm_pinv_fwd / tm_pinv_bwd, prec 0).

Cases: nbh 1 with iters 1 (the F level built on X^T with the "kr" A image), nbh 9 with iters 2 (past one round of the 8 XCDs and not a multiple of 8;
the two-term level, the DOT launch and the AUX row)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAT = 65536
A3_N = 512   # keys of the A3 partials that the _a3 entry point combines beside the last level

CASES = [(1, 1), (9, 2)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _api():
    from transmil_deepgraft_amd import _lib
    from transmil_deepgraft_amd.engine import _p, _stream
    return _lib, _p, _stream


def _input_set(nbh, iters, which):
    """Host copies of one set of inputs: X (softmax rows), dL/dZ, and q / k / v of the A3 partials."""
    g = torch.Generator().manual_seed(5000 * which + 1000 * iters + nbh)
    X = torch.softmax(torch.randn(nbh, 256, 256, generator=g) * 0.3, dim=-1).contiguous()
    gz = (torch.randn(nbh, 256, 256, generator=g) * 1e-3).contiguous()
    ql = torch.randn(nbh, 256, 64, generator=g) * 0.4
    k = (torch.randn(nbh, A3_N, 64, generator=g) * 0.4).to(torch.bfloat16)
    v = torch.randn(nbh, A3_N, 64, generator=g).to(torch.bfloat16)
    return X, gz, ql, k, v


def _fp32_chain(X, gz, nbh, iters):
    """Z_iters and dL/ds of the exact-fp32 chain."""
    _lib, _p, _stream = _api()
    saved = torch.empty(_lib.query("tm_pinv_saved_floats", nbh, iters), device=DEV)
    _lib.call("tm_pinv_fwd", _p(X), nbh, iters, 0, _p(saved), _stream())
    z = saved[iters * nbh * MAT:(iters + 1) * nbh * MAT].view(nbh, 256, 256).clone()
    work = torch.empty(_lib.query("tm_pinv_bwd_workspace_floats", nbh), device=DEV)
    dX = torch.empty(nbh, 256, 256, device=DEV)
    _lib.call("tm_pinv_bwd", _p(X), nbh, iters, 0, _p(saved), _p(gz.clone()), _p(work), _p(dX), _stream())
    ds = torch.empty_like(dX)
    _lib.call("tm_softmax_bwd_rows256", _p(X), _p(dX), _p(ds), nbh * 256, _stream())
    torch.cuda.synchronize()
    return z, ds


class _Buffers:
    """One set of device buffers for the two calls; `load` writes an input set into them in place."""

    def __init__(self, nbh, iters):
        _lib, _, _ = _api()
        self.nbh, self.iters = nbh, iters
        self.X = torch.empty(nbh, 256, 256, device=DEV)
        self.Xs = torch.empty(2 * nbh * MAT, dtype=torch.bfloat16, device=DEV)
        self.gzs = torch.empty(2 * nbh * MAT, dtype=torch.bfloat16, device=DEV)
        self.ql = torch.empty(nbh, 256, 64, device=DEV)
        self.k = torch.empty(nbh, A3_N, 64, dtype=torch.bfloat16, device=DEV)
        self.v = torch.empty(nbh, A3_N, 64, dtype=torch.bfloat16, device=DEV)
        self.work3 = torch.empty(_lib.query("tm_nys_a3_workspace", nbh, A3_N) // 4 + 16, device=DEV)
        self.parts = _lib.query("tm_nys_a3_partials", nbh, A3_N)
        self.saved = torch.empty(_lib.query("tm_pinv_split_saved_floats", nbh, iters), device=DEV)
        self.work = torch.empty(_lib.query("tm_pinv_bwd_split_workspace_floats", nbh), device=DEV)
        self.w = torch.empty(nbh, 256, 64, device=DEV)
        self.lse = torch.empty(nbh, 256, device=DEV)
        self.ds = torch.empty(nbh, 256, 256, device=DEV)

    def load(self, inputs):
        """The inputs of the two calls, in place: X and its split planes, the A3 partials, dL/dZ as
        split planes at the start of the backward's workspace; every output is set to NaN."""
        _lib, _p, _stream = _api()
        from transmil_deepgraft_amd._lib import BF16
        X, gz, ql, k, v = inputs
        self.X.copy_(X); self.ql.copy_(ql); self.k.copy_(k); self.v.copy_(v)
        n = self.nbh * MAT
        _lib.call("tm_split_f32", _p(self.X), _p(self.Xs), n, _stream())
        _lib.call("tm_split_f32", _p(gz.to(DEV)), _p(self.gzs), n, _stream())
        _lib.call("tm_nys_a3_fwd", BF16, _p(self.ql), _p(self.k), _p(self.v), self.nbh, A3_N, _p(self.work3), _p(None),
                  _p(None), _stream())
        for t in (self.saved, self.work, self.w, self.lse, self.ds):
            t.fill_(float("nan"))
        self.work[:n].view(torch.bfloat16).copy_(self.gzs)

    def calls(self):
        _lib, _p, _stream = _api()
        _lib.call("tm_pinv_fwd_split_a3", _p(self.X), _p(self.Xs), self.nbh, self.iters, _p(self.saved), _p(self.work3),
                  self.parts, _p(self.w), _p(self.lse), _stream())
        _lib.call("tm_pinv_bwd_split", _p(self.X), _p(self.Xs), self.nbh, self.iters, _p(self.saved), _p(self.work), 1,
                  _p(self.ds), _stream())

    def outputs(self):
        return dict(saved=self.saved, w=self.w, lse3=self.lse, ds=self.ds)


@pytest.mark.parametrize("nbh,iters", CASES)
def test_stage_preload_graph_replay_equals_eager(nbh, iters):
    sets = [_input_set(nbh, iters, which) for which in (0, 1)]
    zn = nbh * MAT

    # eager, each input set in buffers of its own, against the exact-fp32 chain
    eager = []
    for which, inputs in enumerate(sets):
        b = _Buffers(nbh, iters)
        b.load(inputs)
        b.calls()
        torch.cuda.synchronize()
        out = {n: t.clone() for n, t in b.outputs().items()}
        assert all(torch.isfinite(t).all() for t in out.values())
        z_ref, ds_ref = _fp32_chain(b.X, inputs[1].to(DEV), nbh, iters)
        ez, eds = _rel(out["saved"][:zn].view(nbh, 256, 256), z_ref), _rel(out["ds"], ds_ref)
        print(f"nbh {nbh} iters {iters} set {which}: rel |Z - Z_fp32| {ez:.3e}, rel |ds - ds_fp32| {eds:.3e}")
        assert ez < 5e-4
        assert eds < 4e-3
        eager.append(out)
    assert not torch.equal(eager[0]["saved"].view(torch.int32), eager[1]["saved"].view(torch.int32))

    # one graph of both calls on fixed buffers, captured on the first set; a replay per set
    b = _Buffers(nbh, iters)
    b.load(sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.calls()   # first use outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.calls()
    for which, inputs in enumerate(sets):
        b.load(inputs)
        graph.replay()
        torch.cuda.synchronize()
        for name, t in b.outputs().items():
            assert torch.equal(t.view(torch.int32), eager[which][name].view(torch.int32)), \
                f"replay {which}: {name} differs from the eager call"
