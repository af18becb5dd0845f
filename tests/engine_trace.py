"""Run the engine's host orchestration on CPU tensors and record what it would launch.

``_lib.call`` / ``_lib.query`` / ``ReduceQueue`` / ``_stream`` / ``probe`` / ``Pool`` / ``_p`` of
``transmil_deepgraft_amd.engine`` are replaced by recorders, so no kernel executes and no GPU is
needed.  Two views of one run:

  * ``Tracer.log``: the names only -- ("gemm", site, M, N, K) / ("call", name) / ("ready", i) --
    what test_bench_sites.py and test_gemm_pair_cpu.py assert on;
  * ``Tracer.trace``: every ``_lib.call`` and ``tm_reduce_flush`` as [name, open probe site, args],
    every ``_lib.query`` as ["?name", args], every ``ready(i)`` as ["ready", i].  ints stay ints,
    ``c_float`` / ``c_uint64`` are recorded by value, structs (``byref`` or arrays of them) as
    {field: value} of their non-zero fields, and every pointer -- those in struct fields too -- as
    None or "b<buffer id>+<byte offset>".  Buffer ids count in order of first appearance in the
    trace, so the allocation order is free but any change of aliasing shows; ``Tracer.buffers[id]``
    is that buffer's "dtype:bytes".

Every buffer the engine allocates or is handed is held until the tracer dies, so no address is
used twice within a run.  A pointer that lies in no known buffer is an error.
"""
import bisect
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QUERY_RESULT = 1 << 24      # sizes (bytes or floats): big enough for any view the engine takes


class Tracer:
    def __init__(self, target=None):
        self.target = target        # engine.probe.target, as gemm_pair reads it
        self.site = []
        self.log = []
        self.trace = []
        self.buffers = []           # id -> "dtype:bytes", in order of first appearance
        self._bases = []            # sorted storage base addresses
        self._known = {}            # base -> [size, dtype, id or None]
        self._held = []

    # ---- buffers
    def register(self, t, dtype=None):
        """Hold ``t`` and make its storage known (tensors, or containers of them)."""
        if isinstance(t, dict):
            t = list(t.values())
        if isinstance(t, (list, tuple)):
            for u in t:
                self.register(u)
            return
        if not isinstance(t, torch.Tensor):
            return
        self._held.append(t)
        s = t.untyped_storage()
        base = s.data_ptr()
        if base and base not in self._known:
            bisect.insort(self._bases, base)
            self._known[base] = [s.nbytes(), dtype or str(t.dtype).replace("torch.", ""), None]

    def ptr(self, addr):
        """A raw address -> None or "b<buffer id>[+<byte offset>]"."""
        if isinstance(addr, C.c_void_p):
            addr = addr.value
        if not addr:
            return None
        i = bisect.bisect_right(self._bases, addr) - 1
        base = self._bases[i] if i >= 0 else None
        if base is None or addr >= base + max(self._known[base][0], 1):
            raise AssertionError(f"pointer {addr:#x} lies in no buffer the tracer knows")
        rec = self._known[base]
        if rec[2] is None:
            rec[2] = len(self.buffers)
            self.buffers.append(f"{rec[1]}:{rec[0]}")
        return f"b{rec[2]}+{addr - base}" if addr > base else f"b{rec[2]}"

    # ---- argument encoding
    def _field(self, ctype, v):
        if ctype is C.c_void_p:
            return self.ptr(v)
        if issubclass(ctype, C.Array):      # without its trailing zeros / NULLs
            out = [self._field(ctype._type_, x) for x in v]
            while out and not out[-1]:
                out.pop()
            return out
        if issubclass(ctype, C.Structure):
            return self._struct(v)
        return v

    def _struct(self, s):
        out = {name: self._field(ctype, getattr(s, name)) for name, ctype in s._fields_}
        return {name: v for name, v in out.items() if v}      # a field left out is 0 / NULL

    def _arg(self, a):
        if a is None or isinstance(a, C.c_void_p):
            return self.ptr(a)
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, int):
            return a
        if isinstance(a, (C.c_float, C.c_uint64)):
            return a.value
        if isinstance(a, C.Structure):
            return self._struct(a)
        if isinstance(a, C.Array):
            return [self._struct(x) for x in a]
        if hasattr(a, "_obj"):      # byref(struct)
            return self._struct(a._obj)
        raise AssertionError(f"argument of a kind the tracer does not encode: {a!r}")

    # ---- the recorders
    def call(self, name, *args):
        site = self.site[-1] if self.site else None
        if name == "tm_gemm":
            g = args[3]._obj
            self.log.append(("gemm", site, g.M, g.N, g.K))
        else:
            self.log.append(("call", name))
        self.trace.append([name, site, [self._arg(a) for a in args]])

    def query(self, name, *args):
        self.trace.append(["?" + name, [self._arg(a) for a in args]])
        return QUERY_RESULT

    def ready(self, i):
        self.log.append(("ready", i))
        self.trace.append(["ready", i])

    def flush(self, handle):
        self.log.append(("call", "tm_reduce_flush"))
        self.trace.append(["tm_reduce_flush", self.site[-1] if self.site else None, [self.ptr(handle)]])

    def __call__(self, name):       # engine.probe(name)
        return _Site(self, name)


class _Site:
    def __init__(self, rec, name):
        self.rec, self.name = rec, name

    def __enter__(self):
        self.rec.site.append(self.name)

    def __exit__(self, *exc):
        self.rec.site.pop()
        return False


def install(mp, rec):
    """Replace the engine's ways out to the library and the allocator by ``rec`` (``mp``: a
    pytest MonkeyPatch, which puts them back)."""
    from transmil_deepgraft_amd import engine

    class Queue:
        """Stands in for engine.ReduceQueue; its handle is a buffer of its own, so a trace shows
        which calls were handed the queue and which NULL."""

        def __init__(self):
            self.mem = torch.empty(8, dtype=torch.uint8)
            rec.register(self.mem, "reduce_queue")
            self.handle = C.c_void_p(self.mem.data_ptr())

        def pending(self):
            return 1

        def flush(self):
            rec.flush(self.handle)

        def close(self):
            pass

    class Pool(engine.Pool):
        def __call__(self, numel, dtype=torch.float32):
            t = super().__call__(numel, dtype)
            rec.register(t)
            return t

    real_p = engine._p

    def _p(t):
        rec.register(t)
        return real_p(t)

    mp.setattr(engine._lib, "call", rec.call)
    mp.setattr(engine._lib, "query", rec.query)
    mp.setattr(engine._lib, "lib", lambda: None)
    mp.setattr(engine, "ReduceQueue", Queue)
    mp.setattr(engine, "Pool", Pool)
    mp.setattr(engine, "_p", _p)
    mp.setattr(engine, "_stream", lambda: C.c_void_p(0))
    mp.setattr(engine, "probe", rec)
    return engine


def run_transmil(N, *, dtype=torch.bfloat16, fc1="plain", B=1, parts=2, target=None, pair_gemms=None,
                 cls_only=True, cls_q_rows=None, fused_ce=True):
    """One forward + backward of TransMILEngine; returns the Tracer.  ``fused_ce`` (the training
    step: drop 0.7, device seed + counter, the loss in the head's launch, ``gloss``); False: eval
    dropout, no device seed, plain head with ``dlogits`` given."""
    from transmil_deepgraft_amd.models import TransMIL
    rec = Tracer(target)
    with pytest.MonkeyPatch.context() as mp:
        engine = install(mp, rec)
        if cls_q_rows is not None:
            mp.setattr(engine, "CLS_Q_ROWS", cls_q_rows)
        layout, feat, width = {"plain": (engine.FC1_PLAIN, 512, 512), "rcc2048": (engine.FC1_RCC2048, 2048, 2048),
                               "embed": (engine.FC1_EMBED, 768, 512)}[fc1]
        torch.manual_seed(0)
        model = TransMIL(2, feat, 512).train()
        names, params = model._engine_params(layout)
        prm = dict(zip(names, [p.detach() for p in params]))
        eng = engine.TransMILEngine(dtype, fc1=layout, head="_fc", cls_only=cls_only)
        if pair_gemms is not None:
            eng.pair_gemms = pair_gemms
        x = torch.zeros(B, N, width)
        out = {n: torch.empty_like(p) for n, p in prm.items()}
        rec.register([prm, x, out])
        if fused_ce:
            seed_dev = torch.zeros(1, dtype=torch.int64)
            counter = torch.zeros(1, dtype=torch.int64)
            ce = (torch.zeros(B, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int32))
            gloss = torch.ones(())
            rec.register([seed_dev, counter, ce, gloss])
            logits, ctx = eng.forward(x, prm, 0.7, seed_dev=seed_dev, counter=counter, ce=ce)
            eng.backward(None, ctx, prm, out=out, ready=rec.ready, gloss=gloss, parts=parts)
        else:
            dlogits = torch.ones(B, 2)
            rec.register(dlogits)
            logits, ctx = eng.forward(x, prm, 0.0)
            eng.backward(dlogits, ctx, prm, out=out, ready=rec.ready, parts=parts)
    return rec


def run_nystrom(S, dim, *, dtype=torch.bfloat16, B=2, heads=8):
    """One forward + backward of the standalone NystromEngine at ``dim`` = heads * dim_head
    (landmarks = dim / 2, the TransMIL widths); returns the Tracer."""
    rec = Tracer()
    with pytest.MonkeyPatch.context() as mp:
        engine = install(mp, rec)
        x = torch.zeros(B, S, dim)
        w = [torch.zeros(3 * dim, dim), torch.zeros(dim, dim), torch.zeros(dim), torch.zeros(heads, 1, 33, 1)]
        dout = torch.zeros(B, S, dim)
        rec.register([x, w, dout])
        eng = engine.NystromEngine(dtype)
        y, ctx = eng.forward(x, *w, heads, drop_p=0.1, seed=0x51ED27, dim_head=dim // heads, num_landmarks=dim // 2)
        eng.backward(dout, ctx)
    return rec


_ALL3 = ("out", "qkv", "kv")

# name -> (runner, positional arguments, keyword arguments): the golden traces of
# tests/golden/engine_trace/ (make_golden_engine_trace.py writes them, test_engine_trace_cpu.py
# compares)
CASES = {
    # the bench step's structure: the head rides in the class-row launch
    "bf16_n300": (run_transmil, (300,), {}),
    "bf16_n8192": (run_transmil, (8192,), {}),                    # split-K counts and A3 splits differ with size
    # tm_head_ce_bwd, the inner _fc1 stage, three ready()
    "bf16_b2_rcc_parts3": (run_transmil, (1000,), dict(fc1="rcc2048", B=2, parts=3)),
    "bf16_dense_layer2": (run_transmil, (300,), dict(cls_only=False)),
    "bf16_no_q_rows": (run_transmil, (300,), dict(cls_q_rows=False)),     # tm_nys_assemble_q_slab
    "bf16_plain_head": (run_transmil, (300,), dict(fused_ce=False)),      # tm_head_fwd / tm_head_bwd
    "bf16_pairs_all": (run_transmil, (1000,), dict(pair_gemms=_ALL3)),
    "bf16_pairs_off": (run_transmil, (1000,), dict(pair_gemms=False)),
    "bf16_probe_target": (run_transmil, (1000,), dict(target={"dxn_gemm", "fc1_gemm"})),
    "bf16_embed": (run_transmil, (300,), dict(fc1="embed")),              # the __dx__ path
    "f32_n300": (run_transmil, (300,), dict(dtype=torch.float32)),
    "f32_b2_dense": (run_transmil, (300,), dict(dtype=torch.float32, B=2, cls_only=False)),
    "nys_bf16_512": (run_nystrom, (300, 512), {}),
    "nys_f32_512": (run_nystrom, (300, 512), dict(dtype=torch.float32)),
    "nys_bf16_384": (run_nystrom, (200, 384), {}),                        # dim_head 48, 192 landmarks
    "nys_f32_256": (run_nystrom, (130, 256), dict(dtype=torch.float32)),  # dim_head 32, 128 landmarks
}


def record(case):
    """The golden form of one case: plain JSON types only."""
    fn, args, kw = CASES[case]
    rec = fn(*args, **kw)
    return {"case": case, "buffers": rec.buffers, "trace": rec.trace}
