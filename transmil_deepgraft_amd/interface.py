"""The Lightning-step surface of the hot path, without Lightning.

Mirrors the pieces of ``ModelInterface`` (code/models/model_interface.py:108)
that the TransMIL training step runs, with the same hook names and argument
meaning, so a Lightning user can swap the model in and a plain loop can drive
it on MI355X:

* ``create_loss``       -- ``nn.CrossEntropyLoss()`` (code/MyLoss/loss_factory.py:21-62; soft
                           one-hot target as at model_interface.py:346-347)
* ``add_weight_decay`` / ``create_optimizer`` -- no-decay groups + RAdam, optionally
                           wrapped in Lookahead (code/MyOptimizer/optim_factory.py:25-123)
* ``Lookahead``         -- k-step slow-weight wrapper (alpha 0.5, k 6; multi-tensor ops)
* ``FusedRAdamLookahead`` -- RAdam + Lookahead for the GPU as one HIP elementwise launch
* ``GradBucket`` / ``GradAllReduce`` -- the DDP gradient all-reduce (Lightning DDP,
                           code/train.py:178-201): gradients live as views of one flat fp32
                           bucket in two parts, each averaged with one RCCL all_reduce over
                           xGMI, part 0 overlapping layer1's backward (9.64 MB of fp32 grads)
* ``TransMILTask``      -- ``training_step`` / ``configure_optimizers`` with the reference's
                           batch format ``(bags[B,n,F], labels[B], (names, patients))``, and
                           ``validation_step`` / ``test_step`` with their epoch hooks
* ``EvalRecord``        -- the evaluation epoch's per-slide record on the device (one HIP launch
                           per step, no host sync) and the epoch-end metric reductions
* ``GraphedEvaluation`` -- the evaluation step replayed as one captured hipGraph per bag shape
"""
from __future__ import annotations

import ctypes as C
from collections import defaultdict

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F


def create_loss(base_loss: str = "CrossEntropyLoss") -> nn.Module:
    if not hasattr(nn, base_loss):
        raise ValueError(f"unsupported loss {base_loss}")
    return getattr(nn, base_loss)()


def add_weight_decay(model: nn.Module, weight_decay: float = 1e-5, skip_list=()):
    """1-D tensors and ``.bias`` -> no decay (optim_factory.py:25-37)."""
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if p.dim() == 1 or name.endswith(".bias") or name in skip_list else decay).append(p)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


class Lookahead(torch.optim.Optimizer):
    """Every k inner steps: slow += alpha * (fast - slow); fast = slow.

    Same schedule as the reference wrapper (code/MyOptimizer/lookahead.py; the
    first sync only initialises the slow weights), but branch-free on the device:
    the step counter and the "slow weights initialised" flag are device scalars
    and the update is masked, so the whole optimizer step can be captured in a
    hipGraph and replayed."""

    def __init__(self, base: torch.optim.Optimizer, alpha: float = 0.5, k: int = 6):
        if not 0.0 <= alpha <= 1.0 or k < 1:
            raise ValueError("Lookahead: alpha in [0,1], k >= 1")
        self.base_optimizer = base
        self.param_groups = base.param_groups
        self.defaults = dict(base.defaults, lookahead_alpha=alpha, lookahead_k=k, lookahead_step=0)
        self.state = defaultdict(dict)
        self._dev = None
        for g in self.param_groups:
            g.setdefault("lookahead_alpha", alpha)
            g.setdefault("lookahead_k", k)
            g.setdefault("lookahead_step", 0)

    @torch.no_grad()
    def _sync_group(self, gi, g):
        fast = [p for p in g["params"] if p.grad is not None]
        if not fast:
            return
        key = ("group", gi)
        st = self.state[key]
        if "slow" not in st:
            dev = fast[0].device
            st["slow"] = [torch.zeros_like(p) for p in fast]
            st["step"] = torch.zeros((), device=dev)
            st["init"] = torch.zeros((), device=dev)
        slow, step, init = st["slow"], st["step"], st["init"]
        step.add_(1.0)
        m = (torch.remainder(step, float(g["lookahead_k"])) == 0).float()
        coef = m * (1.0 - init * (1.0 - g["lookahead_alpha"]))
        diff = torch._foreach_sub(fast, slow)
        torch._foreach_add_(slow, torch._foreach_mul(diff, coef))
        back = torch._foreach_sub(slow, fast)
        torch._foreach_add_(fast, torch._foreach_mul(back, m))
        torch.maximum(init, m, out=init)

    def step(self, closure=None):
        loss = self.base_optimizer.step(closure)
        for gi, g in enumerate(self.param_groups):
            g["lookahead_step"] += 1
            self._sync_group(gi, g)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        self.base_optimizer.zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        """``{'state': base state, 'slow_state': ..., 'param_groups': ...}`` as the reference
        wrapper saves it (code/MyOptimizer/lookahead.py:56-68); the slow state is keyed by group
        index and also carries the device step counter and init flag."""
        fast = self.base_optimizer.state_dict()
        slow = {}
        for (_, gi), st in self.state.items():
            slow[gi] = {"slow": [t.detach().clone() for t in st["slow"]],
                        "step": st["step"].detach().clone(), "init": st["init"].detach().clone()}
        return {"state": fast["state"], "slow_state": slow, "param_groups": fast["param_groups"]}

    def load_state_dict(self, state_dict):
        """Restores the base optimizer (its moments and the lookahead_* group fields) and the
        slow weights with their step counter / init flag (lookahead.py:70-88)."""
        self.base_optimizer.load_state_dict({"state": state_dict["state"],
                                             "param_groups": state_dict["param_groups"]})
        self.param_groups = self.base_optimizer.param_groups
        self.state = defaultdict(dict)
        for gi, st in state_dict.get("slow_state", {}).items():
            dev = self.param_groups[int(gi)]["params"][0].device
            self.state[("group", int(gi))] = {"slow": [t.to(dev).clone() for t in st["slow"]],
                                              "step": st["step"].to(dev).clone(),
                                              "init": st["init"].to(dev).clone()}


class FusedRAdamLookahead(torch.optim.Optimizer):
    """``Lookahead(torch.optim.RAdam(groups))`` as ONE HIP launch pair per step.

    Same update as ``torch.optim.RAdam`` (L2 weight decay folded into the gradient,
    ``decoupled_weight_decay=False``; code/MyOptimizer/optim_factory.py:77-79) followed
    by the reference Lookahead sync every ``k`` steps (code/MyOptimizer/lookahead.py,
    wrapped at optim_factory.py:118-121; ``lookahead_k=0`` gives plain RAdam).  The
    moments and slow weights of every parameter live in three flat fp32 buffers, the
    step counters on the device, and the kernel reads each parameter/gradient through
    a pointer table passed by value (``tm_radam_lookahead_step``, csrc/optim.hip), so
    the step is hipGraph-capturable.  ``lr`` / ``weight_decay`` reach the kernel through a
    small device array (``tm_optim_table.hyper``) that every eager step -- and, before each
    replay, ``GraphedOptimizationStep`` via ``refresh_hyper()`` -- rewrites from the groups, so an
    LR scheduler (``configure_optimizers``' ReduceLROnPlateau) also acts on a replayed graph."""

    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 lookahead_alpha=0.5, lookahead_k=6):
        if not 0.0 <= lookahead_alpha <= 1.0 or lookahead_k < 0:
            raise ValueError("Lookahead: alpha in [0,1], k >= 0")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        lookahead_alpha=lookahead_alpha, lookahead_k=lookahead_k, lookahead_step=0)
        super().__init__(params, defaults)
        from . import _lib
        self._lib = _lib
        plist = [p for g in self.param_groups for p in g["params"]]
        if any(p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() for p in plist):
            raise ValueError("fused RAdam: parameters must be contiguous fp32 CUDA tensors")
        for g in self.param_groups:
            for key in ("betas", "eps", "lookahead_alpha", "lookahead_k"):
                if g[key] != self.param_groups[0][key]:
                    raise ValueError(f"fused RAdam: '{key}' must be equal across groups")
        self._all = plist
        self._params = None     # the parameters that receive gradients: fixed at the first step

    def _activate(self, plist):
        """Lay the state of ``plist`` (the parameters with a gradient, in group order) out in three
        flat fp32 buffers.  Parameters that never receive a gradient (modules kept only for the
        state_dict, e.g. CTMIL._fc1) are skipped, as torch.optim.RAdam skips ``grad is None``."""
        if len(plist) > self._lib.OPTIM_MAX_TENSORS:
            raise ValueError(f"fused RAdam: at most {self._lib.OPTIM_MAX_TENSORS} parameter tensors with "
                             "gradients (create_optimizer falls back to torch.optim.RAdam above that)")
        if not plist:
            raise RuntimeError("fused RAdam: no parameter has a gradient")
        self._params = plist
        self._index = {id(p): i for i, p in enumerate(plist)}
        total = sum((p.numel() + 3) // 4 * 4 for p in plist)
        dev = plist[0].device
        self._flat = torch.zeros(3, total, dtype=torch.float32, device=dev)  # exp_avg, exp_avg_sq, slow
        # one (RAdam step, Lookahead step) pair per workgroup of the update launch; pair 0 is checkpointed
        self._counters = torch.zeros(max(3, int(self._lib.query("tm_radam_counters_len", total))),
                                     dtype=torch.int32, device=dev)
        self._offsets = [0]
        for p in plist:     # each tensor's flat state padded to a multiple of 4 (16-B vectors)
            self._offsets.append(self._offsets[-1] + (p.numel() + 3) // 4 * 4)
        self._hyper = torch.zeros(len(plist), 2, dtype=torch.float32, device=dev)   # (lr, weight_decay)
        self._hyper_host = None
        self._bind_state()

    def _hyper_values(self):
        vals = []
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) in self._index:
                    vals.append((float(g["lr"]), float(g["weight_decay"])))
        return vals

    @torch.no_grad()
    def refresh_hyper(self):
        """Write the groups' current lr / weight_decay into the device array the update kernel reads
        (a no-op when they have not changed).  Must run outside stream capture: a captured step
        reads whatever the array holds when it is replayed."""
        if self._params is None:
            return
        vals = self._hyper_values()
        if vals != self._hyper_host:
            self._hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_host = vals

    def _bind_state(self):
        for i, p in enumerate(self._params):
            a, b = self._offsets[i], self._offsets[i] + p.numel()
            self.state[p] = {"exp_avg": self._flat[0, a:b].view_as(p),
                             "exp_avg_sq": self._flat[1, a:b].view_as(p),
                             "slow_buffer": self._flat[2, a:b].view_as(p)}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = self._lib
        if self._params is None:
            self._activate([p for p in self._all if p.grad is not None])
        if not torch.cuda.is_current_stream_capturing():
            self.refresh_hyper()
        tab = lib.OptimTable()
        tab.hyper = self._hyper.data_ptr()
        tab.count = len(self._params)
        i = 0
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) not in self._index:
                    if p.grad is not None:
                        raise RuntimeError("fused RAdam: a parameter without a gradient at the first step has "
                                           "one now (its step count would differ from torch.optim.RAdam's); "
                                           "use opt='radam' on a model whose parameter set is fixed")
                    continue
                if p.grad is None:
                    raise RuntimeError("fused RAdam: a parameter that had a gradient at the first step has "
                                       "none now")
                t = tab.t[i]
                t.param, t.grad, t.numel = p.data_ptr(), p.grad.data_ptr(), p.numel()
                t.lr, t.weight_decay = float(g["lr"]), float(g["weight_decay"])
                tab.offset[i] = self._offsets[i]
                i += 1
            g["lookahead_step"] += 1
        tab.offset[i] = self._offsets[i]
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        lib.call("tm_radam_lookahead_step", C.byref(tab), self._flat[0].data_ptr(), self._flat[1].data_ptr(),
                 self._flat[2].data_ptr(), self._counters.data_ptr(), float(b1), float(b2), float(g0["eps"]),
                 int(g0["lookahead_k"]), float(g0["lookahead_alpha"]),
                 torch.cuda.current_stream(self._flat.device).cuda_stream)
        return loss

    def state_dict(self):
        sd = super().state_dict()
        if self._params is not None:
            sd["fused_counters"] = self._counters[:3].cpu()
        return sd

    def load_state_dict(self, state_dict):
        counters = state_dict.get("fused_counters")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "fused_counters"})
        with torch.no_grad():
            loaded = {p: {k: v.detach().clone() for k, v in self.state[p].items() if torch.is_tensor(v)}
                      for p in self._all if p in self.state}
            if self._params is None:
                stateful = [p for p in self._all if "exp_avg" in loaded.get(p, {})]
                if not stateful:
                    return
                self._activate(stateful)
            self._bind_state()
            self._hyper_host = None
            for i, p in enumerate(self._params):
                st = loaded.get(p, {})
                a, b = self._offsets[i], self._offsets[i] + p.numel()
                for row, key in enumerate(("exp_avg", "exp_avg_sq", "slow_buffer")):
                    if key in st:
                        self._flat[row, a:b].copy_(st[key].reshape(-1))
            if counters is not None:
                self._counters.zero_()
                npairs = self._counters.numel() // 2
                self._counters[:2 * npairs].view(npairs, 2).copy_(counters[:2].to(self._counters).expand(npairs, 2))


def create_optimizer(model: nn.Module, opt: str = "lookahead_radam", lr: float = 2e-4,
                     weight_decay: float = 0.01, eps=None, betas=None):
    """optim_factory.create_optimizer for the optimizers TransMIL configs use (radam / adam / adamw / sgd)."""
    params = add_weight_decay(model, weight_decay) if weight_decay else model.parameters()
    kw = dict(lr=lr, weight_decay=0.0)
    if eps is not None:
        kw["eps"] = eps
    if betas is not None:
        kw["betas"] = betas
    parts = opt.lower().split("_")
    name = parts[-1]
    fused = torch.cuda.is_available()
    on_gpu = fused and all(p.is_cuda for p in model.parameters())
    n_tensors = sum(1 for p in model.parameters() if p.requires_grad)
    if name == "radam" and on_gpu and n_tensors <= _lib_max_tensors():
        la = len(parts) > 1 and parts[0] == "lookahead"
        return FusedRAdamLookahead(params, lookahead_k=6 if la else 0, **kw)
    if name == "radam":
        base = torch.optim.RAdam(params, foreach=True, capturable=fused, **kw)
    elif name == "adam":
        base = torch.optim.Adam(params, foreach=not fused, fused=fused, **kw)
    elif name == "adamw":
        base = torch.optim.AdamW(params, foreach=not fused, fused=fused, **kw)
    elif name == "sgd":
        kw.pop("eps", None)
        base = torch.optim.SGD(params, momentum=0.9, nesterov=True, **kw)
    else:
        raise ValueError(f"optimizer {opt} not supported on this path")
    if len(parts) > 1 and parts[0] == "lookahead":
        return Lookahead(base)
    return base


def _lib_max_tensors():
    from . import _lib
    return _lib.OPTIM_MAX_TENSORS


class GradBucket:
    """One flat fp32 buffer that holds every parameter gradient as a view, laid out in parts in
    the order the fused backward finishes them (``TransMIL.grad_bucket_parts``).

    The fused backward writes its gradient kernels' outputs straight into these views and
    sets ``p.grad`` to them (models/TransMIL.py ``_TransMILFn.backward``), so the bucket IS
    the gradient storage: no copy in or out around the all-reduce, and the addresses are
    stable across steps (a captured hipGraph and the fused optimizer's pointer table stay
    valid).  ``ready(i)`` is called by the backward when part ``i`` is final; ``hooks`` get it."""

    def __init__(self, parts, device=None):
        self.parts_params = [list(part) for part in parts if part]
        self.params = [p for part in self.parts_params for p in part]
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("GradBucket: a parameter appears in two parts")
        dev = device if device is not None else self.params[0].device
        self._off = {}
        self.ranges = []
        off = 0
        for i, part in enumerate(self.parts_params):
            start = off
            for p in part:
                self._off[id(p)] = (off, p.numel())
                off += (p.numel() + 15) // 16 * 16     # every view 64-B aligned (vector stores)
            if i == len(self.parts_params) - 1:
                # the has-gradient flags (one float per parameter) ride at the end of the last part, so
                # the unused-parameter exchange is part of that part's all_reduce (no collective of its own)
                self._flag_off = off
                off += (len(self.params) + 15) // 16 * 16
            self.ranges.append((start, off))
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        # > 0 on every rank that has not written them: averaging keeps them > 0 (see GradAllReduce)
        self.flags = self.flat[self._flag_off:self._flag_off + len(self.params)]
        self.flags.fill_(1.0)
        self.hooks = []

    def view(self, p):
        """A fresh view of ``p``'s slice (fresh, so autograd could steal it without a clone)."""
        o, n = self._off[id(p)]
        return self.flat[o:o + n].view_as(p)

    def owns(self, p):
        """True when ``p.grad`` is this bucket's view of ``p``."""
        g = p.grad
        if g is None or id(p) not in self._off:
            return False
        o, _ = self._off[id(p)]
        return g.data_ptr() == self.flat.data_ptr() + 4 * o and g.shape == p.shape

    def part(self, i):
        a, b = self.ranges[i]
        return self.flat[a:b]

    def bind(self):
        """Make every existing ``p.grad`` the bucket's view (keeps its values by copying them in).
        A parameter without a gradient (a module kept only for the state_dict) keeps ``None``, so
        the optimizer skips it as torch.optim.RAdam does; its slice is zeroed and sums zeros."""
        with torch.no_grad():
            for p in self.params:
                if not self.owns(p):
                    v = self.view(p)
                    if p.grad is None:
                        v.zero_()
                    else:
                        v.copy_(p.grad)
                        p.grad = v

    def ready(self, i):
        for h in self.hooks:
            h(i)


class GradAllReduce:
    """Average gradients over ranks: the DDP gradient all-reduce on a ``GradBucket``.

    Replaces the Lightning DDP reducer (``strategy='ddp_find_unused_parameters_true'``,
    code/train.py:184).  On the fused path every TransMIL parameter receives a gradient each step,
    so no unused-parameter search runs; on the module-by-module path the rank's has-gradient flags
    travel in the bucket's own all_reduce (a tail of the last part) and parameters used on another
    rank adopt the averaged gradient.  With ``model=`` (a TransMIL with
    ``grad_bucket_parts``) the bucket is cut where the fused backward finishes gradients: part 0
    (head, norm, layer2, PPEG; 4.4 MB fp32) is final before layer1's backward is enqueued and, with
    ``overlap``, its RCCL all_reduce is issued right then on RCCL's stream, overlapping layer1 +
    _fc1 backward on the compute stream.  At world > 1 (``split_layer1``) part 1 is layer1 alone
    (4.2 MB), issued before the _fc1 backward, and part 2 (class token, _fc1 + the flags; 1.05 MB)
    is the only message after the whole backward (``exposed_bytes``); at world 1 (no collective)
    layer1 and _fc1 stay one part (5.2 MB), which saves the extra flush launch.  Few ~1-5 MB
    messages keep each xGMI ring step large (per-link bound).

    ``sync = False`` skips the reduction (Lightning's no-sync micro-batches under
    ``accumulate_grad_batches``, code/train.py:199); ``force`` runs the collective even at
    world size 1 (tests of the RCCL path inside a captured hipGraph)."""

    def __init__(self, params, group=None, model=None, overlap=True, force=False, split_layer1=None):
        self.params = [p for p in params if p.requires_grad]
        self.group, self.overlap, self.force = group, overlap, force
        if split_layer1 is None:
            # a third part only where a collective runs: at world 1 its extra flush launch buys nothing
            split_layer1 = self._world() > 1
        parts = [self.params]
        if model is not None and hasattr(model, "grad_bucket_parts"):
            try:
                mp = model.grad_bucket_parts(split_layer1=True) if split_layer1 else model.grad_bucket_parts()
            except TypeError:       # a model whose bucket layout has no layer1 cut
                mp = model.grad_bucket_parts()
            if {id(p) for part in mp for p in part} == {id(p) for p in self.params}:
                parts = mp
        self.bucket = GradBucket(parts, self.params[0].device)
        self.flat = self.bucket.flat
        self._model = model
        if model is not None and hasattr(model, "attach_grad_bucket"):
            model.attach_grad_bucket(self.bucket)
        self.bucket.hooks.append(self._on_ready)
        self.sync = True
        self._works = {}
        self._closed = False

    def exposed_bytes(self):
        """fp32 bytes all-reduced after the whole backward (the last part: nothing left to hide it
        behind); the earlier parts are issued from the backward and overlap what follows them."""
        a, b = self.bucket.ranges[-1]
        return 4 * (b - a) if self.overlap else 4 * self.flat.numel()

    def close(self):
        """Release everything that refers to the process group's communicator, BEFORE
        ``dist.destroy_process_group()``: waits on and drops the outstanding async works, detaches
        the bucket hook (the model's bucket keeps a bound method of this object alive) and the model's
        bucket.  A hipGraph captured over this all-reduce holds the communicator's kernels and
        its registered buffers: release it first (``GraphedOptimizationStep.close()`` or
        ``graph.reset()``).  Idempotent; a closed instance raises when called."""
        if self._closed:
            return
        for w in self._works.values():
            w.wait()
        self._works.clear()
        if self._on_ready in self.bucket.hooks:
            self.bucket.hooks.remove(self._on_ready)
        m = self._model
        if m is not None and getattr(m, "_grad_bucket", None) is self.bucket:
            m.attach_grad_bucket(None)
        self._model = None
        self._closed = True

    def _world(self):
        if not (dist.is_available() and dist.is_initialized()):
            return 0
        return dist.get_world_size(self.group)

    def _active(self):
        w = self._world()
        return self.sync and (w > 1 or (w == 1 and self.force))

    def _on_ready(self, i):
        """Backward hook: issue part ``i``'s all_reduce now (async, on RCCL's stream)."""
        if not (self.overlap and self._active()) or i in self._works:
            return
        self._works[i] = dist.all_reduce(self.bucket.part(i), op=dist.ReduceOp.SUM, group=self.group,
                                         async_op=True)

    def __call__(self):
        if self._closed:
            raise RuntimeError("GradAllReduce: called after close()")
        if not self._active():
            self._works.clear()
            return
        owned = all(self.bucket.owns(p) for p in self.params if p.grad is not None)
        local = None
        if not owned:
            # gradients produced outside the fused backward (module-by-module path): bind them, and
            # write this rank's has-gradient flags into the bucket's flag tail.  Every rank issues
            # the same all_reduces in the same order whichever path it took (the fused path's early
            # part-0 reduce from the backward hook included), so ranks on different paths cannot
            # mismatch collectives; the flags are summed with the gradients.
            local = [p.grad is not None for p in self.params]
            self.bucket.bind()
            self.bucket.flags.copy_(torch.tensor(local, dtype=torch.float32))
        for i in range(len(self.bucket.ranges)):
            if i not in self._works:
                self._works[i] = dist.all_reduce(self.bucket.part(i), op=dist.ReduceOp.SUM, group=self.group,
                                                 async_op=True)
        for i in sorted(self._works):
            self._works[i].wait()       # the compute stream waits on RCCL's stream
        self._works.clear()
        self.flat.mul_(1.0 / self._world())
        if local is not None:
            # as DDP's find_unused_parameters: a parameter without a gradient HERE but with one on
            # another rank receives the averaged gradient (its zeroed slice summed with theirs), so
            # the ranks' optimizer steps stay identical; one used on no rank keeps grad None.  A rank
            # on the fused path never writes its flags: they stay > 0 (1 at creation, then averages
            # of positive and non-negative values), i.e. "used".  (Host read: module path only.)
            used = (self.bucket.flags > 0).tolist()
            for p, here, anywhere in zip(self.params, local, used):
                if anywhere and not here:
                    p.grad = self.bucket.view(p)
        # back to "used" for the next step on EVERY rank, whichever path it took: a fused rank never
        # writes its flags, so it would otherwise carry the average forward and, beside a module-path
        # rank that never uses a parameter, halve it each step until it underflows to 0.  (One tiny
        # launch per reducing step; it runs only where a collective runs.)
        self.bucket.flags.fill_(1.0)


class _CrossEntropyOneHot(torch.autograd.Function):
    """CE(logits, one_hot(label).float()) + softmax + argmax as one HIP launch (tm_ce_fwd) and its
    backward as one (tm_ce_bwd), instead of ~17 small PyTorch kernels per step."""

    @staticmethod
    def forward(ctx, logits, label, stats):
        from . import _lib
        from .engine import _p, _stream
        B, C = logits.shape
        lg = logits.float().contiguous()
        lab = label.to(torch.int64).contiguous()
        loss = torch.empty((), device=logits.device)
        prob = torch.empty(B, C, device=logits.device)
        yhat = torch.empty(B, dtype=torch.int64, device=logits.device)
        _lib.call("tm_ce_fwd", _p(lg), _p(lab), B, C, _p(loss), _p(prob), _p(yhat), _p(stats), _stream())
        ctx.save_for_backward(prob, lab)
        ctx.mark_non_differentiable(prob, yhat)
        ctx.set_materialize_grads(False)    # no zero-filled gradients for prob / yhat (two launches)
        return loss, prob, yhat

    @staticmethod
    def backward(ctx, gloss, _gprob, _gyhat):
        from . import _lib
        from .engine import _p, _stream
        if gloss is None:
            return None, None, None
        prob, lab = ctx.saved_tensors
        B, C = prob.shape
        dl = torch.empty(B, C, device=prob.device)
        _lib.call("tm_ce_bwd", _p(prob), _p(lab), B, C, _p(gloss.float().contiguous()), _p(dl), _stream())
        return dl, None, None


class EvalRecord:
    """The per-slide record of one evaluation epoch and the epoch-end reductions over it.

    ``validation_step`` / ``test_step`` of the reference end in ``loss.item()``, a Python loop over
    ``self.data`` and a list of per-slide tensors (code/models/model_interface.py:459-469).  Here
    a step is one ``tm_eval_record`` launch that writes row ``cursor + b`` of five device arrays
    (``logits`` / ``prob`` fp32 [capacity, C], ``y_hat`` / ``label`` int64, ``nll`` fp32), bumps
    ``class_stats`` (int32 [C, 2] count / correct) and advances the device ``cursor``: no host sync,
    nothing in the launch arguments that changes from step to step, so the step can be captured
    into a hipGraph.  The host only counts rows (``n``).

    ``append`` grows the storage by doubling before a call that would overflow -- unless a
    ``GraphedEvaluation`` holds graphs over it (``pin()``): captured launches carry the arrays'
    addresses, so storage must not move, the kernel drops rows past ``capacity`` while the cursor
    keeps counting, and ``summary()`` raises.  On CPU tensors the same methods run on torch ops
    (no HIP), so the task logic is testable without a GPU."""

    _FIELDS = ("logits", "prob", "y_hat", "label", "nll")

    def __init__(self, n_classes: int, capacity: int = 256, device="cpu"):
        if n_classes < 1 or capacity < 1:
            raise ValueError("EvalRecord: n_classes >= 1 and capacity >= 1")
        self.n_classes, self.device = int(n_classes), torch.device(device)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.class_stats = torch.zeros(self.n_classes, 2, dtype=torch.int32, device=self.device)
        self.n = 0              # rows appended, counted on the host
        self._pins = 0
        self._alloc(int(capacity))

    def _alloc(self, capacity):
        C_, dev = self.n_classes, self.device
        self.capacity = capacity
        self.logits = torch.zeros(capacity, C_, dtype=torch.float32, device=dev)
        self.prob = torch.zeros(capacity, C_, dtype=torch.float32, device=dev)
        self.y_hat = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.label = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.nll = torch.zeros(capacity, dtype=torch.float32, device=dev)

    def pin(self):
        """Storage must not move from now on (a captured graph holds its addresses)."""
        self._pins += 1

    def unpin(self):
        self._pins = max(0, self._pins - 1)

    def reset(self):
        """Clear the record (in place: the arrays, the cursor and the stats keep their addresses)."""
        self.cursor.zero_()
        self.class_stats.zero_()
        self.n = 0

    def _grow(self, need):
        cap = self.capacity
        while cap < need:
            cap *= 2
        old = [getattr(self, f) for f in self._FIELDS]
        self._alloc(cap)
        for f, o in zip(self._FIELDS, old):
            getattr(self, f)[:self.n].copy_(o[:self.n])

    def write(self, logits, label):
        """The device side of ``append`` alone (what a captured graph replays): ``logits`` [B, C]
        fp32 and ``label`` [B] int64, contiguous, on the record's device."""
        B, C_ = logits.shape
        if C_ != self.n_classes or label.numel() != B:
            raise ValueError(f"EvalRecord: logits {tuple(logits.shape)} / {label.numel()} labels for "
                             f"{self.n_classes} classes")
        if logits.is_cuda:
            from . import _lib
            from .engine import _p, _stream
            _lib.call("tm_eval_record", _p(logits), _p(label), B, C_, self.capacity, _p(self.cursor),
                      _p(self.logits), _p(self.prob), _p(self.y_hat), _p(self.label), _p(self.nll),
                      _p(self.class_stats), _stream())
            return
        base = int(self.cursor)
        lse = torch.logsumexp(logits, dim=1)
        y_hat = torch.argmax(logits, dim=1)
        ok = (label >= 0) & (label < C_)
        picked = logits.gather(1, label.clamp(0, C_ - 1).unsqueeze(1)).squeeze(1)
        nll = torch.where(ok, lse - picked, torch.full_like(lse, float("nan")))
        k = max(0, min(B, self.capacity - base))
        for dst, src in zip((self.logits, self.prob, self.y_hat, self.label, self.nll),
                            (logits, torch.softmax(logits, dim=1), y_hat, label, nll)):
            dst[base:base + k] = src[:k]
        for y, h in zip(label[ok].tolist(), y_hat[ok].tolist()):
            self.class_stats[y, 0] += 1
            self.class_stats[y, 1] += int(h == y)
        self.cursor += B

    def append(self, logits, label):
        """One step: ``logits`` [B, C] and ``label`` [B] (any float / int dtype) on the record's
        device.  One launch, no sync."""
        B = logits.shape[0]
        if self.n + B > self.capacity and not self._pins:
            if logits.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EvalRecord: the record is full and cannot grow during stream capture "
                                   "(give it the epoch's capacity up front)")
            self._grow(self.n + B)
        self.write(logits.detach().float().contiguous(), label.reshape(-1).to(torch.int64).contiguous())
        self.n += B

    # ------------------------------------------------------------------ epoch end
    def summary(self, patients, positive_rule: bool = False):
        """The epoch-end reductions: ``patients`` is the host list of the ``n`` slides' patient
        names in append order.  Returns a dict of host values -- ``n``, ``nll_sum``, ``slide_cm`` /
        ``patient_cm`` ([C][C] target x prediction), ``slide_wins2`` / ``slide_npairs`` /
        ``patient_wins2`` / ``patient_npairs`` (per class, one-vs-rest), ``patient_score`` [P, C],
        ``patient_target`` / ``patient_pred`` / ``nslides`` [P], ``patients`` (names in
        first-appearance order) and ``class_stats``.  On the GPU: one upload of the patient ids, six
        launches, one device-to-host copy."""
        M, C_ = self.n, self.n_classes
        if M < 1:
            raise ValueError("EvalRecord.summary: no slide recorded")
        if M > self.capacity:
            raise RuntimeError(f"EvalRecord: {M} slides appended to a record of capacity {self.capacity} whose "
                               "storage a captured graph pins; the rows past it were dropped")
        if len(patients) != M:
            raise ValueError(f"EvalRecord.summary: {len(patients)} patient names for {M} slides")
        index, ids = {}, []
        for p in patients:
            ids.append(index.setdefault(p, len(index)))
        names = list(index)
        P_ = len(names)
        run = self._summary_hip if self.device.type == "cuda" else self._summary_cpu
        out = run(ids, M, C_, P_, bool(positive_rule))
        if out.pop("cursor") != M:
            raise RuntimeError(f"EvalRecord: the device cursor does not match the {M} slides the host counted")
        out.update(n=M, patients=names)
        return out

    def _summary_hip(self, ids, M, C_, P_, positive_rule):
        from . import _lib
        from .engine import _p, _stream
        dev = self.device
        with torch.cuda.device(dev):
            pid = torch.tensor(ids, dtype=torch.int32).to(dev)
            # every result in one buffer of 8-byte words, so one copy brings them all to the host
            w64 = {"nll_sum": 1, "s_w": C_, "s_n": C_, "p_w": C_, "p_n": C_, "ptarget": P_, "ppred": P_}
            w32 = {"s_cm": C_ * C_, "p_cm": C_ * C_, "nslides": P_, "stats": 2 * C_, "cursor": 1, "pscore": P_ * C_}
            off, total = {}, 0
            for k, v in w64.items():
                off[k] = (total, total + v)
                total += v
            for k, v in w32.items():
                off[k] = (total, total + (v + 1) // 2)
                total += (v + 1) // 2
            buf = torch.zeros(total, dtype=torch.int64, device=dev)

            def seg(t, k, dtype=None):
                a, b = off[k]
                s = t[a:b]
                return s if dtype is None else s.view(dtype)[:w32[k]]

            pscore = seg(buf, "pscore", torch.float32)
            st = _stream()
            _lib.call("tm_eval_patients", _p(self.prob), _p(self.y_hat), _p(self.label), _p(pid), M, C_, P_,
                      int(positive_rule), _p(pscore), _p(seg(buf, "ppred")), _p(seg(buf, "ptarget")),
                      _p(seg(buf, "nslides", torch.int32)), st)
            _lib.call("tm_eval_confusion", _p(self.y_hat), _p(self.label), M, C_, _p(seg(buf, "s_cm", torch.int32)),
                      _p(self.nll), _p(seg(buf, "nll_sum")), st)
            _lib.call("tm_eval_confusion", _p(seg(buf, "ppred")), _p(seg(buf, "ptarget")), P_, C_,
                      _p(seg(buf, "p_cm", torch.int32)), None, None, st)
            _lib.call("tm_eval_auc_pairs", _p(self.prob), _p(self.label), M, C_, _p(seg(buf, "s_w")),
                      _p(seg(buf, "s_n")), st)
            _lib.call("tm_eval_auc_pairs", _p(pscore), _p(seg(buf, "ptarget")), P_, C_, _p(seg(buf, "p_w")),
                      _p(seg(buf, "p_n")), st)
            seg(buf, "stats", torch.int32).copy_(self.class_stats.reshape(-1))
            seg(buf, "cursor", torch.int32).copy_(self.cursor)
            host = buf.cpu()        # the epoch's one device-to-host copy (and its one sync)
        return {"nll_sum": float(seg(host, "nll_sum").view(torch.float64)[0]),
                "slide_cm": seg(host, "s_cm", torch.int32).view(C_, C_).tolist(),
                "patient_cm": seg(host, "p_cm", torch.int32).view(C_, C_).tolist(),
                "slide_wins2": seg(host, "s_w").tolist(), "slide_npairs": seg(host, "s_n").tolist(),
                "patient_wins2": seg(host, "p_w").tolist(), "patient_npairs": seg(host, "p_n").tolist(),
                "patient_score": seg(host, "pscore", torch.float32).view(P_, C_).clone(),
                "patient_target": seg(host, "ptarget").clone(), "patient_pred": seg(host, "ppred").clone(),
                "nslides": seg(host, "nslides", torch.int32).tolist(),
                "class_stats": seg(host, "stats", torch.int32).view(C_, 2).tolist(),
                "cursor": int(seg(host, "cursor", torch.int32)[0])}

    def _summary_cpu(self, ids, M, C_, P_, positive_rule):
        prob, y_hat, label = self.prob[:M], self.y_hat[:M], self.label[:M]
        score = torch.zeros(P_, C_, dtype=torch.float32)
        target = torch.full((P_,), -1, dtype=torch.int64)
        nslides = [0] * P_
        rows = [[] for _ in range(P_)]
        for i, p in enumerate(ids):
            rows[p].append(i)
        for p, r in enumerate(rows):
            target[p], nslides[p] = label[r[0]], len(r)
            pos = [i for i in r if int(y_hat[i]) == 1]
            use = pos if positive_rule and pos else r
            acc = torch.zeros(C_, dtype=torch.float32)
            for i in use:               # record order, fp32
                acc = acc + prob[i]
            score[p] = acc / float(len(use))
        pred = (score[:, 1] > 0.5).long() if C_ == 2 else torch.argmax(score, dim=1)

        def confusion(pr, tg):
            cm = [[0] * C_ for _ in range(C_)]
            for a, b in zip(tg.tolist(), pr.tolist()):
                if 0 <= a < C_ and 0 <= b < C_:
                    cm[a][b] += 1
            return cm

        def pairs(s, tg):
            wins2, npairs = [], []
            for c in range(C_):
                sp, sn = s[tg == c, c], s[tg != c, c]
                gt = int((sp[:, None] > sn[None, :]).sum())
                eq = int((sp[:, None] == sn[None, :]).sum())
                wins2.append(2 * gt + eq)
                npairs.append(sp.numel() * sn.numel())
            return wins2, npairs

        s_w, s_n = pairs(prob, label)
        p_w, p_n = pairs(score, target)
        return {"nll_sum": float(self.nll[:M].double().sum()), "slide_cm": confusion(y_hat, label),
                "patient_cm": confusion(pred, target), "slide_wins2": s_w, "slide_npairs": s_n,
                "patient_wins2": p_w, "patient_npairs": p_n, "patient_score": score, "patient_target": target,
                "patient_pred": pred, "nslides": nslides, "class_stats": self.class_stats.tolist(),
                "cursor": int(self.cursor)}


def auroc_from_pairs(wins2, npairs):
    """AUROC from the one-vs-rest Mann-Whitney counts (the trapezoidal ROC area, ties counted half),
    in fp64: column 1 for two classes, else the mean over classes with a class that has no positive
    or no negative counting 0; 0.0 when the targets hold a single class (no pair at all;
    model_interface.py:500-503, 582-585)."""
    if len(wins2) < 2 or not any(npairs):
        return 0.0
    per = [w / (2.0 * n) if n else 0.0 for w, n in zip(wins2, npairs)]
    return per[1] if len(per) == 2 else sum(per) / len(per)


def metrics_from_confusion(cm, prefix=""):
    """The reference's metric collection (model_interface.py:186-209) from a confusion matrix
    ``cm[target][pred]``, in fp64 on the host: Accuracy, CohenKappa, F1Score, Recall, Precision and
    for more than two classes Specificity.  Two classes: class 1 is the positive one; more: macro
    averages over all C classes.  An empty denominator gives 0.  Keys are ``prefix`` + the
    torchmetrics class name (``BinaryF1Score`` / ``MulticlassF1Score`` ...).  torchmetrics itself is
    not available where this project runs, so parity with it is not pinned; the definitions are
    (tests/test_eval.py, against NumPy and scikit-learn)."""
    C_ = len(cm)
    n = float(sum(sum(r) for r in cm))
    rows = [float(sum(cm[c])) for c in range(C_)]                       # targets per class
    cols = [float(sum(cm[t][c] for t in range(C_))) for c in range(C_)]  # predictions per class
    diag = [float(cm[c][c]) for c in range(C_)]

    def div(a, b):
        return a / b if b else 0.0

    po = div(sum(diag), n)
    pe = div(sum(r * c for r, c in zip(rows, cols)), n * n)
    kappa = div(po - pe, 1.0 - pe)
    recall = [div(diag[c], rows[c]) for c in range(C_)]
    precision = [div(diag[c], cols[c]) for c in range(C_)]
    f1 = [div(2.0 * diag[c], rows[c] + cols[c]) for c in range(C_)]
    spec = [div(n - rows[c] - cols[c] + diag[c], n - rows[c]) for c in range(C_)]
    if C_ == 2:
        return {prefix + "BinaryAccuracy": po, prefix + "BinaryCohenKappa": kappa, prefix + "BinaryF1Score": f1[1],
                prefix + "BinaryRecall": recall[1], prefix + "BinaryPrecision": precision[1]}
    mean = lambda v: sum(v) / C_        # noqa: E731
    return {prefix + "MulticlassAccuracy": mean(recall), prefix + "MulticlassCohenKappa": kappa,
            prefix + "MulticlassF1Score": mean(f1), prefix + "MulticlassRecall": mean(recall),
            prefix + "MulticlassPrecision": mean(precision), prefix + "MulticlassSpecificity": mean(spec)}


class _EvalState:
    """One stage's record with the slide / patient names of its rows (host lists, append order)."""

    def __init__(self, record):
        self.record, self.names, self.patients = record, [], []

    def reset(self):
        self.record.reset()
        self.names, self.patients = [], []


def _is_tile_bag(bags):
    from .data import TileBag
    return isinstance(bags, TileBag)


def _model_input(bags):
    """What the model is called with: a tensor batch as fp32 contiguous; a lazy ``data.TileBag`` as
    it is (the encoder gathers it chunk by chunk in its compute dtype: no float bag here)."""
    return bags if _is_tile_bag(bags) else bags.float().contiguous()


def _refuse_tile_bag(who, bags):
    if _is_tile_bag(bags):
        raise TypeError(f"{who}: a lazy TileBag cannot be captured (its gathers are issued per chunk by the "
                        "encoder); pass materialize()d tiles, or run the eager step")


class TransMILTask(nn.Module):
    """``ModelInterface`` training / validation / test step subset for the feature-bag path."""

    def __init__(self, model: nn.Module, lr: float = 2e-4, opt: str = "lookahead_radam",
                 weight_decay: float = 0.01, loss: str = "CrossEntropyLoss", accumulate_grad_batches: int = 1):
        super().__init__()
        if accumulate_grad_batches < 1:
            raise ValueError("accumulate_grad_batches >= 1")
        self.model = model
        self.class_stats = None     # int32 [C][2] per-class count / correct (model_interface.py:350-356)
        self.accumulate_grad_batches = accumulate_grad_batches
        self._micro = 0
        self.n_classes = model.n_classes
        self.loss = create_loss(loss)
        self.lr, self.opt, self.weight_decay = lr, opt, weight_decay
        self._last_loss = None

    def forward(self, x):
        out = self.model(x)
        if isinstance(out, tuple):          # Chowder returns (logits, None), [B, 1, C] for B > 1
            out = out[0]
        if out.dim() == 3 and out.shape[1] == 1:
            out = out.view(out.shape[0], out.shape[2])
        return out

    def step(self, bags):
        logits = self(_model_input(bags))
        y_hat = torch.argmax(logits, dim=1)
        y_prob = F.softmax(logits, dim=1)
        return logits, y_prob, y_hat

    def training_step(self, batch):
        bags, label, _ = batch
        if bags.is_cuda and isinstance(self.loss, nn.CrossEntropyLoss):
            # fused: loss, Y_prob, Y_hat and the per-class count/correct of :350-356 in one launch --
            # the head's own launch where the model offers it (TransMIL.forward_ce), else tm_ce_fwd
            x = _model_input(bags)
            if self.class_stats is None or self.class_stats.device != x.device:
                self.class_stats = torch.zeros(self.n_classes, 2, dtype=torch.int32, device=x.device)
            fused = getattr(self.model, "forward_ce", None)
            if self._forward_hooks or self._forward_pre_hooks:
                fused = None            # hooks on the task run only through self(x)
            out = fused(x, label, self.class_stats) if fused is not None else None
            if out is not None:
                logits, loss, y_prob, y_hat = out
            else:
                logits = self(x)
                loss, y_prob, y_hat = _CrossEntropyOneHot.apply(logits, label, self.class_stats)
        else:
            logits, y_prob, y_hat = self.step(bags)
            one_hot = F.one_hot(label, num_classes=self.n_classes).float()
            loss = self.loss(logits, one_hot)
        self._last_outputs = (y_prob, y_hat)
        if loss.ndim == 0:
            loss = loss.unsqueeze(0)
        # the reference logs loss.item() with sync_dist every step (model_interface.py:364),
        # a host sync + scalar all-reduce per step; here the value stays on the device.
        self._last_loss = loss.detach()
        return loss

    def backward(self, loss):
        """``loss.backward()`` with the seed gradient taken from a persistent ones tensor (no
        ``ones_like`` fill launch per step; Lightning's manual_backward equivalent)."""
        one = getattr(self, "_one", None)
        if one is None or one.device != loss.device or one.shape != loss.shape:
            one = self._one = torch.ones_like(loss)
        loss.backward(one)

    def optimization_step(self, batch, opt, allreduce=None):
        """One micro-batch of Lightning's automatic optimization with
        ``accumulate_grad_batches = K`` (code/train.py:199 uses K = 10 under DDP): the closure
        loss is ``training_step / K``, backward accumulates into the gradient bucket, and only
        every K-th micro-batch all-reduces (DDP no-sync before it), steps the optimizer and
        zeroes the gradients.  Returns the un-normalised training_step loss."""
        k = self.accumulate_grad_batches
        self._micro += 1
        boundary = self._micro % k == 0
        if allreduce is not None:
            allreduce.sync = boundary
        loss = self.training_step(batch)
        self.backward(loss / k if k > 1 else loss)
        if boundary:
            if allreduce is not None:
                allreduce()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return loss

    def configure_optimizers(self):
        # the reference builds its optimizer from self.model, never from model_ft
        # (model_interface.py:862-877): an image model's encoder -- resnet18's trainable fc included --
        # is not optimised
        from .encoder import ImageBagModel
        mil = self.model.model if isinstance(self.model, ImageBagModel) else self.model
        opt = create_optimizer(mil, self.opt, self.lr, self.weight_decay)
        sched = {"scheduler": torch.optim.lr_scheduler.ReduceLROnPlateau(
            opt.base_optimizer if isinstance(opt, Lookahead) else opt, mode="min", factor=0.5),
            "monitor": "val_loss", "frequency": 10}
        return [opt], [sched]

    # ------------------------------------------------------------------ validation / test
    # validation_step / on_validation_epoch_end and test_step / on_test_epoch_end of the reference
    # (model_interface.py:432-607, 609-860) without CSV export, plots and loggers: the step appends
    # to a device-side EvalRecord (no host sync, capturable), the epoch end reduces it on the device
    # and derives every metric on the host from one small copy.

    def eval_state(self, stage: str, device=None, capacity: int = 256) -> "_EvalState":
        """The stage's ("val" / "test") record and name lists, created on first use."""
        if stage not in ("val", "test"):
            raise ValueError("stage must be 'val' or 'test'")
        states = self.__dict__.setdefault("_eval_states", {})    # created by the first evaluation call
        st = states.get(stage)
        if st is None or (device is not None and st.record.device != torch.device(device)):
            if device is None:
                device = next(self.model.parameters()).device
            st = states[stage] = _EvalState(EvalRecord(self.n_classes, capacity, device))
        return st

    def _parse_eval_batch(self, batch):
        """``(bags, label, (wsi_name, coords_or_names, patient))`` -> bags [B, N, F], the label as a
        [B] tensor (an int, a CPU or a device tensor; a CPU label outside [0, C) raises IndexError as
        ``forward_ce`` does) and the B slide / patient names as lists."""
        bags, label, meta = batch
        names, patients = meta[0], meta[-1]
        from .encoder import ImageBagModel
        nd = 5 if isinstance(self.model, ImageBagModel) else 3      # tile bags [B, N, 3, H, W]
        if _is_tile_bag(bags):
            pass                                                    # always [B, bag, 3, H, W]
        elif bags.dim() == nd - 1:
            bags = bags.unsqueeze(0)
        elif bags.dim() > nd:
            bags = bags.squeeze(0)
        B = bags.shape[0]
        if not torch.is_tensor(label):
            label = torch.as_tensor(label, dtype=torch.int64)
        label = label.reshape(-1)
        if label.numel() != B:
            raise ValueError(f"evaluation step: {label.numel()} labels for {B} bags")
        if not label.is_cuda and not (0 <= int(label.min()) and int(label.max()) < self.n_classes):
            raise IndexError(f"evaluation step: labels must lie in [0, {self.n_classes})")
        names = [names] if isinstance(names, str) else list(names)
        patients = [patients] if isinstance(patients, str) else list(patients)
        if len(names) != B or len(patients) != B:
            raise ValueError(f"evaluation step: {len(names)} slide names / {len(patients)} patients for {B} bags")
        return bags, label, names, patients

    def _eval_forward_record(self, record, bags, label):
        """The device side of an evaluation step: the forward (the model in whatever mode it is in,
        under no_grad) and the record launch.  This is what ``GraphedEvaluation`` captures."""
        with torch.no_grad():
            logits = self(_model_input(bags))
            record.write(logits.float().contiguous(), label)
        return logits

    def _eval_step(self, stage, batch):
        bags, label, names, patients = self._parse_eval_batch(batch)
        st = self.eval_state(stage, bags.device)
        with torch.no_grad():
            logits = self(_model_input(bags))
            st.record.append(logits, label.to(device=logits.device, dtype=torch.int64))
        st.names += names            # names stay on the host, in append order
        st.patients += patients
        return logits

    def validation_step(self, batch, batch_idx=None):
        """model_interface.py:432-469: forward, cross entropy, Y_prob, Y_hat and the per-class
        count / correct of one batch, appended to the validation record in one launch.  No host
        sync (with a device label): the call can be captured into a hipGraph.  Returns the logits."""
        return self._eval_step("val", batch)

    def test_step(self, batch, batch_idx=None):
        """model_interface.py:609-660 without the top-k tile bookkeeping; as ``validation_step``."""
        return self._eval_step("test", batch)

    def on_validation_epoch_start(self):
        self.eval_state("val").reset()

    def on_test_epoch_start(self):
        self.eval_state("test").reset()

    def _gathered(self, st, group):
        """The ranks' records and name lists as one record in rank order (every rank builds the same
        one): counts and names first (all_gather_object), then logits and labels padded to the
        longest rank; the rows are re-derived from the gathered logits by the same launch."""
        world = dist.get_world_size(group)
        rec = st.record
        if rec.n > rec.capacity:
            raise RuntimeError(f"EvalRecord: {rec.n} slides appended to a pinned record of capacity {rec.capacity}")
        meta = [None] * world
        dist.all_gather_object(meta, (rec.n, st.names, st.patients), group=group)
        counts = [m[0] for m in meta]
        width = max(max(counts), 1)
        lg = torch.zeros(width, rec.n_classes, dtype=torch.float32, device=rec.device)
        lb = torch.zeros(width, dtype=torch.int64, device=rec.device)
        lg[:rec.n].copy_(rec.logits[:rec.n])
        lb[:rec.n].copy_(rec.label[:rec.n])
        lgs = [torch.empty_like(lg) for _ in range(world)]
        lbs = [torch.empty_like(lb) for _ in range(world)]
        dist.all_gather(lgs, lg, group=group)
        dist.all_gather(lbs, lb, group=group)
        merged = _EvalState(EvalRecord(rec.n_classes, max(sum(counts), 1), rec.device))
        for r, c in enumerate(counts):
            if c:
                merged.record.append(lgs[r][:c], lbs[r][:c])
                merged.names += list(meta[r][1])
                merged.patients += list(meta[r][2])
        return merged

    def _eval_epoch_end(self, stage, group=None):
        st = self.eval_state(stage)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            st = self._gathered(st, group)
        C_ = self.n_classes
        s = st.record.summary(st.patients, positive_rule=(stage == "val" and C_ == 2))   # :539-544 (val only)
        out = {f"{stage}_loss": s["nll_sum"] / s["n"],
               f"{stage}_auc": auroc_from_pairs(s["slide_wins2"], s["slide_npairs"]),
               f"{stage}_patient_auc": auroc_from_pairs(s["patient_wins2"], s["patient_npairs"])}
        if stage == "test":
            out.update(metrics_from_confusion(s["slide_cm"], "test_"))              # :689
        out.update(metrics_from_confusion(s["patient_cm"], f"{stage}_patient"))     # :587, :841
        if stage == "val":
            P_ = len(s["patients"])
            out["val_accuracy"] = sum(s["patient_cm"][c][c] for c in range(C_)) / float(P_)   # :590
        out["class_acc"] = [(correct / count if count else None) for count, correct in s["class_stats"]]
        out["patient_score"] = s["patient_score"]
        out["patient_target"] = s["patient_target"]
        out["patients"] = s["patients"]
        out["slides"] = list(st.names)
        return out

    def on_validation_epoch_end(self, group=None):
        """model_interface.py:472-607 as a returned dict instead of ``self.log`` calls: Python floats
        ``val_loss``, ``val_auc``, ``val_patient_auc``, ``val_accuracy`` (patient level, :590) and the
        ``val_patient*`` collection, plus ``patient_score`` [P, C], ``patient_target``, ``patients``
        (names in first-appearance order), ``slides`` and ``class_acc``.

        ``val_loss`` is the mean nll over the recorded slides.  The reference logs a per-step value
        that Lightning averages with ``batch_size=1``, and its evaluation loaders use batch 1, so the
        two agree there.  AUROC is the Mann-Whitney pair count with ties counted half; the metric
        collection comes from the confusion matrices (``metrics_from_confusion``).  Parity with
        torchmetrics itself is not pinned (the package is absent where this project runs); the
        definitions are pinned by tests/test_eval.py.

        With a process group of world > 1 every rank all-gathers the ranks' records and names and
        computes the same global metrics over the union in rank order.  This deviates from the
        reference, which averages per-rank metrics through ``sync_dist``; it keeps ``val_loss`` --
        and so the ReduceLROnPlateau scheduler -- identical on all ranks."""
        return self._eval_epoch_end("val", group)

    def on_test_epoch_end(self, group=None):
        """model_interface.py:662-860 without CSV / plots / top-k: ``test_loss``, ``test_auc``,
        ``test_patient_auc``, the slide-level ``test_*`` and patient-level ``test_patient*``
        collections (patient score: the plain mean over the patient's slides), and the same extra
        entries as ``on_validation_epoch_end`` (see there for the definitions and the DDP rule)."""
        return self._eval_epoch_end("test", group)


class GraphedOptimizationStep:
    """``TransMILTask.optimization_step`` replayed as captured hipGraphs: each micro-batch (forward,
    fused CE, backward into the gradient bucket; on the accumulation boundary also the all-reduce
    and the optimizer step) is ONE graph launch instead of ~100 host-issued kernel launches -- the
    execution ``bench.py`` times, offered to training loops (a graph in place of a tracing
    compiler; an eager step is host-bound at ~2.2 ms on the bench shape against 1.2 ms replayed).

    The first ``accumulate_grad_batches`` micro-batches run eagerly through
    ``task.optimization_step`` (they are real steps: they also create the optimizer state and the
    engine's buffers); then one graph per accumulation phase (``first`` writes the gradients,
    ``mid`` adds, ``last`` adds, all-reduces and steps -- with K = 1 only ``last``, which writes)
    is captured over static input buffers, and every later call copies the batch in and replays
    the phase's graph.  Capture records, it does not execute, so the sequence of updates is the
    eager one (``tests/test_interface.py``: parameters bitwise equal to ``optimization_step``).
    Dropout keeps drawing fresh masks: its counter lives on the device.

    One bag shape per instance (the reference's loaders sample bags to a fixed size); a batch of
    another shape raises.  Returns the training_step loss tensor of the replayed graph (a static
    buffer: it is overwritten by the next call of the same phase); the eager window's calls return
    their loss detached (the step has run; see ``__call__``).

    Learning rate / weight decay: with ``FusedRAdamLookahead`` the replayed update reads them from
    a device array refreshed from the param groups before every replayed optimizer step, so an LR
    scheduler keeps working; any other optimizer bakes the captured values into the graph, and a
    change of a group's lr / weight_decay after the capture raises instead of being ignored.
    ``lookahead_step`` of every group advances per replayed optimizer step as in the eager path."""

    def __init__(self, task: "TransMILTask", opt, allreduce=None):
        self.task, self.opt, self.allreduce = task, opt, allreduce
        self.k = task.accumulate_grad_batches
        self.graphs = None
        self.shape = None

    def _phase(self, micro):
        k = self.k
        return "last" if micro % k == 0 else ("first" if micro % k == 1 else "mid")

    def _capture(self, bags, label):
        task, opt, ar, k = self.task, self.opt, self.allreduce, self.k
        self.x = bags.detach().clone()
        self.y = label.detach().clone()
        self.loss = {}

        def body(phase):
            if ar is not None:
                ar.sync = phase == "last"
            loss = task.training_step((self.x, self.y, None))
            task.backward(loss / k if k > 1 else loss)
            if phase == "last":
                if ar is not None:
                    ar()
                opt.step()
            return loss

        self._fingerprint = self._hyper_fingerprint()
        la_steps = [g.get("lookahead_step") for g in opt.param_groups]   # capture runs opt.step()'s host side
        pool = torch.cuda.graph_pool_handle()
        self.graphs = {}
        opt.zero_grad(set_to_none=True)        # the first capture takes the writing (=) path,
        for ph in (["last"] if k == 1 else (["first", "mid", "last"] if k > 2 else ["first", "last"])):
            g = torch.cuda.CUDAGraph()          # the ones after it the accumulating (+=) path
            with torch.cuda.graph(g, pool=pool):
                self.loss[ph] = body(ph)
            self.graphs[ph] = g
        for grp, v in zip(opt.param_groups, la_steps):     # ... without a step having run
            if v is not None:
                grp["lookahead_step"] = v

    def _hyper_fingerprint(self):
        return [(g.get("lr"), g.get("weight_decay")) for g in self.opt.param_groups]

    def _before_step_replay(self):
        """The host side of opt.step() that a replay does not run: the fused optimizer's device
        hyper-parameters, the groups' lookahead_step counters; a non-fused optimizer whose lr /
        weight decay changed since the capture raises (its graph holds the old values)."""
        opt = self.opt
        refresh = getattr(opt, "refresh_hyper", None)
        if refresh is not None:
            refresh()
        elif self._hyper_fingerprint() != self._fingerprint:
            raise RuntimeError("GraphedOptimizationStep: lr / weight_decay changed after the capture, and "
                               f"{type(opt).__name__} bakes them into the captured graph (use FusedRAdamLookahead, "
                               "or build a new GraphedOptimizationStep)")
        for g in opt.param_groups:
            if "lookahead_step" in g:
                g["lookahead_step"] += 1

    def close(self):
        """Release the captured graphs, then the all-reduce (``GradAllReduce.close``): a graph
        captured over the RCCL all-reduce holds the communicator's kernels and registered
        buffers, so it must be gone -- destroyed and drained -- before
        ``dist.destroy_process_group()``.  Later calls raise."""
        if self.graphs:
            torch.cuda.synchronize()            # no replay in flight
            for g in self.graphs.values():
                g.reset()
            torch.cuda.synchronize()
        self.graphs, self.loss = None, {}
        self._closed = True
        if self.allreduce is not None:
            self.allreduce.close()

    def __call__(self, batch):
        if getattr(self, "_closed", False):
            raise RuntimeError("GraphedOptimizationStep: called after close()")
        bags, label = batch[0], batch[1]
        _refuse_tile_bag("GraphedOptimizationStep", bags)
        task = self.task
        if self.graphs is None:
            if self.shape is None:
                self.shape = (tuple(bags.shape), tuple(label.shape))
            # The eager steps' losses are returned detached, so that their autograd graphs are gone
            # before the capture.  While such a graph lives, the parameters keep its AccumulateGrad
            # nodes, which are bound to the stream the eager step ran on; a captured backward that
            # reaches them (a model whose gradients autograd accumulates, unlike TransMIL's fused
            # backward) would make that stream wait on the capturing one.
            loss = task.optimization_step(batch, self.opt, allreduce=self.allreduce).detach()
            if task._micro % self.k == 0:        # the eager window is complete: capture
                self._capture(bags, label)
            return loss
        if (tuple(bags.shape), tuple(label.shape)) != self.shape:
            raise ValueError(f"GraphedOptimizationStep was captured for bags {self.shape[0]} and labels "
                             f"{self.shape[1]}, got {tuple(bags.shape)} / {tuple(label.shape)}")
        task._micro += 1
        ph = self._phase(task._micro)
        if ph == "last":
            self._before_step_replay()
        self.x.copy_(bags)
        self.y.copy_(label)
        self.graphs[ph].replay()
        return self.loss[ph]


class GraphedEvaluation:
    """``TransMILTask.validation_step`` / ``test_step`` replayed as captured hipGraphs, one per bag
    shape.  Evaluation bags are small and differ in size per slide (ceil(0.1 n) tiles), so a forward
    is bound by launch and host time; the same slides return every epoch, so a graph captured for
    a shape is replayed from then on.  Same call contract as the step.

    The first time a ``(bags.shape, B)`` is seen the step runs eagerly (it also creates whatever the
    model caches per shape); the second time the forward plus the record launch are captured over
    static input / label buffers on one stream and replayed; every later call copies the batch in
    and replays.  The record's device cursor makes the captured step position-independent.  At most
    ``max_graphs`` graphs are kept (least recently used out first, ``graph.reset()``).  If any
    parameter's ``data_ptr`` changed since the captures, all graphs are dropped and built again
    (in-place optimizer updates do not move parameters, so training between epochs keeps them).

    The record gets ``capacity`` rows up front and is pinned: captured launches hold its addresses,
    so it cannot grow; an epoch longer than ``capacity`` raises at the epoch end.  Returns the
    step's logits (a replay returns the graph's static output, overwritten by the next replay of
    the same shape)."""

    def __init__(self, task: "TransMILTask", stage: str = "val", capacity: int = 4096, max_graphs: int = 64):
        if max_graphs < 1:
            raise ValueError("GraphedEvaluation: max_graphs >= 1")
        self.task, self.stage, self.max_graphs = task, stage, max_graphs
        device = next(task.model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("GraphedEvaluation needs the model on a GPU")
        old = task.__dict__.get("_eval_states", {}).pop(stage, None)
        if old is not None and old.record._pins:
            raise RuntimeError(f"GraphedEvaluation: another instance holds the '{stage}' record")
        self.state = task.eval_state(stage, device, capacity)
        self.state.record.pin()
        self.graphs = {}        # key -> (graph, static bags, static label, logits), in LRU order
        self.seen = set()
        self._pool = None
        self._ptrs = None
        self._closed = False

    def _param_ptrs(self):
        return tuple(p.data_ptr() for p in self.task.model.parameters())

    def _drop(self, keys):
        if not keys:
            return
        torch.cuda.synchronize()                # no replay in flight
        for k in keys:
            self.graphs.pop(k)[0].reset()
        torch.cuda.synchronize()

    def close(self):
        """Release the captured graphs and unpin the record.  Later calls raise."""
        if self._closed:
            return
        self._drop(list(self.graphs))
        self.state.record.unpin()
        self._closed = True

    def live_graphs(self):
        return len(self.graphs)

    def __call__(self, batch, batch_idx=None):
        _refuse_tile_bag("GraphedEvaluation", batch[0])
        if self._closed:
            raise RuntimeError("GraphedEvaluation: called after close()")
        task, st = self.task, self.state
        if task.eval_state(self.stage) is not st:
            raise RuntimeError("GraphedEvaluation: the task's record was replaced after the captures")
        bags, label, names, patients = task._parse_eval_batch(batch)
        rec = st.record
        ptrs = self._param_ptrs()
        if ptrs != self._ptrs:                  # parameters moved: every graph reads stale addresses
            self._drop(list(self.graphs))
            self.seen.clear()
            self._ptrs = ptrs
        key = (tuple(bags.shape), bags.dtype)
        hit = self.graphs.pop(key, None)
        if hit is None and key not in self.seen:
            self.seen.add(key)
            return task._eval_step(self.stage, (bags, label, (names, None, patients)))
        if hit is None:
            x = bags.detach().clone()
            y = label.to(device=x.device, dtype=torch.int64).clone()
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool):
                logits = task._eval_forward_record(rec, x, y)
            hit = (g, x, y, logits)
        else:
            hit[1].copy_(bags)
            hit[2].copy_(label)
        self.graphs[key] = hit                  # most recently used last
        hit[0].replay()
        rec.n += bags.shape[0]
        st.names += names
        st.patients += patients
        if len(self.graphs) > self.max_graphs:
            self._drop(list(self.graphs)[:len(self.graphs) - self.max_graphs])
        return hit[3]
