"""Validation / test steps on the GPU: tm_eval_record and the epoch kernels against the fp64
restatement of tests/test_eval.py, the task end to end on TransMIL, and hipGraph capture."""
import numpy as np
import pytest
import torch

from test_eval import (assert_epoch_equal, ref_class_stats, ref_confusion, ref_epoch, ref_pairs, ref_patients,
                       ref_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------- tm_eval_record
@pytest.mark.parametrize("B,C", [(1, 2), (3, 3), (5, 7)])
def test_eval_record_rows(B, C):
    from transmil_deepgraft_amd.interface import EvalRecord
    g = torch.Generator().manual_seed(B * 10 + C)
    rec = EvalRecord(C, capacity=4 * B, device=DEV)
    logits = torch.randn(3 * B, C, generator=g) * 3
    logits[1] = logits[0]
    if C > 2:
        logits[2, 1] = logits[2, 2] = logits[2].max() + 1.0      # a tied maximum: the first index wins
    label = torch.randint(0, C, (3 * B,), generator=g)
    for k in range(3):
        rec.append(logits[k * B:(k + 1) * B].to(DEV), label[k * B:(k + 1) * B].to(DEV))
    M = 3 * B
    prob, y_hat, nll = ref_rows(logits.numpy(), label.numpy())
    assert int(rec.cursor.cpu()) == M and rec.n == M
    assert torch.equal(rec.logits[:M].cpu(), logits) and torch.equal(rec.label[:M].cpu(), label)
    np.testing.assert_allclose(rec.prob[:M].cpu().numpy(), prob, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rec.nll[:M].cpu().numpy(), nll, rtol=1e-6, atol=1e-6)
    assert rec.y_hat[:M].cpu().tolist() == y_hat.tolist()
    assert rec.class_stats.cpu().tolist() == ref_class_stats(y_hat, label.numpy(), C).tolist()
    assert float(rec.logits[M:].abs().sum()) == 0.0            # rows past the cursor untouched


def test_eval_record_out_of_range_label():
    from transmil_deepgraft_amd.interface import EvalRecord
    rec = EvalRecord(3, capacity=4, device=DEV)
    rec.append(torch.tensor([[1.0, 2.0, 0.0], [0.5, 0.0, 0.1]], device=DEV), torch.tensor([7, -1], device=DEV))
    rec.append(torch.tensor([[1.0, 2.0, 0.0]], device=DEV), torch.tensor([1], device=DEV))
    assert torch.isnan(rec.nll[:2]).all() and not torch.isnan(rec.nll[2])
    assert rec.class_stats.cpu().tolist() == [[0, 0], [1, 1], [0, 0]]
    assert rec.label[:3].cpu().tolist() == [7, -1, 1]


def test_eval_record_overflow_drops_rows_and_keeps_counting():
    """Capacity 4, two appends of 3 on pinned storage: rows 0-3 written, nothing behind any raw
    buffer touched, the cursor reads 6, summary() raises."""
    from transmil_deepgraft_amd.interface import EvalRecord
    C, cap, tail = 3, 4, 8
    rec = EvalRecord(C, capacity=cap, device=DEV)
    rec.pin()
    canary = {}
    for f in EvalRecord._FIELDS:        # raw buffers with a canary tail behind the record's rows
        old = getattr(rec, f)
        raw = torch.full((cap + tail,) + tuple(old.shape[1:]), 77, dtype=old.dtype, device=DEV)
        canary[f] = raw
        setattr(rec, f, raw[:cap])
    logits = torch.randn(6, C, generator=torch.Generator().manual_seed(1))
    label = torch.tensor([0, 1, 2, 0, 1, 2])
    rec.append(logits[:3].to(DEV), label[:3].to(DEV))
    rec.append(logits[3:].to(DEV), label[3:].to(DEV))
    assert int(rec.cursor.cpu()) == 6 and rec.n == 6 and rec.capacity == cap
    prob, y_hat, nll = ref_rows(logits.numpy(), label.numpy())
    assert torch.equal(rec.logits.cpu(), logits[:4])
    np.testing.assert_allclose(rec.prob.cpu().numpy(), prob[:4], rtol=1e-6, atol=1e-7)
    assert rec.y_hat.cpu().tolist() == y_hat[:4].tolist() and rec.label.cpu().tolist() == label[:4].tolist()
    for f, raw in canary.items():
        assert bool((raw[cap:] == 77).all()), f
    assert rec.class_stats.cpu()[:, 0].tolist() == [2, 2, 2]          # the stats still count every bag
    with pytest.raises(RuntimeError, match="capacity"):
        rec.summary(["p"] * 6)


# ---------------------------------------------------------------------------- epoch kernels
@pytest.mark.parametrize("P", [1, 3, 40])
@pytest.mark.parametrize("M", [1, 2, 7, 257, 300])
@pytest.mark.parametrize("C", [2, 3])
def test_epoch_kernels(M, P, C):
    from transmil_deepgraft_amd.interface import EvalRecord
    rng = np.random.default_rng(M * 100 + P * 3 + C)
    logits = torch.from_numpy(np.round(rng.normal(size=(M, C)) * 2).astype(np.float32) / 2)   # coarse: exact ties
    label = torch.from_numpy(rng.integers(0, C, M))
    if M >= 2:      # an exact tie between a positive and a negative of classes 0 and 1
        logits[1] = logits[0]
        label[0], label[1] = 0, 1
    pid = rng.integers(0, min(P, M), M)
    pid[:min(P, M)] = rng.permutation(min(P, M))
    patients = [f"p{i}" for i in pid]
    rec = EvalRecord(C, capacity=M, device=DEV)
    rec.append(logits.to(DEV), label.to(DEV))
    p32 = rec.prob[:M].cpu().numpy()
    y_hat = rec.y_hat[:M].cpu().numpy()
    lab = label.numpy()
    for rule in (False, True):
        s = rec.summary(patients, positive_rule=rule)
        names, score, pred, target, nslides = ref_patients(p32, y_hat, lab, patients, rule)
        assert s["patients"] == names and s["nslides"] == nslides.tolist()
        assert s["patient_target"].tolist() == target.tolist()          # the first slide's label
        assert np.abs(s["patient_score"].double().numpy() - score).max() <= 1e-6
        # the integer results, on the recorded fp32 values
        assert (s["slide_wins2"], s["slide_npairs"]) == ref_pairs(p32, lab, C)
        got_score = s["patient_score"].numpy()
        assert (s["patient_wins2"], s["patient_npairs"]) == ref_pairs(got_score, target, C)
        assert s["slide_cm"] == ref_confusion(y_hat, lab, C).tolist()
        got_pred = (got_score[:, 1] > 0.5).astype(np.int64) if C == 2 else got_score.argmax(axis=1)
        assert s["patient_pred"].tolist() == got_pred.tolist()
        assert s["patient_cm"] == ref_confusion(got_pred, target, C).tolist()
        nll = ref_rows(logits.numpy(), lab)[2]
        assert abs(s["nll_sum"] - nll.sum()) <= 1e-6 * (np.abs(nll).sum() + M)     # the rows' rtol / atol, summed
        assert s["class_stats"] == ref_class_stats(y_hat, lab, C).tolist()
    if M >= 2:
        lab_ties = sum(int((p32[lab == c, c][:, None] == p32[lab != c, c][None, :]).sum()) for c in range(C))
        assert lab_ties > 0, "the scores must hold exact ties"


# ---------------------------------------------------------------------------- end to end
def _model(C, dtype):
    from transmil_deepgraft_amd.models import TransMIL
    torch.manual_seed(C)
    return TransMIL(C, 512).to(DEV).eval().set_compute_dtype(dtype)


_BAGS = {}


def _bags():
    """Four B = 1 bags of N in {1, 3, 100, 257} and one B = 2, N = 100 batch (made once)."""
    if not _BAGS:
        g = torch.Generator().manual_seed(11)
        _BAGS["x"] = [torch.rand(1, n, 512, generator=g).to(DEV) for n in (1, 3, 100, 257)] + \
                     [torch.rand(2, 100, 512, generator=g).to(DEV)]
    return _BAGS["x"]


def _eval_batches(C):
    label = [0, 1, C - 1, 1, 0, C - 1]
    patients = ["a", "b", "a", "c", "b", "c"]
    out, i = [], 0
    for x in _bags():
        b = x.shape[0]
        lab = torch.tensor(label[i:i + b])
        if b == 1:
            out.append((x, int(lab[0]) if i % 2 else lab.to(DEV), (f"s{i}", None, patients[i])))
        else:
            out.append((x, lab, ([f"s{j}" for j in range(i, i + b)], None, patients[i:i + b])))
        i += b
    return out, label, patients


@pytest.mark.parametrize("C,dtype,stage", [(2, torch.float32, "val"), (2, torch.float32, "test"),
                                           (3, torch.float32, "val"), (3, torch.float32, "test"),
                                           (2, torch.bfloat16, "val")])
def test_task_end_to_end(C, dtype, stage):
    from transmil_deepgraft_amd.interface import TransMILTask
    model = _model(C, dtype)
    task = TransMILTask(model)
    batches, label, patients = _eval_batches(C)
    (task.on_validation_epoch_start if stage == "val" else task.on_test_epoch_start)()
    for i, b in enumerate(batches):
        (task.validation_step if stage == "val" else task.test_step)(b, i)
    got = (task.on_validation_epoch_end if stage == "val" else task.on_test_epoch_end)()
    with torch.no_grad():
        logits = torch.cat([model(b[0]) for b in batches]).float()
    rec = task.eval_state(stage).record
    assert rec.n == 6
    assert torch.equal(rec.logits[:6], logits)                  # bitwise
    want, names, score, target = ref_epoch(stage, logits.cpu().numpy(), label, patients, C,
                                           rec.prob[:6].cpu().numpy())
    assert_epoch_equal(got, want, names, score, target)
    assert got["slides"] == [f"s{i}" for i in range(6)]


# ---------------------------------------------------------------------------- capture
def test_validation_step_captures_into_a_graph():
    """The step has no host sync: it captures into a hipGraph, and each replay appends at the
    device cursor."""
    from transmil_deepgraft_amd.interface import TransMILTask
    model = _model(2, torch.float32)
    task = TransMILTask(model)
    x = _bags()[2].clone()
    y = torch.tensor([1], device=DEV)
    batch = (x, y, ("s", None, "p"))
    task.validation_step(batch)                     # eager once: creates the record and the caches
    rec = task.eval_state("val").record
    eager_row = (rec.logits[0].clone(), rec.prob[0].clone(), rec.nll[0].clone())
    task.on_validation_epoch_start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        task.validation_step(batch)
    task.on_validation_epoch_start()                # a capture executes nothing; start from row 0
    x2 = _bags()[2].flip(1).contiguous()
    for k, src in enumerate((_bags()[2], x2, _bags()[2])):
        x.copy_(src)
        graph.replay()
    torch.cuda.synchronize()
    assert int(rec.cursor.cpu()) == 3
    assert rec.class_stats.cpu()[1, 0].item() == 3
    for row in (0, 2):
        assert torch.equal(rec.logits[row], eager_row[0]) and torch.equal(rec.prob[row], eager_row[1])
        assert torch.equal(rec.nll[row], eager_row[2])
    with torch.no_grad():
        assert torch.equal(rec.logits[1], model(x2)[0])
    graph.reset()


def _graphed_epoch(ge, task, shapes, bags):
    task.on_validation_epoch_start()
    for i, n in enumerate(shapes):
        ge((bags[n], torch.tensor([i % 2]), (f"s{i}", None, f"p{i % 3}")), i)
    rec = task.eval_state("val").record
    m = len(shapes)
    out = task.on_validation_epoch_end()
    return [getattr(rec, f)[:m].clone() for f in rec._FIELDS], out


def _eager_epoch(task, shapes, bags):
    task.on_validation_epoch_start()
    for i, n in enumerate(shapes):
        task.validation_step((bags[n], torch.tensor([i % 2]), (f"s{i}", None, f"p{i % 3}")), i)
    rec = task.eval_state("val").record
    m = len(shapes)
    out = task.on_validation_epoch_end()
    return [getattr(rec, f)[:m].clone() for f in rec._FIELDS], out


def _same(a, b):
    return all(torch.equal(x, y) or (x.is_floating_point() and torch.equal(x.isnan(), y.isnan())
                                     and torch.equal(x.nan_to_num(), y.nan_to_num())) for x, y in zip(a, b))


def test_graphed_evaluation_epochs_are_bitwise_equal():
    from transmil_deepgraft_amd.interface import GraphedEvaluation, TransMILTask
    model = _model(2, torch.float32)
    task = TransMILTask(model)
    g = torch.Generator().manual_seed(5)
    bags = {n: torch.rand(1, n, 512, generator=g).to(DEV) for n in (3, 100, 257)}
    shapes = [3, 100, 3, 257]
    ge = GraphedEvaluation(task, "val", capacity=16, max_graphs=8)
    try:
        # epoch 1: 3 eager, 100 eager, 3 captured, 257 eager; epoch 2: replay, capture, replay, capture;
        # epoch 3: replays only
        rows1, out1 = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 1
        rows2, out2 = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 3
        rows3, out3 = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 3
        assert _same(rows1, rows2) and _same(rows1, rows3)
        for k, v in out1.items():
            if isinstance(v, float):
                assert v == out2[k] == out3[k], k
        with torch.no_grad():
            want = torch.cat([model(bags[n]) for n in shapes])
        assert torch.equal(rows3[0], want)

        # in-place parameter updates do not move parameters: the graphs read the new values
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.01)
        rows4, out4 = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 3
    finally:
        ge.close()
    fresh = TransMILTask(model)
    rows5, out5 = _eager_epoch(fresh, shapes, bags)
    assert _same(rows4, rows5) and not torch.equal(rows4[0], rows3[0])
    assert out4["val_loss"] == out5["val_loss"]
    with pytest.raises(RuntimeError, match="close"):
        ge((bags[3], torch.tensor([0]), ("s", None, "p")))


def test_graphed_evaluation_lru_eviction():
    from transmil_deepgraft_amd.interface import GraphedEvaluation, TransMILTask
    model = _model(2, torch.float32)
    g = torch.Generator().manual_seed(6)
    bags = {n: torch.rand(1, n, 512, generator=g).to(DEV) for n in (3, 100, 257)}
    shapes = [3, 100, 257, 3, 100, 257]
    rows_eager, out_eager = _eager_epoch(TransMILTask(model), shapes, bags)
    task = TransMILTask(model)
    ge = GraphedEvaluation(task, "val", capacity=16, max_graphs=2)
    try:
        for _ in range(3):
            rows, out = _graphed_epoch(ge, task, shapes, bags)
            assert ge.live_graphs() <= 2
            assert _same(rows, rows_eager)
            assert out["val_loss"] == out_eager["val_loss"] and out["val_auc"] == out_eager["val_auc"]
        assert ge.live_graphs() == 2
    finally:
        ge.close()
    assert ge.live_graphs() == 0


def test_graphed_evaluation_overflow_raises_at_epoch_end():
    from transmil_deepgraft_amd.interface import GraphedEvaluation, TransMILTask
    model = _model(2, torch.float32)
    task = TransMILTask(model)
    x = _bags()[1]
    ge = GraphedEvaluation(task, "val", capacity=2)
    try:
        task.on_validation_epoch_start()
        for i in range(3):
            ge((x, torch.tensor([i % 2]), (f"s{i}", None, "p")))
        with pytest.raises(RuntimeError, match="capacity"):
            task.on_validation_epoch_end()
    finally:
        ge.close()


def test_graphed_evaluation_recaptures_when_parameters_move():
    """A parameter whose storage moved (data_ptr changed) invalidates every graph: the next calls
    run eagerly, then capture again, and the results follow the new values."""
    from transmil_deepgraft_amd.interface import GraphedEvaluation, TransMILTask
    model = _model(2, torch.float32)
    task = TransMILTask(model)
    g = torch.Generator().manual_seed(7)
    bags = {n: torch.rand(1, n, 512, generator=g).to(DEV) for n in (3, 100)}
    shapes = [3, 100, 3, 100]
    ge = GraphedEvaluation(task, "val", capacity=8)
    try:
        rows1, _ = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 2
        with torch.no_grad():
            for p in model.parameters():
                p.data = p.data * 1.01          # new storage
        rows2, out2 = _graphed_epoch(ge, task, shapes, bags)
        assert ge.live_graphs() == 2            # dropped, seen eagerly, captured again
        rows3, out3 = _graphed_epoch(ge, task, shapes, bags)
    finally:
        ge.close()
    rows_eager, out_eager = _eager_epoch(TransMILTask(model), shapes, bags)
    assert _same(rows2, rows_eager) and _same(rows3, rows_eager) and not torch.equal(rows1[0], rows2[0])
    assert out2["val_loss"] == out3["val_loss"] == out_eager["val_loss"]
