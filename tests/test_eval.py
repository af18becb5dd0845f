"""Validation / test steps and the epoch metrics, without a GPU: EvalRecord on CPU tensors, the
task with a stub model, two gloo ranks, and the argument checks of the HIP entry points.

The reference of every check is the NumPy fp64 restatement below of the rules in
``include/transmil_hip.h`` (evaluation record section) and ``TransMILTask.on_validation_epoch_end``;
scikit-learn cross-checks the metric definitions where it imports."""
import os
import socket

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------- fp64 restatement
def ref_rows(logits, label):
    """Record rows from logits [M, C] and labels [M]: prob, y_hat, nll (fp64)."""
    lg = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(label, dtype=np.int64)
    m = lg.max(axis=1, keepdims=True)
    e = np.exp(lg - m)
    s = e.sum(axis=1, keepdims=True)
    prob = e / s
    lse = (m + np.log(s))[:, 0]
    y_hat = lg.argmax(axis=1)                 # first index of the maximum
    C = lg.shape[1]
    ok = (lab >= 0) & (lab < C)
    nll = np.where(ok, lse - lg[np.arange(len(lab)), np.clip(lab, 0, C - 1)], np.nan)
    return prob, y_hat, nll


def ref_class_stats(y_hat, label, C):
    st = np.zeros((C, 2), dtype=np.int64)
    for h, y in zip(y_hat, label):
        if 0 <= y < C:
            st[y, 0] += 1
            st[y, 1] += int(h == y)
    return st


def ref_patients(prob, y_hat, label, patients, positive_rule):
    """Per patient in first-appearance order: names, score [P, C], pred, target, nslides."""
    prob = np.asarray(prob, dtype=np.float64)
    C = prob.shape[1]
    order, rows = [], {}
    for i, p in enumerate(patients):
        if p not in rows:
            rows[p] = []
            order.append(p)
        rows[p].append(i)
    score = np.zeros((len(order), C))
    pred = np.zeros(len(order), dtype=np.int64)
    target = np.zeros(len(order), dtype=np.int64)
    nslides = np.zeros(len(order), dtype=np.int64)
    for k, p in enumerate(order):
        r = rows[p]
        pos = [i for i in r if y_hat[i] == 1]
        use = pos if (positive_rule and pos) else r
        score[k] = prob[use].sum(axis=0) / len(use)
        target[k] = label[r[0]]
        nslides[k] = len(r)
        pred[k] = int(score[k, 1] > 0.5) if C == 2 else int(score[k].argmax())
    return order, score, pred, target, nslides


def ref_confusion(pred, target, C):
    cm = np.zeros((C, C), dtype=np.int64)
    for p, t in zip(pred, target):
        if 0 <= t < C and 0 <= p < C:
            cm[t, p] += 1
    return cm


def ref_pairs(scores, target, C):
    """One-vs-rest (wins2, npairs) per class over every (positive, negative) pair."""
    scores = np.asarray(scores, dtype=np.float64)
    target = np.asarray(target)
    wins2, npairs = [], []
    for c in range(C):
        sp, sn = scores[target == c, c], scores[target != c, c]
        gt = int((sp[:, None] > sn[None, :]).sum())
        eq = int((sp[:, None] == sn[None, :]).sum())
        wins2.append(2 * gt + eq)
        npairs.append(len(sp) * len(sn))
    return wins2, npairs


def ref_auc(wins2, npairs):
    C = len(wins2)
    if C < 2 or not any(npairs):
        return 0.0
    per = [w / (2.0 * n) if n else 0.0 for w, n in zip(wins2, npairs)]
    return per[1] if C == 2 else float(np.mean(per))


def ref_collection(cm, prefix):
    cm = np.asarray(cm, dtype=np.float64)
    C = cm.shape[0]
    n = cm.sum()
    rows, cols, diag = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)

    def div(a, b):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)

    po = float(div(diag.sum(), n))
    pe = float(div((rows * cols).sum(), n * n))
    kappa = float(div(po - pe, 1.0 - pe))
    rec, prec = div(diag, rows), div(diag, cols)
    f1 = div(2 * diag, rows + cols)
    spec = div(n - rows - cols + diag, n - rows)
    if C == 2:
        return {prefix + "BinaryAccuracy": po, prefix + "BinaryCohenKappa": kappa,
                prefix + "BinaryF1Score": float(f1[1]), prefix + "BinaryRecall": float(rec[1]),
                prefix + "BinaryPrecision": float(prec[1])}
    return {prefix + "MulticlassAccuracy": float(rec.mean()), prefix + "MulticlassCohenKappa": kappa,
            prefix + "MulticlassF1Score": float(f1.mean()), prefix + "MulticlassRecall": float(rec.mean()),
            prefix + "MulticlassPrecision": float(prec.mean()), prefix + "MulticlassSpecificity": float(spec.mean())}


def ref_epoch(stage, logits, label, patients, C, recorded_prob=None):
    """The whole epoch-end dict from logits.  ``recorded_prob``: the fp32 probabilities the record
    holds, used in place of the fp64 softmax for everything that compares scores exactly."""
    prob64, y_hat, nll = ref_rows(logits, label)
    prob = prob64 if recorded_prob is None else np.asarray(recorded_prob, dtype=np.float64)
    label = np.asarray(label, dtype=np.int64)
    names, score, pred, target, _ = ref_patients(prob, y_hat, label, patients, stage == "val" and C == 2)
    out = {f"{stage}_loss": float(nll.sum() / len(nll)),
           f"{stage}_auc": ref_auc(*ref_pairs(prob, label, C)),
           f"{stage}_patient_auc": ref_auc(*ref_pairs(score, target, C))}
    if stage == "test":
        out.update(ref_collection(ref_confusion(y_hat, label, C), "test_"))
    pcm = ref_confusion(pred, target, C)
    out.update(ref_collection(pcm, f"{stage}_patient"))
    if stage == "val":
        out["val_accuracy"] = float(np.trace(pcm) / len(names))
    return out, names, score, target


def assert_epoch_equal(got, want, names, score, target, tol=1e-12, loss_tol=1e-6):
    for k, v in want.items():
        assert isinstance(got[k], float), k
        assert abs(got[k] - v) <= (loss_tol if k.endswith("_loss") else tol), (k, got[k], v)
    assert got["patients"] == names
    assert np.abs(got["patient_score"].double().numpy() - score).max() <= 1e-6
    assert got["patient_target"].tolist() == list(target)


# ---------------------------------------------------------------------------- hand-made epochs
def _epoch(C):
    """8 slides, 4 interleaved patients.  Patient "n" has no slide predicted 1, "o" exactly one (of
    two), "s" several (of four); slides 1/6 and 2/5 have identical logits under different labels (exact score ties between a positive and a negative of every class)."""
    if C == 2:
        logits = [[2.0, -1.0], [0.25, 0.75], [-1.0, 1.5], [1.0, 0.0], [-0.5, 2.0], [-1.0, 1.5], [0.25, 0.75],
                  [3.0, 0.0]]
        label = [0, 1, 1, 0, 1, 0, 0, 1]
    else:
        logits = [[2.0, -1.0, 0.0], [0.25, 0.75, 0.5], [-1.0, 1.5, 1.0], [1.0, 0.5, 2.5], [-0.5, 2.0, 0.0],
                  [-1.0, 1.5, 1.0], [0.25, 0.75, 0.5], [0.0, 0.0, 0.0]]
        label = [0, 1, 1, 2, 1, 2, 0, 2]
    patients = ["n", "o", "s", "o", "s", "s", "q", "s"]
    return (torch.tensor(logits, dtype=torch.float32), torch.tensor(label, dtype=torch.int64), patients)


@pytest.mark.parametrize("C", [2, 3])
def test_eval_record_cpu_matches_restatement(C):
    from transmil_deepgraft_amd.interface import EvalRecord, auroc_from_pairs
    logits, label, patients = _epoch(C)
    rec = EvalRecord(C, capacity=2, device="cpu")        # grows by doubling: 2 -> 4 -> 8
    for a, b in ((0, 3), (3, 4), (4, 8)):
        rec.append(logits[a:b], label[a:b])
    assert rec.n == 8 and rec.capacity == 8 and int(rec.cursor) == 8
    prob, y_hat, nll = ref_rows(logits.numpy(), label.numpy())
    assert torch.equal(rec.logits[:8], logits) and torch.equal(rec.label[:8], label)
    assert rec.y_hat[:8].tolist() == y_hat.tolist()
    np.testing.assert_allclose(rec.prob[:8].numpy(), prob, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rec.nll[:8].numpy(), nll, rtol=1e-6, atol=1e-6)
    assert rec.class_stats.tolist() == ref_class_stats(y_hat, label.numpy(), C).tolist()

    p32 = rec.prob[:8].numpy()
    if C == 2:      # the patients' shapes the positive rule distinguishes
        per = {p: [int(y_hat[i]) for i in range(8) if patients[i] == p] for p in set(patients)}
        assert sum(per["n"]) == 0 and per["o"] == [1, 0] and per["s"] == [1, 1, 1, 0]
    for rule in (False, True):
        s = rec.summary(patients, positive_rule=rule)
        names, score, pred, target, nslides = ref_patients(p32, y_hat, label.numpy(), patients, rule)
        assert s["patients"] == names == ["n", "o", "s", "q"] and s["n"] == 8
        assert s["nslides"] == nslides.tolist() and s["patient_target"].tolist() == target.tolist()
        assert np.abs(s["patient_score"].double().numpy() - score).max() <= 1e-6   # fp32 sums of <= 8 probs
        assert s["patient_pred"].tolist() == pred.tolist()
        assert s["slide_cm"] == ref_confusion(y_hat, label.numpy(), C).tolist()
        assert s["patient_cm"] == ref_confusion(pred, target, C).tolist()
        w, n = ref_pairs(p32, label.numpy(), C)
        assert (s["slide_wins2"], s["slide_npairs"]) == (w, n)
        lab = label.numpy()
        ties = sum(int((p32[lab == c, c][:, None] == p32[lab != c, c][None, :]).sum()) for c in range(C))
        assert ties >= 2, "the epoch must hold exact score ties between a positive and a negative"
        pw, pn = ref_pairs(s["patient_score"].numpy(), target, C)
        assert (s["patient_wins2"], s["patient_npairs"]) == (pw, pn)
        assert abs(s["nll_sum"] - nll.sum()) <= 8e-6
        assert auroc_from_pairs(w, n) == ref_auc(w, n)
    if C == 2:      # the rule changes patients "o" and "s" (they also hold a slide predicted 0), not "n"
        a = rec.summary(patients, positive_rule=False)["patient_score"]
        b = rec.summary(patients, positive_rule=True)["patient_score"]
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])

    rec.reset()
    assert rec.n == 0 and int(rec.cursor) == 0 and rec.class_stats.abs().sum() == 0
    with pytest.raises(ValueError):
        rec.summary([])


@pytest.mark.parametrize("C", [2, 3])
def test_single_class_target_gives_zero_auc(C):
    from transmil_deepgraft_amd.interface import EvalRecord, auroc_from_pairs
    logits, _, patients = _epoch(C)
    rec = EvalRecord(C, capacity=8, device="cpu")
    rec.append(logits, torch.ones(8, dtype=torch.int64))
    s = rec.summary(patients)
    assert not any(s["slide_npairs"]) and not any(s["patient_npairs"])
    assert auroc_from_pairs(s["slide_wins2"], s["slide_npairs"]) == 0.0
    assert auroc_from_pairs(s["patient_wins2"], s["patient_npairs"]) == 0.0


def test_out_of_range_label_in_record_is_nan_and_uncounted():
    from transmil_deepgraft_amd.interface import EvalRecord
    rec = EvalRecord(2, capacity=4, device="cpu")
    rec.append(torch.tensor([[1.0, 2.0], [0.5, 0.0]]), torch.tensor([5, 0]))
    assert torch.isnan(rec.nll[0]) and not torch.isnan(rec.nll[1])
    assert rec.class_stats.tolist() == [[1, 1], [0, 0]]


def test_metric_definitions_against_sklearn():
    """AUROC from pair counts and the confusion-matrix collection against scikit-learn."""
    skm = pytest.importorskip("sklearn.metrics")
    from transmil_deepgraft_amd.interface import auroc_from_pairs, metrics_from_confusion
    rng = np.random.default_rng(3)
    for C in (2, 3, 5):
        M = 60
        target = rng.integers(0, C, M)
        target[:C] = np.arange(C)
        scores = np.round(rng.random((M, C)), 1)            # coarse: many exact ties
        pred = rng.integers(0, max(C - 1, 2), M)            # for C > 2 the last class is never predicted
        w, n = ref_pairs(scores, target, C)
        if C == 2:
            want = skm.roc_auc_score(target, scores[:, 1])
        else:
            want = np.mean([skm.roc_auc_score(target == c, scores[:, c]) for c in range(C)])
        assert abs(auroc_from_pairs(w, n) - want) < 1e-12
        cm = ref_confusion(pred, target, C)
        got = metrics_from_confusion(cm.tolist(), "x_")
        assert got == pytest.approx(ref_collection(cm, "x_"), abs=1e-12)
        kind = "Binary" if C == 2 else "Multiclass"
        kw = dict(zero_division=0) if C == 2 else dict(average="macro", labels=list(range(C)), zero_division=0)
        assert abs(got[f"x_{kind}CohenKappa"] - skm.cohen_kappa_score(target, pred)) < 1e-12
        assert abs(got[f"x_{kind}F1Score"] - skm.f1_score(target, pred, **kw)) < 1e-12
        assert abs(got[f"x_{kind}Precision"] - skm.precision_score(target, pred, **kw)) < 1e-12
        assert abs(got[f"x_{kind}Recall"] - skm.recall_score(target, pred, **kw)) < 1e-12
    empty = metrics_from_confusion([[3, 0], [0, 0]], "")       # no positive anywhere: every ratio 0 / 0
    assert empty["BinaryF1Score"] == 0.0 and empty["BinaryRecall"] == 0.0 and empty["BinaryCohenKappa"] == 0.0


# ---------------------------------------------------------------------------- the task, stub model
class _Stub(torch.nn.Module):
    """Returns preset logits, batch after batch."""

    def __init__(self, C, logits):
        super().__init__()
        self.n_classes = C
        self.w = torch.nn.Parameter(torch.zeros(3, 3))
        self.queue = list(logits)

    def forward(self, x):
        out = self.queue[:x.shape[0]]
        del self.queue[:x.shape[0]]
        return torch.stack(out)


def _batches(logits, label, patients, sizes):
    i = 0
    for b in sizes:
        names = [f"slide{j}" for j in range(i, i + b)]
        if b == 1:      # batch 1 as the reference's loaders give it: plain strings, an int label
            yield torch.zeros(1, 4, 8), int(label[i]), (names[0], None, patients[i])
        else:
            yield torch.zeros(b, 4, 8), label[i:i + b], (names, None, tuple(patients[i:i + b]))
        i += b


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("stage", ["val", "test"])
def test_task_epoch_with_stub_model(C, stage):
    from transmil_deepgraft_amd.interface import TransMILTask
    logits, label, patients = _epoch(C)
    task = TransMILTask(_Stub(C, logits))
    step = task.validation_step if stage == "val" else task.test_step
    start = task.on_validation_epoch_start if stage == "val" else task.on_test_epoch_start
    end = task.on_validation_epoch_end if stage == "val" else task.on_test_epoch_end
    start()
    for i, batch in enumerate(_batches(logits, label, patients, (1, 3, 1, 2, 1))):
        out = step(batch, i)
        assert out.shape[1] == C
    got = end()
    rec = task.eval_state(stage).record
    want, names, score, target = ref_epoch(stage, logits.numpy(), label.numpy(), patients, C, rec.prob[:8].numpy())
    assert_epoch_equal(got, want, names, score, target)
    kind = "Binary" if C == 2 else "Multiclass"
    keys = {f"{stage}_loss", f"{stage}_auc", f"{stage}_patient_auc", "patient_score", "patient_target", "patients",
            "class_acc", "slides"}
    coll = ["Accuracy", "CohenKappa", "F1Score", "Recall", "Precision"] + (["Specificity"] if C > 2 else [])
    keys |= {f"{stage}_patient{kind}{m}" for m in coll}
    if stage == "test":
        keys |= {f"test_{kind}{m}" for m in coll}
    else:
        keys.add("val_accuracy")
    assert set(got) == keys
    assert got["slides"] == [f"slide{j}" for j in range(8)]
    st = ref_class_stats(ref_rows(logits.numpy(), label.numpy())[1], label.numpy(), C)
    assert got["class_acc"] == [c / n if n else None for n, c in st.tolist()]
    if stage == "val":
        # patient level (4 patients), not slide level (8 slides)
        _, _, pred, tgt, _ = ref_patients(rec.prob[:8].numpy(), rec.y_hat[:8].numpy(), label.numpy(), patients, C == 2)
        assert got["val_accuracy"] == float((pred == tgt).sum()) / 4
        slide_acc = float((rec.y_hat[:8] == label).sum()) / 8
        assert got["val_accuracy"] != slide_acc

    # the next epoch starts from an empty record
    task.model.queue = list(logits[:2])
    start()
    assert task.eval_state(stage).record.n == 0 and task.eval_state(stage).names == []
    step((torch.zeros(2, 4, 8), label[:2], (["a", "b"], None, ["p", "p"])))
    again = end()
    assert again["patients"] == ["p"] and len(again["slides"]) == 2
    assert again[f"{stage}_auc"] == (0.0 if label[0] == label[1] else again[f"{stage}_auc"])


def test_val_loss_drives_the_configured_scheduler():
    from transmil_deepgraft_amd.interface import TransMILTask
    logits, label, patients = _epoch(2)
    task = TransMILTask(_Stub(2, logits), lr=1e-3)
    opts, scheds = task.configure_optimizers()
    sched = scheds[0]["scheduler"]
    assert scheds[0]["monitor"] == "val_loss"
    sched.patience = 0
    for epoch in range(2):          # the same loss twice: no improvement -> the rate halves
        task.model.queue = list(logits)
        task.on_validation_epoch_start()
        for batch in _batches(logits, label, patients, (1,) * 8):
            task.validation_step(batch)
        val_loss = task.on_validation_epoch_end()["val_loss"]
        assert isinstance(val_loss, float) and np.isfinite(val_loss)
        sched.step(val_loss)
    assert [g["lr"] for g in opts[0].param_groups] == [5e-4] * len(opts[0].param_groups)


def test_out_of_range_cpu_label_raises_index_error():
    from transmil_deepgraft_amd.interface import TransMILTask
    logits, _, _ = _epoch(2)
    task = TransMILTask(_Stub(2, logits))
    with pytest.raises(IndexError):
        task.validation_step((torch.zeros(1, 4, 8), torch.tensor([2]), ("s", None, "p")))
    with pytest.raises(IndexError):
        task.test_step((torch.zeros(1, 4, 8), -1, ("s", None, "p")))
    assert task.eval_state("val").record.n == 0 and len(task.model.queue) == 8     # nothing ran


# ---------------------------------------------------------------------------- two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _strip(d):
    return {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in d.items()}


def _gloo_eval_worker(rank, world, port, stage, out):
    import torch.distributed as dist
    from transmil_deepgraft_amd.interface import TransMILTask
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    logits, label, patients = _epoch(2)
    lo, hi = (0, 3) if rank == 0 else (3, 8)            # 3 and 5 slides; patients "o" and "s" span both ranks
    task = TransMILTask(_Stub(2, logits[lo:hi]))
    step = task.validation_step if stage == "val" else task.test_step
    for i in range(lo, hi):
        step((torch.zeros(1, 4, 8), label[i:i + 1], ([f"slide{i}"], None, [patients[i]])))
    end = task.on_validation_epoch_end if stage == "val" else task.on_test_epoch_end
    out[rank] = _strip(end())
    dist.destroy_process_group()


@pytest.mark.parametrize("stage", ["val", "test"])
def test_two_gloo_ranks_return_the_single_process_metrics(stage):
    import torch.multiprocessing as mp
    from transmil_deepgraft_amd.interface import TransMILTask
    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_gloo_eval_worker, args=(2, port, stage, out), nprocs=2, join=True)
        res = dict(out)
    logits, label, patients = _epoch(2)
    task = TransMILTask(_Stub(2, logits))
    step = task.validation_step if stage == "val" else task.test_step
    for i in range(8):
        step((torch.zeros(1, 4, 8), label[i:i + 1], ([f"slide{i}"], None, [patients[i]])))
    single = _strip((task.on_validation_epoch_end if stage == "val" else task.on_test_epoch_end)())
    assert single["patients"] == ["n", "o", "s", "q"]
    assert res[0] == single and res[1] == single


# ---------------------------------------------------------------------------- argument checks
def test_eval_entry_points_reject_bad_arguments_without_gpu():
    from transmil_deepgraft_amd import _lib
    with pytest.raises(RuntimeError, match="B and C must be >= 1"):
        _lib.call("tm_eval_record", None, None, 1, 0, 4, None, None, None, None, None, None, None, None)
    assert "C must be >= 1" in _lib.last_error()
    with pytest.raises(RuntimeError, match="capacity must be >= 1"):
        _lib.call("tm_eval_record", None, None, 1, 2, 0, None, None, None, None, None, None, None, None)
    assert "capacity" in _lib.last_error()
    with pytest.raises(RuntimeError, match="null arg"):
        _lib.call("tm_eval_record", None, None, 1, 2, 4, None, None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="eval_patients"):
        _lib.call("tm_eval_patients", None, None, None, None, 1, 2, 0, 0, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="eval_confusion"):
        _lib.call("tm_eval_confusion", None, None, 0, 2, None, None, None, None)
    with pytest.raises(RuntimeError, match="eval_auc_pairs"):
        _lib.call("tm_eval_auc_pairs", None, None, 3, 0, None, None, None)
