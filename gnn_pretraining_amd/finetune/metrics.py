"""Fine-tuning metrics with the keys and aggregation of src/finetune/metrics.py (sklearn scores on host copies;
sample-weighted means over batches).  Reporting only: nothing here feeds back into training."""
from __future__ import annotations

import time
from typing import Dict, List, Sequence

import numpy as np
import torch
from torch import Tensor

from ..constants import NUM_CLASSES


def _aggregate_batch_metrics(batch_metrics: List[Dict[str, float]], epoch: int, prefix: str) -> Dict[str, float]:
    """metrics.py:15-36"""
    names = set(batch_metrics[0].keys()) - {"num_samples"}
    total = sum(b["num_samples"] for b in batch_metrics)
    out = {k: sum(b[k] * b["num_samples"] for b in batch_metrics) / total for k in names}
    if prefix != "val":
        out[f"{prefix}/progress/epoch"] = epoch
    return out


def compute_batch_metrics(domain_name: str, targets: Tensor, predictions: Tensor, probabilities: Tensor, loss: Tensor,
                          prefix: str) -> Dict[str, float]:
    """metrics.py:39-82"""
    from sklearn.metrics import accuracy_score, f1_score, precision_score, recall_score, roc_auc_score
    binary = NUM_CLASSES[domain_name] == 2
    y_true, y_pred = targets.detach().cpu().numpy(), predictions.detach().cpu().numpy()
    y_prob = probabilities.detach().cpu().numpy()
    if binary:
        y_prob = y_prob[:, 1]
    avg = "binary" if binary else "macro"
    m = {f"{prefix}/accuracy": float(accuracy_score(y_true, y_pred)),
         f"{prefix}/f1": float(f1_score(y_true, y_pred, average=avg, zero_division=0)),
         f"{prefix}/precision": float(precision_score(y_true, y_pred, average=avg, zero_division=0)),
         f"{prefix}/recall": float(recall_score(y_true, y_pred, average=avg, zero_division=0))}
    if len(np.unique(y_true)) < 2:
        m[f"{prefix}/auc"] = 0.0
    else:
        try:
            m[f"{prefix}/auc"] = float(roc_auc_score(y_true, y_prob) if binary else roc_auc_score(y_true, y_prob, multi_class="ovr"))
        except (ValueError, RuntimeWarning):
            m[f"{prefix}/auc"] = 0.0
    m[f"{prefix}/loss"] = float(loss.item())
    m["num_samples"] = len(targets)
    return m


def metrics_from_counts(confusion, auc_counts, binary: bool, prefix: str) -> Dict[str, float]:
    """The five scores of compute_batch_metrics and num_samples from integer counts alone, in float64 on the host (no GPU, no scikit-learn):
    confusion [C, C] with [t, p] = rows of target t predicted p, auc_counts [C, 4] = (n_pos, n_neg, n_greater, n_equal) per class
    (ops.cls_counts).  What the scikit-learn calls compute, spelled out:
      accuracy                trace / n
      precision, recall, f1   tp / (tp + fp), tp / (tp + fn), 2 tp / (2 tp + fp + fn), each 0 where its denominator is 0 (zero_division=0);
                              binary: of label 1; otherwise the unweighted mean over the labels that occur as a target or as a prediction
                              (average="macro" over scikit-learn's union of y_true and y_pred)
      auc                     per class (n_greater + n_equal / 2) / (n_pos n_neg), the pair-count form of the area under the ROC curve;
                              binary: of class 1, 0.0 with fewer than two distinct targets; otherwise the mean over all C classes, 0.0 when
                              a class has no target (roc_auc_score raises there and compute_batch_metrics reports 0.0)"""
    conf = np.asarray(confusion, dtype=np.int64)
    auc = np.asarray(auc_counts, dtype=np.int64).reshape(-1, 4)
    c = conf.shape[0]
    if conf.shape != (c, c) or auc.shape != (c, 4):
        raise ValueError(f"metrics_from_counts: confusion {conf.shape}, auc_counts {auc.shape}")
    support, predicted, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    n = int(conf.sum())
    if n == 0:
        raise ValueError("metrics_from_counts: no samples")
    labels = [1] if binary else [k for k in range(c) if support[k] > 0 or predicted[k] > 0]

    def mean_ratio(num, den) -> float:
        return float(np.mean([int(num[k]) / int(den[k]) if den[k] > 0 else 0.0 for k in labels]))

    m = {f"{prefix}/accuracy": int(tp.sum()) / n,
         f"{prefix}/f1": mean_ratio(2 * tp, support + predicted),              # 2 tp + fp + fn = support + predicted
         f"{prefix}/precision": mean_ratio(tp, predicted),
         f"{prefix}/recall": mean_ratio(tp, support)}
    classes = [1] if binary else list(range(c))
    if int((support > 0).sum()) < 2 or any(support[k] == 0 for k in classes):
        m[f"{prefix}/auc"] = 0.0
    else:
        m[f"{prefix}/auc"] = float(np.mean([(int(auc[k, 2]) + 0.5 * int(auc[k, 3])) / (int(auc[k, 0]) * int(auc[k, 1])) for k in classes]))
    m["num_samples"] = n
    return m


def compute_batch_metrics_device(domain_name: str, targets: Tensor, predictions: Tensor, probabilities: Tensor, loss: Tensor,
                                 prefix: str) -> Dict[str, float]:
    """compute_batch_metrics with the counting on the GPU (ops.cls_counts: csrc/cls_metrics.hip): the same keys and values from one
    read-back of C C + 4 C + 1 integers (and the loss) and metrics_from_counts, with no copy of the inputs and no scikit-learn.
    targets / predictions int64 [n] and probabilities fp32 [n, C] on the GPU, 1 <= n <= ops.CLS_MAX_ROWS (the pair count behind the AUC
    is n^2 compares).  Raises ValueError when n is outside that range or a row has a target or prediction outside [0, C) or a non-finite
    probability.  One difference on purpose: roc_auc_score refuses multi-class rows that do not sum to 1 (reported as auc 0.0); the
    counts do not look at row sums -- the callers pass a softmax."""
    from .. import ops
    n, c = int(targets.numel()), int(probabilities.size(1))
    if not 1 <= n <= ops.CLS_MAX_ROWS:
        raise ValueError(f"compute_batch_metrics_device: {n} rows (1 <= n <= {ops.CLS_MAX_ROWS}: the AUC pair count is n^2 compares)")
    buf = ops.cls_counts_packed(targets.detach().contiguous(), predictions.detach().contiguous(), probabilities.detach().contiguous())
    host = buf.cpu().numpy()                                                    # the one read-back
    k = c * c + 4 * c
    counts, status = host[:2 * k].view(np.int64), int(host[2 * k])
    if status != 0:
        raise ValueError(f"compute_batch_metrics_device: {status} of {n} rows have a target or prediction outside [0, {c}) "
                         "or a non-finite probability")
    m = metrics_from_counts(counts[:c * c].reshape(c, c), counts[c * c:].reshape(c, 4), NUM_CLASSES[domain_name] == 2, prefix)
    m.pop("num_samples")
    m[f"{prefix}/loss"] = float(loss.item())
    m["num_samples"] = n
    return m


def knn_probe_accuracy(db_emb: Tensor, db_labels: Tensor, query_emb: Tensor, query_labels: Tensor, num_classes: int, k: int = 20,
                       temperature: float = 0.07) -> Dict:
    """The weighted k-NN probe of Wu et al. 2018 (InstDisc; also DINO's): every query embedding is classified from its k nearest
    labelled database embeddings in cosine similarity, each voting exp(similarity / temperature) for its class (ops.knn_topk +
    ops.knn_vote: csrc/knn.hip, no nq x ndb matrix).  Embeddings fp32 [n, d <= 256] and labels int64 [n] on the GPU.  Returns
    {"accuracy": correct / num_samples, "correct", "num_samples"}: the accuracy is a ratio of two integers counted on the device
    (one read-back).  Needs no trained head; nothing here feeds back into training."""
    from .. import ops
    idx, sim = ops.knn_topk(query_emb.detach().contiguous(), db_emb.detach().contiguous(), k)
    _, pred = ops.knn_vote(idx, sim, db_labels.to(torch.int64).contiguous(), num_classes, temperature)
    n = int(query_labels.numel())
    if n == 0:
        raise ValueError("knn_probe_accuracy: no queries")
    correct = int((pred == query_labels.to(torch.int64)).sum().item())
    return {"accuracy": correct / n, "correct": correct, "num_samples": n}


def linear_eval_probe(train_emb: Tensor, train_labels: Tensor, emb: Tensor, labels: Tensor, num_classes: int, iters: int = 100,
                      lr: float = 0.01, l2: float = 0.0) -> Dict:
    """Linear evaluation of frozen embeddings (the protocol of DGI, GRACE, GraphCL, InfoGraph): a multinomial logistic regression is
    fitted on the L2-normalised train embeddings (ops.logreg_fit: csrc/logreg.hip, `iters` full-batch Adam updates from zero, all
    enqueued at once) and scored on the rows of `emb` (ops.logreg_predict).  Embeddings fp32 [n, d <= 256] and labels int64 [n] in
    [0, num_classes <= 32) on the GPU.  Returns {"accuracy": correct / num_samples, "correct", "num_samples", "train_loss" (the loss
    before the last update), "train_accuracy"}: the accuracies are ratios of integers counted on the device, and everything comes back
    in one read-back.  Nothing here feeds back into training."""
    from .. import ops
    n, n_train = int(labels.numel()), int(train_labels.numel())
    if n == 0 or n_train == 0:
        raise ValueError(f"linear_eval_probe: {n_train} train rows, {n} rows to score")
    x_train, y_train = train_emb.detach().contiguous(), train_labels.to(torch.int64).contiguous()
    fit, status = ops._logreg_enqueue(x_train, y_train, num_classes, iters, lr, l2, None, False, False)
    pred = ops.logreg_predict(emb.detach().contiguous(), fit.state.weight, fit.state.bias)
    pred_train = ops.logreg_predict(x_train, fit.state.weight, fit.state.bias)
    words = torch.stack([status[0].double(), (pred == labels.to(torch.int64)).sum().double(), (pred_train == y_train).sum().double(),
                         fit.loss_history[-1].double()]).tolist()                # the one read-back (the counts are exact in a double)
    bad, correct, correct_train, loss = int(words[0]), int(words[1]), int(words[2]), float(words[3])
    if bad:
        raise ValueError(f"linear_eval_probe: {bad} train rows have a label outside [0, {num_classes})")
    return {"accuracy": correct / n, "correct": correct, "num_samples": n, "train_loss": loss, "train_accuracy": correct_train / n_train}


def clustering_scores(table) -> Dict[str, float]:
    """NMI (arithmetic normalisation), ARI, purity and accuracy of a clustering against class labels, in float64 on the host from the
    integer contingency table alone: table [clusters, classes] with [k, c] = rows of cluster k and class c (ops.contingency).  Clusters
    and classes without rows do not count, as in scikit-learn, whose values these are:
      nmi       I / ((H_clusters + H_classes) / 2), I = sum n_kc / n log(n n_kc / (n_k n_c)); 1.0 when both sides have one group, 0.0 when I = 0
      ari       from the pair counts: 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)) in integers; 1.0 when fn = fp = 0
      purity    sum over clusters of the largest class count / n
      accuracy  the best one-to-one matching of clusters to classes (scipy.optimize.linear_sum_assignment on the table) / n"""
    from scipy.optimize import linear_sum_assignment
    t = np.asarray(table, dtype=np.int64)
    if t.ndim != 2 or bool((t < 0).any()):
        raise ValueError(f"clustering_scores: table of shape {t.shape} (a 2-D array of counts)")
    n = int(t.sum())
    if n == 0:
        raise ValueError("clustering_scores: no samples")
    full = t
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0]
    nk, nc = t.sum(axis=1), t.sum(axis=0)

    def entropy(counts) -> float:
        p = counts.astype(np.float64)
        return 0.0 if p.size == 1 else float(-np.sum(p / n * (np.log(p) - np.log(n))))

    if nk.size == 1 and nc.size == 1:
        nmi = 1.0
    elif nk.size == 1 or nc.size == 1:
        nmi = 0.0
    else:
        kk, cc = np.nonzero(t)
        v = t[kk, cc].astype(np.float64)
        terms = v / n * (np.log(v) - np.log(n)) + v / n * (-np.log((nk[kk] * nc[cc]).astype(np.float64)) + 2.0 * np.log(n))
        terms = np.where(np.abs(terms) < np.finfo(np.float64).eps, 0.0, terms)
        mi = max(float(terms.sum()), 0.0)
        nmi = 0.0 if mi == 0.0 else mi / ((entropy(nk) + entropy(nc)) / 2.0)
    sq = int(sum(int(v) * int(v) for v in t.ravel()))
    tp = sq - n
    fp = int(sum(int(v) * int(v) for v in nk)) - sq             # same cluster, different class
    fn = int(sum(int(v) * int(v) for v in nc)) - sq
    tn = n * n - fp - fn - sq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    rows, cols = linear_sum_assignment(full, maximize=True)
    return {"nmi": float(nmi), "ari": float(ari), "purity": int(t.max(axis=1).sum()) / n, "accuracy": int(full[rows, cols].sum()) / n}


def _kmeans_seeds(x: Tensor, num_clusters: int, init: str, gen: torch.Generator) -> Tensor:
    """Rows of x to start from (indices, on the host).  "random": the first rows of a permutation.  "k-means++": a uniform row, then each
    further one drawn with probability proportional to max(0, 2 - 2 sim_best), the squared distance on the sphere to the nearest centre
    chosen so far (ops.kmeans_assign); all weights zero: the lowest row not yet chosen.  More clusters than rows: every row once in that
    order, then again from the start (the duplicates stay empty)."""
    from .. import ops
    n = x.size(0)
    if init == "random":
        return torch.randperm(n, generator=gen)[torch.arange(num_clusters) % n]
    chosen = [int(torch.randint(n, (1,), generator=gen))]
    while len(chosen) < min(num_clusters, n):
        _, sim_best = ops.kmeans_assign(x, x[torch.tensor(chosen, device=x.device)].contiguous())
        w = (2.0 - 2.0 * sim_best.double().cpu()).clamp_(min=0.0)
        w[torch.tensor(chosen)] = 0.0
        if float(w.sum()) > 0.0:
            chosen.append(int(torch.multinomial(w, 1, generator=gen)))
        else:
            taken = set(chosen)
            chosen.append(next(i for i in range(n) if i not in taken))
    return torch.tensor(chosen)[torch.arange(num_clusters) % n]


def cluster_probe(emb: Tensor, labels: Tensor, num_clusters: int, n_init: int = 10, max_iter: int = 100, seed: int = 0,
                  init: str = "k-means++") -> Dict:
    """The clustering probe for self-supervised embeddings: spherical k-means with num_clusters clusters on emb [n, d <= 256] (fp32, on
    the GPU; ops.kmeans_fit: csrc/kmeans.hip), n_init restarts, the one with the largest sum of similarities kept (ties to the earlier),
    scored against labels int64 [n] in [0, num_clusters) through the integer table of ops.contingency and clustering_scores.  The seeds
    are drawn on the host from a generator of this function's own (seed, restart): nothing else's random state moves, and the result is a
    function of (emb, labels, the arguments).  Returns the four scores and objective, n_iter, converged, empty_clusters, restart of
    the kept fit.  Needs no labelled neighbours and no trained head; nothing here feeds back into training."""
    from .. import ops
    if init not in ("k-means++", "random"):
        raise ValueError(f"cluster_probe: init={init!r} (\"k-means++\" or \"random\")")
    x = emb.detach().contiguous()
    n = int(x.size(0))
    if n < 1 or not 1 <= int(num_clusters) <= ops.KMEANS_MAX_CLUSTERS or int(n_init) < 1:
        raise ValueError(f"cluster_probe: {num_clusters} clusters, {n} rows, n_init={n_init} (rows >= 1, 1 <= clusters <= {ops.KMEANS_MAX_CLUSTERS}, "
                         "n_init >= 1)")
    best = None
    for restart in range(int(n_init)):
        gen = torch.Generator().manual_seed(int(seed) * 1000003 + restart)
        rows = _kmeans_seeds(x, int(num_clusters), init, gen)
        fit = ops.kmeans_fit(x, x[rows.to(x.device)].contiguous(), max_iter)
        objective = float(fit.sim.double().sum().item())
        if best is None or objective > best[0]:
            best = (objective, fit, restart)
    objective, fit, restart = best
    table = ops.contingency(fit.labels, labels.to(torch.int64).contiguous(), int(num_clusters), int(num_clusters)).cpu().numpy()
    out = clustering_scores(table)
    out.update(objective=objective, n_iter=fit.n_iter, converged=fit.converged, empty_clusters=fit.empty, restart=restart)
    return out


def compute_training_metrics(epoch: int, step: int, loss: Tensor, optimizer: torch.optim.Optimizer, domain_name: str,
                             targets: Tensor, predictions: Tensor, probabilities: Tensor, step_start_time: float,
                             model: torch.nn.Module, device_metrics: bool = False) -> Dict[str, float]:
    """metrics.py:85-118 (device_metrics: the batch scores from compute_batch_metrics_device)"""
    batch_metrics = compute_batch_metrics_device if device_metrics else compute_batch_metrics
    m = batch_metrics(domain_name, targets, predictions, probabilities, loss, "train")
    for pg in optimizer.param_groups:
        m[f'train/lr/{pg["name"]}'] = pg["lr"]
    sq = [p.grad.detach().pow(2).sum() for p in model.parameters() if p.grad is not None and p.requires_grad]
    m["train/gradients/model_grad_norm"] = float(torch.stack(sq).sum().sqrt()) if sq else 0.0     # one sync, not one per tensor
    m["train/progress/epoch"], m["train/progress/step"] = epoch, step
    m["train/system/time_per_step"] = time.time() - step_start_time
    return m


def compute_validation_metrics(batch_metrics: List[Dict[str, float]], epoch: int) -> Dict[str, float]:
    return _aggregate_batch_metrics(batch_metrics, epoch, "val")


def compute_test_metrics(batch_metrics: List[Dict[str, float]], epoch: int, epochs_since_improvement: int,
                         training_start_time: float, model: torch.nn.Module) -> Dict[str, float]:
    """metrics.py:128-144"""
    m = _aggregate_batch_metrics(batch_metrics, epoch, "test")
    m["test/convergence_epochs"] = epoch - epochs_since_improvement
    m["test/training_time"] = time.time() - training_start_time
    m["test/total_parameters"] = sum(p.numel() for p in model.parameters())
    m["test/trainable_parameters"] = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return m


def ranking_metrics(ranks, ks: Sequence[int] = (1, 10, 50)) -> Dict[str, float]:
    """MRR and Hits@K of link-prediction ranks (1 = best).  A rank may be fractional: a true edge tied with n_equal candidates sits at
    1 + n_greater + n_equal / 2, the mean over the orders of the tie (LinkPredictionEngine.rank).  hits@K counts rank <= K."""
    r = torch.as_tensor(ranks, dtype=torch.float64).reshape(-1).cpu()
    if r.numel() == 0:
        raise ValueError("ranking_metrics: no ranks")
    if bool((r < 1).any()):
        raise ValueError("ranking_metrics: ranks start at 1")
    out = {"mrr": float((1.0 / r).mean())}
    for k in ks:
        out[f"hits@{int(k)}"] = float((r <= k).to(torch.float64).mean())
    return out
