"""Shared by test_cls_metrics_host.py and test_gpu_cls_metrics.py: seeded (targets, predictions, probabilities) inputs and the CPU
yardstick of the classification counts -- torch integer ops only: confusion by bincount, the AUC pair counts by broadcasting the same
fp32 values in float64 (exact: every fp32 is a float64)."""
import torch

DOMAIN_OF = {7: "Cora_NC", 6: "ENZYMES", 2: "Cora_LP"}       # a domain with that many classes (constants.NUM_CLASSES)


def make_inputs(n, C, seed, kind="random", steps=8):
    """kind: random (softmax of normal logits), ties (probabilities that are multiples of 1/steps and sum to 1: many equal pairs), dup (every
    row occurs twice or more), one_class (all targets equal), all_wrong (no prediction hits its target), absent_target (class C-1 is
    predicted and never a target), absent_both (class 1 is neither)."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.randint(0, C, (n,), generator=g)
    if kind == "ties":
        balls = torch.randint(0, C, (n, steps), generator=g)
        prob = torch.zeros(n, C).scatter_add_(1, balls, torch.ones(n, steps)) / steps
    else:
        prob = torch.softmax(torch.randn(n, C, generator=g) + 1.5 * torch.nn.functional.one_hot(targets, C), dim=1)
    pred = prob.argmax(dim=1)
    if kind == "dup":
        half = max(n // 2, 1)
        idx = torch.cat([torch.arange(half), torch.randint(0, half, (n - half,), generator=g)])
        targets, pred, prob = targets[idx], pred[idx], prob[idx]
    elif kind == "one_class":
        targets = torch.full((n,), C - 1)
    elif kind == "all_wrong":
        pred = (targets + 1 + torch.randint(0, C - 1, (n,), generator=g)) % C
    elif kind == "absent_target":
        targets = torch.where(targets == C - 1, torch.zeros_like(targets), targets)
        pred[0] = C - 1
    elif kind == "absent_both":
        targets = torch.where(targets == 1, torch.zeros_like(targets), targets)
        pred = torch.where(pred == 1, torch.zeros_like(pred), pred)
    return targets.contiguous(), pred.contiguous(), prob.float().contiguous()


def cpu_counts(targets, predictions, prob, C):
    """(confusion [C, C], auc_counts [C, 4], status) as int64 CPU tensors / an int, the definition of gmp_cls_counts in gnnmp.h."""
    targets, predictions, prob = targets.cpu(), predictions.cpu(), prob.cpu()
    ok = (targets >= 0) & (targets < C) & (predictions >= 0) & (predictions < C) & torch.isfinite(prob).all(dim=1)
    t, p, pr = targets[ok], predictions[ok], prob[ok].double()
    confusion = torch.bincount(t * C + p, minlength=C * C).view(C, C)
    auc = torch.zeros(C, 4, dtype=torch.int64)
    for c in range(C):
        pos, neg = pr[t == c, c], pr[t != c, c]
        auc[c, 0], auc[c, 1] = pos.numel(), neg.numel()
        auc[c, 2] = (pos[:, None] > neg[None, :]).sum()
        auc[c, 3] = (pos[:, None] == neg[None, :]).sum()
    return confusion, auc, int((~ok).sum())


def cpu_counts_sorted(targets, predictions, prob, C):
    """cpu_counts for sizes where n^2 booleans do not fit: the same integers from a sort and two binary searches per class (the number of
    negatives below / not above each positive).  Exact like the broadcast form; test_cls_metrics_host.py holds the two equal."""
    targets, predictions, prob = targets.cpu(), predictions.cpu(), prob.cpu()
    ok = (targets >= 0) & (targets < C) & (predictions >= 0) & (predictions < C) & torch.isfinite(prob).all(dim=1)
    t, p, pr = targets[ok], predictions[ok], prob[ok]
    confusion = torch.bincount(t * C + p, minlength=C * C).view(C, C)
    auc = torch.zeros(C, 4, dtype=torch.int64)
    for c in range(C):
        pos, neg = pr[t == c, c].contiguous(), pr[t != c, c].sort().values
        below, not_above = torch.searchsorted(neg, pos, right=False), torch.searchsorted(neg, pos, right=True)
        auc[c, 0], auc[c, 1], auc[c, 2], auc[c, 3] = pos.numel(), neg.numel(), below.sum(), (not_above - below).sum()
    return confusion, auc, int((~ok).sum())
