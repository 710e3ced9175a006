"""Shared by test_knn_host.py and test_gpu_knn.py: the float64 definition of the k-nearest-neighbour probe of csrc/knn.hip (gnnmp.h
gmp_knn_topk / gmp_knn_vote), written from the contract and not from the kernels.

  normalize   z / max(||z||, 1e-12) per row (a zero row stays zero)
  cosine      normalize(q) normalize(db)^T
  topk        per query the k best database rows, similarity descending, ties to the lower database index (a stable sort of the
              negated row); exclude_self drops j == i; behind the last candidate -1 / -inf.  `similarity=` replays the selection on
              someone else's scores (the kernel's own matrix), as oracle.miner does for the miner tests.
  vote        class_scores[q, c] = sum over the neighbours r in order of exp(sim[q, r] / T) where idx[q, r] >= 0 and the label is c;
              pred = argmax, ties to the lower class, -1 without a valid neighbour; status = neighbours with a label outside [0, C)
plus the two exact-arithmetic row generators of the miner tests."""
import numpy as np

NINF = float("-inf")


def normalize(z):
    z = np.asarray(z, dtype=np.float64)
    return z / np.maximum(np.sqrt((z * z).sum(axis=1, keepdims=True)), 1e-12)


def cosine(q, db):
    return normalize(q) @ normalize(db).T


def topk(q, db, k, exclude_self=False, similarity=None):
    """(idx [nq, k] int64, sim [nq, k] in the dtype of the scores)"""
    S = cosine(q, db) if similarity is None else np.asarray(similarity)
    nq, ndb = S.shape
    if exclude_self and nq != ndb:
        raise ValueError("exclude_self is leave-one-out over one set")
    idx = np.full((nq, k), -1, dtype=np.int64)
    sim = np.full((nq, k), NINF, dtype=S.dtype)
    for i in range(nq):
        order = np.argsort(-S[i], kind="stable")                    # score descending, equal scores in index order
        if exclude_self:
            order = order[order != i]
        m = min(k, order.size)
        idx[i, :m] = order[:m]
        sim[i, :m] = S[i, order[:m]]
    return idx, sim


def vote(idx, sim, labels, num_classes, temperature=0.07):
    """(class_scores [nq, C] float64, pred [nq] int64, status)"""
    idx, sim, labels = np.asarray(idx), np.asarray(sim, dtype=np.float64), np.asarray(labels)
    nq, k = idx.shape
    scores = np.zeros((nq, num_classes), dtype=np.float64)
    pred = np.full(nq, -1, dtype=np.int64)
    status = 0
    for q in range(nq):
        used = 0
        for r in range(k):
            if idx[q, r] < 0:
                continue
            c = int(labels[idx[q, r]])
            if not 0 <= c < num_classes:
                status += 1
                continue
            scores[q, c] += np.exp(sim[q, r] / temperature)
            used += 1
        if used:
            pred[q] = int(np.argmax(scores[q]))                     # the first maximum: ties to the lower class
    return scores, pred, status


def four_ones(n, d, seed):
    """rows with exactly four ones: norm 2, normalised entries 0.5, dot products m / 4 -- exact in fp32 in any order"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), dtype=np.float32)
    for i in range(n):
        x[i, rng.choice(d, size=4, replace=False)] = 1.0
    return x


def sixteen_signs(n, d, seed):
    """rows with sixteen +-1 entries: norm 4, normalised entries in {-0.25, 0, 0.25}, dot products m / 16 -- exact in any order"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), dtype=np.float32)
    for i in range(n):
        x[i, rng.choice(d, size=16, replace=False)] = rng.choice([-1.0, 1.0], size=16)
    return x
