"""Label-free statistics of an embedding matrix, for pre-training and fine-tuning alike (no class labels are needed):

  uniformity, alignment   Wang & Isola, "Understanding Contrastive Representation Learning through Alignment and Uniformity on the
                          Hypersphere", ICML 2020: log of the mean Gaussian potential over all pairs of the normalised rows, and the mean
                          distance (to the power alpha) between the two views of a sample
  mean_cosine             the mean cosine similarity over all pairs: near 1 when the embeddings collapse onto one direction
  rankme                  Garrido et al., "RankMe: Assessing the Downstream Performance of Pretrained Self-Supervised Representations by
                          Their Rank", ICML 2023: exp of the entropy of the normalised singular values, an effective rank in [1, d]

The sums come from csrc/repr_stats.hip through ops.repr_*: no n x n array exists, and the Gram matrix behind RankMe is accumulated in
fp64.  Only the eigenvalues of that (at most 256 x 256) matrix are computed on the host.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
from torch import Tensor

from . import ops as O


def _pair_dict(sums, n: int) -> Dict[str, float]:
    pairs = n * (n - 1) / 2
    return {"uniformity": math.log(sums[0] / pairs), "mean_cosine": sums[1] / pairs}


def uniformity(z: Tensor, t: float = 2.0) -> Dict[str, float]:
    """{"uniformity": log of the mean over pairs i < j of exp(-t ||zn_i - zn_j||^2), "mean_cosine": the mean over pairs of <zn_i, zn_j>}
    of the rows of z [n, d], n >= 2, normalised to the unit sphere.  One read-back."""
    return _pair_dict(O.repr_pair_stats(z, t).tolist(), z.size(0))


def alignment(z1: Tensor, z2: Tensor, alpha: float = 2.0) -> float:
    """The mean over rows of ||zn1_i - zn2_i||^alpha, rows normalised to the unit sphere.  One read-back."""
    return float(O.repr_alignment_sum(z1, z2, alpha).item()) / z1.size(0)


def rankme_from_gram(gram: np.ndarray, colsum: np.ndarray, n: int, eps: float = 1e-7, center: bool = False) -> float:
    """RankMe from the fp64 Gram matrix Z^T Z (and, with center, the column sums: the Gram of the centred rows is gram - colsum colsum^T / n):
    sigma_k = sqrt(max(lambda_k, 0)) of its d eigenvalues, p = sigma / sum(sigma) + eps, exp(-sum p log p)."""
    g = np.asarray(gram, dtype=np.float64)
    if center:
        c = np.asarray(colsum, dtype=np.float64)
        g = g - np.outer(c, c) / n
    sigma = np.sqrt(np.maximum(np.linalg.eigvalsh(g), 0.0))
    total = sigma.sum()
    if not total > 0.0:          # an all-zero matrix has no spectrum to speak of: p = eps everywhere
        total = 1.0
    p = sigma / total + eps
    return float(np.exp(-(p * np.log(p)).sum()))


def _gram_host(z: Tensor):
    gram, colsum = O.repr_gram(z)
    d = z.size(1)
    flat = torch.cat([gram.reshape(-1), colsum]).cpu().numpy()          # one copy
    return flat[:d * d].reshape(d, d), flat[d * d:]


def rankme(z: Tensor, eps: float = 1e-7, center: bool = False) -> float:
    """The effective rank of z [n, d] (the rows as they are, not normalised).  One read-back; the eigenvalues are computed on the host."""
    gram, colsum = _gram_host(z)
    return rankme_from_gram(gram, colsum, z.size(0), eps, center)


def embedding_stats(z: Tensor, t: float = 2.0) -> Dict[str, float]:
    """uniformity, mean_cosine and rankme of z [n, d], n >= 2, in one dict.  Two read-backs."""
    out = uniformity(z, t)
    out["rankme"] = rankme(z)
    return out
