"""Shared by test_repr_host.py and test_gpu_repr_stats.py: the float64 definitions of the label-free embedding statistics of
csrc/repr_stats.hip and gnn_pretraining_amd/repr_stats.py, written from the contract (gnnmp.h gmp_repr_*) and not from the kernels.

  normalize       z / max(||z||, 1e-12) per row, in fp64 from the fp32 values (a zero row stays zero)
  pair_stats      (sum over i < j of exp(-2 t (1 - s_ij)), sum over i < j of s_ij), s = normalize(z) normalize(z)^T, the upper triangle
  alignment_sum   sum over i of max(0, 2 - 2 <zn1_i, zn2_i>)^(alpha / 2)
  gram            (Z^T Z, column sums) -- in int64 when the rows are integers, else fp64
  rankme          exp of the entropy of p = sigma / sum(sigma) + eps over the d singular values of Z (np.linalg.svd, padded with zeros to d)
plus the two exact-arithmetic row generators."""
import numpy as np

from knn_ref import four_ones  # noqa: F401  (rows with four ones: norm 2, every s_ij a multiple of 0.25)


def normalize(z):
    z = np.asarray(z, dtype=np.float64)
    return z / np.maximum(np.sqrt((z * z).sum(axis=1, keepdims=True)), 1e-12)


def pair_stats(z, t=2.0):
    zn = normalize(z)
    s = (zn @ zn.T)[np.triu_indices(zn.shape[0], k=1)]
    return float(np.exp(-2.0 * t * (1.0 - s)).sum()), float(s.sum())


def uniformity(z, t=2.0):
    n = np.asarray(z).shape[0]
    e, c = pair_stats(z, t)
    pairs = n * (n - 1) / 2
    return {"uniformity": float(np.log(e / pairs)), "mean_cosine": c / pairs}


def alignment_sum(z1, z2, alpha=2.0):
    s = (normalize(z1) * normalize(z2)).sum(axis=1)
    return float((np.maximum(0.0, 2.0 - 2.0 * s) ** (alpha / 2.0)).sum())


def gram(z):
    z = np.asarray(z)
    z = z.astype(np.int64) if np.all(z == np.round(z)) else z.astype(np.float64)
    return z.T @ z, z.sum(axis=0)


def entropy_rank(sigma, eps=1e-7):
    sigma = np.asarray(sigma, dtype=np.float64)
    p = sigma / sigma.sum() + eps
    return float(np.exp(-(p * np.log(p)).sum()))


def rankme(z, eps=1e-7, center=False):
    z = np.asarray(z, dtype=np.float64)
    if center:
        z = z - z.mean(axis=0, keepdims=True)
    sigma = np.zeros(z.shape[1])
    sv = np.linalg.svd(z, compute_uv=False)
    sigma[:sv.size] = sv
    return entropy_rank(sigma, eps)


def integer_rows(n, d, seed):
    """integer rows in [-8, 8]: every product and every partial sum of a Gram matrix is an exact integer in fp64"""
    return np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(np.float32)
