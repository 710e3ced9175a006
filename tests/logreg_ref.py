"""Shared by test_logreg_host.py and test_gpu_logreg.py: the float64 definition of the linear-evaluation probe of csrc/logreg.hip
(gnnmp.h gmp_logreg_fit / gmp_logreg_predict), written from the contract and not from the kernels.

  normalize   knn_ref.normalize: z / max(||z||, 1e-12) per row (a zero row stays zero)
  logits      xn W^T + b
  loss_grad   L = S_L / n + (l2 / 2) sum(W^2) with S_L the sum of logsumexp(z_i) - z[i, y_i]; gW = S_W / n + l2 W, gb = S_b / n with
              S_W = (p - onehot)^T xn and S_b the column sums of p - onehot.  A row whose label lies outside [0, C) contributes nothing;
              n stays n.  Returns (L, g [C, d + 1] = (gW | gb), status = the number of such rows)
  adam_step   torch.optim.Adam's rule (no amsgrad) with b1 = 0.9, b2 = 0.999, eps = 1e-8 on any array: t is the step count AFTER this
              update; returns (theta, m, v) and writes nothing
  fit         `iters` updates of the block (W | b) from a state (zeros by default); loss_history[k] = L before update k
  predict     argmax of the logits, the first maximum (ties to the lower class)
  blobs       the data of the whole-fit tests: x = centre[y] + noise * randn, y = i % C, from torch.Generator().manual_seed(0)"""
import numpy as np

from knn_ref import normalize

B1, B2, EPS = 0.9, 0.999, 1e-8


def logits(xn, W, b):
    return np.asarray(xn, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)


def loss_grad(xn, y, W, b, l2=0.0):
    xn, W, b, y = np.asarray(xn, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(y)
    n, C = xn.shape[0], W.shape[0]
    z = logits(xn, W, b)
    zmax = z.max(axis=1, keepdims=True)
    e = np.exp(z - zmax)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    ok = (y >= 0) & (y < C)
    yc = np.where(ok, y, 0)
    rows = np.arange(n)
    row_loss = (zmax[:, 0] + np.log(s[:, 0])) - z[rows, yc]
    g = p.copy()
    g[rows, yc] -= 1.0
    g[~ok] = 0.0
    L = row_loss[ok].sum() / n + 0.5 * l2 * (W * W).sum()
    gW = g.T @ xn / n + l2 * W
    gb = g.sum(axis=0) / n
    return float(L), np.concatenate([gW, gb[:, None]], axis=1), int((~ok).sum())


def adam_step(theta, g, m, v, t, lr):
    theta, g, m, v = (np.asarray(a, dtype=np.float64) for a in (theta, g, m, v))
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    theta = theta - lr / (1.0 - B1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - B2 ** t) + EPS)
    return theta, m, v


def fit(x, y, num_classes, iters=100, lr=0.01, l2=0.0, state=None):
    """(W [C, d], b [C], m, v [C, d + 1], t, loss_history [iters]) in float64; state = (W, b, m, v, t) or None for zeros"""
    xn = normalize(x)
    d = xn.shape[1]
    if state is None:
        theta, m, v, t = np.zeros((num_classes, d + 1)), np.zeros((num_classes, d + 1)), np.zeros((num_classes, d + 1)), 0
    else:
        W, b, m, v, t = state
        theta = np.concatenate([np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)[:, None]], axis=1)
        m, v, t = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64), int(t)
    history = np.zeros(iters)
    for k in range(iters):
        history[k], g, _ = loss_grad(xn, y, theta[:, :d], theta[:, d], l2)
        t += 1
        theta, m, v = adam_step(theta, g, m, v, t, lr)
    return theta[:, :d].copy(), theta[:, d].copy(), m, v, t, history


def predict(x, W, b):
    """(pred [n] int64, logits [n, C] float64)"""
    z = logits(normalize(x), W, b)
    return z.argmax(axis=1).astype(np.int64), z                     # the first maximum


BLOB_CASES = [(700, 64, 7, 1.0), (700, 256, 7, 1.0), (1000, 256, 32, 1.0), (300, 40, 2, 1.0)]         # (n, d, C, noise)


def blobs(n, d, num_classes, noise=1.0):
    """(x float32 [n, d], y int64 [n]) as numpy arrays; centres, then noise, both drawn in float64 and the sum rounded to float32"""
    import torch
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(num_classes, d, generator=g, dtype=torch.float64)
    y = torch.arange(n) % num_classes
    x = centres[y] + noise * torch.randn(n, d, generator=g, dtype=torch.float64)
    return x.float().numpy(), y.numpy()
