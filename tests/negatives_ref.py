"""numpy checker for the device-side link-prediction negatives (csrc/augment.hip gmp_aug_negative_edges): what ONE graph's undirected
adjacency gives -- cnt, M, whether the host sampler (pretrain/tasks.py negative_sampling_local) would draw, and the ascending list of
non-edge codes i * n + j -- plus builders of the odd edge lists the tests feed.  Not collected as a test."""
import numpy as np
import torch

from gnn_pretraining_amd.graph import Batch, Data


def graph_ref(loc: np.ndarray, n: int, num_neg: int):
    """loc [2, E]: one graph's edges in local numbering (any direction, duplicates, self loops).  -> (cnt, M, no_draw, codes):
    cnt = coalesced undirected non-loop entries, M = n (n - 1) - cnt, no_draw = the sampler returns without a random draw
    (pop <= int(1.1 * num_neg / prob); also True where the graph gives nothing), codes = every non-edge i * n + j, ascending."""
    pop = n * n - n
    adj = np.zeros((n, n), dtype=bool)
    if loc.size:
        adj[loc[0], loc[1]] = True
        adj[loc[1], loc[0]] = True
    np.fill_diagonal(adj, False)
    cnt = int(adj.sum())
    if n < 2 or cnt >= pop:
        return cnt, 0, True, np.zeros(0, dtype=np.int64)
    non = ~adj
    np.fill_diagonal(non, False)
    codes = np.flatnonzero(non.reshape(-1)).astype(np.int64)
    prob = 1.0 - cnt / pop
    return cnt, pop - cnt, pop <= int(1.1 * num_neg / prob), codes


def batch_ref(b: Batch, num_neg: int):
    ei = b.edge_index.numpy()
    out = []
    for g in range(b.num_graphs):
        s, n = b.ptr_host[g], b.ptr_host[g + 1] - b.ptr_host[g]
        out.append(graph_ref(ei[:, b.edge_ptr_host[g]:b.edge_ptr_host[g + 1]] - s, n, num_neg))
    return out


def split_per_graph(b: Batch, neg: np.ndarray):
    """[2, K] pairs in batch numbering, graphs in batch order -> per graph the codes i * n + j (asserts every pair lies inside one graph)."""
    ptr = np.asarray(b.ptr_host)
    g_of = np.searchsorted(ptr, neg[0], side="right") - 1
    assert np.array_equal(g_of, np.searchsorted(ptr, neg[1], side="right") - 1), "a pair crosses graphs"
    assert (np.diff(g_of) >= 0).all(), "graphs out of batch order"
    out = []
    for g in range(b.num_graphs):
        m = g_of == g
        n = ptr[g + 1] - ptr[g]
        out.append((neg[0, m] - ptr[g]) * n + (neg[1, m] - ptr[g]))
    return out


def pairs_graph(n: int, pairs: np.ndarray, rng: np.random.Generator, messy: bool = True) -> Data:
    """A graph of n nodes whose undirected edge set is `pairs` [P, 2] (i < j).  messy: a third of the pairs in one direction only,
    a third in both, a third in both with one direction repeated; plus a few self loops -- all of which the sampler must see through."""
    cols = []
    for q, (i, j) in enumerate(pairs):
        kind = q % 3 if messy else 0
        cols.append((i, j) if q % 2 else (j, i))
        if kind >= 1:
            cols.append((j, i) if q % 2 else (i, j))
        if kind == 2:
            cols.append((i, j))
    if messy and n >= 1:
        cols += [(int(v), int(v)) for v in rng.integers(0, n, size=min(3, n))]
    ei = torch.tensor(cols, dtype=torch.long).t().contiguous() if cols else torch.zeros(2, 0, dtype=torch.long)
    return Data(torch.zeros(n, 4), ei, torch.zeros(1, dtype=torch.long), torch.zeros(12))


def random_pairs(n: int, count: int, rng: np.random.Generator) -> np.ndarray:
    """`count` distinct undirected pairs (i < j) of an n-node graph."""
    iu = np.stack(np.triu_indices(n, 1), axis=1)
    return iu[np.sort(rng.choice(len(iu), size=count, replace=False))] if count else iu[:0]


def density_pairs(n: int, density, rng: np.random.Generator) -> np.ndarray:
    total = n * (n - 1) // 2
    count = {"empty": 0, "sparse": min(total, max(1, n // 2)) if total else 0, "complete": total}.get(density)
    if count is None:
        count = int(round(float(density) * total))
    return random_pairs(n, count, rng)


def filler(columns: int) -> Data:
    """A complete 2-node graph with `columns` edge columns (repeats of (0, 1)): it gives no negatives and lets a batch's edge-column
    count -- the num_neg sample_negative_edges uses -- be set at will."""
    ei = torch.tensor([[0] * columns, [1] * columns], dtype=torch.long)
    return Data(torch.zeros(2, 4), ei, torch.zeros(1, dtype=torch.long), torch.zeros(12))


def threshold_triples(n_values=(4, 5, 7, 10, 13, 17, 24, 31)):
    """(n, cnt, num_neg, no_draw) found by search, per graph size: a triple where the two sides of pop <= int(1.1 * num_neg / prob) are
    EQUAL (cnt > 0, so prob is a rounded quotient), a neighbouring pair of num_neg one step to either side of the threshold, and a no-draw
    triple with num_neg < M (truncation in code order).  Every triple keeps cnt / 2 <= num_neg: the graph's own edge columns fit a batch
    whose column count is num_neg."""
    out = []
    for n in n_values:
        pop = n * n - n
        exact = sides = trunc = None
        for cnt in range(2, pop - 2, 2):
            prob = 1.0 - cnt / pop
            M = pop - cnt
            for num_neg in range(max(cnt // 2, 1), M + 2):
                size = int(1.1 * num_neg / prob)
                if exact is None and size == pop:
                    exact = [(n, cnt, num_neg, True)]
                if sides is None and size < pop <= int(1.1 * (num_neg + 1) / prob) and cnt >= pop // 3:
                    sides = [(n, cnt, num_neg, False), (n, cnt, num_neg + 1, True)]
                if trunc is None and size >= pop and num_neg < M - 2 and cnt >= pop // 2:
                    trunc = [(n, cnt, num_neg, True)]
        out += (exact or []) + (sides or []) + (trunc or [])
    return out
