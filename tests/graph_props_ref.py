"""Shared by test_graph_props_host.py and test_gpu_graph_props.py: the slot table of gmp_graph_props (include/gnnmp.h) in pure Python
integers from an edge list -- sets for the adjacency, BFS for components and diameter, fractions.Fraction for the clustering sum --
plus the graph makers and the batch collation the tests use.  Shares no code with the kernel, with scipy or with the calculator."""
import random
from collections import deque
from fractions import Fraction

import numpy as np
import torch

SLOTS = 16

# The float bar of the 12 targets.  Measured on the CPU over the 15 graphs of test_graph_props_host.FORMULA_GRAPHS and the 60 kernel-sized
# graphs of end_to_end_graphs() below: the largest |properties_from_counts(ref_counts(g)) - GraphPropertyCalculator()(g)|, both cast to
# float32, is 0.0 -- all 900 values agree bit for bit (the existing calculator is the reference of that number, never the new code).  The
# scipy path sums in fp64 in another order than the integer form, hence a margin of 4 x the worst case; 4 x 0 is 0, so what holds is the
# floor: one float32 ulp of the value.
MEASURED_WORST = 0.0
FLOAT_BAR = 4.0 * MEASURED_WORST


def within_float_bar(got, want):
    """got, want: float32 tensors of one shape.  |got - want| <= max(FLOAT_BAR, one float32 ulp of want), element by element."""
    got, want = got.to(torch.float32), want.to(torch.float32)
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    return bool(((got.double() - want.double()).abs() <= torch.clamp(ulp, min=FLOAT_BAR)).all())


def ref_counts(n, pairs):
    """(slots 0..15 as a list of ints, clustering sum as a Fraction) of the simple undirected graph on n nodes whose edge list is
    `pairs` (local ids): self loops dropped, duplicates and mirrored pairs merged, a pair with an endpoint outside [0, n) dropped and
    each such endpoint counted in the status slot."""
    adj = [set() for _ in range(n)]
    dropped = 0
    for a, b in pairs:
        bad = (0 if 0 <= a < n else 1) + (0 if 0 <= b < n else 1)
        dropped += bad
        if bad == 0 and a != b:
            adj[a].add(b)
            adj[b].add(a)
    deg = [len(s) for s in adj]
    t2 = [sum(len(adj[v] & adj[u]) for u in adj[v]) for v in range(n)]
    csum = sum((Fraction(t2[v], deg[v] * (deg[v] - 1)) for v in range(n) if deg[v] >= 2), Fraction(0))

    def bfs(src):
        dist = {src: 0}
        q = deque([src])
        while q:
            v = q.popleft()
            for u in adj[v]:
                if u not in dist:
                    dist[u] = dist[v] + 1
                    q.append(u)
        return dist

    seen, comps = set(), []
    for v in range(n):                                      # components in order of their smallest node id
        if v not in seen:
            members = sorted(bfs(v))
            seen.update(members)
            comps.append(members)
    diameter = 0
    if comps:
        big = max(comps, key=len)                           # max() keeps the first of equals: the smallest node id
        if len(big) > 1:
            diameter = max(max(bfs(v).values()) for v in big)
    sdeg = sum(deg)
    slots = [n, sdeg // 2, max(deg, default=0), sdeg, sum(d * d for d in deg), sum(t2), sum(d * (d - 1) for d in deg), len(comps), diameter,
             sum(deg[u] * deg[v] for v in range(n) for u in adj[v]), sum(d * d for d in deg), sum(d ** 3 for d in deg), dropped << 8, 0, 0, 0]
    return slots, csum


# ---------------------------------------------------------------------------------------------------------------------
# graphs: (n, list of (a, b) pairs, each undirected edge once)
# ---------------------------------------------------------------------------------------------------------------------
def path(n):
    return n, [(i, i + 1) for i in range(n - 1)]


def cycle(n):
    return n, [(i, (i + 1) % n) for i in range(n)]


def star(n):
    return n, [(0, i) for i in range(1, n)]


def complete(n):
    return n, [(i, j) for i in range(n) for j in range(i + 1, n)]


def empty(n):
    return n, []


def gnp(n, p, seed):
    rng = random.Random(seed)
    return n, [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < p]


def cubic(n, isolated=0):
    """3-regular on n (even) nodes -- a cycle plus the antipodal chords -- followed by `isolated` nodes without edges."""
    assert n % 2 == 0 and n >= 4
    return n + isolated, [(i, (i + 1) % n) for i in range(n)] + [(i, i + n // 2) for i in range(n // 2)]


def two_components(first_is_path):
    """Two components of 4 nodes, a path (diameter 3) and a star (diameter 2), in both id orders (tests/test_data.py)."""
    if first_is_path:
        return 8, [(0, 1), (1, 2), (2, 3), (4, 5), (4, 6), (4, 7)]
    return 8, [(0, 1), (0, 2), (0, 3), (4, 5), (5, 6), (6, 7)]


def messy(n, pairs, seed):
    """The same graph as a messy list: self loops added, each edge 1-3 times in a random direction, shuffled."""
    rng = random.Random(seed)
    out = [(v, v) for v in range(n) if rng.random() < 0.3]
    for a, b in pairs:
        for _ in range(rng.randint(1, 3)):
            out.append((a, b) if rng.random() < 0.5 else (b, a))
    rng.shuffle(out)
    return n, out


def both_directions(pairs):
    return list(pairs) + [(b, a) for a, b in pairs]


def collate(graphs):
    """[(n, pairs)] -> (ptr int64 [B+1], eptr int64 [B+1], edge_index int64 [2, E]) with batch-global ids, CPU tensors."""
    ptr, eptr, src, dst = [0], [0], [], []
    for n, pairs in graphs:
        src += [a + ptr[-1] for a, _ in pairs]
        dst += [b + ptr[-1] for _, b in pairs]
        ptr.append(ptr[-1] + n)
        eptr.append(eptr[-1] + len(pairs))
    return (torch.tensor(ptr, dtype=torch.int64), torch.tensor(eptr, dtype=torch.int64),
            torch.tensor([src, dst], dtype=torch.int64).reshape(2, len(src)))


def as_data(n, pairs):
    """The graph as the library's Data object, every edge in both directions (local ids)."""
    from gnn_pretraining_amd.graph import Data
    ei = torch.tensor(both_directions(pairs), dtype=torch.int64).reshape(-1, 2).t().contiguous()
    return Data(torch.zeros(n, 1), ei)


def end_to_end_graphs():
    """60 random graphs of 3..126 nodes and one of 1025 (too large for the kernel: the fallback) as Data objects."""
    rng = random.Random(2024)
    out = []
    for k in range(60):
        n = rng.randint(3, 126)
        out.append(as_data(*gnp(n, rng.choice([0.02, 0.05, 0.1, 0.3]), 1000 + k)))
    out.insert(17, as_data(*gnp(1025, 0.003, 77)))
    return out
