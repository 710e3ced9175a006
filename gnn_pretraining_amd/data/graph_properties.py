"""The 12 structural targets of the graph-property task (src/data/graph_properties.py:17-96), computed from the
sparse adjacency with numpy / scipy instead of a networkx object per graph.

Order (graph_properties.py:62-75): N, E, density, mean degree, degree variance, max degree, average clustering,
transitivity, #components, diameter of the largest component, degree assortativity, degree centralisation -- on the
simple undirected graph (self loops removed, both directions merged, graph_properties.py:21-24).
tests/test_data.py holds this against oracle/graph_properties.py (the networkx restatement of the reference).

compute_for_dataset(..., device=...) makes the same targets for whole batches on the GPU: ops.graph_properties (csrc/graph_props.hip)
returns exact integer counts per graph and properties_from_counts finishes them here, in the integer form of the formulas below."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import scipy.sparse as sp
import torch
from scipy.sparse import csgraph
from torch import Tensor

from ..graph import Data

GRAPH_PROPERTY_DIM = 12
DEVICE_CHUNK_NODES = 65536      # nodes per collated chunk of compute_for_dataset(device=...): one launch and one read-back each


def _simple_adjacency(edge_index: np.ndarray, n: int) -> sp.csr_matrix:
    s, d = edge_index[0], edge_index[1]
    keep = s != d
    s, d = s[keep], d[keep]
    a = sp.coo_matrix((np.ones(2 * s.size, dtype=np.float64), (np.concatenate([s, d]), np.concatenate([d, s]))),
                      shape=(n, n)).tocsr()
    a.data[:] = 1.0              # duplicates were summed by tocsr(); the graph is simple
    return a


class GraphPropertyCalculator:
    def __call__(self, graph: Data) -> Tensor:
        n = int(graph.num_nodes)
        a = _simple_adjacency(graph.edge_index.cpu().numpy().astype(np.int64), n)
        deg = np.asarray(a.sum(axis=1)).reshape(-1)
        e = float(deg.sum() / 2.0)
        deg_mean, deg_var, deg_max = float(deg.mean()), float(deg.var()), float(deg.max())
        density = 0.0 if (n <= 1 or e == 0) else 2.0 * e / (n * (n - 1))

        # t2[v] = 2 * (#triangles through v) = sum over neighbours of the common-neighbour count
        t2 = np.asarray((a @ a).multiply(a).sum(axis=1)).reshape(-1)
        pairs = deg * (deg - 1.0)
        local = np.divide(t2, pairs, out=np.zeros_like(t2), where=pairs > 0)
        clustering = float(local.mean())
        transitivity = 0.0
        if n > 2 and t2.sum() > 0:
            transitivity = float(t2.sum() / pairs.sum())

        ncomp, label = csgraph.connected_components(a, directed=False)
        sizes = np.bincount(label, minlength=ncomp)
        # largest component; ties go to the one holding the smallest node id (networkx yields components in that order)
        first = np.full(ncomp, n, dtype=np.int64)
        np.minimum.at(first, label, np.arange(n))
        big = min(range(ncomp), key=lambda c: (-sizes[c], first[c]))
        members = np.nonzero(label == big)[0]
        if members.size <= 1:
            diameter = 0.0
        else:
            dist = csgraph.shortest_path(a[members][:, members], method="D", unweighted=True)
            diameter = float(dist.max())

        assort = 0.0
        if deg_var != 0.0 and e > 0:
            coo = a.tocoo()
            x, y = deg[coo.row], deg[coo.col]          # every undirected edge appears in both directions
            vx = float((x * x).mean() - x.mean() ** 2)
            if vx > 0:
                assort = float(((x * y).mean() - x.mean() * y.mean()) / vx)
            if math.isnan(assort) or math.isinf(assort):
                assort = 0.0

        central = float((deg_max - deg).sum() / ((n - 1) * (n - 2))) if n > 2 else 0.0
        return torch.tensor([float(n), e, density, deg_mean, deg_var, deg_max, clustering, transitivity, float(ncomp),
                             diameter, assort, central], dtype=torch.float32)

    def compute_for_dataset(self, dataset_list: Sequence[Data], device=None) -> Tensor:
        """device=None: one graph at a time on the host.  With a device: the graphs are collated in chunks of at most
        DEVICE_CHUNK_NODES nodes (a graph larger than that is a chunk of its own), one ops.graph_properties launch and one read-back of
        [B, 16] integers per chunk, properties_from_counts on the host.  A graph the kernel refuses (status bit 0: more than 1024
        nodes) is recomputed by __call__; an edge endpoint outside its graph raises."""
        out = torch.zeros((len(dataset_list), GRAPH_PROPERTY_DIM), dtype=torch.float32)
        if device is not None:
            return self._compute_on_device(dataset_list, torch.device(device), out)
        for i, g in enumerate(dataset_list):
            out[i] = self(g)
        return out

    def _compute_on_device(self, dataset_list: Sequence[Data], device: torch.device, out: Tensor) -> Tensor:
        from .. import ops
        start, total = 0, len(dataset_list)
        while start < total:
            stop, nodes = start, 0
            while stop < total and (stop == start or nodes + int(dataset_list[stop].num_nodes) <= DEVICE_CHUNK_NODES):
                nodes += int(dataset_list[stop].num_nodes)
                stop += 1
            chunk = dataset_list[start:stop]
            sizes = np.array([int(g.num_nodes) for g in chunk], dtype=np.int64)
            esizes = np.array([int(g.edge_index.size(1)) for g in chunk], dtype=np.int64)
            ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            eptr = np.concatenate([[0], np.cumsum(esizes)]).astype(np.int64)
            ei = torch.cat([g.edge_index.cpu().to(torch.int64) + int(o) for g, o in zip(chunk, ptr[:-1])], dim=1).contiguous()
            counts, csum = ops.graph_properties(torch.from_numpy(ptr).to(device), torch.from_numpy(eptr).to(device), ei.to(device),
                                                max_graph_nodes=int(sizes.max()))
            counts, csum = counts.cpu(), csum.cpu()
            out[start:stop] = properties_from_counts(counts, csum)
            status = counts[:, 12].tolist()
            for k, st in enumerate(status):
                if st >> 8:
                    raise ValueError(f"graph {start + k}: {st >> 8} edge endpoint(s) outside its {int(sizes[k])} nodes")
                if st & 1:
                    out[start + k] = self(chunk[k])
            start = stop
        return out

    def compute_and_standardize_for_dataset(self, dataset_list: Sequence[Data], train_idx: np.ndarray, device=None) -> Tensor:
        """graph_properties.py:88-96: StandardScaler fitted on the train split (population std; zero scale -> 1).  Always on the host in
        fp64; `device` only selects where compute_for_dataset makes the raw targets."""
        props = self.compute_for_dataset(dataset_list, device).numpy().astype(np.float64)
        return torch.from_numpy(standardize(props, np.asarray(train_idx))).float()


def properties_from_counts(counts, clustering_sum) -> Tensor:
    """The 12 targets, float32 [B, 12], from the read-back of ops.graph_properties (counts int64 [B, 16] in the slot order of gnnmp.h
    gmp_graph_props, clustering_sum float64 [B]); host tensors, arrays or nested lists.  Python integers throughout (no overflow), one
    correctly rounded division per value, and the guards of GraphPropertyCalculator.__call__.  A row whose status bit 0 is set (the
    kernel refused the graph) comes out as zeros: the caller recomputes it."""
    rows = counts.tolist() if hasattr(counts, "tolist") else [list(r) for r in counts]
    csum = clustering_sum.tolist() if hasattr(clustering_sum, "tolist") else list(clustering_sum)
    out = np.zeros((len(rows), GRAPH_PROPERTY_DIM), dtype=np.float64)
    for i, row in enumerate(rows):
        n, e, dmax, s1, s2, t2, pr, ncomp, diam, sxy, sx, sxx, status = (int(v) for v in row[:13])
        if status & 1 or n == 0:
            continue
        density = 0.0 if (n <= 1 or e == 0) else 2 * e / (n * (n - 1))
        var_num = n * s2 - s1 * s1
        transitivity = t2 / pr if (n > 2 and t2 > 0) else 0.0
        m = 2 * e
        assort = 0.0
        if var_num != 0 and e != 0 and m * sxx != sx * sx:
            assort = (m * sxy - sx * sx) / (m * sxx - sx * sx)
        central = (n * dmax - s1) / ((n - 1) * (n - 2)) if n > 2 else 0.0
        out[i] = [n, e, density, s1 / n, var_num / (n * n), dmax, float(csum[i]) / n, transitivity, ncomp, diam, assort, central]
    return torch.from_numpy(out).to(torch.float32)


def standardize(values: np.ndarray, fit_rows: np.ndarray) -> np.ndarray:
    """sklearn StandardScaler().fit(values[fit_rows]).transform(values) with scale_==0 replaced by 1."""
    ref = values[fit_rows]
    mean, scale = ref.mean(axis=0), ref.std(axis=0)
    scale[scale == 0] = 1.0
    return (values - mean) / scale
