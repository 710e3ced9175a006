"""Graph containers with the attribute surface the reference uses from
torch_geometric.data (Data / Batch): x, edge_index, batch, ptr, num_graphs,
graph_properties, y, .to(device), to_data_list(), Batch.from_data_list()
(src/pretrain/augmentations.py:91,108-109; src/data/pretrain_data_loaders.py:41;
src/pretrain/pretrain.py:116-117).

Additions for the HIP path: host copies of ``ptr`` / ``edge_ptr`` (so no
``.item()`` sync is ever needed to walk the graphs of a batch) and a per-object
cache of the int32 CSR built by libgnnmp.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor


class SparseFeatures:
    """A node-feature matrix [N, K] in CSR form (int32 ``rowptr`` / ``col``, fp32 ``val``): the bag-of-words features of the
    Planetoid domains (Cora, CiteSeer) keep ~1 % of their entries after NormalizeFeatures (src/data/data_setup.py:154).
    Stands in for a dense ``x`` wherever the input encoder reads it (models/gnn.Linear, finetune/engine.py); ``Data.to`` /
    ``Batch.to`` carry it.  Columns are sorted and unique within a row.  The CSC form the weight gradient reads is built
    once, on first use, and cached (``csc()``); moving the container moves the cached form with it."""

    def __init__(self, rowptr: Tensor, col: Tensor, val: Tensor, shape, csc=None) -> None:
        self.rowptr, self.col, self.val = rowptr, col, val
        self.shape = torch.Size((int(shape[0]), int(shape[1])))
        self._csc = csc                   # (colptr [K+1], row [nnz], val_t [nnz]) once built
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or val.dtype != torch.float32:
            raise TypeError(f"SparseFeatures: int32 rowptr / col and fp32 val expected, got {rowptr.dtype}, {col.dtype}, {val.dtype}")
        if rowptr.numel() != self.shape[0] + 1 or col.numel() != val.numel():
            raise ValueError(f"SparseFeatures: rowptr has {rowptr.numel()} entries for {self.shape[0]} rows, col / val {col.numel()} / {val.numel()}")

    @staticmethod
    def _from_coo(row: Tensor, col: Tensor, val: Tensor, shape) -> "SparseFeatures":
        """(row, col) already in row-major order without duplicates."""
        n = int(shape[0])
        counts = torch.bincount(row, minlength=n) if row.numel() else torch.zeros(n, dtype=torch.long, device=row.device)
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
        rowptr[1:] = counts.cumsum(0)
        return SparseFeatures(rowptr.to(torch.int32), col.to(torch.int32), val.to(torch.float32).contiguous(), shape)

    @staticmethod
    def from_dense(x: Tensor) -> "SparseFeatures":
        if x.dim() != 2:
            raise ValueError(f"SparseFeatures.from_dense: 2-D tensor expected, got {tuple(x.shape)}")
        row, col = (x != 0).nonzero(as_tuple=True)           # row-major order: columns ascending within a row
        return SparseFeatures._from_coo(row, col, x[row, col], x.shape)

    @staticmethod
    def from_torch(t: Tensor) -> "SparseFeatures":
        """From a torch sparse CSR or COO tensor (duplicates summed, columns sorted; stored zeros are kept)."""
        if t.layout not in (torch.sparse_csr, torch.sparse_coo) or t.dim() != 2:
            raise ValueError(f"SparseFeatures.from_torch: a 2-D sparse CSR / COO tensor expected, got {t.layout} {tuple(t.shape)}")
        c = t.to_sparse_coo().coalesce()
        idx = c.indices()
        return SparseFeatures._from_coo(idx[0], idx[1], c.values(), t.shape)

    def to_dense(self) -> Tensor:
        out = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        rows = torch.repeat_interleave(torch.arange(self.shape[0], device=self.device), self.rowptr[1:].long() - self.rowptr[:-1].long())
        out[rows, self.col.long()] = self.val
        return out

    @property
    def device(self) -> torch.device:
        return self.val.device

    @property
    def nnz(self) -> int:
        return int(self.val.numel())

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self) -> int:
        return 2

    def to(self, device, non_blocking: bool = False) -> "SparseFeatures":
        m = lambda t: t.to(device, non_blocking=non_blocking)
        csc = None if self._csc is None else tuple(m(t) for t in self._csc)
        return SparseFeatures(m(self.rowptr), m(self.col), m(self.val), self.shape, csc)

    def cpu(self) -> "SparseFeatures":
        return self.to("cpu")

    def clone(self) -> "SparseFeatures":
        csc = None if self._csc is None else tuple(t.clone() for t in self._csc)
        return SparseFeatures(self.rowptr.clone(), self.col.clone(), self.val.clone(), self.shape, csc)

    def csc(self):
        """(colptr int32 [K+1], row int32 [nnz], val_t fp32 [nnz]): X by columns, ascending row within a column.  Built once:
        on the GPU by gmp_sparse_csc_build (which raises if a column index lies outside [0, K)), on the host by a stable sort."""
        if self._csc is None:
            if self.device.type == "cuda":
                from . import ops
                colptr, row, val_t, status = ops.sparse_csc_build(self)
                if int(status.item()) != 0:
                    raise ValueError(f"SparseFeatures: {int(status.item())} column indices outside [0, {self.shape[1]})")
                self._csc = (colptr, row, val_t)
            else:
                K = self.shape[1]
                col = self.col.long()
                if col.numel() and (int(col.min()) < 0 or int(col.max()) >= K):
                    raise ValueError(f"SparseFeatures: column indices outside [0, {K})")
                rows = torch.repeat_interleave(torch.arange(self.shape[0]), self.rowptr[1:].long() - self.rowptr[:-1].long())
                order = torch.sort(col, stable=True).indices
                colptr = torch.zeros(K + 1, dtype=torch.int64)
                colptr[1:] = torch.bincount(col, minlength=K).cumsum(0)
                self._csc = (colptr.to(torch.int32), rows[order].to(torch.int32), self.val[order].contiguous())
        return self._csc

    def __repr__(self) -> str:
        return f"SparseFeatures(shape={tuple(self.shape)}, nnz={self.nnz}, device={self.device})"


class Data:
    def __init__(self, x: Tensor, edge_index: Tensor, y: Optional[Tensor] = None,
                 graph_properties: Optional[Tensor] = None) -> None:
        self.x, self.edge_index, self.y, self.graph_properties = x, edge_index, y, graph_properties

    @property
    def num_nodes(self) -> int:
        return int(self.x.size(0))

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.size(1))

    @property
    def num_node_features(self) -> int:
        return int(self.x.size(1))

    def clone(self) -> "Data":
        c = lambda t: None if t is None else t.clone()
        return Data(self.x.clone(), self.edge_index.clone(), c(self.y), c(self.graph_properties))

    def to(self, device) -> "Data":
        m = lambda t: None if t is None else t.to(device)
        return Data(self.x.to(device), self.edge_index.to(device), m(self.y), m(self.graph_properties))


class Batch:
    def __init__(self, x, edge_index, batch, ptr, ptr_host: List[int], edge_ptr_host: List[int],
                 y=None, graph_properties=None) -> None:
        self.x, self.edge_index, self.batch, self.ptr = x, edge_index, batch, ptr
        self.ptr_host, self.edge_ptr_host = ptr_host, edge_ptr_host
        self.y, self.graph_properties = y, graph_properties
        self._cache = {}

    # ---- reference-visible surface -------------------------------------------------
    @property
    def num_graphs(self) -> int:
        return len(self.ptr_host) - 1

    @property
    def num_nodes(self) -> int:
        return int(self.x.size(0))

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.size(1))

    @property
    def device(self):
        return self.x.device

    @staticmethod
    def from_data_list(graphs: Sequence[Data]) -> "Batch":
        sizes = [g.num_nodes for g in graphs]
        ptr_h = [0]
        for s in sizes:
            ptr_h.append(ptr_h[-1] + s)
        eptr_h = [0]
        for g in graphs:
            eptr_h.append(eptr_h[-1] + g.num_edges)
        dev = graphs[0].x.device
        x = torch.cat([g.x for g in graphs], dim=0)
        ei = torch.cat([g.edge_index + off for g, off in zip(graphs, ptr_h)], dim=1)
        batch = torch.repeat_interleave(torch.arange(len(graphs), device=dev), torch.tensor(sizes, device=dev))
        ptr = torch.tensor(ptr_h, dtype=torch.long, device=dev)
        y = torch.cat([g.y.reshape(-1) for g in graphs]) if graphs[0].y is not None else None
        gp = (torch.cat([g.graph_properties.reshape(-1) for g in graphs])
              if graphs[0].graph_properties is not None else None)
        return Batch(x, ei, batch, ptr, ptr_h, eptr_h, y, gp)

    @staticmethod
    def empty(num_node_features: int, with_properties: bool = True) -> "Batch":
        """A batch of zero graphs (a domain absent from a step, e.g. single-domain validation passes on the stacked engine)."""
        z = torch.zeros(0, dtype=torch.long)
        return Batch(torch.zeros(0, num_node_features), torch.zeros(2, 0, dtype=torch.long), z, torch.zeros(1, dtype=torch.long), [0], [0],
                     z.clone(), torch.zeros(0) if with_properties else None)

    def to_data_list(self) -> List[Data]:
        B = self.num_graphs
        gp = None if self.graph_properties is None else self.graph_properties.view(B, -1)
        out = []
        for g in range(B):
            s, e = self.ptr_host[g], self.ptr_host[g + 1]
            es, ee = self.edge_ptr_host[g], self.edge_ptr_host[g + 1]
            out.append(Data(self.x[s:e], self.edge_index[:, es:ee] - s,
                            None if self.y is None else self.y[g:g + 1], None if gp is None else gp[g]))
        return out

    def to(self, device) -> "Batch":
        m = lambda t: None if t is None else t.to(device, non_blocking=True)
        out = Batch(m(self.x), m(self.edge_index), m(self.batch), m(self.ptr), self.ptr_host, self.edge_ptr_host,
                    m(self.y), m(self.graph_properties))
        if self.x.device.type == "cpu":
            out._cache["host"] = self        # index work (augmentation, sampling) stays on the host copy
        return out

    def host(self) -> "Batch":
        """The CPU twin of this batch (kept when the batch was moved with .to(); otherwise one D2H copy)."""
        if self.x.device.type == "cpu":
            return self
        if "host" not in self._cache:
            m = lambda t: None if t is None else t.cpu()
            self._cache["host"] = Batch(m(self.x), m(self.edge_index), m(self.batch), m(self.ptr), self.ptr_host,
                                        self.edge_ptr_host, m(self.y), m(self.graph_properties))
        return self._cache["host"]

    # ---- HIP-path extras -----------------------------------------------------------
    @property
    def ptr32(self) -> Tensor:
        """Graph row offsets as device int32 (segment pointer for the pooling kernels)."""
        if "ptr32" not in self._cache:
            self._cache["ptr32"] = torch.tensor(self.ptr_host, dtype=torch.int32).to(self.x.device)
        return self._cache["ptr32"]

    @property
    def max_graph_nodes(self) -> int:
        return max((b - a for a, b in zip(self.ptr_host[:-1], self.ptr_host[1:])), default=0)
