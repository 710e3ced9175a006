"""Host half of the stacked step (engine.py holds the device half): the step's random index draws -- the reference's exact draw order
(csrc_host/hostdraw.cpp, or the Python loop it mirrors), the numpy "vectorized" draws, the stream of link-prediction negatives -- and
its layout as upload arrays (StepHost.plan in numpy, hostdraw.plan_step natively: the same arrays).  No GPU, no libgnnmp.so."""
from __future__ import annotations

import os
import random
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import GnnmpError
from .constants import GRAPH_PROPERTY_DIM
from .graph import Batch
from .models.gnn import GNN_HIDDEN_DIM
from .models.pretrain_model import draw_mask_indices
from .pretrain.augmentations import _augment_one
from .pretrain.tasks import sample_negative_edges

H = GNN_HIDDEN_DIM
SUPPORTED_TASKS = ("node_feat_mask", "link_pred", "node_contrast", "graph_contrast", "graph_prop", "domain_adv")


class StepInputs:
    """Device-resident input of one step (the benchmark keeps a pool of these in HBM):
    all domains' features padded into one matrix + per-domain offsets, plus host twins for index work."""

    def __init__(self, batches: Dict[str, Batch], device, dpad: int) -> None:
        self.domains = list(batches)
        self.host = {d: b.host() for d, b in batches.items()}
        rows, self.row_off = 0, {}
        for d in self.domains:
            self.row_off[d] = rows
            rows += self.host[d].num_nodes
        pin = torch.device(device).type == "cuda"
        x = torch.zeros(rows, dpad, pin_memory=pin)           # pinned (cached by torch's host allocator): the copy below is asynchronous
        gp = []
        for d in self.domains:
            hb = self.host[d]
            x[self.row_off[d]:self.row_off[d] + hb.num_nodes, :hb.x.size(1)] = hb.x
            gp.append(hb.graph_properties.to(torch.float32).view(hb.num_graphs, GRAPH_PROPERTY_DIM))
        self.x_all = x.to(device, non_blocking=pin)
        g = torch.cat(gp)
        self.graph_props = (g.pin_memory() if pin else g).to(device, non_blocking=pin)           # [sum B, 12] in domain order
        self.device = torch.device(device)
        self._dev_graph: Dict[str, tuple] = {}

    def dev_graph(self, d: str):
        """(ptr, eptr, edge_index, view_ptr, mask_ptr) of domain d's batch as int64 device tensors (batch-local numbering; view_ptr /
        mask_ptr = exclusive scans of the per-graph kept-node / masked-node counts, functions of the graph sizes alone) + the two scans
        as numpy arrays -- what the device-side augmentation kernels read; uploaded once per input, on first use (a pageable-memory
        upload synchronises with the stream it is made on: never do it per step)."""
        t = self._dev_graph.get(d)
        if t is None:
            hb = self.host[d]
            dev = self.device
            kept, masked = L_view_sizes(hb.ptr_host)
            vptr = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
            moff = np.concatenate([[0], np.cumsum(masked)]).astype(np.int64)
            t = self._dev_graph[d] = (torch.tensor(hb.ptr_host, dtype=torch.long).to(dev), torch.tensor(hb.edge_ptr_host, dtype=torch.long).to(dev),
                                      hb.edge_index.contiguous().to(dev), torch.from_numpy(vptr).to(dev), torch.from_numpy(moff).to(dev), vptr, moff)
        return t


class StepPlan:
    """Host-side description of one stacked step (pure index data)."""


class Artefacts(dict):
    """draw()'s result {task: {domain: arrays}}; `raw` keeps the native module's own tuples (hostdraw.draw_step) for the native layout
    step (hostdraw.plan_step), which never touches the numpy copies -- so those are only built (`fill`) when somebody reads the dict
    (tests, the oracle harness, the Python layout)."""
    raw = None
    fill = None

    def _need(self) -> None:
        f, self.fill = self.fill, None
        if f is not None:
            f(self)

    def __getitem__(self, k):
        self._need()
        return dict.__getitem__(self, k)

    def __iter__(self):
        self._need()
        return dict.__iter__(self)

    def __len__(self):
        self._need()
        return dict.__len__(self)

    def __contains__(self, k):
        self._need()
        return dict.__contains__(self, k)

    def get(self, k, default=None):
        self._need()
        return dict.get(self, k, default)

    def keys(self):
        self._need()
        return dict.keys(self)

    def items(self):
        self._need()
        return dict.items(self)

    def values(self):
        self._need()
        return dict.values(self)


class _Views(dict):
    """Named views into a packed upload image (StepPlan.a32 / a64 of a natively planned step), built on first use."""

    def __init__(self, cat: np.ndarray, lay) -> None:
        super().__init__()
        self._cat, self._lay = cat, {n: (o, k) for n, o, k in lay}

    _SHAPES = {"lp_edges": (2, -1), "edge_index": (2, -1), "tiles": (-1, 2), "lp_pos": (2, -1)}

    def __missing__(self, name):
        o, k = self._lay[name]
        v = self._cat[o:o + k]
        v = v.reshape(self._SHAPES[name]) if name in self._SHAPES else v
        self[name] = v
        return v

    def __contains__(self, name) -> bool:
        return name in self._lay


class ViewArrays:
    """One augmented view of a whole domain batch as flat index arrays (what Batch.from_data_list of the
    augmented graphs would hold, minus the features): rows = kept nodes (domain-local ids of the base batch),
    edges = [2, e'] in view-local numbering, ptr = per-graph node offsets, rowmask = per-row bitmask of zeroed
    feature columns (None if no graph drew an attribute mask), common = view-local ids of nodes kept in BOTH views."""
    __slots__ = ("rows", "edges", "ptr", "rowmask", "common")

    def __init__(self, rows, edges, ptr, rowmask, common) -> None:
        self.rows, self.edges, self.ptr, self.rowmask, self.common = rows, edges, ptr, rowmask, common


def L_view_sizes(ptr_host):
    from .ops import view_sizes
    return view_sizes(ptr_host)


_HOSTDRAW, _HOSTDRAW_TRIED = None, False


def merge_mirrored_pairs(b: Batch, neg: np.ndarray, offset: int, ord_base: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Unordered pairs [2, K'] (+offset), signed multiplicities (+w positive, -w negative; w = 1 or 2) and ordered positions [2, K'] int32 of
    one domain batch's scored pairs (its edges, then the drawn negatives): the LP scorer's features (heads.py:57-61) are symmetric in
    (src, dst), so (i, j) and (j, i) need one row through the 768 -> 256 layer, not two.  The reference drops every ORDERED row with a mask of
    its own (heads.py:44-52), so each merged row remembers the one or two ordered rows it stands for: ord[0] = position of the first
    occurrence in the reference's list (counted from ord_base: this domain's positives, then its negatives), ord[1] = of the second (-1: none).
    A third occurrence of a pair (a duplicated edge) starts a row of its own.  Native (csrc_host/hostdraw.cpp) when built, numpy otherwise;
    both keep first-occurrence order, positives first."""
    H = hostdraw()
    if H is not None:
        ptr, _, ei = _host_tensors(b)
        pairs, w, ord_ = H.merge_mirrored_pairs(ei, torch.from_numpy(np.ascontiguousarray(neg)), ptr, int(offset), int(ord_base))
        return pairs.numpy(), w.numpy(), ord_.numpy()
    out_p, out_w, out_o, n = [], [], [], max(b.num_nodes, 1)
    base = int(ord_base)
    for sign, e in ((1.0, b.edge_index.numpy()), (-1.0, neg)):
        lo, hi = np.minimum(e[0], e[1]), np.maximum(e[0], e[1])
        key = lo * n + hi
        order = np.argsort(key, kind="stable")
        sk = key[order]
        ar = np.arange(len(sk))
        start = np.ones(len(sk), dtype=bool)
        start[1:] = sk[1:] != sk[:-1]
        rank = ar - np.maximum.accumulate(np.where(start, ar, 0))           # occurrence number of every entry among its equals
        lead = np.flatnonzero(rank % 2 == 0)                                    # sorted positions that open a row
        nxt = np.minimum(lead + 1, len(sk) - 1)
        has2 = (lead + 1 < len(sk)) & (sk[nxt] == sk[lead]) if len(sk) else np.zeros(0, dtype=bool)
        first = order[lead]
        second = np.where(has2, order[nxt], -1)
        emit = np.argsort(first, kind="stable")                                 # rows in first-occurrence order
        first, second, has2 = first[emit], second[emit], has2[emit]
        out_p.append(np.stack([lo[first], hi[first]]) + offset)
        out_w.append((sign * (1 + has2)).astype(np.float32))
        out_o.append(np.stack([first + base, np.where(has2, second + base, -1)]).astype(np.int32))
        base += e.shape[1]
    return np.concatenate(out_p, axis=1), np.concatenate(out_w), np.concatenate(out_o, axis=1)


def hostdraw():
    """The native module for the reference-order draws (csrc_host/hostdraw.cpp), or None when it has not been built: the
    Python implementations it mirrors then run instead (bit-identical, ~10x slower, and they hold the GIL)."""
    global _HOSTDRAW, _HOSTDRAW_TRIED
    if not _HOSTDRAW_TRIED:
        _HOSTDRAW_TRIED = True
        if os.environ.get("GMP_NO_HOSTDRAW") is None:
            try:
                from . import _hostdraw
                _HOSTDRAW = _hostdraw
            except ImportError:
                _HOSTDRAW = None
    return _HOSTDRAW


def _host_tensors(b: Batch):
    """(node ptr, edge ptr, contiguous edge_index) of a host batch as the int64 tensors the native draw module takes, built once
    per batch object (they were rebuilt for every task of every step: 24 torch.tensor calls per step)."""
    t = b._cache.get("host_tensors")
    if t is None:
        t = b._cache["host_tensors"] = (torch.tensor(b.ptr_host, dtype=torch.long), torch.tensor(b.edge_ptr_host, dtype=torch.long),
                                        b.edge_index.contiguous())
    return t


def _draw_args(inp: StepInputs, domains: Sequence[str]) -> list:
    """Per-domain (node ptr, edge ptr, edge_index, feature count) as hostdraw.draw_step / plan_step take them (the tensors are cached)."""
    return [_host_tensors(inp.host[d]) + (int(inp.host[d].x.size(1)),) for d in domains]


def _empty_views():
    z, e = np.zeros(0, dtype=np.int64), np.zeros((2, 0), dtype=np.int64)
    return (ViewArrays(z, e, np.zeros(1, dtype=np.int64), None, z), ViewArrays(z.copy(), e.copy(), np.zeros(1, dtype=np.int64), None, z.copy()))


# what draw() records for a domain that has no graph in this step
_EMPTY_ART = {"node_feat_mask": lambda: np.zeros(0, dtype=np.int64), "link_pred": lambda: np.zeros((2, 0), dtype=np.int64),
              "node_contrast": _empty_views, "graph_contrast": lambda: None, "domain_adv": lambda: None}


class StepHost:
    """draw() (all RNG of a step as index arrays) and plan() (the step laid out as segments, packed into its two upload images).
    Works on its own (the CPU tests, scripts/diag_host_costs.py) and is the base of StepEngine, which adds all that touches the device."""

    def __init__(self, tasks: Sequence[str], domains: Sequence[str], seed: int = 0, rng_mode: str = "reference",
                 neg_rng: Optional[random.Random] = None, max_rows: int = 16384, max_edges: int = 131072) -> None:
        for t in tasks:
            if t not in SUPPORTED_TASKS:
                raise NotImplementedError(f"StepEngine covers {SUPPORTED_TASKS}; '{t}' runs on the module path")
        if rng_mode not in ("reference", "vectorized", "device"):
            raise ValueError("rng_mode must be 'reference', 'vectorized' or 'device'")
        self.tasks, self.domains = list(tasks), list(domains)
        self.seed, self.rng_mode, self._nprng = seed, rng_mode, None
        self.max_rows, self.max_edges = max_rows, max_edges
        self.S_MAX, self.KMAX = 64, max_edges          # segments of one step; link-prediction rows of one step
        # Link-prediction negatives: PyG's sampler draws from Python's `random` (the global, unseeded module in the reference), never
        # from the shared torch generator (pretrain/tasks.py sample_negative_edges).  The engine keeps a stream of its own.
        self.neg_rng = neg_rng if neg_rng is not None else random.Random(0x9E3779B1 * (seed + 1))
        self._neg_native = None
        # score each unordered pair once (the scorer is symmetric in (src, dst)); GMP_LP_MERGE=0 keeps the reference's ordered list
        self.lp_merge = os.environ.get("GMP_LP_MERGE", "1") != "0"
        # row ranges of the stacked forward (gnnmp_step.h fwd_cut_*): GMP_FWD_RANGES = 1 (one pass on main), 2 (default), 3 (measured equal or
        # slightly worse: 1.474-1.484 against 1.455-1.485 ms per step)
        self.fwd_ranges = max(1, min(3, int(os.environ.get("GMP_FWD_RANGES", "2"))))
        self.native_plan = os.environ.get("GMP_NATIVE_PLAN", "1") != "0"

    # what the packed per-step index uploads may hold (the engine's pinned staging buffers have these sizes): functions of the capacities
    i32_cap = property(lambda self: 4 * self.max_rows + 8 * self.S_MAX + 65536 + 2 * self.max_edges)
    i64_cap = property(lambda self: 4 * self.max_edges + 8 * self.max_rows)

    def draw(self, inp: StepInputs, gen: torch.Generator) -> Dict[str, object]:
        """All RNG of one step as index arrays, tasks in ACTIVE_TASKS order, domains in dict order.
        rng_mode 'reference': the reference's exact draw sequence from the caller's CPU torch.Generator (bit-identical
        indices for an equal generator state; per-graph Python loop).  rng_mode 'vectorized': the same distributions
        drawn for all graphs of a domain at once with numpy (different stream, ~10x less host time)."""
        if self.rng_mode == "vectorized":
            return self._draw_vectorized(inp, gen)
        if self.rng_mode == "device":
            raise GnnmpError("engine: rng_mode 'device' draws on the GPU and needs a StepEngine")
        art: Dict[str, object] = {}
        host = {d: inp.host[d] for d in self.domains}
        H = hostdraw()
        if H is not None:
            # one native call for the whole step (GIL released once, generator locked once): the launcher thread's Python is not held up
            # by sixteen hand-overs per step
            kinds = [self.DRAWN_TASKS.index(t) for t in self.tasks if t in self.DRAWN_TASKS]
            art = Artefacts()
            art.raw = H.draw_step(kinds, _draw_args(inp, self.domains), gen, self._native_negatives())
            tasks, names = [t for t in self.tasks if t in self.DRAWN_TASKS], list(host)

            def fill(a: Artefacts) -> None:
                for t, row in zip(tasks, a.raw):
                    out = {}
                    for d, r in zip(names, row):
                        if r is None:
                            out[d] = None
                        elif len(r) == 0:
                            out[d] = _EMPTY_ART[t]()
                        elif len(r) == 1:
                            out[d] = r[0].numpy()
                        else:
                            out[d] = tuple(ViewArrays(*(x.numpy() for x in r[5 * v:5 * v + 3]),
                                                      r[5 * v + 3].numpy().view(np.uint64) if r[5 * v + 3].numel() else None, r[5 * v + 4].numpy())
                                           for v in range(2))
                    dict.__setitem__(a, t, out)

            art.fill = fill
            return art
        for t in self.tasks:                # no native module: the Python implementations it mirrors, task by task
            if t in self.DRAWN_TASKS:
                art[t] = {d: self.draw_task(t, b, gen) for d, b in host.items()}
        return art

    DRAWN_TASKS = ("node_feat_mask", "link_pred", "node_contrast", "graph_contrast")

    def draw_task(self, t: str, b: Batch, gen: torch.Generator):
        """The reference-order draws of ONE task for ONE domain batch -- what task.compute_loss({domain: batch}, generator)
        consumes from the generator (validation walks tasks x domains x batches in that order, pretrain.py:211-221)."""
        if b.num_graphs == 0:
            return _EMPTY_ART[t]()
        H = hostdraw()
        if t == "node_feat_mask":
            return (H.mask_indices(_host_tensors(b)[0], gen) if H is not None else draw_mask_indices(b.ptr_host, gen)).numpy()
        if t == "link_pred":
            return self._negatives(b)
        if t in ("node_contrast", "graph_contrast"):
            return self._draw_views(b, gen) if (t == "node_contrast" or b.num_graphs >= 2) else None
        raise KeyError(t)

    @staticmethod
    def empty_art(t: str):
        return _EMPTY_ART[t]()

    def _negatives(self, b: Batch) -> np.ndarray:
        """batched_negative_sampling(to_undirected(pos), batch, num_neg_samples=E) of one domain batch from the engine's Python-random
        stream: the native CPython-compatible MT19937 (csrc_host/hostdraw.cpp PyRandom, seeded from self.neg_rng's state at first
        use and the owner of the stream from then on) when the module is built, pretrain/tasks.py otherwise -- same negatives."""
        if hostdraw() is None:
            return sample_negative_edges(b, self.neg_rng).numpy()
        return self._native_negatives().negative_edges(*_host_tensors(b)).numpy()

    def _native_negatives(self):
        """The native twin of self.neg_rng (hostdraw.PyRandom), created and seeded from its state at first use."""
        if self._neg_native is None:
            self._neg_native = hostdraw().PyRandom()
            self._neg_native.setstate(torch.tensor(self.neg_rng.getstate()[1], dtype=torch.long))
        return self._neg_native

    def rng_state(self) -> Dict[str, object]:
        """Everything random the host half owns besides the caller's torch.Generator, as plain Python data (pretrain() stores it in the
        checkpoint next to the generator state): the link-prediction negatives' Python-random stream."""
        return {"neg_rng": self.sync_neg_rng().getstate()}

    def set_rng_state(self, st: Dict[str, object]) -> None:
        v, key, g = st["neg_rng"]
        self.neg_rng.setstate((int(v), tuple(int(x) for x in key), g))
        self._neg_native = None                  # re-created from neg_rng at its next use

    def sync_neg_rng(self) -> random.Random:
        """Write the native stream's state back into self.neg_rng (checkpointing / tests) and return it."""
        if self._neg_native is not None:
            st = self.neg_rng.getstate()
            self.neg_rng.setstate((st[0], tuple(int(v) for v in self._neg_native.getstate().tolist()), st[2]))
        return self.neg_rng

    @staticmethod
    def _draw_views(b: Batch, gen: torch.Generator) -> Tuple[ViewArrays, ViewArrays]:
        """Same draws as GraphAugmentor.create_two_views (augmentations.py:88-111), kept as index arrays: the native module
        when it is built, the Python loop below otherwise (bit-identical, tests/test_hostdraw.py)."""
        H = hostdraw()
        if H is None:
            return StepHost._draw_views_python(b, gen)
        r = H.draw_views(*_host_tensors(b), int(b.x.size(1)), gen)
        out = []
        for vi in range(2):
            rows, edges, vptr, rowmask, common = (t.numpy() for t in r[5 * vi:5 * vi + 5])
            out.append(ViewArrays(rows, edges, vptr, rowmask.view(np.uint64) if rowmask.size else None, common))
        return out[0], out[1]

    @staticmethod
    def _draw_views_python(b: Batch, gen: torch.Generator) -> Tuple[ViewArrays, ViewArrays]:
        ei = b.edge_index.numpy()
        F = b.x.size(1)
        acc = [dict(rows=[], edges=[], ptr=[0], masks=[], common=[]) for _ in range(2)]
        for g in range(b.num_graphs):
            s, e = b.ptr_host[g], b.ptr_host[g + 1]
            es, ee = b.edge_ptr_host[g], b.edge_ptr_host[g + 1]
            loc = ei[:, es:ee] - s
            pair = (_augment_one(e - s, loc, F, gen), _augment_one(e - s, loc, F, gen))
            flags = np.zeros((2, e - s), dtype=bool)
            flags[0, pair[0].kept] = True
            flags[1, pair[1].kept] = True
            for vi, v in enumerate(pair):
                a = acc[vi]
                base = a["ptr"][-1]
                a["rows"].append(v.kept + s)
                a["edges"].append(v.edges + base)
                a["common"].append(np.flatnonzero(flags[1 - vi, v.kept]) + base)
                m = 0
                if v.masked_cols is not None:
                    for c in v.masked_cols:
                        m |= 1 << int(c)
                a["masks"].append(np.full(len(v.kept), m, dtype=np.uint64))
                a["ptr"].append(base + len(v.kept))
        out = []
        for a in acc:
            rm = np.concatenate(a["masks"])
            out.append(ViewArrays(np.concatenate(a["rows"]), np.concatenate(a["edges"], axis=1), np.asarray(a["ptr"], dtype=np.int64),
                                  rm if rm.any() else None, np.concatenate(a["common"])))
        return out[0], out[1]

    # ---- vectorized draws (same distributions, numpy stream) --------------------------------------------
    def _np_rng(self, gen: torch.Generator) -> np.random.Generator:
        if self._nprng is None:
            self._nprng = np.random.default_rng(int(torch.randint(0, 2 ** 62, (1,), generator=gen).item()))
        return self._nprng

    @staticmethod
    def _rank_in_group(keys: np.ndarray, group: np.ndarray, gptr: np.ndarray) -> np.ndarray:
        """rank of every element among the elements of its group when ordered by key (groups are contiguous)."""
        order = np.argsort(group + keys)          # keys in [0,1): one float sort orders by (group, key)
        rank = np.empty(len(keys), dtype=np.int64)
        rank[order] = np.arange(len(keys)) - gptr[group[order]]
        return rank

    def _static(self, inp: StepInputs, d: str) -> Dict[str, np.ndarray]:
        """Structures of one domain batch that do not depend on the step's RNG (cached on the batch, like _host_tensors)."""
        hb = inp.host[d]
        if "static" not in hb._cache:
            ptr = np.asarray(hb.ptr_host, dtype=np.int64)
            n = np.diff(ptr)
            ei = hb.edge_index.numpy()
            eptr = np.asarray(hb.edge_ptr_host, dtype=np.int64)
            st = {"ptr": ptr, "n": n, "node_graph": np.repeat(np.arange(len(n)), n), "ei": ei, "eptr": eptr,
                  "edge_graph": np.repeat(np.arange(len(n)), np.diff(eptr)), "F": hb.x.size(1)}
            # candidate negative edges: ordered pairs (i, j), i != j, not adjacent in either direction
            cs, cd, cg = [], [], []
            for g in range(len(n)):
                adj = np.zeros((n[g], n[g]), dtype=bool)
                loc = ei[:, eptr[g]:eptr[g + 1]] - ptr[g]
                adj[loc[0], loc[1]] = True
                adj[loc[1], loc[0]] = True
                np.fill_diagonal(adj, True)
                i, j = np.nonzero(~adj)
                cs.append(i + ptr[g]); cd.append(j + ptr[g]); cg.append(np.full(len(i), g))
            st["cand"] = np.stack([np.concatenate(cs), np.concatenate(cd)])
            st["cand_graph"] = np.concatenate(cg)
            st["cand_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(st["cand_graph"], minlength=len(n)))])
            hb._cache["static"] = st
        return hb._cache["static"]

    def _view_vectorized(self, st, rng: np.random.Generator, keep: np.ndarray) -> Tuple[np.ndarray, ...]:
        """Edge drop + attribute mask for one view of a whole domain batch, given its node keep mask."""
        new_id = np.cumsum(keep) - 1
        rows = np.flatnonzero(keep)
        ei, eg = st["ei"], st["edge_graph"]
        em = keep[ei[0]] & keep[ei[1]]
        edges = new_id[ei[:, em]]
        eg = eg[em]
        G = len(st["n"])
        ecount = np.bincount(eg, minlength=G)
        coin = (rng.random(G) < 0.2) & (ecount >= 3)
        if coin.any():
            eptr = np.concatenate([[0], np.cumsum(ecount)])
            rank = self._rank_in_group(rng.random(len(eg)), eg, eptr)
            keep_e = ecount - np.maximum(1, (ecount * 0.2).astype(np.int64))
            ekeep = ~coin[eg] | (rank < keep_e[eg])
            edges = edges[:, ekeep]
        kept_n = np.bincount(st["node_graph"][keep], minlength=G)
        ptr = np.concatenate([[0], np.cumsum(kept_n)])
        rowmask = None
        F = st["F"]
        coin2 = rng.random(G) < 0.2
        if F >= 3 and coin2.any():
            m = max(1, int(F * 0.2))
            cols = np.argsort(rng.random((G, F)), axis=1)[:, :m]
            bits = np.bitwise_or.reduce(np.uint64(1) << cols.astype(np.uint64), axis=1)
            bits[~coin2] = 0
            rowmask = np.repeat(bits, kept_n)
        return rows, edges, ptr, rowmask, new_id

    def _draw_vectorized(self, inp: StepInputs, gen: torch.Generator) -> Dict[str, object]:
        rng = self._np_rng(gen)
        art: Dict[str, object] = {}
        for t in self.tasks:
            if t == "graph_prop":
                continue
            out = art[t] = {}
            for d in self.domains:
                if inp.host[d].num_graphs == 0:          # a domain absent from this step (single-domain validation passes)
                    out[d] = _EMPTY_ART[t]()
                    continue
                st = self._static(inp, d)
                n, ng, ptr = st["n"], st["node_graph"], st["ptr"]
                if t == "node_feat_mask":
                    k = np.where(n >= 3, np.maximum(1, (n * 0.15).astype(np.int64)), 0)
                    rank = self._rank_in_group(rng.random(len(ng)), ng, ptr)
                    out[d] = np.flatnonzero(rank < k[ng])
                elif t == "link_pred":
                    cptr = st["cand_ptr"]
                    # PyG applies num_neg_samples = E of the WHOLE batch to every graph: min(E, its non-edges) each
                    want = np.minimum(int(st["eptr"][-1]), np.diff(cptr))
                    pick = [cptr[g] + (np.arange(want[g]) if want[g] == cptr[g + 1] - cptr[g] else
                                       rng.choice(cptr[g + 1] - cptr[g], size=want[g], replace=False))
                            for g in range(len(n)) if want[g] > 0]
                    out[d] = st["cand"][:, np.concatenate(pick)] if pick else np.zeros((2, 0), dtype=np.int64)
                else:
                    if t == "graph_contrast" and len(n) < 2:
                        out[d] = None
                        continue
                    keep_n = np.where(n >= 3, n - np.maximum(1, (n * 0.2).astype(np.int64)), n)
                    keeps = [self._rank_in_group(rng.random(len(ng)), ng, ptr) < keep_n[ng] for _ in range(2)]
                    parts = [self._view_vectorized(st, rng, k) for k in keeps]
                    both = keeps[0] & keeps[1]
                    out[d] = tuple(ViewArrays(rows, edges, vptr, rowmask, new_id[both]) for (rows, edges, vptr, rowmask, new_id) in parts)
        return art

    # ---- plan: lay the step out as segments, everything as flat arrays ----------------------------------
    def _plan_native(self, inp: StepInputs, raw) -> StepPlan:
        """hostdraw.plan_step: the layout below in one native call with the GIL released (array for array the same: tests/test_hostdraw.py)."""
        from ._step_desc import TASK_KIND
        D = self.domains
        r = hostdraw().plan_step([TASK_KIND[t] for t in self.tasks], _draw_args(inp, D), [int(inp.row_off[d]) for d in D], raw, self.lp_merge,
                                 self.fwd_ranges, H, GRAPH_PROPERTY_DIM)
        p = StepPlan()
        p.cat32, p.cat64 = r["cat32"].numpy(), r["cat64"].numpy()
        p.lay32, p.lay64 = {n: o for n, o, _ in r["lay32"]}, {n: o for n, o, _ in r["lay64"]}
        p.a32, p.a64 = _Views(p.cat32, r["lay32"]), _Views(p.cat64, r["lay64"])
        p.seg_ptr, p.seg_dom, p.seg_task, p.task_row = r["seg_ptr"], r["seg_dom"], r["seg_task"], r["task_row"]
        p.sizes = {t: int(v) for t, v in zip(self.tasks, r["sizes"])}
        p.skipped = [(int(ti), D[int(di)]) for ti, di in r["skipped"]]
        p.N, p.S, p.E, p.max_seg, p.max_seg_edges, p.num_tiles = r["N"], r["S"], r["E"], r["max_seg"], r["max_seg_edges"], r["num_tiles"]
        p.fwd_cuts = list(zip(r["fwd_cut_seg"], r["fwd_cut_row"]))
        for k in ("nfm_rows", "nc_rows", "nc_n", "gc_rows", "gc_n", "gc_B", "gc_r0", "gc_M", "gp_rows", "gp_B", "gp_r0", "gp_M", "da_B", "da_r0", "da_M",
                  "lp_K", "lp_S", "lp_rows_end", "lp_max_rows", "lp_max_edges"):
            if k in r:
                setattr(p, k, r[k])
        if "lp_K" in r:
            p.lp_labels = r["lp_labels"].numpy()
            if p.lp_K > self.KMAX:
                raise GnnmpError("engine: too many link-prediction edges")
        if p.N > self.max_rows or p.E > self.max_edges or p.S > self.S_MAX:
            raise GnnmpError(f"step of {p.N} rows / {p.E} edges / {p.S} segments exceeds the engine capacity "
                               f"({self.max_rows}/{self.max_edges}/{self.S_MAX})")
        if p.cat32.size > self.i32_cap or p.cat64.size > self.i64_cap:
            raise GnnmpError("engine: staging buffer too small")
        return p

    def plan(self, inp: StepInputs, art: Dict[str, object]) -> StepPlan:
        raw = getattr(art, "raw", None)
        if raw is not None and self.native_plan:
            return self._plan_native(inp, raw)
        p, D = StepPlan(), self.domains
        seg_ptr, seg_dom, seg_task = [0], [], []
        src_rows, edges, rowmasks = [], [], []
        task_row = [0]
        a32: Dict[str, np.ndarray] = {}
        a64: Dict[str, np.ndarray] = {}
        sizes: Dict[str, int] = {}
        p.skipped = []

        def add_segment(ti: int, di: int, rows: np.ndarray, e_local: np.ndarray, rowmask: Optional[np.ndarray]) -> int:
            r0 = seg_ptr[-1]
            src_rows.append(rows)
            edges.append(e_local + r0)
            rowmasks.append((r0, rowmask))
            seg_ptr.append(r0 + len(rows)); seg_dom.append(di); seg_task.append(ti)
            return r0

        for ti, t in enumerate(self.tasks):
            if t in ("node_feat_mask", "link_pred", "graph_prop", "domain_adv"):
                r0s = []
                for di, d in enumerate(D):
                    hb, roff = inp.host[d], inp.row_off[d]
                    r0s.append(add_segment(ti, di, np.arange(roff, roff + hb.num_nodes), hb.edge_index.numpy(), None))
                if t == "node_feat_mask":
                    idx = [np.asarray(art[t][d], dtype=np.int64) + r0 for d, r0 in zip(D, r0s)]
                    rows = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).tolist()
                    p.skipped += [(ti, d) for d, i in zip(D, idx) if len(i) == 0]
                    a64["nfm_idx"] = np.concatenate(idx)
                    p.nfm_rows = rows
                    sizes[t] = rows[-1] * H
                elif t == "link_pred":
                    eds, labs, npos, ordered, ords = [], [], [], 0, []
                    for d, r0 in zip(D, r0s):
                        hb = inp.host[d]
                        neg = np.asarray(art[t][d], dtype=np.int64)
                        ord_base = ordered
                        ordered += hb.edge_index.size(1) + neg.shape[1]
                        if self.lp_merge:
                            pairs, w, od = merge_mirrored_pairs(hb, neg, r0, ord_base)
                            eds.append(pairs); labs.append(w); ords.append(od)
                            npos.append((pairs.shape[1], 0))
                        else:
                            eds += [hb.edge_index.numpy() + r0, neg + r0]
                            npos.append((eds[-2].shape[1], eds[-1].shape[1]))
                            labs += [np.ones(npos[-1][0], dtype=np.float32), -np.ones(npos[-1][1], dtype=np.float32)]
                    e = np.concatenate(eds, axis=1)
                    lab = np.concatenate(labs)
                    if e.shape[1] > self.KMAX:
                        raise GnnmpError("engine: too many link-prediction edges")
                    a64["lp_edges"] = e
                    p.lp_labels, p.lp_K = lab, e.shape[1]
                    sizes[t] = ordered                    # the reference's count: BCE is a mean over its ordered list (tasks.py:120)
                    # block diagonal by domain: the decoder CSR is built one workgroup per (domain, orientation)
                    a32["lp_seg_ptr"] = np.asarray(r0s + [seg_ptr[-1]])
                    a32["lp_seg_eptr"] = np.concatenate([[0], np.cumsum([a + b for a, b in npos])])
                    if self.lp_merge:           # [2, K']: the ordered row(s) of the reference's list every merged row stands for
                        a32["lp_pos"] = np.concatenate(ords, axis=1) if ords else np.zeros((2, 0), dtype=np.int32)
                    p.lp_S, p.lp_rows_end = len(r0s), seg_ptr[-1]
                    p.lp_max_rows = int(np.diff(a32["lp_seg_ptr"]).max())
                    p.lp_max_edges = int(np.diff(a32["lp_seg_eptr"]).max())
                else:
                    starts, rows, labels = [], [0], []
                    for di, (d, r0) in enumerate(zip(D, r0s)):
                        ph = inp.host[d].ptr_host
                        starts += [r0 + v for v in ph[:-1]]
                        rows.append(rows[-1] + len(ph) - 1)
                        labels += [di] * (len(ph) - 1)
                    end = seg_ptr[-1]
                    ptr = np.asarray(starts + [end], dtype=np.int64)
                    if t == "graph_prop":
                        a32["gp_ptr"] = ptr
                        a64["gp_gid"] = np.repeat(np.arange(len(starts)), np.diff(ptr))
                        p.gp_rows, p.gp_B, p.gp_r0, p.gp_M = rows, len(starts), task_row[-1], end - task_row[-1]
                        sizes[t] = rows[-1] * GRAPH_PROPERTY_DIM
                    else:                                   # domain_adv: label = index of the graph's domain (tasks.py:333)
                        a32["da_ptr"] = ptr
                        a64["da_gid"] = np.repeat(np.arange(len(starts)), np.diff(ptr))
                        a64["da_labels"] = np.asarray(labels, dtype=np.int64)
                        p.da_B, p.da_r0, p.da_M = len(starts), task_row[-1], end - task_row[-1]
                        sizes[t] = len(starts)
            else:
                idx, rows, ns, starts = [], [0], [], []
                for di, d in enumerate(D):
                    views, roff = art[t][d], inp.row_off[d]
                    if views is None:
                        ns.append(0); rows.append(rows[-1]); p.skipped.append((ti, d))
                        continue
                    r0s = [add_segment(ti, di, v.rows + roff, v.edges, v.rowmask) for v in views]
                    if t == "node_contrast":
                        c1, c2 = views[0].common, views[1].common
                        n = len(c1) if (len(c1) >= 2 and len(c2) >= 2) else 0        # tasks.py:171-173
                        ns.append(n)
                        if n:
                            idx += [c1 + r0s[0], c2 + r0s[1]]
                        else:
                            p.skipped.append((ti, d))
                        rows.append(rows[-1] + 2 * n)
                    else:
                        for v, r0 in zip(views, r0s):
                            starts.append(v.ptr[:-1] + r0)
                        B = len(views[0].ptr) - 1
                        ns.append(B); rows.append(rows[-1] + 2 * B)
                if t == "node_contrast":
                    a64["nc_idx"] = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
                    p.nc_rows, p.nc_n = rows, ns
                else:
                    st = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
                    ptr = np.concatenate([st, [seg_ptr[-1]]])
                    a32["gc_ptr"] = ptr
                    a64["gc_gid"] = np.repeat(np.arange(len(st)), np.diff(ptr))
                    p.gc_rows, p.gc_n, p.gc_B, p.gc_r0, p.gc_M = rows, ns, len(st), task_row[-1], seg_ptr[-1] - task_row[-1]
                sizes[t] = rows[-1]
            task_row.append(seg_ptr[-1])
        p.seg_ptr, p.seg_dom, p.seg_task, p.task_row, p.sizes = seg_ptr, seg_dom, seg_task, task_row, sizes
        p.N, p.S = seg_ptr[-1], len(seg_dom)
        e_all = np.concatenate(edges, axis=1)
        p.E = e_all.shape[1]
        p.max_seg = max(b - a for a, b in zip(seg_ptr[:-1], seg_ptr[1:]))
        # the stacked forward runs as fwd_ranges row ranges on as many streams (gnnmp_step.h fwd_cut_*): cut k at the segment boundary nearest
        # k N / R, kept only while the cuts ascend strictly inside (0, N)
        p.fwd_cuts, R = [], self.fwd_ranges
        for k in range(1, R):
            if p.S <= 1:
                break
            cut = min(range(1, p.S), key=lambda i: abs(R * seg_ptr[i] - k * p.N))
            if (p.fwd_cuts[-1][1] if p.fwd_cuts else 0) < seg_ptr[cut] < p.N:
                p.fwd_cuts.append((cut, seg_ptr[cut]))
        if p.N > self.max_rows or p.E > self.max_edges or p.S > self.S_MAX:
            raise GnnmpError(f"step of {p.N} rows / {p.E} edges / {p.S} segments exceeds the engine capacity "
                               f"({self.max_rows}/{self.max_edges}/{self.S_MAX})")
        a32["seg_ptr"], a32["seg_dom"], a32["src_row"] = np.asarray(seg_ptr), np.asarray(seg_dom), np.concatenate(src_rows)
        seg_eptr = np.concatenate([[0], np.cumsum([e.shape[1] for e in edges])])       # the batch is block diagonal: one CSR build per segment
        a32["seg_eptr"] = seg_eptr
        p.max_seg_edges = int(np.diff(seg_eptr).max()) if len(edges) else 0
        nt = [(b - a + 31) // 32 for a, b in zip(seg_ptr[:-1], seg_ptr[1:])]
        tile_seg = np.repeat(np.arange(p.S), nt)
        tile_first = np.concatenate([[0], np.cumsum(nt)])[:-1]
        tile_row = np.asarray(seg_ptr[:-1])[tile_seg] + 32 * (np.arange(len(tile_seg)) - tile_first[tile_seg])
        a32["tiles"] = np.stack([tile_seg, tile_row], axis=1)
        p.num_tiles = len(tile_seg)
        a64["edge_index"] = e_all
        if any(m is not None for _, m in rowmasks):
            rm = np.zeros(p.N, dtype=np.uint64)
            for r0, m in rowmasks:
                if m is not None:
                    rm[r0:r0 + len(m)] = m
            a64["rowmask"] = rm.view(np.int64)
        p.a32, p.a64 = a32, a64
        # the upload image of the step, packed here (prefetch thread) so the launcher thread only makes two block copies into
        # its pinned slot: every array starts 16-byte aligned
        def pack(arrs, dtype, gran, cap, what):
            lay, parts, o = {}, [], 0
            for name, arr in arrs.items():
                a = np.ascontiguousarray(np.asarray(arr).reshape(-1), dtype=dtype)
                lay[name] = o
                pad = (-a.size) % gran
                parts.append(a)
                if pad:
                    parts.append(np.zeros(pad, dtype=dtype))
                o += a.size + pad
            if o > cap:
                raise GnnmpError(f"engine: {what} staging buffer too small")
            return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)), lay
        p.cat32, p.lay32 = pack(a32, np.int32, 4, self.i32_cap, "int32")
        p.cat64, p.lay64 = pack(a64, np.int64, 2, self.i64_cap, "int64")
        return p
