"""Plain references for the three kernel families that turn a batch into the first activations (csrc/csr_build.hip, csrc/encoder.hip,
csrc/sparse_linear.hip): integer numpy for the index build, float64 torch for the two linears.  Host only; pinned against the oracle
and against fp32 torch in test_input_ref_host.py, compared with the kernels in test_gpu_input_kernels.py.

Every float reference takes `absolute=True` to run on absolute values: that gives the sum |terms| of the project's error bound
|got - want| <= (n_terms + extra) * 2^-24 * sum |terms| for the same element.
"""
import numpy as np
import torch

H = 256                 # output width of the stacked encoders


# ------------------------------------------------------------------------------------------------ COO -> CSR
def ref_csr(ei, n, by):
    """(rowptr i32 [n+1], col i32 [kept], perm i32 [kept], dropped) of edge_index [2, E] int64 grouped by target (by='dst') or by source
    (by='src').  An edge with an endpoint outside [0, n) is dropped (and counted once); the survivors are ordered by a stable argsort
    of the key, so within a row slots are in ascending COO edge id; perm holds the original edge ids."""
    src, dst = ei[0].numpy().astype(np.int64), ei[1].numpy().astype(np.int64)
    key, other = (dst, src) if by == "dst" else (src, dst)
    ok = (key >= 0) & (key < n) & (other >= 0) & (other < n)
    ids = np.nonzero(ok)[0]
    perm = ids[np.argsort(key[ids], kind="stable")]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(key[ids], minlength=n))
    to = lambda a: torch.from_numpy(a.astype(np.int32))                     # noqa: E731
    return to(rowptr), to(other[perm]), to(perm), int(key.size - ids.size)


# ------------------------------------------------------------------------------------------------ stacked encoders
def encoder_rows(x_all, src_row, colmask, width):
    """xm [N, width] float64: row r is x_all[src_row[r], :width] with the columns whose bit is set in colmask[r] (numpy uint64 [N] or
    None) zeroed; a src_row outside [0, x_all.size(0)) gives a zero row."""
    R = x_all.size(0)
    sr = src_row.long()
    ok = (sr >= 0) & (sr < R)
    xm = x_all.double()[sr.clamp(0, R - 1), :width] * ok.double().unsqueeze(1)
    if colmask is not None:
        bits = (colmask[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)
        xm = xm * torch.from_numpy((bits == 0).astype(np.float64))
    return xm


def ref_encoder_fwd(x_all, src_row, seg_ptr, seg_dom, colmask, params, w_off, b_off, d_in, absolute=False):
    """z [N, 256] float64: per segment s of domain d = seg_dom[s], z = xm[:, :d_in[d]] @ W_d.T + b_d with W_d [256, d_in[d]] at
    params[w_off[d]:] and b_d at params[b_off[d]:]."""
    xm = encoder_rows(x_all, src_row, colmask, max(d_in))
    p = params.double()
    if absolute:
        xm, p = xm.abs(), p.abs()
    z = torch.zeros(int(seg_ptr[-1]), H, dtype=torch.float64)
    for s, d in enumerate(seg_dom.tolist()):
        r0, r1, k = int(seg_ptr[s]), int(seg_ptr[s + 1]), d_in[d]
        W, b = p[w_off[d]:w_off[d] + H * k].view(H, k), p[b_off[d]:b_off[d] + H]
        z[r0:r1] = xm[r0:r1, :k] @ W.T + b
    return z


def ref_encoder_bwd(x_all, src_row, seg_ptr, seg_dom, colmask, gz, gseg, d_in, absolute=False):
    """Per group g (segments gseg[g] .. gseg[g+1] of one domain, consecutive rows): (dW [256, d_in] = gz.T @ xm, db [256] = gz.sum(0),
    rows) in float64."""
    xm, g64 = encoder_rows(x_all, src_row, colmask, max(d_in)), gz.double()
    if absolute:
        xm, g64 = xm.abs(), g64.abs()
    out = []
    for g in range(len(gseg) - 1):
        if gseg[g + 1] == gseg[g]:
            out.append(None)
            continue
        r0, r1, k = int(seg_ptr[gseg[g]]), int(seg_ptr[gseg[g + 1]]), d_in[int(seg_dom[gseg[g]])]
        out.append((g64[r0:r1].T @ xm[r0:r1, :k], g64[r0:r1].sum(0), r1 - r0))
    return out


# ------------------------------------------------------------------------------------------------ sparse linear
def _entries(rowptr, col, K):
    cnt = (rowptr[1:] - rowptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    c = col.long()[int(rowptr[0]):int(rowptr[-1])]
    return rows, c, (c >= 0) & (c < K)


def ref_sparse_fwd(rowptr, col, val, K, W, bias, absolute=False):
    """(Y [N, H] float64, kept entries per row): Y[r] = sum over the entries k of row r of val[k] * W[:, col[k]] + bias, straight from
    the CSR arrays (unsorted and repeated columns stay separate addends); entries with a column outside [0, K) are dropped."""
    rows, c, ok = _entries(rowptr, col, K)
    v, W64 = val.double()[ok], W.double()[:, :K]
    b = torch.zeros(W.size(0), dtype=torch.float64) if bias is None else bias.double()
    if absolute:
        v, W64, b = v.abs(), W64.abs(), b.abs()
    N = rowptr.numel() - 1
    y = torch.zeros(N, W.size(0), dtype=torch.float64).index_add_(0, rows[ok], v.unsqueeze(1) * W64.T[c[ok]])
    return y + b, torch.bincount(rows[ok], minlength=N)


def ref_sparse_wgrad(rowptr, col, val, K, G, absolute=False):
    """(dW [H, K] float64, kept entries per column): dW[h, k] = sum over the entries of column k of val * G[row, h]."""
    rows, c, ok = _entries(rowptr, col, K)
    v, G64 = val.double()[ok], G.double()
    if absolute:
        v, G64 = v.abs(), G64.abs()
    dWt = torch.zeros(K, G.size(1), dtype=torch.float64).index_add_(0, c[ok], v.unsqueeze(1) * G64[rows[ok]])
    return dWt.T.contiguous(), torch.bincount(c[ok], minlength=K)


def ref_csc(rowptr, col, val, K):
    """(colptr i32 [K+1], row i32 [kept], val_t f32 [kept], dropped): X by columns, a stable sort of the kept entries by column
    (ascending entry id, hence ascending row, within a column)."""
    rows, c, ok = _entries(rowptr, col, K)
    ids = torch.nonzero(ok).flatten()
    order = ids[torch.sort(c[ids], stable=True).indices]
    colptr = torch.zeros(K + 1, dtype=torch.int64)
    colptr[1:] = torch.bincount(c[ids], minlength=K).cumsum(0)
    return colptr.to(torch.int32), rows[order].to(torch.int32), val[order].contiguous(), int(c.numel() - ids.numel())


# ================================================================================================ inputs shared by the host pins and the GPU tests
SPECIAL_DEGREES = (33, 0, 1, 32, 64, 300, 65)         # thread / wave switch of the per-row ordering (32 | 33), wave stride (64 | 65), a hub


def special_graph(n, num_edges, rows=None, big=300, seed=0):
    """edge_index [2, num_edges] int64 in random edge order with seven special rows whose in-degree AND out-degree are exactly
    0, 1, 32, 33, 64, 65 and `big`: both directions of every special edge, as hub_graph of test_gpu_kernel_edges.py adds them.  By
    default the specials sit at the first row (33), the last row (65) and five rows in between; `rows` names the seven rows in the
    order of SPECIAL_DEGREES.  The rows of 64 and of `big` entries hold a self loop stored twice; every special row of 32 or more
    repeats a leaf (duplicate edges); the random rest (num_edges minus the special edges, between the other rows) starts with a
    self loop and a duplicate edge.  Returns (ei, {row: degree})."""
    gen = torch.Generator().manual_seed(seed * 1000003 + n + num_edges)
    rows = [0, n // 7, 2 * n // 7 + 1, 3 * n // 7, 4 * n // 7 + 1, 5 * n // 7, n - 1] if rows is None else list(rows)
    degs = dict(zip(rows, SPECIAL_DEGREES[:5] + (big,) + SPECIAL_DEGREES[6:]))
    assert len(degs) == 7 and all(0 <= r < n for r in rows)
    plain = torch.arange(n)[~torch.isin(torch.arange(n), torch.tensor(rows))]
    parts = []
    for h, d in degs.items():
        loop = d in (64, big)
        leaves = plain[torch.randint(0, plain.numel(), (d - 2 if loop else d,), generator=gen)]
        if d >= 32:
            leaves[1] = leaves[0]
        hh = torch.full_like(leaves, h)
        parts += [torch.stack([leaves, hh]), torch.stack([hh, leaves])]
        if loop:
            parts.append(torch.full((2, 2), h, dtype=torch.int64))
    m = num_edges - sum(p.size(1) for p in parts)
    assert m >= 3, "num_edges leaves no room for the random rest"
    rest = plain[torch.randint(0, plain.numel(), (2, m), generator=gen)]
    rest[1, 0] = rest[0, 0]                                                 # a self loop
    rest[:, 2] = rest[:, 1]                                                 # a duplicate edge
    ei = torch.cat(parts + [rest], dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert ei.size(1) == num_edges and all(int(indeg[h]) == d == int(outdeg[h]) for h, d in degs.items())
    return ei, degs


BAD_ENDPOINTS = (-1, None, 2 ** 31, 2 ** 40, -2 ** 40)                      # None: the row count itself


def with_bad_endpoints(ei, n, count=12):
    """A copy of ei where `count` edges, spread over the edge list, got an endpoint outside [0, n): in the target row, in the source
    row, or in both (such an edge still counts once)."""
    ei = ei.clone()
    E = ei.size(1)
    value = lambda i: n if BAD_ENDPOINTS[i % 5] is None else BAD_ENDPOINTS[i % 5]       # noqa: E731
    for i in range(count):
        e = (i * E) // count + i % 5
        if i % 3 in (0, 2):
            ei[1, e] = value(i)
        if i % 3 in (1, 2):
            ei[0, e] = value(i + i % 3)                                     # both bad: two different values
    return ei


def segmented_batch(seed=5):
    """A block-diagonal batch: an empty segment, one of 8,000 rows / 24,000 edges with the special rows (160,008 B of LDS in
    gmp_csr_build_segmented), one of 10 isolated rows, 300 segments of 2 ... 5 rows, an empty last one.
    Returns (ei, N, seg_row, seg_edge)."""
    gen = torch.Generator().manual_seed(seed)
    big, _ = special_graph(8000, 24000, seed=seed)
    seg_row, seg_edge, eds = [0, 0, 8000, 8010], [0, 0, 24000, 24000], [big]
    for _ in range(300):
        nr = int(torch.randint(2, 6, (1,), generator=gen))
        ne = int(torch.randint(0, 9, (1,), generator=gen))
        eds.append(torch.randint(0, nr, (2, ne), generator=gen) + seg_row[-1])
        seg_row.append(seg_row[-1] + nr); seg_edge.append(seg_edge[-1] + ne)
    seg_row.append(seg_row[-1]); seg_edge.append(seg_edge[-1])
    return torch.cat(eds, dim=1).contiguous(), seg_row[-1], seg_row, seg_edge


# ------------------------------------------------------------------------------------------------ stacked encoders
ENC_LAYOUTS = {4: (4, 1, 3), 8: (8, 1, 5), 9: (9, 2, 7), 24: (24, 9, 17), 37: (7, 4, 37, 21), 40: (7, 4, 37, 21),
               41: (41, 1, 33), 64: (64, 1, 33)}                          # dpad -> d_in of the domains in use (41 cannot hold d_in 64)
FWD_SIZES = [0, 1, 31, 32, 33, 64, 100, 0, 5]
# backward: [outside any group | g0: 4 tiles | g1: empty | g2: two rowless segments | g3: 7 + 0 + 10 = 17 tiles | g4: 32 + 1 = 33 tiles |
#            g5: 2 tiles | outside any group]
BWD_SIZES = [7, 100, 0, 0, 193, 0, 320, 1000, 5, 33, 9]
BWD_GSEG = [1, 2, 2, 4, 7, 9, 10]


class EncCase:
    """One stacked-encoder problem on the host.  The domain table holds the layout's d_in plus one absent domain at index 1; segments
    take the domains in use in descending, wrapping order (non-monotonic); the parameters sit at odd offsets of one flat buffer;
    x_all is random in every column (the padding columns [d_in, dpad) too: the kernels must not read them); src_row is a random map
    with repeats, -1 and num_x_rows at chosen rows.  masks: None, 'random' (bits 0, d_in - 1, d_in ... 63 at chosen rows, random
    bits elsewhere) or 'all'."""

    def __init__(self, dpad, sizes, masks, seg_dom=None, seed=0):
        gen = torch.Generator().manual_seed(1000 * dpad + len(sizes) + seed)
        used = list(ENC_LAYOUTS[dpad])
        self.dpad, self.d_in = dpad, [used[0], 2 if dpad >= 2 else 1] + used[1:]
        in_use = [0] + list(range(2, len(self.d_in)))
        self.seg_ptr = torch.zeros(len(sizes) + 1, dtype=torch.int32)
        self.seg_ptr[1:] = torch.tensor(sizes).cumsum(0)
        self.seg_dom = torch.tensor([in_use[::-1][s % len(in_use)] for s in range(len(sizes))] if seg_dom is None else seg_dom, dtype=torch.int32)
        self.N, self.R = int(self.seg_ptr[-1]), 50
        self.x_all = torch.randn(self.R, dpad, generator=gen)
        self.src_row = torch.randint(0, self.R, (self.N,), generator=gen, dtype=torch.int32)
        self.bad_rows = [r for r in (0, 40, self.N - 1) if r < self.N]
        for i, r in enumerate(self.bad_rows):
            self.src_row[r] = -1 if i % 2 == 0 else self.R
        self.w_off, self.b_off, cur = [], [], 3
        for k in self.d_in:
            self.w_off.append(cur); cur += 256 * k + 2                      # every offset stays odd, with gaps between the tensors
            self.b_off.append(cur); cur += 256 + 4
        self.params = torch.randn(cur, generator=gen)
        din_row = torch.tensor(self.d_in)[self.seg_dom.long()].repeat_interleave(self.seg_ptr[1:].long() - self.seg_ptr[:-1].long())
        self.din_row = din_row                                              # d_in of every stacked row
        self.full_rows = []
        if masks is None:
            self.colmask = None
        elif masks == "all":
            self.colmask = np.full(self.N, np.uint64(2 ** 64 - 1), dtype=np.uint64)
        else:
            m = torch.randint(0, 2 ** 62, (self.N,), generator=gen).numpy().astype(np.uint64)
            m &= torch.randint(0, 2 ** 62, (self.N,), generator=gen).numpy().astype(np.uint64)        # ~a quarter of the bits
            one = np.uint64(1)
            for r in range(self.N):
                k = int(din_row[r])
                low = np.uint64(2 ** k - 1)
                if r % 5 == 1:
                    m[r] = one                                              # bit 0 alone
                elif r % 5 == 2:
                    m[r] = one << np.uint64(k - 1)                          # bit d_in - 1 alone (bit 63 when d_in = 64)
                elif r % 5 == 3:
                    m[r] = ~low                                             # only bits at and above d_in: ignored
                elif r % 5 == 4 and r % 3 == 0:
                    m[r] = low                                              # every column of the row masked
                    self.full_rows.append(r)
            self.colmask = m

    def tiles(self):
        t = [(s, r0) for s in range(self.seg_dom.numel()) for r0 in range(int(self.seg_ptr[s]), int(self.seg_ptr[s + 1]), 32)]
        return torch.tensor(t, dtype=torch.int32).view(-1, 2)

    def ref_fwd(self, absolute=False):
        return ref_encoder_fwd(self.x_all, self.src_row, self.seg_ptr, self.seg_dom, self.colmask, self.params, self.w_off, self.b_off,
                               self.d_in, absolute)

    def ref_bwd(self, gz, gseg, absolute=False):
        return ref_encoder_bwd(self.x_all, self.src_row, self.seg_ptr, self.seg_dom, self.colmask, gz, gseg, self.d_in, absolute)


def bwd_case(dpad, masks):
    """The backward problem: BWD_SIZES / BWD_GSEG with one domain per group (the domains in use, wrapping)."""
    n_used = len(ENC_LAYOUTS[dpad])
    in_use = [0] + list(range(2, n_used + 1))
    group_dom = [in_use[::-1][g % n_used] for g in range(len(BWD_GSEG) - 1)]
    seg_dom = [in_use[0]] * len(BWD_SIZES)
    for g, d in enumerate(group_dom):
        for s in range(BWD_GSEG[g], BWD_GSEG[g + 1]):
            seg_dom[s] = d
    c = EncCase(dpad, BWD_SIZES, masks, seg_dom=seg_dom, seed=7)
    if c.colmask is not None and masks == "random":                        # column 0 masked in every row of the last group: dW[:, 0] = 0, db unchanged
        c.colmask[int(c.seg_ptr[BWD_GSEG[-2]]):int(c.seg_ptr[BWD_GSEG[-1]])] |= np.uint64(1)
    return c


# ------------------------------------------------------------------------------------------------ sparse linear
SP_N, SP_K = 70, 200
SP_ROW_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 130, 200]
SP_COLS = {0: 5, 1: 17, 8: 33, 9: 77, 64: 101, 65: 150}                    # entries in the column -> column


def sparse_matrix(seed=0):
    """CSR (rowptr i32, col i32, val f32) of X [70, 200]: rows of 0, 1, 7, 8, 9, 63, 64, 65, 130 and 200 entries (the unroll and wave
    boundaries of the gather), then rows of 3 ... 8; columns in random order within a row; columns of exactly 0, 1, 8, 9, 64 and 65
    entries (SP_COLS).  The row of 200 holds every column but the empty one, one of them twice (a repeated column index)."""
    gen = torch.Generator().manual_seed(seed)
    L = SP_ROW_LENGTHS + torch.randint(3, 9, (SP_N - len(SP_ROW_LENGTHS),), generator=gen).tolist()
    member = {SP_COLS[0]: [], SP_COLS[1]: [9], SP_COLS[8]: [9, 5, 6, 7, 8, 20, 21, 22], SP_COLS[9]: [9, 5, 6, 7, 8, 23, 24, 25, 26],
              SP_COLS[65]: [r for r in range(SP_N) if r not in (0, 10, 11, 12, 13)],
              SP_COLS[64]: [r for r in range(SP_N) if r not in (0, 1, 10, 11, 12, 13)]}
    others = torch.tensor([c for c in range(SP_K) if c not in member])
    cols = []
    for r, n in enumerate(L):
        forced = [c for c, rows in member.items() if r in rows]
        if r == 9:
            c = torch.cat([torch.tensor(forced), others, others[7:8]])      # 5 + 194 + 1 repeat
        else:
            c = torch.cat([torch.tensor(forced, dtype=torch.int64), others[torch.randperm(others.numel(), generator=gen)[:n - len(forced)]]])
        assert c.numel() == n, (r, n, c.numel())
        cols.append(c[torch.randperm(n, generator=gen)])
    rowptr = torch.zeros(SP_N + 1, dtype=torch.int32)
    rowptr[1:] = torch.tensor(L).cumsum(0)
    col = torch.cat(cols).to(torch.int32)
    cnt = torch.bincount(col.long(), minlength=SP_K)
    assert all(int(cnt[c]) == n for n, c in SP_COLS.items())
    return rowptr, col, torch.randn(col.numel(), generator=gen)


def random_csr(N, K, max_len, seed):
    """A small random CSR [N, K]: rows of 0 ... max_len entries, columns drawn with repeats, unsorted."""
    gen = torch.Generator().manual_seed(seed)
    L = torch.randint(0, max_len + 1, (N,), generator=gen)
    L[0] = 0
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = L.cumsum(0)
    nnz = int(rowptr[-1])
    return rowptr, torch.randint(0, K, (nnz,), generator=gen, dtype=torch.int32), torch.randn(nnz, generator=gen)
