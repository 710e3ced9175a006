"""Sparse (CSR) node features, host side: the SparseFeatures container, its CSC index, and the opt-in switch of the fine-tune
config and CLI.  No GPU needed; the kernels are tests/test_gpu_sparse_linear.py."""
import numpy as np
import pytest
import torch

from gnn_pretraining_amd import synthetic as S
from gnn_pretraining_amd.graph import Batch, Data, SparseFeatures


def _citeseer_like(gen):
    return S.cora_like(gen, num_nodes=3327, undirected_edges=4552, dim=3703, density=0.0085, num_classes=6)


@pytest.mark.parametrize("make", [lambda g: S.cora_like(g), _citeseer_like], ids=["cora", "citeseer"])
def test_from_dense_round_trips(make):
    x = make(torch.Generator().manual_seed(1)).x
    sp = SparseFeatures.from_dense(x)
    assert sp.size() == x.shape and sp.size(1) == x.size(1) and sp.device.type == "cpu"
    assert sp.rowptr.dtype == torch.int32 and sp.col.dtype == torch.int32 and sp.val.dtype == torch.float32
    assert sp.nnz == int((x != 0).sum())
    assert torch.equal(sp.to_dense(), x)
    rp, col = sp.rowptr.long(), sp.col.long()
    for r in range(0, x.size(0), 97):                                # columns sorted and unique within a row
        c = col[rp[r]:rp[r + 1]]
        assert bool((c[1:] > c[:-1]).all())


def test_csc_equals_numpy_transpose_with_empty_and_dense_columns():
    gen = torch.Generator().manual_seed(2)
    x = (torch.rand(300, 130, generator=gen) < 0.05).float() * torch.rand(300, 130, generator=gen)
    x[:, 7] = 0.0                                                    # empty columns
    x[:, 128:] = 0.0
    x[5] = 0.0                                                       # a row whose only entry is the dense column's
    x[:, 11] = torch.rand(300, generator=gen) + 0.5                  # a fully dense column
    sp = SparseFeatures.from_dense(x)
    colptr, row, val_t = sp.csc()
    xt = x.numpy().T
    nz_r, nz_c = np.nonzero(xt)                                      # row-major over X^T: by column, ascending row
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(nz_r, minlength=130))])
    assert np.array_equal(colptr.numpy(), want_ptr)
    assert np.array_equal(row.numpy(), nz_c) and np.array_equal(val_t.numpy(), xt[nz_r, nz_c])
    assert colptr[8] - colptr[7] == 0 and colptr[12] - colptr[11] == 300
    assert sp.csc() is sp.csc()                                      # cached


def test_from_torch_agrees_with_from_dense():
    x = S.cora_like(torch.Generator().manual_seed(3), num_nodes=400, dim=333).x
    want = SparseFeatures.from_dense(x)
    for t in (x.to_sparse_csr(), x.to_sparse_coo(), x.to_sparse_coo().coalesce()):
        got = SparseFeatures.from_torch(t)
        assert got.shape == want.shape
        assert torch.equal(got.rowptr, want.rowptr) and torch.equal(got.col, want.col) and torch.equal(got.val, want.val)
    with pytest.raises(ValueError):
        SparseFeatures.from_torch(x)


def test_data_and_batch_carry_sparse_features():
    c = S.cora_like(torch.Generator().manual_seed(4), num_nodes=200, undirected_edges=400, dim=64)
    sp = SparseFeatures.from_dense(c.x)
    sp.csc()
    d = Data(sp, c.edge_index, c.y).to("cpu")
    assert isinstance(d.x, SparseFeatures) and d.num_nodes == 200 and d.num_node_features == 64
    b = Batch.from_data_list([c])
    b.x = sp
    moved = b.to("cpu")
    assert isinstance(moved.x, SparseFeatures) and moved.num_nodes == 200 and moved.x._csc is not None
    assert torch.equal(moved.host().x.to_dense(), c.x)


def test_sparse_features_rejected_for_graph_classification_domains():
    from gnn_pretraining_amd.finetune.finetune import FinetuneConfig
    for d in ("ENZYMES", "PTC_MR"):
        with pytest.raises(ValueError):
            FinetuneConfig(d, "full_finetune", "b1", 7, sparse_features=True)
    for d in ("Cora_NC", "CiteSeer_NC", "Cora_LP", "CiteSeer_LP"):
        cfg = FinetuneConfig(d, "full_finetune", "b1", 7, sparse_features=True)
        assert cfg.sparse_features and cfg.exp_name == f"{d}_full_finetune_b1"
    assert FinetuneConfig("Cora_NC", "full_finetune", "b1", 7).sparse_features is False


def test_cli_threads_the_sparse_features_flag():
    from gnn_pretraining_amd.finetune import finetune as FT
    base = ["--domain_name", "CiteSeer_NC", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "7"]
    assert FT.config_from_args(FT.build_parser().parse_args(base + ["--sparse-features"])).sparse_features is True
    assert FT.config_from_args(FT.build_parser().parse_args(base)).sparse_features is False
