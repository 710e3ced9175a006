"""CPU-side checks: the C-ABI library loads and exports every symbol the header declares;
the product package never imports the oracle; no compute is called here."""
import ast
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from gnn_pretraining_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    l = _lib.lib()
    syms = _lib.declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(l, s), s
    assert set(_lib._SIGS) == set(syms), set(_lib._SIGS) ^ set(syms)
    assert l.gmp_version() >= 100


def test_header_derived_abi_equals_the_snapshot():
    """tests/golden/abi_snapshot.json was written from the hand-kept tables this reader replaced (plus POINTER(struct) where
    the header names the struct): a changed prototype, field or constant shows up here and as a diff of that file."""
    from gnn_pretraining_amd import _abi, _lib
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_snapshot.json")))
    got = _abi.snapshot(_lib.ABI)
    for section in ("constants", "functions", "structs"):
        assert got[section].keys() == want[section].keys(), set(got[section]) ^ set(want[section])
        for name in want[section]:
            assert got[section][name] == want[section][name], name
    assert got == want
    assert _lib.K["GMP_STEP_PHASES"] == 13 and _lib.OK == 0


# every entry point a feature's host test used to assert "declared, bound and exported" one stanza at a time
FEATURE_SYMBOLS = """
gmp_bn_fold gmp_linear_affine_fwd gmp_gemm_f32 gmp_gemm_f32_grouped gmp_gemm_f32_workspace_bytes gmp_colsum gmp_colsum_workspace_bytes
gmp_gate_open_by_next_gemm gmp_gate_open_pending gmp_logreg_workspace_bytes gmp_logreg_fit gmp_logreg_predict
gmp_repr_workspace_bytes gmp_repr_pair_stats gmp_repr_alignment gmp_repr_gram gmp_knn_workspace_bytes gmp_knn_topk gmp_knn_vote
gmp_kmeans_workspace_bytes gmp_kmeans_assign gmp_kmeans_fit gmp_contingency gmp_cls_counts_workspace_bytes gmp_cls_counts
gmp_graph_props_workspace_bytes gmp_graph_props gmp_sp_workspace_bytes gmp_sp_max_unique gmp_sp_features gmp_sp_gram gmp_graph_feature_map
gmp_wl_workspace_bytes gmp_wl_refine gmp_wl_gram gmp_label_propagate_workspace_bytes gmp_label_propagate
gmp_feature_propagate_workspace_bytes gmp_feature_propagate gmp_lp_cn_tile_nodes gmp_lp_cn_rank_workspace_bytes gmp_lp_cn_score
gmp_lp_cn_rank gmp_graph_simple_check gmp_lp_walk_lds_nodes gmp_lp_walk_resident_blocks gmp_lp_walk_workspace_bytes gmp_lp_walk_score
gmp_lp_walk_rank gmp_lp_rank_workspace_bytes gmp_lp_topk_workspace_bytes gmp_lp_rank gmp_lp_topk gmp_emb_link_workspace_bytes
gmp_emb_link_score gmp_emb_link_rank gmp_lp_score_fwd_workspace_bytes gmp_lp_score_bwd_workspace_bytes gmp_lp_score_fwd gmp_lp_score_bwd
gmp_lp_feat_gemm_bwd_fold gmp_lp_feat_gemm_fwd gmp_lp_feat_gemm_wgrad gmp_gc_head_fwd_workspace_bytes gmp_gc_head_fwd gmp_gc_head_bwd
gmp_hard_negative_stream_workspace_bytes gmp_hard_negative_topk_stream gmp_nt_xent_stream_workspace_bytes gmp_nt_xent_stream_fwd
gmp_nt_xent_stream_bwd gmp_aug_negative_edges_workspace_bytes gmp_aug_negative_edges gmp_aug_negative_edges_batch
gmp_mt_surgery_clip_adamw
""".split()


@pytest.mark.parametrize("name", FEATURE_SYMBOLS)
def test_feature_symbol_is_declared_and_exported(name):
    from gnn_pretraining_amd import _lib
    assert name in _lib.declared_symbols(), f"{name} missing from the headers"
    assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} not exported by libgnnmp.so"


EDGE_HEADER = """
#define K 3
#define M (K + 1)   /* parenthesised */
enum { E_A = 0, E_B, E_C = 2 * M };
typedef struct {
    float *a, *b; int32_t c, d;
} gmp_pair;
typedef struct {
    int32_t r[K + 1];    /* a comment with a ; and a ( inside a struct */
    float* h[K + 1];
    gmp_pair inner[K];
    const int64_t* q; size_t n;
} gmp_outer;
int
gmp_f(const float* const* g, const gmp_stream_t* s,
      const gmp_outer* o, int64_t n, double x, const int32_t perm[]);
size_t gmp_g(void);
const char* gmp_h(gmp_stream_t s, uint32_t k);
"""


def test_header_reader_edge_cases():
    from gnn_pretraining_amd import _abi
    abi = _abi.parse(EDGE_HEADER)
    assert abi.constants == {"K": 3, "M": 4, "E_A": 0, "E_B": 1, "E_C": 8}
    pair, outer = abi.structs["gmp_pair"], abi.structs["gmp_outer"]
    layout = lambda s: [(f, getattr(s, f).offset, getattr(s, f).size) for f, _ in s._fields_]
    assert layout(pair) == [("a", 0, 8), ("b", 8, 8), ("c", 16, 4), ("d", 20, 4)] and C.sizeof(pair) == 24
    assert layout(outer) == [("r", 0, 16), ("h", 16, 32), ("inner", 48, 72), ("q", 120, 8), ("n", 128, 8)] and C.sizeof(outer) == 136
    assert [t for _, t in pair._fields_] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    types = dict(outer._fields_)
    assert (types["r"]._type_, types["h"]._type_, types["inner"]._type_) == (C.c_int, C.c_void_p, pair)
    assert (types["r"]._length_, types["h"]._length_, types["inner"]._length_) == (4, 4, 3)
    assert list(abi.functions) == ["gmp_f", "gmp_g", "gmp_h"]
    res, args = abi.functions["gmp_f"]
    assert res is C.c_int and args[:2] == [C.c_void_p, C.c_void_p] and args[3:] == [C.c_int64, C.c_double, C.c_void_p]
    assert args[2]._type_ is outer and C.sizeof(args[2]) == 8
    assert abi.functions["gmp_g"] == (C.c_size_t, [])
    assert abi.functions["gmp_h"] == (C.c_char_p, [C.c_void_p, C.c_uint32])


@pytest.mark.parametrize("header, quoted", [
    ("int gmp_f(int64_t n, unsigned flags);", "unknown type `unsigned` in `int gmp_f(int64_t n, unsigned flags)`"),
    ("typedef struct { int32_t ok; int32_t a[2][3]; } gmp_t;", "cannot parse the declaration `int32_t a[2][3]`"),
    ("#define K 2\ntypedef struct { int32_t a[K + NOPE]; } gmp_t;", "cannot evaluate the constant `K + NOPE` in `int32_t a[K + NOPE]`"),
])
def test_header_reader_refuses_what_it_does_not_recognise(header, quoted):
    from gnn_pretraining_amd import _abi
    with pytest.raises(_abi.GnnmpError, match=re.escape(quoted)):
        _abi.parse(header)


def test_product_never_imports_oracle():
    bad = []
    for base in ("gnn_pretraining_amd",):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if not f.endswith(".py"):
                    continue
                tree = ast.parse(open(os.path.join(dp, f)).read())
                for node in ast.walk(tree):
                    names = []
                    if isinstance(node, ast.Import):
                        names = [a.name for a in node.names]
                    elif isinstance(node, ast.ImportFrom):
                        names = [node.module or ""]
                    if any(n == "oracle" or n.startswith("oracle.") for n in names):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_missing_gpu_tensor_is_a_loud_error():
    import torch
    from gnn_pretraining_amd import ops
    from gnn_pretraining_amd._lib import GnnmpError
    with pytest.raises(GnnmpError):
        ops.csr_build(torch.zeros(2, 3, dtype=torch.long), 4)       # CPU tensor: no fallback
