"""Host-side contract shared by the link rankers and the model-free baselines.  The four all-candidate rankers (gmp_lp_rank,
gmp_lp_cn_rank, gmp_lp_walk_rank, gmp_emb_link_rank) and the three pair scorers beside them: what they refuse, with which code and which
text (every call returns before anything is launched, so no GPU is needed).  The seven rows of finetune.BASELINES: the flag parses into the
config and is off by default, the row is refused off its task type, and its C symbols are declared, bound and exported."""
import ctypes as C
import re

import pytest

from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT

_BUF = C.create_string_buffer(96)
PTR = (C.addressof(_BUF) + 15) // 16 * 16          # any non-null, 16-byte aligned address: a refused call reads nothing behind it


def _rank(name, Q=4, fnnz=0, frow=0, fcol=0, n_equal=None, p=PTR):
    ne = p if n_equal is None else n_equal
    tail = (frow, fcol, fnnz, p, p, ne)
    lead = {"gmp_lp_rank": (p, p, p, 8, Q, 256, 256, p, p, p, p),
            "gmp_lp_cn_rank": (p, p, 8, 16, p, p, Q, 0, 0),
            "gmp_lp_walk_rank": (p, p, 8, 16, p, p, Q, 0, 0.5, 3, 0),
            "gmp_emb_link_rank": (p, 8, 5, 0, p, p, Q)}[name]
    extra = (0,) if name == "gmp_emb_link_rank" else ()                            # matrix_out
    return getattr(L.lib(), name)(*lead, *tail, *extra, 0, 0, None)


def _score(name, P=4, score=None, p=PTR):
    out = p if score is None else score
    args = {"gmp_lp_cn_score": (p, p, 8, 16, p, p, P, 0, 0, out, None),
            "gmp_lp_walk_score": (p, p, 8, 16, p, p, P, 0, 0.5, 3, 0, out, 0, 0, None),
            "gmp_emb_link_score": (p, 8, 5, 0, p, p, P, out, 0, 0, None)}[name]
    return getattr(L.lib(), name)(*args)


RANK_CASES = {"Q=-1": dict(Q=-1), "filter_nnz=-1": dict(fnnz=-1), "filter_rowptr alone": dict(frow=PTR, fnnz=1), "null n_equal": dict(n_equal=0),
              "Q=0, all null": dict(Q=0, p=0)}
SCORE_CASES = {"P=-1": dict(P=-1), "null score": dict(score=0), "P=0, all null": dict(P=0, p=0)}

# (code, gmp_last_error_string()) of every case, recorded from the commit before the rankers shared their front (lpf::rank_front,
# csr::graph_ok); None = the call succeeds and the text is not looked at
EXPECTED = {
    ("gmp_lp_rank", "Q=-1"): (-1, "lp_rank: N=8 Q=-1 filter_nnz=0"),
    ("gmp_lp_rank", "filter_nnz=-1"): (-1, "lp_rank: N=8 Q=4 filter_nnz=-1"),
    ("gmp_lp_rank", "filter_rowptr alone"): (-1, "lp_rank: filter_rowptr and filter_col must both be given or both be null"),
    ("gmp_lp_rank", "null n_equal"): (-1, "lp_rank: null pointer"),
    ("gmp_lp_rank", "Q=0, all null"): (0, None),
    ("gmp_lp_cn_rank", "Q=-1"): (-1, "lp_cn_rank: Q=-1 filter_nnz=0"),
    ("gmp_lp_cn_rank", "filter_nnz=-1"): (-1, "lp_cn_rank: Q=4 filter_nnz=-1"),
    ("gmp_lp_cn_rank", "filter_rowptr alone"): (-1, "lp_cn_rank: filter_rowptr and filter_col must both be given or both be null"),
    ("gmp_lp_cn_rank", "null n_equal"): (-1, "lp_cn_rank: null pointer"),
    ("gmp_lp_cn_rank", "Q=0, all null"): (-1, "lp_cn_rank: null pointer"),
    ("gmp_lp_walk_rank", "Q=-1"): (-1, "lp_walk_rank: Q=-1 filter_nnz=0"),
    ("gmp_lp_walk_rank", "filter_nnz=-1"): (-1, "lp_walk_rank: Q=4 filter_nnz=-1"),
    ("gmp_lp_walk_rank", "filter_rowptr alone"): (-1, "lp_walk_rank: filter_rowptr and filter_col must both be given or both be null"),
    ("gmp_lp_walk_rank", "null n_equal"): (-1, "lp_walk_rank: null pointer"),
    ("gmp_lp_walk_rank", "Q=0, all null"): (-1, "lp_walk_rank: null pointer"),
    ("gmp_emb_link_rank", "Q=-1"): (-1, "emb_link_rank: num_nodes=8 count=-1 dim=5 mode=0 (0 <= num_nodes, count < 2^31, 1 <= dim <= 256, mode 0 or 1)"),
    ("gmp_emb_link_rank", "filter_nnz=-1"): (-1, "emb_link_rank: filter_nnz=-1"),
    ("gmp_emb_link_rank", "filter_rowptr alone"): (-1, "emb_link_rank: filter_rowptr and filter_col must both be given or both be null"),
    ("gmp_emb_link_rank", "null n_equal"): (-1, "emb_link_rank: null pointer"),
    ("gmp_emb_link_rank", "Q=0, all null"): (0, None),
    ("gmp_lp_cn_score", "P=-1"): (-1, "lp_cn_score: P=-1"),
    ("gmp_lp_cn_score", "null score"): (-1, "lp_cn_score: null pointer"),
    ("gmp_lp_cn_score", "P=0, all null"): (-1, "lp_cn_score: null pointer"),
    ("gmp_lp_walk_score", "P=-1"): (-1, "lp_walk_score: P=-1"),
    ("gmp_lp_walk_score", "null score"): (-1, "lp_walk_score: null pointer"),
    ("gmp_lp_walk_score", "P=0, all null"): (-1, "lp_walk_score: null pointer"),
    ("gmp_emb_link_score", "P=-1"): (-1, "emb_link_score: num_nodes=8 count=-1 dim=5 mode=0 (0 <= num_nodes, count < 2^31, 1 <= dim <= 256, mode 0 or 1)"),
    ("gmp_emb_link_score", "null score"): (-1, "emb_link_score: null pointer"),
    ("gmp_emb_link_score", "P=0, all null"): (0, None),
}


def _refusals():
    out = {}
    for name in ("gmp_lp_rank", "gmp_lp_cn_rank", "gmp_lp_walk_rank", "gmp_emb_link_rank"):
        for case, kw in RANK_CASES.items():
            rc = _rank(name, **kw)
            out[(name, case)] = (rc, L.lib().gmp_last_error_string().decode() if rc else None)
    for name in ("gmp_lp_cn_score", "gmp_lp_walk_score", "gmp_emb_link_score"):
        for case, kw in SCORE_CASES.items():
            rc = _score(name, **kw)
            out[(name, case)] = (rc, L.lib().gmp_last_error_string().decode() if rc else None)
    return out


@pytest.fixture(scope="module")
def refusals():
    return _refusals()


@pytest.mark.parametrize("key", list(EXPECTED), ids=lambda k: f"{k[0]}-{k[1]}")
def test_refusals_are_the_parents(refusals, key):
    assert refusals[key] == EXPECTED[key]


def test_refusal_cases_are_complete():
    assert len(EXPECTED) == 4 * len(RANK_CASES) + 3 * len(SCORE_CASES) and _refusals().keys() == EXPECTED.keys()
    assert sum(1 for rc, _ in EXPECTED.values() if rc == 0) >= 3                   # a call without pairs may pass null everything ...
    assert EXPECTED[("gmp_emb_link_rank", "Q=0, all null")] == (0, None)           # ... where no earlier check reads a pointer


# ---------------------------------------------------------------------------- the rows of finetune.BASELINES
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]
H = ops.WL_MAX_ITERS
# per row: a domain it applies to and a value for the flag; two domains of other task types; a second domain at the largest value beside
# flags it must not need; command lines it combines with (extra flags, the config fields they give); whether the module's docstring
# names the flag; its C symbols, the argument counts pinned by hand where a test did, and what else their test asserted
ROWS = {
    "lp_heuristics": dict(
        on=("Cora_LP", True), off=("Cora_NC", "ENZYMES"), top=("CiteSeer_LP", True, dict(lp_engine=True, lp_ranking=True)), combos=(), doc=True,
        symbols=["gmp_lp_cn_tile_nodes", "gmp_lp_cn_rank_workspace_bytes", "gmp_lp_cn_score", "gmp_lp_cn_rank", "gmp_graph_simple_check"]),
    "lp_walks": dict(
        on=("Cora_LP", 6), off=("Cora_NC", "ENZYMES"), top=("CiteSeer_LP", 64, dict(lp_heuristics=True, lp_engine=True)), combos=(), doc=False,
        symbols=["gmp_lp_walk_lds_nodes", "gmp_lp_walk_resident_blocks", "gmp_lp_walk_workspace_bytes", "gmp_lp_walk_score", "gmp_lp_walk_rank"]),
    "wl_baseline": dict(
        on=("PTC_MR", 3), off=("Cora_NC", "Cora_LP"), top=("ENZYMES", H, {}), doc=True,
        combos=[(["--domain_name", "ENZYMES", "--gc-engine", "--wl-baseline", str(H), "--knn-probe", "5", "--cluster-probe", "2", "--logreg-probe", "10"],
                 dict(wl_baseline=H, knn_probe=5, cluster_probe=2, logreg_probe=10, gc_engine=True))],
        symbols=["gmp_wl_workspace_bytes", "gmp_wl_refine", "gmp_wl_gram"],
        more=lambda lib: lib.gmp_wl_workspace_bytes(600, 1024, 7) == 0),                    # everything lives in LDS
    "label_propagation": dict(
        on=("Cora_NC", 5), off=("Cora_LP", "ENZYMES"), top=("CiteSeer_NC", 10000, {}), combos=(), doc=True,
        symbols=["gmp_label_propagate_workspace_bytes", "gmp_label_propagate"],
        more=lambda lib: (lib.gmp_label_propagate_workspace_bytes(2708, 7) >= 2 * 2708 * 7 * 4 and lib.gmp_label_propagate_workspace_bytes(2708, 0) == 0
                          and lib.gmp_label_propagate_workspace_bytes(2708, 33) == 0 and lib.gmp_label_propagate_workspace_bytes(-1, 7) == 0)),
    "sgc_baseline": dict(
        on=("Cora_NC", 2), off=("Cora_LP", "ENZYMES"), top=("CiteSeer_NC", 64, {}), doc=True,
        combos=[(["--domain_name", "CiteSeer_NC", "--sgc-baseline", "3", "--label-propagation", "10", "--sparse-features"],
                 dict(sgc_baseline=3, label_propagation=10, sparse_features=True))],
        symbols=["gmp_feature_propagate_workspace_bytes", "gmp_feature_propagate"], counts=(3, 20), more=lambda lib: _sgc_workspace_rule(lib)),
    "sp_baseline": dict(
        on=("PTC_MR", 8), off=("Cora_NC", "Cora_LP"), top=("ENZYMES", ops.SP_MAX_DIST, {}), doc=True,
        combos=[(["--domain_name", "ENZYMES", "--gc-engine", "--sp-baseline", "1023", "--wl-baseline", "3", "--knn-probe", "5"],
                 dict(sp_baseline=1023, wl_baseline=3, knn_probe=5, gc_engine=True))],
        symbols=["gmp_sp_workspace_bytes", "gmp_sp_max_unique", "gmp_sp_features", "gmp_sp_gram"], counts=(2, 1, 19, 12),
        more=lambda lib: lib.gmp_sp_workspace_bytes(600, 1024) == 0 and lib.gmp_sp_max_unique(256) >= 4096 and lib.gmp_sp_max_unique(1024) >= 1024),
    "feat_baseline": dict(
        on=("PTC_MR", 2), off=("Cora_NC", "Cora_LP"), top=("ENZYMES", ops.GRAPH_FEAT_MAX_ROUNDS, {}), doc=True,
        combos=[(["--domain_name", "ENZYMES", "--gc-engine", "--feat-baseline", "3", "--sp-baseline", "8", "--wl-baseline", "3", "--knn-probe", "5"],
                 dict(feat_baseline=3, sp_baseline=8, wl_baseline=3, knn_probe=5, gc_engine=True))],
        symbols=["gmp_graph_feature_map"], counts=(16,),
        more=lambda lib: (lib.gmp_graph_feature_map(None, -1, None, None, 0, 0, None, None, None, 0, 1, 0, 0, None, None, None) == -1
                          and lib.gmp_graph_feature_map(None, 0, None, None, 0, 0, None, None, None, 0, 1, 0, 0, None, None, None) == 0)),
}
ROW_IDS = [b.field for b in FT.BASELINES]


def _sgc_workspace_rule(lib):
    ws = lib.gmp_feature_propagate_workspace_bytes
    return (ws(2708, 1433, 1) == 0                                                         # one round writes out directly
            and 2708 * 1436 * 4 <= ws(2708, 1433, 2) < 2 * 2708 * 1436 * 4                 # one buffer of n x dpad
            and ws(2708, 1433, 3) >= 2 * 2708 * 1436 * 4 and ws(2708, 1433, 64) == ws(2708, 1433, 3)       # never more than two
            and ws(2708, 0, 2) == 0 and ws(2708, 16385, 2) == 0 and ws(2708, 7, 0) == 0 and ws(2708, 7, 65) == 0 and ws(-1, 7, 2) == 0)


def _argv(b, domain, value):
    return ["--domain_name", domain, b.flag] + ([] if b.max_value is None else [str(value)]) + BASE


def test_the_tables():
    assert ROW_IDS == list(ROWS) and len(FT.PROBES) == 3                                   # the baselines are no probes: that table is untouched
    assert ROW_IDS == ["lp_heuristics", "lp_walks", "wl_baseline", "label_propagation", "sgc_baseline", "sp_baseline", "feat_baseline"]
    assert all(isinstance(b, FT.Baseline) for b in FT.BASELINES)                           # one table: no second tuple beside it
    assert not {b.field for b in FT.BASELINES} & {p.field for p in FT.PROBES}
    assert list(FT.FinetuneConfig.__dataclass_fields__)[-1] == "wl_baseline"              # appended, positional callers are undisturbed


@pytest.mark.parametrize("b", FT.BASELINES, ids=ROW_IDS)
def test_baseline_flag_parses_into_the_config_and_is_off_by_default(b):
    row = ROWS[b.field]
    domain, value = row["on"]
    off = False if b.max_value is None else 0
    cfg = FT.config_from_args(FT.build_parser().parse_args(_argv(b, domain, value)))
    assert getattr(cfg, b.field) == value and type(getattr(cfg, b.field)) is type(value)
    # it needs no engine flag, no ranking, no probe and no other baseline
    assert not cfg.lp_engine and not cfg.gc_engine and not cfg.lp_ranking and not any(getattr(cfg, p.field) for p in FT.PROBES)
    assert not any(getattr(cfg, o.field) for o in FT.BASELINES if o is not b)
    default = getattr(FT.config_from_args(FT.build_parser().parse_args(["--domain_name", domain] + BASE)), b.field)
    assert default == off and type(default) is type(off)                                   # opt-in
    assert getattr(FT.FinetuneConfig(domain, "full_finetune", "b1", 1), b.field) == off
    top_domain, top, beside = row["top"]
    assert getattr(FT.FinetuneConfig(top_domain, "full_finetune", "b1", 1, **{b.field: top}, **beside), b.field) == top
    assert top is True or top == b.max_value
    for extra, want in row["combos"]:
        both = FT.config_from_args(FT.build_parser().parse_args(extra + BASE))
        assert {k: getattr(both, k) for k in want} == want
    assert not row["doc"] or b.flag in FT.__doc__


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("b", FT.BASELINES, ids=ROW_IDS)
def test_baseline_is_refused_off_its_task_type(b, which):
    domain, value = ROWS[b.field]["off"][which], ROWS[b.field]["on"][1]
    assert FT.TASK_TYPES[domain] != b.task_type
    with pytest.raises(ValueError, match=b.field):
        FT.config_from_args(FT.build_parser().parse_args(_argv(b, domain, value)))
    with pytest.raises(ValueError, match=f"{b.field} applies to the .* domains \\({re.escape(b.domains)}\\), not to {domain}"):
        FT.FinetuneConfig(domain_name=domain, finetune_strategy="full_finetune", pretrained_scheme="b1", seed=1, **{b.field: value})
    assert not getattr(FT.FinetuneConfig(domain, "full_finetune", "b1", 1), b.field)        # off, it is at home everywhere


# the two rankers that need an engine and are no rows of the table have their symbols checked the same way
SYMBOLS = {**{field: row for field, row in ROWS.items()},
           "lp_rank": dict(symbols=["gmp_lp_rank_workspace_bytes", "gmp_lp_topk_workspace_bytes", "gmp_lp_rank", "gmp_lp_topk"]),
           "emb_link": dict(symbols=["gmp_emb_link_workspace_bytes", "gmp_emb_link_score", "gmp_emb_link_rank"], counts=(3, 11, 17))}


@pytest.mark.parametrize("family", list(SYMBOLS))
def test_symbols_are_declared_bound_and_exported(family):
    row = SYMBOLS[family]
    for i, name in enumerate(row["symbols"]):       # declared and exported: test_layout.FEATURE_SYMBOLS
        assert "counts" not in row or len(L._SIGS[name][1]) == row["counts"][i]
    assert "more" not in row or row["more"](L.lib())
