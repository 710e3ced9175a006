"""The flags and FinetuneConfig fields of the three embedding probes (finetune.PROBES: --knn-probe, --cluster-probe, --logreg-probe):
defaults, parsing, bounds, and the configurations each is refused in.  Runs without a GPU."""
import pytest

from gnn_pretraining_amd.finetune import finetune as FT

BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]
# field, flag, a value inside the bounds, the upper bound, a value far beyond it
PROBES = [("knn_probe", "--knn-probe", 20, 64, 1000), ("cluster_probe", "--cluster-probe", 10, 64, 1000),
          ("logreg_probe", "--logreg-probe", 100, 10000, 100000)]


def test_the_table_lists_the_three_probes_in_order_with_their_bounds():
    assert [(p.field, p.flag, p.max_value) for p in FT.PROBES] == [(f, flag, top) for f, flag, _, top, _ in PROBES]


@pytest.mark.parametrize("field,flag,value,top,far", PROBES, ids=[p[0] for p in PROBES])
def test_probe_flag_and_config_field(field, flag, value, top, far):
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC"] + BASE)
    assert getattr(a, field) == 0 and getattr(FT.config_from_args(a), field) == 0
    assert getattr(FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1), field) == 0
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC", flag, str(value)] + BASE)
    assert getattr(a, field) == value and getattr(FT.config_from_args(a), field) == value
    others = [(f, fl, 2 + i) for i, (f, fl, *_) in enumerate(PROBES) if f != field]          # the upper bound, beside the other two probes
    a = FT.build_parser().parse_args(["--domain_name", "ENZYMES", "--gc-engine", flag, str(top)] + [s for _, fl, v in others for s in (fl, str(v))] + BASE)
    cfg = FT.config_from_args(a)
    assert getattr(cfg, field) == top and cfg.gc_engine and all(getattr(cfg, f) == v for f, _, v in others)
    for k in (-1, top + 1, far):
        with pytest.raises(ValueError, match=field):
            FT.config_from_args(FT.build_parser().parse_args(["--domain_name", "Cora_NC", flag, str(k)] + BASE))
    with pytest.raises(SystemExit):
        FT.build_parser().parse_args(["--domain_name", "Cora_NC", flag, "many"] + BASE)


@pytest.mark.parametrize("field,flag,value,top,far", PROBES, ids=[p[0] for p in PROBES])
def test_probe_is_refused_without_class_labels_or_without_an_engine(field, flag, value, top, far, monkeypatch):
    for domain in ("Cora_LP", "CiteSeer_LP"):
        with pytest.raises(ValueError, match="no class labels"):
            FT.FinetuneConfig(domain, "full_finetune", "b1", 1, lp_engine=True, **{field: value})
    with pytest.raises(ValueError, match="--gc-engine"):
        FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1, **{field: value})
    assert getattr(FT.FinetuneConfig("PTC_MR", "linear_probe", "b1", 1, gc_engine=True, **{field: value}), field) == value
    monkeypatch.setenv("GMP_FINETUNE_ENGINE", "0")
    with pytest.raises(ValueError, match="GMP_FINETUNE_ENGINE=0"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1, **{field: value})
    assert getattr(FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1), field) == 0          # off: nothing to refuse
