"""The step descriptor of include/gnnmp_step.h, as _abi.py reads it (gmp_step_desc_size() is compared against the
header's size when the library loads)."""
from ._lib import ABI, K

Mlp2, TaskDesc, LayerDesc, StepDesc = (ABI.structs["gmp_" + n] for n in ("mlp2", "task_desc", "layer_desc", "step_desc"))
MAXD, MAXT, LAYERS, MAXG = K["GMP_STEP_MAX_DOMAINS"], K["GMP_STEP_MAX_TASKS"], K["GMP_STEP_LAYERS"], K["GMP_STEP_MAX_ENC_GROUPS"]
TASK_KIND = {"node_feat_mask": K["GMP_TASK_NFM"], "link_pred": K["GMP_TASK_LP"], "node_contrast": K["GMP_TASK_NC"],
             "graph_contrast": K["GMP_TASK_GC"], "graph_prop": K["GMP_TASK_GP"], "domain_adv": K["GMP_TASK_DA"]}
