"""What the reference's `mrgcn/tasks/utils.py` exports, for scripts that import `mrgcn.tasks.utils` after
`mrgcn_amd.install_as_mrgcn()`: the optimizer's parameter groups and `EarlyStop`."""
from ..train import EarlyStop  # noqa: F401


def optimizer_params(model, optim_config, featureless):
    """Parameter groups as the reference forms them (tasks/utils.py:8-45): group 0 takes everything without a
    configuration of its own; unless `featureless`, group 1 takes `gate_weights` with `optim_config["gate_weights"]`;
    the parameters of an encoder `module_dict.<prefix>_<type>_...` share one group per datatype `<prefix>.<type>`,
    created on first sight and configured by `optim_config[datatype]`.  Frozen parameters are left out."""
    groups = [{"params": []}]
    where = {"default": 0}
    if not featureless:
        groups.append({"params": []})
        where["gates"] = 1
    for name, p in model.named_parameters(recurse=True):
        if not p.requires_grad:
            continue
        parts = name.split(".")
        if parts[0] == "module_dict":
            datatype = ".".join(parts[1].split("_")[:2])
            if datatype not in where:
                where[datatype] = len(groups)
                groups.append({"params": []})
            g = groups[where[datatype]]
            g["params"].append(p)
            g.update(optim_config[datatype])
        elif parts[0] == "gate_weights" and not featureless:
            g = groups[where["gates"]]
            g["params"].append(p)
            g.update(optim_config["gate_weights"])
        else:
            groups[where["default"]]["params"].append(p)
    return groups
