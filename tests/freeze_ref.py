"""The reference's freeze rule (engine/trainer.py:247-267) restated over plain lists of key strings, written separately from
`train.apply_freeze`.  Pure Python: no torch, no package import.

    flags = frozen_flags(keys, floating, arrived_trainable, freeze)

keys: the `named_parameters()` keys in order; floating[i]: the parameter is floating point; arrived_trainable[i]: its requires_grad
before the rule ran; freeze: None, an int n or a list of layer indices.  -> requires_grad per key after the rule.

The package's on-purpose difference that changes a flag (and only one does): a key ending in `depth_bin_values` that matches no name
keeps the flag it arrived with (the reference would switch that constant table on).  `KEEPS` names it."""

KEEPS = ("depth_bin_values",)


def layer_indices(freeze):
    if isinstance(freeze, list):
        return list(freeze)
    if isinstance(freeze, int):
        return list(range(freeze))
    return []


def layer_names(freeze):
    out = []
    for x in layer_indices(freeze):
        out.append("model." + str(x) + ".")
    out.append(".dfl")
    return out


def matches(key, names):
    for n in names:
        if key.find(n) >= 0:
            return True
    return False


def frozen_flags(keys, floating, arrived_trainable, freeze):
    names = layer_names(freeze)
    flags = []
    for k, fl, rg in zip(keys, floating, arrived_trainable):
        if matches(k, names):
            flags.append(False)
        elif not rg and fl and not k.endswith(KEEPS):
            flags.append(True)
        else:
            flags.append(bool(rg))
    return flags


def frozen_keys(keys, freeze):
    names = layer_names(freeze)
    return [k for k in keys if matches(k, names)]
