"""Model helpers of the harness (the role of utils/modelutils.py:5-15)."""
import torch
import torch.nn as nn

DEV = torch.device('cuda:0')


def find_layers(module, layers=(nn.Conv2d, nn.Linear), name=''):
    """{qualified name: layer} for every module below `module` (itself included, under `name`) whose exact type is
    listed in `layers`, in registration order; the search does not descend into a matching module -- the
    contract of utils/modelutils.py:8-15, here as one walk over `named_modules` instead of a recursion."""
    wanted = tuple(layers)
    hits, closed = {}, []
    for path, sub in module.named_modules():
        if any(c == '' or path == c or path.startswith(c + '.') for c in closed):
            continue                                  # inside a layer that was already taken
        if type(sub) in wanted:
            hits[(name + '.' + path if name and path else name or path)] = sub
            closed.append(path)
    return hits


def find_experts(module, name=''):
    """{qualified name: module} for every sub-module that keeps its experts as stacked 3-D parameters ``gate_up_proj``
    [E, 2I, H] and ``down_proj`` [E, H, I] (current transformers' Mixtral: the `w1` / `w3` / `w2` Linears that
    utils/modelutils.py:8-15 found in the reference's transformers generation no longer exist).  Duck-typed: no
    transformers class is named."""
    hits = {}
    for path, sub in module.named_modules():
        gu, dn = getattr(sub, 'gate_up_proj', None), getattr(sub, 'down_proj', None)
        if isinstance(gu, nn.Parameter) and isinstance(dn, nn.Parameter) and gu.ndim == 3 and dn.ndim == 3:
            hits[(name + '.' + path if name and path else name or path)] = sub
    return hits
