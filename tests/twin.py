"""A module's twin: a newly constructed module that holds the same weights and has never seen an optimizer step.

Every cache of a twin (the towers' weight packs and W^T copies, the L2 quantiser's norms, the decoder's layer-0 constant block) is built
by its first forward from the weights it was handed, so a twin is the reference for "what do these weights imply": the same kernels
with nothing remembered.  It does not rely on `invalidate_packs()` naming every cache."""
import copy

import torch


def fresh_twin(module: torch.nn.Module, build):
    """`build()` is the constructor call the test made for `module`.  The twin loads `module.state_dict()` (strict), goes to each
    tensor's device and dtype, and takes over `training` of every submodule and every tower's `activation_recompute`."""
    twin = build()
    twin.load_state_dict(module.state_dict(), strict=True)          # into the constructor's fp32: exact for bf16 and fp32 sources
    device = next(module.parameters()).device
    twin = twin.to(device)
    theirs = dict(module.named_parameters())
    theirs.update(dict(module.named_buffers()))
    mine = dict(twin.named_parameters())
    mine.update(dict(twin.named_buffers()))
    assert mine.keys() == theirs.keys()
    for name, t in mine.items():
        if t.dtype != theirs[name].dtype:                           # per tensor: a module may keep fp32 masters beside bf16 weights
            t.data = t.data.to(theirs[name].dtype)
        assert t.device == theirs[name].device and t.shape == theirs[name].shape, name
        assert t.data_ptr() != theirs[name].data_ptr(), name
    for (_, a), (_, b) in zip(module.named_modules(), twin.named_modules()):
        b.training = a.training
        if hasattr(a, "activation_recompute"):
            b.activation_recompute = a.activation_recompute
    return twin


def twin_optimizer(optimizer, make):
    """`make()` builds the twin's optimizer as the test built `optimizer`; it starts from a copy of `optimizer.state_dict()`, so that
    step counts and moments are aligned."""
    other = make()
    other.load_state_dict(copy.deepcopy(optimizer.state_dict()))
    return other
