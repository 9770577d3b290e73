"""Shared by test_step_recovery_host and test_gpu_step_recovery: how the tests look at HipAdam's gradient-pointer tables without
depending on the names of its attributes."""
import torch


def owned_tensors(obj):
    """every tensor reachable from the attributes of ``obj`` through lists, tuples and dicts"""
    out, seen = [], set()

    def visit(v):
        if id(v) in seen:
            return
        seen.add(id(v))
        if torch.is_tensor(v):
            out.append(v)
        elif isinstance(v, (list, tuple)):
            for e in v:
                visit(e)
        elif isinstance(v, dict):
            for e in v.values():
                visit(e)
    visit(vars(obj))
    return out


def owner_of(opt, addr):
    """the tensor at device (or host) address ``addr`` that the optimiser keeps alive, or None"""
    for t in owned_tensors(opt):
        if t.data_ptr() == addr and t.dtype == torch.int64:
            return t
    return None


def stale_table_entries(opt):
    """the keys of ``opt._tables`` (gradient addresses) whose table does not hold those addresses"""
    return [key for key, entry in opt._tables.items() if entry[0].tolist() != list(key)]
