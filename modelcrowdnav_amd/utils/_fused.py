"""What Trainer(fused=True) and Trainer_Sim(fused=True) both do to a module's parameters on the way to the HIP training
steps (csrc/sarl_train.hip, csrc/value_train.hip, csrc/world_train.hip, csrc/world_mlp_train.hip): the flat float32 buffers and their layout, the check of a state_dict
against a shape table, the workspace, and the pointer and row arithmetic of a launch."""
import ctypes as C

import torch


def layout(model):
    """[(state_dict key, offset, shape)] of the flat buffers, and their length: state_dict order, each tensor in
    torch's own row-major layout (include/mcn.h: mcn_sarl_train_param_count and its like)."""
    table, off = [], 0
    for k, v in model.state_dict().items():
        table.append((k, off, tuple(v.shape)))
        off += v.numel()
    return table, off


def linear_shapes(layers):
    """{state_dict key: shape} of the Linear layers `layers` ({layer: weight shape}): each one's .weight, then its .bias."""
    out = {}
    for k, shp in layers.items():
        out[k + ".weight"], out[k + ".bias"] = tuple(shp), tuple(shp[:1])
    return out


def mismatch(sd, expect, count, layers_why, count_why):
    """Why the state_dict `sd` is not the network of `expect` ({state_dict key: shape}, in state_dict order) in float32
    with count() parameters (the library's own figure, asked for last), or None: the caller's two texts, or the first
    tensor of another shape."""
    if list(sd.keys()) != list(expect):
        return layers_why
    for k, shp in expect.items():
        if tuple(sd[k].shape) != shp:
            return "%s is %s, expected %s" % (k, tuple(sd[k].shape), shp)
    if any(v.dtype != torch.float32 for v in sd.values()):
        return "its parameters are not float32"
    return count_why if sum(v.numel() for v in sd.values()) != count() else None


def buffers(z, names, params, dev):
    """`z` if it holds buffers of the parameters' size on `dev`, else new zero buffers under `names` and no workspace yet;
    z["params"] is loaded from the module, the master copy: load_state_dict, sync_weights or apply(init_weight) since the
    last call are honoured."""
    count = sum(p.numel() for p in params)
    if z is None or z["params"].numel() != count or z["params"].device != dev:
        z = dict({k: torch.zeros(count, dtype=torch.float32, device=dev) for k in names}, ws=None)
    torch.cat([p.detach().reshape(-1) for p in params], out=z["params"])
    return z


def store(z, params, table):
    # p.copy_ (not p.data): the version counters move, so packed HIP weights of the model are re-made
    for p, (_, off, _shape) in zip(params, table):
        p.copy_(z["params"][off:off + p.numel()].view_as(p))


def workspace(z, need):
    """z["ws"] with room for `need` bytes: it only grows."""
    if z["ws"] is None or z["ws"].numel() < need:
        z["ws"] = torch.empty(need, dtype=torch.uint8, device=z["params"].device)
    return z["ws"]


def at(t, first, width=1):
    """Pointer to row `first` of the contiguous tensor t taken as rows of `width` elements."""
    return C.c_void_p(t.data_ptr() + first * width * t.element_size())


def bad_row(rows, n):
    """The kernels trust their rows, so the host checks them: an entry of the int64 host tensor `rows` outside 0 .. n-1
    (the largest if that is too large, else the smallest), or None."""
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        return int(rows.max()) if int(rows.max()) >= n else int(rows.min())
    return None
