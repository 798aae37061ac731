"""Host-side packing of a Linear layer into the MFMA fragments the network kernels read (include/mcn.h:
mcn_pack_linear), and the slot maps that say which feature sits in which of a tile's 16 slots."""
import ctypes as C

import numpy as np
import torch

from . import _hip


def ident(kin, tiles, offset=0):
    """Slot -> feature map of a `kin`-wide activation held in `tiles` tiles of 16.  Full tiles are in natural
    order; the ragged last tile is packed "q first" (feature j at slot 4(j%4) + j/4) so that its consumers need
    only ceil(w/4) k-steps (include/mcn.h, mcn_pack_linear).  offset: first weight column."""
    m = np.full(tiles * 16, -1, np.int32)
    full = (kin // 16) * 16 if kin % 16 else kin
    m[:full] = np.arange(full)
    for j in range(kin - full):
        m[full + 4 * (j % 4) + j // 4] = full + j
    m[m >= 0] += offset
    return m


def natural(kin, tiles, offset=0):
    """Feature j at slot j, the ragged tile included."""
    m = np.full(tiles * 16, -1, np.int32)
    m[:kin] = np.arange(kin) + offset
    return m


def pack_linear(W, b, kmap, omap, dev, bias=True, host=False, what="mcn_pack_linear"):
    """One layer (weight [nout, kin], bias [nout] float32 numpy) -> (device weight fragments, device bias fragments)
    through mcn_pack_linear; kmap / omap: input / output slot maps (KT = len(kmap) / 16, NT = len(omap) / 16;
    omap None: natural order, NT = ceil(nout / 16)).  bias=False: no bias fragment (None in its place);
    host=True: the host weight fragment as a third result (what mcn_pack_x3 regroups)."""
    W, b = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32)
    nout, kin = W.shape
    kmap = np.ascontiguousarray(kmap, np.int32)
    KT = len(kmap) // 16
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    if omap is None:
        NT, om = (nout + 15) // 16, None
    else:
        omap = np.ascontiguousarray(omap, np.int32)
        NT, om = len(omap) // 16, omap.ctypes.data_as(ip)
    wf = np.zeros((NT, KT, 64, 4), np.float32)
    bf = np.zeros((NT, 64, 4), np.float32)
    _hip.check(_hip.lib.mcn_pack_linear(W.ctypes.data_as(fp), b.ctypes.data_as(fp), nout, kin, kmap.ctypes.data_as(ip),
                                        KT, om, NT, wf.ctypes.data_as(fp), bf.ctypes.data_as(fp) if bias else None), what)
    out = (torch.from_numpy(wf).to(dev), torch.from_numpy(bf).to(dev) if bias else None)
    return out + (wf,) if host else out


def pack_layers(net, plan, dev):
    """A network of Linear layers into the ctypes struct `net`: plan rows (name, weight, bias, kmap, omap) go through
    pack_linear into the fields w_<name> / b_<name>.  Returns (net, [device tensors kept alive])."""
    keep = []
    for name, W, b, kmap, omap in plan:
        dw, db = pack_linear(W, b, kmap, omap, dev)
        keep += [dw, db]
        setattr(net, "w_" + name, dw.data_ptr())
        setattr(net, "b_" + name, db.data_ptr())
    return net, keep
