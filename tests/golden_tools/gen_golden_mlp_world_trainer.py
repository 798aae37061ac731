"""Golden fixture for the MlpWorld trainer, from the real reference (run in a container that has it):

    python -m tests.golden_tools.gen_golden_mlp_world_trainer

  g27_mlp_world_trainer  the reference's own Trainer_Sim (crowd_nav/utils/trainer_sim.py:26-110: Adam, MSE, 80 / 20 split
               after random.shuffle, early stopping, best weights restored, model.mse) on its own
               MlpWorld(5, drop_rate=0.0) (world_model.py:22-51) with seeded default-init weights.  p = 0 makes nn.Dropout
               the identity, so the run is reproducible: the only random inputs are `random.shuffle(memory)` (Python's
               generator, seeded here) and the two DataLoaders' shuffles, which draw from torch's global generator and
               are recorded by replaying identical DataLoaders over row indices from the same generator state, as
               g20_trainer_sim does (gen_golden_nets.py).  240 rows, batch 1000 (one batch per epoch), lr 1e-3, two calls
               of 5 and 3 epochs; the rows and the law they follow are g20's.
Keys: cur, next, w0__<tensor>, short_w1__<tensor> ('.' -> '__'), short_call<c>_train_perms, short_call<c>_val_perms,
short_best, short_mse, short_counter, short_stopped, short_rows.
"""
import os
import random
import tempfile

import numpy as np
import torch

from tests.golden_tools import gen_golden as G
from tests.golden_tools.gen_golden_nets import _state_dict_arrays

OUT = G.OUT


def g27_mlp_world_trainer():
    import torch.utils.data as tud
    from crowd_sim.envs.utils.state import JointState  # noqa: F401  (first: the reference's packages import each other)
    from crowd_nav.policy.world_model import MlpWorld
    from crowd_nav.utils.memory import ReplayMemory
    from crowd_nav.utils.trainer_sim import Trainer_Sim
    if not hasattr(np, "Inf"):              # pytorchtools.py:25 reads an alias numpy 2.x removed: this process only
        np.Inf = np.inf
    rng = np.random.RandomState(20)
    N, rows, calls, lr, tag = 5, 240, (5, 3), 1e-3, "short"
    cur = rng.uniform(-3, 3, (rows, N, 4)).astype(np.float32)
    nxt = (0.8 * cur[:, :, 2:4] + 0.05 * np.tanh(cur[:, :, 0:2])).astype(np.float32)        # a smooth law to fit
    rec = {"cur": cur, "next": nxt}

    class _Rows(tud.Dataset):
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            return i

    def replay(n_train, n_val, epochs):
        tl, vl = tud.DataLoader(_Rows(n_train), 1000, shuffle=True), tud.DataLoader(_Rows(n_val), 1000, shuffle=True)
        tp, vp = [], []
        for _ in range(epochs):
            tp.append(np.concatenate([b.numpy() for b in tl]).astype(np.int64))
            vp.append(np.concatenate([b.numpy() for b in vl]).astype(np.int64))
        return np.stack(tp), np.stack(vp)

    torch.manual_seed(200)
    model = MlpWorld(N, drop_rate=0.0)
    rec.update(_state_dict_arrays(model, "w0__"))
    mem = ReplayMemory(10000)
    for i in range(rows):
        mem.push((torch.from_numpy(cur[i]), torch.from_numpy(nxt[i])))
    n_train = int(rows * 0.8)
    with tempfile.TemporaryDirectory() as d:
        tr = Trainer_Sim(model, mem, torch.device("cpu"), 1000, os.path.join(d, "checkpoint.pt"))
        tr.set_learning_rate(lr)
        random.seed(2000)
        torch.manual_seed(201)
        state = torch.get_rng_state()
        bests = [tr.optimize_epoch(e) for e in calls]                # a second call keeps the best score
    torch.set_rng_state(state)
    for c, e in enumerate(calls):
        tp, vp = replay(n_train, rows - n_train, e)
        rec["%s_call%d_train_perms" % (tag, c)], rec["%s_call%d_val_perms" % (tag, c)] = tp, vp
    rec[tag + "_best"] = np.array(bests, np.float64)
    rec[tag + "_mse"] = np.array(model.mse, np.float64)
    rec[tag + "_counter"] = np.array(tr.early_stopping.counter)
    rec[tag + "_stopped"] = np.array(bool(tr.early_stopping.early_stop))
    rec[tag + "_rows"] = np.array(rows)
    rec.update(_state_dict_arrays(model, tag + "_w1__"))
    print("  %s: best %s, mse %.6g, counter %d, stopped %s" % (tag, bests, model.mse, tr.early_stopping.counter,
                                                             tr.early_stopping.early_stop))
    np.savez_compressed(os.path.join(OUT, "g27_mlp_world_trainer.npz"), **rec)
    print("g27_mlp_world_trainer: %d arrays" % len(rec))


if __name__ == "__main__":
    g27_mlp_world_trainer()
