"""Golden fixture for the trainers of LSTM-RL and CADRL, from the real reference (run in a container that has it):

    python -m tests.golden_tools.gen_golden_value_trainers

  g26_value_trainers  the reference's own Trainer (crowd_nav/utils/trainer.py:19-82: SGD momentum 0.9, MSE) on its own
               lstm_rl.ValueNetwork1 (lstm_rl.py:9-33) and cadrl.ValueNetwork (cadrl.py:22-29) with seeded default-init
               weights and the shipped dimensions.  Per network: the weights w0, a memory of 100 (state, value) pairs
               -- state [5, 13] for LSTM-RL, [13] for CADRL -- which is exactly one batch, so every step sees all rows
               (the DataLoader's shuffle only permutes them inside the batch); lr 0.01; three optimize_batch(1); their
               losses and the weights w1 after them.
Keys: <policy>_w0__<tensor>, <policy>_w1__<tensor> ('.' -> '__', in state_dict order: the order the flat buffers of
csrc/value_train.hip rely on, recorded as <policy>_keys), <policy>_states, <policy>_values, <policy>_losses.
"""
import os

import numpy as np
import torch

from tests.golden_tools import gen_golden as G
from tests.golden_tools.gen_golden_nets import _state_dict_arrays

OUT = G.OUT
MLP_DIMS = [150, 100, 100, 1]


def g26_value_trainers():
    from crowd_sim.envs.utils.state import JointState  # noqa: F401  (first: the reference's packages import each other)
    from crowd_nav.policy.cadrl import ValueNetwork
    from crowd_nav.policy.lstm_rl import ValueNetwork1
    from crowd_nav.utils.memory import ReplayMemory
    from crowd_nav.utils.trainer import Trainer
    rec = {}
    rng = np.random.RandomState(26)
    for policy, shape in (("lstm_rl", (5, 13)), ("cadrl", (13,))):
        torch.manual_seed(26)
        model = ValueNetwork1(13, 6, MLP_DIMS, 50) if policy == "lstm_rl" else ValueNetwork(13, MLP_DIMS)
        rec[policy + "_keys"] = np.array(list(model.state_dict().keys()))
        rec.update(_state_dict_arrays(model, policy + "_w0__"))
        states = rng.normal(0, 1, (100,) + shape).astype(np.float32)
        if policy == "lstm_rl":
            states[:, :, :6] = states[:, :1, :6]            # the robot's columns are shared by the rows of a state
        values = rng.uniform(-0.5, 1.0, (100, 1)).astype(np.float32)
        mem = ReplayMemory(100)
        for s_, v_ in zip(states, values):
            mem.push((torch.from_numpy(s_), torch.from_numpy(v_)))
        tr = Trainer(model, mem, torch.device("cpu"), 100)
        tr.set_learning_rate(0.01)
        torch.manual_seed(77)
        losses = [tr.optimize_batch(1) for _ in range(3)]
        rec[policy + "_states"], rec[policy + "_values"] = states, values
        rec[policy + "_losses"] = np.array(losses, np.float64)
        rec.update(_state_dict_arrays(model, policy + "_w1__"))
    np.savez_compressed(os.path.join(OUT, "g26_value_trainers.npz"), **rec)
    print("g26_value_trainers: %d arrays" % len(rec))


if __name__ == "__main__":
    g26_value_trainers()
