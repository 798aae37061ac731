"""World-model trainer (reference: crowd_nav/utils/trainer_sim.py:26-110 + pytorchtools.py EarlyStopping): Adam + MSE
on (humans' [px,py,vx,vy], their next velocities) pairs -- the `rawob` rows the explorers collect
(explorer.py:84-86) or `RealData.world_pairs()` -- with an 80 / 20 train / validation split, early stopping
(patience 7) on the validation loss, the best weights restored at the end and `model.mse` set to the best validation
loss (MlpWorld.noise_pre uses it).

The pairs are stacked into two device tensors once and mini-batches are index slices of them (the reference builds
two torch DataLoaders over Python lists per call); pairs whose pedestrian count differs from the first pair's are
dropped, as its collate_fn does (trainer_sim.py:15-23).

`Trainer_Sim(..., fused=True)` (opt-in; `Trainer_Sim.fused_default` for drop-in users) replaces autograd and torch's Adam
by the HIP training step of csrc/world_train.hip for the default-shaped AttentionWorld: per mini-batch one
mcn_attn_world_loss_grad and one mcn_adam_step on flat parameter / gradient / moment buffers, the validation pass as
forward-only launches, the row indices of an epoch uploaded once and its validation losses read back once.  The split,
the batches, early stopping and the best weights are those of the torch path.  Known difference:
`model.attention_weights` is not updated, because no torch forward runs.

An MlpWorld (4N -> 128 -> 64 -> 12 -> 2N, both Dropouts with the same p in [0, 1)) is trained the same way by
csrc/world_mlp_train.hip: mcn_mlp_world_loss_grad in place of mcn_attn_world_loss_grad, everything else as above
(`_fused_step` picks the step by the model's class).  Its dropout masks come from the library's own counter hash
(include/mcn.h: mcn_dropout_mask) under `trainer.dropout_seed` -- settable; by default torch.initial_seed(), read at the
first fused call -- and a count of the fused training steps since the trainer was made, which nothing resets: a round
that starts Adam over (set_learning_rate) does not replay the masks of an earlier round.  Two known differences from
the torch path: the masks are not torch's; and without `perms` the torch path's LATER permutations differ from the
fused path's, because its dropout draws from the same device generator as `randperm`.
"""
import collections
import copy
import logging
import random

import torch
import torch.nn as nn
import torch.optim as optim

from . import _fused


# What differs between the fused steps: the launch's name, the library's workspace(B, N) and launch(params, cur, nxt, rows,
# B, N, ws, grad, loss, stream, mask_step) -- mask_step is the trainer's count of fused training steps, which only a step
# with dropout looks at --, the model's own pedestrian count (None: any) and what the device refusal says.
_Step = collections.namedtuple("_Step", "name workspace launch humans no_gpu")


def _fused_step(trainer):
    """(the _Step that trains trainer.model, None), or (None, why there is none)."""
    from .. import _hip
    from ..policy.world_model import AttentionWorld, MlpWorld
    lib, m = _hip.lib, trainer.model
    if isinstance(m, MlpWorld):
        lin = [k for k in m.mlp if isinstance(k, nn.Linear)]
        N = lin[0].in_features // 4 if lin else 0
        expect = {"mlp.0": (128, 4 * N), "mlp.3": (64, 128), "mlp.6": (12, 64), "mlp.8": (2 * N, 12)}
        drops = [float(k.p) for k in m.mlp if isinstance(k, nn.Dropout)]
        if not lin or lin[0].in_features != 4 * N or not 1 <= N <= _hip.MAX_HUMANS:
            why = "mlp.0 takes %s inputs, not 4 N with N in 1 .. %d" % (lin[0].in_features if lin else "no", _hip.MAX_HUMANS)
        else:
            why = _fused.mismatch(
                m.state_dict(), _fused.linear_shapes(expect), lambda: int(lib.mcn_mlp_world_train_param_count(N)),
                "its layers are not MlpWorld's (mlp.0, mlp.3, mlp.6, mlp.8: 4N-128-64-12-2N)",
                "its parameter count is not mcn_mlp_world_train_param_count(N)")
        if why is None and (len(drops) != 2 or drops[0] != drops[1]):
            why = "its dropout rates are %s, not one rate for both layers" % (drops,)
        if why is None and not 0.0 <= drops[0] < 1.0:
            why = "its dropout rate is %g, outside [0, 1)" % drops[0]
        if why is not None:
            return None, "world_mlp_train.hip is built for MlpWorld (4N-128-64-12-2N); this model cannot be trained by it: " + why
        p = drops[0]

        def launch(params, cur, nxt, rows, B, n, ws, grad, loss, stream, mask_step):
            return lib.mcn_mlp_world_loss_grad(params, cur, nxt, rows, B, n, p, trainer._mask_seed(), mask_step, ws, grad,
                                               loss, stream)
        return _Step("mcn_mlp_world_loss_grad", lib.mcn_mlp_world_train_workspace_bytes, launch, N,
                     "the MlpWorld step draws its dropout masks on the device; "), None
    expect = {"mlp1.0": (150, 4), "mlp1.2": (100, 150), "mlp2.0": (100, 100), "mlp2.2": (50, 100),
              "attention.0": (100, 200), "attention.2": (100, 100), "attention.4": (1, 100),
              "mlp3.0": (150, 54), "mlp3.2": (100, 150), "mlp3.4": (100, 100), "mlp3.6": (2, 100)}
    if not isinstance(m, AttentionWorld) or m.input_dim != 4 or not m.with_global_state:
        why = "it is not an AttentionWorld with input_dim 4 and the global state"
    else:
        why = _fused.mismatch(
            m.state_dict(), _fused.linear_shapes(expect), lambda: int(lib.mcn_attn_world_train_param_count()),
            "its layers are not the default ones (mlp1 150-100, mlp2 100-50, attention 100-100-1, mlp3 150-100-100-2)",
            "its parameter count is not mcn_attn_world_train_param_count()")
    if why is not None:
        return None, "world_train.hip is built for the default AttentionWorld; this model cannot be trained by it: " + why

    def launch(params, cur, nxt, rows, B, n, ws, grad, loss, stream, mask_step):
        return lib.mcn_attn_world_loss_grad(params, cur, nxt, rows, B, n, ws, grad, loss, stream)
    return _Step("mcn_attn_world_loss_grad", lib.mcn_attn_world_train_workspace_bytes, launch, None, ""), None


class EarlyStopping(object):
    """pytorchtools.py:6-52: stop after `patience` epochs without a validation-loss improvement of more than delta;
    the best weights are kept (in memory, and at `path` when given)."""

    def __init__(self, patience=7, delta=0, path=None):
        self.patience, self.delta, self.path = patience, delta, path
        self.counter, self.best_score, self.early_stop = 0, None, False
        self.best_state = None

    def __call__(self, val_loss, model):
        score = -val_loss
        if self.best_score is None or not (score < self.best_score + self.delta):
            self.best_score = score
            self.best_state = copy.deepcopy(model.state_dict())
            if self.path is not None:
                torch.save(self.best_state, self.path)
            self.counter = 0
        else:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True


class Trainer_Sim(object):
    fused_default = False        # what `fused=None` means; a drop-in user may flip it

    def __init__(self, model, memory, device, batch_size, path=None, fused=None):
        self.model, self.memory, self.device, self.batch_size = model, memory, device, batch_size
        self.criterion = nn.MSELoss().to(device)
        self.optimizer = None
        self.train_size = 0.8
        self.patience = 7
        self.path = path
        self.early_stopping = EarlyStopping(patience=self.patience, path=path)
        self.fused = bool(Trainer_Sim.fused_default if fused is None else fused)
        self._fz = None                  # fused path: flat params / grad / Adam moments, workspace, step count
        self.dropout_seed = None         # fused MlpWorld: the seed of the masks; None = torch.initial_seed() at the first call
        self.mask_step = 0               # fused training steps since the trainer was made: the masks' step, never reset
        self.last_rows = None            # fused path: per epoch of the latest call (train row order, validation row order
        #                                  or None for rows 0 .. n_val-1), device tensors; rows index what _pairs() stacked
        if self.fused:
            self._fused_check()

    def set_learning_rate(self, learning_rate):
        logging.info("Current learning rate: %f", learning_rate)
        self.optimizer = optim.Adam(self.model.parameters(), lr=learning_rate)
        if self._fz is not None:         # the reference makes a new optimizer here: moments and step count start over
            self._fz["m"].zero_()
            self._fz["v"].zero_()
            self._fz["step"] = 0

    def _pairs(self):
        rows = self.memory.memory if hasattr(self.memory, "memory") else self.memory
        if not isinstance(rows, list):
            rows = list(rows)
        random.shuffle(rows)            # trainer_sim.py:55: Python's RNG, and IN PLACE -- the memory itself is reordered,
        #                                 so a second call splits what the first one left
        n_train = int(len(rows) * self.train_size)

        def stack(part):
            if not part:
                return None, None
            shape = tuple(part[0][0].shape)
            part = [p for p in part if tuple(p[0].shape) == shape]
            cur = torch.stack([torch.as_tensor(p[0], dtype=torch.float32) for p in part]).to(self.device)
            nxt = torch.stack([torch.as_tensor(p[1], dtype=torch.float32) for p in part]).to(self.device)
            return cur.reshape(cur.shape[0], -1), nxt.reshape(nxt.shape[0], -1)
        return stack(rows[:n_train]), stack(rows[n_train:])

    def optimize_epoch(self, num_epochs, reset=False, perms=None):
        """trainer_sim.py:48-110.  Returns the best validation loss.
        perms (optional): (train [num_epochs][n_train], validation [num_epochs][n_val]) row orders that replace the
        shuffles drawn here -- the reference's two DataLoaders draw theirs from torch's global generator."""
        if self.optimizer is None:
            raise ValueError("Learning rate is not set!")
        if self.fused:
            return self._fused_optimize(num_epochs, reset, perms)
        (tx, ty), (vx, vy) = self._pairs()
        if tx is None or vx is None:
            raise ValueError("not enough pairs to split into training and validation sets")
        es = self.early_stopping
        es.counter, es.early_stop = 0, False
        if reset:
            es.best_score = None
        B = self.batch_size
        for ep in range(num_epochs):
            self.model.train()
            if perms is None:
                perm = torch.randperm(tx.shape[0], device=tx.device)
            else:
                perm = torch.as_tensor(perms[0][ep], dtype=torch.long, device=tx.device)
                vperm = torch.as_tensor(perms[1][ep], dtype=torch.long, device=vx.device)
            for i in range(0, tx.shape[0], B):
                idx = perm[i:i + B]
                loss = self.criterion(self.model(tx[idx]), ty[idx])
                self.optimizer.zero_grad()
                loss.backward()
                self.optimizer.step()
            self.model.eval()
            with torch.no_grad():
                ex, ey = (vx, vy) if perms is None else (vx[vperm], vy[vperm])
                losses = [self.criterion(self.model(ex[i:i + B]), ey[i:i + B]).item() for i in range(0, ex.shape[0], B)]
            es(sum(losses) / len(losses), self.model)
            if es.early_stop:
                break
        self.model.load_state_dict(es.best_state)               # load best model
        self.model.mse = 0 - es.best_score                      # used to add noise to the MLP world
        return -es.best_score

    # ------------------------------------------------------------------ fused HIP step (csrc/world_train.hip, world_mlp_train.hip)
    def _fused_layout(self):
        return _fused.layout(self.model)

    def _mask_seed(self):
        if self.dropout_seed is None:
            self.dropout_seed = int(torch.initial_seed())
        return int(self.dropout_seed) & 0xFFFFFFFFFFFFFFFF

    def _fused_check(self):
        """ValueError for what the fused step is not built for."""
        self._step_hip, why = _fused_step(self)
        if why is not None:
            raise ValueError("Trainer_Sim(fused=True): " + why)
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise ValueError("Trainer_Sim(fused=True) runs HIP kernels: %sthe trainer's device is %s, not a GPU" %
                             (self._step_hip.no_gpu, dev))
        want = torch.cuda.current_device() if dev.index is None else dev.index
        for k, p in self.model.named_parameters():
            if p.device.type != "cuda" or p.device.index != want:
                raise ValueError("Trainer_Sim(fused=True): the model lives on %s (%s), the trainer on %s" % (p.device, k, dev))

    def _fused_optimize(self, num_epochs, reset, perms):
        from .. import _hip
        self._fused_check()              # the module may have been changed or moved since the trainer was made
        (tx, ty), (vx, vy) = self._pairs()
        if tx is None or vx is None:
            raise ValueError("not enough pairs to split into training and validation sets")
        dev = tx.device
        N = int(tx.shape[1]) // 4
        if tx.shape[1] != 4 * N or ty.shape[1] != 2 * N or vx.shape[1] != 4 * N or vy.shape[1] != 2 * N or \
                not 1 <= N <= _hip.MAX_HUMANS:
            raise ValueError("Trainer_Sim(fused=True): pairs are %s -> %s, the model takes [N <= %d][4] -> [N][2]" %
                             (tuple(tx.shape[1:]), tuple(ty.shape[1:]), _hip.MAX_HUMANS))
        step = self._step_hip
        if step.humans is not None and step.humans != N:
            raise ValueError("Trainer_Sim(fused=True): the pairs hold %d pedestrians, the model is built for %d" %
                             (N, step.humans))
        tx, ty, vx, vy = tx.contiguous(), ty.contiguous(), vx.contiguous(), vy.contiguous()
        nt, nv, B = int(tx.shape[0]), int(vx.shape[0]), int(self.batch_size)
        if B < 1:
            raise ValueError("Trainer_Sim(fused=True): batch size %d" % B)
        params = [p for _, p in self.model.named_parameters()]
        table, count = self._fused_layout()
        z = self._fz = _fused.buffers(self._fz, ("params", "grad", "m", "v"), params, dev)
        if "step" not in z:
            z["step"] = 0
            z["loss"] = torch.zeros(1, dtype=torch.float32, device=dev)      # a training batch's loss (never read back)
        group = self.optimizer.param_groups[0]
        lr, (beta1, beta2), eps = float(group["lr"]), group["betas"], float(group["eps"])
        es = self.early_stopping
        es.counter, es.early_stop = 0, False
        if reset:
            es.best_score = None
        stream = _hip.stream_ptr(dev)
        lib, ptr, at = _hip.lib, _hip.ptr, _fused.at
        self.last_rows = []
        self.model.eval()                # the mode the torch path leaves the module in
        with torch.no_grad():
            vloss = None
            for ep in range(num_epochs):
                if perms is None:
                    perm, vperm = torch.randperm(nt, device=dev), None
                else:
                    # the kernel trusts the rows: checked here, on the host, before they are uploaded
                    hp, hv = (torch.as_tensor(q[ep], dtype=torch.long).reshape(-1).cpu() for q in perms)
                    for h, n, what in ((hp, nt, "training"), (hv, nv, "validation")):
                        bad = _fused.bad_row(h, n)
                        if bad is not None:
                            raise IndexError("Trainer_Sim(fused=True): a %s permutation names row %d of %d" % (what, bad, n))
                    perm, vperm = hp.to(dev), hv.to(dev)
                self.last_rows.append((perm, vperm))
                n_rows = nv if vperm is None else int(vperm.numel())
                n_batches = -(-n_rows // B)
                # room for the largest batch of this epoch and for one loss per validation batch
                ws = _fused.workspace(z, int(step.workspace(min(B, max(int(perm.numel()), n_rows, 1)), N)))
                if vloss is None or vloss.numel() < n_batches:
                    vloss = torch.empty(n_batches, dtype=torch.float32, device=dev)
                for i in range(0, int(perm.numel()), B):
                    b = min(B, int(perm.numel()) - i)
                    _hip.check(step.launch(ptr(z["params"]), ptr(tx), ptr(ty), at(perm, i, 1), b, N, ptr(ws), ptr(z["grad"]),
                                           ptr(z["loss"]), stream, self.mask_step), step.name)
                    z["step"] += 1
                    self.mask_step += 1
                    _hip.check(lib.mcn_adam_step(ptr(z["params"]), ptr(z["m"]), ptr(z["v"]), ptr(z["grad"]), count, lr,
                                                 beta1, beta2, eps, z["step"], stream), "mcn_adam_step")
                for k in range(n_batches):
                    b = min(B, n_rows - k * B)
                    if vperm is None:        # rows k B .. of the validation tensors, in their own order
                        rc = step.launch(ptr(z["params"]), at(vx, k * B, 4 * N), at(vy, k * B, 2 * N), None, b, N, ptr(ws), None,
                                         at(vloss, k, 1), stream, 0)
                    else:
                        rc = step.launch(ptr(z["params"]), ptr(vx), ptr(vy), at(vperm, k * B, 1), b, N, ptr(ws), None,
                                         at(vloss, k, 1), stream, 0)
                    _hip.check(rc, step.name)
                losses = vloss[:n_batches].cpu().tolist()      # the epoch's one read-back
                _fused.store(z, params, table)
                es(sum(losses) / len(losses), self.model)
                if es.early_stop:
                    break
        self.model.load_state_dict(es.best_state)               # load best model
        self.model.mse = 0 - es.best_score                      # used to add noise to the MLP world
        return -es.best_score
