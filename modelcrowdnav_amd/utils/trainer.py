"""Value-network trainer (reference: crowd_nav/utils/trainer.py:19-82): SGD(momentum 0.9) + MSE on
(state, value) pairs from the replay memory.

Data-parallel: when torch.distributed is initialised every rank trains on its own memory shard and the
gradients are averaged with ONE all-reduce of a single flat bucket per step (96 502 floats = 386 KB: latency-
bound on xGMI, so one message, not one per tensor).  Weights start identical (broadcast from rank 0 in
`sync_weights`) and stay identical because every rank applies the same averaged gradient.  Ranks hold different
amounts of experience (episode lengths differ per env shard), so the number of steps of an epoch is agreed on ONCE
per epoch (all-reduce MAX of the local batch counts) and a rank that runs out of rows wraps around its own
permutation: every rank issues the same number of collectives, every batch is full.

The arithmetic (one SGD-momentum step of the MSE loss) is pinned against the reference's own Trainer by
tests/golden/g10_trainer.npz (tests/test_training_cpu.py).

`Trainer(..., fused=True)` (opt-in; `Trainer.fused_default` for drop-in users) replaces autograd and the torch optimizer
by a HIP training step: per mini-batch three launches (loss and per-workgroup gradients, their sum, SGD-momentum) on flat
parameter / gradient / momentum buffers, the row indices of all batches of a call uploaded once and the losses read back
once.  It draws the same batches from the same generator as the torch path.  Which file trains what (`_fused_step`):
csrc/sarl_train.hip the shipped SARL / OM-SARL ValueNetwork, csrc/value_train.hip the shipped LSTM-RL ValueNetwork1 and
the shipped CADRL ValueNetwork; the 150-100-100-1 head with its loss (train_head.hpp) and the SGD-momentum kernel
(sarl_train.hip) are the same for all three.
"""
import collections
import logging

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.optim as optim

from . import _fused


# What differs between the fused steps: the launch's name, the shape of one state in the memory (None: the human count N,
# 1 .. MCN_MAX_HUMANS), and the library's workspace(B, N) and launch(params, states, values, rows, B, N, ws, grad, loss,
# stream) with the network's own extra arguments bound.
_Step = collections.namedtuple("_Step", "name state_shape workspace launch")


def _fused_step(m):
    """(the _Step that trains the module `m`, None), or (None, why there is none)."""
    from .. import _hip
    from ..policy import cadrl, lstm_rl, sarl
    lib = _hip.lib
    if isinstance(m, lstm_rl.ValueNetwork1):
        layers, lstm = lstm_rl.shipped_shapes()
        expect = dict(_fused.linear_shapes(layers), **lstm)
        why = "its self state is not 6 wide" if m.self_state_dim != 6 else _fused.mismatch(
            m.state_dict(), expect, lambda: int(lib.mcn_lstm_rl_train_param_count()),
            "its tensors are not the shipped ones (policy.config [lstm_rl]: global_state_dim = 50, mlp2_dims = 150, 100, 100, 1)",
            "its parameter count is not mcn_lstm_rl_train_param_count()")
        if why is not None:
            return None, ("value_train.hip is built for the shipped LSTM-RL ValueNetwork1; this model cannot be trained by "
                          "it: " + why)
        return _Step("mcn_lstm_rl_loss_grad", (None, 13), lib.mcn_lstm_rl_train_workspace_bytes, lib.mcn_lstm_rl_loss_grad), None
    if isinstance(m, cadrl.ValueNetwork):
        why = _fused.mismatch(
            m.state_dict(), _fused.linear_shapes(cadrl.shipped_shapes()),
            lambda: int(lib.mcn_cadrl_train_param_count()),
            "its layers are not the shipped ones (policy.config [cadrl]: mlp_dims = 150, 100, 100, 1)",
            "its parameter count is not mcn_cadrl_train_param_count()")
        if why is not None:
            return None, ("value_train.hip is built for the shipped CADRL ValueNetwork; this model cannot be trained by it: "
                          + why)
        return _Step("mcn_cadrl_loss_grad", (13,), lambda B, N: lib.mcn_cadrl_train_workspace_bytes(B),
                     lambda params, states, values, rows, B, N, *out: lib.mcn_cadrl_loss_grad(params, states, values, rows, B,
                                                                                                *out)), None
    if isinstance(m, sarl.ValueNetwork):
        if not m.with_global_state or m.self_state_dim != 6:
            why = "it is not a SARL ValueNetwork with the global state and a 6-wide self state"
        else:
            sd = m.state_dict()
            D = sd["mlp1.0.weight"].shape[1] if "mlp1.0.weight" in sd else -1
            why = _fused.mismatch(sd, _fused.linear_shapes(sarl.shipped_shapes(D)) if D in (13, 61) else {},   # (no layers:
                                  lambda: int(lib.mcn_sarl_train_param_count(D)),                  # any state_dict differs)
                                  "its layers are not the shipped ones (policy.config:44-50, input_dim 13 or 61)",
                                  "its parameter count is not mcn_sarl_train_param_count(%d)" % D)
        if why is not None:
            return None, ("sarl_train.hip is built for the shipped SARL value network; this model cannot be trained by it: "
                          + why)
        return _Step("mcn_sarl_loss_grad", (None, D), lambda B, N: lib.mcn_sarl_train_workspace_bytes(B, N, D),
                     lambda params, *rest: lib.mcn_sarl_loss_grad(params, D, *rest)), None
    return None, ("the HIP training steps are built for the shipped SARL value network (sarl_train.hip), the shipped LSTM-RL "
                  "ValueNetwork1 and the shipped CADRL ValueNetwork (value_train.hip); this model is a %s, which none of "
                  "them can train" % type(m).__name__)


class Trainer(object):
    fused_default = False        # what `fused=None` means; a drop-in user may flip it

    def __init__(self, model, memory, device, batch_size, fused=None):
        self.model = model
        self.device = device
        self.criterion = nn.MSELoss().to(device)
        self.memory = memory
        self.data_loader = None          # kept for attribute compatibility; batches come from memory.sample
        self.batch_size = batch_size
        self.optimizer = None
        self._flat = None
        self._gen = torch.Generator()
        self.fused = bool(Trainer.fused_default if fused is None else fused)
        self._fz = None                  # fused path: flat params / grad / momentum, workspace
        self._step_hip = None            # fused path: the _Step that trains this model
        self.last_rows = None            # fused path: the memory rows of each mini-batch of the latest call (host)
        if self.fused:
            self._fused_check()

    def set_learning_rate(self, learning_rate):
        logging.info("Current learning rate: %f", learning_rate)
        self.optimizer = optim.SGD(self.model.parameters(), lr=learning_rate, momentum=0.9)
        if self._fz is not None:
            self._fz["mom"].zero_()      # the reference makes a new optimizer here: the momentum starts over

    # ------------------------------------------------------------------ data parallel helpers
    @staticmethod
    def _grouped():
        return dist.is_available() and dist.is_initialized()

    @staticmethod
    def _world():
        return dist.get_world_size() if Trainer._grouped() else 1

    @staticmethod
    def _collective(fn, t):
        """Run collective `fn` on tensor t where the backend can see it: RCCL ('nccl') works on device memory; under
        gloo (CPU rehearsals, several ranks sharing one GPU in tests) device tensors make the trip through a host copy."""
        if t.is_cuda and dist.get_backend() == "gloo":
            h = t.cpu()
            fn(h)
            t.copy_(h)
        else:
            fn(t)

    def sync_weights(self, src=0):
        """Every rank takes rank `src`'s parameters.  A collective's in-place write does not bump a tensor's version
        counter, so each parameter is broadcast into a buffer and copied in under no_grad: the copy bumps it, and packed
        HIP weights of the model (_hip.weights_stamp) are re-made at their next use."""
        if self._world() > 1:
            with torch.no_grad():
                for p in self.model.parameters():
                    buf = p.detach().clone()
                    self._collective(lambda t: dist.broadcast(t, src), buf)
                    p.copy_(buf)

    def _allreduce_grads(self):
        # a process group of ONE rank still runs the collective (the world-size-1 RCCL test exercises exactly the
        # call an N-rank job makes); without a group there is nothing to reduce
        if not self._grouped():
            return
        ws = self._world()
        params = [p for p in self.model.parameters() if p.grad is not None]
        n = sum(p.grad.numel() for p in params)
        if self._flat is None or self._flat.numel() != n or self._flat.device != params[0].grad.device:
            self._flat = torch.empty(n, dtype=params[0].grad.dtype, device=params[0].grad.device)
        off = 0
        for p in params:
            k = p.grad.numel()
            self._flat[off:off + k].copy_(p.grad.reshape(-1))
            off += k
        self._collective(dist.all_reduce, self._flat)          # one bucket, one collective
        if ws > 1:
            self._flat.div_(ws)
        off = 0
        for p in params:
            k = p.grad.numel()
            p.grad.copy_(self._flat[off:off + k].view_as(p.grad))
            off += k

    def _step(self, inputs, values):
        self.optimizer.zero_grad()
        loss = self.criterion(self.model(inputs), values)
        loss.backward()
        self._allreduce_grads()
        self.optimizer.step()
        return loss.data.item()

    # ------------------------------------------------------------------ fused HIP step (csrc/sarl_train.hip, value_train.hip)
    def _fused_layout(self):
        return _fused.layout(self.model)

    def _fused_check(self):
        """ValueError for what the fused step is not built for.  The memory is looked at again at every call: rows
        arrive after the trainer is made."""
        self._step_hip, why = _fused_step(self.model)
        if why is not None:
            raise ValueError("Trainer(fused=True): " + why)
        self._fused_check_memory()
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise ValueError("Trainer(fused=True) runs HIP kernels: the trainer's device is %s, not a GPU" % (dev,))

    def _fused_check_memory(self):
        mem = self.memory
        if getattr(mem, "_odd", None):
            raise ValueError("Trainer(fused=True): the memory holds %d _odd rows (states of another human count than its "
                             "tensor store), which the fused step cannot gather" % len(mem._odd))
        st = getattr(mem, "_states", None)
        if st is not None:
            from .. import _hip
            want = self._step_hip.state_shape
            got = tuple(st.shape[1:])
            if len(got) != len(want) or any(g != w if w is not None else not 1 <= g <= _hip.MAX_HUMANS
                                            for g, w in zip(got, want)):
                raise ValueError("Trainer(fused=True): memory states are %s, the model takes %s" %
                                 (got, "".join("[N <= %d]" % _hip.MAX_HUMANS if w is None else "[%d]" % w for w in want)))
            dev = torch.device(self.device)
            same = st.device.type == dev.type and (dev.type != "cuda" or st.device.index ==
                                                   (torch.cuda.current_device() if dev.index is None else dev.index))
            if not same:
                raise ValueError("Trainer(fused=True): the memory lives on %s, the trainer on %s; the fused step gathers "
                                 "its batches on the device (ReplayMemory(capacity, device=...))" % (st.device, dev))

    def _fused_run(self, batches):
        """One fused training step per entry of `batches` (1-D int64 host tensors of memory rows); returns the list of
        their float32 losses as Python floats, read back with one copy after the last step."""
        from .. import _hip
        self._fused_check()
        n = len(self.memory)
        if n < 1 or any(b.numel() < 1 for b in batches):
            raise ValueError("Trainer(fused=True): the memory holds no rows to train on")
        self.last_rows = batches
        rows = torch.cat(batches)
        bad = _fused.bad_row(rows, n)                            # the kernel trusts the rows: checked here, on the host
        if bad is not None:
            raise IndexError("Trainer(fused=True): a batch names memory row %d; the memory holds %d rows" % (bad, n))
        dev = self.memory._states.device
        params = [p for _, p in self.model.named_parameters()]
        if any(p.device != dev for p in params):
            raise ValueError("Trainer(fused=True): the model lives on %s, the memory on %s" % (params[0].device, dev))
        states, values = self.memory._states, self.memory._values
        step = self._step_hip
        N = int(states.shape[1]) if step.state_shape[0] is None else 1
        table, count = self._fused_layout()
        z = self._fz = _fused.buffers(self._fz, ("params", "grad", "mom"), params, dev)
        self._flat = z["grad"]                                   # data parallel: the flat gradient is the bucket
        ws = _fused.workspace(z, max(int(step.workspace(int(b.numel()), N)) for b in batches))
        group = self.optimizer.param_groups[0]
        lr, momentum = float(group["lr"]), float(group["momentum"])
        grouped, world = self._grouped(), self._world()
        with torch.no_grad():
            rows_dev = rows.to(dev)
            losses = torch.empty(len(batches), dtype=torch.float32, device=dev)
            stream, lib, ptr = _hip.stream_ptr(dev), _hip.lib, _hip.ptr
            at = 0
            for s, b in enumerate(batches):
                B = int(b.numel())
                _hip.check(step.launch(ptr(z["params"]), ptr(states), ptr(values), _fused.at(rows_dev, at), B, N, ptr(ws),
                                       ptr(z["grad"]), _fused.at(losses, s), stream), step.name)
                at += B
                if grouped:
                    self._collective(dist.all_reduce, z["grad"])          # one bucket, one collective
                    if world > 1:
                        z["grad"].div_(world)
                _hip.check(lib.mcn_sgd_momentum_step(ptr(z["params"]), ptr(z["mom"]), ptr(z["grad"]), count, lr, momentum,
                                                     stream), "mcn_sgd_momentum_step")
            _fused.store(z, params, table)
            return losses.cpu().tolist()

    def _fused_epoch(self, num_epochs, perms):
        n = len(self.memory)
        multi = self._world() > 1
        batches, per_epoch = [], []
        for ep in range(num_epochs):
            perm = torch.randperm(n, generator=self._gen) if perms is None else torch.as_tensor(perms[ep], dtype=torch.long)
            steps = self._agreed_steps(n)
            for b in range(steps):
                lo = b * self.batch_size
                batches.append(perm[(lo + torch.arange(self.batch_size)) % n] if multi else perm[lo:lo + self.batch_size])
            per_epoch.append(steps)
        losses = self._fused_run(batches) if batches else []
        average_epoch_loss, at = 0, 0
        for steps in per_epoch:
            epoch_loss = 0
            for v in losses[at:at + steps]:
                epoch_loss += v
            at += steps
            average_epoch_loss = epoch_loss / n
        return average_epoch_loss

    def _fused_batch(self, num_batches):
        n = len(self.memory)
        batches = [torch.randperm(n, generator=self._gen)[:min(self.batch_size, n)] for _ in range(num_batches)]
        losses = 0
        for v in (self._fused_run(batches) if batches else []):
            losses += v
        average_loss = losses / num_batches
        logging.debug("Average loss : %.2E", average_loss)
        return average_loss

    # ------------------------------------------------------------------ reference surface
    def _agreed_steps(self, n_local):
        """Mini-batches per epoch: the local count, or with several ranks the largest count of any rank."""
        steps = -(-n_local // self.batch_size)
        if self._world() > 1:
            dev = self.device if dist.get_backend() == "nccl" else torch.device("cpu")
            t = torch.tensor([steps], dtype=torch.int64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            steps = int(t.item())
        return steps

    def optimize_epoch(self, num_epochs, perms=None):
        """trainer.py:38-62: full passes over the memory in shuffled mini-batches; returns epoch_loss / len(memory).
        perms (optional, [num_epochs][n] index rows) replaces the shuffles this trainer would draw itself -- the
        reference's DataLoader draws them from torch's global generator."""
        if self.optimizer is None:
            raise ValueError("Learning rate is not set!")
        if self.fused:
            return self._fused_epoch(num_epochs, perms)
        average_epoch_loss = 0
        n = len(self.memory)
        multi = self._world() > 1
        for ep in range(num_epochs):
            epoch_loss = 0
            perm = torch.randperm(n, generator=self._gen) if perms is None else torch.as_tensor(perms[ep], dtype=torch.long)
            steps = self._agreed_steps(n)
            for b in range(steps):
                lo = b * self.batch_size
                if multi:
                    # every rank runs `steps` full batches; a rank with fewer rows wraps around its permutation
                    idx = perm[(lo + torch.arange(self.batch_size)) % n]
                else:
                    idx = perm[lo:lo + self.batch_size]
                idx = idx.to(self.memory._states.device)
                epoch_loss += self._step(self.memory._states[idx].to(self.device), self.memory._values[idx].to(self.device))
            average_epoch_loss = epoch_loss / n
        return average_epoch_loss

    def optimize_batch(self, num_batches):
        """trainer.py:64-82: num_batches independent random mini-batches; returns the mean loss."""
        if self.optimizer is None:
            raise ValueError("Learning rate is not set!")
        if self.fused:
            return self._fused_batch(num_batches)
        losses = 0
        for _ in range(num_batches):
            inputs, values = self.memory.sample(self.batch_size, self._gen)
            losses += self._step(inputs.to(self.device), values.to(self.device))
        average_loss = losses / num_batches
        logging.debug("Average loss : %.2E", average_loss)
        return average_loss
