"""Child process of tests/test_fused_value_trainers_gpu.py: Trainer(fused=True) on cuda:0 without a process group, then -- from
the same weights and the same draws -- inside a process group of ONE rank, where every step runs the all-reduce of the
flat gradient between mcn_sarl_loss_grad and mcn_sgd_momentum_step.  Started as a fresh
`python -m tests.fused_dp_worker <port> <backend> <out.pt>` process; both results go into <out.pt>."""
import copy
import os
import sys


def main():
    port, backend, out = sys.argv[1:4]
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from modelcrowdnav_amd import dist as mdist
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    from tests import value_trainer_ref as R
    dev = torch.device("cuda", 0)
    model0 = R.value_network("sarl", 4)
    states, values = R.states_and_values("sarl", 77, 5, seed=31)

    def run():
        model = copy.deepcopy(model0).to(dev)
        mem = ReplayMemory(100, device=dev)
        mem.push_batch(states.to(dev), values.reshape(-1).to(dev))
        tr = Trainer(model, mem, dev, 32, fused=True)
        tr._gen.manual_seed(13)
        tr.sync_weights()
        tr.set_learning_rate(0.01)
        losses = [tr.optimize_batch(2), tr.optimize_epoch(1)]           # the epoch: 32 + 32 + 13 rows
        return tr, losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    assert not Trainer._grouped()
    _, losses_alone, alone = run()
    mdist.init_from_env(backend, force=True)
    assert Trainer._grouped() and dist.get_world_size() == 1
    tr, losses_grouped, grouped = run()
    torch.save({"start": {k: v.detach().clone() for k, v in model0.state_dict().items()}, "alone": alone, "grouped": grouped,
                "losses_alone": losses_alone, "losses_grouped": losses_grouped, "backend": dist.get_backend(),
                "world": dist.get_world_size(), "bucket_is_grad": tr._flat is tr._fz["grad"] and tr._flat.is_cuda}, out)
    dist.barrier()
    torch.cuda.synchronize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
