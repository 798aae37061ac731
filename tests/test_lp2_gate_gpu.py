"""The quad ORCA solve on the batches of tests/lp2_gate_states.py: mcn_env_step (6 calls) and mcn_env_rollout (one 6-step
launch) against the C oracle's replay, bit for bit -- state, human_act and the step record.

tests/test_lp2_gate_states_cpu.py proves on the CPU what each batch holds: a whole group whose humans all keep the
clipped preferred velocity, one quad taking next to free group mates, the preferred velocity exactly on a line, a
violated line beyond nl, NaN half-planes, idle lanes next to an env 0 that takes at every step, a 3-D LP entry next to
free group mates, and for all_free a free step after and before a taking one inside the launch.  Comparisons are
bitwise (tests/helpers.py bit_mismatch): -0.0 against +0.0 fails, NaN matches NaN.  The oracle's replay is computed
once per batch (lp2_gate_states.trace) and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import lp2_gate_states as S  # noqa: E402

RECORD = ("reward", "done", "info", "dmin", "hh_count", "human_act")


def _env(family, E, N, visible):
    env = H.make_vec_env(E, N, robot_visible=visible)
    for k, v in S.orca_variant(family).items():
        setattr(env._orca, k, v)
    st, ax, ay = S.batch(family, E, N, visible)
    H.upload(env, st)
    return env, np.stack([ax, ay], -1)


def _record(env):
    return dict(reward=env.reward.cpu().numpy(), done=env.done.cpu().numpy(), info=env.info.cpu().numpy(),
                dmin=env.dmin.cpu().numpy(), hh_count=env.hh_count.cpu().numpy(), human_act=env.human_act.cpu().numpy())


def _assert_record(got, ref, what):
    for k in RECORD:
        bad = H.bit_mismatch(got[k], ref[k])
        assert len(bad) == 0, (what, k, bad[:4].tolist())


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_step_matches_oracle_bitwise(family, split, tuning):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    tuning(quad_max_envs=1 << 30, quad_split=split)
    for E, N, visible in S.SHAPES:
        tr = S.trace(family, E, N, visible)
        env, acts = _env(family, E, N, visible)
        acts_d = torch.from_numpy(acts).to(env.device)
        for t in range(S.T):
            env.step(acts_d[t])
            torch.cuda.synchronize()
            what = "%s step %d E=%d N=%d visible=%d split=%d" % (family, t, E, N, visible, split)
            _assert_record(_record(env), tr["refs"][t], what)
            H.assert_state_equal(H.download(env), tr["states"][t], what=what)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_rollout_matches_oracle_bitwise(family, split, tuning):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    tuning(rollout_fused=1, rollout_split=split)
    for E, N, visible in S.SHAPES:
        tr = S.trace(family, E, N, visible)
        env, acts = _env(family, E, N, visible)
        env.rollout(torch.from_numpy(acts).to(env.device))
        torch.cuda.synchronize()
        what = "%s %d-step launch E=%d N=%d visible=%d split=%d" % (family, S.T, E, N, visible, split)
        _assert_record(_record(env), tr["refs"][-1], what)
        H.assert_state_equal(H.download(env), tr["states"][-1], what=what)
