"""The quad kernels' 3-D LP round and step top after the lean rewrite (quad_common.hpp, env_rollout_quad.hip).

GPU: packed crowds (every pair of humans overlaps) send most humans into the 3-D LP, where four colliding lines make
several rounds the common case instead of the rare one: a T-step rollout launch must equal T single steps, and (without
pool restarts) the oracle's trajectory, bit for bit.
CPU (needs hipcc): the static budgets of the flagship instantiation (tools/isa_census.py) and the register / scratch
budgets of every 4- and 5-human quad kernel (tools/kernel_resources.py).
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests.rollout_harness import ROOT, assert_same_bytes, kernel_resources, need_gpu, pool_env, snapshot

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _packed_rollout_env(E, N, visible, with_pool, seed):
    env = pool_env(E, N, visible, with_pool)
    st = H.download(env)
    # every env's humans inside a disc of radius 0.45 around one point (as the LP3-queue test packs them)
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(-3, 3, (E, 1)), rng.uniform(-3, 3, (E, 1))
    ang, d = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.0, 0.45, (E, N))
    st.hpx[:], st.hpy[:] = cx + d * np.cos(ang), cy + d * np.sin(ang)
    H.upload(env, st)
    return env, st


@pytest.mark.gpu
@pytest.mark.parametrize("N,visible", [(5, False), (4, True)])
@pytest.mark.parametrize("with_pool", [True, False])
@pytest.mark.parametrize("split", [0, 1])
def test_packed_crowd_rollout_equals_single_steps_and_oracle(N, visible, with_pool, split, tuning):
    torch = need_gpu()
    E, T = 777, 40
    rng = np.random.RandomState(50 + N)
    sp, aa = rng.uniform(0, 1, (T, E)), rng.uniform(0, 2 * np.pi, (T, E))
    ax, ay = sp * np.cos(aa), sp * np.sin(aa)
    tuning(rollout_fused=1)
    tuning(rollout_split=split)
    a, st = _packed_rollout_env(E, N, visible, with_pool, seed=7 + N)
    b, _ = _packed_rollout_env(E, N, visible, with_pool, seed=7 + N)
    acts_d = torch.from_numpy(np.stack([ax, ay], -1)).to(a.device)
    a.rollout(acts_d[:13]); a.rollout(acts_d[13:])
    for t in range(T):
        b.step(acts_d[t])
    torch.cuda.synchronize()
    assert_same_bytes(snapshot(a), snapshot(b))
    if with_pool:
        return
    # no restarts: the oracle steps the same trajectory; the packed start drives it through the 3-D LP
    cfg = H.oracle_cfg_for(a)
    cport.lp3_entries(reset=True)
    for t in range(T):
        ref = cport.env_step(cfg, st, ax[t].copy(), ay[t].copy(), update=True)
        if t == 0:
            assert cport.lp3_entries(reset=False) > E * N // 4, "packed crowds should send most humans into the 3-D LP"
    H.assert_state_equal(H.download(a), st, what="packed crowd, %d-step launch" % T)
    assert np.array_equal(a.reward.cpu().numpy(), ref["reward"]) and np.array_equal(a.done.cpu().numpy(), ref["done"])
    assert np.array_equal(a.human_act.cpu().numpy(), ref["human_act"])


def _need_hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")


def test_flagship_step_loop_instruction_budget():
    """Static instruction counts of the flagship instantiation's step loop, fast path (out-of-line IEEE fall-backs
    excluded): the common path (step top to the 3-D LP entry) and one 3-D LP round."""
    _need_hipcc()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_census.py")], capture_output=True, text=True,
                         check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(common|lp3 round)\s+(\d+)\s+.*\s(\d+)$", line)
        if m:
            rows[m.group(1)] = int(m.group(2)) - int(m.group(3))
    assert set(rows) == {"common", "lp3 round"}, out
    assert rows["common"] <= 440, rows
    assert rows["lp3 round"] <= 270, rows


def test_quad_kernels_registers_and_scratch():
    """Every 4- / 5-human instantiation of both quad kernels fits the 168-VGPR cap of __launch_bounds__(128, 3)
    without scratch (read from the built library's code objects)."""
    _need_hipcc()
    csrc = os.path.join(ROOT, "modelcrowdnav_amd", "csrc")
    if not os.path.exists(os.path.join(csrc, "env_rollout_quad.o")):
        pytest.skip("needs the built library (build())")
    out = kernel_resources("quad_kernel<")
    seen = 0
    for name, (vgpr, _, _, scratch, _, _) in out.items():
        m = re.search(r"(env_rollout_quad_kernel|env_step_quad_kernel)<(\d+),", name)
        if not m or int(m.group(2)) not in (4, 5):
            continue
        seen += 1
        assert vgpr <= 168, (name, vgpr)
        assert scratch == 0, (name, scratch)
    assert seen == 12 + 6, out
