"""The ORCA wavefronts' sorted half-planes through an LDS table (quad_common.hpp: QuadTable; env_rollout_wg4_kernel,
rollout_split = 2).

In the four-wavefront rollout form lane l of an ORCA wavefront writes its half-plane to slot (l & ~3) | rank of a table
that belongs to its wavefront, and reads its quad's four slots and its own; the 3-D LP reads its run-time line from the
same table.  Every other kernel keeps the ds_permute + DPP path.  What can go wrong there and nowhere else:

  * rank -> slot: exact ties of the squared distance (stable order), one to four candidates out of range (their slots
    fill in lane order; the table must still hold a permutation);
  * the 3-D LP's run-time read, over one, two and three rounds;
  * a read that overtakes the write, or a write of the next step that overtakes a read: every launch length, every cut;
  * quads that straddle two wavefronts (envs 3 and 6 of a workgroup), idle quads (a lone env leaves 35), a partial last
    workgroup; a restart beside a 3-D LP in the same workgroup-step; NaN half-planes and a NaN goal.

The batch below puts each of these into envs 0 .. 18, and `_replay` proves from the C oracle on the CPU that they are
there (test_batch_holds_what_it_is_for, no GPU).  The GPU tests compare BYTES: full state, step record, Explorer records
and finished-episode arrays of the forced four-wavefront form after EVERY launch against single mcn_env_step calls at
that step, for the first T = 1, 2, 3, 8 steps of one sequence cut at every position, and forms 1 and 0 at the end.
"""
import functools
import os

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests.rollout_harness import (ROOT, every_cut, kernel_resources, launches_against, parse_resources,
                                   single_steps)

N = 5
T_MAX = 8
LENGTHS = (1, 2, 3, 8)
SHAPES = (1, 8, 9, 19)
FAR = (40.0, 40.0)
f32 = np.float32
EPS = f32(1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# the batch: env e holds scene e (mod the list)
def _packed(st, e, seed, spread):
    """every human inside a disc of radius `spread`, goals across: the quads enter the 3-D LP"""
    rng = np.random.RandomState(seed)
    ang, d = rng.uniform(0, 2 * np.pi, N), rng.uniform(0.05, spread, N)
    st.hpx[e], st.hpy[e] = d * np.cos(ang), d * np.sin(ang)
    st.hgx[e], st.hgy[e] = -6 * np.cos(ang), -6 * np.sin(ang)


def _cross(st, e):
    """human 0 in the middle of four others on the axes, 2 m away: all four squared distances are 4 exactly; each outer
    human has two neighbours at squared distance 8 exactly"""
    st.hpx[e], st.hpy[e] = (0.0, 2.0, 0.0, -2.0, 0.0), (0.0, 0.0, 2.0, 0.0, -2.0)
    st.hgx[e], st.hgy[e] = (3.0, -6.0, 0.0, 6.0, 0.0), (0.5, 0.0, -6.0, 0.0, 6.0)


def _far(st, e, k):
    """k of human 0's four candidates stand more than neighbor_dist (10 m) away, the others 1.5 m from it"""
    ring = [(1.5, 0.0), (0.0, 1.5), (-1.5, 0.0), (0.0, -1.5)]
    away = [(12.0, 0.0), (0.0, 12.0), (-12.0, 0.0), (0.0, -12.0)]
    # the far ones take the FIRST candidate lanes for odd k and the last for even k: lane order and rank differ
    far_idx = set(range(k)) if k % 2 else set(range(4 - k, 4))
    st.hpx[e, 0], st.hpy[e, 0] = 0.0, 0.0
    st.hgx[e, 0], st.hgy[e, 0] = 4.0, 1.0
    for c in range(4):
        x, y = away[c] if c in far_idx else ring[c]
        st.hpx[e, c + 1], st.hpy[e, c + 1] = x, y
        st.hgx[e, c + 1], st.hgy[e, c + 1] = -x, -y + 0.25


def _coincident(st, e):
    """humans 0 and 1 coincide, with equal velocities and goals: their mutual half-plane is 0 / 0 at every step"""
    _cross(st, e)
    for k in ("hpx", "hpy", "hvx", "hvy", "hgx", "hgy"):
        getattr(st, k)[e, 1] = getattr(st, k)[e, 0]


def _nan_goal(st, e):
    _packed(st, e, 5, 0.9)
    st.hgx[e, 2] = np.nan


# seeds / spreads of the packed scenes were chosen for what `_replay` then proves: 3-D LPs of one, two and three rounds
_SCENES = (
    lambda st, e: _packed(st, e, 11, 0.30),          # env 0: the lone env of E = 1
    _cross,
    lambda st, e: _far(st, e, 1),
    lambda st, e: _far(st, e, 2),                    # env 3 straddles ORCA wavefronts 0 and 1
    lambda st, e: _far(st, e, 3),
    lambda st, e: _far(st, e, 4),
    lambda st, e: _packed(st, e, 12, 0.30),          # env 6 straddles ORCA wavefronts 1 and 2
    _coincident,
    lambda st, e: _packed(st, e, 13, 0.30),          # env 8: the partial workgroup of E = 9
    _nan_goal,
    lambda st, e: _packed(st, e, 14, 0.45),
    lambda st, e: _packed(st, e, 15, 0.45),
    lambda st, e: _packed(st, e, 16, 0.45),
    lambda st, e: _packed(st, e, 17, 0.30),
    lambda st, e: _packed(st, e, 18, 0.30),
    lambda st, e: _packed(st, e, 19, 0.45),
    lambda st, e: _packed(st, e, 20, 0.30),
    lambda st, e: _packed(st, e, 21, 0.45),
    lambda st, e: _packed(st, e, 22, 0.30),
)


@functools.lru_cache(maxsize=None)
def _batch(E):
    st = cport.EnvState(E, N)
    st.hr[:] = 0.3; st.hvpref[:] = 1.0; st.rr[:] = 0.3
    for e in range(E):
        _SCENES[e % len(_SCENES)](st, e)
    st.rpx[:], st.rpy[:] = FAR
    st.rgx[:], st.rgy[:] = FAR[0], FAR[1] + 25.0
    rng = np.random.RandomState(100 + E)
    acts = rng.randint(-8, 9, (T_MAX, E, 2)) / 16.0
    return st, acts


def batch(E):
    st, acts = _batch(E)
    return st.copy(), acts.copy()


# ---------------------------------------------------------------------------------------------------------------------
# what the oracle says about the batch.  The oracle counts 3-D LP entries but not rounds, so the 2-D / 3-D LP is restated
# here in float32, operation by operation (RVO2's linearProgram1-3 as orca_device.hpp writes them), over the ORACLE's own
# sorted lines; the restatement is only believed where its velocity is the oracle's, bit for bit.
def _det(ax, ay, bx, by):
    return ax * by - ay * bx


def _dot(ax, ay, bx, by):
    return ax * bx + ay * by


def _lp1(L, no, radius, optx, opty, dir_opt):
    px, py, dx, dy = L[no]
    dp = _dot(px, py, dx, dy)
    disc = dp * dp + radius * radius - _dot(px, py, px, py)
    if disc < 0:
        return None
    sq = np.sqrt(disc)
    tl, tr = -dp - sq, -dp + sq
    for i in range(no):
        qx, qy, ex, ey = L[i]
        den = _det(dx, dy, ex, ey)
        num = _det(ex, ey, px - qx, py - qy)
        if np.abs(den) <= EPS:
            if num < 0:
                return None
            continue
        t = num / den
        if den >= 0:
            tr = np.fmin(tr, t)
        else:
            tl = np.fmax(tl, t)
        if tl > tr:
            return None
    if dir_opt:
        t = tr if _dot(optx, opty, dx, dy) > 0 else tl
    else:
        t = _dot(dx, dy, optx - px, opty - py)
        if t < tl:
            t = tl
        elif t > tr:
            t = tr
    return px + t * dx, py + t * dy


def _lp2(L, radius, optx, opty, dir_opt):
    if dir_opt:
        rx, ry = radius * optx, radius * opty
    elif _dot(optx, opty, optx, opty) > radius * radius:
        inv = f32(1) / np.sqrt(_dot(optx, opty, optx, opty))
        rx, ry = radius * (optx * inv), radius * (opty * inv)
    else:
        rx, ry = optx, opty
    for i in range(len(L)):
        px, py, dx, dy = L[i]
        if _det(dx, dy, px - rx, py - ry) > 0:
            got = _lp1(L, i, radius, optx, opty, dir_opt)
            if got is None:
                return i, rx, ry
            rx, ry = got
    return len(L), rx, ry


def _lp3(L, begin, radius, rx, ry):
    """-> (rx, ry, rounds): a round is a line the running result violates by more than `dist`"""
    dist, rounds = f32(0), 0
    for i in range(begin, len(L)):
        px, py, dx, dy = L[i]
        if _det(dx, dy, px - rx, py - ry) > dist:
            rounds += 1
            P = []
            for j in range(i):
                qx, qy, ex, ey = L[j]
                dt = _det(dx, dy, ex, ey)
                if np.abs(dt) <= EPS:
                    if _dot(dx, dy, ex, ey) > 0:
                        continue
                    sx, sy = f32(0.5) * (px + qx), f32(0.5) * (py + qy)
                else:
                    s = _det(ex, ey, px - qx, py - qy) / dt
                    sx, sy = px + s * dx, py + s * dy
                ddx, ddy = ex - dx, ey - dy
                inv = f32(1) / np.sqrt(_dot(ddx, ddy, ddx, ddy))
                P.append((sx, sy, ddx * inv, ddy * inv))
            fail, nx, ny = _lp2(P, radius, -dy, dx, True)
            if fail == len(P):
                rx, ry = nx, ny
            dist = _det(dx, dy, px - rx, py - ry)
    return rx, ry, rounds


def solve_rounds(lines, ms, prefx, prefy):
    """(vx, vy, 3-D LP rounds; 0 when the 2-D LP succeeds) of one human, float32 throughout"""
    with np.errstate(all="ignore"):
        L = [tuple(f32(v) for v in l) for l in lines]
        fail, rx, ry = _lp2(L, f32(ms), f32(prefx), f32(prefy), False)
        if fail == len(L):
            return rx, ry, 0
        return _lp3(L, fail, f32(ms), rx, ry)


def _same_f32(a, b):
    a, b = f32(a), f32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))


@functools.lru_cache(maxsize=None)
def _replay(E):
    """T_MAX oracle steps of the batch.  Returns dict: rounds [T, E, N] (3-D LP rounds of each solve, from the restatement
    checked against the oracle's velocity), n_out [T, E, N] (candidates not inside neighbor_dist, float32 as the kernels
    rank them), ties / nonfinite / nonfinite_lp3 [T] (the oracle's own edge counters), nan_vel (a NaN velocity came out),
    states (EnvState after each step), refs (cport.env_step's outputs)."""
    from tests import lp2_gate_states as LG
    st, acts = batch(E)
    cfg = cport.default_cfg(robot_visible=0)
    range_sq = f32(cfg.orca_neighbor_dist) * f32(cfg.orca_neighbor_dist)
    out = dict(rounds=np.zeros((T_MAX, E, N), int), n_out=np.zeros((T_MAX, E, N), int), ties=np.zeros(T_MAX, int),
               nonfinite=np.zeros(T_MAX, int), nonfinite_lp3=np.zeros(T_MAX, int), nan_vel=False, states=[], refs=[])
    for t in range(T_MAX):
        before = st.copy()
        cport.edge_counts(reset=True)
        ref = cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        ec = cport.edge_counts(reset=True)
        out["ties"][t], out["nonfinite"][t], out["nonfinite_lp3"][t] = ec["dist_tie"], ec["nonfinite_line"], ec["nonfinite_line_in_lp3"]
        out["nan_vel"] |= bool(np.isnan(ref["human_act"]).any())
        with np.errstate(all="ignore"):
            px, py = before.hpx.astype(f32), before.hpy.astype(f32)
            for e in range(E):
                for i in range(N):
                    dx, dy = px[e, i] - np.delete(px[e], i), py[e, i] - np.delete(py[e], i)
                    out["n_out"][t, e, i] = int((~(dx * dx + dy * dy < range_sq)).sum())
                    lines = LG.human_lines(cfg, before, e, i)
                    pref = (f32(before.hgx[e, i] - before.hpx[e, i]), f32(before.hgy[e, i] - before.hpy[e, i]))
                    vx, vy, r = solve_rounds(lines, before.hvpref[e, i], pref[0], pref[1])
                    assert _same_f32(vx, ref["human_act"][e, i, 0]) and _same_f32(vy, ref["human_act"][e, i, 1]), \
                        "the restated LP leaves the oracle at step %d env %d human %d" % (t, e, i)
                    out["rounds"][t, e, i] = r
        out["states"].append(st.copy())
        out["refs"].append(ref)
    return out


@pytest.mark.parametrize("E", SHAPES)
def test_batch_holds_what_it_is_for(E):
    """No GPU: the oracle's replay of the batch shows every situation the GPU tests are about, inside the first steps."""
    rp = _replay(E)
    rounds = rp["rounds"]
    assert (rounds[0] >= 1).any(), "no 3-D LP on the first step (T = 1 launches)"
    if E >= 8:
        assert rp["ties"][0] > 0, "no exact tie of squared distances"
        for k in (1, 2, 3, 4):
            assert (rp["n_out"][0, :, 0] == k).any(), "no human with %d candidates out of range" % k
        assert rp["nonfinite"].min() > 0, "no NaN half-plane at every step"
        # envs 3 and 6 of a workgroup straddle two ORCA wavefronts: both solve over a table split between them
        assert (rp["n_out"][0, 3] > 0).any() and (rounds[:, 6] >= 1).any()
    if E >= 9:
        assert (rounds[:, 8:] >= 1).any(), "no 3-D LP in the partial last workgroup"
    if E >= 19:
        for k in (1, 2, 3):
            assert (rounds == k).any(), "no 3-D LP of %d round(s): %s" % (k, np.bincount(rounds.ravel()))
        assert rp["nan_vel"], "the NaN goal produced no NaN velocity"
        # two and three rounds inside the first three steps too, where every launch length sees them
        assert (rounds[:3] >= 2).any()


# ---------------------------------------------------------------------------------------------------------------------
def _all_lengths(build, acts, snaps, what):
    for T in LENGTHS:
        for cuts in every_cut(T):
            launches_against(build, acts, 2, cuts, snaps, what)
        for split in (1, 0):
            launches_against(build, acts, split, (0, T), snaps, what)


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("E", SHAPES)
def test_line_table_equals_single_steps(E, kinematics, tuning):
    """The first 1, 2, 3 and 8 steps of one sequence, cut at every position: the four-wavefront form leaves the bytes of
    the single steps after every launch, forms 1 and 0 at the end; the single steps are the oracle's (whose replay holds
    the ties, out-of-range candidates, 3-D LP rounds and NaNs: test_batch_holds_what_it_is_for)."""
    tuning(rollout_fused=1)
    st, acts = batch(E)

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        H.upload(env, st)
        env.attach_rollout(gamma=0.9, pool=None, fin_slots=2)
        return env
    env, snaps, _, _ = single_steps(build, acts)
    if kinematics == "holonomic":                              # (the replay's robot is holonomic; the humans never see it)
        H.assert_state_equal(H.download(env), _replay(E)["states"][-1], what="single steps against the oracle, E=%d" % E)
    else:
        want = _replay(E)["states"][-1]
        got = H.download(env)
        H.assert_state_equal(got, want, fields=cport.EnvState.FIELDS_H, what="humans against the oracle, E=%d" % E)
    _all_lengths(build, acts, snaps, "line table %s E=%d" % (kinematics, E))


# ---------------------------------------------------------------------------------------------------------------------
# a restart beside a 3-D LP: the same batch on staggered clocks (0.5 s + 0.25 s x (e mod 3)) with time_limit 2, so env e times
# out at 1 s -- and restarts from the pool -- at step 2 - (e mod 3), while its workgroup mates solve on
_P = 8


def _lp3_entries(cfg, snap, e):
    """3-D LP entries of env e's humans in the step that starts from `snap` (the oracle on the device's own bytes)"""
    o = cport.EnvState(1, N)
    hp, hv, hg = snap["hpos"][e], snap["hvel"][e], snap["hgoal"][e]
    o.hpx[0], o.hpy[0], o.hvx[0], o.hvy[0] = hp[:, 0], hp[:, 1], hv[:, 0], hv[:, 1]
    o.hgx[0], o.hgy[0], o.hr[0], o.hvpref[0] = hg[:, 0], hg[:, 1], snap["hrad"][e], snap["hvpref"][e]
    o.rpx[0], o.rpy[0] = snap["rpos"][e]
    o.rgx[0], o.rgy[0] = snap["rgoal"][e]
    o.rr[0] = 0.3
    cport.lp3_entries(reset=True)
    cport.env_step(cfg, o, np.zeros(1), np.zeros(1), update=False)
    return cport.lp3_entries(reset=True)


@pytest.mark.gpu
@pytest.mark.parametrize("E,kinematics", [(8, "holonomic"), (9, "holonomic"), (19, "holonomic"), (9, "unicycle")])
def test_restart_beside_a_3d_lp(E, kinematics, tuning):
    """From the single-step run and the oracle on its states: at some step an env of a workgroup restarts from the pool
    while another env of the same workgroup is in the 3-D LP.  Then every length and cut as above."""
    from modelcrowdnav_amd.envs import scenarios as S
    tuning(rollout_fused=1)
    st, acts = batch(E)
    st.gtime[:] = 0.5 + 0.25 * (np.arange(E) % 3)

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics, **{"env.time_limit": 2})
        H.upload(env, st)
        pool = S.scenario_pool(env.spec(), "test", range(_P), N, "circle_crossing")
        env.attach_rollout(gamma=0.9, pool=pool, case_stride=1, first_cases=(np.arange(E) + 1) % _P, fin_slots=2)
        return env
    env, snaps, first, done = single_steps(build, acts)
    cfg = H.oracle_cfg_for(env)
    beside = False
    for t in range(3):
        before = first if t == 0 else snaps[t - 1]
        lp3 = np.array([_lp3_entries(cfg, before, e) > 0 for e in range(E)])
        for w in range(0, E, 8):
            d, l = done[t, w:w + 8], lp3[w:w + 8]
            beside |= any(d[a] and l[b] for a in range(len(d)) for b in range(len(d)) if a != b)
    assert done[:3].any() and not done[:3].all(1).any(), "the restarts are not staggered: %s" % done[:3]
    assert beside, "no restart beside a 3-D LP in one workgroup-step"
    _all_lengths(build, acts, snaps, "restart beside 3-D LP %s E=%d" % (kinematics, E))


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: what the table costs, and that nobody else pays
WG4_LDS = 2560 + 3 * 64 * 16        # the hand-off arrays + three wavefronts' tables of 64 float4 slots


def test_line_table_kernel_resources():
    """Read from the built code objects: both env_rollout_wg4_kernel instantiations run without scratch in no more VGPRs
    than before the table (124 holonomic / 147 unicycle), their LDS is 5 632 B per workgroup, and every other kernel of
    the library has the registers, scratch and LDS recorded in profiles/r17_kernel_resources.txt -- but for three
    non-ORCA kernels whose overlap pre-filter stopped reading cfg.orca_safety_space since: their rows are those of
    profiles/r21_kernel_resources.txt (2 VGPRs either way, the same occupancy, no scratch or LDS change)."""
    now = kernel_resources()
    txt = open(os.path.join(ROOT, "profiles", "r17_kernel_resources.txt")).read()
    then = parse_resources(txt[txt.index("# after, every kernel:"):])
    txt = open(os.path.join(ROOT, "profiles", "r21_kernel_resources.txt")).read()
    since = parse_resources(txt[txt.index("# after, the kernels that changed"):])
    assert len(since) == 3 and set(since) <= set(then) and not any("wg4" in k for k in since)
    for name, row in since.items():                   # same occupancy class (VGPRs come in blocks of 8), nothing else moved
        assert (row[0] + 7) // 8 == (then[name][0] + 7) // 8 and row[1:] == then[name][1:], (name, row, then[name])
    then.update(since)
    assert len(then) > 150 and sorted(now) == sorted(then), sorted(set(now) ^ set(then))
    for name in sorted(then):
        vgpr, agpr, sgpr, scratch, lds, vspill = now[name]
        if "env_rollout_wg4_kernel<" in name:
            print("%s: vgpr %d sgpr %d scratch %d lds %d" % (name, vgpr, sgpr, scratch, lds))
            assert (scratch, vspill, agpr) == (0, 0, 0), (name, now[name])
            assert vgpr <= then[name][0] and then[name][0] == (147 if "true" in name else 124), (name, now[name])
            assert lds == WG4_LDS and then[name][4] == 2560, (name, now[name])
        else:
            assert now[name] == then[name], (name, now[name], then[name])
