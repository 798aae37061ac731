"""Edge-case env batches for the ORCA kernels: dyadic states on which float32 arithmetic is exact, so that exact ties,
exact zeros and non-finite half-planes actually happen (random float states almost never produce them).

  positions on a 1/8 grid, velocities on a 1/16 grid, human and robot radius 0.3025 ((float)(0.3025 + 0.01) = 0.3125,
  and 0.375 with safety_space 0.0625), dyadic v_pref and robot actions.

Every batch is a concatenation of blocks (see edge_batch); the oracle's edge counters (cport.edge_counts) show which
branches a batch reaches, and tests/test_oracle_edges.py asserts that each counter is reached in both human-count
families, so the coverage cannot rot unnoticed.
"""
import functools

import numpy as np

from oracle import cport

HR = 0.3025                      # (float)(HR + 0.01 + safety_space) is dyadic for safety_space 0 and 0.0625
VPREF = (0.5, 0.75, 1.0, 1.25)
# non-default ORCA parameters (orca.py:60-66 are neighbor_dist 10, max_neighbors 10, safety_space 0): the kernels read
# them from env._orca, the oracle from its config.  max_neighbors 2 / 3 exist for the lane-per-human kernels only (the
# quad kernels need at least 4 line slots and the dispatcher does not route such configs to them).
ORCA_VARIANTS = ({}, {"max_neighbors": 2}, {"max_neighbors": 3}, {"neighbor_dist": 1.5}, {"safety_space": 0.0625})
SHIFTS = (0.0, 2.0 ** 10, 2.0 ** 20)     # translated copies: at 2^20 float32 keeps only the 1/8 grid
BLOCK = 16
PAD = 5                          # 13 blocks x 16 x 3 copies + 5 = 629 envs: ragged for every envs-per-wavefront tiling
# ring of 12 lattice offsets with |p|^2 == 25 (equal-distance neighbours)
_RING = np.array([(5, 0), (4, 3), (3, 4), (0, 5), (-3, 4), (-4, 3), (-5, 0), (-4, -3), (-3, -4), (0, -5), (3, -4),
                  (4, -3)], np.float64)
_AXES = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float64)


def orca_cfg(variant):
    o = dict(neighbor_dist=10.0, max_neighbors=10, safety_space=0.0)
    o.update(variant)
    return o


def _grid(rng, lo, hi, shape, step):
    return rng.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape) * step


def _random(rng, E, N, spread=4.0):
    """Dyadic mid-episode states: humans anywhere in the square, the robot among them."""
    st = cport.EnvState(E, N)
    st.hpx[:] = _grid(rng, -spread, spread, (E, N), 1 / 8); st.hpy[:] = _grid(rng, -spread, spread, (E, N), 1 / 8)
    st.hvx[:] = _grid(rng, -1, 1, (E, N), 1 / 16); st.hvy[:] = _grid(rng, -1, 1, (E, N), 1 / 16)
    st.hgx[:] = _grid(rng, -5, 5, (E, N), 1 / 8); st.hgy[:] = _grid(rng, -5, 5, (E, N), 1 / 8)
    st.hr[:] = HR; st.hvpref[:] = rng.choice(VPREF, (E, N))
    st.rpx[:] = _grid(rng, -spread, spread, E, 1 / 8); st.rpy[:] = _grid(rng, -spread, spread, E, 1 / 8)
    st.rvx[:] = _grid(rng, -1, 1, E, 1 / 16); st.rvy[:] = _grid(rng, -1, 1, E, 1 / 16)
    st.rgx[:] = _grid(rng, -5, 5, E, 1 / 8); st.rgy[:] = _grid(rng, -5, 5, E, 1 / 8)
    st.rr[:] = HR
    st.gtime[:] = rng.choice([0.0, 2.5, 10.25, 23.75, 24.0], E, p=[0.5, 0.2, 0.2, 0.05, 0.05])
    return st


def _actions(rng, E):
    return _grid(rng, -1, 1, E, 1 / 16), _grid(rng, -1, 1, E, 1 / 16)


def _lattice(rng, E, N, spacing):
    """Humans on a square lattice (random origin and cell per env) with random dyadic velocities and lattice goals."""
    st = _random(rng, E, N)
    side = int(np.ceil(np.sqrt(N))) + 1
    for e in range(E):
        cells = rng.choice(side * side, N, replace=False)
        ox, oy = _grid(rng, -2, 2, 2, 1 / 8)
        st.hpx[e] = ox + (cells % side) * spacing; st.hpy[e] = oy + (cells // side) * spacing
        st.rpx[e] = ox + rng.randint(-1, side + 1) * spacing; st.rpy[e] = oy + rng.randint(-1, side + 1) * spacing
    return st


def _blocks(rng, N, visible, variant):
    """The blocks of one (N, ORCA variant) batch, each [BLOCK] envs: (name, EnvState, ax, ay)."""
    nd = orca_cfg(variant)["neighbor_dist"]
    out = []

    def add(name, st, ax=None, ay=None):
        if ax is None:
            ax, ay = _actions(rng, BLOCK)
        out.append((name, st, ax, ay))

    add("lattice", _lattice(rng, BLOCK, N, 0.75))
    # packed lattice (spacing below the radius sum 0.625: overlapping discs, the 3-D LP) with a coincident pair of
    # equal velocity (0/0: a NaN half-plane inside the 3-D LP); with one human the robot is its coincident partner
    st = _lattice(rng, BLOCK, N, 0.5)
    if N >= 2:
        st.hpx[:, 1], st.hpy[:, 1], st.hvx[:, 1], st.hvy[:, 1] = st.hpx[:, 0], st.hpy[:, 0], st.hvx[:, 0], st.hvy[:, 0]
    else:
        st.rpx[:], st.rpy[:], st.rvx[:], st.rvy[:] = st.hpx[:, 0], st.hpy[:, 0], st.hvx[:, 0], st.hvy[:, 0]
    add("packed-coincident", st)
    # a neighbour at exactly neighbor_dist (strict <: left out), the others near
    st = _random(rng, BLOCK, N, spread=1.0)
    offs = [a * nd for a in _AXES] + ([np.array(p) * 2 for p in _RING[[1, 2, 4, 5, 7, 8, 10, 11]]] if nd == 10 else [])
    for e in range(BLOCK):
        off = offs[rng.randint(len(offs))]
        if N >= 2:
            st.hpx[e, 1], st.hpy[e, 1] = st.hpx[e, 0] + off[0], st.hpy[e, 0] + off[1]
        else:
            st.rpx[e], st.rpy[e] = st.hpx[e, 0] + off[0], st.hpy[e, 0] + off[1]
    add("at-neighbor-dist", st)
    # equal-distance neighbours: human 0 in the middle of a ring, the others (and the robot) on it
    st = _random(rng, BLOCK, N, spread=2.0)
    for e in range(BLOCK):
        s = rng.choice([1 / 8, 1 / 4, 1 / 2, 3 / 8])
        pts = _RING[rng.choice(len(_RING), len(_RING), replace=False)] * s
        st.hpx[e, 1:] = st.hpx[e, 0] + pts[:N - 1, 0]; st.hpy[e, 1:] = st.hpy[e, 0] + pts[:N - 1, 1]
        st.rpx[e], st.rpy[e] = st.hpx[e, 0] + pts[N - 1, 0], st.hpy[e, 0] + pts[N - 1, 1]
    add("equal-distance", st)
    # the degenerate blocks of tests/test_env_step_gpu.py::test_degenerate_configurations_match_oracle, dyadic
    st = _random(rng, BLOCK, N); st.hgx[:], st.hgy[:] = st.hpx, st.hpy
    add("on-goal", st)
    st = _random(rng, BLOCK, N); st.hvx[:] = 0; st.hvy[:] = 0; st.rvx[:] = 0; st.rvy[:] = 0
    add("at-rest", st)
    st = _random(rng, BLOCK, N)
    if N >= 2:
        st.hpx[:, 1], st.hpy[:, 1] = st.hpx[:, 0] + 0.125, st.hpy[:, 0]
    add("overlapping", st)
    st = _random(rng, BLOCK, N)
    if N >= 3:
        st.hpx[:, 2], st.hpy[:, 2], st.hvx[:, 2], st.hvy[:, 2] = st.hpx[:, N - 1], st.hpy[:, N - 1], st.hvx[:, N - 1], st.hvy[:, N - 1]
    add("coincident", st)
    st = _random(rng, BLOCK, N); st.rgx[:], st.rgy[:] = st.rpx, st.rpy
    add("robot-on-goal", st)
    st = _random(rng, BLOCK, N); st.rpx[:], st.rpy[:] = st.hpx[:, N - 1], st.hpy[:, N - 1]
    add("robot-inside-human", st)
    st = _random(rng, BLOCK, N, spread=30.0)
    add("far-apart", st)
    st = _random(rng, BLOCK, N); st.hvx[:, 0] = 0; st.hvy[:, 0] = 0
    add("zero-action", st, np.zeros(BLOCK), np.zeros(BLOCK))
    # searched: packed random crowds in which a projected line of the 3-D LP is tangent to the speed disc
    add("searched-lp3-tangent", *_search_lp3_tangent(N, visible, variant))
    return out


def _search_lp3_tangent(N, visible, variant):
    """Up to 4 envs whose ORCA solves hit disc_zero_lp3, found by a seeded search over packed dyadic crowds (about 1 env
    in 5000 qualifies; none can with fewer than two candidate neighbours); the rest of the block is packed crowds."""
    rng = np.random.RandomState(1000 + 17 * N + 7 * visible + 3 * ORCA_VARIANTS.index(variant))
    cfg = _oracle_cfg(1 if visible else 0, variant)
    found = []
    for _ in range(4 if N - 1 + visible >= 2 else 0):
        st = _random(rng, 4096, N, spread=0.625)
        ax, ay = _actions(rng, 4096)
        cand = [(0, 4096)]
        while cand and len(found) < 4:      # bisect the batch down to the envs that move the counter
            lo, hi = cand.pop()
            sub = _take(st, np.arange(lo, hi))
            cport.edge_counts(reset=True)
            cport.env_step(cfg, sub, ax[lo:hi], ay[lo:hi], update=False)
            if cport.edge_counts(reset=True)["disc_zero_lp3"] == 0:
                continue
            if hi - lo == 1:
                found.append((st, lo, ax[lo], ay[lo]))
            else:
                mid = (lo + hi) // 2
                cand += [(mid, hi), (lo, mid)]
        if len(found) >= 4:
            break
    fill = _random(rng, BLOCK, N, spread=0.625)
    fax, fay = _actions(rng, BLOCK)
    for i, (st, e, a, b) in enumerate(found):
        _put(fill, i, st, e)
        fax[i], fay[i] = a, b
    return fill, fax, fay


def _fields():
    return cport.EnvState.FIELDS_H + cport.EnvState.FIELDS_R + ("gtime", "rtheta", "human_times")


def _take(st, idx):
    o = cport.EnvState(len(idx), st.N)
    for k in _fields():
        setattr(o, k, np.ascontiguousarray(getattr(st, k)[idx]))
    return o


def _put(dst, i, src, j):
    for k in _fields():
        getattr(dst, k)[i] = getattr(src, k)[j]


def _concat(sts):
    o = cport.EnvState(sum(s.E for s in sts), sts[0].N)
    for k in _fields():
        setattr(o, k, np.ascontiguousarray(np.concatenate([getattr(s, k) for s in sts], 0)))
    return o


def _oracle_cfg(robot_visible, variant, **kw):
    o = orca_cfg(variant)
    return cport.default_cfg(robot_visible=robot_visible, orca_neighbor_dist=o["neighbor_dist"],
                             orca_max_neighbors=o["max_neighbors"], orca_safety_space=o["safety_space"], **kw)


@functools.lru_cache(maxsize=None)
def _edge_batch(N, visible, vidx, seed):
    return _build_batch(N, visible, ORCA_VARIANTS[vidx], seed)


def edge_batch(N, visible, variant=None, seed=0):
    """One batch of N-human envs for the given ORCA variant: every block, then the same blocks translated by 2^10 and
    2^20, then PAD random envs (ragged E).  Returns (EnvState, ax, ay, names) with names[e] the block of env e.
    Built once per process; the caller gets its own copy."""
    st, ax, ay, names = _edge_batch(N, bool(visible), ORCA_VARIANTS.index(variant or {}), seed)
    return st.copy(), ax.copy(), ay.copy(), list(names)


def _build_batch(N, visible, variant, seed):
    rng = np.random.RandomState(seed * 7919 + 31 * N + 11 * visible + 5 * ORCA_VARIANTS.index(variant))
    blocks = _blocks(rng, N, bool(visible), variant)
    base = _concat([b[1] for b in blocks])
    ax = np.concatenate([b[2] for b in blocks]); ay = np.concatenate([b[3] for b in blocks])
    names = [b[0] for b in blocks for _ in range(b[1].E)]
    parts, axs, ays, nms = [], [], [], []
    for s in SHIFTS:
        c = _concat([base])
        for k in ("hpx", "hpy", "hgx", "hgy", "rpx", "rpy", "rgx", "rgy"):
            getattr(c, k)[:] += s
        parts.append(c); axs.append(ax); ays.append(ay); nms += ["%s@%g" % (n, s) if s else n for n in names]
    pad = _random(rng, PAD, N)
    pax, pay = _actions(rng, PAD)
    st = _concat(parts + [pad])
    return st, np.concatenate(axs + [pax]), np.concatenate(ays + [pay]), nms + ["pad"] * PAD


# The ORCA variants a 5-human, invisible-robot quad path can run (max_neighbors >= 4): what the four-wavefront rollout
# form is built for.
WG4_VARIANTS = tuple(v for v in ORCA_VARIANTS if orca_cfg(v)["max_neighbors"] >= 4)
# tests/test_oracle_edges.py CASES["parallel_same_lp3"] (searched): the agent, then its three neighbours
_PARALLEL_SAME_LP3 = dict(pos=(-1.75, 1.875), vel=(0.1875, 1.0), vpref=0.5, pref=(0.6875, 0.125),
                          opos=((2.375, 1.125), (-0.25, 1.25), (0.5, 1.25)),
                          ovel=((0.25, 0.25), (-0.5, -0.9375), (-0.625, 0.875)))
SUPPLEMENT = 8                   # one env per slot of an 8-env workgroup


def lp3_parallel_supplement():
    """SUPPLEMENT 5-human envs (robot invisible, default ORCA parameters) whose first step reaches parallel_same_lp3,
    the one quad event that edge_batch(5, False, .) reaches under no variant.  The searched single-agent case is laid out
    as an env: the agent (v_pref 0.5, goal = position + preferred velocity), its three neighbours (at rest on their
    goals as far as their own preference goes), a fifth human at (40, 40) and the robot at (-40, -40), both out of
    range.  Env c holds the five roles rotated by c human slots, so that the agent sits in each lane group of a quad
    layout.  It is a batch of its own: edge_batch and its blocks are what they were.
    Returns (EnvState, ax, ay, names)."""
    c = _PARALLEL_SAME_LP3
    N, E = 5, SUPPLEMENT
    pos = np.array((c["pos"],) + c["opos"] + ((40.0, 40.0),))
    vel = np.array((c["vel"],) + c["ovel"] + ((0.0, 0.0),))
    goal = pos.copy()
    goal[0] += c["pref"]
    vpref = np.array([c["vpref"], 1.0, 1.0, 1.0, 1.0])
    st = cport.EnvState(E, N)
    for e in range(E):
        k = (np.arange(N) + e) % N           # role i sits in human slot k[i]
        st.hpx[e, k], st.hpy[e, k] = pos[:, 0], pos[:, 1]
        st.hvx[e, k], st.hvy[e, k] = vel[:, 0], vel[:, 1]
        st.hgx[e, k], st.hgy[e, k] = goal[:, 0], goal[:, 1]
        st.hvpref[e, k] = vpref
    st.hr[:] = HR
    st.rpx[:], st.rpy[:], st.rgx[:], st.rgy[:] = -40.0, -40.0, -40.0, -35.0
    st.rvx[:] = 0; st.rvy[:] = 0; st.rr[:] = HR
    st.gtime[:] = 0
    return st, np.zeros(E), np.zeros(E), ["parallel-same-lp3"] * E


def with_supplement(batch):
    """An edge_batch(5, False, .) result with lp3_parallel_supplement() appended."""
    st, ax, ay, names = batch
    s, sax, say, snames = lp3_parallel_supplement()
    return _concat([st, s]), np.concatenate([ax, sax]), np.concatenate([ay, say]), names + snames


def take(st, idx):
    """The envs idx of st, in that order (a copy)."""
    return _take(st, np.asarray(idx))


def oracle_cfg(robot_visible, variant=None, **kw):
    """The oracle config of an edge batch (ModelCrowdNav env defaults + the ORCA variant)."""
    return _oracle_cfg(1 if robot_visible else 0, variant or {}, **kw)
