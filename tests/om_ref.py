"""numpy float64 restatement of OM-SARL's occupancy maps (multi_human_rl.py:109-163 at cell_num = 4,
om_channel_size = 3) for the tests: the maps, the pre-floor grid coordinates that decide them (the "edge band"), and
the torch-float32 look-ahead values of one env on [13 rotated features | 48 map entries].

A map entry is decided by floor(), so a coordinate within rounding noise of a cell edge may legitimately differ between
numpy's libm and the device's.  Tests compare maps only where every pre-floor coordinate of a pair with d > 0 is further
than EDGE_BAND from each integer 0 .. 4 (coincident humans are exact: x' = y' = +-0, cell (2, 2)), and assert that this
leaves nothing out."""
import numpy as np
import torch

from oracle import pyref
from tests import policy_ref as R

CELL_NUM, CHANNELS = 4, 3
WIDTH = CELL_NUM ** 2 * CHANNELS
EDGE_BAND = 1e-9


def _turned(hum, i, cell_size):
    """For human i of hum [N,4] (px, py, vx, vy): the other humans' indices, pre-floor grid coordinates (gx, gy),
    distances and velocities in i's frame, in the reference's operation sequence."""
    hum = np.asarray(hum, np.float64)
    others = np.array([k for k in range(len(hum)) if k != i], np.int64)
    o = hum[others]
    dx, dy = o[:, 0] - hum[i, 0], o[:, 1] - hum[i, 1]
    thv = np.arctan2(hum[i, 3], hum[i, 2])
    rot = np.arctan2(dy, dx) - thv
    d = np.sqrt(dx * dx + dy * dy)
    gx = np.cos(rot) * d / cell_size + CELL_NUM / 2
    gy = np.sin(rot) * d / cell_size + CELL_NUM / 2
    rv = np.arctan2(o[:, 3], o[:, 2]) - thv
    speed = np.sqrt(o[:, 2] * o[:, 2] + o[:, 3] * o[:, 3])
    return others, gx, gy, d, np.cos(rv) * speed, np.sin(rv) * speed


def maps(hum, cell_size=1.0, count=None):
    """[N,48] float32: entry 3 * (4 iy + ix) + channel = (occupied, mean vx', mean vy') over the OTHER humans in the cell,
    summed in index order.  count: only the first `count` humans exist (rows beyond it, and a lone human's, are zero)."""
    hum = np.asarray(hum, np.float64)
    N = len(hum)
    n = N if count is None else max(1, min(int(count), N))
    out = np.zeros((N, WIDTH), np.float32)
    if n < 2:
        return out
    for i in range(n):
        _, gx, gy, _, vx, vy = _turned(hum[:n], i, cell_size)
        members = [[] for _ in range(CELL_NUM ** 2)]
        for k in range(len(gx)):
            fx, fy = np.floor(gx[k]), np.floor(gy[k])
            if 0 <= fx < CELL_NUM and 0 <= fy < CELL_NUM:          # NaN compares false
                members[int(CELL_NUM * fy + fx)].append(k)
        for c, ks in enumerate(members):
            if ks:
                sx = sy = 0
                for k in ks:
                    sx, sy = sx + vx[k], sy + vy[k]
                out[i, 3 * c:3 * c + 3] = (1.0, sx / len(ks), sy / len(ks))
    return out


def edge_margin(hum, cell_size=1.0, count=None):
    """Smallest distance of a pre-floor coordinate (pairs with d > 0) to an integer 0 .. 4; inf without such a pair."""
    hum = np.asarray(hum, np.float64)
    n = len(hum) if count is None else max(1, min(int(count), len(hum)))
    best = np.inf
    for i in range(n if n > 1 else 0):
        _, gx, gy, d, _, _ = _turned(hum[:n], i, cell_size)
        g = np.concatenate([gx[d > 0], gy[d > 0]])
        g = g[np.isfinite(g)]
        if len(g):
            best = min(best, float(np.abs(g[:, None] - np.arange(CELL_NUM + 1)[None]).min()))
    return best


def edge_margin_batch(hum, cell_size=1.0):
    """edge_margin for every env of hum [E,N,4] at once (all N humans seen): [E]."""
    hum = np.asarray(hum, np.float64)
    E, N, _ = hum.shape
    dx = hum[:, None, :, 0] - hum[:, :, None, 0]                    # [E, i, k]: other k seen from human i
    dy = hum[:, None, :, 1] - hum[:, :, None, 1]
    thv = np.arctan2(hum[:, :, 3], hum[:, :, 2])[:, :, None]
    rot = np.arctan2(dy, dx) - thv
    d = np.sqrt(dx * dx + dy * dy)
    g = np.stack([np.cos(rot) * d / cell_size + CELL_NUM / 2, np.sin(rot) * d / cell_size + CELL_NUM / 2], -1)
    m = np.abs(g[..., None] - np.arange(CELL_NUM + 1)).min(-1).min(-1)                  # [E, i, k]
    skip = np.eye(N, dtype=bool)[None] | ~(d > 0) | ~np.isfinite(m)
    return np.where(skip, np.inf, m).reshape(E, -1).min(1)


def next_humans(hum, time_step=0.25, nexts=None):
    """[N,4] states the look-ahead's maps are built from: constant velocity, or the env's (query_env)."""
    hum = np.asarray(hum, np.float64)
    if nexts is not None:
        return np.asarray(nexts, np.float64)[:, :4]
    return np.stack([hum[:, 0] + hum[:, 2] * time_step, hum[:, 1] + hum[:, 3] * time_step, hum[:, 2], hum[:, 3]], 1)


def rows61(self_row, hum, table, kinematics, time_step=0.25, nexts=None, rewards=None, cell_size=1.0):
    """([A,N,61] float32 network inputs of every candidate action, rewards [A]) for one env whose N humans are all seen."""
    xr, rew = R.rotated_rows(self_row, hum, table, kinematics, time_step, nexts, rewards)
    om = torch.from_numpy(maps(next_humans(hum, time_step, nexts), cell_size))
    return torch.cat([xr, om.unsqueeze(0).expand(xr.shape[0], -1, -1)], 2), rew


def values(w, self_row, hum, table, kinematics, time_step=0.25, gamma=0.9, nexts=None, rewards=None, cell_size=1.0):
    """Look-ahead values [A] (float64) of one env: pyref.sarl_forward in the dtype of the weights w."""
    x, rew = rows61(self_row, hum, table, kinematics, time_step, nexts, rewards, cell_size)
    dtype = next(iter(w.values())).dtype
    with torch.no_grad():
        V = pyref.sarl_forward(w, x.to(dtype))[0].double().numpy()
    g = pow(gamma, time_step * float(self_row[7]))
    return np.array([rew[a] + g * float(V[a]) for a in range(len(rew))])
