"""Inputs and restatements for the Social-GAN step (sgan_step.hip, mcn_sgan_step) away from VecSGANWorld's own use.

  * ring_after / window: a numpy restatement of the device ring -- the call writes np.around(cur_pos, 4) into slot
    push_slot and nothing else, and the network reads the 8 slots from `oldest` on (the pushed frame included);
  * net_inputs: the float32 positions and displacements the kernel feeds the network (differences of the rounded
    float64 frames, then float32);
  * round4_values: float64 positions on which a 1e-4 rounding goes wrong if it is not np.around's
    rint(x * 1e4) / 1e4: exact half-ties of x * 1e4 (found by a float64 search), values that round to -0.0,
    magnitudes where x * 1e4 is an exact integer, both signs;
  * saturating: the shipped weights with encoder / decoder LSTM layers scaled until the gates saturate and the
    encoder's cell state grows over the 8 steps (encoder_cell_max measures it).

The CPU self-tests are tests/test_sgan_states_cpu.py."""
import os

import numpy as np
import torch

from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights(tag, dtype=torch.float32):
    """The shipped zara1_8 generator weights of tests/golden/g6_sgan.npz ('p': with pool_net, 'np': without) as a
    state_dict of CPU tensors."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g6_sgan.npz"))
    pre = tag + "__w__"
    return {k[len(pre):].replace("__", "."): torch.from_numpy(np.asarray(g[k])).to(dtype) for k in g.files
            if k.startswith(pre)}


def saturating(w, scale=3.0, forget_bias=4.0):
    """w with every LSTM weight and bias of the encoder and the decoder multiplied by `scale` and `forget_bias` added
    to the forget gates' input bias (rows 32:64 in PyTorch's i, f, g, o order)."""
    out = {k: v.clone() for k, v in w.items()}
    for cell in ("encoder.encoder", "decoder.decoder"):
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            out[cell + "." + k] *= scale
        out[cell + ".bias_ih_l0"][32:64] += forget_bias
    return out


def load(gen, w):
    """Write state_dict w into generator gen in place (its packed weights follow: load_state_dict bumps versions)."""
    gen.load_state_dict({k: v.to(torch.float32) for k, v in w.items()})
    return gen


def histories(rng, E, N, spread=4.0, speed=0.8, dt=0.25):
    """[E,8,N,2] float64 frames on the 1e-4 grid: constant-velocity walks with jitter, oldest first."""
    pos = rng.uniform(-spread, spread, (E, 1, N, 2))
    vel = rng.uniform(-speed, speed, (E, 1, N, 2))
    k = np.arange(-7, 1, dtype=np.float64).reshape(1, 8, 1, 1)
    return np.around(pos + vel * dt * k + rng.normal(0, 0.01, (E, 8, N, 2)), 4)


def next_positions(rng, hist, oldest, dt=0.25):
    """Plausible next frame [E,N,2] (not rounded) continuing the newest frame of the window that starts at `oldest`."""
    newest = hist[:, (oldest + 7) & 7]
    prev = hist[:, (oldest + 6) & 7]
    return newest + (newest - prev) + rng.normal(0, 0.01, newest.shape)


def ring_after(hist, push_slot, cur_pos):
    """The ring after one mcn_sgan_step: only slot push_slot changes, to np.around(cur_pos, 4); unchanged without
    cur_pos."""
    out = np.array(hist, np.float64, copy=True)
    if cur_pos is not None:
        out[:, push_slot] = np.around(np.asarray(cur_pos, np.float64), 4)
    return out


def window(hist, oldest):
    """[8, E*N, 2] float64: the frames the network reads, slot (oldest + t) & 7 at t."""
    E, T, N, _ = hist.shape
    return np.stack([hist[:, (oldest + t) & 7] for t in range(8)], 0).reshape(8, E * N, 2)


def net_inputs(win):
    """(positions, displacements) as the kernel feeds them, float32 [8, B, 2]: displacement t is the float64
    difference of the rounded frames t and t - 1 (0 at t = 0), then float32."""
    rel = np.zeros_like(win)
    rel[1:] = win[1:] - win[:-1]
    return torch.from_numpy(win).float(), torch.from_numpy(rel).float()


def reference(w, win, N, noise, pooling, dtype=torch.float32, time_step=0.25):
    """(pred_rel [B,2], velocities [B,2] float64) of pyref.sgan_generator on the window, in `dtype` from the float32
    inputs the kernel sees."""
    t32, r32 = net_inputs(win)
    wd = {k: v.to(dtype) for k, v in w.items()}
    noise = torch.as_tensor(noise)
    with torch.no_grad():
        pr = pyref.sgan_generator(wd, t32.to(dtype), r32.to(dtype), N, noise.to(dtype), pooling)
    vel = pyref.sgan_velocities(pr.float(), t32[-1], time_step) if dtype == torch.float32 else None
    return pr.numpy(), vel


def encoder_cell_max(w, win):
    """max |c| of the encoder LSTM after each of the 8 steps (float64): [8]."""
    _, r32 = net_inputs(win)
    x = r32.double()
    wd = {k: v.double() for k, v in w.items()}
    emb = torch.nn.functional.linear(x, wd["encoder.spatial_embedding.weight"], wd["encoder.spatial_embedding.bias"])
    B = x.shape[1]
    h = torch.zeros(B, 32, dtype=torch.float64)
    c = torch.zeros(B, 32, dtype=torch.float64)
    out = []
    for t in range(8):
        h, c = pyref._lstm_cell(emb[t], h, c, wd["encoder.encoder.weight_ih_l0"], wd["encoder.encoder.weight_hh_l0"],
                                wd["encoder.encoder.bias_ih_l0"], wd["encoder.encoder.bias_hh_l0"])
        out.append(float(c.abs().max()))
    return np.array(out)


def half_ties(count, lo=-40000, hi=40000, seed=0):
    """`count` float64 x (both signs, even and odd k) with x * 1e4 == k + 0.5 exactly in float64."""
    rng = np.random.RandomState(seed)
    found = []
    for k in rng.permutation(np.arange(lo, hi)):
        x = (float(k) + 0.5) / 1e4
        if x * 1e4 == float(k) + 0.5:
            found.append(x)
            if len(found) == count:
                break
    return np.array(found)


def round4_values():
    """float64 positions on the edges of np.around(x, 4) (see the module docstring), shuffled with a fixed seed."""
    ties = half_ties(48)
    near = np.concatenate([np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf)])
    to_minus_zero = np.array([-1e-5, -4.9999e-5, -0.00005, -1e-300, -5e-324, -0.0, -3.3e-5])
    big = np.array([1e11, -1e11, 123456789012.0, -98765432109.5, 2.5e12, -7e13, 3.0e15, 2.0 ** 60, -(2.0 ** 70)])
    small = np.array([0.0, 1e-5, 0.00005, 0.00015, 0.00025, -0.00015, -0.00025, 1.23455, -1.23455, 2.00005])
    vals = np.concatenate([ties, near, to_minus_zero, big, small])
    return vals[np.random.RandomState(1).permutation(len(vals))]
