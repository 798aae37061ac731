"""Float64 numpy restatement of the Social-GAN generator for decoder.seq_len = T steps and K noise samples per scene
(reference: sgan/models.py -- Encoder :28-71, PoolHiddenNet :167-232, TrajectoryGenerator.forward :501-553, add_noise
:454-490, Decoder.forward :127-164 with pool_every_timestep = False).  It stands for mcn_sgan_predict where
oracle/pyref.sgan_generator stands for the one-step mcn_sgan_step: the yardstick of tests/test_sgan_horizon_gpu.py,
itself checked against the reference's recorded outputs in tests/test_sgan_horizon_cpu.py.

Everything is evaluated in float64 from the float32 inputs the kernels see (positions and displacements of the 1e-4
grid rounded to float32, float32 weights and noise)."""
import numpy as np

from tests import sgan_states as S


def weights64(tag):
    """The shipped zara1_8 weights of tests/golden/g6_sgan.npz as float64 numpy arrays by state_dict key."""
    return {k: v.double().numpy() for k, v in S.weights(tag).items()}


def _lin(x, w, name):
    return x @ w[name + ".weight"].T + w[name + ".bias"]


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _cell(x, h, c, w, name):
    g = x @ w[name + ".weight_ih_l0"].T + w[name + ".bias_ih_l0"] + h @ w[name + ".weight_hh_l0"].T + w[name + ".bias_hh_l0"]
    i, f, gg, o = np.split(g, 4, axis=1)
    c = _sigmoid(f) * c + _sigmoid(i) * np.tanh(gg)
    return _sigmoid(o) * np.tanh(c), c


def inputs(win):
    """(last positions [B,2], displacements [8,B,2]) in float64 holding the float32 values the kernels feed the
    network, from a window [8,B,2] of float64 frames on the 1e-4 grid (sgan_states.window)."""
    t32, r32 = S.net_inputs(np.asarray(win, np.float64))
    return t32[-1].double().numpy(), r32.double().numpy()


def context(w, last_pos, obs_rel, sizes, pooling):
    """mlp_decoder_context's output [B,24] and what precedes it: independent of the noise and of the decoder step."""
    B = obs_rel.shape[1]
    h, c = np.zeros((B, 32)), np.zeros((B, 32))
    for t in range(obs_rel.shape[0]):
        h, c = _cell(_lin(obs_rel[t], w, "encoder.spatial_embedding"), h, c, w, "encoder.encoder")
    x = h
    if pooling:
        pooled, a = [], 0
        for n in sizes:
            hs, ps = h[a:a + n], last_pos[a:a + n]
            rel = ps[None, :, :] - ps[:, None, :]                            # [i, k] = P_k - P_i
            emb = _lin(rel.reshape(n * n, 2), w, "pool_net.spatial_embedding")
            y = np.concatenate([emb, np.tile(hs, (n, 1))], 1)                # partner k's hidden state beside (i, k)
            y = np.maximum(_lin(y, w, "pool_net.mlp_pre_pool.0"), 0.0)
            y = np.maximum(_lin(y, w, "pool_net.mlp_pre_pool.2"), 0.0)
            pooled.append(y.reshape(n, n, -1).max(1))
            a += n
        x = np.concatenate([h, np.concatenate(pooled, 0)], 1)
    x = np.maximum(_lin(x, w, "mlp_decoder_context.0"), 0.0)
    return np.maximum(_lin(x, w, "mlp_decoder_context.2"), 0.0)


def predict(w, last_pos, obs_rel, sizes, noise, T, pooling):
    """pred_traj_fake_rel [K,T,B,2] float64.  w: weights64(); last_pos [B,2], obs_rel [8,B,2]: inputs(); sizes: the
    scenes' pedestrian counts in row order; noise [K,S,8]."""
    sizes = [int(n) for n in sizes]
    assert sum(sizes) == obs_rel.shape[1] and noise.shape[1:] == (len(sizes), 8)
    ctx = context(w, last_pos, obs_rel, sizes, pooling)
    out = np.zeros((noise.shape[0], T, obs_rel.shape[1], 2))
    for k in range(noise.shape[0]):
        z = np.repeat(np.asarray(noise[k], np.float64), sizes, axis=0)
        h, c = np.concatenate([ctx, z], 1), np.zeros((obs_rel.shape[1], 32))
        x = obs_rel[-1]
        for t in range(T):
            h, c = _cell(_lin(x, w, "decoder.spatial_embedding"), h, c, w, "decoder.decoder")
            x = _lin(h, w, "decoder.hidden2pos")
            out[k, t] = x
    return out


def positions(last_pos, rel):
    """last_pos [B,2] + running float64 sum over the steps of rel [K,T,B,2] (what out_pos holds)."""
    return np.cumsum(np.asarray(rel, np.float64), axis=1) + last_pos[None, None]


def predict_ring(w, hist, oldest, noise, T, pooling, counts=None):
    """predict() for a device ring hist [E,8,N,2] read from slot `oldest`: [K,T,E,N,2]; with counts, scene e is run on
    its first counts[e] pedestrians and the other slots are NaN."""
    E, _, N, _ = hist.shape
    if counts is None:
        last, rel = inputs(S.window(hist, oldest))
        return predict(w, last, rel, [N] * E, noise, T, pooling).reshape(noise.shape[0], T, E, N, 2)
    out = np.full((noise.shape[0], T, E, N, 2), np.nan)
    for e in range(E):
        n = int(counts[e])
        last, rel = inputs(S.window(hist[e:e + 1, :, :n], oldest))
        out[:, :, e, :n] = predict(w, last, rel, [n], noise[:, e:e + 1], T, pooling)
    return out
