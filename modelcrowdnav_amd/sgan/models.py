"""TrajectoryGenerator of the shipped Social-GAN checkpoints (reference: sgan/models.py).

The module tree reproduces the reference's parameter names so `checkpoint['g_state']` of
sgan/models/sgan-models/*.pt and sgan-p-models/*.pt loads with load_state_dict
(encoder.encoder.*, encoder.spatial_embedding.*, decoder.decoder.*, decoder.spatial_embedding.*,
decoder.hidden2pos.*, pool_net.spatial_embedding.*, pool_net.mlp_pre_pool.{0,2}.*,
mlp_decoder_context.{0,2}.*).  Inference does not run these modules: `pack()` permutes the
weights into MFMA operand order and sgan_step.hip evaluates the network (models.py:501-553: one step per
mcn_sgan_step for the world model, decoder.seq_len steps x K noise samples per mcn_sgan_predict).  SocialPooling, the discriminator, batch-norm variants and
pool_every_timestep are not used by any shipped checkpoint and are not built.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from .._pack import natural as _natural, pack_linear


def make_mlp(dim_list):
    """models.py:5-17 with batch_norm=False, dropout=0 (the shipped configuration): Linear+ReLU pairs."""
    layers = []
    for a, b in zip(dim_list[:-1], dim_list[1:]):
        layers += [nn.Linear(a, b), nn.ReLU()]
    return nn.Sequential(*layers)


class _Encoder(nn.Module):
    def __init__(self, emb, h):
        super().__init__()
        self.encoder = nn.LSTM(emb, h, 1)
        self.spatial_embedding = nn.Linear(2, emb)


class _Decoder(nn.Module):
    def __init__(self, emb, h):
        super().__init__()
        self.seq_len = 1
        self.decoder = nn.LSTM(emb, h, 1)
        self.spatial_embedding = nn.Linear(2, emb)
        self.hidden2pos = nn.Linear(h, 2)


class _PoolHiddenNet(nn.Module):
    def __init__(self, emb, h, bottleneck):
        super().__init__()
        self.spatial_embedding = nn.Linear(2, emb)
        self.mlp_pre_pool = make_mlp([emb + h, 512, bottleneck])


class _SganNet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_elstm", "b_elstm", "w_p1", "b_p1", "w_p2", "b_p2", "w_c1", "b_c1",
                                          "w_c2", "b_c2", "w_dlstm", "b_dlstm", "w_h2p", "b_h2p")] + [("pooling", C.c_int32)]


_hip.check_mirrors({_hip.SIZEOF_SGAN_NET: _SganNet})


def _fold_embedding(W, b, W_se, b_se):
    """A layer W [nout, 16 + h] applied to [spatial_embedding(d), h] equals [W_e W_se | W_h] applied to [d, h] with
    bias b + W_e b_se (the embedding is a plain Linear(2, 16): sgan/models.py:47,66 / 120,142 / 186,221-223).
    Composed in float64 and rounded once."""
    W, W_se = W.astype(np.float64), W_se.astype(np.float64)
    Wf = np.concatenate([W[:, :16] @ W_se, W[:, 16:]], 1)
    bf = b.astype(np.float64) + W[:, :16] @ b_se.astype(np.float64)
    return Wf.astype(np.float32), bf.astype(np.float32)


def _kmap_rel_h():
    """Input tiles of a folded layer: tile 0 = displacement (x in slot 0, y in slot 4: one MFMA k-step), tiles 1-2 =
    the 32 hidden features."""
    m = np.full(48, -1, np.int32)
    m[0], m[4] = 0, 1
    m[16:48] = 2 + np.arange(32)
    return m


class TrajectoryGenerator(nn.Module):
    def __init__(self, obs_len=8, pred_len=1, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64,
                 num_layers=1, noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type=None,
                 pool_every_timestep=False, dropout=0.0, bottleneck_dim=8, activation="relu", batch_norm=False,
                 neighborhood_size=2.0, grid_size=8, device=None):
        super().__init__()
        if pooling_type and str(pooling_type).lower() == "none":
            pooling_type = None
        supported = (embedding_dim == 16 and encoder_h_dim == 32 and decoder_h_dim == 32 and mlp_dim == 64 and
                     num_layers == 1 and tuple(noise_dim) == (8,) and noise_mix_type == "global" and
                     bottleneck_dim == 8 and not batch_norm and not pool_every_timestep and
                     pooling_type in (None, "pool_net"))
        if not supported:
            raise NotImplementedError("sgan_step.hip is built for the architecture of the shipped checkpoints "
                                      "(emb 16, h 32, mlp 64, bottleneck 8, noise (8,) global, no batch norm)")
        self.obs_len, self.pred_len = obs_len, pred_len
        self.noise_type, self.noise_dim, self.pooling_type = noise_type, tuple(noise_dim), pooling_type
        self.device = device
        self.encoder = _Encoder(embedding_dim, encoder_h_dim)
        self.decoder = _Decoder(embedding_dim, decoder_h_dim)
        if pooling_type == "pool_net":
            self.pool_net = _PoolHiddenNet(embedding_dim, encoder_h_dim, bottleneck_dim)
        ctx_in = encoder_h_dim + (bottleneck_dim if pooling_type else 0)
        self.mlp_decoder_context = make_mlp([ctx_in, mlp_dim, decoder_h_dim - noise_dim[0]])
        self._packed = None

    # ------------------------------------------------------------------ packing
    def pack(self, dev):
        """(ctypes mcn_sgan_net, [device tensors kept alive]), re-packed when a parameter changed since they were made
        or the device changed (_hip.weights_stamp).  Writes through `p.data` (`p.data.copy_`) are invisible: call
        refresh() after them."""
        version = _hip.weights_stamp(self.parameters(), dev)
        if self._packed is not None and self._packed[0] == version:
            return self._packed[1]
        sd = {k: v.detach().to("cpu", torch.float32).contiguous().numpy() for k, v in self.state_dict().items()}
        net, keep = _SganNet(), []

        def put(name, W, b, kmap):
            for pre, t in zip(("w_", "b_"), pack_linear(W, b, kmap, None, dev)):
                keep.append(t)
                setattr(net, pre + name, t.data_ptr())

        def lstm(prefix):
            W = np.concatenate([sd[prefix + ".weight_ih_l0"], sd[prefix + ".weight_hh_l0"]], 1)     # [128, 16+32]
            return W, sd[prefix + ".bias_ih_l0"] + sd[prefix + ".bias_hh_l0"]

        put("elstm", *_fold_embedding(*lstm("encoder.encoder"), sd["encoder.spatial_embedding.weight"],
                                      sd["encoder.spatial_embedding.bias"]), _kmap_rel_h())
        if self.pooling_type:
            put("p1", *_fold_embedding(sd["pool_net.mlp_pre_pool.0.weight"], sd["pool_net.mlp_pre_pool.0.bias"],
                                       sd["pool_net.spatial_embedding.weight"], sd["pool_net.spatial_embedding.bias"]),
                _kmap_rel_h())
            put("p2", sd["pool_net.mlp_pre_pool.2.weight"], sd["pool_net.mlp_pre_pool.2.bias"], _natural(512, 32))
            put("c1", sd["mlp_decoder_context.0.weight"], sd["mlp_decoder_context.0.bias"], _natural(40, 3))
        else:
            put("c1", sd["mlp_decoder_context.0.weight"], sd["mlp_decoder_context.0.bias"], _natural(32, 2))
        put("c2", sd["mlp_decoder_context.2.weight"], sd["mlp_decoder_context.2.bias"], _natural(64, 4))
        put("dlstm", *_fold_embedding(*lstm("decoder.decoder"), sd["decoder.spatial_embedding.weight"],
                                      sd["decoder.spatial_embedding.bias"]), _kmap_rel_h())
        put("h2p", sd["decoder.hidden2pos.weight"], sd["decoder.hidden2pos.bias"], _natural(32, 2))
        net.pooling = 1 if self.pooling_type else 0
        self._packed = (version, (net, keep))
        return self._packed[1]

    def refresh(self):
        """Re-pack the weights at the next step (after a write the weight stamp cannot see)."""
        self._packed = None

    # ------------------------------------------------------------------ reference call signature
    def forward(self, obs_traj, obs_traj_rel, seq_start_end, user_noise=None):
        """models.py:501-553.  obs_traj [8,B,2]; returns [decoder.seq_len,B,2] float32 on obs_traj's device (seq_len is
        1 unless the caller sets it, whatever pred_len the checkpoint carries: world_model.py:252).  Scenes may differ
        in size.  obs_traj_rel is recomputed from obs_traj (identical values)."""
        S = int(seq_start_end.shape[0])
        noise = user_noise if user_noise is not None else torch.randn(S, self.noise_dim[0]).to(obs_traj.device)
        return self.sample(obs_traj, seq_start_end, noise.view(1, S, -1), int(self.decoder.seq_len))[0]

    def sample(self, obs_traj, seq_start_end, noise, steps):
        """K futures of `steps` decoder steps from one encoder / pooling pass: noise [K,S,8] (one user_noise vector per
        sample and scene) -> pred_traj_fake_rel [K,steps,B,2] float32, rows in obs_traj's order.  Scenes of different
        sizes are scattered into an [S, Nmax] padded ring whose unused slots the pooling module does not look at
        (mcn_sgan_predict's hcount)."""
        dev = obs_traj.device
        if dev.type != "cuda":
            raise RuntimeError("TrajectoryGenerator inference only exists as HIP kernels; move inputs to the GPU")
        if int(steps) < 1:
            raise ValueError("steps must be >= 1")
        sse = torch.as_tensor(seq_start_end).to("cpu", torch.long)
        sizes = sse[:, 1] - sse[:, 0]
        S, N, B = int(sse.shape[0]), int(sizes.max()), int(obs_traj.shape[1])
        noise = noise.to(dev, torch.float32).contiguous()
        if noise.dim() != 3 or tuple(noise.shape[1:]) != (S, self.noise_dim[0]):
            raise ValueError("noise must be [K, %d, %d]" % (S, self.noise_dim[0]))
        if bool((sizes == N).all()) and S * N == B and int(sse[0, 0]) == 0 and bool((sse[1:, 0] == sse[:-1, 1]).all()):
            hist = obs_traj.double().view(8, S, N, 2).permute(1, 0, 2, 3).contiguous()
            rel, _ = sgan_predict(self, hist, 0, noise, steps, want_pos=False)
            return rel
        if bool((sizes < 1).any()):
            raise ValueError("every scene of seq_start_end needs at least one pedestrian")
        # row b of the batch -> slot (scene, index in scene) of the padded ring
        scene = torch.repeat_interleave(torch.arange(S), sizes)
        rows = torch.cat([torch.arange(int(a), int(b)) for a, b in sse.tolist()])
        slot = (scene * N + (torch.arange(len(rows)) - torch.repeat_interleave(sizes.cumsum(0) - sizes, sizes))).to(dev)
        rows = rows.to(dev)
        padded = torch.zeros(8, S * N, 2, dtype=torch.float64, device=dev)
        padded[:, slot] = obs_traj.double()[:, rows]
        hist = padded.view(8, S, N, 2).permute(1, 0, 2, 3).contiguous()
        rel, _ = sgan_predict(self, hist, 0, noise, steps, hcount=sizes.to(dev, torch.int32), want_pos=False)
        out = torch.zeros(rel.shape[0], rel.shape[1], B, 2, dtype=torch.float32, device=dev)
        out[:, :, rows] = rel[:, :, slot]
        return out


_WS = {}


def _workspace(E, N, dev):
    """The step's and the prediction's scratch buffer (mcn_sgan_workspace_bytes), one kept per process."""
    key = (E, N, str(dev))
    if key not in _WS:
        _WS.clear()
        _WS[key] = torch.empty(_hip.lib.mcn_sgan_workspace_bytes(E, N) // 4, dtype=torch.float32, device=dev)
    return _WS[key]


def sgan_step(gen, hist, push_slot, oldest, cur_pos, noise, time_step, want_rel=False, out_vel=None, hcount=None):
    """Thin wrapper over mcn_sgan_step.  hist [E,8,N,2] f64 (modified in place when cur_pos is given)."""
    E, T, N, _ = hist.shape
    dev = hist.device
    net, _keep = gen.pack(dev)
    if out_vel is None:
        out_vel = torch.empty(E, N, 2, dtype=torch.float64, device=dev)
    rel = torch.empty(E * N, 2, dtype=torch.float32, device=dev) if want_rel else None
    rc = _hip.lib.mcn_sgan_step(C.byref(net), _hip.ptr(hist), int(push_slot), int(oldest), _hip.ptr(cur_pos),
                                _hip.ptr(noise), _hip.ptr(hcount), _hip.ptr(_workspace(E, N, dev)), _hip.ptr(out_vel), _hip.ptr(rel),
                                float(time_step), E, N, _hip.stream_ptr(dev))
    _hip.check(rc, "mcn_sgan_step")
    return out_vel, rel


def sgan_predict(gen, hist, oldest, noise, steps, hcount=None, want_pos=True):
    """Thin wrapper over mcn_sgan_predict.  hist [E,8,N,2] f64 (read only), noise [K,E,8] f32 ->
    (rel [K,steps,E*N,2] f32, pos [K,steps,E*N,2] f64 or None)."""
    E, _, N, _ = hist.shape
    K, T = int(noise.shape[0]), int(steps)
    dev = hist.device
    net, _keep = gen.pack(dev)
    rel = torch.empty(K, T, E * N, 2, dtype=torch.float32, device=dev)
    pos = torch.empty(K, T, E * N, 2, dtype=torch.float64, device=dev) if want_pos else None
    rc = _hip.lib.mcn_sgan_predict(C.byref(net), _hip.ptr(hist), int(oldest), _hip.ptr(noise), K, T, _hip.ptr(hcount),
                                   _hip.ptr(_workspace(E, N, dev)), _hip.ptr(rel), _hip.ptr(pos), E, N,
                                   _hip.stream_ptr(dev))
    _hip.check(rc, "mcn_sgan_predict")
    return rel, pos
