"""Golden fixture for the full-horizon, K-sample Social-GAN prediction, from the real reference (run in a container
that has it):

    python -m tests.golden_tools.gen_golden_sgan_horizon

  g25_sgan_horizon  both shipped zara1_8 generators ('np': sgan-models, 'p': sgan-p-models; their weights are in
                    g6_sgan.npz and are not stored again), TrajectoryGenerator.forward (sgan/models.py:501-553) with
                    decoder.seq_len = 8 and 12 on scenes (S, N) = (6, 5), (3, 10), (4, 1) and one ragged batch of scene
                    sizes [3, 5, 1, 4], K = 3 user_noise vectors per scene.  Per case ('<tag>__<case>__'):
                      obs_traj [8,B,2] (rounded to 1e-4, float32), sizes [S], noise [3,S,8],
                      T<seq_len>__pred_rel [3,T,B,2], T<seq_len>__pred_abs (relative_to_abs, sgan/utils.py:85-98),
                      gt [12,B,2] synthetic ground truth (its first T frames for seq_len T), mask [B] (consider_ped),
                      T<seq_len>__ade_{sum,raw}[_mask], T<seq_len>__fde_{sum,raw}[_mask]: displacement_error /
                      final_displacement_error (sgan/losses.py:74-120) of every sample against gt.
Arrays only.
"""
import os

import numpy as np
import torch

from tests.golden_tools import gen_golden as G

OUT, REF = G.OUT, G.REF
CASES = (("S6_N5", [5] * 6), ("S3_N10", [10] * 3), ("S4_N1", [1] * 4), ("ragged", [3, 5, 1, 4]))
SEQ_LENS = (8, 12)
K = 3


def g25_sgan_horizon():
    from crowd_nav.policy.world_model import get_generator
    from sgan.losses import displacement_error, final_displacement_error
    from sgan.utils import relative_to_abs
    rng = np.random.RandomState(25)
    rec = {}
    dev = torch.device("cpu")
    for fam in ("sgan-models", "sgan-p-models"):
        ck = torch.load(os.path.join(REF, "sgan", "models", fam, "zara1_8_model.pt"), map_location="cpu", weights_only=True)
        gen = get_generator(ck, dev)
        tag = "p" if "p-models" in fam else "np"
        for name, sizes in CASES:
            B, S = sum(sizes), len(sizes)
            pos0 = rng.uniform(-4, 4, (B, 2))
            vel = rng.uniform(-0.4, 0.4, (B, 2))
            traj = np.stack([pos0 + vel * t + rng.normal(0, 0.02, (B, 2)) for t in range(8)], 0)
            traj = np.around(traj, 4).astype(np.float32)
            rel = np.zeros_like(traj); rel[1:] = traj[1:] - traj[:-1]
            ends = np.cumsum(sizes)
            sse = torch.tensor(np.stack([ends - np.array(sizes), ends], 1), dtype=torch.long)
            noise = rng.normal(0, 1, (K, S, 8)).astype(np.float32)
            gt = np.stack([traj[-1] + vel * (t + 1) + rng.normal(0, 0.05, (B, 2)) for t in range(12)], 0).astype(np.float32)
            mask = (rng.uniform(0, 1, B) < 0.6).astype(np.float32)
            key = "%s__%s__" % (tag, name)
            rec[key + "obs_traj"], rec[key + "sizes"], rec[key + "noise"] = traj, np.array(sizes, np.int64), noise
            rec[key + "gt"], rec[key + "mask"] = gt, mask
            for T in SEQ_LENS:
                gen.decoder.seq_len = T
                out = {n: [] for n in ("pred_rel", "pred_abs", "ade_sum", "ade_raw", "ade_sum_mask", "ade_raw_mask",
                                       "fde_sum", "fde_raw", "fde_sum_mask", "fde_raw_mask")}
                g_t, m_t = torch.from_numpy(gt[:T]), torch.from_numpy(mask)
                for k in range(K):
                    with torch.no_grad():
                        pr = gen(torch.from_numpy(traj), torch.from_numpy(rel), sse, user_noise=torch.from_numpy(noise[k]))
                        pa = relative_to_abs(pr, torch.from_numpy(traj)[-1])
                    out["pred_rel"].append(pr.numpy()); out["pred_abs"].append(pa.numpy())
                    for mode in ("sum", "raw"):
                        for sfx, cp in (("", None), ("_mask", m_t)):
                            out["ade_%s%s" % (mode, sfx)].append(displacement_error(pa, g_t, cp, mode=mode).numpy())
                            out["fde_%s%s" % (mode, sfx)].append(final_displacement_error(pa[-1], g_t[-1], cp, mode=mode).numpy())
                for n, v in out.items():
                    rec["%sT%d__%s" % (key, T, n)] = np.stack(v, 0)
    np.savez_compressed(os.path.join(OUT, "g25_sgan_horizon.npz"), **rec)
    print("g25_sgan_horizon: %d arrays" % len(rec))


if __name__ == "__main__":
    g25_sgan_horizon()
