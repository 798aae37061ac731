"""Trajectory errors the Social-GAN evaluation reports (reference: sgan/losses.py:74-120, used by check_accuracy in
crowd_nav/utils/trainer_sgan.py:136-218 and by the best-of-K "variety" scores minADE / minFDE)."""
import torch


def _apply(err, consider_ped, mode):
    if consider_ped is not None:
        err = err * consider_ped
    if mode == "raw":
        return err
    return torch.sum(err)


def displacement_error(pred_traj, pred_traj_gt, consider_ped=None, mode="sum"):
    """Per pedestrian, the Euclidean distance between prediction and ground truth summed over the steps (ADE times the
    number of steps).  pred_traj, pred_traj_gt: [T,B,2]; consider_ped: [B] weights or None; mode 'raw' returns the [B]
    errors, 'sum' their total."""
    if mode not in ("sum", "raw"):
        raise ValueError("mode must be 'sum' or 'raw'")
    dist = torch.sqrt(((pred_traj_gt - pred_traj) ** 2).sum(dim=2))        # [T,B]
    return _apply(dist.sum(dim=0), consider_ped, mode)


def final_displacement_error(pred_pos, pred_pos_gt, consider_ped=None, mode="sum"):
    """Euclidean distance between the predicted and the true final positions [B,2] (FDE): [B] for mode 'raw', their
    total otherwise."""
    dist = torch.sqrt(((pred_pos_gt - pred_pos) ** 2).sum(dim=1))
    return _apply(dist, consider_ped, mode)
