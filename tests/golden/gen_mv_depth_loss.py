#!/usr/bin/env python
"""Generate tests/golden/mv_depth_loss.npz by running the REFERENCE's MVDepthLoss (losses.py:143-261) on the fixtures of
tests/mv_consistency_ref.py, in fp32 and in fp64.  Like gen_golden.py it runs only where the reference is, never on the GPU box.

Per case ``<name>``: the inputs (``<name>/pred``, ``cur``, ``invK``, ``world_T_cam``, ``src_depth``, ``src_K``, ``src_cam_T_world``,
float32) and, per precision ``f32`` / ``f64``: ``mask`` (B,K,h,w) and ``sampled`` (B,K,h,w) of ``get_valid_mask``, ``err`` (B,K,h,w) -
|log sampled - log projected| formed with the reference's own modules as ``get_error_for_pair`` forms it, before the masked select -
and ``loss``, the value of ``forward``.  ``self_*`` repeat mask, err and loss with the tested map as its own gate (cur = pred).

    python tests/golden/gen_mv_depth_loss.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import gen_golden
import mv_consistency_ref as ref


def blur_pool2d(input: torch.Tensor, kernel_size: int, stride: int = 2) -> torch.Tensor:
    """Stands in for kornia.filters.blur_pool2d so that the reference's losses.py imports (TorchScript wants a function with source);
    MVDepthLoss does not call it."""
    return input


def run(loss_mod, fx, dtype, self_gate):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in fx.items()}
    cur = t["pred"] if self_gate else t["cur"]
    K = t["src_depth"].shape[1]
    masks, sampled, errs = [], [], []
    with torch.no_grad():
        for k in range(K):
            m, s = loss_mod.get_valid_mask(cur, t["src_depth"][:, k], t["invK"], t["src_K"][:, k], t["world_T_cam"], t["src_cam_T_world"][:, k])
            pts = t["world_T_cam"] @ loss_mod.backproject(t["pred"], t["invK"])
            z = loss_mod.project(pts, t["src_K"][:, k], t["src_cam_T_world"][:, k]).view(-1, 3, *cur.shape[2:])[:, 2:]
            masks.append(m[:, 0]), sampled.append(s[:, 0]), errs.append(torch.abs(torch.log(s) - torch.log(z))[:, 0])
        loss = loss_mod(t["pred"], cur, t["src_depth"], t["invK"], t["src_K"], t["world_T_cam"], t["src_cam_T_world"])
    masks, errs = torch.stack(masks, 1), torch.stack(errs, 1)
    errs = torch.where(masks, errs, torch.full_like(errs, float("nan")))  # what masked_select leaves out is not part of the result
    return masks.numpy(), torch.stack(sampled, 1).numpy(), errs.numpy(), np.asarray(float(loss), np.float64)


def main():
    gen_golden.import_reference()
    sys.modules["kornia.filters"].blur_pool2d = blur_pool2d
    from losses import MVDepthLoss

    out = {}
    for name, (h, w, B, K, _) in ref.CASES.items():
        fx = ref.fixture(name)
        share = ref.ambiguous_share(fx)
        assert share <= ref.CAP, (name, share)
        for k, v in fx.items():
            out[f"{name}/{k}"] = v
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            loss_mod = MVDepthLoss(h, w).to(dtype)
            m, s, e, l = run(loss_mod, fx, dtype, False)
            out[f"{name}/{tag}/mask"], out[f"{name}/{tag}/sampled"], out[f"{name}/{tag}/err"], out[f"{name}/{tag}/loss"] = m, s, e, l
            m, s, e, l = run(loss_mod, fx, dtype, True)
            out[f"{name}/{tag}/self_mask"], out[f"{name}/{tag}/self_err"], out[f"{name}/{tag}/self_loss"] = m, e, l
        print(f"  {name}: {B} x {K} x {h} x {w}, ambiguous pixels {100 * share:.2f} %, visible {100 * out[f'{name}/f64/mask'].mean():.0f} %, "
              f"loss {float(out[f'{name}/f64/loss']):.6f}")
    path = os.path.join(HERE, "mv_depth_loss.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote mv_depth_loss.npz  {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
