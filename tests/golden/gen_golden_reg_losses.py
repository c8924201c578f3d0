#!/usr/bin/env python
"""Golden G18 of DepthModel's validation losses: the REFERENCE's own ``DepthModel.compute_losses``
(experiment_modules/depth_model.py:442-540) called unbound on a shim that carries what it reads - ``run_opts.dataset`` and ``si_loss``,
``abs_loss``, ``grad_loss``, ``normals_loss``, ``mv_depth_loss``, ``ms_loss_fn`` built as the constructor builds them (:175-188).  The
reference is imported as gen_golden.py does (stub modules, PYTORCH_JIT=0); ``kornia.filters.blur_pool2d`` and
``kornia.filters.spatial_gradient`` are ``tests/reg_losses_ref.blur_pool32`` / ``spatial_gradient32``, the restated compositions, so the
fixture pins the pyramid loop, the masks, the nearest resize, every mean and the cocktail to the reference's code, not to our reading of it.
Inputs are closed forms (``reg_losses_ref.inputs``); the fixture holds results only: per case the nine values in ``reg_losses_ref.KEYS``
order.

    python tests/golden/gen_golden_reg_losses.py       # rewrites tests/golden/g18_reg_losses.npz
"""
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

from gen_golden import _stub, import_reference, save

B, H, W, K = 2, 24, 32, 2
SCALES = {"all": (0, 1, 2, 3), "s0": (0,)}


def main():
    import reg_losses_ref as R

    import_reference()
    for name in ("pytorch_lightning", "moviepy", "moviepy.editor"):
        _stub(name)
    sys.modules["pytorch_lightning"].LightningModule = torch.nn.Module
    sys.modules["moviepy"].editor = sys.modules["moviepy.editor"]
    sys.modules["kornia.filters"].blur_pool2d = R.blur_pool32
    sys.modules["kornia.filters"].spatial_gradient = R.spatial_gradient32
    from experiment_modules.depth_model import DepthModel
    from losses import MSGradientLoss, MVDepthLoss, NormalsLoss, ScaleInvariantLoss

    out = {"shape": np.array([B, H, W, K])}
    for dataset in ("scannet", "hypersim"):
        for sname, scales in SCALES.items():
            cur, src, outputs = R.inputs(B, H, W, K, scales=scales)
            shim = types.SimpleNamespace(run_opts=types.SimpleNamespace(dataset=dataset), si_loss=ScaleInvariantLoss(), abs_loss=torch.nn.L1Loss(),
                                         grad_loss=MSGradientLoss(), normals_loss=NormalsLoss(), mv_depth_loss=MVDepthLoss(H, W))
            shim.ms_loss_fn = shim.abs_loss
            with torch.no_grad():
                losses = DepthModel.compute_losses(shim, cur, src, outputs)
            vals = np.array([float(losses[k]) for k in R.KEYS], dtype=np.float32)
            mine = R.compute_losses32(cur, src, outputs, dataset == "hypersim")
            assert np.array_equal(vals, np.array([float(mine[k]) for k in R.KEYS], dtype=np.float32)), (dataset, sname)
            assert np.isfinite(vals).all(), (dataset, sname, vals)
            out[f"{dataset}_{sname}"] = vals
            print(f"  {dataset} {sname}: " + " ".join(f"{k}={v:.7g}" for k, v in zip(R.KEYS, vals)))
    save("g18_reg_losses", **out)


if __name__ == "__main__":
    main()
