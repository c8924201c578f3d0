#!/usr/bin/env python
"""Golden G17 of the edge mask and the validation losses: the REFERENCE's own ``get_edge_mask`` (utils/generic_utils.py:286-292), the
dataset's ``GenericMVSDataset.get_edge_mask`` (datasets/generic_mvs_dataset.py:650-658) and ``BDModel.compute_binary_losses``
(experiment_modules/bd_model.py:451-495) called unbound on a shim that carries what it reads - ``run_opts(bd_edge_regularision,
bd_regularisation_weight)``, ``bce_loss`` and ``sigmoid`` as the constructor builds them (:100-102).  The reference is imported as
gen_golden.py does (stub modules, PYTORCH_JIT=0); ``kornia.filters.sobel`` is ``tests/edge_mask_ref.sobel32``, the restated composition, so
the fixture pins the quantile, the comparison, the dilation and the loss to the reference's code, not to our reading of it.
Inputs are closed forms (``normals_ref.field``, ``edge_mask_ref.with_zero_patch`` / ``loss_inputs``); the fixture holds results only.

    python tests/golden/gen_golden_edge.py       # rewrites tests/golden/g17_edge.npz
"""
import importlib.util
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

from gen_golden import REF, _stub, import_reference, save

H, W = 24, 32
REG_WEIGHTS = (0.0, 0.5)


def main():
    import edge_mask_ref as E

    import_reference()
    for name in ("pytorch_lightning", "moviepy", "moviepy.editor"):
        _stub(name)
    sys.modules["pytorch_lightning"].LightningModule = torch.nn.Module
    sys.modules["moviepy"].editor = sys.modules["moviepy.editor"]
    sys.modules["kornia"].filters.sobel = E.sobel32
    from experiment_modules.bd_model import BDModel
    from utils.generic_utils import get_edge_mask

    # the reference's datasets/ is a namespace package that an installed `datasets` distribution shadows: load the module by its path
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].ColorJitter = lambda *a, **k: None  # (a default argument of the class's constructor)
    spec = importlib.util.spec_from_file_location("ref_generic_mvs_dataset", os.path.join(REF, "datasets", "generic_mvs_dataset.py"))
    mvs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mvs)
    GenericMVSDataset = mvs.GenericMVSDataset

    out = {"shape": np.array([2, H, W])}
    plain = E.field(2, H, W)
    for name, depth in (("plain", plain), ("patch", E.with_zero_patch(plain))):
        for dil in (True, False):
            m = get_edge_mask(depth, dilate=dil)
            assert set(np.unique(m.numpy())) <= {0.0, 1.0}
            out[f"{name}_mask_dilate{int(dil)}"] = np.packbits(m.numpy().astype(bool))
        ds = torch.stack([GenericMVSDataset.get_edge_mask(d) for d in depth])  # (2,1,H,W) bool: 0.975, no dilation
        out[f"{name}_dataset_mask"] = np.packbits(ds.numpy())
        print(f"  {name}: {int(get_edge_mask(depth).sum())} mask pixels, {int(ds.sum())} in the dataset's variant")

    pred, rendered, depth = E.loss_inputs(2, 3, H, W)
    edge = get_edge_mask(depth)
    cases = {"edge": (True, edge), "noedge": (False, None), "emptyreg": (True, torch.zeros_like(edge))}
    for cname, (flag, em) in cases.items():
        for wgt in REG_WEIGHTS:
            shim = types.SimpleNamespace(run_opts=types.SimpleNamespace(bd_edge_regularision=flag, bd_regularisation_weight=wgt),
                                         bce_loss=torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.tensor((1.0,)).float()),
                                         sigmoid=torch.nn.Sigmoid())
            inputs = {"rendered_depth": rendered, "depth_b1hw": depth}
            if em is not None:
                inputs["edge_mask"] = em
            with torch.no_grad():
                losses = BDModel.compute_binary_losses(shim, inputs, {"pred_0": pred}, "val")
            vals = np.array([losses["binary_loss/0"].item(), losses["reg_loss/0"].item(), losses["binary_loss"].item()], dtype=np.float32)
            out[f"loss_{cname}_w{wgt}"] = vals
            print(f"  loss {cname} w={wgt}: {vals}")
    mask = (depth > 0) * (rendered > 0)
    out["loss_counts"] = np.array([int(mask.sum()), int((edge * mask).bool().sum())])
    out["loss_edge_mask"] = np.packbits(edge.numpy().astype(bool))
    save("g17_edge", **out)


if __name__ == "__main__":
    main()
