#!/usr/bin/env python
"""Golden of the sparse-ray occlusion path: the REFERENCE's ``BDModel.run_mlp_train`` (experiment_modules/bd_model.py:313-393) called
unbound on a shim that carries what it reads - ``run_opts(full_depth_supervision=False, bd_edge_regularision=False, use_prior=False)`` and
``binary_mlp = BinaryMLPNetwork([64, 64, 128, 256])``.  The reference is imported as gen_golden.py does (stub modules, PYTORCH_JIT=0).
Inputs and weights come from ``tests/ray_query_ref.golden_inputs`` / ``golden_net`` (synthetic.py seeds); the fixture holds the rays, the
depths and pred_0..3 only.

    python tests/golden/gen_golden_rays.py       # rewrites tests/golden/ray_query.npz
"""
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch

from gen_golden import _stub, import_reference, save


def main():
    import_reference()
    for name in ("pytorch_lightning", "moviepy", "moviepy.editor"):
        _stub(name)
    sys.modules["pytorch_lightning"].LightningModule = torch.nn.Module
    sys.modules["moviepy"].editor = sys.modules["moviepy.editor"]
    sys.modules["kornia"].filters.sobel = None
    from experiment_modules.bd_model import BDModel
    from modules.networks import BinaryMLPNetwork

    import ray_query_ref as Q

    feats, rays, depths = Q.golden_inputs()
    net = Q.golden_net(BinaryMLPNetwork).eval()
    shim = types.SimpleNamespace(run_opts=types.SimpleNamespace(full_depth_supervision=False, bd_edge_regularision=False, use_prior=False),
                                 binary_mlp=net)
    gh, gw = Q.GOLDEN_GRID
    inputs = {"depth_b1hw": torch.ones(Q.GOLDEN_B, 1, gh, gw), "sampled_rays": rays.clone(),  # (run_mlp_train normalises its rays in place)
              "sampled_depths": depths.clone()}
    with torch.no_grad():
        out = BDModel.run_mlp_train(shim, inputs, {f"feature_s{s}_b1hw": f for s, f in feats.items()})
    save("ray_query", rays=rays, depths=depths, **{f"pred_{s}": out[f"pred_{s}"] for s in range(4)})
    for s in range(4):
        print(f"  pred_{s}", tuple(out[f"pred_{s}"].shape))


if __name__ == "__main__":
    main()
