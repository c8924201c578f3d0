#!/usr/bin/env python
"""Generate tests/golden/g15_temporal.npz from the parts of the REFERENCE's temporal evaluation that run without pytorch3d
(utils/binary_metrics_utils.py:247-329): ``TemporalEvaluator.mask_prediction_edges``, ``compute_vertex_occlusion_changes`` on seeded
(T, V) histories, and ``Pytorch3DRasterizer.create_plane_from_camera`` with a recording stand-in for ``Meshes``.  Same stubs and
``.cuda()`` patch as gen_golden.py, and like it runs only where the reference checkout it imports is present.  Inputs come from implicit_depth_amd.synthetic;
only outputs are stored, and of the 2 M-row plane only a strided subset.

    python tests/golden/gen_golden_temporal.py
"""
import types

import numpy as np
import torch

import gen_golden as gg

VERT_STRIDE = 4099                      # plane vertices kept: every 4099th (256 of 1 048 576)
FACE_ROWS = [0, 1, 2, 3, 2044, 2045, 2046, 2047, 1046528, 1046529, 2093056, 2093057]
HISTORIES = [(6, 500, 1), (2, 64, 2), (30, 2000, 3)]  # (T, V, seed)
PLANES = [(0, 2.0), (1, 3.25)]          # (synthetic.plane_pose index, distance)


class RecordedMeshes:
    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces


def main():
    gg.import_reference()
    gg._stub_pytorch3d()
    import implicit_depth_amd.synthetic as syn
    import utils.binary_metrics_utils as bmu

    torch.set_grad_enabled(False)
    bmu.Meshes = RecordedMeshes
    bmu.RasterizationSettings = lambda **k: None
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        print("G15 temporal evaluation")
        for h, w in ((24, 32), (9, 20), (8, 8)):
            p = syn.randn((1, 1, h, w), 80, "edge_pred").clone()
            bmu.TemporalEvaluator.mask_prediction_edges(p)
            out[f"edges_{h}x{w}"] = p
        for T, V, seed in HISTORIES:
            ev = bmu.TemporalEvaluator()
            ev.rasterizer = types.SimpleNamespace(gt_vertex_predictions=list(syn.vertex_histories(T, V, seed)))
            ev.compute_vertex_occlusion_changes()
            ev.compute_vertex_occlusion_changes()  # the totals accumulate
            out[f"changes_{T}x{V}_s{seed}"] = np.array([float(ev.total_diffs), float(ev.total_verts)])
        r = bmu.Pytorch3DRasterizer(height=192, width=256)
        for i, dist in PLANES:
            r.create_plane_from_camera(syn.plane_pose(i), distance=torch.tensor(dist))
            v, f = r.mesh.verts[0], r.mesh.faces[0]
            assert v.shape == (1024 * 1024, 3) and f.shape == (2 * 1023 * 1023, 3)
            out[f"plane{i}_verts"] = v[::VERT_STRIDE]
            out[f"plane{i}_vert_sum"] = v.double().sum(0)
            out[f"plane{i}_face_rows"] = f[FACE_ROWS]
            out[f"plane{i}_face_colsum"] = f.long().sum(0)
        out["face_rows_index"] = np.array(FACE_ROWS)
        out["vert_stride"] = np.array(VERT_STRIDE)
    finally:
        torch.Tensor.cuda = cuda
    gg.save("g15_temporal", **out)


if __name__ == "__main__":
    main()
