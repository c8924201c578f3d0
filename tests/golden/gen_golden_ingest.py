"""Writes tests/golden/g_ingest.npz: what the reference's frame loader produces, made with Pillow and torch on the CPU.

The reference's ``read_image_file`` (utils/generic_utils.py:166-214) needs torchvision; the three lines it stands for are stated here:

    img = img.resize((width, height), resample=mode)      Image.resize            (generic_utils.py:210)
    img = TF.to_tensor(img).float()                        u8 -> float32 / 255     (:212)
    image = TF.normalize(image, mean, std)                 .sub_(mean).div_(std)   (:149-152)

and for depths ``img.resize(..., NEAREST)`` of an I;16 image, ``* 1e-3`` and the validity masks (datasets/scannet_dataset.py:515-530).
Stored: the seeded uint8 / uint16 inputs, Pillow's resized bytes for both filters, the depth triples, and the two float tables
(``to_tensor`` of every byte, ``normalize`` of every byte per channel) from which the float images follow exactly.

    python tests/golden/gen_golden_ingest.py
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ingest_ref as ref  # noqa: E402

PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def to_tensor(u8_hwc):  # torchvision.transforms.functional.to_tensor for a uint8 RGB image
    return torch.from_numpy(np.ascontiguousarray(u8_hwc)).permute(2, 0, 1).contiguous().float().div(255)


def normalize(t):  # torchvision.transforms.functional.normalize
    mean = torch.as_tensor((0.485, 0.456, 0.406), dtype=torch.float32)[:, None, None]
    std = torch.as_tensor((0.229, 0.224, 0.225), dtype=torch.float32)[:, None, None]
    return t.clone().sub_(mean).div_(std)


def main():
    out = {}
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (1, 256, 3))
    out["to_tensor_table"] = to_tensor(ramp)[:, 0].numpy()            # (3,256), rows equal
    out["normalize_table"] = normalize(to_tensor(ramp))[:, 0].numpy()  # (3,256)
    assert np.array_equal(out["to_tensor_table"], ref.to_tensor(ramp)[:, 0])
    assert np.array_equal(out["normalize_table"], ref.normalize(ref.to_tensor(ramp))[:, 0])
    for i, (name, src, dst) in enumerate(ref.COLOR_CASES):
        x = ref.color_input(name, src, 100 + i)
        out[f"{name}_in"] = x
        for fname, pf in PIL_FILTER.items():
            if src == dst:
                got = x.copy()  # generic_utils.py:202: no resize when the size already matches
            else:
                got = np.stack([np.asarray(Image.fromarray(f).resize((dst[1], dst[0]), resample=pf)) for f in x])
            assert np.array_equal(got, ref.load_color(x, dst, ref.FILTER_NAMES[fname])[1]), (name, fname)
            f32 = torch.stack([normalize(to_tensor(f)) for f in got]).numpy()
            assert np.array_equal(f32, ref.load_color(x, dst, ref.FILTER_NAMES[fname])[0]), (name, fname)
            out[f"{name}_{fname}_u8"] = got
    name, fname = ref.WIDE_INTERMEDIATE_CASE
    src, dst = next((s, d) for n, s, d in ref.COLOR_CASES if n == name)
    wide = np.stack([ref.resize_u8_wide_intermediate(f, dst, ref.FILTER_NAMES[fname]) for f in out[f"{name}_in"]])
    assert not np.array_equal(wide, out[f"{name}_{fname}_u8"])
    for i, (name, src, dst) in enumerate(ref.DEPTH_CASES):
        d = ref.depth_input(src, 200 + i)
        out[f"{name}_in"] = d
        r = d if dst is None else np.stack([np.asarray(Image.fromarray(f).resize((dst[1], dst[0]), resample=Image.NEAREST)) for f in d])
        assert r.dtype == np.uint16
        depth = torch.from_numpy(r.astype(np.int32))[:, None].float() * 1e-3
        mask_b = (depth > 1e-3) & (depth < 10.0)
        mask = mask_b.float()
        depth[~mask_b] = torch.tensor(np.nan)
        out[f"{name}_depth"], out[f"{name}_mask"], out[f"{name}_mask_b"] = depth.numpy(), mask.numpy(), mask_b.numpy()
        rd, rm, rb = ref.load_depth(d, dst)
        assert np.array_equal(rd, depth.numpy(), equal_nan=True) and np.array_equal(rm, mask.numpy()) and np.array_equal(rb, mask_b.numpy()), name
    path = os.path.join(HERE, "g_ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
