"""The native ResNet18 matching stem, host side (no GPU): the modules of backbone.py (architecture, state-dict keys, BlurPool),
stem_is_native_eligible, the opt-in checks of ResnetMatchingEncoder / dropin, and the size query of the C entry idh_matching_stem_*."""
import contextlib
import ctypes
import io
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import ROOT

STEM_KEYS = (["net.0.weight"] + [f"net.1.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")] + ["net.3.1.filt"]
             + [f"net.4.{b}.{c}" for b in (0, 1) for c in ["conv1.weight"] + [f"bn1.{k}" for k in ("weight", "bias", "running_mean", "running_var",
                                                                                                    "num_batches_tracked")]
                + ["conv2.weight"] + [f"bn2.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]])
HEAD_KEYS = ["net.5.weight", "net.5.bias", "net.8.weight", "net.8.bias"]


def _stem(eval_mode=True):
    from implicit_depth_amd import backbone

    mods = backbone.resnet18_stem()
    if eval_mode:
        for m in mods:
            m.eval()
    return mods


def test_encoder_without_backbone_has_the_reference_key_set():
    from implicit_depth_amd import networks as net

    e = net.ResnetMatchingEncoder(None)
    assert e.native_stem
    assert sorted(e.state_dict()) == sorted(STEM_KEYS + HEAD_KEYS)
    assert e.net[3][1].filt.shape == (64, 1, 4, 4)
    # passing the modules keeps the torch-module behaviour
    e2 = net.ResnetMatchingEncoder(_stem(), 16)
    assert not e2.native_stem and sorted(e2.state_dict()) == sorted(e.state_dict())


def test_module_attributes_follow_the_package():
    mods = _stem()
    conv1, bn1, relu, pool, layer1 = mods
    assert (conv1.kernel_size, conv1.stride, conv1.padding, conv1.bias) == ((7, 7), (2, 2), (3, 3), None)
    bp = pool[1]
    assert (bp.filt_size, bp.stride, bp.channels, list(bp.pad_sizes)) == (4, 2, 64, [1, 2, 1, 2])
    assert isinstance(bp.pad, nn.ReflectionPad2d) and isinstance(pool[0], nn.MaxPool2d)
    assert (pool[0].kernel_size, pool[0].stride) == (2, 1)
    assert len(layer1) == 2 and all(b.downsample is None and b.conv1.stride == (1, 1) for b in layer1)


@pytest.mark.parametrize("hw", [(8, 8), (9, 11), (24, 32), (25, 33)])
def test_blurpool_matches_independent_restatement(hw):
    from implicit_depth_amd import backbone

    a = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    filt = (a[:, None] * a[None, :]) / 64.0
    bp = backbone.BlurPool(64).double()
    assert torch.equal(bp.filt, filt[None, None].repeat(64, 1, 1, 1))
    x = torch.randn(2, 64, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1]))
    ref = F.conv2d(F.pad(x, (1, 2, 1, 2), mode="reflect"), filt[None, None].expand(64, 1, 4, 4), stride=2, groups=64)
    assert torch.allclose(bp(x), ref, rtol=0, atol=1e-12)
    assert ref.shape[-2:] == ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)


def test_native_eligibility():
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import backbone

    ok = _stem()
    assert backbone.stem_is_native_eligible(ok)
    s = syn.StubResnetStem()
    assert not backbone.stem_is_native_eligible([s.conv1, s.bn1, s.relu, s.maxpool, s.layer1])
    train = _stem()
    train[4][1].bn2.train()
    assert not backbone.stem_is_native_eligible(train)
    bad_filt = _stem()
    with torch.no_grad():
        bad_filt[3][1].filt[3, 0, 1, 2] += 1e-3
    assert not backbone.stem_is_native_eligible(bad_filt)
    strided = _stem()
    strided[4][0].conv1 = nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False)
    assert not backbone.stem_is_native_eligible(strided)
    assert not backbone.stem_is_native_eligible(ok[:4])


def test_training_mode_stem_is_refused_before_any_launch():
    from implicit_depth_amd import _lib
    from implicit_depth_amd import networks as net

    e = net.ResnetMatchingEncoder(None)  # freshly built modules are in training mode
    with pytest.raises(_lib.IdhError, match="inference-only"):
        e(torch.zeros(1, 3, 32, 32))


def test_dropin_refuses_an_ineligible_stem():
    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import _lib, dropin
    from implicit_depth_amd import networks as net

    m = nn.Module()
    s = syn.StubResnetStem()
    m.matching_model = net.ResnetMatchingEncoder([s.conv1, s.bn1, s.relu, s.maxpool, s.layer1], 16)
    with pytest.raises(_lib.IdhError, match="native_matching_stem"):
        dropin.convert(m, native_matching_stem=True)


def test_matching_stem_sizes_and_refusals():
    from implicit_depth_amd import _lib, net_abi

    L = _lib.lib()
    e_keep = []
    from implicit_depth_amd import networks as net

    enc = net.ResnetMatchingEncoder(None).eval()
    sp = net_abi.stem_params(enc.net[:5], e_keep)
    sz = net_abi.NetSizes()
    rc = L.idh_matching_stem_sizes(ctypes.byref(sp), 256, ctypes.byref(net_abi.nchw(None, 3, 384, 512)),
                                   ctypes.byref(net_abi.nhwc(None, 64, 96, 128, 64)), ctypes.byref(sz))
    assert rc == 0
    d = sz.as_dict()
    assert d["ops"] == 5 and d["wino4"] == 4  # stem pass + four layer1 convs on conv3x3_wino4_k
    assert d["launches"] == 5
    assert d["weight_floats"] >= L.idh_stem_weight_floats() + 4 * (64 * 64 * 9 + 64)
    assert d["workspace_floats"] >= 2 * 256 * 96 * 128 * 64
    assert L.idh_stem_weight_floats() == 4 * 42 * 64 + 64
    rc = L.idh_matching_stem_sizes(ctypes.byref(sp), 1, ctypes.byref(net_abi.nchw(None, 3, 8, 8)), ctypes.byref(net_abi.nhwc(None, 64, 2, 2, 64)),
                                   ctypes.byref(sz))
    assert rc == 0 and sz.wino4 == 4  # the same kernels at every size: batch-size-independent results
    for H, W in ((7, 512), (384, 7), (6, 6)):
        out = net_abi.nhwc(None, 64, max(((H + 1) // 2) // 2, 1), max(((W + 1) // 2) // 2, 1), 64)
        assert L.idh_matching_stem_sizes(ctypes.byref(sp), 4, ctypes.byref(net_abi.nchw(None, 3, H, W)), ctypes.byref(out), ctypes.byref(sz)) == -1
    # wrong output size, wrong channel count
    assert L.idh_matching_stem_sizes(ctypes.byref(sp), 4, ctypes.byref(net_abi.nchw(None, 3, 64, 64)),
                                     ctypes.byref(net_abi.nhwc(None, 64, 15, 16, 64)), ctypes.byref(sz)) == -1
    assert L.idh_matching_stem_sizes(ctypes.byref(sp), 4, ctypes.byref(net_abi.nchw(None, 4, 64, 64)),
                                     ctypes.byref(net_abi.nhwc(None, 64, 16, 16, 64)), ctypes.byref(sz)) == -1
    # the op itself: validation without a launch (idh_count_launches)
    from implicit_depth_amd import nhwc

    op = nhwc.Op()
    op.kind, op.N = nhwc.OP_STEM, 2
    s = op.src[0]
    s.in_, s.w, s.H, s.W, s.Cin = 0x1000, 0x2000, 64, 64, 3
    op.out, op.out_cs, op.Ho, op.Wo, op.Cout = 0x3000, 64, 16, 16, 64
    assert L.idh_count_launches(ctypes.byref(op), 1) == 1
    s.H = 7
    assert L.idh_count_launches(ctypes.byref(op), 1) == -1


# ---- the reference's own BDModel with the stem modules of backbone.py (needs the reference tree; child interpreter, PYTORCH_JIT=0) ----
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")
def test_convert_reference_model_with_native_stem_keeps_state_dict():
    env = dict(os.environ, PYTORCH_JIT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "native stem converted ok" in r.stdout, r.stdout


def _child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_dropin_reference_cpu import _import_reference

    BDModel, DepthModel, Options = _import_reference()
    import antialiased_cnns

    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import backbone, dropin

    class _Resnet(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1, self.relu, self.maxpool, self.layer1 = backbone.resnet18_stem()

    antialiased_cnns.resnet18 = lambda *a, **kw: _Resnet()
    o = Options()
    o.image_width, o.image_height = 128, 96
    o.matching_num_depth_bins = 16
    o.feature_volume_type = "mlp_feature_volume"
    o.model_num_views = 8
    o.binary_loss_positive_weight = 1.0
    o.bd_edge_regularision = False
    with contextlib.redirect_stdout(io.StringIO()):
        m = BDModel(o)
    syn.fill_state_dict(m, seed=5)
    m.eval()
    keys = [k for k in m.state_dict() if k.startswith("matching_model.")]
    assert sorted(keys) == sorted("matching_model." + k for k in STEM_KEYS + HEAD_KEYS), keys
    before = {k: v.clone() for k, v in m.state_dict().items()}
    dropin.convert(m, native_matching_stem=True)
    after = m.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    hot = dropin.hot_path_of(m, native_matching_stem=True)
    assert hot.matching_model is m.matching_model
    print("native stem converted ok", len(before), "tensors")


if __name__ == "__main__":
    _child()
