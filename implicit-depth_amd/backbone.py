"""The ResNet18 stem of the matching encoder: ``conv1, bn1, relu, maxpool, layer1`` of
``antialiased_cnns.resnet18(pretrained, filter_size=4, pool_only=True)`` (antialiased-cnns 0.3, the version the
reference pins in binarydepth_env.yml; used by reference modules/networks.py:236-287).

These are fresh torch modules with that package's architecture and state-dict layout, written from its published
source: the package itself is not a dependency of this project, so the definitions could not be checked against it
here.  Every kernel test pins the gfx950 stem against torch's composition of exactly these modules; if a difference
from the real package turns up, only this file changes.

Layout (index = position in ``ResnetMatchingEncoder.net``):

    net[0]  Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    net[1]  BatchNorm2d(64)
    net[2]  ReLU(inplace=True)
    net[3]  Sequential(MaxPool2d(kernel_size=2, stride=1), BlurPool(64))     (``net.3.1.filt``)
    net[4]  Sequential(BasicBlock(64, 64), BasicBlock(64, 64))                 (torchvision attribute names)

``stem_is_native_eligible`` is the duck-typed check the native path (csrc/stem.hip + the Winograd 3x3 kernels) uses; it
accepts these modules and the real package's alike.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn.functional as F
from torch import nn

BLUR_TAPS = (1.0, 3.0, 3.0, 1.0)  # binomial [1, 3, 3, 1]: filt = outer(a, a) / 64


def blur_filter(channels: int) -> torch.Tensor:
    a = torch.tensor(BLUR_TAPS, dtype=torch.float32)
    filt = a[:, None] * a[None, :]
    filt = filt / filt.sum()
    return filt[None, None].repeat(channels, 1, 1, 1)


class BlurPool(nn.Module):
    """Anti-aliased downsampling: ReflectionPad2d((1, 2, 1, 2)) then a depthwise stride-2 conv with the 4x4 binomial
    ``filt`` (a persistent buffer of shape (channels, 1, 4, 4))."""

    def __init__(self, channels: int, filt_size: int = 4, stride: int = 2):
        super().__init__()
        if filt_size != 4:
            raise ValueError("only the filt_size=4 BlurPool of resnet18(filter_size=4) is provided")
        self.filt_size = filt_size
        self.stride = stride
        self.channels = channels
        self.pad_off = 0
        self.pad_sizes = [1, 2, 1, 2]  # left, right, top, bottom
        self.off = 0
        self.register_buffer("filt", blur_filter(channels))
        self.pad = nn.ReflectionPad2d(self.pad_sizes)

    def forward(self, x):
        return F.conv2d(self.pad(x), self.filt, stride=self.stride, groups=x.shape[1])


def _conv3x3(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    """torchvision / antialiased-cnns ResNet BasicBlock with stride 1 and no downsample (layer1 of resnet18)."""

    expansion = 1

    def __init__(self, inplanes: int = 64, planes: int = 64):
        super().__init__()
        self.conv1 = _conv3x3(inplanes, planes)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        self.stride = 1

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + x)


def resnet18_stem() -> list:
    """The five modules conv1, bn1, relu, maxpool, layer1 (randomly initialised like torchvision's ResNet)."""
    conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    bn1 = nn.BatchNorm2d(64)
    maxpool = nn.Sequential(nn.MaxPool2d(kernel_size=2, stride=1), BlurPool(64, filt_size=4, stride=2))
    layer1 = nn.Sequential(BasicBlock(64, 64), BasicBlock(64, 64))
    for m in [conv1] + [c for blk in layer1 for c in (blk.conv1, blk.conv2)]:
        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return [conv1, bn1, nn.ReLU(inplace=True), maxpool, layer1]


# --- eligibility of the native stem -----------------------------------------------------------------------------------------
def _bn_ok(bn, c: int = 64) -> bool:
    return (isinstance(bn, nn.BatchNorm2d) and bn.num_features == c and not bn.training and bn.track_running_stats
            and bn.running_mean is not None and bn.running_var is not None)


def _conv_ok(conv, cin, cout, k, stride, pad) -> bool:
    return (isinstance(conv, nn.Conv2d) and conv.in_channels == cin and conv.out_channels == cout and conv.kernel_size == (k, k)
            and conv.stride == (stride, stride) and conv.padding == (pad, pad) and conv.dilation == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros")


def _blur_ok(bp) -> bool:
    filt = getattr(bp, "filt", None)
    if not (isinstance(bp, nn.Module) and getattr(bp, "filt_size", None) == 4 and getattr(bp, "stride", None) == 2
            and getattr(bp, "channels", None) == 64 and list(getattr(bp, "pad_sizes", [])) == [1, 2, 1, 2]
            and isinstance(getattr(bp, "pad", None), nn.ReflectionPad2d) and isinstance(filt, torch.Tensor)
            and tuple(filt.shape) == (64, 1, 4, 4)):
        return False
    return bool(torch.equal(filt.detach().float().cpu(), blur_filter(64)))


def _block_ok(blk) -> bool:
    return (_conv_ok(getattr(blk, "conv1", None), 64, 64, 3, 1, 1) and _bn_ok(getattr(blk, "bn1", None))
            and _conv_ok(getattr(blk, "conv2", None), 64, 64, 3, 1, 1) and _bn_ok(getattr(blk, "bn2", None))
            and getattr(blk, "downsample", None) is None and isinstance(getattr(blk, "relu", None), nn.ReLU))


def stem_is_native_eligible(modules: Sequence[nn.Module]) -> bool:
    """True when ``modules`` (conv1, bn1, relu, maxpool, layer1) are exactly the resnet18(filter_size=4, pool_only=True)
    stem the native path computes: shapes and hyper-parameters as listed in the module docstring, ``filt`` the binomial,
    every BatchNorm in eval mode.  Duck-typed: no class of the third-party package is imported or named."""
    try:
        mods = list(modules)
    except TypeError:
        return False
    if len(mods) != 5:
        return False
    conv1, bn1, relu, pool, layer1 = mods
    if not (_conv_ok(conv1, 3, 64, 7, 2, 3) and _bn_ok(bn1) and isinstance(relu, nn.ReLU)):
        return False
    if not (isinstance(pool, nn.Sequential) and len(pool) == 2 and isinstance(pool[0], nn.MaxPool2d)):
        return False
    mp = pool[0]
    as2 = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if not (as2(mp.kernel_size) == (2, 2) and as2(mp.stride) == (1, 1) and as2(mp.padding) == (0, 0) and as2(mp.dilation) == (1, 1)
            and not mp.ceil_mode and _blur_ok(pool[1])):
        return False
    return isinstance(layer1, nn.Sequential) and len(layer1) == 2 and all(_block_ok(b) for b in layer1)


def stem_bns(modules: Sequence[nn.Module]) -> list:
    """The five BatchNorms of the stem: bn1, layer1[0].bn1, layer1[0].bn2, layer1[1].bn1, layer1[1].bn2."""
    mods = list(modules)
    return [mods[1]] + [bn for blk in mods[4] for bn in (blk.bn1, blk.bn2)]
