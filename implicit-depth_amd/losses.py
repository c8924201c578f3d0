"""The loss modules of the reference's ``losses.py`` that ``DepthModel`` holds, forward value only, on the gfx950 kernels
(csrc/reg_losses.hip, csrc/mv_consistency.hip; contracts: include/idh_geometry.h), without kornia.
``dropin.convert(model, native_losses=True)`` puts them in place of ``grad_loss``, ``normals_loss`` and ``mv_depth_loss``, so that the
reference's own ``compute_losses`` scores a validation batch under ``torch.no_grad()``.  ``evaluation.reg_val_losses`` is the fused form
of the whole of ``compute_losses``.  There is no backward pass: an input that requires grad raises instead of returning a value that
silently carries no gradient."""
import torch
from torch import nn

from . import _lib
from .evaluation import _forward_only, reg_losses_call
from .geometry import MVDepthLoss

__all__ = ["MSGradientLoss", "NormalsLoss", "MVDepthLoss"]


class MSGradientLoss(nn.Module):
    """The reference's ``MSGradientLoss`` (losses.py:77-101): the sum over ``num_scales`` levels of a ``blur_pool2d`` pyramid of the mean
    absolute difference of the Sobel gradients where the ground truth's is finite.  One launch per level and a finalise; 1 <= num_scales
    <= 4."""

    def __init__(self, num_scales: int = 4):
        super().__init__()
        if not 1 <= int(num_scales) <= 4:
            raise _lib.IdhError(f"num_scales must be 1 .. 4, got {num_scales}")
        self.num_scales = int(num_scales)

    def forward(self, depth_gt: torch.Tensor, depth_pred: torch.Tensor) -> torch.Tensor:
        _forward_only("MSGradientLoss", (("depth_gt", depth_gt), ("depth_pred", depth_pred)))
        return reg_losses_call(depth_gt, depth_pred, terms=_lib.REG_TERM_GRAD, num_scales=self.num_scales)[2].float()


class NormalsLoss(nn.Module):
    """The reference's ``NormalsLoss`` (losses.py:119-140): the mean of ``0.5 (1 - n_gt . n_pred)`` over the pixels at which all six
    components are finite; NaN when there is none."""

    def forward(self, normals_gt_b3hw: torch.Tensor, normals_pred_b3hw: torch.Tensor) -> torch.Tensor:
        _forward_only("NormalsLoss", (("normals_gt_b3hw", normals_gt_b3hw), ("normals_pred_b3hw", normals_pred_b3hw)))
        return reg_losses_call(normals_gt=normals_gt_b3hw, normals_pred=normals_pred_b3hw, terms=_lib.REG_TERM_NORMALS)[4].float()
