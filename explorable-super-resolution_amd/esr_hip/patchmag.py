"""Host side of the patch-magnitude Z objective (reference codes/Z_optimization.py:391-394, 450-455, 717-722): what the GUI's "increase /
decrease variance" tool sends with its special-behaviour button checked, 'local_Mag_increase' / 'local_Mag_decrease'.

* The patch set is ReturnPatchExtractionMat(image_mask, 7, patches_overlap=0.5): the 7 x 7 windows inside the opened mask that survive the
  greedy half-overlap scan (esr_hip.kde.patch_extraction_indexes, the reference's slot quirk included) - one corner in 16 to 27.
* desired_patches: with Q[:, p] the 49 values of patch p of g0 = mean_c I0 (I0 the clamped initial output, image 0),
      m_p = mean(Q[:, p]),  s_p = max(std_unbiased(Q[:, p]), 1/255),  desired[:, p] = (Q[:, p] - m_p) / s_p * (s_p + sign * increment) + m_p
  in float32 and in the reference's order of operations; a negative s_p - increment is kept as the reference keeps it.
* patch_mag(x, spec) -> [B]: mean over the 49 x P entries of (patches(mean_c clamp(x_b, 0, 1)) - desired)^2.  GPU: csrc/esr_patchmag.hip
  (an int32 map of patch ordinals per corner, a gather-form backward without atomics); CPU: the defining torch expression.
"""
import numpy as np
import torch

from . import _lib
from ._image import PATCH, DeviceCopies, detach_f32, to_numpy
from ._lib import check
from .act import stream_ptr
from .kde import patch_extraction_indexes

OVERLAP = 0.5        # desired_overlap of the 'local' names without 'STD' (reference :392)
STD_FLOOR = 1 / 255


def desired_patches(initial_first, patch_indexes, increment, sign):
    """[49, P] float32, the reference's self.desired_patches (:451-454).  initial_first: [C, H, W], the clamped initial output's image 0;
    patch_indexes: [P, 49] flat pixel indexes; sign: +1 ('increase') or -1 ('decrease')."""
    g0 = initial_first.detach().float().cpu().mean(dim=0).reshape(-1)
    Q = g0[torch.as_tensor(patch_indexes, dtype=torch.int64)].t()                        # [49, P], as the sparse product's view([49, -1])
    s = torch.max(torch.std(Q, dim=0, keepdim=True), torch.tensor(STD_FLOOR))
    m = torch.mean(Q, dim=0, keepdim=True)
    return ((Q - m) / s * (s + increment * (1 if sign > 0 else -1)) + m).contiguous()


class MagSpec(DeviceCopies):
    """the patch set and the desired patches of one edit, built once and reused every iteration (device copies cached).
    image_mask None: the whole H x W image.  initial_first: [C, H, W], image 0 of the clamped initial output.  ValueError when no patch fits."""

    def __init__(self, image_mask, H, W, initial_first, increment, sign):
        if image_mask is None:
            m = np.ones((H, W), dtype=np.float32)
        else:
            m = to_numpy(image_mask)
        self.H, self.W = m.shape
        if (H is not None and H != self.H) or (W is not None and W != self.W):
            raise ValueError('patch magnitude: image mask %s for a %s x %s image' % (m.shape, H, W))
        self.patches = patch_extraction_indexes(m, PATCH, OVERLAP) if min(m.shape) >= PATCH else np.zeros((0, PATCH * PATCH), np.int64)
        if self.patches.shape[0] == 0:
            raise ValueError('patch magnitude: the image mask holds no %d x %d patch' % (PATCH, PATCH))
        if tuple(initial_first.shape[-2:]) != (self.H, self.W) or initial_first.dim() != 3:
            raise ValueError('patch magnitude: initial image %s, expected [C, %d, %d]' % (tuple(initial_first.shape), self.H, self.W))
        # the ordinal of the selected window per top-left corner, -1 elsewhere
        self.corner_index = np.full((self.H - PATCH + 1, self.W - PATCH + 1), -1, dtype=np.int32)
        y0, x0 = np.divmod(self.patches[:, 0], self.W)
        self.corner_index[y0, x0] = np.arange(self.P, dtype=np.int32)
        self.increment, self.sign = float(increment), (1 if sign > 0 else -1)
        self.desired = desired_patches(initial_first, self.patches, increment, sign)
        self.forget_devices()

    @property
    def P(self):
        return int(self.patches.shape[0])

    def replace_desired(self, desired):
        """another [49, P] set of desired patches (a multi-GPU search gives every rank those of rank 0)"""
        if tuple(desired.shape) != (PATCH * PATCH, self.P):
            raise ValueError('patch magnitude: desired patches %s, expected [49, %d]' % (tuple(desired.shape), self.P))
        self.desired = desired.detach().float().cpu().contiguous()
        self.forget_devices()

    def _to_device(self, device):
        """on(device): (corner_index [H-6, W-6] int32, desired [P, 49], patch indexes [P, 49] int64)"""
        return torch.from_numpy(self.corner_index).to(device), self.desired.t().contiguous().to(device), torch.from_numpy(self.patches).to(device)


def _patch_mag_cpu(x, spec):
    """the defining expression (reference :717-722) -> [B]"""
    _, desired, idx = spec.on(x.device)
    v = torch.clamp(x, 0, 1).mean(1).reshape(x.size(0), -1)
    return ((v[:, idx] - desired.to(v.dtype)) ** 2).mean(dim=(1, 2))


class _PatchMag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, spec):
        xd = detach_f32(x)
        B, Cc, H, W = xd.shape
        index, desired, _ = spec.on(xd.device)
        partial = torch.empty(B, int(_lib.lib.esr_patch_mag_blocks(H, W)), dtype=torch.float64, device=xd.device)
        check(_lib.lib.esr_patch_mag(xd.data_ptr(), B, Cc, H, W, index.data_ptr(), desired.data_ptr(), spec.P, partial.data_ptr(), stream_ptr()),
              'esr_patch_mag')
        ctx.save_for_backward(xd)
        ctx.spec = spec
        return (partial.sum(1) / (PATCH * PATCH * spec.P)).float()

    @staticmethod
    def backward(ctx, g):
        xd, = ctx.saved_tensors
        B, Cc, H, W = xd.shape
        index, desired, _ = ctx.spec.on(xd.device)
        g = g.detach().float().contiguous()
        dx = torch.empty_like(xd)
        check(_lib.lib.esr_patch_mag_grad(xd.data_ptr(), B, Cc, H, W, index.data_ptr(), desired.data_ptr(), ctx.spec.P, g.data_ptr(), dx.data_ptr(), 0,
                                          stream_ptr()), 'esr_patch_mag_grad')
        return dx, None


def patch_mag(x, spec):
    """[B]: per image of x [B, C, H, W] the mean over the 49 x P entries of (patches(mean_c clamp(x_b, 0, 1)) - desired)^2"""
    if x.dim() != 4 or (x.size(2), x.size(3)) != (spec.H, spec.W):
        raise ValueError('patch_mag: images %s, spec for %d x %d' % (tuple(x.shape), spec.H, spec.W))
    if not x.is_cuda:
        return _patch_mag_cpu(x, spec)
    return _PatchMag.apply(x, spec)
