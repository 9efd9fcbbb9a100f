"""Host scaffold shared by the image-space Z objectives (local, patchmag, scribble, pairmin, zobj): how their wrappers hand tensors to the
kernels of csrc/esr_*.hip, and the per-device cache of what an objective builds once per edit."""
import numpy as np
import torch

PATCH = 7            # the reference's PATCH_SIZE_4_STD: the patch side of the local-STD and patch-magnitude objectives (csrc/esr_image.h: Patch7)


def as_f32(x):
    """x as a contiguous float32 tensor, x itself when it is one (stays attached to the graph)"""
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    return x


def detach_f32(x):
    """what a kernel reads: x detached, float32, contiguous"""
    return as_f32(x.detach())


def to_numpy(a):
    """a tensor (any device) or anything array-like as a NumPy array"""
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def mask_on(mask, device, H, W):
    """the image mask as a contiguous float32 [H, W] tensor on `device` (a broadcastable mask is expanded)"""
    return mask.detach().to(device=device, dtype=torch.float32).expand(H, W).contiguous()


def ptr(t):
    """the device pointer of an optional tensor, null for None"""
    return 0 if t is None else t.data_ptr()


class DeviceCopies:
    """Base of the per-edit specs: host data built once, its device copies built once per device.  A subclass gives _to_device(device) and
    calls forget_devices() when its host data is set or replaced."""

    def forget_devices(self):
        self._dev = {}

    def on(self, device):
        """the spec's tensors on `device` (what the subclass's _to_device returns), cached"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self._to_device(device)
        return self._dev[key]
