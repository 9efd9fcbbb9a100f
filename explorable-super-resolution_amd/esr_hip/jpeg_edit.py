"""Host side of the explorable JPEG decoder's editing tools (csrc/esr_jpeg_edit.hip): what the reference's JPEG GUI does around its model.

* ycbcr_to_rgb(x) -> [B, 3, H, W] RGB in 0...1, un-clamped, of a YCbCr image in 0...255: util.Tensor_YCbCR2RGB(x / 255) (codes/utils/util.py:328-330),
  the colour model's Output_Batch(within_0_1=True) before its clamp.  Differentiable.
* consistency_violation(candidates, coef, qtab) -> [N] float64: sum over all coefficients of max(0, |compress(c, unrounded) - coef| - 0.5), the
  imprint search's score (codes/GUI.py:1026-1033): 0 for a candidate that compresses to `coef`.  candidates [N, 1, H, W] in 0...255; coef
  [1 | N, 64, H/8, W/8]; qtab [1 | N, 64] (any shape with 64 or N * 64 entries).  No gradient.
* consistent_plane(desired, coef, qtab) -> [B, 1, H, W]: the image whose unrounded coefficients are those of `desired` clamped to within 0.5 of
  the quantised `coef` (codes/models/DecompCNN_model.py:320-324).  No gradient.
* consistent_chroma(desired, coef128, qtab) -> [B, 2, H, W]: the same for Cb and Cr on 16x16 blocks (:325-333): the low 8x8 frequencies are
  clamped against the 128 quantised chroma coefficients (coef128 [B, 128, h, w], or the compressor's [B, 384, h, w], whose last 128 they are),
  the high ones stay the desired image's.  desired [B, 3, H, W] YCbCr (Y is not read) or [B, 2, H, W]; qtab the padded tables.  No gradient.
* smear_mask_to_blocks(mask, block_size=8): every block takes its largest value (codes/utils/util.py:318-326), NumPy.

GPU tensors take the kernels; CPU tensors the defining torch expressions below, compositions of esr_hip.jpeg's ops (which the tests and a
CPU-side caller run)."""
import numpy as np
import torch

from . import _lib
from . import jpeg as J
from ._image import detach_f32
from ._lib import check
from .act import stream_ptr

# the reference's constants (utils/util.py:329-330), per unit of an 8-bit value: ITU-R BT.601 studio-range YCbCr to full-range RGB
YCBCR2RGB = np.array([[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]])
YCBCR2RGB_OFFSET = (-222.921, 135.576, -276.836)


# ------------------------------------------------------------------------------------------------ CPU: the defining expressions
def _ycbcr_to_rgb_cpu(x):
    image = x / 255
    mat = torch.from_numpy(255 * YCBCR2RGB.transpose()).view(1, 3, 3, 1, 1).to(device=image.device, dtype=image.dtype)
    offset = torch.tensor(YCBCR2RGB_OFFSET, device=image.device, dtype=image.dtype).view(1, 3, 1, 1) / 255
    return (mat * image.unsqueeze(1)).sum(2) + offset


def _violation_cpu(candidates, coef, qtab):
    d = J.compress(candidates, qtab, False) - coef
    return torch.clamp(d.abs() - 0.5, min=0).double().sum(dim=(1, 2, 3))


def _correct(desired_coef, constraining_coef):
    return torch.clamp(desired_coef - constraining_coef, -0.5, 0.5) + constraining_coef


def _plane_cpu(desired, coef, qtab):
    return J.extract(_correct(J.compress(desired, qtab, False), coef), qtab)[1]


def _chroma_cpu(desired, coef128, qtab):
    B, _, H, W = desired.shape
    h, w = H // 16, W // 16
    if desired.size(1) == 2:                                      # (the compressor takes three planes; Y's coefficients are not used)
        desired = torch.cat([torch.zeros_like(desired[:, :1]), desired], 1)
    chroma = J.compress16(desired, qtab, False)[:, 256:].reshape(B, 2, 16, 16, h, w).clone()
    chroma[:, :, :8, :8] = _correct(chroma[:, :, :8, :8], coef128[:, -128:].reshape(B, 2, 8, 8, h, w))
    return J.extract16(chroma.reshape(B, 512, h, w), qtab)[1]


# ------------------------------------------------------------------------------------------------ GPU: csrc/esr_jpeg_edit.hip
def _rgb_launch(name, x):
    xd = detach_f32(x)
    B, _, H, W = xd.shape
    out = torch.empty_like(xd)
    with torch.cuda.device(xd.device):
        check(getattr(_lib.lib, name)(xd.data_ptr(), B, H, W, out.data_ptr(), stream_ptr()), name)
    return out


class _YCbCr2RGB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _rgb_launch('esr_ycbcr_rgb', x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_rgb):
        return _rgb_launch('esr_ycbcr_rgb_grad', d_rgb)


def _tables8(qtab, n, device):
    """[1 | n, 64] float32 on `device`"""
    q = qtab.detach().reshape(-1, 64).to(device=device, dtype=torch.float32).contiguous()
    if q.size(0) not in (1, n):
        raise ValueError('JPEG: %d quantisation tables for %d images' % (q.size(0), n))
    return q


def _check_plane(x, what):
    if x.dim() != 4 or x.size(1) != 1 or x.size(2) % 8 or x.size(3) % 8 or x.numel() == 0:
        raise ValueError('%s: a [B, 1, H, W] image with H and W multiples of 8, got %s' % (what, tuple(x.shape)))


# ------------------------------------------------------------------------------------------------ public
def ycbcr_to_rgb(x):
    if x.dim() != 4 or x.size(1) != 3 or x.numel() == 0:
        raise ValueError('ycbcr_to_rgb: a [B, 3, H, W] image, got %s' % (tuple(x.shape),))
    if not x.is_cuda:
        return _ycbcr_to_rgb_cpu(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _YCbCr2RGB.apply(x)
    return _rgb_launch('esr_ycbcr_rgb', x)


def consistency_violation(candidates, coef, qtab):
    _check_plane(candidates, 'consistency_violation')
    N, _, H, W = candidates.shape
    if coef.dim() != 4 or coef.size(0) not in (1, N) or tuple(coef.shape[1:]) != (64, H // 8, W // 8) or coef.device != candidates.device:
        raise ValueError('consistency_violation: coefficients [1 | %d, 64, %d, %d] on %s, got %s on %s' % (
            N, H // 8, W // 8, candidates.device, tuple(coef.shape), coef.device))
    q = _tables8(qtab, N, candidates.device)
    if not candidates.is_cuda:
        with torch.no_grad():
            return _violation_cpu(candidates.float(), coef.float(), q)
    cd, kd = detach_f32(candidates), detach_f32(coef)
    with torch.cuda.device(cd.device):
        partial = torch.empty(N, int(_lib.lib.esr_jpeg_violation_partials(H, W)), dtype=torch.float64, device=cd.device)
        score = torch.empty(N, dtype=torch.float64, device=cd.device)
        check(_lib.lib.esr_jpeg_violation(cd.data_ptr(), N, H, W, kd.data_ptr(), kd.size(0), q.data_ptr(), q.size(0), partial.data_ptr(),
                                          score.data_ptr(), stream_ptr()), 'esr_jpeg_violation')
    return score


def consistent_plane(desired, coef, qtab):
    _check_plane(desired, 'consistent_plane')
    B, _, H, W = desired.shape
    if tuple(coef.shape) != (B, 64, H // 8, W // 8) or coef.device != desired.device:
        raise ValueError('consistent_plane: coefficients [%d, 64, %d, %d] on %s, got %s on %s' % (
            B, H // 8, W // 8, desired.device, tuple(coef.shape), coef.device))
    q = _tables8(qtab, B, desired.device).expand(B, 64).contiguous()
    if not desired.is_cuda:
        with torch.no_grad():
            return _plane_cpu(desired.float(), coef.float(), q)
    dd, kd = detach_f32(desired), detach_f32(coef)
    out = torch.empty_like(dd)
    with torch.cuda.device(dd.device):
        check(_lib.lib.esr_jpeg_pair(dd.data_ptr(), B, H, W, kd.data_ptr(), q.data_ptr(), out.data_ptr(), stream_ptr()), 'esr_jpeg_pair')
    return out


def consistent_chroma(desired, coef128, qtab):
    if desired.dim() != 4 or desired.size(1) not in (2, 3) or desired.size(2) % 16 or desired.size(3) % 16 or desired.numel() == 0:
        raise ValueError('consistent_chroma: a [B, 3 | 2, H, W] image with H and W multiples of 16, got %s' % (tuple(desired.shape),))
    B, C_, H, W = desired.shape
    h, w = H // 16, W // 16
    if coef128.dim() != 4 or coef128.size(0) != B or coef128.size(1) not in (128, 384) or tuple(coef128.shape[2:]) != (h, w) or \
            coef128.device != desired.device:
        raise ValueError('consistent_chroma: chroma coefficients [%d, 128 | 384, %d, %d] on %s, got %s on %s' % (
            B, h, w, desired.device, tuple(coef128.shape), coef128.device))
    q = J._tables(J._B16, qtab, B, desired.device)
    if not desired.is_cuda:
        with torch.no_grad():
            return _chroma_cpu(desired.float(), coef128.float(), q)
    dd, kd = detach_f32(desired), detach_f32(coef128)
    out = torch.empty(B, 2, H, W, dtype=torch.float32, device=dd.device)
    with torch.cuda.device(dd.device):
        check(_lib.lib.esr_jpeg16_pair(dd.data_ptr(), C_, B, H, W, kd.data_ptr(), kd.size(1), kd.size(1) - 128, q.data_ptr(), out.data_ptr(),
                                       stream_ptr()), 'esr_jpeg16_pair')
    return out


def smear_mask_to_blocks(mask, block_size=8):
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.shape[0] % block_size or mask.shape[1] % block_size:
        raise ValueError('smear_mask_to_blocks: a 2-D mask of whole %d x %d blocks, got %s' % (block_size, block_size, mask.shape))
    h, w = mask.shape[0] // block_size, mask.shape[1] // block_size
    top = mask.reshape(h, block_size, w, block_size).max(axis=(1, 3), keepdims=True)
    return (top * np.ones([1, block_size, 1, block_size], dtype=mask.dtype)).reshape(mask.shape)
