"""Host side of the JPEG consistency layer (reference codes/JPEG_module/JPEG.py, Y channel, block size 8): the 8x8 block DCT between an image
[B, 1, H, W] (0...255) and its coefficient planes [B, 64, H/8, W/8] (channel 8u + v), the per-image quantisation table, and the generator's
sigmoid tail (codes/models/modules/architecture.py:206, 214).

* compress(x, qtab, quantize) -> coefficients = DCT(x - 128) / qtab, torch.round when quantize (whose gradient is zero, as the reference's).
* extract(coef, qtab, y=None) -> (c, image): c = coef when y is None, else coef + sigmoid(y) - 0.5; image = 128 + iDCT(c * qtab).
GPU tensors: csrc/esr_jpeg.hip through autograd functions (input gradients; qtab carries none).  CPU tensors: the defining torch expression
against the explicit 8x8 DCT matrix, differentiated by torch itself — what the CPU tests and a CPU-side caller run.
qtab is [B, 64] (or [1, 64], one table for every image), row-major (u, v)."""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import check
from .act import stream_ptr


def dct_matrix(dtype=torch.float32, device='cpu'):
    """D[k, n] = a(k) cos((2n + 1) k pi / 16), a(0) = sqrt(1/8), a(k > 0) = 1/2: orthonormal, so D^-1 = D^T.  Computed in float64."""
    k = torch.arange(8, dtype=torch.float64).view(8, 1)
    n = torch.arange(8, dtype=torch.float64).view(1, 8)
    D = torch.cos((2 * n + 1) * k * math.pi / 16) * 0.5
    D[0] = math.sqrt(0.125)
    return D.to(dtype=dtype, device=device)


def _qtab_for(qtab, B, device):
    q = qtab.detach().reshape(-1, 64).to(device=device, dtype=torch.float32)
    if q.size(0) != B:
        if q.size(0) != 1:
            raise ValueError('JPEG: %d quantisation tables for %d images' % (q.size(0), B))
        q = q.expand(B, 64)
    return q.contiguous()


# ------------------------------------------------------------------------------------------------ CPU: the defining expressions
def _compress_cpu(x, qtab, quantize):
    B, _, H, W = x.shape
    D = dct_matrix(x.dtype, x.device)
    blocks = x.reshape(B, H // 8, 8, W // 8, 8) - 128
    out = torch.einsum('ur,birjs,vs->buvij', D, blocks, D) / qtab.view(B, 8, 8, 1, 1).to(x.dtype)
    if quantize:
        out = torch.round(out)
    return out.reshape(B, 64, H // 8, W // 8)


def _extract_cpu(coef, qtab, y):
    B, _, h, w = coef.shape
    D = dct_matrix(coef.dtype, coef.device)
    c = coef if y is None else coef + (torch.sigmoid(y) - 0.5)
    img = torch.einsum('ur,buvij,vs->birjs', D, c.reshape(B, 8, 8, h, w) * qtab.view(B, 8, 8, 1, 1).to(coef.dtype), D) + 128
    return c, img.reshape(B, 1, 8 * h, 8 * w)


# ------------------------------------------------------------------------------------------------ GPU: csrc/esr_jpeg.hip
def _f32c(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class _Compress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, qtab, quantize):
        xd = _f32c(x)
        B, _, H, W = xd.shape
        coef = torch.empty(B, 64, H // 8, W // 8, dtype=torch.float32, device=xd.device)
        check(_lib.lib.esr_jpeg_compress(xd.data_ptr(), B, H, W, qtab.data_ptr(), 1 if quantize else 0, coef.data_ptr(), None, stream_ptr()),
              'esr_jpeg_compress')
        ctx.quantize, ctx.qtab = quantize, qtab
        return coef

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_coef):
        B, _, h, w = d_coef.shape
        if ctx.quantize:                              # torch.round: zero gradient (JPEG.py:162)
            return torch.zeros(B, 1, 8 * h, 8 * w, dtype=torch.float32, device=d_coef.device), None, None
        g = _f32c(d_coef)
        dx = torch.empty(B, 1, 8 * h, 8 * w, dtype=torch.float32, device=g.device)
        check(_lib.lib.esr_jpeg_compress_grad(g.data_ptr(), B, h, w, ctx.qtab.data_ptr(), dx.data_ptr(), stream_ptr()), 'esr_jpeg_compress_grad')
        return dx, None, None


def _extract_launch(coef, y, qtab, want_c):
    B, _, h, w = coef.shape
    img = torch.empty(B, 1, 8 * h, 8 * w, dtype=torch.float32, device=coef.device)
    c = torch.empty_like(coef) if want_c else None
    check(_lib.lib.esr_jpeg_extract(coef.data_ptr(), None if y is None else y.data_ptr(), B, h, w, qtab.data_ptr(),
                                    None if c is None else c.data_ptr(), img.data_ptr(), stream_ptr()), 'esr_jpeg_extract')
    return c, img


class _Extract(torch.autograd.Function):
    """(coef, y | None, qtab) -> (c, image).  Backward: one esr_jpeg_extract_grad launch for the image's gradient; a gradient arriving at c
    itself (a loss on the coefficients) is added with torch ops."""

    @staticmethod
    def forward(ctx, coef, y, qtab):
        cd, yd = _f32c(coef), (None if y is None else _f32c(y))
        c, img = _extract_launch(cd, yd, qtab, want_c=True)      # (an output of its own also without y: a Function does not hand an input back)
        ctx.qtab, ctx.y = qtab, yd
        ctx.set_materialize_grads(False)
        return c, img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_c, d_img):
        y, need_coef, need_y = ctx.y, ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.y is not None
        d_coef = d_y = None
        if d_img is not None:
            g = _f32c(d_img)
            B, h, w = g.size(0), g.size(2) // 8, g.size(3) // 8
            d_coef = torch.empty(B, 64, h, w, dtype=torch.float32, device=g.device) if (need_coef or d_c is not None) else None
            d_y = torch.empty(B, 64, h, w, dtype=torch.float32, device=g.device) if need_y else None
            if d_coef is not None or d_y is not None:
                check(_lib.lib.esr_jpeg_extract_grad(g.data_ptr(), None if d_y is None else y.data_ptr(), B, h, w, ctx.qtab.data_ptr(),
                                                     None if d_coef is None else d_coef.data_ptr(), None if d_y is None else d_y.data_ptr(),
                                                     stream_ptr()), 'esr_jpeg_extract_grad')
        if d_c is not None:
            d_c = d_c.detach().float()
            d_coef = d_c if d_coef is None else d_coef + d_c
            if need_y:
                s = torch.sigmoid(y)
                d_y = d_c * s * (1 - s) + (0 if d_y is None else d_y)
        return (d_coef if need_coef else None), (d_y if need_y else None), None


# ------------------------------------------------------------------------------------------------ public
def _check_image(x):
    if x.dim() != 4 or x.size(1) != 1 or x.size(2) % 8 or x.size(3) % 8 or x.size(2) == 0 or x.size(3) == 0:
        raise ValueError('JPEG compress: a [B, 1, H, W] image with H and W multiples of 8, got %s' % (tuple(x.shape),))


def _check_coef(c, what='coefficients'):
    if c.dim() != 4 or c.size(1) != 64 or c.numel() == 0:
        raise ValueError('JPEG extract: %s [B, 64, h, w], got %s' % (what, tuple(c.shape)))


def compress(x, qtab, quantize):
    """[B, 1, H, W] -> [B, 64, H/8, W/8] (JPEG.py:131-163)"""
    _check_image(x)
    q = _qtab_for(qtab, x.size(0), x.device)
    if not x.is_cuda:
        return _compress_cpu(x, q, quantize)
    return _Compress.apply(x, q, bool(quantize))


def extract(coef, qtab, y=None):
    """(c, image): c = coef [+ sigmoid(y) - 0.5], image [B, 1, 8h, 8w] = 128 + iDCT(c * qtab) (JPEG.py:193-197)"""
    _check_coef(coef)
    if y is not None:
        _check_coef(y, 'the generator output')
        if y.shape != coef.shape or y.device != coef.device:
            raise ValueError('JPEG extract: generator output %s on %s for coefficients %s on %s' % (tuple(y.shape), y.device, tuple(coef.shape), coef.device))
    q = _qtab_for(qtab, coef.size(0), coef.device)
    if not coef.is_cuda:
        return _extract_cpu(coef, q, y)
    if torch.is_grad_enabled() and (coef.requires_grad or (y is not None and y.requires_grad)):
        return _Extract.apply(coef, y, q)
    cd, yd = _f32c(coef), (None if y is None else _f32c(y))
    c, img = _extract_launch(cd, yd, q, want_c=yd is not None)
    return (cd if c is None else c), img


def compress_into(x, qtab, quantize, act_view, want_coef=True):
    """The compressor with its result also (or only) written into groups [0, 8) of an activation view (esr_jpeg_compress's act_out): the
    generator's input without a second pass.  No gradient.  Returns the fp32 coefficients or None."""
    _check_image(x)
    xd = _f32c(x)
    B, _, H, W = xd.shape
    q = _qtab_for(qtab, B, xd.device)
    coef = torch.empty(B, 64, H // 8, W // 8, dtype=torch.float32, device=xd.device) if want_coef else None
    check(_lib.lib.esr_jpeg_compress(xd.data_ptr(), B, H, W, q.data_ptr(), 1 if quantize else 0, None if coef is None else coef.data_ptr(),
                                     C.byref(act_view), stream_ptr()), 'esr_jpeg_compress')
    return coef
