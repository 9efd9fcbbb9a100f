"""Host side of the JPEG consistency layer (reference codes/JPEG_module/JPEG.py): for the Y channel (block size 8) the 8x8 block DCT between an
image [B, 1, H, W] (0...255) and its coefficient planes [B, 64, H/8, W/8] (channel 8u + v), the per-image quantisation table, and the generator's
sigmoid tail (codes/models/modules/architecture.py:206, 214); for the colour model (chroma_mode, block size 16) the 16x16 transform of a YCbCr
image, compress16 / extract16 at the end of this file.

* compress(x, qtab, quantize) -> coefficients = DCT(x - 128) / qtab, torch.round when quantize (whose gradient is zero, as the reference's).
* extract(coef, qtab, y=None) -> (c, image): c = coef when y is None, else coef + sigmoid(y) - 0.5; image = 128 + iDCT(c * qtab).
GPU tensors: csrc/esr_jpeg.hip through autograd functions (input gradients; qtab carries none).  CPU tensors: the defining torch expression
against the explicit 8x8 DCT matrix, differentiated by torch itself — what the CPU tests and a CPU-side caller run.
qtab is [B, 64] (or [1, 64], one table for every image), row-major (u, v)."""
import collections
import ctypes as C
import math

import torch

from . import _lib
from ._image import detach_f32
from ._lib import check
from .act import stream_ptr


def dct_matrix(dtype=torch.float32, device='cpu'):
    """D[k, n] = a(k) cos((2n + 1) k pi / 16), a(0) = sqrt(1/8), a(k > 0) = 1/2: orthonormal, so D^-1 = D^T.  Computed in float64."""
    k = torch.arange(8, dtype=torch.float64).view(8, 1)
    n = torch.arange(8, dtype=torch.float64).view(1, 8)
    D = torch.cos((2 * n + 1) * k * math.pi / 16) * 0.5
    D[0] = math.sqrt(0.125)
    return D.to(dtype=dtype, device=device)


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


# ================================================================================================ the colour model: 16x16 blocks
# (reference JPEG.py with chroma_mode=True, block_size=16, FACTORIZE_CHROMA_HIGH_FREQS).  Image [B, 3, H, W] YCbCr 0...255, h = H/16, w = W/16.
# An image plane keeps K = 16 frequencies per axis (256 channels, 16u + v) or K = 8 (64 channels, 8u + v: the chroma down-sampling).
# qtab is the padded table [B, 3, 16, 16, 1, 1] (JPEG.padded_Q_table), any shape with B * 768 or 768 entries.
#   compress16(x, qtab, mode): mode False -> [B, 768, h, w] (Y | Cb | Cr, K = 16, unrounded); 'downsample_only' -> [B, 384, h, w]
#       (Y K = 16 | Cb | Cr K = 8, unrounded); True -> the same with Cb and Cr rounded (zero gradient there); Y is never rounded.
#   extract16(coef, qtab, y=None) -> (c, image): by the channel count 128 (Cb, Cr low -> [B, 2, H, W]), 512 (Cb, Cr full -> [B, 2, H, W]) or
#       384 (Y | Cb, Cr low -> [B, 3, H, W], + 128 on Y).  With y [B, 128, h, w], the chroma generator's last conv output, coef is the
#       generator's 384 input coefficients (or their last 128): c = coef[:, -128:] + sigmoid(y) - 0.5, image [B, 2, H, W].
MODES16 = {False: 0, 'downsample_only': 1, True: 2}          # ESR_JPEG16_ALL / _DOWNSAMPLE / _QUANTIZE


def dct_matrix16(dtype=torch.float32, device='cpu'):
    """D[k, n] = a(k) cos((2n + 1) k pi / 32), a(0) = 1/4, a(k > 0) = sqrt(1/8): orthonormal.  Computed in float64."""
    k = torch.arange(16, dtype=torch.float64).view(16, 1)
    n = torch.arange(16, dtype=torch.float64).view(1, 16)
    D = torch.cos((2 * n + 1) * k * math.pi / 32) * math.sqrt(0.125)
    D[0] = 0.25
    return D.to(dtype=dtype, device=device)


def _mode16(mode):
    if not any(mode is m for m in (True, False)) and mode != 'downsample_only':
        raise ValueError("JPEG compress16: mode True, False or 'downsample_only', got %r" % (mode,))
    return MODES16[mode]


def _planes16(form):
    """(image planes, K per plane) of an extractor form"""
    return {128: (2, (8, 8)), 512: (2, (16, 16)), 384: (3, (16, 8, 8))}[form]


def _compress16_cpu(x, qtab, mode):
    B, _, H, W = x.shape
    h, w = H // 16, W // 16
    D = dct_matrix16(x.dtype, x.device)
    blocks = x.reshape(B, 3, h, 16, w, 16) - torch.tensor([128., 0., 0.], dtype=x.dtype, device=x.device).view(1, 3, 1, 1, 1, 1)
    out = torch.einsum('ur,bcirjs,vs->bcuvij', D, blocks, D) / qtab.view(B, 3, 16, 16, 1, 1).to(x.dtype)
    if mode == 0:
        return out.reshape(B, 768, h, w)
    chroma = out[:, 1:, :8, :8]
    if mode == 2:
        chroma = torch.round(chroma)
    return torch.cat([out[:, 0].reshape(B, 256, h, w), chroma.reshape(B, 128, h, w)], 1)


def _extract16_cpu(coef, qtab, y):
    B, C, h, w = coef.shape
    if y is not None:
        coef = coef[:, C - 128:] + (torch.sigmoid(y) - 0.5)
    form = coef.size(1)
    n, Ks = _planes16(form)
    D = dct_matrix16(coef.dtype, coef.device)
    planes, c0 = [], 0
    for K in Ks:
        p = coef[:, c0:c0 + K * K].reshape(B, 1, K, K, h, w)
        planes.append(p if K == 16 else torch.nn.functional.pad(p, [0, 0, 0, 0, 0, 8, 0, 8]))
        c0 += K * K
    full = torch.cat(planes, 1) * qtab.view(B, 3, 16, 16, 1, 1)[:, 3 - n:].to(coef.dtype)
    img = torch.einsum('ur,bcuvij,vs->bcirjs', D, full, D).reshape(B, n, 16 * h, 16 * w)
    if n == 3:
        img = img + torch.tensor([128., 0., 0.], dtype=img.dtype, device=img.device).view(1, 3, 1, 1)
    return coef, img


# ================================================================================================ GPU: csrc/esr_jpeg.hip, csrc/esr_jpeg16.hip
# What differs between the two block sizes.  A `form` is the channel count of the coefficients an extractor launch transforms, a `mode` the
# compressor's integer (8-point: 1 rounds, 0 does not; 16-point: MODES16).  The four entry points are given one argument order:
#   compress(x, B, H, W, qtab, mode, coef, stream)                    compress_grad(d_coef, mode, B, h, w, qtab, d_x, stream)
#   extract(coef, C, form, y, B, h, w, qtab, coef_out, img, stream)   extract_grad(d_img, y, form, B, h, w, qtab, d_coef, d_y, stream)
_Block = collections.namedtuple('_Block', [
    'N',              # block side
    'prefix',         # of the entry points' names
    'table',          # shape of one image's table(s)
    'image_C',        # planes of the compressor's image
    'compress_C',     # mode -> coefficient channels of the compressor
    'grad_planes',    # mode -> image planes esr_*_compress_grad writes (the planes behind a rounding get zero gradient and no launch)
    'planes',         # form -> image planes of the extractor
    'tail',           # the form with y: channels of y, c and d_y
    'c_from_kernel',  # the extractor's c without y: written by the kernel (coef_out), else a clone of the input
    'compress', 'compress_grad', 'extract', 'extract_grad', 'compress_cpu', 'extract_cpu'])

_B8 = _Block(
    N=8, prefix='esr_jpeg_', table=(64,), image_C=1, compress_C=lambda mode: 64, grad_planes=lambda mode: 0 if mode else 1, planes={64: 1},
    tail=64, c_from_kernel=True,
    compress=lambda x, B, H, W, q, mode, coef, s: _lib.lib.esr_jpeg_compress(x, B, H, W, q, mode, coef, None, s),
    compress_grad=lambda g, mode, B, h, w, q, dx, s: _lib.lib.esr_jpeg_compress_grad(g, B, h, w, q, dx, s),
    extract=lambda coef, C_, form, y, B, h, w, q, c, img, s: _lib.lib.esr_jpeg_extract(coef, y, B, h, w, q, c, img, s),
    extract_grad=lambda g, y, form, B, h, w, q, dc, dy, s: _lib.lib.esr_jpeg_extract_grad(g, y, B, h, w, q, dc, dy, s),
    compress_cpu=lambda *a: _compress_cpu(*a), extract_cpu=lambda *a: _extract_cpu(*a))       # (by name: the GPU tests patch them)

_B16 = _Block(
    N=16, prefix='esr_jpeg16_', table=(3, 256), image_C=3, compress_C=lambda mode: 768 if mode == 0 else 384,
    grad_planes=lambda mode: 1 if mode == 2 else 3,               # quantising mode: the kernel writes the Y plane only (JPEG.py:148)
    planes={form: _planes16(form)[0] for form in (128, 384, 512)}, tail=128,
    c_from_kernel=False,                                          # esr_jpeg16_extract takes coef_out with y only
    compress=lambda x, B, H, W, q, mode, coef, s: _lib.lib.esr_jpeg16_compress(x, B, H, W, q, mode, coef, s),
    compress_grad=lambda g, mode, B, h, w, q, dx, s: _lib.lib.esr_jpeg16_compress_grad(g, mode, B, h, w, q, dx, s),
    extract=lambda coef, C_, form, y, B, h, w, q, c, img, s: _lib.lib.esr_jpeg16_extract(coef, C_, C_ - form, y, form, B, h, w, q, c, img, s),
    extract_grad=lambda g, y, form, B, h, w, q, dc, dy, s: _lib.lib.esr_jpeg16_extract_grad(g, y, form, B, h, w, q, dc, dy, s),
    compress_cpu=lambda *a: _compress16_cpu(*a), extract_cpu=lambda *a: _extract16_cpu(*a))


def _launch(bk, what, *args):
    check(getattr(bk, what)(*args, stream_ptr()), bk.prefix + what)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _new(ref, *shape, zero=False):
    return (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device=ref.device)


def _tables(bk, qtab, B, device):
    q = qtab.detach().reshape(-1, *bk.table).to(device=device, dtype=torch.float32)
    if q.size(0) != B:
        if q.size(0) != 1:
            raise ValueError('JPEG: %d quantisation tables for %d images' % (q.size(0), B))
        q = q.expand(B, *bk.table)
    return q.contiguous()


class _Compress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bk, x, qtab, mode):
        xd = detach_f32(x)
        B, _, H, W = xd.shape
        coef = _new(xd, B, bk.compress_C(mode), H // bk.N, W // bk.N)
        _launch(bk, 'compress', xd.data_ptr(), B, H, W, qtab.data_ptr(), mode, coef.data_ptr())
        ctx.bk, ctx.mode, ctx.qtab = bk, mode, qtab
        return coef

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_coef):
        bk, (B, _, h, w) = ctx.bk, d_coef.shape
        written = bk.grad_planes(ctx.mode)                        # torch.round: zero gradient (JPEG.py:148, :162)
        dx = _new(d_coef, B, bk.image_C, bk.N * h, bk.N * w, zero=written < bk.image_C)
        if written:
            g = detach_f32(d_coef)
            _launch(bk, 'compress_grad', g.data_ptr(), ctx.mode, B, h, w, ctx.qtab.data_ptr(), dx.data_ptr())
        return None, dx, None, None


def _extract_launch(bk, coef, y, qtab, want_c):
    B, C_, h, w = coef.shape
    form = C_ if y is None else bk.tail
    img = _new(coef, B, bk.planes[form], bk.N * h, bk.N * w)
    c = _new(coef, B, form, h, w) if want_c else None
    _launch(bk, 'extract', coef.data_ptr(), C_, form, _ptr(y), B, h, w, qtab.data_ptr(), _ptr(c), img.data_ptr())
    return c, img


class _Extract(torch.autograd.Function):
    """(coef, y | None, qtab) -> (c, image).  Backward: one esr_*_extract_grad launch for the image's gradient; a gradient arriving at c
    itself (a loss on the coefficients) is added with torch ops.  With y, the 16-point coef may be the generator's whole 384-channel input:
    its leading channels get zero."""

    @staticmethod
    def forward(ctx, bk, coef, y, qtab):
        cd, yd = detach_f32(coef), (None if y is None else detach_f32(y))
        c, img = _extract_launch(bk, cd, yd, qtab, want_c=yd is not None or bk.c_from_kernel)
        ctx.bk, ctx.qtab, ctx.y, ctx.C = bk, qtab, yd, cd.size(1)
        ctx.set_materialize_grads(False)
        return (cd.clone() if c is None else c), img              # (an output of its own also without y: a Function does not hand an input back)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_c, d_img):
        bk, y, need_coef, need_y = ctx.bk, ctx.y, ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.y is not None
        form = ctx.C if y is None else bk.tail
        d_coef = d_y = None
        if d_img is not None:
            g = detach_f32(d_img)
            B, h, w = g.size(0), g.size(2) // bk.N, g.size(3) // bk.N
            d_coef = _new(g, B, form, h, w) if (need_coef or d_c is not None) else None
            d_y = _new(g, B, bk.tail, h, w) if need_y else None
            if d_coef is not None or d_y is not None:
                _launch(bk, 'extract_grad', g.data_ptr(), None if d_y is None else y.data_ptr(), form, B, h, w, ctx.qtab.data_ptr(), _ptr(d_coef),
                        _ptr(d_y))
        if d_c is not None:
            d_c = d_c.detach().float()
            d_coef = d_c if d_coef is None else d_coef + d_c
            if need_y:
                s = torch.sigmoid(y)
                d_y = d_c * s * (1 - s) + (0 if d_y is None else d_y)
        if need_coef and d_coef is not None and d_coef.size(1) != ctx.C:
            d_coef = torch.nn.functional.pad(d_coef, [0, 0, 0, 0, ctx.C - d_coef.size(1), 0])
        return None, (d_coef if need_coef else None), (d_y if need_y else None), None


def _compress(bk, x, qtab, mode):
    q = _tables(bk, qtab, x.size(0), x.device)
    if not x.is_cuda:
        return bk.compress_cpu(x, q, mode)
    return _Compress.apply(bk, x, q, mode)


def _extract(bk, coef, qtab, y):
    q = _tables(bk, qtab, coef.size(0), coef.device)
    if not coef.is_cuda:
        return bk.extract_cpu(coef, q, y)
    if torch.is_grad_enabled() and (coef.requires_grad or (y is not None and y.requires_grad)):
        return _Extract.apply(bk, coef, y, q)
    cd, yd = detach_f32(coef), (None if y is None else detach_f32(y))
    c, img = _extract_launch(bk, cd, yd, q, want_c=yd is not None)
    return (cd if c is None else c), img


# ------------------------------------------------------------------------------------------------ public
def _check_image(x):
    if x.dim() != 4 or x.size(1) != 1 or x.size(2) % 8 or x.size(3) % 8 or x.size(2) == 0 or x.size(3) == 0:
        raise ValueError('JPEG compress: a [B, 1, H, W] image with H and W multiples of 8, got %s' % (tuple(x.shape),))


def _check_coef(c, what='coefficients'):
    if c.dim() != 4 or c.size(1) != 64 or c.numel() == 0:
        raise ValueError('JPEG extract: %s [B, 64, h, w], got %s' % (what, tuple(c.shape)))


def _check_image16(x):
    if x.dim() != 4 or x.size(1) != 3 or x.size(2) % 16 or x.size(3) % 16 or x.size(2) == 0 or x.size(3) == 0:
        raise ValueError('JPEG compress16: a [B, 3, H, W] image with H and W multiples of 16, got %s' % (tuple(x.shape),))


def compress(x, qtab, quantize):
    """[B, 1, H, W] -> [B, 64, H/8, W/8] (JPEG.py:131-163)"""
    _check_image(x)
    return _compress(_B8, x, qtab, 1 if quantize else 0)


def extract(coef, qtab, y=None):
    """(c, image): c = coef [+ sigmoid(y) - 0.5], image [B, 1, 8h, 8w] = 128 + iDCT(c * qtab) (JPEG.py:193-197)"""
    _check_coef(coef)
    if y is not None:
        _check_coef(y, 'the generator output')
        if y.shape != coef.shape or y.device != coef.device:
            raise ValueError('JPEG extract: generator output %s on %s for coefficients %s on %s' % (tuple(y.shape), y.device, tuple(coef.shape), coef.device))
    return _extract(_B8, coef, qtab, y)


def compress_into(x, qtab, quantize, act_view, want_coef=True):
    """The compressor with its result also (or only) written into groups [0, 8) of an activation view (esr_jpeg_compress's act_out): the
    generator's input without a second pass.  No gradient.  Returns the fp32 coefficients or None."""
    _check_image(x)
    xd = detach_f32(x)
    B, _, H, W = xd.shape
    q = _tables(_B8, qtab, B, xd.device)
    coef = _new(xd, B, 64, H // 8, W // 8) if want_coef else None
    check(_lib.lib.esr_jpeg_compress(xd.data_ptr(), B, H, W, q.data_ptr(), 1 if quantize else 0, _ptr(coef), C.byref(act_view), stream_ptr()),
          'esr_jpeg_compress')
    return coef


def compress16(x, qtab, mode):
    """[B, 3, H, W] YCbCr -> [B, 768 | 384, H/16, W/16] (JPEG.py:131-154)"""
    _check_image16(x)
    return _compress(_B16, x, qtab, _mode16(mode))


def extract16(coef, qtab, y=None):
    """(c, image) (JPEG.py:165-201; with y the chroma generator's tail, architecture.py:206-212, in front)"""
    if coef.dim() != 4 or coef.numel() == 0 or coef.size(1) not in ((128, 384) if y is not None else (128, 384, 512)):
        raise Exception('Unexpected input size')                # (the reference's words, JPEG.py:185)
    if y is not None and (y.dim() != 4 or y.size(1) != 128 or y.shape[2:] != coef.shape[2:] or y.size(0) != coef.size(0) or y.device != coef.device):
        raise ValueError('JPEG extract16: generator output %s on %s for coefficients %s on %s' % (tuple(y.shape), y.device, tuple(coef.shape), coef.device))
    return _extract(_B16, coef, qtab, y)
