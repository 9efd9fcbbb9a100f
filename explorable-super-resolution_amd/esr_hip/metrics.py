"""Scores of the SR output: PSNR, SSIM and the per-pixel spread over Z samples (reference codes/utils/util.py:196-228 tensor2img, :340-391
calculate_psnr / ssim / calculate_ssim; codes/test.py:198-242 and its 'stats' mode, :224-233) without OpenCV or torchvision.

* psnr_ssim(a, b, min_max, out_type, crop_border) -> (psnr [B], ssim [B]) float64: both batches go through tensor2img's conversion in fp32
  ((clip(x, lo, hi) - lo) / (hi - lo), times 255, .round() for uint8), lose crop_border pixels on every side and are compared in float64:
  PSNR = 20 log10(255 / sqrt(mean (a - b)^2)) (inf where the images agree), SSIM = the mean over channels and valid 11 x 11 Gaussian windows
  (sigma 1.5) of util.ssim's map.  (util.calculate_ssim passes the whole three-channel image to ssim() three times, :383-387, and
  cv2.filter2D filters every channel: the mean over the channels.)  GPU tensors: csrc/esr_metrics.hip, one pass over both images, the [B]
  results finalised on the device, no synchronisation.  CPU tensors and arrays: the defining NumPy / torch float64 expression below.
  hi - lo is taken in fp32, which is the reference's quotient whenever lo and hi are fp32 numbers ((0, 1), (-1, 1), (0, 255)).
* calculate_psnr / calculate_ssim(img1, img2): the reference's signatures — HWC or HW arrays in [0, 255] (or CHW tensors) -> float.
* tensor2img: the reference's conversion of a 2-D / 3-D tensor to a BGR HWC array.
* sample_std(x [S, B, C, H, W]) -> (map [B, C, H, W] float32, mean [B] float64): 255 np.std over the S samples of clamp(x, 0, 1) and its mean
  per image (test.py:229-230; the projection it subtracts is common to the samples of an image and cancels).
"""
import math

import numpy as np
import torch

from . import _lib
from ._image import detach_f32
from ._lib import check
from .act import stream_ptr

TAPS = 11                      # cv2.getGaussianKernel(11, 1.5)
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian_window():
    """[11] float64: exp(-(i - 5)^2 / (2 1.5^2)) normalised to sum 1"""
    g = np.exp(-(np.arange(TAPS) - (TAPS - 1) / 2) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def _quantize(out_type):
    if out_type in (np.uint8, 'uint8', torch.uint8):
        return True
    if out_type in (np.float32, 'float32', torch.float32):
        return False
    raise ValueError('metrics: out_type is np.uint8 or np.float32, got %r' % (out_type,))


def _pixels_cpu(x, lo, hi, quantize):
    """tensor2img's arithmetic (util.py:224-226) on a float32 array"""
    lo, hi = np.float32(lo), np.float32(hi)
    p = (np.clip(x, lo, hi) - lo) / (hi - lo)
    p = p * np.float32(255.0)
    return p.round() if quantize else p


def _sums_cpu(pa, pb):
    """float64 [B, 2]: the squared error and the sum of the SSIM map (util.py:350-370) of [B, C, H, W] pixel arrays in 0...255"""
    a, b = torch.from_numpy(pa.astype(np.float64)), torch.from_numpy(pb.astype(np.float64))
    B, C, H, W = a.shape
    sse = ((a - b) ** 2).sum(dim=(1, 2, 3))
    if H < TAPS or W < TAPS:
        return torch.stack([sse, torch.zeros_like(sse)], 1)
    g = torch.from_numpy(gaussian_window())
    window = torch.outer(g, g).view(1, 1, TAPS, TAPS)
    filt = lambda t: torch.nn.functional.conv2d(t.reshape(B * C, 1, H, W), window)          # noqa: E731  (valid windows: filter2D's [5:-5, 5:-5])
    mu1, mu2 = filt(a), filt(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = filt(a ** 2) - mu1_sq, filt(b ** 2) - mu2_sq, filt(a * b) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return torch.stack([sse, ssim_map.reshape(B, -1).sum(1)], 1)


def _as_batch(x, name):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x))
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError('metrics: %s is [B, C, H, W] or [C, H, W], got %s' % (name, tuple(x.shape)))
    if not x.is_floating_point():
        x = x.float()
    return x


def _scores(a, b, lo, hi, mode, border, need_ssim):
    a, b = _as_batch(a, 'the first image'), _as_batch(b, 'the second image')
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    B, C, H, W = a.shape
    if C not in (1, 3):
        raise ValueError('metrics: images have 1 or 3 channels, got %d' % C)
    border = int(border)
    Hc, Wc = H - 2 * border, W - 2 * border
    if border < 0 or Hc < 1 or Wc < 1:
        raise ValueError('metrics: crop_border %d leaves nothing of a %d x %d image' % (border, H, W))
    if need_ssim and (Hc < TAPS or Wc < TAPS):
        raise ValueError('SSIM needs %d x %d pixels, %d x %d are left after cropping' % (TAPS, TAPS, Hc, Wc))
    if mode != _lib.PIXELS_RAW and not float(np.float32(hi)) > float(np.float32(lo)):
        raise ValueError('metrics: min_max needs max > min, got (%r, %r)' % (lo, hi))
    if a.device != b.device:
        raise ValueError('metrics: the images are on %s and %s' % (a.device, b.device))
    if a.is_cuda:
        ad, bd = detach_f32(a), detach_f32(b)
        with torch.cuda.device(ad.device):
            n = int(_lib.lib.esr_psnr_ssim_partials(C, H, W, border))
            partial = torch.empty(B, n, 2, dtype=torch.float64, device=ad.device)
            sums = torch.empty(B, 2, dtype=torch.float64, device=ad.device)
            check(_lib.lib.esr_psnr_ssim(ad.data_ptr(), bd.data_ptr(), B, C, H, W, float(lo), float(hi), mode, border, partial.data_ptr(), sums.data_ptr(),
                                         stream_ptr()), 'esr_psnr_ssim')
    else:
        crop = (slice(None), slice(None), slice(border, H - border), slice(border, W - border))
        pa, pb = (t.detach().float().numpy()[crop] for t in (a, b))
        if mode != _lib.PIXELS_RAW:
            pa, pb = (_pixels_cpu(p, lo, hi, mode == _lib.PIXELS_ROUND) for p in (pa, pb))
        sums = _sums_cpu(pa, pb)
    mse = sums[:, 0] / (C * Hc * Wc)
    psnr = 20 * torch.log10(255.0 / torch.sqrt(mse))                    # inf where mse = 0, as util.calculate_psnr returns
    windows = C * (Hc - TAPS + 1) * (Wc - TAPS + 1)
    ssim = sums[:, 1] / windows if windows > 0 else torch.full_like(mse, float('nan'))
    return psnr, ssim


def psnr_ssim(a, b, min_max=(0, 1), out_type=np.float32, crop_border=0):
    """(psnr [B], ssim [B]) float64 on the inputs' device, of [B, C, H, W] (or [C, H, W]) batches in the range min_max, C 1 or 3; any float dtype
    or stride.  out_type np.uint8: the pixels are rounded as tensor2img rounds them before they are compared."""
    mode = _lib.PIXELS_ROUND if _quantize(out_type) else _lib.PIXELS_FLOAT
    return _scores(a, b, min_max[0], min_max[1], mode, crop_border, True)


def psnr(a, b, min_max=(0, 1), out_type=np.float32, crop_border=0):
    mode = _lib.PIXELS_ROUND if _quantize(out_type) else _lib.PIXELS_FLOAT
    return _scores(a, b, min_max[0], min_max[1], mode, crop_border, False)[0]


def ssim(a, b, min_max=(0, 1), out_type=np.float32, crop_border=0):
    return psnr_ssim(a, b, min_max, out_type, crop_border)[1]


def _images_0_255(img1, img2):
    """the reference's image pair — HWC / HW arrays, or CHW / HW tensors — as [1, C, H, W] in 0...255, with the checks of util.calculate_ssim"""
    if tuple(img1.shape) != tuple(img2.shape):
        raise ValueError('Input images must have the same dimensions.')
    if img1.ndim not in (2, 3):
        raise ValueError('Wrong input image dimensions.')
    out = []
    for im in (img1, img2):
        if torch.is_tensor(im):
            im = im.detach()
            out.append(im[None, None] if im.dim() == 2 else im[None])
        else:
            im = np.asarray(im, dtype=np.float64)
            out.append(torch.from_numpy(im[None, None] if im.ndim == 2 else im.transpose(2, 0, 1)[None]))
    if out[0].size(1) not in (1, 3):
        raise ValueError('Wrong input image dimensions.')
    return out


def calculate_psnr(img1, img2):
    """util.calculate_psnr (:340-347): img1 and img2 have range [0, 255]"""
    a, b = _images_0_255(img1, img2)
    if a.is_cuda:
        return float(_scores(a, b, 0.0, 255.0, _lib.PIXELS_RAW, 0, False)[0][0])
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float('inf') if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))


def calculate_ssim(img1, img2):
    """util.calculate_ssim (:373-391).  A side below 11 is a ValueError (the reference returns the mean of an empty map)."""
    a, b = _images_0_255(img1, img2)
    if a.is_cuda:
        return float(_scores(a, b, 0.0, 255.0, _lib.PIXELS_RAW, 0, True)[1][0])
    if a.size(2) < TAPS or a.size(3) < TAPS:
        raise ValueError('SSIM needs %d x %d pixels, the image has %d x %d' % (TAPS, TAPS, a.size(2), a.size(3)))
    s = _sums_cpu(a.double().numpy(), b.double().numpy())
    return float(s[0, 1]) / (a.size(1) * (a.size(2) - TAPS + 1) * (a.size(3) - TAPS + 1))


def tensor2img(tensor, out_type=np.uint8, min_max=(0, 1), chroma_mode=None):
    """util.tensor2img (:196-228) for 3D (C, H, W) and 2D (H, W) tensors, any range, RGB channel order -> 3D (H, W, C) BGR or 2D (H, W), [0, 255]
    np.uint8 (default) or [0, 1] of another type.  The make_grid form (4D) and the chroma modes are not part of this build."""
    if chroma_mode is not None:
        raise NotImplementedError('tensor2img: chroma_mode %r (the JPEG colour conversions) is not implemented' % (chroma_mode,))
    tensor = tensor.detach().squeeze().float().cpu()
    n_dim = tensor.dim()
    if n_dim == 4:
        raise NotImplementedError('tensor2img: the image grid of a 4D tensor (torchvision.utils.make_grid) is not implemented')
    if n_dim == 3:
        img_np = np.transpose(tensor.numpy()[[2, 1, 0], :, :], (1, 2, 0))       # HWC, BGR
    elif n_dim == 2:
        img_np = tensor.numpy()
    else:
        raise TypeError('Only support 4D, 3D and 2D tensor. But received with dimension: {:d}'.format(n_dim))
    img_np = (np.clip(img_np, min_max[0], min_max[1]) - min_max[0]) / (min_max[1] - min_max[0])
    if out_type == np.uint8:
        img_np = (img_np * 255.0).round()
    return img_np.astype(out_type)


def sample_std(x):
    """x [S, B, C, H, W], S samples of a batch -> (map [B, C, H, W] float32: 255 times the population STD over S of clamp(x, 0, 1); mean [B] float64: its
    mean per image, from the un-rounded values)"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x))
    if x.dim() != 5:
        raise ValueError('sample_std: x is [S, B, C, H, W], got %s' % (tuple(x.shape),))
    S, B, C, H, W = x.shape
    if min(S, B, C, H, W) < 1:
        raise ValueError('sample_std: empty input %s' % (tuple(x.shape),))
    if not x.is_floating_point():
        x = x.float()
    if not x.is_cuda:
        sd = 255 * np.std(np.clip(x.detach().float().numpy(), 0, 1).astype(np.float64), axis=0)
        return torch.from_numpy(sd.astype(np.float32)), torch.from_numpy(sd.reshape(B, -1).mean(1))
    xd = detach_f32(x)
    with torch.cuda.device(xd.device):
        std_map = torch.empty(B, C, H, W, dtype=torch.float32, device=xd.device)
        partial = torch.empty(B, int(_lib.lib.esr_sample_std_partials(C, H, W)), dtype=torch.float64, device=xd.device)
        sums = torch.empty(B, dtype=torch.float64, device=xd.device)
        check(_lib.lib.esr_sample_std(xd.data_ptr(), S, B, C, H, W, std_map.data_ptr(), partial.data_ptr(), sums.data_ptr(), stream_ptr()), 'esr_sample_std')
    return std_map, sums / (C * H * W)
