"""Pictures and scores of the explorable JPEG decoder's output — what the reference's codes/test_JPEG.py:165-327 computes on the host after
copying every sample as fp32: util.tensor2img's chroma branches (utils/util.py:209-226), PSNR / SSIM of every decoded sample and of the
plainly decompressed image against the ground truth, and in 'stats' mode the per-pixel STD over the Z samples.  esr_hip.metrics keeps the SR
half's conversions (its tensor2img refuses chroma_mode); this module is the JPEG half's, under names of its own.

The decoder's images hold 0...255: one plane for chroma_mode 'Y', three (Y, Cb, Cr) for 'YCbCr'.  A pixel becomes three 0...255 values
(R, G, B) by the chain include/esr_hip.h states before esr_ycbcr_image — tensor2img through data.util.ycbcr2rgb in fp32 and fp64, then
tensor2img's clip and rounding; both routes below compute it.

* image(t, chroma_mode, out_type, min_max) -> the NumPy HWC BGR array tensor2img returns (a list for a batch).  CUDA tensors with uint8
  output: esr_ycbcr_image and one 3-byte-per-pixel copy.  CPU tensors, other out_types: the defining NumPy expression.
* psnr_ssim(a, b, chroma_mode, min_max, crop_border) -> (psnr [Ba], ssim [Ba]) float64 of the uint8 pictures; b holds one image or Ba.
  CUDA: esr_psnr_ssim_ycbcr, nothing converted is written, no synchronisation.  CPU: image() and metrics.calculate_psnr / calculate_ssim.
* sample_std(x [S, B, C, H, W], chroma_mode) -> (map [B, 3, H, W] float32 in R, G, B planes, mean [B] float64): np.std over the S pictures.
* evaluate(model, loader, Z, crop_border): the reference's evaluation loop without its files.

On the device the chain's fp64 terms are added in the stated order without fused multiply-adds; NumPy's matmul may differ by one fp64 ulp,
which can move a rounded pixel by one level only where the value before rounding lies within about 1e-5 of a half-integer.
"""
import numpy as np
import torch

import data.util as data_util
from . import _lib, metrics
from ._image import detach_f32
from ._lib import check
from .act import stream_ptr

MODES = ('Y', 'YCbCr')


def _mode_planes(chroma_mode):
    if chroma_mode not in MODES:
        raise ValueError("jpeg_metrics: chroma_mode is 'Y' or 'YCbCr', got %r" % (chroma_mode,))
    return 1 if chroma_mode == 'Y' else 3


def _as_batch(t, chroma_mode, leading=0):
    """t as a float tensor [..., C, H, W] with `leading` + 1 batch axes in front of C; (tensor, whether a batch axis was given).  A 2-D or
    [1, H, W] image is 'Y', a [3, H, W] image is 'YCbCr': the other pairing is refused with the reference's message (util.py:210, :217)."""
    C = _mode_planes(chroma_mode)
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.asarray(t))
    if not t.is_floating_point():
        t = t.float()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    batched = t.dim() == 4 + leading
    if t.dim() == 3:
        t = t[(None,) * (1 + leading)]
    if t.dim() != 4 + leading:
        raise TypeError('Only support 4D, 3D and 2D tensor. But received with dimension: {:d}'.format(t.dim()))
    if t.size(-3) == 3 and C == 1:
        raise ValueError('3-channels image input with %s chroma mode' % (chroma_mode,))
    if t.size(-3) == 1 and C == 3:
        raise ValueError('Single-channels image input with %s chroma mode' % (chroma_mode,))
    if t.size(-3) != C:
        raise ValueError('jpeg_metrics: %d-channel images (chroma mode %s takes %d)' % (t.size(-3), chroma_mode, C))
    if min(t.shape) < 1:
        raise ValueError('jpeg_metrics: empty input %s' % (tuple(t.shape),))
    return t, batched


def _range(min_max):
    lo, hi = float(np.float32(min_max[0])), float(np.float32(min_max[1]))
    if not hi > lo:
        raise ValueError('jpeg_metrics: min_max needs max > min, got (%r, %r)' % (min_max[0], min_max[1]))
    return lo, hi


def bgr_0_255(img, chroma_mode):
    """tensor2img's chroma branch (util.py:213, :220) on one float32 [C, H, W] array in 0...255 -> float32 HWC in B, G, R order, before the clip"""
    assert img.dtype == np.float32
    if chroma_mode == 'YCbCr':
        ycc = np.transpose(img / 255, (1, 2, 0))
    else:
        ycc = np.stack([img[0] / 255] + 2 * [128 / 255 * np.ones_like(img[0])], -1)
    return 255 * data_util.ycbcr2rgb(ycc)[:, :, [2, 1, 0]]


def _image_cpu(img, chroma_mode, lo, hi, out_type):
    quantize = out_type == np.uint8
    p = metrics._pixels_cpu(bgr_0_255(img, chroma_mode), lo, hi, quantize)
    return (p if quantize else p / np.float32(255.0)).astype(out_type)


def image(t, chroma_mode, out_type=np.uint8, min_max=(0, 255)):
    """util.tensor2img(t, out_type, min_max, chroma_mode): a 2-D or [1, H, W] tensor ('Y') or a [3, H, W] tensor ('YCbCr') in the range min_max
    -> [H, W, 3] BGR, [0, 255] np.uint8 (default) or [0, 1] of another type; a tensor with a leading batch axis -> the list of its images."""
    t, batched = _as_batch(t, chroma_mode)
    lo, hi = _range(min_max)
    B, C, H, W = t.shape
    if t.is_cuda and out_type == np.uint8:
        x = detach_f32(t)
        with torch.cuda.device(x.device):
            out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
            check(_lib.lib.esr_ycbcr_image(x.data_ptr(), B, C, H, W, lo, hi, out.data_ptr(), stream_ptr()), 'esr_ycbcr_image')
        imgs = list(out.cpu().numpy())
    else:
        x = t.detach().float().cpu().numpy()
        imgs = [_image_cpu(im, chroma_mode, lo, hi, out_type) for im in x]
    return imgs if batched else imgs[0]


def _check_pair(a, b, chroma_mode, crop_border):
    a, _ = _as_batch(a, chroma_mode)
    b, _ = _as_batch(b, chroma_mode)
    if a.shape[1:] != b.shape[1:] or b.size(0) not in (1, a.size(0)):
        raise ValueError('Input images must have the same dimensions.')
    if a.device != b.device:
        raise ValueError('jpeg_metrics: the images are on %s and %s' % (a.device, b.device))
    border = int(crop_border)
    Hc, Wc = a.size(2) - 2 * border, a.size(3) - 2 * border
    if border < 0 or Hc < 1 or Wc < 1:
        raise ValueError('jpeg_metrics: crop_border %d leaves nothing of a %d x %d image' % (border, a.size(2), a.size(3)))
    if Hc < metrics.TAPS or Wc < metrics.TAPS:
        raise ValueError('SSIM needs %d x %d pixels, %d x %d are left after cropping' % (metrics.TAPS, metrics.TAPS, Hc, Wc))
    return a, b, border, Hc, Wc


def psnr_ssim(a, b, chroma_mode, min_max=(0, 255), crop_border=0):
    """(psnr [Ba], ssim [Ba]) float64 on the inputs' device, of the uint8 pictures of a ([Ba, C, H, W] or one image) against those of b (as many
    images, or one that every image of a is scored against), crop_border pixels dropped on every side (util.calculate_psnr / calculate_ssim of
    tensor2img's outputs, test_JPEG.py:239-275)"""
    a, b, border, Hc, Wc = _check_pair(a, b, chroma_mode, crop_border)
    lo, hi = _range(min_max)
    Ba, C, H, W = a.shape
    if a.is_cuda:
        ad, bd = detach_f32(a), detach_f32(b)
        with torch.cuda.device(ad.device):
            n = int(_lib.lib.esr_psnr_ssim_ycbcr_partials(C, H, W, border))
            partial = torch.empty(Ba, n, 2, dtype=torch.float64, device=ad.device)
            sums = torch.empty(Ba, 2, dtype=torch.float64, device=ad.device)
            check(_lib.lib.esr_psnr_ssim_ycbcr(ad.data_ptr(), bd.data_ptr(), Ba, C, H, W, C * H * W if bd.size(0) == Ba and Ba > 1 else 0, lo, hi, border,
                                               partial.data_ptr(), sums.data_ptr(), stream_ptr()), 'esr_psnr_ssim_ycbcr')
        mse = sums[:, 0] / (3 * Hc * Wc)
        return 20 * torch.log10(255.0 / torch.sqrt(mse)), sums[:, 1] / (3 * (Hc - metrics.TAPS + 1) * (Wc - metrics.TAPS + 1))
    crop = (slice(border, H - border), slice(border, W - border))
    ia, ib = ([im[crop] for im in image(t, chroma_mode, np.uint8, min_max)] for t in (a, b))
    pairs = [(ia[i], ib[i if len(ib) > 1 else 0]) for i in range(Ba)]
    return (torch.tensor([metrics.calculate_psnr(x, y) for x, y in pairs], dtype=torch.float64),
            torch.tensor([metrics.calculate_ssim(x, y) for x, y in pairs], dtype=torch.float64))


def _sample_std_cpu(x, chroma_mode):
    """float64 [B, 3, H, W]: np.std(np.stack(sr_imgs), 0) of test_JPEG.py:263, as R, G, B planes"""
    S, B = x.shape[:2]
    maps = [np.std(np.stack([image(x[s, b], chroma_mode) for s in range(S)]), 0) for b in range(B)]
    return np.stack([np.ascontiguousarray(m[:, :, ::-1].transpose(2, 0, 1)) for m in maps])


def sample_std(x, chroma_mode):
    """x [S, B, C, H, W], S samples of a batch in 0...255 -> (map [B, 3, H, W] float32: the population STD over S of the uint8 pictures, in R, G,
    B planes; mean [B] float64: its mean per image, from the un-rounded values).  S = 1 gives zeros."""
    if torch.is_tensor(x) and x.dim() != 5 or not torch.is_tensor(x) and np.ndim(x) != 5:
        raise ValueError('sample_std: x is [S, B, C, H, W], got %s' % (tuple(np.shape(x)),))
    x, _ = _as_batch(x, chroma_mode, leading=1)
    S, B, C, H, W = x.shape
    if not x.is_cuda:
        sd = _sample_std_cpu(x, chroma_mode)
        return torch.from_numpy(sd.astype(np.float32)), torch.from_numpy(sd.reshape(B, -1).mean(1))
    xd = detach_f32(x)
    with torch.cuda.device(xd.device):
        std_map = torch.empty(B, 3, H, W, dtype=torch.float32, device=xd.device)
        partial = torch.empty(B, int(_lib.lib.esr_sample_std_ycbcr_partials(C, H, W)), dtype=torch.float64, device=xd.device)
        sums = torch.empty(B, dtype=torch.float64, device=xd.device)
        check(_lib.lib.esr_sample_std_ycbcr(xd.data_ptr(), S, B, C, H, W, 0.0, 255.0, std_map.data_ptr(), partial.data_ptr(), sums.data_ptr(),
                                            stream_ptr()), 'esr_sample_std_ycbcr')
    return std_map, sums / (3 * H * W)


def evaluate(model, loader, Z=None, crop_border=0):
    """The evaluation loop of codes/test_JPEG.py:165-327 without its file output, over the items of `loader` (one image each: a JpegDataset
    behind data.create_dataloader in a 'val' / 'test' phase).  Z: [S, nz, 1, 1] latent samples, spatially uniform — every image is decoded S
    times in one batch; None: one pass with Z = 0 (the reference's Z_latent = [0]).  Per image: PSNR / SSIM of every decoded sample and of the
    plainly decompressed image (model.Return_Compressed) against the item's own 'Uncomp' — kept aside before feed_data, because the colour
    model's generated Y plane is not the ground truth's (the reference's gt_im_YCbCr) — and the per-pixel STD over the S samples.
    -> {'psnr', 'ssim': float64 [N, S]; 'psnr_quantized', 'ssim_quantized', 'pixel_std': [N]; 'paths': the N 'Uncomp_path's; and the three
    lines of the reference's stats.txt (:321-326) as numbers: 'std_of_image_mean_std', 'mean_pixel_std', 'std_of_pixel_std'}.
    With a model on the GPU every score stays there until the last image is done: one synchronisation for the whole set."""
    chroma_mode = 'YCbCr' if model.chroma_mode else 'Y'
    if Z is not None:
        Z = torch.as_tensor(Z)
        if Z.dim() != 4 or Z.shape[2:] != (1, 1):
            raise ValueError('evaluate: Z is [S, nz, 1, 1], got %s' % (tuple(Z.shape),))
    S = 1 if Z is None else Z.size(0)
    scores, quantized, maps, sums, paths = [], [], [], [], []
    for item in loader:
        gt = item['Uncomp'].clone()
        if gt.size(0) != 1:
            raise ValueError('evaluate: the loader yields one image per item, got a batch of %d' % gt.size(0))
        data = {'Uncomp': item['Uncomp'].repeat(S, 1, 1, 1), 'QF': torch.as_tensor(item['QF']).reshape(-1).repeat(S)}
        if model.latent_input is not None:
            data['Z'] = 0 if Z is None else Z.to(torch.float32)
        model.feed_data(data, need_GT=True)
        model.test()
        decoded = model.Output_Batch(within_0_1=False).detach()
        gt = gt.to(decoded.device)
        scores.append(torch.stack(psnr_ssim(decoded, gt, chroma_mode, crop_border=crop_border)))
        for module in model.JPEG.values():
            module.Set_Q_Table(data['QF'][:1])
        with torch.no_grad():
            quantized.append(torch.cat(psnr_ssim(model.Return_Compressed(gt), gt, chroma_mode, crop_border=crop_border)))
        if decoded.is_cuda:
            std_map, mean = sample_std(decoded.unsqueeze(1), chroma_mode)
            std_map = std_map.double()
        else:                                                   # the float64 map np.std gives, not its float32 copy
            std_map = torch.from_numpy(_sample_std_cpu(decoded.unsqueeze(1), chroma_mode))
            mean = std_map.reshape(1, -1).mean(1)
        maps.append(std_map[0].reshape(3, -1))
        sums.append(mean[0] * std_map[0].numel())
        paths.append(item['Uncomp_path'][0] if 'Uncomp_path' in item else None)
    if not scores:
        raise ValueError('evaluate: the loader is empty')
    scores, quantized = torch.stack(scores), torch.stack(quantized)                   # [N, 2, S], [N, 2]
    counts = torch.tensor([m.numel() for m in maps], dtype=torch.float64, device=scores.device)
    sums = torch.stack(sums)
    every = torch.cat(maps, 1)                                                        # [3, all pixels]: the reference's concatenated [-1, 3] array
    stats = torch.stack([(sums / counts).std(unbiased=False), sums.sum() / counts.sum(), every.std(dim=1, unbiased=False).mean()])
    scores, quantized, pixel_std, stats = (t.cpu().numpy() for t in (scores, quantized, sums / counts, stats))
    return {'psnr': scores[:, 0], 'ssim': scores[:, 1], 'psnr_quantized': quantized[:, 0], 'ssim_quantized': quantized[:, 1],
            'pixel_std': pixel_std, 'paths': paths, 'std_of_image_mean_std': float(stats[0]), 'mean_pixel_std': float(stats[1]),
            'std_of_pixel_std': float(stats[2])}
