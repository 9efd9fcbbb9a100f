#!/usr/bin/env python
"""What evaluating the JPEG decoder's output costs (esr_hip/jpeg_metrics.py, csrc/esr_metrics.hip): prints JSON lines.

    python tools/bench_jpeg_metrics.py [--steps 20] [--warmup 3] [--host-steps 3] [--model chroma|y|both]

One image of the decoder's own shape, 1 x 512 x 768, decoded for S = 50 latent samples: a [50, C, 512, 768] tensor in 0...255 on the GPU
(C = 3 YCbCr for the chroma model, C = 1 for the Y model) and its ground truth.  Both routes produce what codes/test_JPEG.py:165-327 produces
per image — PSNR and SSIM of every sample, the mean of the per-pixel STD over the samples, and the S uint8 BGR pictures on the host:

  device  jpeg_metrics.psnr_ssim + sample_std + image (the pictures cross as uint8, 3 bytes per pixel) + the scores' copy to the host;
          also the three kernels alone between device events
  host    the reference's pattern: an fp32 copy of every sample (12 or 4 bytes per pixel), the NumPy conversion (image() on CPU tensors),
          metrics.calculate_psnr / calculate_ssim per sample, np.std of the stacked pictures

Every timed region ends in a synchronisation (the host route's copies are synchronisations themselves).  Both routes are warmed up, their
rounds alternate in blocks, and the median and the minimum are printed; `max_score_difference` is the largest |device - host| over the 50 PSNR and SSIM values.
No threshold: the figures go into DESIGN.md with their date and commit.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

S, H, W = 50, 512, 768


def decoded(C):
    """(samples [S, C, H, W], ground truth [1, C, H, W]) on the GPU: a smooth image in the YCbCr of natural pictures plus noise per sample"""
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing='ij')
    base = torch.stack([60 + 120 * yy + 40 * torch.sin(9 * xx), 128 + 30 * (xx - 0.5), 128 - 30 * (yy - 0.5)])[:C]
    gt = (base + 6 * torch.randn(C, H, W, generator=g))[None]
    x = gt + 4 * torch.randn(S, C, H, W, generator=g)
    return x.cuda(), gt.cuda()


def timed(fn):
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def alternating_rounds(device_route, host_route, steps, warmup, host_steps):
    """both routes warmed up, then host_steps blocks of (steps / host_steps device rounds, one host round): the two share whatever else the machine
    is doing"""
    for _ in range(warmup):
        device_route()
    host_route()
    torch.cuda.synchronize()
    t_dev, t_host = [], []
    for _ in range(host_steps):
        for _ in range(max(1, steps // host_steps)):
            dev, t = timed(device_route)
            t_dev.append(t)
        host, t = timed(host_route)
        t_host.append(t)
    return dev, t_dev, host, t_host


def kernels_alone(x, gt, C, steps, warmup):
    from esr_hip import _lib
    from esr_hip.act import stream_ptr
    lib, s = _lib.lib, stream_ptr()
    partial = torch.empty(S, int(lib.esr_psnr_ssim_ycbcr_partials(C, H, W, 0)), 2, dtype=torch.float64, device='cuda')
    sums = torch.empty(S, 2, dtype=torch.float64, device='cuda')
    std_map = torch.empty(1, 3, H, W, device='cuda')
    std_partial = torch.empty(int(lib.esr_sample_std_ycbcr_partials(C, H, W)), dtype=torch.float64, device='cuda')
    std_sum = torch.empty(1, dtype=torch.float64, device='cuda')
    pictures = torch.empty(S, H, W, 3, dtype=torch.uint8, device='cuda')
    calls = {
        'psnr_ssim': lambda: lib.esr_psnr_ssim_ycbcr(x.data_ptr(), gt.data_ptr(), S, C, H, W, 0, 0.0, 255.0, 0, partial.data_ptr(), sums.data_ptr(), s),
        'sample_std': lambda: lib.esr_sample_std_ycbcr(x.data_ptr(), S, 1, C, H, W, 0.0, 255.0, std_map.data_ptr(), std_partial.data_ptr(), std_sum.data_ptr(), s),
        'image': lambda: lib.esr_ycbcr_image(x.data_ptr(), S, C, H, W, 0.0, 255.0, pictures.data_ptr(), s),
    }
    out = {}
    for name, fn in calls.items():
        for _ in range(warmup):
            _lib.check(fn(), name)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        end.record()
        torch.cuda.synchronize()
        out[name + '_kernels_ms'] = round(start.elapsed_time(end) / steps, 4)
    return out


def bench(C, steps, warmup, host_steps):
    from esr_hip import jpeg_metrics, metrics
    mode = 'YCbCr' if C == 3 else 'Y'
    x, gt = decoded(C)

    def device_route():
        psnr, ssim = jpeg_metrics.psnr_ssim(x, gt, mode)
        _, std = jpeg_metrics.sample_std(x.unsqueeze(1), mode)
        pictures = jpeg_metrics.image(x, mode)
        return psnr.cpu().numpy(), ssim.cpu().numpy(), float(std), pictures

    def host_route():
        samples, truth = x.float().cpu(), gt.float().cpu()
        gt_img = jpeg_metrics.image(truth[0], mode)
        pictures = [jpeg_metrics.image(t, mode) for t in samples]
        psnr = np.array([metrics.calculate_psnr(im, gt_img) for im in pictures])
        ssim = np.array([metrics.calculate_ssim(im, gt_img) for im in pictures])
        return psnr, ssim, float(np.mean(np.std(np.stack(pictures), 0))), pictures

    dev, t_dev, host, t_host = alternating_rounds(device_route, host_route, steps, warmup, host_steps)
    differing = sum(int((a != b).any(-1).sum()) for a, b in zip(dev[3], host[3]))
    ms = lambda t: round(t * 1e3, 3)            # noqa: E731
    line = {'model': 'chroma' if C == 3 else 'y', 'shape': [S, C, H, W],
            'device_ms_median': ms(statistics.median(t_dev)), 'device_ms_min': ms(min(t_dev)), 'device_rounds': len(t_dev),
            'host_ms_median': ms(statistics.median(t_host)), 'host_ms_min': ms(min(t_host)), 'host_rounds': len(t_host),
            'max_score_difference': float(max(np.abs(dev[0] - host[0]).max(), np.abs(dev[1] - host[1]).max())),
            'pixel_std_difference': abs(dev[2] - host[2]), 'differing_pixels': differing, 'pixels': S * H * W,
            'copied_MB_device': S * H * W * 3 / 1e6, 'copied_MB_host': 4 * (S + 1) * C * H * W / 1e6, 'torch_threads': torch.get_num_threads()}
    line.update(kernels_alone(x, gt, C, steps, warmup))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-steps', type=int, default=3)
    ap.add_argument('--model', default='both', choices=['chroma', 'y', 'both'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_jpeg_metrics.py measures on an MI355X'
    for C, name in ((3, 'chroma'), (1, 'y')):
        if a.model in ('both', name):
            bench(C, a.steps, a.warmup, a.host_steps)


if __name__ == '__main__':
    main()
