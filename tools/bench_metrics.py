#!/usr/bin/env python
"""What scoring an SR output costs (esr_hip/metrics.py, csrc/esr_metrics.hip): prints JSON lines.

    python tools/bench_metrics.py [--steps 200] [--warmup 20] [--part all|device|host|std]

  device  psnr_ssim on 512 x 512 x 3 pairs on the GPU: the wrapper call (allocations, both launches, the [B] finalisation; a host clock around
          `steps` calls that end in one synchronise) and the two launches alone between device events, for one pair and for a batch of 64, against
          the algorithmic traffic of 2 x 4 B per pixel
  host    the same pair the way SRRaGANModel.perform_validation scores it — get_current_visuals() (two device-to-host copies, each a
          synchronise) and the NumPy PSNR — and the float64 SSIM of the host path (metrics.psnr_ssim on CPU tensors), for scale
  std     sample_std over 64 Z samples of one 512 x 512 x 3 image against its traffic (every sample read once, the fp32 map written once;
          the second read of the samples is left to the caches)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

C, H, W = 3, 512, 512


def host_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def event_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / steps


def pair(B):
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(B, C, H, W, generator=g)
    return (hr + 0.05 * torch.randn(B, C, H, W, generator=g)), hr


def bench_device(steps, warmup):
    from esr_hip import _lib, metrics
    from esr_hip.act import stream_ptr
    for B in (1, 64):
        sr, hr = (t.cuda() for t in pair(B))
        call = host_timed(lambda: metrics.psnr_ssim(sr, hr), steps, warmup)
        partial = torch.empty(B, int(_lib.lib.esr_psnr_ssim_partials(C, H, W, 0)), 2, dtype=torch.float64, device='cuda')
        sums = torch.empty(B, 2, dtype=torch.float64, device='cuda')
        s = stream_ptr()
        kernels = event_timed(lambda: _lib.check(_lib.lib.esr_psnr_ssim(sr.data_ptr(), hr.data_ptr(), B, C, H, W, 0.0, 1.0, 0, 0, partial.data_ptr(),
                                                                         sums.data_ptr(), s), 'esr_psnr_ssim'), steps, warmup)
        nbytes = 2 * 4 * B * C * H * W
        print(json.dumps({'part': 'device', 'shape': [B, C, H, W], 'call_us_per_pair': round(call / B * 1e6, 2), 'kernels_us_per_pair': round(kernels / B * 1e6, 2),
                          'call_ms': round(call * 1e3, 4), 'kernels_ms': round(kernels * 1e3, 4), 'algorithmic_MB': nbytes / 1e6,
                          'kernels_GBps': round(nbytes / kernels / 1e9, 1)}), flush=True)


def bench_host(steps, warmup):
    from esr_hip import metrics
    sr, hr = (t.cuda() for t in pair(1))

    def parent_route():                                    # get_current_visuals() + the PSNR lines of perform_validation
        s, h = sr[0].detach().float().cpu(), hr[0].detach().float().cpu()
        a = 255 * np.clip(s.numpy(), 0, 1).transpose(1, 2, 0).astype(np.float32)
        b = 255 * np.clip(h.numpy(), 0, 1).transpose(1, 2, 0).astype(np.float32)
        mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
        return float('inf') if mse == 0 else 20 * np.log10(255.0 / np.sqrt(mse))

    t_parent = host_timed(parent_route, steps, warmup)
    cs, ch = sr.cpu(), hr.cpu()
    n = max(1, steps // 20)
    t = time.perf_counter()
    for _ in range(n):
        metrics.psnr_ssim(cs, ch)
    t_ssim = (time.perf_counter() - t) / n
    print(json.dumps({'part': 'host', 'shape': [1, C, H, W], 'copy_and_numpy_psnr_ms': round(t_parent * 1e3, 3),
                      'host_float64_psnr_ssim_ms': round(t_ssim * 1e3, 2), 'torch_threads': torch.get_num_threads()}), flush=True)


def bench_std(steps, warmup):
    from esr_hip import metrics
    S = 64
    x = torch.rand(S, 1, C, H, W, generator=torch.Generator().manual_seed(9)).cuda()
    call = host_timed(lambda: metrics.sample_std(x), steps, warmup)
    nbytes = 4 * (S + 1) * C * H * W
    print(json.dumps({'part': 'std', 'shape': [S, 1, C, H, W], 'call_ms': round(call * 1e3, 4), 'algorithmic_MB': nbytes / 1e6,
                      'call_GBps': round(nbytes / call / 1e9, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--part', default='all', choices=['all', 'device', 'host', 'std'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_metrics.py measures on an MI355X'
    if a.part in ('all', 'device'):
        bench_device(a.steps, a.warmup)
    if a.part in ('all', 'host'):
        bench_host(a.steps, a.warmup)
    if a.part in ('all', 'std'):
        bench_std(a.steps, a.warmup)


if __name__ == '__main__':
    main()
