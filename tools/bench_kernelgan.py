#!/usr/bin/env python
"""What one kernel-estimation iteration costs on the device (esr_hip/kernelgan.py, csrc/esr_kgan.hip): prints JSON lines.

    python tools/bench_kernelgan.py [--steps 100] [--warmup 20] [--rounds 5] [--batches 1,4,16] [--recover ITERS]

  step     ms per iteration (G step + D step on 64 x 64 / 26 x 26 crops, 64 channels) of the 'hip' engine at E = 1, 4, 16 and of the 'stock'
           engine (torch.nn modules on the same GPU, one estimation) in the same process, alternating: `rounds` windows of `steps` iterations
           each, a host clock around work that ends in a synchronise, the median window.  ms per estimation = ms per iteration / E.
  recover  (--recover ITERS > 0) a textured image blurred by a known anisotropic Gaussian and sub-sampled by 2: the 'hip' engine's x2 kernel after
           ITERS iterations, its distance to the true kernel and the bicubic kernel's distance, both as the L2 norm of the difference of the
           kernels centred on a 21 x 21 canvas.
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


def window(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def bench_step(steps, warmup, rounds, batches):
    from esr_hip.kernelgan import KernelGanEngine
    from KernelGAN.configs import Config
    from KernelGAN.kernelGAN import StockEngine
    conf = Config().parse([])
    g = torch.Generator().manual_seed(3)
    runs = {}
    for E in batches:
        eng = KernelGanEngine(E, conf)
        g_in, d_in = (torch.rand(E, 3, 64, 64, generator=g) * 2 - 1).cuda(), (torch.rand(E, 3, 26, 26, generator=g) * 2 - 1).cuda()
        noise = torch.randn(E, 3, 26, 26, generator=g).cuda()
        runs['hip E=%d' % E] = (E, lambda eng=eng, a=g_in, b=d_in, n=noise: eng.step(a, b, n, slot=0))
    stock = StockEngine(conf, 'cuda', torch.float32)
    sg, sd = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).cuda(), (torch.rand(1, 3, 26, 26, generator=g) * 2 - 1).cuda()
    sn = torch.randn(1, 3, 26, 26, generator=g).cuda()
    runs['stock E=1'] = (1, lambda: stock.train(sg, sd, sn))
    for _, fn in runs.values():
        window(fn, warmup)
    times = {k: [] for k in runs}
    for _ in range(rounds):                                   # alternate the engines: whatever else the host does hits all of them
        for k, (_, fn) in runs.items():
            times[k].append(window(fn, steps))
    base = statistics.median(times['stock E=1'])
    for k, (E, _) in runs.items():
        med = statistics.median(times[k])
        print(json.dumps({'part': 'step', 'engine': k, 'ms_per_iteration': round(med, 4), 'ms_per_estimation_iteration': round(med / E, 4),
                          'windows_ms': [round(t, 4) for t in times[k]], 'stock_over_this_per_estimation': round(base / (med / E), 2),
                          'seconds_per_3000_iterations_per_estimation': round(med / E * 3, 2)}), flush=True)


def true_kernel(size=13):
    yy, xx = np.mgrid[:size, :size] - (size - 1) / 2 - 0.5            # centre of mass where a x2 kernel has it
    k = np.exp(-(yy ** 2 / (2 * 2.2 ** 2) + xx ** 2 / (2 * 1.0 ** 2) + 0.25 * yy * xx))
    return k / k.sum()


def blurred_image(k, seed=0, H=192, W=160):
    rng = np.random.RandomState(seed)
    pad = k.shape[0]
    big = np.kron(rng.rand((2 * H + 2 * pad) // 6 + 2, (2 * W + 2 * pad) // 6 + 2, 3), np.ones((6, 6, 1)))[:2 * H + pad, :2 * W + pad]
    big = 0.6 * big + 0.4 * rng.rand(*big.shape)
    from scipy.signal import correlate2d
    out = np.stack([correlate2d(big[:, :, c], k, 'valid')[::2, ::2][:H, :W] for c in range(3)], axis=2)
    return np.clip(np.round(out * 255), 0, 255).astype(np.uint8)


def on_canvas(k, side=21):
    from scipy.ndimage import center_of_mass, shift
    c = np.zeros((side, side))
    o = (side - k.shape[0]) // 2
    c[o:o + k.shape[0], o:o + k.shape[1]] = k
    return shift(c, (side - 1) / 2 - np.array(center_of_mass(c)))


def kernel_distance(a, b):
    return float(np.linalg.norm(on_canvas(a / a.sum()) - on_canvas(b / b.sum())))


def bench_recover(iters):
    from KernelGAN import train as KernelGAN
    from KernelGAN import util
    k = true_kernel()
    conf = KernelGAN.Config().parse(['--max_iters', str(iters)])
    conf.LR_image = blurred_image(k)
    torch.manual_seed(0)
    np.random.seed(0)
    t = time.perf_counter()
    est = KernelGAN.train(conf, engine='hip')
    dt = time.perf_counter() - t
    b = 0.5 * util.cubic(0.5 * (np.arange(8) - 3.5))
    print(json.dumps({'part': 'recover', 'engine': 'hip', 'iterations': iters, 'seconds': round(dt, 2), 'distance_estimated_to_true': round(kernel_distance(est, k), 4),
                      'distance_bicubic_to_true': round(kernel_distance(np.outer(b, b), k), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', default='1,4,16')
    ap.add_argument('--recover', type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_kernelgan.py measures on an MI355X'
    bench_step(a.steps, a.warmup, a.rounds, [int(b) for b in a.batches.split(',')])
    if a.recover > 0:
        bench_recover(a.recover)


if __name__ == '__main__':
    main()
