#!/usr/bin/env python
"""What the patch-magnitude Z objective costs (esr_hip/patchmag.py, csrc/esr_patchmag.hip): prints JSON lines.

    python tools/bench_special_z.py [--steps 20] [--warmup 5]

Per batch size (1 and 64) at 3 x 512 x 512, whole-image patch set (9325 patches, one corner in 27): microseconds per forward + backward of
  kernel   patch_mag(x, spec).sum().backward()
  torch    the same loss written with torch indexing ops on the same GPU: clamp, channel mean, a gather of the [P, 49] patch indexes,
           the squared difference to the desired patches and a mean, differentiated by autograd (its backward scatters with index_put)
and the largest difference between the two gradients, so that the two are known to compute the same thing.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

C, H, W = 3, 512, 512


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_special_z.py measures on an MI355X'
    from esr_hip import patchmag
    gen = torch.Generator().manual_seed(5)
    spec = patchmag.MagSpec(None, H, W, torch.rand(C, H, W, generator=gen), 0.03, 1)
    _, desired, idx = spec.on('cuda')
    for B in (1, 64, 1, 64):                                    # twice, interleaved: the second pair is free of one-off set-up
        x = (torch.rand(B, C, H, W, generator=gen) * 1.2 - 0.1).cuda().requires_grad_(True)

        def kernel():
            x.grad = None
            patchmag.patch_mag(x, spec).sum().backward()

        def torch_ops():
            x.grad = None
            v = torch.clamp(x, 0, 1).mean(1).reshape(B, -1)
            ((v[:, idx] - desired) ** 2).mean(dim=(1, 2)).sum().backward()
        tk = timed(kernel, a.steps, a.warmup)
        gk = x.grad.clone()
        tt = timed(torch_ops, a.steps, a.warmup)
        diff = float((gk - x.grad).abs().max() / x.grad.abs().max())
        print(json.dumps({'term': 'patch_mag fwd+bwd', 'shape': [B, C, H, W], 'patches_per_image': spec.P, 'kernel_us': round(tk * 1e6, 1),
                          'torch_ops_us': round(tt * 1e6, 1), 'torch_over_kernel': round(tt / tk, 2), 'grad_rel_diff': diff}), flush=True)


if __name__ == '__main__':
    main()
