#!/usr/bin/env python
"""What the JPEG consistency layer and the DnCNN generator cost (csrc/esr_jpeg.hip, csrc/esr_jpeg16.hip, esr_hip/jpeg.py, esr_hip/dncnn.py):
prints JSON lines.

    python tools/bench_jpeg.py [--steps 20] [--warmup 5]

(i) at 16 x 1 x 256 x 256 and 1 x 1 x 2048 x 2048, microseconds per call (device events around the timed calls, after a warm-up) of the
    compress, extract and extract-grad kernels, each against the reference's formulation in torch ops on the same GPU (a broadcast against
    the cosine grid, a sum and a permute per axis, JPEG.py:108-120 — restated below), with the bytes a call must move (read the input once,
    write the output once: 8 bytes per element) over its time as a fraction of the 8 TB/s HBM peak (about 6.3 TB/s is achievable by a copy);
(i') the colour model's 16-point kernels at 16 x 3 x 256 x 256 and 1 x 3 x 2048 x 2048 next to them: the quantising and the all-coefficient
    compressor, the 384-channel extractor, the 128-channel extractor with the chroma generator's tail, and extractor forward + gradient, each
    against the defining einsum expression of esr_hip/jpeg.py in torch ops on the same GPU; bytes moved = the planes read plus the planes
    written (a K = 8 chroma plane is a quarter of a K = 16 one on the coefficient side);
(ii) the DnCNN(n_channels=320, depth=10, latent 64, 'all_layers') generator at 16 x 32 x 32 blocks: forward, and forward + input gradient,
    on the library's kernels ('split') against the same module on stock torch (MIOpen) on the same GPU.
Each pair is measured twice, interleaved; the second pass is free of one-off set-up."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / steps


class Broadcast:
    """The reference's evaluation of the block transforms in torch ops: per axis a [B, 8, 8, h, w, 8] product with the cosine grid, a sum,
    and a permute that brings the new axis back into place."""

    def __init__(self, device):
        k = torch.arange(8, dtype=torch.float32, device=device)
        self.fwd_grid = torch.cos(math.pi * k.view(1, 8) / 16 * (2 * k.view(8, 1) + 1))                 # [n, k]
        self.fwd_scale = torch.tensor([1 / math.sqrt(8)] + [0.5] * 7, device=device)
        self.inv_grid = self.fwd_grid.t().contiguous() * self.fwd_scale.view(8, 1)                       # [k, n], scaled

    def _axis(self, blocks, axis, grid, scale=None):
        shape = [1] * 6
        shape[axis], shape[5] = 8, 8
        out = (grid.view(shape) * blocks.unsqueeze(-1)).sum(axis)
        if scale is not None:
            out = out * scale
        return out.permute(list(range(axis)) + [4] + list(range(axis, 4)))

    def compress(self, x, q, quantize):
        B, _, H, W = x.shape
        blocks = x.view(B, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3) - 128
        out = self._axis(self._axis(blocks, 1, self.fwd_grid, self.fwd_scale), 2, self.fwd_grid, self.fwd_scale) / q.view(B, 8, 8, 1, 1)
        if quantize:
            out = torch.round(out)
        return out.contiguous().view(B, 64, H // 8, W // 8)

    def extract(self, c, q):
        B, _, h, w = c.shape
        blocks = c.view(B, 8, 8, h, w) * q.view(B, 8, 8, 1, 1)
        out = self._axis(self._axis(blocks, 1, self.inv_grid), 2, self.inv_grid) + 128
        return out.permute(0, 3, 1, 4, 2).contiguous().view(B, 1, 8 * h, 8 * w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_jpeg.py measures on an MI355X'
    from esr_hip import jpeg as J
    import models.modules.architecture as arch
    dev = 'cuda:0'
    gen = torch.Generator().manual_seed(11)
    bc = Broadcast(dev)
    for rep in range(2):
        for shape in ((16, 1, 256, 256), (1, 1, 2048, 2048)):
            B, _, H, W = shape
            x = torch.floor(torch.rand(shape, generator=gen) * 256).to(dev)
            q = torch.randint(1, 100, (B, 64), generator=gen).float().to(dev)
            coef = J.compress(x, q, True)
            d_img = torch.rand(shape, generator=gen).to(dev)
            nbytes = 8 * x.numel()

            def extract_grad_kernel():
                c = coef.detach().requires_grad_(True)
                (J.extract(c, q)[1]).backward(d_img)

            def extract_grad_torch():
                c = coef.detach().requires_grad_(True)
                bc.extract(c, q).backward(d_img)
            check = float((bc.compress(x, q, False) - J.compress(x, q, False)).abs().max()), float((bc.extract(coef, q) - J.extract(coef, q)[1]).abs().max())
            for name, kernel, torch_ops in (('compress (quantising)', lambda: J.compress(x, q, True), lambda: bc.compress(x, q, True)),
                                            ('extract', lambda: J.extract(coef, q), lambda: bc.extract(coef, q)),
                                            ('extract fwd + grad', extract_grad_kernel, extract_grad_torch)):
                tk, tt = timed(kernel, a.steps, a.warmup), timed(torch_ops, a.steps, a.warmup)
                moved = nbytes * (2 if 'grad' in name else 1)
                print(json.dumps({'pass': rep, 'op': name, 'shape': list(shape), 'kernel_us': round(tk * 1e6, 1), 'torch_ops_us': round(tt * 1e6, 1),
                                  'torch_over_kernel': round(tt / tk, 2), 'kernel_GBps': round(moved / tk / 1e9, 1),
                                  'fraction_of_hbm_peak': round(moved / tk / HBM_PEAK, 3), 'max_abs_diff_compress_extract': check}), flush=True)
        for shape in ((16, 3, 256, 256), (1, 3, 2048, 2048)):
            B, _, H, W = shape
            n = B * H * W                                                                   # pixels of one plane
            x = torch.floor(torch.rand(shape, generator=gen) * 256).to(dev)
            q = torch.randint(1, 100, (B, 3, 256), generator=gen).float().to(dev)
            cq, ca = J.compress16(x, q, True), J.compress16(x, q, False)
            y = (torch.rand(B, 128, H // 16, W // 16, generator=gen) * 6 - 3).to(dev)
            d_img = torch.rand(shape, generator=gen).to(dev)
            check = (float((J._compress16_cpu(x, q, 0) - ca).abs().max()), float((J._extract16_cpu(cq, q, None)[1] - J.extract16(cq, q)[1]).abs().max()))

            def grad_of(fn):
                def run():
                    c = cq.detach().requires_grad_(True)
                    fn(c, q, None)[1].backward(d_img)
                return run
            rows = (('compress16 (quantising: Y | Cb, Cr low)', lambda: J.compress16(x, q, True), lambda: J._compress16_cpu(x, q, 2), 4 * (3 * n + 1.5 * n)),
                    ('compress16 (all 3 x 256)', lambda: J.compress16(x, q, False), lambda: J._compress16_cpu(x, q, 0), 4 * (3 * n + 3 * n)),
                    ('extract16 (384 -> YCbCr)', lambda: J.extract16(cq, q), lambda: J._extract16_cpu(cq, q, None), 4 * (1.5 * n + 3 * n)),
                    ('extract16 (128 + generator tail -> Cb, Cr)', lambda: J.extract16(cq, q, y), lambda: J._extract16_cpu(cq, q, y),
                     4 * (0.5 * n + 0.5 * n + 0.5 * n + 2 * n)),
                    ('extract16 (384) fwd + grad', grad_of(J.extract16), grad_of(J._extract16_cpu), 2 * 4 * (1.5 * n + 3 * n)))
            for name, kernel, torch_ops, moved in rows:
                tk, tt = timed(kernel, a.steps, a.warmup), timed(torch_ops, a.steps, a.warmup)
                print(json.dumps({'pass': rep, 'op': name, 'shape': list(shape), 'kernel_us': round(tk * 1e6, 1), 'torch_ops_us': round(tt * 1e6, 1),
                                  'torch_over_kernel': round(tt / tk, 2), 'kernel_GBps': round(moved / tk / 1e9, 1),
                                  'fraction_of_hbm_peak': round(moved / tk / HBM_PEAK, 3), 'max_abs_diff_compress_extract': check}), flush=True)
        net = arch.DnCNN(n_channels=320, depth=10, in_nc=64, out_nc=64, norm_type='batch', latent_input='all_layers', num_latent_channels=64,
                         avoid_padding=False, output_layer='Sigmoid').to(dev).eval()
        for p in net.parameters():
            p.requires_grad_(False)
        xin = torch.cat([torch.rand(16, 64, 32, 32, generator=gen) * 2 - 1, torch.round(torch.rand(16, 64, 32, 32, generator=gen) * 16 - 8)], 1).to(dev)

        def both(fn):
            def run():
                xi = xin.detach().requires_grad_(True)
                fn(xi).sum().backward()
            return run
        with torch.no_grad():
            tkf, ttf = timed(lambda: net.pre_output(xin), a.steps, a.warmup), timed(lambda: net._torch_chain(xin, True), a.steps, a.warmup)
        tkb, ttb = timed(both(net.pre_output), a.steps, a.warmup), timed(both(lambda t: net._torch_chain(t, True)), a.steps, a.warmup)
        print(json.dumps({'pass': rep, 'op': 'DnCNN 320 x 10, latent 64, all_layers', 'shape': list(xin.shape), 'kernel_fwd_us': round(tkf * 1e6, 1),
                          'torch_fwd_us': round(ttf * 1e6, 1), 'kernel_fwd_bwd_us': round(tkb * 1e6, 1), 'torch_fwd_bwd_us': round(ttb * 1e6, 1),
                          'torch_over_kernel_fwd': round(ttf / tkf, 2), 'torch_over_kernel_fwd_bwd': round(ttb / tkb, 2)}), flush=True)


if __name__ == '__main__':
    main()
