#!/usr/bin/env python
"""What the scribble Z objective costs (esr_hip/scribble.py, csrc/esr_scribble.hip): prints JSON lines.

    python tools/bench_scribble.py [--steps 5] [--warmup 2] [--part all|terms|torch|z]

  terms   forward and forward + backward of the fused term at configs[3]'s shape, 64 x 3 x 512^2, with 8 TV regions, the L1 labels and the
          region constraint on (I0 of batch 64), against its algorithmic bytes (every input read once, every output written once)
  torch   the reference's formulation restated in torch (codes/Z_optimization.py:424-446 and the constraining l1: per image one masked L1 and,
          per TV region, four shifted masked differences; one l1 for the constraint) on the same GPU, forward + backward
  z       one Z_optimizer.optimize() iteration at bench.py --workload c4's shape (RRDB-23 x4 lat 3 + CEM, 64 Z samples of 512^2) with
          'scribble' (region constraint on) against the same iteration with 'STD_increase', same masks, in one process
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, C, H, W = 64, 3, 512, 512
REGIONS = 8


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def edit():
    """an image mask (a 320 x 320 square) and a label map inside it: colour, brighten, darken strips and 8 TV regions side by side"""
    mask = np.zeros((H, W), np.float32)
    mask[96:416, 96:416] = 1
    s = np.zeros((H, W), np.int64)
    s[100:140, 100:400] = 1
    s[140:170, 100:400] = 2
    s[170:200, 100:400] = 3
    for k in range(REGIONS):
        s[210:410, 100 + 37 * k: 137 + 37 * k] = 4 + k
    return mask, s


def bench_terms(steps, warmup):
    from esr_hip import scribble
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, C, H, W, generator=g).cuda().requires_grad_(True)
    I0 = torch.rand(B, C, H, W, generator=g).cuda()
    D = torch.rand(1, C, H, W, generator=g).cuda()
    mask, s = edit()
    spec = scribble.ScribbleSpec(s, mask, D, constraint=True, initial=I0)
    fwd = timed(lambda: scribble.scribble_loss(x, spec), steps, warmup)

    def fb():
        x.grad = None
        L, Cn = scribble.scribble_loss(x, spec)
        (L.sum() + Cn).backward()
    both = timed(fb, steps, warmup)
    img, small = B * C * H * W * 4, C * H * W * 4 + H * W
    fwd_bytes, bwd_bytes = 2 * img + small, 2 * img + small + img          # x and I0 read (D, labels: one image); the backward writes dx too
    print(json.dumps({'part': 'terms', 'shape': [B, C, H, W], 'tv_regions': REGIONS, 'i0_batch': B, 'fwd_ms': round(fwd * 1e3, 3),
                      'bwd_ms': round((both - fwd) * 1e3, 3), 'fwd_GB': fwd_bytes / 1e9, 'bwd_GB': bwd_bytes / 1e9,
                      'fwd_GBps': fwd_bytes / fwd / 1e9, 'bwd_GBps': bwd_bytes / max(both - fwd, 1e-9) / 1e9}), flush=True)
    return both


def bench_torch(steps, warmup, fused=None):
    """the reference's formulation, restated (it is not imported: this tool runs where the reference is absent)"""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, C, H, W, generator=g).cuda().requires_grad_(True)
    I0 = torch.rand(B, C, H, W, generator=g).cuda()
    D = torch.rand(1, C, H, W, generator=g).cuda()
    mask, s = edit()
    lm = torch.from_numpy(mask).cuda()
    st = torch.from_numpy(s).float().cuda()
    L1_mask = lm * ((st > 0) * (st < 4)).float()
    tv_masks = [lm * (st == k).float().unsqueeze(0).unsqueeze(0) for k in torch.unique(st * lm) if k > 3]
    cm = 1 - lm

    def sub(im, y, xx):                                   # Return_Translated_SubImage
        return im[:, :, (y if y > 0 else None):(y if y < 0 else None), (xx if xx > 0 else None):(xx if xx < 0 else None)]

    def loss():
        out = torch.clamp(x, 0, 1)
        per = []
        for b in range(B):
            im = out[b:b + 1]
            v = F.l1_loss(im * L1_mask, D * L1_mask)
            for m in tv_masks:
                for y, xx in ((-1, -1), (-1, 0), (0, -1), (1, -1)):
                    v = v + (sub(m, y, xx) * sub(m, -y, -xx) * (sub(im, y, xx) - sub(im, -y, -xx)).abs()).mean(dim=(1, 2, 3))
            per.append(v)
        return torch.stack(per).mean() + F.l1_loss(out * cm, I0 * cm)

    fwd = timed(loss, steps, warmup)

    def fb():
        x.grad = None
        loss().backward()
    both = timed(fb, steps, warmup)
    rec = {'part': 'torch', 'shape': [B, C, H, W], 'tv_regions': REGIONS, 'fwd_ms': round(fwd * 1e3, 3), 'fwd_bwd_ms': round(both * 1e3, 3)}
    if fused:
        rec['speedup_fwd_bwd'] = round(both / fused, 1)
    print(json.dumps(rec), flush=True)


def bench_z(steps, warmup):
    import bench_paths
    import models
    from Z_optimization import Z_optimizer
    with contextlib.redirect_stdout(io.StringIO()):
        model = models.create_model(bench_paths.make_opt(False))
    model.netG.generated_image_model.set_precision('split')
    lr = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(3000)).cuda()
    mask, s = edit()
    desired = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(3001)).cuda()
    data = {'LR': lr, 'STD_increment': 0.01, 'desired': desired, 'scribble_mask': s, 'brightness_factor': 0.2}
    res = {}
    for objective in ('STD_increase', 'scribble', 'STD_increase', 'scribble'):     # interleaved: clock drift hits both
        model.feed_data({'LR': lr.expand(B, -1, -1, -1), 'Z': torch.zeros(B, 3, H, W, device='cuda')}, need_GT=False)
        model.test()
        with contextlib.redirect_stdout(io.StringIO()):
            zo = Z_optimizer(objective=objective, Z_size=[H, W], model=model, Z_range=1, max_iters=max(warmup, 1), data=data, initial_LR=0.1,
                             batch_size=B, image_mask=mask, Z_mask=np.ones((H, W), np.float32), initial_Z=torch.zeros(B, 3, H, W, device='cuda'),
                             non_local_Z_optimization=True)
            zo.optimize()
            zo.max_iters = steps
            torch.cuda.synchronize()
            t = time.perf_counter()
            zo.optimize()
            torch.cuda.synchronize()
        res.setdefault(objective, []).append((time.perf_counter() - t) / steps)
        del zo
    base, scr = min(res['STD_increase']), min(res['scribble'])
    print(json.dumps({'part': 'z', 'shape': [B, C, H, W], 'iter_ms': {'STD_increase': round(base * 1e3, 2), 'scribble': round(scr * 1e3, 2)},
                      'all_ms': {k: [round(v * 1e3, 2) for v in vs] for k, vs in res.items()}, 'overhead_pct': round((scr / base - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--part', default='all', choices=['all', 'terms', 'torch', 'z'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_scribble.py measures on an MI355X'
    fused = None
    if a.part in ('all', 'terms'):
        fused = bench_terms(a.steps, a.warmup)
    if a.part in ('all', 'torch'):
        bench_torch(max(1, a.steps // 2), 1, fused)
        torch.cuda.empty_cache()
    if a.part in ('all', 'z'):
        bench_z(max(1, a.steps // 2), 1)


if __name__ == '__main__':
    main()
