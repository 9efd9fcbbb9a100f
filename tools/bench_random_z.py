#!/usr/bin/env python
"""What the random-alternatives Z objectives cost (esr_hip/pairmin.py, csrc/esr_pairmin.hip): prints JSON lines.

    python tools/bench_random_z.py [--steps 5] [--warmup 2] [--part all|terms|torch|z]

  terms   forward and forward + backward of the fused term at configs[3]'s shape, 64 x 3 x 512^2, plain ('random_l1') and with the image mask and
          the limited term (init of batch 64), against its algorithmic bytes (every input read once, every output written once)
  torch   the reference's formulation restated in torch (codes/Z_optimization.py:688-699: a [B, B, C, H, W] difference, abs, + eye, min) on the same
          GPU, forward + backward, at the largest batch of 64, 32, 16, 8 whose intermediates fit in memory (12.9 GB each at 64)
  z       one Z_optimizer.optimize() iteration at bench.py --workload c4's shape (RRDB-23 x4 lat 3 + CEM, 64 Z samples of 512^2) with
          'random_l1' against the same iteration with 'STD_increase', in one process, interleaved
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, C, H, W = 64, 3, 512, 512


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def bench_terms(steps, warmup):
    from esr_hip import pairmin
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, C, H, W, generator=g) * 1.2 - 0.1).cuda().requires_grad_(True)
    init = torch.rand(B, C, H, W, generator=g).cuda()
    mask = torch.zeros(H, W)
    mask[96:416, 96:416] = 1
    mask = mask.cuda()
    img = B * C * H * W * 4
    plain = None
    for name, kw, extra in (('random_l1', {}, 0), ('random_l1_limited+mask', dict(mask=mask, init=init, w=0.3), img + H * W * 4)):
        fwd = timed(lambda: pairmin.random_share(x, **kw), steps, warmup)

        def fb():
            x.grad = None
            pairmin.random_share(x, **kw)[1].backward()
        both = timed(fb, steps, warmup)
        fwd_bytes, bwd_bytes = img + extra, 2 * img + extra              # x (and init, mask) read; the backward writes dx too
        print(json.dumps({'part': 'terms', 'objective': name, 'shape': [B, C, H, W], 'fwd_ms': round(fwd * 1e3, 3), 'bwd_ms': round((both - fwd) * 1e3, 3),
                          'pair_steps_G': B * B * C * H * W / 1e9, 'fwd_GB': fwd_bytes / 1e9, 'bwd_GB': bwd_bytes / 1e9, 'fwd_GBps': fwd_bytes / fwd / 1e9,
                          'bwd_GBps': bwd_bytes / max(both - fwd, 1e-9) / 1e9}), flush=True)
        plain = plain or both
    return plain


def bench_torch(steps, warmup, fused=None):
    """the reference's formulation, restated (it is not imported: this tool runs where the reference is absent)"""
    g = torch.Generator().manual_seed(5)
    full = (torch.rand(B, C, H, W, generator=g) * 1.2 - 0.1).cuda()
    for b in (64, 32, 16, 8):
        x = full[:b].clone().requires_grad_(True)
        eye = torch.eye(b, device='cuda').view(b, b, 1, 1, 1)

        def loss():
            D = torch.clamp(x, 0, 1)
            return (-1 * torch.min((D.unsqueeze(0) - D.unsqueeze(1)).abs() + eye, dim=0)[0].mean(dim=(1, 2, 3))).mean()

        def fb():
            x.grad = None
            loss().backward()
        try:
            fwd = timed(loss, steps, warmup)
            both = timed(fb, steps, warmup)
        except torch.OutOfMemoryError:
            print(json.dumps({'part': 'torch', 'batch': b, 'fits': False, 'one_intermediate_GB': b * b * C * H * W * 4 / 1e9}), flush=True)
            x = None
            torch.cuda.empty_cache()
            continue
        rec = {'part': 'torch', 'batch': b, 'fits': True, 'shape': [b, C, H, W], 'fwd_ms': round(fwd * 1e3, 3), 'fwd_bwd_ms': round(both * 1e3, 3),
               'peak_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
        if b != B:
            from esr_hip import pairmin

            def fused_fb():
                x.grad = None
                pairmin.random_share(x)[1].backward()
            rec['fused_fwd_bwd_ms_same_batch'] = round(timed(fused_fb, steps, warmup) * 1e3, 3)
        elif fused:
            rec['fused_fwd_bwd_ms_same_batch'] = round(fused * 1e3, 3)
        rec['speedup_fwd_bwd'] = round(both * 1e3 / rec['fused_fwd_bwd_ms_same_batch'], 1) if 'fused_fwd_bwd_ms_same_batch' in rec else None
        print(json.dumps(rec), flush=True)
        return


def bench_z(steps, warmup):
    import bench_paths
    import models
    from Z_optimization import Z_optimizer
    with contextlib.redirect_stdout(io.StringIO()):
        model = models.create_model(bench_paths.make_opt(False))
    model.netG.generated_image_model.set_precision('split')
    lr = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(3000)).cuda()
    z0 = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3002)) * 0.2 - 0.1).cuda()
    data = {'LR': lr, 'STD_increment': 0.01}
    res = {}
    for objective in ('STD_increase', 'random_l1', 'STD_increase', 'random_l1'):     # interleaved: clock drift hits both
        model.feed_data({'LR': lr.expand(B, -1, -1, -1), 'Z': torch.zeros(B, 3, H, W, device='cuda')}, need_GT=False)
        model.test()
        with contextlib.redirect_stdout(io.StringIO()):
            zo = Z_optimizer(objective=objective, Z_size=[H, W], model=model, Z_range=1, max_iters=max(warmup, 1), data=data, initial_LR=0.1,
                             batch_size=B, initial_Z=z0.clone())
            zo.optimize()
            zo.max_iters = steps
            torch.cuda.synchronize()
            t = time.perf_counter()
            zo.optimize()
            torch.cuda.synchronize()
        res.setdefault(objective, []).append((time.perf_counter() - t) / steps)
        del zo
    base, rnd = min(res['STD_increase']), min(res['random_l1'])
    print(json.dumps({'part': 'z', 'shape': [B, C, H, W], 'iter_ms': {'STD_increase': round(base * 1e3, 2), 'random_l1': round(rnd * 1e3, 2)},
                      'all_ms': {k: [round(v * 1e3, 2) for v in vs] for k, vs in res.items()}, 'overhead_pct': round((rnd / base - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--part', default='all', choices=['all', 'terms', 'torch', 'z'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_random_z.py measures on an MI355X'
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
