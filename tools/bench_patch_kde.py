#!/usr/bin/env python
"""What the patch-histogram / dictionary Z objectives cost (esr_hip/kde.py, csrc/esr_kde.hip): prints JSON lines.

    python tools/bench_patch_kde.py [--steps 5] [--warmup 2] [--part all|loss|z]

  loss  SoftHistogramLoss forward and forward + backward of 'patchdict_noDC' and 'patchhist' on square regions of 128^2, 256^2 and 512^2,
        batch 1 and 8, the desired image the same size: N patches (overlap 0.5) against M de-duplicated bins (overlap 30/36); pair-dims per
        second = N * M * 36 / time per pass
  z     one Z iteration (generator forward + backward + Adam) at configs[3]'s per-sample shape (tools/bench_paths.make_opt) with
        'patchdict_noDC' against the same iteration with 'max_STD'
Run the kernel counters in a process of their own:
    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d <dir> -o kde -- python tools/bench_patch_kde.py --part loss --regions 512 --steps 1 --warmup 0
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def bench_loss(steps, warmup, regions=(128, 256, 512)):
    from Z_optimization import SoftHistogramLoss, hist_objective_config
    from oracle.weights import seeded_uniform
    for side in regions:
        coarse = seeded_uniform((1, 3, side // 16, side // 16), 7).cuda()
        desired = torch.nn.functional.interpolate(coarse, size=(side, side), mode='bilinear', align_corners=True)
        for objective in ('patchdict_noDC', 'patchhist'):
            t0 = time.perf_counter()
            loss_fn = SoftHistogramLoss(desired_hist_image=[desired], desired_hist_image_mask=None, gray_scale=True, **hist_objective_config(objective))
            torch.cuda.synchronize()
            setup = time.perf_counter() - t0
            for B in (1, 8):
                cur = (desired + 0.05 * (seeded_uniform((B, 3, side, side), 8).cuda() - 0.5)).clamp(0, 1).requires_grad_(True)
                loss_fn(cur[:1])                                   # patch selection (cached) outside the window
                fwd = timed(lambda: loss_fn(cur), steps, warmup)

                def fb():
                    cur.grad = None
                    loss_fn(cur).sum().backward()
                both = timed(fb, steps, warmup)
                N = [v for k, v in loss_fn._patch_index.items() if k[2] == 0.5][0].size(0)      # the current image's patches (overlap 0.5)
                M = loss_fn.bins.size(0)
                pd = float(N) * M * 36 * B
                print(json.dumps({'part': 'loss', 'objective': objective, 'region': side, 'batch': B, 'N': N, 'M': M, 'setup_s': round(setup, 3),
                                  'fwd_ms': round(fwd * 1e3, 3), 'bwd_ms': round((both - fwd) * 1e3, 3),
                                  'fwd_pairdims_per_s': pd / fwd, 'bwd_pairdims_per_s': pd / max(both - fwd, 1e-9)}), flush=True)


def bench_z(steps, warmup):
    import bench_paths
    import models
    from Z_optimization import Z_optimizer
    from oracle.weights import fill_formula_weights, seeded_uniform
    m = models.create_model(bench_paths.make_opt(False))             # RRDB-23 x4 + CEM, latent 3: configs[3]'s generator
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 128, 128), 30).to(m.device)            # one sample of configs[3] (512 x 512 output)
    sf = 4
    H, W = lr.shape[2] * sf, lr.shape[3] * sf
    z0 = seeded_uniform((1, m.num_latent_channels, H, W), 31, -0.3, 0.3).to(m.device)
    m.feed_data({'LR': lr, 'Z': z0}, need_GT=False)
    m.test()
    desired = m.fake_H.detach().clamp(0, 1) * 0.6 + 0.2
    out = {}
    for objective in ('max_STD', 'patchdict_noDC'):
        zo = Z_optimizer(objective=objective, Z_size=[H, W], model=m, Z_range=1, max_iters=1, initial_Z=z0.clone(), initial_LR=0.01, batch_size=1,
                         data={'LR': lr, 'desired': [desired]})
        out[objective] = timed(zo.optimize, steps, warmup)
    print(json.dumps({'part': 'z', 'shape': [H, W], 'iter_ms': {k: round(v * 1e3, 3) for k, v in out.items()},
                      'added_ms': round((out['patchdict_noDC'] - out['max_STD']) * 1e3, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--part', default='all', choices=['all', 'loss', 'z'])
    ap.add_argument('--regions', type=int, nargs='+', default=[128, 256, 512], help='region sides of the loss part')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_patch_kde.py measures on an MI355X'
    if a.part in ('all', 'loss'):
        bench_loss(a.steps, a.warmup, a.regions)
    if a.part in ('all', 'z'):
        bench_z(a.steps, a.warmup)


if __name__ == '__main__':
    main()
