#!/usr/bin/env python
"""What the local-STD and periodicity Z objectives cost (esr_hip/local.py, csrc/esr_local.hip): prints JSON lines.

    python tools/bench_local_z.py [--steps 5] [--warmup 2] [--part all|terms|sparse|z]

  terms   forward and forward + backward of the local-STD term (patch_std, full mask) and of the periodicity term (shift_l1, two non-integer
          points) at configs[3]'s shape, 64 x 3 x 512^2, with their algorithmic bytes (every input read once, every output written once)
  sparse  the reference's formulation restated in torch (a (49 P) x (H W) sparse extraction matrix, torch.sparse.mm per image, std over the
          49 rows; codes/Z_optimization.py:616-627) on the same GPU, forward + backward, at a batch that fits; per-image time
  z       one Z_optimizer.optimize() iteration at bench.py --workload c4's shape (RRDB-23 x4 lat 3 + CEM, 64 Z samples of 512^2) with
          'local_STD_increase' against the same iteration with 'STD_increase', in one process
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
    from esr_hip import local
    x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    ps = local.PatchSet(None, H, W)
    P = ps.P
    img, grid = B * C * H * W * 4, B * P * 4
    fwd = timed(lambda: local.patch_std(x, ps), steps, warmup)

    def fb_std():
        x.grad = None
        local.patch_std(x, ps).sum().backward()
    both = timed(fb_std, steps, warmup)
    # forward: x, S and mean written; backward: x, S, mean, dS read, dx written
    fwd_bytes, bwd_bytes = img + 2 * grid, img + 3 * grid + img
    print(json.dumps({'part': 'terms', 'term': 'local_STD', 'shape': [B, C, H, W], 'patches_per_image': P, 'fwd_ms': round(fwd * 1e3, 3),
                      'bwd_ms': round((both - fwd) * 1e3, 3), 'fwd_GB': fwd_bytes / 1e9, 'bwd_GB': bwd_bytes / 1e9,
                      'fwd_GBps': fwd_bytes / fwd / 1e9, 'bwd_GBps': bwd_bytes / max(both - fwd, 1e-9) / 1e9}), flush=True)
    mask = torch.ones(H, W, device='cuda')
    pairs = [local.ShiftPair(p, H, W, interpolated=True) for p in ((2.5, 3.25), (-1.75, 4.5))]
    fwd = timed(lambda: local.shift_l1(x, mask, pairs), steps, warmup)

    def fb_shift():
        x.grad = None
        local.shift_l1(x, mask, pairs).sum().backward()
    both = timed(fb_shift, steps, warmup)
    n = len(pairs)
    out = sum(B * C * p.ny * p.nx * 4 for p in pairs)
    fwd_bytes, bwd_bytes = n * (img + H * W * 4), n * (img + H * W * 4) + 2 * out + img      # per point: x read; G written and read; dx written
    print(json.dumps({'part': 'terms', 'term': 'periodicity (2 non-integer points)', 'shape': [B, C, H, W], 'fwd_ms': round(fwd * 1e3, 3),
                      'bwd_ms': round((both - fwd) * 1e3, 3), 'fwd_GB': fwd_bytes / 1e9, 'bwd_GB': bwd_bytes / 1e9,
                      'fwd_GBps': fwd_bytes / fwd / 1e9, 'bwd_GBps': bwd_bytes / max(both - fwd, 1e-9) / 1e9}), flush=True)


def bench_sparse(steps, warmup, batch=8):
    """the reference's sparse-matrix Masked_STD, restated (it is not imported: this tool runs where the reference is absent)"""
    from esr_hip import local
    ps = local.PatchSet(None, H, W)
    idx = torch.from_numpy(local.corner_patch_indexes(ps.corners, W))                       # [P, 49]
    P = idx.size(0)
    rows = torch.arange(idx.numel())
    mat = torch.sparse_coo_tensor(torch.stack([rows, idx.t().reshape(-1)]), torch.ones(idx.numel()), (idx.numel(), H * W)).cuda()
    x = torch.rand(batch, C, H, W, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)

    def std():
        out = torch.clamp(x, 0, 1)
        return torch.stack([torch.sparse.mm(mat, out[b].mean(0).view(-1, 1)).view(49, -1).std(0) for b in range(batch)], 1)
    fwd = timed(std, steps, warmup)

    def fb():
        x.grad = None
        std().sum().backward()
    both = timed(fb, steps, warmup)
    print(json.dumps({'part': 'sparse', 'batch': batch, 'patches_per_image': P, 'matrix_entries': int(idx.numel()), 'fwd_ms': round(fwd * 1e3, 3),
                      'bwd_ms': round((both - fwd) * 1e3, 3), 'fwd_ms_per_image': round(fwd * 1e3 / batch, 3),
                      'fwd_bwd_ms_at_64': round(both * 1e3 / batch * B, 3)}), flush=True)


def bench_z(steps, warmup):
    import bench_paths
    import models
    from Z_optimization import Z_optimizer
    with contextlib.redirect_stdout(io.StringIO()):
        model = models.create_model(bench_paths.make_opt(False))
    model.netG.generated_image_model.set_precision('split')
    lr = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(3000)).cuda()
    res = {}
    for objective in ('STD_increase', 'local_STD_increase', 'STD_increase', 'local_STD_increase'):     # interleaved: clock drift hits both
        model.feed_data({'LR': lr.expand(B, -1, -1, -1), 'Z': torch.zeros(B, 3, H, W, device='cuda')}, need_GT=False)
        model.test()
        with contextlib.redirect_stdout(io.StringIO()):
            kw = dict(image_mask=None, Z_mask=None)
            zo = Z_optimizer(objective=objective, Z_size=[H, W], model=model, Z_range=1, max_iters=max(warmup, 1), data={'LR': lr, 'STD_increment': 0.01},
                             initial_LR=0.1, batch_size=B, **kw)
            zo.optimize()
            zo.max_iters = steps
            torch.cuda.synchronize()
            t = time.perf_counter()
            zo.optimize()
            torch.cuda.synchronize()
        res.setdefault(objective, []).append((time.perf_counter() - t) / steps)
        del zo
    base, loc = min(res['STD_increase']), min(res['local_STD_increase'])
    print(json.dumps({'part': 'z', 'shape': [B, C, H, W], 'iter_ms': {'STD_increase': round(base * 1e3, 2), 'local_STD_increase': round(loc * 1e3, 2)},
                      'all_ms': {k: [round(v * 1e3, 2) for v in vs] for k, vs in res.items()}, 'overhead_pct': round((loc / base - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--part', default='all', choices=['all', 'terms', 'sparse', 'z'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_local_z.py measures on an MI355X'
    if a.part in ('all', 'terms'):
        bench_terms(a.steps, a.warmup)
    if a.part in ('all', 'sparse'):
        bench_sparse(a.steps, a.warmup)
        torch.cuda.empty_cache()
    if a.part in ('all', 'z'):
        bench_z(max(1, a.steps // 2), 1)


if __name__ == '__main__':
    main()
