#!/usr/bin/env python
"""What the JPEG decoder's editing tools cost on the device (esr_hip/jpeg_edit.py, csrc/esr_jpeg_edit.hip): prints JSON lines, each with the
route the parent commit would take for the same result beside it, from the same run.

    python tools/bench_jpeg_edit.py [--steps 100] [--warmup 10] [--part all|rgb|score|pair|search] [--nb 17]

  rgb     ycbcr_to_rgb forward + backward on [2, 3, 256, 384] against the torch expression Output_Batch(within_0_1=True) ran
          (Tensor_YCbCR2RGB(x / 255): a [B, 3, 3, H, W] broadcast and its sum)
  score   consistency_violation for 1296 candidates of 64 x 64 against compress-then-reduce with the existing ops (the [N, 64, 8, 8]
          coefficients written, then |.| - 0.5, clamp and sum as torch ops)
  pair    Enforce_pair_Consistency on a 256 x 384 image (host conversions included) against the same method with the two corrections and
          the colour conversion composed of the existing ops (compress, clamp, extract as separate launches; the torch broadcast)
  search  one Z iteration (max_iters = 1 of a constructed Z_optimizer) of 'scribble' and of 'local_STD_increase' on the colour model at
          256 x 384 (DnCNN generators of --nb layers, formula weights), against the same iteration with the parent's colour conversion
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

H, W = 256, 384


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def report(part, what, ours, parent, **more):
    print(json.dumps(dict({'part': part, 'what': what, 'ms': round(ours, 4), 'parent_route_ms': round(parent, 4), 'ratio': round(parent / ours, 2)}, **more)),
          flush=True)


def bench_rgb(steps, warmup):
    from esr_hip import jpeg_edit
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    x = (255 * torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1))).cuda()
    g = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()

    def both(fn):
        def run():
            xr = x.clone().requires_grad_(True)
            (fn(xr) * g).sum().backward()
        return run
    report('rgb', 'ycbcr_to_rgb forward + backward [2, 3, %d, %d]' % (H, W), timed(both(jpeg_edit.ycbcr_to_rgb), steps, warmup),
           timed(both(lambda t: Tensor_YCbCR2RGB(t / 255)), steps, warmup))
    with torch.no_grad():
        ours, parent = timed(lambda: jpeg_edit.ycbcr_to_rgb(x), steps, warmup), timed(lambda: Tensor_YCbCR2RGB(x / 255), steps, warmup)
    report('rgb', 'forward alone', ours, parent, algorithmic_MB=2 * x.numel() * 4 / 1e6, GBps=round(2 * x.numel() * 4 / ours / 1e6, 1))


def bench_score(steps, warmup):
    from esr_hip import jpeg as J, jpeg_edit
    from JPEG_module.JPEG import JPEG
    N = 1296
    gen = torch.Generator().manual_seed(3)
    fixed = torch.round(255 * torch.rand(1, 1, 64, 64, generator=gen))
    cand = (fixed + 20 * (torch.rand(N, 1, 64, 64, generator=gen) - 0.5)).cuda()
    m = JPEG(compress=True, downsample_or_quantize=True)
    m.Set_Q_Table(torch.tensor([40.]))
    q = m.Q_table.reshape(1, 64).cuda()
    coef = J.compress(fixed.cuda(), q, True)
    with torch.no_grad():
        ours = timed(lambda: jpeg_edit.consistency_violation(cand, coef, q), steps, warmup)
        parent = timed(lambda: torch.clamp((J.compress(cand, q, False) - coef).abs() - 0.5, min=0).sum(dim=(1, 2, 3)), steps, warmup)
    report('score', 'consistency_violation, %d candidates of 64 x 64' % N, ours, parent, algorithmic_MB=cand.numel() * 4 / 1e6,
           GBps=round(cand.numel() * 4 / ours / 1e6, 1))


def colour_model(nb):
    from models import create_model
    from options import options as option
    from oracle.weights import fill_formula_weights
    tmp = tempfile.mkdtemp()
    cfg = {'name': 'jpeg_run', 'model': 'dncnn', 'gpu_ids': [0], 'scale': 4,
           'datasets': {'test_1': {'name': 'set', 'mode': 'JPEG', 'dataroot_Uncomp': 'images/uncomp'}},
           'path': {'root': tmp, 'datasets': os.path.join(tmp, 'data'), 'pretrained_model_G': None, 'Y_channel_model_G': None},
           'network_G': {'which_model_G': 'DnCNN', 'norm_type': 'batch', 'CEM_arch': 0, 'padding': 1, 'latent_input': 'all_layers',
                         'latent_channels': {'ModelY': 64, 'ModelChroma': 64}, 'nf': {'ModelY': 64, 'ModelChroma': 64}, 'nb': nb},
           'network_G_Y': {'nf': 64, 'nb': nb}}
    path = os.path.join(tmp, 'bench_JPEG.json')
    with open(path, 'w') as f:
        json.dump(cfg, f)
    model = create_model(option.dict_to_nonedict(option.parse(path, is_train=False, JPEG=True, chroma=True)), chroma_mode=True)
    for net in (model.netG, model.netG_Y):
        fill_formula_weights(net, gain=0.7)
    return model


def parent_routes():
    """the new operations composed of what the parent commit has: esr_hip.jpeg's kernels one launch each, torch ops between them"""
    from esr_hip import jpeg_edit
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    return {'ycbcr_to_rgb': lambda x: Tensor_YCbCR2RGB(x / 255), 'consistent_plane': jpeg_edit._plane_cpu,
            'consistent_chroma': lambda d, k, q: jpeg_edit._chroma_cpu(d, k, q.reshape(-1, 3, 256))}


def bench_pair(model, steps, warmup):
    from esr_hip import jpeg_edit
    from JPEG_module.JPEG import JPEG
    model.JPEG['compressor_Y_non_quantized'] = JPEG(compress=True, chroma_mode=False, downsample_or_quantize=False, block_size=8)
    model.JPEG['compressor_non_quantized'] = JPEG(compress=True, chroma_mode=True, downsample_or_quantize=False, block_size=16)
    for m in model.JPEG.values():
        m.Set_Q_Table(torch.tensor([40.]).cuda())
    rng = np.random.RandomState(4)
    a, b = rng.rand(H, W, 3).astype(np.float32), rng.rand(H, W, 3).astype(np.float32)
    ours = timed(lambda: model.Enforce_pair_Consistency(a, b), steps, warmup)
    kept = {k: getattr(jpeg_edit, k) for k in parent_routes()}
    try:
        for k, f in parent_routes().items():
            setattr(jpeg_edit, k, f)
        parent = timed(lambda: model.Enforce_pair_Consistency(a, b), steps, warmup)
    finally:
        for k, f in kept.items():
            setattr(jpeg_edit, k, f)
    report('pair', 'Enforce_pair_Consistency %d x %d (host conversions and copies included)' % (H, W), ours, parent)
    with torch.no_grad():
        d = (255 * torch.rand(1, 3, H, W)).cuda()
        ky, kc = model.JPEG['compressor_Y'](d[:, :1]), model.JPEG['compressor'](d)
        qy, qc = model.JPEG['compressor_Y']._table_on(d.device), model.JPEG['compressor']._table_on(d.device)
        d2 = d + 10
        p = parent_routes()
        report('pair', 'consistent_plane alone', timed(lambda: jpeg_edit.consistent_plane(d2[:, :1], ky, qy), steps, warmup),
               timed(lambda: p['consistent_plane'](d2[:, :1], ky, qy.reshape(1, 64)), steps, warmup))
        report('pair', 'consistent_chroma alone', timed(lambda: jpeg_edit.consistent_chroma(d2, kc, qc), steps, warmup),
               timed(lambda: p['consistent_chroma'](d2, kc, qc), steps, warmup))


def bench_search(model, steps, warmup):
    from esr_hip import jpeg_edit
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    from Z_optimization import Z_optimizer
    x = (255 * torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5))).round().cuda()
    qf = torch.tensor([40.]).cuda()
    mask = np.zeros((H, W), np.float32)
    mask[64:192, 96:288] = 1
    s = np.zeros((H, W), np.int64)
    s[80:120, 112:200] = 1
    s[136:176, 120:180] = 5
    for objective in ('scribble', 'local_STD_increase'):
        data = {'Uncomp': x, 'QF': qf}
        if objective == 'scribble':
            data.update(desired=torch.rand(1, 3, H, W).cuda(), scribble_mask=jpeg_edit.smear_mask_to_blocks(s))
        Z0 = torch.zeros(1, 64, H // 8, W // 8).cuda()
        model.feed_data(dict(data, Z=Z0), need_GT=False)
        model.test()
        zo = Z_optimizer(objective, [H // 8, W // 8], model, Z_range=1.0, max_iters=1, data=data, initial_Z=Z0, initial_LR=0.01, batch_size=1,
                         image_mask=mask, Z_mask=mask.reshape(H // 8, 8, W // 8, 8).max((1, 3)), non_local_Z_optimization=objective == 'scribble',
                         jpeg_extractor=model.JPEG['extractor'])
        ours = timed(zo.optimize, steps, warmup)
        real = model.Output_Image_0_1
        try:
            model.Output_Image_0_1 = lambda: Tensor_YCbCR2RGB(model.output_image / 255)
            parent = timed(zo.optimize, steps, warmup)
        finally:
            model.Output_Image_0_1 = real
        report('search', "one Z iteration of '%s' on the colour model, %d x %d" % (objective, H, W), ours, parent)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--nb', type=int, default=17)
    ap.add_argument('--part', default='all', choices=['all', 'rgb', 'score', 'pair', 'search'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_jpeg_edit.py measures on an MI355X'
    if a.part in ('all', 'rgb'):
        bench_rgb(a.steps, a.warmup)
    if a.part in ('all', 'score'):
        bench_score(a.steps, a.warmup)
    if a.part in ('all', 'pair', 'search'):
        model = colour_model(a.nb)
        if a.part in ('all', 'pair'):
            bench_pair(model, a.steps, a.warmup)
        if a.part in ('all', 'search'):
            bench_search(model, max(1, a.steps // 4), max(1, a.warmup // 2))


if __name__ == '__main__':
    main()
