#!/usr/bin/env python
"""What the VGG feature loss costs (esr_hip/vgg.py; reference codes/models/SRRaGAN_model.py:442-451): prints JSON lines.

    python tools/bench_feature_loss.py [--steps 5] [--warmup 2] [--rounds 3] [--part all|step|extractor]

  step       the configs[2]-shaped G + D step (tools/bench_paths.make_opt(with_D=True): RRDB-23 x4 + CEM, lat 3, 32 crops of 52x52, bf16 critic
             and generator) with train.feature_weight null and with 1 (l1, VGG19-54 on the 208x208 output): two models in this process, timed
             in alternating rounds after their warm-up
  extractor  VGG19-54 alone at 32 x 3 x 208 x 208, forward + input gradient, 'bf16' and 'split'; achieved TFLOP/s from the layer shapes
             (2 FLOP per multiply-add, the data gradient counted as the forward's), and the share of the 2.5 PFLOP/s dense bf16 MFMA peak;
             the 2x2 max pool and its backward on the largest map against HBM's 8 TB/s
The weights are seeded (the timings do not depend on them).  Run the kernel profile in a process of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o vgg -- python tools/bench_feature_loss.py --part extractor --steps 3 --rounds 1
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF16_PEAK = 2.5e15          # dense bf16 MFMA, FLOP/s (MI355X spec)
HBM_PEAK = 8.0e12           # bytes/s (spec)


def seeded_vgg19_file(dirname):
    from esr_hip.vgg import layer_table
    g = torch.Generator().manual_seed(0)
    sd = {}
    for i, e in enumerate(layer_table('vgg19', 34)):
        if e[0] == 'conv':
            sd['features.%d.weight' % i] = torch.randn(e[2], e[1], 3, 3, generator=g) * (2.0 / (e[2] * 9)) ** 0.5
            sd['features.%d.bias' % i] = torch.zeros(e[2])
    p = os.path.join(dirname, 'vgg19_seeded.pth')
    torch.save(sd, p)
    return p


def conv_flops(B, H, W, arch='vgg19', feature_layer=34):
    """2 * multiply-adds of the forward's convs at B x 3 x H x W."""
    from esr_hip.vgg import layer_table
    total, h, w = 0, H, W
    for e in layer_table(arch, feature_layer):
        if e[0] == 'conv':
            total += 2 * B * h * w * e[1] * e[2] * 9
        elif e[0] == 'pool':
            h, w = h // 2, w // 2
    return total


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def part_step(a, wfile):
    import bench_paths
    import models
    res = {}
    ms = {'fea_null': [], 'fea_1': []}
    runs = {}
    for name, fw in (('fea_null', None), ('fea_1', 1)):
        torch.manual_seed(0)
        opt = bench_paths.make_opt(True, with_D=True)
        opt['network_D']['precision'] = 'bf16'
        opt['path']['pretrained_model_F'] = wfile
        opt['train']['feature_weight'] = fw
        opt['train']['feature_criterion'] = 'l1'
        with contextlib.redirect_stdout(io.StringIO()):
            model = models.create_model(opt)
        model.netG.generated_image_model.set_precision('bf16')
        model.D_dtype = torch.bfloat16
        g = torch.Generator().manual_seed(2000)
        dev = torch.device('cuda', 0)
        data = {'LR': torch.rand(32, 3, 52, 52, generator=g).to(dev), 'HR': torch.rand(32, 3, 208, 208, generator=g).to(dev),
                'Z': (torch.rand(32, 3, 208, 208, generator=g) * 2 - 1).to(dev)}

        def step(model=model, data=data):
            model.feed_data(data)
            model.optimize_parameters()
        for _ in range(a.warmup):
            step()
        runs[name] = (model, step)
    for _ in range(a.rounds):
        for name, (model, step) in runs.items():
            ms[name].append(timed(step, a.steps))
    for name in ms:
        res[name + '_ms'] = sorted(ms[name])
    med = lambda v: sorted(v)[len(v) // 2]
    res['feature_loss_ms'] = med(ms['fea_1']) - med(ms['fea_null'])
    res['l_g_fea'] = runs['fea_1'][0].get_current_log().get('l_g_fea')
    return res


def part_extractor(a, wfile):
    import models.modules.architecture as arch
    from esr_hip import _lib
    from esr_hip.act import new_at, view_of
    dev = torch.device('cuda', 0)
    sd = torch.load(wfile)
    net = arch.VGGFeatureExtractor(state_dict=sd).to(dev).eval()
    B, H, W = 32, 208, 208
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    flops_fwd = conv_flops(B, H, W)
    out = {'shape': [B, 3, H, W], 'flop_forward': flops_fwd, 'flop_forward_and_input_grad': 2 * flops_fwd}
    for precision in ('bf16', 'split'):
        net.set_precision(precision)
        cot = torch.rand(B, 512, H // 16, W // 16, device=dev)

        def fwd():
            with torch.no_grad():
                net(x)

        def fwd_bwd():
            xg = x.detach().requires_grad_(True)
            (net(xg) * cot).sum().backward()
        for _ in range(a.warmup):
            fwd_bwd()
        t_f = min(timed(fwd, a.steps) for _ in range(a.rounds))
        t_fb = min(timed(fwd_bwd, a.steps) for _ in range(a.rounds))
        # (split runs 3 MFMAs per product: its 'issued' share counts them)
        mult = 3 if precision == 'split' else 1
        out[precision] = {'forward_ms': t_f, 'forward_input_grad_ms': t_fb,
                          'forward_tflops': flops_fwd / t_f * 1e-9, 'forward_input_grad_tflops': 2 * flops_fwd / t_fb * 1e-9,
                          'share_of_bf16_peak_forward': mult * flops_fwd / (t_f * 1e-3) / BF16_PEAK,
                          'share_of_bf16_peak_forward_input_grad': mult * 2 * flops_fwd / (t_fb * 1e-3) / BF16_PEAK}
        # the max pool and its backward on the largest map (conv1_2's output: 64 channels at 208 x 208)
        P = 2 if precision == 'split' else 1
        xt = new_at(P, B, 8, H, W, dev).normal_()
        y = new_at(P, B, 8, H // 2, W // 2, dev)
        dx = new_at(P, B, 8, H, W, dev)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pool = lambda: _lib.check(_lib.lib.esr_maxpool2x2(C.byref(view_of(xt)), C.byref(view_of(y)), B, s), 'esr_maxpool2x2')
        pool_bwd = lambda: _lib.check(_lib.lib.esr_maxpool2x2_grad(C.byref(view_of(xt)), C.byref(view_of(y)), 1, C.byref(view_of(dx)), B, s),
                                      'esr_maxpool2x2_grad')
        pool()
        pool_bwd()
        t_p = min(timed(pool, 20) for _ in range(a.rounds))
        t_pb = min(timed(pool_bwd, 20) for _ in range(a.rounds))
        nb = lambda t: t.numel() * t.element_size()
        bytes_p, bytes_pb = nb(xt) + nb(y), nb(xt) + nb(y) + nb(dx)        # algorithmic: every input read once, every output written once
        out[precision]['pool'] = {'us': t_p * 1e3, 'bytes': bytes_p, 'TBps': bytes_p / t_p * 1e-9, 'share_of_hbm': bytes_p / (t_p * 1e-3) / HBM_PEAK}
        out[precision]['pool_backward'] = {'us': t_pb * 1e3, 'bytes': bytes_pb, 'TBps': bytes_pb / t_pb * 1e-9,
                                           'share_of_hbm': bytes_pb / (t_pb * 1e-3) / HBM_PEAK}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--part', default='all', choices=['all', 'step', 'extractor'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    with tempfile.TemporaryDirectory(prefix='esr_fea_') as d:
        wfile = seeded_vgg19_file(d)
        res = {'tool': 'bench_feature_loss', 'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds}
        if a.part in ('all', 'extractor'):
            res['extractor'] = part_extractor(a, wfile)
            print(json.dumps(res['extractor']), flush=True)
        if a.part in ('all', 'step'):
            res['step'] = part_step(a, wfile)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
