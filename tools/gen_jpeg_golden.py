#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/jpeg_dncnn.npz by running the REFERENCE's own JPEG module
(codes/JPEG_module/JPEG.py) and DnCNN generator (codes/models/modules/architecture.py:109-214), imported read-only through oracle/_refshim.
Run:
    python tools/gen_jpeg_golden.py

The reference indexes with torch.cuda.LongTensor (JPEG.py:116); this script sets torch.cuda.LongTensor = torch.LongTensor, which is all it
needs to run on the CPU.  Weights are formula weights (oracle.weights.fill_formula_weights, gain 0.7) with the BatchNorm scale and running
statistics from seeded_uniform (fill_batchnorm below), so only inputs and outputs are stored.  The helpers of this file that do not touch
the reference (inputs, BatchNorm fill, the float64 restatement of the transform) are imported by the tests.

(a) module level: B = 6, 48 x 64, QF = [5, 10, 30, 50, 75, 95], images 'noise' (uniform integers 0...255) and 'smooth' (a smooth pattern plus
    noise, rounded to integers):
  a/qf [6], a/tables [6, 64], a/<image>/x (uint8), cq (quantised coefficients, int16), cn (non-quantised), img_q, img_n (the extractor's image
  of either); a/explicit/table [8, 8], qf (the derived self.QF), q_table [64] (what the reference then divides by), cq, img_q on image 0 of 'smooth'
(b) generator level: DnCNN(n_channels=64, depth=5, latent 64, Sigmoid output, BatchNorm), 6 x 9 blocks, B = 2, QF = [10, 40], a smooth pattern
    plus noise compressed by the reference's quantising compressor, Z seeded in [-1, 1]; for latent_input 'all_layers', 'first_layer', 'None':
  b/x (uint8), b/coef, b/Z, b/r, b/tables, b/<mode>/keys (the state_dict key list), out (the generator's coefficients), img (the extractor's
  image), grad (d sum(img * r) / d input, input = [Z | coef] or coef), y (the last conv's output, before the sigmoid)
(c) a reference Z_optimizer('l1', jpeg_extractor=...) run is NOT stored: it was not attempted for this fixture, and the GPU search test compares
    with this build's CPU path instead.

Two conditions are asserted here and again by tests/test_host_jpeg.py: fewer than 1 % of the last conv's outputs have |y| > 6 in each
latent mode (no saturated sigmoid), and at most 1 % of the quantised coefficients of any stored case lie within 1e-3 of a rounding tie in
float64 (those are excluded from exact comparisons)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.weights import fill_formula_weights, seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_dncnn.npz')
QF_A = [5, 10, 30, 50, 75, 95]
QF_B = [10, 40]
MODES = ('all_layers', 'first_layer', 'None')
GAIN = 0.7
TIE_WINDOW, TIE_CAP, SATURATION, SATURATION_CAP = 1e-3, 0.01, 6.0, 0.01


# ------------------------------------------------------------------------------------------------ shared with the tests (no reference)
def smooth_pattern(B, H, W, seed):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    out = []
    for b in range(B):
        base = 128 + 70 * torch.sin(xx / (7 + b)) * torch.cos(yy / (5 + 0.5 * b)) + 20 * torch.sin((xx + 2 * yy) / 23)
        out.append(base + 24 * (seeded_uniform((H, W), seed + b).double() - 0.5))
    return torch.stack(out).unsqueeze(1).round().clamp(0, 255).float()


def images_a():
    return {'noise': torch.floor(seeded_uniform((6, 1, 48, 64), 3100) * 256).clamp(0, 255).float(), 'smooth': smooth_pattern(6, 48, 64, 3200)}


def image_b():
    return smooth_pattern(2, 48, 72, 3300)


def latent_b():
    return seeded_uniform((2, 64, 6, 9), 3400, -1.0, 1.0)


def cotangent_b():
    return seeded_uniform((2, 1, 48, 72), 3500, -1.0, 1.0)


def explicit_table():
    from_k1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                        [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 36, 55, 64, 81, 104, 113, 92],
                        [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64)
    return np.round(from_k1 * 0.6 + 2)


def fill_batchnorm(net, seed=3600):
    """BatchNorm scale in [0.5, 1.5], running mean in [-0.3, 0.3], running variance in [0.5, 1.5], seeded per layer."""
    k = 0
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(seeded_uniform((n,), seed + 3 * k, 0.5, 1.5))
                m.running_mean.copy_(seeded_uniform((n,), seed + 3 * k + 1, -0.3, 0.3))
                m.running_var.copy_(seeded_uniform((n,), seed + 3 * k + 2, 0.5, 1.5))
                k += 1


def fill_generator(net):
    fill_formula_weights(net, gain=GAIN)
    fill_batchnorm(net)
    return net


def dct64():
    k = torch.arange(8, dtype=torch.float64).view(8, 1)
    n = torch.arange(8, dtype=torch.float64).view(1, 8)
    D = 0.5 * torch.cos((2 * n + 1) * k * np.pi / 16)
    D[0] = np.sqrt(0.125)
    return D


def compress64(x, tables):
    """float64 coefficients before any rounding: [B, 64, H/8, W/8]; tables [B, 64]"""
    B, _, H, W = x.shape
    D = dct64()
    c = torch.einsum('ur,birjs,vs->buvij', D, x.double().reshape(B, H // 8, 8, W // 8, 8) - 128, D)
    return (c / tables.double().view(-1, 8, 8, 1, 1)).reshape(B, 64, H // 8, W // 8)


def extract64(c, tables):
    B, _, h, w = c.shape
    D = dct64()
    return (torch.einsum('ur,buvij,vs->birjs', D, c.double().reshape(B, 8, 8, h, w) * tables.double().view(-1, 8, 8, 1, 1), D) + 128).reshape(B, 1, 8 * h, 8 * w)


def tie_mask(pre_rounding64):
    """True where the float64 pre-rounding value lies within TIE_WINDOW of a half-integer"""
    f = pre_rounding64 - torch.floor(pre_rounding64)
    return (f - 0.5).abs() < TIE_WINDOW


# ------------------------------------------------------------------------------------------------ the reference
def main():
    from oracle import _refshim
    _refshim.install()
    torch.cuda.LongTensor = torch.LongTensor
    from JPEG_module.JPEG import JPEG
    import models.modules.architecture as arch
    out = {}

    def modules(qf_or_table, QF=True):
        ms = {'q': JPEG(compress=True, downsample_or_quantize=True), 'n': JPEG(compress=True, downsample_or_quantize=False), 'e': JPEG(compress=False)}
        for m in ms.values():
            m.Set_Q_Table(qf_or_table, QF=QF)
        return ms

    ms = modules(torch.tensor(QF_A, dtype=torch.float32))
    tables = ms['q'].Q_table.reshape(6, 64)
    out['a/qf'], out['a/tables'] = np.array(QF_A, np.float32), tables.numpy()
    for name, x in images_a().items():
        cq, cn = ms['q'](x), ms['n'](x)
        ties = float(tie_mask(compress64(x, tables)).double().mean())
        ref_err = float((cn.double() - compress64(x, tables)).abs().max())
        print('(a) %-6s ties within %g of a half-integer: %.3f %% (cap %.0f %%); reference fp32 vs float64: compressor %.2e, extractor %.2e / %.2e' % (
            name, TIE_WINDOW, 100 * ties, 100 * TIE_CAP, ref_err, float((ms['e'](cq).double() - extract64(cq, tables)).abs().max()),
            float((ms['e'](cn).double() - extract64(cn, tables)).abs().max())))
        assert ties <= TIE_CAP
        assert float(cq.abs().max()) < 32767 and torch.equal(cq, cq.round())
        out['a/%s/x' % name] = x.numpy().astype(np.uint8)
        out['a/%s/cq' % name], out['a/%s/cn' % name] = cq.numpy().astype(np.int16), cn.numpy()
        out['a/%s/img_q' % name], out['a/%s/img_n' % name] = ms['e'](cq).numpy(), ms['e'](cn).numpy()
    T = explicit_table()
    ms = modules([T], QF=False)
    x0 = images_a()['smooth'][:1]
    cq = ms['q'](x0)
    ties = float(tie_mask(compress64(x0, ms['q'].Q_table.reshape(1, 64))).double().mean())
    print('(a) explicit table: derived QF %.4f, ties %.3f %%' % (float(ms['q'].QF), 100 * ties))
    assert ties <= TIE_CAP
    out['a/explicit/table'], out['a/explicit/qf'], out['a/explicit/q_table'] = T, np.float64(ms['q'].QF), ms['q'].Q_table.reshape(64).numpy()
    out['a/explicit/cq'], out['a/explicit/img_q'] = cq.numpy(), ms['e'](cq).numpy()

    ms = modules(torch.tensor(QF_B, dtype=torch.float32))
    xb, Z, r = image_b(), latent_b(), cotangent_b()
    tb = ms['q'].Q_table.reshape(2, 64)
    coef = ms['q'](xb)
    ties = float(tie_mask(compress64(xb, tb)).double().mean())
    print('(b) ties %.3f %%' % (100 * ties))
    assert ties <= TIE_CAP
    out['b/x'], out['b/coef'], out['b/Z'], out['b/r'], out['b/tables'] = xb.numpy().astype(np.uint8), coef.numpy(), Z.numpy(), r.numpy(), tb.numpy()
    for mode in MODES:
        li = None if mode == 'None' else mode
        net = fill_generator(arch.DnCNN(n_channels=64, depth=5, in_nc=64, out_nc=64, norm_type='batch', latent_input=li, num_latent_channels=64,
                                        avoid_padding=False, output_layer='Sigmoid')).eval()
        pre = {}
        hook = net.dncnn[-2].register_forward_hook(lambda m, i, o: pre.__setitem__('y', o.detach().clone()))
        inp = (torch.cat([Z, coef], 1) if li else coef.clone()).requires_grad_(True)
        fake = net(inp)
        img = ms['e'](fake)
        (img * r).sum().backward()
        hook.remove()
        y = pre['y']
        sat = float((y.abs() > SATURATION).double().mean())
        gz = float(inp.grad[:, :64].abs().max()) if li else 0.0
        print('(b) %-11s |y| > %g: %.3f %% (cap %.0f %%), median |y| %.3f, max |y| %.3f; max |d/dZ| %.3g, max |d/dcoef| %.3g' % (
            mode, SATURATION, 100 * sat, 100 * SATURATION_CAP, float(y.abs().median()), float(y.abs().max()), gz, float(inp.grad[:, -64:].abs().max())))
        assert sat < SATURATION_CAP
        out['b/%s/keys' % mode] = np.array(list(net.state_dict().keys()))
        out['b/%s/out' % mode], out['b/%s/img' % mode] = fake.detach().numpy(), img.detach().numpy()
        out['b/%s/grad' % mode], out['b/%s/y' % mode] = inp.grad.numpy(), y.numpy()
    np.savez_compressed(GOLDEN, **out)
    print('%s: %d arrays, %d bytes' % (GOLDEN, len(out), os.path.getsize(GOLDEN)))


if __name__ == '__main__':
    main()
