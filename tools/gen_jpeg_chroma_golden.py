#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/jpeg_chroma.npz by running the REFERENCE's own JPEG module with
chroma_mode (codes/JPEG_module/JPEG.py), its DnCNN generators (codes/models/modules/architecture.py:109-214, Y and chroma forms) and
Tensor_YCbCR2RGB (codes/utils/util.py:328-330), imported read-only through oracle/_refshim.  Run:
    python tools/gen_jpeg_chroma_golden.py

As tools/gen_jpeg_golden.py does, this script sets torch.cuda.LongTensor = torch.LongTensor, which is all the reference needs to run on the CPU.
Weights are formula weights (fill_generator of tools/gen_jpeg_golden.py), so only inputs and outputs are stored.  The helpers of this file that
do not touch the reference (inputs, the float64 restatement of the 16-point transform) are imported by the tests.

(a) tables: QF = [5, 10, 30, 50, 75, 95] -> a/qf, a/padded [6, 3, 256], a/q [6, 3, 64]; the explicit form Set_Q_Table([lum, chroma], QF=False)
    -> a/explicit/lum, chroma [8, 8] (the tables passed), padded [3, 256], q [3, 64], qf
(b) module level: B = 3, 32 x 48 YCbCr (2 x 3 blocks), QF = [10, 40, 80]: b/tables [3, 3, 256], b/cq (compressor, quantising), b/cd
    ('downsample_only'), b/ca (all 768 channels), b/img128, b/img384, b/img512 (the extractor on cq[:, 256:], cq, ca[:, 256:]);
    b/explicit/cq, img384 on image 0 with the explicit tables;
    b/err/<name>: the reference's own fp32 distance from the float64 restatement, absolute (max) and relative to the largest value, for the
    compressor (unrounded) and the three extractor forms, and b/err/explicit/* for the explicit-table case — the tests' bounds are 4 x these
(c) model level: B = 2, 64 x 96, QF = [10, 40]; Y = smooth_pattern(seed 4100), Cb, Cr = 128 + 0.5 (smooth_pattern(seed 4110 / 4120) - 128),
    rounded; Z seeded in [-1, 1] on the Y grid [8, 12]; generators DnCNN(n_channels=64, depth=5, latent 64, Sigmoid, BatchNorm).
    For latent_input 'all_layers', 'first_layer', 'None' the composition of the reference's modules that DecompCNNModel.test() is
      y_channel_input = clamp(extractor_Y(netG_Y([Z | compressor_Y(Y)])), 0, 255);  var_Comp = compressor([y_channel_input | Cb | Cr])
      fake_H = netG([interpolate(Z) | var_Comp]);  output_image = [y_channel_input | extractor(fake_H)];  rgb = clamp(YCbCr2RGB(output_image / 255), 0, 1)
    c/<mode>/y (the chroma generator's last conv output, before the sigmoid), fake_H, keys (state_dict key list); for 'all_layers' also
    y_channel_input, var_Comp, output_image, rgb and grad = d sum(chroma image * r) / d [Z | var_Comp] of the chroma generator alone
(d) a reference Z_optimizer run on the colour model is NOT stored: it was not attempted for this fixture (the reference's search needs its
    GUI-side data plumbing), and the GPU search test compares with this build's CPU path instead, as for the Y model.

Conditions asserted here and again by tests/test_host_jpeg_chroma.py: fewer than 1 % of the chroma generator's pre-sigmoid outputs have
|y| > 6 in each latent mode, and at most 1 % of the rounded chroma coefficients of any stored case lie within 1e-3 of a rounding tie in float64."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.weights import seeded_uniform  # noqa: E402


def _load_y_tool():
    spec = importlib.util.spec_from_file_location('gen_jpeg_golden', os.path.join(ROOT, 'tools', 'gen_jpeg_golden.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


Y = _load_y_tool()            # smooth_pattern, fill_generator, tie_mask, the Y model's float64 restatement and the shared constants
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_chroma.npz')
QF_A = Y.QF_A
QF_B = [10, 40, 80]
QF_C = [10, 40]
MODES = Y.MODES
TIE_CAP, SATURATION, SATURATION_CAP = Y.TIE_CAP, Y.SATURATION, Y.SATURATION_CAP


# ------------------------------------------------------------------------------------------------ shared with the tests (no reference)
def ycbcr_pattern(B, H, W, seed):
    """Y a smooth pattern plus noise; Cb, Cr the same kind at half the contrast around 128; integers 0...255"""
    y = Y.smooth_pattern(B, H, W, seed)
    cb, cr = (torch.round(128 + 0.5 * (Y.smooth_pattern(B, H, W, seed + 10 * k) - 128)) for k in (1, 2))
    return torch.cat([y, cb, cr], 1)


def image_b():
    return ycbcr_pattern(3, 32, 48, 6100)


def image_c():
    return ycbcr_pattern(2, 64, 96, 4100)


def latent_c():
    return seeded_uniform((2, 64, 8, 12), 6200, -1.0, 1.0)


def cotangent_c():
    return seeded_uniform((2, 2, 64, 96), 6300, -1.0, 1.0)


def explicit_tables(chroma_k2):
    """the two explicit 8x8 tables of the Set_Q_Table([lum, chroma], QF=False) case"""
    return Y.explicit_table(), np.round(np.asarray(chroma_k2, dtype=np.float64) * 0.6 + 2)


def dct64_16():
    k = torch.arange(16, dtype=torch.float64).view(16, 1)
    n = torch.arange(16, dtype=torch.float64).view(1, 16)
    D = np.sqrt(0.125) * torch.cos((2 * n + 1) * k * np.pi / 32)
    D[0] = 0.25
    return D


def compress64_16(x, padded):
    """float64 coefficients of every plane before any rounding or truncation: [B, 3, 16, 16, h, w]; padded [B, 3, 256]"""
    B, _, H, W = x.shape
    D = dct64_16()
    blocks = x.double().reshape(B, 3, H // 16, 16, W // 16, 16) - torch.tensor([128., 0., 0.], dtype=torch.float64).view(1, 3, 1, 1, 1, 1)
    return torch.einsum('ur,bcirjs,vs->bcuvij', D, blocks, D) / padded.double().view(-1, 3, 16, 16, 1, 1)


def channels64_16(c, mode):
    """the compressor's channel layout of compress64_16's result: mode False (768), 'downsample_only' (384), True (384, chroma rounded)"""
    B, h, w = c.size(0), c.size(4), c.size(5)
    if mode is False:
        return c.reshape(B, 768, h, w)
    chroma = c[:, 1:, :8, :8].reshape(B, 128, h, w)
    return torch.cat([c[:, 0].reshape(B, 256, h, w), torch.round(chroma) if mode is True else chroma], 1)


def extract64_16(c, padded):
    """float64 image of an extractor input of 128 / 384 / 512 channels"""
    B, C, h, w = c.shape
    n, Ks = {128: (2, (8, 8)), 512: (2, (16, 16)), 384: (3, (16, 8, 8))}[C]
    D = dct64_16()
    full = torch.zeros(B, n, 16, 16, h, w, dtype=torch.float64)
    c0 = 0
    for k, K in enumerate(Ks):
        full[:, k, :K, :K] = c[:, c0:c0 + K * K].double().reshape(B, K, K, h, w)
        c0 += K * K
    img = torch.einsum('ur,bcuvij,vs->bcirjs', D, full * padded.double().view(-1, 3, 16, 16, 1, 1)[:, 3 - n:], D).reshape(B, n, 16 * h, 16 * w)
    if n == 3:
        img[:, 0] += 128
    return img


def chroma_ties(c64):
    """share of the rounded (low chroma) coefficients within the tie window of a half-integer, and the mask over the 384 channels"""
    B, h, w = c64.size(0), c64.size(4), c64.size(5)
    low = c64[:, 1:, :8, :8].reshape(B, 128, h, w)
    mask = torch.cat([torch.zeros(B, 256, h, w, dtype=torch.bool), Y.tie_mask(low)], 1)
    return float(Y.tie_mask(low).double().mean()), mask


def make_generators(arch, mode):
    """(netG_Y, netG) of a colour model at the fixture's size, formula weights"""
    li = None if mode == 'None' else mode
    kw = dict(n_channels=64, depth=5, norm_type='batch', latent_input=li, num_latent_channels=64, avoid_padding=False, output_layer='Sigmoid')
    g_y = Y.fill_generator(arch.DnCNN(in_nc=64, out_nc=64, **kw)).eval()
    g_c = Y.fill_generator(arch.DnCNN(in_nc=384, out_nc=128, chroma_generator=True, **kw)).eval()
    return g_y, g_c


# ------------------------------------------------------------------------------------------------ the reference
def main():
    from oracle import _refshim
    _refshim.install()
    torch.cuda.LongTensor = torch.LongTensor
    import JPEG_module.JPEG as RJ
    import models.modules.architecture as arch
    from utils.util import Tensor_YCbCR2RGB
    JPEG = RJ.JPEG
    out = {}

    def chroma_modules(qf_or_table, QF=True):
        ms = {'q': JPEG(True, True, chroma_mode=True, block_size=16), 'd': JPEG(True, 'downsample_only', chroma_mode=True, block_size=16),
              'a': JPEG(True, False, chroma_mode=True, block_size=16), 'e': JPEG(False, chroma_mode=True, block_size=16)}
        for m in ms.values():
            m.Set_Q_Table(qf_or_table, QF=QF)
        return ms

    # (a)
    ms = chroma_modules(torch.tensor(QF_A, dtype=torch.float32))
    assert ms['q'].padded_Q_table.shape == (6, 3, 16, 16, 1, 1) and ms['q'].Q_table.shape == (6, 3, 8, 8, 1, 1)
    out['a/qf'], out['a/padded'], out['a/q'] = np.array(QF_A, np.float32), ms['q'].padded_Q_table.reshape(6, 3, 256).numpy(), ms['q'].Q_table.reshape(6, 3, 64).numpy()
    lum, chroma = explicit_tables(RJ.CHROMINANCE_QUANTIZATION_TABLE)
    mx = chroma_modules([lum, chroma], QF=False)
    out['a/explicit/lum'], out['a/explicit/chroma'], out['a/explicit/qf'] = lum, chroma, np.float64(mx['q'].QF)
    out['a/explicit/padded'], out['a/explicit/q'] = mx['q'].padded_Q_table.reshape(3, 256).numpy(), mx['q'].Q_table.reshape(3, 64).numpy()

    # (b)
    ms = chroma_modules(torch.tensor(QF_B, dtype=torch.float32))
    xb = image_b()
    tb = ms['q'].padded_Q_table.reshape(3, 3, 256)
    c64 = compress64_16(xb, tb)
    ties, _ = chroma_ties(c64)
    print('(b) ties %.3f %% (cap %.0f %%)' % (100 * ties, 100 * TIE_CAP))
    assert ties <= TIE_CAP
    cq, cd, ca = ms['q'](xb), ms['d'](xb), ms['a'](xb)
    assert cq.shape == (3, 384, 2, 3) and cd.shape == (3, 384, 2, 3) and ca.shape == (3, 768, 2, 3)
    imgs = {'img128': ms['e'](cq[:, 256:]), 'img384': ms['e'](cq), 'img512': ms['e'](ca[:, 256:])}
    assert imgs['img128'].shape == (3, 2, 32, 48) and imgs['img384'].shape == (3, 3, 32, 48) and imgs['img512'].shape == (3, 2, 32, 48)
    out['b/tables'], out['b/cq'], out['b/cd'], out['b/ca'] = tb.numpy(), cq.numpy(), cd.numpy(), ca.numpy()
    for k, v in imgs.items():
        out['b/' + k] = v.numpy()

    def distance(name, got, want64, centre=0.0):
        e = float((got.double() - want64).abs().max())
        out['b/err/' + name] = np.array([e, e / float((want64 - centre).abs().max())])
        print('(b) reference fp32 vs float64, %-10s: %.2e absolute, %.2e relative' % (name, e, out['b/err/' + name][1]))
    distance('compress', ca, channels64_16(c64, False))
    distance('extract128', imgs['img128'], extract64_16(cq[:, 256:], tb))
    distance('extract384', imgs['img384'], extract64_16(cq, tb), centre=128.0)
    distance('extract512', imgs['img512'], extract64_16(ca[:, 256:], tb))
    tx = mx['q'].padded_Q_table.reshape(1, 3, 256)
    ties, _ = chroma_ties(compress64_16(xb[:1], tx))
    assert ties <= TIE_CAP
    out['b/explicit/cq'] = mx['q'](xb[:1]).numpy()
    out['b/explicit/img384'] = mx['e'](mx['q'](xb[:1])).numpy()
    # (the explicit tables are taken through process_Q_table, i.e. divided by 100: coefficients a hundred times larger, and so their error)
    distance('explicit/compress', mx['a'](xb[:1]), channels64_16(compress64_16(xb[:1], tx), False))
    distance('explicit/extract384', mx['e'](mx['q'](xb[:1])), extract64_16(mx['q'](xb[:1]), tx), centre=128.0)

    # (c)
    xc, Z, r = image_c(), latent_c(), cotangent_c()
    qf = torch.tensor(QF_C, dtype=torch.float32)
    ms = chroma_modules(qf)
    comp_y, ext_y = JPEG(True, True), JPEG(False)
    comp_y.Set_Q_Table(qf)
    ext_y.Set_Q_Table(qf)
    tc = ms['q'].padded_Q_table.reshape(2, 3, 256)
    out['c/tables'] = tc.numpy()
    Zc = torch.nn.functional.interpolate(Z, size=[4, 6], mode='bilinear', align_corners=True)
    for mode in MODES:
        g_y, g_c = make_generators(arch, mode)
        lat = mode != 'None'
        with torch.no_grad():
            coef_y = comp_y(xc[:, :1])
            y_in = torch.clamp(ext_y(g_y(torch.cat([Z, coef_y], 1) if lat else coef_y)), 0, 255)
            both = torch.cat([y_in, xc[:, 1:]], 1)
            var_comp = ms['q'](both)
        ties, _ = chroma_ties(compress64_16(both, tc))
        assert ties <= TIE_CAP
        pre = {}
        hook = g_c.dncnn[-2].register_forward_hook(lambda m, i, o: pre.__setitem__('y', o.detach().clone()))
        inp = (torch.cat([Zc, var_comp], 1) if lat else var_comp.clone()).requires_grad_(True)
        fake = g_c(inp)
        chroma_img = ms['e'](fake)
        (chroma_img * r).sum().backward()
        hook.remove()
        y = pre['y']
        sat = float((y.abs() > SATURATION).double().mean())
        print('(c) %-11s ties %.3f %%; |y| > %g: %.3f %% (cap %.0f %%), median |y| %.3f, max |y| %.3f; max |d/dZ| %.3g' % (
            mode, 100 * ties, SATURATION, 100 * sat, 100 * SATURATION_CAP, float(y.abs().median()), float(y.abs().max()),
            float(inp.grad[:, :64].abs().max()) if lat else 0.0))
        assert sat < SATURATION_CAP and fake.shape == (2, 128, 4, 6) and chroma_img.shape == (2, 2, 64, 96)
        out['c/%s/keys' % mode] = np.array(list(g_c.state_dict().keys()))
        out['c/%s/y' % mode], out['c/%s/fake_H' % mode] = y.numpy(), fake.detach().numpy()
        if mode == 'all_layers':
            image = torch.cat([y_in, chroma_img.detach()], 1)
            rgb = torch.clamp(Tensor_YCbCR2RGB(image / 255), 0, 1)
            out['c/all_layers/y_channel_input'], out['c/all_layers/var_Comp'] = y_in.numpy(), var_comp.numpy()
            out['c/all_layers/output_image'], out['c/all_layers/rgb'], out['c/all_layers/grad'] = image.numpy(), rgb.numpy(), inp.grad.numpy()
    np.savez_compressed(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print('%s: %d arrays, %d bytes' % (GOLDEN, len(out), size))
    assert size < os.path.getsize(Y.GOLDEN), 'the colour fixture stays smaller than the Y one'


if __name__ == '__main__':
    main()
