#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/jpeg_edit.npz by running the REFERENCE's own code for the JPEG decoder's
editing tools, imported read-only through oracle/_refshim: utils.util.SmearMask2JpegBlocks (codes/utils/util.py:318-326), its JPEG modules
(codes/JPEG_module/JPEG.py) and DecompCNNModel.Enforce_pair_Consistency / Return_Compressed (codes/models/DecompCNN_model.py:316-334, :731-740)
called as plain functions on a stand-in object that carries reference JPEG modules under the keys the methods read (the model's own and the two
its GUI adds, GUI.py:2357-2360).  Run:
    python tools/gen_jpeg_edit_golden.py

skvideo is not installed here and the reference's model file imports it at the top (for a score this fixture never calls): it is stubbed before
the import, as oracle/_refshim stubs cv2 and the like.  As tools/gen_jpeg_golden.py does, this script sets torch.cuda.LongTensor =
torch.LongTensor, which is all the reference's JPEG module needs to run on the CPU.  The helpers of this file that do not touch the reference
(inputs, the float64 restatements) are imported by the tests.

(a) a/smeared [32, 48]: SmearMask2JpegBlocks of label_mask(): labels 0...5 with several different non-zero values inside one block
(b) the imprint score (GUI.py:1026-1033), 32 x 48, QF 40: b/table [1, 64]; b/fixed_coef [1, 64, 4, 6], the quantising compressor's coefficients
    of fixed_image(); b/cand_coef [3, 64, 4, 6], the non-quantising compressor's of candidates() (the fixed image with a rectangle of another
    image imprinted, three positions); b/score [3], the reference's expression on them (fp32)
(c) Enforce_pair_Consistency, 48 x 64, QF 40: c/q8 [1, 64], c/padded [1, 3, 256] the tables; c/compressed [48, 64, 3] RGB 0...1 float32, a
    really decompressed image: Return_Compressed of ycbcr_image() through the reference's modules, converted with its Tensor_YCbCR2RGB and
    clamped; c/same = the method on (compressed, compressed), c/other = on (compressed, other_image(compressed)); c/err/same, c/err/other: the
    reference's own fp32 distance (max abs, in the 0...1 output) from pair64(), the float64 restatement below, on the same inputs.  The
    tests' bar is 4 x these.  For the second case also the two corrections on their own, the reference's modules composed as :320-333 composes
    them: c/coef_y [1, 64, 6, 8] and c/coef_chroma [1, 128, 3, 4] (the compressed image's quantised coefficients, int16), c/planes [1, 3, 48, 64]
    (Y | Cb | Cr on the planes the method works on) and c/err/plane_y, c/err/plane_chroma, their fp32 distance from planes64().
Asserted here and again by tests/test_host_jpeg_edit.py: no coefficient that Enforce_pair_Consistency re-quantises (the compressed image's Y and
low chroma coefficients on the planes the method builds, in float64) lies within 0.05 of a half-integer, so rounding cannot differ between two
fp32 implementations; should a change of seed or QF ever break this, requantised() reports the share, which must stay under 1 %."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import importlib.util  # noqa: E402

from oracle.weights import seeded_uniform  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


C = _load('gen_jpeg_chroma_golden')        # ycbcr_pattern, the 16-point float64 restatement; C.Y: the 8-point one
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_edit.npz')
QF = 40.0
TIE_MARGIN, TIE_CAP = 0.05, 0.01
# the reference's conversion constants (utils/util.py:329-330; data/util.py:165-166)
YCBCR2RGB = np.array([[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]])
YCBCR2RGB_OFFSET = np.array([-222.921, 135.576, -276.836])
RGB2YCBCR = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])


# ------------------------------------------------------------------------------------------------ shared with the tests (no reference)
def label_mask():
    """[32, 48] uint8 labels 0...5: blocks with one label, with several, with a single pixel, and empty ones"""
    m = np.zeros((32, 48), dtype=np.uint8)
    m[2:7, 3:6] = 1
    m[5:12, 4:20] = 2            # crosses blocks, meets label 1 inside block (0, 0)
    m[9, 30] = 5                 # a single pixel
    m[16:24, 8:16] = 3           # exactly one block
    m[20:27, 14:18] = 4          # meets 3 inside block (2, 1)
    m[31, 47] = 1                # the last pixel
    return m


def fixed_image():
    return C.Y.smooth_pattern(1, 32, 48, 8100)


def candidates():
    """[3, 1, 32, 48]: the fixed image with a 12 x 16 rectangle of another image imprinted at three positions (one of them block-aligned)"""
    fixed, other = fixed_image(), C.Y.smooth_pattern(1, 32, 48, 8200)
    out = []
    for top, left in ((8, 16), (3, 5), (17, 29)):
        im = fixed.clone()
        im[:, :, top:top + 12, left:left + 16] = 0.5 * (other[:, :, top:top + 12, left:left + 16] + fixed[:, :, top:top + 12, left:left + 16])
        out.append(im)
    return torch.cat(out, 0)


def ycbcr_image():
    """[1, 3, 48, 64] YCbCr, 0...255, moderate contrast (its RGB stays inside [0, 1] almost everywhere)"""
    x = C.ycbcr_pattern(1, 48, 64, 8300)
    return torch.cat([128 + 0.6 * (x[:, :1] - 128), 128 + 0.5 * (x[:, 1:] - 128)], 1).round()


def other_image(compressed):
    """the second case's desired image: the compressed image with a smooth colour change and an imprinted rectangle, HWC RGB in 0...1 float32"""
    H, W, _ = compressed.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    wave = np.stack([0.08 * np.sin(xx / 5 + k) * np.cos(yy / 7 - k) for k in range(3)], -1)
    noise = 0.1 * (seeded_uniform((H, W, 3), 8400).double().numpy() - 0.5)
    out = compressed.astype(np.float64) + wave + noise
    out[10:30, 20:44] = 0.5 + 0.3 * np.sin(xx[10:30, 20:44, None] / 3 + np.arange(3))
    return np.clip(out, 0, 1).astype(np.float32)


def planes_of(im):
    """what the reference's im_2_tensor builds (DecompCNN_model.py:317-318 with data/util.py:150-171 on a 0...255 FLOAT image): the image is
    multiplied by 255 a second time, so after the final division the offsets are (16, 128, 128) / 255.  float32 in, float64 product, float32 out."""
    x = (255 * np.asarray(im, dtype=np.float32)) * np.float32(255.)
    ycc = (np.matmul(x, RGB2YCBCR) / 255.0 + [16, 128, 128]) / 255.
    return torch.from_numpy(np.ascontiguousarray(ycc.astype(np.float32).transpose((2, 0, 1)))).unsqueeze(0)


def requantised(compressed, q8, padded):
    """(float64 pre-rounding Y coefficients [1, 64, h8, w8], low chroma [1, 2, 8, 8, h, w], share within TIE_MARGIN of a half-integer)"""
    p = planes_of(compressed)
    cy = C.Y.compress64(p[:, :1], q8)
    cc = C.compress64_16(p, padded)[:, 1:, :8, :8]
    both = torch.cat([cy.reshape(-1), cc.reshape(-1)])
    f = both - torch.floor(both)
    return cy, cc, float(((f - 0.5).abs() < TIE_MARGIN).double().mean())


def planes64(compressed, desired, q8, padded):
    """float64 restatement of DecompCNN_model.py:319-333 from the float32 planes on: the corrected [1, 3, H, W] planes (Y | Cb | Cr)"""
    def correct(d, k):
        return torch.clamp(d - k, -0.5, 0.5) + k
    dp = planes_of(desired)
    cy, cc, _ = requantised(compressed, q8, padded)
    Yp = C.Y.extract64(correct(C.Y.compress64(dp[:, :1], q8), torch.round(cy)), q8)
    d16 = C.compress64_16(dp, padded)[:, 1:].clone()
    d16[:, :, :8, :8] = correct(d16[:, :, :8, :8], torch.round(cc))
    h, w = d16.shape[-2:]
    return torch.cat([Yp, C.extract64_16(d16.reshape(1, 512, h, w), padded)], 1)


def pair64(compressed, desired, q8, padded):
    """float64 restatement of the whole method (:316-334): HWC RGB float64 in 0...1"""
    image = planes64(compressed, desired, q8, padded)
    mat = torch.from_numpy(255 * YCBCR2RGB.transpose())
    rgb = (torch.einsum('rc,bchw->brhw', mat, image) + torch.from_numpy(YCBCR2RGB_OFFSET).view(1, 3, 1, 1) / 255) / 255
    return torch.clamp(rgb, 0, 1)[0].numpy().transpose((1, 2, 0))


# ------------------------------------------------------------------------------------------------ the reference
def main():
    from oracle import _refshim
    _refshim.install()
    torch.cuda.LongTensor = torch.LongTensor
    sk = _refshim._stub('skvideo')
    sk.measure = _refshim._stub('skvideo.measure', niqe=None)
    import JPEG_module.JPEG as RJ
    from utils import util as rutil
    from models.DecompCNN_model import DecompCNNModel as RefModel
    JPEG = RJ.JPEG
    qf = torch.tensor([QF], dtype=torch.float32)
    out = {}

    # (a)
    out['a/smeared'] = rutil.SmearMask2JpegBlocks(label_mask())
    assert out['a/smeared'].shape == (32, 48) and len(np.unique(out['a/smeared'])) > 3

    # (b)
    comp_q, comp_n = JPEG(compress=True, downsample_or_quantize=True), JPEG(compress=True, downsample_or_quantize=False)
    for m in (comp_q, comp_n):
        m.Set_Q_Table(qf)
    fixed_coef, cand_coef = comp_q(fixed_image()), comp_n(candidates())
    score = torch.max(torch.tensor(0).type(fixed_coef.type()), (cand_coef - fixed_coef).abs() - 0.5).sum(-1).sum(-1).sum(-1)
    out['b/table'], out['b/fixed_coef'], out['b/cand_coef'], out['b/score'] = comp_q.Q_table.reshape(1, 64).numpy(), fixed_coef.numpy(), cand_coef.numpy(), score.numpy()
    print('(b) scores', score.tolist())
    assert cand_coef.shape == (3, 64, 4, 6) and float(score.min()) > 0

    # (c)
    stand_in = types.SimpleNamespace(chroma_mode=True, JPEG={
        'compressor_Y': JPEG(compress=True, chroma_mode=False, downsample_or_quantize=True, block_size=8),
        'extractor_Y': JPEG(compress=False, chroma_mode=False, block_size=8),
        'compressor': JPEG(compress=True, chroma_mode=True, downsample_or_quantize=True, block_size=16),
        'extractor': JPEG(compress=False, chroma_mode=True, block_size=16),
        'compressor_Y_non_quantized': JPEG(compress=True, chroma_mode=False, downsample_or_quantize=False, block_size=8),
        'compressor_non_quantized': JPEG(compress=True, chroma_mode=True, downsample_or_quantize=False, block_size=16)})
    for m in stand_in.JPEG.values():
        m.Set_Q_Table(qf)
    q8 = stand_in.JPEG['compressor_Y'].Q_table.reshape(1, 64)
    padded = stand_in.JPEG['compressor'].padded_Q_table.reshape(1, 3, 256)
    out['c/q8'], out['c/padded'] = q8.numpy(), padded.numpy()
    decompressed = RefModel.Return_Compressed(stand_in, ycbcr_image())
    rgb = torch.clamp(rutil.Tensor_YCbCR2RGB(decompressed / 255), 0, 1)
    print('(c) RGB of the decompressed image: %.3f %% of the values clamped' % (100 * float(((rgb == 0) | (rgb == 1)).double().mean())))
    compressed = np.ascontiguousarray(rgb[0].numpy().transpose((1, 2, 0))).astype(np.float32)
    out['c/compressed'] = compressed
    _, _, share = requantised(compressed, q8, padded)
    print('(c) re-quantised coefficients within %.2f of a half-integer: %.3f %%' % (TIE_MARGIN, 100 * share))
    assert share == 0.0, 'choose another seed or QF (the tie rule of tests/test_host_jpeg.py would allow up to %.0f %%)' % (100 * TIE_CAP)
    for name, desired in (('same', compressed), ('other', other_image(compressed))):
        got = RefModel.Enforce_pair_Consistency(stand_in, compressed.copy(), desired.copy())
        want = pair64(compressed, desired, q8, padded)
        assert got.shape == (48, 64, 3) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        out['c/' + name], out['c/err/' + name] = got, np.float64(err)
        print('(c) %-5s reference fp32 vs float64: %.3g; moved the desired image by up to %.3g; clamped %.3f %%' % (
            name, err, float(np.abs(got - desired).max()), 100 * float(((got == 0) | (got == 1)).mean())))
        assert 0 < err < 1e-4
    # the two corrections on their own, for the second case: the reference's modules composed as :320-333 composes them
    J_ = stand_in.JPEG
    other = other_image(compressed)
    cp, dp = planes_of(compressed), planes_of(other)
    coef_y, coef_c = J_['compressor_Y'](cp[:, :1]), J_['compressor'](cp)[:, 256:]
    Yp = J_['extractor_Y'](torch.clamp(J_['compressor_Y_non_quantized'](dp[:, :1]) - coef_y, -0.5, 0.5) + coef_y)
    full = J_['compressor_non_quantized'](dp)[:, 256:].reshape(1, 2, 16, 16, 3, 4).clone()
    low = coef_c.reshape(1, 2, 8, 8, 3, 4)
    full[:, :, :8, :8] = torch.clamp(full[:, :, :8, :8] - low, -0.5, 0.5) + low
    planes = torch.cat([Yp, J_['extractor'](full.reshape(1, 512, 3, 4))], 1)
    want = planes64(compressed, other, q8, padded)
    cy64, cc64, _ = requantised(compressed, q8, padded)
    assert torch.equal(coef_y.double(), torch.round(cy64)) and torch.equal(coef_c.double(), torch.round(cc64).reshape(1, 128, 3, 4))
    out['c/coef_y'], out['c/coef_chroma'], out['c/planes'] = coef_y.numpy().astype(np.int16), coef_c.numpy().astype(np.int16), planes.numpy()
    for k, name in ((slice(0, 1), 'plane_y'), (slice(1, 3), 'plane_chroma')):
        out['c/err/' + name] = np.float64((planes[:, k].double() - want[:, k]).abs().max())
        print('(c) %-12s reference fp32 vs float64: %.3g (0...255 planes)' % (name, out['c/err/' + name]))
    np.savez_compressed(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print('%s: %d arrays, %d bytes' % (GOLDEN, len(out), size))
    assert size < os.path.getsize(C.GOLDEN) // 4, 'the fixture stays well under the size of jpeg_chroma.npz'


if __name__ == '__main__':
    main()
