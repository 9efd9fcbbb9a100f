"""CPU tests of the JPEG decoder's editing tools against tests/golden/jpeg_edit.npz (the reference's SmearMask2JpegBlocks, JPEG modules and
Enforce_pair_Consistency, written by tools/gen_jpeg_edit_golden.py): esr_hip.jpeg_edit's defining expressions, the model's
Enforce_pair_Consistency, the block-grid Z mask and the editing Z objectives through the colour model.

Bounds.  The fp32 expressions here run other torch ops, in another order, than the reference's modules; each is held to 4 x the reference's OWN
fp32 distance from a float64 restatement on the same input (c/err/* in the fixture), the convention of tests/test_gpu_jpeg.py.  Properties of
the projection are stated with the slack measured on the spot as the fp32 result's distance from float64."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle.weights import seeded_uniform
from test_host_jpeg_chroma import C, make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, 'tests', 'golden', 'jpeg_edit.npz')


def _load_tool():
    spec = importlib.util.spec_from_file_location('gen_jpeg_edit_golden', os.path.join(ROOT, 'tools', 'gen_jpeg_edit_golden.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E = _load_tool()              # inputs and float64 restatements shared with the fixture's generator
_golden = {}


def golden():
    if not _golden:
        with np.load(FX) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def gt(key):
    return torch.from_numpy(np.asarray(golden()[key]))


def test_fixture_holds_its_conditions():
    g = golden()
    assert os.path.getsize(FX) < os.path.getsize(C.GOLDEN) // 4
    cy, cc, share = E.requantised(g['c/compressed'], gt('c/q8'), gt('c/padded'))
    assert share == 0.0                                           # no re-quantised coefficient within 0.05 of a rounding tie
    assert torch.equal(torch.round(cy), gt('c/coef_y').double()) and torch.equal(torch.round(cc).reshape(1, 128, 3, 4), gt('c/coef_chroma').double())
    for k in ('same', 'other', 'plane_y', 'plane_chroma'):
        assert 0 < float(g['c/err/' + k]) < 1e-3


# ------------------------------------------------------------------------------------------------ colour conversion
def test_ycbcr_to_rgb_on_the_cpu_is_the_models_expression_bit_for_bit():
    from esr_hip import jpeg_edit
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    x = C.ycbcr_pattern(2, 32, 48, 9100) + seeded_uniform((2, 3, 32, 48), 9101, -20.0, 20.0)       # also values outside 0...255
    assert torch.equal(jpeg_edit.ycbcr_to_rgb(x), Tensor_YCbCR2RGB(x / 255))
    assert torch.equal(jpeg_edit.ycbcr_to_rgb(x.double()), Tensor_YCbCR2RGB(x.double() / 255))
    with pytest.raises(ValueError, match='ycbcr_to_rgb'):
        jpeg_edit.ycbcr_to_rgb(x[:, :2])


def test_ycbcr_to_rgb_gradient_is_the_transposed_matrix():
    from esr_hip import jpeg_edit
    x = C.ycbcr_pattern(1, 16, 16, 9110).double().requires_grad_(True)
    g = seeded_uniform((1, 3, 16, 16), 9111, -1.0, 1.0).double()
    (jpeg_edit.ycbcr_to_rgb(x) * g).sum().backward()
    want = torch.einsum('cr,brhw->bchw', torch.from_numpy(E.YCBCR2RGB), g)                           # (255 M^T)^T / 255 = M
    assert float((x.grad - want).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------ candidate score
def test_consistency_violation_against_float64_and_the_fixture():
    from esr_hip import jpeg_edit
    g = golden()
    cand, coef, table = E.candidates(), gt('b/fixed_coef'), gt('b/table')
    want = torch.clamp((C.Y.compress64(cand, table) - coef.double()).abs() - 0.5, min=0).sum(dim=(1, 2, 3))
    got = jpeg_edit.consistency_violation(cand, coef, table)
    assert got.shape == (3,) and got.dtype == torch.float64
    # the reference's own coefficients and its fp32 sum: the score's distance from float64 bounds ours at 4 x
    ref_err = float((torch.from_numpy(g['b/score']).double() - want).abs().max())
    print('score %s, float64 %s; reference off by %.3g, this build by %.3g' % (got.tolist(), want.tolist(), ref_err, float((got - want).abs().max())))
    assert ref_err > 0 and float((got - want).abs().max()) <= 4 * ref_err
    assert float((got - torch.from_numpy(g['b/score']).double()).abs().max()) <= 5 * ref_err
    assert torch.equal(torch.argsort(got), torch.argsort(want))
    # one coefficient tensor and table for all, or one per candidate
    per = jpeg_edit.consistency_violation(cand, coef.expand(3, -1, -1, -1).contiguous(), table.expand(3, -1).contiguous())
    assert torch.equal(per, got)
    # different coefficients per candidate: each row is the one-candidate call
    coefs = torch.cat([coef, coef + 1, torch.round(C.Y.compress64(cand[2:], table)).float()], 0)
    rows = jpeg_edit.consistency_violation(cand, coefs, table)
    for n in range(3):
        assert torch.equal(rows[n:n + 1], jpeg_edit.consistency_violation(cand[n:n + 1], coefs[n:n + 1], table))
    assert float(rows[2]) < 1e-3 and float(rows[1]) > float(rows[0])         # a candidate scored against its own code: inside the set
    with pytest.raises(ValueError, match='consistency_violation'):
        jpeg_edit.consistency_violation(cand, coef[:, :32], table)
    with pytest.raises(ValueError, match='tables'):
        jpeg_edit.consistency_violation(cand, coef, table.expand(2, -1))


# ------------------------------------------------------------------------------------------------ pair consistency
def _pair_case():
    g = golden()
    compressed = g['c/compressed']
    return E.planes_of(compressed), E.planes_of(E.other_image(compressed)), gt('c/coef_y').float(), gt('c/coef_chroma').float(), gt('c/q8'), gt('c/padded')


def test_consistent_plane_and_chroma_against_the_fixture():
    from esr_hip import jpeg_edit
    g = golden()
    cp, dp, ky, kc, q8, padded = _pair_case()
    want = E.planes64(g['c/compressed'], E.other_image(g['c/compressed']), q8, padded)
    y = jpeg_edit.consistent_plane(dp[:, :1], ky, q8)
    ch = jpeg_edit.consistent_chroma(dp, kc, padded)
    assert y.shape == (1, 1, 48, 64) and ch.shape == (1, 2, 48, 64)
    for got, k, name in ((y, slice(0, 1), 'plane_y'), (ch, slice(1, 3), 'plane_chroma')):
        ref_err = float(g['c/err/' + name])
        err64, err_fx = float((got.double() - want[:, k]).abs().max()), float((got - gt('c/planes')[:, k]).abs().max())
        print('%s: %.3g from float64 (reference %.3g), %.3g from the fixture' % (name, err64, ref_err, err_fx))
        assert err64 <= 4 * ref_err and err_fx <= 5 * ref_err
    # two planes alone, and the compressor's 384 channels in place of their last 128
    assert torch.equal(jpeg_edit.consistent_chroma(dp[:, 1:].contiguous(), kc, padded), ch)
    assert torch.equal(jpeg_edit.consistent_chroma(dp, torch.cat([torch.zeros(1, 256, 3, 4), kc], 1), padded), ch)
    with pytest.raises(ValueError, match='consistent_plane'):
        jpeg_edit.consistent_plane(dp, ky, q8)
    with pytest.raises(ValueError, match='consistent_chroma'):
        jpeg_edit.consistent_chroma(dp, kc[:, :64], padded)


def test_projection_properties():
    from esr_hip import jpeg as J, jpeg_edit
    g = golden()
    cp, dp, ky, kc, q8, padded = _pair_case()
    want = E.planes64(g['c/compressed'], E.other_image(g['c/compressed']), q8, padded)
    y, ch = jpeg_edit.consistent_plane(dp[:, :1], ky, q8), jpeg_edit.consistent_chroma(dp, kc, padded)
    # re-compressed unrounded, the result lies within 0.5 of the quantised coefficients; slack: the result's fp32 distance from float64, which
    # a coefficient sees divided by its table entry (>= 1) and, the transform being orthonormal, multiplied by at most the block side
    slack_y = 8 * float((y.double() - want[:, :1]).abs().max()) / float(q8.min()) + 1e-12
    slack_c = 16 * float((ch.double() - want[:, 1:]).abs().max()) / float(padded.min()) + 1e-12
    dev_y = float((C.Y.compress64(y, q8) - ky.double()).abs().max())
    low = C.compress64_16(torch.cat([torch.zeros(1, 1, 48, 64), ch], 1), padded)[:, 1:]
    dev_c = float((low[:, :, :8, :8].reshape(1, 128, 3, 4) - kc.double()).abs().max())
    print('largest deviation from the code: Y %.7f (slack %.2g), chroma %.7f (slack %.2g)' % (dev_y, slack_y, dev_c, slack_c))
    assert 0.4 < dev_y <= 0.5 + slack_y and 0.4 < dev_c <= 0.5 + slack_c          # (the desired image does push against the bound)
    # the 16-point form leaves the desired chroma's high frequencies as they were
    high_want = C.compress64_16(dp, padded)[:, 1:].clone()
    high_want[:, :, :8, :8] = 0
    high_got = low.clone()
    high_got[:, :, :8, :8] = 0
    assert float(high_want.abs().max()) > 1e-2 and float((high_got - high_want).abs().max()) <= slack_c
    # an image that is consistent already comes back unchanged; applying the projection twice equals applying it once
    for once, again, image64, what in ((y, jpeg_edit.consistent_plane(y, ky, q8), want[:, :1], 'Y'),
                                       (ch, jpeg_edit.consistent_chroma(ch, kc, padded), want[:, 1:], 'chroma')):
        # (the projection clamps orthonormal coordinates: it is non-expansive in L2, so the second pass moves `once` by at most twice its
        # distance from the exact projection, plus its own rounding of the same size)
        slack = 4 * float((once.double() - image64).norm())
        print('%s: twice vs once %.3g in L2 (slack %.3g)' % (what, float((again - once).norm()), slack))
        assert float((again - once).norm()) <= slack
    same_y = jpeg_edit.consistent_plane(cp[:, :1], ky, q8)
    same_c = jpeg_edit.consistent_chroma(cp, kc, padded)
    # (the compressed image's own planes: its chroma holds no high frequencies, its coefficients sit near integers)
    assert float((same_y - cp[:, :1]).abs().max()) <= 4 * float(g['c/err/plane_y'])
    assert float((same_c - cp[:, 1:]).abs().max()) <= 4 * float(g['c/err/plane_chroma'])
    # the CPU expressions are the compositions of the existing ops that the module names
    c = J.compress(dp[:, :1], q8, False)
    assert torch.equal(y, J.extract(torch.clamp(c - ky, -.5, .5) + ky, q8)[1])


# ------------------------------------------------------------------------------------------------ mask smearing
def test_smear_mask_to_blocks():
    from esr_hip import jpeg_edit
    m = E.label_mask()
    got = jpeg_edit.smear_mask_to_blocks(m)
    assert got.dtype == m.dtype and np.array_equal(got, golden()['a/smeared'])
    assert got[0, 0] == 2 and got[16, 8] == 4 and got[8, 24] == 5 and got[24, 40] == 1 and got[0, 40] == 0      # the largest label of a block wins
    assert np.array_equal(jpeg_edit.smear_mask_to_blocks(m.astype(np.float32), 16), np.kron(m.reshape(2, 16, 3, 16).max((1, 3)), np.ones((16, 16), np.float32)))
    for bad in (np.zeros((30, 48)), np.zeros((32, 47)), np.zeros((32,))):
        with pytest.raises(ValueError, match='whole'):
            jpeg_edit.smear_mask_to_blocks(bad)


# ------------------------------------------------------------------------------------------------ the model
def _with_gui_keys(model):
    from JPEG_module.JPEG import JPEG
    model.JPEG['compressor_Y_non_quantized'] = JPEG(compress=True, chroma_mode=False, downsample_or_quantize=False, block_size=8)
    model.JPEG['compressor_non_quantized'] = JPEG(compress=True, chroma_mode=True, downsample_or_quantize=False, block_size=16)
    for m in model.JPEG.values():
        m.Set_Q_Table(torch.tensor([E.QF], dtype=torch.float32).to(model.device))
    return model


def check_enforce_pair_consistency(model):
    """shared with the GPU test: the method against the fixture, 4 x the reference's own fp32 distance from float64 (+ the reference's own)"""
    g = golden()
    compressed = g['c/compressed']
    with pytest.raises(NotImplementedError, match='Enforce_pair_Consistency'):
        model.Enforce_pair_Consistency(compressed, compressed)                   # a fresh model: the two keys are the GUI's to add
    keys = set(model.JPEG)
    _with_gui_keys(model)
    assert set(model.JPEG) == keys | {'compressor_Y_non_quantized', 'compressor_non_quantized'}
    for name, desired in (('same', compressed), ('other', E.other_image(compressed))):
        kept = (compressed.copy(), desired.copy())
        got = model.Enforce_pair_Consistency(compressed, desired)
        assert np.array_equal(compressed, kept[0]) and np.array_equal(desired, kept[1])          # the caller's arrays are left alone
        assert isinstance(got, np.ndarray) and got.shape == (48, 64, 3) and got.dtype == np.float32 and got.min() >= 0 and got.max() <= 1
        ref_err = float(g['c/err/' + name])
        err64 = float(np.abs(got - E.pair64(compressed, desired, gt('c/q8'), gt('c/padded'))).max())
        err_fx = float(np.abs(got - g['c/' + name]).max())
        print('%s: %.3g from float64 (reference %.3g), %.3g from the fixture' % (name, err64, ref_err, err_fx))
        assert err64 <= 4 * ref_err and err_fx <= 5 * ref_err
    assert float(np.abs(model.Enforce_pair_Consistency(compressed, compressed) - compressed).max()) < 1e-5     # consistent already: unchanged
    with pytest.raises(ValueError, match='multiples of 16'):
        model.Enforce_pair_Consistency(compressed[:40], compressed[:40])


def test_enforce_pair_consistency_matches_the_fixture(tmp_path):
    model = make_model(tmp_path)
    with pytest.raises(NotImplementedError, match='Enforce_pair_Consistency'):
        model.Enforce_pair_Consistency(None, None)
    check_enforce_pair_consistency(model)


def test_output_image_on_the_cpu_is_unchanged(tmp_path):
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    model = make_model(tmp_path)
    model.output_image = C.ycbcr_pattern(1, 32, 48, 9200)
    assert torch.equal(model.Output_Image_0_1(), Tensor_YCbCR2RGB(model.output_image / 255))


# ------------------------------------------------------------------------------------------------ the block-grid Z mask
def _z_mask_restated(image_mask, jpeg):
    """reference Z_optimization.py:353-363 with scipy's maximum filter for cv2.dilate(mask, ones(16, 16)): OpenCV anchors an even kernel at
    (8, 8), so output (y, x) is the maximum over input rows y - 8 ... y + 7, which is maximum_filter's window at origin 0; outside the image
    nothing is set"""
    from scipy import ndimage
    m = np.asarray(image_mask, dtype=np.float64)
    dilated = ndimage.maximum_filter(m, footprint=np.ones((16, 16)), mode='constant', cval=0.0, origin=0)
    margins = 24
    if jpeg:
        new = np.zeros((m.shape[0] // 8, m.shape[1] // 8))
        new[margins // 8:-margins // 8, margins // 8:-margins // 8] = 1
        dilated = np.max(np.max(dilated.reshape([new.shape[0], 8, new.shape[1], 8]), -1), 1)
    else:
        new = np.zeros(m.shape)
        new[margins:-margins, margins:-margins] = 1
    return np.minimum(1, new + dilated)


@pytest.mark.parametrize('case', ['border', 'interior', 'small'])
def test_block_grid_z_mask(case):
    from esr_hip import scribble
    H, W = (32, 40) if case == 'small' else (96, 128)
    m = np.zeros((H, W), np.float32)
    if case == 'border':
        m[0:5, 100:128] = 1
        m[60:70, 0:3] = 1
    elif case == 'interior':
        m[40:47, 52:61] = 1
    else:
        m[10:12, 17:19] = 1
    got = scribble.rebuilt_z_mask(m, block_size=8)
    assert got.shape == (H // 8, W // 8) and got.dtype == np.float32
    assert np.array_equal(got, _z_mask_restated(m, True))
    assert 0 < got.sum() < got.size or case != 'small'
    if case == 'small':                                            # smaller than the margins: E is empty, only the dilated mask is left
        assert got.sum() == 9 and got[0:3, 1:4].all()              # pixels 10-11, 17-18 dilate to rows 3...19, columns 10...26
    # the SR form is what it was: the pixel grid, margins of 24
    sr = scribble.rebuilt_z_mask(m)
    E_ = np.zeros((H, W))
    E_[24:-24, 24:-24] = 1
    assert sr.shape == (H, W) and np.array_equal(sr, np.minimum(1, E_ + scribble.dilate16(m)).astype(np.float32))
    assert np.array_equal(sr, _z_mask_restated(m, False))
    with pytest.raises(ValueError, match='whole'):
        scribble.rebuilt_z_mask(np.zeros((30, 40)), block_size=8)


# ------------------------------------------------------------------------------------------------ Z search through the colour model
H_, W_ = 32, 48


class SRStandIn:
    """An SR-mode model whose fake_H is the JPEG model's Output_Image_0_1(): what the JPEG-mode objectives are defined on"""

    def __init__(self, jpeg_model):
        self.m = jpeg_model
        self.device, self.num_latent_channels, self.netG = jpeg_model.device, jpeg_model.num_latent_channels, jpeg_model.netG

    def feed_data(self, data, need_GT=False):
        B = data['Z'].size(0)
        self.m.feed_data({'Uncomp': data['Uncomp'].expand(B, -1, -1, -1), 'QF': data['QF'].expand(B), 'Z': data['Z']}, need_GT=False, detach_Y=False)

    def test(self, prevent_grads_calc=True):
        self.m.test(prevent_grads_calc=prevent_grads_calc)
        self.fake_H = self.output_image = self.m.Output_Image_0_1()

    def GetLatent(self):
        return self.m.GetLatent()

    def Output_Batch(self, within_0_1):
        return torch.clamp(self.fake_H, 0, 1)


def poison_fake_H(model):
    """fake_H holds coefficients in JPEG mode: NaN after every test(), so that an objective that still reads it as an image fails loudly"""
    real = model.test

    def test(*a, **k):
        real(*a, **k)
        model.fake_H = torch.full_like(model.fake_H.detach(), float('nan'))
    model.test = test
    return model


def edit_case(objective, device='cpu'):
    """(data, optimizer keywords, batch) of one objective of every newly accepted family, at 32 x 48"""
    x = C.image_c()[:1, :, :H_, :W_].contiguous().to(device)
    data = {'Uncomp': x, 'QF': torch.tensor(C.QF_C[:1], dtype=torch.float32).to(device)}
    kw, batch = {}, 1
    mask = np.zeros((H_, W_), np.float32)
    mask[8:24, 8:32] = 1                                           # whole blocks, as the GUI's smeared masks
    desired = seeded_uniform((1, 3, H_, W_), 9300, 0.2, 0.8).to(device)
    if objective == 'scribble':
        s = np.zeros((H_, W_), np.int64)
        s[9:13, 10:20] = 1
        s[16:22, 12:18] = 2
        s[14:23, 24:30] = 5
        from esr_hip import jpeg_edit
        data.update(desired=desired, scribble_mask=jpeg_edit.smear_mask_to_blocks(s), brightness_factor=0.2)
        kw.update(image_mask=mask, Z_mask=mask.reshape(4, 8, 6, 8).max((1, 3)), non_local_Z_optimization=True)
    elif objective in ('local_min_STD', 'local_STD_increase', 'local_Mag_increase'):
        data['STD_increment'] = 0.03
        kw.update(image_mask=mask, Z_mask=mask.reshape(4, 8, 6, 8).max((1, 3)))
    elif 'periodicity' in objective:
        data.update(periodicity_points=[[2.5, 1.25]], STD_increment=0.03)
        kw.update(image_mask=mask, Z_mask=mask.reshape(4, 8, 6, 8).max((1, 3)))
    elif objective in ('hist', 'patchdict_noDC'):
        data['desired'] = [desired[0]] if objective == 'hist' else desired
    elif objective.startswith('random_l1'):
        data['rmse_weight'] = 0.5
        batch = 2
    return data, kw, batch


def run_edit_search(model, objective, jpeg, iters=6, seed=9400):
    """The model's current output (what an objective takes its initial STD, brightened pixels and constraint image from) is that of a seeded Z;
    the search starts from a second one close by, so that the region constraint's |out - initial| has no ties at 0, whose gradient sign would
    be rounding noise in any implementation (as tools/gen_scribble_golden.py arranges it).  Returns (optimizer, final Z, starting Z)."""
    import Z_optimization
    data, kw, batch = edit_case(objective, model.device)
    Z0 = seeded_uniform((batch, 64, 4, 6), seed, -0.5, 0.5).to(model.device)
    Z1 = Z0 + seeded_uniform((batch, 64, 4, 6), seed + 1, -0.05, 0.05).to(model.device)
    inner = model.m if isinstance(model, SRStandIn) else model
    inner.feed_data({'Uncomp': data['Uncomp'].expand(batch, -1, -1, -1), 'QF': data['QF'].expand(batch), 'Z': Z0}, need_GT=False)
    model.test()
    real_mask = Z_optimization.esr_scribble.rebuilt_z_mask
    if not jpeg:
        data['LR'] = torch.zeros(1, 1, 1, 1)
        # SR mode rebuilds the Z mask on the pixel grid; the stand-in's Z lives on the block grid, so it gets the block-grid mask
        Z_optimization.esr_scribble.rebuilt_z_mask = lambda m, block_size=1: real_mask(m, block_size=8)
    torch.manual_seed(seed)                                       # ('random_l1_limited' perturbs its start)
    try:
        zo = Z_optimization.Z_optimizer(objective, [4, 6], model, Z_range=1.0, max_iters=iters, data=data, initial_Z=Z1, initial_LR=0.05,
                                        batch_size=batch, **(dict(kw, jpeg_extractor=inner.JPEG['extractor']) if jpeg else kw))
    finally:
        Z_optimization.esr_scribble.rebuilt_z_mask = real_mask
    Z = zo.optimize()
    return zo, Z, Z1


# ('hist' and the patch-histogram / dictionary names run on the soft-histogram and KDE kernels, which have no CPU expression:
# tests/test_gpu_jpeg_edit.py; here they only have to pass the JPEG gate)
EDIT_OBJECTIVES = ['local_STD_increase', 'local_min_STD', 'nonInt_periodicity', 'local_STD_nonInt_periodicityPlus', 'local_Mag_increase', 'scribble',
                   'random_l1', 'random_l1_limited']


@pytest.mark.parametrize('objective', EDIT_OBJECTIVES)
def test_editing_objectives_through_the_colour_model(tmp_path, objective):
    """JPEG mode is, by definition, the SR-mode objective on Output_Image_0_1(): the same search, value for value"""
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    zo, Z, Z0 = run_edit_search(poison_fake_H(make_model(tmp_path / 'a')), objective, jpeg=True)
    assert zo.jpeg_mode and Z.shape == Z0.shape and len(zo.loss_values) >= 1 and np.all(np.isfinite(zo.loss_values)) and bool(torch.isfinite(Z).all())
    sr, Z_sr, _ = run_edit_search(SRStandIn(make_model(tmp_path / 'b')), objective, jpeg=False)
    assert not sr.jpeg_mode
    print('%s: JPEG mode %s\n    SR mode on Output_Image_0_1() %s' % (objective, zo.loss_values, sr.loss_values))
    assert zo.loss_values[0] == pytest.approx(sr.loss_values[0], rel=1e-5, abs=1e-9)
    np.testing.assert_allclose(zo.loss_values, sr.loss_values, rtol=1e-4, atol=1e-9)
    assert float((Z - Z_sr).abs().max()) < 1e-4
    if objective in ('scribble', 'local_min_STD', 'random_l1'):
        assert len(zo.loss_values) == 6 and zo.loss_values[-1] < zo.loss_values[0]
    if objective != 'scribble':
        return
    # the region constraint: only Z entries the rebuilt block-grid mask allows have moved
    from esr_hip import scribble
    data, kw, _ = edit_case(objective)
    allowed = scribble.rebuilt_z_mask(kw['image_mask'], block_size=8)
    assert zo.non_local_Z_optimization and np.array_equal(zo.Z_mask, allowed) and 0 < allowed.sum() < allowed.size
    moved = (Z - Z0).abs().amax(dim=(0, 1)).numpy()
    assert moved[allowed == 0].max() < 1e-6 and moved[allowed == 1].min() > 1e-4


def test_y_model_and_other_refusals_stay(tmp_path):
    from esr_hip._lib import EsrError
    from Z_optimization import JPEG_EDIT_OBJECTIVES, Z_optimizer
    model = make_model(tmp_path)
    ext = model.JPEG['extractor']
    for objective in ('hist', 'patchdict_noDC'):                  # accepted: they get as far as their kernels
        with pytest.raises(EsrError, match='GPU'):
            run_edit_search(model, objective, jpeg=True)
    for objective in ('VGG', 'max_VGG', 'random_VGG', 'digit'):
        with pytest.raises(NotImplementedError):
            Z_optimizer(objective, [4, 6], model, Z_range=1.0, max_iters=1, data={}, initial_LR=0.1, jpeg_extractor=ext)
    with pytest.raises(NotImplementedError, match='JPEG mode'):
        Z_optimizer('scribble', [4, 6], model, Z_range=1.0, max_iters=1, data={}, initial_LR=0.1, jpeg_extractor=ext, HR_unpadder=lambda t: t)
    model.chroma_mode = False                                      # what the Y-only model answers
    for objective in JPEG_EDIT_OBJECTIVES:
        with pytest.raises(NotImplementedError, match='JPEG mode'):
            Z_optimizer(objective, [4, 6], model, Z_range=1.0, max_iters=1, data={}, initial_LR=0.1, jpeg_extractor=ext)
