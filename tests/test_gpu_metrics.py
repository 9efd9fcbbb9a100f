"""esr_psnr_ssim and esr_sample_std (csrc/esr_metrics.hip) through esr_hip/metrics.py on the GPU, against the float64 restatement of the
reference written in tests/test_host_metrics.py (scipy's full 11 x 11 correlation, not a separable pass).

Tolerances: PSNR (dB) and SSIM 5e-7 absolute — half a unit of the last digit the reference prints ({:.6f}, codes/test.py:273); the STD map 1e-5
absolute in 0...255 units (a population STD of values in [0, 255] is at most 127.5, where one fp32 ulp is 7.6e-6); its mean 1e-9 relative.
"""
import math

import numpy as np
import pytest
import torch

from test_host_metrics import (CASES, TOL, known_answer_inputs, make_pair, ref_sample_std, ref_scores, sample_stack, tie_image)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(got, want, what):
    got = [g.cpu().numpy() for g in got]
    err = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
    print('%s: |PSNR - ref| %.3e dB, |SSIM - ref| %.3e' % (what, err[0], err[1]))
    assert err[0] <= TOL and err[1] <= TOL, (what, err)


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
@pytest.mark.parametrize('shape,border', CASES, ids=['x'.join(map(str, s)) + ('_crop%d' % c if c else '') for s, c in CASES])
def test_psnr_ssim_matches_the_restated_reference(shape, border, kind):
    """one tile and less (11 x 11: exactly one window), strips, several 21 x 32 tiles with ragged edges in both directions, a crop"""
    from esr_hip import metrics
    a, b = make_pair(kind, shape)
    for out_type in (np.float32, np.uint8):
        p, s = metrics.psnr_ssim(_gpu(a), _gpu(b), out_type=out_type, crop_border=border)
        assert p.is_cuda and p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (shape[0],)
        _close((p, s), ref_scores(a, b, quantize=out_type == np.uint8, border=border), '%s %s %s' % (shape, kind, out_type.__name__))


def test_strided_and_float64_inputs():
    from esr_hip import metrics
    a, b = make_pair('noise', (2, 3, 23, 74))
    want = ref_scores(a[..., ::2] * 2 - 1, b[..., ::2] * 2 - 1, min_max=(-1, 1))
    ta, tb = _gpu(a * 2 - 1), _gpu(b * 2 - 1)
    _close(metrics.psnr_ssim(ta[..., ::2].double(), tb[..., ::2], min_max=(-1, 1)), want, 'a float64 input against a non-contiguous slice')
    one = metrics.psnr_ssim(ta[1, :, :, ::2], tb[1, :, :, ::2], min_max=(-1, 1))                  # 3-D: one image
    assert one[0].shape == (1,)
    _close(one, [w[1:] for w in want], 'one 3-D image')
    assert torch.equal(metrics.psnr(ta, tb, min_max=(-1, 1)), metrics.psnr_ssim(ta, tb, min_max=(-1, 1))[0])
    assert torch.equal(metrics.ssim(ta, tb, min_max=(-1, 1)), metrics.psnr_ssim(ta, tb, min_max=(-1, 1))[1])


@pytest.mark.parametrize('scaled', [False, True], ids=['unit_range', 'range_0_255'])
def test_uint8_conversion_rounds_ties_to_even_after_a_true_division(scaled):
    """every pixel k + 0.5 is an exact tie: rounding half up moves 128 of them, a multiplication by 1 / (hi - lo) moves others off the tie in the
    second range — either changes the integer squared error.  The values at -0.2 and 1.3 of the range check the clamp."""
    from esr_hip import metrics
    img, sse = tie_image(scaled)
    x = _gpu(img)
    p = metrics.psnr(x, torch.zeros_like(x), min_max=(0, 255) if scaled else (0, 1), out_type=np.uint8)
    want = 20 * math.log10(255.0 / math.sqrt(sse / img.size))
    print('PSNR %.9f, from the integer squared error %.9f' % (float(p), want))
    assert abs(float(p) - want) <= TOL


@pytest.mark.parametrize('case', range(3), ids=['identical', 'offset', 'constant'])
def test_known_answers(case):
    from esr_hip import metrics
    a, b, kw, psnr, ssim = known_answer_inputs()[case]
    p, s = metrics.psnr_ssim(_gpu(a), _gpu(b), **kw)
    print('PSNR %r (%r), SSIM %r (%r)' % (float(p), psnr, float(s), ssim))
    assert float(p) == psnr if math.isinf(psnr) else abs(float(p) - psnr) <= TOL
    if ssim is not None:
        assert abs(float(s) - ssim) <= (1e-12 if case == 0 else TOL)


def test_reference_signatures_take_device_tensors():
    """calculate_psnr / calculate_ssim on CHW tensors that hold 0...255 pixels already: nothing is converted or clamped"""
    from esr_hip import metrics
    from test_host_metrics import ref_psnr, ref_ssim
    a, b = make_pair('noise', (1, 3, 23, 37))
    pa, pb = a[0] * 300 - 20, b[0] * 300 - 20                                              # leaves [0, 255] on both sides
    psnr, ssim = metrics.calculate_psnr(_gpu(pa), _gpu(pb)), metrics.calculate_ssim(_gpu(pa), _gpu(pb))
    assert isinstance(psnr, float) and isinstance(ssim, float)
    assert abs(psnr - ref_psnr(pa, pb)) <= TOL and abs(ssim - ref_ssim(pa, pb)) <= TOL
    with pytest.raises(ValueError, match='11'):
        metrics.calculate_ssim(_gpu(pa[:, :10]), _gpu(pb[:, :10]))


def test_two_calls_give_the_same_bits():
    from esr_hip import metrics
    a, b = make_pair('noise', (2, 3, 83, 149), seed=4)
    ta, tb = _gpu(a), _gpu(b)
    first, second = metrics.psnr_ssim(ta, tb), metrics.psnr_ssim(ta, tb)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    x = _gpu(sample_stack())
    m1, m2 = metrics.sample_std(x), metrics.sample_std(x)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])


@pytest.mark.parametrize('S', [1, 2, 7])
def test_sample_std(S):
    from esr_hip import metrics
    x = sample_stack()[:S]
    want_map, want_mean = ref_sample_std(x)
    got_map, got_mean = metrics.sample_std(_gpu(x))
    assert got_map.is_cuda and got_map.dtype == torch.float32 and got_map.shape == (2, 3, 9, 13)
    assert got_mean.is_cuda and got_mean.dtype == torch.float64 and got_mean.shape == (2,)
    err_map = float(np.abs(got_map.cpu().numpy() - want_map).max())
    err_mean = float((np.abs(got_mean.cpu().numpy() - want_mean) / np.maximum(np.abs(want_mean), 1e-300)).max())
    print('S = %d: map error %.3e (0...255 units), relative error of the mean %.3e' % (S, err_map, err_mean))
    assert err_map <= 1e-5 and err_mean <= 1e-9
    if S == 1:
        assert not got_map.any() and not got_mean.any()


def test_sample_std_over_several_workgroups():
    """more pixels per image than one workgroup takes (1024), a ragged last one, a non-contiguous float64 input"""
    from esr_hip import metrics
    x = np.random.Generator(np.random.PCG64(12)).uniform(-0.3, 1.3, (3, 2, 3, 21, 66)).astype(np.float32)
    want_map, want_mean = ref_sample_std(x[..., ::2])
    got_map, got_mean = metrics.sample_std(_gpu(x).double()[..., ::2])
    assert float(np.abs(got_map.cpu().numpy() - want_map).max()) <= 1e-5
    assert (np.abs(got_mean.cpu().numpy() - want_mean) <= 1e-9 * np.abs(want_mean)).all()


def test_current_metrics_of_the_model():
    from esr_hip import metrics
    from oracle.weights import seeded_uniform
    from test_gpu_model import _model
    m = _model(nb=1, lat=0, is_train=False)
    m.feed_data({'LR': seeded_uniform((2, 3, 16, 16), 31), 'HR': seeded_uniform((2, 3, 64, 64), 32)})
    m.test()
    got = m.current_metrics()
    vis = m.get_current_visuals(entire_batch=True, to_cpu=False)
    want = metrics.psnr_ssim(vis['SR'], vis['HR'])
    assert set(got) == {'psnr', 'ssim'} and got['psnr'].is_cuda and got['psnr'].shape == (2,)
    assert torch.equal(got['psnr'], want[0]) and torch.equal(got['ssim'], want[1])
    assert torch.isfinite(got['psnr']).all() and torch.isfinite(got['ssim']).all()
    host = ref_scores(vis['SR'].cpu().numpy(), vis['HR'].cpu().numpy())
    _close((got['psnr'], got['ssim']), host, 'current_metrics')
    cropped = m.current_metrics(crop_border=2, out_type=np.uint8)
    _close((cropped['psnr'], cropped['ssim']), ref_scores(vis['SR'].cpu().numpy(), vis['HR'].cpu().numpy(), quantize=True, border=2), 'current_metrics, cropped uint8')
