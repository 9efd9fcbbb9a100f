"""CPU tests of esr_hip/metrics.py: its NumPy / torch float64 path (what CPU tensors and arrays take) against a float64 reference written here,
and answers that need no implementation at all.

The reference's own functions (codes/utils/util.py) import OpenCV and torchvision, which this build does not have, so `ref_scores` restates
them line by line: util.tensor2img :224-226 (clip, subtract, divide, times 255.0, .round() for uint8 — in float32, as NumPy computes on a float32
array), util.calculate_psnr :340-347, util.ssim :350-370 with cv2.getGaussianKernel(11, 1.5) and cv2.filter2D(...)[5:-5, 5:-5] written as
scipy.signal.correlate2d(., outer(g, g), 'valid') — the full 11 x 11 window, not a separable pass — and util.calculate_ssim :373-391 (ssim() of
the whole image: the mean over the channels).  tests/test_gpu_metrics.py compares the device path with the same functions.
"""
import math

import numpy as np
import pytest
import torch
from scipy.signal import correlate2d

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
TOL = 5e-7                 # PSNR (dB) and SSIM: half a unit of the last digit the reference prints ({:.6f}, codes/test.py:273)


def ref_pixels(x, min_max=(0, 1), quantize=False):
    """util.tensor2img :224-226 on a float32 array"""
    assert x.dtype == np.float32
    p = (np.clip(x, min_max[0], min_max[1]) - min_max[0]) / (min_max[1] - min_max[0])
    p = p * 255.0
    assert p.dtype == np.float32
    return p.round() if quantize else p


def ref_window():
    g = np.exp(-(np.arange(11) - 5.0) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    return np.outer(g, g)


def ref_psnr(img1, img2):
    mse = np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2)
    return float('inf') if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))


def ref_ssim(img1, img2):
    """util.ssim on [C, H, W] pixel arrays: the mean of the SSIM map over channels and valid windows"""
    img1, img2 = img1.astype(np.float64), img2.astype(np.float64)
    window = ref_window()
    maps = []
    for a, b in zip(img1, img2):
        f = lambda t: correlate2d(t, window, 'valid')          # noqa: E731
        mu1, mu2 = f(a), f(b)
        mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
        sigma1_sq, sigma2_sq, sigma12 = f(a ** 2) - mu1_sq, f(b ** 2) - mu2_sq, f(a * b) - mu1_mu2
        maps.append(((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2)))
    return float(np.mean(maps))


def ref_scores(a, b, min_max=(0, 1), quantize=False, border=0):
    """(psnr [B], ssim [B]) of float32 [B, C, H, W] arrays"""
    H, W = a.shape[2:]
    crop = lambda p: p[:, :, border:H - border, border:W - border]          # noqa: E731
    pa, pb = crop(ref_pixels(a, min_max, quantize)), crop(ref_pixels(b, min_max, quantize))
    return np.array([ref_psnr(x, y) for x, y in zip(pa, pb)]), np.array([ref_ssim(x, y) for x, y in zip(pa, pb)])


def make_pair(kind, shape, seed=0):
    """'noise': two independent images that leave [0, 1] on both sides; 'smooth': a ramp and the ramp plus small noise (where fp32 moments fail)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, C, H, W = shape
    if kind == 'noise':
        a, b = rng.uniform(-0.1, 1.1, shape), rng.uniform(-0.1, 1.1, shape)
    else:
        yy, xx = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing='ij')
        a = (0.1 + 0.5 * yy + 0.3 * xx)[None, None] + 0.05 * np.arange(B * C).reshape(B, C, 1, 1)
        b = a + rng.normal(0, 2e-3, shape)
    return a.astype(np.float32), b.astype(np.float32)


def tie_image(scaled):
    """[1, 1, 11, 257] float32 whose pixels k + 0.5, k = 0...254, are exact ties of the uint8 rounding, plus one value below and one above the
    range; and the squared error against zeros that half-to-even rounding gives, in integers.  scaled: values in (0, 255), else in (0, 1)."""
    k = np.arange(255)
    row = (k + 0.5).astype(np.float32) if scaled else ((k + 0.5) / 255).astype(np.float32)
    unit = 255.0 if scaled else 1.0
    row = np.concatenate([row, np.array([-0.2 * unit, 1.3 * unit], np.float32)])
    assert (ref_pixels(row[:255], (0, unit))[:255] == k + 0.5).all()           # every product is a tie in float32
    rounded = np.concatenate([k + (k & 1), [0, 255]])                           # half to even; the clamp
    return np.tile(row, (11, 1))[None, None], 11 * int((rounded.astype(np.int64) ** 2).sum())


CASES = [((2, 3, 23, 37), 0), ((1, 3, 83, 149), 0), ((1, 1, 11, 11), 0), ((1, 1, 11, 70), 0), ((1, 1, 70, 11), 0), ((2, 3, 40, 52), 4)]


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
@pytest.mark.parametrize('shape,border', CASES, ids=['x'.join(map(str, s)) + ('_crop%d' % c if c else '') for s, c in CASES])
def test_psnr_ssim_matches_the_restated_reference(shape, border, kind):
    from esr_hip import metrics
    a, b = make_pair(kind, shape)
    for out_type in (np.float32, np.uint8):
        want_p, want_s = ref_scores(a, b, quantize=out_type == np.uint8, border=border)
        p, s = metrics.psnr_ssim(torch.from_numpy(a), torch.from_numpy(b), out_type=out_type, crop_border=border)
        assert p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (shape[0],)
        assert np.abs(p.numpy() - want_p).max() <= TOL and np.abs(s.numpy() - want_s).max() <= TOL
    assert torch.equal(metrics.psnr(a, b, crop_border=border), metrics.psnr_ssim(a, b, crop_border=border)[0])       # arrays are accepted too
    assert torch.equal(metrics.ssim(a, b, crop_border=border), metrics.psnr_ssim(a, b, crop_border=border)[1])


def test_other_ranges_dtypes_and_strides():
    from esr_hip import metrics
    a, b = make_pair('noise', (2, 3, 23, 74))
    want = ref_scores(a[..., ::2] * 2 - 1, b[..., ::2] * 2 - 1, min_max=(-1, 1))
    ta, tb = torch.from_numpy(a * 2 - 1), torch.from_numpy(b * 2 - 1)
    got = metrics.psnr_ssim(ta[..., ::2].double(), tb[..., ::2], min_max=(-1, 1))          # a float64 input against a strided float32 one
    for g, w in zip(got, want):
        assert np.abs(g.numpy() - w).max() <= TOL
    one = metrics.psnr_ssim(ta[0, :, :, ::2], tb[0, :, :, ::2], min_max=(-1, 1))               # 3-D: one image
    assert one[0].shape == (1,) and abs(float(one[0]) - want[0][0]) <= TOL and abs(float(one[1]) - want[1][0]) <= TOL


@pytest.mark.parametrize('scaled', [False, True], ids=['unit_range', 'range_0_255'])
def test_uint8_conversion_rounds_ties_to_even_after_a_true_division(scaled):
    from esr_hip import metrics
    img, sse = tie_image(scaled)
    p = metrics.psnr(torch.from_numpy(img), torch.zeros(img.shape), min_max=(0, 255) if scaled else (0, 1), out_type=np.uint8)
    assert abs(float(p) - 20 * math.log10(255.0 / math.sqrt(sse / img.size))) <= TOL


def known_answer_inputs():
    """(a, b, kwargs, psnr, ssim) whose scores follow from the definitions alone (None: not determined)"""
    rng = np.random.Generator(np.random.PCG64(3))
    img = rng.uniform(0, 1, (1, 3, 17, 19)).astype(np.float32)
    k = rng.integers(0, 251, (1, 3, 17, 19))
    const = lambda c: np.full((1, 1, 13, 15), c / 255, np.float32)          # noqa: E731
    c1, c2 = 40, 200
    return [(img, img.copy(), {}, float('inf'), 1.0),
            ((k / 255).astype(np.float32), ((k + 3) / 255).astype(np.float32), {'out_type': np.uint8}, 20 * math.log10(255 / 3), None),
            (const(c1), const(c2), {'out_type': np.uint8}, 20 * math.log10(255 / (c2 - c1)), (2 * c1 * c2 + C1) / (c1 ** 2 + c2 ** 2 + C1))]


@pytest.mark.parametrize('case', range(3), ids=['identical', 'offset', 'constant'])
def test_known_answers(case):
    from esr_hip import metrics
    a, b, kw, psnr, ssim = known_answer_inputs()[case]
    p, s = metrics.psnr_ssim(torch.from_numpy(a), torch.from_numpy(b), **kw)
    assert float(p) == psnr if math.isinf(psnr) else abs(float(p) - psnr) <= 1e-9
    if ssim is not None:
        assert abs(float(s) - ssim) <= 1e-12


def test_reference_signatures_on_image_arrays():
    """calculate_psnr / calculate_ssim on HWC and HW arrays in [0, 255], as codes/test.py:237-240 calls them, and on CHW tensors"""
    from esr_hip import metrics
    a, b = make_pair('noise', (1, 3, 23, 37))
    pa, pb = ref_pixels(a)[0], ref_pixels(b)[0]                                      # CHW, 0...255
    hwc = lambda p: np.ascontiguousarray(p.transpose(1, 2, 0)[:, :, ::-1])           # noqa: E731  (BGR, as tensor2img returns)
    psnr, ssim = metrics.calculate_psnr(hwc(pa), hwc(pb)), metrics.calculate_ssim(hwc(pa), hwc(pb))
    assert isinstance(psnr, float) and isinstance(ssim, float)
    assert abs(psnr - ref_psnr(pa, pb)) <= 1e-9 and abs(ssim - ref_ssim(pa, pb)) <= TOL
    assert abs(metrics.calculate_ssim(pa[0], pb[0]) - ref_ssim(pa[:1], pb[:1])) <= TOL             # HW
    assert abs(metrics.calculate_ssim(hwc(pa)[:, :, :1], hwc(pb)[:, :, :1]) - ref_ssim(pa[2:], pb[2:])) <= TOL    # HW1
    assert abs(metrics.calculate_ssim(torch.from_numpy(pa), torch.from_numpy(pb)) - ref_ssim(pa, pb)) <= TOL      # CHW tensors
    assert metrics.calculate_psnr(hwc(pa), hwc(pa)) == float('inf')
    # the test.py call pattern: tensor2img -> * 255 -> calculate_*
    sr, gt = (metrics.tensor2img(torch.from_numpy(t[0]), out_type=np.float32) * 255. for t in (a, b))
    assert abs(metrics.calculate_psnr(sr, gt) - ref_psnr(pa, pb)) <= TOL and abs(metrics.calculate_ssim(sr, gt) - ref_ssim(pa, pb)) <= TOL


def test_tensor2img():
    from esr_hip import metrics
    rng = np.random.Generator(np.random.PCG64(5))
    t = rng.uniform(-0.4, 1.4, (3, 5, 7)).astype(np.float32)
    assert (t < 0).any() and (t > 1).any()
    img = metrics.tensor2img(torch.from_numpy(t))
    assert img.dtype == np.uint8 and img.shape == (5, 7, 3)
    for c in range(3):                                                               # BGR: channel c of the image is channel 2 - c of the tensor
        assert (img[:, :, c] == (np.clip(t[2 - c], 0, 1) * 255.0).round().astype(np.uint8)).all()
    assert img.min() == 0 and img.max() == 255
    f = metrics.tensor2img(torch.from_numpy(t), out_type=np.float32, min_max=(-1, 1))
    assert f.dtype == np.float32 and np.array_equal(f[:, :, 0], (np.clip(t[2], -1, 1) + 1) / 2)
    g = metrics.tensor2img(torch.from_numpy(t[:1]))                                  # squeezed to 2-D
    assert g.shape == (5, 7) and g.dtype == np.uint8
    with pytest.raises(NotImplementedError):
        metrics.tensor2img(torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        metrics.tensor2img(torch.zeros(3, 4, 4), chroma_mode='YCbCr')
    with pytest.raises(TypeError):
        metrics.tensor2img(torch.zeros(4))


def test_refusals():
    from esr_hip import metrics
    z = np.zeros
    with pytest.raises(ValueError, match='same dimensions'):
        metrics.calculate_ssim(z((12, 12, 3)), z((12, 13, 3)))
    with pytest.raises(ValueError, match='same dimensions'):
        metrics.calculate_psnr(z((12, 12, 3)), z((12, 13, 3)))
    with pytest.raises(ValueError, match='Wrong input image dimensions'):
        metrics.calculate_ssim(z((1, 12, 12, 3)), z((1, 12, 12, 3)))
    with pytest.raises(ValueError, match='Wrong input image dimensions'):
        metrics.calculate_ssim(z((12, 12, 2)), z((12, 12, 2)))
    with pytest.raises(ValueError, match='11'):
        metrics.calculate_ssim(z((10, 40, 3)), z((10, 40, 3)))
    with pytest.raises(ValueError, match='11'):
        metrics.psnr_ssim(torch.zeros(1, 3, 18, 40), torch.zeros(1, 3, 18, 40), crop_border=4)
    with pytest.raises(ValueError, match='same dimensions'):
        metrics.psnr_ssim(torch.zeros(1, 3, 18, 40), torch.zeros(1, 3, 18, 41))
    with pytest.raises(ValueError):
        metrics.psnr_ssim(torch.zeros(1, 2, 18, 40), torch.zeros(1, 2, 18, 40))
    with pytest.raises(ValueError):
        metrics.psnr_ssim(torch.zeros(1, 3, 18, 40), torch.zeros(1, 3, 18, 40), out_type=np.float64)
    with pytest.raises(ValueError):
        metrics.sample_std(torch.zeros(2, 3, 8, 8))
    assert float(metrics.psnr(torch.zeros(1, 3, 4, 5), torch.ones(1, 3, 4, 5))) == 0.0       # PSNR alone needs no window


def sample_stack():
    """[7, 2, 3, 9, 13] float32 from -0.3 to 1.3"""
    return np.random.Generator(np.random.PCG64(11)).uniform(-0.3, 1.3, (7, 2, 3, 9, 13)).astype(np.float32)


def ref_sample_std(x):
    """255 np.std over the samples (codes/test.py:229) of the clamped images in float64, and its mean per image (:230)"""
    sd = 255 * np.std(np.clip(x, 0, 1).astype(np.float64), axis=0)
    return sd, sd.reshape(sd.shape[0], -1).mean(1)


@pytest.mark.parametrize('S', [1, 2, 7])
def test_sample_std(S):
    from esr_hip import metrics
    x = sample_stack()[:S]
    want_map, want_mean = ref_sample_std(x)
    got_map, got_mean = metrics.sample_std(torch.from_numpy(x))
    assert got_map.dtype == torch.float32 and got_map.shape == (2, 3, 9, 13) and got_mean.dtype == torch.float64 and got_mean.shape == (2,)
    assert np.abs(got_map.numpy() - want_map).max() <= 1e-5
    assert (np.abs(got_mean.numpy() - want_mean) <= 1e-9 * np.abs(want_mean)).all()
    if S == 1:
        assert not got_map.any() and not got_mean.any()


def test_cabi_refusals_without_a_gpu():
    """esr_psnr_ssim / esr_sample_std and their size queries check their arguments on the host (fake pointers, never dereferenced)"""
    from esr_hip import _lib
    h = _lib.load_library()
    E_ARG, E_UNSUPPORTED = -1, -2
    assert h.esr_psnr_ssim_partials(3, 83, 149, 0) == 3 * 4 * 5 and h.esr_psnr_ssim_partials(1, 40, 52, 4) == 2 * 2       # 21 x 32 tiles
    assert h.esr_psnr_ssim_partials(2, 40, 52, 0) == E_ARG and h.esr_psnr_ssim_partials(3, 8, 8, 4) == E_ARG
    assert h.esr_psnr_ssim(None, 16, 1, 3, 16, 16, 0.0, 1.0, 0, 0, 16, 16, None) == E_ARG
    assert h.esr_psnr_ssim(16, 16, 1, 3, 16, 16, 1.0, 1.0, 0, 0, 16, 16, None) == E_ARG              # hi == lo
    assert h.esr_psnr_ssim(16, 16, 1, 3, 16, 16, 0.0, 1.0, 3, 0, 16, 16, None) == E_ARG              # no such pixel mode
    assert h.esr_psnr_ssim(16, 16, 30000, 3, 16, 16, 0.0, 1.0, 0, 0, 16, 16, None) == E_UNSUPPORTED
    assert h.esr_sample_std_partials(3, 9, 13) == 1 and h.esr_sample_std_partials(3, 512, 512) == 768
    assert h.esr_sample_std(16, 0, 1, 3, 8, 8, 16, 16, 16, None) == E_ARG
    assert h.esr_sample_std(16, 2, 70000, 3, 8, 8, 16, 16, 16, None) == E_UNSUPPORTED
