"""esr_ycbcr_image, esr_psnr_ssim_ycbcr and esr_sample_std_ycbcr (csrc/esr_metrics.hip) through esr_hip/jpeg_metrics.py on the GPU, against the
host route of the same module — which tests/test_host_jpeg_eval.py pins to the reference's own pictures.

The device chain is fp32 / fp64 in a stated order without fused multiply-adds; NumPy's 3-term matmul may order or fuse differently by one fp64
ulp, which can flip a rounded pixel only where the value before rounding lies within about 1e-5 of a half-integer.  So:
  * on TIE-FREE inputs (every host pre-rounding value at least TIE_BAND = 1e-3 from a half-integer, offending pixels re-drawn) the pictures are
    equal bit for bit and the scores agree to the tolerances of tests/test_gpu_metrics.py: PSNR (dB) and SSIM 5e-7 absolute — half a unit of
    the last digit the reference prints; the STD map 1e-5 absolute (at most 127.5, where one fp32 ulp is 7.6e-6); its mean 1e-9 relative;
  * on unrestricted inputs every differing pixel differs by exactly one level and is a near-tie on the host, and such pixels are capped at
    0.5 % of the image: an indexing or channel error cannot hide under that;
  * model outputs are not tie-free: there the scores are bounded by what the k pixels could change in which the device's picture differs from
    the host's (flip_bounds; each checked to be a near-tie moved by one level), after asserting k is within the cap.
crop_border 4 is scored where 11 pixels are left for an SSIM window (23 x 45 and 48 x 80); on 11 x 11 and 16 x 16 it is the ValueError of both routes.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_host_jpeg_eval import (EVAL_KEYS, MODES, decoder_like, eval_loader, host_evaluate, host_scores, host_std, latent_samples, near_tie,
                                 ref_pre_round, tie_free)
from test_host_metrics import TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 0.005                # the largest share of an image's pixels that may differ (by one level, at near-ties)
SHAPES = [(11, 11), (16, 16), (23, 45), (48, 80)]        # one window; less than a tile; strips and part-filled 21 x 32 tiles, more than two each way


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)                   # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def pair(mode, H, W, min_max=(0, 255)):
    """(a [3, C, H, W], gt [3, C, H, W]) tie-free: decoder-like ground truths and the same plus noise of a few levels"""
    gt = tie_free(decoder_like((3, H, W), mode, 31 + H), mode, min_max, seed=H)
    noisy = gt + np.random.Generator(np.random.PCG64(32 + W)).normal(0, 4.0, gt.shape).astype(np.float32)
    a = tie_free(noisy, mode, min_max, seed=W)
    a.setflags(write=False)
    gt.setflags(write=False)
    return a, gt


def _host_images(x, mode, min_max=(0, 255)):
    from esr_hip import jpeg_metrics
    return np.stack(jpeg_metrics.image(torch.from_numpy(np.array(x)), mode, min_max=min_max))


# ------------------------------------------------------------------------------------------------ pictures
@pytest.mark.parametrize('min_max', [(0, 255), (16, 235)], ids=['0_255', '16_235'])
@pytest.mark.parametrize('W', [56, 45], ids=['four_pixels_per_thread', 'one_pixel_per_thread'])
@pytest.mark.parametrize('mode', list(MODES))
def test_pictures_equal_the_host_route_bit_for_bit_on_tie_free_inputs(mode, W, min_max):
    from esr_hip import jpeg_metrics
    a, _ = pair(mode, 48, W, min_max)
    want = _host_images(a, mode, min_max)
    got = jpeg_metrics.image(_gpu(a), mode, min_max=min_max)
    assert isinstance(got, list) and len(got) == 3 and got[0].dtype == np.uint8 and got[0].shape == (48, W, 3)
    assert np.array_equal(np.stack(got), want)
    assert (want == 0).any() and (want == 255).any()                                       # both sides of the clip
    one = jpeg_metrics.image(_gpu(a[1] if mode == 'YCbCr' else a[1, 0]), mode, min_max=min_max)              # [3, H, W] / [H, W]: one array
    assert isinstance(one, np.ndarray) and np.array_equal(one, want[1])
    if W % 4 == 0:
        # the same planes 4 bytes off a 16-byte boundary take the one-pixel kernel: the same bits
        flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        shifted = flat[1:].view(a.shape)
        shifted.copy_(_gpu(a))
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        assert np.array_equal(np.stack(jpeg_metrics.image(shifted, mode, min_max=min_max)), want)
    f32 = jpeg_metrics.image(_gpu(a[0]), mode, out_type=np.float32, min_max=min_max)     # other types: the host expression
    assert f32.dtype == np.float32 and np.array_equal(f32, jpeg_metrics.image(torch.from_numpy(np.array(a[0])), mode, out_type=np.float32, min_max=min_max))


@pytest.mark.parametrize('kind', ['decoder_like', 'uniform'])
@pytest.mark.parametrize('mode', list(MODES))
def test_pictures_of_unrestricted_inputs_differ_only_at_near_ties_by_one_level(mode, kind):
    from esr_hip import jpeg_metrics
    if kind == 'uniform':
        x = np.random.Generator(np.random.PCG64(41)).uniform(-20, 275, (2, MODES[mode], 48, 56)).astype(np.float32)
    else:
        x = decoder_like((2, 48, 56), mode, 42)
    want = _host_images(x, mode).astype(np.int32)
    got = np.stack(jpeg_metrics.image(_gpu(x), mode)).astype(np.int32)
    ties = np.stack([near_tie(ref_pre_round(im if mode == 'YCbCr' else im[0], mode)) for im in x])
    differ = (got != want).any(-1)
    print('%s %s: %d of %d pixels differ, %d are near-ties on the host (%.3f %%)' % (mode, kind, differ.sum(), differ.size, ties.sum(), 100 * ties.mean()))
    assert differ.mean() <= CAP
    assert np.abs(got - want).max() <= 1
    assert not (differ & ~ties).any()


# ------------------------------------------------------------------------------------------------ scores
def _close(got, want, what):
    got = [g.cpu().numpy() for g in got]
    err = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
    print('%s: |PSNR - host| %.3e dB, |SSIM - host| %.3e' % (what, err[0], err[1]))
    assert err[0] <= TOL and err[1] <= TOL, (what, err)


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize('mode', list(MODES))
def test_scores_match_the_host_route_on_tie_free_inputs(mode, shape):
    from esr_hip import jpeg_metrics
    a, gt = pair(mode, *shape)
    ta, tg = _gpu(a), _gpu(gt)
    for border in (0, 4):
        if min(shape) - 2 * border < 11:
            with pytest.raises(ValueError, match='11'):
                jpeg_metrics.psnr_ssim(ta, tg, mode, crop_border=border)
            with pytest.raises(ValueError, match='11'):
                jpeg_metrics.psnr_ssim(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(gt)), mode, crop_border=border)
            continue
        p, s = jpeg_metrics.psnr_ssim(ta, tg, mode, crop_border=border)
        assert p.is_cuda and p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (3,)
        _close((p, s), host_scores(a, gt, mode, border), '%s %s border %d, three pairs' % (mode, shape, border))
        _close(jpeg_metrics.psnr_ssim(ta, tg[1:2], mode, crop_border=border), host_scores(a, gt[1:2], mode, border),
               '%s %s border %d, three images against one' % (mode, shape, border))
    p, s = jpeg_metrics.psnr_ssim(tg, tg.clone(), mode)
    assert torch.isinf(p).all() and (p > 0).all() and float((s - 1).abs().max()) <= 1e-12
    one = jpeg_metrics.psnr_ssim(ta[2], tg[2], mode)                                       # single images
    _close(one, [w[2:] for w in host_scores(a, gt, mode)], 'one image')


def test_other_range_dtype_and_strides():
    from esr_hip import jpeg_metrics
    a, gt = pair('YCbCr', 48, 56, (16, 235))
    want = host_scores(a[..., ::2], gt[..., ::2], 'YCbCr', 0, (16, 235))
    _close(jpeg_metrics.psnr_ssim(_gpu(a).double()[..., ::2], _gpu(gt)[..., ::2], 'YCbCr', min_max=(16, 235)), want, 'a float64 input against a slice')


def _std_close(x, mode):
    from esr_hip import jpeg_metrics
    want_map, want_mean = host_std(x, mode)
    got_map, got_mean = jpeg_metrics.sample_std(_gpu(x), mode)
    S, B, _, H, W = x.shape
    assert got_map.is_cuda and got_map.dtype == torch.float32 and got_map.shape == (B, 3, H, W)
    assert got_mean.is_cuda and got_mean.dtype == torch.float64 and got_mean.shape == (B,)
    err_map = float(np.abs(got_map.cpu().numpy() - want_map).max())
    err_mean = float((np.abs(got_mean.cpu().numpy() - want_mean) / np.maximum(np.abs(want_mean), 1e-300)).max())
    print('%s S = %d, %d x %d: map error %.3e (0...255 units), relative error of the mean %.3e' % (mode, S, H, W, err_map, err_mean))
    assert err_map <= 1e-5 and err_mean <= 1e-9
    return got_map, got_mean


@functools.lru_cache(maxsize=None)
def samples(mode, H, W):
    """[5, 2, C, H, W] tie-free: five noisy versions of two images"""
    base = decoder_like((2, H, W), mode, 51)
    x = base[None] + np.random.Generator(np.random.PCG64(52)).normal(0, 5.0, (5,) + base.shape).astype(np.float32)
    x = tie_free(x.reshape((10,) + base.shape[1:]), mode, seed=53).reshape(x.shape)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('S', [1, 2, 5])
@pytest.mark.parametrize('mode', list(MODES))
def test_sample_std(mode, S):
    got_map, got_mean = _std_close(np.array(samples(mode, 13, 18)[:S]), mode)
    if S == 1:
        assert not got_map.any() and not got_mean.any()
    else:
        assert float(got_mean.min()) > 1


@pytest.mark.parametrize('mode', list(MODES))
def test_sample_std_over_several_workgroups(mode):
    """more pixels per image than one workgroup takes (1024) and a ragged last one"""
    _std_close(np.array(samples(mode, 21, 66)[:3]), mode)


def test_two_calls_give_the_same_bits():
    from esr_hip import jpeg_metrics
    a, gt = pair('YCbCr', 48, 80)
    ta, tg = _gpu(a), _gpu(gt)
    first, second = jpeg_metrics.psnr_ssim(ta, tg, 'YCbCr'), jpeg_metrics.psnr_ssim(ta, tg, 'YCbCr')
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    x = _gpu(np.array(samples('YCbCr', 21, 66)))
    m1, m2 = jpeg_metrics.sample_std(x, 'YCbCr'), jpeg_metrics.sample_std(x, 'YCbCr')
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    assert np.array_equal(np.stack(jpeg_metrics.image(ta, 'YCbCr')), np.stack(jpeg_metrics.image(ta, 'YCbCr')))


def test_error_returns_are_negative_and_write_nothing():
    from esr_hip import _lib
    from esr_hip.act import stream_ptr
    h = _lib.lib
    x = torch.full((2, 2, 3, 16, 16), 100.0, device=DEV)                                    # [S, B, C, H, W], or two batches of two
    picture = torch.full((2, 16, 16, 3), 77, dtype=torch.uint8, device=DEV)
    partial = torch.full((2, 3, 2), -7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((2, 2), -7.0, dtype=torch.float64, device=DEV)
    std_map = torch.full((2, 3, 16, 16), -7.0, device=DEV)
    p = lambda t: t.data_ptr()              # noqa: E731
    ok = dict(x=p(x), B=2, C=3, H=16, W=16, lo=0.0, hi=255.0, out=p(picture))
    image_bad = dict(null_input=dict(x=None), null_output=dict(out=None), two_planes=dict(C=2), no_planes=dict(C=0), empty_batch=dict(B=0), no_rows=dict(H=0),
                     no_columns=dict(W=-1), empty_range=dict(hi=0.0), reversed_range=dict(lo=255.0, hi=0.0), nan_range=dict(lo=float('nan')),
                     batch_above_the_grid=dict(B=70000))
    for name, kw in image_bad.items():
        a = dict(ok, **kw)
        rc = h.esr_ycbcr_image(a['x'], a['B'], a['C'], a['H'], a['W'], a['lo'], a['hi'], a['out'], stream_ptr())
        assert rc < 0, (name, rc)
    ok = dict(a=p(x), b=p(x[1]), B=2, C=3, H=16, W=16, stride=768, lo=0.0, hi=255.0, border=0, partial=p(partial), sums=p(sums))
    score_bad = dict(null_a=dict(a=None), null_b=dict(b=None), null_partial=dict(partial=None), null_sums=dict(sums=None), two_planes=dict(C=2), empty_batch=dict(B=0),
                     no_rows=dict(H=0), no_columns=dict(W=0), stride_of_one_plane=dict(stride=256), negative_stride=dict(stride=-768), empty_range=dict(hi=0.0),
                     border_leaves_nothing=dict(border=8), negative_border=dict(border=-1), batch_above_the_grid=dict(B=30000))
    for name, kw in score_bad.items():
        a = dict(ok, **kw)
        rc = h.esr_psnr_ssim_ycbcr(a['a'], a['b'], a['B'], a['C'], a['H'], a['W'], C.c_int64(a['stride']), a['lo'], a['hi'], a['border'], a['partial'], a['sums'],
                                   stream_ptr())
        assert rc < 0, (name, rc)
    assert h.esr_psnr_ssim_ycbcr_partials(2, 16, 16, 0) < 0 and h.esr_psnr_ssim_ycbcr_partials(3, 16, 16, 8) < 0
    ok = dict(x=p(x), S=2, B=2, C=3, H=16, W=16, lo=0.0, hi=255.0, map=p(std_map), partial=p(partial), sums=p(sums))
    std_bad = dict(null_x=dict(x=None), null_map=dict(map=None), null_partial=dict(partial=None), null_sums=dict(sums=None), no_samples=dict(S=0), empty_batch=dict(B=0),
                   four_planes=dict(C=4), no_rows=dict(H=0), no_columns=dict(W=0), empty_range=dict(lo=255.0), batch_above_the_grid=dict(B=70000))
    for name, kw in std_bad.items():
        a = dict(ok, **kw)
        rc = h.esr_sample_std_ycbcr(a['x'], a['S'], a['B'], a['C'], a['H'], a['W'], a['lo'], a['hi'], a['map'], a['partial'], a['sums'], stream_ptr())
        assert rc < 0, (name, rc)
    assert h.esr_sample_std_ycbcr_partials(2, 16, 16) < 0 and h.esr_sample_std_ycbcr_partials(3, 0, 16) < 0
    torch.cuda.synchronize()
    assert bool((picture == 77).all()) and bool((partial == -7.0).all()) and bool((sums == -7.0).all()) and bool((std_map == -7.0).all())


# ------------------------------------------------------------------------------------------------ evaluate and current_metrics
def flip_bounds(k, pixels, psnr, windows):
    """What k differing pixels of a picture (3 k channel values, each able to move by one level) can change.
    PSNR: a value that moves by one level changes its squared error d^2 by |2 d +- 1| <= 511, so the squared error SSE = 3 pixels 255^2 10^(-PSNR / 10)
    moves by at most D = 1533 k, and PSNR by at most 10 log10(SSE / (SSE - D)).  SSIM: a pixel lies in at most 121 windows of its channel, and one
    window's SSIM lies in [-1, 1]: at most 2 * 121 * 3 k of the 3 * windows terms' sum."""
    if k == 0:
        return TOL, TOL
    sse, d = 3 * pixels * 255.0 ** 2 * 10 ** (-psnr / 10), 1533.0 * k
    assert sse > 2 * d, 'the bound needs a squared error well above what the flips can move'
    return TOL + 10 * np.log10(sse / (sse - d)), TOL + 2.0 * 121 * k / windows


@pytest.mark.parametrize('chroma', [False, True], ids=['Y', 'colour'])
def test_evaluate_and_current_metrics_match_the_host_loop(tmp_path, chroma):
    """a formula-weighted model over the 3 colour images of the fixture, S = 3 latent samples, crop_border 2.  The host loop copies every decoded
    sample as fp32 (get_current_visuals) and converts it in NumPy.  A model's output is not tie-free: k counts the pixels of a sample whose device
    picture differs from the host's (host_evaluate checks each is a near-tie moved by one level); it is held to the cap before the bounds of
    flip_bounds are used (with k = 0 they are the tolerances above)."""
    from esr_hip import jpeg_metrics
    if chroma:
        from test_host_jpeg_chroma import make_model
    else:
        from test_host_jpeg import make_model
    model = make_model(tmp_path, gpu=True)
    loader, Z, border = eval_loader(tmp_path / 'images', chroma), latent_samples(3), 2
    got = jpeg_metrics.evaluate(model, loader, Z=Z, crop_border=border)
    want = host_evaluate(model, loader, Z, border=border)
    assert got['psnr'].shape == got['ssim'].shape == (3, 3) and got['pixel_std'].shape == (3,)
    total_k = 0
    for n in range(3):
        pixels = int(want['pixels'][n])
        H_W = [tuple(item['Uncomp'].shape[-2:]) for item in loader][n]
        windows = (H_W[0] - 2 * border - 10) * (H_W[1] - 2 * border - 10)
        for s in range(3):
            k = int(want['flips'][n][s])
            assert k <= CAP * pixels, (n, s, k, pixels)
            bound_psnr, bound_ssim = flip_bounds(k, pixels, want['psnr'][n, s], windows)
            err = abs(got['psnr'][n, s] - want['psnr'][n, s]), abs(got['ssim'][n, s] - want['ssim'][n, s])
            print('image %d sample %d: %d of %d pixels differ, |PSNR - host| %.3e (bound %.3e), |SSIM - host| %.3e (bound %.3e)' % (
                n, s, k, pixels, err[0], bound_psnr, err[1], bound_ssim))
            assert err[0] <= bound_psnr and err[1] <= bound_ssim
        # the STD map covers the whole picture: one level in one sample moves a pixel's STD by at most 1 / sqrt(S) <= 1
        k_full, full = int(sum(want['flips_full'][n])), int(want['pixels_full'][n])
        assert k_full <= CAP * 3 * full
        assert abs(got['pixel_std'][n] - want['pixel_std'][n]) <= 1e-9 * want['pixel_std'][n] + k_full / full
        total_k += k_full
        # the plainly decompressed image: the JPEG modules' output, not tie-free either
        k = int(want['flips_quantized'][n])
        assert k <= CAP * pixels
        bound_psnr, bound_ssim = flip_bounds(k, pixels, want['psnr_quantized'][n], windows)
        assert abs(got['psnr_quantized'][n] - want['psnr_quantized'][n]) <= bound_psnr
        assert abs(got['ssim_quantized'][n] - want['ssim_quantized'][n]) <= bound_ssim
    every = float(sum(want['pixels_full']))
    assert abs(got['mean_pixel_std'] - want['mean_pixel_std']) <= 1e-5 + total_k / every
    assert abs(got['std_of_image_mean_std'] - want['std_of_image_mean_std']) <= 1e-5 + total_k / every * 3
    assert abs(got['std_of_pixel_std'] - want['std_of_pixel_std']) <= 1e-5 + np.sqrt(total_k / every)
    assert set(EVAL_KEYS) <= set(got)
    # current_metrics: the last test(), scored on the device
    item = next(iter(loader))
    model.feed_data({'Uncomp': item['Uncomp'], 'QF': item['QF'], 'Z': Z[:1]}, need_GT=True)
    model.test()
    if chroma:
        with pytest.raises(ValueError, match='gt'):
            model.current_metrics()
    m = model.current_metrics(gt=item['Uncomp'], crop_border=border)
    assert set(m) == {'psnr', 'ssim'} and m['psnr'].is_cuda and m['psnr'].shape == (1,) and m['psnr'].dtype == torch.float64
    direct = jpeg_metrics.psnr_ssim(model.Output_Batch(within_0_1=False), item['Uncomp'].to(DEV), 'YCbCr' if chroma else 'Y', crop_border=border)
    assert torch.equal(m['psnr'], direct[0]) and torch.equal(m['ssim'], direct[1])
    if not chroma:
        assert torch.equal(model.current_metrics(crop_border=border)['psnr'], m['psnr'])
