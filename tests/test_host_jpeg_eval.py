"""CPU tests of data/JPEG_dataset.py and of the NumPy route of esr_hip/jpeg_metrics.py (what CPU tensors take), against
tests/golden/jpeg_eval.npz — items, quality-factor schedules and util.tensor2img chroma outputs recorded from the reference's own code by
tools/gen_jpeg_eval_golden.py (codes/utils/util.py imports under oracle/_refshim, so the pictures in the fixture are the reference's own, not a
restatement's).

`ref_pre_round` restates utils/util.py:209-226 with data/util.py:198-215 inlined, up to the value BEFORE .round() — which the reference never
returns, and which the tie-free inputs of tests/test_gpu_jpeg_eval.py are selected by; its rounding is checked against the fixture here.
The helpers below (inputs, the written-out evaluation loop) are shared with tests/test_gpu_jpeg_eval.py.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_eval.npz')
MODES = {'Y': 1, 'YCbCr': 3}
TIE_BAND = 1e-3            # a host pre-rounding value this close to a half-integer may round the other way under another fp64 summation order
_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def write_images(folder, which=None):
    """the fixture's source images as img_00.png ... (the names the reference's dataset saw)"""
    from PIL import Image
    g = golden()
    os.makedirs(str(folder), exist_ok=True)
    for i in (range(4) if which is None else which):
        Image.fromarray(g['img/%d' % i]).save(os.path.join(str(folder), 'img_%02d.png' % i))
    return str(folder)


def case_opt(name, root, prefix='case'):
    opt = json.loads(str(golden()['%s/%s/opt' % (prefix, name)]))
    return dict(opt, dataroot_Uncomp=root)


def ref_pre_round(img, chroma_mode, min_max=(0, 255)):
    """util.tensor2img's chroma branches on a float32 [3, H, W] ('YCbCr') or [H, W] ('Y') array, up to `img_np * 255.0` of :226"""
    img_np = np.array(img, dtype=np.float32)
    if chroma_mode == 'YCbCr':                                                             # :213
        ycc = np.transpose(img_np / 255, (1, 2, 0))
    else:                                                                                  # :220
        ycc = np.stack([img_np / 255] + 2 * [128 / 255 * np.ones_like(img_np)], -1)
    assert ycc.dtype == np.float32
    ycc *= 255.                                                                            # data/util.py:207
    rlt = np.matmul(ycc, [[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071],
                          [0.00625893, -0.00318811, 0]]) * 255.0 + [-222.921, 135.576, -276.836]
    rlt /= 255.
    img_np = 255 * rlt.astype(np.float32)[:, :, [2, 1, 0]]
    img_np = (np.clip(img_np, min_max[0], min_max[1]) - min_max[0]) / (min_max[1] - min_max[0])
    assert img_np.dtype == np.float32
    return img_np * 255.0


def near_tie(pre):
    """[H, W] bool: a channel of the pixel lies within TIE_BAND of a half-integer"""
    return (np.abs(pre - np.floor(pre) - 0.5) < TIE_BAND).any(-1)


def decoder_like(shape, chroma_mode, seed):
    """float32 [B, C, H, W] in 0...255 as the decoder gives it: bgr2ycbcr of random RGB images plus noise of a few levels, with a band of rows
    pushed above and one below [0, 255] so that the clip is exercised (uniform random YCbCr leaves the RGB gamut in 44 % of its pixels)"""
    import data.util as util
    rng = np.random.Generator(np.random.PCG64(seed))
    B, H, W = shape
    out = []
    for _ in range(B):
        bgr = rng.integers(0, 256, (H, W, 3)).astype(np.float32) / 255.
        ycc = 255 * util.bgr2ycbcr(bgr, only_y=False).astype(np.float64) + rng.normal(0, 3.0, (H, W, 3))
        ycc[1:3] += 100.0
        ycc[4:5] -= 100.0
        out.append(ycc.transpose(2, 0, 1)[:MODES[chroma_mode]])
    return np.ascontiguousarray(np.stack(out)).astype(np.float32)


def tie_free(x, chroma_mode, min_max=(0, 255), seed=0):
    """x with the pixels re-drawn whose host pre-rounding value is a near-tie in some channel, until none is left"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    x = x.copy()
    for _ in range(20):
        bad = np.stack([near_tie(ref_pre_round(im if chroma_mode == 'YCbCr' else im[0], chroma_mode, min_max)) for im in x])
        if not bad.any():
            return x
        x[np.broadcast_to(bad[:, None], x.shape)] += rng.uniform(-2, 2, int(bad.sum()) * x.shape[1]).astype(np.float32)
    raise AssertionError('near-ties left after 20 re-draws')


def host_scores(a, b, chroma_mode, border=0, min_max=(0, 255)):
    """the loop of test_JPEG.py:239-275 written out: image() of every sample and of the ground truth, calculate_psnr / calculate_ssim"""
    from esr_hip import jpeg_metrics, metrics
    H, W = a.shape[-2:]
    crop = lambda im: im[border:H - border, border:W - border]                             # noqa: E731
    ia = [crop(jpeg_metrics.image(torch.from_numpy(im), chroma_mode, min_max=min_max)) for im in a]
    ib = [crop(jpeg_metrics.image(torch.from_numpy(im), chroma_mode, min_max=min_max)) for im in b]
    pairs = [(x, ib[i if len(ib) > 1 else 0]) for i, x in enumerate(ia)]
    return np.array([metrics.calculate_psnr(x, y) for x, y in pairs]), np.array([metrics.calculate_ssim(x, y) for x, y in pairs])


def host_std(x, chroma_mode):
    """np.std(np.stack(sr_imgs), 0) of test_JPEG.py:263 per image of x [S, B, C, H, W] -> (float64 [B, 3, H, W] in R, G, B planes, mean [B])"""
    from esr_hip import jpeg_metrics
    maps = []
    for b in range(x.shape[1]):
        imgs = [jpeg_metrics.image(torch.from_numpy(x[s, b]), chroma_mode) for s in range(x.shape[0])]
        maps.append(np.std(np.stack(imgs), 0)[:, :, ::-1].transpose(2, 0, 1))
    maps = np.stack(maps)
    return maps, maps.reshape(len(maps), -1).mean(1)


def host_evaluate(model, loader, Z, border=0):
    """the loop of test_JPEG.py:165-327 on the host: get_current_visuals (an fp32 copy of every sample), image(), calculate_*, np.std;
    also `flips`: in how many pixels the picture image() makes of the tensor where it lies (esr_ycbcr_image for a model on the GPU) differs from
    the host's, for every decoded sample and for the plainly decompressed image, inside the crop and in the whole picture — each such pixel
    checked to be a near-tie on the host that moved by one level (none when the model is on the CPU: the routes are then the same)"""
    from esr_hip import jpeg_metrics, metrics
    mode = 'YCbCr' if model.chroma_mode else 'Y'
    S = 1 if Z is None else len(Z)
    res = {k: [] for k in ('psnr', 'ssim', 'psnr_quantized', 'ssim_quantized', 'pixel_std', 'flips', 'flips_full', 'flips_quantized', 'pixels', 'pixels_full')}
    stds = []
    for item in loader:
        gt = 1 * item['Uncomp']
        data = {'Uncomp': torch.cat([item['Uncomp']] * S, 0), 'QF': torch.cat([item['QF']] * S, 0), 'Z': 0 if Z is None else Z}
        model.feed_data(data, need_GT=True)
        model.test()
        visuals = model.get_current_visuals(need_Uncomp=True, entire_batch=True)
        for module in model.JPEG.values():
            module.Set_Q_Table(data['QF'][:1])
        H, W = gt.shape[-2:]
        crop = lambda im: im[border:H - border, border:W - border]                         # noqa: E731
        gt_img = jpeg_metrics.image(gt[0], mode)
        sr = [jpeg_metrics.image(visuals['Decomp'][s], mode) for s in range(S)]
        quantized = jpeg_metrics.image(model.Return_Compressed(gt.to(model.device))[0].cpu(), mode)
        res['psnr'].append([metrics.calculate_psnr(crop(im), crop(gt_img)) for im in sr])
        res['ssim'].append([metrics.calculate_ssim(crop(im), crop(gt_img)) for im in sr])
        res['psnr_quantized'].append(metrics.calculate_psnr(crop(quantized), crop(gt_img)))
        res['ssim_quantized'].append(metrics.calculate_ssim(crop(quantized), crop(gt_img)))
        stds.append(np.std(np.stack(sr), 0))
        res['pixel_std'].append(np.mean(stds[-1]))
        def flips(tensor, host_img):
            there = jpeg_metrics.image(tensor, mode).astype(np.int32)
            moved = (there != host_img).any(-1)
            t = tensor.cpu().numpy()
            assert np.abs(there - host_img).max() <= 1 and not (moved & ~near_tie(ref_pre_round(t if mode == 'YCbCr' else t[0], mode))).any()
            return moved
        moved = [flips(d, im) for d, im in zip(model.Output_Batch(within_0_1=False).detach(), sr)]
        res['flips'].append([int(crop(m).sum()) for m in moved])
        res['flips_full'].append([int(m.sum()) for m in moved])
        res['flips_quantized'].append(int(crop(flips(model.Return_Compressed(gt.to(model.device))[0], quantized)).sum()))
        res['pixels'].append((H - 2 * border) * (W - 2 * border))
        res['pixels_full'].append(H * W)
    flat = [v.reshape([-1, 3]) for v in stds]                                               # :321-326
    res['std_of_image_mean_std'] = float(np.std(np.stack([np.mean(v) for v in flat])))
    every = np.concatenate(flat, 0)
    res['mean_pixel_std'] = float(every.mean())
    res['std_of_pixel_std'] = float(np.std(every, 0).mean())
    return {k: np.array(v) if isinstance(v, list) else v for k, v in res.items()}


# ------------------------------------------------------------------------------------------------ JpegDataset
@pytest.mark.parametrize('name', ['train_y', 'train_chroma', 'val_y', 'test_chroma'])
def test_items_equal_the_reference_bit_for_bit(tmp_path, name):
    """train and test phases, Y and chroma, a grey file (img_03), [lo, hi] ranges with and without QF_probs, 16-pixel blocks"""
    from data.JPEG_dataset import JpegDataset
    g = golden()
    ds = JpegDataset(case_opt(name, write_images(tmp_path)))
    assert len(ds) == int(g['case/%s/len' % name]) == 4
    assert [os.path.basename(p) for p in ds.paths_Uncomp] == list(g['case/%s/names' % name])
    seed = int(g['case/%s/seed' % name])
    random.seed(seed)
    np.random.seed(seed)
    for j, i in enumerate(g['case/%s/indices' % name]):
        item = ds[int(i)]
        want = g['case/%s/%d/Uncomp' % (name, j)]
        assert set(item) == {'Uncomp', 'Uncomp_path', 'QF'} and item['Uncomp'].dtype == torch.float32
        assert item['Uncomp'].shape == want.shape and item['Uncomp'].shape[0] == (3 if 'chroma' in name else 1)
        assert np.array_equal(item['Uncomp'].numpy(), want), (name, j)
        assert int(item['QF']) == int(g['case/%s/%d/QF' % (name, j)]), (name, j)
        assert os.path.basename(item['Uncomp_path']) == str(g['case/%s/%d/name' % (name, j)])
    if name == 'val_y':
        assert tuple(ds[3]['Uncomp'].shape) == (1, 40, 40)                    # the 41 x 46 grey file, cropped to whole 8-pixel blocks
    if name == 'test_chroma':
        assert ds.block_size == 16 and tuple(ds[0]['Uncomp'].shape) == (3, 32, 48)


@pytest.mark.parametrize('name', ['single', 'longer_list', 'longer_small', 'one_range', 'two_ranges', 'numbers'])
def test_qf_schedule_of_the_test_phase(tmp_path, name):
    from data.JPEG_dataset import JpegDataset
    ds = JpegDataset(case_opt(name, write_images(tmp_path), prefix='qf'))
    want = golden()['qf/%s/schedule' % name]
    assert [int(q) for q in ds.per_index_QF] == want.tolist()
    if len(want) == len(ds):
        assert [int(ds[i]['QF']) for i in range(len(ds))] == want.tolist()


def test_dataset_refusals_and_lists(tmp_path):
    from data.JPEG_dataset import JpegDataset
    root = write_images(tmp_path / 'img')
    opt = case_opt('train_y', root)
    with pytest.raises((NotImplementedError, ImportError), match='lmdb'):
        JpegDataset(dict(opt, data_type='lmdb'))
    with pytest.raises(AssertionError, match='8x8 blocks'):
        JpegDataset(dict(opt, patch_size=36))
    with pytest.raises(AssertionError, match='8x8 blocks'):
        JpegDataset(dict(case_opt('train_chroma', root), patch_size=24))           # chroma trains on 16-pixel blocks
    assert len(JpegDataset(dict(case_opt('val_y', root), patch_size=36))) == 4     # (only training asserts it)
    with pytest.raises(AssertionError):
        JpegDataset(dict(opt, QF_probs=[1.0, 1.0]))
    # subset_file (train phase only) and scales
    subset = tmp_path / 'subset.txt'
    subset.write_text('img_02.png\nimg_00.png\n')
    ds = JpegDataset(dict(opt, subset_file=str(subset)))
    assert [os.path.basename(p) for p in ds.paths_Uncomp] == ['img_00.png', 'img_02.png']
    assert len(JpegDataset(dict(case_opt('val_y', root), subset_file=str(subset)))) == 4
    scaled = tmp_path / 'scaled'
    scaled.mkdir()
    from PIL import Image
    for n in ('a_scale0_x.png', 'b_scale1_x.png', 'c_scale2_x.png', 'd.png'):
        Image.fromarray(golden()['img/0']).save(str(scaled / n))
    ds = JpegDataset(dict(opt, dataroot_Uncomp=str(scaled), scales=[2, 0, 1]))
    assert [os.path.basename(p) for p in ds.paths_Uncomp] == ['a_scale0_x.png', 'a_scale0_x.png', 'c_scale2_x.png']
    with pytest.raises(AssertionError, match='empty'):
        JpegDataset(dict(opt, dataroot_Uncomp=str(scaled), scales=[0, 0, 0]))
    ds.random_scale_list = [1, 0.5]
    with pytest.raises(ValueError, match='random_scale_list'):
        ds[0]


def test_create_dataloader_over_the_dataset(tmp_path):
    """create_dataset keeps refusing the mode (tests/test_host_data.py); the class goes to the unchanged create_dataloader by hand"""
    import data
    from data.JPEG_dataset import JpegDataset
    root = write_images(tmp_path)
    with pytest.raises(NotImplementedError):
        data.create_dataset(case_opt('val_y', root))
    opt = case_opt('train_chroma', root)
    batches = list(data.create_dataloader(JpegDataset(opt), opt))
    assert len(batches) == 2
    for b in batches:
        assert b['Uncomp'].shape == (2, 3, 32, 32) and b['Uncomp'].dtype == torch.float32 and b['QF'].shape == (2,) and len(b['Uncomp_path']) == 2
    opt = case_opt('val_y', write_images(tmp_path / 'three', which=[0, 1, 2]))
    batches = list(data.create_dataloader(JpegDataset(opt), opt))
    assert [tuple(b['Uncomp'].shape) for b in batches] == [(1, 1, 40, 48), (1, 1, 48, 40), (1, 1, 56, 40)]
    assert all(int(b['QF']) == 15 for b in batches)


# ------------------------------------------------------------------------------------------------ jpeg_metrics.image
@pytest.mark.parametrize('rname,min_max', [('0_255', (0, 255)), ('16_235', (16, 235))])
@pytest.mark.parametrize('key,mode', [('ycbcr', 'YCbCr'), ('y', 'Y')])
def test_image_equals_the_reference_pictures(key, mode, rname, min_max):
    from esr_hip import jpeg_metrics
    g = golden()
    x = g['t2i/' + key]
    want = g['t2i/%s_%s_u8' % (key, rname)]
    got = jpeg_metrics.image(torch.from_numpy(x), mode, min_max=min_max)
    assert got.dtype == np.uint8 and got.shape == want.shape == x.shape[-2:] + (3,)
    assert np.array_equal(got, want)
    assert np.array_equal(ref_pre_round(x, mode, min_max).round(), want)                   # the restatement the tie-free inputs rely on
    assert ((want == 0).mean() > 0.02 and (want == 255).mean() > 0.02) or min_max != (0, 255)       # the clip worked on both sides
    f32 = jpeg_metrics.image(torch.from_numpy(x), mode, out_type=np.float32, min_max=min_max)
    want_f = g['t2i/%s_%s_f32' % (key, rname)]
    assert f32.dtype == np.float32 and float(np.abs(f32 - want_f).max()) * 255 <= 2.0 ** -16            # one fp32 ulp of 255, in 0...255 units
    if mode == 'Y':
        assert np.array_equal(jpeg_metrics.image(torch.from_numpy(x[None]), mode, min_max=min_max), want)      # [1, H, W]
        pre = ref_pre_round(x, mode, min_max)                                  # grey, but the three channels are not equal before rounding
        assert 0 < float(np.abs(pre[..., 0] - pre[..., 1]).max()) < 2e-3 and 0 < float(np.abs(pre[..., 1] - pre[..., 2]).max()) < 2e-3
    both = jpeg_metrics.image(torch.from_numpy(np.stack([x.reshape((-1,) + x.shape[-2:])] * 2)), mode, min_max=min_max)
    assert isinstance(both, list) and len(both) == 2 and np.array_equal(both[0], want) and np.array_equal(both[1], want)
    assert np.array_equal(jpeg_metrics.image(torch.from_numpy(x).double(), mode, min_max=min_max), want)


def test_image_refusals():
    from esr_hip import jpeg_metrics, metrics
    y, ycc = torch.zeros(12, 12), torch.zeros(3, 12, 12)
    with pytest.raises(ValueError, match='3-channels image input with Y chroma mode'):
        jpeg_metrics.image(ycc, 'Y')
    with pytest.raises(ValueError, match='Single-channels image input with YCbCr chroma mode'):
        jpeg_metrics.image(y, 'YCbCr')
    with pytest.raises(ValueError, match='Single-channels'):
        jpeg_metrics.image(y[None], 'YCbCr')
    with pytest.raises(ValueError, match='chroma_mode'):
        jpeg_metrics.image(ycc, None)
    with pytest.raises(ValueError, match='2-channel'):
        jpeg_metrics.image(torch.zeros(2, 12, 12), 'Y')
    with pytest.raises(TypeError, match='dimension'):
        jpeg_metrics.image(torch.zeros(1, 1, 3, 12, 12), 'YCbCr')
    with pytest.raises(ValueError, match='min_max'):
        jpeg_metrics.image(ycc, 'YCbCr', min_max=(255, 0))
    with pytest.raises(ValueError, match='same dimensions'):
        jpeg_metrics.psnr_ssim(torch.zeros(2, 3, 12, 12), torch.zeros(1, 3, 12, 13), 'YCbCr')
    with pytest.raises(ValueError, match='same dimensions'):
        jpeg_metrics.psnr_ssim(torch.zeros(3, 3, 12, 12), torch.zeros(2, 3, 12, 12), 'YCbCr')
    with pytest.raises(ValueError, match='11'):
        jpeg_metrics.psnr_ssim(ycc, ycc, 'YCbCr', crop_border=1)
    with pytest.raises(ValueError, match='crop_border'):
        jpeg_metrics.psnr_ssim(ycc, ycc, 'YCbCr', crop_border=6)
    with pytest.raises(ValueError, match='S, B, C, H, W'):
        jpeg_metrics.sample_std(torch.zeros(2, 3, 12, 12), 'YCbCr')
    with pytest.raises(NotImplementedError):                                   # the SR half's conversion keeps refusing (tests/test_host_metrics.py)
        metrics.tensor2img(ycc, chroma_mode='YCbCr')


# ------------------------------------------------------------------------------------------------ scores on the CPU route
@pytest.mark.parametrize('mode', list(MODES))
def test_cpu_scores_equal_the_written_out_loop(mode):
    from esr_hip import jpeg_metrics
    gt = decoder_like((3, 23, 45), mode, 5)
    a = (gt + np.random.Generator(np.random.PCG64(6)).normal(0, 4.0, gt.shape)).astype(np.float32)
    for b, border in ((gt, 0), (gt[:1], 0), (gt, 4)):
        p, s = jpeg_metrics.psnr_ssim(torch.from_numpy(a), torch.from_numpy(b), mode, crop_border=border)
        assert p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (3,)
        want = host_scores(a, b, mode, border)
        assert np.abs(p.numpy() - want[0]).max() <= 1e-12 and np.abs(s.numpy() - want[1]).max() <= 1e-12
        assert 5 < float(p.min()) and float(p[0]) > 25 and -1 < float(s.min()) and float(s.max()) < 1        # (against gt[:1], images 1 and 2 are unrelated)
    p, s = jpeg_metrics.psnr_ssim(torch.from_numpy(a[0] if mode == 'YCbCr' else a[0, 0]), torch.from_numpy(gt[0]), mode)    # single images
    assert p.shape == (1,) and abs(float(p) - host_scores(a[:1], gt[:1], mode)[0][0]) <= 1e-12
    p, s = jpeg_metrics.psnr_ssim(torch.from_numpy(gt), torch.from_numpy(gt), mode)
    assert torch.isinf(p).all() and float((s - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('S', [1, 3])
def test_cpu_sample_std_equals_np_std_of_the_pictures(mode, S):
    from esr_hip import jpeg_metrics
    base = decoder_like((2, 13, 18), mode, 7)
    x = (base[None] + np.random.Generator(np.random.PCG64(8)).normal(0, 5.0, (S,) + base.shape)).astype(np.float32)
    got_map, got_mean = jpeg_metrics.sample_std(torch.from_numpy(x), mode)
    want_map, want_mean = host_std(x, mode)
    assert got_map.dtype == torch.float32 and got_map.shape == (2, 3, 13, 18) and got_mean.dtype == torch.float64 and got_mean.shape == (2,)
    assert np.array_equal(got_map.numpy(), want_map.astype(np.float32)) and np.abs(got_mean.numpy() - want_mean).max() <= 1e-12
    assert (S == 1) == (not got_map.any())


def eval_loader(folder, chroma):
    """the 3 colour images of the fixture behind create_dataloader in the test phase: 8-pixel blocks for the Y model, 16 for the colour model"""
    import data
    from data.JPEG_dataset import JpegDataset
    opt = dict(case_opt('test_chroma' if chroma else 'val_y', write_images(folder, which=[0, 1, 2])), jpeg_quality_factor=20)
    return data.create_dataloader(JpegDataset(opt), opt)


def latent_samples(S, nz=64, seed=9):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (S, nz, 1, 1)).astype(np.float32))


EVAL_KEYS = ('psnr', 'ssim', 'psnr_quantized', 'ssim_quantized', 'pixel_std', 'std_of_image_mean_std', 'mean_pixel_std', 'std_of_pixel_std')


@pytest.mark.parametrize('chroma', [False, True], ids=['Y', 'colour'])
def test_cpu_evaluate_equals_the_written_out_loop(tmp_path, chroma):
    from esr_hip import jpeg_metrics
    if chroma:
        from test_host_jpeg_chroma import make_model
    else:
        from test_host_jpeg import make_model
    model = make_model(tmp_path)
    loader, Z = eval_loader(tmp_path / 'images', chroma), latent_samples(3)
    got = jpeg_metrics.evaluate(model, loader, Z=Z, crop_border=2)
    want = host_evaluate(model, loader, Z, border=2)
    assert got['psnr'].shape == got['ssim'].shape == (3, 3) and got['psnr_quantized'].shape == got['pixel_std'].shape == (3,)
    assert [os.path.basename(p) for p in got['paths']] == ['img_00.png', 'img_01.png', 'img_02.png']
    for k in EVAL_KEYS:
        assert np.abs(np.asarray(got[k]) - want[k]).max() <= 1e-12, k
    assert np.isfinite(got['psnr']).all() and (got['pixel_std'] > 0).all() and got['std_of_pixel_std'] > 0
    assert len({round(float(v), 6) for v in got['psnr'][0]}) == 3                          # the samples differ: Z reaches the decoder
    one = jpeg_metrics.evaluate(model, loader)                                             # one pass, Z = 0
    assert one['psnr'].shape == (3, 1) and not one['pixel_std'].any() and one['mean_pixel_std'] == 0
    # current_metrics: the last test() against the ground truth
    item = next(iter(loader))
    model.feed_data({'Uncomp': item['Uncomp'], 'QF': item['QF'], 'Z': 0}, need_GT=True)
    model.test()
    if chroma:
        with pytest.raises(ValueError, match='gt'):
            model.current_metrics()
    else:
        m = model.current_metrics()
        assert torch.equal(m['psnr'], model.current_metrics(gt=item['Uncomp'])['psnr'])
    m = model.current_metrics(gt=item['Uncomp'])
    assert set(m) == {'psnr', 'ssim'} and m['psnr'].shape == (1,) and m['psnr'].dtype == torch.float64
    assert abs(float(m['psnr']) - one['psnr'][0, 0]) <= 1e-12 and abs(float(m['ssim']) - one['ssim'][0, 0]) <= 1e-12


def test_cabi_refusals_without_a_gpu():
    """argument checks run before anything touches the device: every refusal is a negative code"""
    import ctypes as C
    from esr_hip import _lib
    from esr_hip._lib import ESR_E_ARG, ESR_E_UNSUPPORTED
    h = _lib.load_library()
    p = 4096
    assert h.esr_ycbcr_image(None, 1, 3, 8, 8, 0.0, 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 1, 3, 8, 8, 0.0, 255.0, None, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 1, 2, 8, 8, 0.0, 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 0, 3, 8, 8, 0.0, 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 1, 3, 0, 8, 0.0, 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 1, 3, 8, 8, 255.0, 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 1, 3, 8, 8, float('nan'), 255.0, p, None) == ESR_E_ARG
    assert h.esr_ycbcr_image(p, 70000, 3, 8, 8, 0.0, 255.0, p, None) == ESR_E_UNSUPPORTED
    assert h.esr_psnr_ssim_ycbcr_partials(3, 48, 80, 0) == 3 * 3 * 3 and h.esr_psnr_ssim_ycbcr_partials(1, 11, 11, 0) == 3
    assert h.esr_psnr_ssim_ycbcr_partials(2, 48, 80, 0) == ESR_E_ARG and h.esr_psnr_ssim_ycbcr_partials(3, 8, 8, 4) == ESR_E_ARG
    ok = (p, p, 2, 3, 16, 16, C.c_int64(768), 0.0, 255.0, 0, p, p, None)
    for i, bad in ((0, None), (1, None), (2, 0), (3, 2), (4, 0), (5, -1), (6, C.c_int64(256)), (8, 0.0), (9, 8), (9, -1), (10, None), (11, None)):
        args = list(ok)
        args[i] = bad
        assert h.esr_psnr_ssim_ycbcr(*args) == ESR_E_ARG, i
    assert h.esr_psnr_ssim_ycbcr(p, p, 30000, 3, 16, 16, C.c_int64(0), 0.0, 255.0, 0, p, p, None) == ESR_E_UNSUPPORTED
    assert h.esr_sample_std_ycbcr_partials(3, 21, 66) == 2 and h.esr_sample_std_ycbcr_partials(4, 21, 66) == ESR_E_ARG
    ok = (p, 2, 1, 3, 8, 8, 0.0, 255.0, p, p, p, None)
    for i, bad in ((0, None), (1, 0), (2, 0), (3, 4), (4, 0), (5, 0), (7, -1.0), (8, None), (9, None), (10, None)):
        args = list(ok)
        args[i] = bad
        assert h.esr_sample_std_ycbcr(*args) == ESR_E_ARG, i
    assert h.esr_sample_std_ycbcr(p, 2, 70000, 3, 8, 8, 0.0, 255.0, p, p, p, None) == ESR_E_UNSUPPORTED
