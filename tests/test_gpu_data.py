"""esr_data_lrhr_batch (csrc/esr_data.hip) through esr_hip/data.py on the GPU, against a float64 restatement of its formula written here, and
DeviceLRHRLoader against the host LRHRDataset under the same seed.

hr is compared with torch.equal: it is u8.astype(float32) / 255. re-ordered (or the mix, whose fp64 expression is rounded to fp32 once).
lr: |lr - float64| <= (k^2 + 2) 2^-24 sum|taps| — the worst case of k^2 fp32 products of values in [0, 1] added in fp32, plus the rounding of
the taps and of the pixels to fp32 (about 3e-5 at k = 17; neighbouring random pixels differ by 0.3, so no indexing error passes).  Shapes:
a workgroup's tile is 8 x 8 LR pixels, so LR crops of 9, 10, 11, 17 and 33 a side have part-filled last tiles and those of 6 a part-filled only one;
most crops touch an image border."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

from test_host_data import GOLDEN, case_opt, write_set
from test_host_api import _opt

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _images(shapes, seed, lo=0, hi=256):
    rng = np.random.RandomState(seed)
    return [rng.randint(lo, hi, s).astype(np.uint8) for s in shapes]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the float64 restatement
def ref_convert(u8, cmap):
    """[H, W, Co] float32: the mapped image (RGB order)"""
    from esr_hip import _lib
    x = u8.astype(np.float32) / np.float32(255.)
    if u8.shape[2] == 1:
        return x
    if cmap.mode == _lib.DATA_MAP_RGB:
        return x[:, :, ::-1]
    t = (x * np.float32(cmap.scale)).astype(np.float64)
    acc = (t[..., 0] * cmap.w[0] + t[..., 1] * cmap.w[1]) + t[..., 2] * cmap.w[2]
    return ((acc / cmap.scale + cmap.b) / cmap.scale).astype(np.float32)[:, :, None]


def ref_augment(a, flags):
    """[H, W, C] -> util.augment's result for the three flag bits"""
    if flags & 1:
        a = a[:, ::-1]
    if flags & 2:
        a = a[::-1]
    if flags & 4:
        a = a.transpose(1, 0, 2)
    return a


def ref_item(u8, logical, y0, x0, flags, sf, taps, pre, ph, pw, cmap, lr_u8=None):
    """(hr [Co, ph, pw] float32, lr [Co, ph / sf, pw / sf] float64) of one item: the formula of include/esr_hip.h, term by term"""
    H, W = logical
    x = ref_convert(u8[:H, :W], cmap)
    hr = x[y0:y0 + ph, x0:x0 + pw]
    lh, lw, i0, j0 = ph // sf, pw // sf, y0 // sf, x0 // sf
    if lr_u8 is not None:
        lr = ref_convert(lr_u8, cmap)[i0:i0 + lh, j0:j0 + lw].astype(np.float64)
    else:
        k = taps.shape[0]
        half = k // 2
        x64 = x.astype(np.float64)
        lr = np.zeros((lh, lw, x.shape[2]))
        rows = np.clip(pre + sf * (i0 + np.arange(lh))[:, None] + half - np.arange(k)[None, :], 0, H - 1)          # [lh, k]
        cols = np.clip(pre + sf * (j0 + np.arange(lw))[:, None] + half - np.arange(k)[None, :], 0, W - 1)          # [lw, k]
        for c in range(x.shape[2]):
            lr[:, :, c] = np.einsum('uv,iujv->ij', taps, x64[:, :, c][rows[:, :, None, None], cols[None, None, :, :]])
    return ref_augment(hr, flags).transpose(2, 0, 1), ref_augment(lr, flags).transpose(2, 0, 1)


def lr_bound(taps):
    return (taps.size + 2) * 2.0 ** -24 * np.abs(taps).sum()


def run_batch(specs, sf, taps, pre, patch, cmap):
    """specs: dicts of u8, logical, y0, x0, flags[, lr_u8].  Runs the kernel once on all of them and compares every item."""
    from esr_hip import _lib, data as D
    ph, pw = (patch, patch) if isinstance(patch, int) else patch
    keep, items = [], []
    for s in specs:
        t = _dev(s['u8'])
        l = _dev(s['lr_u8']) if s.get('lr_u8') is not None else None
        keep.append((t, l))
        it = _lib.DataItem(hr=t.data_ptr(), lr=l.data_ptr() if l is not None else None, H=s['logical'][0], W=s['logical'][1], stride=s['u8'].shape[1],
                           channels=s['u8'].shape[2], y0=s['y0'], x0=s['x0'], flags=s['flags'])
        if l is not None:
            it.lr_H, it.lr_W, it.lr_stride = l.size(0), l.size(1), l.size(1)
        items.append(it)
    taps_d = _dev(taps.astype(np.float32)) if taps is not None else None
    hr, lr = D.lrhr_batch(items, sf, taps_d, pre, patch, cmap)
    torch.cuda.synchronize()
    hr, lr = hr.cpu().numpy(), lr.cpu().numpy()
    bound = lr_bound(taps) if taps is not None else 0.0
    worst = 0.0
    for n, s in enumerate(specs):
        want_hr, want_lr = ref_item(s['u8'], s['logical'], s['y0'], s['x0'], s['flags'], sf, taps, pre, ph, pw, cmap, s.get('lr_u8'))
        assert hr[n].shape == want_hr.shape and lr[n].shape == want_lr.shape
        assert np.array_equal(hr[n], want_hr), ('hr', n, {k: v for k, v in s.items() if k not in ('u8', 'lr_u8')})
        if s.get('lr_u8') is not None:
            assert np.array_equal(lr[n], want_lr.astype(np.float32)), ('supplied lr', n)
        else:
            err = float(np.abs(lr[n] - want_lr).max())
            worst = max(worst, err)
            assert err <= bound, ('lr', n, err, bound, {k: v for k, v in s.items() if k not in ('u8', 'lr_u8')})
    print('B %d sf %d k %s pre %d: worst |lr - float64| %.3e, bound %.3e' % (len(specs), sf, None if taps is None else taps.shape[0], pre, worst, bound))
    return hr, lr


def corner_specs(images, patch, sf, flag_codes):
    specs = []
    for u8 in images:
        H, W = u8.shape[:2]
        ph, pw = (patch, patch) if isinstance(patch, int) else patch
        inner = ((H - ph) // 2 // sf * sf, (W - pw) // 2 // sf * sf)
        for (y0, x0), flags in itertools.product([(0, 0), (0, W - pw), (H - ph, 0), (H - ph, W - pw), inner], flag_codes):
            specs.append(dict(u8=u8, logical=(H, W), y0=y0, x0=x0, flags=flags))
    return specs


# ---- the kernel
def test_plan():
    from esr_hip import _lib
    out = (C.c_int32 * 3)()
    for (sf, k, pre), tile in (((4, 17, 1), 8), ((8, 45, 3), 8), ((2, 9, 0), 8), ((3, 11, 1), 8), ((8, 63, 3), 8), ((16, 63, 7), 4)):
        assert _lib.lib.esr_data_lrhr_plan(sf, k, pre, out) == 0
        assert out[0] == tile and out[2] ** 2 * 4 <= 64 * 1024 and out[1] == max(k // 2 - pre, 0), (sf, k, list(out))
    assert _lib.lib.esr_data_lrhr_plan(4, 16, 1, out) < 0 and _lib.lib.esr_data_lrhr_plan(4, 65, 1, out) < 0 and _lib.lib.esr_data_lrhr_plan(4, 17, 4, out) < 0


def test_sf4_bicubic_every_augmentation_at_corners_and_interior():
    from esr_hip import data as D
    taps, pre = D.downscale_taps(4)
    assert taps.shape == (17, 17) and pre == 1
    specs = corner_specs(_images([(40, 48, 3), (48, 40, 3)], 1), 24, 4, range(8))
    run_batch(specs, 4, taps, pre, 24, D.channel_map(None))
    run_batch(corner_specs(_images([(40, 48, 3), (48, 40, 3)], 1), 40, 4, range(8)), 4, taps, pre, 40, D.channel_map(None))       # LR 10: tiles of 8 and 2


@pytest.mark.parametrize('pre', [0, 1])
def test_sf2(pre):
    """calc_strides gives pre 0 at sf 2; the odd one is run as well (the formula holds for any pre below sf)"""
    from esr_hip import data as D
    taps, pre0 = D.downscale_taps(2)
    assert taps.shape == (9, 9) and pre0 == 0
    run_batch(corner_specs(_images([(38, 42, 3)], 2), 34, 2, (0, 3, 5)), 2, taps, pre, 34, D.channel_map(None))          # LR 17: odd
    run_batch(corner_specs(_images([(72, 70, 1)], 2), 66, 2, (0, 6)), 2, taps, pre, 66, D.channel_map(None))            # LR 33: four tiles of 8 and one of 1


def test_sf3():
    from esr_hip import data as D
    taps, pre = D.downscale_taps(3)
    assert taps.shape == (11, 11) and pre == 1
    run_batch(corner_specs(_images([(39, 45, 3)], 3), 33, 3, (0, 6, 7)), 3, taps, pre, 33, D.channel_map(None))
    run_batch(corner_specs(_images([(39, 45, 3)], 3), (33, 27), 3, (0, 1, 2, 3)), 3, taps, pre, (33, 27), D.channel_map(None))       # no transpose: any rectangle


def test_sf8_non_separable_kernel():
    from CEM.imresize_CEM import imresize
    from esr_hip import data as D
    yy, xx = np.mgrid[-8:9, -8:9].astype(np.float64)
    th = 0.6
    a, b = np.cos(th) * xx + np.sin(th) * yy, -np.sin(th) * xx + np.cos(th) * yy
    kernel = np.exp(-0.5 * ((a / 4.5) ** 2 + (b / 2.0) ** 2))
    kernel /= kernel.sum()
    try:
        taps, pre = D.downscale_taps(8, kernel)
    finally:
        imresize(np.zeros((8, 8)), scale_factor=[1 / 8.], kernel='reset_2_default', return_upscale_kernel=True)
    k = taps.shape[0]
    assert k % 2 == 1 and k <= 63 and pre == 3 and np.linalg.matrix_rank(taps) > 1
    specs = corner_specs(_images([(96, 88, 3)], 4), 72, 8, (0, 5))          # LR 9 x 9: a second, one-pixel tile each way
    run_batch(specs, 8, taps, pre, 72, D.channel_map(None))
    assert np.array_equal(D.downscale_taps(8)[0], D.downscale_taps(8, 'reset_2_default')[0])


def test_validation_form_clamps_at_the_logical_size():
    from esr_hip import data as D
    taps, pre = D.downscale_taps(4)
    u8 = _images([(50, 59, 3)], 5, 0, 40)[0]
    u8[48:] = 255
    u8[:, 56:] = 255
    run_batch([dict(u8=u8, logical=(48, 56), y0=0, x0=0, flags=0)], 4, taps, pre, (48, 56), D.channel_map(None))


def test_every_byte_value_is_exact():
    from esr_hip import data as D
    taps, pre = D.downscale_taps(4)
    yy, xx = np.mgrid[0:32, 0:32]
    u8 = np.stack([(yy * 32 + xx + 85 * c) % 256 for c in range(3)], -1).astype(np.uint8)
    for color in (None, 'y', 'gray'):
        hr, _ = run_batch([dict(u8=u8, logical=(32, 32), y0=0, x0=0, flags=0)], 4, taps, pre, 32, D.channel_map(color))
        if color is None:
            assert all(len(np.unique(hr[0, c])) == 256 for c in range(3))
    run_batch([dict(u8=u8[:, :, :1], logical=(32, 32), y0=0, x0=0, flags=4)], 4, taps, pre, 32, D.channel_map('y'))       # 1 channel passes a mix through


@pytest.mark.parametrize('color', ['y', 'gray'])
def test_colour_mix_before_the_filter(color):
    from esr_hip import data as D
    taps, pre = D.downscale_taps(4)
    hr, lr = run_batch(corner_specs(_images([(40, 48, 3)], 6), 24, 4, (0, 7)), 4, taps, pre, 24, D.channel_map(color))
    assert hr.shape == (10, 1, 24, 24) and lr.shape == (10, 1, 6, 6)


@pytest.mark.parametrize('color', [None, 'y'])
def test_supplied_lr_is_the_plain_crop(color):
    from esr_hip import data as D
    u8, = _images([(40, 48, 3)], 7)
    lr_u8, = _images([(10, 12, 3)], 8)
    specs = [dict(s, lr_u8=lr_u8) for s in corner_specs([u8], 24, 4, (0, 1, 6))]
    run_batch(specs, 4, None, 0, 24, D.channel_map(color))
    # a batch may mix both kinds
    taps, pre = D.downscale_taps(4)
    run_batch(specs[:3] + corner_specs([u8], 24, 4, (2,)), 4, taps, pre, 24, D.channel_map(color))


def test_error_returns_are_negative_and_write_nothing():
    from esr_hip import _lib, data as D
    from esr_hip.act import stream_ptr
    taps, pre = D.downscale_taps(4)
    taps_d = _dev(taps.astype(np.float32))
    taps16 = _dev(np.ones((16, 16), np.float32))
    taps65 = _dev(np.ones((65, 65), np.float32))
    u8 = _dev(_images([(40, 48, 3)], 9)[0])
    u1 = _dev(_images([(40, 48, 1)], 9)[0])
    hr = torch.full((2, 3, 24, 24), -7.0, device=DEV)
    lr = torch.full((2, 3, 6, 6), -7.0, device=DEV)
    table_d = torch.zeros(2 * C.sizeof(_lib.DataItem), dtype=torch.uint8, device=DEV)
    rgb = D.channel_map(None)

    def call(B=2, sf=4, t=taps_d, k=17, pre=pre, ph=24, pw=24, cmap=rgb, items=True, dev=True, hr_p=True, lr_p=True, **edit):
        table = (_lib.DataItem * 2)()
        for n in range(2):
            table[n] = _lib.DataItem(hr=u8.data_ptr(), H=40, W=48, stride=48, channels=3, y0=8, x0=4, flags=0)
        for name, v in edit.items():
            setattr(table[1], name, v)
        return _lib.lib.esr_data_lrhr_batch(C.addressof(table) if items else None, table_d.data_ptr() if dev else None, B, sf,
                                            t.data_ptr() if t is not None else None, k, pre, ph, pw, C.byref(cmap) if cmap is not None else None,
                                            hr.data_ptr() if hr_p else None, lr.data_ptr() if lr_p else None, stream_ptr())
    bad = dict(
        patch_height_no_multiple=dict(ph=22), patch_width_no_multiple=dict(pw=26), crop_leaves_bottom=dict(y0=20), crop_leaves_right=dict(x0=28),
        crop_leaves_logical_size=dict(H=28), negative_origin=dict(y0=-4), origin_no_multiple=dict(x0=6), k_even=dict(t=taps16, k=16), k_above_63=dict(t=taps65, k=65),
        sf_zero=dict(sf=0), pre_not_below_sf=dict(pre=4), transpose_of_a_rectangle=dict(flags=4, pw=28), null_items=dict(items=False), null_device_items=dict(dev=False),
        null_taps=dict(t=None), null_map=dict(cmap=None), null_hr=dict(hr_p=False), null_lr=dict(lr_p=False), null_source=dict(hr=None), two_channels=dict(channels=2),
        mixed_channel_counts=dict(hr=u1.data_ptr(), channels=1), stride_below_width=dict(stride=40), unknown_flag=dict(flags=8), empty_batch=dict(B=0),
        lr_image_too_small=dict(lr=u8.data_ptr(), lr_H=7, lr_W=12, lr_stride=12))
    for name, kw in bad.items():
        rc = call(**kw)
        assert rc < 0, (name, rc)
    torch.cuda.synchronize()
    assert bool((hr == -7.0).all()) and bool((lr == -7.0).all())
    with pytest.raises(_lib.EsrError):
        D.lrhr_batch([_lib.DataItem(hr=u8.data_ptr(), H=40, W=48, stride=48, channels=3, y0=20, x0=0)], 4, taps_d, pre, 24, rgb, out=(hr[:1], lr[:1]))
    assert bool((hr == -7.0).all())


# ---- the loader
def _host_items(opt, indices, seed, kernel=None):
    from data.LRHR_dataset import LRHRDataset
    ds = LRHRDataset(opt, kernel=kernel)
    random.seed(seed)
    items = [ds[i] for i in indices]
    return torch.stack([it['HR'] for it in items]), torch.stack([it['LR'] for it in items]), [it['HR_path'] for it in items]


def _loader(opt, **extra):
    import data
    opt = dict(opt, device_batches=True, **extra)
    loader = data.create_dataloader(data.create_dataset(opt), opt)
    assert type(loader).__name__ == 'DeviceLRHRLoader'
    return loader


def _bicubic_bound():
    from esr_hip import data as D
    return lr_bound(D.downscale_taps(4)[0])


def test_loader_equals_the_host_dataset_under_the_same_seed(golden, tmp_path):
    opt = case_opt(golden, 'train_x4', write_set(golden, 'train', str(tmp_path / 'hr')))
    assert opt['batch_size'] == 4 and opt['patch_size'] == 24 and opt['scale'] == 4
    loader = _loader(opt)
    assert len(loader) == 1 and loader.dataset.opt['dataroot_HR'] == opt['dataroot_HR']           # 5 images, batch 4, drop_last
    random.seed(21)
    batches = list(loader)
    assert len(batches) == 1
    b = batches[0]
    want_hr, want_lr, paths = _host_items(opt, [0, 1, 2, 3], 21)
    assert b['HR'].is_cuda and b['LR'].is_cuda and b['HR_path'] == paths == b['LR_path']
    assert torch.equal(b['HR'].cpu(), want_hr)
    err = float((b['LR'].cpu().double() - want_lr.double()).abs().max())
    print('loader: |LR - host| %.3e, bound %.3e' % (err, _bicubic_bound()))
    assert err <= _bicubic_bound() + 2.0 ** -24                       # the host item is the float64 result rounded to fp32
    # a second epoch continues the same stream of draws, and shuffling takes torch's permutation
    shuffled = _loader(dict(opt, use_shuffle=True))
    torch.manual_seed(5)
    order = torch.randperm(5).tolist()
    torch.manual_seed(5)
    random.seed(22)
    b = next(iter(shuffled))
    want_hr, want_lr, paths = _host_items(opt, order[:4], 22)
    assert b['HR_path'] == paths and torch.equal(b['HR'].cpu(), want_hr)
    assert float((b['LR'].cpu().double() - want_lr.double()).abs().max()) <= _bicubic_bound() + 2.0 ** -24


def test_loader_validation_phase_and_colour(golden, tmp_path):
    opt = case_opt(golden, 'val_x4', write_set(golden, 'val', str(tmp_path / 'hr')))
    loader = _loader(opt)
    assert len(loader) == 3
    got = list(loader)
    for n, b in enumerate(got):
        want_hr, want_lr, paths = _host_items(opt, [n], 0)
        assert b['HR_path'] == paths and torch.equal(b['HR'].cpu(), want_hr), n          # modcrop: 50 x 59 -> 48 x 56, ...
        assert float((b['LR'].cpu().double() - want_lr.double()).abs().max()) <= _bicubic_bound() + 2.0 ** -24
    opt = case_opt(golden, 'train_x4_y', write_set(golden, 'train', str(tmp_path / 'hr2')))
    random.seed(23)
    b = next(iter(_loader(opt)))
    want_hr, want_lr, _ = _host_items(opt, [0, 1, 2, 3], 23)
    assert b['HR'].shape == (4, 1, 24, 24) and torch.equal(b['HR'].cpu(), want_hr)
    assert float((b['LR'].cpu().double() - want_lr.double()).abs().max()) <= _bicubic_bound() + 2.0 ** -24


def test_cache_eviction_changes_nothing(golden, tmp_path):
    opt = case_opt(golden, 'train_x4', write_set(golden, 'train', str(tmp_path / 'hr')))
    roomy, tight = _loader(opt), _loader(opt, device_cache_GB=12000 / 2.0 ** 30)              # images are 5.8 to 7.4 kB: two fit
    out = []
    for loader in (roomy, tight):
        random.seed(31)
        out.append([loader.batch(idx) for idx in ([0, 1, 2, 3], [4, 0, 3, 1], [2, 4, 1, 0])])
    assert len(roomy._cache) == 5 and len(tight._cache) <= 2 and tight._cached <= 12000
    for a, b in zip(*out):
        assert torch.equal(a['HR'], b['HR']) and torch.equal(a['LR'], b['LR']) and a['HR_path'] == b['HR_path']


def test_one_training_step_on_a_device_batch(tmp_path):
    """feed_data and optimize_parameters on what the loader yields (RRDB-1, one latent channel, as tests/test_gpu_model.py builds it)"""
    from PIL import Image
    import models
    from oracle.weights import fill_formula_weights
    folder = tmp_path / 'hr'
    folder.mkdir()
    for n, a in enumerate(_images([(112, 104, 3), (104, 120, 3)], 41)):
        Image.fromarray(a).save(str(folder / ('%d.png' % n)))
    dopt = dict(name='e2e', mode='LRHR', phase='train', scale=4, data_type='img', dataroot_HR=str(folder), dataroot_LR=None, subset_file=None, color=None,
                patch_size=96, batch_size=2, use_shuffle=True, use_flip=True, use_rot=True, n_workers=0)
    opt = _opt(nb=1, lat=1, cem=True, is_train=True)
    opt['gpu_ids'] = [0]
    m = models.create_model(opt)
    fill_formula_weights(m.netG, gain=1.0)
    random.seed(41)
    batch = next(iter(_loader(dopt)))
    assert batch['LR'].shape == (2, 3, 24, 24) and batch['HR'].shape == (2, 3, 96, 96) and batch['LR'].is_cuda
    for _ in range(2):          # without a discriminator the first call is idle
        m.feed_data(batch)
        assert m.var_L.data_ptr() == batch['LR'].data_ptr()           # .to(device) had nothing to do
        m.optimize_parameters()
    log = m.get_current_log()
    assert 'l_g_pix' in log and np.isfinite(log['l_g_pix']), log
