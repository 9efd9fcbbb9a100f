"""One CEM kernel per image of a batch on the GPU: the esr_cem_*_per_image entry points (taps [B][k][k]) against the float64 contract of
oracle/cem_contract_ref.py evaluated image by image with that image's taps, then CEM_PyTorch.set_per_image_kernels, SRRaGANModel.set_kernels and
tools/super_resolve.py on top of them.

Scale 4, B = 3, C = 3 and 1, a 74 x 70 low-resolution frame (24 x 20 padded by the batch's margin 25: ragged tiles both ways, not square).  Taps:
full-rank synthetic ones (R.synthetic_2d, three seeds per size, k = 9, 17, 43) and the product's — bicubic and two rotated anisotropic Gaussians
zero-padded to 17 / 43 (tests/test_host_cem_per_image.py).  Destinations are carved out of NaN-sentinel allocations.  The upscale reference is
R.upscale at crop 0, cut to the crop window afterwards: R crops as its last step, so this is R.upscale(crop=c) element for element, at a third of
the float64 work.

Bound: R.bound(n = k^2, S, ref, ...) / R.bound_mode2, the derived bound of the single-kernel 2-D tests, k the (padded) size handed to the kernel.
For the projection (three kernels in a row) the bound is composed: a stage's own R.bound plus the previous stage's bound carried through the
stage's |taps| (the ops are linear; |tanh'| <= 1 for the range-limited form) — project_ref below.

Record (MI355X, worst |error| / bound per family; a record, not a tolerance):
  downscale_per_image 0.028 (k 9, fused)   lrfilter_per_image 0.047 (k 9)   upscale_per_image 0.032 (k 9, mode 0)   planes > 65535 0.099 (lrfilter, k 5)
  CEM_PyTorch projection 0.004   model 0.004
(the error of n products grows like sqrt(n), the bound like n: the small filters come closest.  What shows that the bound still tells one image's
taps from another's is the wrong-image check of every entry-point test.)"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cem_contract_ref as R
from oracle.weights import fill_formula_weights
from test_host_api import _opt
from test_host_cem_per_image import SF, conf_for, kernels, nets, wrap

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0x7FC0DEAD          # a quiet NaN with a recognisable payload
GUARD = 64
PRE = SF - SF // 2 - 1
B, H, W = 3, 74, 70
WORST = {}


def _L():
    from esr_hip import _lib
    return _lib.lib


def _stream():
    from esr_hip.act import stream_ptr
    return stream_ptr()


class Carved:
    """A destination inside a sentinel-filled allocation."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.raw = torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(torch.float32).view(shape)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all()), 'the launch wrote outside its destination'
        assert not bool((self.raw[GUARD:GUARD + self.n] == SENT).any()), 'part of the destination was never written'


def ptr(t):
    return t.data_ptr() if t is not None else None


def judge(family, got, ref, bnd, what=''):
    r = R.worst_ratio(got, ref, bnd)
    WORST[family] = max(WORST.get(family, 0.0), r)
    print('%s error/bound %.3f %s (worst so far %.3f)' % (family, r, what, WORST[family]))
    assert r <= 1.0, (family, what, r)
    return r


def per_image(fn):
    """fn(b) -> (value, S) of image b alone; the batch's (value, S), concatenated (tuples: element-wise)."""
    parts = [fn(b) for b in range(B)]

    def cat(items):
        return tuple(cat([it[j] for it in items]) for j in range(len(items[0]))) if isinstance(items[0], tuple) else torch.cat(items)
    return cat([p[0] for p in parts]), cat([p[1] for p in parts])


@pytest.fixture(scope='module')
def product_taps():
    """The product's three per-image tap arrays [3, k, k] (CPU, fp32): what set_per_image_kernels hands the kernels."""
    cem = wrap(nets()[0])
    cem.set_per_image_kernels(nets())
    return {'down': cem.DownscaleOP.taps().clone(), 'filt': cem.Conv_LR_with_Inv_hTh_OP.taps().clone(), 'up': cem.Upscale_OP.taps().clone()}


def tap_set(name, op, product):
    if name == 'product':
        return product[op]
    k = int(name[3:])
    return torch.stack([R.synthetic_2d(k, seed) for seed in (k, k + 100, k + 200)])


TAPS = ['syn9', 'syn17', 'syn43', 'product']


def cut(x, crop):
    if isinstance(x, tuple):
        return tuple(cut(v, crop) for v in x)
    return x[:, :, crop:x.shape[-2] - crop, crop:x.shape[-1] - crop] if crop else x


# ---- the three entry points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('name', TAPS)
def test_downscale_per_image(name, C, product_taps):
    """cem_downscale_tiled_kernel<true>: plain, fused with lr_pad 0 and 3; and the tap sets handed over in another order are refused by the bound."""
    taps = tap_set(name, 'down', product_taps)
    k = taps.shape[-1]
    td = taps.to(DEV).contiguous()
    y = R.uniform((B, C, H * SF, W * SF), 1).to(DEV)
    for fused, lr_pad in ((False, 0), (True, 0), (True, 3)):
        lr = R.uniform((B, C, H - 2 * lr_pad, W - 2 * lr_pad), 2).to(DEV) if fused else None
        d = Carved((B, C, H, W))
        assert _L().esr_cem_downscale_per_image(y.data_ptr(), B, C, H, W, SF, PRE, td.data_ptr(), k, ptr(lr), lr_pad, d.ptr, _stream()) == 0
        d.check()
        ref, S = per_image(lambda b: R.downscale(y[b:b + 1], taps[b], SF, PRE, lr[b:b + 1] if fused else None, lr_pad))
        bnd = R.bound(k * k, S, ref)
        judge('downscale_per_image', d.t, ref, bnd, '%s C%d%s' % (name, C, ' fused pad %d' % lr_pad if fused else ''))
        if not fused:
            wrong = Carved((B, C, H, W))
            tw = td[[1, 2, 0]].contiguous()
            assert _L().esr_cem_downscale_per_image(y.data_ptr(), B, C, H, W, SF, PRE, tw.data_ptr(), k, None, 0, wrong.ptr, _stream()) == 0
            wrong.check()
            assert not R.accepts(wrong.t, ref, bnd), 'permuted tap sets pass: the image index does not select the taps'
            for b in range(B):          # ... and every image is refused on its own, not just the batch
                assert not R.accepts(wrong.t[b], ref[b], bnd[b])


@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('name', TAPS)
def test_lrfilter_per_image(name, C, product_taps):
    """cem_lrfilter_tiled_kernel<true> (two ragged 64-column tiles, five 16-row tiles)."""
    taps = tap_set(name, 'filt', product_taps)
    k = taps.shape[-1]
    td = taps.to(DEV).contiguous()
    x = R.uniform((B, C, H, W), 3).to(DEV)
    o = Carved((B, C, H, W))
    assert _L().esr_cem_lrfilter_per_image(x.data_ptr(), B, C, H, W, td.data_ptr(), k, o.ptr, _stream()) == 0
    o.check()
    ref, S = per_image(lambda b: R.lrfilter(x[b:b + 1], taps[b]))
    bnd = R.bound(k * k, S, ref)
    judge('lrfilter_per_image', o.t, ref, bnd, '%s C%d' % (name, C))
    wrong = Carved((B, C, H, W))
    tw = td[[2, 0, 1]].contiguous()
    assert _L().esr_cem_lrfilter_per_image(x.data_ptr(), B, C, H, W, tw.data_ptr(), k, wrong.ptr, _stream()) == 0
    wrong.check()
    for b in range(B):
        assert not R.accepts(wrong.t[b], ref[b], bnd[b])


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('name', TAPS)
def test_upscale_per_image(name, C, mode, product_taps):
    """cem_upscale_tiled_kernel<mode >= 2, true>, crops 0, sf and 2 sf + 1 (the last breaks the 16-byte alignment of the rows)."""
    taps = tap_set(name, 'up', product_taps)
    k = taps.shape[-1]
    td = taps.to(DEV).contiguous()
    rng = 0.75
    f = R.uniform((B, C, H, W), 4).to(DEV)
    f2 = R.uniform((B, C, H, W), 5).to(DEV) if mode >= 2 else None
    g = R.uniform((B, C, H * SF, W * SF), 6, 0.0, 1.0).to(DEV) if mode >= 1 else None
    ref0, S0 = per_image(lambda b: R.upscale(f[b:b + 1], taps[b], SF, PRE, f2=f2[b:b + 1] if mode >= 2 else None,
                                             g=g[b:b + 1] if mode >= 1 else None, crop=0, mode=mode, range=rng))
    for crop in (0, SF, 2 * SF + 1):
        Ho, Wo = H * SF - 2 * crop, W * SF - 2 * crop
        out = Carved((B, C, Ho, Wo))
        out2 = Carved((B, C, Ho, Wo)) if mode == 3 else None

        def launch(t, o, o2):
            return _L().esr_cem_upscale_per_image(f.data_ptr(), ptr(f2), B, C, H, W, SF, PRE, t.data_ptr(), k, ptr(g), crop, mode, rng, o.ptr,
                                                  o2.ptr if o2 else None, _stream())
        assert launch(td, out, out2) == 0
        out.check()
        ref, S = cut(ref0, crop), cut(S0, crop)
        gc = cut(g, crop) if g is not None else None
        what = '%s C%d mode %d crop %d' % (name, C, mode, crop)
        if mode == 0:
            bnd = R.bound(k * k, S, ref)
        elif mode == 1:
            bnd = R.bound(k * k, S, ref, gc)
        elif mode == 2:
            # (S = (S of U(f), S of g - U(f2), U(f), g - U(f2)), already cut; bound_mode2 cuts g itself)
            bnd = R.bound_mode2(k * k, S, g, crop, rng)
        if mode < 3:
            judge('upscale_per_image', out.t, ref, bnd, what)
        else:
            out2.check()
            bnd = R.bound(k * k, S[0], ref[0])
            judge('upscale_per_image', out.t, ref[0], bnd, what + ' out')
            judge('upscale_per_image', out2.t, ref[1], R.bound(k * k, S[1], ref[1], gc), what + ' out2')
            ref = ref[0]
        if crop == SF:
            wrong = Carved((B, C, Ho, Wo))
            wrong2 = Carved((B, C, Ho, Wo)) if mode == 3 else None
            assert launch(td[[1, 2, 0]].contiguous(), wrong, wrong2) == 0
            wrong.check()
            for b in range(B):
                assert not R.accepts(wrong.t[b], ref[b], bnd[b])


def test_more_planes_than_grid_z_through_cem_ops():
    """B * C = 65538 planes (B = 21846, C = 3, 4 x 4, k = 5) through cem_ops: the flat kernels' <true> instantiations, the image index taken per
    thread.  Images and tap sets repeat with periods 3 and 5: the first 15 images are judged against float64, every later image must repeat the
    image 15 k before it bit for bit (the arithmetic of a plane does not depend on where it lies)."""
    from esr_hip import cem_ops
    Bn, C, h, k = 21846, 3, 4, 5
    pool_t = torch.stack([R.synthetic_2d(k, 300 + i) for i in range(5)])
    taps = pool_t[torch.arange(Bn) % 5].contiguous()
    idx = torch.arange(Bn) % 3
    x = R.uniform((3, C, h, h), 7)[idx].to(DEV)
    y = R.uniform((3, C, h * SF, h * SF), 8)[idx].to(DEV)
    lr = R.uniform((3, C, h, h), 9)[idx].to(DEV)
    g = R.uniform((3, C, h * SF, h * SF), 10, 0.0, 1.0)[idx].to(DEV)
    td = taps.to(DEV)
    got = {
        'down': cem_ops.downscale_raw(y, td, SF, PRE, lr=lr, lr_pad=0),
        'filt': cem_ops.lr_filter_raw(x, td),
        'up': cem_ops.upscale_raw(x, td, SF, PRE, g=g, crop=1, mode=1),
    }
    n = 15
    for b in range(n):
        s = slice(b, b + 1)
        ref, S = R.downscale(y[s], taps[b], SF, PRE, lr[s], 0)
        judge('planes > 65535', got['down'][s], ref, R.bound(k * k, S, ref), 'downscale image %d' % b)
        ref, S = R.lrfilter(x[s], taps[b])
        judge('planes > 65535', got['filt'][s], ref, R.bound(k * k, S, ref), 'lrfilter image %d' % b)
        ref, S = R.upscale(x[s], taps[b], SF, PRE, g=g[s], crop=1, mode=1)
        judge('planes > 65535', got['up'][s], ref, R.bound(k * k, S, ref, cut(g[s], 1)), 'upscale image %d' % b)
    for name, out in got.items():
        assert out.shape[0] == Bn
        first = out[:n]
        reps = first.repeat((Bn + n - 1) // n, 1, 1, 1)[:Bn]
        assert torch.equal(out, reps), name
    assert not torch.equal(got['filt'][0], got['filt'][3])          # same image, another tap set


# ---- CEM_PyTorch, pair input ----------------------------------------------------------------------------------------------------------------------
def project_ref(lr, g, td, ti, tu, lr_pad, crop, rng):
    """The projection of ONE image in float64 — g + U(K(lr_p - D g)), or U(K lr_p) + tanh(g - U(K D g)) rng — and its composed bound: every
    stage's own R.bound (n = k^2 of the taps handed over) plus the previous stage's bound carried through the stage's |taps|."""
    nd, ni, nu = td.shape[-1] ** 2, ti.shape[-1] ** 2, tu.shape[-1] ** 2

    def K_abs(b):
        return R.lrfilter(b, ti.abs())[0]

    def U_abs(b):
        return R.upscale(b, tu.abs(), SF, PRE, crop=crop)[0]
    if rng is None:
        e, Se = R.downscale(g, td, SF, PRE, lr, lr_pad)
        be = R.bound(nd, Se, e)
        f, Sf = R.lrfilter(e, ti)
        bf = R.bound(ni, Sf, f) + K_abs(be)
        out, So = R.upscale(f, tu, SF, PRE, g=g, crop=crop, mode=1)
        return out, R.bound(nu, So, out, cut(g, crop)) + U_abs(bf)
    lrp = R.pad_replicate(lr.double(), lr_pad)
    dg, Sd = R.downscale(g, td, SF, PRE)
    bd = R.bound(nd, Sd, dg)
    fx, Sx = R.lrfilter(lrp, ti)
    bx = R.bound(ni, Sx, fx)
    fg, Sg = R.lrfilter(dg, ti)
    bg = R.bound(ni, Sg, fg) + K_abs(bd)
    out, S = R.upscale(fx, tu, SF, PRE, f2=fg, g=g, crop=crop, mode=2, range=rng)
    return out, R.bound_mode2(nu, S, g, crop, rng) + U_abs(bx) + abs(rng) * U_abs(bg)


def check_projection(family, out, single_outs, lr, g, taps, lr_pad, crop, rng, what):
    """out: the batch's output; single_outs[i]: image i through a single-kernel CEM of its own (unpadded) filters.  Both compute the float64
    projection with image i's filters: the batch within the composed bound, the two within twice that of each other (the single kernel's own
    bound is no larger: fewer taps, or rank-one taps as two passes)."""
    for i in range(B):
        ref, bnd = project_ref(lr[i:i + 1], g[i:i + 1], taps['down'][i], taps['filt'][i], taps['up'][i], lr_pad, crop, rng)
        judge(family, out[i:i + 1], ref, bnd, '%s image %d' % (what, i))
        assert single_outs[i].shape == ref.shape
        assert R.accepts(out[i:i + 1], single_outs[i].double(), 2 * bnd), (what, i)
    # image 1 (the 33 x 33 Gaussian: ds_kernel 17, inv_hTh 43) is not padded and not rank one: its single-kernel CEM runs the shared 2-D kernels
    # on these very taps, and the per-image kernels repeat their arithmetic
    assert torch.equal(out[1:2], single_outs[1]), what


@pytest.mark.parametrize('limit', [False, True])
@pytest.mark.parametrize('train', [True, False])
def test_cem_pytorch_pair_input(train, limit, product_taps):
    settings = dict(sigmoid_range_limit=limit, input_range=np.array([0.0, 1.0]))
    cem = wrap(nets()[0], **settings).to(DEV)
    cem.set_per_image_kernels(nets())
    cem.train(train)
    lr = R.uniform((B, 3, 24, 20), 11, 0.0, 1.0).to(DEV)
    g = R.uniform((B, 3, 96, 80), 12, 0.0, 1.0).to(DEV)
    with torch.no_grad():
        out = cem([lr, g])
        singles = []
        for i, net in enumerate(nets()):
            one = wrap(net, margin=25, **settings).to(DEV).train(train)
            assert one.DownscaleOP.taps().dim() == 2 and one.margins_LR == 25
            singles.append(one([lr[i:i + 1], g[i:i + 1]]))
    assert tuple(out.shape) == (B, 3, 96, 80)
    mL = 0 if train else 25
    gp = R.pad_replicate(g, SF * mL)
    check_projection('CEM_PyTorch projection', out, singles, lr, gp, product_taps, mL, SF * mL, 1.0 if limit else None,
                     '%s%s' % ('train' if train else 'eval', ' range-limited' if limit else ''))


def test_cem_pytorch_per_image_refuses_gradients():
    from esr_hip._lib import EsrError
    cem = wrap(nets()[0]).to(DEV)
    cem.set_per_image_kernels(nets())
    lr = torch.rand(B, 3, 24, 20, device=DEV)
    g = torch.rand(B, 3, 96, 80, device=DEV, requires_grad=True)
    with pytest.raises(EsrError, match='per-image kernels: forward only'):
        cem([lr, g])
    with pytest.raises(EsrError, match='per-image kernels: forward only'):
        cem.DownscaleOP(g)
    with torch.no_grad():
        assert tuple(cem.DownscaleOP(g).shape) == (B, 3, 24, 20)
    with pytest.raises(ValueError, match='per-image kernels'):
        cem.DownscaleOP(g.detach()[:2])


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def resize_cache():
    """create_model(opt, kernel=k) leaves k in imresize's process-wide cache: hand the cache back as it was."""
    from CEM.imresize_CEM import imresize
    had, before = hasattr(imresize, 'kernels'), dict(getattr(imresize, 'kernels', {}))
    yield
    imresize.kernels = before
    if not had:
        del imresize.kernels


def _model(kernel=None):
    import models
    opt = _opt(nb=1)
    opt['gpu_ids'] = [0]
    if kernel is not None:
        opt['test']['kernel'] = 'estimated'
    m = models.create_model(opt, kernel=kernel)
    fill_formula_weights(m.netG, gain=1.0)
    return m


def test_model_set_kernels(resize_cache, product_taps):
    from esr_hip._lib import EsrError
    ks = kernels()
    m = _model()
    x = R.uniform((B, 3, 24, 20), 13, 0.0, 1.0)
    m.feed_data({'LR': x}, need_GT=False)
    m.test()
    plain = m.fake_H.clone()
    G = m.netG.generated_image_model
    engine, packs, params = G.engine, dict(G.engine._packed), list(m.netG.parameters())
    assert packs

    m.set_kernels(ks)
    m.feed_data({'LR': x}, need_GT=False)
    m.test()
    out = m.fake_H.clone()
    assert tuple(out.shape) == (B, 3, 96, 80) and not torch.equal(out, plain)
    # the generator was not touched: the same module, engine, parameters and weight packs
    assert m.netG.generated_image_model is G and G.engine is engine and G.engine._packed.keys() == packs.keys()
    assert all(G.engine._packed[k] is packs[k] for k in packs)
    assert all(a is b for a, b in zip(m.netG.parameters(), params))
    with torch.no_grad():
        m.netG.eval()
        g = G(x.to(DEV), pad=25)
        m.netG.train()
    singles = []
    for i, k in enumerate(ks):
        one = _model(k)
        one.netG.set_margins_LR(25)
        one.feed_data({'LR': x[i:i + 1]}, need_GT=False)
        one.test()
        singles.append(one.fake_H.clone())
        with torch.no_grad():
            one.netG.eval()
            assert torch.equal(one.netG.generated_image_model(x[i:i + 1].to(DEV), pad=25), g[i:i + 1]), 'the generator depends on the batch'
    check_projection('model', out, singles, x.to(DEV), g, product_taps, 25, 100, None, 'model')

    with pytest.raises(EsrError, match='per-image kernels: forward only'):
        m.test(prevent_grads_calc=False)
    m.set_kernels(None)
    m.feed_data({'LR': x}, need_GT=False)
    m.test()
    assert torch.equal(m.fake_H, plain)
    assert all(G.engine._packed[k] is packs[k] for k in packs)


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------------
def test_super_resolve_tool(tmp_path, resize_cache):
    import json
    import scipy.io
    from PIL import Image
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import super_resolve
    folder = tmp_path / 'pictures'
    folder.mkdir()
    rs = np.random.RandomState(5)
    names = ['a.png', 'b.png', 'c.png']
    for n in names:
        Image.fromarray(rs.randint(0, 256, (24, 20, 3)).astype(np.uint8)).save(str(folder / n))
    for n, k in zip(names[:2], kernels()[1:]):
        scipy.io.savemat(super_resolve.kernel_path(str(folder / n), SF), {'Kernel': k})
    cfg = {'name': 'per_image', 'model': 'srragan', 'scale': SF, 'gpu_ids': [0], 'range': [0, 1],
           'path': {'root': str(tmp_path), 'pretrained_model_G': None},
           'network_G': {'which_model_G': 'RRDB_net', 'CEM_arch': 1, 'sigmoid_range_limit': 0, 'latent_input': 'None', 'latent_input_domain': 'HR_downscaled',
                         'latent_channels': 0, 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32},
           'network_D': None, 'test': {'kernel': None}}
    opt = tmp_path / 'test_SR.json'
    opt.write_text(json.dumps(cfg))
    super_resolve.main([str(folder), '--opt', str(opt), '--kernels', 'estimated', '--batch', '4'])
    for n in names:
        with Image.open(str(folder / (n[:-4] + '_SR.png'))) as im:
            assert im.size == (80, 96) and im.mode == 'RGB'
    assert sorted(os.listdir(str(folder))) == sorted(names + [n[:-4] + '_SR.png' for n in names] + [n[:-4] + '_kernel_x4.mat' for n in names[:2]])
