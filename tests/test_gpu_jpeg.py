"""GPU tests (-m gpu) of explorable JPEG decoding: the block-DCT kernels (csrc/esr_jpeg.hip, esr_hip/jpeg.py, JPEG_module/JPEG.py), the DnCNN
generator on the conv kernels (esr_hip/dncnn.py, architecture.DnCNN), DecompCNNModel and the Z search through it.

Kernel tolerances are not constants of this file: each is 4 x the REFERENCE's own fp32 distance from a float64 restatement of the transform
on the same input, computed here from tests/golden/jpeg_dncnn.npz (the factor 4 allows another association of two 8-term fp32 sums and a
cosine table in place of torch.cos).  For quantities the fixture does not hold (the adjoints, the 16 x 1 x 256 x 256 input) the reference's
RELATIVE distance on the fixture input of the same kind is used: the transforms are linear and the inputs are drawn alike, so the error scales
with the magnitude of the result.  The quantised compressor is compared under the tie rule of tests/test_host_jpeg.py.  The CPU fallbacks
are patched to raise, so a silent fallback cannot pass.

Shapes beyond the fixture's (B, h x w blocks of 8 x 8 pixels, rows of the fixture's tables): 'one' a single block; 'ragged' w = 35 — not a
multiple of 4, so the scalar tail of the 16-byte path, and one workgroup tile of 32 blocks plus a remainder of 3; 'vector' w = 36, the 16-byte
path with a partial second tile of 4."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.check_golden import rel_l2
from oracle.weights import seeded_uniform
from test_host_jpeg import FX, G, golden, make_generator

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SPLIT_BAR = 1e-3          # the generator and VGG tests' relative bar


@pytest.fixture(autouse=True)
def no_cpu_fallback(monkeypatch):
    from esr_hip import jpeg as J

    def refuse(*a, **k):
        raise AssertionError('the CPU fallback ran in a GPU test')
    monkeypatch.setattr(J, '_compress_cpu', refuse)
    monkeypatch.setattr(J, '_extract_cpu', refuse)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _noise(B, h, w, seed):
    return torch.floor(seeded_uniform((B, 1, 8 * h, 8 * w), seed) * 256)


# name -> (fixture input of the same kind, table rows, input)
SHAPES = {'one': ('smooth', [3], lambda: G.smooth_pattern(1, 8, 8, 4305)),
          'ragged': ('noise', [1, 3, 5], lambda: _noise(3, 2, 35, 4310)),
          'vector': ('noise', [2, 4], lambda: _noise(2, 2, 36, 4320))}
_cases = {}


def _case(name):
    """(x, tables, reference cn / cq / img_q / img_n or None, the reference's distances) — computed once per name, left unchanged"""
    if name not in _cases:
        _cases[name] = _make_case(name)
    return _cases[name]


def _make_case(name):
    """a module-level case of the fixture; 'user': 16 x 1 x 256 x 256 noise, bounds of 'noise'; a SHAPES entry: bounds of its kind"""
    g = golden()
    kind = 'noise' if name == 'user' else SHAPES[name][0] if name in SHAPES else name
    ref = {k: torch.from_numpy(np.asarray(g['a/%s/%s' % (kind, k)])).float() for k in ('x', 'cq', 'cn', 'img_q', 'img_n')}
    tables = torch.from_numpy(g['a/tables'])
    # the reference's own distances from float64, absolute and relative to the largest value
    c64 = G.compress64(ref['x'], tables)
    d = {'compress': float((ref['cn'].double() - c64).abs().max()), 'compress_rel': float((ref['cn'].double() - c64).abs().max() / c64.abs().max())}
    for k, c in (('q', ref['cq']), ('n', ref['cn'])):
        i64 = G.extract64(c, tables)
        d['extract_' + k] = float((ref['img_' + k].double() - i64).abs().max())
        d['extract_%s_rel' % k] = d['extract_' + k] / float((i64 - 128).abs().max())
    if name == 'user':
        x = torch.floor(seeded_uniform((16, 1, 256, 256), 4100) * 256).clamp(0, 255)
        tables = tables.repeat(3, 1)[:16]
        return x, tables, None, d
    if name in SHAPES:
        return SHAPES[name][2](), tables[SHAPES[name][1]].contiguous(), None, d
    return ref['x'], tables, ref, d


@pytest.mark.parametrize('name', ['noise', 'smooth', 'user', 'one', 'ragged', 'vector'])
def test_kernels_against_float64(name):
    from esr_hip import jpeg as J
    x, tables, ref, d = _case(name)
    xg, tg = x.to(DEV), tables.to(DEV)
    c64 = G.compress64(x, tables)
    cn = J.compress(xg, tg, False)
    err = float((cn.cpu().double() - c64).abs().max())
    bound = 4 * (d['compress'] if ref is not None else d['compress_rel'] * float(c64.abs().max()))
    print('%s compressor: kernel %.3g, reference %.3g (bound %.3g)' % (name, err, bound / 4, bound))
    assert err <= bound
    assert torch.equal(cn, J.compress(xg, tg, False))                                   # two calls, equal bits
    for key, c in (('q', torch.round(c64).float()), ('n', c64.float())):
        i64 = G.extract64(c, tables)
        same, img = J.extract(c.to(DEV), tg)
        err = float((img.cpu().double() - i64).abs().max())
        bound = 4 * (d['extract_' + key] if ref is not None and key == 'n' else d['extract_%s_rel' % key] * float((i64 - 128).abs().max()))
        print('%s extractor (%s): kernel %.3g (bound %.3g)' % (name, key, err, bound))
        assert err <= bound
        assert torch.equal(same.cpu(), c)
        assert torch.equal(img, J.extract(c.to(DEV), tg)[1])
    if ref is not None:                                                                 # on the reference's own coefficient inputs
        for key in ('q', 'n'):
            img = J.extract(ref['c' + key].to(DEV), tg)[1]
            err = float((img.cpu().double() - G.extract64(ref['c' + key], tables)).abs().max())
            print('%s extractor on the stored c%s: kernel %.3g, reference %.3g' % (name, key, err, d['extract_' + key]))
            assert err <= 4 * d['extract_' + key]


@pytest.mark.parametrize('name', ['smooth', 'user', 'ragged', 'vector'])
def test_adjoint_kernels(name):
    """d_coef = qtab * DCT(d_img) and d_x = iDCT(d_coef / qtab) against float64, and <A x, y> = <x, A^T y> with both sides from the kernels"""
    from esr_hip import jpeg as J
    x, tables, _, d = _case(name)
    B, _, H, W = x.shape
    tg = tables.to(DEV)
    rel = 4 * max(d['compress_rel'], d['extract_n_rel'])
    d_img = seeded_uniform((B, 1, H, W), 4200, -1.0, 1.0)
    d_coef = seeded_uniform((B, 64, H // 8, W // 8), 4201, -1.0, 1.0)
    y = seeded_uniform((B, 64, H // 8, W // 8), 4202, -3.0, 3.0)
    q = tables.double().view(B, 64, 1, 1)
    # extractor: c = coef + sigmoid(y) - 0.5, img = 128 + iDCT(c q)
    coef = (x[:, :, :H // 8, :W // 8] / 16).round().expand(B, 64, H // 8, W // 8).contiguous()
    cg, yg = coef.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    c_out, img = J.extract(cg, tg, yg)
    s = torch.sigmoid(y.double())
    assert float((c_out.detach().cpu().double() - (coef.double() + s - 0.5)).abs().max()) < 1e-5
    i64 = G.extract64(coef.double() + s - 0.5, tables)
    assert float((img.detach().cpu().double() - i64).abs().max()) <= rel * float((i64 - 128).abs().max())
    (img * d_img.to(DEV)).sum().backward()
    g64 = G.compress64(d_img.double() + 128, torch.ones(B, 64)) * q                    # DCT(d_img) * q
    for got, want, what in ((cg.grad, g64, 'd_coef'), (yg.grad, g64 * s * (1 - s), 'd_y')):
        err = float((got.cpu().double() - want).abs().max())
        print('%s %s: kernel %.3g (bound %.3g)' % (name, what, err, rel * float(want.abs().max())))
        assert err <= rel * float(want.abs().max())
    ax = (G.extract64(d_coef, tables) - 128)
    lhs = float((ax * d_img.double()).sum())                                           # <A x, y>, A = iDCT(. q)
    ax_k = J.extract(d_coef.to(DEV), tg)[1].cpu().double() - 128
    assert abs(float((ax_k * d_img.double()).sum()) - float((d_coef.double() * cg.grad.cpu().double()).sum())) <= rel * float(ax.norm() * d_img.double().norm())
    assert abs(lhs - float((d_coef.double() * g64).sum())) <= 1e-9 * float(ax.norm() * d_img.double().norm())
    # non-quantising compressor: coef = DCT(x - 128) / q
    xg = x.to(DEV).requires_grad_(True)
    cn = J.compress(xg, tg, False)
    (cn * d_coef.to(DEV)).sum().backward()
    dx64 = G.extract64(d_coef.double() / (q * q), tables) - 128                        # iDCT(d_coef / q)
    err = float((xg.grad.cpu().double() - dx64).abs().max())
    print('%s d_x: kernel %.3g (bound %.3g)' % (name, err, rel * float(dx64.abs().max())))
    assert err <= rel * float(dx64.abs().max())
    bx = J.compress(d_img.to(DEV) + 128, tg, False).cpu().double()                     # B y, B = DCT(.) / q
    assert abs(float((bx * d_coef.double()).sum()) - float((d_img.double() * xg.grad.cpu().double()).sum())) <= rel * float(bx.norm() * d_coef.double().norm())
    # the quantising compressor's gradient is zero, as torch.round's
    xq = x.to(DEV).requires_grad_(True)
    J.compress(xq, tg, True).sum().backward()
    assert float(xq.grad.abs().max()) == 0.0


@pytest.mark.parametrize('name', ['noise', 'smooth', 'user', 'one', 'ragged', 'vector'])
def test_quantised_compressor_under_the_tie_rule(name):
    from esr_hip import jpeg as J
    x, tables, ref, _ = _case(name)
    c64 = G.compress64(x, tables)
    ties = G.tie_mask(c64)
    assert float(ties.double().mean()) <= G.TIE_CAP
    cq = J.compress(x.to(DEV), tables.to(DEV), True).cpu()
    want = ref['cq'] if ref is not None else torch.round(c64).float()
    assert torch.equal(cq[~ties], want[~ties])
    assert bool(((cq[ties].double() == torch.floor(c64[ties])) | (cq[ties].double() == torch.ceil(c64[ties]))).all())
    print('%s: %.3f %% of the coefficients excluded as ties, %d of them differ from the reference' % (
        name, 100 * float(ties.double().mean()), int((cq[ties] != want[ties]).sum())))


@pytest.mark.parametrize('planes', [2, 1])
@pytest.mark.parametrize('quantize', [True, False])
def test_act_out_equals_pack_of_the_fp32_result(planes, quantize):
    from esr_hip import _lib, jpeg as J
    from esr_hip.act import new_zeroed, view_of
    for name in ('smooth', 'ragged'):                                                  # 'ragged': a partial tile, the j < nb guard of the store
        x, tables, _, _ = _case(name)
        xg, tg = x.to(DEV), tables.to(DEV)
        B, h, w = x.size(0), x.size(2) // 8, x.size(3) // 8
        for lead in (0, 8):                                                            # behind `lead` groups of a wider buffer, as behind Z
            a, b = new_zeroed(planes, B, lead + 8, h, w, DEV), new_zeroed(planes, B, lead + 8, h, w, DEV)
            coef = J.compress_into(xg, tg, quantize, view_of(a, lead, 8))
            assert torch.equal(coef, J.compress(xg, tg, quantize))
            assert _lib.lib.esr_pack_nchw(coef.data_ptr(), 0, B, 64, h, w, 0, 64, 0, 1, C.byref(view_of(b, lead, 8)), _stream()) == 0
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            assert J.compress_into(xg, tg, quantize, view_of(a, lead, 8), want_coef=False) is None


def _off16(t):
    """(guard buffer, a copy of t that starts 4 bytes behind a 16-byte boundary: the guard's element 0 lies in front of it)"""
    buf = torch.zeros(t.numel() + 1, device=DEV)
    off = buf[1:].view(t.shape)
    off.copy_(t)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    return buf, off


def test_unaligned_coefficient_pointers_take_the_scalar_path_and_give_the_same_bits():
    """w = 36 would take the 16-byte path; a coefficient pointer 4 bytes off a 16-byte boundary must fall back: every coefficient-side
    pointer of the three entry points that have one, one at a time, against the aligned call"""
    from esr_hip import _lib
    L = _lib.lib
    x, tables, _, _ = _case('vector')
    B, h, w = x.size(0), x.size(2) // 8, x.size(3) // 8
    xg, tg = x.to(DEV), tables.to(DEV)
    new = lambda *shape: torch.zeros(*shape, device=DEV)
    # esr_jpeg_compress: the output
    coef = new(B, 64, h, w)
    assert L.esr_jpeg_compress(xg.data_ptr(), B, 8 * h, 8 * w, tg.data_ptr(), 1, coef.data_ptr(), None, _stream()) == 0
    buf, off = _off16(coef * 0)
    assert L.esr_jpeg_compress(xg.data_ptr(), B, 8 * h, 8 * w, tg.data_ptr(), 1, off.data_ptr(), None, _stream()) == 0
    assert torch.equal(off, coef) and float(buf[0]) == 0.0
    # esr_jpeg_extract: coef, y, coef_out
    y = seeded_uniform((B, 64, h, w), 4330, -3.0, 3.0).to(DEV)
    c_a, img_a = new(B, 64, h, w), new(B, 1, 8 * h, 8 * w)
    assert L.esr_jpeg_extract(coef.data_ptr(), y.data_ptr(), B, h, w, tg.data_ptr(), c_a.data_ptr(), img_a.data_ptr(), _stream()) == 0
    for which in ('coef', 'y', 'coef_out'):
        args = {'coef': coef, 'y': y, 'coef_out': new(B, 64, h, w)}
        buf, args[which] = _off16(args[which])
        img = new(B, 1, 8 * h, 8 * w)
        assert L.esr_jpeg_extract(args['coef'].data_ptr(), args['y'].data_ptr(), B, h, w, tg.data_ptr(), args['coef_out'].data_ptr(),
                                  img.data_ptr(), _stream()) == 0, which
        assert torch.equal(img, img_a) and torch.equal(args['coef_out'], c_a), which
        assert float(buf[0]) == 0.0, which
    # esr_jpeg_extract_grad: d_coef, d_y
    d_img = seeded_uniform((B, 1, 8 * h, 8 * w), 4331, -1.0, 1.0).to(DEV)
    dc_a, dy_a = new(B, 64, h, w), new(B, 64, h, w)
    assert L.esr_jpeg_extract_grad(d_img.data_ptr(), y.data_ptr(), B, h, w, tg.data_ptr(), dc_a.data_ptr(), dy_a.data_ptr(), _stream()) == 0
    for which in ('d_coef', 'd_y'):
        args = {'d_coef': new(B, 64, h, w), 'd_y': new(B, 64, h, w)}
        buf, args[which] = _off16(args[which])
        assert L.esr_jpeg_extract_grad(d_img.data_ptr(), y.data_ptr(), B, h, w, tg.data_ptr(), args['d_coef'].data_ptr(),
                                       args['d_y'].data_ptr(), _stream()) == 0, which
        assert torch.equal(args['d_coef'], dc_a) and torch.equal(args['d_y'], dy_a), which
        assert float(buf[0]) == 0.0, which


def test_jpeg_module_on_the_gpu_matches_the_fixture():
    from JPEG_module.JPEG import JPEG
    g = golden()
    x = torch.from_numpy(g['a/smooth/x']).float().to(DEV)
    tables = torch.from_numpy(g['a/tables'])
    comp, ext = JPEG(True, True), JPEG(False)
    for m in (comp, ext):
        m.Set_Q_Table(torch.from_numpy(g['a/qf']).to(DEV))
    assert torch.equal(comp.Q_table.reshape(6, 64).cpu(), tables)
    ties = G.tie_mask(G.compress64(x.cpu(), tables))
    cq = comp(x)
    assert torch.equal(cq.cpu()[~ties], torch.from_numpy(g['a/smooth/cq']).float()[~ties])
    ref_img = torch.from_numpy(g['a/smooth/img_q'])
    ref_err = float((ref_img.double() - G.extract64(torch.from_numpy(g['a/smooth/cq']).float(), tables)).abs().max())
    assert float((ext(torch.from_numpy(g['a/smooth/cq']).float().to(DEV)).cpu() - ref_img).abs().max()) <= 5 * ref_err     # 4 x + the reference's own
    assert torch.equal(ext.Multiply_By_Q_table(cq).cpu(), cq.cpu() * tables.view(6, 64, 1, 1))


# ------------------------------------------------------------------------------------------------ generator
def _oracle64(net64, x, masks=None):
    """float64 pre-sigmoid output of the module (CPU).  masks: per activation the GPU's pattern (stored output > 0), forced."""
    L = net64.num_latent_channels
    z, y = x[:, :L], x[:, L:]
    ai = 0
    for i, m in enumerate(net64.dncnn):
        if isinstance(m, torch.nn.Sigmoid):
            break
        if isinstance(m, torch.nn.Conv2d):
            if L and (net64.latent_input == 'all_layers' or i == 0):
                y = torch.cat([z, y], 1)
            y = m(y)
        elif isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
            slope = 0.0 if isinstance(m, torch.nn.ReLU) else m.negative_slope
            if masks is None:
                y = F.leaky_relu(y, slope)
            else:
                y = y * (masks[ai].double() + (~masks[ai]).double() * slope)
            ai += 1
        else:
            y = m(y)
    return y


def _gpu_masks(net, saved):
    from esr_hip import _lib
    from esr_hip.act import view_of
    _, ins = saved
    masks = []
    for k, t in enumerate(ins[1:]):
        ly, zg = net.engine.layers[k], net.engine.layers[k + 1].lat // 8
        out = torch.empty(t.shape[1], ly.cout, t.shape[3] - 2, t.shape[4] - 2, dtype=torch.float32, device=t.device)
        assert _lib.lib.esr_unpack_nchw(C.byref(view_of(t, zg)), t.shape[1], ly.cout, out.data_ptr(), _stream()) == 0
        masks.append((out > 0).cpu())
    return masks


@pytest.mark.parametrize('mode', ['all_layers', 'first_layer', 'None'])
def test_generator_against_float64_under_the_gpu_pattern(mode):
    g = golden()
    cpu = make_generator(mode)
    net = copy.deepcopy(cpu).to(DEV).eval()
    coef, Z = torch.from_numpy(g['b/coef']), torch.from_numpy(g['b/Z'])
    x = torch.cat([Z, coef], 1) if mode != 'None' else coef.clone()
    xg = x.to(DEV).requires_grad_(True)
    y = net.pre_output(xg)
    masks = _gpu_masks(net, y.grad_fn.saved)
    cot = seeded_uniform(tuple(y.shape), 4300, -1.0, 1.0)
    (y * cot.to(DEV)).sum().backward()
    net64 = copy.deepcopy(cpu).double().eval()
    x64 = x.double().requires_grad_(True)
    own = _oracle64(net64, x64.detach())
    y64 = _oracle64(net64, x64, masks)
    (y64 * cot.double()).sum().backward()
    flips = float((own - y64).detach().abs().max())
    e_y, e_g = rel_l2(y.detach().cpu().double(), y64.detach()), rel_l2(xg.grad.cpu().double(), x64.grad)
    print('%s: pre-sigmoid rel-L2 %.3g, input gradient rel-L2 %.3g (forcing the pattern moved the oracle by %.3g)' % (mode, e_y, e_g, flips))
    assert e_y < SPLIT_BAR and e_g < SPLIT_BAR
    # the graph-free pass (two ping-pong buffers) gives the same bits as the one that keeps every layer
    with torch.no_grad():
        assert torch.equal(net.pre_output(x.to(DEV)), y.detach())


@pytest.mark.parametrize('mode', ['all_layers', 'first_layer', 'None'])
def test_generator_and_extractor_match_the_fixture(mode):
    from JPEG_module.JPEG import JPEG
    g = golden()
    net = make_generator(mode).to(DEV).eval()
    ext = JPEG(False)
    ext.Set_Q_Table(torch.tensor(G.QF_B, dtype=torch.float32))
    coef, Z, r = (torch.from_numpy(g['b/' + k]).to(DEV) for k in ('coef', 'Z', 'r'))
    x = (torch.cat([Z, coef], 1) if mode != 'None' else coef.clone()).requires_grad_(True)
    fake = net(x)
    img = ext(fake)
    (img * r).sum().backward()
    for got, key in ((fake, 'out'), (img, 'img'), (x.grad, 'grad')):
        want = torch.from_numpy(g['b/%s/%s' % (mode, key)])
        err = rel_l2(got.detach().cpu().double(), want.double()) if key == 'grad' else float((got.detach().cpu() - want).abs().max() / want.abs().max())
        print('%s %s: %.3g' % (mode, key, err))
        assert err < SPLIT_BAR


def test_batchnorm_folding_follows_the_running_statistics():
    g = golden()
    net = make_generator('all_layers').to(DEV).eval()
    x = torch.cat([torch.from_numpy(g['b/Z']), torch.from_numpy(g['b/coef'])], 1).to(DEV)
    with torch.no_grad():
        before = net(x)
        net.dncnn[3].running_var.mul_(1.7)
        net.dncnn[6].running_mean.add_(0.2)
        after = net(x)
        want = net._torch_chain(x, False) - 0.5 + x[:, 64:]
    assert float((before - after).abs().max()) > 1e-3
    assert rel_l2(after.cpu().double(), want.cpu().double()) < SPLIT_BAR
    sd = make_generator('all_layers').state_dict()
    net.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(net(x), before)


def test_shipped_generator_shape_against_torch_on_the_gpu():
    """n_channels 320, depth 10, latent 64 at 16 x 32 x 32 blocks, once, against the stock modules on the same device"""
    import models.modules.architecture as arch
    net = G.fill_generator(arch.DnCNN(n_channels=320, depth=10, in_nc=64, out_nc=64, norm_type='batch', latent_input='all_layers',
                                      num_latent_channels=64, avoid_padding=False, output_layer='Sigmoid')).to(DEV).eval()
    x = torch.cat([seeded_uniform((16, 64, 32, 32), 4400, -1.0, 1.0), (seeded_uniform((16, 64, 32, 32), 4401, -8.0, 8.0)).round()], 1).to(DEV)
    torch.backends.cudnn.allow_tf32 = False
    xg = x.clone().requires_grad_(True)
    y = net.pre_output(xg)
    cot = seeded_uniform(tuple(y.shape), 4402, -1.0, 1.0).to(DEV)
    (y * cot).sum().backward()
    xt = x.clone().requires_grad_(True)
    yt = net._torch_chain(xt, True)
    (yt * cot).sum().backward()
    e_y, e_g = rel_l2(y.detach().cpu().double(), yt.detach().cpu().double()), rel_l2(xg.grad.cpu().double(), xt.grad.cpu().double())
    print('320 x 10: pre-sigmoid rel-L2 %.3g, input gradient rel-L2 %.3g against torch on the GPU (unforced pattern)' % (e_y, e_g))
    assert e_y < SPLIT_BAR
    assert e_g < 5e-2          # unforced: a flipped LeakyReLU branch among 5e6 activations moves this figure; the forced comparison above holds SPLIT_BAR


# ------------------------------------------------------------------------------------------------ model and Z search
def test_model_test_equals_the_composition_of_the_modules(tmp_path):
    from test_host_jpeg import make_model
    g = golden()
    model = make_model(tmp_path, gpu=True)
    assert model.device.type == 'cuda' and next(model.netG.parameters()).is_cuda
    x, Z, qf = G.image_b(), G.latent_b(), torch.tensor(G.QF_B, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)
    ties = G.tie_mask(G.compress64(x, torch.from_numpy(g['b/tables'])))
    assert torch.equal(model.var_Comp.cpu()[~ties], torch.from_numpy(g['b/coef'])[~ties])
    model.test()
    assert model.fake_H.shape == (2, 64, 6, 9) and model.output_image.shape == (2, 1, 48, 72)
    with torch.no_grad():
        fake = model.netG(model.model_input)                        # the module's own tail (torch sigmoid) behind the same engine
        img = model.JPEG['extractor'](fake)
    assert float((model.fake_H - fake).abs().max()) <= 1e-6         # expf in the kernel against torch.sigmoid
    assert float((model.output_image - img).abs().max()) <= 1e-6 * 255 * 64
    for got, key in ((model.fake_H, 'out'), (model.output_image, 'img')):
        want = torch.from_numpy(g['b/all_layers/' + key])
        assert float((got.cpu() - want).abs().max() / want.abs().max()) < SPLIT_BAR
    assert torch.equal(model.Output_Batch(True), torch.clamp(model.output_image / 255, 0, 1))
    assert float(model.Output_Batch(True).min()) >= 0 and float(model.Output_Batch(True).max()) <= 1
    assert model.Return_Compressed(x.to(DEV)).shape == x.shape


@pytest.mark.parametrize('objective', ['l1', 'TV'])
def test_z_search_history_matches_the_cpu_path(tmp_path, objective, monkeypatch):
    """six iterations; tolerance of tests/test_gpu_local_z.py for histories: rtol 1e-3, atol 1e-3 |loss[0]|.  The fixture holds no reference
    search (tools/gen_jpeg_golden.py (c)), so the comparison is with this build's CPU path."""
    from esr_hip import jpeg as J
    from test_host_jpeg import _search, make_model
    (tmp_path / 'gpu').mkdir()
    (tmp_path / 'cpu').mkdir()
    gpu_losses, gpu_Z = _search(make_model(tmp_path / 'gpu', gpu=True), objective)
    monkeypatch.undo()                                              # the CPU side of the comparison runs the CPU expressions
    cpu_losses, cpu_Z = _search(make_model(tmp_path / 'cpu'), objective)
    print('%s: GPU %s\n    CPU %s' % (objective, gpu_losses, cpu_losses))
    assert len(gpu_losses) == len(cpu_losses) == 6
    np.testing.assert_allclose(gpu_losses, cpu_losses, rtol=1e-3, atol=1e-3 * abs(cpu_losses[0]))
    assert gpu_losses[-1] < gpu_losses[0]
    assert float((gpu_Z.cpu() - cpu_Z).abs().max()) < 1e-2
