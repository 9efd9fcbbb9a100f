"""GPU tests (-m gpu) of the colour (chroma) model of the explorable JPEG decoder: the 16-point block-DCT kernels (csrc/esr_jpeg16.hip,
esr_hip/jpeg.py, JPEG_module/JPEG.py with chroma_mode), the chroma DnCNN generator on the conv kernels, DecompCNNModel(chroma_mode=True) and
the Z search through both generators.

Conventions of tests/test_gpu_jpeg.py.  A kernel's bound is 4 x the REFERENCE's own fp32 distance from a float64 restatement of the transform
(tests/golden/jpeg_chroma.npz, b/err/*, measured by tools/gen_jpeg_chroma_golden.py).  The shapes here are not the fixture's, so the reference's
RELATIVE distance (to the largest value of the result) is used: the transforms are linear and the inputs are drawn alike, so the error scales
with the magnitude of the result.  Rounded planes are compared exactly outside a 1e-3 window around rounding ties in float64 (at most 1 % of
them inside).  The CPU fallbacks are patched to raise, so a silent fallback cannot pass.

Shapes (h x w blocks of 16 x 16 pixels): 'one' a single block; 'ragged' w = 19 — not a multiple of 4, so the scalar tail of the 16-byte path,
and one workgroup tile of 16 blocks plus a remainder of 3 — with h = 2 and three images of different QF (10, 40, 80); 'vector' w = 20, the
16-byte path with a partial second tile; 'explicit' the two-table form."""
import copy
import ctypes as C_

import numpy as np
import pytest
import torch

from oracle.check_golden import rel_l2
from oracle.weights import seeded_uniform
from test_host_jpeg_chroma import C, chroma_modules, golden, gt, make_generators

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SPLIT_BAR = 1e-3          # the generator tests' relative bar (tests/test_gpu_jpeg.py)
SHAPES = {'one': (1, 1, 1, [25]), 'ragged': (3, 2, 19, [10, 40, 80]), 'vector': (2, 2, 20, [30, 75]), 'explicit': (1, 2, 4, None)}


@pytest.fixture(autouse=True)
def no_cpu_fallback(monkeypatch):
    from esr_hip import jpeg as J

    def refuse(*a, **k):
        raise AssertionError('the CPU fallback ran in a GPU test')
    for name in ('_compress_cpu', '_extract_cpu', '_compress16_cpu', '_extract16_cpu'):
        monkeypatch.setattr(J, name, refuse)


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


_cases = {}


def _case(name):
    """(x [B, 3, 16h, 16w] YCbCr, padded tables [B, 3, 256], float64 coefficients [B, 3, 16, 16, h, w]) — computed once per shape"""
    if name not in _cases:
        B, h, w, qf = SHAPES[name]
        x = C.ycbcr_pattern(B, 16 * h, 16 * w, 7100 + 100 * len(_cases))
        if qf is None:
            tables = gt('a/explicit/padded').view(1, 3, 256)
        else:
            tables = chroma_modules(torch.tensor(qf, dtype=torch.float32))['q'].padded_Q_table.reshape(B, 3, 256)
        _cases[name] = (x, tables, C.compress64_16(x, tables))
    return _cases[name]


def _rel(*names):
    g = golden()
    return 4 * max(float(g['b/err/' + n][1]) for n in names)


@pytest.mark.parametrize('name', list(SHAPES))
def test_compressor_modes_against_float64(name):
    from esr_hip import jpeg as J
    x, tables, c64 = _case(name)
    xg, tg = x.to(DEV), tables.to(DEV)
    share, ties = C.chroma_ties(c64)
    assert share <= C.TIE_CAP
    for mode in (False, 'downsample_only', True):
        want = C.channels64_16(c64, mode)
        got = J.compress16(xg, tg, mode)
        assert got.shape == want.shape
        assert torch.equal(got, J.compress16(xg, tg, mode))                             # two calls, equal bits
        got = got.cpu()
        bound = _rel('compress') * float(want.abs().max())
        if mode is True:
            err = float((got[:, :256].double() - want[:, :256]).abs().max())            # Y: never rounded
            low, low64 = got[:, 256:], C.channels64_16(c64, 'downsample_only')[:, 256:]
            t = ties[:, 256:]
            assert torch.equal(low[~t].double(), want[:, 256:][~t])
            assert bool(((low[t].double() == torch.floor(low64[t])) | (low[t].double() == torch.ceil(low64[t]))).all())
        else:
            err = float((got.double() - want).abs().max())
        print('%s compressor %r: kernel %.3g (bound %.3g)' % (name, mode, err, bound))
        assert err <= bound


@pytest.mark.parametrize('name', list(SHAPES))
def test_extractor_forms_against_float64(name):
    from esr_hip import jpeg as J
    x, tables, c64 = _case(name)
    tg = tables.to(DEV)
    full, low = C.channels64_16(c64, False).float(), C.channels64_16(c64, True).float()
    for form, src in ((128, low[:, 256:]), (384, low), (512, full[:, 256:])):
        src = src.contiguous()
        i64 = C.extract64_16(src, tables)
        same, img = J.extract16(src.to(DEV), tg)
        assert img.shape == i64.shape and torch.equal(same.cpu(), src)
        err = float((img.cpu().double() - i64).abs().max())
        bound = _rel('extract%d' % form) * float((i64 - (128 if form == 384 else 0)).abs().max())
        print('%s extractor %d: kernel %.3g (bound %.3g)' % (name, form, err, bound))
        assert err <= bound
        assert torch.equal(img, J.extract16(src.to(DEV), tg)[1])


def test_unaligned_coefficient_pointers_take_the_scalar_path_and_give_the_same_bits():
    """w = 20 would take the 16-byte path; a coefficient pointer 4 bytes off a 16-byte boundary must fall back, in both directions"""
    from esr_hip import _lib, jpeg as J
    x, tables, c64 = _case('vector')
    B, h, w = x.size(0), x.size(2) // 16, x.size(3) // 16
    xg, tg = x.to(DEV), tables.to(DEV)
    aligned = J.compress16(xg, tg, True)
    buf = torch.zeros(aligned.numel() + 1, device=DEV)
    off = buf[1:].view(aligned.shape)
    assert off.data_ptr() % 16 == 4
    assert _lib.lib.esr_jpeg16_compress(xg.data_ptr(), B, 16 * h, 16 * w, tg.data_ptr(), 2, off.data_ptr(), _stream()) == 0
    assert torch.equal(off, aligned) and float(buf[0]) == 0.0
    for form in (128, 384):
        src = aligned[:, 384 - form:].contiguous()
        buf = torch.zeros(src.numel() + 1, device=DEV)
        buf[1:].copy_(src.reshape(-1))
        off = buf[1:].view(src.shape)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert torch.equal(J.extract16(off, tg)[1], J.extract16(src, tg)[1])
    # the slice of a wider tensor, read in place: channel 256 of 384 with the chroma generator's tail
    y = seeded_uniform((B, 128, h, w), 7300, -3.0, 3.0).to(DEV)
    c_a, img_a = J.extract16(aligned, tg, y)
    c_b, img_b = J.extract16(aligned[:, 256:].contiguous(), tg, y)
    assert torch.equal(c_a, c_b) and torch.equal(img_a, img_b)


@pytest.mark.parametrize('name', ['ragged', 'vector'])
def test_adjoint_kernels(name):
    """every compressor mode's and extractor form's input gradient against float64 autograd through the restatement, <A x, g> = <x, A^T g>
    with both sides from the kernels, the tail's d_y, and zero gradient into the rounded planes"""
    from esr_hip import jpeg as J
    x, tables, c64 = _case(name)
    B, h, w = x.size(0), x.size(2) // 16, x.size(3) // 16
    tg = tables.to(DEV)
    rel = _rel('compress', 'extract128', 'extract384', 'extract512')
    shift = torch.tensor([128., 0, 0]).view(1, 3, 1, 1)
    for mode, nc in ((False, 768), ('downsample_only', 384), (True, 384)):
        gc = seeded_uniform((B, nc, h, w), 7400, -1.0, 1.0)
        xg = x.to(DEV).requires_grad_(True)
        (J.compress16(xg, tg, mode) * gc.to(DEV)).sum().backward()
        x64 = x.double().requires_grad_(True)
        (C.channels64_16(C.compress64_16(x64, tables), mode) * gc.double()).sum().backward()
        err = float((xg.grad.cpu().double() - x64.grad).abs().max())
        print('%s d_x, mode %r: kernel %.3g (bound %.3g)' % (name, mode, err, rel * float(x64.grad.abs().max())))
        assert err <= rel * float(x64.grad.abs().max())
        if mode is True:
            assert float(xg.grad[:, 1:].abs().max()) == 0.0 and float(xg.grad[:, :1].abs().max()) > 0      # rounded planes: zero
            continue
        d = seeded_uniform((B, 3, 16 * h, 16 * w), 7401, -1.0, 1.0)
        lin = J.compress16((d + shift).to(DEV), tg, mode).cpu().double()
        lhs, rhs = float((lin * gc.double()).sum()), float((d.double() * xg.grad.cpu().double()).sum())
        assert abs(lhs - rhs) <= rel * float(lin.norm() * gc.double().norm())
    for form in (128, 384, 512):
        n = 3 if form == 384 else 2
        c = seeded_uniform((B, form, h, w), 7402, -2.0, 2.0)
        gi = seeded_uniform((B, n, 16 * h, 16 * w), 7403, -1.0, 1.0)
        cg = c.to(DEV).requires_grad_(True)
        (J.extract16(cg, tg)[1] * gi.to(DEV)).sum().backward()
        c64_ = c.double().requires_grad_(True)
        (C.extract64_16(c64_, tables) * gi.double()).sum().backward()
        err = float((cg.grad.cpu().double() - c64_.grad).abs().max())
        print('%s d_coef, form %d: kernel %.3g (bound %.3g)' % (name, form, err, rel * float(c64_.grad.abs().max())))
        assert err <= rel * float(c64_.grad.abs().max())
        d = seeded_uniform((B, form, h, w), 7404, -1.0, 1.0)
        lin = J.extract16(d.to(DEV), tg)[1].cpu().double() - (shift.double() if n == 3 else 0)
        lhs, rhs = float((lin * gi.double()).sum()), float((d.double() * cg.grad.cpu().double()).sum())
        assert abs(lhs - rhs) <= rel * float(lin.norm() * gi.double().norm())
    # the chroma generator's tail in front of the extractor: c = coef[:, 256:] + sigmoid(y) - 0.5
    coef = C.channels64_16(c64, True).float()
    y = seeded_uniform((B, 128, h, w), 7405, -3.0, 3.0)
    gi = seeded_uniform((B, 2, 16 * h, 16 * w), 7406, -1.0, 1.0)
    cg, yg = coef.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    c_out, img = J.extract16(cg, tg, yg)
    s = torch.sigmoid(y.double())
    c_want = coef[:, 256:].double() + s - 0.5
    assert float((c_out.detach().cpu().double() - c_want).abs().max()) < 1e-5 * max(1.0, float(c_want.abs().max()))
    i64 = C.extract64_16(c_want, tables)
    assert float((img.detach().cpu().double() - i64).abs().max()) <= rel * float(i64.abs().max())
    (img * gi.to(DEV)).sum().backward()
    cw = c_want.clone().requires_grad_(True)
    (C.extract64_16(cw, tables) * gi.double()).sum().backward()
    assert float(cg.grad[:, :256].abs().max()) == 0.0
    for got, want, what in ((cg.grad[:, 256:], cw.grad, 'd_coef'), (yg.grad, cw.grad * s * (1 - s), 'd_y')):
        err = float((got.cpu().double() - want).abs().max())
        print('%s tail %s: kernel %.3g (bound %.3g)' % (name, what, err, rel * float(want.abs().max())))
        assert err <= rel * float(want.abs().max())


def test_jpeg_module_on_the_gpu_matches_the_fixture():
    g = golden()
    ms = chroma_modules(torch.tensor(C.QF_B, dtype=torch.float32).to(DEV))
    x, tables = C.image_b(), gt('b/tables')
    assert torch.equal(ms['q'].padded_Q_table.reshape(3, 3, 256).cpu(), tables)
    _, ties = C.chroma_ties(C.compress64_16(x, tables))
    cq = ms['q'](x.to(DEV)).cpu()
    assert torch.equal(cq[:, 256:][~ties[:, 256:]], gt('b/cq')[:, 256:][~ties[:, 256:]])
    for key, m in (('ca', 'a'), ('cd', 'd')):
        assert float((ms[m](x.to(DEV)).cpu() - gt('b/' + key)).abs().max()) <= 5 * float(g['b/err/compress'][0])      # 4 x + the reference's own
    for form, src in ((128, gt('b/cq')[:, 256:]), (384, gt('b/cq')), (512, gt('b/ca')[:, 256:])):
        img = ms['e'](src.contiguous().to(DEV)).cpu()
        assert float((img - gt('b/img%d' % form)).abs().max()) <= 5 * float(g['b/err/extract%d' % form][0])
    with pytest.raises(Exception, match='Unexpected input size'):
        ms['e'](torch.zeros(1, 64, 2, 2, device=DEV))


# ------------------------------------------------------------------------------------------------ chroma generator
@pytest.mark.parametrize('mode', ['all_layers', 'first_layer', 'None'])
def test_chroma_generator_against_float64_under_the_gpu_pattern(mode):
    from test_gpu_jpeg import _gpu_masks, _oracle64
    _, cpu = make_generators(mode)
    net = copy.deepcopy(cpu).to(DEV).eval()
    var_comp = gt('c/all_layers/var_Comp')
    Zc = torch.nn.functional.interpolate(C.latent_c(), size=[4, 6], mode='bilinear', align_corners=True)
    x = torch.cat([Zc, var_comp], 1) if mode != 'None' else var_comp.clone()
    xg = x.to(DEV).requires_grad_(True)
    y = net.pre_output(xg)
    assert y.shape == (2, 128, 4, 6)
    masks = _gpu_masks(net, y.grad_fn.saved)
    cot = seeded_uniform(tuple(y.shape), 7500, -1.0, 1.0)
    (y * cot.to(DEV)).sum().backward()
    net64 = copy.deepcopy(cpu).double().eval()
    x64 = x.double().requires_grad_(True)
    own = _oracle64(net64, x64.detach())
    y64 = _oracle64(net64, x64, masks)
    (y64 * cot.double()).sum().backward()
    e_y, e_g = rel_l2(y.detach().cpu().double(), y64.detach()), rel_l2(xg.grad.cpu().double(), x64.grad)
    print('%s: pre-sigmoid rel-L2 %.3g, input gradient rel-L2 %.3g (forcing the pattern moved the oracle by %.3g); |y| > 6 on %.3f %%' % (
        mode, e_y, e_g, float((own - y64).detach().abs().max()), 100 * float((y64.detach().abs() > C.SATURATION).double().mean())))
    assert float((y64.detach().abs() > C.SATURATION).double().mean()) < C.SATURATION_CAP
    assert e_y < SPLIT_BAR and e_g < SPLIT_BAR
    with torch.no_grad():
        assert torch.equal(net.pre_output(x.to(DEV)), y.detach())
        # the module's forward: the 128 low chroma coefficients + sigmoid - 0.5
        out = net(x.to(DEV))
    want = x[:, -128:].double() + torch.sigmoid(y64.detach()) - 0.5
    assert out.shape == (2, 128, 4, 6) and float((out.cpu().double() - want).abs().max() / want.abs().max()) < SPLIT_BAR


# ------------------------------------------------------------------------------------------------ model and Z search
def test_model_test_equals_the_composition_of_the_modules(tmp_path):
    from test_host_jpeg_chroma import make_model
    model = make_model(tmp_path, gpu=True)
    assert model.device.type == 'cuda' and next(model.netG.parameters()).is_cuda and next(model.netG_Y.parameters()).is_cuda
    x, Z, qf = C.image_c(), C.latent_c(), torch.tensor(C.QF_C, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)
    model.test()
    assert model.fake_H.shape == (2, 128, 4, 6) and model.output_image.shape == (2, 3, 64, 96) and model.output_image.is_cuda
    with torch.no_grad():
        J = model.JPEG
        fake_y = model.netG_Y(torch.cat([Z.to(DEV), J['compressor_Y'](x[:, :1].to(DEV))], 1))     # the modules' own tails (torch sigmoid)
        y_in = torch.clamp(J['extractor_Y'](fake_y), 0, 255)
        fake = model.netG(model.model_input)
        chroma = J['extractor'](fake)
    assert float((model.y_channel_input - y_in).abs().max()) <= 1e-6 * 255 * 64          # the Y model's tolerances (tests/test_gpu_jpeg.py)
    assert float((model.fake_H - fake).abs().max()) <= 1e-6
    assert float((model.output_image[:, 1:] - chroma).abs().max()) <= 1e-6 * 255 * 64
    for key in ('y_channel_input', 'fake_H', 'output_image'):
        want = gt('c/all_layers/' + key)
        err = float((getattr(model, key).cpu() - want).abs().max() / want.abs().max())
        print('%s: %.3g of the largest value from the fixture' % (key, err))
        assert err < SPLIT_BAR
    rgb = model.Output_Batch(True)
    assert float(rgb.min()) >= 0 and float(rgb.max()) <= 1 and float((rgb.cpu() - gt('c/all_layers/rgb')).abs().max()) < SPLIT_BAR
    first = model.output_image.clone()
    model.feed_data({'Comp': J['compressor_Y'](x[:, :1].to(DEV)), 'QF': qf, 'Z': Z}, need_GT=False)
    model.test(uncompressed_chroma=x[:, 1:])
    assert torch.equal(model.output_image, first)
    assert model.Return_Compressed(x.to(DEV)).shape == x.shape and model.Return_Compressed(x[:, :1].to(DEV)).shape == (2, 1, 64, 96)


@pytest.mark.parametrize('objective', ['l1', 'TV'])
def test_z_search_history_matches_the_cpu_path(tmp_path, objective, monkeypatch):
    """six iterations; rtol 1e-3, atol 1e-3 |loss[0]|, as for the Y model.  The fixture holds no reference search
    (tools/gen_jpeg_chroma_golden.py (d)), so the comparison is with this build's CPU path."""
    from test_host_jpeg_chroma import _search, make_model
    (tmp_path / 'gpu').mkdir()
    (tmp_path / 'cpu').mkdir()
    gpu_losses, gpu_Z = _search(make_model(tmp_path / 'gpu', gpu=True), objective, 'Comp')
    monkeypatch.undo()                                              # the CPU side of the comparison runs the CPU expressions
    cpu_losses, cpu_Z = _search(make_model(tmp_path / 'cpu'), objective, 'Comp')
    print('%s: GPU %s\n    CPU %s' % (objective, gpu_losses, cpu_losses))
    assert len(gpu_losses) == len(cpu_losses) == 6
    np.testing.assert_allclose(gpu_losses, cpu_losses, rtol=1e-3, atol=1e-3 * abs(cpu_losses[0]))
    assert gpu_losses[-1] < gpu_losses[0]
    assert float((gpu_Z.cpu() - cpu_Z).abs().max()) < 1e-2
