"""CPU tests of the colour (chroma) model of the explorable JPEG decoder against tests/golden/jpeg_chroma.npz (the reference's own JPEG module
with chroma_mode, its DnCNN generators and Tensor_YCbCR2RGB, written by tools/gen_jpeg_chroma_golden.py): tables, the 16-point CPU paths,
the refusals that stay and the calls that are now accepted, the options, the model in both feed_data flows, the C-ABI's argument checks and
the Z search through both generators.

Bounds, as in tests/test_host_jpeg.py.  The 16-point compressor / extractor run fp32 torch ops in another order than the reference, so each
is held to 4 x the reference's OWN distance from a float64 restatement on the same input (stored in the fixture, b/err/*).  The rounded chroma
planes must equal the reference exactly wherever the float64 pre-rounding value is more than 1e-3 from a half-integer; at most 1 % of them
may be excluded this way (the reference has 0 % on these inputs).  Model-level quantities pass through two fp32 transforms and two
generators before they are compared; their bound is MODEL_BAR below."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle.check_golden import rel_l2
from oracle.weights import seeded_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, 'tests', 'golden', 'jpeg_chroma.npz')
# Model level: the chroma generator's input differs from the reference's by the fp32 distance of the Y extractor and the 16-point compressor
# (b/err/*: < 4e-5 on 0...255 pixels, i.e. < 1e-5 of a coefficient after the division by a table entry >= 3), and the same fp32 torch modules
# then run on it.  1e-4 relative leaves a factor 10 for the generators' amplification and is a tenth of the GPU kernels' bar (1e-3).
MODEL_BAR = 1e-4


def _load_tool():
    spec = importlib.util.spec_from_file_location('gen_jpeg_chroma_golden', os.path.join(ROOT, 'tools', 'gen_jpeg_chroma_golden.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


C = _load_tool()              # inputs and the float64 restatement shared with the fixture's generator; C.Y: the Y model's tool
_golden = {}


def golden():
    if not _golden:
        with np.load(FX) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def gt(key):
    return torch.from_numpy(np.asarray(golden()[key]))


def chroma_modules(qf_or_table, QF=True):
    from JPEG_module.JPEG import JPEG
    ms = {'q': JPEG(True, True, chroma_mode=True, block_size=16), 'd': JPEG(True, 'downsample_only', chroma_mode=True, block_size=16),
          'a': JPEG(True, False, chroma_mode=True, block_size=16), 'e': JPEG(False, chroma_mode=True, block_size=16)}
    for m in ms.values():
        m.Set_Q_Table(qf_or_table, QF=QF)
    return ms


def make_generators(mode):
    import models.modules.architecture as arch
    return C.make_generators(arch, mode)


# ------------------------------------------------------------------------------------------------ the fixture's own conditions
def test_fixture_is_smaller_than_the_y_fixture_and_holds_its_conditions():
    g = golden()
    assert os.path.getsize(FX) < os.path.getsize(C.Y.GOLDEN)
    ties, _ = C.chroma_ties(C.compress64_16(C.image_b(), gt('b/tables')))
    assert ties <= C.TIE_CAP
    both = torch.cat([gt('c/all_layers/y_channel_input'), C.image_c()[:, 1:]], 1)
    ties, _ = C.chroma_ties(C.compress64_16(both, gt('c/tables')))
    assert ties <= C.TIE_CAP
    for mode in C.MODES:
        y = g['c/%s/y' % mode]
        sat = float((np.abs(y) > C.SATURATION).mean())
        print('%s: |y| > 6 on %.3f %%, median |y| %.3f, max %.3f' % (mode, 100 * sat, float(np.median(np.abs(y))), float(np.abs(y).max())))
        assert sat < C.SATURATION_CAP
    for name in ('compress', 'extract128', 'extract384', 'extract512'):
        assert 0 < g['b/err/' + name][0] < 1e-3          # an fp32 distance: the bounds below are 4 x these


# ------------------------------------------------------------------------------------------------ JPEG module
def test_tables_for_every_quality_factor_and_the_explicit_form():
    g = golden()
    ms = chroma_modules(torch.from_numpy(g['a/qf']))
    for m in ms.values():
        assert m.synthetic_padded_Q_table.shape == (1, 3, 16, 16, 1, 1) and m.synthetic_Q_table.shape == (1, 3, 8, 8, 1, 1)
        assert m.padded_Q_table.shape == (6, 3, 16, 16, 1, 1) and m.Q_table.shape == (6, 3, 8, 8, 1, 1)
        assert np.array_equal(m.padded_Q_table.reshape(6, 3, 256).numpy(), g['a/padded'])
        assert np.array_equal(m.Q_table.reshape(6, 3, 64).numpy(), g['a/q'])
    p = ms['q'].padded_Q_table
    assert torch.equal(p[:, 1], p[:, 2]) and float(p.min()) >= 1 and float(p.max()) <= 255
    assert torch.equal(p[:, :, 8:, :8], p[:, :, 7:8, :8].expand(-1, -1, 8, -1, -1, -1))          # edge padding
    ms = chroma_modules([g['a/explicit/lum'], g['a/explicit/chroma']], QF=False)
    assert ms['e'].padded_Q_table.shape == (1, 3, 16, 16, 1, 1) and ms['e'].Q_table.shape == (1, 3, 8, 8, 1, 1)
    assert np.array_equal(ms['e'].padded_Q_table.reshape(3, 256).numpy(), g['a/explicit/padded'])
    assert np.array_equal(ms['e'].Q_table.reshape(3, 64).numpy(), g['a/explicit/q'])
    assert ms['e'].QF == pytest.approx(float(g['a/explicit/qf']), rel=1e-12)


def test_compressor_and_extractor_cpu_paths():
    g = golden()
    x, tables = C.image_b(), gt('b/tables')
    ms = chroma_modules(torch.tensor(C.QF_B, dtype=torch.float32))
    assert torch.equal(ms['q'].padded_Q_table.reshape(3, 3, 256), tables)
    c64 = C.compress64_16(x, tables)
    share, ties = C.chroma_ties(c64)
    assert share <= C.TIE_CAP
    bound = 4 * float(g['b/err/compress'][0])
    ca, cd, cq = ms['a'](x), ms['d'](x), ms['q'](x)
    assert ca.shape == (3, 768, 2, 3) and cd.shape == (3, 384, 2, 3) and cq.shape == (3, 384, 2, 3)
    for got, mode, key in ((ca, False, 'ca'), (cd, 'downsample_only', 'cd')):
        err = float((got.double() - C.channels64_16(c64, mode)).abs().max())
        print('%s: CPU path %.3g from float64 (bound %.3g), %.3g from the reference' % (key, err, bound, float((got - gt('b/' + key)).abs().max())))
        assert err <= bound
    assert float((cq[:, :256].double() - C.channels64_16(c64, True)[:, :256]).abs().max()) <= bound       # Y: never rounded
    want = gt('b/cq')
    assert torch.equal(cq[:, 256:][~ties[:, 256:]], want[:, 256:][~ties[:, 256:]])
    inside = ties[:, 256:]
    low64 = C.channels64_16(c64, 'downsample_only')[:, 256:]
    assert bool(((cq[:, 256:][inside].double() == torch.floor(low64[inside])) | (cq[:, 256:][inside].double() == torch.ceil(low64[inside]))).all())
    assert torch.equal(cq[:, 256:], cq[:, 256:].round()) and not torch.equal(cd[:, 256:], cd[:, 256:].round())
    for form, src in ((128, want[:, 256:]), (384, want), (512, gt('b/ca')[:, 256:])):
        i64 = C.extract64_16(src, tables)
        img = ms['e'](src)
        assert img.shape == (3, 3 if form == 384 else 2, 32, 48)
        err, bound = float((img.double() - i64).abs().max()), 4 * float(g['b/err/extract%d' % form][0])
        print('extractor %d: CPU path %.3g from float64 (bound %.3g)' % (form, err, bound))
        assert err <= bound
    with pytest.raises(Exception, match='Unexpected input size'):
        ms['e'](torch.zeros(1, 64, 2, 2))


def test_explicit_table_case():
    g = golden()
    ms = chroma_modules([g['a/explicit/lum'], g['a/explicit/chroma']], QF=False)
    x = C.image_b()[:1]
    tables = gt('a/explicit/padded').view(1, 3, 256)
    c64 = C.compress64_16(x, tables)
    share, ties = C.chroma_ties(c64)
    assert share <= C.TIE_CAP
    cq, want = ms['q'](x), gt('b/explicit/cq')
    assert torch.equal(cq[:, 256:][~ties[:, 256:]], want[:, 256:][~ties[:, 256:]])
    assert float((cq[:, :256].double() - C.channels64_16(c64, True)[:, :256]).abs().max()) <= 4 * float(g['b/err/explicit/compress'][0])
    i64 = C.extract64_16(want, tables)
    assert float((ms['e'](want).double() - i64).abs().max()) <= 4 * float(g['b/err/explicit/extract384'][0])


def test_cpu_gradients_of_the_16_point_ops():
    """the adjoint identity <A x, g> = <x, A^T g> of every compressor mode and extractor form, and zero gradient into the rounded planes"""
    from esr_hip import jpeg as J
    tables = gt('b/tables')
    x0 = C.image_b()
    for mode, nc in ((False, 768), ('downsample_only', 384), (True, 384)):
        x = x0.clone().requires_grad_(True)
        gc = seeded_uniform((3, nc, 2, 3), 6400, -1.0, 1.0)
        (J.compress16(x, tables, mode) * gc).sum().backward()
        if mode is True:
            assert float(x.grad[:, 1:].abs().max()) == 0.0 and float(x.grad[:, :1].abs().max()) > 0
            continue
        d = seeded_uniform((3, 3, 32, 48), 6401, -1.0, 1.0)
        lin = J.compress16(d + torch.tensor([128., 0, 0]).view(1, 3, 1, 1), tables, mode)          # the linear part: shift removed
        lhs, rhs = float((lin.double() * gc.double()).sum()), float((d.double() * x.grad.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float(lin.double().norm() * gc.double().norm())
    for form in (128, 384, 512):
        c = seeded_uniform((3, form, 2, 3), 6402, -2.0, 2.0).requires_grad_(True)
        gi = seeded_uniform((3, 3 if form == 384 else 2, 32, 48), 6403, -1.0, 1.0)
        same, img = J.extract16(c, tables)
        (img * gi).sum().backward()
        d = seeded_uniform((3, form, 2, 3), 6404, -1.0, 1.0)
        lin = J.extract16(d, tables)[1] - (torch.tensor([128., 0, 0]).view(1, 3, 1, 1) if form == 384 else 0)
        lhs, rhs = float((lin.double() * gi.double()).sum()), float((d.double() * c.grad.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float(lin.double().norm() * gi.double().norm())
    # the generator's tail: c = coef[:, -128:] + sigmoid(y) - 0.5
    coef = seeded_uniform((3, 384, 2, 3), 6405, -4.0, 4.0).round().requires_grad_(True)
    y = seeded_uniform((3, 128, 2, 3), 6406, -3.0, 3.0).requires_grad_(True)
    c, img = J.extract16(coef, tables, y)
    assert torch.allclose(c, coef[:, 256:] + torch.sigmoid(y) - 0.5) and img.shape == (3, 2, 32, 48)
    gi = seeded_uniform((3, 2, 32, 48), 6407, -1.0, 1.0)
    (img * gi).sum().backward()
    s = torch.sigmoid(y.detach())
    assert float(coef.grad[:, :256].abs().max()) == 0.0
    assert torch.allclose(y.grad, coef.grad[:, 256:] * s * (1 - s), rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError):
        J.compress16(torch.zeros(1, 3, 24, 32), tables[:1], True)
    with pytest.raises(ValueError):
        J.compress16(torch.zeros(1, 1, 32, 32), tables[:1], True)
    with pytest.raises(ValueError):
        J.extract16(torch.zeros(2, 384, 2, 2), tables)          # three tables for two images


def test_pinned_refusals_stay_and_the_chroma_calls_are_accepted(tmp_path):
    from JPEG_module.JPEG import JPEG
    import models.modules.architecture as arch
    import models.networks as networks
    with pytest.raises(NotImplementedError, match='chroma_mode'):
        JPEG(compress=False, chroma_mode=True)                                   # chroma on 8x8 blocks
    with pytest.raises(NotImplementedError, match='block_size'):
        JPEG(compress=False, block_size=16)                                      # 16x16 blocks without chroma
    with pytest.raises(NotImplementedError, match='downsample_only'):
        JPEG(compress=True, downsample_or_quantize='downsample_only')
    with pytest.raises(NotImplementedError, match='chroma_generator'):
        arch.DnCNN(64, 5, chroma_generator=True)                                 # out_nc 64: the reference's block-size assert fails too
    assert JPEG(compress=False, chroma_mode=True, block_size=16).block_size == 16
    for mode in (True, False, 'downsample_only'):
        assert JPEG(compress=True, downsample_or_quantize=mode, chroma_mode=True, block_size=16).chroma_mode
    net = arch.DnCNN(64, 5, in_nc=384, out_nc=128, chroma_generator=True, latent_input='all_layers', num_latent_channels=64, output_layer='Sigmoid')
    assert net.chroma_generator and net.dncnn[0].in_channels == 448 and net.dncnn[-2].out_channels == 128
    opt = {'gpu_ids': None, 'is_train': False, 'scale': 16,
           'network_G': {'which_model_G': 'DnCNN', 'nf': 64, 'nb': 5, 'norm_type': 'batch', 'latent_input': 'all_layers', 'padding': 1, 'CEM_arch': 0}}
    net = networks.define_G(opt, num_latent_channels=64, chroma_mode=True)
    assert isinstance(net, arch.DnCNN) and net.chroma_generator and net.dncnn[0].in_channels == 16 ** 2 + 128 + 64 and net.dncnn[-2].out_channels == 128
    with pytest.raises(NotImplementedError, match='no_high_freq_chroma_reconstruction'):
        networks.define_G(opt, num_latent_channels=64, chroma_mode=True, no_high_freq_chroma_reconstruction=False)
    assert networks.define_G(opt, num_latent_channels=64).dncnn[0].in_channels == 128          # chroma_mode off: the Y generator, as before


@pytest.mark.parametrize('mode', ['all_layers', 'first_layer', 'None'])
def test_chroma_generator_cpu_path_and_state_dict(mode):
    g = golden()
    g_y, g_c = make_generators(mode)
    assert list(g_c.state_dict().keys()) == [str(k) for k in g['c/%s/keys' % mode]] == list(g_y.state_dict().keys())
    if mode != 'all_layers':
        return
    var_comp, Z = gt('c/all_layers/var_Comp'), C.latent_c()
    Zc = torch.nn.functional.interpolate(Z, size=[4, 6], mode='bilinear', align_corners=True)
    x = torch.cat([Zc, var_comp], 1).requires_grad_(True)
    ext = chroma_modules(torch.tensor(C.QF_C, dtype=torch.float32))['e']
    fake = g_c(x)
    assert fake.shape == (2, 128, 4, 6)
    # same fp32 torch modules as the reference on the same input: fp32 rounding of identical ops
    assert float((fake.detach() - gt('c/all_layers/fake_H')).abs().max()) <= 1e-5
    assert float((g_c._torch_chain(x, True).detach() - gt('c/all_layers/y')).abs().max()) <= 1e-5 * float(gt('c/all_layers/y').abs().max()) + 1e-5
    (ext(fake) * C.cotangent_c()).sum().backward()
    assert rel_l2(x.grad.double(), gt('c/all_layers/grad').double()) < 1e-5


def test_checkpoints_of_both_generators_load_positionally(tmp_path):
    src_y, src_c = make_generators('all_layers')
    ck_y, ck_c = str(tmp_path / 'Y_G.pth'), str(tmp_path / 'chroma_G.pth')
    torch.save({'module.' + k: v for k, v in src_y.state_dict().items()}, ck_y)
    torch.save({'module.' + k: v for k, v in src_c.state_dict().items()}, ck_c)
    model = make_model(tmp_path, fill=False, paths={'pretrained_model_G': ck_c, 'Y_channel_model_G': ck_y})
    for src, dst in ((src_y, model.netG_Y), (src_c, model.netG)):
        for (k, a), b in zip(src.state_dict().items(), dst.state_dict().values()):
            assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ C-ABI
def test_cabi_argument_checks_with_fake_pointers():
    """bad arguments come back as ESR_E_ARG / ESR_E_UNSUPPORTED before anything touches the device (include/esr_hip.h)"""
    from esr_hip import _lib
    from esr_hip._lib import ESR_E_ARG, ESR_E_UNSUPPORTED
    h = _lib.load_library()
    p, q = 0x1000, 0x2000
    assert h.esr_jpeg16_compress(None, 1, 16, 16, q, 2, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress(p, 1, 16, 16, None, 2, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress(p, 1, 16, 16, q, 2, None, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress(p, 1, 24, 16, q, 2, p, None) == ESR_E_ARG               # H not a multiple of 16
    assert h.esr_jpeg16_compress(p, 1, 16, 40, q, 2, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress(p, 0, 16, 16, q, 2, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress(p, 1, 16, 16, q, 3, p, None) == ESR_E_ARG               # no such mode
    assert h.esr_jpeg16_compress(p + 4, 1, 16, 16, q, 2, p, None) == ESR_E_ARG           # image not 16-byte aligned
    assert h.esr_jpeg16_compress(p, 21846, 16, 16, q, 2, p, None) == ESR_E_UNSUPPORTED   # B * 3 planes beyond the grid
    assert h.esr_jpeg16_extract(None, 128, 0, None, 128, 1, 1, 1, q, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 1, 1, 1, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 1, 0, 1, q, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 1, 1, 1, None, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_extract(p, 64, 0, None, 64, 1, 1, 1, q, None, p, None) == ESR_E_ARG            # no such form
    assert h.esr_jpeg16_extract(p, 384, 300, None, 128, 1, 1, 1, q, None, p, None) == ESR_E_ARG        # the slice leaves the tensor
    assert h.esr_jpeg16_extract(p, 384, 0, p, 384, 1, 1, 1, q, None, p, None) == ESR_E_ARG             # the tail belongs to form 128
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 1, 1, 1, q, p, p, None) == ESR_E_ARG             # coef_out without y
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 40000, 1, 1, q, None, p, None) == ESR_E_UNSUPPORTED
    assert h.esr_jpeg16_extract(p, 128, 0, None, 128, 1, 70000, 1, q, None, p, None) == ESR_E_UNSUPPORTED
    assert h.esr_jpeg16_extract_grad(None, None, 128, 1, 1, 1, q, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg16_extract_grad(p, None, 128, 1, 1, 1, q, None, None, None) == ESR_E_ARG          # no output
    assert h.esr_jpeg16_extract_grad(p, None, 128, 1, 1, 1, q, p, p, None) == ESR_E_ARG                # d_y without y
    assert h.esr_jpeg16_extract_grad(p, p, 384, 1, 1, 1, q, p, p, None) == ESR_E_ARG                   # d_y belongs to form 128
    assert h.esr_jpeg16_extract_grad(p, None, 100, 1, 1, 1, q, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress_grad(None, 0, 1, 1, 1, q, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress_grad(p, 0, 1, 1, 1, q, None, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress_grad(p, 0, 1, 1, -1, q, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress_grad(p, 5, 1, 1, 1, q, p, None) == ESR_E_ARG
    assert h.esr_jpeg16_compress_grad(p, 0, 1, 1, 1, q, p + 8, None) == ESR_E_ARG


# ------------------------------------------------------------------------------------------------ options, model, Z search
SETTINGS = {
    'name': 'jpeg_run', 'model': 'dncnn', 'gpu_ids': None, 'scale': 4,
    'datasets': {'test_1': {'name': 'set', 'mode': 'JPEG', 'dataroot_Uncomp': 'images/uncomp'}},
    'path': {'root': None, 'datasets': None, 'pretrained_model_G': None, 'Y_channel_model_G': None},
    'network_G': {'which_model_G': 'DnCNN', 'norm_type': 'batch', 'CEM_arch': 0, 'padding': 1, 'latent_input': 'all_layers',
                  'latent_channels': {'ModelY': 64, 'ModelChroma': 64}, 'nf': {'ModelY': 64, 'ModelChroma': 64}, 'nb': 5},
    'network_G_Y': {'nf': 64, 'nb': 5},
}


def _options(tmp_path, gpu=False, chroma=True, paths=None, **network_G):
    from options import options as option
    cfg = json.loads(json.dumps(SETTINGS))
    cfg['path']['root'] = str(tmp_path)
    cfg['path']['datasets'] = str(tmp_path / 'data')
    cfg['path'].update(paths or {})
    cfg['gpu_ids'] = [0] if gpu else None
    cfg['network_G'].update(network_G)
    path = str(tmp_path / 'test_JPEG.json')
    with open(path, 'w') as f:
        f.write('// settings written by the test\n' + json.dumps(cfg, indent=1))
    return option.dict_to_nonedict(option.parse(path, is_train=False, JPEG=True, chroma=chroma)), path


def make_model(tmp_path, gpu=False, fill=True, paths=None, **network_G):
    from models import create_model
    opt, _ = _options(tmp_path, gpu=gpu, paths=paths, **network_G)
    model = create_model(opt, chroma_mode=True)
    if fill:
        C.Y.fill_generator(model.netG)
        C.Y.fill_generator(model.netG_Y)
    return model


def test_options_parse_chroma(tmp_path):
    from options import options as option
    opt, path = _options(tmp_path)
    assert opt['scale'] == 16 and opt['input_downsampling'] == 2 and opt['name'] == os.path.join('JPEG', 'chroma_jpeg_run')
    assert opt['network_G']['latent_channels'] == 64 and opt['network_G']['scale'] == 16 and opt['network_G_Y']['nf'] == 64
    assert opt['datasets']['test_1']['mode'] == 'JPEG_chroma' and opt['datasets']['test_1']['input_downsampling'] == 2
    assert opt['datasets']['test_1']['scale'] == 16
    assert opt['path']['models'] == os.path.join(str(tmp_path), 'experiments', 'JPEG', 'chroma_jpeg_run', 'models')
    again = option.parse(path, is_train=False, JPEG=True, chroma=True)
    assert again['name'] == opt['name']
    y_opt, _ = _options(tmp_path, chroma=False)                                  # the same file still gives the Y model
    assert y_opt['scale'] == 8 and y_opt['name'] == os.path.join('JPEG', 'jpeg_run') and y_opt['datasets']['test_1']['mode'] == 'JPEG'
    # a latent count the chroma generator's first conv cannot take is refused where the options are read, by name
    for bad in (3, 8, 100):
        with pytest.raises(NotImplementedError, match=r'chroma.*latent_channels|latent_channels.*chroma') as e:
            _options(tmp_path, latent_channels={'ModelY': 64, 'ModelChroma': bad})
        assert '64' in str(e.value) and '128' in str(e.value)


def test_create_model_its_keys_and_its_refusals(tmp_path):
    from models import create_model
    from models.DecompCNN_model import DecompCNNModel
    model = make_model(tmp_path, nf={'ModelY': 64, 'ModelChroma': 128})          # network_G_Y overrides nf for the Y generator
    assert isinstance(model, DecompCNNModel) and model.chroma_mode and model.num_latent_channels == 64
    assert set(model.JPEG) == {'compressor', 'extractor', 'compressor_Y', 'extractor_Y', 'non_quantized_compressor_Y', 'non_quantized_compressor'}
    assert model.JPEG['compressor'].chroma_mode and model.JPEG['compressor'].block_size == 16 and model.JPEG['compressor'].downsample_or_quantize is True
    assert model.JPEG['non_quantized_compressor'].downsample_or_quantize == 'downsample_only' and model.JPEG['non_quantized_compressor'].chroma_mode
    assert not model.JPEG['compressor_Y'].chroma_mode and model.JPEG['non_quantized_compressor_Y'].downsample_or_quantize is False
    assert model.netG.chroma_generator and model.netG.dncnn[0].out_channels == 128 and model.netG.dncnn[0].in_channels == 448
    assert not model.netG_Y.chroma_generator and model.netG_Y.dncnn[0].out_channels == 64 and model.netG_Y.dncnn[0].in_channels == 128
    assert not model.netG.training and not model.netG_Y.training
    opt, _ = _options(tmp_path)
    with pytest.raises(NotImplementedError, match='chroma'):
        DecompCNNModel(opt)                                                      # chroma options without chroma_mode
    y_opt, _ = _options(tmp_path, chroma=False)
    with pytest.raises(NotImplementedError, match='chroma_mode'):
        DecompCNNModel(y_opt, chroma_mode=True)
    with pytest.raises(NotImplementedError, match='Enforce_pair_Consistency'):
        model.Enforce_pair_Consistency(None, None)
    opt['is_train'] = True
    with pytest.raises(NotImplementedError, match='is_train'):
        create_model(opt, chroma_mode=True)


def test_model_test_equals_the_fixtures_composition_in_both_flows(tmp_path):
    model = make_model(tmp_path)
    x, Z, qf = C.image_c(), C.latent_c(), torch.tensor(C.QF_C, dtype=torch.float32)
    kept = x.clone()
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)              # as test_JPEG.py feeds it
    assert torch.equal(x, kept)                                                  # the caller's image is left alone
    assert model.var_Comp.shape == (2, 384, 4, 6) and model.model_input.shape == (2, 448, 4, 6) and model.y_channel_input.shape == (2, 1, 64, 96)
    # Z resize: the Y grid's Z on the chroma grid, bilinear with aligned corners
    assert torch.equal(model.GetLatent(), torch.nn.functional.interpolate(Z, size=[4, 6], mode='bilinear', align_corners=True))
    assert torch.equal(model.GetLatent()[:, :, 0, 0], Z[:, :, 0, 0]) and torch.equal(model.GetLatent()[:, :, -1, -1], Z[:, :, -1, -1])
    model.test()
    assert model.fake_H.shape == (2, 128, 4, 6) and model.output_image.shape == (2, 3, 64, 96)
    first = {k: getattr(model, k).clone() for k in ('y_channel_input', 'var_Comp', 'fake_H', 'output_image')}
    share, ties = C.chroma_ties(C.compress64_16(torch.cat([gt('c/all_layers/y_channel_input'), x[:, 1:]], 1), gt('c/tables')))
    for key in ('y_channel_input', 'fake_H', 'output_image'):
        want = gt('c/all_layers/' + key)
        err = float((first[key] - want).abs().max() / want.abs().max())
        print('%s: %.3g of the largest value from the fixture' % (key, err))
        assert err < MODEL_BAR
    assert torch.equal(first['var_Comp'][:, 256:][~ties[:, 256:]], gt('c/all_layers/var_Comp')[:, 256:][~ties[:, 256:]])
    rgb = model.Output_Batch(True)
    assert rgb.shape == (2, 3, 64, 96) and float(rgb.min()) >= 0 and float(rgb.max()) <= 1
    assert float((rgb - gt('c/all_layers/rgb')).abs().max()) < MODEL_BAR
    assert model.Output_Batch(False) is model.output_image
    vis = model.get_current_visuals(need_Uncomp=False)
    assert list(vis) == ['Comp', 'Decomp'] and vis['Decomp'].shape == (3, 64, 96)
    # the composition of the modules, by hand
    with torch.no_grad():
        J = model.JPEG
        y_in = torch.clamp(J['extractor_Y'](model.netG_Y(torch.cat([Z, J['compressor_Y'](x[:, :1])], 1))), 0, 255)
        comp = J['compressor'](torch.cat([y_in, x[:, 1:]], 1))
        image = torch.cat([y_in, J['extractor'](model.netG(torch.cat([model.GetLatent(), comp], 1)))], 1)
    assert torch.equal(image, first['output_image'])
    # the GUI's flow: the Y coefficients as 'Comp', then test(uncompressed_chroma=...)
    coef_y = model.JPEG['compressor_Y'](x[:, :1])
    model.feed_data({'Comp': coef_y, 'QF': qf, 'Z': Z}, need_GT=False)
    assert model.var_Comp.shape == (2, 64, 8, 12) and torch.equal(model.GetLatent(), Z)
    model.test(uncompressed_chroma=x[:, 1:])
    for key, want in first.items():
        assert torch.equal(getattr(model, key), want), key
    model.feed_data({'Comp': coef_y[:1], 'QF': qf[:1], 'Z': Z[:1]}, need_GT=False)
    model.test(uncompressed_chroma=x[:1, 1:], chroma_Z=torch.zeros(1, 64, 4, 6))
    assert float((model.output_image[:, 1:] - first['output_image'][:1, 1:]).abs().max()) > 0          # chroma_Z replaces the resized Z
    assert float((model.output_image[:, :1] - first['output_image'][:1, :1]).abs().max()) < 255 * MODEL_BAR    # (a batch of 1: other conv blocking)
    with pytest.raises(ValueError, match='Z of size'):
        model.feed_data({'Uncomp': x, 'QF': qf, 'Z': torch.zeros(2, 64, 5, 7)}, need_GT=False)


def test_return_compressed_for_one_and_three_channels(tmp_path):
    model = make_model(tmp_path)
    x, qf = C.image_c(), torch.tensor(C.QF_C, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': 0.0}, need_GT=False)
    J = model.JPEG
    one = model.Return_Compressed(x[:, :1])
    assert one.shape == (2, 1, 64, 96) and torch.equal(one, J['extractor_Y'](J['compressor_Y'](x[:, :1])))
    three = model.Return_Compressed(x)
    assert three.shape == (2, 3, 64, 96)
    assert torch.equal(three, J['extractor'](J['compressor'](torch.cat([one, x[:, 1:]], 1))))
    # Y passes the 16-point pair unrounded: it comes back as the 8-point pair left it; the chroma planes lose what the rounding and
    # the truncation to 8x8 frequencies take
    assert float((three[:, :1] - one).abs().max()) < 1e-3 and float((three[:, 1:] - x[:, 1:]).abs().max()) > 1


def _search(model, objective, flow, iters=6, detach_Y=False, seed=6500):
    """six iterations on image 0 of the fixture's colour image, cropped to 32 x 48.  flow 'Uncomp': the colour image as test_JPEG.py feeds
    it; 'Comp': the Y coefficients plus data['uncompressed_chroma'], as the GUI does"""
    from Z_optimization import Z_optimizer
    from models.DecompCNN_model import Tensor_YCbCR2RGB
    x, qf = C.image_c()[:1, :, :32, :48].contiguous().to(model.device), torch.tensor(C.QF_C[:1], dtype=torch.float32).to(model.device)
    if flow == 'Uncomp':
        data = {'Uncomp': x, 'QF': qf}
    else:
        model.JPEG['compressor_Y'].Set_Q_Table(qf)
        data = {'Comp': model.JPEG['compressor_Y'](x[:, :1]), 'QF': qf, 'uncompressed_chroma': x[:, 1:].contiguous()}
    if objective == 'l1':
        data['desired'] = torch.clamp(Tensor_YCbCR2RGB(x / 255), 0, 1)
    Z0 = seeded_uniform((1, 64, 4, 6), seed, -0.5, 0.5).to(model.device)
    if detach_Y:
        real_test = model.test
        model.test = lambda *a, **k: real_test(*a, **dict(k, detach_Y=True)) if 'uncompressed_chroma' in k else real_test(*a, **k)
    model.feed_data({k: v for k, v in dict(data, Z=Z0).items() if k not in ('desired', 'uncompressed_chroma')}, need_GT=False)
    model.test(**({'uncompressed_chroma': data['uncompressed_chroma']} if flow == 'Comp' else {}))
    zo = Z_optimizer(objective, [4, 6], model, Z_range=1.0, max_iters=iters, data=data, initial_Z=Z0, initial_LR=0.05, batch_size=1,
                     jpeg_extractor=model.JPEG['extractor'])
    Z = zo.optimize()
    return zo.loss_values, Z


def test_z_gradient_runs_through_both_generators(tmp_path):
    model = make_model(tmp_path)
    x, qf = C.image_c()[:1, :, :32, :48].contiguous(), torch.tensor(C.QF_C[:1], dtype=torch.float32)
    comp_y = model.JPEG['compressor_Y']
    comp_y.Set_Q_Table(qf)
    grads = {}
    for detach in (False, True):
        Z = seeded_uniform((1, 64, 4, 6), 6500, -0.5, 0.5).requires_grad_(True)
        model.feed_data({'Comp': comp_y(x[:, :1]), 'QF': qf, 'Z': Z}, need_GT=False)
        model.test(prevent_grads_calc=False, uncompressed_chroma=x[:, 1:], detach_Y=detach)
        assert model.y_channel_input.requires_grad == (not detach)
        model.Output_Batch(True).mean().backward()
        grads[detach] = Z.grad.clone()
        # the colour image as 'Uncomp' with detach_Y passed to feed_data gives the same gradient
        Z2 = Z.detach().clone().requires_grad_(True)
        model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z2}, need_GT=False, detach_Y=detach)
        model.test(prevent_grads_calc=False)
        model.Output_Batch(True).mean().backward()
        assert torch.allclose(Z2.grad, grads[detach], rtol=1e-5, atol=1e-9)
    through_chroma, through_y = grads[True], grads[False] - grads[True]
    assert float(through_chroma.abs().max()) > 0 and float(through_y.abs().max()) > 1e-3 * float(grads[False].abs().max())


@pytest.mark.parametrize('objective', ['l1', 'TV'])
def test_z_search_on_a_colour_image_decreases_and_uses_both_generators(tmp_path, objective):
    losses, Z = _search(make_model(tmp_path), objective, 'Comp')
    assert Z.shape == (1, 64, 4, 6) and len(losses) >= 2 and np.all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    same, Z_same = _search(make_model(tmp_path), objective, 'Uncomp')            # the other feed_data flow: the same search
    np.testing.assert_allclose(same, losses, rtol=1e-5, atol=1e-8)
    frozen, _ = _search(make_model(tmp_path), objective, 'Comp', detach_Y=True)  # the Y generator's share of the gradient taken away
    assert frozen[0] == pytest.approx(losses[0], rel=1e-6)
    n = min(len(frozen), len(losses))
    assert n >= 2 and not np.allclose(frozen[1:n], losses[1:n], rtol=1e-4, atol=0)
