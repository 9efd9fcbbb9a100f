"""CPU tests of explorable JPEG decoding against tests/golden/jpeg_dncnn.npz (the reference's own JPEG module and DnCNN generator, written by
tools/gen_jpeg_golden.py): the package's CPU paths, state_dict parity, the refusals, the options, the model, the C-ABI's argument checks and
the Z search in JPEG mode.

Bounds.  The compressor / extractor / generator run the same fp32 torch ops as the reference in another order, so each is held to 4 x the
reference's OWN distance from a float64 restatement on the same input (computed here from the fixture).  The quantised compressor must equal
the reference exactly wherever the float64 pre-rounding value is more than 1e-3 from a half-integer (twenty times the reference's fp32 error:
an fp32 evaluation cannot flip anything outside that window); inside it, it must be one of the two neighbouring integers; at most 1 % of the
coefficients of any case may be excluded this way (the reference alone sits at 0.27 %)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle.check_golden import rel_l2
from oracle.weights import seeded_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, 'tests', 'golden', 'jpeg_dncnn.npz')


def _load_generator_script():
    spec = importlib.util.spec_from_file_location('gen_jpeg_golden', os.path.join(ROOT, 'tools', 'gen_jpeg_golden.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load_generator_script()          # inputs, BatchNorm fill and the float64 restatement shared with the fixture's generator
_golden = {}


def golden():
    if not _golden:
        with np.load(FX) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def make_generator(mode):
    import models.modules.architecture as arch
    return G.fill_generator(arch.DnCNN(n_channels=64, depth=5, in_nc=64, out_nc=64, norm_type='batch', latent_input=None if mode == 'None' else mode,
                                       num_latent_channels=64, avoid_padding=False, output_layer='Sigmoid')).eval()


def _modules(qf_or_table, QF=True):
    from JPEG_module.JPEG import JPEG
    ms = {'q': JPEG(compress=True, downsample_or_quantize=True), 'n': JPEG(compress=True, downsample_or_quantize=False), 'e': JPEG(compress=False)}
    for m in ms.values():
        m.Set_Q_Table(qf_or_table, QF=QF)
    return ms


# ------------------------------------------------------------------------------------------------ the fixture's own conditions
def test_fixture_inputs_are_the_seeded_ones_and_hold_their_conditions():
    g = golden()
    for name, x in G.images_a().items():
        assert np.array_equal(g['a/%s/x' % name], x.numpy().astype(np.uint8))
        ties = G.tie_mask(G.compress64(x, torch.from_numpy(g['a/tables'])))
        assert float(ties.double().mean()) <= G.TIE_CAP
    assert np.array_equal(g['b/x'], G.image_b().numpy().astype(np.uint8))
    assert np.array_equal(g['b/Z'], G.latent_b().numpy()) and np.array_equal(g['b/r'], G.cotangent_b().numpy())
    assert float(G.tie_mask(G.compress64(G.image_b(), torch.from_numpy(g['b/tables']))).double().mean()) <= G.TIE_CAP
    for mode in G.MODES:
        y = g['b/%s/y' % mode]
        sat = float((np.abs(y) > G.SATURATION).mean())
        print('%s: |y| > 6 on %.3f %%, median |y| %.3f, max %.3f' % (mode, 100 * sat, float(np.median(np.abs(y))), float(np.abs(y).max())))
        assert sat < G.SATURATION_CAP                  # no saturated sigmoid: the output layer's arithmetic is really exercised


# ------------------------------------------------------------------------------------------------ JPEG module
def test_tables_for_every_quality_factor_are_the_references():
    g = golden()
    ms = _modules(torch.from_numpy(g['a/qf']))
    assert ms['q'].Q_table.shape == (6, 8, 8, 1, 1)
    assert np.array_equal(ms['q'].Q_table.reshape(6, 64).numpy(), g['a/tables'])
    ms = _modules([g['a/explicit/table']], QF=False)
    assert np.array_equal(ms['e'].Q_table.reshape(64).numpy(), g['a/explicit/q_table'])
    assert ms['e'].QF == pytest.approx(float(g['a/explicit/qf']), rel=1e-12)


@pytest.mark.parametrize('name', ['noise', 'smooth'])
def test_compressor_and_extractor_cpu_paths(name):
    g = golden()
    tables = torch.from_numpy(g['a/tables'])
    x = torch.from_numpy(g['a/%s/x' % name]).float()
    ref = {k: torch.from_numpy(np.asarray(g['a/%s/%s' % (name, k)])).float() for k in ('cq', 'cn', 'img_q', 'img_n')}
    ms = _modules(torch.from_numpy(g['a/qf']))
    c64 = G.compress64(x, tables)
    ref_err = float((ref['cn'].double() - c64).abs().max())
    cn = ms['n'](x)
    assert cn.shape == (6, 64, 6, 8)
    assert float((cn.double() - c64).abs().max()) <= 4 * ref_err
    ties = G.tie_mask(c64)
    assert float(ties.double().mean()) <= G.TIE_CAP
    cq = ms['q'](x)
    assert torch.equal(cq[~ties], ref['cq'][~ties])
    assert bool(((cq[ties].double() == torch.floor(c64[ties])) | (cq[ties].double() == torch.ceil(c64[ties]))).all())
    for key in ('q', 'n'):
        i64 = G.extract64(ref['c' + key], tables)
        ref_err = float((ref['img_' + key].double() - i64).abs().max())
        img = ms['e'](ref['c' + key])
        assert img.shape == (6, 1, 48, 64)
        assert float((img.double() - i64).abs().max()) <= 4 * ref_err
    assert torch.equal(ms['e'].Multiply_By_Q_table(ref['cq']), ref['cq'] * tables.view(6, 64, 1, 1))


def test_explicit_table_case():
    g = golden()
    ms = _modules([g['a/explicit/table']], QF=False)
    x = G.images_a()['smooth'][:1]
    q = torch.from_numpy(g['a/explicit/q_table']).view(1, 64)
    c64 = G.compress64(x, q)
    ties = G.tie_mask(c64)
    cq, want = ms['q'](x), torch.from_numpy(g['a/explicit/cq'])
    assert torch.equal(cq[~ties], want[~ties])
    i64 = G.extract64(want, q)
    ref_err = float((torch.from_numpy(g['a/explicit/img_q']).double() - i64).abs().max())
    assert float((ms['e'](want).double() - i64).abs().max()) <= 4 * ref_err


def test_cpu_gradients_of_the_jpeg_ops():
    from esr_hip import jpeg as J
    tables = torch.from_numpy(golden()['b/tables'])
    x = G.image_b().requires_grad_(True)
    d_coef = seeded_uniform((2, 64, 6, 9), 5100, -1.0, 1.0)
    (J.compress(x, tables, False) * d_coef).sum().backward()
    q = tables.double().view(2, 64, 1, 1)
    assert rel_l2(x.grad.double(), G.extract64(d_coef.double() / (q * q), tables) - 128) < 1e-5
    xq = G.image_b().requires_grad_(True)
    J.compress(xq, tables, True).sum().backward()
    assert float(xq.grad.abs().max()) == 0.0
    with pytest.raises(ValueError):
        J.compress(torch.zeros(1, 1, 12, 16), tables[:1], True)
    with pytest.raises(ValueError):
        J.extract(torch.zeros(3, 64, 2, 2), tables)


def test_jpeg_refusals_by_name():
    from JPEG_module.JPEG import JPEG
    with pytest.raises(NotImplementedError, match='chroma_mode'):
        JPEG(compress=False, chroma_mode=True)
    with pytest.raises(NotImplementedError, match='block_size'):
        JPEG(compress=False, block_size=16)
    with pytest.raises(NotImplementedError, match='downsample_only'):
        JPEG(compress=True, downsample_or_quantize='downsample_only')


# ------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize('mode', ['all_layers', 'first_layer', 'None'])
def test_generator_cpu_path_and_state_dict(mode):
    from JPEG_module.JPEG import JPEG
    g = golden()
    net = make_generator(mode)
    assert list(net.state_dict().keys()) == [str(k) for k in g['b/%s/keys' % mode]]
    ext = JPEG(False)
    ext.Set_Q_Table(torch.tensor(G.QF_B, dtype=torch.float32))
    coef, Z, r = (torch.from_numpy(g['b/' + k]) for k in ('coef', 'Z', 'r'))
    x = (torch.cat([Z, coef], 1) if mode != 'None' else coef.clone()).requires_grad_(True)
    fake = net(x)
    img = ext(fake)
    (img * r).sum().backward()
    # same fp32 torch modules as the reference, same order: the generator's part agrees to fp32 rounding of identical ops
    assert float((fake.detach() - torch.from_numpy(g['b/%s/out' % mode])).abs().max()) <= 1e-5
    i64 = G.extract64(torch.from_numpy(g['b/%s/out' % mode]), torch.from_numpy(g['b/tables']))
    ref_err = float((torch.from_numpy(g['b/%s/img' % mode]).double() - i64).abs().max())
    assert float((img.detach().double() - i64).abs().max()) <= 4 * ref_err + 1e-5 * float(torch.from_numpy(g['b/tables']).max())
    assert rel_l2(x.grad.double(), torch.from_numpy(g['b/%s/grad' % mode]).double()) < 1e-5


def test_reference_style_checkpoint_loads_positionally(tmp_path):
    """BaseModel.load_network matches tensors by position: a checkpoint with the reference's DataParallel key prefix loads"""
    from models.base_model import BaseModel
    src, dst = make_generator('all_layers'), make_generator('all_layers')
    with torch.no_grad():
        for p in dst.parameters():
            p.zero_()
    path = str(tmp_path / 'G.pth')
    torch.save({'module.' + k: v for k, v in src.state_dict().items()}, path)
    loader = BaseModel.__new__(BaseModel)
    loader.opt = {'network_G': {'CEM_arch': 0}}
    loader.load_network(path, dst, strict=True)
    for (k, a), b in zip(src.state_dict().items(), dst.state_dict().values()):
        assert torch.equal(a, b), k


def test_generator_refusals_by_name():
    import models.modules.architecture as arch
    import models.networks as networks
    from esr_hip import EsrError
    with pytest.raises(NotImplementedError, match='discriminator'):
        arch.DnCNN(64, 5, discriminator=True, expected_input_size=16)
    with pytest.raises(NotImplementedError, match='chroma_generator'):
        arch.DnCNN(64, 5, chroma_generator=True)
    for norm in ('layer', 'instance'):
        with pytest.raises(NotImplementedError, match='norm_type'):
            arch.DnCNN(64, 5, norm_type=norm)
    with pytest.raises(NotImplementedError, match='"padding": 1'):
        arch.DnCNN(64, 5, avoid_padding=True)
    with pytest.raises(EsrError, match='conv 0 of 5'):
        arch.DnCNN(64, 5, latent_input='all_layers', num_latent_channels=8)          # 72 input channels
    with pytest.raises(EsrError, match='multiple of 8'):
        arch.DnCNN(64, 5, latent_input='all_layers', num_latent_channels=3)
    with pytest.raises(EsrError, match='conv 0 of 4'):
        arch.DnCNN(100, 4)
    arch.DnCNN(320, 10, latent_input='all_layers', num_latent_channels=64)           # the shipped configuration: 128 / 384 / 320
    opt = {'gpu_ids': None, 'is_train': False, 'scale': 8,
           'network_G': {'which_model_G': 'DnCNN', 'nf': 64, 'nb': 5, 'norm_type': 'batch', 'latent_input': 'all_layers', 'padding': 1, 'CEM_arch': 0}}
    net = networks.define_G(opt, num_latent_channels=64)
    assert isinstance(net, arch.DnCNN) and isinstance(net.dncnn[-1], torch.nn.Sigmoid) and net.dncnn[0].in_channels == 128
    opt['network_G']['padding'] = None
    with pytest.raises(NotImplementedError, match='"padding": 1'):
        networks.define_G(opt, num_latent_channels=64)
    for which in ('sr_resnet', 'MSRResNet'):
        opt['network_G']['which_model_G'] = which
        with pytest.raises(NotImplementedError):
            networks.define_G(opt, num_latent_channels=64)
    with pytest.raises(NotImplementedError, match='DnCNN_D'):
        networks.define_D({'network_D': {'which_model_D': 'DnCNN_D', 'pre_clipping': 0, 'decomposed_input': 0}, 'datasets': {'train': {'patch_size': 64}}})


# ------------------------------------------------------------------------------------------------ C-ABI
def test_cabi_argument_checks_with_fake_pointers():
    """bad arguments come back as ESR_E_ARG before anything touches the device (include/esr_hip.h)"""
    from esr_hip import _lib
    from esr_hip._lib import ActView, ESR_E_ARG, ESR_E_UNSUPPORTED
    h = _lib.load_library()
    p, q = 0x1000, 0x2000
    assert h.esr_jpeg_compress(None, 1, 8, 8, q, 1, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg_compress(p, 1, 8, 8, None, 1, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg_compress(p, 1, 8, 8, q, 1, None, None, None) == ESR_E_ARG          # neither destination
    assert h.esr_jpeg_compress(p, 1, 12, 8, q, 1, p, None, None) == ESR_E_ARG            # H not a multiple of 8
    assert h.esr_jpeg_compress(p, 1, 8, 20, q, 1, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg_compress(p, 0, 8, 8, q, 1, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg_compress(p + 4, 1, 8, 8, q, 1, p, None, None) == ESR_E_ARG         # image not 16-byte aligned
    assert h.esr_jpeg_compress(p, 70000, 8, 8, q, 1, p, None, None) == ESR_E_UNSUPPORTED
    small = ActView(p, None, 4, 1, 1, 9, 9, 0)
    assert h.esr_jpeg_compress(p, 1, 8, 8, q, 1, p, small, None) == ESR_E_ARG            # fewer than 8 groups
    wrong = ActView(p, None, 8, 2, 1, 12, 12, 0)
    assert h.esr_jpeg_compress(p, 1, 8, 8, q, 1, p, wrong, None) == ESR_E_ARG            # view of another size
    assert h.esr_jpeg_extract(None, None, 1, 1, 1, q, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg_extract(p, None, 1, 1, 1, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg_extract(p, None, 1, 0, 1, q, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg_extract(p, None, 1, 1, 1, None, None, p, None) == ESR_E_ARG
    assert h.esr_jpeg_extract(p, None, 1, 70000, 1, q, None, p, None) == ESR_E_UNSUPPORTED
    assert h.esr_jpeg_extract_grad(None, None, 1, 1, 1, q, p, None, None) == ESR_E_ARG
    assert h.esr_jpeg_extract_grad(p, None, 1, 1, 1, q, None, None, None) == ESR_E_ARG   # no output
    assert h.esr_jpeg_extract_grad(p, None, 1, 1, 1, q, p, p, None) == ESR_E_ARG         # d_y without y
    assert h.esr_jpeg_compress_grad(None, 1, 1, 1, q, p, None) == ESR_E_ARG
    assert h.esr_jpeg_compress_grad(p, 1, 1, 1, q, None, None) == ESR_E_ARG
    assert h.esr_jpeg_compress_grad(p, 1, 1, -1, q, p, None) == ESR_E_ARG


# ------------------------------------------------------------------------------------------------ options, model, Z search
SETTINGS = {
    'name': 'jpeg_run', 'model': 'dncnn', 'gpu_ids': None, 'scale': 4,
    'datasets': {'test_1': {'name': 'set', 'mode': 'JPEG', 'dataroot_Uncomp': 'images/uncomp'}},
    'path': {'root': None, 'datasets': None, 'pretrained_model_G': None},
    'network_G': {'which_model_G': 'DnCNN', 'norm_type': 'batch', 'CEM_arch': 0, 'padding': 1, 'latent_input': 'all_layers',
                  'latent_channels': {'ModelY': 64, 'ModelChroma': 3}, 'nf': {'ModelY': 64, 'ModelChroma': 128}, 'nb': 5},
}


def _options(tmp_path, gpu=False, **network_G):
    from options import options as option
    cfg = json.loads(json.dumps(SETTINGS))
    cfg['path']['root'] = str(tmp_path)
    cfg['path']['datasets'] = str(tmp_path / 'data')
    cfg['gpu_ids'] = [0] if gpu else None
    cfg['network_G'].update(network_G)
    path = str(tmp_path / 'test_JPEG.json')
    with open(path, 'w') as f:
        f.write('// settings written by the test\n' + json.dumps(cfg, indent=1))
    return option.dict_to_nonedict(option.parse(path, is_train=False, JPEG=True)), path


def make_model(tmp_path, gpu=False, **network_G):
    from models import create_model
    opt, _ = _options(tmp_path, gpu=gpu, **network_G)
    model = create_model(opt)
    G.fill_generator(model.netG)
    return model


def test_options_parse_jpeg(tmp_path):
    from options import options as option
    opt, path = _options(tmp_path)
    assert opt['scale'] == 8 and opt['input_downsampling'] == 1 and opt['name'] == os.path.join('JPEG', 'jpeg_run')
    assert opt['network_G']['residual'] == 1 and opt['network_G']['latent_channels'] == 64 and opt['network_G']['nf'] == 64
    assert opt['network_G']['scale'] == 8 and opt['is_train'] is False
    assert opt['datasets']['test_1']['dataroot_Uncomp'] == os.path.join(str(tmp_path), 'data', 'images/uncomp')
    assert opt['path']['models'] == os.path.join(str(tmp_path), 'experiments', 'JPEG', 'jpeg_run', 'models')
    with pytest.raises(NotImplementedError, match='chroma'):
        option.parse(path, is_train=False, JPEG=True, chroma=True)


def test_create_model_and_its_refusals(tmp_path):
    from models import create_model
    from models.DecompCNN_model import DecompCNNModel
    model = make_model(tmp_path)
    assert isinstance(model, DecompCNNModel) and model.num_latent_channels == 64 and model.device == torch.device('cpu')
    assert set(model.JPEG) == {'compressor', 'extractor', 'non_quantized_compressor'}
    assert not model.netG.training
    opt, _ = _options(tmp_path)
    with pytest.raises(NotImplementedError, match='chroma_mode'):
        DecompCNNModel(opt, chroma_mode=True)
    opt['is_train'] = True
    with pytest.raises(NotImplementedError, match='is_train'):
        create_model(opt)
    with pytest.raises(NotImplementedError, match='Enforce_pair_Consistency'):
        model.Enforce_pair_Consistency(None, None)
    opt, _ = _options(tmp_path, padding=0)
    with pytest.raises(NotImplementedError, match='"padding": 1'):
        create_model(opt)


def test_model_loads_pretrained_generator(tmp_path):
    from models import create_model
    src = make_generator('all_layers')
    ckpt = str(tmp_path / 'ref_G.pth')
    torch.save({'module.' + k: v for k, v in src.state_dict().items()}, ckpt)
    opt, _ = _options(tmp_path)
    opt['path']['pretrained_model_G'] = ckpt
    model = create_model(opt)
    for (k, a), b in zip(src.state_dict().items(), model.netG.state_dict().values()):
        assert torch.equal(a, b), k


def test_model_test_equals_the_composition_and_the_fixture(tmp_path):
    g = golden()
    model = make_model(tmp_path)
    x, Z, qf = G.image_b(), G.latent_b(), torch.tensor(G.QF_B, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)
    assert torch.equal(model.var_Comp, torch.from_numpy(g['b/coef']))               # (b) has 0.014 % near-ties; none flips on this path
    assert torch.equal(model.GetLatent(), Z)
    model.test()
    assert float((model.fake_H - torch.from_numpy(g['b/all_layers/out'])).abs().max()) <= 1e-5
    assert torch.equal(model.output_image, model.JPEG['extractor'](model.netG(torch.cat([Z, model.JPEG['compressor'](x)], 1))).detach())
    assert torch.equal(model.Output_Batch(True), torch.clamp(model.output_image / 255, 0, 1)) and model.Output_Batch(False) is model.output_image
    vis = model.get_current_visuals(need_Uncomp=False)
    assert list(vis) == ['Comp', 'Decomp'] and vis['Decomp'].shape == (1, 48, 72)
    # re-compressing the output gives the input's coefficients back wherever the estimate stays clear of +-0.5: the consistency the model is about
    back = model.JPEG['compressor'](model.output_image)
    clear = (model.fake_H - model.var_Comp).abs() < 0.499
    assert torch.equal(back[clear], model.var_Comp[clear]) and float(clear.float().mean()) > 0.99
    assert model.Return_Compressed(x).shape == x.shape
    # Z broadcasting (reference :361-366): a scalar, a [B, C, 1, 1] tensor; 'Comp' in place of 'Uncomp'
    model.feed_data({'Comp': model.var_Comp.clone(), 'QF': qf, 'Z': 0.25}, need_GT=False)
    assert model.model_input.shape == (2, 128, 6, 9) and float((model.GetLatent() - 0.25).abs().max()) == 0
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z[:, :, :1, :1]}, need_GT=False)
    assert torch.equal(model.GetLatent(), Z[:, :, :1, :1].expand(2, 64, 6, 9))


def _search(model, objective, iters=6, batch=2, seed=5200):
    from Z_optimization import Z_optimizer
    from esr_hip import dist as esr_dist
    x, qf = G.image_b()[:batch], torch.tensor(G.QF_B, dtype=torch.float32)[:batch]
    data = {'Uncomp': x.to(model.device), 'QF': qf.to(model.device)}
    if objective == 'l1':
        data['desired'] = (x / 255).to(model.device)
    Z0 = seeded_uniform((batch, 64, 6, 9), seed, -0.5, 0.5).to(model.device)
    lo, hi = esr_dist.shard_range(batch)          # the model holds this rank's share of the batch when the search is built
    model.feed_data({k: v[lo:hi] for k, v in dict(data, Z=Z0).items() if k != 'desired'}, need_GT=False)
    model.test()
    zo = Z_optimizer(objective, [6, 9], model, Z_range=1.0, max_iters=iters, data=data, initial_Z=Z0, initial_LR=0.05, batch_size=batch,
                     jpeg_extractor=model.JPEG['extractor'])
    Z = zo.optimize()
    return zo.loss_values, Z


@pytest.mark.parametrize('objective', ['l1', 'TV', 'max_STD', 'min_STD', 'STD_increase', 'STD_decrease'])
def test_z_search_in_jpeg_mode_decreases_without_touching_fake_H(tmp_path, objective):
    model = make_model(tmp_path)
    real_test = model.test

    def test_then_hide(*a, **k):
        real_test(*a, **k)
        model.fake_H = None                       # the six objectives read the image only: coefficients in fake_H would be a silent mistake
    model.test = test_then_hide
    losses, Z = _search(model, objective)
    assert Z.shape == (2, 64, 6, 9) and len(losses) >= 1 and np.all(np.isfinite(losses))
    if objective in ('l1', 'TV', 'min_STD', 'max_STD'):
        assert len(losses) == 1 or losses[-1] < losses[0]


def test_z_search_refusals_in_jpeg_mode(tmp_path):
    from Z_optimization import Z_optimizer
    model = make_model(tmp_path)
    for objective in ('hist', 'VGG', 'random_l1', 'scribble', 'local_STD_increase', 'periodicity'):
        with pytest.raises(NotImplementedError, match='JPEG mode'):
            Z_optimizer(objective, [6, 9], model, Z_range=1.0, max_iters=2, data={}, initial_LR=0.1, jpeg_extractor=model.JPEG['extractor'])


def _rank_search(rank, world, port, tmp, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import pathlib
        model = make_model(pathlib.Path(tmp) / ('rank%d' % rank))
        losses, Z = _search(model, 'TV', iters=4)
        torch.save({'loss': losses, 'Z': Z}, os.path.join(out, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_search_equals_the_one_rank_run(tmp_path):
    import socket
    import torch.multiprocessing as mp
    (tmp_path / 'rank0').mkdir()
    (tmp_path / 'rank1').mkdir()
    (tmp_path / 'one').mkdir()
    losses, Z = _search(make_model(tmp_path / 'one'), 'TV', iters=4)
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_search, args=(2, port, str(tmp_path), str(tmp_path)), nprocs=2, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r)) for r in range(2)]
    np.testing.assert_allclose(parts[0]['loss'], losses, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(parts[1]['loss'], losses, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(torch.cat([p['Z'] for p in parts]).numpy(), Z.numpy(), rtol=1e-4, atol=1e-5)
