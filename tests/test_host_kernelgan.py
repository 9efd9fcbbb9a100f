"""Kernel estimation (the KernelGAN package) on the host: the 'stock' engine, the learner, the data maps and the post-processing against
what the reference's own classes computed (tests/golden/kernelgan.npz: G_chan = D_chan = 8, a seeded initialisation, three consecutive
train() calls on recorded crops and recorded noise, the third with lambda_centralized = 1 and lambda_sparse = 5).

Every step is compared FROM THE REFERENCE'S STATE: parameters and power-iteration vectors are loaded from the fixture before each half
step, so no test compares trajectories (Adam's first steps are +-lr whatever the gradient's size: one sign of a near-zero gradient would
move a parameter by 4e-4).

Bars, per tensor as max|a - b| / max|b|.  The recorded values are fp32 results.  Losses, curr_k and u / v are short sums (at most a few
thousand fp32 terms of similar size): 1e-5, some 150 fp32 roundings.  Gradients are sums of up to 3 * 26 * 26 products behind BatchNorm's
subtraction of two means: n * eps = 1.2e-4 for the worst ordering, times a cancellation factor of some 10: 1e-3.  The bars hold for the
fp32 engine (the same operations) and for the fp64 engine (whose distance from the record is the record's own rounding).  The conv biases
in front of a BatchNorm (the first layer's too: no activation separates it from the next conv) have an analytically zero gradient (the mean is subtracted): both sides hold rounding noise there,
and those tensors are only required to be small: below 1e-3 of the largest gradient element of the critic (the noise of a sum of 400
cancelling fp32 terms is some 1e-5 of it)."""
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kernelgan.npz')
DEAD_BIASES = ['first_layer.bias'] + ['feature_block.%d.bias' % i for i in (0, 3, 6, 9, 12)]


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def small_conf(chan=8, crop=64, extra=()):
    from KernelGAN.configs import Config
    return Config().parse(['--G_chan', str(chan), '--D_chan', str(chan), '--input_crop_size', str(crop)] + list(extra))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def load_state(module, golden, prefix):
    sd = {k[len(prefix) + 1:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(prefix + '/')}
    assert sd
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected and all('running' in m or 'num_batches' in m for m in missing), (missing, unexpected)


@pytest.mark.parametrize('dtype,composed', [(torch.float32, False), (torch.float32, True), (torch.float64, False), (torch.float64, True)])
def test_stock_engine_reproduces_the_recorded_iterations(golden, dtype, composed):
    from KernelGAN.kernelGAN import StockEngine
    eng = StockEngine(small_conf(), 'cpu', dtype, composed)
    assert eng.d_input_shape == 26 and eng.d_output_shape == 20
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    for it in range(3):
        load_state(eng.G, golden, 's0/G' if it == 0 else 'it%d/G_after' % (it - 1))
        load_state(eng.D, golden, 's0/D' if it == 0 else 'it%d/D_after' % (it - 1))
        eng.lambdas = dict(zip(('bicubic', 'sum2one', 'boundaries', 'centralized', 'sparse'), golden['it%d/lambdas' % it].tolist()))
        g_in, d_in, noise = t(golden['it%d/g_in' % it]), t(golden['it%d/d_in' % it]), t(golden['it%d/noise' % it])
        eng.train_g(g_in, update=False)
        assert abs(float(eng.loss_g) - float(golden['it%d/loss_g' % it])) < 1e-5 * float(golden['it%d/loss_g' % it])
        assert abs(float(eng.loss_bicubic) - float(golden['it%d/loss_bicubic' % it])) < 1e-5 * float(golden['it%d/loss_bicubic' % it])
        assert rel(eng.curr_k, golden['it%d/curr_k' % it]) < 1e-5
        for i, m in enumerate(eng.G.layers()):
            assert rel(m.weight.grad, golden['it%d/G_grad/%d' % (it, i)]) < 1e-3, (it, i)
        for n, b in eng.D.named_buffers():
            if n.endswith('_u') or n.endswith('_v'):
                assert rel(b, golden['it%d/D_mid/%s' % (it, n)]) < 1e-5, (it, n)
        load_state(eng.G, golden, 'it%d/G_after' % it)
        eng.train_d(g_in, d_in, noise, update=False)
        assert abs(float(eng.loss_d_fake) - float(golden['it%d/loss_d_fake' % it])) < 1e-5
        assert abs(float(eng.loss_d_real) - float(golden['it%d/loss_d_real' % it])) < 1e-5
        gmax = max(float(np.abs(golden['it%d/D_grad/%s' % (it, n)]).max()) for n, _ in eng.D.named_parameters())
        for n, p in eng.D.named_parameters():
            ref = golden['it%d/D_grad/%s' % (it, n)]
            if n in DEAD_BIASES:
                assert float(p.grad.abs().max()) < 1e-3 * gmax and float(np.abs(ref).max()) < 1e-3 * gmax, (it, n)
            else:
                assert rel(p.grad, ref) < 1e-3, (it, n)
        for n, b in eng.D.named_buffers():
            if n.endswith('_u') or n.endswith('_v'):
                assert rel(b, golden['it%d/D_after/%s' % (it, n)]) < 1e-5, (it, n)


def test_optimizer_steps_move_the_parameters_like_the_record(golden):
    """One full train() from the initial state: Adam's first step is lr * sign(gradient), so every parameter moves by at most lr (1e-7 of slack) and the
    elements whose recorded gradient is not tiny land where the record says."""
    from KernelGAN.kernelGAN import StockEngine
    eng = StockEngine(small_conf(), 'cpu', torch.float32, False)
    load_state(eng.G, golden, 's0/G')
    load_state(eng.D, golden, 's0/D')
    t = lambda a: torch.from_numpy(np.asarray(a))
    eng.train(t(golden['it0/g_in']), t(golden['it0/d_in']), t(golden['it0/noise']))
    for i, m in enumerate(eng.G.layers()):
        before, after, g = golden['s0/G/' + ['first_layer', 'feature_block.0', 'feature_block.1', 'feature_block.2', 'feature_block.3', 'final_layer'][i] + '.weight'], \
            m.weight.detach().numpy(), golden['it0/G_grad/%d' % i]
        assert np.abs(after - before).max() <= 2e-4 + 1e-7
        big = np.abs(g) > 1e-3 * np.abs(g).max()
        assert np.abs(after - (before - 2e-4 * np.sign(g)))[big].max() < 1e-6


@pytest.mark.parametrize('dtype,bar', [(torch.float32, 1e-5), (torch.float64, 1e-13)])
def test_composed_kernel_forward_equals_the_layers(golden, dtype, bar):
    """G(x) = (x corr curr_k)[::2, ::2]: the same module run both ways, on a 64 x 64 crop and on a 16 x 18 one (2 x 3 outputs).  The two differ by
    the reassociation of sums of 169 (composed) against 49 + 8 * 25 + ... (layers) terms: 1e-5 in fp32, 1e-13 in fp64."""
    from KernelGAN import networks
    G = networks.Generator(small_conf())
    load_state(G, golden, 's0/G')
    G = G.to(dtype)
    for x in (torch.from_numpy(golden['it0/g_in']).to(dtype), torch.from_numpy(golden['it1/g_in'][:, :, 4:20, 6:24].copy()).to(dtype)):
        a, b = G(x, composed=True), G(x, composed=False)
        assert a.shape == b.shape == (1, 3, (x.shape[2] - 12) // 2, (x.shape[3] - 12) // 2)
        assert rel(a.detach(), b.detach()) < bar
    k = G.curr_k()
    assert k.shape == (13, 13) and rel(k.detach(), golden['it0/curr_k']) < 1e-5


def test_bicubic_table_and_penalty_mask(golden):
    from KernelGAN import util
    b = util.bicubic_table()
    assert b[3, 3] == 0.43359375 ** 2 and b[3, 2] == 0.43359375 * 0.11328125             # exact dyadic numbers
    assert abs(b.sum() - 1) < 1e-15
    assert np.abs(b - golden['bicubic_table']).max() < 1e-9       # upstream's table is the same numbers typed with 16 digits and stored in fp32
    assert np.abs(util.create_penalty_mask(13, 30) - golden['penalty_mask']).max() < 1e-12


def test_post_processing_against_the_record(golden):
    from KernelGAN import util
    k2 = util.post_process_k(torch.from_numpy(golden['post/k_in']), n=40)
    assert k2.shape == golden['post/k_x2'].shape and np.abs(k2 - golden['post/k_x2']).max() < 1e-12
    k4 = util.analytic_kernel(k2)
    assert k4.shape == golden['post/k_x4'].shape and np.abs(k4 - golden['post/k_x4']).max() < 1e-12
    from scipy.ndimage import center_of_mass
    assert np.abs(np.array(center_of_mass(k2)) - util.wanted_center(k2.shape, 2)).max() < 0.05     # (spline shifting moves the mass a little)


def test_data_maps_and_corners_against_the_record(golden):
    from KernelGAN.data import DataGenerator
    conf = small_conf(8, 32, ['--max_iters', '40'])
    conf.LR_image = golden['data/image']
    np.random.seed(5)
    dg = DataGenerator(conf, types.SimpleNamespace(d_input_shape=10))
    assert tuple(dg.input_image.shape) == tuple(golden['data/shape'])
    big, sml = dg.create_prob_maps(0.5)
    # float64 maps that sum to 1; the record's small map went through a float32 image on its way (PIL's nearest-neighbour resize)
    assert rel(big, golden['data/prob_big']) < 1e-12 and abs(big.sum() - 1) < 1e-12
    assert rel(sml, golden['data/prob_sml']) < 1e-6
    # the corners follow from the drawn centres; with the record's centres they are the record's corners
    dg.crop_indices_for_g, dg.crop_indices_for_d = golden['data/idx_g'], golden['data/idx_d']
    tab = dg.corner_table()
    assert tab.dtype == np.int32 and (tab % 2 == 0).all()
    assert (tab[:, :2] == golden['data/tl_g']).all() and (tab[:, 2:] == golden['data/tl_d']).all()
    g_in, d_in = dg[3]
    assert g_in.shape == (1, 3, 32, 32) and d_in.shape == (1, 3, 10, 10) and float(g_in.abs().max()) <= 1
    # the real crop's noise stays out of the image (the intended divergence from the reference's in-place add)
    before = dg.input_image.copy()
    dg.next_crop(False, 0)
    assert (dg.input_image == before).all()


def test_learner_schedule_and_its_200_iteration_replay():
    """A hand-written loss sequence: above 0.4 until iteration 150 (with two short dips that must not count), below from then on."""
    from KernelGAN.learner import Learner
    loss = lambda i: 0.3 if (i >= 150 or i in (40, 41, 90)) else 0.5
    gan = types.SimpleNamespace(lambda_bicubic=5., lambda_centralized=0., lambda_sparse=0., loss_bicubic=0.,
                                optimizer_G=types.SimpleNamespace(param_groups=[{'lr': 2e-4}]), optimizer_D=types.SimpleNamespace(param_groups=[{'lr': 2e-4}]))
    a, trace = Learner(), {}
    for i in range(3000):
        gan.loss_bicubic = loss(i)
        a.update(i, gan)
        trace[i] = (gan.lambda_bicubic, gan.lambda_centralized, gan.lambda_sparse, gan.optimizer_G.param_groups[0]['lr'])
    assert trace[151][0] == 5. and a.similar_to_bicubic
    assert trace[199][:3] == (5., 0., 0.) and trace[200][:3] == (0.05, 0., 0.)
    assert trace[400][:3] == (5e-4, 1, 5) and trace[600][0] == pytest.approx(5e-6) and trace[800][0] == pytest.approx(5e-6)
    assert trace[749][3] == 2e-4 and trace[750][3] == pytest.approx(2e-5) and trace[2250][3] == pytest.approx(2e-7)
    # the replay: 200 recorded losses at a time, read when the iteration is a multiple of 200 — the same decisions at the same iterations
    b, lambdas = Learner(), dict(bicubic=5., sum2one=0.5, boundaries=0.5, centralized=0., sparse=0.)
    for i in range(3000):
        if i and i % 200 == 0:
            slots = {j % 200: loss(j) for j in range(i - 199, i + 1)}                     # what the device log holds: slot = iteration % 200
            changed = b.replay(i, [slots[s] for s in list(range(1, 200)) + [0]], lambdas)
            assert changed == (trace[i][:3] != trace[i - 1][:3])
        if i % 200 == 0:
            assert (lambdas['bicubic'], lambdas['centralized'], lambdas['sparse']) == pytest.approx(trace[i][:3])
    assert [i for i in range(1, 3000) if b.lr_falls(i)] == [750, 1500, 2250]


def test_config_parse_leaves_no_directory_behind(tmp_path, monkeypatch):
    from KernelGAN import train as KernelGAN
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('CUDA_VISIBLE_DEVICES', '')
    conf = KernelGAN.Config().parse(['--X4', '--input_image_path', 'some/folder/real_photo_.png'])
    assert os.listdir(tmp_path) == [] and os.environ['CUDA_VISIBLE_DEVICES'] == ''
    assert conf.X4 and conf.G_structure == [7, 5, 3, 1, 1, 1] and (conf.input_crop_size, conf.G_chan, conf.D_chan, conf.G_kernel_size) == (64, 64, 64, 13)
    assert (conf.D_n_layers, conf.D_kernel_size, conf.max_iters, conf.g_lr, conf.d_lr, conf.beta1, conf.n_filtering) == (7, 7, 3000, 2e-4, 2e-4, 0.5, 40)
    assert conf.scale_factor == 0.5 and conf.real_image is False and conf.img_name == '_photo'


def test_estimated_kernels_round_trip_through_lr_dataset(tmp_path):
    """tools/estimate_kernels.py's writer puts <name>_kernel_x4.mat where LRDataset(kernel='estimated') looks, under both naming rules."""
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location('estimate_kernels', os.path.join(ROOT, 'tools', 'estimate_kernels.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.RandomState(0)
    names = ['img_7.png', 'photo.png']
    for n in names:
        Image.fromarray(rng.randint(0, 255, (12, 10, 3), dtype=np.uint8)).save(str(tmp_path / n))
    assert os.path.basename(tool.kernel_path(str(tmp_path / 'img_7.png'), 4)) == 'kernel__7_x4.mat'
    assert os.path.basename(tool.kernel_path(str(tmp_path / 'photo.png'), 4)) == 'photo_kernel_x4.mat'
    kernels = {n: rng.rand(33, 33) for n in names}
    for n in names:
        tool.write_kernel(str(tmp_path / n), kernels[n], 4)
    assert sorted(tool.image_files(str(tmp_path))) == sorted(str(tmp_path / n) for n in names)           # the .mat files are not taken for images
    from data.LR_dataset import LRDataset
    ds = LRDataset({'data_type': 'img', 'dataroot_LR': str(tmp_path)}, kernel='estimated')
    assert len(ds) == 2
    for i in range(2):
        item = ds[i]
        assert (item['kernel'] == kernels[os.path.basename(item['LR_path'])]).all()


def test_refusals_by_name():
    from esr_hip import EsrError
    from KernelGAN.kernelGAN import KernelGAN
    with pytest.raises(EsrError, match='no CPU fallback'):
        KernelGAN(small_conf(), engine='hip', device='cpu')
    with pytest.raises(ValueError, match="'hip' or 'stock'"):
        KernelGAN(small_conf(), engine='triton')
    from KernelGAN.data import DataGenerator
    conf = small_conf()
    conf.LR_image = np.zeros((70, 70, 3), dtype=np.uint8)             # 50 x 50 after the shave: no 64-pixel crop fits
    with pytest.raises(ValueError, match='smaller than one 64-pixel crop'):
        DataGenerator(conf, types.SimpleNamespace(d_input_shape=26))


def test_entry_points_refuse_before_touching_the_device():
    """Argument checks come first, so they answer on a machine without a GPU: ESR_E_ARG for NULL pointers / E < 1, ESR_E_UNSUPPORTED for shapes."""
    from esr_hip import _lib
    L = _lib.load_library()
    one = 64                                                             # any non-NULL address: it is never dereferenced on these paths
    assert L.esr_kgan_d_param_count(64) == 148 * 64 + 5 * (64 * 64 + 3 * 64) + 65 and L.esr_kgan_d_uv_count(8) == 12 * 8 + 148
    assert L.esr_kgan_d_param_count(12) == _lib.ESR_E_UNSUPPORTED and L.esr_kgan_d_param_count(72) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_apply_blocks(64, 64) == 3 and L.esr_kgan_apply_blocks(12, 64) == _lib.ESR_E_UNSUPPORTED and L.esr_kgan_apply_blocks(15, 16) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_compose(None, one, one, 1, 8, 8, 7, 5, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_compose(one, one, one, 0, 8, 8, 7, 5, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_compose(one, one, one, 1, 8, 8, 11, 5, None) == _lib.ESR_E_UNSUPPORTED          # would compose to 15 x 15
    assert L.esr_kgan_compose_bwd(one, one, one, one, one, 1, 72, 8, 7, 5, None) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_apply(one, one, one, None, one, None, one, one, 1, 12, 12, None) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_apply(one, one, one, None, one, None, None, one, 1, 64, 64, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_dk(one, None, None, None, None, one, 1, 64, 64, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_constraints(one, one, one, one, one, 3, 2028, one, one, 200, 200, 1, None) == _lib.ESR_E_ARG      # slot outside the log
    assert L.esr_kgan_gather(one, one, one, None, one, 70000, 64, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_d_spectral(one, one, one, one, one, 1, 12, 1, None) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_d_spectral(one, one, one, one, one, 1, 8, 3, None) == _lib.ESR_E_ARG
    args = (one, one, one, one, one, one, 1., 0., 1., one, one, one, None)
    assert L.esr_kgan_d_forward(*args, 1, 8, 6, 26, 1, None) == _lib.ESR_E_UNSUPPORTED
    assert L.esr_kgan_d_forward(*args, 1, 8, 60, 60, 1, None) == _lib.ESR_E_UNSUPPORTED               # 54 * 54 positions > 2048
    assert L.esr_kgan_d_backward(one, one, one, one, one, one, one, one, None, None, 1, 8, 26, 26, 1, None) == _lib.ESR_E_ARG
    assert L.esr_kgan_d_finish(one, one, one, one, None, 1, 8, 2, None) == _lib.ESR_E_ARG


def test_header_and_binding_agree_on_the_new_entry_points():
    import re
    from esr_hip import _lib
    hdr = open(os.path.join(ROOT, 'include', 'esr_hip.h')).read()
    declared = set(re.findall(r'^int\s+(esr_kgan_\w+)\s*\(', hdr, flags=re.M))
    assert len(declared) == 13 and declared == {n for n in _lib.EXPORTS if n.startswith('esr_kgan_')}
