"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C-ABI of libesr_hip.so, against the CPU
oracle on the same seeded inputs and against the golden vectors generated from the reference.

Tolerances (stated per the north star): generator outputs within 1e-3 relative of the fp32 CPU path (split-bf16 operands give
~1e-5); CEM filter ops are plain fp32 (<= 2e-6 abs on O(1) data); integer conventions (sizes, margins, strides) exact."""
import numpy as np
import pytest
import torch

from oracle import cem_oracle as co
from oracle import rrdb_oracle as ro
from oracle.check_golden import load, rel_l2, rel_max
from oracle.weights import fill_formula_weights, seeded_uniform
from oracle.gen_golden import aniso_gaussian_kernel

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_library_loaded_on_gpu_box():
    from esr_hip import load_library, library_path
    assert load_library().esr_version() >= 100
    import os
    assert os.path.exists(library_path())


def test_pack_unpack_roundtrip():
    from esr_hip import act as A
    x = seeded_uniform((2, 11, 9, 13), 1, -2.0, 2.0).to(DEV)
    buf = A.ActBuf(2, 2, 9, 13, DEV, split=True)
    A.pack_nchw(x, buf.view(), 0, 11)
    y = buf.to_nchw(11)
    assert (y - x).abs().max().item() < 2e-5           # hi+lo carries ~16 mantissa bits
    hi = buf.hi.cpu()
    assert hi[:, :, 0].abs().sum() == 0 and hi[:, :, -1].abs().sum() == 0 and hi[:, :, :, 0].abs().sum() == 0 and hi[:, :, :, -1].abs().sum() == 0
    # replicate padding folded into the pack
    buf2 = A.ActBuf(2, 2, 9 + 6, 13 + 6, DEV, split=True)
    A.pack_nchw(x, buf2.view(), 0, 11, pad=3)
    ref = torch.nn.functional.pad(x, (3,) * 4, mode='replicate')
    assert (buf2.to_nchw(11) - ref).abs().max().item() < 2e-5


@pytest.mark.parametrize('cin,cout,H,W,slope', [(3, 64, 12, 16, 1.0), (64, 32, 17, 23, 0.2), (67, 32, 9, 40, 0.2), (192, 64, 33, 21, 1.0),
                                                (64, 3, 40, 37, 1.0), (96, 128, 10, 10, 0.2),
                                                (32, 96, 11, 13, 0.2), (40, 72, 9, 10, 1.0)])     # a short last slice: 32 rows, 8 rows
def test_conv3x3_matches_torch_cpu(cin, cout, H, W, slope):
    from esr_hip import act as A
    x = seeded_uniform((2, cin, H, W), cin + cout, -1.0, 1.0)
    w = seeded_uniform((cout, cin, 3, 3), cin * 7 + cout, -1.0, 1.0) * float(np.sqrt(2.0 / (9 * cin)))
    b = seeded_uniform((cout,), cout, -0.1, 0.1)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1), slope)
    y = A.conv3x3_nchw(x.to(DEV), w.to(DEV), b.to(DEV), slope, split=True).cpu()
    assert rel_l2(y.numpy(), ref.numpy()) < 5e-5 and rel_max(y.numpy(), ref.numpy()) < 1e-4
    yb = A.conv3x3_nchw(x.to(DEV), w.to(DEV), b.to(DEV), slope, split=False).cpu()     # plain bf16 operands
    assert rel_l2(yb.numpy(), ref.numpy()) < 1.5e-2


@pytest.mark.parametrize('B,cin,cout,H,W', [(32, 64, 32, 52, 52),      # configs[2] per-GPU shape: 256 tiles of 7 x 52, two-stage kernel, 8 DMA slots per plane
                                            (6, 96, 32, 148, 148),     # configs[1] geometry, > 320 tiles: one-stage kernel, two workgroups per CU, 9 slots
                                            (3, 64, 64, 148, 148),     # the same tiles on the two-stage kernel (180 tiles), 64 output channels
                                            (5, 32, 32, 61, 200),      # tiles of 1 x 200 pixels + pitch: the widest a tile gets
                                            (7, 40, 24, 5, 7)])        # an image smaller than a tile, ragged channel counts
def test_conv3x3_tile_geometries(B, cin, cout, H, W):
    """Every wave copies exactly its share of the tile's 1-KiB slots and weight fragments (dma_share in esr_conv.hip) and the two-stage kernels
    wait on a run-time count: sweep the tile geometries that change those shares, in both operand modes, against an fp64 convolution."""
    from esr_hip import act as A
    x = seeded_uniform((B, cin, H, W), B + cin + W, -1.0, 1.0)
    w = seeded_uniform((cout, cin, 3, 3), cin * 5 + cout, -1.0, 1.0) * float(np.sqrt(2.0 / (9 * cin)))
    b = seeded_uniform((cout,), cout + 3, -0.1, 0.1)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1), 0.2).numpy()
    y = A.conv3x3_nchw(x.to(DEV), w.to(DEV), b.to(DEV), 0.2, split=True).cpu().numpy()
    assert rel_l2(y, ref) < 5e-5 and rel_max(y, ref) < 1e-4
    yb = A.conv3x3_nchw(x.to(DEV), w.to(DEV), b.to(DEV), 0.2, split=False).cpu().numpy()
    assert rel_l2(yb, ref) < 1.5e-2


F2_CASES = [('cubic_x4', 4, None, None), ('cubic_x2', 2, None, None), ('cubic_x3', 3, None, None), ('aniso_x4', 4, aniso_gaussian_kernel(), 0.1)]


def _cem(sf, kernel, bound):
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    conf = C.Get_CEM_Conf(sf)
    if bound:
        conf.lower_magnitude_bound = bound
    return C.CEMnet(conf, upscale_kernel=kernel)


@pytest.mark.parametrize('name,sf,kernel,bound', F2_CASES, ids=[c[0] for c in F2_CASES])
def test_cem_filter_ops_match_reference_golden(name, sf, kernel, bound):
    g = load('cem_filter_ops.npz')
    net = _cem(sf, kernel, bound).WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    lr = seeded_uniform((2, 3, 20, 24), 11).to(DEV)
    hr = seeded_uniform((2, 3, 20 * sf, 24 * sf), 12).to(DEV)
    with torch.no_grad():
        np.testing.assert_allclose(net.DownscaleOP(hr).cpu().numpy(), g[name + '/DownscaleOP'], atol=3e-6)
        np.testing.assert_allclose(net.Conv_LR_with_Inv_hTh_OP(lr).cpu().numpy(), g[name + '/Conv_LR_with_Inv_hTh_OP'], atol=6e-6)
        np.testing.assert_allclose(net.Upscale_OP(lr).cpu().numpy(), g[name + '/Upscale_OP'], atol=3e-6)
    if kernel is None:
        import CEM.CEMnet as C
        from CEM.imresize_CEM import imresize
        imresize.kernels = {}
        with torch.no_grad():
            np.testing.assert_allclose(C.CEM_downsampler(sf).to(DEV)(hr).cpu().numpy(), g[name + '/CEM_downsampler'], atol=3e-6)
            np.testing.assert_allclose(C.CEM_downsampler(sf, grayscale=True).to(DEV)(hr[:, :1].contiguous()).cpu().numpy(),
                                       g[name + '/CEM_downsampler_gray'], atol=3e-6)


def test_cem_pair_forward_matches_reference_golden():
    g = load('cem_forward.npz')
    for name, sf, kernel, bound in [('cubic_x4', 4, None, None), ('cubic_x2', 2, None, None), ('aniso_x4', 4, aniso_gaussian_kernel(), 0.1)]:
        net = _cem(sf, kernel, bound).WrapArchitecture_PyTorch(generated_image=None).to(DEV)
        lr = seeded_uniform((2, 3, 12, 16), 21).to(DEV)
        gen = seeded_uniform((2, 3, 12 * sf, 16 * sf), 22).to(DEV)
        with torch.no_grad():
            net.train()
            np.testing.assert_allclose(net([lr, gen]).cpu().numpy(), g[name + '/train'], atol=2e-5)
            net.eval()
            np.testing.assert_allclose(net([lr, gen]).cpu().numpy(), g[name + '/eval'], atol=2e-5)
    import CEM.CEMnet as C
    lr = seeded_uniform((2, 3, 12, 16), 21).to(DEV)
    gen = seeded_uniform((2, 3, 48, 64), 22).to(DEV)
    cem = _cem(4, None, None)
    cem.conf.sigmoid_range_limit = True
    cem.conf.input_range = np.array([0, 1])
    net = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    with torch.no_grad():
        np.testing.assert_allclose(net.train()([lr, gen]).cpu().numpy(), g['cubic_x4_sigmoid/train'], atol=2e-5)
    cem = _cem(4, None, None)
    cem.conf.decomposed_output = True
    net = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    with torch.no_grad():
        o = net.train()([lr, gen])
        np.testing.assert_allclose(o[0].cpu().numpy(), g['cubic_x4_decomposed/train_ortho'], atol=2e-5)
        np.testing.assert_allclose(o[1].cpu().numpy(), g['cubic_x4_decomposed/train_NS'], atol=2e-5)
        np.testing.assert_allclose(net.eval()([lr, gen]).cpu().numpy(), g['cubic_x4_decomposed/eval'], atol=2e-5)


F4_CASES = [('nb1_x4', 1, 4, 0), ('nb3_x4', 3, 4, 0), ('nb1_x8', 1, 8, 0), ('nb1_x2', 1, 2, 0),
            ('nb1_x4_lat3', 1, 4, 3), ('nb2_x4_lat3', 2, 4, 3), ('nb1_x2_lat1', 1, 2, 1)]


def _rrdb(nb, sf, lat):
    import models.modules.architecture as arch
    net = arch.RRDBNet(in_nc=3, out_nc=3, nf=64, nb=nb, gc=32, upscale=sf, norm_type=None, act_type='leakyrelu', mode='CNA',
                       upsample_mode='upconv', latent_input='all_layers_HR_downscaled' if lat else None, num_latent_channels=lat)
    fill_formula_weights(net, gain=1.0)
    return net


def _f4_input(nb, sf, lat):
    h, w = (12, 16) if sf != 8 else (8, 8)
    x = seeded_uniform((1, 3 + lat * sf * sf, h, w), 31 + nb + sf + lat, -1.0 if lat else 0.0, 1.0)
    if lat:
        x[:, -3:] = x[:, -3:] * 0.5 + 0.5
    return x


@pytest.mark.parametrize('precision', ['split', 'mixed'])
@pytest.mark.parametrize('name,nb,sf,lat', F4_CASES, ids=[c[0] for c in F4_CASES])
def test_rrdb_forward_matches_reference_golden(name, nb, sf, lat, precision):
    """Forward of 7 generator variants against outputs of the reference itself, in the fp32 path ('split') and in the 'mixed' fp16
    inference mode — the same 1e-4 assertion for both (bar: 1e-3)."""
    g = load('rrdb_fwd_bwd.npz')
    net = _rrdb(nb, sf, lat)
    assert sum(p.numel() for p in net.parameters()) == int(g[name + '/nparams'][1])
    net = net.to(DEV)
    net.set_precision(precision)
    x = _f4_input(nb, sf, lat)
    with torch.no_grad():
        y = net(x.to(DEV)).cpu().numpy()
    # 1e-3 relative is the contract; split-bf16 lands around 1e-5
    assert rel_l2(y, g[name + '/out']) < 1e-4 and rel_max(y, g[name + '/out']) < 3e-4, (rel_l2(y, g[name + '/out']), rel_max(y, g[name + '/out']))
    # and against the CPU oracle evaluated here on the same weights
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = ro.rrdb_forward(sd, x, nb, sf, lat).numpy()
    assert rel_l2(y, ref) < 1e-4


def test_c1_end_to_end_matches_reference_golden():
    """BASELINE config 1 (RRDB-3 x4 + CEM, eval, [1,3,32,32]) and its explorable (lat=3) variant."""
    g = load('c1_end_to_end.npz')
    import CEM.CEMnet as C
    cem = _cem(4, None, None)
    G = cem.WrapArchitecture_PyTorch(_rrdb(3, 4, 0))
    fill_formula_weights(G, gain=1.0)
    assert list(G.state_dict().keys()) == [str(k) for k in g['c1/keys']]
    assert [str(tuple(v.shape)) for v in G.state_dict().values()] == [str(s) for s in g['c1/key_shapes']]
    G = G.to(DEV)
    x = seeded_uniform((1, 3, 32, 32), 51).to(DEV)
    with torch.no_grad():
        y = G.eval()(x)
        assert y.shape == (1, 3, 128, 128)
        yt = G.train()(x)
    assert rel_l2(y.cpu().numpy(), g['c1/out']) < 1e-4 and rel_max(y.cpu().numpy(), g['c1/out']) < 3e-4
    assert rel_l2(yt.cpu().numpy(), g['c1/out_train_mode']) < 1e-4
    # downsample-consistency of the CEM output (interior), measured with the HIP CEM_downsampler-equivalent
    with torch.no_grad():
        d = G.DownscaleOP(y)
    m = int(cem.invalidity_margins_LR)
    rmse = float(((d - x)[:, :, m:-m, m:-m] ** 2).mean().sqrt())
    assert rmse < 5e-5, rmse     # the reference itself measures 1.0e-5 on these O(3)-amplitude formula weights (golden)
    assert abs(rmse - float(g['c1/consistency_interior_rmse'])) < 3e-5

    G = cem.WrapArchitecture_PyTorch(_rrdb(2, 4, 3))
    fill_formula_weights(G, gain=1.0)
    assert list(G.state_dict().keys()) == [str(k) for k in g['c1_lat3/keys']]
    G = G.to(DEV)
    z = seeded_uniform((1, 3, 128, 128), 52, -1.0, 1.0).to(DEV)
    xin = torch.cat([z.contiguous().view(1, 48, 32, 32), x], 1)
    with torch.no_grad():
        y = G.eval()(xin)
    assert rel_l2(y.cpu().numpy(), g['c1_lat3/out']) < 1e-4


@pytest.mark.parametrize('precision,tol', [('split', 1e-4), ('mixed', 3e-4), ('f16x2', 1e-3), ('f16', 3e-3), ('bf16', 3e-2)])
def test_c5_style_x8_blurry_kernel_eval_forward(precision, tol):
    """BASELINE configs[4] in miniature: x8 generator, non-bicubic CEM kernel ('blurry_cubic_2.0': margin 12 LR pixels), eval mode,
    in the fp32-class mode (bar 1e-3, asserted at 1e-4) and in the reduced-precision single-MFMA mode the reference has no
    counterpart of (tolerances are the modes' own: fp16 operands ~1e-3 — configs[4] names fp16 —, bf16 operands ~1e-2)."""
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    sf, nb = 8, 2
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel='blurry_cubic_2.0')
    G = cem.WrapArchitecture_PyTorch(_rrdb(nb, sf, 0))
    fill_formula_weights(G, gain=1.0)
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    G = G.to(DEV).eval()
    G.generated_image_model.set_precision(precision)
    x = seeded_uniform((2, 3, 9, 11), 301)
    with torch.no_grad():
        y = G(x.to(DEV)).cpu()
    t = co.CEMTaps(sf, 'blurry_cubic_2.0')
    assert t.margins_LR == int(cem.invalidity_margins_LR) == 12
    xp = torch.nn.functional.pad(x, (t.margins_LR,) * 4, mode='replicate')
    gen = ro.rrdb_forward(sd, xp, nb, sf, 0, prefix='generated_image_model.model')
    ref = co.cem_combine(xp, gen, t, crop=True)
    assert y.shape == ref.shape == (2, 3, 72, 88)
    assert rel_l2(y.numpy(), ref.numpy()) < tol
    # whatever the generator's precision, the CEM keeps the output consistent with the LR input (fp32 filters)
    back = co.downscale_op(y, t)
    assert float((back - x)[..., 3:-3, 3:-3].abs().max()) < 2e-5 * max(1.0, float(y.abs().max()))
    imresize.kernels = {}


def test_hip_graph_replay_is_bit_identical():
    """esr_hip.graph.GraphedForward: the whole CEM-wrapped forward captured into a HIP graph replays to the same bits, follows new
    inputs, and is re-captured after a parameter update."""
    import CEM.CEMnet as C
    from esr_hip.graph import GraphedForward
    G = _cem(4, None, None).WrapArchitecture_PyTorch(_rrdb(1, 4, 0)).to(DEV).eval()
    fast = GraphedForward(G)
    xs = [seeded_uniform((1, 3, 16, 20), 400 + i).to(DEV) for i in range(3)]
    with torch.no_grad():
        for x in xs:
            assert torch.equal(G(x), fast(x))
        for p in G.generated_image_model.parameters():
            p.mul_(0.5)
        assert torch.equal(G(xs[0]), fast(xs[0]))
        # an image whose CEM projection takes the wave-streaming kernels (their strip count is asked of the occupancy API at launch: also under capture)
        big = seeded_uniform((1, 3, 112, 120), 404).to(DEV)
        assert G.DownscaleOP.taps() is not None and __import__('esr_hip')._lib.lib.esr_cem_sep_form(2, 4, 27, 1, 132, 140) == 2
        fast_big = GraphedForward(G)
        ref = G(big)
        assert torch.equal(ref, fast_big(big)) and torch.equal(ref, fast_big(big))


@pytest.mark.parametrize('sf,kernel', [(4, None), (2, None), (4, 'blurry_cubic_1.0')])
def test_gpu_lr_synthesis_equals_the_dataset_paths_imresize(sf, kernel):
    """the LR images the reference's dataset code makes on the CPU with imresize(HR, 1/sf)
    (LRHR_dataset.py:87; replicate-pad, anti-aliasing filter, stride) are what DownscaleOP computes on the GPU with the strided-blur
    kernel — whole image, borders included — and Mask_Invalid_Regions_PyTorch applies the same loss mask to both images."""
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel)
    net = cem.WrapArchitecture_PyTorch(generated_image=None, training_patch_size=32 * sf).to(DEV)
    hr = seeded_uniform((2, 3, 24 * sf, 20 * sf), 601)
    lr_gpu = net.DownscaleOP(hr.to(DEV)).cpu().numpy()
    for b in range(2):
        im = hr[b].permute(1, 2, 0).numpy().astype(np.float64)
        # the checker is the ORACLE's restatement of imresize (pinned to the reference by fixture F3, tests/test_oracle_golden.py); the product's
        # own host-side imresize must agree with it too
        ref = co.imresize_np(im, sf_down=sf, kernel_up=co.upscale_kernel(sf, kernel))
        np.testing.assert_allclose(lr_gpu[b].transpose(1, 2, 0), ref, atol=2e-6)
        np.testing.assert_allclose(imresize(im, scale_factor=[1.0 / sf], kernel=kernel), ref, atol=1e-12)
    a, b2 = seeded_uniform((1, 3, 32 * sf, 32 * sf), 602).to(DEV), seeded_uniform((1, 3, 32 * sf, 32 * sf), 603).to(DEV)
    ma, mb = cem.Mask_Invalid_Regions_PyTorch(a, b2)
    m = int(cem.invalidity_margins_HR)
    assert float(ma[..., :m, :].abs().max()) == 0 and torch.equal(ma[..., m:-m, m:-m], a[..., m:-m, m:-m]) and torch.equal(mb[..., m:-m, m:-m], b2[..., m:-m, m:-m])
    imresize.kernels = {}


def test_x3_generator_forward_and_input_gradient():
    """upscale = 3 (one nearest-x3 upsampler, architecture.py:260-261; the reference's own constructor is broken for it, so there is no
    golden fixture): forward and d/dx against the oracle, which implements the intended architecture."""
    net = _rrdb(1, 3, 0)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(DEV)
    x = seeded_uniform((2, 3, 10, 13), 901)
    xg = x.clone().to(DEV).requires_grad_(True)
    y = net(xg)
    xc = x.clone().requires_grad_(True)
    yo = ro.rrdb_forward(sd, xc, 1, 3, 0, prefix='model')
    assert y.shape == yo.shape == (2, 3, 30, 39)
    assert rel_l2(y.detach().cpu().numpy(), yo.detach().numpy()) < 1e-4
    cot = seeded_uniform(tuple(yo.shape), 902, -1, 1)
    (y * cot.to(DEV)).sum().backward()
    (yo * cot).sum().backward()
    from test_gpu_backward import assert_grad_close
    assert_grad_close(xg.grad.cpu().numpy(), xc.grad.numpy(), 'x3 input gradient')


@pytest.mark.parametrize('name,nb,sf,lat', [('nb1_x4_lat3_first', 1, 4, 3), ('nb2_x2_lat1_first', 2, 2, 1)])
def test_rrdb_first_layer_latent_matches_reference_golden(name, nb, sf, lat):
    """latent_input = 'first_layer_HR_downscaled': Z (bilinear / sf) enters fea_conv only; forward and d/dx (LR and Z channels)."""
    import models.modules.architecture as arch
    g = load('rrdb_first_layer.npz')
    net = arch.RRDBNet(in_nc=3, out_nc=3, nf=64, nb=nb, gc=32, upscale=sf, norm_type=None, act_type='leakyrelu', mode='CNA', upsample_mode='upconv',
                       latent_input='first_layer_HR_downscaled', num_latent_channels=lat)
    n = fill_formula_weights(net, gain=1.0)
    assert [n, sum(p.numel() for p in net.parameters())] == [int(v) for v in g[name + '/nparams']]
    net = net.to(DEV)
    x = seeded_uniform((1, 3 + lat * sf * sf, 12, 16), 61 + nb + sf + lat, -1.0, 1.0)
    x[:, -3:] = x[:, -3:] * 0.5 + 0.5
    x = x.to(DEV).requires_grad_(True)
    y = net(x)
    assert rel_l2(y.detach().cpu().numpy(), g[name + '/out']) < 1e-4
    cot = seeded_uniform(tuple(y.shape), 71 + nb + sf + lat, -1.0, 1.0).to(DEV)
    (y * cot).sum().backward()
    dx, ref = x.grad.cpu().numpy(), g[name + '/dx']
    from test_gpu_backward import assert_grad_close
    assert_grad_close(dx, ref, name)


@pytest.mark.parametrize('precision,tol', [('split', 1e-4), ('mixed', 3e-4), ('f16x2', 1e-3)])
def test_c2_rrdb23_probe_matches_reference_golden(precision, tol):
    """The full-depth generator of BASELINE configs[1] (RRDB-23 x4 + CEM, eval, one 128x128 image) against outputs of the REFERENCE itself
    (fixture F6: a 64x64 crop and a stride-8 sampling of the 512x512 result).  Bar: 1e-3.  Measured: split 3.9e-5 (asserted at 1e-4),
    mixed 1.25e-4 (asserted at 3e-4), f16x2 7.5e-4 (asserted at the bar)."""
    g = load('c2_rrdb23_probe.npz')
    cem = _cem(4, None, None)
    G = cem.WrapArchitecture_PyTorch(_rrdb(23, 4, 0))
    n = fill_formula_weights(G, gain=0.6)
    assert sum(p.numel() for p in G.generated_image_model.parameters()) == int(g['nparams'][0]) == 16697987
    G = G.to(DEV).eval()
    G.generated_image_model.set_precision(precision)
    x = seeded_uniform((1, 3, 128, 128), 61).to(DEV)
    with torch.no_grad():
        y = G(x).cpu().numpy()
    assert y.shape == (1, 3, 512, 512)
    e1, e2 = rel_l2(y[:, :, 200:264, 300:364], g['crop64']), rel_l2(y[:, :, 3::8, 5::8], g['stride8'])
    print("F6 %s: crop %.2e stride8 %.2e" % (precision, e1, e2))
    assert e1 < tol and e2 < tol, (precision, e1, e2)


@pytest.mark.parametrize('kernel', [None, 'blurry_cubic_2.0'])
def test_streaming_downscale_matches_the_2d_kernel_over_several_strips(kernel):
    """x8 kernels (k = 33 / 45) on small images take the streaming form of the separable downscale (csrc/esr_cem.hip: strips of 32 x 64 outputs walked 16
    window rows at a time through a ring of horizontal-pass rows): 70 x 50 outputs = 2 x 2 strips with ragged last strips, plain and fused
    (lr_pad - D(y)) outputs, against the k^2 2-D kernel."""
    from esr_hip import cem_ops
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    import CEM.CEMnet as C
    sf = 8
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel)
    G = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    td = G.DownscaleOP.taps()
    pre = sf - sf // 2 - 1
    h, w = 70, 50             # (under 64 x 64 low-resolution pixels: larger images take the wave-streaming kernel, tested below)
    assert cem_ops._lib.lib.esr_cem_sep_form(0, sf, int(td.shape[-1]), pre, h, w) == 1
    y = seeded_uniform((2, 3, sf * h, sf * w), 311).to(DEV)
    lr = seeded_uniform((2, 3, h - 8, w - 8), 312).to(DEV)
    try:
        cem_ops.USE_SEPARABLE = True
        a = [cem_ops.downscale_raw(y, td, sf, pre), cem_ops.downscale_raw(y, td, sf, pre, lr=lr, lr_pad=4)]
        cem_ops.USE_SEPARABLE = False
        b = [cem_ops.downscale_raw(y, td, sf, pre), cem_ops.downscale_raw(y, td, sf, pre, lr=lr, lr_pad=4)]
    finally:
        cem_ops.USE_SEPARABLE = True
    imresize.kernels = {}
    for u, v in zip(a, b):
        assert float((u - v).abs().max()) < 2e-6 * max(1.0, float(v.abs().max()))


@pytest.mark.parametrize('sf,kernel,hw,B', [(4, None, (148, 148), 2), (4, None, (131, 270), 1), (4, None, (70, 131), 1), (4, None, (65, 67), 3), (3, None, (70, 67), 2), (3, None, (64, 64), 1),
                                            (8, None, (64, 64), 1), (8, 'blurry_cubic_2.0', (150, 70), 2), (4, 'blurry_cubic_1.0', (64, 80), 2), (4, 'blurry_cubic_1.0', (129, 134), 1),
                                            (2, None, (80, 90), 2)])
def test_wave_streaming_cem_kernels_match_the_2d_kernels(sf, kernel, hw, B):
    """Low-resolution images of at least 64 x 64 pixels take the wave-streaming separable kernels (round 6; csrc/esr_cem.hip cem_downscale_wave_kernel /
    cem_lrfilter_wave_kernel / cem_upscale_wave_kernel: a wave walks down a strip of the image, vertical pass in registers, no workgroup barrier) — checked,
    through esr_cem_sep_form, to be what runs here.  Against the k^2 2-D kernels: plain and fused downscale, the LR filter, every upscale mode, crops that keep and that break the 16-byte
    alignment of g / out rows (x3: image rows are not multiples of 4 words at all — the element-wise paths), several column tiles and row strips with ragged
    last ones, batches of 1..3.  x2 has pre = 0: its upscale keeps the tile kernel (the replicate rule of the zero-stuffed image's first row)."""
    from esr_hip import cem_ops
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    import CEM.CEMnet as C
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel)
    G = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    td, ti, tu = G.DownscaleOP.taps(), G.Conv_LR_with_Inv_hTh_OP.taps(), G.Upscale_OP.taps()
    pre = sf - sf // 2 - 1
    h, w = hw
    form = cem_ops._lib.lib.esr_cem_sep_form
    assert form(0, sf, int(td.shape[-1]), pre, h, w) == 2 and form(1, sf, int(tu.shape[-1]), pre, h, w) == (2 if sf > 2 else 0)
    assert form(2, sf, int(ti.shape[-1]), pre, h, w) == (2 if h * w >= 128 * 128 else 0)           # (the LR filter: from 128 x 128 pixels)
    y = seeded_uniform((B, 3, sf * h, sf * w), 321).to(DEV)
    lr = seeded_uniform((B, 3, h - 6, w - 6), 322).to(DEV)
    x = seeded_uniform((B, 3, h, w), 323, -1.0, 1.0).to(DEV)
    x2 = seeded_uniform((B, 3, h, w), 324, -1.0, 1.0).to(DEV)

    def run():
        out = [cem_ops.downscale_raw(y, td, sf, pre), cem_ops.downscale_raw(y, td, sf, pre, lr=lr, lr_pad=3), cem_ops.lr_filter_raw(x, ti),
               cem_ops.upscale_raw(x, tu, sf, pre), cem_ops.upscale_raw(x, tu, sf, pre, g=y, crop=2 * sf, mode=1), cem_ops.upscale_raw(x, tu, sf, pre, g=y, crop=2 * sf + 1, mode=1),
               cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=sf, mode=2, rng=1.0), cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=3, mode=2, rng=0.5)]
        out += list(cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=0, mode=3))
        out += list(cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=5, mode=3))
        return out
    try:
        cem_ops.USE_SEPARABLE = True
        a = run()
        # a batch and its single images run the same arithmetic (the form is chosen from the image geometry alone)
        one = cem_ops.downscale_raw(y[:1].contiguous(), td, sf, pre, lr=lr[:1].contiguous(), lr_pad=3)
        assert torch.equal(one, a[1][:1])
        one = cem_ops.upscale_raw(x[:1].contiguous(), tu, sf, pre, g=y[:1].contiguous(), crop=2 * sf, mode=1)
        assert torch.equal(one, a[4][:1])
        assert torch.equal(cem_ops.lr_filter_raw(x[:1].contiguous(), ti), a[2][:1])
        cem_ops.USE_SEPARABLE = False
        b = run()
    finally:
        cem_ops.USE_SEPARABLE = True
    imresize.kernels = {}
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and bool(torch.isfinite(u).all())
        assert float((u - v).abs().max()) < 2e-6 * max(1.0, float(v.abs().max())), (i, float((u - v).abs().max()))


# ---- separable CEM fast path (rank-one taps: bicubic ds_kernel / inv_hTh) against the general 2-D kernels
@pytest.mark.parametrize('sf,kernel', [(2, None), (3, None), (4, None), (8, None), (4, 'blurry_cubic_1.0')])
def test_separable_cem_kernels_match_the_2d_kernels(sf, kernel):
    """The three filters and the fused projection (all modes) evaluated by the separable kernels (esr_cem_*_sep: tv (x) th factors of the
    taps, 2k MACs per output) and by the 2-D kernels (k^2 MACs): same index conventions (strided pick at sf*i+pre, zero-stuffing offset,
    replicate clamps, crop), results equal to fp32 rounding of the tap products."""
    from esr_hip import cem_ops
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    import CEM.CEMnet as C
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel)
    G = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    td, ti, tu = G.DownscaleOP.taps(), G.Conv_LR_with_Inv_hTh_OP.taps(), G.Upscale_OP.taps()
    assert all(cem_ops._taps_entry(t, torch.device(DEV, 0))[1] is not None for t in (td, ti, tu)), 'bicubic-family kernels are rank one'
    pre = sf - sf // 2 - 1
    h, w = 21, 37
    y = seeded_uniform((2, 3, sf * h, sf * w), 301).to(DEV)
    lr = seeded_uniform((2, 3, h - 6, w - 6), 302).to(DEV)
    x = seeded_uniform((2, 3, h, w), 303, -1.0, 1.0).to(DEV)
    x2 = seeded_uniform((2, 3, h, w), 304, -1.0, 1.0).to(DEV)

    def run():
        out = [cem_ops.downscale_raw(y, td, sf, pre), cem_ops.downscale_raw(y, td, sf, pre, lr=lr, lr_pad=3), cem_ops.lr_filter_raw(x, ti),
               cem_ops.upscale_raw(x, tu, sf, pre), cem_ops.upscale_raw(x, tu, sf, pre, g=y, crop=2 * sf, mode=1),
               cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=sf, mode=2, rng=1.0)]
        out += list(cem_ops.upscale_raw(x, tu, sf, pre, f2=x2, g=y, crop=0, mode=3))
        return out
    try:
        cem_ops.USE_SEPARABLE = True
        a = run()
        cem_ops.USE_SEPARABLE = False
        b = run()
    finally:
        cem_ops.USE_SEPARABLE = True
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape
        assert float((u - v).abs().max()) < 2e-6 * max(1.0, float(v.abs().max())), (i, float((u - v).abs().max()))


@pytest.mark.parametrize('sf,kernel,hw', [(2, None, (21, 37)), (3, None, (21, 37)), (4, None, (21, 37)), (4, None, (148, 148)), (8, None, (19, 23)),
                                          (8, 'blurry_cubic_2.0', (40, 33)), (4, 'blurry_cubic_1.0', (21, 37))])
def test_filter_folded_into_the_upscale_launch_is_bit_identical_to_the_two_launches(sf, kernel, hw):
    """Round 6: esr_cem_filter_upscale_sep — the LR filter K = inv_hTh evaluated per tile inside the upscale launch (every tile
    filters its own clamped window of the LR operand on chip, with the separate kernel's two passes and summation order) against
    esr_cem_lrfilter_sep followed by esr_cem_upscale_sep: every mode (plain, g + U(K e) with crop, tanh range with two operands, decomposed),
    ragged sizes (tiles that stick out of the image, windows that reach past every border: the replicate clamp of K and the zero frame of U),
    one LR-sized intermediate and one launch fewer per projection.  Equal to the last bit; so are project() and its differentiable form."""
    from esr_hip import cem_ops
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    import CEM.CEMnet as C
    cem = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel)
    G = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    td, ti, tu = G.DownscaleOP.taps(), G.Conv_LR_with_Inv_hTh_OP.taps(), G.Upscale_OP.taps()
    pre = sf - sf // 2 - 1
    h, w = hw
    y = seeded_uniform((2, 3, sf * h, sf * w), 311).to(DEV)
    x = seeded_uniform((2, 3, h, w), 313, -1.0, 1.0).to(DEV)
    x2 = seeded_uniform((2, 3, h, w), 314, -1.0, 1.0).to(DEV)
    lr = seeded_uniform((2, 3, h - 6, w - 6), 312).to(DEV)

    def run():
        out = [cem_ops.filter_upscale_raw(x, ti, tu, sf, pre), cem_ops.filter_upscale_raw(x, ti, tu, sf, pre, g=y, crop=2 * sf, mode=1),
               cem_ops.filter_upscale_raw(x, ti, tu, sf, pre, e2=x2, g=y, crop=sf, mode=2, rng=1.0)]
        out += list(cem_ops.filter_upscale_raw(x, ti, tu, sf, pre, e2=x2, g=y, crop=0, mode=3))
        out.append(cem_ops.project(lr, y, td, ti, tu, sf, pre, lr_pad=3, crop=3 * sf))
        out.append(cem_ops.project(lr, y, td, ti, tu, sf, pre, lr_pad=3, crop=3 * sf, sigmoid_range=1.0))
        yg = y.clone().requires_grad_(True)
        o = cem_ops.project(lr, yg, td, ti, tu, sf, pre, lr_pad=3, crop=3 * sf)
        o.sum().backward()
        return out + [o.detach(), yg.grad]
    calls = []
    real = cem_ops._lib.lib.esr_cem_filter_upscale_sep
    try:
        cem_ops.FUSE_FILTER_UPSCALE = True
        cem_ops._lib.lib.esr_cem_filter_upscale_sep = lambda *a: (calls.append(real(*a)), calls[-1])[1]
        a = run()
        cem_ops._lib.lib.esr_cem_filter_upscale_sep = real
        cem_ops.FUSE_FILTER_UPSCALE = False
        b = run()
    finally:
        cem_ops._lib.lib.esr_cem_filter_upscale_sep = real
        cem_ops.FUSE_FILTER_UPSCALE = None
    assert len(calls) == 7 and all(rc == 0 for rc in calls), calls            # the folded launch really ran (no quiet fallback to the two launches)
    # The fold evaluates K with the TILE kernel's passes and summation order: where the separate launch is that kernel, to the last bit.  Images of at
    # least 64 x 64 low-resolution pixels take the wave-streaming filter (vertical pass first, one accumulator): equal to fp32 rounding there (the fold
    # itself is only used for small launches: cem_ops.FOLD_MAX_TILES).
    tile_filter = cem_ops._lib.lib.esr_cem_sep_form(2, sf, int(ti.shape[-1]), pre, h, w) == 0
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape
        if tile_filter:
            assert torch.equal(u, v), (i, float((u - v).abs().max()))
        else:
            assert float((u - v).abs().max()) < 4e-6 * max(1.0, float(v.abs().max())), (i, float((u - v).abs().max()))


def test_anisotropic_kernels_keep_the_2d_path():
    from esr_hip import cem_ops
    from oracle.gen_golden import aniso_gaussian_kernel
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    import CEM.CEMnet as C
    conf = C.Get_CEM_Conf(4)
    conf.lower_magnitude_bound = 0.1
    cem = C.CEMnet(conf, upscale_kernel=aniso_gaussian_kernel())
    G = cem.WrapArchitecture_PyTorch(generated_image=None).to(DEV)
    assert cem_ops._taps_entry(G.DownscaleOP.taps(), torch.device(DEV, 0))[1] is None
    imresize.kernels = {}
