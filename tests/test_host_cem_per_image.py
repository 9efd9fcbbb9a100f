"""One CEM kernel per image of a batch, the host side (no GPU): CEMnet.build_per_image, CEM_PyTorch.set_per_image_kernels, SRRaGANModel.set_kernels
and the argument checks of the esr_cem_*_per_image entry points.

The kernels (scale 4) are the ones tests/test_gpu_cem_per_image.py runs: bicubic (None) and two rotated anisotropic Gaussians, 33 x 33 (sigma 5 / 2,
angle 0.6) and 17 x 17 (sigma 2.5 / 1.2, angle 1.1).  Built on the CPU they give ds_kernel 17 / 17 / 9, inv_hTh 27 / 43 / 31 and margins 10 / 25 / 10:
the batch's common sizes are 17 and 43, its margin 25."""
import functools

import numpy as np
import pytest
import torch
from scipy.signal import correlate2d

SF = 4
SIZES = {'ds_kernel': (17, 17, 9), 'inv_hTh': (27, 43, 31), 'margin': (10, 25, 10)}


def gaussian(n, s1, s2, angle):
    """n x n anisotropic Gaussian, standard deviations s1 / s2 along axes rotated by `angle`, summing to 1."""
    r = np.arange(n) - (n - 1) / 2.0
    X, Y = np.meshgrid(r, r)
    c, s = np.cos(angle), np.sin(angle)
    k = np.exp(-0.5 * ((c * X + s * Y) ** 2 / s1 ** 2 + (c * Y - s * X) ** 2 / s2 ** 2))
    return k / k.sum()


def kernels():
    return [None, gaussian(33, 5.0, 2.0, 0.6), gaussian(17, 2.5, 1.2, 1.1)]


def conf_for(kernel, **settings):
    """The configuration SRRaGANModel.set_kernels builds an image's CEM with."""
    import CEM.CEMnet as C
    conf = C.Get_CEM_Conf(SF)
    if isinstance(kernel, np.ndarray):
        conf.lower_magnitude_bound = 0.1
    for k, v in settings.items():
        setattr(conf, k, v)
    return conf


@functools.lru_cache(maxsize=None)
def nets():
    """The three CEMnet objects, built once (never modified by a test)."""
    import CEM.CEMnet as C
    return tuple(C.CEMnet.build_per_image(conf_for, kernels()))


def wrap(net, margin=None, **settings):
    """A single-kernel CEM_PyTorch (pair input) of `net`'s filters, optionally with another eval-mode margin."""
    import copy
    net = copy.copy(net)
    net.conf = conf_for(None, **settings)
    if margin is not None:
        net.invalidity_margins_LR = margin
    return net.WrapArchitecture_PyTorch()


def test_built_sizes_are_the_stated_ones():
    got = nets()
    assert tuple(n.ds_kernel.shape[0] for n in got) == SIZES['ds_kernel']
    assert tuple(n.inv_hTh.shape[0] for n in got) == SIZES['inv_hTh']
    assert tuple(int(n.invalidity_margins_LR) for n in got) == SIZES['margin']
    for n, rank_one in zip(got, (True, False, False)):
        sv = np.linalg.svd(n.ds_kernel, compute_uv=False)
        assert (sv[1] <= 1e-6 * sv[0]) == rank_one          # estimated-style kernels take the general k^2 filters


def test_padded_taps_are_centred_and_give_the_unpadded_result():
    """Every image's three filters, zero-padded to the batch's largest size, correlated in float64 against a random 40 x 40 image (replicate
    padding, as the kernels apply it) give what the image's own unpadded fp32 taps give, to 1e-12: the padding is symmetric, the centre stays at
    floor(k / 2)."""
    cem = wrap(nets()[0])
    names = ('DownscaleOP', 'Upscale_OP', 'Conv_LR_with_Inv_hTh_OP')
    cem.set_per_image_kernels(nets())
    want = {'DownscaleOP': 17, 'Upscale_OP': 17, 'Conv_LR_with_Inv_hTh_OP': 43}
    image = np.random.RandomState(0).rand(40, 40)
    for name in names:
        padded = getattr(cem, name).taps()
        assert padded.dtype == torch.float32 and tuple(padded.shape) == (3, want[name], want[name])
        for i, net in enumerate(nets()):
            own = getattr(wrap(net), name).taps().double().numpy()
            big = padded[i].double().numpy()
            a = correlate2d(np.pad(image, own.shape[0] // 2, mode='edge'), own, mode='valid')
            b = correlate2d(np.pad(image, big.shape[0] // 2, mode='edge'), big, mode='valid')
            assert a.shape == b.shape == (40, 40)
            assert np.abs(a - b).max() <= 1e-12, (name, i, np.abs(a - b).max())
            m = (big.shape[0] - own.shape[0]) // 2
            assert np.array_equal(big[m:big.shape[0] - m, m:big.shape[0] - m], own) and np.count_nonzero(big) == np.count_nonzero(own)


def test_common_margin_is_the_maximum_and_none_restores():
    cem = wrap(nets()[0])
    assert cem.margins_LR == 10
    cem.set_per_image_kernels(nets())
    assert cem.margins_LR == 25 == max(SIZES['margin'])
    x = torch.zeros(1, 3, 6, 5)
    assert tuple(cem.LR_padder(x).shape) == (1, 3, 56, 55) and tuple(cem.HR_padder(x).shape) == (1, 3, 206, 205)
    assert tuple(cem.HR_unpadder(cem.HR_padder(x)).shape) == tuple(x.shape)
    cem.set_per_image_kernels(None)
    assert cem.margins_LR == 10 and tuple(cem.LR_padder(x).shape) == (1, 3, 26, 25)
    assert cem.DownscaleOP.taps().dim() == 2 and cem.DownscaleOP.per_image_taps is None


def test_build_per_image_leaves_the_resize_kernel_cache_as_found():
    """Building a CEMnet around a kernel overwrites the process-wide imresize.kernels[str(sf)]; build_per_image hands the cache back: same keys,
    the same array objects."""
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    imresize(np.ones((8, 8)), [SF])                              # the cache exists and holds the default kernel
    before = dict(imresize.kernels)
    assert str(SF) in before
    built = C.CEMnet.build_per_image(conf_for, kernels()[::-1])      # None LAST: it still means the kernel in use before the call
    after = imresize.kernels
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)
    assert np.array_equal(built[-1].ds_kernel, nets()[0].ds_kernel) and np.array_equal(built[0].ds_kernel, nets()[2].ds_kernel)
    with pytest.raises(AssertionError):                          # a failing build hands it back too
        C.CEMnet.build_per_image(conf_for, [kernels()[1], np.ones((5, 5))])
    assert list(imresize.kernels) == list(before) and all(imresize.kernels[k] is before[k] for k in before)


def test_state_dict_is_unchanged_by_per_image_kernels():
    cem = wrap(nets()[0])
    before = {k: v.clone() for k, v in cem.state_dict().items()}
    params, buffers = [n for n, _ in cem.named_parameters()], [n for n, _ in cem.named_buffers()]
    cem.set_per_image_kernels(nets())
    after = cem.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in cem.named_parameters()] == params and [n for n, _ in cem.named_buffers()] == buffers


def test_batch_size_mismatch_is_a_value_error():
    cem = wrap(nets()[0]).eval()
    cem.set_per_image_kernels(nets())
    with pytest.raises(ValueError, match='per-image kernels'):
        cem([torch.zeros(2, 3, 6, 5), torch.zeros(2, 3, 24, 20)])
    cem.set_per_image_kernels(nets()[:2])
    with pytest.raises(ValueError, match='per-image kernels'):
        cem([torch.zeros(3, 3, 6, 5), torch.zeros(3, 3, 24, 20)])


def test_training_model_refuses_set_kernels():
    from models import create_model
    from test_host_api import _opt
    m = create_model(_opt(nb=1, is_train=True))
    with pytest.raises(NotImplementedError, match='inference'):
        m.set_kernels(kernels())
    with pytest.raises(NotImplementedError, match='inference'):
        m.set_kernels(None)


def test_inference_model_set_kernels_keeps_the_generator_and_restores():
    """On the CPU: set_kernels swaps the CEM's filters and nothing else; None entries are the model's own CEMnet object."""
    from models import create_model
    from test_host_api import _opt
    m = create_model(_opt(nb=1))
    G = m.netG.generated_image_model
    keys = list(m.netG.state_dict())
    m.set_kernels(kernels())
    assert m.netG.generated_image_model is G and list(m.netG.state_dict()) == keys
    assert m.netG.margins_LR == 25 and tuple(m.netG.Conv_LR_with_Inv_hTh_OP.taps().shape) == (3, 43, 43)
    assert torch.equal(m.netG.DownscaleOP.taps()[0], m.netG.DownscaleOP.Filter_OP.weight[0, 0])          # 17 of 17: no padding for image 0
    m.set_kernels(None)
    assert m.netG.margins_LR == 10 and m.netG.DownscaleOP.taps().dim() == 2


def test_per_image_entry_points_check_their_arguments_with_fake_pointers():
    """Bad arguments come back as ESR_E_ARG before anything touches the device — the conditions of the single-kernel entry points."""
    from esr_hip import _lib
    from esr_hip._lib import ESR_E_ARG
    h = _lib.load_library()
    p, q, t, g = 0x1000, 0x2000, 0x3000, 0x4000
    down = h.esr_cem_downscale_per_image
    assert down(None, 2, 3, 8, 8, 4, 1, t, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 3, 8, 8, 4, 1, None, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 3, 8, 8, 4, 1, t, 5, None, 0, None, None) == ESR_E_ARG
    assert down(p, 0, 3, 8, 8, 4, 1, t, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 0, 8, 8, 4, 1, t, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 3, 0, 8, 4, 1, t, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 3, 8, 8, 0, 0, t, 5, None, 0, q, None) == ESR_E_ARG
    assert down(p, 2, 3, 8, 8, 4, 4, t, 5, None, 0, q, None) == ESR_E_ARG            # pre outside [0, sf)
    assert down(p, 2, 3, 8, 8, 4, 1, t, 4, None, 0, q, None) == ESR_E_ARG            # even k
    assert down(p, 2, 3, 8, 8, 4, 1, t, 5, g, 4, q, None) == ESR_E_ARG               # lr_pad leaves no LR image
    assert down(p, 2, 3, 8, 8, 4, 1, t, 5, g, -1, q, None) == ESR_E_ARG
    filt = h.esr_cem_lrfilter_per_image
    assert filt(None, 2, 3, 8, 8, t, 5, q, None) == ESR_E_ARG
    assert filt(p, 2, 3, 8, 8, None, 5, q, None) == ESR_E_ARG
    assert filt(p, 2, 3, 8, 8, t, 5, None, None) == ESR_E_ARG
    assert filt(p, 2, 3, 8, 8, t, 6, q, None) == ESR_E_ARG
    assert filt(p, 2, 3, 8, 0, t, 5, q, None) == ESR_E_ARG
    assert filt(p, -1, 3, 8, 8, t, 5, q, None) == ESR_E_ARG
    up = h.esr_cem_upscale_per_image
    assert up(None, None, 2, 3, 8, 8, 4, 1, t, 5, None, 0, 0, 0.0, q, None, None) == ESR_E_ARG
    assert up(p, None, 2, 3, 8, 8, 4, 1, None, 5, None, 0, 0, 0.0, q, None, None) == ESR_E_ARG
    assert up(p, None, 2, 3, 8, 8, 4, 1, t, 5, None, 0, 0, 0.0, None, None, None) == ESR_E_ARG
    assert up(p, None, 2, 3, 8, 8, 1, 0, t, 5, None, 0, 0, 0.0, q, None, None) == ESR_E_ARG          # sf < 2
    assert up(p, None, 2, 3, 8, 8, 4, 1, t, 5, None, 0, 4, 0.0, q, None, None) == ESR_E_ARG          # mode outside 0..3
    assert up(p, None, 2, 3, 8, 8, 4, 1, t, 5, None, 16, 0, 0.0, q, None, None) == ESR_E_ARG         # the crop leaves nothing
    assert up(p, None, 2, 3, 8, 8, 4, 1, t, 5, None, 0, 1, 0.0, q, None, None) == ESR_E_ARG          # mode 1 without g
    assert up(p, None, 2, 3, 8, 8, 4, 1, t, 5, g, 0, 2, 0.5, q, None, None) == ESR_E_ARG             # mode 2 without f2
    assert up(p, p, 2, 3, 8, 8, 4, 1, t, 5, g, 0, 3, 0.0, q, None, None) == ESR_E_ARG                # mode 3 without out2
