"""CPU tests of the VGG feature extractor's host side (define_F, VGGFeatureExtractor; reference codes/models/networks.py:185-197,
codes/models/modules/architecture.py:658-705): the module tree and state_dict keys follow torchvision's VGG `features`, the cut point follows
define_F's arch rule, weights come from the listed sources only, and what this build does not implement is refused."""
import os

import pytest
import torch
import torch.nn.functional as F

# torchvision.models.vgg cfgs, restated here so that the product's own table is checked against them
CFG = {'vgg16': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M'],
       'vgg19': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']}


def tv_features(arch):
    """[(kind, weight shape or None)] of torchvision's `features` for a cfg: Conv2d + ReLU per number, MaxPool2d per 'M'."""
    out, cin = [], 3
    for v in CFG[arch]:
        if v == 'M':
            out.append(('pool', None))
        else:
            out += [('conv', (v, cin, 3, 3)), ('relu', None)]
            cin = v
    return out


def seeded_state_dict(arch, upto, seed=0, extra=True):
    """A torchvision-format VGG state_dict (features.<i>.weight / bias, plus classifier entries the extractor ignores)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (kind, shape) in enumerate(tv_features(arch)[:upto + 1]):
        if kind == 'conv':
            sd['features.%d.weight' % i] = torch.randn(shape, generator=g) * (2.0 / (shape[0] * 9)) ** 0.5
            sd['features.%d.bias' % i] = torch.randn(shape[0], generator=g) * 0.01
    if extra:
        sd['classifier.0.weight'] = torch.zeros(4, 4)
    return sd


def _opt(path=None):
    from options.options import dict_to_nonedict
    return dict_to_nonedict({'gpu_ids': None, 'path': {'pretrained_model_F': path}})


def test_define_F_vgg19_keys_shapes_and_mode():
    import models.networks as networks
    sd = seeded_state_dict('vgg19', 34)
    netF = networks.define_F(_opt(), use_bn=False, state_dict=sd)
    expect = tv_features('vgg19')[:35]               # VGG19-54: conv5_4, before its ReLU (feature_layer 34)
    keys = [k for k in netF.state_dict()]
    want = []
    for i, (kind, shape) in enumerate(expect):
        if kind == 'conv':
            want += ['features.%d.weight' % i, 'features.%d.bias' % i]
    assert keys == ['mean', 'std'] + want or keys == want + ['mean', 'std'], keys
    for i, (kind, shape) in enumerate(expect):
        m = netF.features[i]
        assert {'conv': torch.nn.Conv2d, 'relu': torch.nn.ReLU, 'pool': torch.nn.MaxPool2d}[kind] is type(m), (i, m)
        if kind == 'conv':
            assert tuple(m.weight.shape) == shape and torch.equal(m.weight.detach(), sd['features.%d.weight' % i])
    assert len(netF.features) == 35 and isinstance(netF.features[-1], torch.nn.Conv2d)
    assert not netF.training
    assert not any(p.requires_grad for p in netF.parameters())
    assert torch.allclose(netF.mean.view(-1), torch.tensor([0.485, 0.456, 0.406])) and torch.allclose(netF.std.view(-1), torch.tensor([0.229, 0.224, 0.225]))


def test_cpu_forward_is_the_stock_chain():
    """CPU tensors run the stock modules (as Discriminator_VGG_128 does): normalisation, then features."""
    import models.modules.architecture as arch
    sd = seeded_state_dict('vgg16', 9, seed=3)
    net = arch.VGGFeatureExtractor(feature_layer=9, state_dict=sd, arch='vgg16')
    x = torch.rand(1, 3, 20, 18, generator=torch.Generator().manual_seed(4))
    y = (x - net.mean) / net.std
    for i in (0, 2, 5, 7):
        y = F.conv2d(y, sd['features.%d.weight' % i], sd['features.%d.bias' % i], padding=1)
        y = F.relu(y)
        if i in (2, 7):
            y = F.max_pool2d(y, 2)
    with torch.no_grad():
        got = net(x)
    assert got.shape == (1, 128, 5, 4)
    assert torch.allclose(got, y, rtol=1e-5, atol=1e-6)


def test_define_F_arch_suffix_cuts_where_the_reference_cuts():
    import models.networks as networks
    from esr_hip.vgg import parse_arch
    assert parse_arch('vgg16_22') == ('vgg16', 22) and parse_arch('vgg19') == ('vgg19', 34) and parse_arch('vgg19_35') == ('vgg19', 35)
    sd = seeded_state_dict('vgg16', 22, seed=1)
    netF = networks.define_F(_opt(), arch='vgg16_22', state_dict=sd)
    expect = tv_features('vgg16')[:23]          # ends with relu4_3
    assert len(netF.features) == 23 and isinstance(netF.features[-1], torch.nn.ReLU)
    assert [type(m).__name__ for m in netF.features] == [{'conv': 'Conv2d', 'relu': 'ReLU', 'pool': 'MaxPool2d'}[k] for k, _ in expect]


def test_weights_from_the_options_path(tmp_path):
    import models.networks as networks
    sd = seeded_state_dict('vgg19', 34, seed=2)
    p = str(tmp_path / 'vgg19_tv.pth')
    torch.save(sd, p)
    netF = networks.define_F(_opt(p))
    assert torch.equal(netF.features[34].weight.detach(), sd['features.34.weight'])


def test_missing_weights_name_every_source(tmp_path):
    import models.networks as networks
    old = torch.hub.get_dir()
    torch.hub.set_dir(str(tmp_path / 'hub'))
    try:
        with pytest.raises(FileNotFoundError) as e:
            networks.define_F(_opt(str(tmp_path / 'nothing.pth')))
    finally:
        torch.hub.set_dir(old)
    msg = str(e.value)
    assert 'state_dict=' in msg and 'pretrained_model_F' in msg and str(tmp_path / 'nothing.pth') in msg
    assert os.path.join(str(tmp_path / 'hub'), 'checkpoints', 'vgg19-dcbb9e9d.pth') in msg


def test_unsupported_variants_are_refused():
    import models.modules.architecture as arch
    import models.networks as networks
    sd = seeded_state_dict('vgg19', 34)
    with pytest.raises(NotImplementedError):
        networks.define_F(_opt(), use_bn=True, state_dict=sd)
    with pytest.raises(NotImplementedError):
        arch.VGGFeatureExtractor(state_dict=sd, arch_config='untrained_')
    with pytest.raises(NotImplementedError):
        arch.VGGFeatureExtractor(state_dict=sd, arch='SegNetAE')


def test_z_optimizer_lists_the_vgg_objectives():
    from Z_optimization import Z_optimizer
    assert 'VGG' in Z_optimizer.SUPPORTED and 'max_VGG' in Z_optimizer.SUPPORTED
