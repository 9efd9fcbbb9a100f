"""Pins oracle/cem_contract_ref.py — the float64 restatement tests/test_gpu_cem_contract.py judges the CEM kernels by — and its comparator.
CPU only.

The restatement: reproduces the reference project's own outputs (tests/golden/cem_filter_ops.npz = F2, cem_forward.npz = F3, every case) from
the product's host-built fp32 taps to 1e-6 in relative L2 (one stated exception: the decomposed NS output of F3, see the test); agrees with oracle.cem_oracle, both evaluated in
float64 on the same float64 taps, to 1e-12; its separable (two 1-D passes) and 2-D evaluations agree to 1e-13.

The comparator: accepts the reference rounded to fp32 and REJECTS every planted error — one (smallest-magnitude) tap dropped, taps reversed
along one axis, tv and th swapped, pre off by one, the clamp replaced by zero padding on one side, one output row taken from the neighbouring
strip — for every op at the asymmetric synthetic taps of the GPU tests.  That is what keeps the derived bound from hiding a failure."""
import numpy as np
import pytest
import torch

from oracle import cem_contract_ref as R
from oracle import cem_oracle as co
from oracle.check_golden import load, rel_l2
from oracle.weights import seeded_uniform
from oracle.gen_golden import aniso_gaussian_kernel

F2_CASES = [('cubic_x4', 4, None, None), ('cubic_x2', 2, None, None), ('cubic_x3', 3, None, None), ('aniso_x4', 4, aniso_gaussian_kernel(), 0.1)]


def _product(sf, kernel, bound, **conf_over):
    """The product's CEM (host construction only): (module with the three fp32 tap sets, pre, margins_LR)."""
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    conf = C.Get_CEM_Conf(sf)
    if bound:
        conf.lower_magnitude_bound = bound
    cem = C.CEMnet(conf, upscale_kernel=kernel)
    for k, v in conf_over.items():
        setattr(cem.conf, k, v)
    net = cem.WrapArchitecture_PyTorch(generated_image=None)
    imresize.kernels = {}
    return net, net.pre_stride, int(cem.invalidity_margins_LR)


def _taps(net):
    return (net.DownscaleOP.taps().detach(), net.Conv_LR_with_Inv_hTh_OP.taps().detach(), net.Upscale_OP.taps().detach())


@pytest.mark.parametrize('name,sf,kernel,bound', F2_CASES, ids=[c[0] for c in F2_CASES])
def test_reproduces_reference_filter_ops(name, sf, kernel, bound):
    g = load('cem_filter_ops.npz')
    net, pre, _ = _product(sf, kernel, bound)
    td, ti, tu = _taps(net)
    lr = seeded_uniform((2, 3, 20, 24), 11)
    hr = seeded_uniform((2, 3, 20 * sf, 24 * sf), 12)
    assert rel_l2(R.downscale(hr, td, sf, pre)[0].numpy(), g[name + '/DownscaleOP']) < 1e-6
    assert rel_l2(R.lrfilter(lr, ti)[0].numpy(), g[name + '/Conv_LR_with_Inv_hTh_OP']) < 1e-6
    assert rel_l2(R.upscale(lr, tu, sf, pre)[0].numpy(), g[name + '/Upscale_OP']) < 1e-6
    if kernel is None:
        # CEM_downsampler: HR replicate-padded by sf * ds_half, downscaled, un-padded (reference CEMnet.py:414-428)
        m = co.CEMTaps(sf).ds_half
        for key, y in (('/CEM_downsampler', hr), ('/CEM_downsampler_gray', hr[:, :1])):
            d = R.downscale(R.pad_replicate(y.double(), sf * m), td, sf, pre)[0][:, :, m:-m, m:-m]
            assert rel_l2(d.numpy(), g[name + key]) < 1e-6


def _project(lr, gen, net, pre, sf, mL, mode=1, rng=0.0):
    """CEM_PyTorch.forward after the generator call out of the restatement: mL = 0 is train mode, else eval (pad both, crop sf * mL).
    Returns (value, S) as filter_upscale does (S of the last stage, its operand taken as exact)."""
    td, ti, tu = _taps(net)
    gp = R.pad_replicate(gen.double(), sf * mL)
    if mode == 1:
        e = R.downscale(gp, td, sf, pre, lr=lr, lr_pad=mL)[0]
        return R.filter_upscale(e, ti, tu, sf, pre, g=gp, crop=sf * mL, mode=1)
    lrp = R.pad_replicate(lr.double(), mL)
    return R.filter_upscale(lrp, ti, tu, sf, pre, e2=R.downscale(gp, td, sf, pre)[0], g=gp, crop=sf * mL, mode=mode, range=rng)


def test_reproduces_reference_forward():
    g = load('cem_forward.npz')
    for name, sf, kernel, bound in [('cubic_x4', 4, None, None), ('cubic_x2', 2, None, None), ('aniso_x4', 4, aniso_gaussian_kernel(), 0.1)]:
        net, pre, mL = _product(sf, kernel, bound)
        lr = seeded_uniform((2, 3, 12, 16), 21)
        gen = seeded_uniform((2, 3, 12 * sf, 16 * sf), 22)
        assert rel_l2(_project(lr, gen, net, pre, sf, 0)[0].numpy(), g[name + '/train']) < 1e-6, name
        assert rel_l2(_project(lr, gen, net, pre, sf, mL)[0].numpy(), g[name + '/eval']) < 1e-6, name
    net, pre, mL = _product(4, None, None)
    lr = seeded_uniform((2, 3, 12, 16), 21)
    gen = seeded_uniform((2, 3, 48, 64), 22)
    assert rel_l2(_project(lr, gen, net, pre, 4, 0, mode=2, rng=1.0)[0].numpy(), g['cubic_x4_sigmoid/train']) < 1e-6       # tanh range: input_range [0, 1]
    (ortho, ns), (_, s_ns) = _project(lr, gen, net, pre, 4, 0, mode=3)
    assert rel_l2(ortho.numpy(), g['cubic_x4_decomposed/train_ortho']) < 1e-6
    # The one exception.  NS = g - U(K(D(g))) is what is left of g after three chained fp32 filters in the fixture: the fixture's own rounding
    # scales with the magnitude S = |g| + U(K(D(|g|))) on absolute taps (13 x the norm of NS here), not with NS.  Plain relative L2 is 1.4e-6
    # for this output (the restatement agrees with cem_oracle in float64 to 1e-12 on it, below); it is held to 1e-6 of the norm of S instead.
    assert float((ns - torch.from_numpy(g['cubic_x4_decomposed/train_NS']).double()).norm() / s_ns.norm()) < 1e-6
    assert rel_l2(_project(lr, gen, net, pre, 4, mL)[0].numpy(), g['cubic_x4_decomposed/eval']) < 1e-6


@pytest.mark.parametrize('name,sf,kernel,bound', F2_CASES, ids=[c[0] for c in F2_CASES])
def test_agrees_with_cem_oracle_in_float64(name, sf, kernel, bound):
    """Same float64 taps, same float64 inputs (the F2 and F3 ones) through both restatements."""
    t = co.CEMTaps(sf, kernel, lower_magnitude_bound=bound or 0.01)
    td = torch.from_numpy(np.ascontiguousarray(np.rot90(t.ds_kernel, 2)))
    ti = torch.from_numpy(np.ascontiguousarray(t.inv_hTh))
    tu = torch.from_numpy(np.ascontiguousarray(t.ds_kernel * sf ** 2))
    lr = seeded_uniform((2, 3, 20, 24), 11).double()
    hr = seeded_uniform((2, 3, 20 * sf, 24 * sf), 12).double()
    assert (R.downscale(hr, td, sf, t.pre)[0] - co.downscale_op(hr, t)).abs().max() < 1e-12
    assert (R.lrfilter(lr, ti)[0] - co.conv_lr_with_inv_hTh(lr, t)).abs().max() < 1e-12
    assert (R.upscale(lr, tu, sf, t.pre)[0] - co.upscale_op(lr, t)).abs().max() < 1e-12
    lr = seeded_uniform((2, 3, 12, 16), 21).double()
    gen = seeded_uniform((2, 3, 12 * sf, 16 * sf), 22).double()
    e = R.downscale(gen, td, sf, t.pre, lr=lr)[0]
    assert (R.filter_upscale(e, ti, tu, sf, t.pre, g=gen, mode=1)[0] - co.cem_project(lr, gen, t)).abs().max() < 1e-12
    dg = R.downscale(gen, td, sf, t.pre)[0]
    assert (R.filter_upscale(lr, ti, tu, sf, t.pre, e2=dg, g=gen, mode=2, range=1.0)[0] - co.cem_project(lr, gen, t, sigmoid_range=(0, 1))).abs().max() < 1e-12
    o = co.cem_project(lr, gen, t, decomposed=True)
    mine = R.filter_upscale(lr, ti, tu, sf, t.pre, e2=dg, g=gen, mode=3)[0]
    assert (mine[0] - o[0]).abs().max() < 1e-12 and (mine[1] - o[1]).abs().max() < 1e-12
    mL = t.margins_LR
    gp = R.pad_replicate(gen, sf * mL)
    e = R.downscale(gp, td, sf, t.pre, lr=lr, lr_pad=mL)[0]
    assert (R.filter_upscale(e, ti, tu, sf, t.pre, g=gp, crop=sf * mL, mode=1)[0] - co.cem_project(lr, gen, t, pre_pad=True)).abs().max() < 1e-12


@pytest.mark.parametrize('sf,k,pre', [(1, 7, 0), (2, 9, 1), (3, 15, 2), (4, 17, 0), (5, 11, 3), (8, 33, 7)])
def test_separable_and_2d_evaluations_agree(sf, k, pre):
    sep = R.synthetic_sep(k, k + sf)
    full = R.taps_2d(sep)
    hr, lr = R.uniform((2, 2, 6 * sf, 7 * sf), 1), R.uniform((2, 2, 6, 7), 2)
    g = R.uniform((2, 2, 6 * sf, 7 * sf), 3, 0.0, 1.0)
    for a, b in ((R.downscale(hr, sep, sf, pre, lr=lr[:, :, 1:-1, 1:-1], lr_pad=1), R.downscale(hr, full, sf, pre, lr=lr[:, :, 1:-1, 1:-1], lr_pad=1)),
                 (R.lrfilter(lr, sep), R.lrfilter(lr, full))):
        assert (a[0] - b[0]).abs().max() < 1e-13 and (a[1] - b[1]).abs().max() < 1e-13
    if sf > 1:
        a, b = R.upscale(lr, sep, sf, pre, g=g, crop=1, mode=1), R.upscale(lr, full, sf, pre, g=g, crop=1, mode=1)
        assert (a[0] - b[0]).abs().max() < 1e-13 and (a[1] - b[1]).abs().max() < 1e-13
        a, b = R.adjoint('upscale', hr, sep, sf, pre, lr.shape), R.adjoint('upscale', hr, full, sf, pre, lr.shape)
        assert (a[0] - b[0]).abs().max() < 1e-13 and (a[1] - b[1]).abs().max() < 1e-13


# ---- the comparator ------------------------------------------------------------------------------------------------------------------
# (op, sf, k, pre): the synthetic taps of the GPU families — a wave-kernel size, a generic-sf tile size, the x2 replicate rule, a filter size
OPS = [('down', 4, 17, 1), ('down', 8, 33, 3), ('down', 5, 11, 0), ('down_fused', 3, 15, 2), ('filt', 1, 27, 0), ('up0', 4, 17, 1), ('up1', 3, 15, 1),
       ('up2', 2, 9, 0), ('up3', 8, 33, 6), ('up0', 2, 9, 1), ('fold', 4, 17, 1), ('adj_down', 4, 17, 3), ('adj_filt', 1, 27, 0), ('adj_up', 2, 9, 0)]
ERRORS = ['drop', 'reverse', 'swap', 'pre', 'zero_pad', 'row']
KF = 27
RANGE = 0.75


def _evaluate(op, taps, sf, pre, sep):
    """(value(s), bound(s)) of one op on its fixed seeded inputs: lists of tensors, one entry per output."""
    k = R.tap_size(taps)
    n = 2 * k if sep else k * k
    h, w = 9, 11
    lr = R.uniform((1, 2, h, w), 11)
    lr2 = R.uniform((1, 2, h, w), 12)
    hr = R.uniform((1, 2, h * sf, w * sf), 13)
    g = R.uniform((1, 2, h * sf, w * sf), 14, 0.0, 1.0)
    if op == 'down':
        v, S = R.downscale(hr, taps, sf, pre)
        return [v], [R.bound(n, S, v)]
    if op == 'down_fused':
        v, S = R.downscale(hr, taps, sf, pre, lr=lr[:, :, 2:-2, 2:-2], lr_pad=2)
        return [v], [R.bound(n, S, v)]
    if op == 'filt':
        v, S = R.lrfilter(lr, taps)
        return [v], [R.bound(n, S, v)]
    if op in ('up0', 'up1', 'up2', 'up3', 'fold'):
        mode = 1 if op == 'fold' else int(op[2])
        if op == 'fold':
            v, S = R.filter_upscale(lr, R.synthetic_sep(KF, 77), taps, sf, pre, g=g, crop=1, mode=1)
            n += 2 * KF
        else:
            v, S = R.upscale(lr, taps, sf, pre, f2=lr2, g=g, crop=1, mode=mode, range=RANGE)
        if mode == 0:
            return [v], [R.bound(n, S, v)]
        if mode == 1:
            return [v], [R.bound(n, S, v, g[:, :, 1:-1, 1:-1])]
        if mode == 2:
            return [v], [R.bound_mode2(n, S, g, 1, RANGE)]
        return list(v), [R.bound(n, S[0], v[0]), R.bound(n, S[1], v[1], g[:, :, 1:-1, 1:-1])]
    kind = {'adj_down': 'downscale', 'adj_filt': 'lrfilter', 'adj_up': 'upscale'}[op]
    dy, shape = (lr, hr.shape) if kind == 'downscale' else (lr, lr.shape) if kind == 'lrfilter' else (hr, lr.shape)
    v, S = R.adjoint(kind, dy, taps, sf, pre, shape)
    return [v], [R.bound(R.adjoint_terms(k, sf if kind == 'downscale' else 1, dy.shape[2], dy.shape[3], sep), S, v)]


def _smallest_dropped(taps, sep):
    if sep:
        tv, th = taps[0].clone(), taps[1].clone()
        th[th.abs().argmin()] = 0.0
        return tv, th
    t = taps.clone()
    t.view(-1)[t.abs().argmin()] = 0.0
    return t


def _cases():
    for op, sf, k, pre in OPS:
        for sep in (True, False):
            for err in ERRORS:
                if err == 'pre' and sf == 1:
                    continue          # the LR filter has no pre
                if err == 'zero_pad' and (op.startswith('up') or op == 'adj_up') and 0 < pre < sf - 1:
                    continue          # the upscale pads a zero-stuffed image: with no sample on its border rows the padding holds zeros either way
                yield pytest.param(op, sf, k, pre, sep, err, id='%s-x%d-k%d-pre%d-%s-%s' % (op, sf, k, pre, 'sep' if sep else '2d', err))


@pytest.mark.parametrize('op,sf,k,pre,sep', [pytest.param(*o, s, id='%s-x%d-k%d-pre%d-%s' % (*o, 'sep' if s else '2d')) for o in OPS for s in (True, False)])
def test_comparator_accepts_the_reference_rounded_to_fp32(op, sf, k, pre, sep):
    taps = R.synthetic_sep(k, 3) if sep else R.synthetic_2d(k, 3)
    if sep:
        assert not torch.equal(taps[0], taps[1]) and not torch.equal(taps[0], taps[0].flip(0)) and not torch.equal(taps[1], taps[1].flip(0))
        assert (taps[0] < 0).any() and (taps[0] > 0).any() and min(float(taps[0].abs().min()), float(taps[1].abs().min())) >= 0.2 / k
    assert float(R.taps_2d(taps).abs().min()) >= 0.2 / k
    vals, bnds = _evaluate(op, taps, sf, pre, sep)
    for v, b in zip(vals, bnds):
        assert R.accepts(v.float(), v, b)
        assert not R.accepts(torch.full_like(v, float('nan')).float(), v, b)


@pytest.mark.parametrize('op,sf,k,pre,sep,err', list(_cases()))
def test_comparator_rejects_planted_error(op, sf, k, pre, sep, err, monkeypatch):
    taps = R.synthetic_sep(k, 3) if sep else R.synthetic_2d(k, 3)
    vals, bnds = _evaluate(op, taps, sf, pre, sep)
    if err == 'row':                 # one output row taken from the next one (the first row of the neighbouring strip)
        wrong = [v.clone() for v in vals]
        for v in wrong:
            v[:, :, v.shape[2] // 2] = v[:, :, v.shape[2] // 2 + 1]
    else:
        wt, wpre = taps, pre
        if err == 'drop':
            wt = _smallest_dropped(taps, sep)
        elif err == 'reverse':
            wt = (taps[0].flip(0), taps[1]) if sep else taps.flip(0)
        elif err == 'swap':
            wt = (taps[1], taps[0]) if sep else taps.t().contiguous()
        elif err == 'pre':
            wpre = (pre + 1) % sf
        else:
            real = R.pad_replicate
            # (the side whose padding holds samples: the zero-stuffed image of an upscale with pre == sf - 1 has them on its LAST row only)
            bottom = (op.startswith('up') or op == 'adj_up') and pre == sf - 1 and pre > 0

            def zero_side(x, p):
                xp = real(x, p).clone()
                if p:
                    xp[..., (xp.shape[-2] - p if bottom else 0):(xp.shape[-2] if bottom else p), :] = 0.0
                return xp
            monkeypatch.setattr(R, 'pad_replicate', zero_side)
        wrong, _ = _evaluate(op, wt, sf, wpre, sep)
    assert not all(R.accepts(wv.float(), v, b) for wv, v, b in zip(wrong, vals, bnds))
