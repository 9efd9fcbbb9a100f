"""The phase launch of esr_conv3x3 (esr_conv3x3_desc.upsample_phases = 2, include/esr_hip.h): the conv behind a nearest x2 upsample as four
4-tap convs on the input grid with folded weights, against the float64 restatement of

    out = alpha * LeakyReLU(conv3x3(nearest_x2(in1)) + bias)

on the STORED operand values — the method, the buffers and the element-wise bound of tests/test_gpu_conv_contract.py (imported unchanged):

    |y - ref| <= c_w * S + c_out * |ref| + K * 2^-24 * S,   S = alpha * conv(|x|, |w|) + |bias|  (the UNFOLDED |w|),   K = 9 * input channels

The bound covers the phase form as it stands: a folded weight is a sum of at most four original taps, so |folded w| <= sum |w| and the weight
rounding c_w * S only shrinks; the fold itself adds at most three fp32 roundings per weight (3 * 2^-24 relative to sum |w|, inside
K * 2^-24 * S with K >= 144) and the accumulation has 4 * cin terms instead of 9 * cin.

Also here: the folded pack, read back, against the fold done in torch (bit for bit); the engine's inference forward, which runs every nearest
x2 upsampler in this form, against the reference's own outputs (the F4 golden, at that test's bars) and recorded against eager; and the
forwards that keep activations for a backward pass, which stay on the nine-tap launch.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_contract import DEV, E_ARG, E_UNSUPPORTED, FMTS, SENT, Buf, _A, _conv_rc

pytestmark = pytest.mark.gpu

SLOPE, ALPHA = 0.2, 0.75


def _weights(cin, cout, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    w = ((torch.rand(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(9 * cin)).float()
    b = ((torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1) * 0.25).float()
    return w, b


def fold_fp32(w):
    """[cout][cin][3][3] fp32 -> [4][cout][cin][3][3]: per phase p = 2 py + px the folded weight at its tap positions, zero elsewhere; fp32
    sums in the order of the header: row sums (lower index first), then the two column terms."""
    out = torch.zeros((4,) + tuple(w.shape), dtype=torch.float32)
    sets = {0: {0: (0,), 1: (1, 2)}, 1: {1: (0, 1), 2: (2,)}}          # phase bit -> tap position -> original taps
    for p in range(4):
        for ty, rows in sets[p >> 1].items():
            rs = w[:, :, rows[0], :] if len(rows) == 1 else w[:, :, rows[0], :] + w[:, :, rows[1], :]
            for tx, cols in sets[p & 1].items():
                out[p, :, :, ty, tx] = rs[:, :, cols[0]] if len(cols) == 1 else rs[:, :, cols[0]] + rs[:, :, cols[1]]
    return out


def _layout(B, Hs, Ws, cin, cout, fmt, seed):
    f = FMTS[fmt]
    w, b = _weights(cin, cout, seed)
    x = Buf(f, B, (cin + 7) // 8, Hs, Ws, fill='random', seed=seed)
    nout = (cout + 7) // 8
    o = Buf(f, B, nout + 2, 2 * Hs, 2 * Ws, fill='sentinel')          # one sentinel group in front of and one behind the destination
    return f, w, b, x, o, nout


def _reference(f, w, b, x, cin, wk=None):
    """float64 reference and bound scale S of alpha * LeakyReLU(conv(nearest_x2(stored x)) + bias), [B][cout][2H][2W]."""
    hi = x.values(lo=False)
    lo = x.values(lo=True) - hi
    up = lambda t: F.pad(t[:, :, 1:-1, 1:-1].repeat_interleave(2, 2).repeat_interleave(2, 3), (1, 1, 1, 1))
    Wk = torch.zeros(w.shape[0], hi.shape[1], 3, 3, dtype=torch.float64)
    Wk[:, :cin] = w.double() if wk is None else wk
    pre = F.conv2d(up(hi + lo), Wk) + b.double().view(1, -1, 1, 1)
    ref = ALPHA * torch.where(pre > 0, pre, SLOPE * pre)
    Wa = torch.zeros_like(Wk)
    Wa[:, :cin] = w.double().abs()
    S = ALPHA * F.conv2d(up(hi.abs() + lo.abs()), Wa) + b.double().abs().view(1, -1, 1, 1)
    return ref, S


def _excess(f, y, ref, S, cin_groups):
    K = 9 * 8 * cin_groups
    c_out = f.c_out_hilo if f.planes == 2 else f.c_out_hi
    err = (y - ref).abs()
    e = err / (f.c_w * S + c_out * ref.abs() + K * 2.0 ** -24 * S)
    e[err == 0] = 0.0
    e[torch.isnan(err)] = float('inf')
    return float(e.max())


def _run(fmt, B, Hs, Ws, cin, cout, seed=1, lds_stages=0):
    A = _A()
    f, w, b, x, o, nout = _layout(B, Hs, Ws, cin, cout, fmt, seed)
    ref, S = _reference(f, w, b, x, cin)
    G = (cin + 7) // 8

    def stored(buf):
        bits = buf.bits()
        written = torch.zeros(bits.shape[1:], dtype=torch.bool)
        written[:, 1:1 + nout, 1:-1, 1:-1] = True
        assert (bits[:, ~written] == SENT).all(), 'the launch wrote a border pixel or a group outside [0, ceil(cout/8))'
        return buf.values(1, nout)[:, :cout, 1:-1, 1:-1]

    saved = A.LDS_STAGES
    A.LDS_STAGES = lds_stages
    try:
        wd, bd = w.to(DEV), b.to(DEV)
        A.conv3x3(A.PackedConvPhases(wd, bd, split=f.split).get(), x.view(), B, Hs, Ws, cout, upsample_phases=2, act_slope=SLOPE, alpha=ALPHA,
                  out=o.view(1, nout + 1))
        torch.cuda.synchronize()
        y = stored(o)
        # the same inputs through upsample = 2 meet the same bound
        o2 = Buf(f, B, nout + 2, 2 * Hs, 2 * Ws, fill='sentinel')
        pc = (A.PackedConvSlices if cout > 64 else A.PackedConv)(wd, bd, 0, split=f.split).get()
        A.conv3x3(pc, x.view(), B, 2 * Hs, 2 * Ws, cout, upsample=2, act_slope=SLOPE, alpha=ALPHA, out=o2.view(1, nout + 1))
        torch.cuda.synchronize()
        y2 = stored(o2)
    finally:
        A.LDS_STAGES = saved
    e, e2 = _excess(f, y, ref, S, G), _excess(f, y2, ref, S, G)
    print('%s B%d %dx%d %d->%d stages %d: worst |y-ref|/bound phases %.3g, upsample=2 %.3g' % (fmt, B, Hs, Ws, cin, cout, lds_stages, e, e2))
    assert e <= 1.0, 'phase launch: element-wise bound exceeded, worst |y-ref|/bound = %.3g' % e
    assert e2 <= 1.0, 'upsample = 2 launch: element-wise bound exceeded, worst |y-ref|/bound = %.3g' % e2
    # planted error: the two folded rows of phase 0 swapped (tap rows 0 and 1 of the folded weight, i.e. source rows y - 1 and y)
    fw = fold_fp32(w).double()
    sw = fw[0].clone()
    sw[:, :, 0], sw[:, :, 1] = fw[0][:, :, 1], fw[0][:, :, 0]
    hi = x.values(lo=True)
    Wk = torch.zeros(cout, hi.shape[1], 3, 3, dtype=torch.float64)
    Wk[:, :cin] = sw
    pre = F.conv2d(hi, Wk) + b.double().view(1, -1, 1, 1)             # phase 0 on the source grid: out[2y][2x]
    bad = ref.clone()
    bad[:, :, 0::2, 0::2] = ALPHA * torch.where(pre > 0, pre, SLOPE * pre)
    assert _excess(f, y, bad, S, G) > 1.0, 'the comparator accepts a planted error: folded rows of phase 0 swapped'
    # (and the folded reference itself is the unfolded one: the restatement above is not what is being tested)
    Wk[:, :cin] = fw[0]
    pre = F.conv2d(hi, Wk) + b.double().view(1, -1, 1, 1)
    assert torch.allclose(ALPHA * torch.where(pre > 0, pre, SLOPE * pre), ref[:, :, 0::2, 0::2], rtol=0, atol=1e-5)


# (fmt, B, source H, source W, cin, cout): between them the five formats cover every shape, each format runs the two-tile shape 23 x 80
CASES = [
    ('split', 2, 9, 13, 64, 64), ('f16x3', 2, 9, 13, 16, 32), ('bf16', 2, 9, 13, 16, 32),
    ('split', 1, 23, 80, 64, 64), ('bf16', 1, 23, 80, 64, 64), ('f16', 1, 23, 80, 64, 64), ('f16x2', 1, 23, 80, 64, 64), ('f16x3', 1, 23, 80, 64, 64),
    ('split', 1, 1, 3, 64, 64), ('f16', 1, 1, 3, 64, 64),
    ('f16x2', 1, 7, 75, 64, 64), ('bf16', 1, 7, 75, 64, 64), ('split', 1, 7, 75, 64, 64),
]


@pytest.mark.parametrize('fmt,B,Hs,Ws,cin,cout', CASES, ids=['%s-B%d-%dx%d-%d-%d' % c for c in CASES])
def test_phase_launch(fmt, B, Hs, Ws, cin, cout):
    run_tiles = _tiling(fmt, B, Hs, Ws, cin, cout)
    if (Hs, Ws) == (23, 80):
        assert run_tiles[0] >= 2 and run_tiles[1] >= 2, run_tiles       # phase stores meet at tile edges in both directions
    _run(fmt, B, Hs, Ws, cin, cout)


def _tiling(fmt, B, Hs, Ws, cin, cout):
    import ctypes as C
    from esr_hip import _lib
    f = FMTS[fmt]
    d = _lib.Conv3x3Desc()
    d.in1 = Buf(f, B, (cin + 7) // 8, Hs, Ws).view()
    d.B, d.H, d.W, d.cout, d.upsample_phases = B, Hs, Ws, cout, 2
    t = (C.c_int32 * 4)()
    assert _lib.lib.esr_conv3x3_tiling(C.byref(d), t) == 0
    assert t[2] == 2 and t[3] == 2 * ((cout + 31) // 32)
    return list(t)


@pytest.mark.parametrize('fmt', ['split', 'bf16', 'f16x3'])
@pytest.mark.parametrize('stages', [1, 2])
def test_phase_launch_both_lds_forms(fmt, stages):
    """The one-stage form (two workgroups per CU, what the large launches run) and the two-stage form (small launches), forced."""
    _run(fmt, 1, 23, 80, 64, 64, seed=3, lds_stages=stages)


def test_phase_launch_many_tiles_one_stage():
    """More than 320 workgroups (14 images x 6 tiles x 4 slices): the launch size picks the one-stage form, and the slice-fastest tile order
    walks several images, an odd share per XCD."""
    assert 14 * 4 * math.prod(_tiling('split', 14, 23, 80, 64, 64)[:2]) > 320
    _run('split', 14, 23, 80, 64, 64, seed=5)


def test_phase_launch_wide_layers():
    """cout > 64 (four 32-channel blocks: eight slices) and a cout that fills neither its last block nor its last group."""
    _run('bf16', 1, 9, 13, 16, 128, seed=7)
    _run('split', 1, 9, 13, 16, 44, seed=8)


def test_phase_refusals():
    A = _A()
    f = FMTS['split']
    w, b = _weights(16, 32, 1)
    pc = A.PackedConvPhases(w.to(DEV), b.to(DEV), split=True).get()
    x = Buf(f, 1, 2, 8, 8, fill='random')
    o = Buf(f, 1, 4, 16, 16)
    side = lambda: Buf(f, 1, 4, 16, 16).view()
    base = dict(upsample_phases=2, act_slope=0.2, out=o.view())
    assert _conv_rc(pc, x.view(), 1, 8, 8, 32, **base) == 0
    for kw in (dict(in0=Buf(f, 1, 1, 8, 8).view()), dict(res1=side(), beta1=1.0), dict(res1=side(), beta1=1.0, res2=side(), beta2=1.0),
               dict(mask_src=side(), mask_cg=(0, 4)), dict(out2=side()), dict(out=None, out_nchw=torch.zeros(32 * 256, device=DEV)),
               dict(out_nchw=torch.zeros(32 * 256, device=DEV)), dict(pixel_shuffle=2), dict(in1_lo_groups=-1), dict(in1_lo_groups=1),
               dict(out=o.view(lo=False)), dict(upsample_phases=3), dict(upsample_phases=1)):
        assert _conv_rc(pc, x.view(), 1, 8, 8, 32, **dict(base, **kw)) == E_UNSUPPORTED, kw
    # sizes: H, W are the source size, the destination is twice as large; not together with upsample
    assert _conv_rc(pc, x.view(), 1, 8, 8, 32, **dict(base, out=Buf(f, 1, 4, 8, 8).view())) == E_ARG
    assert _conv_rc(pc, x.view(), 1, 16, 16, 32, **base) == E_ARG
    assert _conv_rc(pc, x.view(), 1, 16, 16, 32, **dict(base, upsample=2)) == E_ARG
    # upsample = 2 itself keeps working on the plain pack
    plain = A.PackedConv(w.to(DEV), b.to(DEV), 0, split=True).get()
    assert _conv_rc(plain, x.view(), 1, 16, 16, 32, upsample=2, act_slope=0.2, out=o.view()) == 0


@pytest.mark.parametrize('fmt', ['split', 'bf16', 'f16', 'f16x3'])
def test_folded_pack_bits(fmt):
    """The folded pack, unpacked on the host, is the fp32 fold computed in torch, split (or rounded to one plane) like any weight — bit for bit,
    through esr_pack_conv_weights and through the batched table path; the five dead tap positions of every phase hold zeros."""
    A = _A()
    f = FMTS[fmt]
    cin, cout = 24, 44
    w, b = _weights(cin, cout, 11)
    wd = w.to(DEV)
    planes = 2 if fmt in ('split', 'f16x3') else 1
    ncp = (cin // 8 + 1) // 2
    fw = fold_fp32(w)
    # expected[slice][cp][tap][mtile][plane][lane][8]: lane = (row & 31) + 32 * (K group & 1)
    want = torch.zeros(4, ncp, 9, 2, planes, 64, 8, dtype=torch.int16)
    for s in range(4):
        for m in range(2):
            p, c0 = (2 * s + m) & 3, 32 * (s >> 1)
            v = torch.zeros(32, ncp * 16, 3, 3)
            nr = min(32, cout - c0)
            v[:nr, :cin] = fw[p, c0:c0 + nr]
            v = v.reshape(32, ncp, 2, 8, 9).permute(1, 4, 2, 0, 3).reshape(ncp, 9, 64, 8)      # [cp][tap][half * 32 + row][8]
            hi = v.to(f.dtype)
            want[s, :, :, m, 0] = hi.view(torch.int16)
            if planes == 2:
                want[s, :, :, m, 1] = (v - hi.float()).to(f.dtype).view(torch.int16)
    pk = A.PackedConvPhases(wd, b.to(DEV), split=f.split).get()
    torch.cuda.synchronize()
    got = pk.wpack.cpu().view(torch.int16).reshape(want.shape)
    assert torch.equal(got, want)
    live = {0: (0, 1, 3, 4), 1: (1, 2, 4, 5), 2: (3, 4, 6, 7), 3: (4, 5, 7, 8)}
    for s in range(4):
        for m in range(2):
            dead = [t for t in range(9) if t not in live[(2 * s + m) & 3]]
            assert (got[s, :, dead, m] == 0).all()
    assert torch.equal(pk.bias[:cout].cpu(), b)
    # the batched path (what the engine's re-pack runs)
    pk2 = A.PackedConvPhases(wd, b.to(DEV), split=f.split)
    A.PackBatch().run([pk2])
    torch.cuda.synchronize()
    assert torch.equal(pk2.wpack.cpu().view(torch.int16).reshape(want.shape), want)


@pytest.mark.parametrize('precision', ['split', 'mixed'])
def test_engine_forward_uses_phases(precision):
    """RRDBNet x4, nb = 1, on 2 x 3 x 12 x 16: both upsamplers run the phase form (one launch each, the reference's outputs at the F4 test's
    bars), and the recorded replay equals the eager launches bit for bit."""
    from oracle.check_golden import load, rel_l2, rel_max
    from test_gpu_parity import _f4_input, _rrdb
    A = _A()
    g = load('rrdb_fwd_bwd.npz')['nb1_x4/out']
    net = _rrdb(1, 4, 0).to(DEV)
    net.set_precision(precision)
    eng = net.engine
    x = _f4_input(1, 4, 0)
    x2 = torch.cat([x, x], 0).to(DEV)
    seen, conv = [], A.conv3x3

    def spy(*a, **kw):
        if str(kw.get('name', '')).startswith('upconv'):
            seen.append((kw.get('upsample_phases', 0), kw.get('upsample', 1)))
        return conv(*a, **kw)

    outs = {}
    A.conv3x3 = spy
    try:
        for plans in (False, True):
            eng.use_plans = plans
            with torch.no_grad():
                outs[plans] = net(x2).cpu()
    finally:
        A.conv3x3 = conv
        eng.use_plans = True
    assert seen == [(2, 1)] * 4, seen                  # two upsamplers, issued once eagerly and once into the recording
    assert torch.equal(outs[True], outs[False])
    for i in range(2):
        y = outs[True][i:i + 1].numpy()
        assert rel_l2(y, g) < 1e-4 and rel_max(y, g) < 3e-4, (rel_l2(y, g), rel_max(y, g))


@pytest.mark.parametrize('train', [False, True], ids=['masks', 'activations'])
def test_engine_differentiable_forward_keeps_nine_taps(train):
    """A forward that keeps activations (train: every one, a parameter wants its gradient) or LeakyReLU masks (frozen weights, the Z search) for a
    backward pass launches its upsamplers with upsample = 2 on the nine-tap pack — the arithmetic the golden gradients were taken against — and
    agrees with the inference forward to the two forms' rounding (no bit identity between the two: DESIGN.md 3.1)."""
    from oracle.check_golden import rel_l2
    from test_gpu_parity import _f4_input, _rrdb
    A = _A()
    net = _rrdb(1, 4, 0).to(DEV)
    for p in net.parameters():
        p.requires_grad_(train)
    x = _f4_input(1, 4, 0).to(DEV)
    seen, conv = [], A.conv3x3

    def spy(pc, *a, **kw):
        if str(kw.get('name', '')).startswith('upconv'):
            seen.append((kw.get('upsample_phases', 0), kw.get('upsample', 1), type(pc).__name__))
        return conv(pc, *a, **kw)

    A.conv3x3 = spy
    net.engine.use_plans = False
    try:
        y = net(x.clone().requires_grad_(True))
        with torch.no_grad():
            y0 = net(x)
    finally:
        A.conv3x3 = conv
        net.engine.use_plans = True
    assert seen == [(0, 2, 'PackedConv')] * 2 + [(2, 1, 'PackedConvPhases')] * 2, seen
    # each form is held to 1e-4 of the reference's output (the F4 bars): 2e-4 between them
    assert rel_l2(y.detach().cpu().numpy(), y0.cpu().numpy()) < 2e-4
