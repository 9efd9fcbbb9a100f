"""CPU-only: pins oracle/layout_ref.py (the restatement tests/test_gpu_layout_contract.py judges the boundary kernels by), shows that its
comparisons reject the errors such kernels make, and checks the argument refusals of the five entry points (host arithmetic, fake pointers).

  pack64       against F.pad(replicate) + F.interpolate(scale_factor=1/down, 'bilinear', align_corners=False) in float64
  exactness    the premise of the bit-exact /down family: on the 1/1024 grid an fp32 evaluation of the four-tap form equals the float64 one
  encode       against an integer-arithmetic round-to-nearest-even written here with numpy bit operations
  mutations    swapped lanes, a group shift, c0 + 1, a nonzero border vector / unused lane, zero padding for the clamp, the half-pixel offset
               dropped, the batch stride ignored, the lo plane left at zero: each changes the frame's bits, and each that changes a value fails the bound
  refusals     every ESR_E_ARG condition of esr_pack_nchw, esr_unpack_nchw, esr_zero, esr_pack_nchw_norm, esr_unpack_grad_nchw_norm, one at a time"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layout_ref as R


# ----------------------------------------------------------------------------- pack64
@pytest.mark.parametrize('down,pad,h,w', [(1, 0, 5, 7), (1, 3, 4, 1), (2, 0, 6, 8), (2, 1, 6, 4), (2, 2, 2, 6), (3, 0, 9, 3), (3, 3, 6, 9),
                                          (4, 0, 8, 12), (4, 2, 4, 8), (4, 4, 8, 4), (8, 0, 16, 8), (8, 4, 8, 16), (8, 8, 8, 8)])
def test_pack64_is_replicate_pad_then_interpolate(down, pad, h, w):
    B, C, c0, nc, extra = 2, 5, 1, 3, 11
    src = R.uniform((B, C * h * w + extra), down * 10 + pad).double()
    got = R.pack64(src, c0, nc, pad=pad, down=down, batch_stride=C * h * w + extra, hw=(h, w), channels=C)
    x = src[:, :C * h * w].view(B, C, h, w)[:, c0:c0 + nc]
    ref = F.pad(x, (pad,) * 4, mode='replicate') if pad else x
    if down > 1:
        ref = F.interpolate(ref, scale_factor=1.0 / down, mode='bilinear', align_corners=False)
    assert got.shape == ref.shape == (B, nc, (h + 2 * pad) // down, (w + 2 * pad) // down)
    assert float((got - ref).abs().max()) <= 4 * 2.0 ** -53          # values in [-1, 1]: a few float64 roundings
    # the 4-D form (no raw view) is the same function
    assert torch.equal(R.pack64(src[:, :C * h * w].view(B, C, h, w), c0, nc, pad=pad, down=down), got)


@pytest.mark.parametrize('down,pad', [(2, 0), (2, 1), (3, 3), (4, 2), (4, 4), (8, 4), (8, 8)])
def test_grid_inputs_make_the_fp32_four_tap_form_exact(down, pad):
    """Integers / 1024 in [-2, 2]: odd factors copy one pixel, even ones average with weights 0.5 — every product and sum is exact in fp32."""
    x = R.grid((2, 3, 8 * down, 3 * down), down + pad)
    p = R.pad_replicate(x, pad)
    hp, wp = p.shape[-2:]
    y0, y1, ly = R._taps(hp // down, hp, down, 0.5)
    x0, x1, lx = R._taps(wp // down, wp, down, 0.5)
    ly, lx = ly.float()[:, None], lx.float()
    one = torch.ones((), dtype=torch.float32)
    r0, r1 = p.index_select(-2, y0), p.index_select(-2, y1)
    v = (one - ly) * ((one - lx) * r0.index_select(-1, x0) + lx * r0.index_select(-1, x1)) \
        + ly * ((one - lx) * r1.index_select(-1, x0) + lx * r1.index_select(-1, x1))
    assert v.dtype == torch.float32
    assert torch.equal(v.double(), R.pack64(x, 0, 3, pad=pad, down=down))
    assert set(ly.flatten().tolist()) <= {0.0, 0.5} and set(lx.flatten().tolist()) <= {0.0, 0.5}


# ----------------------------------------------------------------------------- encode / decode
def _rne_bf16(u):
    """fp32 bit patterns (uint64 array) -> bf16 bit patterns, round to nearest even (finite inputs)."""
    keep, rem = u >> 16, u & 0xFFFF
    up = (rem > 0x8000) | ((rem == 0x8000) & ((keep & 1) == 1))
    return (keep + up) & 0xFFFF


def _rne_f16(u):
    """fp32 bit patterns -> fp16 bit patterns, round to nearest even, subnormal results included (|x| < 65520)."""
    sign, exp, man = (u >> 31) << 15, (u >> 23) & 0xFF, u & 0x7FFFFF
    e = exp.astype(np.int64) - 127 + 15
    full = man | 0x800000                                   # 24 significant bits
    shift = np.where(e >= 1, 13, np.clip(14 - e, 13, 40))   # bits dropped: 13 in the normal range, more below it
    keep = np.where(e >= 1, (e << 10) | (man >> 13), full >> shift)
    rem = np.where(e >= 1, man & 0x1FFF, full & ((np.int64(1) << shift) - 1))
    half = np.int64(1) << (shift - 1)
    up = (rem > half) | ((rem == half) & ((keep & 1) == 1))
    out = np.where(exp == 0, 0, keep + up)                  # fp32 zeros and subnormals: far below half the smallest fp16 subnormal
    return sign | out


def _np_encode(v, fmt):
    u = v.view(np.uint32).astype(np.int64)
    hi = (_rne_f16(u) if fmt else _rne_bf16(u)).astype(np.uint16)
    back = hi.view(np.float16).astype(np.float32) if fmt else (hi.astype(np.uint32) << 16).view(np.float32)
    res = (v - back).astype(np.float32)
    ur = res.view(np.uint32).astype(np.int64)
    lo = (_rne_f16(ur) if fmt else _rne_bf16(ur)).astype(np.uint16)
    return hi.view(np.int16), lo.view(np.int16)


def _check_encode(v, fmt):
    hi, lo = R.encode(v, fmt, 2)
    nh, nl = _np_encode(v.numpy(), fmt)
    assert np.array_equal(hi.numpy(), nh), 'hi'
    assert np.array_equal(lo.numpy(), nl), 'lo'
    assert torch.equal(R.encode(v, fmt, 1)[0], hi) and R.encode(v, fmt, 1)[1] is None
    return hi, lo


@pytest.mark.parametrize('fmt', [0, 1])
def test_encode_is_integer_rne(fmt):
    hi, lo = _check_encode(torch.cat([R.uniform((4096,), 1, -2.0, 2.0), R.uniform((4096,), 2, -1e-2, 1e-2), R.uniform((1024,), 3, -300.0, 300.0)]), fmt)
    assert int((lo != 0).sum()) > 4000                       # the residue plane is exercised
    # exact ties, both parities of the kept mantissa, both signs: to even
    drop = 13 if fmt else 16
    base = np.array([0x3F800000, 0x40490000, 0x3E99A000, 0xBF800000, 0xC2F6E000], dtype=np.int64) & ~((1 << (drop + 1)) - 1)
    for parity in (0, 1):
        u = base | (parity << drop) | (1 << (drop - 1))
        v = torch.from_numpy(u.astype(np.uint32).view(np.float32).copy())
        hi, lo = _check_encode(v, fmt)
        kept = (u >> drop) + parity                          # even stays, odd goes up
        want = (kept & 0xFFFF) if fmt == 0 else None
        if fmt == 0:
            assert np.array_equal(hi.numpy().view(np.uint16), want.astype(np.uint16))
        assert ((hi.numpy().view(np.uint16) & 1) == 0).all()
        back = R.decode(hi, lo, fmt)
        assert torch.equal(back, v)                          # the residue of a tie is half an ulp of hi: lo holds it exactly
    # already representable: lo is +0; +-0 keep their sign in hi and leave +0 in lo
    v = torch.tensor([1.0, -1.5, 0.15625, 2.0, 0.0, -0.0, 0.333251953125], dtype=torch.float32)
    hi, lo = _check_encode(v, fmt)
    if fmt:
        assert torch.equal(R.decode(hi, None, fmt), v)
    assert not bool(lo[:6].any())
    assert hi[4].item() == 0 and hi[5].item() == -32768
    # an absent lo counts as +0: a stored -0 decodes to +0 (and with a +0 lo as well)
    for l in (None, lo[5:6]):
        d = R.decode(hi[5:6], l, fmt)
        assert d.view(torch.int32).item() == 0
    for s in R.specials(fmt).split(1):
        _check_encode(s, fmt)


def test_encode_fp16_subnormal_range():
    v = torch.cat([R.uniform((4096,), 4, -6e-5, 6e-5), R.uniform((1024,), 5, -2.0 ** -24, 2.0 ** -24),
                   torch.tensor([2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-10, -1e-10])])
    hi, lo = _check_encode(v, 1)
    n = v.numel()
    assert hi[n - 8].item() == 1 and hi[n - 7].item() == 0 and hi[n - 6].item() == -32768 and hi[n - 5].item() == 2      # ties to even at the bottom
    assert hi[n - 3].item() == 0x0400                        # the tie below the smallest normal rounds up to it
    assert int(((hi.numpy().view(np.uint16) & 0x7C00) == 0).sum()) > 4000
    err = (R.decode(hi, lo, 1).double() - v.double()).abs()
    assert float(err.max()) <= 2.0 ** -25


def test_frame_and_unframe():
    v = R.uniform((2, 11, 3, 5), 6)
    for form, (fmt, planes) in R.FORMS.items():
        f = R.frame(v, fmt, planes, 3)
        assert f.shape == (planes, 2, 3, 5, 7, 8)
        got, clean = R.unframe(f, fmt, 11)
        hi, lo = R.encode(v, fmt, planes)
        assert clean and torch.equal(got, R.decode(hi, lo, fmt))
        assert R.accepts(got, v.double(), R.store_bound(form, v.double())), form
        assert f[0, 1, 1, 2, 3, 2].item() == hi[1, 10, 1, 2].item()          # channel 10 = group 1, lane 2; pixel (1, 2) at frame (2, 3)
        assert not bool(f[:, :, 1, :, :, 3:].any()) and not bool(f[:, :, 2].any())


# ----------------------------------------------------------------------------- mutations
def _mutation_case(down, pad):
    B, C, h, w, c0, nc, ncg, extra = 2, 13, 6, 8, 1, 11, 3, 37
    bs = C * h * w + extra
    src = R.uniform((B, bs), 20 + down)
    kw = dict(pad=pad, down=down, batch_stride=bs, hw=(h, w), channels=C)
    ref = R.pack64(src, c0, nc, **kw)
    S = R.pack64(src.abs(), c0, nc, **kw)
    return src, (B, C, h, w, c0, nc, ncg, bs), kw, ref, S


@pytest.mark.parametrize('form', list(R.FORMS))
def test_comparisons_reject_planted_errors(form):
    fmt, planes = R.FORMS[form]
    down, pad = 2, 1
    src, (B, C, h, w, c0, nc, ncg, bs), kw, ref, S = _mutation_case(down, pad)
    bound = 3 * R.U * S + R.store_bound(form, ref)
    good = R.frame(ref.float(), fmt, planes, ncg)
    got, clean = R.unframe(good, fmt, nc)
    assert clean and R.accepts(got, ref, bound)

    def planted(values):
        return R.frame(values.float(), fmt, planes, ncg)

    x = R.raw_view(src, B, C, h, w, c0, nc, bs)
    value_mutations = {
        'two lanes swapped': good[..., [0, 2, 1, 3, 4, 5, 6, 7]],
        'channels shifted by one group': torch.roll(good, 1, dims=2),
        'c0 off by one': planted(R.pack64(src, c0 + 1, nc, **kw)),
        'zero padding for the replicate clamp': planted(R.bilinear_down(F.pad(x, (pad,) * 4), down)),
        'half-pixel offset dropped': planted(R.bilinear_down(R.pad_replicate(x, pad), down, offset=0.0)),
        'batch stride ignored': planted(R.bilinear_down(R.pad_replicate(R.raw_view(src, B, C, h, w, c0, nc, 0), pad), down)),
    }
    if planes == 2:
        lo0 = good.clone()
        lo0[1] = 0
        value_mutations['lo plane left at zero'] = lo0
    for what, bad in value_mutations.items():
        assert not torch.equal(bad, good), what
        v, _ = R.unframe(bad, fmt, nc)
        assert R.worst_ratio(v, ref, bound) > 1.0, 'the comparator accepts: ' + what
    one = int(torch.tensor(1.0).to(R.DTYPE[fmt]).view(torch.int16))
    border = good.clone()
    border[0, 1, 0, 0, 2] = one
    lane = good.clone()
    lane[planes - 1, 0, (nc - 1) // 8, 2, 3, nc % 8] = one
    group = good.clone()
    group[0, 1, ncg - 1, 2, 2, 0] = one                      # (ncg = 3 groups hold 11 channels: the third is all zero)
    for what, bad in (('a nonzero border vector', border), ('a nonzero unused lane', lane), ('a nonzero group past the channels', group)):
        assert not torch.equal(bad, good), what
        v, clean = R.unframe(bad, fmt, nc)
        assert not clean, 'unframe calls clean: ' + what
        assert torch.equal(v, got)                           # (the interior values do not show it: the frame comparison has to)


def test_worst_ratio_edges():
    ref = torch.tensor([1.0, 0.0], dtype=torch.float64)
    b = torch.tensor([1e-6, 0.0], dtype=torch.float64)
    assert R.worst_ratio(ref.float(), ref, b) == 0.0                          # exact where the bound is zero
    assert R.worst_ratio(torch.tensor([1.0, 1e-30]), ref, b) > 1.0            # any error where the bound is zero
    assert R.worst_ratio(torch.tensor([float('nan'), 0.0]), ref, b) == float('inf')
    assert R.worst_ratio(torch.zeros(3), ref, b) == float('inf')
    assert abs(R.worst_ratio(torch.tensor([1.0 + 2.0 ** -21, 0.0]), ref, b) - 2.0 ** -21 / 1e-6) < 1e-9


# ----------------------------------------------------------------------------- refusals
E_ARG = -1


def _view(ncg=1, H=4, W=5, hi=16, lo=32, fmt=0):
    from esr_hip import _lib
    return _lib.ActView(hi, lo, ncg, H, W, ncg * (H + 2) * (W + 2), (H + 2) * (W + 2), fmt)


PACK_BASE = dict(src=64, sbs=0, B=2, C=5, h=6, w=8, c0=1, nc=3, pad=1, down=2, dst=dict())       # -> 4 x 5
PACK_REFUSED = {
    'src NULL': dict(src=None), 'dst NULL': dict(dst=None), 'dst->hi NULL': dict(dst=dict(hi=None)), 'B = 0': dict(B=0), 'B < 0': dict(B=-1),
    'nc = 0': dict(nc=0), 'c0 < 0': dict(c0=-1), 'c0 + nc > C': dict(c0=3), 'pad < 0': dict(pad=-1, dst=dict(H=2, W=3)),
    'down = 0': dict(down=0), 'down < 0': dict(down=-2),
    '(h + 2 pad) % down': dict(h=7), '(w + 2 pad) % down': dict(w=9), 'dst->H': dict(dst=dict(H=5)), 'dst->W': dict(dst=dict(W=4)),
    'dst->H is h, not the padded size': dict(dst=dict(H=3)), 'dst->ncg * 8 < nc': dict(C=12, nc=9),
    'h = 0': dict(h=0, dst=dict(H=1)), 'w = 0': dict(w=0, dst=dict(W=1)), 'h < 0': dict(h=-2, pad=2, dst=dict(H=1, W=6)),
    'w < 0': dict(w=-2, pad=2, dst=dict(H=5, W=1)),
}


def test_pack_nchw_refusals():
    import ctypes as C
    from esr_hip import _lib
    h = _lib.load_library()
    assert len(PACK_REFUSED) == 21
    for what, change in PACK_REFUSED.items():
        a = dict(PACK_BASE, **change)
        dst = _view(**a['dst']) if a['dst'] is not None else None
        rc = h.esr_pack_nchw(a['src'], a['sbs'], a['B'], a['C'], a['h'], a['w'], a['c0'], a['nc'], a['pad'], a['down'],
                             C.byref(dst) if dst is not None else None, None)
        assert rc == E_ARG, what


def test_unpack_nchw_and_zero_refusals():
    import ctypes as C
    from esr_hip import _lib
    h = _lib.load_library()
    cases = {'src NULL': (None, 2, 3, 64), 'src->hi NULL': (_view(hi=None), 2, 3, 64), 'dst NULL': (_view(), 2, 3, None), 'B = 0': (_view(), 0, 3, 64),
             'nc = 0': (_view(), 2, 0, 64), 'nc < 0': (_view(), 2, -8, 64), 'src->ncg * 8 < nc': (_view(), 2, 9, 64), 'H = 0': (_view(H=0), 2, 3, 64),
             'W = 0': (_view(W=0), 2, 3, 64), 'H < 0': (_view(H=-1, W=-1), 2, 3, 64)}
    for what, (v, B, nc, dst) in cases.items():
        assert h.esr_unpack_nchw(C.byref(v) if v is not None else None, B, nc, dst, None) == E_ARG, what
    assert h.esr_zero(None, 4, None) == E_ARG
    assert h.esr_zero(64, -1, None) == E_ARG
    assert h.esr_zero(64, 0, None) == 0                      # nothing to do, nothing launched


def test_pack_nchw_norm_refusals():
    import ctypes as C
    from esr_hip import _lib
    h = _lib.load_library()
    base = dict(src=64, B=2, C=3, h=4, w=5, mean=128, std=256, dst=dict())
    cases = {'src NULL': dict(src=None), 'dst NULL': dict(dst=None), 'dst->hi NULL': dict(dst=dict(hi=None)), 'B = 0': dict(B=0), 'C = 0': dict(C=0),
             'h = 0': dict(h=0, dst=dict(H=0)), 'w = 0': dict(w=0, dst=dict(W=0)), 'mean without std': dict(std=None), 'std without mean': dict(mean=None),
             'dst->H': dict(dst=dict(H=5)), 'dst->W': dict(dst=dict(W=4)), 'dst->ncg * 8 < C': dict(C=9)}
    for what, change in cases.items():
        a = dict(base, **change)
        dst = _view(**a['dst']) if a['dst'] is not None else None
        rc = h.esr_pack_nchw_norm(a['src'], a['B'], a['C'], a['h'], a['w'], a['mean'], a['std'], C.byref(dst) if dst is not None else None, None)
        assert rc == E_ARG, what


def test_unpack_grad_nchw_norm_refusals():
    import ctypes as C
    from esr_hip import _lib
    h = _lib.load_library()
    cases = {'G NULL': (None, 2, 3, 64), 'G->hi NULL': (_view(hi=None), 2, 3, 64), 'dst NULL': (_view(), 2, 3, None), 'B = 0': (_view(), 0, 3, 64),
             'C = 0': (_view(), 2, 0, 64), 'G->ncg * 8 < C': (_view(), 2, 9, 64), 'G->H = 0': (_view(H=0), 2, 3, 64), 'G->H < 0': (_view(H=-3), 2, 3, 64),
             'G->W = 0': (_view(W=0), 2, 3, 64)}
    for what, (v, B, Cc, dst) in cases.items():
        for std in (None, 128):
            assert h.esr_unpack_grad_nchw_norm(C.byref(v) if v is not None else None, B, Cc, std, dst, None) == E_ARG, what
