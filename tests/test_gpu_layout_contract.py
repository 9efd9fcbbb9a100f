"""The entry points that move data across the module boundary — esr_pack_nchw, esr_unpack_nchw, esr_zero (csrc/esr_pack.hip), esr_pack_nchw_norm,
esr_unpack_grad_nchw_norm (csrc/esr_vgg.hip) — against oracle/layout_ref.py, bit for bit wherever the header leaves no freedom.  (The restatement is
pinned on the CPU by tests/test_host_layout_ref.py, which also shows that the comparisons used here reject swapped lanes, a group shift, c0 + 1, a
nonzero border / unused lane, zero padding for the clamp, a dropped half-pixel offset, an ignored batch stride and a missing lo plane.)

Method (as tests/test_gpu_bwd_helpers.py): the C ABI is called directly through esr_hip._lib.  Every family runs over the four forms bf16,
split bf16 (hi + lo), f16, f16 hi + lo unless noted.  Shapes are the smallest that break a one-thread-per-vector kernel: B = 2 or 3, nc in
{3, 8, 11, 13}, H != W down to W = 1 or H = 1, totals that are no multiple of 256 and exceed one block.

Guards: every destination is a view (images [0, B) of B + 1, groups [1, 1 + ncg) of ncg + 2) of a buffer that lies, 64 words either side, inside an
allocation filled with the sentinel 0x7FA5 (a NaN in both formats): after the launch everything outside the view is bit-identical and no sentinel
survives inside.  fp32 destinations are carved the same way.  Sources hold NaN wherever the launch must not read: channels outside [c0, c0 + nc),
the gap between images, and for stored sources the border, the lanes >= nc and the groups outside the view.

Families:
  pack_exact        down = 1: planes == frame(encode(x)) on both planes; pad {0, 1, 3} x c0 {0, 2, C - nc}, a view one group wider than nc needs
                    (the c0 = 2 launches); uniform [-2, 2] plus +-0, exact ties of both 16-bit roundings, representable values, 1e30 (bf16 forms);
                    the fp16 subnormal range in a case of its own
  pack_down_exact   down {2, 3, 4, 8} x pad {0, down / 2, down} on integers / 1024: every fp32 product and sum is exact, so the planes equal
                    encode(pack64) — every index, clamp and the half-pixel offset with no tolerance
  pack_down_bound   the same on uniform [-1, 1]:  |decode(stored) - pack64| <= 3 u S + c |ref| + a, u = 2^-24, S the same form of |x| (three additions
                    round, the products by 0 / 0.5 / 1 are exact, contraction only removes roundings); c, a: layout_ref.STORE
  raw_view          esr_hip.act.pack_nchw as the generator engine calls it: the latent through the raw HR view (down = sf and its down = 1 twin) and
                    the LR image at c0 = Ct - 3
  views             ActBuf.view(cg0 = 2) of 5 groups, LaneBuf (b0 = 1), act.stacked_at + view_of: same bits as the plain buffer, neighbours untouched;
                    ActBuf.to_nchw(nc, cg0) == decode
  unpack_exact      planes written here (random hi, a lo that is not hi's residue, -0, NaN in border / unused lanes / other groups) == decode, bitwise
  zero              n16 in {0, 1, 255, 256, 257, 4096 * 256 + 257} (the last: the grid-stride loop), 16 bytes into the allocation
  pack_norm         no mean / std: bit-exact; std a power of two with mean = k / 1024 on the 1 / 1024 grid: bit-exact; VGG's mean / std on uniform [0, 1]:
                    4 u |ref| + store (u the subtraction, relative to its result; 3 u a division expanded into reciprocal, multiply, correction);
                    C in {3, 11}, a view one group wider than C, border zero
  unpack_grad_norm  std NULL / a power of two: bit-exact; VGG's std: 3 u |ref|; C ragged against G->ncg, the other lanes and groups NaN
  adjoint           <decode(pack(x)), decode(G)> == <x, esr_unpack_grad_nchw(G)> in float64, x on the 1 / 1024 grid (the pack rounds nothing),
                    within sum |x| 4 ((pad + 1)^2 + 1) u S (tests/test_gpu_bwd_helpers.py's unpack_grad bound, S the adjoint of |G|)
  run_list          [OP_ZERO, OP_PACK_NCHW, OP_UNPACK_NCHW] through esr_run == the three direct calls, byte for byte
  repeatability     two calls of each entry point give equal bits

Largest observed error / bound per bounded family on an MI355X (a record, not a tolerance; comparisons in brackets):
  pack_down_bound 0.986 (44)   pack_norm 0.979 (8)   unpack_grad_norm 0.319 (8)   adjoint 2.4e-06 (20)
(pack_down_bound and pack_norm: the single bf16 plane, whose store constant 2^-8 is the format's own half ulp at the bottom of a binade; the
two-plane forms stay below 0.9.  adjoint: a stored G carries 16 significant bits or fewer, so nearly every fp32 sum of the gather is exact.)"""
import ctypes as C
import math

import pytest
import torch

from oracle import layout_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0x7FA5                   # NaN as bf16 and as fp16
GUARD = 64                      # words either side of a carved buffer (keeps its 16-byte alignment)
FORMS = list(R.FORMS)
NAN = float('nan')
VGG_MEAN, VGG_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _L():
    from esr_hip import _lib
    return _lib


def _lib():
    return _L().load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(family, ratio):
    print('layout_contract %s %.3g' % (family, ratio))


class Carve:
    """An activation buffer [planes][B + 1][ncg + 2][H + 2][W + 2][8] inside a sentinel-filled allocation; the view is images [0, B), groups
    [1, 1 + ncg)."""

    def __init__(self, form, B, ncg, H, W):
        self.fmt, self.P = R.FORMS[form]
        self.B, self.ncg, self.H, self.W = B, ncg, H, W
        self.shape = (self.P, B + 1, ncg + 2, H + 2, W + 2, 8)
        self.n = math.prod(self.shape)
        self.all = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.int16, device=DEV)
        self.t = self.all[GUARD:GUARD + self.n].view(self.shape)
        assert self.t.data_ptr() % 16 == 0

    def view(self):
        cs = (self.H + 2) * (self.W + 2)
        hi = self.t.data_ptr() + cs * 16
        return _L().ActView(hi, hi + self.t.stride(0) * 2 if self.P == 2 else None, self.ncg, self.H, self.W, (self.ncg + 2) * cs, cs, self.fmt)

    def put(self, img):
        """img: int16 [planes][B][ncg][H + 2][W + 2][8], the whole view."""
        self.t[:, :self.B, 1:1 + self.ncg] = img.to(DEV)

    def verify(self):
        """The view's image after a launch that had to write all of it and nothing else."""
        a = self.all.cpu()
        box = a[GUARD:GUARD + self.n].view(self.shape)
        inside = box[:, :self.B, 1:1 + self.ncg].clone()
        box[:, :self.B, 1:1 + self.ncg] = SENT
        assert bool((a == SENT).all()), 'written outside the destination view'
        assert not bool((inside == SENT).any()), 'a sentinel survives inside the destination view'
        return inside


class CarveF32:
    """fp32 [shape] with GUARD NaN words either side, NaN inside until written."""

    def __init__(self, *shape):
        self.shape, self.n = shape, math.prod(shape)
        self.all = torch.full((GUARD + self.n + GUARD,), NAN, dtype=torch.float32, device=DEV)
        self.t = self.all[GUARD:GUARD + self.n].view(shape)

    def verify(self):
        a = self.all.cpu()
        assert bool(torch.isnan(a[:GUARD]).all()) and bool(torch.isnan(a[GUARD + self.n:]).all()), 'written outside the fp32 destination'
        return a[GUARD:GUARD + self.n].view(self.shape).clone()


def _source(x, C_, c0, extra=0):
    """x [B][nc][h][w] as channels [c0, c0 + nc) of a NaN-filled [B][C_ * h * w + extra] fp32 buffer: (cpu tensor, device tensor, batch stride arg)."""
    B, nc, h, w = x.shape
    s = torch.full((B, C_ * h * w + extra), NAN, dtype=torch.float32)
    s[:, :C_ * h * w].view(B, C_, h, w)[:, c0:c0 + nc] = x
    return s, s.to(DEV), (C_ * h * w + extra if extra else 0)


def _pack(dev_src, sbs, B, C_, h, w, c0, nc, pad, down, carve):
    v = carve.view()
    assert _lib().esr_pack_nchw(dev_src.data_ptr(), sbs, B, C_, h, w, c0, nc, pad, down, C.byref(v), _stream()) == 0
    torch.cuda.synchronize()
    return carve.verify()


def _with_specials(x, fmt):
    s = R.specials(fmt)
    flat = x.view(x.shape[0], -1)
    assert flat.shape[1] >= s.numel()
    for b in range(x.shape[0]):
        flat[b, :s.numel()] = s.roll(b)
    return x


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _planes_diff(got, want):
    """'' when equal, else where the first differing element lies."""
    if torch.equal(got, want):
        return ''
    i = (got != want).nonzero()[0].tolist()
    return 'first difference at [plane, b, cg, Y, X, lane] = %s: got 0x%04X, want 0x%04X (%d elements differ)' % (
        i, got[tuple(i)].item() & 0xFFFF, want[tuple(i)].item() & 0xFFFF, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# pack_exact

EXACT_SHAPES = [(2, 13, 3, 5, 7), (3, 13, 8, 1, 9), (2, 16, 11, 6, 1), (2, 15, 13, 23, 17)]        # (B, C, nc, h, w)


@pytest.mark.parametrize('B,Cc,nc,h,w', EXACT_SHAPES, ids=['%dx%dx%dx%d' % (s[0], s[2], s[3], s[4]) for s in EXACT_SHAPES])
@pytest.mark.parametrize('form', FORMS)
def test_pack_exact(form, B, Cc, nc, h, w):
    fmt, planes = R.FORMS[form]
    for pad in (0, 1, 3):
        for c0 in (0, 2, Cc - nc):
            ncg = (nc + 7) // 8 + (1 if c0 == 2 else 0)
            x = _with_specials(R.uniform((B, nc, h, w), 100 * pad + c0 + nc, -2.0, 2.0), fmt)
            cpu, dev, sbs = _source(x, Cc, c0, extra=0 if c0 == 0 else 19)
            got = _pack(dev, sbs, B, Cc, h, w, c0, nc, pad, 1, Carve(form, B, ncg, h + 2 * pad, w + 2 * pad))
            want = R.frame(R.pad_replicate(x, pad), fmt, planes, ncg)
            assert torch.equal(R.pack64(cpu, c0, nc, pad=pad, batch_stride=sbs, hw=(h, w), channels=Cc), R.pad_replicate(x, pad).double())
            d = _planes_diff(got, want)
            assert not d, 'pad %d c0 %d: %s' % (pad, c0, d)


@pytest.mark.parametrize('form', ['f16', 'f16x2'])
def test_pack_exact_fp16_subnormal_range(form):
    fmt, planes = R.FORMS[form]
    B, Cc, c0, nc, h, w = 2, 5, 1, 3, 7, 9
    x = R.uniform((B, nc, h, w), 31, -6e-5, 6e-5)
    x.view(-1)[:8] = torch.tensor([2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-10, -1e-10])
    cpu, dev, sbs = _source(x, Cc, c0)
    got = _pack(dev, sbs, B, Cc, h, w, c0, nc, 1, 1, Carve(form, B, 1, h + 2, w + 2))
    d = _planes_diff(got, R.frame(R.pad_replicate(x, 1), fmt, planes, 1))
    assert not d, d


# ---------------------------------------------------------------------------------------------------------------------------------------
# pack_down_exact / pack_down_bound

DOWN = [(2, 0), (2, 1), (2, 2), (3, 0), (3, 3), (4, 0), (4, 2), (4, 4), (8, 0), (8, 4), (8, 8)]     # (down, pad)


def _down_case(down, pad, x_of):
    """Two launches per (down, pad): 7 x 6 outputs (more than one block), and with pad == 0 also 2 x 1."""
    B, Cc, c0, nc = 2, 13, 1, 11
    for Hd, Wd in [(7, 6)] + ([(2, 1), (1, 3)] if pad == 0 else []):
        h, w = Hd * down - 2 * pad, Wd * down - 2 * pad
        assert h >= 1 and w >= 1 and max(h, w) <= 64
        x = x_of((B, nc, h, w), 10 * down + pad + Hd)
        cpu, dev, sbs = _source(x, Cc, c0, extra=5)
        yield B, Cc, c0, nc, h, w, Hd, Wd, cpu, dev, sbs


@pytest.mark.parametrize('down,pad', DOWN, ids=['d%d-p%d' % dp for dp in DOWN])
@pytest.mark.parametrize('form', FORMS)
def test_pack_down_exact(form, down, pad):
    fmt, planes = R.FORMS[form]
    for B, Cc, c0, nc, h, w, Hd, Wd, cpu, dev, sbs in _down_case(down, pad, R.grid):
        ref = R.pack64(cpu, c0, nc, pad=pad, down=down, batch_stride=sbs, hw=(h, w), channels=Cc)
        assert ref.shape == (B, nc, Hd, Wd) and torch.equal(ref.float().double(), ref)
        got = _pack(dev, sbs, B, Cc, h, w, c0, nc, pad, down, Carve(form, B, 2, Hd, Wd))
        d = _planes_diff(got, R.frame(ref.float(), fmt, planes, 2))
        assert not d, '%d x %d: %s' % (Hd, Wd, d)


@pytest.mark.parametrize('down,pad', DOWN, ids=['d%d-p%d' % dp for dp in DOWN])
@pytest.mark.parametrize('form', FORMS)
def test_pack_down_bound(form, down, pad):
    fmt, planes = R.FORMS[form]
    worst = 0.0
    for B, Cc, c0, nc, h, w, Hd, Wd, cpu, dev, sbs in _down_case(down, pad, R.uniform):
        kw = dict(pad=pad, down=down, batch_stride=sbs, hw=(h, w), channels=Cc)
        ref = R.pack64(cpu, c0, nc, **kw)
        S = R.pack64(cpu.abs(), c0, nc, **kw)
        got, clean = R.unframe(_pack(dev, sbs, B, Cc, h, w, c0, nc, pad, down, Carve(form, B, 2, Hd, Wd)), fmt, nc)
        assert clean, 'border, unused lanes or unused groups are not zero'
        bound = 3 * R.U * S + R.store_bound(form, ref)
        r = R.worst_ratio(got, ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, '%d x %d: worst |stored - ref| / bound = %.3g' % (Hd, Wd, r)
    _report('pack_down_bound', worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# raw_view: the generator engine's three input packs

@pytest.mark.parametrize('sf,p', [(2, 0), (2, 1), (4, 0), (4, 1)])
@pytest.mark.parametrize('form', FORMS)
def test_raw_view(form, sf, p):
    from esr_hip import act as A
    fmt, planes = R.FORMS[form]
    B, lat, h0, w0 = 2, 3, 5, 3
    lat1, Ct = lat * sf * sf, lat * sf * sf + 3
    x = R.grid((B, Ct, h0, w0), sf + p)
    z_only, lr_only = x.clone(), x.clone()
    z_only[:, lat1:] = NAN
    lr_only[:, :lat1] = NAN
    zsrc = x[:, :lat1].reshape(B, lat, sf * h0, sf * w0)
    kw = dict(hw=(sf * h0, sf * w0), batch_stride=Ct * h0 * w0, channels=lat)
    h, w = h0 + 2 * p, w0 + 2 * p

    def run(src, carve, *a, **k):
        A.pack_nchw(src.to(DEV), carve.view(), *a, **k)
        torch.cuda.synchronize()
        return carve.verify()

    zlr = run(z_only, Carve(form, B, 1, h, w), 0, lat, pad=sf * p, down=sf, **kw)
    ref = R.pack64(zsrc, 0, lat, pad=sf * p, down=sf)
    assert torch.equal(ref, R.pack64(z_only, 0, lat, pad=sf * p, down=sf, **kw)) and torch.equal(ref.float().double(), ref)
    d = _planes_diff(zlr, R.frame(ref.float(), fmt, planes, 1))
    assert not d, 'latent /sf: ' + d
    zhr = run(z_only, Carve(form, B, 1, sf * h, sf * w), 0, lat, pad=sf * p, **kw)
    d = _planes_diff(zhr, R.frame(R.pad_replicate(zsrc, sf * p), fmt, planes, 1))
    assert not d, 'latent at HR: ' + d
    xin = run(lr_only, Carve(form, B, 1, h, w), Ct - 3, 3, pad=p)
    d = _planes_diff(xin, R.frame(R.pad_replicate(x[:, Ct - 3:], p), fmt, planes, 1))
    assert not d, 'LR image: ' + d


# ---------------------------------------------------------------------------------------------------------------------------------------
# views

def _act_split(form):
    return {'bf16': False, 'split': True, 'f16': 'f16', 'f16x2': 'f16x2'}[form]


def _actbuf_planes(buf):
    return torch.stack([buf.hi.cpu()] + ([buf.lo.cpu()] if buf.lo is not None else []))


@pytest.mark.parametrize('form', FORMS)
def test_views_actbuf_and_lanebuf(form):
    from esr_hip import act as A
    fmt, planes = R.FORMS[form]
    B, Bbuf, nc, h, w, pad = 2, 3, 11, 5, 7, 1
    H, W = h + 2 * pad, w + 2 * pad
    x = R.uniform((B, nc, h, w), 41, -2.0, 2.0)
    cpu, dev, sbs = _source(x, nc + 2, 1)
    plain = _pack(dev, sbs, B, nc + 2, h, w, 1, nc, pad, 1, Carve(form, B, 2, H, W))
    assert not _planes_diff(plain, R.frame(R.pad_replicate(x, pad), fmt, planes, 2))
    hi, lo = R.encode(R.pad_replicate(x, pad), fmt, planes)
    want = R.decode(hi, lo, fmt)
    buf = A.ActBuf(Bbuf, 5, H, W, DEV, _act_split(form))
    assert (buf.fmt, buf.nplanes) == (fmt, planes)
    for views, b0 in ((buf, 0), (A.LaneBuf(buf, 1), 1)):
        buf.hi.fill_(SENT)
        if buf.lo is not None:
            buf.lo.fill_(SENT)
        A.pack_nchw(dev, views.view(2, 2), 1, nc, pad=pad, hw=(h, w), channels=nc + 2)
        torch.cuda.synchronize()
        img = _actbuf_planes(buf)
        assert not _planes_diff(img[:, b0:b0 + B, 2:4], plain), 'b0 = %d' % b0
        img[:, b0:b0 + B, 2:4] = SENT
        assert bool((img == SENT).all()), 'a neighbouring group or image was written (b0 = %d)' % b0
        out = CarveF32(B, nc, H, W)
        v = views.view(2, 2)
        assert _lib().esr_unpack_nchw(C.byref(v), B, nc, out.t.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert _same_bits(out.verify(), want)
    # ActBuf.to_nchw(nc, cg0): the helper the other contract tests read GPU buffers with (the LaneBuf launch left images 1, 2 packed)
    buf.hi[0] = buf.hi[1]
    if buf.lo is not None:
        buf.lo[0] = buf.lo[1]
    got = buf.to_nchw(nc, 2).cpu()
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[0]) and _same_bits(got[2], want[1])
    got3 = buf.to_nchw(3, 3).cpu()                     # channels 8 .. 10 through cg0 = 3
    assert _same_bits(got3[1], want[0, 8:11])


@pytest.mark.parametrize('form', ['bf16', 'split'])
def test_views_stacked(form):
    """act.stacked_at: [planes][CG][B][H + 2][W + 2][8], batch_stride < cg_stride (bf16 formats: view_of has no other)."""
    from esr_hip import act as A
    fmt, planes = R.FORMS[form]
    B, Bbuf, nc, h, w = 2, 3, 11, 6, 4
    x = R.uniform((B, nc, h, w), 43, -2.0, 2.0)
    cpu, dev, sbs = _source(x, nc, 0)
    want_img = R.frame(x, fmt, planes, 2)
    t = A.stacked_at(planes, Bbuf, 4, h, w, DEV)
    bits = t.view(torch.int16)
    bits.fill_(SENT)
    v = A.view_of(t, cg0=1, ncg=2, b0=1)
    assert v.batch_stride < v.cg_stride and (v.lo is not None) == (planes == 2)
    A.pack_nchw(dev, v, 0, nc, hw=(h, w), channels=nc)
    torch.cuda.synchronize()
    img = bits.cpu().permute(0, 2, 1, 3, 4, 5).clone()              # [planes][B][CG]...
    assert not _planes_diff(img[:, 1:3, 1:3].contiguous(), want_img)
    img[:, 1:3, 1:3] = SENT
    assert bool((img == SENT).all()), 'a neighbouring group or image of the stacked tensor was written'
    out = CarveF32(B, nc, h, w)
    assert _lib().esr_unpack_nchw(C.byref(v), B, nc, out.t.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    hi, lo = R.encode(x, fmt, planes)
    assert _same_bits(out.verify(), R.decode(hi, lo, fmt))


# ---------------------------------------------------------------------------------------------------------------------------------------
# unpack_exact

def _stored_planes(form, B, ncg, nc, H, W, seed, scale=2.0):
    """int16 [planes][B][ncg][H + 2][W + 2][8]: random finite hi (some -0), a lo that is NOT hi's residue, the sentinel in the border, in lanes
    >= nc and in the groups past ceil(nc / 8); and (hi, lo) as [B][nc][H][W]."""
    fmt, planes = R.FORMS[form]
    hi = R.uniform((B, nc, H, W), seed, -scale, scale).to(R.DTYPE[fmt]).view(torch.int16)
    hi.view(-1)[::7] = -32768                                                          # -0
    lo = R.uniform((B, nc, H, W), seed + 1, -scale / 64, scale / 64).to(R.DTYPE[fmt]).view(torch.int16) if planes == 2 else None
    img = torch.full((planes, B, ncg, H + 2, W + 2, 8), SENT, dtype=torch.int16)
    keep = R.to_lanes(torch.ones(B, nc, H, W, dtype=torch.bool), ncg)
    for p, plane in enumerate([hi] + ([lo] if planes == 2 else [])):
        img[p, :, :, 1:-1, 1:-1] = torch.where(keep, R.to_lanes(plane, ncg), torch.tensor(SENT, dtype=torch.int16))
    return img, hi, lo


UNPACK_SHAPES = [(2, 3, 5, 7), (3, 8, 1, 9), (2, 11, 6, 1), (2, 13, 23, 17)]             # (B, nc, H, W)


@pytest.mark.parametrize('B,nc,H,W', UNPACK_SHAPES, ids=['%dx%dx%dx%d' % s for s in UNPACK_SHAPES])
@pytest.mark.parametrize('form', FORMS)
def test_unpack_exact(form, B, nc, H, W):
    fmt, planes = R.FORMS[form]
    for wide in (0, 1):                                  # the view as wide as nc needs, and one group wider
        ncg = (nc + 7) // 8 + wide
        img, hi, lo = _stored_planes(form, B, ncg, nc, H, W, 50 + nc + wide)
        src = Carve(form, B, ncg, H, W)
        src.put(img)
        out = CarveF32(B, nc, H, W)
        v = src.view()
        assert _lib().esr_unpack_nchw(C.byref(v), B, nc, out.t.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        got, want = out.verify(), R.decode(hi, lo, fmt)
        assert torch.equal(got, want) and _same_bits(got, want)
        if planes == 1:
            assert not bool((got.view(torch.int32) == -2 ** 31).any())        # a stored -0 decodes to +0
        assert not _same_bits(got, R.decode(hi, None, fmt)) or planes == 1     # (the lo plane matters to the comparison)


# ---------------------------------------------------------------------------------------------------------------------------------------
# zero

@pytest.mark.parametrize('n16', [0, 1, 255, 256, 257, 4096 * 256 + 257])
def test_zero(n16):
    a = torch.full((8 + 8 * n16 + 64,), SENT, dtype=torch.int16, device=DEV)
    assert _lib().esr_zero(a.data_ptr() + 16, n16, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((a[:8] == SENT).all()) and bool((a[8 + 8 * n16:] == SENT).all()), 'written outside [0, n16)'
    assert bool((a[8:8 + 8 * n16] == 0).all()), 'a vector inside [0, n16) is not zero'


# ---------------------------------------------------------------------------------------------------------------------------------------
# pack_norm

def _mean_std(mode, Cc):
    if mode == 'none':
        return None, None
    if mode == 'pow2':
        return (torch.tensor([(37 * c - 400) / 1024.0 for c in range(Cc)], dtype=torch.float32),
                torch.tensor([[0.5, 2.0, 4.0][c % 3] for c in range(Cc)], dtype=torch.float32))
    return (torch.tensor([VGG_MEAN[c % 3] for c in range(Cc)], dtype=torch.float32), torch.tensor([VGG_STD[c % 3] for c in range(Cc)], dtype=torch.float32))


NORM_SHAPES = {3: [(2, 5, 7), (3, 1, 9)], 11: [(2, 6, 1), (2, 13, 9)]}                    # C: [(B, h, w)]


@pytest.mark.parametrize('mode', ['none', 'pow2', 'real'])
@pytest.mark.parametrize('Cc', [3, 11])
@pytest.mark.parametrize('form', FORMS)
def test_pack_norm(form, Cc, mode):
    fmt, planes = R.FORMS[form]
    mean, std = _mean_std(mode, Cc)
    dmean, dstd = (mean.to(DEV), std.to(DEV)) if mean is not None else (None, None)
    worst = 0.0
    for k, (B, h, w) in enumerate(NORM_SHAPES[Cc]):
        ncg = (Cc + 7) // 8 + k                          # the second launch: a view one group wider than C needs
        if mode == 'none':
            x = _with_specials(R.uniform((B, Cc, h, w), 60 + Cc, -2.0, 2.0), fmt) if Cc * h * w >= 20 else R.uniform((B, Cc, h, w), 60 + Cc, -2.0, 2.0)
        elif mode == 'pow2':
            x = R.grid((B, Cc, h, w), 61 + Cc)
        else:
            x = R.uniform((B, Cc, h, w), 62 + Cc, 0.0, 1.0)
        dst = Carve(form, B, ncg, h, w)
        v = dst.view()
        dev = x.to(DEV)
        assert _lib().esr_pack_nchw_norm(dev.data_ptr(), B, Cc, h, w, dmean.data_ptr() if mean is not None else None,
                                         dstd.data_ptr() if std is not None else None, C.byref(v), _stream()) == 0
        torch.cuda.synchronize()
        img = dst.verify()
        ref = R.pack_norm64(x, mean, std)
        if mode != 'real':
            assert torch.equal(ref.float().double(), ref)
            d = _planes_diff(img, R.frame(ref.float(), fmt, planes, ncg))
            assert not d, '%s %d x %d: %s' % (mode, h, w, d)
            continue
        got, clean = R.unframe(img, fmt, Cc)
        assert clean, 'border, unused lanes or unused groups are not zero'
        r = R.worst_ratio(got, ref, 4 * R.U * ref.abs() + R.store_bound(form, ref))
        worst = max(worst, r)
        assert r <= 1.0, '%d x %d: worst |stored - ref| / bound = %.3g' % (h, w, r)
        assert R.worst_ratio(got, R.pack_norm64(x, mean.roll(1), std), 4 * R.U * ref.abs() + R.store_bound(form, ref)) > 1.0
    if mode == 'real':
        _report('pack_norm', worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# unpack_grad_norm

@pytest.mark.parametrize('mode', ['none', 'pow2', 'real'])
@pytest.mark.parametrize('Cc', [3, 11])
@pytest.mark.parametrize('form', FORMS)
def test_unpack_grad_norm(form, Cc, mode):
    fmt, planes = R.FORMS[form]
    _, std = _mean_std(mode, Cc)
    dstd = std.to(DEV) if std is not None else None
    worst = 0.0
    for B, H, W in NORM_SHAPES[Cc]:
        img, hi, lo = _stored_planes(form, B, 2, Cc, H, W, 70 + Cc)          # G->ncg = 2: C = 3 leaves a whole group of NaN, C = 11 five lanes
        G = Carve(form, B, 2, H, W)
        G.put(img)
        out = CarveF32(B, Cc, H, W)
        v = G.view()
        assert _lib().esr_unpack_grad_nchw_norm(C.byref(v), B, Cc, dstd.data_ptr() if std is not None else None, out.t.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        got = out.verify()
        g = R.decode(hi, lo, fmt)
        ref = R.unpack_grad_norm64(g, std)
        if mode != 'real':
            assert torch.equal(ref.float().double(), ref)
            assert _same_bits(got, ref.float()), '%s %d x %d' % (mode, H, W)
            continue
        r = R.worst_ratio(got, ref, 3 * R.U * ref.abs())
        worst = max(worst, r)
        assert r <= 1.0, '%d x %d: worst |dst - ref| / bound = %.3g' % (H, W, r)
        assert R.worst_ratio(got, R.unpack_grad_norm64(g, std.roll(1)), 3 * R.U * ref.abs()) > 1.0
    if mode == 'real':
        _report('unpack_grad_norm', worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# adjoint: esr_pack_nchw and esr_unpack_grad_nchw are transposes of each other

ADJOINT = [(0, 1, 0, 5, 7), (3, 1, 2, 5, 7), (4, 4, 0, 8, 12), (1, 2, 0, 6, 8), (3, 3, 0, 6, 9)]          # (pad, down, c0, h, w)


@pytest.mark.parametrize('extra', [0, 29], ids=['dense', 'strided'])
@pytest.mark.parametrize('pad,down,c0,h,w', ADJOINT, ids=['p%d-d%d-c%d' % a[:3] for a in ADJOINT])
@pytest.mark.parametrize('form', ['split', 'f16x2'])
def test_adjoint(form, pad, down, c0, h, w, extra):
    fmt, planes = R.FORMS[form]
    B, Cc, nc = 2, 5, 3
    Hd, Wd = (h + 2 * pad) // down, (w + 2 * pad) // down
    x = R.grid((B, nc, h, w), 80 + pad + down)
    cpu, dev, sbs = _source(x, Cc, c0, extra)
    px, clean = R.unframe(_pack(dev, sbs, B, Cc, h, w, c0, nc, pad, down, Carve(form, B, 1, Hd, Wd)), fmt, nc)
    ref = R.pack64(cpu, c0, nc, pad=pad, down=down, batch_stride=sbs, hw=(h, w), channels=Cc)
    assert clean and torch.equal(px.double(), ref), 'the pack of grid values is not exact'
    img, ghi, glo = _stored_planes(form, B, 1, nc, Hd, Wd, 90 + pad, scale=1.0)
    G = Carve(form, B, 1, Hd, Wd)
    G.put(img)
    g = R.decode(ghi, glo, fmt).double()
    stride = Cc * h * w + extra
    dst = torch.full((B, stride), NAN, dtype=torch.float32, device=DEV)
    v = G.view()
    assert _lib().esr_unpack_grad_nchw(C.byref(v), dst.data_ptr(), sbs, B, Cc, h, w, c0, nc, pad, down, 0, _stream()) == 0
    torch.cuda.synchronize()
    dcpu = dst.cpu()
    gx = dcpu[:, :Cc * h * w].view(B, Cc, h, w)[:, c0:c0 + nc].double()
    mine = torch.zeros(B, stride, dtype=torch.bool)
    mine[:, :Cc * h * w].view(B, Cc, h, w)[:, c0:c0 + nc] = True
    assert bool(torch.isnan(dcpu[~mine]).all()) and bool(torch.isfinite(gx).all())
    x0 = torch.zeros(B, nc, h, w, dtype=torch.float64, requires_grad=True)
    (R.bilinear_down(R.pad_replicate(x0, pad), down) * g.abs()).sum().backward()
    S = x0.grad
    tol = float((x.double().abs() * 4 * ((pad + 1) ** 2 + 1) * R.U * S).sum())
    lhs, rhs = float((px.double() * g).sum()), float((x.double() * gx).sum())
    r = abs(lhs - rhs) / tol
    _report('adjoint', r)
    assert r <= 1.0, '<P x, G> = %.17g, <x, P^T G> = %.17g, tolerance %.3g' % (lhs, rhs, tol)
    assert abs(lhs - float((x.double() * gx.roll(1, 3)).sum())) > tol, 'the identity does not notice a gradient one pixel over'


# ---------------------------------------------------------------------------------------------------------------------------------------
# run_list and repeatability

@pytest.mark.parametrize('form', FORMS)
def test_run_list_matches_direct_calls(form):
    L, lib = _L(), _lib()
    B, Cc, c0, nc, h, w, pad, down = 2, 13, 1, 11, 10, 6, 1, 2
    Hd, Wd = (h + 2 * pad) // down, (w + 2 * pad) // down
    cpu, dev, sbs = _source(R.uniform((B, nc, h, w), 95), Cc, c0, 7)
    results = []
    for listed in (False, True):
        z = torch.full((8 * 400,), SENT, dtype=torch.int16, device=DEV)
        act, out = Carve(form, B, 2, Hd, Wd), CarveF32(B, nc, Hd, Wd)
        v = act.view()
        if listed:
            arr = (L.Cmd * 3)()
            arr[0].op, arr[0].u.zero = L.OP_ZERO, L.CmdZero(z.data_ptr(), 300)
            arr[1].op, arr[1].u.pack_nchw = L.OP_PACK_NCHW, L.CmdPackNchw(dev.data_ptr(), sbs, B, Cc, h, w, c0, nc, pad, down, v)
            arr[2].op, arr[2].u.unpack_nchw = L.OP_UNPACK_NCHW, L.CmdUnpackNchw(v, B, nc, out.t.data_ptr())
            failed = C.c_int(-7)
            assert lib.esr_run(arr, 3, C.byref(failed), _stream()) == 0 and failed.value == -1
        else:
            assert lib.esr_zero(z.data_ptr(), 300, _stream()) == 0
            assert lib.esr_pack_nchw(dev.data_ptr(), sbs, B, Cc, h, w, c0, nc, pad, down, C.byref(v), _stream()) == 0
            assert lib.esr_unpack_nchw(C.byref(v), B, nc, out.t.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        results.append((z.cpu(), act.verify(), out.verify()))
    (z0, a0, o0), (z1, a1, o1) = results
    assert torch.equal(z0, z1) and bool((z0[:2400] == 0).all()) and bool((z0[2400:] == SENT).all())
    assert torch.equal(a0, a1) and _same_bits(o0, o1)
    assert _same_bits(o0, R.unframe(a0, R.FORMS[form][0], nc)[0])


@pytest.mark.parametrize('form', FORMS)
def test_repeatability(form):
    lib = _lib()
    fmt, planes = R.FORMS[form]
    B, Cc, c0, nc, h, w, pad, down = 2, 13, 1, 11, 10, 6, 1, 2
    Hd, Wd = (h + 2 * pad) // down, (w + 2 * pad) // down
    cpu, dev, sbs = _source(R.uniform((B, nc, h, w), 96), Cc, c0, 7)
    xn = R.uniform((B, nc, h, w), 97, 0.0, 1.0).to(DEV)
    mean, std = [t.to(DEV) for t in _mean_std('real', nc)]
    img, _, _ = _stored_planes(form, B, 2, nc, Hd, Wd, 98)
    runs = []
    for _ in range(2):
        a = _pack(dev, sbs, B, Cc, h, w, c0, nc, pad, down, Carve(form, B, 2, Hd, Wd))
        n = Carve(form, B, 2, h, w)
        v = n.view()
        assert lib.esr_pack_nchw_norm(xn.data_ptr(), B, nc, h, w, mean.data_ptr(), std.data_ptr(), C.byref(v), _stream()) == 0
        src = Carve(form, B, 2, Hd, Wd)
        src.put(img)
        o1, o2 = CarveF32(B, nc, Hd, Wd), CarveF32(B, nc, Hd, Wd)
        v = src.view()
        assert lib.esr_unpack_nchw(C.byref(v), B, nc, o1.t.data_ptr(), _stream()) == 0
        assert lib.esr_unpack_grad_nchw_norm(C.byref(v), B, nc, std.data_ptr(), o2.t.data_ptr(), _stream()) == 0
        z = torch.full((8 * 600,), SENT, dtype=torch.int16, device=DEV)
        assert lib.esr_zero(z.data_ptr(), 513, _stream()) == 0
        torch.cuda.synchronize()
        runs.append((a, n.verify(), o1.verify(), o2.verify(), z.cpu()))
    for first, second in zip(*runs):
        assert first.dtype == second.dtype and torch.equal(first.view(torch.int16) if first.dtype == torch.int16 else first.view(torch.int32),
                                                           second.view(torch.int16) if second.dtype == torch.int16 else second.view(torch.int32))
