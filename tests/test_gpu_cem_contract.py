"""The CEM filter entry points (include/esr_hip.h; csrc/esr_cem.hip), option by option, against the float64 restatement oracle/cem_contract_ref.py
(pinned on the CPU by tests/test_host_cem_contract_ref.py, which also shows that the comparator used here rejects a dropped tap, reversed taps,
swapped factors, a shifted pre, zero padding for the clamp and a row from the neighbouring strip).

Method (as tests/test_gpu_conv_contract.py): the C ABI is called directly through esr_hip._lib (cem_ops.*_raw only where the dispatch is the
subject: the B*C > 65535 fallback and adjoint_raw); every test asserts through esr_cem_sep_form that the kernel form it means to reach is the one
that runs; taps are synthetic, seeded and ASYMMETRIC (tv != th, neither equal to its reverse, mixed signs, every |tap| >= 0.2 / k; a full-rank
k x k array for the 2-D entry points) plus one case per op with the product's real taps; inputs are fp32 uniform in [-1, 1], g in [0, 1].

Bound: element-wise and derived (cem_contract_ref.bound):  |got - ref| <= (n + 2) u S + u |ref|, u = 2^-24, n = 2k (separable), k^2 (2-D),
+ 2 kf (folded filter), gather terms + 1 (adjoints); modes 1 / 3 add u |g|; mode 2 adds range (bound(g - U(f_g)) + 2^-21) — the 2^-21 is an
allowance for the device tanhf: an assumption, not a derivation.  Where the header promises bit equality the tests assert torch.equal.

Guards: every destination (d, out, out2, dx, tmp) is carved out of a larger allocation filled with a NaN sentinel: the words around it must be
bit-identical after the launch (the float4 store paths of ragged tiles) and no sentinel may survive inside it.

Families -> kernels (the float64 references run on the GPU; each test prints its worst error / bound):
  downscale_wave  cem_downscale_wave_kernel<SF, NA>, SF in {2,3,4,8} x NA in {4,5,6}, the smallest and largest k of each NA, both walking directions
                  (4 strips), 2 ragged column tiles, pre in {0, shipped, sf-1}, plain / fused with lr_pad 0 / 3, the non-`fast` loads
  upscale_wave    cem_upscale_wave_kernel<TWO, SF, NA>, TWO x SF in {3,4,8} x NA in {4,5,6}; modes 0-3, crop in {0, 1, sf, 2sf+1}, a crop that
                  leaves 4 rows, unaligned g / out / out2
  lrfilter_wave   cem_lrfilter_wave_kernel<27> and <35>
  thin            the three wave kernels on images thinner than one tap window
  stream          cem_downscale_stream_kernel<8> (k 33, 45) and <0> (sf 6, k 25: enumerating esr_cem_sep_form(0, ...) on the host finds form 1 outside
                  sf 2 / 3 / 4 / 8 for sf 5 from k 41, sf 6 from k 25 and the larger factors)
  tile_sep        cem_downscale_sep_kernel<2,3,4,0> (sf 1, 5, 6 generic; at sf 8 EVERY k the tile kernel could take streams instead: its <8>
                  instantiation is unreachable), cem_lrfilter_sep_kernel, cem_upscale_sep_kernel<TWO, 2/3/4/8/0, FILT>
  tile_2d         cem_downscale_tiled_kernel, cem_lrfilter_tiled_kernel, cem_upscale_tiled_kernel<TWO> on several tiles, full-rank taps
  untiled         cem_downscale_kernel, cem_lrfilter_kernel, cem_upscale_kernel<TWO>: B*C = 65536 planes through cem_ops.*_raw (the separable
                  entry returns ESR_E_UNSUPPORTED, the 2-D one runs)
  batch           96 planes against each plane alone, bit for bit (the strip cut of the upscale / LR-filter wave kernels moves with the batch)
  adjoint         cem_adjoint_kernel (accumulate 0 / 1) and cem_adjoint_1d_kernel<0 / 1> (base, alpha +-1), float64 autograd of the restatement
  fixes           the upscale with pre == sf - 1 (samples on the last row / column: the replicate pad repeats them) and the adjoints on frames of
                  one row or column
  refusals        every ESR_E_ARG condition of the eight entry points returns it and writes nothing

Largest observed error / bound per family on an MI355X (a record, not a tolerance; comparisons in brackets):
  downscale_wave 0.084 (56)   upscale_wave 0.102 (87)   lrfilter_wave 0.019 (4)   thin 0.101 (14)   stream 0.009 (9)   tile_sep 0.104 (153)
  tile_2d 0.038 (59)   untiled 0.055 (8)   product_taps 0.093 (14)   adjoint 0.255 (282)   fixes 0.100 (128)
(adjoint: n = cem_contract_ref.adjoint_terms, the exact maximum of the gather, min(nq, ceil(k / sq)) outputs per axis; the 0.255 is a 2 x 2 frame at sf 8.)"""
import numpy as np
import pytest
import torch

from oracle import cem_contract_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0x7FC0DEAD          # a quiet NaN with a recognisable payload
GUARD = 64                 # words either side of a destination (keeps its 16-byte alignment)


def _lib():
    from esr_hip import _lib as L
    return L


def _stream():
    from esr_hip.act import stream_ptr
    return stream_ptr()


def _form(op, sf, k, pre, h, w):
    return _lib().lib.esr_cem_sep_form(op, sf, k, pre, h, w)


def _shipped_pre(sf):
    return sf - sf // 2 - 1


class Carved:
    """A destination inside a sentinel-filled allocation, `off` words (4 bytes each) off 16-byte alignment."""

    def __init__(self, shape, off=0):
        self.n = int(np.prod(shape))
        self.raw = torch.full((self.n + 2 * GUARD + 4,), SENT, dtype=torch.int32, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.lo = GUARD + off
        self.t = self.raw[self.lo:self.lo + self.n].view(torch.float32).view(shape)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def load(self, values):
        self.t.copy_(values)
        return self

    def check(self, written=True):
        torch.cuda.synchronize()
        assert bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all()), 'the launch wrote outside its destination'
        inner = self.raw[self.lo:self.lo + self.n]
        if written:
            assert not bool((inner == SENT).any()), 'part of the destination was never written'
        else:
            assert bool((inner == SENT).all()), 'a refused call wrote to its destination'


def put(t, off=0):
    """Device copy of t whose base is `off` words off 16-byte alignment."""
    raw = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    v = raw[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def ptr(t):
    return t.data_ptr() if t is not None else None


def judge(family, got, ref, bnd, what=''):
    r = R.worst_ratio(got, ref, bnd)
    print('%s error/bound %.3f %s' % (family, r, what))
    assert r <= 1.0, (family, what, r)
    return r


def make_taps(k, seed, sep):
    return R.synthetic_sep(k, seed) if sep else R.synthetic_2d(k, seed)


def dev_taps(taps):
    return tuple(t.to(DEV) for t in taps) if R.is_sep(taps) else taps.to(DEV).contiguous()


# ---- the launches and their float64 restatements --------------------------------------------------------------------------------------
def run_down(family, BC, h, w, sf, k, pre, form=None, sep=True, fused=False, lr_pad=0, off=0, taps=None, seed=0):
    B, C = BC
    taps = make_taps(k, seed, sep) if taps is None else taps
    td = dev_taps(taps)
    y = put(R.uniform((B, C, h * sf, w * sf), 10 * seed + 1), off)
    lr = put(R.uniform((B, C, h - 2 * lr_pad, w - 2 * lr_pad), 10 * seed + 2), off) if fused else None
    d = Carved((B, C, h, w), off)
    L = _lib().lib
    if sep:
        assert _form(0, sf, k, pre, h, w) == form, (sf, k, pre, h, w, _form(0, sf, k, pre, h, w))
        rc = L.esr_cem_downscale_sep(y.data_ptr(), B, C, h, w, sf, pre, td[0].data_ptr(), td[1].data_ptr(), k, ptr(lr), lr_pad, d.ptr, _stream())
    else:
        rc = L.esr_cem_downscale(y.data_ptr(), B, C, h, w, sf, pre, td.data_ptr(), k, ptr(lr), lr_pad, d.ptr, _stream())
    assert rc == 0, rc
    d.check()
    ref, S = R.downscale(y, taps, sf, pre, lr, lr_pad)
    judge(family, d.t, ref, R.bound(2 * k if sep else k * k, S, ref), 'downscale x%d k%d pre%d %dx%d%s' % (sf, k, pre, h, w, ' fused pad %d' % lr_pad if fused else ''))
    return d.t


def run_filt(family, BC, h, w, k, form=None, sep=True, off=0, taps=None, seed=0):
    B, C = BC
    taps = make_taps(k, seed, sep) if taps is None else taps
    td = dev_taps(taps)
    x = put(R.uniform((B, C, h, w), 10 * seed + 3), off)
    o = Carved((B, C, h, w), off)
    L = _lib().lib
    if sep:
        assert _form(2, 1, k, 0, h, w) == form, (k, h, w, _form(2, 1, k, 0, h, w))
        rc = L.esr_cem_lrfilter_sep(x.data_ptr(), B, C, h, w, td[0].data_ptr(), td[1].data_ptr(), k, o.ptr, _stream())
    else:
        rc = L.esr_cem_lrfilter(x.data_ptr(), B, C, h, w, td.data_ptr(), k, o.ptr, _stream())
    assert rc == 0, rc
    o.check()
    ref, S = R.lrfilter(x, taps)
    judge(family, o.t, ref, R.bound(2 * k if sep else k * k, S, ref), 'lrfilter k%d %dx%d' % (k, h, w))
    return o.t


def run_up(family, BC, h, w, sf, k, pre, mode, crop=0, form=None, sep=True, off=0, taps=None, seed=0, rng=0.75, fold_kf=0, inputs=None):
    """esr_cem_upscale / _sep, or (fold_kf > 0) esr_cem_filter_upscale_sep.  Returns (out, out2, (f, f2, g), rc)."""
    B, C = BC
    taps = make_taps(k, seed, sep) if taps is None else taps
    td = dev_taps(taps)
    Ho, Wo = h * sf - 2 * crop, w * sf - 2 * crop
    if inputs is None:
        f = put(R.uniform((B, C, h, w), 10 * seed + 4))
        f2 = put(R.uniform((B, C, h, w), 10 * seed + 5)) if mode >= 2 else None
        g = put(R.uniform((B, C, h * sf, w * sf), 10 * seed + 6, 0.0, 1.0), off) if mode >= 1 else None
    else:
        f, f2, g = inputs
    out = Carved((B, C, Ho, Wo), off)
    out2 = Carved((B, C, Ho, Wo), off) if mode == 3 else None
    L = _lib().lib
    tail = (ptr(g), crop, mode, float(rng), out.ptr, out2.ptr if out2 else None, _stream())
    n = 2 * k if sep else k * k
    if fold_kf:
        tf = R.synthetic_sep(fold_kf, 50 + seed)
        tfd = dev_taps(tf)
        rc = L.esr_cem_filter_upscale_sep(f.data_ptr(), ptr(f2), B, C, h, w, sf, pre, tfd[0].data_ptr(), tfd[1].data_ptr(), fold_kf, td[0].data_ptr(),
                                          td[1].data_ptr(), k, *tail)
        n += 2 * fold_kf
        if rc == _lib().ESR_E_UNSUPPORTED:          # the windows do not fit on chip: documented, and nothing may have been written
            out.check(written=False)
            return None, None, (f, f2, g), rc
    elif sep:
        assert _form(1, sf, k, pre, h, w) == form, (sf, k, pre, h, w, _form(1, sf, k, pre, h, w))
        rc = L.esr_cem_upscale_sep(f.data_ptr(), ptr(f2), B, C, h, w, sf, pre, td[0].data_ptr(), td[1].data_ptr(), k, *tail)
    else:
        rc = L.esr_cem_upscale(f.data_ptr(), ptr(f2), B, C, h, w, sf, pre, td.data_ptr(), k, *tail)
    assert rc == 0, rc
    out.check()
    if out2:
        out2.check()
    if fold_kf:
        ref, S = R.filter_upscale(f, tf, taps, sf, pre, e2=f2, g=g, crop=crop, mode=mode, range=rng)
    else:
        ref, S = R.upscale(f, taps, sf, pre, f2=f2, g=g, crop=crop, mode=mode, range=rng)
    what = '%s x%d k%d pre%d mode%d crop%d %dx%d' % ('fold kf%d' % fold_kf if fold_kf else 'upscale', sf, k, pre, mode, crop, h, w)
    gc = g[:, :, crop:h * sf - crop, crop:w * sf - crop] if g is not None else None
    if mode == 0:
        judge(family, out.t, ref, R.bound(n, S, ref), what)
    elif mode == 1:
        judge(family, out.t, ref, R.bound(n, S, ref, gc), what)
    elif mode == 2:
        judge(family, out.t, ref, R.bound_mode2(n, S, g, crop, rng), what)
    else:
        judge(family, out.t, ref[0], R.bound(n, S[0], ref[0]), what + ' out')
        judge(family, out2.t, ref[1], R.bound(n, S[1], ref[1], gc), what + ' out2')
    return out.t, (out2.t if out2 else None), (f, f2, g), rc


KINDS = {'downscale': 0, 'lrfilter': 2, 'upscale': 1}


def _adjoint_geometry(kind, sf, pre, h, w):
    """(dy shape, input shape, (sq, oq, Ny, Nx, sn, on)) of the adjoint of one op on an h x w low-resolution image (cem_ops.adjoint_raw's table)."""
    if kind == 'downscale':
        return (h, w), (h * sf, w * sf), (sf, pre, h * sf, w * sf, 1, 0)
    if kind == 'lrfilter':
        return (h, w), (h, w), (1, 0, h, w, 1, 0)
    return (h * sf, w * sf), (h, w), (1, 0, h * sf, w * sf, sf, pre)


def run_adjoint(family, kind, BC, h, w, sf, k, pre, sep, variant, seed=0):
    """variant: sep 0: plain, 1: base + adjoint, 2: base - adjoint;  2-D 0: accumulate = 0, 1: accumulate = 1."""
    from esr_hip import autograd as AG
    B, C = BC
    taps = make_taps(k, seed, sep)
    (hq, wq), (hn, wn), (sq, oq, Ny, Nx, sn, on) = _adjoint_geometry(kind, sf, pre, h, w)
    dy = put(R.uniform((B, C, hq, wq), 10 * seed + 7))
    base = R.uniform((B, C, hn, wn), 10 * seed + 8).to(DEV) if variant else None
    dx = Carved((B, C, hn, wn))
    L = _lib().lib
    if sep:
        tv, th = AG.tap_tables_1d(taps[0]).to(DEV), AG.tap_tables_1d(taps[1]).to(DEV)
        tmp = Carved((B * C * hq * wn,))
        alpha = -1.0 if variant == 2 else 1.0
        rc = L.esr_cem_adjoint_sep(dy.data_ptr(), B, C, hq, wq, sq, oq, Ny, Nx, tv.data_ptr(), th.data_ptr(), k, hn, wn, sn, on, tmp.ptr, ptr(base), alpha,
                                   dx.ptr, _stream())
        assert rc == 0, rc
        tmp.check()
    else:
        alpha = 1.0
        tabs = AG.tap_tables(taps).to(DEV)
        if variant:
            dx.load(base)
        rc = L.esr_cem_adjoint(dy.data_ptr(), B, C, hq, wq, sq, oq, Ny, Nx, tabs.data_ptr(), k, hn, wn, sn, on, dx.ptr, 1 if variant else 0, _stream())
        assert rc == 0, rc
    dx.check()
    adj, S = R.adjoint(kind, dy, taps, sf, pre, (B, C, hn, wn))
    ref = alpha * adj if base is None else base.double() + alpha * adj
    S = S if base is None else S + base.double().abs()
    judge(family, dx.t, ref, R.bound(R.adjoint_terms(k, sq, hq, wq, sep), S, ref),
          'adjoint of %s x%d k%d pre%d %dx%d %s variant %d' % (kind, sf, k, pre, h, w, 'sep' if sep else '2d', variant))


def _ks(sf, na):
    """the smallest and the largest odd k with ceil(k / sf) == na"""
    ks = [k for k in range(1, 100, 2) if (k + sf - 1) // sf == na]
    return sorted({ks[0], ks[-1]})


BC6 = (2, 3)


# ---- downscale_wave ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf,na', [(s, n) for s in (2, 3, 4, 8) for n in (4, 5, 6)])
def test_downscale_wave(sf, na):
    """cem_downscale_wave_kernel<sf, na> (form 2) on LR 48 x 90: 4 strips of 12 rows — even strips walk down, odd ones up with the vertical taps
    reversed — and 2 column tiles of 45; both ends of the k range of this NA; pre 0 / shipped / sf - 1 paired with plain / fused lr_pad 0 / fused lr_pad 3."""
    pres = sorted({0, _shipped_pre(sf), sf - 1})
    for i, k in enumerate(_ks(sf, na)):
        for j, pre in enumerate(pres):
            v = (i + j) % 3
            run_down('downscale_wave', BC6, 48, 90, sf, k, pre, form=2, fused=v > 0, lr_pad=3 if v == 2 else 0, seed=sf + na + i)


def test_downscale_wave_unaligned():
    """y, lr and d based 4 bytes off 16-byte alignment: the kernel's four clamped scalar loads in place of the 16-byte vector (`fast` false)."""
    run_down('downscale_wave', BC6, 48, 90, 4, 17, 1, form=2, fused=True, lr_pad=3, off=1, seed=3)
    run_down('downscale_wave', BC6, 48, 90, 3, 15, 2, form=2, off=1, seed=4)


# ---- upscale_wave ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf,na', [(s, n) for s in (3, 4, 8) for n in (4, 5, 6)])
def test_upscale_wave(sf, na):
    """cem_upscale_wave_kernel<false, sf, na> (modes 0, 1) and <true, sf, na> (modes 2, 3), form 2, LR 48 x 90; mode m runs crop {0, 1, sf, 2sf+1}[m],
    pre cycling through {1, shipped, sf - 2} and the two ends of the k range."""
    pres = sorted({1, _shipped_pre(sf), sf - 2})
    ks = _ks(sf, na)
    for mode in range(4):
        for i, k in enumerate(ks):
            run_up('upscale_wave', BC6, 48, 90, sf, k, pres[(mode + i) % len(pres)], mode, crop=(0, 1, sf, 2 * sf + 1)[(mode + i) % 4], form=2, seed=sf + na + mode)


def test_upscale_wave_crop_to_four_rows_and_unaligned():
    """A crop that leaves Ho = 4 (one short strip); g, out and out2 4 bytes off alignment (element-wise loads and stores)."""
    run_up('upscale_wave', BC6, 48, 90, 4, 17, 1, 1, crop=94, form=2, seed=5)
    run_up('upscale_wave', BC6, 48, 90, 4, 17, 2, 3, crop=4, form=2, off=1, seed=6)
    run_up('upscale_wave', BC6, 48, 90, 8, 33, 3, 2, crop=0, form=2, off=1, seed=7)


def test_upscale_forms_agree_to_the_bit():
    """The header: 'the upscale forms agree to the bit'.  The same LR image as 48 x 90 (wave kernel) and cut to its first 80 columns (3840 pixels: tile
    kernel): wherever no tap reaches past the cut the two outputs are the same sums in the same order."""
    sf, k, pre = 4, 17, 1
    for mode in (1, 3):
        taps = make_taps(k, 9, True)
        f = R.uniform((2, 3, 48, 90), 41)
        f2 = R.uniform((2, 3, 48, 90), 42)
        g = R.uniform((2, 3, 192, 360), 43, 0.0, 1.0)
        wide = run_up('upscale_wave', BC6, 48, 90, sf, k, pre, mode, form=2, taps=taps, inputs=(put(f), put(f2), put(g)))
        cut = run_up('tile_sep', BC6, 48, 80, sf, k, pre, mode, form=0, taps=taps,
                     inputs=(put(f[..., :80].contiguous()), put(f2[..., :80].contiguous()), put(g[..., :320].contiguous())))
        safe = 80 * sf - k // 2 - sf
        assert torch.equal(wide[0][..., :safe], cut[0][..., :safe])
        if mode == 3:
            assert torch.equal(wide[1][..., :safe], cut[1][..., :safe])


# ---- lrfilter_wave, thin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [27, 35])
def test_lrfilter_wave(k):
    """cem_lrfilter_wave_kernel<k> (form 2) on LR 100 x 168: 2 column tiles, several strips."""
    run_filt('lrfilter_wave', BC6, 100, 168, k, form=2, seed=k)
    run_filt('lrfilter_wave', BC6, 100, 168, k, form=2, off=1, seed=k + 1)


@pytest.mark.parametrize('h,w', [(3, 1400), (1400, 3)])
def test_thin_images_down_and_up(h, w):
    """The wave kernels (form 2) on an image thinner than one tap window: cem_downscale_wave_kernel<4,5>, cem_upscale_wave_kernel<*,4,5>, <*,8,5>."""
    run_down('thin', BC6, h, w, 4, 17, 1, form=2, fused=True, lr_pad=1, seed=1)
    run_down('thin', BC6, h, w, 2, 9, 1, form=2, seed=2)
    run_up('thin', BC6, h, w, 4, 17, 1, 1, crop=2, form=2, seed=3)
    run_up('thin', BC6, h, w, 8, 33, 3, 3, crop=0, form=2, seed=4)


@pytest.mark.parametrize('h,w', [(5, 3300), (3300, 5)])
def test_thin_images_lrfilter(h, w):
    """cem_lrfilter_wave_kernel<27> / <35> (form 2) on 5 rows / 5 columns: every window row or column but five is the clamp."""
    run_filt('thin', BC6, h, w, 27, form=2, seed=5)
    run_filt('thin', BC6, h, w, 35, form=2, seed=6)


# ---- stream ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf,k', [(8, 33), (8, 45), (6, 25)])
def test_downscale_stream(sf, k):
    """cem_downscale_stream_kernel<8> and — sf 6, k 25: a geometry outside sf 2 / 3 / 4 / 8 for which esr_cem_sep_form(0, ...) returns 1 — <0>;
    LR 70 x 40: 2 strips of 64 / 6 rows, 2 column tiles of 32 / 8."""
    pres = sorted({0, _shipped_pre(sf), sf - 1})
    for j, pre in enumerate(pres):
        run_down('stream', BC6, 70, 40, sf, k, pre, form=1, fused=j > 0, lr_pad=3 if j == 2 else 0, off=1 if j == 1 else 0, seed=sf + k + j)


# ---- tile_sep ----------------------------------------------------------------------------------------------------------------------------
TILE_SIZES = [(21, 37), (16, 16), (32, 64), (1, 1), (1, 5), (5, 1)]
TILE_K = {1: 7, 2: 9, 3: 15, 4: 17, 8: 33, 5: 11, 6: 13}
DOWN_FORM = {1: 0, 2: 0, 3: 0, 4: 0, 8: 1, 5: 0, 6: 0}          # (x8: every k the tile kernel could hold takes the streaming kernel)


@pytest.mark.parametrize('sf', [1, 2, 3, 4, 8, 5, 6])
def test_tile_sep_downscale(sf):
    """cem_downscale_sep_kernel<sf> (form 0; <0> for sf 1, 5, 6; sf 8 lands on the streaming kernel, form 1) on every small size, every pre, plain and fused."""
    k = TILE_K[sf]
    for i in range(max(len(TILE_SIZES), sf)):
        h, w = TILE_SIZES[i % len(TILE_SIZES)]
        lr_pad = 1 if (i % 3 == 2 and min(h, w) > 2) else 0
        run_down('tile_sep', BC6, h, w, sf, k, i % sf, form=DOWN_FORM[sf], fused=i % 3 > 0, lr_pad=lr_pad, seed=sf + i)


@pytest.mark.parametrize('k', [7, 27, 35])
def test_tile_sep_lrfilter(k):
    """cem_lrfilter_sep_kernel (form 0) on every small size."""
    for i, (h, w) in enumerate(TILE_SIZES):
        run_filt('tile_sep', BC6, h, w, k, form=0, off=i % 2, seed=k + i)


def _fold_fits(sf, k, kf, mode):
    """The on-chip budget of esr_cem_filter_upscale_sep (64 KiB of LDS; upscale_sep_launch in csrc/esr_cem.hip): the sample windows, the 64-row vertical pass,
    the taps, and the raw window of e with its horizontal pass."""
    wr = wc = (64 + 2 * (k // 2)) // sf + 3
    two = 2 if mode >= 2 else 1
    vp = wc + (16 - wc % 32 + 32) % 32
    er, ec = wr + kf - 1, wc + kf - 1
    return 4 * (two * wr * wc + two * 64 * vp + 2 * k + er * (ec | 1) + er * (wc | 1)) <= 64 * 1024


# how many of a factor's fold launches below fit on chip (the rest return ESR_E_UNSUPPORTED and must write nothing): stated, so that a silent
# ESR_E_UNSUPPORTED cannot empty the bit-equality check
FOLDED = {sf: sum(_fold_fits(sf, TILE_K[sf], (27, 35)[i % 2], i % 4) for i in range(max(len(TILE_SIZES), sf, 4))) for sf in (2, 3, 4, 8, 5, 6)}


@pytest.mark.parametrize('sf', [2, 3, 4, 8, 5, 6])
def test_tile_sep_upscale_and_fold(sf):
    """cem_upscale_sep_kernel<TWO, sf, FILT> (form 0; sf 5, 6: the generic <.., 0, ..>) on every small size, every pre in [0, sf - 1) (sf - 1: test_upscale_pre_last),
    every mode; the fold (FILT, kf 27 / 35) is bit-identical to esr_cem_lrfilter_sep's tile kernel followed by esr_cem_upscale_sep."""
    k = TILE_K[sf]
    L = _lib().lib
    folded = 0
    for i in range(max(len(TILE_SIZES), sf, 4)):
        h, w = TILE_SIZES[i % len(TILE_SIZES)]
        pre, mode = i % max(sf - 1, 1), i % 4
        crop = min(i % 3, (min(h, w) * sf - 1) // 2)
        taps = make_taps(k, sf + i, True)
        run_up('tile_sep', BC6, h, w, sf, k, pre, mode, crop=crop, form=0, taps=taps, off=i % 2, seed=sf + i)
        kf = (27, 35)[i % 2]
        o, o2, (e, e2, g), rc = run_up('tile_sep', BC6, h, w, sf, k, pre, mode, crop=crop, taps=taps, seed=sf + i, fold_kf=kf)
        # ESR_E_UNSUPPORTED exactly where the header says so: the fold's windows do not fit on chip
        assert (rc == 0) == _fold_fits(sf, k, kf, mode), (sf, k, kf, mode, rc)
        if rc != 0:
            continue
        folded += 1
        # the two (three) launches
        assert _form(2, 1, kf, 0, h, w) == 0
        tf = dev_taps(R.synthetic_sep(kf, 50 + sf + i))
        fk = torch.empty_like(e)
        assert L.esr_cem_lrfilter_sep(e.data_ptr(), 2, 3, h, w, tf[0].data_ptr(), tf[1].data_ptr(), kf, fk.data_ptr(), _stream()) == 0
        fk2 = None
        if e2 is not None:
            fk2 = torch.empty_like(e2)
            assert L.esr_cem_lrfilter_sep(e2.data_ptr(), 2, 3, h, w, tf[0].data_ptr(), tf[1].data_ptr(), kf, fk2.data_ptr(), _stream()) == 0
        td = dev_taps(taps)
        p, p2 = torch.empty_like(o), torch.empty_like(o)
        assert L.esr_cem_upscale_sep(fk.data_ptr(), ptr(fk2), 2, 3, h, w, sf, pre, td[0].data_ptr(), td[1].data_ptr(), k, ptr(g), crop, mode, 0.75, p.data_ptr(),
                                     p2.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(o, p)
        if mode == 3:
            assert torch.equal(o2, p2)
    assert folded == FOLDED[sf], (sf, folded)


# ---- tile_2d, untiled --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf,k', [(2, 9), (3, 15), (4, 17), (5, 11)])
def test_tile_2d(sf, k):
    """cem_downscale_tiled_kernel, cem_lrfilter_tiled_kernel, cem_upscale_tiled_kernel<false / true> with full-rank taps on LR 21 x 37 and 40 x 70
    (several ragged tiles)."""
    for i, (h, w) in enumerate([(21, 37), (40, 70)]):
        for pre in range(sf):
            j = i + pre
            run_down('tile_2d', BC6, h, w, sf, k, pre, sep=False, fused=j % 2 == 1, lr_pad=(j % 4 == 3) * 2, off=j % 2, seed=sf + j)
            if pre < sf - 1:                                # (pre == sf - 1: test_upscale_pre_last)
                run_up('tile_2d', BC6, h, w, sf, k, pre, j % 4, crop=(0, 1, sf)[j % 3], sep=False, off=j % 2, seed=sf + j)
        run_filt('tile_2d', BC6, h, w, k + 10, sep=False, seed=sf + i)


def test_untiled_kernels_behind_the_plane_limit():
    """B * C = 65536 planes of 2 x 3 LR at sf 2, k 9 with rank-one taps through cem_ops.*_raw: the separable entries return ESR_E_UNSUPPORTED (more than 65535
    planes) and the 2-D entries run cem_downscale_kernel, cem_lrfilter_kernel and cem_upscale_kernel<false / true> (no tile kernel either)."""
    from esr_hip import cem_ops
    L, E = _lib().lib, _lib().ESR_E_UNSUPPORTED
    B, C, h, w, sf, k, pre = 256, 256, 2, 3, 2, 9, 0
    tv, th = R.synthetic_sep(k, 21)
    t2 = torch.outer(tv, th).to(DEV)                        # (fp32 products: what the 2-D kernels are handed)
    assert cem_ops._sep(t2, torch.device(DEV, torch.cuda.current_device())) is not None
    y = R.uniform((B, C, h * sf, w * sf), 31).to(DEV)
    x = R.uniform((B, C, h, w), 32).to(DEV)
    x2 = R.uniform((B, C, h, w), 33).to(DEV)
    g = R.uniform((B, C, h * sf, w * sf), 34, 0.0, 1.0).to(DEV)
    d = torch.empty(B, C, h, w, device=DEV)
    tvd, thd = tv.to(DEV), th.to(DEV)
    assert L.esr_cem_downscale_sep(y.data_ptr(), B, C, h, w, sf, pre, tvd.data_ptr(), thd.data_ptr(), k, None, 0, d.data_ptr(), _stream()) == E
    assert L.esr_cem_lrfilter_sep(x.data_ptr(), B, C, h, w, tvd.data_ptr(), thd.data_ptr(), k, d.data_ptr(), _stream()) == E
    n = k * k
    got = cem_ops.downscale_raw(y, t2, sf, pre, lr=x)
    ref, S = R.downscale(y, t2, sf, pre, lr=x)
    judge('untiled', got, ref, R.bound(n, S, ref), 'downscale fused')
    got = cem_ops.lr_filter_raw(x, t2)
    ref, S = R.lrfilter(x, t2)
    judge('untiled', got, ref, R.bound(n, S, ref), 'lrfilter')
    for pre in (0, 1):
        got = cem_ops.upscale_raw(x, t2, sf, pre, g=g, crop=1, mode=1)
        ref, S = R.upscale(x, t2, sf, pre, g=g, crop=1, mode=1)
        judge('untiled', got, ref, R.bound(n, S, ref, g[:, :, 1:-1, 1:-1]), 'upscale mode 1 pre %d' % pre)
        got = cem_ops.upscale_raw(x, t2, sf, pre, f2=x2, g=g, crop=0, mode=3)
        ref, S = R.upscale(x, t2, sf, pre, f2=x2, g=g, crop=0, mode=3)
        judge('untiled', got[0], ref[0], R.bound(n, S[0], ref[0]), 'upscale mode 3 out pre %d' % pre)
        judge('untiled', got[1], ref[1], R.bound(n, S[1], ref[1], g), 'upscale mode 3 out2 pre %d' % pre)


# ---- batch -------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_and_its_planes_run_the_same_arithmetic():
    """esr_cem_sep_form: 'decided from these arguments alone, never from the batch, so that a batch and its chunks run the same arithmetic'.  96 planes
    against each plane alone, bit for bit: the wave kernels (form 2) cut the upscale and LR-filter strips by wave_strips_target / (B C nct), which
    moves between 96 planes and one."""
    L = _lib().lib
    B, C, sf, k, pre, kf = 32, 3, 4, 17, 1, 27
    assert _form(0, sf, k, pre, 64, 64) == 2 and _form(1, sf, k, pre, 64, 64) == 2 and _form(2, 1, kf, 0, 128, 128) == 2
    tv, th = dev_taps(make_taps(k, 1, True))
    fv, fh = dev_taps(make_taps(kf, 2, True))
    y = R.uniform((B, C, 256, 256), 51).to(DEV)
    lr = R.uniform((B, C, 64, 64), 52).to(DEV)
    g = R.uniform((B, C, 256, 256), 53, 0.0, 1.0).to(DEV)
    x = R.uniform((B, C, 128, 128), 54).to(DEV)
    d, u, fo = torch.empty_like(lr), torch.empty_like(g), torch.empty_like(x)
    assert L.esr_cem_downscale_sep(y.data_ptr(), B, C, 64, 64, sf, pre, tv.data_ptr(), th.data_ptr(), k, lr.data_ptr(), 0, d.data_ptr(), _stream()) == 0
    assert L.esr_cem_upscale_sep(lr.data_ptr(), None, B, C, 64, 64, sf, pre, tv.data_ptr(), th.data_ptr(), k, g.data_ptr(), 0, 1, 0.0, u.data_ptr(), None, _stream()) == 0
    assert L.esr_cem_lrfilter_sep(x.data_ptr(), B, C, 128, 128, fv.data_ptr(), fh.data_ptr(), kf, fo.data_ptr(), _stream()) == 0
    d1, u1, fo1 = torch.empty_like(lr), torch.empty_like(g), torch.empty_like(x)
    for b in range(B):
        for c in range(C):
            assert L.esr_cem_downscale_sep(y[b, c].data_ptr(), 1, 1, 64, 64, sf, pre, tv.data_ptr(), th.data_ptr(), k, lr[b, c].data_ptr(), 0, d1[b, c].data_ptr(), _stream()) == 0
            assert L.esr_cem_upscale_sep(lr[b, c].data_ptr(), None, 1, 1, 64, 64, sf, pre, tv.data_ptr(), th.data_ptr(), k, g[b, c].data_ptr(), 0, 1, 0.0,
                                         u1[b, c].data_ptr(), None, _stream()) == 0
            assert L.esr_cem_lrfilter_sep(x[b, c].data_ptr(), 1, 1, 128, 128, fv.data_ptr(), fh.data_ptr(), kf, fo1[b, c].data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, d1) and torch.equal(u, u1) and torch.equal(fo, fo1)


# ---- real taps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf,kernel', [(4, None), (3, 'blurry_cubic_1.0'), (8, 'blurry_cubic_2.0')])
def test_product_taps(sf, kernel):
    """The product's own taps (factors as cem_ops hands them to the kernels) at LR 48 x 90: downscale and upscale wave kernels (form 2; x3 blurry_cubic_1.0 is
    k 17 = <3, 6>), the LR filter's tile kernel (k 27 / 41 / 35) and, 128 x 132, its wave kernel where k is 27 or 35."""
    import CEM.CEMnet as C
    from CEM.imresize_CEM import imresize
    from esr_hip import cem_ops
    imresize.kernels = {}
    net = C.CEMnet(C.Get_CEM_Conf(sf), upscale_kernel=kernel).WrapArchitecture_PyTorch(generated_image=None)
    imresize.kernels = {}
    dev = torch.device(DEV, torch.cuda.current_device())
    pre = net.pre_stride
    sd, si, su = (tuple(t.cpu() for t in cem_ops._sep(op.taps(), dev)) for op in (net.DownscaleOP, net.Conv_LR_with_Inv_hTh_OP, net.Upscale_OP))
    k, kf = sd[0].shape[0], si[0].shape[0]
    run_down('product_taps', BC6, 48, 90, sf, k, pre, form=2, fused=True, lr_pad=2, taps=sd)
    run_up('product_taps', BC6, 48, 90, sf, k, pre, 1, crop=sf, form=2, taps=su)
    run_up('product_taps', BC6, 48, 90, sf, k, pre, 2, crop=0, form=2, taps=su, rng=1.0)
    run_filt('product_taps', BC6, 48, 90, kf, form=0, taps=si)
    if kf in (27, 35):
        run_filt('product_taps', BC6, 128, 132, kf, form=2, taps=si)


# ---- adjoint -----------------------------------------------------------------------------------------------------------------------------
ADJ_K = {1: 27, 2: 9, 3: 15, 4: 17, 8: 33, 5: 11}
ADJ_FRAMES = [(13, 9), (2, 2), (3, 2)]          # LR sizes; the small ones give N < k on both axes (one-row / one-column frames: the test after this one)


@pytest.mark.parametrize('sep', [True, False], ids=['sep', '2d'])
@pytest.mark.parametrize('sf', [1, 2, 3, 4, 8, 5])
def test_adjoint(sf, sep):
    """esr_cem_adjoint_sep (cem_adjoint_1d_kernel<0> then <1>; plain / base + / base -) and esr_cem_adjoint (cem_adjoint_kernel; accumulate 0 / 1) against float64
    autograd of the restatement, asymmetric taps, every pre, the three ops (sf 1: the LR filter and the x1 downscale)."""
    k = ADJ_K[sf] if sep else min(ADJ_K[sf], 17)
    i = 0
    for h, w in ADJ_FRAMES:
        for pre in range(sf):
            for kind in (('lrfilter', 'downscale') if sf == 1 else ('downscale', 'upscale')):
                run_adjoint('adjoint', kind, BC6, h, w, sf, k, pre, sep, i % (3 if sep else 2), seed=sf + i)
                i += 1


@pytest.mark.parametrize('sep', [True, False], ids=['sep', '2d'])
def test_adjoint_on_a_frame_of_one_row_or_column(sep):
    """A frame position that is both the first and the last of its axis (Ny == 1 or Nx == 1) receives EVERY tap of every output: the forward is
    (sum of the taps) x[0] there."""
    for i, (h, w) in enumerate([(1, 7), (7, 1), (1, 1)]):
        run_adjoint('fixes', 'lrfilter', BC6, h, w, 1, 27 if sep else 9, 0, sep, i % 2, seed=i)
        run_adjoint('fixes', 'downscale', BC6, h, w, 1, 7, 0, sep, 0, seed=3 + i)


def test_adjoint_raw_dispatch():
    """cem_ops.adjoint_raw: rank-one taps take esr_cem_adjoint_sep, full-rank taps esr_cem_adjoint; both with base and alpha."""
    from esr_hip import autograd as AG
    from esr_hip import cem_ops
    sf, k, pre, h, w = 4, 17, 1, 13, 9
    tv, th = R.synthetic_sep(k, 5)
    for taps, sep in ((torch.outer(tv, th).to(DEV), True), (R.synthetic_2d(k, 5).to(DEV), False)):
        tabs = AG.AdjointTables(taps)
        assert (tabs.v is not None) == sep
        ref_taps = tuple(t.cpu() for t in cem_ops._sep(taps, taps.device)) if sep else taps.cpu()
        for kind, key in (('downscale', 'downscale'), ('lrfilter', 'lr_filter'), ('upscale', 'upscale')):
            s = 1 if kind == 'lrfilter' else sf
            (hq, wq), (hn, wn), (sq, _, _, _, _, _) = _adjoint_geometry(kind, s, pre if s > 1 else 0, h, w)
            dy = R.uniform((2, 3, hq, wq), 61).to(DEV)
            base = R.uniform((2, 3, hn, wn), 62).to(DEV)
            got = cem_ops.adjoint_raw(dy, tabs, key, s, pre if s > 1 else 0, (2, 3, hn, wn), base=base, alpha=-1.0)
            adj, S = R.adjoint(kind, dy, ref_taps, s, pre if s > 1 else 0, (2, 3, hn, wn))
            ref = base.double() - adj
            judge('adjoint', got, ref, R.bound(R.adjoint_terms(k, sq, hq, wq, sep), S + base.double().abs(), ref), 'adjoint_raw %s %s' % (kind, 'sep' if sep else '2d'))


# ---- fixes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sf', [2, 3, 4, 8, 5])
def test_upscale_pre_last(sf):
    """pre == sf - 1: the last row and column of the zero-stuffed image hold samples and the replicate pad repeats them (the header's 'zero-stuff at
    (pre, pre), replicate-pad k / 2, correlate').
    cem_upscale_sep_kernel / cem_upscale_tiled_kernel / (B*C > 65535) cem_upscale_kernel fold the last sample row and column as they fold the first for
    pre == 0, and the wave kernel, whose premise is a frame of zeros, takes 0 < pre < sf - 1 only (form 0 here at any size)."""
    k, pre = TILE_K[sf], sf - 1
    for i, (h, w) in enumerate([(21, 37), (1, 5), (5, 1), (48, 90)]):
        crop = min((0, 1, sf)[i % 3], (min(h, w) * sf - 1) // 2)
        run_up('fixes', BC6, h, w, sf, k, pre, i % 4, crop=crop, form=0, off=i % 2, seed=sf + i)
        run_up('fixes', BC6, h, w, sf, k, pre, (i + 2) % 4, crop=crop, sep=False, seed=sf + i + 4)
        run_up('fixes', BC6, h, w, sf, k, pre, (i + 1) % 4, crop=crop, seed=sf + i + 8, fold_kf=27)
        # and its adjoint agrees with it
        run_adjoint('fixes', 'upscale', BC6, h, w, sf, k, pre, True, i % 3, seed=sf + i)
        run_adjoint('fixes', 'upscale', BC6, h, w, sf, min(k, 17), pre, False, i % 2, seed=sf + i)


def test_upscale_pre_last_behind_the_plane_limit():
    """cem_upscale_kernel<false / true> (B * C = 65536) with pre == sf - 1: test_untiled_kernels_behind_the_plane_limit runs pre 0 and 1 at sf 2; here sf 3, pre 2."""
    from esr_hip import cem_ops
    B, C, h, w, sf, k, pre = 256, 256, 2, 3, 3, 9, 2
    tv, th = R.synthetic_sep(k, 22)
    t2 = torch.outer(tv, th).to(DEV)
    x = R.uniform((B, C, h, w), 35).to(DEV)
    x2 = R.uniform((B, C, h, w), 36).to(DEV)
    g = R.uniform((B, C, h * sf, w * sf), 37, 0.0, 1.0).to(DEV)
    got = cem_ops.upscale_raw(x, t2, sf, pre, f2=x2, g=g, crop=0, mode=2, rng=0.5)
    ref, S = R.upscale(x, t2, sf, pre, f2=x2, g=g, crop=0, mode=2, range=0.5)
    judge('fixes', got, ref, R.bound_mode2(k * k, S, g, 0, 0.5), 'untiled upscale mode 2 x3 pre 2')


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    """Every ESR_E_ARG condition of the eight entry points: the call returns ESR_E_ARG and its destinations keep their sentinels."""
    L, E = _lib().lib, _lib().ESR_E_ARG
    B, C, h, w, sf, k, pre = 2, 3, 8, 10, 4, 17, 1
    tv, th = dev_taps(make_taps(k, 1, True))
    t2 = dev_taps(make_taps(k, 1, False))
    fv, fh = dev_taps(make_taps(27, 2, True))
    y = put(R.uniform((B, C, h * sf, w * sf), 71))
    x = put(R.uniform((B, C, h, w), 72))
    g = put(R.uniform((B, C, h * sf, w * sf), 73, 0.0, 1.0))
    s = _stream()

    def refused(call, *dsts):
        assert call() == E
        for d in dsts:
            d.check(written=False)

    # downscale, both entry points: (sf, pre, k, lr_pad with lr, h)
    for bad in ({'k': 16}, {'pre': sf}, {'pre': -1}, {'sf': 0}, {'lr_pad': 4}, {'lr_pad': 5}, {'lr_pad': -1}, {'h': 0}, {'w': 0}, {'B': 0}, {'C': 0}, {'k': 0}, {'y': None}, {'taps': None}, {'th': None}):
        a = dict(y=y.data_ptr(), B=B, C=C, h=h, w=w, sf=sf, pre=pre, k=k, lr=x.data_ptr() if 'lr_pad' in bad else None, lr_pad=0, taps=True, th=th.data_ptr())
        a.update(bad)
        d = Carved((B, C, h, w))
        refused(lambda: L.esr_cem_downscale_sep(a['y'], a['B'], a['C'], a['h'], a['w'], a['sf'], a['pre'], tv.data_ptr() if a['taps'] else None, a['th'], a['k'],
                                                a['lr'], a['lr_pad'], d.ptr, s), d)
        if 'th' not in bad:
            refused(lambda: L.esr_cem_downscale(a['y'], a['B'], a['C'], a['h'], a['w'], a['sf'], a['pre'], t2.data_ptr() if a['taps'] else None, a['k'], a['lr'],
                                                a['lr_pad'], d.ptr, s), d)
    d = Carved((B, C, h, w))
    # no destination
    assert L.esr_cem_downscale_sep(y.data_ptr(), B, C, h, w, sf, pre, tv.data_ptr(), th.data_ptr(), k, None, 0, None, s) == E
    assert L.esr_cem_downscale(y.data_ptr(), B, C, h, w, sf, pre, t2.data_ptr(), k, None, 0, None, s) == E
    assert L.esr_cem_lrfilter_sep(x.data_ptr(), B, C, h, w, fv.data_ptr(), fh.data_ptr(), 27, None, s) == E
    assert L.esr_cem_lrfilter(x.data_ptr(), B, C, h, w, t2.data_ptr(), k, None, s) == E
    # LR filter
    for bad in ({'k': 26}, {'k': 0}, {'w': 0}, {'h': 0}, {'C': 0}, {'B': 0}, {'x': None}, {'tv': None}, {'th': None}):
        a = dict(x=x.data_ptr(), B=B, C=C, h=h, w=w, k=27, tv=fv.data_ptr(), th=fh.data_ptr())
        a.update(bad)
        refused(lambda: L.esr_cem_lrfilter_sep(a['x'], a['B'], a['C'], a['h'], a['w'], a['tv'], a['th'], a['k'], d.ptr, s), d)
        if 'th' not in bad:
            refused(lambda: L.esr_cem_lrfilter(a['x'], a['B'], a['C'], a['h'], a['w'], t2.data_ptr() if a['tv'] else None, a['k'], d.ptr, s), d)
    # upscale, three entry points
    o, o2 = Carved((B, C, h * sf, w * sf)), Carved((B, C, h * sf, w * sf))
    for bad in ({'k': 18}, {'pre': sf}, {'pre': -1}, {'sf': 1}, {'crop': 16}, {'crop': 20}, {'crop': -1}, {'mode': 4}, {'mode': -1}, {'mode': 1, 'g': None}, {'mode': 2, 'f2': None},
                {'mode': 3, 'out2': None}, {'mode': 3, 'g': None}, {'h': 0}, {'w': 0}, {'B': 0}, {'C': 0}, {'k': 0}, {'f': None}, {'tv': None}, {'th': None},
                {'out': None}):
        a = dict(f=x.data_ptr(), f2=x.data_ptr(), B=B, C=C, h=h, w=w, sf=sf, pre=pre, k=k, g=g.data_ptr(), crop=0, mode=0, out=o.ptr, out2=o2.ptr,
                 tv=tv.data_ptr(), th=th.data_ptr())
        a.update(bad)
        head = (a['f'], a['f2'], a['B'], a['C'], a['h'], a['w'], a['sf'], a['pre'])
        tail = (a['k'], a['g'], a['crop'], a['mode'], 0.5, a['out'], a['out2'], s)
        refused(lambda: L.esr_cem_upscale_sep(*head, a['tv'], a['th'], *tail), o, o2)
        if 'th' not in bad:
            refused(lambda: L.esr_cem_upscale(*head, t2.data_ptr() if a['tv'] else None, *tail), o, o2)
        refused(lambda: L.esr_cem_filter_upscale_sep(*head, fv.data_ptr(), fh.data_ptr(), 27, a['tv'], a['th'], *tail), o, o2)
    head = (x.data_ptr(), None, B, C, h, w, sf, pre)
    tail = (k, None, 0, 0, 0.0, o.ptr, None, s)
    for kf, a, b in ((0, fv.data_ptr(), fh.data_ptr()), (26, fv.data_ptr(), fh.data_ptr()), (27, None, fh.data_ptr()), (27, fv.data_ptr(), None)):
        refused(lambda: L.esr_cem_filter_upscale_sep(*head, a, b, kf, tv.data_ptr(), th.data_ptr(), *tail), o)
    # adjoints: extents past the frame, even k, missing pointers
    from esr_hip import autograd as AG
    tabs = AG.tap_tables(make_taps(k, 1, False)).to(DEV)
    tb = AG.tap_tables_1d(make_taps(k, 1, True)[0]).to(DEV)
    dy = put(R.uniform((B, C, h, w), 74))
    dx, tmp = Carved((B, C, h * sf, w * sf)), Carved((B * C * h * w * sf,))
    good = dict(hq=h, wq=w, sq=sf, oq=pre, Ny=h * sf, Nx=w * sf, k=k, hn=h * sf, wn=w * sf, sn=1, on=0)
    for bad in ({'Ny': h * sf - 1}, {'Nx': w * sf - 1}, {'oq': sf + 1}, {'on': 1}, {'hn': h * sf + 1}, {'k': 16}, {'sq': 0}, {'sn': 0}, {'hq': 0}, {'wq': 0}, {'hn': 0}, {'wn': 0},
                {'wn': w * sf + 1}, {'k': 0}, {'B': 0}, {'C': 0}, {'dy': None}, {'tab': None}, {'dx': None}):
        a = dict(good, B=B, C=C, dy=dy.data_ptr(), tab=True, dx=dx.ptr)
        a.update(bad)
        refused(lambda: L.esr_cem_adjoint(a['dy'], a['B'], a['C'], a['hq'], a['wq'], a['sq'], a['oq'], a['Ny'], a['Nx'], tabs.data_ptr() if a['tab'] else None, a['k'], a['hn'], a['wn'], a['sn'],
                                          a['on'], a['dx'], 0, s), dx)
        refused(lambda: L.esr_cem_adjoint_sep(a['dy'], a['B'], a['C'], a['hq'], a['wq'], a['sq'], a['oq'], a['Ny'], a['Nx'], tb.data_ptr() if a['tab'] else None, tb.data_ptr(), a['k'], a['hn'],
                                              a['wn'], a['sn'], a['on'], tmp.ptr, None, 1.0, a['dx'], s), dx, tmp)
    refused(lambda: L.esr_cem_adjoint_sep(dy.data_ptr(), B, C, h, w, sf, pre, h * sf, w * sf, tb.data_ptr(), None, k, h * sf, w * sf, 1, 0, tmp.ptr, None, 1.0,
                                          dx.ptr, s), dx, tmp)
    refused(lambda: L.esr_cem_adjoint_sep(dy.data_ptr(), B, C, h, w, sf, pre, h * sf, w * sf, tb.data_ptr(), tb.data_ptr(), k, h * sf, w * sf, 1, 0, None, None, 1.0,
                                          dx.ptr, s), dx)
    # esr_cem_sep_form itself
    assert _form(3, sf, k, pre, h, w) == E and _form(0, sf, 16, pre, h, w) == E and _form(0, 0, k, pre, h, w) == E and _form(1, sf, k, pre, 0, w) == E
