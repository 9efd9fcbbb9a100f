"""The esr_conv3x3_wgrad descriptor contract (include/esr_hip.h) and its batch forms, against a float64 restatement of

    dW[co][e][ky][kx] = d0 + alpha * sum_{b,y,x} dY[b,co,y,x] * Xpad_up[b,e,y+ky,x+kx]      e over [latent channels][main channels]
    db[co]            = d0 + alpha * sum_{b,y,x} dY[b,co,y,x]

written here (Xpad_up: the nearest x`upsample` of X with a one-pixel zero border; d0: what dW / db held before the launch).  Operands are
buffers this file lays out itself ([planes][B][CG][H+2][W+2][8], zero border); the reference reads the STORED planes back and sums hi (+ lo)
in float64, so it multiplies exactly what the kernel multiplied.  Launches go straight through the C-ABI, so every field can be set.

Element-wise bound, for every dW and db element (u = 2^-24, the fp32 unit roundoff):

    |dw - ref| <= c_fmt * S + L * u * (S + |d0|),      S = |alpha| * sum |dY| |X|   (db: X = 1)

c_fmt covers the products the kernel does not form.  One-plane bf16 and fp16: none — a product of two stored 16-bit values (8 x 8 or 11 x 11
significant bits) is exact in fp32 — so c_fmt = 0.  split (hi+lo bf16: dYhi*Xhi + dYhi*Xlo + dYlo*Xhi): the dropped dYlo*Xlo, each |lo| at most
half an ulp of its hi, 2^-8 |hi|, so 2^-16 |dYhi| |Xhi|, and |hi| <= (1 + 2^-8) |hi + lo|: c_fmt = 2^-15.
L is the longest fp32 addition chain into one result.  A wave multiplies 4 K steps of 16 pixels per 256-pixel tile, with 1 MFMA per step (3 in
split, all into one accumulator), over the T = ceil(tiles / slices) tiles of its slice; one MFMA sums 16 products (counted as 16 additions);
then the 4-wave LDS sum (4), the slice fold (nslices additions, from 0), the alpha multiply and the final += (1 each):

    L = 16 + 4 * T * mfmas + 4 + nslices + 2

(the batch forms slice by a granule of the whole set: there T and nslices are bounded by the layer's 8 x 32 tile count).
fp16 subnormal operands are NOT flushed by the fp16 MFMA: test_f16_subnormal_dy holds an all-subnormal dY (k * 2^-24, the range a scaled
mixed-precision gradient reaches) to the same c_fmt = 0 bound.

Outputs are pre-filled with random d0 (the header: ACCUMULATED into) between NaN guard words, which must keep their bits; nothing past cout or
lat + cin_main is written.  The lanes past cout / cin_main / lat of a partial last group and every group in front of and behind a view hold
NaN, so a read of any of them reaches a stored element as NaN; the workspace starts as NaN too (it must be written before it is read).

Every case asserts the path esr_conv3x3_wgrad_tiling reports (tile shape, slices, ESR_WGRAD_FORM_* bits) and that its comparator rejects
planted errors: the last tile column and the last tile row dropped, X shifted by one pixel for one tap, latent and main channels swapped,
the bias summed over image 0 only, alpha missing on the bias, and (split) one operand's lo plane left out.

Which test reaches which path (bf16 / split / f16 each, except where named):
    8x32 tiles, general copies (hi+lo, or upsample)   test_single[split-*], test_single[*-ups*]
    8x32 tiles, fast copies (one plane, no upsample)   test_single[bf16-*], test_single[f16-*]
    27-column latent tile (lat 1-3)                    test_single[*-lat1/2/3], test_s2d[*-lat2_defect1]
    main input run as the 27-column tile (cin <= 3)    test_single[*-cin1/2/3]
    regular latent tile (lat 4, 8)                     test_single[*-lat4/8], test_s2d[*-lat5_16x16]
    S2D tap-skipping kernel, 8x32 / 16x16 / 32x8       test_s2d[bf16|split-*] (shape 0: 8x8, lat2; shape 1: 16x16; shape 2: stacked 4x4)
    plain kernel under s2d-looking hints               test_s2d[*-cin96], test_s2d[*-other_masks], test_s2d[f16-*]
    one slice, direct += into dW                       test_single[*-direct*], test_single[*-geom1x1x1], test_batch_* (big sets)
    workspace slices + fold kernel                     almost every test_single case
    upsample 2, 3, 4, 5, 6, 8 with partial tiles       test_single[*-ups*]
    group-slice views, stacked (tall) views            test_single[*-views], test_single[*-tall], test_s2d[*-stacked4x4]
    batch: _batch, _upload + _run, parts, _run_side,   test_batch[*], test_batch_parts_with_s2d[*], test_batch_rebase
    rebase
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_UNSUPPORTED = -1, -2
NAN16 = 0x7FA5         # a NaN both as bf16 and as fp16
GUARD32 = 0x7FC0DEAD   # an fp32 NaN: the guard words around dW / db
NG = 64                # guard words on each side
U = 2.0 ** -24
S2D = (432, 216, 54, 27)
FORM_LAT27, FORM_MAIN27, FORM_S2D, FORM_FAST = 1, 2, 4, 8


class Fmt:
    def __init__(self, name, planes, vfmt, dtype, c_fmt, mfmas):
        self.name, self.planes, self.vfmt, self.dtype, self.c_fmt, self.mfmas = name, planes, vfmt, dtype, c_fmt, mfmas


FMTS = {f.name: f for f in (Fmt('split', 2, 0, torch.bfloat16, 2.0 ** -15, 3), Fmt('bf16', 1, 0, torch.bfloat16, 0.0, 1),
                            Fmt('f16', 1, 1, torch.float16, 0.0, 1))}


def _lib():
    from esr_hip import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands

class Operand:
    """`nch` channels in groups [cg0, cg0 + ceil(nch/8)) of a [planes][B][CG][H+2][W+2][8] buffer with `behind` more groups after them
    (stacked: [planes][CG][B][H+2][W+2][8], viewed as one tall image).  Interior values uniform(-scale, scale) (or `values`) rounded to the
    format (split: hi + the bf16 residue); zero border; NaN in the pad lanes of the last group and in every other group."""

    def __init__(self, fmt, B, H, W, nch, cg0=0, behind=0, scale=1.0, seed=0, stacked=False, values=None):
        f = self.f = FMTS[fmt]
        self.B, self.H, self.W, self.nch, self.cg0, self.stacked = B, H, W, nch, cg0, stacked
        ncg = self.ncg = (nch + 7) // 8
        CG = cg0 + ncg + behind
        if values is None:
            g = torch.Generator().manual_seed(seed)
            values = (torch.rand(B, ncg * 8, H, W, generator=g, dtype=torch.float64) * 2 - 1) * scale
        hi = values.to(f.dtype)
        lo = (values - hi.double()).to(f.dtype)
        t = torch.zeros(f.planes, B, CG, H + 2, W + 2, 8, dtype=torch.int16)
        for p, v in enumerate((hi, lo)[:f.planes]):
            t[p, :, cg0:cg0 + ncg, 1:-1, 1:-1] = v.view(torch.int16).reshape(B, ncg, 8, H, W).permute(0, 1, 3, 4, 2)
        if nch % 8:
            t[:, :, cg0 + ncg - 1, 1:-1, 1:-1, nch % 8:] = NAN16
        t[:, :, :cg0] = NAN16
        t[:, :, cg0 + ncg:] = NAN16
        self.bits = t
        self.t = (t.permute(0, 2, 1, 3, 4, 5).contiguous() if stacked else t).to(DEV)

    def view(self):
        L = _lib()
        if self.stacked:
            P, CG, B, Hp, Wp, _ = self.t.shape
            cs = B * Hp * Wp
            hi = self.t.data_ptr() + self.cg0 * cs * 16
            return L.ActView(hi, hi + self.t.stride(0) * 2 if P == 2 else None, self.ncg, B * Hp - 2, Wp - 2, cs * CG, cs, self.f.vfmt)
        P, B, CG, Hp, Wp, _ = self.t.shape
        cs = Hp * Wp
        hi = self.t.data_ptr() + self.cg0 * cs * 16
        return L.ActView(hi, hi + self.t.stride(0) * 2 if P == 2 else None, self.ncg, self.H, self.W, CG * cs, cs, self.f.vfmt)

    def padded(self, hi_only=False):
        """float64 [B][nch][H+2][W+2] of the stored values with their border (stacked: [1][nch][B*(H+2)][W+2], one tall image)."""
        t = self.bits[:, :, self.cg0:self.cg0 + self.ncg]
        v = t[0].view(self.f.dtype).double()
        if self.f.planes == 2 and not hi_only:
            v = v + t[1].view(self.f.dtype).double()
        v = v.permute(0, 1, 4, 2, 3).reshape(self.B, self.ncg * 8, self.H + 2, self.W + 2)[:, :self.nch]
        if self.stacked:
            v = v.permute(1, 0, 2, 3).reshape(1, self.nch, self.B * (self.H + 2), self.W + 2)
        return v.to(DEV)


def _contract(dyp, xp, ups):
    """(sum dY * Xpad_up, sum |dY| |Xpad_up|) as [cout][cin][3][3], and (sum dY, sum |dY|) as [cout], from padded float64 operands."""
    dy = dyp[:, :, 1:-1, 1:-1]
    if ups > 1:
        xp = F.pad(xp[:, :, 1:-1, 1:-1].repeat_interleave(ups, 2).repeat_interleave(ups, 3), (1, 1, 1, 1))
    Bn, co = dy.shape[:2]
    cols = F.unfold(xp, 3)
    d = dy.reshape(Bn, co, -1)
    g = torch.einsum('bop,bkp->ok', d, cols).view(co, -1, 3, 3)
    s = torch.einsum('bop,bkp->ok', d.abs(), cols.abs()).view(co, -1, 3, 3)
    return g, s, d.sum((0, 2)), d.abs().sum((0, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# one layer: operands, guarded outputs, descriptor, reference

class Layer:
    def __init__(self, fmt='split', B=2, H=9, W=31, cin=13, cout=24, lat=0, ups=1, alpha=1.0, masks=None, db=True, x_cg0=0, x_behind=0,
                 dy_cg0=0, dy_behind=0, stacked=False, dy_scale=1.0, seed=0, dy_values=None, shape=0, out=None):
        self.fmt, self.f = fmt, FMTS[fmt]
        self.B, self.H, self.W, self.cin, self.cout, self.lat, self.ups = B, H, W, cin, cout, lat, ups
        self.alpha, self.masks, self.has_db, self.stacked, self.shape = alpha, masks, db, stacked, shape
        s = 97 * seed + 7 * cin + 13 * cout + H + 3 * W + 11 * lat + ups
        self.dy = Operand(fmt, B, H, W, cout, dy_cg0, dy_behind, dy_scale, seed=s + 1, stacked=stacked, values=dy_values)
        self.x = Operand(fmt, B, H // ups, W // ups, cin, x_cg0, x_behind, 1.0, seed=s + 2, stacked=stacked)
        self.xl = Operand(fmt, B, H, W, lat, 0, 0, 1.0, seed=s + 3, stacked=stacked) if lat else None
        self.nw, self.cin_t = cout * (lat + cin) * 9, lat + cin
        g = torch.Generator().manual_seed(s + 4)
        self.d0w = ((torch.rand(self.nw, generator=g, dtype=torch.float64) * 2 - 1)).float()
        self.d0b = ((torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1)).float()
        if out is None:           # own guarded buffers: [NG guards][dW][NG guards][db][NG guards]
            self.buf = torch.full((3 * NG + self.nw + cout,), GUARD32, dtype=torch.int32)
            self.woff, self.boff = NG, 2 * NG + self.nw
            self.buf[self.woff:self.woff + self.nw] = self.d0w.view(torch.int32)
            self.buf[self.boff:self.boff + cout] = self.d0b.view(torch.int32)
            self.buf = self.buf.to(DEV)
        else:                     # (flat buffer, word offset of dW, of db): the caller filled it
            self.buf, self.woff, self.boff = out
        self.init = self.buf.clone()

    def desc(self):
        L = _lib()
        d = L.WgradDesc()
        d.dy, d.x = self.dy.view(), self.x.view()
        if self.xl is not None:
            d.xlat = self.xl.view()
        d.lat, d.upsample, d.cout, d.cin_main = self.lat, self.ups, self.cout, self.cin
        d.B, d.H, d.W = (1, self.B * (self.H + 2) - 2, self.W) if self.stacked else (self.B, self.H, self.W)
        d.alpha = self.alpha
        d.dw = self.buf.data_ptr() + 4 * self.woff
        d.db = self.buf.data_ptr() + 4 * self.boff if self.has_db else None
        if self.masks:
            d.tap_masks[:] = self.masks
        return d

    def reset(self):
        self.buf.copy_(self.init)

    def tiling(self):
        t = (C.c_int32 * 5)()
        assert _lib().load_library().esr_conv3x3_wgrad_tiling(C.byref(self.desc()), t) == 0
        return tuple(t)

    def expected_form(self):
        s2d = tuple(self.masks or ()) == S2D and self.cin % 128 == 0 and self.fmt != 'f16'
        return ((FORM_LAT27 if 1 <= self.lat <= 3 else 0) | (FORM_MAIN27 if not self.lat and self.cin <= 3 and self.ups == 1 else 0) |
                (FORM_S2D if s2d else 0) | (FORM_FAST if self.f.planes == 1 and self.ups == 1 else 0))

    def launch(self):
        lib = _lib().load_library()
        d = self.desc()
        need = lib.esr_conv3x3_wgrad_workspace_floats(C.byref(d))
        assert need > 0
        ws = torch.full((need,), float('nan'), dtype=torch.float32, device=DEV)
        d.workspace, d.workspace_floats = ws.data_ptr(), need
        assert lib.esr_conv3x3_wgrad(C.byref(d), _stream()) == 0
        torch.cuda.synchronize()

    def l_bound(self, tiles_x=None, tiles_y=None, nslices=None):
        """L of the docstring.  Without a tiling (the batch forms): T and nslices at most the 8 x 32 tile count."""
        Bl, Hl = (1, self.B * (self.H + 2) - 2) if self.stacked else (self.B, self.H)
        if tiles_x is None:
            nt = -(-self.W // 32) * -(-Hl // 8) * Bl
            T, ns = nt, nt
        else:
            nt = tiles_x * tiles_y * Bl
            T, ns = -(-nt // nslices), nslices
        return 16 + 4 * T * self.f.mfmas + 4 + ns + 2

    def check(self, Lb, teeth=True, tw=None):
        """Guards, the element-wise bound, the masked-out entries, and (teeth) the planted errors."""
        raw = self.buf.cpu()
        init = self.init.cpu()
        written = torch.zeros(raw.numel(), dtype=torch.bool)
        written[self.woff:self.woff + self.nw] = True
        if self.has_db:
            written[self.boff:self.boff + self.cout] = True
        assert torch.equal(raw[~written], init[~written]), 'a guard word / an element outside dW, db was written'
        dw = raw[self.woff:self.woff + self.nw].view(torch.float32).double().view(self.cout, self.cin_t, 3, 3).to(DEV)
        db = raw[self.boff:self.boff + self.cout].view(torch.float32).double().to(DEV)
        d0w = self.d0w.double().view(self.cout, self.cin_t, 3, 3).to(DEV)
        d0b = self.d0b.double().to(DEV)
        dyp = self.dy.padded()
        xs = [self.xl.padded()] if self.xl is not None else []
        xp = torch.cat(xs + [self.x.padded()], 1)
        if self.xl is not None and self.ups > 1:
            raise AssertionError('a latent with upsample is refused')
        g, s, gb, sb = _contract(dyp, xp, self.ups)
        a = self.alpha
        ref, S = d0w + a * g, abs(a) * s
        refb, Sb = d0b + a * gb, abs(a) * sb
        bound = self.f.c_fmt * S + Lb * U * (S + d0w.abs())
        boundb = self.f.c_fmt * Sb + Lb * U * (Sb + d0b.abs())
        outside = None
        if self.masks and self.expected_form() & FORM_S2D:
            # the S2D kernel leaves the entries outside the masks as they were (esr_wgrad_desc.tap_masks)
            outside = torch.zeros(self.cout, self.cin_t, 9, dtype=torch.bool, device=DEV)
            for c in range(self.cin):
                m = self.masks[(c // 32) & 3]
                for t in range(9):
                    if not (m >> t) & 1:
                        outside[:, self.lat + c, t] = True
            outside = outside.view(self.cout, self.cin_t, 3, 3)
            assert torch.equal(dw[outside], d0w[outside]), 'the S2D kernel changed a dW entry outside the tap masks'
            ref = torch.where(outside, d0w, ref)

        def excess(y, r, bd):
            err = (y - r).abs()
            e = err / bd
            e[err == 0] = 0.0
            e[torch.isnan(err)] = float('inf')
            return float(e.max()) if e.numel() else 0.0

        ew = excess(dw, ref, bound)
        assert ew <= 1.0, 'dW: element-wise bound exceeded, worst |dw-ref|/bound = %.3g' % ew
        if self.has_db:
            eb = excess(db, refb, boundb)
            assert eb <= 1.0, 'db: element-wise bound exceeded, worst %.3g' % eb
        else:
            assert torch.equal(db, d0b), 'db == NULL: ... but the db storage changed'
        if not teeth:
            return dw, db
        planted = []
        tw = tw or (32, 8)
        dyi = dyp.clone()
        dyi[:, :, 1:-1, 1:-1][..., ((dyp.shape[3] - 2 - 1) // tw[0]) * tw[0]:] = 0      # without the last tile column
        planted.append(('last tile column dropped', d0w + a * _contract(dyi, xp, self.ups)[0], None))
        dyi = dyp.clone()
        dyi[:, :, 1:-1, 1:-1][:, :, ((dyp.shape[2] - 2 - 1) // tw[1]) * tw[1]:] = 0
        planted.append(('last tile row dropped', d0w + a * _contract(dyi, xp, self.ups)[0], None))
        bad = ref.clone()
        bad[:, :, 1, 1] = (d0w + a * g)[:, :, 1, 2]
        planted.append(('X shifted by one pixel at the centre tap', bad, None))
        if self.lat and self.cin >= self.lat:
            k = self.lat
            bad = ref.clone()
            bad[:, :k], bad[:, k:2 * k] = ref[:, k:2 * k].clone(), ref[:, :k].clone()
            planted.append(('latent and main channels swapped', bad, None))
        if self.has_db and self.B > 1 and not self.stacked:
            planted.append(('bias over image 0 only', None, d0b + a * dyp[0, :, 1:-1, 1:-1].sum((1, 2))))
        if self.has_db and a != 1.0:
            planted.append(('alpha missing on the bias', None, d0b + gb))
        if self.f.planes == 2:
            xh = torch.cat(([self.xl.padded(hi_only=True)] if self.xl is not None else []) + [self.x.padded(hi_only=True)], 1)
            planted.append(("X's lo plane left out", d0w + a * _contract(dyp, xh, self.ups)[0], None))
        for what, bw, bb in planted:
            if bw is not None:
                if outside is not None:
                    bw = torch.where(outside, d0w, bw)
                assert excess(dw, bw, bound) > 1.0, 'the comparator accepts a planted error: ' + what
            if bb is not None:
                assert excess(db, bb, boundb) > 1.0, 'the comparator accepts a planted error: ' + what
        return dw, db


def run_single(layer, direct=None):
    """One esr_conv3x3_wgrad launch of `layer`: path assertions, launch, check."""
    tx, ty, shape, ns, form = layer.tiling()
    assert shape == layer.shape, 'tile shape %d, expected %d' % (shape, layer.shape)
    assert form == layer.expected_form(), 'form bits %d, expected %d' % (form, layer.expected_form())
    Bl, Hl = (1, layer.B * (layer.H + 2) - 2) if layer.stacked else (layer.B, layer.H)
    tw, th = 32 >> shape, 8 << shape
    assert (tx, ty) == (-(-layer.W // tw), -(-Hl // th))
    if direct is not None:
        assert (ns == 1) == direct, 'nslices %d' % ns
    layer.launch()
    return layer.check(layer.l_bound(tx, ty, ns), tw=(tw, th))


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. the single launch

def _single_cases():
    cs = []
    for fmt in ('split', 'bf16', 'f16'):
        dys = 1000.0 if fmt == 'f16' else 1.0        # fp16 gradients as GradScaler leaves them: max |dY| in [2^9, 2^10)
        for B, H, W in ((1, 1, 1), (1, 2, 3), (1, 8, 32), (2, 8, 32), (3, 9, 31), (2, 17, 23), (1, 40, 37), (2, 64, 9), (5, 3, 70)):
            cs.append(('%s-geom%dx%dx%d' % (fmt, B, H, W), dict(fmt=fmt, B=B, H=H, W=W, dy_scale=dys)))
        for cin in (1, 2, 3, 8, 13, 40, 67, 128, 192):
            cs.append(('%s-cin%d' % (fmt, cin), dict(fmt=fmt, cin=cin, cout=40, H=9, W=31, dy_scale=dys)))
        for cout in (3, 8, 24, 40, 64, 96, 192):
            cs.append(('%s-cout%d' % (fmt, cout), dict(fmt=fmt, cin=40, cout=cout, H=9, W=31)))
        for lat in (1, 2, 3, 4, 8):
            cs.append(('%s-lat%d' % (fmt, lat), dict(fmt=fmt, lat=lat, cin=40, cout=24, H=9, W=31, dy_scale=dys)))
        cs.append(('%s-lat2-cin3' % fmt, dict(fmt=fmt, lat=2, cin=3, cout=8, B=3, H=17, W=23)))
        for ups, (h, w) in ((2, (5, 7)), (3, (3, 11)), (4, (3, 9)), (5, (2, 7)), (6, (2, 6)), (8, (2, 5))):
            cs.append(('%s-ups%d' % (fmt, ups), dict(fmt=fmt, ups=ups, H=h * ups, W=w * ups, cin=13, cout=24)))
        cs.append(('%s-ups2-cin2' % fmt, dict(fmt=fmt, ups=2, H=10, W=70, cin=2, cout=8)))
        for alpha in (0.375, -2.0, 2.0 ** -12):
            cs.append(('%s-alpha%g' % (fmt, alpha), dict(fmt=fmt, alpha=alpha, dy_scale=dys, lat=3, cin=13, cout=24)))
        cs.append(('%s-nodb' % fmt, dict(fmt=fmt, db=False, alpha=0.375)))
        cs.append(('%s-direct' % fmt, dict(fmt=fmt, B=1, H=8, W=32, cin=40, cout=64, lat=2)))
        cs.append(('%s-direct-cin3' % fmt, dict(fmt=fmt, B=1, H=7, W=20, cin=3, cout=40)))
        cs.append(('%s-views' % fmt, dict(fmt=fmt, cin=13, cout=40, x_cg0=2, x_behind=1, dy_cg0=1, dy_behind=2, lat=4)))
        cs.append(('%s-tall' % fmt, dict(fmt=fmt, stacked=True, B=6, H=4, W=4, cin=40, cout=64)))
    return cs


SINGLE = _single_cases()


@pytest.mark.parametrize('kw', [k for _, k in SINGLE], ids=[n for n, _ in SINGLE])
def test_single(kw):
    L = Layer(**kw)
    direct = True if (L.B == 1 and L.H <= 8 and L.W <= 32 and not L.stacked) else None
    run_single(L, direct=direct)


def test_both_slicing_paths_are_reached():
    """The direct += form (one slice) and the workspace + fold form, in every operand format."""
    for fmt in FMTS:
        assert Layer(fmt=fmt, B=1, H=8, W=32, cin=40, cout=64).tiling()[3] == 1
        assert Layer(fmt=fmt, B=2, H=9, W=31).tiling()[3] > 1


S2D_CASES = [
    # (name, layer fields, expected shape)
    ('16x16', dict(cin=128, cout=64, B=2, H=16, W=16, masks=S2D), 1),
    ('8x8', dict(cin=256, cout=64, B=2, H=8, W=8, masks=S2D), 0),
    ('stacked4x4', dict(cin=128, cout=64, B=8, H=4, W=4, masks=S2D, stacked=True), 2),
    ('lat2_defect1', dict(cin=128, cout=64, B=1, H=16, W=16, lat=2, masks=S2D), 0),
    ('lat5_16x16', dict(cin=128, cout=40, B=2, H=16, W=16, lat=5, masks=S2D), 1),
    ('cin96', dict(cin=96, cout=64, B=2, H=16, W=16, masks=S2D), 0),
    ('other_masks', dict(cin=64, cout=32, B=2, H=16, W=16, masks=(1, 2, 4, 8)), 0),
]


@pytest.mark.parametrize('fmt', ['bf16', 'split', 'f16'])
@pytest.mark.parametrize('name,kw,shape', S2D_CASES, ids=[c[0] for c in S2D_CASES])
def test_s2d(fmt, name, kw, shape):
    """Space-to-depth tap masks: the S2D kernel (bf16 formats, cin_main % 128 == 0) with its 16x16 / 32x8 tiles leaves the dW entries outside
    the masks as they were; fp16 operands, cin_main % 128 != 0 and other patterns run the plain kernel, which adds the true gradient there.
    lat2_defect1: a 27-column latent tile in a space-to-depth layer whose map would take the 16x16 tiles keeps the 8x32 tiles (that form
    exists for them only: with the 16x16 plan it covered rows 0-7 of the latent part)."""
    run_single(Layer(fmt=fmt, dy_scale=1000.0 if fmt == 'f16' else 1.0, shape=shape if fmt != 'f16' else 0, **kw))


def test_f16_subnormal_dy():
    """fp16 dY of subnormals only (k * 2^-24, k in 1..1023, both signs): the fp16 MFMA multiplies them as they are (no flush to zero), so the
    one-plane bound with c_fmt = 0 holds; a flushed dY would leave dW at d0."""
    g = torch.Generator().manual_seed(5)
    k = torch.randint(1, 1024, (2, 24, 9, 31), generator=g).double() * (torch.randint(0, 2, (2, 24, 9, 31), generator=g) * 2 - 1)
    L = Layer(fmt='f16', B=2, H=9, W=31, cin=13, cout=24, dy_values=k * 2.0 ** -24, alpha=1.0)
    dw, _ = run_single(L)
    assert float((dw - L.d0w.double().view(dw.shape).to(DEV)).abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. the batch forms

def _set(fmt, s2d=False):
    dys = 1000.0 if fmt == 'f16' else 1.0
    kws = [dict(B=2, H=9, W=31, cin=13, cout=24, dy_scale=dys), dict(lat=2, cin=40, cout=40, H=12, W=20),
           dict(lat=8, cin=16, cout=8, B=1, H=17, W=23), dict(ups=2, H=10, W=14, cin=24, cout=40), dict(cin=3, cout=64, H=16, W=16),
           dict(cin=67, cout=96, B=3, H=8, W=8), dict(cin=40, cout=24, x_cg0=1, x_behind=1, dy_cg0=2, H=5, W=37, alpha=-2.0),
           dict(cin=8, cout=3, B=1, H=1, W=1, db=False)]
    if s2d:        # a space-to-depth layer and a plain one on the same 16x16 map (the latter takes the 16x16 tiles only in such a set)
        kws[4:4] = [dict(cin=128, cout=64, B=2, H=16, W=16, masks=S2D), dict(cin=40, cout=64, B=2, H=16, W=16, lat=5)]
    return [Layer(fmt=fmt, seed=i, **kw) for i, kw in enumerate(kws)]


def _arr(layers):
    L = _lib()
    return (L.WgradDesc * len(layers))(*[l.desc() for l in layers])


def _snap(layers):
    torch.cuda.synchronize()
    out = [l.buf.clone() for l in layers]
    for l in layers:
        l.reset()
    return out


def _run_batch(layers):
    lib = _lib().load_library()
    arr = _arr(layers)
    need = lib.esr_conv3x3_wgrad_batch_workspace_bytes(arr, len(layers))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert lib.esr_conv3x3_wgrad_batch(arr, len(layers), ws.data_ptr(), need, _stream()) == 0


def _upload(layers, unit=0):
    L = _lib()
    lib = L.load_library()
    arr = _arr(layers)
    n = len(layers)
    need = lib.esr_conv3x3_wgrad_batch_part_workspace_bytes(arr, n, unit) if unit else lib.esr_conv3x3_wgrad_batch_workspace_bytes(arr, n)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    plan = L.WgradBatchPlan()
    if unit:
        assert lib.esr_conv3x3_wgrad_batch_part_upload(arr, n, ws.data_ptr(), need, C.byref(plan), unit, _stream()) == 0
    else:
        assert lib.esr_conv3x3_wgrad_batch_upload(arr, n, ws.data_ptr(), need, C.byref(plan), _stream()) == 0
    return ws, plan


def _bits_equal(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), '%s: layer %d differs from the one launch' % (what, i)


@pytest.mark.parametrize('fmt', list(FMTS))
def test_batch(fmt):
    """A heterogeneous set in one launch, every layer element-wise against float64; _upload + _run, 2-3 contiguous parts with the whole set's
    _unit, and _run_side (one-plane sets) bit-identical to it."""
    lib = _lib().load_library()
    layers = _set(fmt)
    _run_batch(layers)
    torch.cuda.synchronize()
    for l in layers:
        l.check(l.l_bound(), teeth=(l is layers[0]))
    one = _snap(layers)
    ws, plan = _upload(layers)
    assert lib.esr_conv3x3_wgrad_batch_run(ws.data_ptr(), C.byref(plan), _stream()) == 0
    _bits_equal(one, _snap(layers), '_upload + _run')
    unit = lib.esr_conv3x3_wgrad_batch_unit(_arr(layers), len(layers))
    assert unit > 0
    for cuts in ((3,), (1, 5), (2, 6)):
        bounds = [0] + list(cuts) + [len(layers)]
        keep = []
        for p0, p1 in zip(bounds, bounds[1:]):
            ws_p, plan_p = _upload(layers[p0:p1], unit)
            keep.append(ws_p)
            assert lib.esr_conv3x3_wgrad_batch_run(ws_p.data_ptr(), C.byref(plan_p), _stream()) == 0
        _bits_equal(one, _snap(layers), 'parts %s' % (cuts,))
    if FMTS[fmt].planes == 1:
        # (the results are those of _run whatever the occupancy; esr_conv3x3_wgrad_side_occupancy only says whether the form helps)
        assert lib.esr_conv3x3_wgrad_side_occupancy(1 if fmt == 'f16' else 0) >= 1
        ws, plan = _upload(layers)
        assert lib.esr_conv3x3_wgrad_batch_run_side(ws.data_ptr(), C.byref(plan), _stream()) == 0
        _bits_equal(one, _snap(layers), '_run_side')


@pytest.mark.parametrize('fmt', ['bf16', 'split'])
def test_batch_parts_with_s2d(fmt):
    """A set with a space-to-depth layer runs the 16x16 / 32x8 tiles for all its layers; a part that does not hold that layer must tile and
    slice its layers as the one launch does (the unit carries the decision), so every split — one isolating the s2d layer — is bit-identical."""
    lib = _lib().load_library()
    layers = _set(fmt, s2d=True)
    _run_batch(layers)
    torch.cuda.synchronize()
    for l in layers:
        l.check(l.l_bound(), teeth=(l.masks is not None))
    one = _snap(layers)
    unit = lib.esr_conv3x3_wgrad_batch_unit(_arr(layers), len(layers))
    s = next(i for i, l in enumerate(layers) if l.masks)
    for cuts in ((s, s + 1), (s + 1,), (s,), (2, 7)):
        bounds = [0] + list(cuts) + [len(layers)]
        keep = []
        for p0, p1 in zip(bounds, bounds[1:]):
            ws_p, plan_p = _upload(layers[p0:p1], unit)
            keep.append(ws_p)
            assert lib.esr_conv3x3_wgrad_batch_run(ws_p.data_ptr(), C.byref(plan_p), _stream()) == 0
        _bits_equal(one, _snap(layers), 'parts %s' % (cuts,))


def test_batch_rebase():
    """A table uploaded against flat buffer A and rebased to B: the results land in B (A keeps every bit, guards included); running the table
    twice accumulates twice."""
    lib = _lib().load_library()
    proto = _set('bf16')
    sizes = [(l.nw, l.cout) for l in proto]
    n = NG + sum(a + b + 2 * NG for a, b in sizes)
    A = torch.full((n,), GUARD32, dtype=torch.int32, device=DEV)
    Bf = torch.zeros(n, dtype=torch.int32, device=DEV)
    layers, off = [], NG
    for i, (l, (nw, co)) in enumerate(zip(proto, sizes)):
        kw = dict(B=l.B, H=l.H, W=l.W, cin=l.cin, cout=l.cout, lat=l.lat, ups=l.ups, alpha=l.alpha, db=l.has_db)
        layers.append(Layer(fmt='bf16', seed=i, out=(A, off, off + nw + NG), **kw))
        off += nw + co + 2 * NG
    A_bits = A.clone()
    ws, plan = _upload(layers)
    assert lib.esr_conv3x3_wgrad_batch_rebase(ws.data_ptr(), C.byref(plan), Bf.data_ptr() - A.data_ptr(), _stream()) == 0
    assert lib.esr_conv3x3_wgrad_batch_run(ws.data_ptr(), C.byref(plan), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(A, A_bits), 'the rebased table wrote into the old buffer'
    r1 = Bf.clone()
    mine = torch.zeros(n, dtype=torch.bool)
    for l in layers:
        mine[l.woff:l.woff + l.nw] = True
        if l.has_db:
            mine[l.boff:l.boff + l.cout] = True
    assert (r1.cpu()[~mine] == 0).all(), 'written outside the layers\' dW / db in the new buffer'
    for l in layers:          # the results in B, against float64 with d0 = 0
        l.buf, l.init, l.d0w, l.d0b = r1, r1.clone(), torch.zeros_like(l.d0w), torch.zeros_like(l.d0b)
        l.check(l.l_bound(), teeth=False)
    assert lib.esr_conv3x3_wgrad_batch_run(ws.data_ptr(), C.byref(plan), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(A, A_bits)
    f1, f2 = r1.view(torch.float32), Bf.view(torch.float32)
    assert torch.equal(f2, 2 * f1), 'the second run did not add the same gradient again'
    assert float(f1.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals that need real views (the host-only ones are in tests/test_host_api.py)

def test_narrow_views_refused():
    """Views narrower than the channels named: ESR_E_ARG — never a silent zero gradient (the kernel reads a missing group as zeros)."""
    lib = _lib().load_library()
    L = Layer(fmt='bf16', cin=40, cout=40, lat=5)
    for field, ncg in (('x', 4), ('dy', 4), ('xlat', 0)):
        d = L.desc()
        getattr(d, field).ncg = ncg
        ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)
        d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()
        assert lib.esr_conv3x3_wgrad(C.byref(d), _stream()) == E_ARG, field
        t = (C.c_int32 * 5)()
        assert lib.esr_conv3x3_wgrad_tiling(C.byref(d), t) == E_ARG, field
    torch.cuda.synchronize()
    assert torch.equal(L.buf, L.init)
