"""The backward helpers of csrc/esr_bwd.hip (include/esr_hip.h) against float64 restatements: esr_act_combine, esr_pixel_unshuffle,
esr_unpack_grad_nchw, esr_grad_absmax / esr_grad_scale.  Buffers are laid out here ([planes][B][CG][H+2][W+2][8]); inputs hold NaN wherever
the launch must not read (borders, groups past the destination's), destinations a NaN sentinel wherever it must not write.

Bounds (u = 2^-24; the reference reads the stored planes back and sums hi + lo in float64):
    act_combine     out = alpha*A + beta*sum_{s x s} Bv, times mask_slope where the mask's stored hi is not > 0: one multiply and s^2 fused
                    multiply-adds in fp32, then the mask multiply -> (s^2 + 2) u S with S = |alpha A| + |beta| sum |Bv|; then the store,
                    c_out |ref|: bf16 2^-8, split (hi + bf16 residue) 2^-15, f16 2^-10, f16 hi+lo 2^-21 plus 2^-25 absolute (a subnormal lo).
    unpack_grad     a sum of at most 4 (pad+1)^2 weighted terms, weights exact in fp32 (0.5, or 1 for odd factors): 4 ((pad+1)^2 + 1) u S,
                    S the same adjoint of |G|; accumulate adds one more rounding.
    pixel_unshuffle, grad_absmax, grad_scale: bit-exact.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0x7FA5                   # NaN as bf16 and as fp16
U = 2.0 ** -24
OUT_FMTS = {  # name: (dtype, planes, c_out, absolute)
    'bf16': (torch.bfloat16, 1, 2.0 ** -8, 0.0), 'split': (torch.bfloat16, 2, 2.0 ** -15, 0.0),
    'f16': (torch.float16, 1, 2.0 ** -10, 0.0), 'f16x2': (torch.float16, 2, 2.0 ** -21, 2.0 ** -25)}


def _L():
    from esr_hip import _lib
    return _lib


def _stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """int16 [planes][B][CG][H+2][W+2][8] of one dtype.  random: interior uniform(-scale, scale) (hi + residue), border NaN; else NaN."""

    def __init__(self, dtype, planes, B, CG, H, W, random=False, seed=0, scale=1.0, border=SENT, values=None):
        self.dtype, self.P, self.B, self.CG, self.H, self.W = dtype, planes, B, CG, H, W
        t = torch.full((planes, B, CG, H + 2, W + 2, 8), SENT, dtype=torch.int16)
        if random or values is not None:
            if values is None:
                g = torch.Generator().manual_seed(seed)
                values = (torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1) * scale
            hi = values.to(dtype)
            t[0, :, :, 1:-1, 1:-1] = hi.view(torch.int16)
            if planes == 2:
                t[1, :, :, 1:-1, 1:-1] = (values - hi.double()).to(dtype).view(torch.int16)
            t[:, :, :, 0] = border
            t[:, :, :, -1] = border
            t[:, :, :, :, 0] = border
            t[:, :, :, :, -1] = border
        self.t = t.to(DEV)

    def view(self, cg0=0, ncg=None, lo=True):
        L = _L()
        P, B, CG, Hp, Wp, _ = self.t.shape
        cs = Hp * Wp
        hi = self.t.data_ptr() + cg0 * cs * 16
        return L.ActView(hi, hi + self.t.stride(0) * 2 if (P == 2 and lo) else None, CG - cg0 if ncg is None else ncg, Hp - 2, Wp - 2, CG * cs, cs,
                         1 if self.dtype == torch.float16 else 0)

    def values(self, cg0=0, ncg=None, lo=True):
        """float64 [B][8*ncg][H][W] (interior) of hi (+ lo)."""
        t = self.t.cpu()
        ncg = self.CG - cg0 if ncg is None else ncg
        v = t[0].view(self.dtype).double()
        if self.P == 2 and lo:
            v = v + t[1].view(self.dtype).double()
        v = v[:, cg0:cg0 + ncg, 1:-1, 1:-1].permute(0, 1, 4, 2, 3)
        return v.reshape(self.B, ncg * 8, self.H, self.W)


def _excess(y, ref, bound):
    err = (y - ref).abs()
    e = err / bound
    e[err == 0] = 0.0
    e[torch.isnan(err)] = float('inf')
    return float(e.max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# esr_act_combine

COMBINE = [
    # (name, A?, Bv?, mask (dtype, slope) or None, s, out fmt, in place)
    ('A', True, False, None, 1, 'split', False), ('Bv_s2', False, True, None, 2, 'bf16', False),
    ('A_Bv_s1', True, True, None, 1, 'f16x2', False), ('A_Bv_s3_mask', True, True, (torch.float16, 0.2), 3, 'split', False),
    ('Bv_s4_mask_relu', False, True, (torch.bfloat16, 0.0), 4, 'f16', False), ('mask_only', False, False, (torch.bfloat16, 0.2), 1, 'bf16', False),
    ('A_mask_inplace', True, False, (torch.bfloat16, 0.0), 1, 'bf16', True), ('A_Bv_inplace', True, True, None, 1, 'split', True),
    ('A_Bv_s2_mask_f16', True, True, (torch.float16, 0.2), 2, 'f16', False),
]


@pytest.mark.parametrize('name,hasA,hasB,mask,s,ofmt,inplace', COMBINE, ids=[c[0] for c in COMBINE])
def test_act_combine(name, hasA, hasB, mask, s, ofmt, inplace):
    lib = _L().load_library()
    dtype, P, c_out, absolute = OUT_FMTS[ofmt]
    B, H, W, ng = 2, 5, 7, 2
    alpha, beta = 0.75, -1.5
    out = Buf(dtype, P, B, ng + 2, H, W)                       # destination: groups [1, 1 + ng), the rest must keep the sentinel
    if inplace:
        out = Buf(dtype, P, B, ng + 2, H, W, random=True, seed=1)
        out.t[:, :, 0] = SENT
        out.t[:, :, ng + 1:] = SENT
    A = out if inplace else (Buf(dtype, P, B, ng + 2, H, W, random=True, seed=1) if hasA else None)
    if A is not None and not inplace:
        A.t[:, :, ng + 1:, 1:-1, 1:-1] = SENT                     # the view is wider than out: its last group is never read
    Bv = Buf(torch.float16 if ofmt.startswith('f16') else torch.bfloat16, 2, B, ng + 1, H * s, W * s, random=True, seed=2) if hasB else None
    if Bv is not None:
        Bv.t[:, :, ng:, 1:-1, 1:-1] = SENT
    M = None
    if mask is not None:
        mdt, slope = mask
        g = torch.Generator().manual_seed(3)
        mv = (torch.rand(B, ng + 1, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1)
        M = Buf(mdt, 1, B, ng + 1, H, W, values=mv)
        bits = M.t[0, :, :, 1:-1, 1:-1].reshape(-1)
        special = torch.tensor([0x0000, 0x8000 - 65536, 0x0001, 0x8001 - 65536], dtype=torch.int16, device=DEV)     # +0, -0, tiny, -tiny
        bits[:4 * 16].view(16, 4)[:] = special
        M.t[0, :, :, 1:-1, 1:-1] = bits.view(B, ng + 1, H, W, 8)
    else:
        slope = 1.0
    Av0 = A.values(1, ng) if A is not None else None
    ov = out.view(1, ng)
    av = (A.view(1, ng) if inplace else A.view(1, ng + 1)) if A is not None else None
    bv = Bv.view(0, ng + 1) if Bv is not None else None
    mv_ = M.view(0, ng + 1) if M is not None else None
    import ctypes as C
    ref_ = lambda v: C.byref(v) if v is not None else None
    before = out.t.cpu()
    assert lib.esr_act_combine(ref_(av), alpha, ref_(bv), beta, s, ref_(mv_), slope, C.byref(ov), B, _stream()) == 0
    torch.cuda.synchronize()
    after = out.t.cpu()
    written = torch.zeros(after.shape[1:], dtype=torch.bool)
    written[:, 1:1 + ng, 1:-1, 1:-1] = True
    assert torch.equal(after[:, ~written], before[:, ~written]), 'written outside the interior of the destination groups'

    def reference(shift_b=0, shift_m=0, no_alpha=False):
        v = torch.zeros(B, 8 * ng, H, W, dtype=torch.float64)
        S = torch.zeros_like(v)
        if A is not None:
            a = 1.0 if no_alpha else alpha
            v, S = v + a * Av0, S + abs(a) * Av0.abs()
        if Bv is not None:
            bvals = Bv.values(0, ng).roll(shift_b, 3).view(B, 8 * ng, H, s, W, s)
            v, S = v + beta * bvals.sum((3, 5)), S + abs(beta) * bvals.abs().sum((3, 5))
        if M is not None:
            hb = M.t.cpu()[0, :, 0:ng, 1:-1, 1:-1].permute(0, 1, 4, 2, 3).reshape(B, 8 * ng, H, W).roll(shift_m, 3)
            v = torch.where(hb > 0, v, slope * v)
        return v, S

    ref, S = reference()
    y = out.values(1, ng)
    bound = (s * s + 2) * U * S + c_out * ref.abs() + absolute
    e = _excess(y, ref, bound)
    assert e <= 1.0, 'worst |out-ref|/bound = %.3g' % e
    planted = []
    if Bv is not None:
        planted.append(('Bv window one pixel over', reference(shift_b=1)[0]))
    if M is not None and slope != 1.0 and float(ref.abs().max()) > 0:     # (mask alone: out = 0 whatever the mask)
        planted.append(('mask one pixel over', reference(shift_m=1)[0]))
    if A is None and Bv is None:
        assert float(y.abs().max()) == 0
    if A is not None:
        planted.append(('alpha missing', reference(no_alpha=True)[0]))
    for what, bad in planted:
        assert _excess(y, bad, bound) > 1.0, 'the comparator accepts a planted error: ' + what


# ---------------------------------------------------------------------------------------------------------------------------------------
# esr_pixel_unshuffle

@pytest.mark.parametrize('r,dtype,sp,dp', [(2, torch.bfloat16, 2, 2), (3, torch.float16, 1, 2), (4, torch.bfloat16, 1, 1), (2, torch.float16, 2, 1)])
def test_pixel_unshuffle(r, dtype, sp, dp):
    """An exact bit permutation dst[g*r^2 + s][y][x] = src[g][r*y + s/r][r*x + s%r]; dst's lo plane zeroed when src has none."""
    import ctypes as C
    lib = _L().load_library()
    B, G, H, W = 2, 2, 3, 5
    src = Buf(dtype, sp, B, G, r * H, r * W, random=True, seed=r)
    dst = Buf(dtype, dp, B, G * r * r + 2, H, W)
    before = dst.t.cpu()
    assert lib.esr_pixel_unshuffle(C.byref(src.view()), r, C.byref(dst.view(1, G * r * r)), B, _stream()) == 0
    torch.cuda.synchronize()
    after = dst.t.cpu()
    s = src.t.cpu()[:, :, :, 1:-1, 1:-1].reshape(sp, B, G, H, r, W, r, 8).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(sp, B, G * r * r, H, W, 8)
    got = after[:, :, 1:1 + G * r * r, 1:-1, 1:-1]
    assert torch.equal(got[0], s[0]), 'hi plane is not the permutation'
    if dp == 2:
        assert torch.equal(got[1], s[1] if sp == 2 else torch.zeros_like(got[1])), 'lo plane'
    written = torch.zeros(after.shape[1:], dtype=torch.bool)
    written[:, 1:1 + G * r * r, 1:-1, 1:-1] = True
    assert torch.equal(after[:, ~written], before[:, ~written]), 'written outside the destination interior'
    bad = s[0].clone()
    bad[:, :G] = s[0][:, G:2 * G]
    assert not torch.equal(got[0], bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# esr_unpack_grad_nchw

UNPACK = [
    # (down, pad, h, w, C, c0, nc, accumulate, batch stride extra, G dtype, planes)
    (1, 0, 5, 7, 4, 0, 4, False, 0, torch.bfloat16, 2), (1, 2, 6, 9, 11, 2, 5, True, 0, torch.bfloat16, 1),
    (2, 1, 8, 10, 3, 0, 3, False, 37, torch.bfloat16, 2), (3, 0, 9, 12, 9, 1, 8, True, 0, torch.float16, 1),
    (3, 1, 7, 10, 5, 3, 2, False, 0, torch.bfloat16, 2), (4, 2, 12, 8, 3, 0, 3, True, 100, torch.bfloat16, 2),
    (4, 4, 8, 12, 10, 1, 9, False, 0, torch.float16, 2), (8, 0, 16, 24, 2, 0, 2, True, 0, torch.bfloat16, 2),
    (2, 2, 6, 4, 12, 3, 9, False, 0, torch.bfloat16, 1),
]


@pytest.mark.parametrize('down,pad,h,w,Cc,c0,nc,acc,extra,dtype,planes', UNPACK, ids=['d%d-p%d-%dx%d-c%d+%d' % (u[0], u[1], u[2], u[3], u[5], u[6])
                                                                                      for u in UNPACK])
def test_unpack_grad_nchw(down, pad, h, w, Cc, c0, nc, acc, extra, dtype, planes):
    """The adjoint of replicate padding + bilinear /down: float64 autograd of F.interpolate(F.pad(x, replicate), scale_factor=1/down,
    'bilinear', align_corners=False); channels outside [c0, c0 + nc) and the batch-stride gap keep their bits."""
    import ctypes as C
    lib = _L().load_library()
    B = 2
    Hd, Wd = (h + 2 * pad) // down, (w + 2 * pad) // down
    ng = (nc + 7) // 8
    G = Buf(dtype, planes, B, ng, Hd, Wd, random=True, seed=down + pad)
    if nc % 8:
        G.t[:, :, ng - 1, 1:-1, 1:-1, nc % 8:] = SENT              # pad lanes: never stored
    stride = Cc * h * w + extra
    g = torch.Generator().manual_seed(7)
    d0 = (torch.rand(B * stride, generator=g, dtype=torch.float64) * 2 - 1).float()
    dst = d0.clone().to(DEV)
    assert lib.esr_unpack_grad_nchw(C.byref(G.view()), dst.data_ptr(), stride if extra else 0, B, Cc, h, w, c0, nc, pad, down, 1 if acc else 0,
                                    _stream()) == 0
    torch.cuda.synchronize()
    got = dst.cpu()
    Gv = G.values()[:, :nc]

    def adjoint(Gm):
        x = torch.zeros(B, nc, h, w, dtype=torch.float64, requires_grad=True)
        y = F.pad(x, (pad,) * 4, mode='replicate') if pad else x
        if down > 1:
            y = F.interpolate(y, scale_factor=1.0 / down, mode='bilinear', align_corners=False)
        (y * Gm).sum().backward()
        return x.grad

    ref_core, S = adjoint(Gv), adjoint(Gv.abs())
    mine = torch.zeros(B, stride, dtype=torch.bool)
    mine[:, :Cc * h * w].view(B, Cc, h, w)[:, c0:c0 + nc] = True
    assert torch.equal(got.view(B, stride)[~mine], d0.view(B, stride)[~mine]), 'written outside channels [c0, c0 + nc)'
    y = got.view(B, stride)[:, :Cc * h * w].view(B, Cc, h, w)[:, c0:c0 + nc].double()
    base = d0.view(B, stride)[:, :Cc * h * w].view(B, Cc, h, w)[:, c0:c0 + nc].double()
    ref = ref_core + (base if acc else 0)
    bound = 4 * ((pad + 1) ** 2 + 1) * U * (S + (base.abs() if acc else 0))
    e = _excess(y, ref, bound)
    assert e <= 1.0, 'worst |dst-ref|/bound = %.3g' % e
    bad = ref.clone()
    bad[:, :, 0, 0] = (ref_core + (base if acc else 0))[:, :, 0, 1]           # the pad ring folded onto the wrong edge pixel
    if not torch.equal(bad, ref):
        assert _excess(y, bad, bound) > 1.0
    if not acc:
        assert _excess(y, ref + base, bound) > 1.0, 'accumulate off: the old contents must not be added'


# ---------------------------------------------------------------------------------------------------------------------------------------
# esr_grad_absmax / esr_grad_scale

def _f16_buf(B, CG, H, W, planes, hi_vals, lo_vals=None):
    t = torch.zeros(planes, B, CG, H + 2, W + 2, 8, dtype=torch.int16)
    t[0, :, :, 1:-1, 1:-1] = hi_vals.half().view(torch.int16)
    if planes == 2 and lo_vals is not None:
        t[1, :, :, 1:-1, 1:-1] = lo_vals.half().view(torch.int16)
    b = Buf(torch.float16, planes, B, CG, H, W)
    b.t = t.to(DEV)
    return b


def _k_for(m, exp):
    """k with m * 2^k in [2^(exp-1), 2^exp)."""
    _, e = math.frexp(m)          # m = f * 2^e, f in [0.5, 1)
    return exp - e


MAXIMA = [2.0 ** -24, 2.0 ** -20, 3 * 2.0 ** -17, 2.0 ** -14 * (1 - 2.0 ** -10), 0.7, 1.0, 1.999, 512.0, 1023.5, 16384.0, 32752.0, 65504.0]


@pytest.mark.parametrize('exp', [1, 10, 15])
def test_grad_absmax_and_scale(exp):
    """slot = the max |hi| bit pattern (lo ignored); f = 2^k with max * f in [2^(exp-1), 2^exp); planes bit-equal to (h.float() * f).half() (lo
    underflow included); scale_out = scale_in * f.  Maxima: subnormal, the subnormal / normal edge, 2^(exp-1) and just below 2^exp."""
    import ctypes as C
    lib = _L().load_library()
    B, CG, H, W = 2, 3, 4, 5
    maxima = MAXIMA + [2.0 ** (exp - 1), 2.0 ** exp * (1 - 2.0 ** -11)]
    for i, m in enumerate(maxima):
        g = torch.Generator().manual_seed(i)
        hv = (torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1) * m
        hv[1, 2, 3, 4, 7] = -m if i % 2 else m
        lv = (torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1) * 60000.0     # lo: ignored by the max
        src = _f16_buf(B, CG, H, W, 2, hv, lv)
        assert float(src.t.cpu()[0].view(torch.float16).abs().max()) == float(torch.tensor(m, dtype=torch.float64).half())
        slot = torch.zeros(1, dtype=torch.int32, device=DEV)
        sc = torch.tensor([0.375, -1.0], dtype=torch.float32, device=DEV)
        assert lib.esr_grad_absmax(C.byref(src.view()), B, slot.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        mb = int(torch.tensor(m, dtype=torch.float64).half().view(torch.int16).item()) & 0x7FFF
        assert int(slot.item()) == mb, (m, int(slot.item()), mb)
        k = _k_for(float(torch.tensor(m, dtype=torch.float64).half()), exp)
        f = 2.0 ** k
        assert 2.0 ** (exp - 1) <= float(torch.tensor(m, dtype=torch.float64).half()) * f < 2.0 ** exp
        before = src.t.cpu()
        assert lib.esr_grad_scale(C.byref(src.view()), C.byref(src.view()), B, slot.data_ptr(), exp, sc.data_ptr(), None, sc.data_ptr() + 4,
                                  _stream()) == 0
        torch.cuda.synchronize()
        after = src.t.cpu()
        for p in range(2):
            want = (before[p].view(torch.float16).float() * f).half().view(torch.int16)
            assert torch.equal(after[p], want), ('plane', p, m, k)
        assert float(sc[1].item()) == 0.375 * f


def test_grad_absmax_zero_view_and_explicit_factor():
    """An all-zero hi plane leaves the slot at 0 and scales by 1; slot == NULL scales by scale_in / scale_den (fp32); src != dst with
    dst.ncg < src.ncg writes dst's groups only."""
    import ctypes as C
    lib = _L().load_library()
    B, CG, H, W = 2, 3, 4, 5
    g = torch.Generator().manual_seed(11)
    z = _f16_buf(B, CG, H, W, 2, torch.zeros(B, CG, H, W, 8, dtype=torch.float64), torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64))
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    sc = torch.tensor([2.0, -1.0], dtype=torch.float32, device=DEV)
    assert lib.esr_grad_absmax(C.byref(z.view()), B, slot.data_ptr(), _stream()) == 0
    before = z.t.cpu()
    assert lib.esr_grad_scale(C.byref(z.view()), C.byref(z.view()), B, slot.data_ptr(), 10, sc.data_ptr(), None, sc.data_ptr() + 4, _stream()) == 0
    torch.cuda.synchronize()
    assert int(slot.item()) == 0 and float(sc[1].item()) == 2.0 and torch.equal(z.t.cpu(), before)
    hv = (torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1) * 3000.0
    lv = (torch.rand(B, CG, H, W, 8, generator=g, dtype=torch.float64) * 2 - 1) * 2.0 ** -14
    src = _f16_buf(B, CG, H, W, 2, hv, lv)
    dst = Buf(torch.float16, 2, B, CG, H, W)                       # sentinel; the view covers 2 of its 3 groups
    num = torch.tensor([1.0], dtype=torch.float32, device=DEV)
    den = torch.tensor([3.0], dtype=torch.float32, device=DEV)
    dv = dst.view(0, 2)
    assert lib.esr_grad_scale(C.byref(src.view()), C.byref(dv), B, None, 0, num.data_ptr(), den.data_ptr(), None, _stream()) == 0
    torch.cuda.synchronize()
    f = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(3.0, dtype=torch.float32))
    s, d = src.t.cpu(), dst.t.cpu()
    for p in range(2):
        want = (s[p][:, :2].view(torch.float16).float() * f).half().view(torch.int16)
        assert torch.equal(d[p][:, :2], want), p
    assert (d[:, :, 2] == SENT).all(), 'a group past dst.ncg was written'
