"""The esr_conv3x3 descriptor contract (include/esr_hip.h), option by option, against a float64 restatement of

    out = alpha * act(conv(in0 ++ in1) + bias) + beta1*res1 + beta2*res2      (then the mask, then the store)

written here.  Launches go through esr_hip.act.conv3x3 on buffers this file lays out itself ([planes][B][CG][H+2][W+2][8] 16-bit, read
with view_of / tall_view), so that every option of the descriptor can be set.

Reference inputs are the STORED values: the planes are read back with torch as bfloat16 / float16 and summed (hi + lo) in float64, so the
reference multiplies exactly what the kernel multiplied; weights and bias are the fp32 tensors the packs were made from.

Element-wise bound, for every output element:

    |y - ref| <= c_w * S + c_out * |ref| + K * 2^-24 * S
    S = alpha * conv(|x|, |w|) + |bias| + |beta1 res1| + |beta2 res2|,   K = 9 * input channels (8 per group)

c_w is the weight rounding of the format, c_out the rounding of the destination, K * 2^-24 the fp32 accumulation.  Derivation (u = unit
roundoff, round to nearest even):
    bf16   one bf16 weight plane, u = 2^-9                                    -> c_w = 2^-8
    split  hi+lo bf16 weights: residue 2^-18, dropped Wlo*Xlo term 2^-18      -> c_w = 2^-16
    f16    one fp16 weight plane (also f16x2), u = 2^-11                      -> c_w = 2^-10
    f16x3  hi+lo fp16 weights: residue 2^-22, dropped Wlo*Xlo 2^-22; the lo planes of small weights are fp16 subnormals (absolute
           rounding 2^-25), so one more factor of 2                           -> c_w = 2^-20
    destinations: bf16 hi 2^-9 -> 2^-8; bf16 hi+lo 2^-18 -> 2^-17; fp16 hi 2^-11 -> 2^-10; fp16 hi+lo 2^-22 (+ subnormal lo) -> 2^-20;
    fp32 NCHW 2^-24 -> 2^-23.
A LeakyReLU whose pre-activation lies within rounding of zero may take the other branch; the difference is below |pre| and so below the
bound: no activation pattern is forced.

Every family also checks that its comparator rejects a planted error (a dropped corner tap, a residual read from the neighbouring group,
a mask window shifted by one group), and that nothing outside the launch's destination changed: borders, groups outside
[0, ceil(cout/8)), the lo plane of a hi-only out2, the guard elements around out_nchw and the pixel-shuffle groups of other row groups
keep a NaN sentinel bit for bit.

Which test reaches which epilogue of ConvEpis (esr_conv.hip) and which operand form of conv_kernel_exists:
    plain        test_epilogues[<fmt>-plain], test_epilogues[<fmt>-plain_relu_nobias], test_geometry[plain-*], test_four_stage_ring
    RES1         test_epilogues[<fmt>-res1], test_resin_near_misses, test_partial_lo, test_cout
    RES1|RES2    test_epilogues[<fmt>-res12], test_formats, test_geometry[heavy-*], test_slices
    RESIN        test_epilogues[<fmt>-resin], test_resin_with_latent, test_two_slice_form
    RESIN|RES2   test_epilogues[<fmt>-resin_res2]
    NCHW         test_epilogues[<fmt>-nchw], test_four_stage_ring
    OUT2         test_epilogues[<fmt>-out2], test_epilogues[<fmt>-out2_hi]
    MASK         test_epilogues[<fmt>-mask], test_epilogues[<fmt>-mask_relu], test_slices, test_two_slice_form
    RES1|MASK    test_epilogues[bf16|split-res1_mask*], test_geometry[heavy-*] (bf16 formats only: test_refusals)
    PS           test_pixel_shuffle
    formats      bf16 / split / f16 / f16x2 (weight_planes 1) / f16x3 (weight_planes 2) in test_epilogues and test_formats; partial lo
                 (in1_lo_groups > 0, < 0, out.lo == NULL) in test_partial_lo
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_UNSUPPORTED = -1, -2
SENT = 0x7FA5          # a NaN both as bf16 and as fp16: what every byte a launch must not write holds before and after it
SENT32 = 0x7FC0DEAD    # the same for the fp32 guard elements around out_nchw


class Fmt:
    def __init__(self, name, planes, vfmt, dtype, c_w, c_out_hilo, c_out_hi, split):
        self.name, self.planes, self.vfmt, self.dtype, self.c_w, self.c_out_hilo, self.c_out_hi, self.split = \
            name, planes, vfmt, dtype, c_w, c_out_hilo, c_out_hi, split


FMTS = {f.name: f for f in (
    Fmt('bf16', 1, 0, torch.bfloat16, 2.0 ** -8, None, 2.0 ** -8, False),
    Fmt('split', 2, 0, torch.bfloat16, 2.0 ** -16, 2.0 ** -17, 2.0 ** -8, True),
    Fmt('f16', 1, 1, torch.float16, 2.0 ** -10, None, 2.0 ** -10, 'f16'),
    Fmt('f16x2', 2, 1, torch.float16, 2.0 ** -10, 2.0 ** -20, 2.0 ** -10, 'f16x2'),
    Fmt('f16x3', 2, 1, torch.float16, 2.0 ** -20, 2.0 ** -20, 2.0 ** -10, 'f16x3'),
)}
C_NCHW = 2.0 ** -23


def _A():
    from esr_hip import act as A
    return A


# ---------------------------------------------------------------------------------------------------------------------------------------
# activation buffers

class Buf:
    """[planes][B][CG][H+2][W+2][8] int16 storage of one element format (stacked=True: [planes][CG][B][H+2][W+2][8], see act.stacked_at)."""

    def __init__(self, fmt, B, ncg, H, W, planes=None, stacked=False, fill=None, seed=0, scale=1.0):
        self.f = FMTS[fmt] if isinstance(fmt, str) else fmt
        self.P = planes or self.f.planes
        self.B, self.ncg, self.H, self.W, self.stacked = B, ncg, H, W, stacked
        shape = (self.P, ncg, B, H + 2, W + 2, 8) if stacked else (self.P, B, ncg, H + 2, W + 2, 8)
        t = torch.zeros(shape, dtype=torch.int16)
        if fill == 'sentinel':
            t.fill_(SENT)
        elif fill == 'random':
            g = torch.Generator().manual_seed(seed)
            x = (torch.rand(shape[1:3] + (H, W, 8), generator=g, dtype=torch.float64) * 2 - 1).float() * scale
            hi = x.to(self.f.dtype)
            t[0, :, :, 1:-1, 1:-1] = hi.view(torch.int16)
            if self.P == 2:
                t[1, :, :, 1:-1, 1:-1] = (x - hi.float()).to(self.f.dtype).view(torch.int16)
        self.t = t.to(DEV)
        if stacked:
            self.t._esr_stacked = True

    def view(self, cg0=0, ncg=None, lo=True):
        v = _A().view_of(self.t, cg0, ncg)
        v.fmt = self.f.vfmt
        if not lo:
            v.lo = None
        return v

    def tall(self, cg0=0):
        v, rows = _A().tall_view(self.t)
        cs = v.cg_stride * 16
        v.hi += cg0 * cs
        if v.lo:
            v.lo += cg0 * cs
        v.ncg -= cg0
        v.fmt = self.f.vfmt
        return v, rows

    def bits(self):
        return self.t.cpu()

    def values(self, cg0=0, ncg=None, lo=True, tall=False, t=None):
        """float64 [B][8*ncg][H+2][W+2] of hi (+ lo) (tall: the stacked images as one image, [1][8*ncg][B*(H+2)][W+2])."""
        t = self.bits() if t is None else t
        ncg = self.ncg - cg0 if ncg is None else ncg
        v = t[0].view(self.f.dtype).double()
        if lo and self.P == 2:
            v = v + t[1].view(self.f.dtype).double()
        if self.stacked:
            v = v[cg0:cg0 + ncg]                                   # [CG][B][Hp][Wp][8]
            if tall:
                v = v.reshape(ncg, 1, self.B * (self.H + 2), self.W + 2, 8)
            v = v.permute(1, 0, 4, 2, 3)
        else:
            v = v[:, cg0:cg0 + ncg].permute(0, 1, 4, 2, 3)
        return v.reshape(v.shape[0], ncg * 8, v.shape[3], v.shape[4])


def _sign_positive(buf, cg0, ncg):
    """The mask operand as the epilogue reads it: the stored hi element is > 0 (sign clear, magnitude not zero)."""
    h = buf.bits()[0][:, cg0:cg0 + ncg].permute(0, 1, 4, 2, 3).reshape(buf.B, ncg * 8, buf.H + 2, buf.W + 2)
    return (h.int() > 0)[:, :, 1:-1, 1:-1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch and its float64 restatement

class Case:
    """One esr_conv3x3 launch.  Channels: in0 = one latent group of `lat` channels (PackedConv's K layout), in1 = `cin` channels at group
    `in1_off` of a buffer with `in1_extra` more groups behind.  res1 / res2 / mask_src are their own buffers unless res1 == 'resin'
    (a group slice of in1 at `resin_g`, same strides).  Every option of the descriptor is an attribute."""

    def __init__(self, fmt='split', B=2, H=12, W=17, cin=16, cout=32, lat=0, ups=1, in1_off=0, in1_extra=0, act_slope=0.2, alpha=0.75,
                 bias=True, res1=None, beta1=0.5, res2=False, beta2=-0.25, resin_g=1, out='act', out_lo=True, out2=None, mask=None,
                 ps=None, in1_lo_groups=0, reverse=0, lds_stages=0, tall=False, seed=1, wscale=None):
        self.__dict__.update(locals())
        del self.__dict__['self']
        self.f = FMTS[fmt]


def _weights(case):
    A = _A()
    cin_w = case.lat + case.cin
    rows = case.cout if case.ps is None else case.ps[2]
    g = torch.Generator().manual_seed(1000 + case.seed)
    s = case.wscale if case.wscale is not None else 1.0 / math.sqrt(9 * cin_w)
    w = ((torch.rand(rows, cin_w, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) * s).float()
    b = ((torch.rand(rows, generator=g, dtype=torch.float64) * 2 - 1) * 0.25).float()
    wd, bd = w.to(DEV), b.to(DEV)
    if case.ps is not None:
        r, rg0, _ = case.ps
        # launch row -> conv channel ((g / r^2) * 8 + row % 8) * r^2 + s with row group g = ps_rowgroup0 + row / 8 (esr_conv3x3_desc.pixel_shuffle)
        prow = [((((rg0 + j // 8) // (r * r)) * 8 + j % 8) * r * r + (rg0 + j // 8) % (r * r)) for j in range(case.cout)]
        pc = A.PackedConv(wd, bd, case.lat, split=case.f.split, rows=prow).get()
        return w, b, pc, prow
    if case.cout > 64:
        pc = A.PackedConvSlices(wd, bd, case.lat, split=case.f.split).get()
    else:
        pc = A.PackedConv(wd, bd, case.lat, split=case.f.split).get()
    return w, b, pc, list(range(case.cout))


class Result:
    pass


def run(case, teeth=True, check_only=False):
    """Build, launch, compare with the float64 reference (returns a Result with the raw destination bits for bit-identity checks)."""
    A = _A()
    c, f = case, case.f
    ups = c.ups
    Hin, Win = c.H // ups, c.W // ups
    w, b, pc, rows = _weights(c)
    ncg1 = (c.cin + 7) // 8
    G = (1 if c.lat else 0) + ncg1                                     # K groups of the launch
    nout = (c.cout + 7) // 8                                           # output groups the launch writes
    # inputs
    if c.tall:
        x1 = Buf(f, c.B, ncg1, Hin, Win, fill='random', seed=c.seed, stacked=True)
        for p in range(x1.P):                                          # the rows between stacked images are their zero borders
            x1.t[p, :, :, 0] = 0
            x1.t[p, :, :, -1] = 0
        in1, rows_tall = x1.tall()
        Bl, Hl, Wl = 1, rows_tall, c.W
    else:
        x1 = Buf(f, c.B, c.in1_off + ncg1 + c.in1_extra, Hin, Win, fill='random', seed=c.seed)
        in1 = x1.view(c.in1_off, ncg1)
        Bl, Hl, Wl = c.B, c.H, c.W
    x0 = in0 = None
    if c.lat:
        x0 = Buf(f, c.B, 1, c.H, c.W, fill='random', seed=c.seed + 7)
        in0 = x0.view()
    # which groups' lo planes the kernel multiplies: all (hi+lo formats), none (in1_lo_groups < 0), or the leading chunks
    lo_groups = G if f.planes == 2 else 0
    if f.planes == 2 and c.in1_lo_groups < 0:
        lo_groups = 0
    elif f.planes == 2 and 0 < c.in1_lo_groups < ncg1:
        lo_groups = 2 * ((G - ncg1 + c.in1_lo_groups + 1) // 2)       # whole K chunks: an odd count reads the next group's lo plane too
    first = G - ncg1                                                   # in0 groups in front of in1's
    big_lo = f.name == 'f16x2' and c.in1_lo_groups != 0
    if f.planes == 2 and (lo_groups < G or big_lo):
        # the lo planes the kernel must not multiply hold hi-sized values (not a residue): multiplying one is a gross error.  In the 2-MFMA
        # form (f16x2: one weight plane, Whi*Xhi + Whi*Xlo) the ones it multiplies may too: skipping one is then a gross error as well.  (The
        # 3-MFMA form drops Wlo*Xlo, which is within its bound only for a residue.)
        g = torch.Generator().manual_seed(c.seed + 23)
        for q in range(0 if big_lo else lo_groups, G):
            buf, gi = (x0, 0) if q < first else (x1, q - first + (0 if c.tall else c.in1_off))
            sl = buf.t[1, gi] if buf.stacked else buf.t[1, :, gi]
            junk = (torch.rand(sl[..., 1:-1, 1:-1, :].shape, generator=g, dtype=torch.float64) * 2 - 1).to(f.dtype)
            sl[..., 1:-1, 1:-1, :] = junk.view(torch.int16).to(DEV)
    # residuals and the mask operand
    r1 = r2 = mk = None
    res1 = res2 = mask_src = None
    if c.res1 in ('resin', 'resin_stride'):
        assert c.resin_g + nout <= ncg1 and not c.tall, 'the residual slice must lie inside in1'
    if c.res1 == 'resin':
        res1 = x1.view(c.in1_off + c.resin_g, nout)
    elif c.res1 == 'resin_stride':                                     # the same values, another buffer with a different cg_stride
        r1 = Buf(f, c.B, 1 + nout, c.H + 1, c.W, fill='random', seed=c.seed + 11)
        r1.t[:, :, 1:1 + nout, :c.H + 2] = x1.t[:, :, c.in1_off + c.resin_g:c.in1_off + c.resin_g + nout]
        r1.t[:, :, 1:1 + nout, c.H + 2:] = 0
        res1 = r1.view(1, nout)
        res1.H = c.H
    elif c.res1:
        r1 = Buf(f, c.B, nout + 2, c.H, c.W, fill='random', seed=c.seed + 11)
        res1 = r1.view(1, nout + 1)
    if c.res2:
        r2 = Buf(f, c.B, nout + 1, c.H, c.W, fill='random', seed=c.seed + 13)
        res2 = r2.view(0, nout + 1)
    if c.mask is not None:
        m0, m1, mslope, mfmt = c.mask
        mk = Buf(mfmt, c.B, (m1 - m0) + 1 + 16, c.H, c.W, fill='random', seed=c.seed + 17)    # (16 spare groups: any slice offset reads inside)
        mask_src = mk.view(1, m1 - m0)
    # destinations, sentinel-filled: the view starts one group into its buffer and covers one group more than the launch writes
    o = o2 = onchw = None
    out = out2 = None
    out_planes = f.planes if c.out_lo else 1
    if c.out == 'nchw':
        n = c.B * c.cout * c.H * c.W
        onchw = torch.full((n + 128,), SENT32, dtype=torch.int32, device=DEV)
    elif c.ps is not None:
        r, rg0, _ = c.ps
        nps = (rg0 + nout + r * r - 1) // (r * r)
        o = Buf(f, Bl, nps + 2, r * Hl, r * Wl, planes=out_planes, fill='sentinel')
        out = o.view(1, nps, lo=c.out_lo)
    elif c.tall:
        o = Buf(f, c.B, nout + 2, c.H, c.W, planes=out_planes, fill='sentinel', stacked=True)
        out, _ = o.tall(1)
        if not c.out_lo:
            out.lo = None
    else:
        o = Buf(f, Bl, nout + 2, Hl, Wl, planes=out_planes, fill='sentinel')
        out = o.view(1, nout + 1, lo=c.out_lo)
    if c.out2 is not None:
        o2 = Buf(f, Bl, nout + 2, Hl, Wl, planes=out_planes, fill='sentinel')        # 'hi': the buffer has a lo plane the launch must not touch
        out2 = o2.view(1, nout + 1, lo=(c.out2 == 'same'))
    kw = dict(in0=in0, upsample=ups, act_slope=c.act_slope, alpha=c.alpha, res1=res1, beta1=c.beta1, res2=res2, beta2=c.beta2, out=out,
              out2=out2, use_bias=c.bias, reverse=bool(c.reverse), in1_lo_groups=c.in1_lo_groups)
    if onchw is not None:
        kw['out_nchw'] = onchw[64:64 + c.B * c.cout * c.H * c.W]
    if mask_src is not None:
        kw.update(mask_src=mask_src, mask_cg=(c.mask[0], c.mask[1]), mask_slope=c.mask[2])
    if c.ps is not None:
        kw.update(pixel_shuffle=c.ps[0], ps_rowgroup0=c.ps[1])
    saved = A.LDS_STAGES
    A.LDS_STAGES = c.lds_stages
    try:
        A.conv3x3(pc, in1, Bl, Hl, Wl, c.cout, **kw)
    finally:
        A.LDS_STAGES = saved
    torch.cuda.synchronize()

    # ---- the float64 reference
    def stored_input(nlo, absolute=False):
        """The concatenated input as stored, with the lo planes of its first `nlo` groups (upsampled, with its zero border); absolute:
        |hi| + |lo| (each plane is multiplied on its own: the weight rounding scales with both)."""
        off = c.in1_off if not c.tall else 0
        his = ([x0.values(lo=False)] if c.lat else []) + [x1.values(off, ncg1, lo=False, tall=c.tall)]
        los = ([x0.values(lo=True)] if c.lat else []) + [x1.values(off, ncg1, lo=True, tall=c.tall)]
        hi = torch.cat(his, 1)
        lo = torch.cat(los, 1) - hi                                    # (exact: hi + lo was summed in float64)
        lo[:, 8 * nlo:] = 0
        X_ = hi.abs() + lo.abs() if absolute else hi + lo
        if ups > 1:
            X_ = F.pad(X_[:, :, 1:-1, 1:-1].repeat_interleave(ups, 2).repeat_interleave(ups, 3), (1, 1, 1, 1))
        return X_

    X = stored_input(lo_groups)
    # the weight over the launch's K lanes: [latent group (lat channels, zero pad)] [in1 groups]
    Wk = torch.zeros(len(rows), 8 * G, 3, 3, dtype=torch.float64)
    wd = w.double()[rows]
    k0 = 0
    if c.lat:
        Wk[:, :c.lat] = wd[:, :c.lat]
        k0 = 8
    Wk[:, k0:k0 + c.cin] = wd[:, c.lat:]
    conv = F.conv2d(X, Wk)
    aconv = F.conv2d(stored_input(lo_groups, absolute=True), Wk.abs())
    bias = b.double()[rows] if c.bias else torch.zeros(len(rows), dtype=torch.float64)
    K = 9 * 8 * G
    # destination-layout values of the launch's groups (all 8 lanes: rows past cout have zero weights and bias)
    nl = 8 * nout
    Bc = conv.shape[0]

    def lanes(t):
        out_ = torch.zeros(Bc, nl, conv.shape[2], conv.shape[3], dtype=torch.float64)
        out_[:, :t.shape[1]] = t
        return out_

    res_vals = []
    if res1 is not None:
        if c.res1 == 'resin':
            # RESIN reads the residual out of the input tile the K loop stages: hi (+ lo where those chunks carry one)
            g0 = c.in1_off + c.resin_g
            rv = x1.values(g0, nout + 1 if g0 + nout < x1.ncg else nout, lo=f.planes == 2)[:, :, 1:-1, 1:-1]
        elif c.res1 == 'resin_stride':
            rv = r1.values(1, nout)[:, :, 1:c.H + 1, 1:-1]
        else:
            rv = r1.values(1, nout + 1)[:, :, 1:-1, 1:-1]
        res_vals.append((c.beta1, rv))
    if res2 is not None:
        res_vals.append((c.beta2, r2.values(0, nout + 1)[:, :, 1:-1, 1:-1]))
    mpos = _sign_positive(mk, 1, c.mask[1] - c.mask[0]) if mk is not None else None

    def epilogue(conv_, shift_res=0, shift_mask=0):
        pre = lanes(conv_ + bias.view(1, -1, 1, 1))
        v = c.alpha * torch.where(pre > 0, pre, c.act_slope * pre)
        S = lanes(c.alpha * aconv + bias.abs().view(1, -1, 1, 1))
        for beta, rv in res_vals:
            rr = rv[:, 8 * shift_res:8 * shift_res + nl]
            if rr.shape[1] < nl:
                rr = torch.cat([rr, rv[:, :nl - rr.shape[1]]], 1)
            v = v + beta * rr
            S = S + abs(beta) * rr.abs()
        if mpos is not None:
            m0, m1, ms = c.mask[0] + shift_mask, c.mask[1] + shift_mask, c.mask[2]
            for g in range(max(0, m0), min(m1, nout)):
                src = g - c.mask[0] - shift_mask
                fac = torch.where(mpos[:, 8 * src:8 * src + 8], 1.0, ms) if 0 <= src < mpos.shape[1] // 8 else torch.full_like(v[:, :8], ms)
                v[:, 8 * g:8 * g + 8] = v[:, 8 * g:8 * g + 8] * fac
        return v, S

    ref, S = epilogue(conv)
    res = Result()
    res.case = c
    # ---- what the kernel stored, in the reference's layout, and the sentinel check
    if c.out == 'nchw':
        raw = onchw.cpu()
        assert (raw[:64] == SENT32).all() and (raw[64 + c.B * c.cout * c.H * c.W:] == SENT32).all(), 'out_nchw guard elements written'
        y = raw[64:64 + c.B * c.cout * c.H * c.W].view(torch.float32).double().reshape(c.B, c.cout, c.H, c.W)
        ref, S = ref[:, :c.cout], S[:, :c.cout]
        c_out = C_NCHW
        res.raw = [raw]

        def fold(t):
            return t[:, :c.cout]
    elif c.ps is not None:
        r, rg0, _ = c.ps
        ob = o.bits()
        res.raw = [ob]
        written = torch.zeros(ob.shape[1:], dtype=torch.bool)          # [B][CG][Hp][Wp][8]
        for j in range(nout):
            g = rg0 + j
            sp = g % (r * r)
            written[:, 1 + g // (r * r), 1 + sp // r:1 + r * Hl:r, 1 + sp % r:1 + r * Wl:r] = True
        assert (ob[:, ~written] == SENT).all(), 'pixel-shuffle store wrote outside its row groups / interior'
        yall = o.values(1, o.ncg - 2, lo=c.out_lo)[:, :, 1:-1, 1:-1]

        def fold(t):
            """[B][8*nout][H][W] launch rows -> [B][nout][8][H][W], the layout of y below (row group j at its shuffled position)"""
            return torch.stack([t[:, 8 * j:8 * j + 8] for j in range(nout)], 1)

        ys = []
        for j in range(nout):
            g = rg0 + j
            sp = g % (r * r)
            cg = g // (r * r)
            ys.append(yall[:, 8 * cg:8 * cg + 8, sp // r::r, sp % r::r])
        y = torch.stack(ys, 1)
        ref, S = fold(ref), fold(S)
        c_out = f.c_out_hilo if (c.out_lo and f.planes == 2) else f.c_out_hi
    else:
        ob = o.bits()
        res.raw = [ob]
        written = torch.zeros(ob.shape[1:], dtype=torch.bool)
        if c.tall:                                                     # [CG][B][Hp][Wp][8]: the launch's interior = rows 1 .. B*(H+2)-2
            tw = written.view(written.shape[0], -1, written.shape[3], 8)
            tw[1:1 + nout, 1:-1, 1:-1] = True
        else:
            written[:, 1:1 + nout, 1:-1, 1:-1] = True
        assert (ob[:, ~written] == SENT).all(), 'the launch wrote a border pixel or a group outside [0, ceil(cout/8))'
        y = o.values(1, nout, lo=c.out_lo, tall=c.tall)[:, :, 1:-1, 1:-1]
        if o2 is not None:
            ob2 = o2.bits()
            res.raw.append(ob2)
            if c.out2 == 'hi' and o2.P == 2:
                assert (ob2[1] == SENT).all(), 'a hi-only out2 had its lo plane written'
            assert (ob2[:, ~written] == SENT).all(), 'out2: written outside the destination groups'
            # the same values: out2's planes equal out's bit for bit
            assert torch.equal(ob2[0, :, 1:1 + nout], ob[0, :, 1:1 + nout]), 'out2 hi plane differs from out'
            if c.out2 == 'same' and o2.P == 2:
                assert torch.equal(ob2[1, :, 1:1 + nout], ob[1, :, 1:1 + nout]), 'out2 lo plane differs from out'

        def fold(t):
            return t
        c_out = f.c_out_hilo if (c.out_lo and f.planes == 2) else f.c_out_hi
    bound_of = lambda S_, r_: f.c_w * S_ + c_out * r_.abs() + K * 2.0 ** -24 * S_

    def excess(y_, ref_, S_):
        err = (y_ - ref_).abs()
        e = err / bound_of(S_, ref_)
        e[err == 0] = 0.0                                              # (lanes past cout without residuals: 0 / 0)
        e[torch.isnan(err)] = float('inf')
        return e

    e = excess(y, ref, S)
    worst = float(e.max())
    res.y, res.ref, res.S, res.excess = y, ref, S, worst
    if check_only:
        return res
    if not worst <= 1.0:
        bad = (e > 1.0).nonzero()
        at = tuple(int(i) for i in np.unravel_index(int(e.argmax()), e.shape))
        raise AssertionError('element-wise bound exceeded at %d elements (channels %s): worst |y-ref|/bound = %.3g at %s, y = %r, ref = %r'
                             % (bad.shape[0], sorted(set(bad[:, 1].tolist()))[:16], worst, at, float(y[at]), float(ref[at])))
    if teeth:
        planted = []
        if c.alpha != 0:
            # a dropped corner tap: output pixel (last row, last column) of image 0 without tap (0, 0) (1-pixel images: the centre tap)
            Y, Xo = conv.shape[2] - 1, conv.shape[3] - 1
            dy, dx = (0, 0) if Y > 0 and Xo > 0 else (1, 1)
            bad = conv.clone()
            bad[0, :, Y, Xo] -= (Wk[:, :, dy, dx] * X[0, :, Y + dy, Xo + dx]).sum(1)
            planted.append(('dropped corner tap', fold(epilogue(bad)[0])))
        if res_vals:
            planted.append(('residual from the neighbouring group', fold(epilogue(conv, shift_res=1)[0])))
        if mpos is not None and c.alpha != 0:
            planted.append(('mask window shifted by one group', fold(epilogue(conv, shift_mask=1)[0])))
        if f.planes == 2 and c.in1_lo_groups != 0:
            # one lo plane more (a hi-sized one) or, where the read ones are hi-sized too, one fewer
            if lo_groups < G:
                planted.append(('one lo plane more', fold(epilogue(F.conv2d(stored_input(lo_groups + 1), Wk))[0])))
            if lo_groups > 0 and big_lo:
                planted.append(('one lo plane fewer', fold(epilogue(F.conv2d(stored_input(lo_groups - 1), Wk))[0])))
        assert planted
        for what, bad in planted:
            assert float(excess(y, bad, S).max()) > 1.0, 'the comparator accepts a planted error: ' + what
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------
# epilogues x formats

EPILOGUES = {
    'plain': dict(),
    'plain_relu_nobias': dict(act_slope=0.0, bias=False, alpha=1.3),
    'res1': dict(res1=True, act_slope=0.2),
    'res12': dict(res1=True, res2=True, act_slope=1.0, alpha=0.2),
    'resin': dict(res1='resin', act_slope=1.0, alpha=0.2, beta1=1.0, cin=48, in1_off=1, resin_g=2),
    'resin_res2': dict(res1='resin', res2=True, act_slope=1.0, alpha=0.2, beta1=1.0, cin=40, in1_off=1, resin_g=1),
    'nchw': dict(out='nchw', cout=24, act_slope=0.2),
    'out2': dict(out2='same', act_slope=0.2),
    'out2_hi': dict(out2='hi', act_slope=0.2),
    'mask': dict(mask=(1, 3, 0.2, 'f16'), act_slope=1.0, cout=40),
    'mask_relu': dict(mask=(2, 4, 0.0, 'bf16'), act_slope=1.0, cout=40),
    'res1_mask': dict(res1=True, mask=(1, 3, 0.2, 'f16'), act_slope=1.0, cout=32),
    'res1_mask_relu': dict(res1=True, mask=(1, 2, 0.0, 'bf16'), act_slope=1.0, cout=24),
}
F16_EPI = ['plain', 'plain_relu_nobias', 'res1', 'res12', 'resin', 'resin_res2', 'nchw', 'out2', 'out2_hi', 'mask', 'mask_relu']
EPI_CASES = [(fm, e) for fm in ('bf16', 'split') for e in EPILOGUES] + [(fm, e) for fm in ('f16', 'f16x2', 'f16x3') for e in F16_EPI]


@pytest.mark.parametrize('fmt,epi', EPI_CASES, ids=['%s-%s' % c for c in EPI_CASES])
def test_epilogues(fmt, epi):
    kw = dict(EPILOGUES[epi])
    if epi == 'out2_hi' and FMTS[fmt].planes == 1:
        kw['out2'] = 'same'
    run(Case(fmt=fmt, **kw))


def test_resin_near_misses():
    """res1 values that only LOOK like the RESIN slice take the RES1 path and must meet the same bound: the values in another buffer with a
    different cg_stride, act_slope 0.2, alpha = 0 (out = beta1 * res1)."""
    base = dict(fmt='split', res1='resin', cin=48, in1_off=1, resin_g=2, beta1=1.0, alpha=0.2, act_slope=1.0)
    run(Case(**dict(base, res1='resin_stride')))
    run(Case(**dict(base, act_slope=0.2)))
    r = run(Case(**dict(base, alpha=0.0, fmt='bf16')))
    assert float(r.ref.abs().max()) > 0


def test_resin_with_latent():
    """RESIN with an in0 segment in front: the residual group index counts the latent group (resin_g0 = in0.ncg + offset)."""
    for fmt in ('split', 'f16x2'):
        run(Case(fmt=fmt, lat=3, cin=48, res1='resin', resin_g=2, beta1=1.0, alpha=0.2, act_slope=1.0, cout=32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# formats and channel layouts

FORMAT_CASES = [
    # (fmt, cin, cout, lat, in1_off, in1_extra)
    ('bf16', 24, 3, 3, 0, 0),           # in0 + 3 in1 groups: 4 groups, no straddle
    ('split', 16, 8, 5, 0, 0),          # in0 + 2 groups = 3: K chunk 0 straddles in0 / in1 (the latent case), chunk 1 reads a past-end group
    ('split', 64, 24, 3, 2, 1),         # latent, in1 view mid-buffer, 9 groups
    ('split', 40, 40, 0, 3, 2),
    ('f16', 40, 64, 5, 1, 0),
    ('f16x2', 16, 128, 5, 0, 0),
    ('f16x3', 24, 32, 3, 2, 1),
    ('bf16', 8, 192, 0, 1, 0),
    ('f16x3', 64, 192, 0, 0, 1),
]


@pytest.mark.parametrize('fmt,cin,cout,lat,off,extra', FORMAT_CASES, ids=['%s-%d-%d-l%d-o%d' % c[:5] for c in FORMAT_CASES])
def test_formats(fmt, cin, cout, lat, off, extra):
    run(Case(fmt=fmt, cin=cin, cout=cout, lat=lat, in1_off=off, in1_extra=extra, H=9, W=14, res1=cout <= 64, res2=cout <= 64))


@pytest.mark.parametrize('fmt,cin,lo_groups,out_lo,lat', [('f16x2', 48, 3, True, 0), ('f16x2', 48, 2, True, 3), ('f16x3', 48, -1, True, 0),
                                                         ('f16x3', 48, 3, True, 0), ('f16x3', 48, 2, True, 0),
                                                         ('f16x3', 96, 8, True, 3), ('f16x2', 96, 8, False, 3),
                                                         ('f16x2', 32, 0, False, 0), ('f16x3', 48, 4, False, 3), ('f16x2', 40, 3, True, 3)])
def test_partial_lo(fmt, cin, lo_groups, out_lo, lat):
    """fp16 partial lo (esr_conv3x3_desc.in1_lo_groups, out.lo == NULL).  The lo planes the kernel must not multiply hold hi-sized values:
    those behind the first in1_lo_groups groups except the one that completes the last K chunk with lo planes (whole chunks of two groups,
    in0's included: esr_hip.h), all of them with in1_lo_groups < 0; in the 2-MFMA form (f16x2) the ones it multiplies too.  The comparator
    must reject the reference with one lo plane more and, in f16x2, one fewer: that pins the chunk rounding (3 lo groups read the 4th group's
    lo plane; latent + 2 read in1's 3rd; the dense block's latent + 8 trunk groups read the 9th's)."""
    run(Case(fmt=fmt, cin=cin, lat=lat, cout=32, in1_lo_groups=lo_groups, out_lo=out_lo, res1=True, act_slope=0.2))


@pytest.mark.parametrize('cout', [3, 8, 24, 32, 40, 64, 128, 192])
def test_cout(cout):
    run(Case(fmt='split', cin=24, cout=cout, H=7, W=11, res1=cout <= 64, act_slope=0.2))


def test_slices():
    """Multi-slice cout (128, 192): res1 / res2 / mask_src / bias indexed by absolute output channel, a mask window spanning two slices."""
    run(Case(fmt='split', cin=16, cout=128, H=6, W=9, res1=True, res2=True, act_slope=0.2))
    run(Case(fmt='split', cin=16, cout=128, H=6, W=9, mask=(6, 11, 0.2, 'split'), act_slope=1.0))
    run(Case(fmt='bf16', cin=16, cout=192, H=6, W=9, res1=True, mask=(3, 20, 0.0, 'bf16'), act_slope=1.0))
    run(Case(fmt='f16', cin=16, cout=128, H=6, W=9, mask=(7, 9, 0.2, 'f16'), act_slope=1.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# tile geometry, as the library's own picker chooses it (esr_conv3x3_tiling: the same decision esr_conv3x3 makes), to place the shapes below
# on its boundaries

def tiling(B, H, W, cout, split=True, **fields):
    """(tiles along x, tiles along y, M tiles per workgroup, output slices) of a launch with these sizes and descriptor fields."""
    import ctypes as C
    from esr_hip import _lib
    d = _lib.Conv3x3Desc()
    d.in1 = _lib.ActView(16, 16 if split else None, 1, H, W, 0, 0, 0)       # (never dereferenced: a host-only query)
    d.B, d.H, d.W, d.cout = B, H, W, cout
    for k, v in fields.items():
        setattr(d, k, v)
    t = (C.c_int32 * 4)()
    assert _lib.load_library().esr_conv3x3_tiling(C.byref(d), t) == 0
    return tuple(t)


def workgroups(B, H, W, cout, split=True, **fields):
    tx, ty, _, ns = tiling(B, H, W, cout, split, **fields)
    return tx * ty * B * ns


def test_picker_boundaries_used_below():
    # the column split of the picker (one tile column below, two above), for the 1-, 2- and two-slice forms
    assert tiling(1, 5, 74, 64)[0] == 1 and tiling(1, 5, 75, 64)[0] == 2
    assert tiling(1, 1, 189, 32, split=False)[0] == 1 and tiling(1, 1, 190, 32, split=False)[0] == 2
    assert tiling(1, 1, 189, 64)[0] == 1 and tiling(1, 1, 190, 64)[0] == 2
    # 320 / 321 workgroups: the small (multi-stage) and the large form
    assert workgroups(320, 4, 4, 32) == 320 and workgroups(321, 4, 4, 32) == 321
    assert workgroups(160, 4, 4, 64, split=False) == 320 and workgroups(161, 4, 4, 64, split=False) == 322     # as two 32-channel slices
    # the two-slice form of a 64-channel layer stops at 320 tiles
    assert tiling(320, 4, 4, 64, split=False) == (1, 1, 1, 2) and tiling(321, 4, 4, 64, split=False) == (1, 1, 2, 1)
    for n in (1, 3, 7, 9, 13, 17):                  # below 8 and not multiples of 8: the XCD remap
        assert workgroups(n, 6, 10, 32) == n


GEOM = [
    # (B, H, W, cin, cout, fmt)
    (1, 1, 1, 16, 32, 'split'), (2, 1, 9, 8, 24, 'bf16'), (2, 7, 1, 8, 40, 'split'),
    (1, 5, 74, 16, 64, 'split'), (1, 5, 75, 16, 64, 'split'), (1, 1, 189, 8, 32, 'bf16'), (1, 1, 190, 8, 32, 'bf16'),
    (1, 1, 189, 16, 64, 'split'), (1, 1, 190, 16, 64, 'split'),
    (2, 20, 29, 16, 40, 'split'), (1, 33, 21, 24, 32, 'f16x2'), (2, 67, 70, 16, 32, 'split'),
    (1, 6, 10, 16, 32, 'split'), (3, 6, 10, 16, 32, 'split'), (7, 6, 10, 16, 64, 'bf16'), (9, 6, 10, 16, 32, 'split'),
    (13, 6, 10, 8, 24, 'f16'), (17, 6, 10, 16, 32, 'split'),
    (320, 4, 4, 16, 32, 'split'), (321, 4, 4, 16, 32, 'split'), (320, 4, 4, 16, 64, 'bf16'), (321, 4, 4, 16, 64, 'bf16'),
    (160, 4, 4, 16, 64, 'bf16'), (161, 4, 4, 16, 64, 'bf16'),
]


@pytest.mark.parametrize('B,H,W,cin,cout,fmt', GEOM, ids=['%dx%dx%d-%d-%d-%s' % g for g in GEOM])
@pytest.mark.parametrize('heavy', [False, True], ids=['plain', 'heavy'])
def test_geometry(B, H, W, cin, cout, fmt, heavy):
    """Images smaller than a tile, widths on both sides of the picker's column split, ragged last tiles, 1-17 tiles (the XCD remap) and
    320 / 321 tiles (the small / large form switch); on the plain and on the heaviest epilogue (res1 + res2 + out2, or res1 + mask)."""
    kw = dict(fmt=fmt, B=B, H=H, W=W, cin=cin, cout=cout, seed=B + H + W)
    if heavy and (cout <= 32 or B > 300):
        kw.update(res1=True, res2=True, act_slope=0.2)
    elif heavy:
        kw.update(res1=True, mask=(1, 3, 0.2, 'bf16'), act_slope=1.0)
    run(Case(**kw))


def _mask_view_stub():
    from esr_hip import _lib
    return _lib.ActView(16, None, 4, 12, 17, 0, 0, 0)


def test_two_slice_form():
    """A 64-channel launch of few tiles runs as two 32-channel slices (mslice); with a partial mask window it does not.  Both meet the bound."""
    assert tiling(2, 12, 17, 64)[3] == 2
    assert tiling(2, 12, 17, 64, mask_src=_mask_view_stub(), mask_cg0=2, mask_cg1=6)[3] == 1
    run(Case(fmt='split', B=2, H=12, W=17, cin=16, cout=64, res1=True, res2=True, act_slope=0.2))
    run(Case(fmt='split', B=2, H=12, W=17, cin=16, cout=64, mask=(0, 8, 0.2, 'split'), act_slope=1.0))
    run(Case(fmt='split', B=2, H=12, W=17, cin=16, cout=64, mask=(2, 6, 0.2, 'split'), act_slope=1.0))
    run(Case(fmt='f16x2', B=2, H=12, W=17, cin=72, cout=64, res1='resin', resin_g=1, beta1=1.0, alpha=0.2, act_slope=1.0))


PS_CASES = [('split', 2, 3, 32, 2), ('bf16', 3, 5, 64, 2), ('f16x2', 2, 1, 24, 2), ('f16', 3, 10, 40, 3), ('f16x3', 2, 4, 32, 2)]


@pytest.mark.parametrize('fmt,r,rg0,cout,nps', PS_CASES, ids=['%s-r%d-rg%d-%d' % c[:4] for c in PS_CASES])
def test_pixel_shuffle(fmt, r, rg0, cout, nps):
    """The pixel-shuffle store of row groups [rg0, rg0 + cout/8) of a conv to nps*8*r^2 channels, against F.pixel_shuffle of the float64
    conv: each row group lands at its (output group, sub-position); every other position of the shuffled buffer keeps its sentinel."""
    c = Case(fmt=fmt, cin=16, cout=cout, ps=(r, rg0, nps * 8 * r * r), H=7, W=9, act_slope=0.2, alpha=1.0)
    run(c)
    # the same values through torch's own shuffle of the whole conv: the launch's rows are a slice of it
    w, b, _, prow = _weights(c)
    assert sorted(prow) == sorted(set(prow))
    full = torch.zeros(1, nps * 8 * r * r, c.H, c.W, dtype=torch.float64)
    for k, ch in enumerate(prow):
        full[0, ch] = k + 1                                            # conv channel of launch row k carries k + 1
    shuffled = F.pixel_shuffle(full, r)
    for j in range(cout // 8):
        g = rg0 + j
        sp = g % (r * r)
        got = shuffled[0, 8 * (g // (r * r)):8 * (g // (r * r)) + 8, sp // r::r, sp % r::r]
        assert torch.equal(got, torch.arange(8 * j + 1, 8 * j + 9, dtype=torch.float64).view(8, 1, 1).expand_as(got))


def test_tall_view():
    """A launch over stacked images (stacked_at / tall_view): one image of B*(H+2)-2 rows whose inter-image rows are zero in the input."""
    run(Case(fmt='bf16', B=5, H=4, W=6, cin=32, cout=64, tall=True))
    run(Case(fmt='split', B=3, H=8, W=8, cin=16, cout=32, tall=True, res1=None, act_slope=0.2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# fused nearest upsample

@pytest.mark.parametrize('ups,H,W,fmt', [(2, 14, 22, 'split'), (3, 15, 21, 'bf16'), (2, 10, 6, 'f16x2'), (3, 9, 27, 'f16')])
def test_upsample(ups, H, W, fmt):
    run(Case(fmt=fmt, ups=ups, H=H, W=W, cin=16, cout=32, res1=True, act_slope=0.2))


UPS_EXACT = (1, 2, 3, 4, 6, 8)


@pytest.mark.parametrize('ups', range(1, 9))
def test_upsample_factor_at_the_coordinate_limit(ups):
    """Every factor up to 8 at the widest image the entry point accepts (W + 2 < 32768).  The kernel forms the source column (X - 1 + ups) / ups
    as a multiplication by ceil(2^16 / ups) (setup_tile): exact at every reachable coordinate for ups in {1, 2, 3, 4, 6, 8}; for 5 and 7 one
    too large from X = 16380 / 13104 on (the next source column was read: 732110 / 978081 elements of these launches off), so esr_conv3x3
    refuses those two factors."""
    Win = 32765 // ups
    c = Case(fmt='bf16', ups=ups, B=1, H=ups, W=Win * ups, cin=8, cout=16, act_slope=0.2, seed=ups)
    if ups in UPS_EXACT:
        run(c)
    else:
        assert _launch_rc(c) == E_UNSUPPORTED


def test_upsample_with_in0_refused():
    assert _launch_rc(Case(fmt='split', lat=3, ups=2, H=8, W=8)) == E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------------
# hints with no effect on the result

@pytest.mark.parametrize('epi', ['plain', 'res12', 'resin', 'mask', 'out2_hi'])
def test_hints_bit_identical(epi):
    kw = dict(EPILOGUES[epi])
    kw.update(fmt='split', B=2, H=20, W=23)
    base = None
    for rev in (0, 1):
        for st in (0, 1, 2):
            r = run(Case(reverse=rev, lds_stages=st, **kw), teeth=(rev == 0 and st == 0))
            if base is None:
                base = r.raw
            else:
                assert all(torch.equal(a, b) for a, b in zip(base, r.raw)), 'reverse_order=%d lds_stages=%d changed the result' % (rev, st)


def test_four_stage_ring():
    """Few small tiles with a long K axis: plain bf16 launches of the 64-row kernel run the four-stage ring (>= 16 chunks; >= 8 with an
    fp32 NCHW destination).  (A 64-channel act-layout launch this small runs as two 32-channel slices instead: cout 128.)"""
    assert tiling(2, 6, 6, 128, split=False)[2] == 2 and workgroups(2, 6, 6, 128, split=False) <= 320
    assert tiling(2, 6, 6, 64, split=False)[3] == 2             # (the act-layout 64-channel launch: two slices of the 32-channel kernel)
    run(Case(fmt='bf16', B=2, H=6, W=6, cin=256, cout=128, act_slope=1.0))
    run(Case(fmt='bf16', B=2, H=6, W=6, cin=128, cout=64, act_slope=0.2, out='nchw', bias=False))


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp16 range watch

def _bias_launch(fmt, bias_vals, tag_watch=None, cout=8):
    """A launch whose output is exactly its bias (zero weights): stores chosen values."""
    A = _A()
    f = FMTS[fmt]
    w = torch.zeros(cout, 8, 3, 3, device=DEV)
    b = torch.tensor(bias_vals + [0.0] * (cout - len(bias_vals)), dtype=torch.float32, device=DEV)
    pc = A.PackedConv(w, b, 0, split=f.split).get()
    x = Buf(f, 1, 1, 5, 6, fill='random')
    o = Buf(f, 1, 1, 5, 6)
    A.conv3x3(pc, x.view(), 1, 5, 6, cout, act_slope=1.0, alpha=1.0, out=o.view())
    return o


def test_range_watch():
    A = _A()
    cases = [('f16', [32752.0, -32752.0], False), ('f16x2', [32768.0], True), ('f16', [-40000.0], True), ('f16', [float('inf')], True),
             ('f16x3', [float('nan')], True), ('f16', [1.0, 65504.0 / 4], False)]
    for fmt, vals, fires in cases:
        w = A.RangeWatch(DEV)
        with A.watching(w):
            o = _bias_launch(fmt, vals)
        torch.cuda.synchronize()
        got = int(w.flag.item())
        assert (got == 0) == fires and (got == -1) == (not fires), (fmt, vals, got)
        stored = o.values()[0, :len(vals), 3, 3]
        if not any(math.isnan(v) for v in vals) and all(abs(v) < 65504 for v in vals):
            assert stored.tolist() == vals
    # several launches with distinct tags, the later ones overflowing: the smallest overflowing tag stays in the word
    w = A.RangeWatch(DEV)
    with A.watching(w):
        _bias_launch('f16', [100.0])
        _bias_launch('f16x2', [5.0])
        _bias_launch('f16', [50000.0])
        _bias_launch('f16', [1.0])
        _bias_launch('f16x3', [float('inf')])
    torch.cuda.synchronize()
    assert int(w.flag.item()) == 2 and len(w.names) == 5
    # a bf16 launch never touches the word, whatever it stores
    w = A.RangeWatch(DEV)
    with A.watching(w):
        _bias_launch('bf16', [1e30])
        _bias_launch('split', [float('inf')])
    torch.cuda.synchronize()
    assert int(w.flag.item()) == -1


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: each limit of the header's paragraph returns its documented code

def _conv_rc(pc, *args, **kw):
    """act.conv3x3's esr_conv3x3 return code (act.conv3x3 raises on failure: its check is swapped for a recorder around the call)."""
    A = _A()
    rcs, saved = [], A.check
    A.check = lambda rc, what: rcs.append(rc)
    try:
        A.conv3x3(pc, *args, **kw)
    finally:
        A.check = saved
    torch.cuda.synchronize()
    assert len(rcs) == 1
    return rcs[0]


def _launch_rc(case, **over):
    """The return code of esr_conv3x3 for `case` with descriptor fields overridden."""
    c = case
    w, b, pc, _ = _weights(c)
    ncg1 = (c.cin + 7) // 8
    x1 = Buf(c.f, c.B, ncg1, c.H // c.ups, c.W // c.ups, fill='random')
    nout = (c.cout + 7) // 8
    kw = dict(upsample=c.ups, act_slope=c.act_slope, alpha=c.alpha, in1_lo_groups=c.in1_lo_groups)
    if c.lat:
        kw['in0'] = Buf(c.f, c.B, 1, c.H, c.W, fill='random').view()
    o = Buf(c.f, c.B, max(nout, 1) + 1, c.H, c.W)
    kw['out'] = o.view(0, nout)
    kw.update(over)
    return _conv_rc(pc, x1.view(), c.B, c.H, c.W, c.cout, **kw)


def test_refusals():
    base = Case(fmt='split', B=1, H=8, W=8, cin=16, cout=32)
    assert _launch_rc(base) == 0
    o = Buf('split', 1, 8, 8, 8)
    ps_out = Buf('split', 1, 2, 16, 16)
    for kw, want in [
        (dict(act_slope=-0.1), E_ARG), (dict(act_slope=1.5), E_ARG), (dict(alpha=float('nan')), E_ARG), (dict(alpha=-1.0), E_ARG),
        (dict(out=Buf('f16x2', 1, 4, 8, 8).view()), E_ARG),                           # out in another element format
        (dict(out=o.view(0, 3)), E_ARG),                                              # out.ncg * 8 < cout
        (dict(res1=Buf('split', 1, 4, 8, 8).view(0, 3), beta1=1.0), E_ARG),             # res1 covers too few groups
        (dict(res2=Buf('split', 1, 4, 8, 8).view(0, 2), beta2=1.0), E_ARG),
        (dict(mask_src=Buf('split', 1, 4, 8, 8).view(0, 1), mask_cg=(0, 3)), E_ARG),    # mask_src covers too few of the masked groups
        (dict(out_nchw=torch.zeros(32 * 64, device=DEV)), E_UNSUPPORTED),             # two destination kinds
        (dict(out2=Buf('split', 1, 4, 8, 8).view(0, 4)), 0),
        (dict(out=o.view(0, 4, lo=False), out2=Buf('split', 1, 4, 8, 8).view(0, 4)), E_ARG),   # out2 may drop a lo plane, not add one
        (dict(in1_lo_groups=-1), E_UNSUPPORTED),                                      # partial lo in bf16
        (dict(out=o.view(0, 4, lo=False)), E_UNSUPPORTED),                            # out.lo == NULL with hi+lo bf16 inputs
        (dict(upsample=2), E_ARG),                                                    # in1 is not H / upsample x W / upsample
        (dict(pixel_shuffle=2, out=ps_out.view(), out2=Buf('split', 1, 4, 8, 8).view()), E_UNSUPPORTED),     # pixel shuffle with out2
        (dict(pixel_shuffle=2, out=ps_out.view(), res1=Buf('split', 1, 4, 8, 8).view(), beta1=1.0), E_UNSUPPORTED),
        (dict(pixel_shuffle=2, out=ps_out.view(0, 1), ps_rowgroup0=1), E_ARG),          # row groups 1..4 need two shuffled groups
        (dict(pixel_shuffle=2, out=ps_out.view(0, 1)), 0),
        # epilogue combinations without a kernel (esr_hip.h): res2 without res1, out2 with a residual
        (dict(res2=Buf('split', 1, 4, 8, 8).view(), beta2=1.0), E_UNSUPPORTED),
        (dict(res1=Buf('split', 1, 4, 8, 8).view(), res2=Buf('split', 1, 4, 8, 8).view(), out2=Buf('split', 1, 4, 8, 8).view()), E_UNSUPPORTED),
    ]:
        assert _launch_rc(base, **kw) == want, kw
    # the upsample factor: 9 and above, and the factors whose source-coordinate division is not exact (test_upsample_factor_at_the_coordinate_limit)
    for ups in (5, 7, 9, 16):
        assert _launch_rc(Case(fmt='bf16', B=1, H=ups, W=2 * ups, cin=8, cout=8, ups=ups)) == E_UNSUPPORTED, ups
    # an image at the 2^15 coordinate limit
    assert _launch_rc(Case(fmt='bf16', B=1, H=1, W=32765, cin=8, cout=8)) == 0
    assert _launch_rc(Case(fmt='bf16', B=1, H=1, W=32766, cin=8, cout=8)) == E_UNSUPPORTED
    # cout = 96: neither <= 64 nor a multiple of 64; out_nchw with output slices; an out in another format
    pc = _weights(Case(fmt='bf16', cin=8, cout=64))[2]
    x = Buf('bf16', 1, 1, 4, 4, fill='random')
    assert _conv_rc(pc, x.view(), 1, 4, 4, 96, out=Buf('bf16', 1, 12, 4, 4).view()) == E_UNSUPPORTED
    assert _conv_rc(pc, x.view(), 1, 4, 4, 128, out_nchw=torch.zeros(128 * 16, device=DEV)) == E_UNSUPPORTED
    assert _conv_rc(pc, x.view(), 1, 4, 4, 8, out=Buf('f16', 1, 1, 4, 4).view()) == E_ARG
    # the fp16 formats have no RES1|MASK kernel (esr_conv3x3_desc: the data gradient of 'mixed' masks without a residual)
    assert _launch_rc(Case(fmt='f16x2', B=1, H=8, W=8, cin=16, cout=32), res1=Buf('f16x2', 1, 4, 8, 8).view(), beta1=1.0,
                      mask_src=Buf('f16', 1, 4, 8, 8).view(), mask_cg=(0, 4)) == E_UNSUPPORTED
