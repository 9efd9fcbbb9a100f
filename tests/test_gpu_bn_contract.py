"""The esr_bn_* contract (include/esr_hip.h, csrc/esr_critic.hip): BatchNorm + LeakyReLU, its gradient and the gradient of that gradient, every
entry point launched through the C-ABI and held to a float64 restatement of what it read.

Formulas (per statistics group g of B/groups images and channel c; N = (B/groups) H W; sc, sh, mu, rs, gm the STORED fp32 scale, shift, mean,
rstd, gamma as float64 — absent pointers read as 1, 0, 0, 1, 1; S, T the GIVEN double sums2, sums3; y, dz, u the STORED planes, hi + lo):

    pre = sc y + sh,   m = 1 if pre > 0 else slope,   dyb = dz m,   xh = (y - mu) rs,   k1 = gm rs
    reduce 0: (sum y, sum y^2)        reduce 1: (sum dyb, sum dyb xh)        reduce 2: (sum u, sum u xh, sum u dyb)
    apply 0 : z    = m pre
    apply 1 : dy   = k1 (dyb - S1/N - xh S2/N)                                         const_stats: sc dyb
    apply 2 : g_dz = m k1 (u - T1/N - xh T2/N)                                         const_stats: m sc u
              g_y  = -k1 rs (xh Q + (S2/N) uterm + (T2/N) dterm),  Q = T3/N - T1 S1/N^2 - T2 S2/N^2          const_stats: exactly 0
    finalize: mean = s/N, var = ss/N - mean^2 (>= 0), rstd = (var + eps)^-1/2, scale = gamma rstd, shift = beta - scale mean;
              running r <- (1 - mom) r + mom stat once per group, in order, the variance unbiased (N / (N - 1))
    param_grads: dgamma = sum_g S2, dbeta = sum_g S1, g_gamma = sum_g rstd (T3 - T1 S1/N - T2 S2/N)

Bounds (u = 2^-24, the fp32 unit roundoff).  None is fitted to an observed error; each test prints its worst |err| / bound.  On an MI355X the
worst ratios were: reduce 0.065, apply 0.997 and finalize 0.982 (a value that round-to-nearest leaves half a unit in the last place of the stored
format from its reference sits at 1 by construction), param_grads 0.905, chained 0.124 of the 2e-5 bar.

  reduce   |sum - ref| <= (L + 4) u sum|term|,  L = ceil(N / 256).  A thread adds at most ceil(N / (256 nsplit)) <= L terms into an fp32
           accumulator (L u sum|term| whatever nsplit is); the longest term, dyb xh = (dz m)((y - mu) rs), takes four fp32 roundings (4 u |term|);
           the fold and the atomics are fp64: 64 (the largest nsplit) roundings of 2^-53 (|s0| + sum|term|), added to the bound, s0 being the
           nonzero value the target held (the kernel adds).
  apply    |out - ref| <= r_fmt |ref| + k u M (+ 2^-25 for fp16, half its subnormal spacing).  r_fmt is store8's rounding (esr_common.h
           encode8): one plane keeps 8 (bf16) or 11 (fp16) significant bits, r = 2^-8 / 2^-11; split stores hi = bf16(v) and lo = bf16(v - hi),
           |v - hi| <= 2^-8 |v| and the residual is rounded to 8 bits again: r = 2^-16.  M is the sum of the magnitudes of the terms before
           they cancel, k the fp32 roundings on the longest path into one term, counted in bn_apply_kernel (fused multiply-adds only remove some):
             mode 0  k = 3   M = |sc y| + |sh|                      product, sum, slope product
             mode 1  k = 7   M = |k1| (|dyb| + |S1/N| + |xh S2/N|)  the xh S2/N term: xh 2, (float)(S2/N) 1, product 1, one subtraction (the first
                                                                    one does not involve it), times k1 (its own product 1, the result's 1)
                     const_stats: k = 2, M = |sc dyb|
             mode 2  out0: k = 8, M = |m k1| (|u| + |T1/N| + |xh T2/N|)   as mode 1 plus the m k1 product;  const_stats: k = 2, M = |m sc u|
                     out1: k = 13, M = |k1 rs| (|xh| Mq + |S2/N| Mu + |T2/N| Md), Mq = |T3/N| + |T1 S1|/N^2 + |T2 S2|/N^2, Mu, Md the M's of
                           uterm, dterm: the xh Q term takes xh 2, Q 5 (t1 1, s1 1, their product 1, two subtractions), the product 1, two
                           additions, and the prefactor -k1 rs its 3 (k1, k1 rs, the final product)
  finalize mean: 1 rounding; rstd: 1; scale: 2 (rstd, product); shift: k = 5 on M = |beta| + |scale mean| (scale 2, (float)mean 1, product 1,
           subtraction 1); running statistics after `groups` steps: 5 roundings a step (1 - mom, its product, the statistic's conversion, mom's
           product, the sum) on M = |r0| + mom sum_g |stat_g|, which bounds every intermediate value: k = 5 groups.  The fp64 part of both
           sides (ss/N - mean^2 cancels) adds 2^-48 kappa, kappa = (ss/N + mean^2) / (var + eps), relative.
  param_grads  one fp32 rounding of an fp64 sum: u |ref| + 2^-48 sum of the magnitudes of the terms.
  chained  relative L2 below 2e-5 against torch autograd in float64: the bar tests/test_gpu_critic.py holds for this comparison (split operands
           carry 16 significant bits).

Branch ties: the kernel picks the LeakyReLU branch by pre > 0 in fp32.  An element with |pre| <= 4 u (|sc y| + |sh|) in float64 is a tie: apply may
take either branch there, reduce's bound grows by (1 - slope) |dz| (|dz xh|, |dz u| for the sums that carry dyb).  Every case asserts that at most
1e-4 of its elements are ties (y uniform in (-1, 2), gamma in (0.5, 1.5), beta in (-0.5, 0.5) has none at these shapes on the CPU).

Buffers are laid out here (Act / place, after the Operand of tests/test_gpu_wgrad_contract.py, which has no image offset, no batch-strided
stacked view and no space-to-depth order): [planes][Bt][CG][H+2][W+2][8], or stacked [planes][CG][Bt][H+2][W+2][8] with batch stride one image.  EVERY word starts
as NaN; inputs then receive their interior values in the channels < C of the groups and images the launch addresses, so a read of a pad lane, of
a group in front of, between (space-to-depth) or behind the view's addressed groups, of an image outside [b0, b0 + B) or of a border reaches a result
as NaN.  Outputs stay all NaN: afterwards the addressed groups hold their interior, exact zeros in the pad lanes (the next conv multiplies them by
zero weights, and NaN * 0 is NaN) and exact zero bits in the whole one-pixel border (stacked: the rows between images included); every other word
keeps its NaN bits.  Before any call, span_ok recomputes from the view's own fields the smallest and largest vector offset the launch addresses
in it (voff's rule, border writes included) and asserts they lie inside the plane the view points into: no test relies on the library to stay
in bounds.

Planted errors (each must make the case's own check fail): group 0's statistics used for every group (test_reduce, test_apply: 'chunks'),
x&1 and y&1 swapped and the header's former 4 cg + s order in the space-to-depth store (test_apply s2d cases), the last 256-pixel chunk of a
plane dropped from a sum / left unwritten in an output ('chunks'), g_y without its T2 dterm term and g_dz without lrelu' (test_apply mode 2),
biased variance in running_var (test_finalize), a nonzero pad lane and a nonzero border vector (test_apply).

Which test reaches which instantiation (ids are fmt-case-mode; every fmt of split, bf16, f16):
    bn_reduce_kernel<0, false>                 test_reduce[*-small-0], [*-chunks-0] (nsplit 2: the paired loop plus its odd tail)
    bn_reduce_kernel<1, false>, <2, false>     test_reduce[*-small-1/2], [*-chunks-1/2], [*-eval-*], [*-noscale-*], [*-slope1-*]
    bn_reduce_kernel<1, true>, <2, true>       test_reduce[*-small_s2d-1/2], [*-chunks_s2d-1/2], [*-quad-*], [*-offset-*], [*-stacked-*]
    bn_apply_kernel<0, false, 1>, <0, true, 1> test_apply[*-small-0], [*-small_s2d-0], [*-quad-0], [*-offset-0], [*-stacked-0]
    bn_apply_kernel<1, false, 1>, <1, true, 1> test_apply[*-small-1], [*-small_s2d-1], [*-quad-1], [*-offset-1], [*-stacked-1]
    bn_apply_kernel<2, false, 1>, <2, true, 1> test_apply[*-small-2], [*-small_s2d-2], [*-quad-2], [*-offset-2], [*-stacked-2]
    bn_apply_kernel<0, false, 4>, <0, true, 4> test_apply[*-chunks-0], [*-chunks_s2d-0]       (hw = 1088: the second chunk has 64 live pixels)
    bn_apply_kernel<1, false, 4>, <1, true, 4> test_apply[*-chunks-1], [*-chunks_s2d-1]
    bn_apply_kernel<2, false, 2>, <2, true, 2> test_apply[*-chunks-2], [*-chunks_s2d-2]       (three chunks of 512, the last with 64 live)
    bn_apply_kernel<0, false, 1, true>, <0, true, 1, true>   test_finalize_apply[*-small], [*-small_s2d], [*-quad]
    bn_apply_kernel<0, false, 4, true>, <0, true, 4, true>   test_finalize_apply[*-chunks], [*-chunks_s2d]
    bn_finalize_kernel, bn_param_grads_kernel  test_finalize, test_param_grads, test_chain
    const_stats (eval affine; scale == NULL), slope 1      test_reduce / test_apply [*-eval-*], [*-noscale-*], [*-slope1-*]
    the nine launches in the critic's order, direct and as one esr_run list                    test_chain[plain], test_chain[s2d]
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN16 = 0x7FA5          # a NaN both as bf16 and as fp16
NAN64 = 0x7FF8DEADBEEF0001
TIE_CAP = 1e-4
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # what the library receives for eps = 1e-5f
MOM = float(torch.tensor(0.1, dtype=torch.float32))
WORST = {}              # family -> worst |err| / bound seen in this process (printed by every test that moves it)


class Fmt:
    def __init__(self, name, planes, vfmt, dtype, r, tiny):
        self.name, self.planes, self.vfmt, self.dtype, self.r, self.tiny = name, planes, vfmt, dtype, r, tiny


FMTS = {f.name: f for f in (Fmt('split', 2, 0, torch.bfloat16, 2.0 ** -16, 0.0), Fmt('bf16', 1, 0, torch.bfloat16, 2.0 ** -8, 0.0),
                            Fmt('f16', 1, 1, torch.float16, 2.0 ** -11, 2.0 ** -25))}


def _lib():
    from esr_hip import _lib as L
    return L


def _dev():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if torch.cuda.is_available() else None


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _note(family, ratio):
    if ratio > WORST.get(family, -1.0):
        WORST[family] = ratio
    print('[bn-contract] %s: worst |err|/bound of this test %.3g (so far %.3g)' % (family, ratio, WORST[family]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the layout

def gidx(cg, s):
    """Space-to-depth group of channel group cg at parity s = 2 (y & 1) + (x & 1): voff<true> of csrc/esr_critic.hip."""
    return 16 * (cg // 4) + 4 * s + cg % 4


def gidx_former(cg, s):
    """The order include/esr_hip.h used to document."""
    return 4 * cg + s


def groups_of(n, s2d, rule=gidx):
    return [rule(cg, s) for cg in range(n) for s in range(4)] if s2d else list(range(n))


class Act:
    """[planes][Bt][CG][H+2][W+2][8] 16-bit words (on the device stacked as [planes][CG][Bt][H+2][W+2][8]); `bits` is the host copy in the
    first order whatever the device order.  Every word is NaN until something is placed."""

    def __init__(self, fmt, Bt, CG, H, W, stacked=False):
        self.f, self.Bt, self.CG, self.H, self.W, self.stacked = FMTS[fmt], Bt, CG, H, W, stacked
        self.bits = torch.full((self.f.planes, Bt, CG, H + 2, W + 2, 8), NAN16, dtype=torch.int16)
        self.t = None

    def upload(self):
        b = self.bits.permute(0, 2, 1, 3, 4, 5) if self.stacked else self.bits
        self.t = b.contiguous().to(_dev())
        return self

    def download(self):
        b = self.t.cpu()
        return (b.permute(0, 2, 1, 3, 4, 5) if self.stacked else b).contiguous()

    def view(self, b0, cg0, ncg):
        """esr_act_view of `ncg` declared groups from group cg0, starting at image b0."""
        Hp, Wp = self.H + 2, self.W + 2
        bs, cs = (Hp * Wp, self.Bt * Hp * Wp) if self.stacked else (self.CG * Hp * Wp, Hp * Wp)
        hi = self.t.data_ptr() + (b0 * bs + cg0 * cs) * 16
        lo = hi + self.t.stride(0) * 2 if self.f.planes == 2 else None
        return _lib().ActView(hi, lo, ncg, self.H, self.W, bs, cs, self.f.vfmt)


def place(act, vals, b0, cg0, s2d):
    """Logical float64 [B][nch][H][W] into the interior of the groups a launch addresses, rounded to the format (split: hi + the residue)."""
    B, nch, H, W = vals.shape
    hi = vals.to(act.f.dtype)
    planes = [hi] + ([(vals - hi.double()).to(act.f.dtype)] if act.f.planes == 2 else [])
    for p, v in enumerate(planes):
        w = v.view(torch.int16)
        for cg in range((nch + 7) // 8):
            ne = min(8, nch - 8 * cg)
            blk = w[:, 8 * cg:8 * cg + ne]
            if s2d:
                for s in range(4):
                    act.bits[p, b0:b0 + B, cg0 + gidx(cg, s), 1:-1, 1:-1, :ne] = blk[:, :, s >> 1::2, s & 1::2].permute(0, 2, 3, 1)
            else:
                act.bits[p, b0:b0 + B, cg0 + cg, 1:-1, 1:-1, :ne] = blk.permute(0, 2, 3, 1)


def fetch(bits, B, n, H, W, b0, cg0, s2d, rule=gidx, swap=False):
    """The words of the logical pixels, all 8 lanes of each of the n groups: int16 [planes][B][8 n][H][W].  rule / swap: planted layouts."""
    out = torch.empty(bits.shape[0], B, 8 * n, H, W, dtype=torch.int16)
    for cg in range(n):
        if s2d:
            for s in range(4):
                py, px = (s & 1, s >> 1) if swap else (s >> 1, s & 1)
                out[:, :, 8 * cg:8 * cg + 8, py::2, px::2] = bits[:, b0:b0 + B, cg0 + rule(cg, s), 1:-1, 1:-1, :].permute(0, 1, 4, 2, 3)
        else:
            out[:, :, 8 * cg:8 * cg + 8] = bits[:, b0:b0 + B, cg0 + cg, 1:-1, 1:-1, :].permute(0, 1, 4, 2, 3)
    return out


def decode(raw, f):
    """hi + lo in float64."""
    return raw.contiguous().view(f.dtype).double().sum(0)


def span_ok(act, v, B, n, s2d, border, declared=True):
    """The smallest and largest vector offset a launch over B images and n channel groups addresses in view v (the kernel's voff rule; with
    `border` the zero border it writes around every addressed plane), computed from the view's fields, must lie inside the plane of the
    backing tensor that the view points into."""
    base = v.hi - act.t.data_ptr()
    assert base % 16 == 0
    base //= 16
    gs = groups_of(n, s2d)
    if declared:
        assert v.ncg > max(gs), 'the view declares fewer groups than the launch addresses'
    P = v.W + 2
    first = 0 if border else P + 1
    last = (v.H + 1) * P + v.W + 1 if border else v.H * P + v.W
    lo_ = base + min(gs) * v.cg_stride + first
    hi_ = base + (B - 1) * v.batch_stride + max(gs) * v.cg_stride + last
    plane = act.t.numel() // 8 // act.f.planes
    assert 0 <= lo_ and hi_ < plane, 'the launch would leave its buffer: vectors [%d, %d] of a plane of %d' % (lo_, hi_, plane)
    if v.lo:
        assert v.lo - v.hi == plane * 16


def check_out(bits, f, B, C_, H, W, b0, cg0, s2d):
    """What esr_bn_apply must leave in an all-NaN buffer besides the values: zero pad lanes, zero borders, nothing else touched."""
    n = (C_ + 7) // 8
    gs = [cg0 + g for g in groups_of(n, s2d)]
    mine = torch.zeros(bits.shape[1:5], dtype=torch.bool)
    mine[b0:b0 + B, gs] = True
    assert (bits[:, ~mine] == NAN16).all(), 'a word outside the addressed groups and images was written'
    own = bits[:, b0:b0 + B][:, :, gs]
    edge = torch.ones(own.shape[3:5], dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    assert (own[:, :, :, edge] == 0).all(), 'a border vector of a written group is not zero bits'
    if C_ % 8:
        last = [cg0 + g for g in (groups_of(n, s2d)[-4:] if s2d else [n - 1])]
        assert (bits[:, b0:b0 + B][:, :, last][:, :, :, 1:-1, 1:-1, C_ % 8:] == 0).all(), 'a pad lane of the partial last group is not an exact zero'


def excess(got, ref, bound, alt=None, alt_bound=None):
    """max |got - ref| / bound (0 where equal, inf where NaN); with `alt`, each element may meet either reference."""
    def one(r, b):
        err = (got - r).abs()
        e = err / b
        e[err == 0] = 0.0
        e[torch.isnan(e)] = float('inf')
        return e
    e = one(ref, bound)
    if alt is not None:
        e = torch.minimum(e, one(alt, alt_bound))
    return float(e.max()) if e.numel() else 0.0


def _f32(t):
    return None if t is None else t.to(torch.float32).contiguous().to(_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def guarded(vals):
    """A double array between 64 NaN guard words: (tensor, pointer to the payload, payload slice)."""
    n = vals.numel()
    t = torch.full((n + 128,), NAN64, dtype=torch.int64)
    t[64:64 + n] = vals.reshape(-1).double().view(torch.int64)
    t = t.to(_dev())
    return t, t.data_ptr() + 64 * 8, slice(64, 64 + n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one case: operands, parameters, the float64 restatement

SHAPES = {
    # name: B, groups, C, H, W, s2d, extra
    'small': (4, 2, 12, 6, 10, False, {}),
    'small_s2d': (4, 2, 12, 6, 10, True, {}),
    'chunks': (16, 2, 12, 34, 32, False, {}),
    'chunks_s2d': (16, 2, 12, 34, 32, True, {}),
    'quad': (6, 3, 40, 8, 12, True, {}),
    'offset': (4, 2, 40, 8, 12, True, dict(Bt=8, b0=2)),
    'stacked': (4, 2, 32, 8, 8, True, dict(stacked=True)),
    'eval': (4, 2, 12, 6, 10, False, dict(const='eval')),
    'noscale': (4, 2, 12, 6, 10, True, dict(const='noscale')),
    'slope1': (4, 2, 12, 6, 10, False, dict(slope=1.0)),
}


class Case:
    def __init__(self, fmt, B, groups, C_, H, W, s2d=False, Bt=None, b0=0, stacked=False, const=None, slope=0.2, seed=0, const_channel=None):
        self.fmt, self.f = fmt, FMTS[fmt]
        self.B, self.groups, self.C, self.H, self.W, self.s2d = B, groups, C_, H, W, s2d
        self.Bt, self.b0, self.stacked, self.const = Bt or B, b0, stacked, const
        self.slope = float(torch.tensor(slope, dtype=torch.float32))
        self.n, self.Bg, self.N = (C_ + 7) // 8, B // groups, (B // groups) * H * W
        self.cg0, self.behind = 1, 1
        g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * C_ + H + 3 * W + groups)
        rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
        yv = rand(B, C_, H, W) * 3 - 1
        self.beta = (rand(C_) - 0.5).float()
        if const_channel is not None:
            yv[:, const_channel] = 0.5
            self.beta[const_channel] = 0.375
        self.y_act = self.new_input(yv, False)
        self.dz_act = self.new_input(rand(B, C_, H, W) * 2 - 1, s2d)
        self.u_act = self.new_input(rand(B, C_, H, W) * 2 - 1, False)
        self.y, self.dz, self.u = self.stored(self.y_act, False), self.stored(self.dz_act, s2d), self.stored(self.u_act, False)
        self.gamma = (rand(C_) + 0.5).float()
        yg = self.y.view(groups, self.Bg, C_, H, W)
        mean, var = yg.mean((1, 3, 4)), yg.var((1, 3, 4), unbiased=False)
        self.scale = self.shift = self.mean = self.rstd = None
        if const is None:
            self.mean, self.rstd = mean.float(), (var + EPS).rsqrt().float()
            self.scale = self.gamma * self.rstd
            self.shift = self.beta - self.scale * self.mean
        elif const == 'eval':          # running statistics (one set per group, so that a group mix-up shows)
            rm, rv = rand(groups, C_) * 0.6 + 0.2, rand(groups, C_) + 0.5
            self.scale = (self.gamma.double() / (rv + EPS).sqrt()).float()
            self.shift = (self.beta.double() - self.scale.double() * rm).float()
        else:
            self.gamma = None
        self.d_scale, self.d_shift, self.d_mean, self.d_rstd, self.d_gamma = map(_f32, (self.scale, self.shift, self.mean, self.rstd, self.gamma))
        self.g0_everywhere = False     # planted: group 0's parameters for every group
        # the sums of the backward passes, as the library is given them
        r = self.terms()
        self.sums2 = self.gsum([r['dyb'], r['dyb'] * r['xh']])
        self.sums3 = self.gsum([self.u, self.u * r['xh'], self.u * r['dyb']])
        self.d_sums2, self.d_sums3 = self.sums2.to(_dev()), self.sums3.to(_dev())
        ties = float(r['tie'].double().mean())
        assert ties <= TIE_CAP, 'more than 1e-4 of the elements are LeakyReLU ties: %g' % ties

    # -- buffers
    def geometry(self, s2d):
        need = max(groups_of(self.n, s2d)) + 1
        H, W = (self.H // 2, self.W // 2) if s2d else (self.H, self.W)
        return need, H, W

    def new_act(self, s2d):
        need, H, W = self.geometry(s2d)
        return Act(self.fmt, self.Bt, self.cg0 + need + self.behind, H, W, self.stacked)

    def new_input(self, vals, s2d):
        a = self.new_act(s2d)
        place(a, vals, self.b0, self.cg0, s2d)
        return a.upload()

    def new_output(self, s2d):
        return self.new_act(s2d).upload()

    def stored(self, act, s2d, bits=None, **kw):
        raw = fetch(act.bits if bits is None else bits, self.B, self.n, self.H, self.W, self.b0, self.cg0, s2d, **kw)
        return decode(raw, self.f)[:, :self.C]

    def view(self, act, s2d, border):
        v = act.view(self.b0, self.cg0, self.geometry(s2d)[0])
        span_ok(act, v, self.B, self.n, s2d, border)
        return v

    def desc(self, dz=False, u=False, out0=None, out0_s2d=False, out1=None):
        d = _lib().BnDesc()
        d.y = self.view(self.y_act, False, False)
        if dz:
            d.dz = self.view(self.dz_act, self.s2d, False)
        if u:
            d.u = self.view(self.u_act, False, False)
        if out0 is not None:
            d.out0 = self.view(out0, out0_s2d, True)
        if out1 is not None:
            d.out1 = self.view(out1, False, True)
        d.B, d.groups, d.C = self.B, self.groups, self.C
        d.scale, d.shift, d.mean, d.rstd, d.gamma = map(_ptr, (self.d_scale, self.d_shift, self.d_mean, self.d_rstd, self.d_gamma))
        d.sums2, d.sums3 = self.d_sums2.data_ptr(), self.d_sums3.data_ptr()
        d.slope, d.const_stats, d.s2d = self.slope, 1 if self.const else 0, 1 if self.s2d else 0
        return d

    # -- float64
    def per(self, t, fill):
        """A [groups][C] (or [C]) fp32 parameter as float64 [B][C][1][1]; an absent one reads as `fill`."""
        if t is None:
            return torch.full((1, 1, 1, 1), fill, dtype=torch.float64)
        t = t.double()
        if t.dim() == 1:
            return t.view(1, -1, 1, 1)
        if self.g0_everywhere:
            t = t[:1].expand_as(t)
        return t.repeat_interleave(self.Bg, 0)[:, :, None, None]

    def terms(self, flip=False):
        sc, sh, mu, rs = self.per(self.scale, 1.0), self.per(self.shift, 0.0), self.per(self.mean, 0.0), self.per(self.rstd, 1.0)
        pre = sc * self.y + sh
        mag = (sc * self.y).abs() + sh.abs()
        tie = pre.abs() <= 4 * U * mag
        pos = pre > 0
        if flip:
            pos = pos ^ tie
        m = torch.where(pos, torch.tensor(1.0, dtype=torch.float64), torch.tensor(self.slope, dtype=torch.float64))
        return dict(sc=sc, sh=sh, mu=mu, rs=rs, pre=pre, mag=mag, tie=tie, m=m, dyb=self.dz * m, xh=(self.y - mu) * rs,
                    k1=self.per(self.gamma, 1.0) * rs)

    def gsum(self, ts, keep=None):
        """[groups][C][K] group sums; keep: a [H][W] mask of the pixels that count (planted)."""
        out = []
        for t in ts:
            t = t.expand(self.B, self.C, self.H, self.W)
            if keep is not None:
                t = t * keep
            out.append(t.reshape(self.groups, self.Bg, self.C, self.H, self.W).sum((1, 3, 4)))
        return torch.stack(out, -1).contiguous()

    def reduce_ref(self, mode, keep=None):
        """(sums, sum |term|, the widening for ties) as [groups][C][K]."""
        r = self.terms()
        y, u, dyb, xh = self.y, self.u, r['dyb'], r['xh']
        ts = [[y, y * y], [dyb, dyb * xh], [u, u * xh, u * dyb]][mode]
        w = (1 - self.slope) * self.dz.abs() * r['tie']
        z = torch.zeros_like(y)
        ws = [[z, z], [w, w * xh.abs()], [z, z, w * u.abs()]][mode]
        return self.gsum(ts, keep), self.gsum([t.abs() for t in ts]), self.gsum(ws)

    def apply_ref(self, mode, flip=False, no_t2_dterm=False, no_lrelu=False, scale=None, shift=None):
        """[(ref, bound)] of out0 (and out1) as [B][C][H][W]; flip: the other branch at every tie; scale / shift: stored results to use
        (esr_bn_finalize_apply); no_*: planted."""
        r = self.terms(flip)
        if scale is not None:
            keep = self.scale, self.shift
            self.scale, self.shift = scale, shift
            r = self.terms(flip)
            self.scale, self.shift = keep
        f, m, y, u, dyb, xh, k1, sc, rs = self.f, r['m'], self.y, self.u, r['dyb'], r['xh'], r['k1'], r['sc'], r['rs']
        bd = lambda ref, k, M: f.r * ref.abs() + k * U * M + f.tiny
        if mode == 0:
            ref = m * r['pre']
            return [(ref, bd(ref, 3, r['mag']))]
        mm = torch.ones_like(m) if no_lrelu else m
        if self.const:
            if mode == 1:
                ref = sc * dyb
                return [(ref, bd(ref, 2, ref.abs()))]
            ref = mm * sc * u
            z = torch.zeros_like(ref)
            return [(ref, bd(ref, 2, ref.abs())), (z, z)]
        N = float(self.N)
        S1, S2 = (self.per(self.sums2[..., i], 0.0) / N for i in range(2))
        T1, T2, T3 = (self.per(self.sums3[..., i], 0.0) / N for i in range(3))
        dterm, Md = dyb - S1 - xh * S2, dyb.abs() + S1.abs() + (xh * S2).abs()
        if mode == 1:
            ref = k1 * dterm
            return [(ref, bd(ref, 7, k1.abs() * Md))]
        uterm, Mu = u - T1 - xh * T2, u.abs() + T1.abs() + (xh * T2).abs()
        Q, Mq = T3 - T1 * S1 - T2 * S2, T3.abs() + (T1 * S1).abs() + (T2 * S2).abs()
        ref0 = mm * k1 * uterm
        ref1 = -k1 * rs * (xh * Q + S2 * uterm + (0 if no_t2_dterm else T2 * dterm))
        M1 = (k1 * rs).abs() * (xh.abs() * Mq + S2.abs() * Mu + T2.abs() * Md)
        return [(ref0, bd(ref0, 8, (m * k1).abs() * Mu)), (ref1, bd(ref1, 13, M1))]


def make_case(fmt, name, **kw):
    B, groups, C_, H, W, s2d, extra = SHAPES[name]
    return Case(fmt, B, groups, C_, H, W, s2d=s2d, **dict(extra, **kw))


def last_chunk(H, W):
    """[H][W] mask without the last 256-pixel chunk of the plane."""
    keep = torch.ones(H * W, dtype=torch.float64)
    keep[(H * W - 1) // 256 * 256:] = 0
    return keep.view(H, W)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. each entry point alone

CASES = list(SHAPES)
FMT_NAMES = list(FMTS)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('fmt', FMT_NAMES)
def test_reduce(fmt, name, mode):
    """esr_bn_reduce: every sums[g][c][k] against the float64 sum of the same terms, added to what the target held."""
    c = make_case(fmt, name)
    K = 3 if mode == 2 else 2
    gen = torch.Generator().manual_seed(5)
    s0 = torch.rand(c.groups, c.C, K, generator=gen, dtype=torch.float64) + 0.5
    t, p, sl = guarded(s0)
    before = t.clone()
    assert _lib().load_library().esr_bn_reduce(C.byref(c.desc(dz=mode >= 1, u=mode == 2)), mode, p, _stream()) == 0
    _sync()
    after = t.cpu()
    guard = torch.ones(t.numel(), dtype=torch.bool)
    guard[sl] = False
    assert torch.equal(after[guard], before.cpu()[guard]), 'a word outside sums[groups][C][K] was written (a channel >= C?)'
    got = after[sl].view(torch.float64).view(c.groups, c.C, K)
    ref, mag, widen = c.reduce_ref(mode)
    Lc = -(-c.N // 256)
    bound = (Lc + 4) * U * mag + widen + 64 * 2.0 ** -53 * (s0.abs() + mag)
    e = excess(got, s0 + ref, bound)
    _note('reduce', e)
    assert e <= 1.0, 'esr_bn_reduce mode %d: worst |sum - ref| / bound = %.3g' % (mode, e)
    assert float((got - s0).abs().max()) > 0
    # planted errors
    assert excess(got, ref, bound) > 1.0, 'the comparator accepts a target that was overwritten, not added to'
    if name.startswith('chunks'):
        assert excess(got, s0 + c.reduce_ref(mode, keep=last_chunk(c.H, c.W))[0], bound) > 1.0, 'planted: last 256-pixel chunk dropped from the sum'
        if mode >= 1:
            c.g0_everywhere = True
            bad = c.reduce_ref(mode)[0]
            c.g0_everywhere = False
            assert excess(got, s0 + bad, bound) > 1.0, "planted: group 0's statistics used for group 1"


def _check_apply(c, mode, outs, refs, alts, what):
    """outs: [(Act, s2d)]; refs / alts: apply_ref()'s lists.  Returns the decoded results and the bits."""
    worst, res = 0.0, []
    for (act, s2d), (ref, bd), (alt, abd) in zip(outs, refs, alts):
        bits = act.download()
        check_out(bits, c.f, c.B, c.C, *c.geometry(s2d)[1:], c.b0, c.cg0, s2d)
        got = c.stored(act, s2d, bits=bits)
        worst = max(worst, excess(got, ref, bd, alt, abd))
        res.append((got, bits))
    _note('apply', worst)
    assert worst <= 1.0, '%s mode %d: worst |out - ref| / bound = %.3g' % (what, mode, worst)
    return res


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('fmt', FMT_NAMES)
def test_apply(fmt, name, mode):
    """esr_bn_apply: every interior element against the header's formulas; pad lanes, borders and everything outside the addressed groups."""
    c = make_case(fmt, name)
    o0 = c.new_output(c.s2d and mode != 1)
    o1 = c.new_output(False) if mode == 2 else None
    s0 = c.s2d and mode != 1
    d = c.desc(dz=mode >= 1, u=mode == 2, out0=o0, out0_s2d=s0, out1=o1)
    assert _lib().load_library().esr_bn_apply(C.byref(d), mode, _stream()) == 0
    _sync()
    outs = [(o0, s0)] + ([(o1, False)] if mode == 2 else [])
    refs, alts = c.apply_ref(mode), c.apply_ref(mode, flip=True)
    res = _check_apply(c, mode, outs, refs, alts, 'apply')
    if mode == 2 and c.const:
        raw = fetch(res[1][1], c.B, c.n, c.H, c.W, c.b0, c.cg0, False)
        assert (raw == 0).all(), 'const_stats: out1 must be exact zeros'
    # planted errors
    got0, bits0 = res[0]
    ref0, bd0 = refs[0]
    if s0:
        assert excess(c.stored(o0, True, bits=bits0, swap=True), ref0, bd0) > 1.0, 'planted: x&1 and y&1 swapped in the space-to-depth order'
        assert excess(c.stored(o0, True, bits=bits0, rule=gidx_former), ref0, bd0) > 1.0, "planted: the header's former 4 cg + s order"
    if name.startswith('chunks'):
        c.g0_everywhere = True
        bad = c.apply_ref(mode)
        c.g0_everywhere = False
        assert excess(got0, bad[0][0], bd0) > 1.0, "planted: group 0's statistics used for group 1"
        hole = got0.clone()
        hole[:, :, last_chunk(c.H, c.W) == 0] = float('nan')
        assert excess(hole, ref0, bd0) > 1.0, 'planted: last 256-pixel chunk left unwritten'
    if mode == 2 and not c.const:
        assert excess(res[1][0], c.apply_ref(2, no_t2_dterm=True)[1][0], refs[1][1]) > 1.0, 'planted: g_y without its T2 dterm term'
        if c.slope != 1.0:
            assert excess(got0, c.apply_ref(2, no_lrelu=True)[0][0], bd0) > 1.0, "planted: g_dz without lrelu'"
    geo = (c.f, c.B, c.C) + c.geometry(s0)[1:] + (c.b0, c.cg0, s0)
    if c.C % 8:
        bad = bits0.clone()
        g_last = c.cg0 + groups_of(c.n, s0)[-1]
        bad[0, c.b0, g_last, 2, 2, 7] = 0x3C00
        with pytest.raises(AssertionError, match='pad lane'):
            check_out(bad, *geo)
    bad = bits0.clone()
    bad[-1, c.b0 + c.B - 1, c.cg0, -1, 3, 0] = 1
    with pytest.raises(AssertionError, match='border'):
        check_out(bad, *geo)
    bad = bits0.clone()
    bad[0, c.b0, 0, 1, 1, 0] = 0
    with pytest.raises(AssertionError, match='outside'):
        check_out(bad, *geo)


# -- finalize

def finalize_ref(sums, N, gamma, beta, rm0, rv0, biased=False):
    """float64 statistics of [groups][C][2] sums and their bounds: dict name -> (ref, bound)."""
    s, ss = sums[..., 0], sums[..., 1]
    mean = s / N
    raw = ss / N - mean * mean
    var = raw.clamp_min(0.0)
    kappa = (ss / N + mean * mean) / (var + EPS)
    d64 = 2.0 ** -48 * kappa
    rstd = (var + EPS).rsqrt()
    gm, bt = gamma.double(), beta.double()
    scale = gm * rstd
    shift = bt - scale * mean
    out = dict(mean=(mean, U * mean.abs() + 2.0 ** -48 * (s / N).abs()), rstd=(rstd, (U + d64) * rstd),
               scale=(scale, (2 * U + d64) * scale.abs()), shift=(shift, (5 * U + d64) * (bt.abs() + (scale * mean).abs())))
    G = sums.shape[0]
    unb = var if biased else var * N / (N - 1)
    for name, r0, stat in (('running_mean', rm0, mean), ('running_var', rv0, unb)):
        r, M = r0.double().clone(), r0.double().abs()
        for g in range(G):
            r = (1 - MOM) * r + MOM * stat[g]
            M = M + MOM * stat[g].abs()
        out[name] = (r, 5 * G * U * M + 2.0 ** -48 * kappa.max(0).values * M)
    return out


def _fin_outputs(G, C_):
    nanf = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=_dev())
    return dict(mean=nanf(G, C_), rstd=nanf(G, C_), scale=nanf(G, C_), shift=nanf(G, C_))


def _check_finalize(outs, run, ref, family='finalize'):
    worst = 0.0
    for k, t in list(outs.items()) + list(run.items()):
        e = excess(t.cpu().double(), ref[k][0], ref[k][1])
        assert e <= 1.0, '%s: worst |got - float64| / bound = %.3g' % (k, e)
        worst = max(worst, e)
    _note(family, worst)


def _y_sums(c):
    return c.gsum([c.y, c.y * c.y])


def test_finalize():
    """esr_bn_finalize over groups = 3 from float64 sums: statistics of every group, the running statistics' recurrence in order (unbiased
    variance, momentum 0.1, from non-trivial values), NULL running pointers, and a constant channel (variance exactly 0)."""
    lib = _lib().load_library()
    c = make_case('split', 'quad', const_channel=5)
    G, Cc = c.groups, c.C
    sums = _y_sums(c)
    d_sums = sums.to(_dev())
    gen = torch.Generator().manual_seed(11)
    rm0, rv0 = torch.rand(Cc, generator=gen) - 0.5, torch.rand(Cc, generator=gen) + 0.5
    gamma, beta = c.gamma, c.beta
    dg, db = _f32(gamma), _f32(beta)
    outs, run = _fin_outputs(G, Cc), dict(running_mean=rm0.clone().to(_dev()), running_var=rv0.clone().to(_dev()))
    args = lambda o, r: (d_sums.data_ptr(), G, Cc, c.N, EPS, MOM, dg.data_ptr(), db.data_ptr(), o['mean'].data_ptr(), o['rstd'].data_ptr(),
                         o['scale'].data_ptr(), o['shift'].data_ptr(), _ptr(r.get('running_mean')), _ptr(r.get('running_var')), _stream())
    assert lib.esr_bn_finalize(*args(outs, run)) == 0
    _sync()
    ref = finalize_ref(sums, c.N, gamma, beta, rm0, rv0)
    _check_finalize(outs, run, ref)
    assert (sums[:, 5, 1] / c.N - (sums[:, 5, 0] / c.N) ** 2 == 0).all()
    assert torch.equal(outs['rstd'][:, 5].cpu(), torch.full((G,), 1.0 / math.sqrt(EPS), dtype=torch.float64).float()), 'constant channel: rstd = 1/sqrt(eps)'
    # planted: biased variance in running_var; group 0's statistics for every group
    bad = finalize_ref(sums, c.N, gamma, beta, rm0, rv0, biased=True)
    assert excess(run['running_var'].cpu().double(), bad['running_var'][0], ref['running_var'][1]) > 1.0, 'planted: biased variance in running_var'
    assert excess(outs['mean'].cpu().double(), ref['mean'][0][:1].expand(G, Cc), ref['mean'][1]) > 1.0, "planted: group 0's mean for every group"
    # running pointers NULL: accepted, the same statistics
    outs2 = _fin_outputs(G, Cc)
    assert lib.esr_bn_finalize(*args(outs2, {})) == 0
    _sync()
    for k in outs:
        assert torch.equal(outs[k], outs2[k]), k


FIN_CASES = ['small', 'small_s2d', 'chunks', 'chunks_s2d', 'quad']


@pytest.mark.parametrize('name', FIN_CASES)
@pytest.mark.parametrize('fmt', FMT_NAMES)
def test_finalize_apply(fmt, name):
    """esr_bn_finalize_apply: the statistics of every group and the running statistics (moved once, by one block, not once per block) as
    esr_bn_finalize's, and out0 to the mode-0 bound with the scale / shift the launch stored."""
    L = _lib()
    lib = L.load_library()
    c = make_case(fmt, name)
    G, Cc = c.groups, c.C
    sums = _y_sums(c)
    d_sums = sums.to(_dev())
    gen = torch.Generator().manual_seed(12)
    rm0, rv0 = torch.rand(Cc, generator=gen) - 0.5, torch.rand(Cc, generator=gen) + 0.5
    dg, db = _f32(c.gamma), _f32(c.beta)
    outs, run = _fin_outputs(G, Cc), dict(running_mean=rm0.clone().to(_dev()), running_var=rv0.clone().to(_dev()))
    o0 = c.new_output(c.s2d)
    d = c.desc(out0=o0, out0_s2d=c.s2d)
    d.scale = d.shift = d.mean = d.rstd = None            # not read: the launch derives them
    f = L.CmdBnFinalize(d_sums.data_ptr(), G, Cc, c.N, EPS, MOM, dg.data_ptr(), db.data_ptr(), outs['mean'].data_ptr(), outs['rstd'].data_ptr(),
                        outs['scale'].data_ptr(), outs['shift'].data_ptr(), run['running_mean'].data_ptr(), run['running_var'].data_ptr())
    assert lib.esr_bn_finalize_apply(C.byref(d), C.byref(f), _stream()) == 0
    _sync()
    _check_finalize(outs, run, finalize_ref(sums, c.N, c.gamma, c.beta, rm0, rv0))
    sc, sh = outs['scale'].cpu(), outs['shift'].cpu()
    refs, alts = c.apply_ref(0, scale=sc, shift=sh), c.apply_ref(0, flip=True, scale=sc, shift=sh)
    _check_apply(c, 0, [(o0, c.s2d)], refs, alts, 'finalize_apply out0')


def test_param_grads():
    """esr_bn_param_grads over groups = 3 from given sums, against float64; any output may be NULL."""
    lib = _lib().load_library()
    c = make_case('split', 'quad')
    G, Cc, N = c.groups, c.C, float(c.N)
    S, T, rs = c.sums2, c.sums3, c.rstd.double()
    ref = dict(dgamma=S[..., 1].sum(0), dbeta=S[..., 0].sum(0),
               g_gamma=(rs * (T[..., 2] - T[..., 0] * S[..., 0] / N - T[..., 1] * S[..., 1] / N)).sum(0))
    mag = dict(dgamma=S[..., 1].abs().sum(0), dbeta=S[..., 0].abs().sum(0),
               g_gamma=(rs * (T[..., 2].abs() + (T[..., 0] * S[..., 0]).abs() / N + (T[..., 1] * S[..., 1]).abs() / N)).sum(0))
    names = ('dgamma', 'dbeta', 'g_gamma')
    worst = 0.0
    for present in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        out = {k: torch.full((Cc,), float('nan'), dtype=torch.float32, device=_dev()) for k in names}
        ptrs = [out[k].data_ptr() if p else None for k, p in zip(names, present)]
        s3 = c.d_sums3.data_ptr() if present[2] else None
        assert lib.esr_bn_param_grads(c.d_sums2.data_ptr(), s3, c.d_rstd.data_ptr() if present[2] else None, G, Cc, c.N, *ptrs, _stream()) == 0
        _sync()
        for k, p in zip(names, present):
            if not p:
                assert torch.isnan(out[k]).all(), '%s is NULL in this call, but its array of another call changed' % k
                continue
            e = excess(out[k].cpu().double(), ref[k], U * ref[k].abs() + 2.0 ** -48 * mag[k])
            assert e <= 1.0, '%s: worst |got - float64| / bound = %.3g' % (k, e)
            worst = max(worst, e)
    _note('param_grads', worst)
    assert excess(out['dgamma'].cpu().double(), S[0, :, 1], U * ref['dgamma'].abs() + 2.0 ** -48 * mag['dgamma']) > 1.0, 'planted: group 0 only'


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. the flow as the critic chains it

def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


class Chain:
    """reduce 0 -> finalize -> apply 0 -> reduce 1 -> param_grads -> apply 1 -> reduce 2 -> param_grads -> apply 2 on one case's operands,
    with its own outputs; `cmds()` are the nine launches as esr_cmd entries, `direct()` the same nine C calls."""

    def __init__(self, c):
        self.c = c
        G, Cc = c.groups, c.C
        dev = _dev()
        self.sums = [torch.zeros(G, Cc, k, dtype=torch.float64, device=dev) for k in (2, 2, 3)]
        self.stat = _fin_outputs(G, Cc)
        self.pg = {k: torch.full((Cc,), float('nan'), dtype=torch.float32, device=dev) for k in ('dgamma', 'dbeta', 'g_gamma')}
        self.z, self.dy, self.g_dz, self.g_y = c.new_output(c.s2d), c.new_output(False), c.new_output(c.s2d), c.new_output(False)
        self.gamma, self.beta = _f32(c.gamma), _f32(c.beta)

    def desc(self, **kw):
        d = self.c.desc(**kw)
        d.scale, d.shift, d.mean, d.rstd = (self.stat[k].data_ptr() for k in ('scale', 'shift', 'mean', 'rstd'))
        d.gamma, d.sums2, d.sums3 = self.gamma.data_ptr(), self.sums[1].data_ptr(), self.sums[2].data_ptr()
        return d

    def cmds(self):
        L, c, st = _lib(), self.c, self.stat
        fin = L.CmdBnFinalize(self.sums[0].data_ptr(), c.groups, c.C, c.N, EPS, MOM, self.gamma.data_ptr(), self.beta.data_ptr(), st['mean'].data_ptr(),
                              st['rstd'].data_ptr(), st['scale'].data_ptr(), st['shift'].data_ptr(), None, None)
        pg1 = L.CmdBnParamGrads(self.sums[1].data_ptr(), None, None, c.groups, c.C, c.N, self.pg['dgamma'].data_ptr(), self.pg['dbeta'].data_ptr(), None)
        pg2 = L.CmdBnParamGrads(self.sums[1].data_ptr(), self.sums[2].data_ptr(), st['rstd'].data_ptr(), c.groups, c.C, c.N, None, None,
                                self.pg['g_gamma'].data_ptr())
        s = c.s2d
        return [(L.OP_BN_REDUCE, L.CmdBn(self.desc(), 0, self.sums[0].data_ptr())),
                (L.OP_BN_FINALIZE, fin),
                (L.OP_BN_APPLY, L.CmdBn(self.desc(out0=self.z, out0_s2d=s), 0, None)),
                (L.OP_BN_REDUCE, L.CmdBn(self.desc(dz=True), 1, self.sums[1].data_ptr())),
                (L.OP_BN_PARAM_GRADS, pg1),
                (L.OP_BN_APPLY, L.CmdBn(self.desc(dz=True, out0=self.dy), 1, None)),
                (L.OP_BN_REDUCE, L.CmdBn(self.desc(dz=True, u=True), 2, self.sums[2].data_ptr())),
                (L.OP_BN_PARAM_GRADS, pg2),
                (L.OP_BN_APPLY, L.CmdBn(self.desc(dz=True, u=True, out0=self.g_dz, out0_s2d=s, out1=self.g_y), 2, None))]

    def direct(self):
        L = _lib()
        lib = L.load_library()
        st = _stream()
        for op, m in self.cmds():
            if op == L.OP_BN_REDUCE:
                rc = lib.esr_bn_reduce(C.byref(m.d), m.mode, m.sums, st)
            elif op == L.OP_BN_APPLY:
                rc = lib.esr_bn_apply(C.byref(m.d), m.mode, st)
            elif op == L.OP_BN_FINALIZE:
                rc = lib.esr_bn_finalize(m.sums, m.groups, m.C, m.n_per_group, m.eps, m.momentum, m.gamma, m.beta, m.mean, m.rstd, m.scale, m.shift,
                                         m.running_mean, m.running_var, st)
            else:
                rc = lib.esr_bn_param_grads(m.sums2, m.sums3, m.rstd, m.groups, m.C, m.n_per_group, m.dgamma, m.dbeta, m.g_gamma, st)
            assert rc == 0, (op, rc)
        _sync()

    def as_list(self):
        L = _lib()
        cmds = self.cmds()
        arr = (L.Cmd * len(cmds))()
        for i, (op, m) in enumerate(cmds):
            arr[i].op = op
            C.memmove(C.addressof(arr[i].u), C.addressof(m), C.sizeof(m))
        failed = C.c_int(-1)
        rc = L.load_library().esr_run(arr, len(cmds), C.byref(failed), _stream())
        assert rc == 0 and failed.value == -1, (rc, failed.value)
        _sync()

    def results(self):
        c = self.c
        acts = dict(z=(self.z, c.s2d), dy=(self.dy, False), g_dz=(self.g_dz, c.s2d), g_y=(self.g_y, False))
        return {k: (a.download(), s) for k, (a, s) in acts.items()}


@pytest.mark.parametrize('s2d', [False, True], ids=['plain', 's2d'])
def test_chain(s2d):
    """The nine launches in the critic's order, groups = 2, against torch autograd in float64 through F.leaky_relu(F.batch_norm(training=True))
    per group — z, dy, dgamma, dbeta, g_dz, g_y, g_gamma to relative L2 < 2e-5 — and the same nine commands as ONE esr_run list: the same bits
    everywhere (the double sums, fp64 atomics, to 1e-12 relative)."""
    tol = 2e-5
    c = Case('split', 4, 2, 40, 8, 12, s2d=s2d, seed=3)
    ch = Chain(c)
    ch.direct()
    res = ch.results()
    got = {}
    for k, (bits, s) in res.items():
        check_out(bits, c.f, c.B, c.C, *c.geometry(s)[1:], c.b0, c.cg0, s)
        got[k] = c.stored(None, s, bits=bits)
    # torch autograd, float64, one graph over both groups
    y, dz = c.y.clone().requires_grad_(True), c.dz.clone().requires_grad_(True)
    gm, bt = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    z = torch.cat([F.leaky_relu(F.batch_norm(y[g * c.Bg:(g + 1) * c.Bg], None, None, gm, bt, training=True, eps=EPS), c.slope) for g in range(c.groups)])
    dy, dgamma, dbeta = torch.autograd.grad(z, [y, gm, bt], dz, create_graph=True)
    g_y, g_gamma, g_dz = torch.autograd.grad(dy, [y, gm, dz], c.u)
    ref = dict(z=z.detach(), dy=dy.detach(), g_dz=g_dz, g_y=g_y, dgamma=dgamma.detach(), dbeta=dbeta.detach(), g_gamma=g_gamma)
    got.update({k: v.cpu() for k, v in ch.pg.items()})
    errs = {k: rel(got[k], ref[k]) for k in ref}
    _note('chained (relative L2 / 2e-5)', max(errs.values()) / tol)
    for k, e in errs.items():
        assert e < tol, '%s: relative L2 %.3g' % (k, e)
    # planted: the comparator notices group 0's statistics used for group 1, and a parity swap
    zr0 = F.leaky_relu(F.batch_norm(c.y[c.Bg:], c.y[:c.Bg].mean((0, 2, 3)), c.y[:c.Bg].var((0, 2, 3), unbiased=False), gm, bt, training=False,
                                    eps=EPS), c.slope).detach()
    assert rel(got['z'][c.Bg:], zr0) >= tol, "planted: group 0's statistics used for group 1"
    if s2d:
        assert rel(c.stored(None, True, bits=res['z'][0], swap=True), ref['z']) >= tol, 'planted: x&1 and y&1 swapped'
    # the same nine commands as one launch list
    ls = Chain(c)
    ls.as_list()
    for k, (bits, s) in ls.results().items():
        assert torch.equal(bits, res[k][0]), '%s: the launch list and the direct calls differ' % k
    for k in ch.stat:
        assert torch.equal(ch.stat[k], ls.stat[k]), k
    for k in ch.pg:
        assert torch.equal(ch.pg[k], ls.pg[k]), k
    for a, b in zip(ch.sums, ls.sums):
        assert float(((a - b).abs() / a.abs().clamp_min(1e-300)).max()) <= 1e-12
