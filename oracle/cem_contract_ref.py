"""TEST INFRASTRUCTURE ONLY.  The contract of the CEM filter entry points (include/esr_hip.h: esr_cem_downscale / _lrfilter / _upscale, their
separable variants, esr_cem_filter_upscale_sep and the two adjoints) restated in float64 — plain torch, device-agnostic, no import from the
package under test or from the other oracle modules — and the comparator that judges a kernel by it.

Taps are either a k x k array or a pair (tv, th) of 1-D factors; the pair stands for taps = outer(tv, th) formed in float64 from the values handed
over, and is evaluated as two 1-D float64 passes.  Any sf >= 1, any pre in [0, sf).

Every forward returns (value, S): S is the same expression evaluated on |taps|, |x|, |g|, |lr| — the magnitude an fp32 evaluation's rounding
error scales with.  The adjoints are float64 autograd of these very functions (adjoint()): there is no second restatement.

The bound (bound(), element-wise, u = 2^-24):   |got - ref| <= (n + 2) u S + u |ref|
n = fused multiply-adds per output: 2k for a separable entry point (k per pass plus the stored intermediate), k^2 for a 2-D one, + 2 kf for a
folded filter; the number of gather terms (+ 1 for the fp32 rounding of the host-built cumulative tables) for an adjoint.  Modes 1 and 3 add
u |g|.  Mode 2:  bound(out) = bound(U(f_x)) + range (bound(g - U(f_g)) + 2^-21), by |tanh'| <= 1; the 2^-21 allows for the device tanhf and is
an ASSUMPTION (about 4 ulp at |tanh| ~ 1), not a derivation."""
import torch

U = 2.0 ** -24
TANH_ALLOWANCE = 2.0 ** -21


# ----------------------------------------------------------------------------- taps
def is_sep(taps):
    return isinstance(taps, (tuple, list))


def _f64(t, like=None):
    t = torch.as_tensor(t)
    return t.to(dtype=torch.float64, device=like.device if like is not None else t.device)


def tap_size(taps):
    return int(taps[0].shape[0]) if is_sep(taps) else int(taps.shape[-1])


def taps_2d(taps):
    """The k x k float64 array the taps stand for."""
    if is_sep(taps):
        return torch.outer(_f64(taps[0]), _f64(taps[1]))
    return _f64(taps)


def _abs(taps):
    return (torch.as_tensor(taps[0]).abs(), torch.as_tensor(taps[1]).abs()) if is_sep(taps) else torch.as_tensor(taps).abs()


# ----------------------------------------------------------------------------- building blocks
def pad_replicate(x, p):
    """Replicate padding by p >= 0 pixels on every side, as index clamping (any p, any size; differentiable)."""
    if p == 0:
        return x
    H, W = x.shape[-2:]
    iy = torch.arange(-p, H + p, device=x.device).clamp(0, H - 1)
    ix = torch.arange(-p, W + p, device=x.device).clamp(0, W - 1)
    return x.index_select(-2, iy).index_select(-1, ix)


def correlate(xp, taps):
    """'valid' cross-correlation of every plane of xp [B][C][H][W] (float64) with the taps: out[i][j] = sum_ab taps[a][b] xp[i + a][j + b]."""
    if is_sep(taps):
        return _pass(_pass(xp, taps[1], -1), taps[0], -2)
    t = _f64(taps).cpu()
    k = t.shape[0]
    n = xp.shape[-2] - k + 1
    return sum(_pass(xp.narrow(-2, a, n), t[a], -1) for a in range(k))


def _pass(x, t, dim):
    """One 1-D 'valid' pass along `dim` as a plain sum of shifted slices (no convolution library: the same arithmetic on every device)."""
    t = [float(v) for v in _f64(t).cpu()]
    n = x.shape[dim] - len(t) + 1
    out = x.narrow(dim, 0, n) * t[0]
    for a in range(1, len(t)):
        out = out + x.narrow(dim, a, n) * t[a]
    return out


def _same(x, taps):
    return correlate(pad_replicate(x, tap_size(taps) // 2), taps)


def _stuff(f, sf, pre):
    B, C, h, w = f.shape
    z = torch.zeros(B, C, h * sf, w * sf, dtype=f.dtype, device=f.device)
    z[:, :, pre::sf, pre::sf] = f
    return z


def _crop(x, crop):
    return x[:, :, crop:x.shape[-2] - crop, crop:x.shape[-1] - crop] if crop else x


# ----------------------------------------------------------------------------- the three filters
def _downscale(y, taps, sf, pre, lr, lr_pad):
    d = _same(y, taps)[..., pre::sf, pre::sf]
    return d if lr is None else (pad_replicate(lr, lr_pad), d)


def downscale(y, taps, sf, pre, lr=None, lr_pad=0):
    """DownscaleOP: conv2d(pad_replicate(y, k // 2), taps)[..., pre::sf, pre::sf]; with lr: pad_replicate(lr, lr_pad) - D(y)."""
    assert 0 <= pre < sf
    y = _f64(y)
    if lr is None:
        return _downscale(y, taps, sf, pre, None, 0), _downscale(y.abs(), _abs(taps), sf, pre, None, 0)
    lr = _f64(lr)
    a, d = _downscale(y, taps, sf, pre, lr, lr_pad)
    sa, sd = _downscale(y.abs(), _abs(taps), sf, pre, lr.abs(), lr_pad)
    return a - d, sa + sd


def lrfilter(x, taps):
    """Conv_LR_with_Inv_hTh_OP: replicate-pad k // 2, correlate."""
    x = _f64(x)
    return _same(x, taps), _same(x.abs(), _abs(taps))


def _up(f, taps, sf, pre, crop):
    return _crop(_same(_stuff(f, sf, pre), taps), crop)


def _upscale_modes(u1, s1, u2, s2, g, crop, mode, rng):
    if mode == 0:
        return u1, s1
    g = _crop(_f64(g), crop)
    if mode == 1:
        return g + u1, g.abs() + s1
    ns, s_ns = g - u2, g.abs() + s2
    if mode == 2:
        return u1 + torch.tanh(ns) * rng, (s1, s_ns, u1, ns)
    return (u1, ns), (s1, s_ns)


def upscale(f, taps, sf, pre, f2=None, g=None, crop=0, mode=0, range=0.0):
    """Upscale_OP: stuff f into zeros at [pre::sf, pre::sf], replicate-pad k // 2, correlate, crop.
    mode 0: U(f); 1: g + U(f); 2: U(f) + tanh(g - U(f2)) range; 3: (U(f), g - U(f2)).
    S: mode 0 / 1 one tensor; mode 3 a pair; mode 2 (S of U(f), S of g - U(f2), U(f), g - U(f2)) — what bound_mode2 composes."""
    assert 0 <= pre < sf
    f = _f64(f)
    at = _abs(taps)
    u1, s1 = _up(f, taps, sf, pre, crop), _up(f.abs(), at, sf, pre, crop)
    u2 = s2 = None
    if mode >= 2:
        f2 = _f64(f2)
        u2, s2 = _up(f2, taps, sf, pre, crop), _up(f2.abs(), at, sf, pre, crop)
    return _upscale_modes(u1, s1, u2, s2, g, crop, mode, range)


def filter_upscale(e, taps_f, taps, sf, pre, e2=None, g=None, crop=0, mode=0, range=0.0):
    """upscale() with K(e) (and K(e2)) in place of f (f2), K = lrfilter with taps_f."""
    assert 0 <= pre < sf
    e = _f64(e)
    at, atf = _abs(taps), _abs(taps_f)
    u1, s1 = _up(_same(e, taps_f), taps, sf, pre, crop), _up(_same(e.abs(), atf), at, sf, pre, crop)
    u2 = s2 = None
    if mode >= 2:
        e2 = _f64(e2)
        u2, s2 = _up(_same(e2, taps_f), taps, sf, pre, crop), _up(_same(e2.abs(), atf), at, sf, pre, crop)
    return _upscale_modes(u1, s1, u2, s2, g, crop, mode, range)


# ----------------------------------------------------------------------------- adjoints: float64 autograd of the functions above
def adjoint(kind, dy, taps, sf, pre, in_shape):
    """Transpose of 'downscale' | 'lrfilter' | 'upscale' (plain forms) applied to dy; in_shape: the forward's input shape.  Returns (dx, S)."""
    dy = _f64(dy)

    def run(t, cot):
        x = torch.zeros(in_shape, dtype=torch.float64, device=dy.device, requires_grad=True)
        if kind == 'downscale':
            y = _downscale(x, t, sf, pre, None, 0)
        elif kind == 'lrfilter':
            y = _same(x, t)
        else:
            y = _up(x, t, sf, pre, 0)
        assert y.shape == cot.shape, (tuple(y.shape), tuple(cot.shape))
        return torch.autograd.grad(y, x, cot)[0]
    return run(taps, dy), run(_abs(taps), dy.abs())


def adjoint_terms(k, sq, nq_y, nq_x, sep):
    """The most terms one unknown gathers, + 1 for the fp32 rounding of the host-built prefix / suffix tables.  Per axis the outputs q (nq of them,
    at frame positions m(q) = q sq + oq, 0 <= oq, m(q) <= N - 1) whose window reaches frame position f:
      interior          m(q) in [f + p - (k - 1), f + p]: k consecutive positions hold at most ceil(k / sq) multiples of the stride;
      first (f = 0)     m(q) in [oq, p]:          at most floor(p / sq) + 1 <= ceil(k / sq)   (k = 2p + 1);
      last (f = N - 1)  m(q) in [N - 1 - p, N - 1]: the same;
      N == 1            every output, and m(q) <= N - 1 leaves nq = 1.
    So min(nq, ceil(k / sq)) per axis, attained in the interior.  2-D gather: the product of the two axes; separable: their sum and the stored
    intermediate."""
    per_axis = -(-k // sq)
    ny, nx = min(nq_y, per_axis), min(nq_x, per_axis)
    return (ny + nx + 1 if sep else ny * nx) + 1


# ----------------------------------------------------------------------------- the comparator
def bound(n, S, ref, g=None):
    """(n + 2) u S + u |ref| (+ u |g|: modes 1 and 3)."""
    b = (n + 2) * U * S + U * ref.abs()
    return b if g is None else b + U * _f64(g, ref).abs()


def bound_mode2(n, S, g, crop, rng):
    """S as upscale(mode=2) returns it."""
    s1, s_ns, u1, ns = S
    return bound(n, s1, u1) + abs(rng) * (bound(n, s_ns, ns, _crop(_f64(g, ns), crop)) + TANH_ALLOWANCE)


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over the elements (inf where got is not finite or the shapes differ)."""
    got = _f64(got, ref)
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return float('inf')
    return float(((got - ref).abs() / bnd.clamp_min(1e-300)).max()) if ref.numel() else 0.0


def accepts(got, ref, bnd):
    return worst_ratio(got, ref, bnd) <= 1.0


# ----------------------------------------------------------------------------- synthetic taps
def synthetic_factor(k, seed):
    """k seeded fp32 taps of mixed signs, |tap| in [0.5, 1] / sqrt(k) (so |tv[a] th[b]| >= 0.25 / k >= 0.2 / k and every factor entry >= 0.2 / k),
    not equal to its own reverse."""
    gen = torch.Generator().manual_seed(1000 + seed)
    mag = (0.5 + 0.5 * torch.rand(k, generator=gen, dtype=torch.float64)) / k ** 0.5
    sgn = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0).double()
    if k > 1:
        sgn[0], sgn[-1] = 1.0, -1.0          # mixed signs and no flip symmetry, whatever the draw
    return (mag * sgn).float()


def synthetic_sep(k, seed):
    """(tv, th), tv != th."""
    return synthetic_factor(k, 2 * seed), synthetic_factor(k, 2 * seed + 1)


def synthetic_2d(k, seed):
    """A full-rank seeded k x k fp32 array of mixed signs, |tap| in [0.25, 1] / k."""
    gen = torch.Generator().manual_seed(5000 + seed)
    mag = (0.25 + 0.75 * torch.rand(k, k, generator=gen, dtype=torch.float64)) / k
    sgn = torch.where(torch.rand(k, k, generator=gen) < 0.5, -1.0, 1.0).double()
    if k > 1:
        sgn[0, 0], sgn[-1, -1], sgn[0, -1], sgn[-1, 0] = 1.0, -1.0, 1.0, -1.0
    return (mag * sgn).float()


def uniform(shape, seed, lo=-1.0, hi=1.0):
    gen = torch.Generator().manual_seed(9000 + seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)).float()
