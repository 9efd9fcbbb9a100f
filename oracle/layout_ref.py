"""TEST INFRASTRUCTURE ONLY.  The contract of the entry points that move data across the module boundary (include/esr_hip.h: esr_pack_nchw,
esr_unpack_nchw, esr_pack_nchw_norm, esr_unpack_grad_nchw_norm) restated on the CPU — plain torch, no import from the package under test or from
the other oracle modules — and the comparator that judges a kernel by it.

The activation layout: [planes][B][CG][H+2][W+2][8] 16-bit elements, a `hi` plane and an optional `lo` plane of residuals, a one-pixel zero border.
A form is (fmt, planes): fmt 0 = bf16, 1 = fp16 (ESR_FMT_*).  Stored images are int16 tensors (bit patterns).

    encode   hi = RNE(v), lo = RNE(v - float(hi)), the subtraction in fp32 (it is exact there for every finite v whose hi is finite)
    decode   float(hi) + float(lo) as ONE fp32 addition; an absent lo counts as +0.f, so a stored -0 decodes to +0
    frame    the whole expected buffer image of a pack: zero border, zero lanes >= nc, zero groups past ceil(nc / 8)
    pack64   float64: the raw view of image b at src + b*batch_stride, channels [c0, c0 + nc), replicate-padded by `pad`, then the bilinear /down
             with source coordinate sy = max((y + 0.5) down - 0.5, 0), taps (y0, min(y0 + 1, hp - 1)), the same along x
             (= F.interpolate(F.pad(x, replicate), scale_factor=1/down, 'bilinear', align_corners=False); tests/test_host_layout_ref.py pins it)

The store term of a bounded comparison (STORE[form] = (c, a): |stored - v| <= c |v| + a).  RNE to p significant bits errs by 2^-p |v|:
bf16 p = 8, fp16 p = 11 (normal range); with a lo plane the residue of the residue is left: 2^-16 and 2^-22.  The constants are those of
tests/test_gpu_bwd_helpers.py::OUT_FMTS: bf16's is that figure itself (2^-8, attained at the bottom of a binade), the others are one binade
above it: 2^-15, 2^-10, 2^-21 + 2^-25 absolute (a subnormal fp16 lo).  A single fp16 plane has no absolute term: below 2^-14 its error is up to
2^-25 whatever |v|, so the bound holds there only for |v| >= 2^-15 — the bounded families draw from [-1, 1] and [0, 1], where the seeded inputs
keep away from it, and the subnormal range has a bit-exact case of its own."""
import torch

U = 2.0 ** -24
FORMS = {'bf16': (0, 1), 'split': (0, 2), 'f16': (1, 1), 'f16x2': (1, 2)}          # name: (fmt, planes)
STORE = {'bf16': (2.0 ** -8, 0.0), 'split': (2.0 ** -15, 0.0), 'f16': (2.0 ** -10, 0.0), 'f16x2': (2.0 ** -21, 2.0 ** -25)}
DTYPE = {0: torch.bfloat16, 1: torch.float16}


# ----------------------------------------------------------------------------- the element formats
def encode(v, fmt, planes):
    """fp32 tensor -> (hi, lo) int16 bit images of the same shape; lo is None for planes == 1."""
    assert v.dtype == torch.float32
    dt = DTYPE[fmt]
    hi = v.to(dt)
    lo = (v - hi.float()).to(dt).view(torch.int16) if planes == 2 else None
    return hi.view(torch.int16), lo


def decode(hi, lo, fmt):
    """(hi, lo | None) int16 bit images -> fp32."""
    dt = DTYPE[fmt]
    h = hi.view(dt).float()
    return h + (lo.view(dt).float() if lo is not None else torch.zeros_like(h))


def to_lanes(x, ncg):
    """[B][nc][H][W] -> [B][ncg][H][W][8], channel c in lane c % 8 of group c // 8, zeros in the lanes and groups past nc."""
    B, nc, H, W = x.shape
    assert ncg * 8 >= nc
    out = torch.zeros(B, ncg * 8, H, W, dtype=x.dtype)
    out[:, :nc] = x
    return out.view(B, ncg, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_lanes(img, nc):
    """[B][ncg][H+2][W+2][8] -> the interior [B][nc][H][W]."""
    B, ncg, Hp, Wp, _ = img.shape
    return img[:, :, 1:-1, 1:-1].permute(0, 1, 4, 2, 3).reshape(B, ncg * 8, Hp - 2, Wp - 2)[:, :nc].contiguous()


def frame(values, fmt, planes, ncg):
    """fp32 [B][nc][H][W] -> the int16 buffer image [planes][B][ncg][H+2][W+2][8] a pack of these values leaves."""
    B, nc, H, W = values.shape
    out = torch.zeros(planes, B, ncg, H + 2, W + 2, 8, dtype=torch.int16)
    hi, lo = encode(values, fmt, planes)
    out[0, :, :, 1:-1, 1:-1] = to_lanes(hi, ncg)
    if planes == 2:
        out[1, :, :, 1:-1, 1:-1] = to_lanes(lo, ncg)
    return out


def unframe(img, fmt, nc):
    """int16 [planes][B][ncg][H+2][W+2][8] -> (fp32 [B][nc][H][W] decoded interior, True when every element outside it — border, lanes >= nc,
    groups past ceil(nc / 8) — is a zero bit pattern on every plane)."""
    planes = img.shape[0]
    hi = from_lanes(img[0], nc)
    lo = from_lanes(img[1], nc) if planes == 2 else None
    rest = img.clone()
    keep = to_lanes(torch.ones(img.shape[1], nc, img.shape[3] - 2, img.shape[4] - 2, dtype=torch.bool), img.shape[2])
    rest[:, :, :, 1:-1, 1:-1] = torch.where(keep, torch.zeros((), dtype=torch.int16), rest[:, :, :, 1:-1, 1:-1])
    return decode(hi, lo, fmt), not bool(rest.any())


# ----------------------------------------------------------------------------- esr_pack_nchw in float64, as building blocks
def raw_view(src, B, C, h, w, c0, nc, batch_stride=0):
    """Channels [c0, c0 + nc) of the B images [C][h][w] that start at src + b*batch_stride floats (0 = C*h*w), float64 [B][nc][h][w]."""
    flat = src.reshape(-1)
    bs = batch_stride if batch_stride else C * h * w
    imgs = [flat[b * bs:b * bs + C * h * w].view(C, h, w)[c0:c0 + nc] for b in range(B)]
    return torch.stack(imgs).double()


def pad_replicate(x, p):
    """Replicate padding by p >= 0 pixels on every side, as index clamping (any p, any size)."""
    if p == 0:
        return x
    H, W = x.shape[-2:]
    iy = torch.arange(-p, H + p).clamp(0, H - 1)
    ix = torch.arange(-p, W + p).clamp(0, W - 1)
    return x.index_select(-2, iy).index_select(-1, ix)


def _taps(n_out, n_in, down, offset):
    s = ((torch.arange(n_out, dtype=torch.float64) + offset) * down - offset).clamp_min(0.0)
    i0 = s.floor().long()
    return i0, (i0 + 1).clamp_max(n_in - 1), s - i0.double()


def bilinear_down(p, down, offset=0.5):
    """The bilinear /down of a float64 [..][hp][wp] frame (down divides hp and wp): four taps, weights (1 - ly, ly) x (1 - lx, lx).
    offset: the half-pixel offset of align_corners=False (the contract: 0.5)."""
    if down == 1:
        return p
    hp, wp = p.shape[-2:]
    assert hp % down == 0 and wp % down == 0
    y0, y1, ly = _taps(hp // down, hp, down, offset)
    x0, x1, lx = _taps(wp // down, wp, down, offset)
    ly = ly[:, None]
    r0, r1 = p.index_select(-2, y0), p.index_select(-2, y1)
    top = (1 - lx) * r0.index_select(-1, x0) + lx * r0.index_select(-1, x1)
    bot = (1 - lx) * r1.index_select(-1, x0) + lx * r1.index_select(-1, x1)
    return (1 - ly) * top + ly * bot


def pack64(src, c0, nc, pad=0, down=1, batch_stride=0, hw=None, channels=None):
    """What esr_pack_nchw stores, before the store's rounding: float64 [B][nc][(h + 2 pad) / down][(w + 2 pad) / down].  src: a tensor whose
    first dimension is the batch; [B][C][h][w] unless hw / channels / batch_stride describe a raw view of its memory (esr_hip.act.pack_nchw)."""
    B = src.shape[0]
    C = src.shape[1] if channels is None else channels
    h, w = (src.shape[2], src.shape[3]) if hw is None else hw
    return bilinear_down(pad_replicate(raw_view(src, B, C, h, w, c0, nc, batch_stride), pad), down)


def pack_norm64(x, mean=None, std=None):
    """esr_pack_nchw_norm before the store: (x - mean[c]) / std[c] in float64 from the fp32 values handed over (both None: x)."""
    x = x.double()
    if mean is None:
        return x
    return (x - mean.double().view(1, -1, 1, 1)) / std.double().view(1, -1, 1, 1)


def unpack_grad_norm64(g, std=None):
    """esr_unpack_grad_nchw_norm: decoded gradient [B][C][H][W] / std[c] in float64 (None: g)."""
    g = g.double()
    return g if std is None else g / std.double().view(1, -1, 1, 1)


# ----------------------------------------------------------------------------- the comparator
def store_bound(form, ref):
    c, a = STORE[form]
    return c * ref.abs() + a


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; an exact element counts 0 whatever its bound; inf where got is not finite or the shapes differ."""
    got = got.double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return float('inf')
    if not ref.numel():
        return 0.0
    err = (got - ref).abs()
    r = err / bound.clamp_min(1e-300)
    r[err == 0] = 0.0
    return float(r.max())


def accepts(got, ref, bound):
    return worst_ratio(got, ref, bound) <= 1.0


# ----------------------------------------------------------------------------- inputs
def uniform(shape, seed, lo=-1.0, hi=1.0):
    gen = torch.Generator().manual_seed(7000 + seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)).float()


def grid(shape, seed, denom=1024, amp=2):
    """Seeded integers / denom in [-amp, amp], fp32 (exact)."""
    gen = torch.Generator().manual_seed(8000 + seed)
    return (torch.randint(-amp * denom, amp * denom + 1, shape, generator=gen).double() / denom).float()


def from_bits(bits):
    """fp32 values from their 32-bit patterns."""
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def specials(fmt):
    """fp32 values that exercise the 16-bit rounding: +-0, exact ties of the bf16 and of the fp16 rounding with the kept mantissa even and odd
    (both signs), values both formats hold exactly, and (bf16, whose exponent range is fp32's) 1e30."""
    bits = [0x00000000, 0x80000000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x40FE8000, 0x40FF8000,      # bf16 ties: lower 16 bits 0x8000, bit 16 = 0 / 1
            0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3FFFD000, 0x3FFFF000,      # fp16 ties: lower 13 bits 0x1000, bit 13 = 0 / 1
            0x3F800000, 0xBFC00000, 0x3E200000, 0x40000000]                              # 1, -1.5, 0.15625, 2
    v = from_bits(bits)
    return torch.cat([v, torch.tensor([1e30, -1e30], dtype=torch.float32)]) if fmt == 0 else v
