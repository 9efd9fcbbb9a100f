"""Float64 restatement of the Z-objective entry points of include/esr_hip.h (esr_soft_hist_*, esr_kde_*, esr_img_stats*, esr_patch_std*,
esr_shift_l1*, esr_scribble*, esr_patch_mag*, esr_pairmin*) at the granularity of the C-ABI and from the header's wording: every function takes
the fp32 arrays as they are stored (plus the scalars the ABI takes) and returns, in float64 on the CPU, what the header says the caller folds.
Gradients are float64 autograd of the forward restatement, composed with the coef / g / dS / g_row / g_bin that the ABI takes.  Next to a value
the functions of the add / multiply / sqrt kernels return `mag`, the sum of the magnitudes of the operands before they cancel: the tests bound
|err| <= k u mag with k counted in the kernel (tests/test_gpu_zobj_contract.py states every count).

The comparator (`compare`) and the tie rules live here as well, so that tests/test_host_zobj_contract_ref.py can pin them without a GPU.
The float64 helpers of the older GPU test files (std64, shift64, definition64, _ref_stats, _scores, _ref_rows, _ref_cols) moved here unchanged;
those files import them."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
U64 = 2.0 ** -53
TIE = 1e-6              # pairmin: two smallest distances nearer than this are a tie (tests/test_gpu_random_z.py)
TIE_CAP = 1e-4          # every other family: at most this share of elements may be ties
PAIRMIN_TIE_CAP = 1e-2


# ------------------------------------------------------------------------------------------------ the comparator
def compare(got, ref, bound, what=''):
    """Asserts |got - ref| <= bound element by element (a NaN or inf anywhere in `got` fails) and returns the worst |err| / bound."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    bound = torch.as_tensor(bound).double().cpu().expand_as(ref)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), '%s: %d values are not finite' % (what, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where((err == 0), torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError('%s: |err| / bound = %.3g at flat index %d (got %.9g, reference %.9g, bound %.3g); %d of %d beyond the bound' % (
            what, worst, i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i]), int((ratio > 1).sum()), ratio.numel()))
    return worst


def rtol_bound(ref, rtol, atol_of_max=0.0):
    """The bars of the __expf kernels: rtol |ref| + atol_of_max max|ref|"""
    ref = torch.as_tensor(ref).double()
    return rtol * ref.abs() + (atol_of_max * float(ref.abs().max()) if ref.numel() else 0.0)


def accumulated(base, grad):
    """dx after an accumulate = 1 call on dx = base, and the one extra rounding's bound"""
    r = base.double() + grad
    return r, U * r.abs()


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def _image(x, clamp01=True, mask=None):
    v = torch.clamp(x, 0, 1) if clamp01 else x
    return v if mask is None else v * mask


# ------------------------------------------------------------------------------------------------ esr_soft_hist_*
def wrapped(delta, period):
    """min(|d|, |d - P|, |d + P|)"""
    return torch.minimum(torch.minimum(delta.abs(), (delta - period).abs()), (delta + period).abs())


def soft_hist_centres(K, lo, hi):
    k = torch.arange(K, dtype=torch.float64)
    return lo + k * ((hi - lo) / (K - 1)) if K > 1 else torch.full((1,), float(lo), dtype=torch.float64)


def soft_hist(v, K, lo, hi, T, eps, period=None, chunk=4096):
    """sum over the slabs of partial[slab][k] = sum_i exp(-(d(v_i, c_k) + eps)^2 / T), the distance wrapped with period hi (NOT hi - lo)"""
    period = hi if period is None else period
    c = soft_hist_centres(K, lo, hi)
    out = 0
    for vc in v.double().flatten().split(chunk):
        out = out + torch.exp(-(wrapped(vc[:, None] - c[None], period) + eps) ** 2 / T).sum(0)
    return out


def soft_hist_grad(v, K, lo, hi, T, eps, gh):
    """d (sum_k gh[k] sum_i exp(...)) / dv"""
    x = _d(v).flatten().requires_grad_(True)
    (soft_hist(x, K, lo, hi, T, eps) * _d(gh)).sum().backward()
    return x.grad.reshape(v.shape)


# ------------------------------------------------------------------------------------------------ esr_kde_*
def _scores(x, b, P=1.0, eps=1e-7):
    """[r, M] s_ij = mean_d (min(|δ|, |δ - P|, |δ + P|) + eps)^2, float64"""
    d = x[:, None, :] - b[None]
    w = torch.minimum(torch.minimum(d.abs(), (d - P).abs()), (d + P).abs())
    return ((w + eps) ** 2).mean(2)


def _ref_rows(X, bins, T, g, chunk=48):
    """lse_i = log sum_j exp(-s_ij/T) and d (sum_i g_i lse_i) / dX, float64, chunked over rows"""
    lse, grads = [], []
    b = bins.double()
    for xc, gc in zip(X.double().split(chunk), g.split(chunk)):
        xc = xc.clone().requires_grad_(True)
        l = torch.logsumexp(-_scores(xc, b) / T, 1)
        (l * gc).sum().backward()
        lse.append(l.detach())
        grads.append(xc.grad)
    return torch.cat(lse), torch.cat(grads)


def _ref_cols(X, counts, bins, T, g, chunk=48):
    """lse_bj = log sum_{i in image b} exp(-s_ij/T) and d (sum g_bj lse_bj) / dX, float64 (the gradient through a surrogate with lse fixed)"""
    b = bins.double()
    Xd = X.double()
    lse, r = [], 0
    for n in counts:
        lse.append(torch.logsumexp(torch.cat([-_scores(xc, b) / T for xc in Xd[r:r + n].split(chunk)], 0), 0))
        r += n
    lse = torch.stack(lse)
    img = torch.repeat_interleave(torch.arange(len(counts), device=X.device), torch.tensor(counts, device=X.device))
    grads = []
    for xc, ic in zip(Xd.split(chunk), img.split(chunk)):
        xc = xc.clone().requires_grad_(True)
        (g[ic] * torch.exp(-_scores(xc, b) / T - lse[ic])).sum().backward()
        grads.append(xc.grad)
    return lse, torch.cat(grads)


def kde_fwd(outer, inner, ranges, period, T, dtype=torch.float64, chunk=64, skip_d=None):
    """[n_ranges][n_outer] log sum over the range of exp(-s_oi / T) = log(psum) + pmax.  `dtype` float32 gives the fp32 CPU evaluation of the
    same formula (the yardstick where a bar is missed); skip_d leaves one coordinate out (a planted error)."""
    o, b = outer.to(dtype), inner.to(dtype)
    D = o.size(1)
    keep = [d for d in range(D) if d != skip_d]
    out = []
    for r0, r1 in ranges:
        rows = []
        for oc in o.split(chunk):
            s = _scores(oc[:, keep], b[r0:r1][:, keep], P=period) * (len(keep) / D)
            rows.append(torch.logsumexp(-s / T, 1))
        out.append(torch.cat(rows))
    return torch.stack(out).double()


def kde_fwd_graph(outer, inner, period, T, chunk=64):
    """[n_outer] log sum_i exp(-s_oi / T) over all of `inner`, float64, with the autograd graph attached to both arguments"""
    o, b = outer.double(), inner.double()
    return torch.cat([torch.logsumexp(-_scores(oc, b, P=period) / T, 1) for oc in o.split(chunk)])


def kde_bwd(X, tiles, bins, period, T, g_row=None, l_row=None, g_bin=None, l_bin=None, dtype=torch.float64, chunk=64):
    """[R][D] (the slabs summed): d/dX of sum_{i in tiles, j} g_row[i] g_bin[b][j] exp(-s_ij / T - l_row[i] - l_bin[b][j]) with the l's held fixed;
    rows outside every tile stay NaN (the kernel does not address them)."""
    Xd, b = X.to(dtype), bins.to(dtype)
    out = torch.full(tuple(X.shape), float('nan'), dtype=dtype)
    for img, t0, t1 in tiles:
        for r0 in range(t0, t1, chunk):
            r1 = min(t1, r0 + chunk)
            xc = Xd[r0:r1].clone().requires_grad_(True)
            e = -_scores(xc, b, P=period) / T
            if l_row is not None:
                e = e - l_row[r0:r1].to(dtype)[:, None]
            if l_bin is not None:
                e = e - l_bin[img].to(dtype)[None]
            w = torch.exp(e)
            if g_row is not None:
                w = w * g_row[r0:r1].to(dtype)[:, None]
            if g_bin is not None:
                w = w * g_bin[img].to(dtype)[None]
            w.sum().backward()
            out[r0:r1] = xc.grad
    return out.double()


def kde_dedup(bins, half_width):
    """keep[i] = 0 iff some j > i has |b_id - b_jd| < half_width in every d.  The comparison is of fp32 values against an fp32 width: the
    differences are taken in fp32 as the kernel must (a float64 difference would decide the exact-boundary pairs differently)."""
    b = bins.float()
    M = b.size(0)
    near = ((b[:, None, :] - b[None]).abs() < torch.tensor(half_width, dtype=torch.float32)).all(2)
    later = torch.arange(M)[None, :] > torch.arange(M)[:, None]
    return (~(near & later).any(1)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ esr_img_stats*
def _ref_stats(x, mask, clamp01, kind):
    v = x.double()
    if clamp01:
        v = torch.clamp(v, 0, 1)
    if mask is not None:
        v = v * mask.double()
    if kind == 0:
        return torch.std(v, dim=(1, 2, 3))
    if kind == 1:
        return (v[:, :, :, :-1] - v[:, :, :, 1:]).abs().mean(dim=(1, 2, 3)) + (v[:, :, :-1, :] - v[:, :, 1:, :]).abs().mean(dim=(1, 2, 3))
    ix = (v[..., :, 1:] - v[..., :, :-1])[..., :-1, :]
    iy = (v[..., 1:, :] - v[..., :-1, :])[..., :, :-1]
    return torch.stack([(ix * ix).mean(dim=(1, 2, 3)), (iy * iy).mean(dim=(1, 2, 3)), (ix * iy).mean(dim=(1, 2, 3))], 0)


def img_stats(x, mask, clamp01, kind, with_mag=False):
    """sums[b][3] of the header (the third entry 0 for kinds 0 and 1); mag: the same sums over the operands' magnitudes"""
    v = _image(x.double(), clamp01, None if mask is None else mask.double())
    a = v.abs()
    s = lambda t: t.sum(dim=(1, 2, 3))  # noqa: E731
    z = torch.zeros(v.size(0), dtype=torch.float64)
    if kind == 0:
        out, mag = (s(v), s(v * v), z), (s(a), s(a * a), z)
    elif kind == 1:
        out = (s((v[..., :, :-1] - v[..., :, 1:]).abs()), s((v[..., :-1, :] - v[..., 1:, :]).abs()), z)
        mag = (s(a[..., :, :-1] + a[..., :, 1:]), s(a[..., :-1, :] + a[..., 1:, :]), z)
    else:
        ix = (v[..., :, 1:] - v[..., :, :-1])[..., :-1, :]
        iy = (v[..., 1:, :] - v[..., :-1, :])[..., :, :-1]
        ax = (a[..., :, 1:] + a[..., :, :-1])[..., :-1, :]
        ay = (a[..., 1:, :] + a[..., :-1, :])[..., :, :-1]
        out, mag = (s(ix * ix), s(iy * iy), s(ix * iy)), (s(ax * ax), s(ay * ay), s(ax * ay))
    out = torch.stack(out, 1)
    return (out, torch.stack(mag, 1)) if with_mag else out


def img_stats_objective(sums, coef, kind):
    """the scalar whose gradient esr_img_stats_grad writes, as the header states it per kind"""
    c = coef
    if kind == 0:
        return (0.5 * c[:, 0] * sums[:, 1] + c[:, 1] * sums[:, 0]).sum()
    if kind == 1:
        return (c[:, 0] * sums[:, 0] + c[:, 1] * sums[:, 1]).sum()
    return (0.5 * c[:, 0] * sums[:, 0] + 0.5 * c[:, 1] * sums[:, 1] + c[:, 2] * sums[:, 2]).sum()


def img_stats_grad(x, mask, clamp01, kind, coef):
    """dx = d img_stats_objective / dx by autograd, and mag: the same chain rule over magnitudes (an upper bound of sum|term|)"""
    xd = _d(x).requires_grad_(True)
    img_stats_objective(img_stats(xd, _d(mask), clamp01, kind), _d(coef), kind).backward()
    v = _image(_d(x), clamp01, _d(mask)).abs()
    c = _d(coef).abs()[:, :, None, None, None]
    m = 1.0 if mask is None else _d(mask).abs()
    if kind == 0:
        mag = (c[:, 0] * v + c[:, 1]) * m
    elif kind == 1:
        mag = (2 * c[:, 0] + 2 * c[:, 1]) * m * torch.ones_like(v)
    else:
        nb = 9 * F.avg_pool2d(F.pad(v, (1, 1, 1, 1)), 3, stride=1)                      # the 3 x 3 sum bounds every |v| + |neighbour| below
        mag = 2 * (c[:, 0] + c[:, 1] + 2 * c[:, 2]) * nb * m
    return xd.grad, mag


def img_stats_grad_closed(x, mask, clamp01, kind, coef):
    """the closed forms written in csrc/esr_zobj.hip and include/esr_hip.h, float64"""
    raw = _d(x)
    mk = _d(mask)
    v = _image(raw, clamp01, mk)
    c0, c1, c2 = [_d(coef)[:, k, None, None, None] for k in range(3)]
    sg = torch.sign
    if kind == 0:
        g = c0 * v + c1
    elif kind == 1:
        g = torch.zeros_like(v)
        g[..., :, :-1] += c0 * sg(v[..., :, :-1] - v[..., :, 1:])
        g[..., :, 1:] -= c0 * sg(v[..., :, :-1] - v[..., :, 1:])
        g[..., :-1, :] += c1 * sg(v[..., :-1, :] - v[..., 1:, :])
        g[..., 1:, :] -= c1 * sg(v[..., :-1, :] - v[..., 1:, :])
    else:
        g = torch.zeros_like(v)
        if v.size(2) > 1 and v.size(3) > 1:
            ix = (v[..., :, 1:] - v[..., :, :-1])[..., :-1, :]
            iy = (v[..., 1:, :] - v[..., :-1, :])[..., :, :-1]
            A, Bf = c0 * ix + c2 * iy, c1 * iy + c2 * ix
            g[..., :-1, :-1] -= A + Bf
            g[..., :-1, 1:] += A
            g[..., 1:, :-1] += Bf
    if clamp01:
        g = g * ((raw >= 0) & (raw <= 1))
    return g if mk is None else g * mk


# ------------------------------------------------------------------------------------------------ esr_patch_std*
def std64(x, ps):
    """float64 restatement: the unbiased STD of every selected window of mean_c clamp(x, 0, 1) -> [P, B], with the zero gradient at flat windows
    (torch.std's is NaN there)"""
    v = torch.clamp(x, 0, 1).mean(1)
    p = v.unfold(1, 7, 1).unfold(2, 7, 1).reshape(v.size(0), -1, 49)[:, ps.flat_idx.to(x.device)]
    d = p - p.mean(-1, keepdim=True)
    var = (d * d).sum(-1) / 48
    return torch.where(var > 0, var.clamp_min(1e-300).sqrt(), torch.zeros_like(var)).t()


def _gray(x):
    return torch.clamp(x, 0, 1).mean(1)


def patch_std(x, corners):
    """S, mean [B][H-6][W-6]: the unbiased std and the mean of the 7 x 7 window at every selected corner of mean_c clamp(x_c, 0, 1), 0 elsewhere.
    The deviations are taken from the window's first value, so a flat window has S = 0 exactly (and gradient 0) at any level."""
    v = _gray(x.double())
    p = v.unfold(1, 7, 1).unfold(2, 7, 1).reshape(v.size(0), v.size(1) - 6, v.size(2) - 6, 49)
    q = p - p[..., :1]
    md = q.mean(-1, keepdim=True)
    var = ((q - md) ** 2).sum(-1) / 48
    sel = (torch.as_tensor(corners) != 0)[None]
    S = torch.where(sel & (var > 0), var.clamp_min(1e-300).sqrt(), torch.zeros_like(var))
    return S, torch.where(sel, (p[..., :1] + md)[..., 0], torch.zeros_like(var))


def patch_std_grad(x, corners, dS):
    """dx = d/dx sum_p dS[p] S[p]; mag_a = BoxT(|a|) / C and mag_t = (|v| BoxT(|a|) + BoxT(|a| |mean|)) / C with a = dS / (48 S), the sums of the
    weights and of the operands' magnitudes over the windows that cover a pixel"""
    xd = _d(x).requires_grad_(True)
    S, mean = patch_std(xd, corners)
    (S * _d(dS)).sum().backward()
    S, mean = S.detach(), mean.detach()
    a = torch.where(S > 0, _d(dS).abs() / (48 * S.clamp_min(1e-300)), torch.zeros_like(S))
    box = lambda t: F.conv_transpose2d(t[:, None], torch.ones(1, 1, 7, 7, dtype=torch.float64))  # noqa: E731
    C = x.size(1)
    v = _gray(_d(x))[:, None]
    return xd.grad, box(a) / C, (v * box(a) + box(a * mean.abs())) / C


def patch_std_grad_closed(x, corners, dS):
    """the header's gather form: dv = sum over the covering corners of a[p] (v - mean[p]), dx_c = dv / C [0 <= x_c <= 1]"""
    raw = _d(x)
    S, mean = patch_std(raw, corners)
    a = torch.where(S > 0, _d(dS) / (48 * S.clamp_min(1e-300)), torch.zeros_like(S))
    box = lambda t: F.conv_transpose2d(t[:, None], torch.ones(1, 1, 7, 7, dtype=torch.float64))  # noqa: E731
    dv = _gray(raw)[:, None] * box(a) - box(a * mean)
    return dv / raw.size(1) * ((raw >= 0) & (raw <= 1))


# ------------------------------------------------------------------------------------------------ esr_patch_mag*
def _selected(corner_index, P):
    ci = torch.as_tensor(corner_index)
    return [(int(cy), int(cx), int(ci[cy, cx])) for cy, cx in torch.nonzero((ci >= 0) & (ci < P))]


def patch_mag(x, corner_index, desired, P, with_mag=False):
    """sum_k partial[b][k] = sum over the selected windows p and j < 49 of (v(window, j) - desired[p][j])^2 -> [B]; mag: (sum e^2, sum |e|)"""
    v = _gray(x.double())
    d = desired.double().reshape(-1, 7, 7)
    s2 = torch.zeros(v.size(0), dtype=torch.float64)
    s1 = torch.zeros(v.size(0), dtype=torch.float64)
    for cy, cx, p in _selected(corner_index, P):
        e = v[:, cy:cy + 7, cx:cx + 7] - d[p]
        s2 = s2 + (e * e).sum(dim=(1, 2))
        s1 = s1 + e.detach().abs().sum(dim=(1, 2))
    return (s2, s1) if with_mag else s2


def patch_mag_grad(x, corner_index, desired, P, g):
    """dx = d/dx sum_b g[b] / (49 P) sum (v - desired)^2; mag: |a_b| / C times (cover count, sum over the covering windows of |v| + |desired|)"""
    xd = _d(x).requires_grad_(True)
    (patch_mag(xd, corner_index, _d(desired), P) * _d(g) / (49.0 * P)).sum().backward()
    H, W = x.shape[2:]
    cnt = torch.zeros(H, W, dtype=torch.float64)
    dsum = torch.zeros(H, W, dtype=torch.float64)
    d = _d(desired).reshape(-1, 7, 7).abs()
    for cy, cx, p in _selected(corner_index, P):
        cnt[cy:cy + 7, cx:cx + 7] += 1
        dsum[cy:cy + 7, cx:cx + 7] += d[p]
    a = (2 * _d(g).abs() / (49.0 * P) / x.size(1))[:, None, None, None]
    v = _gray(_d(x))[:, None]
    return xd.grad, a * cnt, a * (cnt * v + dsum)


# ------------------------------------------------------------------------------------------------ esr_shift_l1*
def shift64(x, mask, pairs):
    """float64 restatement of the periodicity term with grid_sample / crops -> [B]"""
    image = torch.clamp(x, 0, 1)
    m = mask.view(1, 1, *mask.shape)
    loss = 0
    for pr in pairs:
        if pr.interpolated:
            gp, gm = pr.grids(x.device, torch.float64)
            gs = lambda im, g: torch.nn.functional.grid_sample(im, g.repeat([im.size(0), 1, 1, 1]), align_corners=False)  # noqa: E731
            loss = loss + (gs(m, gp) * gs(m, gm) * (gs(image, gp) - gs(image, gm)).abs()).mean(dim=(1, 2, 3))
        else:
            (a0, a1, b0, b1), (c0, c1, d0, d1) = pr.crops
            loss = loss + (m[:, :, a0:a1, b0:b1] * m[:, :, c0:c1, d0:d1] * (image[:, :, a0:a1, b0:b1] - image[:, :, c0:c1, d0:d1]).abs()).mean(dim=(1, 2, 3))
    return loss


def tap_matrix(base, frac, size):
    """[n_out][size]: weights (1 - frac, frac) on (base, base + 1), taps outside [0, size) dropped (zero padding)"""
    n = base.numel()
    Wm = torch.zeros(n, size + 2, dtype=torch.float64)
    r = torch.arange(n)
    b = base.long().clamp(-1, size) + 1          # column c of the padded matrix is source index c - 1
    far = (base.long() < -1) | (base.long() > size - 1)
    f = frac.double()
    Wm[r, b] = torch.where(far, torch.zeros_like(f), 1 - f)
    b1 = (base.long() + 1).clamp(-1, size) + 1
    far1 = (base.long() + 1 < 0) | (base.long() + 1 > size - 1)
    Wm[r, b1] += torch.where(far1, torch.zeros_like(f), f)
    return Wm[:, 1:size + 1].contiguous()


def _samplers(base_x, frac_x, base_y, frac_y, H, W):
    return [(tap_matrix(base_y[s], frac_y[s], H), tap_matrix(base_x[s], frac_x[s], W)) for s in (0, 1)]


def shift_l1_parts(x, mask, base_x, frac_x, base_y, frac_y):
    """(M [ny][nx], GS+ and GS- of clamp(x, 0, 1) [B][C][ny][nx])"""
    H, W = x.shape[2:]
    (Yp, Xp), (Ym, Xm) = _samplers(base_x, frac_x, base_y, frac_y, H, W)
    v = torch.clamp(x.double(), 0, 1)
    gs = lambda im, Y, X: Y @ im @ X.t()  # noqa: E731
    return gs(mask.double(), Yp, Xp) * gs(mask.double(), Ym, Xm), gs(v, Yp, Xp), gs(v, Ym, Xm)


def shift_l1(x, mask, base_x, frac_x, base_y, frac_y, with_mag=False):
    """partial[b][i] = sum_{c,j} M(i,j) |GS+(v) - GS-(v)|; mag: sum_{c,j} |M| (GS+(v) + GS-(v))"""
    M, gp, gm = shift_l1_parts(x, mask, base_x, frac_x, base_y, frac_y)
    out = (M * (gp - gm).abs()).sum(dim=(1, 3))
    return (out, (M.abs() * (gp + gm)).detach().sum(dim=(1, 3))) if with_mag else out


def shift_l1_grad(x, mask, base_x, frac_x, base_y, frac_y, g):
    """dx = d/dx sum_b g[b] sum_i partial[b][i]; mag: the adjoint of |G| with the same weights; cnt: the number of nonzero products a pixel
    adds; tie: the pixels reached by an output position whose sign is within 4 u of its scale from the switch (fractional taps only: with
    integer taps both samples are stored values and their difference's sign is exact)"""
    xd = _d(x).requires_grad_(True)
    (shift_l1(xd, _d(mask), base_x, frac_x, base_y, frac_y) * _d(g)[:, None]).sum().backward()
    H, W = x.shape[2:]
    M, gp, gm = shift_l1_parts(_d(x), _d(mask), base_x, frac_x, base_y, frac_y)
    G = (M.abs() * _d(g).abs()[:, None, None, None]).expand_as(gp)
    d = gp - gm
    integer = bool((frac_x == 0).all()) and bool((frac_y == 0).all())
    near = (d.abs() <= 4 * U * (gp + gm)) & (M != 0) & ((d != 0) | (not integer))
    mag = torch.zeros_like(_d(x))
    cnt = torch.zeros_like(_d(x))
    tie = torch.zeros_like(_d(x))
    for Y, X in _samplers(base_x, frac_x, base_y, frac_y, H, W):
        mag += Y.t() @ G @ X
        cnt += (Y != 0).double().t() @ (G != 0).double() @ (X != 0).double()
        tie += (Y != 0).double().t() @ near.double() @ (X != 0).double()
    return xd.grad, mag, cnt, tie > 0


def tight_ranges(base, n_out, size):
    """ranges [2][size][2]: per sign and source index the half-open range of outputs whose taps (base, base + 1) touch it; (0, 0) where none"""
    r = torch.zeros(2, size, 2, dtype=torch.int32)
    for s in (0, 1):
        for src in range(size):
            hit = torch.nonzero((base[s] == src) | (base[s] + 1 == src)).flatten()
            if hit.numel():
                r[s, src, 0], r[s, src, 1] = int(hit.min()), int(hit.max()) + 1
    return r


# ------------------------------------------------------------------------------------------------ esr_scribble*
LAB_L1, LAB_CON, LAB_TV = 0x80, 0x40, 0x3F


def scribble(x, desired, labels, i0):
    """sum_y partial[b][y][5] = (l1, tv_d, tv_v, tv_h, con) per image -> [B][5]; i0 None: con = 0 (bit 6 ignored)"""
    v = torch.clamp(x.double(), 0, 1)
    lab = torch.as_tensor(labels).long()
    t = lab & LAB_TV
    s = lambda q: q.sum(dim=(1, 2, 3))  # noqa: E731
    l1 = s(((lab & LAB_L1) != 0) * (v - desired.double()).abs())

    def pair(a, b, ta, tb):
        return s(((ta == tb) & (ta > 0)) * (a - b).abs())
    tv_d = pair(v[..., :-1, :-1], v[..., 1:, 1:], t[:-1, :-1], t[1:, 1:]) + pair(v[..., 1:, :-1], v[..., :-1, 1:], t[1:, :-1], t[:-1, 1:])
    tv_v = pair(v[..., :-1, :], v[..., 1:, :], t[:-1, :], t[1:, :])
    tv_h = pair(v[..., :, :-1], v[..., :, 1:], t[:, :-1], t[:, 1:])
    con = s(((lab & LAB_CON) != 0) * (v - i0.double()).abs()) if i0 is not None else torch.zeros_like(l1)
    return torch.stack([l1, tv_d, tv_v, tv_h, con], 1)


def scribble_weights(C, H, W):
    """the weights of (l1, tv_d, tv_v, tv_h) in L_b; a term whose frame is empty (H = 1 or W = 1) has weight 0"""
    inv = lambda n: 1.0 / n if n > 0 else 0.0  # noqa: E731
    return torch.tensor([inv(C * H * W), inv(C * (H - 1) * (W - 1)), inv(C * (H - 1) * W), inv(C * H * (W - 1))], dtype=torch.float64)


def scribble_grad(x, desired, labels, i0, g, g_con):
    """dx = d/dx (sum_b g[b] L_b + g_con sum_b con_b); mag [B]: |g_b| (w_l1 + 4 w_d + 2 w_v + 2 w_h) + |g_con|, every term present"""
    xd = _d(x).requires_grad_(True)
    p = scribble(xd, _d(desired), labels, _d(i0))
    w = scribble_weights(*x.shape[1:])
    ((p[:, :4] * w).sum(1) * _d(g)).sum().backward(retain_graph=True)
    if i0 is not None:
        (g_con * p[:, 4].sum()).backward()
    mag = _d(g).abs() * float(w[0] + 4 * w[1] + 2 * w[2] + 2 * w[3]) + abs(g_con)
    return xd.grad, mag[:, None, None, None]


# ------------------------------------------------------------------------------------------------ esr_pairmin*
def definition64(x, clamp01, mask, init, w):
    """float64: Z_loss [B] of the definition (the reference's expression, :688-699) with the graph attached to x, and the excluded positions
    [C, H, W] of the module docstring"""
    D = torch.clamp(x, 0, 1) if clamp01 else x
    B = D.size(0)
    dist = (D.unsqueeze(0) - D.unsqueeze(1)).abs() + torch.eye(B, dtype=D.dtype, device=D.device).view(B, B, 1, 1, 1)        # [a, b, ...]
    v = dist.min(dim=0)[0]
    if init is not None:
        v = v - w * (D - init.double()).abs()
    if mask is not None:
        v = v * mask.double()
    Z = -v.mean(dim=(1, 2, 3))
    with torch.no_grad():
        if B == 1:
            return Z, torch.zeros(D.shape[1:], dtype=torch.bool, device=D.device)
        two, idx = torch.topk(dist, 2, dim=0, largest=False)                                  # the two smallest over a, and who they are
        tied = (two[1] - two[0]) < TIE                                                        # [b, ...]
        raw = x.detach()
        clamped = ((raw <= 0) | (raw >= 1)) if clamp01 else torch.zeros_like(raw, dtype=torch.bool)
        both_clamped = torch.gather(clamped, 0, idx[0]) & torch.gather(clamped, 0, idx[1])
        excluded = (tied & ~both_clamped).any(dim=0)
    return Z, excluded


def _pairmin_v(xc, lo, hi, clamp01, mask_flat, init, w, highest_on_tie=False):
    """xc [Bg][m] (a chunk of elements) -> v [hi - lo][m], |terms| [hi - lo][m], tie [m]"""
    I = torch.clamp(xc, 0, 1) if clamp01 else xc
    Bg = I.size(0)
    dist = (I[lo:hi, None] - I[None]).abs()                                                      # [r, a, m]
    r = torch.arange(lo, hi)
    dist = dist.clone()
    dist[r - lo, r] = 1.0
    # the winner is named explicitly (torch.min leaves the choice on a tie open): the LOWEST index a among the minima, the diagonal as index r
    low = dist.detach().min(1, keepdim=True)[0]
    eq = dist.detach() == low
    if highest_on_tie:
        first = eq & (eq.flip(1).cumsum(1).flip(1) == 1)
    else:
        first = eq & (eq.cumsum(1) == 1)
    near = (dist * first).sum(1)
    v, mag = near, near.detach().clone()
    if init is not None:
        t = w * (I[lo:hi] - init).abs()
        v, mag = v - t, mag + t.detach().abs()
    if mask_flat is not None:
        v, mag = v * mask_flat, mag * mask_flat.abs()
    return v, mag


def pairmin(x, lo, hi, clamp01, mask, init, w, chunk=None, drop=None):
    """sum_k partial[r - lo][k] = sum_e v(r, e) -> [hi - lo], and mag.  init: [1 or hi - lo][C][H][W] or None.  `drop`: a boolean [n] of elements
    left out (planted errors)."""
    Bg = x.size(0)
    chunk = chunk or max(64, (1 << 23) // (Bg * (hi - lo)))
    xf = x.double().reshape(Bg, -1)
    n = xf.size(1)
    hw = x.size(2) * x.size(3)
    mf = None if mask is None else mask.double().flatten().repeat(n // hw)
    inf = None if init is None else init.double().reshape(init.size(0), -1).expand(hi - lo, n)
    out = torch.zeros(hi - lo, dtype=torch.float64)
    mag = torch.zeros(hi - lo, dtype=torch.float64)
    for e0 in range(0, n, chunk):
        sl = slice(e0, min(n, e0 + chunk))
        v, m = _pairmin_v(xf[:, sl], lo, hi, clamp01, None if mf is None else mf[sl], None if inf is None else inf[:, sl], w)
        if drop is not None:
            v, m = v * ~drop[sl], m * ~drop[sl]
        out, mag = out + v.sum(1), mag + m.sum(1)
    return out, mag


def pairmin_grad(x, lo, hi, clamp01, mask, init, w, scale, chunk=None, highest_on_tie=False):
    """dx [hi - lo][C][H][W] = scale d/dx[lo:hi] sum over ALL Bg rows of sum_e v(r, e) (init applies to the rows [lo, hi) as the ABI hands it
    only those); tie [C][H][W]: the positions of definition64's rule, evaluated on the same chunk"""
    Bg = x.size(0)
    chunk = chunk or max(64, (1 << 23) // (Bg * Bg))
    xf = _d(x).reshape(Bg, -1)
    n = xf.size(1)
    hw = x.size(2) * x.size(3)
    mf = None if mask is None else _d(mask).flatten().repeat(n // hw)
    inf = None if init is None else _d(init).reshape(init.size(0), -1).expand(hi - lo, n)
    dx = torch.zeros(hi - lo, n, dtype=torch.float64)
    tie = torch.zeros(n, dtype=torch.bool)
    for e0 in range(0, n, chunk):
        sl = slice(e0, min(n, e0 + chunk))
        xc = xf[:, sl].clone().requires_grad_(True)
        msl = None if mf is None else mf[sl]
        v, _ = _pairmin_v(xc, 0, Bg, clamp01, msl, None, 0.0, highest_on_tie)
        tot = v.sum()
        if inf is not None:
            I = torch.clamp(xc[lo:hi], 0, 1) if clamp01 else xc[lo:hi]
            t = w * (I - inf[:, sl]).abs()
            tot = tot - (t if msl is None else t * msl).sum()
        (scale * tot).backward()
        dx[:, sl] = xc.grad[lo:hi]
        if Bg > 1:
            with torch.no_grad():
                I = torch.clamp(xc, 0, 1) if clamp01 else xc.detach()
                dist = (I[:, None] - I[None]).abs() + torch.eye(Bg, dtype=torch.float64)[:, :, None]
                two, idx = torch.topk(dist, 2, dim=0, largest=False)
                raw = xc.detach()
                clamped = ((raw <= 0) | (raw >= 1)) if clamp01 else torch.zeros_like(raw, dtype=torch.bool)
                both = torch.gather(clamped, 0, idx[0]) & torch.gather(clamped, 0, idx[1])
                tie[sl] = (((two[1] - two[0]) < TIE) & ~both).any(0)
    return dx.reshape(hi - lo, *x.shape[1:]), tie.reshape(x.shape[1:])
