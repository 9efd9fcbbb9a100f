"""EPI_RESIN with the K loop cut into plain and residual chunk ranges (esr_conv.hip: `span`): the residual slice at every position of K.

The 192->64 conv that ends a dense block adds its residual (a channel-group slice of its own input) inside the K loop, from the staged LDS
tile.  Only the chunks [resin_g0 / 2, ceil((resin_g0 + ceil(cout / 8)) / 2)) carry that code; the chunks in front of and behind them run the
plain body, and the PARTLO kernels cut both kinds of range again at lo_chunks.  The one-stage kernels (lds_stages 1) unroll the residual
chunks, the k-th with its pair of output groups as constants and one arm per parity of resin_g0; the two-stage kernels (lds_stages 2) loop
over them and find the groups at run time.  A wrong range bound or group pair drops, doubles or misplaces the residual of whole channel groups, so every case here is a launch of test_gpu_conv_contract.py's case builder held to that file's element-wise bound for its
resin / resin_res2 cases (run(): float64 reference of the stored operands, c_w / c_out of the format, planted errors rejected, sentinels kept).

Shapes: B = 2 at 11 x 80 (two column tiles, a ragged last tile row) and at 7 x 37.  Layouts (LAYOUTS): the slice's first group resin_g in
{0, 1, 2, 5} of in1, with and without an odd-width in0 group in front (which makes an even resin_g an odd resin_g0 and the reverse), for
cout 64, 40 (five groups: a half-filled last pair) and 16, the slice ending with the last input group (`tail` 0: with an odd group count the
last chunk's second group is past the end), three groups before it, or far enough before it that the launch has 12 chunks.  The host
admits no slice that reaches past the input (conv_plan), so the clamp of the range to the chunk count is met at its boundary there and, in
the PARTLO cases, inside the range: a residual range that is longer than what is left of the span with lo planes.
"""
import pytest
import torch

import test_gpu_conv_contract as CT
from test_gpu_conv_contract import Case, run

pytestmark = pytest.mark.gpu

SHAPES = {'11x80': (2, 11, 80), '7x37': (2, 7, 37)}
RESIN = dict(res1='resin', act_slope=1.0, alpha=0.2, beta1=1.0)


def _layouts():
    out = []
    for g in (0, 1, 2, 5):
        for lat in (0, 3):
            for i, cout in enumerate((64, 40, 16)):
                nout = (cout + 7) // 8
                first = 1 if lat else 0
                # groups of in1 behind the slice: none / three / up to 12 chunks (24 groups with in0's)
                tail = (0, 3, 24 - first - g - nout)[(i + g + first) % 3]
                out.append((g, lat, cout, tail))
    return out


LAYOUTS = _layouts()


def test_layouts_cover_what_they_claim():
    """No GPU work: the table has the slice at the start, in the middle and at the very end of K, odd and even resin_g0, and 12 chunks."""
    ncps, ends, g0s = set(), set(), set()
    for g, lat, cout, tail in LAYOUTS:
        first, nout = (1 if lat else 0), (cout + 7) // 8
        G = first + g + nout + tail
        ncps.add((G + 1) // 2)
        ends.add('end' if tail == 0 else 'mid')
        g0s.add((first + g) & 1)
        if first + g == 0:
            ends.add('start')
    assert max(ncps) == 12 and ends == {'start', 'mid', 'end'} and g0s == {0, 1}
    # an odd group count with the slice at the end: the last residual chunk's second group does not exist
    assert any(tail == 0 and ((1 if lat else 0) + g + (cout + 7) // 8) % 2 == 1 for g, lat, cout, tail in LAYOUTS)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('stages', [1, 2])
@pytest.mark.parametrize('res2', [False, True], ids=['resin', 'resin_res2'])
@pytest.mark.parametrize('fmt', ['split', 'bf16', 'f16'])
def test_slice_positions(fmt, res2, stages, shape):
    """Every layout, with and without RES2, in both LDS forms."""
    B, H, W = SHAPES[shape]
    for i, (g, lat, cout, tail) in enumerate(LAYOUTS):
        nout = (cout + 7) // 8
        run(Case(fmt=fmt, B=B, H=H, W=W, cin=8 * (g + nout + tail), cout=cout, lat=lat, resin_g=g, res2=res2, lds_stages=stages, seed=3 + i,
                 **RESIN))


def _lo_groups(first, ncg1, in1_lo_groups):
    """K groups whose lo plane the launch multiplies (whole chunks: run() of the contract tests)."""
    return 2 * ((first + in1_lo_groups + 1) // 2) if 0 < in1_lo_groups < ncg1 else first + ncg1


def _run_partlo(case):
    """run() with the residual of the groups behind the lo range restated.  The builder's reference adds hi + lo for every group of the slice; the
    descriptor contract (esr_hip.h, in1_lo_groups) says that the lo plane of a group behind the leading ones is not read, and the builder
    fills exactly those planes with hi-sized junk.  The epilogue of a RESIN launch is linear (act_slope 1), so the reference is corrected
    by beta1 * lo of those groups, the bound's magnitude S by |beta1| (|hi| - |hi + lo|), and the comparison is run()'s."""
    c, f = case, case.f
    made = []

    base = CT.Buf

    class Rec(base):                                                    # run() keeps its buffers to itself: note them as it makes them
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            made.append(self)

    CT.Buf = Rec
    try:
        res = run(c, check_only=True)
    finally:
        CT.Buf = base
    x1 = made[0]                                                        # run() lays out in1's buffer first
    first, ncg1, nout = (1 if c.lat else 0), (c.cin + 7) // 8, (c.cout + 7) // 8
    logr = _lo_groups(first, ncg1, c.in1_lo_groups)
    ref, S = res.ref.clone(), res.S.clone()
    fixed = 0
    for j in range(nout):
        if first + c.resin_g + j < logr:
            continue
        gi = c.in1_off + c.resin_g + j
        hi = x1.values(gi, 1, lo=False)[:, :, 1:-1, 1:-1]
        both = x1.values(gi, 1, lo=True)[:, :, 1:-1, 1:-1]
        ref[:, 8 * j:8 * j + 8] -= c.beta1 * (both - hi)
        S[:, 8 * j:8 * j + 8] += abs(c.beta1) * (hi.abs() - both.abs())
        fixed += 1
    c_out = f.c_out_hilo if (c.out_lo and f.planes == 2) else f.c_out_hi
    K = 9 * 8 * (first + ncg1)

    def excess(ref_):
        err = (res.y - ref_).abs()
        e = err / (f.c_w * S + c_out * ref_.abs() + K * 2.0 ** -24 * S)
        e[err == 0] = 0.0
        e[torch.isnan(err)] = float('inf')
        return float(e.max())

    worst = excess(ref)
    print('partlo %s lat %d resin_g %d cout %d in1_lo_groups %d: %d residual groups hi-only, worst |y-ref|/bound %.3g' % (
        c.fmt, c.lat, c.resin_g, c.cout, c.in1_lo_groups, fixed, worst))
    assert worst <= 1.0
    if fixed:
        assert excess(res.ref) > 1.0, 'the comparator accepts a residual read with the lo plane it must not read'
    # the residual taken from the neighbouring group (every group of the slice moved by one) must be rejected as well
    moved = ref.clone()                                                 # (ref = linear part + beta1 * slice: only the slice term moves)
    sl = []
    for j in range(nout + 1):
        gi = c.in1_off + c.resin_g + j
        if gi >= x1.ncg:
            gi = c.in1_off + c.resin_g
        lo = first + c.resin_g + j < logr
        sl.append(x1.values(gi, 1, lo=lo)[:, :, 1:-1, 1:-1])
    for j in range(nout):
        moved[:, 8 * j:8 * j + 8] += c.beta1 * (sl[j + 1] - sl[j])
    assert excess(moved) > 1.0, 'the comparator accepts the residual of the neighbouring group'
    return fixed


# (fmt, lat, resin_g, cout, tail, in1_lo_groups): lo range [0, first + in1_lo_groups) rounded up to chunks, slice [first + resin_g, + cout / 8)
PARTLO = [
    ('f16x3', 0, 5, 64, 3, 2),      # before: lo groups [0, 2), slice [5, 13): every residual group hi-only, odd resin_g0
    ('f16x3', 3, 2, 64, 3, 2),      # inside by one group: in0 + 2 groups round up to the chunk boundary 4, slice [3, 11)
    ('f16x2', 0, 2, 64, 3, 6),      # inside: the residual range [1, 5) is cut at lo_chunks = 3
    ('f16x3', 3, 1, 40, 0, 4),      # inside, five groups [2, 7) at the very end of seven: the last chunk's second group is past the end
    ('f16x3', 0, 1, 16, 3, 2),      # the cut between the slice's two chunks: group 1 with lo (chunk 0), group 2 without (chunk 1)
    ('f16x2', 0, 0, 64, 3, 8),      # behind: the slice is the leading groups, all with lo (a dense block's last conv in `mixed`)
    ('f16x3', 3, 0, 64, 15, 9),     # behind with in0 in front: slice [1, 9), lo groups [0, 10), 12 chunks
    ('f16x2', 0, 2, 16, 3, 6),      # behind by a whole chunk: slice [2, 4), lo groups [0, 6)
]


@pytest.mark.parametrize('stages', [1, 2])
@pytest.mark.parametrize('fmt,lat,g,cout,tail,lo', PARTLO, ids=['%s-l%d-g%d-c%d-t%d-lo%d' % p for p in PARTLO])
def test_partial_lo_cuts(fmt, lat, g, cout, tail, lo, stages):
    """PARTLO kernels: in1_lo_groups before, inside and behind the residual range; both shapes, RES2 on the first."""
    nout = (cout + 7) // 8
    for k, (B, H, W) in enumerate(SHAPES.values()):
        _run_partlo(Case(fmt=fmt, B=B, H=H, W=W, cin=8 * (g + nout + tail), cout=cout, lat=lat, resin_g=g, res2=(k == 0), in1_lo_groups=lo,
                         lds_stages=stages, seed=11 + k, **RESIN))


def test_partial_lo_table_has_all_three():
    """No GPU work: the PARTLO table has the cut in front of, inside and behind the slice, and every entry is a partial-lo launch."""
    kinds = set()
    for fmt, lat, g, cout, tail, lo in PARTLO:
        first, nout = (1 if lat else 0), (cout + 7) // 8
        ncg1 = g + nout + tail
        assert 0 < lo < ncg1
        logr, q0 = _lo_groups(first, ncg1, lo), first + g
        kinds.add('before' if logr <= q0 else ('behind' if logr >= q0 + nout else 'inside'))
    assert kinds == {'before', 'inside', 'behind'}


@pytest.mark.parametrize('fmt', ['split', 'bf16', 'f16', 'f16x2'])
def test_two_slice_form(fmt):
    """A 64-channel launch of few tiles runs as two 32-channel slices of the 32-channel kernel: slice 1's residual groups start four groups
    further along the input (the kernel shifts resin_g0).  test_gpu_conv_contract.py::test_two_slice_form's configuration (the library takes
    this form only when it chooses the LDS form itself: lds_stages 0), slice positions as above."""
    assert CT.tiling(2, 12, 17, 64, split=CT.FMTS[fmt].planes == 2)[3] == 2
    assert CT.tiling(2, 12, 17, 64, split=CT.FMTS[fmt].planes == 2, lds_stages=1)[3] == 1
    for i, (g, lat, tail) in enumerate([(0, 0, 0), (1, 0, 1), (1, 3, 0), (2, 3, 3), (5, 0, 11)]):
        for res2 in (False, True):
            run(Case(fmt=fmt, B=2, H=12, W=17, cin=8 * (g + 8 + tail), cout=64, lat=lat, resin_g=g, res2=res2, lds_stages=0, seed=20 + i, **RESIN))
