"""The weight gradient's host-side queries (they need no device and launch nothing): esr_conv3x3_wgrad_tiling, _workspace_floats and the batch
queries _batch_unit / _batch_workspace_bytes / _batch_part_workspace_bytes all answer from the one launch plan in csrc/esr_bwd.hip (WgradPlan), so
this pins which tiles, slices and kernel forms every descriptor gets.  Descriptors carry fake pointers, as _wgrad_desc in test_host_api.py.
Every literal below (the Counter, the digest, the units and byte counts, the return codes) was recorded from the library as it was BEFORE the
plan was introduced: the restructuring must answer exactly as the code it replaced."""
import ctypes as C
import hashlib
import struct
from collections import Counter

import pytest

from esr_hip import _lib

E_ARG = -1
LAT27, MAIN27, S2D, FAST_COPY = 1, 2, 4, 8
S2D_MASKS = (432, 216, 54, 27)
OTHER_MASKS = (27, 54, 216, 432)

OPERANDS = [(0, True), (0, False), (1, False)]                  # (fmt, hi+lo): bf16 hi+lo, bf16 one plane, fp16 one plane
HW = [(4, 4), (8, 8), (8, 32), (9, 31), (16, 16), (46, 4), (52, 52), (18, 70)]


@pytest.fixture(scope='module')
def h():
    return _lib.load_library()


def _desc(fmt=0, split=True, B=2, H=16, W=16, cin=128, cout=64, lat=0, ups=1, masks=None):
    v = lambda ncg, hh, ww: _lib.ActView(16, 32 if split else None, ncg, hh, ww, 0, 0, fmt)
    d = _lib.WgradDesc()
    d.dy, d.x = v((cout + 7) // 8, H, W), v((cin + 7) // 8, H // ups, W // ups)
    if lat:
        d.xlat = v(1, H, W)
    d.lat, d.upsample, d.cout, d.cin_main, d.B, d.H, d.W, d.alpha, d.dw = lat, ups, cout, cin, B, H, W, 1.0, 48
    if masks:
        d.tap_masks[:] = masks
    return d


def _grid():
    for fmt, split in OPERANDS:
        for B in (1, 2, 5):
            for H, W in HW:
                for cin in (3, 13, 64, 128, 256):
                    for cout in (3, 24, 64, 128):
                        for lat, ups in ((0, 1), (2, 1), (5, 1), (0, 2)):
                            if ups == 2 and (H % 2 or W % 2):
                                continue
                            for masks in (None, S2D_MASKS, OTHER_MASKS):
                                yield dict(fmt=fmt, split=split, B=B, H=H, W=W, cin=cin, cout=cout, lat=lat, ups=ups, masks=masks)


def _groups(kw, forms):
    """(input tiles x output tiles, output tiles) of a layer: 32 channels each, the latent segment one more input tile; a main input run as the
    27-column tile (ESR_WGRAD_FORM_MAIN27) is one tile."""
    mt = -(-kw['cout'] // 32)
    ncit = 1 if forms & MAIN27 else -(-kw['cin'] // 32) + (1 if kw['lat'] else 0)
    return ncit * mt, mt


# recorded from the library before the plan: how the grid's points divide over (tile shape, ESR_WGRAD_FORM_* bits), and sha256 over their
# (tiles x, tiles y, shape, slices, forms) packed as five little-endian int32 in grid order
SWEEP_COUNTS = {(0, 0): 5652, (0, 1): 1248, (0, 2): 288, (0, 4): 624, (0, 5): 192, (0, 8): 4800, (0, 9): 2688, (0, 10): 576, (0, 12): 288, (0, 13): 192,
                (1, 4): 48, (1, 12): 48, (2, 4): 48, (2, 12): 48}
SWEEP_DIGEST = '9acb4752f8737b7fe855e48c2fcef7611a9dcac907b2b94cd5d3538ec5a1045d'


def test_single_launch_queries_over_the_grid(h):
    t = (C.c_int32 * 5)()
    counts, digest, slices, npoints = Counter(), hashlib.sha256(), set(), 0
    for kw in _grid():
        d = _desc(**kw)
        rc = h.esr_conv3x3_wgrad_tiling(C.byref(d), t)
        if rc != 0:                                              # a refused point: the entry point refuses it the same way (nothing is launched)
            d.workspace, d.workspace_floats = 64, 1 << 40
            assert h.esr_conv3x3_wgrad(C.byref(d), None) == rc, kw
            t[:] = (rc, 0, 0, 0, 0)
        else:
            tx, ty, shape, ns, forms = t
            ngroups, mt = _groups(kw, forms)
            want = 1 if ns == 1 else ngroups * ns * 9216 + mt * ns * 32
            assert h.esr_conv3x3_wgrad_workspace_floats(C.byref(d)) == want, (kw, tuple(t))
            counts[shape, forms] += 1
            slices.add(min(ns, 2))
        digest.update(struct.pack('<5i', *t))
        npoints += 1
    assert npoints == 3 * 3 * (7 * 4 + 1 * 3) * 5 * 4 * 3          # (9, 31) has no upsample = 2 points
    assert {s for s, _ in counts} == {0, 1, 2}
    for bit in (LAT27, MAIN27, S2D, FAST_COPY):
        assert any(f & bit for _, f in counts), bit
    assert slices == {1, 2}                                      # nslices == 1 and nslices > 1 both occur
    assert dict(counts) == SWEEP_COUNTS, dict(counts)
    assert digest.hexdigest() == SWEEP_DIGEST, digest.hexdigest()


# ---- batch queries: three descriptor sets, their (unit, workspace bytes) as recorded from the library before the plan
PLAIN = [dict(B=5, H=52, W=52, cin=256, cout=128), dict(B=2, H=52, W=52, cin=96, cout=32), dict(B=2, H=104, W=104, cin=64, cout=64, ups=2),
         dict(B=2, H=104, W=104, cin=64, cout=3), dict(B=2, H=9, W=31, cin=13, cout=24), dict(B=2, H=52, W=52, cin=64, cout=64, lat=5)]
WITH_S2D = [dict(B=5, H=64, W=64, cin=256, cout=128, masks=S2D_MASKS), dict(B=2, H=32, W=32, cin=64, cout=64), dict(B=2, H=46, W=4, cin=64, cout=128),
            dict(B=2, H=8, W=8, cin=256, cout=128, masks=S2D_MASKS), dict(B=2, H=64, W=64, cin=40, cout=64, masks=OTHER_MASKS)]
WITH_27 = [dict(B=2, H=64, W=64, cin=3, cout=64), dict(B=5, H=128, W=128, cin=64, cout=64, lat=2), dict(B=2, H=32, W=32, cin=64, cout=64),
           dict(B=5, H=18, W=70, cin=128, cout=24, lat=3)]
SETS = {'plain': PLAIN, 's2d': WITH_S2D, 'lat27': WITH_27}
UNIT_SHAPES = 1 << 48                                            # the unit's flag: the set runs the 16x16 / 32x8 tile shapes
BATCH_LITERALS = {'plain': (4, 29346692), 's2d': (UNIT_SHAPES | 3, 34540804), 'lat27': (2, 41481092)}     # name -> (unit, workspace bytes)


def _arr(layers, **common):
    return (_lib.WgradDesc * len(layers))(*[_desc(**dict(l, **common)) for l in layers])


def _work_items(layers, unit):
    """Workgroups of the batch launch for these layers under `unit`: a layer's tiles (the shape with the fewest, when the set has the shapes and the
    layer can take them: bf16, no upsample, no 27-column tile) are cut into ceil(tiles / granule) slices, each run by every group."""
    shapes, granule, n = bool(unit & UNIT_SHAPES), unit & (UNIT_SHAPES - 1), 0
    for l in layers:
        lat, cin = l.get('lat', 0), l['cin']
        any_shape = shapes and l.get('ups', 1) == 1 and not (0 < lat <= 3) and not (lat == 0 and cin <= 3)
        tiles = min(-(-l['W'] // tw) * -(-l['H'] // th) for tw, th in ((32, 8), (16, 16), (8, 32))[:3 if any_shape else 1]) * l['B']
        ns = max(1, min(tiles, -(-tiles // granule)))
        ngroups, _ = _groups(dict(l, lat=lat), MAIN27 if lat == 0 and cin <= 3 and l.get('ups', 1) == 1 else 0)
        n += ngroups * ns
    return n


def _partial_bytes(h, layers, unit):
    """The partial-sum bytes inside _part_workspace_bytes: the workspace less the descriptor table (measured on as many layers of one workgroup and no
    partial sums each: their map is one round of 1024 16-byte entries, then 4 bytes) and less this set's workgroup map."""
    n = len(layers)
    tiny = [dict(B=1, H=4, W=4, cin=8, cout=8)] * n
    table = h.esr_conv3x3_wgrad_batch_workspace_bytes(_arr(tiny), n) - 1024 * 16 - 4
    assert table > 0 and table % 256 == 0
    items = -(-_work_items(layers, unit) // 1024) * 1024
    return h.esr_conv3x3_wgrad_batch_part_workspace_bytes(_arr(layers), n, unit) - table - items * 16 - 4


@pytest.mark.parametrize('name', sorted(SETS))
def test_batch_queries(h, name):
    layers = SETS[name]
    arr, n = _arr(layers), len(layers)
    unit, need = h.esr_conv3x3_wgrad_batch_unit(arr, n), h.esr_conv3x3_wgrad_batch_workspace_bytes(arr, n)
    assert (unit, need) == BATCH_LITERALS[name], (unit, need)
    assert bool(unit & UNIT_SHAPES) == (name == 's2d')
    assert h.esr_conv3x3_wgrad_batch_part_workspace_bytes(arr, n, unit) == need
    # split into parts that are sized with the whole set's unit: every layer is cut as in the one launch, so the partial sums add up
    whole = _partial_bytes(h, layers, unit)
    assert whole >= 0 and whole % 4 == 0
    for cut in range(1, n):
        parts = [layers[:cut], layers[cut:]] if cut > 1 else [layers[:1], layers[1:2], layers[2:]]
        assert sum(_partial_bytes(h, p, unit) for p in parts) == whole, cut


def test_batch_queries_cover_partial_sums_and_single_slices(h):
    """The three sets together hold layers that add straight into dW (no partial sums) and layers that go through the workspace."""
    t = [_partial_bytes(h, [l], h.esr_conv3x3_wgrad_batch_unit(_arr(s), len(s))) for s in SETS.values() for l in s]
    assert 0 in t and any(v > 0 for v in t)


def test_batch_queries_refuse_as_before(h):
    arr = _arr(PLAIN)
    for f in (h.esr_conv3x3_wgrad_batch_unit, h.esr_conv3x3_wgrad_batch_workspace_bytes):
        assert f(arr, 0) == E_ARG and f(arr, -3) == E_ARG and f(None, 2) == E_ARG
    part = h.esr_conv3x3_wgrad_batch_part_workspace_bytes
    assert part(arr, 0, 7) == E_ARG and part(None, 2, 7) == E_ARG and part(arr, 2, -1) == E_ARG
    for field in ('B', 'H', 'W', 'cout', 'cin_main'):
        for bad in (0, -4):
            arr = _arr(PLAIN)
            setattr(arr[3], field, bad)
            assert h.esr_conv3x3_wgrad_batch_unit(arr, len(PLAIN)) == E_ARG, field
            assert h.esr_conv3x3_wgrad_batch_workspace_bytes(arr, len(PLAIN)) == E_ARG, field
            assert part(arr, len(PLAIN), 7) == E_ARG, field
            assert h.esr_conv3x3_wgrad_workspace_floats(C.byref(arr[3])) == E_ARG, field
            assert h.esr_conv3x3_wgrad_batch_unit(arr, 3) > 0          # the bad layer is not among the first three
