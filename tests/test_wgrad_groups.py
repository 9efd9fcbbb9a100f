"""Host tests of the generator's weight-gradient grouping (esr_hip.engine.wgrad_groups / cover_spans: plain Python, no torch tensors, no GPU)
on the RRDB-23 layer table: the exchange buckets of the one-stream backward and the readiness groups of the two-stream one.  The expected
groups are literals recorded from the grouping code this function replaced; the launches, streams and exchanged stretches follow them."""
import pytest

from esr_hip.engine import cover_spans, wgrad_groups

NB = 23


def layer_table():
    """(cout, cin) of every conv of an RRDB-23 x4 generator (nf 64, gc 32, no latent input) in the flat gradient buffer's order."""
    convs = [(64, 3)]
    for _ in range(3 * NB):
        convs += [(32, 64), (32, 96), (32, 128), (32, 160), (64, 192)]
    return convs + [(64, 64)] * 4 + [(3, 64)]          # lr_conv, up0, up1, hr0, hr1


def layers():
    out, o = [], 0
    for cout, cin in layer_table():
        out.append((o, o + cout * cin * 9 + cout))
        o = out[-1][1]
    return out


def record_order():
    """The layer of each descriptor in the order the backward records them: hr1, hr0, up1, up0, lr_conv, then every RDB from the last one,
    conv4 to conv0, and fea last — the reverse of the buffer's order."""
    return list(reversed(range(len(layer_table()))))


N = 16697987                # floats in the flat buffer
# 256 KB buckets: the flat start of every group and its number of descriptors (each group: the next descriptors, counted from the LAST one)
LO_256K = [0, 84832, 241600, 324640, 481408, 564448, 721216, 804256, 961024, 1044064, 1200832, 1283872, 1440640, 1523680, 1680448, 1763488, 1920256,
           2003296, 2160064, 2243104, 2399872, 2482912, 2639680, 2722720, 2879488, 2962528, 3119296, 3202336, 3359104, 3442144, 3598912, 3681952,
           3838720, 3921760, 4078528, 4161568, 4318336, 4401376, 4558144, 4641184, 4797952, 4880992, 5037760, 5120800, 5277568, 5360608, 5517376,
           5600416, 5757184, 5840224, 5996992, 6080032, 6236800, 6319840, 6476608, 6559648, 6716416, 6799456, 6956224, 7039264, 7196032, 7279072,
           7435840, 7518880, 7675648, 7758688, 7915456, 7998496, 8155264, 8238304, 8395072, 8478112, 8634880, 8717920, 8874688, 8957728, 9114496,
           9197536, 9354304, 9437344, 9594112, 9677152, 9833920, 9916960, 10073728, 10156768, 10313536, 10396576, 10553344, 10636384, 10793152,
           10876192, 11032960, 11116000, 11272768, 11355808, 11512576, 11595616, 11752384, 11835424, 11992192, 12075232, 12232000, 12315040,
           12471808, 12554848, 12711616, 12794656, 12951424, 13034464, 13191232, 13274272, 13431040, 13514080, 13670848, 13753888, 13910656,
           13993696, 14150464, 14233504, 14390272, 14473312, 14630080, 14713120, 14869888, 14952928, 15109696, 15192736, 15349504, 15432544,
           15589312, 15672352, 15829120, 15912160, 16068928, 16151968, 16308736, 16391776, 16548544, 16622400, 16696256]
COUNT_256K = [4] + [2, 3] * 68 + [2, 2, 2, 1]
LO_32M, COUNT_32M = [0, 8395072], [176, 175]
# two-stream groups: (first descriptor, count), each group's stretch of the buffer, the position (= descriptor index here) of every side launch
OVERLAP = {
    2: ([(0, 175), (175, 176)], [(8395072, N), (0, 8395072)]),
    3: ([(0, 117), (117, 117), (234, 117)], [(11116000, N), (5535840, 11116000), (0, 5535840)]),
    5: ([(0, 70), (70, 70), (140, 70), (210, 70), (280, 71)],
        [(13431040, N), (10073728, 13431040), (6716416, 10073728), (3359104, 6716416), (0, 3359104)]),
}


def check_partition(groups, nd):
    spans = sorted((lo, hi) for lo, hi, *_ in groups)
    assert spans[0][0] == 0 and spans[-1][1] == N
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(spans, spans[1:]))          # disjoint, no gap
    assert sorted(i for _, _, idx, _, _ in groups for i in idx) == list(range(nd))      # every descriptor in exactly one group


def test_layer_table():
    assert layers()[-1][1] == N and len(record_order()) == 351


@pytest.mark.parametrize('kb', [256, 32 * 1024])
def test_exchange_buckets_of_the_one_stream_backward(kb):
    L, dl = layers(), record_order()
    ready = list(range(len(dl)))
    groups = wgrad_groups(L, dl, ready, bucket_bytes=kb * 1024)
    check_partition(groups, len(dl))
    lo, count = (LO_256K, COUNT_256K) if kb == 256 else (LO_32M, COUNT_32M)
    assert len(groups) == len(lo) == len(count)
    assert all(not side and pos is None for *_, side, pos in groups)               # all on the main stream, behind the pass
    assert [g[0] for g in groups] == lo and [g[1] for g in groups] == lo[1:] + [N]
    last = len(dl)
    for (_, _, idx, _, _), c in zip(groups, count):
        assert idx == list(range(last - c, last))
        last -= c


@pytest.mark.parametrize('G', [2, 3, 5])
@pytest.mark.parametrize('bucket_bytes', [None, 32 << 20])
def test_readiness_groups_of_the_two_stream_backward(G, bucket_bytes):
    L, dl = layers(), record_order()
    ready = list(range(len(dl)))
    groups = wgrad_groups(L, dl, ready, bucket_bytes=bucket_bytes, overlap=G)
    check_partition(groups, len(dl))
    first_count, spans = OVERLAP[G]
    assert [(idx[0], len(idx)) for _, _, idx, _, _ in groups] == first_count
    assert all(idx == list(range(idx[0], idx[0] + len(idx))) for _, _, idx, _, _ in groups)
    assert [(lo, hi) for lo, hi, *_ in groups] == spans
    assert [side for *_, side, _ in groups] == [True] * (G - 1) + [False]
    # a side group goes in behind the launch that wrote its last dy: where the next group's first layer was recorded
    assert [pos for *_, pos in groups] == [f for f, _ in first_count[1:]] + [None]


def test_one_group_without_exchange_or_overlap():
    L, dl = layers(), record_order()
    assert wgrad_groups(L, dl, [None] * len(dl)) == [(0, N, list(range(len(dl))), False, None)]


def test_cover_spans():
    assert cover_spans([(10, 20), (30, 40), (0, 5)], 50) == [(5, 20), (20, 50), (0, 5)]
    assert cover_spans([(3, 7)], 9) == [(0, 9)]
