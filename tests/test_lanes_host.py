"""CPU-only tests of the rule that decides which inference forwards run as two half-batch lanes (esr_hip.act.forward_lane_count and the
helpers around it): a pure function of the precision, the tiles of a lane's dense-block launch and the CU count."""
from esr_hip import act as A

CUS = 256          # MI355X


def lanes_for(precision, B, h, w, cus=CUS):
    planes = A.act_planes({'split': True, 'bf16': False}.get(precision, precision))[0]
    n = A.LANE_TABLE.get(precision, 1)
    return A.forward_lane_count(precision, (B // max(n, 1)) * A.dense_conv_tiles(h, w, planes), cus)


def test_the_headline_forward_runs_as_two_lanes():
    assert A.dense_conv_tiles(148, 148, 2) == 60          # 32 x 60 = the 1920 tiles per launch of profiles/r07_v1_split_conv_launches.csv
    assert lanes_for('split', 32, 148, 148) == 2
    assert A.lane_batches(32, 2) == [[(0, 16)], [(16, 16)]]


def test_unmeasured_precisions_stay_single_lane():
    assert 'mixed' not in A.LANE_TABLE
    for precision in ('mixed', 'f16', 'f16x2', 'bf16'):
        assert lanes_for(precision, 32, 148, 148) == 1
        assert A.forward_lane_count(precision, 960, CUS) == 1


def test_lanes_with_fewer_tiles_than_slots_stay_single_lane():
    assert lanes_for('split', 32, 52, 52) == 1            # the training crops
    assert lanes_for('split', 1, 148, 148) == 1           # one image (B = 1: a lane of no images)
    assert lanes_for('split', 1, 52, 52) == 1
    assert lanes_for('split', 1, 32, 32) == 1             # configs[0]
    assert A.forward_lane_count('split', 2 * CUS - 1, CUS) == 1 and A.forward_lane_count('split', 2 * CUS, CUS) == 2
    # a smaller device has fewer slots to fill
    assert A.forward_lane_count('split', 300, 128) == 2
    # launches of many rounds have no tail worth filling
    assert A.forward_lane_count('split', A.LANE_MAX_ROUNDS * CUS + 1, CUS) == 1


def test_sub_batches_are_dealt_round_robin():
    assert A.lane_batches(3, 2) == [[(0, 2)], [(2, 1)]]
    assert A.lane_batches(5, 2, 4) == [[(0, 2), (3, 1)], [(2, 1), (4, 1)]]
    assert A.lane_batches(2, 2, 4) == [[(0, 1)], [(1, 1)]]
    for B, lanes, subs in ((32, 2, None), (32, 2, 4), (7, 2, 3), (5, 2, 4)):
        cut = sorted(s for lane in A.lane_batches(B, lanes, subs) for s in lane)
        assert cut[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(cut, cut[1:])) and cut[-1][0] + cut[-1][1] == B
