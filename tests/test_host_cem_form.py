"""esr_cem_sep_form on the host (it needs no device): the wave-streaming rule as include/esr_hip.h states it, the streaming / tile boundary of the
downscale at a small image, and the argument errors.  The query is the shape part of the launch plans in csrc/esr_cem.hip, so this pins which kernel
form every geometry runs."""
from collections import Counter

import pytest

from esr_hip import _lib

HW = [(1, 1), (16, 16), (63, 65), (64, 64), (70, 40), (127, 129), (128, 128), (300, 200)]


@pytest.fixture(scope='module')
def form():
    return _lib.load_library().esr_cem_sep_form


def _wave(op, sf, k, pre, h, w):
    """The comment above esr_cem_sep_form: form 2 for low-resolution images of h * w >= 4096 pixels, sf 2 / 3 / 4 / 8 with ceil(k / sf) in 4..6; the
    upscale: sf 3 / 4 / 8 and 0 < pre < sf - 1; the LR filter: k = 27 or 35 and h * w >= 16384 pixels."""
    na = -(-k // sf)
    if op == 0:
        return h * w >= 4096 and sf in (2, 3, 4, 8) and 4 <= na <= 6
    if op == 1:
        return h * w >= 4096 and sf in (3, 4, 8) and 4 <= na <= 6 and 0 < pre < sf - 1
    return k in (27, 35) and h * w >= 16384


def test_wave_form_is_the_rule_the_header_states(form):
    counts = Counter()
    for op in range(3):
        for sf in range(1, 10):
            for k in range(1, 64, 2):
                for pre in range(sf):
                    for h, w in HW:
                        got = form(op, sf, k, pre, h, w)
                        assert got in ((0, 1, 2) if op == 0 else (0, 2)), (op, sf, k, pre, h, w, got)
                        assert (got == 2) == _wave(op, sf, k, pre, h, w), (op, sf, k, pre, h, w, got)
                        counts[op, got] += 1
    # how the 34,560 calls of this grid divide (recorded when the plans were introduced)
    assert counts == {(0, 0): 4944, (0, 1): 6024, (0, 2): 552, (1, 0): 11168, (1, 2): 352, (2, 0): 11340, (2, 2): 180}, counts


def test_streaming_downscale_begins_and_ends_where_it_did(form):
    """h = w = 16 (no wave form): the odd k below 100 at which the downscale takes the streaming tile kernel (form 1) instead of the tile kernel (form 0)."""
    ks = {sf: [k for k in range(1, 100, 2) if form(0, sf, k, 0, 16, 16) == 1] for sf in range(1, 13)}
    assert [ks[sf][0] for sf in range(2, 11)] == [89, 73, 57, 41, 25, 9, 1, 1, 1]
    assert (ks[8][-1], ks[9][-1], ks[10][-1]) == (65, 33, 3)
    assert ks[1] == [] and ks[11] == [] and ks[12] == []
    assert all(form(0, sf, k, 0, 16, 16) == 0 for sf in range(1, 13) for k in range(1, 100, 2) if k not in ks[sf])


@pytest.mark.parametrize('args', [(3, 4, 17, 1, 64, 64), (-1, 4, 17, 1, 64, 64), (0, 4, 16, 1, 64, 64), (1, 0, 17, 0, 64, 64), (2, 4, 27, 1, 0, 64),
                                  (0, 4, 17, 1, 64, 0)])
def test_bad_arguments_are_refused(form, args):
    assert form(*args) == _lib.ESR_E_ARG
