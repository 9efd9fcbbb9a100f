"""GPU tests (-m gpu) of inference forwards run as lanes (esr_run_lanes, include/esr_hip.h; RRDBEngine.forward_lanes): sub-batches of one
forward recorded as independent launch lists over disjoint images of the SAME buffer set and issued interleaved on two streams.  Images are
independent chains, so every lane form must give the single-lane result bit for bit; the caller's stream must see the call as ordered."""
import ctypes as C

import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform

pytestmark = pytest.mark.gpu


def make_net(lat=0, precision='split'):
    import models.modules.architecture as arch
    net = arch.RRDBNet(in_nc=3, out_nc=3, nf=64, nb=1, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA', upsample_mode='upconv',
                       latent_input='all_layers_HR_downscaled' if lat else None, num_latent_channels=lat)
    fill_formula_weights(net, gain=0.5)
    net = net.cuda()
    net.set_precision(precision)
    return net


def inputs(B, lat, seed):
    return seeded_uniform((B, 3 + lat * 16, 12, 16), seed).cuda()


def forward(net, x, lanes, subs=None):
    net.engine.forward_lanes, net.engine.forward_sub_batches = lanes, subs
    with torch.no_grad():
        return net(x, pad=2)


def fwd_plans(eng):
    return {k: p for b in eng._bufs.values() for k, p in b['_plans'].items() if k[0] == 'fwd'}


@pytest.mark.parametrize('precision,lat', [('split', 0), ('mixed', 0), ('split', 3)])
def test_lane_forwards_are_bit_identical_to_the_single_lane_forward(precision, lat):
    net = make_net(lat, precision)
    eng = net.engine
    for B, subs, layout in ((2, None, (((0, 1),), ((1, 1),))), (3, None, (((0, 2),), ((2, 1),))), (5, 4, (((0, 2), (3, 1)), ((2, 1), (4, 1))))):
        x = inputs(B, lat, 300 + B)
        ref = forward(net, x, 1).clone()
        got = forward(net, x, 2, subs)
        assert torch.equal(ref, got), (precision, lat, B)
        lane_plans = [p for k, p in fwd_plans(eng).items() if k[1][0] == B and p.side]
        assert len(lane_plans) == 1 and len(lane_plans[0].side) == 1                       # two streams: one side lane
        assert eng._lane_layout(B, 16, 20, x.device, False) == layout
        single = [p for k, p in fwd_plans(eng).items() if k[1][0] == B and not p.side][0]
        assert lane_plans[0].n_cmds + lane_plans[0].side[0].n_cmds == len(sum(layout, ())) * single.n_cmds
    # one image: nothing to split
    x1 = inputs(1, lat, 299)
    ref = forward(net, x1, 1).clone()
    assert torch.equal(ref, forward(net, x1, 2))
    assert not any(p.side for k, p in fwd_plans(eng).items() if k[1][0] == 1)


def test_replayed_lanes_follow_new_inputs_and_outputs():
    net = make_net()
    xs = [inputs(3, 0, 310 + i) for i in range(2)]
    ref = [forward(net, x, 1).clone() for x in xs]
    got = [forward(net, x, 2) for x in xs]                 # call 0 records the lanes, call 1 replays them with x and g patched per lane
    assert got[0].data_ptr() != got[1].data_ptr()
    for r, g in zip(ref, got):
        assert torch.equal(r, g)
    assert not torch.equal(ref[0], ref[1])


def test_event_bracket_covers_all_lanes_and_the_join_precedes_return():
    net = make_net()
    eng = net.engine
    x = inputs(3, 0, 320)
    ref = forward(net, x, 1).cpu()
    forward(net, x, 2)                                     # (recorded)
    torch.cuda.synchronize()
    e0, e1, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    eng._ev = (e0, e1)
    try:
        y = forward(net, x, 2)
    finally:
        eng._ev = None
    done.record()                                          # the caller's stream, right behind the forward
    done.synchronize()
    # no other synchronisation: the copy runs on a stream that waits for nothing
    with torch.cuda.stream(torch.cuda.Stream()):
        got = y.to('cpu', non_blocking=False)
    assert torch.equal(ref, got)
    assert e0.elapsed_time(e1) > 0


def test_keep_and_capture_stay_single_lane():
    net = make_net()
    eng = net.engine
    x = inputs(2, 0, 330)
    ref = forward(net, x, 1).clone()
    eng.forward_lanes = 2
    g, bufs = eng.run_forward(x, pad=2, keep=True)
    kept = [p for k, p in bufs['_plans'].items() if k[0] == 'fwd']
    assert kept and not any(p.side for p in kept)
    assert eng._lane_layout(2, 16, 20, x.device, True) is None and eng._lane_layout(2, 16, 20, x.device, 'masks') is None
    # under a graph capture: one list on the capturing stream (warm-up off the capture, as esr_hip.graph.GraphedForward does)
    static_x = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        forward(net, static_x, 1)
        forward(net, static_x, 2)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    eng.forward_lanes = 2
    with torch.no_grad(), torch.cuda.graph(graph):
        assert eng._lane_layout(2, 16, 20, x.device, False) is None
        static_y = net(static_x, pad=2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, ref)


def _zero_cmd(cmd, buf, n16):
    from esr_hip import _lib
    cmd.op = _lib.OP_ZERO
    cmd.u.zero.p, cmd.u.zero.n16 = buf.data_ptr(), n16


def test_esr_run_lanes_entry_point():
    from esr_hip import _lib
    from esr_hip import act as A
    lib = _lib.lib
    dev = torch.device('cuda')
    src = seeded_uniform((1, 3, 6, 10), 340).cuda()

    def fresh():
        return (torch.ones(64, dtype=torch.int32, device=dev), torch.ones(64, dtype=torch.int32, device=dev), A.ActBuf(1, 1, 6, 10, dev, True),
                torch.ones(64, dtype=torch.int32, device=dev))

    def lists(a, b, act, c):
        l0, l1 = (_lib.Cmd * 3)(), (_lib.Cmd * 1)()
        _zero_cmd(l0[0], a, 4)
        _zero_cmd(l0[1], b, 8)
        l0[2].op = _lib.OP_PACK_NCHW
        l0[2].u.pack_nchw = _lib.CmdPackNchw(src.data_ptr(), 0, 1, 3, 6, 10, 0, 3, 0, 1, act.view())
        _zero_cmd(l1[0], c, 12)
        return l0, l1

    def state(a, b, act, c):
        return [t.clone() for t in (a, b, act.hi, act.lo, c)]

    def lanes_call(ls, stream=None):
        ptrs = (C.POINTER(_lib.Cmd) * len(ls))(*[C.cast(l, C.POINTER(_lib.Cmd)) if l is not None else None for l in ls])
        ns = (C.c_int * len(ls))(*[len(l) if l is not None else 2 for l in ls])
        lane, idx = C.c_int(-7), C.c_int(-7)
        return lib.esr_run_lanes(ptrs, ns, len(ls), C.byref(lane), C.byref(idx), stream), lane.value, idx.value

    # the single-stream result
    one = fresh()
    l0, l1 = lists(*one)
    failed = C.c_int(-7)
    assert lib.esr_run(l0, 3, C.byref(failed), None) == 0 and lib.esr_run(l1, 1, C.byref(failed), None) == 0
    torch.cuda.synchronize()
    want = state(*one)
    assert int(want[0][:16].abs().sum()) == 0 and int(want[0][16:].sum()) == 48 and int(want[4][:48].abs().sum()) == 0

    # two lanes of unequal length; the null stream's order covers them: the clone below is enqueued behind the join
    two = fresh()
    assert lanes_call(lists(*two)) == (0, -1, -1)
    got = state(*two)
    assert all(torch.equal(w, g) for w, g in zip(want, got))

    # lanes == 1 is esr_run
    solo = fresh()
    l0, l1 = lists(*solo)
    assert lanes_call([l0]) == (0, -1, -1) and lanes_call([l1]) == (0, -1, -1)
    assert all(torch.equal(w, g) for w, g in zip(want, state(*solo)))

    # argument errors
    l0, l1 = lists(*fresh())
    assert lib.esr_run_lanes(None, None, 0, None, None, None) == _lib.ESR_E_ARG
    ptrs = (C.POINTER(_lib.Cmd) * 5)(*[C.cast(l0, C.POINTER(_lib.Cmd))] * 5)
    ns = (C.c_int * 5)(1, 1, 1, 1, 1)
    assert lib.esr_run_lanes(ptrs, ns, 0, None, None, None) == _lib.ESR_E_ARG
    assert lib.esr_run_lanes(ptrs, ns, 5, None, None, None) == _lib.ESR_E_ARG
    assert lanes_call([l0, None])[0] == _lib.ESR_E_ARG                 # a null list with n > 0

    # a command the entry point rejects on the host (nothing launched for it) in lane 1: reported with its lane and index, and the join still
    # orders the caller's stream behind what was issued
    bad = fresh()
    l0, _ = lists(*bad)
    lb = (_lib.Cmd * 2)()
    _zero_cmd(lb[0], bad[3], 12)
    lb[1].op = 99
    assert lanes_call([l0, lb]) == (_lib.ESR_E_ARG, 1, 1)
    after = state(*bad)
    assert int(after[0][:16].abs().sum()) == 0 and int(after[4][:48].abs().sum()) == 0          # commands 0 of both lanes ran
    # and a following valid call works
    again = fresh()
    assert lanes_call(lists(*again)) == (0, -1, -1)
    assert all(torch.equal(w, g) for w, g in zip(want, state(*again)))
