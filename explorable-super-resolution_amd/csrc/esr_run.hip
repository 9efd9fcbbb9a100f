// Launch lists: a whole forward / backward pass of the generator replayed with ONE C-ABI call (esr_run, include/esr_hip.h).
// Host code only: every command dispatches to the entry point of the same name; what this file removes is the per-launch trip through
// the caller's FFI (ctypes: ~19 us per call, ~1,100 calls per training step).
#include "esr_common.h"
#include <mutex>

// one command on `stream`: the entry point of the same name
static int run_cmd(const esr_cmd& c, esr_stream_t stream) {
    int rc;
    switch (c.op) {
        case ESR_OP_CONV3X3: rc = esr_conv3x3(&c.u.conv, stream); break;
        case ESR_OP_PACK_NCHW: {
            const esr_cmd_pack_nchw& a = c.u.pack_nchw;
            rc = esr_pack_nchw(a.src, a.src_batch_stride, a.B, a.C, a.h, a.w, a.c0, a.nc, a.pad, a.down, &a.dst, stream);
        } break;
        case ESR_OP_UNPACK_GRAD_NCHW: {
            const esr_cmd_unpack_grad_nchw& a = c.u.unpack_grad_nchw;
            rc = esr_unpack_grad_nchw(&a.G, a.dst, a.dst_batch_stride, a.B, a.C, a.h, a.w, a.c0, a.nc, a.pad, a.down, a.accumulate, stream);
        } break;
        case ESR_OP_ACT_COMBINE: {
            const esr_cmd_act_combine& a = c.u.act_combine;
            rc = esr_act_combine(a.A.hi ? &a.A : nullptr, a.alpha, a.Bv.hi ? &a.Bv : nullptr, a.beta, a.s, a.mask.hi ? &a.mask : nullptr, a.mask_slope,
                                 &a.out, a.B, stream);
        } break;
        case ESR_OP_PIXEL_UNSHUFFLE: rc = esr_pixel_unshuffle(&c.u.pixel_unshuffle.src, c.u.pixel_unshuffle.r, &c.u.pixel_unshuffle.dst, c.u.pixel_unshuffle.B, stream); break;
        case ESR_OP_GRAD_ABSMAX: rc = esr_grad_absmax(&c.u.grad_absmax.v, c.u.grad_absmax.B, c.u.grad_absmax.slot, stream); break;
        case ESR_OP_GRAD_SCALE: {
            const esr_cmd_grad_scale& a = c.u.grad_scale;
            rc = esr_grad_scale(&a.src, &a.dst, a.B, a.slot, a.exp, a.scale_in, a.scale_den, a.scale_out, stream);
        } break;
        case ESR_OP_WGRAD_BATCH_RUN: rc = esr_conv3x3_wgrad_batch_run(c.u.wgrad_batch_run.workspace, &c.u.wgrad_batch_run.plan, stream); break;
        case ESR_OP_PACK_BATCH_RUN: rc = esr_pack_batch_run(c.u.pack_batch_run.workspace, c.u.pack_batch_run.n, c.u.pack_batch_run.nblocks, stream); break;
        case ESR_OP_ZERO: rc = esr_zero(c.u.zero.p, c.u.zero.n16, stream); break;
        case ESR_OP_UNPACK_NCHW: rc = esr_unpack_nchw(&c.u.unpack_nchw.src, c.u.unpack_nchw.B, c.u.unpack_nchw.nc, c.u.unpack_nchw.dst, stream); break;
        case ESR_OP_WGRAD: rc = esr_conv3x3_wgrad(&c.u.wgrad, stream); break;
        case ESR_OP_BN_REDUCE: rc = esr_bn_reduce(&c.u.bn.d, c.u.bn.mode, c.u.bn.sums, stream); break;
        case ESR_OP_BN_APPLY: rc = esr_bn_apply(&c.u.bn.d, c.u.bn.mode, stream); break;
        case ESR_OP_BN_FINALIZE: {
            const esr_cmd_bn_finalize& a = c.u.bn_finalize;
            rc = esr_bn_finalize(a.sums, a.groups, a.C, a.n_per_group, a.eps, a.momentum, a.gamma, a.beta, a.mean, a.rstd, a.scale, a.shift, a.running_mean,
                                 a.running_var, stream);
        } break;
        case ESR_OP_BN_PARAM_GRADS: {
            const esr_cmd_bn_param_grads& a = c.u.bn_param_grads;
            rc = esr_bn_param_grads(a.sums2, a.sums3, a.rstd, a.groups, a.C, a.n_per_group, a.dgamma, a.dbeta, a.g_gamma, stream);
        } break;
        case ESR_OP_BN_FINALIZE_APPLY: rc = esr_bn_finalize_apply(&c.u.bn_finalize_apply.d, &c.u.bn_finalize_apply.f, stream); break;
        default: rc = ESR_E_ARG;
    }
    return rc;
}

extern "C" int esr_run(const esr_cmd* cmds, int n, int* failed, esr_stream_t stream) {
    if (failed) *failed = -1;
    if (n < 0 || (n > 0 && !cmds)) return ESR_E_ARG;
    for (int i = 0; i < n; ++i) {
        const int rc = run_cmd(cmds[i], stream);
        if (rc != ESR_OK) {
            if (failed) *failed = i;
            return rc;
        }
    }
    return ESR_OK;
}

// ---- esr_run_lanes: independent launch lists side by side (include/esr_hip.h) ----
// Lane 0 runs on the caller's stream, lanes 1.. on side streams owned by the library: created once per device at first use, non-blocking,
// never destroyed, at most ESR_MAX_LANES - 1 of them, so that a process whose work is on one stream stays within HIP's default four
// hardware queues.  Fork and join are events with timing disabled, created with the streams.
// Why interleaved, and why in here (profiles/r08_lanes_ab.log): the earlier two-stream experiment issued one lane's whole forward per call
// from Python on pool streams and came out bimodal, 67.4 or 75.9 ms for the same forward.  The kernel trace of a slow run shows what the slow
// mode is: the lanes do not overlap.  One queue runs its lane's launches back to back while the other has nothing to run (one conv in
// flight for 196 ms of a 218 ms window, two for 21 ms; in a fast run two for 198.4 of 199.0 ms), and a sub-batch alone on the device runs
// slower than the whole batch.  Lane-by-lane feeding overlaps only as long as the host stays a whole lane (351 launches) ahead of the GPU;
// whenever it does not, the lanes take turns.  Fed command by command both queues always hold work of the same depth, whatever the host's
// lead is, and the streams are made here once so that their placement on the hardware queues does not depend on what else took pool streams.
namespace {
struct LaneSet {
    hipStream_t side[ESR_MAX_LANES - 1];
    hipEvent_t fork, join[ESR_MAX_LANES - 1];
    int nside;          // side streams (and join events) created so far
    bool have_fork;
};
LaneSet g_lanes[64];                 // per device
std::mutex g_lanes_mutex;            // one esr_run_lanes at a time: the side streams and events are shared by every caller of a device

// the first `want` side streams of device `dev`, created on demand
bool lane_set(int dev, int want, LaneSet*& out) {
    LaneSet& s = g_lanes[dev & 63];
    if (!s.have_fork) {
        if (hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) != hipSuccess) return false;
        s.have_fork = true;
    }
    while (s.nside < want) {
        hipStream_t st;
        hipEvent_t ev;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(st);
            return false;
        }
        s.side[s.nside] = st;
        s.join[s.nside] = ev;
        ++s.nside;
    }
    out = &s;
    return true;
}
}  // namespace

extern "C" int esr_run_lanes(const esr_cmd* const* cmds, const int* n, int lanes, int* failed_lane, int* failed, esr_stream_t main) {
    if (failed_lane) *failed_lane = -1;
    if (failed) *failed = -1;
    if (lanes < 1 || lanes > ESR_MAX_LANES || !cmds || !n) return ESR_E_ARG;
    int longest = 0;
    for (int l = 0; l < lanes; ++l) {
        if (n[l] < 0 || (n[l] > 0 && !cmds[l])) return ESR_E_ARG;
        longest = n[l] > longest ? n[l] : longest;
    }
    if (lanes == 1) {
        const int rc = esr_run(cmds[0], n[0], failed, main);
        if (rc != ESR_OK && failed_lane) *failed_lane = 0;
        return rc;
    }
    // a capture would turn the fork into parallel graph branches: not something this library replays
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    ESR_CLEAR_ERR();
    if (hipStreamIsCapturing((hipStream_t)main, &cap) != hipSuccess) {
        ESR_CLEAR_ERR();
        return ESR_E_UNSUPPORTED;
    }
    if (cap != hipStreamCaptureStatusNone) return ESR_E_UNSUPPORTED;

    std::lock_guard<std::mutex> lock(g_lanes_mutex);
    int dev = 0;
    LaneSet* s = nullptr;
    if (hipGetDevice(&dev) != hipSuccess || !lane_set(dev, lanes - 1, s)) return ESR_E_LAUNCH;
    esr_stream_t on[ESR_MAX_LANES];
    on[0] = main;
    for (int l = 1; l < lanes; ++l) on[l] = (esr_stream_t)s->side[l - 1];

    // fork: the side lanes start behind everything the caller's stream holds so far (empty lanes take no part)
    bool forked[ESR_MAX_LANES] = {};
    if (hipEventRecord(s->fork, (hipStream_t)main) != hipSuccess) return ESR_E_LAUNCH;
    int rc = ESR_OK;
    for (int l = 1; l < lanes && rc == ESR_OK; ++l) {
        if (!n[l]) continue;
        if (hipStreamWaitEvent(s->side[l - 1], s->fork, 0) != hipSuccess) rc = ESR_E_LAUNCH;
        else forked[l] = true;
    }
    // command i of every lane, then command i + 1 of every lane: the queues are fed evenly, lane l one launch behind lane l - 1
    for (int i = 0; i < longest && rc == ESR_OK; ++i) {
        for (int l = 0; l < lanes; ++l) {
            if (i >= n[l]) continue;
            rc = run_cmd(cmds[l][i], on[l]);
            if (rc != ESR_OK) {
                if (failed_lane) *failed_lane = l;
                if (failed) *failed = i;
                break;
            }
        }
    }
    // join, also behind a failure: the caller's stream never runs ahead of a side lane
    for (int l = 1; l < lanes; ++l) {
        if (!forked[l]) continue;
        if (hipEventRecord(s->join[l - 1], s->side[l - 1]) != hipSuccess || hipStreamWaitEvent((hipStream_t)main, s->join[l - 1], 0) != hipSuccess) {
            if (rc == ESR_OK) rc = ESR_E_LAUNCH;
        }
    }
    return rc;
}

extern "C" int64_t esr_cmd_bytes(void) { return (int64_t)sizeof(esr_cmd); }
