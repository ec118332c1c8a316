"""ta3n_time_phases on the MI355X: the timing entry point starts every launch kind through the dispatch that ta3n_forward / ta3n_loss /
ta3n_backward / ta3n_train_step use (ta3n_api.hip: launch_phase), one plan per family of kinds at the smallest shapes the families' own
tests use.  Through the C ABI on raw buffers: it returns the plan's number of phases, reports the kinds and groups of the plan's
description in order, every time is finite and not negative, and the device is sound afterwards."""
import ctypes as C
import math

import pytest
import torch

from ta3n_amd import _lib, parallel
from ta3n_amd.synthetic import synth_batch, synth_rnn_state, synth_state, synth_temconv_state

pytestmark = pytest.mark.gpu

Bs, Bt, D, FC, CN = 6, 4, 512, 64, 12
ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
TRN = ADV | _lib.FLAG_ATTN_ENTROPY
# family -> (T, flags, Plan keywords)
PLANS = {
    "trn_fused": (5, TRN | _lib.FLAG_TRANS_ATTN, {}),
    "trn_bn_shared": (5, TRN | _lib.FLAG_TRANS_ATTN | _lib.FLAG_BN_SHARED, {}),
    "trn_frame_attn": (5, TRN | _lib.FLAG_TRANS_ATTN | _lib.FLAG_FRAME_ATTN, {}),
    "trn_general_attn": (5, TRN | _lib.FLAG_GENERAL_ATTN, {}),
    "avgpool_source_only": (5, 0, dict(aggregation=_lib.AGG_AVGPOOL)),
    "avgpool_da": (5, ADV, dict(aggregation=_lib.AGG_AVGPOOL)),
    "rnn_lstm": (5, ADV, dict(aggregation=_lib.AGG_RNN, rnn_cell=0, n_ts=2)),
    "rnn_gru": (5, ADV, dict(aggregation=_lib.AGG_RNN, rnn_cell=1, n_ts=2)),
    "temconv": (3, ADV, dict(aggregation=_lib.AGG_TEMCONV)),
}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("family", list(PLANS))
def test_time_phases_runs_every_launch_of_the_plan(family):
    T, flags, kw = PLANS[family]
    plan = _lib.Plan(Bs, Bt, T, D, FC, CN, flags, **kw)
    if family == "trn_fused":
        assert plan.has_fused_step
    L = _lib.lib()
    P, G, M = (torch.zeros(plan.param_floats, device="cuda") for _ in range(3))
    ws = torch.zeros(plan.ws_floats, device="cuda")
    _lib.check(L.ta3n_init_workspace(plan.handle, ws.data_ptr(), _stream()), "ta3n_init_workspace")
    shapes = {n: s for n, _, s, _ in plan.params}
    state = synth_state({k: s for k, s in shapes.items() if not k.startswith(("tcl_", "conv_fusion."))})
    state.update(synth_rnn_state(shapes, seed=7))
    state.update(synth_temconv_state(shapes, seed=7))
    for name, off, shape, _ in plan.params:
        if name in state:
            P[off:off + state[name].numel()] = state[name].reshape(-1).float().cuda()
    xs, xt, ys, yt = synth_batch(CN, T, D, Bs, Bt)
    X = torch.cat((xs, xt), 0).reshape(-1, D).float().cuda().contiguous()
    off, n = plan.region("labels")
    ws[off:off + n].view(torch.int32)[:Bs + Bt] = torch.cat((ys, yt)).to(torch.int32).cuda()
    h = _lib.Hyper()
    h.beta[0], h.beta[1], h.beta[2] = 0.75, 0.75, 0.5
    h.gamma, h.lr, h.momentum, h.weight_decay, h.clip = 0.003, 0.01, 0.9, 1e-4, 20.0
    h.p_drop_i = h.p_drop_v = 0.0
    h.seed_i, h.seed_v = 1, 2
    for k, v in parallel.loss_normalisers(Bs, Bt, T, flags).items():
        setattr(h, k, v)
    h.valid_source, h.valid_target, h.train = Bs, Bt, 1
    _lib.check(L.ta3n_set_hyper(plan.handle, ws.data_ptr(), C.byref(h), _stream()), "ta3n_set_hyper")

    want = plan.description["phases"]
    cap = len(want)
    ms = (C.c_float * cap)()
    kind = (C.c_int32 * cap)()
    group = (C.c_int32 * cap)()
    got = _lib.check(L.ta3n_time_phases(plan.handle, X.data_ptr(), P.data_ptr(), G.data_ptr(), M.data_ptr(), ws.data_ptr(), _stream(), 2,
                                        ms, kind, group, cap), "ta3n_time_phases")
    print(f"\n[time phases] {family}: {got} launches, kinds {sorted(set(kind))}, {sum(ms) * 1e3:.0f} us in all")
    assert got == len(want)
    assert list(kind) == [ph["kind"] for ph in want]
    assert list(group) == [ph["group"] for ph in want]
    assert all(math.isfinite(t) and t >= 0 for t in ms)
    torch.cuda.synchronize()
