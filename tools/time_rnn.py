#!/usr/bin/env python
"""What the recurrent aggregator (--frame_aggregation rnn) costs at the headline shape: resnet101 features, fc_dim 512, 128 + 74 videos x
5 segments, n_ts 5, 12 classes, fp32, place_adv N Y Y.  In one run:
  - ms per ta3n_train_step of the TA3N_AGG_RNN plan with an LSTM, with a GRU, and of the general TemPooling plan with the same flags
    (the difference is the recurrence),
  - the sum of the aggregator's own launches (slot pooling, Gx, n_ts x {Gh, cell}, n_ts x {cell backward, gh}, weight gradients + gXp,
    pooling backward), each timed by itself with HIP events (ta3n_time_phases),
  - torch.nn.LSTM / nn.GRU forward + backward on the same GPU at [202, 5, 512], hidden 512.
One resident batch, `steps` iterations between two HIP events, best of `repeats`.  One JSON line per row.

    python tools/time_rnn.py [--steps 200] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd import _lib  # noqa: E402
from ta3n_amd.synthetic import synth_batch, synth_rnn_state, synth_state  # noqa: E402

Bs, Bt, T, D, FC, NC, N_TS = 128, 74, 5, 2048, 512, 12, 5
FLAGS = _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
RNN_KINDS = (16, 17, 18, 19)      # PH_RNN_POOL_FWD, PH_RNN_CELL_FWD, PH_RNN_CELL_BWD, PH_RNN_POOL_BWD (ta3n_types.h)


def best_of(fn, steps, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / steps)
    return best


class Step:
    def __init__(self, **plan_kw):
        self.plan = p = _lib.Plan(Bs, Bt, T, D, FC, NC, FLAGS, **plan_kw)
        self.L = _lib.lib()
        shapes = {n: s for n, _, s, _ in p.params}
        state = synth_state(shapes, seed=7)
        state.update(synth_rnn_state(shapes, seed=7))
        self.P, self.G, self.M = (torch.zeros(p.param_floats, device="cuda") for _ in range(3))
        for name, off, shape, _ in p.params:
            self.P[off:off + state[name].numel()] = state[name].reshape(-1).cuda()
        self.ws = torch.zeros(p.ws_floats, device="cuda")
        st = self.stream()
        _lib.check(self.L.ta3n_init_workspace(p.handle, self.ws.data_ptr(), st), "ta3n_init_workspace")
        xs, xt, ys, _ = synth_batch(NC, T, D, Bs, Bt, seed=1234)
        self.X = torch.cat((xs, xt)).reshape(-1, D).cuda().contiguous()
        off, _ = p.region("labels")
        self.ws[off:off + Bs].view(torch.int32).copy_(ys.to(torch.int32))
        h = _lib.Hyper()
        h.beta[0], h.beta[1], h.beta[2] = 0.75, 0.75, 0.5
        h.lr, h.momentum, h.weight_decay, h.clip = 1e-4, 0.9, 1e-4, 20.0
        h.inv_n_cls, h.inv_n_vid, h.inv_n_frm = 1.0 / Bs, 1.0 / (Bs + Bt), 1.0 / ((Bs + Bt) * T)
        h.valid_source, h.valid_target, h.train = Bs, Bt, 1
        _lib.check(self.L.ta3n_set_hyper(p.handle, self.ws.data_ptr(), C.byref(h), st), "ta3n_set_hyper")

    @staticmethod
    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def train_step(self):
        _lib.check(self.L.ta3n_train_step(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.ws.data_ptr(), self.stream()),
                   "ta3n_train_step")

    def phases(self, reps):
        """[(kind, group, ms)] of every launch of the plan, each timed by itself."""
        cap = 512
        ms, kind, group = (C.c_float * cap)(), (C.c_int32 * cap)(), (C.c_int32 * cap)()
        n = _lib.check(self.L.ta3n_time_phases(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(),
                                              self.ws.data_ptr(), self.stream(), reps, ms, kind, group, cap), "ta3n_time_phases")
        return [(kind[i], group[i], ms[i]) for i in range(n)]


def aggregator_launches(rows):
    """The launches of ta3n_train_step (group 4) that belong to the recurrence: from the slot pooling to the last cell step, and from the
    first cell-backward step to the pooling backward, GEMM launches in between included."""
    fused = [(k, ms) for k, g, ms in rows if g == 4]
    idx = [i for i, (k, _) in enumerate(fused) if k in RNN_KINDS]
    last_fwd = max(i for i in idx if fused[i][0] == 17)
    first_bwd = min(i for i in idx if fused[i][0] == 18)
    mine = list(range(idx[0], last_fwd + 1)) + list(range(first_bwd, idx[-1] + 1))
    return sum(fused[i][1] for i in mine), len(mine), sum(ms for _, ms in fused), len(fused)


def torch_rnn(cell, steps, repeats):
    rnn = (torch.nn.LSTM if cell == "LSTM" else torch.nn.GRU)(FC, FC, 1, batch_first=True).cuda()
    x = torch.randn(Bs + Bt, N_TS, FC, device="cuda", requires_grad=True)
    gout = torch.randn(Bs + Bt, FC, device="cuda")

    def it():
        rnn.zero_grad(set_to_none=True)
        x.grad = None
        out, _ = rnn(x)
        out[:, -1, :].backward(gout)
    for _ in range(10):
        it()
    return best_of(it, steps, repeats)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps(dict(shape=dict(Bs=Bs, Bt=Bt, T=T, D=D, fc_dim=FC, C=NC, n_ts=N_TS), arithmetic="fp32", place_adv="N Y Y", steps=a.steps,
                          repeats=a.repeats, library=_lib.lib().ta3n_version().decode())), flush=True)
    avg = Step(aggregation=_lib.AGG_AVGPOOL)
    for _ in range(10):
        avg.train_step()
    base = best_of(avg.train_step, a.steps, a.repeats)
    print(json.dumps(dict(row="general TemPooling plan, ta3n_train_step", ms=round(base, 4))), flush=True)
    for cell in ("LSTM", "GRU"):
        s = Step(aggregation=_lib.AGG_RNN, rnn_cell=_lib.RNN_CELLS[cell], n_ts=N_TS)
        for _ in range(10):
            s.train_step()
        ms = best_of(s.train_step, a.steps, a.repeats)
        agg, n_agg, total, n_all = aggregator_launches(s.phases(20))
        torch.cuda.synchronize()
        assert torch.isfinite(s.G).all()
        print(json.dumps(dict(row=f"rnn plan, {cell}: ta3n_train_step", ms=round(ms, 4), over_tempooling_ms=round(ms - base, 4),
                              aggregator_launches=n_agg, aggregator_launches_sum_ms=round(agg, 4), launches=n_all,
                              launches_sum_ms=round(total, 4))), flush=True)
        print(json.dumps(dict(row=f"torch.nn.{cell} forward + backward, [202, 5, 512], hidden 512", ms=round(torch_rnn(cell, a.steps, a.repeats), 4))),
              flush=True)


if __name__ == "__main__":
    main()
