#!/usr/bin/env python
"""What the temporal-convolution aggregator (--frame_aggregation temconv) costs at the headline shape: resnet101 features, fc_dim 512,
128 + 74 videos x 5 segments, 12 classes, fp32, place_adv N Y Y.  In one run:
  - ms per ta3n_train_step of the TA3N_AGG_TEMCONV plan and of the general TemPooling plan with the same flags (the yardstick: the
    difference is the filter, one more pass over F1 on the way back, and the launch that sums the parameter gradients),
  - the aggregator's own launches of either plan (temconv: forward, backward, parameter-gradient sum; TemPooling: mean, spread), each
    timed by itself with HIP events (ta3n_time_phases).
One resident batch, `steps` iterations between two HIP events, best of `repeats`.  One JSON line per row.

    python tools/time_temconv.py [--steps 200] [--repeats 3]
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
from ta3n_amd.synthetic import synth_batch, synth_state, synth_temconv_state  # noqa: E402

Bs, Bt, T, D, FC, NC = 128, 74, 5, 2048, 512, 12
FLAGS = _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
KIND_NAMES = {8: "pool_avg_fwd", 9: "pool_avg_bwd", 20: "temconv_fwd", 21: "temconv_bwd", 22: "temconv_wgrad"}      # PhaseKind (ta3n_types.h)


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
        state = synth_state({k: s for k, s in shapes.items() if not k.startswith("tcl_")}, seed=7)
        state.update(synth_temconv_state(shapes, seed=7))
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


def row(name, step, steps, repeats, base=None):
    for _ in range(10):
        step.train_step()
    ms = best_of(step.train_step, steps, repeats)
    fused = [(k, t) for k, g, t in step.phases(20) if g == 4]
    torch.cuda.synchronize()
    assert torch.isfinite(step.G).all()
    out = dict(row=name, ms=round(ms, 4), launches=len(fused), launches_sum_ms=round(sum(t for _, t in fused), 4),
               aggregator_launches_ms={KIND_NAMES[k]: round(t, 4) for k, t in fused if k in KIND_NAMES})
    if base is not None:
        out["over_tempooling_ms"] = round(ms - base, 4)
    print(json.dumps(out), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps(dict(shape=dict(Bs=Bs, Bt=Bt, T=T, D=D, fc_dim=FC, C=NC), arithmetic="fp32", place_adv="N Y Y", steps=a.steps,
                          repeats=a.repeats, library=_lib.lib().ta3n_version().decode())), flush=True)
    base = row("general TemPooling plan, ta3n_train_step", Step(aggregation=_lib.AGG_AVGPOOL), a.steps, a.repeats)
    row("temconv plan, ta3n_train_step", Step(aggregation=_lib.AGG_TEMCONV), a.steps, a.repeats, base)


if __name__ == "__main__":
    main()
