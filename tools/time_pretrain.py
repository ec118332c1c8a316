#!/usr/bin/env python
"""Per-iteration time of --pretrain_source at the headline shape (resnet101 features, fc_dim 512, 128 + 74 videos x 5 segments, bf16 MFMA
operands read from bf16 twins, the TA3N options of the headline command), in one run:
  - the engine with the source-only pass (TrainEngine(pretrain_source=True): pass + ta3n_sgd_live + step + update per train_step call),
  - the plain step driven the same way (one train_step call per step) and as one ta3n_train_steps call (what bench.py times),
  - the module path with the pass (VideoModel + torch loss assembly + clip_grad_norm_ + SGD.step twice per iteration, ta3n_amd.accel on),
  - the launches of one pass and one step by themselves (HIP events around each, best of `repeats`), so that what the iteration costs over
    twice the plain step can be named: the two parameter-twin refreshes and the pass's own launches.
One resident batch, `steps` iterations timed with HIP events (the module path: wall clock), best of `repeats`.  One JSON line per row.

    python tools/time_pretrain.py [--steps 100] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd import _lib, accel  # noqa: E402
from ta3n_amd.engine import TrainEngine  # noqa: E402
from ta3n_amd.loss import attentive_entropy  # noqa: E402
from ta3n_amd.models import VideoModel  # noqa: E402
from ta3n_amd.synthetic import synth_batch, synth_state  # noqa: E402

Bs, Bt, T, D, FC, NC = 128, 74, 5, 2048, 512, 12
BETA, GAMMA, LR = [0.75, 0.75, 0.5], 0.003, 1e-4


def best_of(fn, steps, repeats, events=True):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / steps if events else 1e3 * (time.perf_counter() - t0) / steps)
    return best


def engine(pretrain):
    eng = TrainEngine(Bs, Bt, T, D, FC, NC, bf16=True, bf16_store=True, pretrain_source=pretrain)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    xs, xt, ys, yt = synth_batch(NC, T, D, Bs, Bt, seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    return eng


def engine_rows(steps, repeats):
    rows = []
    plain = engine(False)
    step = lambda e: (lambda: e.train_step(BETA, GAMMA, LR))      # noqa: E731
    for _ in range(10):
        step(plain)()
    rows.append(dict(row="plain step, one train_step call per step", ms_per_iteration=round(best_of(step(plain), steps, repeats), 4)))
    sched = [(BETA, GAMMA, LR)] * steps
    plain.train_steps(sched[:10])
    rows.append(dict(row="plain step, one ta3n_train_steps call", ms_per_iteration=round(best_of(lambda: plain.train_steps(sched), 1, repeats) / steps, 4)))
    plain.flush()
    pre = engine(True)
    for _ in range(10):
        step(pre)()
    rows.append(dict(row="pass + step (pretrain_source), one train_step call per iteration",
                     ms_per_iteration=round(best_of(step(pre), steps, repeats), 4), describe=pre.describe()))
    # the pieces of one iteration by themselves
    L, st = pre._L, pre._stream
    X, P, G, M = pre.X.data_ptr(), pre.P.data_ptr(), pre.G.data_ptr(), pre.M.data_ptr()
    hp, wp, hs, ws = pre.plan_pre.handle, pre.ws_pre.data_ptr(), pre.plan.handle, pre.ws.data_ptr()
    pieces = {
        "pass: ta3n_refresh_bf16 of the parameters (its workspace)": lambda: L.ta3n_refresh_bf16(hp, None, P, wp, st()),
        "pass: ta3n_train_step of the source-only plan": lambda: L.ta3n_train_step(hp, X, P, G, wp, st()),
        "pass: ta3n_sgd_live": lambda: L.ta3n_sgd_live(hp, P, G, M, wp, 1, C.c_float(LR), C.c_float(0.9), C.c_float(1e-4), C.c_float(20.0), st()),
        "step: ta3n_refresh_bf16 of the parameters (its workspace)": lambda: L.ta3n_refresh_bf16(hs, None, P, ws, st()),
        "step: ta3n_train_step": lambda: L.ta3n_train_step(hs, X, P, G, ws, st()),
        "step: ta3n_sgd_step_fused": lambda: L.ta3n_sgd_step_fused(hs, P, G, M, ws, st()),
    }
    for name, fn in pieces.items():
        fn()
        rows.append(dict(row=name, ms=round(best_of(fn, steps, repeats), 4)))
    torch.cuda.synchronize()
    assert torch.isfinite(pre.P).all() and torch.isfinite(plain.P).all()
    return rows


def module_row(steps, repeats):
    xs, xt, ys, yt = synth_batch(NC, T, D, Bs, Bt, seed=1234)
    xs, xt, ys = xs.cuda(), xt.cuda(), ys.cuda()
    m = VideoModel(NC, "video", "trn-m", "RGB", train_segments=T, val_segments=T, base_model="resnet101", fc_dim=FC, verbose=False).cuda()
    m.train()
    opt = torch.optim.SGD(m.parameters(), LR, momentum=0.9, weight_decay=1e-4, nesterov=True)
    accel.install()

    def update(loss):
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 20)
        opt.step()

    def iteration():
        o = m(xs, xt, BETA, 0, True, False)
        update(F.cross_entropy(o[1], ys))
        o = m(xs, xt, BETA, 0, True, False)
        loss = F.cross_entropy(o[1], ys)
        pd_all = []
        for l in range(3):
            ps, pt = o[3][l].reshape(-1, 2), o[8][l].reshape(-1, 2)
            lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long().cuda()
            pd_all.append(torch.cat((ps, pt)))
            loss = loss + F.cross_entropy(pd_all[-1], lab)
        update(loss + GAMMA * attentive_entropy(torch.cat((o[1], o[6])), pd_all[1]))
    for _ in range(10):
        iteration()
    ms = best_of(iteration, steps, repeats, events=False)
    accel.uninstall()
    return dict(row="module path, pass + step (fp32, VideoModel + torch loss assembly, ta3n_amd.accel)", ms_per_iteration=round(ms, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps(dict(shape=dict(Bs=Bs, Bt=Bt, T=T, D=D, fc_dim=FC, C=NC), arithmetic="bf16 twins", steps=a.steps, repeats=a.repeats,
                          library=_lib.lib().ta3n_version().decode())), flush=True)
    for row in engine_rows(a.steps, a.repeats) + [module_row(a.steps, a.repeats)]:
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
