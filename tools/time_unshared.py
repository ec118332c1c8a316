#!/usr/bin/env python
"""Per-step time of --share_params N (TrainEngine(share_params="N"): the plain unfused launch lists with five GEMMs cut at the domain
boundary) beside the plain unfused lists (TrainEngine(fused=False)) at the headline shape (resnet101 features, fc_dim 512, 128 + 74
videos x 5 segments), bf16 MFMA operands read from bf16 twins and fp32: one resident batch, the two engines ALTERNATING in the same
run, HIP events around `steps` train_step calls, best of 3 repeats per engine, and the per-launch times of both (ta3n_time_phases)
so that a difference can be named.  One JSON line per engine and arithmetic, then their ratio and the plain engine's own spread.

    python tools/time_unshared.py [--steps 100] [--repeats 3] [--only plain|unshared] [--arithmetic bf16|fp32]

--only / --arithmetic run one engine in one arithmetic (no ratio): what a kernel trace of one side needs
(rocprofv3 --kernel-trace --stats -- python tools/time_unshared.py --only unshared --arithmetic bf16).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd.engine import TrainEngine  # noqa: E402
from ta3n_amd.synthetic import synth_batch, synth_state  # noqa: E402

Bs, Bt, T, D, F, C = 128, 74, 5, 2048, 512, 12


def make_engine(share_params: str, bf16: bool) -> TrainEngine:
    eng = TrainEngine(Bs, Bt, T, D, F, C, dropout_i=0.5, dropout_v=0.5, clip=20.0, bf16=bf16, bf16_store=bf16, fused=False,
                      share_params=share_params)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7, scale="init"))
    xs, xt, ys, _ = synth_batch(C, T, D, Bs, Bt, seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    for _ in range(30):                          # warm-up (code objects, caches)
        eng.train_step([0.75, 0.75, 0.5], 0.003, 0.03)
    torch.cuda.synchronize()
    return eng


def time_once(eng: TrainEngine, steps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        eng.train_step([0.75, 0.75, 0.5], 0.003, 0.03)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("plain", "unshared"), default=None)
    ap.add_argument("--arithmetic", choices=("bf16", "fp32"), default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sides = {"plain unfused lists": "Y", "share_params N": "N"}
    if a.only:
        sides = {k: v for k, v in sides.items() if (v == "N") == (a.only == "unshared")}
    for bf16 in (True, False):
        if a.arithmetic and (a.arithmetic == "bf16") != bf16:
            continue
        engines = {k: make_engine(v, bf16) for k, v in sides.items()}
        runs = {k: [] for k in engines}
        for _ in range(a.repeats):               # alternating: both engines see the same drift of the machine
            for k, eng in engines.items():
                runs[k].append(time_once(eng, a.steps))
        arith = "bf16 twins" if bf16 else "fp32"
        for k, eng in engines.items():
            assert torch.isfinite(eng.P).all()
            ph = eng.time_phases(reps=50)
            print(json.dumps(dict(engine=k, arithmetic=arith, ms_per_step=round(min(runs[k]), 4), runs=[round(v, 4) for v in runs[k]],
                                  steps=a.steps, launches_us=[[kind, ntasks, round(1e3 * ms, 1)] for kind, _, ntasks, ms in ph],
                                  describe=eng.describe())), flush=True)
        if len(engines) < 2:
            continue
        p, n = runs["plain unfused lists"], runs["share_params N"]
        print(json.dumps(dict(arithmetic=arith, ratio=round(min(n) / min(p), 4), plain_spread=round((max(p) - min(p)) / min(p), 4),
                              unshared_spread=round((max(n) - min(n)) / min(n), 4))), flush=True)


if __name__ == "__main__":
    main()
