#!/usr/bin/env python
"""What the train-mode segment sampler costs, at the headline shape (resnet101 features, fc_dim 512, 128 + 74 videos x 5 segments, TA3N, bf16
twins) with a fresh device-gathered batch every step - bench.py's fresh-batch protocol: 640 synthetic videos of 16 - 47 frames packed in
bf16, random video ids per step, train_steps(feeds=...) so that the batch is assembled by the launch that opens the step:
 (a) ms per step over `--steps` steps after `--warmup`, sampler "test" and sampler "train" alternating in this one process, `--repeats`
     times each, wall clock around flush + synchronize; both ranges are printed;
 (b) FeatureStore.gather on the bf16 store at 202 x 5 x 2048: the torch branch it had (frame counts to the host, a Python loop over
     ta3n_segment_indices, rows widened by torch - kept here as old_bf16_gather) beside the kernel (ta3n_gather_segments_bf16), us per call.
One JSON line per measurement.

    python tools/time_sampler.py [--steps 200] [--warmup 20] [--repeats 3]
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd import _lib  # noqa: E402
from ta3n_amd.engine import TrainEngine  # noqa: E402
from ta3n_amd.feature_store import FeatureStore  # noqa: E402
from ta3n_amd.synthetic import synth_state  # noqa: E402

SHAPE = dict(Bs=128, Bt=74, T=5, D=2048, F=512, C=12)
HYPER = ([0.75, 0.75, 0.5], 0.003, 1e-4)


def synthetic_store(seed: int = 4321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nf = torch.randint(16, 48, (640,), generator=g)
    rows = torch.randn(int(nf.sum()), SHAPE["D"], device="cuda").abs_().to(torch.bfloat16).view(torch.int16)
    return FeatureStore.from_tensors(rows, nf.cuda(), torch.randint(0, SHAPE["C"], (640,), generator=g).cuda()), g


def old_bf16_gather(store, ids, T):
    """FeatureStore.gather on a bf16 store before ta3n_gather_segments_bf16: one device-to-host copy, a host loop, torch indexing."""
    seg = torch.tensor([[s - 1 for s in _lib.segment_indices(int(nf), T)] for nf in store.num_frames[ids.long()].tolist()],
                       device=store.device, dtype=torch.long)
    rows = store.first_row[ids.long()].unsqueeze(1) + seg
    return store.store[rows.reshape(-1)].view(torch.bfloat16).to(torch.float32).view(ids.numel(), T, store.feature_dim), store.labels[ids.long()]


def time_steps(steps: int, warmup: int, repeats: int):
    s = SHAPE
    eng = TrainEngine(s["Bs"], s["Bt"], s["T"], s["D"], s["F"], s["C"], dropout_i=0.5, dropout_v=0.5, clip=20.0, bf16=True, bf16_store=True)
    eng.load_state(synth_state({n: sh for n, _, sh, _ in eng.plan.params}, seed=7))
    assert eng.can_batch_steps()
    store, g = synthetic_store()
    views = {"test": (store, store), "train": (store.sampled("train", 5), store.sampled("train", 6))}
    out = {k: [] for k in views}
    gc.disable()
    for _ in range(repeats):
        for name, (src, tgt) in views.items():
            ids = [torch.randint(0, 640, (warmup + steps, n), generator=g, dtype=torch.int32).cuda() for n in (s["Bs"], s["Bt"])]
            eng.train_steps([HYPER] * warmup, feeds=((src, ids[0][:warmup]), (tgt, ids[1][:warmup])))
            eng.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.train_steps([HYPER] * steps, feeds=((src, ids[0][warmup:]), (tgt, ids[1][warmup:])))
            eng.flush()
            torch.cuda.synchronize()
            out[name].append(1e3 * (time.perf_counter() - t0) / steps)
    gc.enable()
    print(json.dumps(dict(measurement="fresh_batch_state", parameters_finite=bool(torch.isfinite(eng.P).all()), steps_run=eng.step_count)), flush=True)
    for name, ms in out.items():
        print(json.dumps(dict(measurement="fresh_batch_step", sampler=name, ms_per_step_min=round(min(ms), 4), ms_per_step_max=round(max(ms), 4),
                              ms_per_step=[round(v, 4) for v in ms], steps=steps, warmup=warmup, repeats=repeats)), flush=True)
    print(json.dumps(dict(measurement="fresh_batch_step_train_over_test", ratio_of_minima=round(min(out["train"]) / min(out["test"]), 4))), flush=True)


def time_gather(repeats: int, calls: int = 50):
    store, g = synthetic_store()
    T = SHAPE["T"]
    ids = torch.randint(0, 640, (SHAPE["Bs"] + SHAPE["Bt"],), generator=g, dtype=torch.int32).cuda()
    old_x, old_y = old_bf16_gather(store, ids, T)
    new_x, new_y = store.gather(ids, T)
    torch.cuda.synchronize()
    assert torch.equal(old_x.view(torch.int32), new_x.view(torch.int32)) and torch.equal(old_y, new_y)
    out = torch.empty_like(new_x)
    lab = torch.empty_like(new_y)
    for name, fn in (("torch_branch", lambda: old_bf16_gather(store, ids, T)), ("kernel", lambda: store.gather(ids, T, out=out, labels_out=lab))):
        us = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0) / calls)
        print(json.dumps(dict(measurement="bf16_store_gather", path=name, us_per_call_min=round(min(us), 1), us_per_call_max=round(max(us), 1),
                              videos=int(ids.numel()), segments=T, feature_dim=SHAPE["D"], calls=calls, repeats=repeats)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    time_steps(a.steps, a.warmup, a.repeats)
    time_gather(a.repeats)


if __name__ == "__main__":
    main()
