"""The library calls every step schedule of TrainEngine (ta3n_amd/engine.py) makes, in order and with their arguments, for a fixed
matrix of engine configurations: what "the host side enqueues the same work" means for a restructuring of the engine.

    python tests/golden/make_engine_call_traces.py        # writes tests/golden/engine_call_traces.json

Run it on the commit whose schedules are the REFERENCE (the parent of an engine refactor), never on the code under test: the JSON is
the evidence, tests/test_engine_call_traces_cpu.py records every trace again and compares.  Host-only: no GPU and no library is touched.

The engine is a stand-in: object.__new__(TrainEngine) with the attributes the step methods read, CPU tensors for its buffers, a plan
stub, and a fake library whose every entry records (name, arguments) and returns TA3N_OK (ta3n_has_pipelined_step: 1,
ta3n_num_phases: 8).  torch.cuda's streams and events are trivial fakes that record their edges.  An argument is recorded as
  - the buffer's name where it is the address of one of the engine's buffers ("P", "G", "M", "V", "ws", "X", "plan"),
  - "stream:<n>" / "event:<n>" for the fake streams and events, numbered in the order they were created (0: the current stream),
  - an int as it is (ranges, fused_norm, the Adam step number, n_steps),
  - a float as "f32:<repr of the value rounded to fp32>" (exact: eps = 1e-8 survives; never rounded to decimals),
  - a ta3n_hyper as ["hyper", lr, seed_i, valid_source, valid_target], an array of them entry by entry, a ta3n_feed as ["feed", ...].
"""
import contextlib
import ctypes as C
import json
import os
import sys
from unittest import mock

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

JSON_PATH = os.path.join(HERE, "engine_call_traces.json")
LIVE, N_FIRST, PARAM = 64, 24, 80      # the stub plan: live prefix, where the shared frame FC ends, all parameter floats


def _f32(x):
    import numpy as np
    return "f32:" + repr(float(np.float32(x)))


class _Stream:
    def __init__(self, rec, n):
        self.rec, self.cuda_stream = rec, 1000 + n

    def wait_event(self, ev):
        self.rec.trace.append(["stream.wait_event", [f"stream:{self.cuda_stream - 1000}", f"event:{ev.cuda_event - 2000}"]])

    def wait_stream(self, other):
        self.rec.trace.append(["stream.wait_stream", [f"stream:{self.cuda_stream - 1000}", f"stream:{other.cuda_stream - 1000}"]])


class _Event:
    def __init__(self, rec, n):
        self.rec, self.cuda_event = rec, 2000 + n

    def record(self, stream):
        self.rec.trace.append(["event.record", [f"event:{self.cuda_event - 2000}", f"stream:{stream.cuda_stream - 1000}"]])


class _Plan:
    handle, live_floats, param_floats, regions = 77, LIVE, PARAM, {}

    def region(self, name):
        return 0, 16


class Recorder:
    """The fake library (every attribute a recording function), the fake streams / events and the trace they write."""

    def __init__(self):
        self.trace, self.names, self.n_streams, self.n_events = [], {_Plan.handle: "plan"}, 1, 0
        self.main = _Stream(self, 0)

    def stream(self, *a, **k):
        self.n_streams += 1
        return _Stream(self, self.n_streams - 1)

    def event(self, *a, **k):
        self.n_events += 1
        return _Event(self, self.n_events - 1)

    def _hyper(self, h):
        return ["hyper", _f32(h.lr), int(h.seed_i), int(h.valid_source), int(h.valid_target)]

    def _address(self, v):
        if v is None:
            return None
        if v in self.names:
            return self.names[v]
        if 1000 <= v < 2000:
            return f"stream:{v - 1000}"
        if 2000 <= v < 3000:
            return f"event:{v - 2000}"
        return v

    def norm(self, args):
        from ta3n_amd import _lib
        out = []
        for i, a in enumerate(args):
            if type(a).__name__ == "CArgObject":      # C.byref(x)
                a = a._obj
            if a is None or isinstance(a, str):
                out.append(a)
            elif isinstance(a, bool):
                out.append(int(a))
            elif isinstance(a, int):
                out.append(self._address(a))
            elif isinstance(a, float):
                out.append(_f32(a))
            elif isinstance(a, C.c_void_p):
                out.append(self._address(a.value))
            elif isinstance(a, _lib.Hyper):
                out.append(self._hyper(a))
            elif isinstance(a, C.Array) and a._type_ is _lib.Hyper:
                out.append(["hypers"] + [self._hyper(h) for h in a])
            elif isinstance(a, C.POINTER(_lib.Hyper)):      # (ta3n_train_steps*: the number of entries is the argument behind it)
                out.append(["hypers"] + [self._hyper(a[k]) for k in range(int(args[i + 1]))] if a else None)
            elif isinstance(a, (_lib.Feed, C.POINTER(_lib.Feed))):
                f = a if isinstance(a, _lib.Feed) else (a.contents if a else None)
                out.append(None if f is None else ["feed", int(f.ids_per_step), int(f.bf16), self._address(f.store)])
            else:
                out.append(type(a).__name__)
        return out

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args):
            self.trace.append([name, self.norm(args)])
            return {"ta3n_has_pipelined_step": 1, "ta3n_num_phases": 8}.get(name, 0)
        return call


class _Store:
    """Feature-store stub of train_steps' feeds: the fields ta3n_feed takes, and gather_into as a trace entry."""

    def __init__(self, rec, name):
        import torch
        self.rec, self.name, self.bf16 = rec, name, False
        self.store, self.first_row, self.num_frames, self.labels = (torch.zeros(8) for _ in range(4))
        rec.names[self.store.data_ptr()] = name

    def gather_into(self, eng, ids, first, labels_out=None):
        self.rec.trace.append(["gather_into", [self.name, [int(v) for v in ids], int(first), None if labels_out is None else int(labels_out.numel())]])


def stand_in(rec, optimizer="SGD", side_update=True, selftest=False, buckets=1, sharded=False, fused=True, unfused_norm=False):
    import torch
    from ta3n_amd import _lib, engine
    e = object.__new__(engine.TrainEngine)
    e.Bs, e.Bt, e.T, e.D, e.C, e.F = 3, 2, 4, 8, 5, 8
    e.B = e.Bs + e.Bt
    e.world, e.rank, e.pg, e.device = 1, 0, None, torch.device("cpu")
    e.momentum, e.weight_decay, e.clip, e.dropout_i, e.dropout_v = 0.9, 1e-4, 20.0, 0.5, 0.3
    e.optimizer, e.betas, e.eps, e.adam_step_count, e.force_unfused_norm = optimizer, (0.9, 0.999), 1e-8, 0, bool(unfused_norm)
    e.plan, e._L, e._flags = _Plan(), rec, engine.ALL_FLAGS
    e.P, e.G, e.X, e.ws = torch.zeros(PARAM), torch.zeros(PARAM), torch.zeros(e.B * e.T, e.D), torch.zeros(256)
    e.M, e.V = torch.zeros(LIVE), torch.zeros(LIVE) if optimizer == "Adam" else None
    for name in ("P", "G", "X", "ws", "M", "V"):
        if getattr(e, name) is not None:
            rec.names[getattr(e, name).data_ptr()] = name
    e._labels = torch.zeros(e.B, dtype=torch.int32)
    e.fused, e._sharded, e._ddp_selftest, e._ddp_buckets = bool(fused), bool(sharded), bool(selftest), int(buckets)
    e._side_update = bool(side_update) and optimizer != "Adam"
    e._n_first, e._shard_own, e._shard_layout = N_FIRST, [0, 12, 24, 44], [12, 24, 20, 64]
    e.comm = e.peer = e.comm_fallback = e._g16 = e._comm_stream = e._side = e._pending = e._P2 = e.graph = None
    e.skip_collective, e.step_count, e.bn_running, e.bn_batches, e.bf16_store = False, 0, None, 0, False
    e.dis_DA, e.ens_DA, e.use_bn, e.target_labels, e.target_entropy = "none", "none", "none", False, False
    e.class_weights = e.domain_weights = e._job_last_hyper = e._disc_scratch = None
    e._mcd_native = False
    e._global_source, e._global_target, e._hyper = e.Bs, e.Bt, _lib.Hyper()
    resolve = getattr(engine, "_resolve_switches", None)      # (an engine that settles its environment switches at construction reads them here)
    if resolve is not None:
        e._switches = resolve(env={})
    return e


def schedule(n, k0=0):
    """(beta, gamma, lr) of steps k0 .. k0 + n - 1 as main.py would evaluate them."""
    from ta3n_amd.engine import beta_dann, lr_dann
    out = []
    for k in range(k0, k0 + n):
        p = k / 40.0
        out.append(([beta_dann(p), 0.75 * beta_dann(p), 0.5 * beta_dann(p)], 0.003, lr_dann(3e-2, p)))
    return out


def _feeds(rec, n):
    import torch
    ids = torch.arange(2 * n, dtype=torch.int32).view(n, 2)
    return ((_Store(rec, "source_store"), ids), (_Store(rec, "target_store"), ids + 100))


def _program(name):
    def step(e, rec):
        for s in schedule(2):
            e.train_step(*s)

    def pipelined(e, rec):
        for s in schedule(3):
            e.train_step_pipelined(*s)
        e.flush()

    def deferred(e, rec):
        for s in schedule(2):
            e.train_step_deferred(*s)
        e.flush()

    def steps(e, rec):
        e.train_steps(schedule(5))
        e.flush()

    def steps_twice(e, rec):      # the second call opens with the update the first left pending
        e.train_steps(schedule(2))
        e.train_steps(schedule(3, 2))
        e.flush()

    def steps_feeds(e, rec):
        e.train_steps(schedule(5), feeds=_feeds(rec, 5))
        e.flush()
    return locals()[name]


def matrix():
    """name -> (stand_in keywords, program)."""
    out = {}

    def add(name, programs, **kw):
        for p in programs:
            out[f"{name}/{p}"] = (kw, p)
    fused_programs = ("step", "pipelined", "deferred", "steps", "steps_twice", "steps_feeds")
    for side in (True, False):
        for selftest in (False, True):
            for buckets in (1, 2):
                add(f"sgd/side{int(side)}/selftest{int(selftest)}/buckets{buckets}", fused_programs, side_update=side, selftest=selftest,
                    buckets=buckets)
    add("adam", fused_programs, optimizer="Adam")
    add("adam/unfused_norm", fused_programs, optimizer="Adam", unfused_norm=True)
    add("sharded", fused_programs, sharded=True, selftest=True)      # (comm None: the torch.distributed form of the sharded update)
    for opt in ("SGD", "Adam"):
        add(f"unfused/{opt.lower()}", ("step", "steps", "steps_feeds"), optimizer=opt, fused=False)
    add("unfused/sgd/selftest1", ("step",), fused=False, selftest=True)
    return out


@contextlib.contextmanager
def patched(rec):
    import torch
    from ta3n_amd import parallel

    def all_reduce_sum_async(t, group, selftest=False):
        rec.trace.append(["parallel.all_reduce_sum_async", [int(t.numel()), int(bool(selftest))]])
        return None
    with mock.patch.object(torch.cuda, "current_stream", lambda *a, **k: rec.main), mock.patch.object(torch.cuda, "Stream", rec.stream), \
            mock.patch.object(torch.cuda, "Event", rec.event), mock.patch.object(parallel, "all_reduce_sum_async", all_reduce_sum_async):
        yield


def trace(kw, program):
    """The trace of one configuration: every call in order, closed by the host state the schedule left behind."""
    rec = Recorder()
    with patched(rec):
        e = stand_in(rec, **kw)
        e._stream = lambda: C.c_void_p(rec.main.cuda_stream)
        _program(program)(e, rec)
    rec.trace.append(["state", [int(e.step_count), int(e.adam_step_count), int(e.bn_batches),
                                None if e._pending is None else [_f32(v) for v in e._pending], _f32(e._hyper.lr), int(e._hyper.seed_i)]])
    return rec.trace


def main():
    import subprocess
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        if subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "ta3n_amd"], text=True).strip():
            commit += " + local changes under ta3n_amd"
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    entries = {name: trace(kw, p) for name, (kw, p) in matrix().items()}
    with open(JSON_PATH, "w") as f:      # one line per call
        f.write('{"generated_from": %s,\n"entries": {\n' % json.dumps({"commit": commit}))
        f.write(",\n".join("%s: [\n%s]" % (json.dumps(k), ",\n".join(json.dumps(c) for c in v)) for k, v in sorted(entries.items())))
        f.write("\n}}\n")
    print("wrote", JSON_PATH, os.path.getsize(JSON_PATH), "bytes;", len(entries), "entries,", sum(len(v) for v in entries.values()), "calls")


if __name__ == "__main__":
    main()
