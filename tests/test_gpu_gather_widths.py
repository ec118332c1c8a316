"""Device batch assembly at the widths and schedules training runs: gather_kernel, both copy bodies of gather_row
(ta3n_gather_segments, ta3n_gather_segments_into, ta3n_gather_segments_bf16_into), the batch rows of the launch that opens a pipelined
step (sgd_open_feed_kernel under TrainEngine.train_steps(feeds=...)) and ta3n_train_steps_adam's gathers, bit for bit against the CPU
reference of tests/gather_cases.py (rows by the oracle's Python sampler, twin planes by torch's own bf16 conversion) - at feature widths
on both sides of every trip count of the 256-thread row loops, the element-wise copy of widths that are no multiple of 4, twin planes
at first_video > 0, the segment arithmetic at 2 .. 64 segments, schedules long enough to be split into pieces, and repeated calls.
Every buffer a gather writes is preset to a sentinel, so a row, tail element or plane that was not written - or was written where it
should not be - shows.  All comparisons are on bit patterns (int32 / int16 views): -0.0 is not +0.0, and nothing is a tolerance."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

import gather_cases as gc
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gather_refusals as mg  # noqa: E402
from ta3n_amd import _lib
from ta3n_amd.engine import TrainEngine
from ta3n_amd.feature_store import FeatureStore
from ta3n_amd.synthetic import synth_state

pytestmark = pytest.mark.gpu

SENT32 = 0x3EAC0DE5      # fp32 0.336..: a finite input value, so that a step on rows nobody assembled stays finite
SENT16 = 0x3EAC          # bf16 0.3359375
ENGINES = {"f32": {}, "bf16": dict(bf16=True, bf16_store=True), "pair": dict(f32_split=True, bf16_store=True)}      # pair: hi + lo twin planes
TINY = (6, 4, 5, 64, 32, 7)      # Bs, Bt, T, D, fc_dim, C


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32).cpu()


def _plane(eng, name) -> torch.Tensor:
    """A twin plane of the input as int16 [B T, D] on the CPU (the region holds exactly B T D bf16 elements)."""
    r = eng.region(name).view(torch.int16)
    assert r.numel() == eng.X.numel()
    return r.cpu().view(eng.B * eng.T, eng.D)


def _preset(eng) -> None:
    eng.X.view(torch.int32).fill_(SENT32)
    for name in ("x16", "x16_lo"):
        if name in eng.plan.regions:
            eng.region(name).view(torch.int16).fill_(SENT16)


def _buffers(eng, kind):
    """(X bits, hi plane, lo plane) of an engine; None where the engine keeps no such plane."""
    torch.cuda.synchronize()
    assert ("x16" in eng.plan.regions) == (kind != "f32") and ("x16_lo" in eng.plan.regions) == (kind == "pair")
    return (_bits(eng.X), _plane(eng, "x16") if kind != "f32" else None, _plane(eng, "x16_lo") if kind == "pair" else None)


def _expected(dims, kind, store_bf16, parts):
    """What _buffers must return after gathers into preset buffers.  parts: (first_video, Case, ids) per gather."""
    Bs, Bt, T, D = dims[:4]
    rows = (Bs + Bt) * T
    X = torch.full((rows, D), SENT32, dtype=torch.int32)
    hi = torch.full((rows, D), SENT16, dtype=torch.int16)
    lo = torch.full((rows, D), SENT16, dtype=torch.int16)
    twin = kind != "f32"
    for first, case, ids in parts:
        ref = case.reference(ids, bf16_store=store_bf16)
        r0, r1 = first * T, (first + len(ids)) * T
        if not (store_bf16 and twin):      # a bf16 store feeding a twin-reading engine writes no fp32 rows
            X[r0:r1] = ref["x"].contiguous().view(torch.int32)
        hi[r0:r1], lo[r0:r1] = ref["hi"], ref["lo"]
    return X, hi if twin else None, lo if kind == "pair" else None


def _assert_buffers(got, want, what):
    for name, g, w in zip(("X", "hi plane", "lo plane"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None and not torch.equal(g, w):
            bad = (g != w).nonzero()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} elements, first (row, column) {bad[0].tolist()}, last {bad[-1].tolist()}")


# ---- a. ta3n_gather_segments ----
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("D", gc.F32_VECTOR_WIDTHS + gc.F32_SCALAR_WIDTHS)
def test_gather_segments_rows_labels_and_frame_numbers(D, T):
    case = gc.case(T, D)
    store = case.store()
    ids = gc.id_list(len(case), 9, seed=D + T)
    n = len(ids)
    ref = case.reference(ids)
    buf = torch.empty((n * T + 2, D), dtype=torch.float32, device="cuda")      # a guard row in front and behind
    lab = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    seg = torch.empty(n * T + 2, dtype=torch.int32, device="cuda")

    def preset():
        buf.view(torch.int32).fill_(SENT32)
        lab.fill_(-7)
        seg.fill_(-7)
    preset()
    x, y = store.gather(torch.tensor(ids, dtype=torch.int32).cuda(), T, out=buf[1:1 + n * T], labels_out=lab[1:1 + n],
                        segment_ids_out=seg[1:1 + n * T])
    torch.cuda.synchronize()
    assert x.shape == (n, T, D) and x.data_ptr() == buf[1].data_ptr()
    got = _bits(buf)
    assert torch.equal(got[1:-1], ref["x"].contiguous().view(torch.int32)), (D, T)
    assert (got[0] == SENT32).all() and (got[-1] == SENT32).all(), "guard rows"
    assert torch.equal(lab[1:-1].cpu(), ref["labels"]) and lab[0].item() == -7 and lab[-1].item() == -7
    assert torch.equal(seg[1:-1].cpu(), ref["seg"]) and seg[0].item() == -7 and seg[-1].item() == -7
    # n_videos = 0: accepted, and nothing is written
    preset()
    p = lambda t: C.c_void_p(t.data_ptr())
    dev_ids = torch.tensor(ids, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().ta3n_gather_segments(p(store.store), p(store.first_row), p(store.num_frames), p(store.labels), p(dev_ids), 0, T, D,
                                               p(buf[1]), p(lab[1:]), p(seg[1:]), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "ta3n_gather_segments")
    torch.cuda.synchronize()
    assert (_bits(buf) == SENT32).all() and (lab == -7).all() and (seg == -7).all()


# ---- b. the segment arithmetic on the device ----
@pytest.mark.parametrize("T", gc.INDEX_SEGMENTS)
def test_device_segment_indices_equal_the_python_oracle(T):
    lengths = list(range(1, 401)) + list(gc.LONG_CLIPS)
    total, D = sum(lengths), 4
    assert total < 1 << 24                                                      # row numbers are exact in fp32
    blob = torch.arange(total, dtype=torch.float32).view(-1, 1).expand(total, D).contiguous().cuda()      # row r holds the value r
    store = FeatureStore.from_tensors(blob, torch.tensor(lengths), torch.zeros(len(lengths), dtype=torch.int32))
    ids = list(range(len(lengths) - 1, -1, -1))
    seg = torch.empty(len(ids) * T, dtype=torch.int32, device="cuda")
    x, _ = store.gather(torch.tensor(ids, dtype=torch.int32).cuda(), T, segment_ids_out=seg)
    torch.cuda.synchronize()
    want = torch.tensor([gc.segment_frames(lengths[v], T) for v in ids], dtype=torch.int64)
    first = torch.cumsum(torch.tensor(lengths), 0) - torch.tensor(lengths)
    assert torch.equal(seg.view(-1, T).cpu().to(torch.int64), want)
    want_rows = (first[torch.tensor(ids)].view(-1, 1) + want - 1).to(torch.float32)
    got = x.cpu()
    for col in range(D):
        assert torch.equal(got[:, :, col], want_rows), col


# ---- c. gather_into for every (engine, store) pair that trains ----
def _gather_into_widths(store_bf16):
    """(D, refused): the widths of the store's table, and the widths its entry point refuses by the % 4 / % 8 rule."""
    if store_bf16:
        return [(D, False) for D in gc.BF16_WIDTHS] + [(D, True) for D in gc.F32_VECTOR_WIDTHS if D % 8]
    return [(D, False) for D in gc.F32_VECTOR_WIDTHS] + [(D, True) for D in (37, 1030)]


@pytest.mark.parametrize("kind,store_bf16,D,refused", [(k, s, D, r) for k in ENGINES for s in (False, True) for D, r in _gather_into_widths(s)])
def test_gather_into_writes_rows_and_twin_planes_at_every_width(kind, store_bf16, D, refused):
    Bs, Bt, F, Cn = 3, 2, 32, 5
    T = 5 if 1024 <= D <= 2056 else 2
    case = gc.case(T, D)
    store = case.store(bf16=store_bf16)
    eng = TrainEngine(Bs, Bt, T, D, F, Cn, dropout_i=0.0, dropout_v=0.0, **ENGINES[kind])
    _preset(eng)
    eng._labels.fill_(-7)
    ids_s, ids_t = gc.id_list(len(case), Bs, seed=D), gc.id_list(len(case), Bt - 1, seed=D + 1)      # one target video stays unassembled
    dev = lambda ids: torch.tensor(ids, dtype=torch.int32).cuda()
    dims = (Bs, Bt, T, D)
    if refused:
        rule = 8 if store_bf16 else 4
        assert D % rule
        for ids, first in ((ids_s, 0), (ids_t, Bs)):
            with pytest.raises(ValueError, match=f"feature_dim % {rule} and 16-byte alignment required"):
                store.gather_into(eng, dev(ids), first, labels_out=eng._labels[:Bs] if first == 0 else None)
        _assert_buffers(_buffers(eng, kind), _expected(dims, kind, store_bf16, []), f"refused width {D}")
        assert (eng._labels[:Bs] == -7).all()
        return
    store.gather_into(eng, dev(ids_s), 0, labels_out=eng._labels[:Bs])
    store.gather_into(eng, dev(ids_t), Bs)
    want = _expected(dims, kind, store_bf16, [(0, case, ids_s), (Bs, case, ids_t)])
    if store_bf16 and kind != "f32":
        assert (want[0] == SENT32).all()                                          # X untouched
    assert (want[0][(Bs + Bt - 1) * T:] == SENT32).all()                         # the last video's rows: sentinel in all three
    _assert_buffers(_buffers(eng, kind), want, f"{kind} engine, {'bf16' if store_bf16 else 'fp32'} store, width {D}")
    assert torch.equal(eng._labels[:Bs].cpu(), case.reference(ids_s)["labels"])


# ---- d / e / f. the batch rows of train_steps(feeds=...) against one gather_into + train_step_pipelined per step ----
def _schedule(n):
    return [([0.75, 0.75, 0.5], 0.003, 2e-3 * (1.0 + 0.05 * k)) for k in range(n)]


def _state(eng, kind):
    eng.flush()
    torch.cuda.synchronize()
    out = dict(P=_bits(eng.P), M=_bits(eng.M), losses=_bits(eng.region("losses")[:6]), labels=eng._labels[: eng.Bs].cpu())
    if eng.V is not None:
        out["V"] = _bits(eng.V)
    out["X"], out["hi"], out["lo"] = _buffers(eng, kind)
    assert torch.isfinite(eng.P).all() and torch.isfinite(eng.region("losses")[:6]).all() and eng.losses()["loss"] > 0
    return out


def _same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs at {(a[k] != b[k]).sum().item()} of {a[k].numel()} elements"


def _train(dims, kind, store_bf16, n_steps, calls=None, halves=(True, True), fewer=(0, 0), optimizer="SGD", before=None, between=None, host_tables=False):
    """calls None: per step, one gather_into per fed half + train_step_pipelined.  calls [(lo, hi), ...]: train_steps(feeds=...) over
    those step ranges; before(engine, k) / between(engine, k) run right before / after the k-th call.  Returns (state, cases, id tables,
    engine)."""
    Bs, Bt, T, D, F, Cn = dims
    cases = (gc.case(T, D, seed=1, train=True), gc.case(T, D, seed=2, train=True))
    stores = [c.store(bf16=store_bf16) for c in cases]
    tables = [gc.id_table(len(c), n_steps, half - less, seed=11 + i) for i, (c, half, less) in enumerate(zip(cases, (Bs, Bt), fewer))]
    eng = TrainEngine(Bs, Bt, T, D, F, Cn, dropout_i=0.5, dropout_v=0.5, optimizer=optimizer, **ENGINES[kind])
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    _preset(eng)
    eng._labels.zero_()
    sched = _schedule(n_steps)
    # host_tables: int64 tables on the host - the engine then builds the device tables itself and nothing else keeps them alive
    given = [t.to(torch.int64) if host_tables else t.cuda() for t in tables]
    if calls is None:
        for k, (beta, gamma, lr) in enumerate(sched):
            if halves[0]:
                stores[0].gather_into(eng, tables[0][k].cuda(), 0, labels_out=eng._labels[:Bs])
            if halves[1]:
                stores[1].gather_into(eng, tables[1][k].cuda(), Bs)
            eng.train_step_pipelined(beta, gamma, lr)
    else:
        assert eng.can_batch_steps()      # one library call per piece: the batches are assembled by the launch that opens each step
        for i, (lo, hi) in enumerate(calls):
            if before is not None:
                before(eng, i)
            eng.train_steps(sched[lo:hi], feeds=tuple((st if on else None, ids[lo:hi] if on else None)
                                                      for st, ids, on in zip(stores, given, halves)))
            if between is not None:
                between(eng, i)
    assert eng.step_count == n_steps
    return _state(eng, kind), cases, tables, eng


def _assert_last_batch(state, dims, kind, store_bf16, cases, tables, halves=(True, True)):
    """X, the twin planes and the labels after the run: the reference rows of the LAST step's ids, the sentinel everywhere else."""
    Bs = dims[0]
    parts = [(first, c, t[-1].tolist()) for first, c, t, on in zip((0, Bs), cases, tables, halves) if on]
    _assert_buffers((state["X"], state["hi"], state["lo"]), _expected(dims[:4], kind, store_bf16, parts), "last step's batch")
    if halves[0]:
        n = tables[0].shape[1]
        assert torch.equal(state["labels"][:n], cases[0].reference(tables[0][-1].tolist())["labels"])


WIDE = (6, 4, 5, 2048, 64, 7)


@pytest.mark.parametrize("kind,store_bf16,D", [("f32", False, 2048), ("bf16", False, 2048), ("bf16", True, 2048), ("pair", False, 2048),
                                               ("pair", True, 2048), ("bf16", True, 4096)])
def test_opening_launch_assembles_the_batches_of_per_step_gathers(kind, store_bf16, D):
    dims = WIDE[:3] + (D,) + WIDE[4:]
    n = 5
    a, cases, tables, _ = _train(dims, kind, store_bf16, n)
    b, _, _, _ = _train(dims, kind, store_bf16, n, calls=[(0, n)])
    _same_state(a, b, f"{kind} engine, {'bf16' if store_bf16 else 'fp32'} store, width {D}")
    _assert_last_batch(b, dims, kind, store_bf16, cases, tables)


@pytest.mark.parametrize("halves", [(True, False), (False, True)], ids=["source_only", "target_only"])
@pytest.mark.parametrize("kind,store_bf16", [("f32", False), ("pair", True)])
def test_opening_launch_with_one_half_absent(kind, store_bf16, halves):
    n = 5
    a, cases, tables, _ = _train(WIDE, kind, store_bf16, n, halves=halves)
    b, _, _, _ = _train(WIDE, kind, store_bf16, n, calls=[(0, n)], halves=halves)
    _same_state(a, b, f"{kind}, halves {halves}")
    _assert_last_batch(b, WIDE, kind, store_bf16, cases, tables, halves=halves)      # the half nobody feeds keeps the sentinel


@pytest.mark.parametrize("kind,store_bf16", [("f32", False), ("bf16", True), ("pair", False)])
def test_opening_launch_with_fewer_ids_than_the_batch_half(kind, store_bf16):
    n, fewer = 5, (2, 1)
    a, cases, tables, _ = _train(WIDE, kind, store_bf16, n, fewer=fewer)
    b, _, _, _ = _train(WIDE, kind, store_bf16, n, calls=[(0, n)], fewer=fewer)
    assert tables[0].shape == (n, WIDE[0] - 2) and tables[1].shape == (n, WIDE[1] - 1)
    _same_state(a, b, f"{kind}, fewer ids")
    _assert_last_batch(b, WIDE, kind, store_bf16, cases, tables)                      # the rows behind each half's ids keep the sentinel


def test_opening_launch_with_the_update_grid_at_its_cap():
    """The shared frame FC longer than 2048 blocks x 256 threads x 4 floats: the update workgroups stride over their range and the batch
    rows start at blockIdx.x - 2048."""
    dims = (3, 2, 2, 4096, 520, 5)
    n = 4
    a, cases, tables, eng = _train(dims, "pair", False, n)
    (_, off0, shape0, _), (_, off1, shape1, _) = eng.plan.params[:2]
    assert off0 == 0 and tuple(shape0) == (520, 4096) and tuple(shape1) == (520,)
    opening = off1 + shape1[0]                                                     # the range the opening launch updates: weight + bias
    assert opening > 2048 * 256 * 4, opening
    b, _, _, _ = _train(dims, "pair", False, n, calls=[(0, n)])
    _same_state(a, b, "capped update grid")
    _assert_last_batch(b, dims, "pair", False, cases, tables)


@pytest.mark.parametrize("kind,store_bf16", [("f32", False), ("bf16", True)])
def test_long_and_repeated_schedules_keep_every_id_table(kind, store_bf16):
    """40 steps in one call (pieces of 1, 16 and 23 steps, each with its own slice of the id tables), then a second call of 6.  The
    tables are given on the host, so the device tables are the engine's own; they must all be alive while their gathers are queued.
    After each call other valid ids are written into fresh tensors of the tables' shapes (on the step's stream and once more from a
    second stream): a table read after its release yields wrong rows, never an index outside the store.  Work on one stream runs in
    order and the caching allocator hands a freed block to that stream first, so a table released too early is usually rewritten only
    behind the gathers that read it and the rows alone need not show it: the count of live device allocations around the first call
    does, whatever the timing (with `_feed_keep` replaced per piece it grows by 2 instead of 4)."""
    n, first_call = 46, 40
    live = lambda: torch.cuda.memory_stats()["allocation.all.current"]
    scribbled, marks = [], []
    side = torch.cuda.Stream()

    def before(eng, i):
        marks.append(live())

    def between(eng, i):
        marks.append(live())
        for c, half in zip((0, 1), TINY[:2]):
            for steps in (1, 16, 23, 5, 6, n):
                ref = gc.id_table(12, steps, half, seed=11 + c)
                t = gc.other_ids(ref, 12).cuda()                # allocated and filled on the step's stream
                with torch.cuda.stream(side):
                    t.copy_(gc.other_ids(ref, 12).flip(0), non_blocking=True)      # ... and rewritten without waiting for it
                t.record_stream(side)
                scribbled.append(t)

    a, cases, tables, _ = _train(TINY, kind, store_bf16, n)
    b, _, _, eng = _train(TINY, kind, store_bf16, n, calls=[(0, first_call), (first_call, n)], before=before, between=between,
                          host_tables=True)
    assert len(cases[0]) == 12 and len(cases[1]) == 12
    _same_state(a, b, f"{kind}: 40 + 6 steps by train_steps against one call per step")
    _assert_last_batch(b, TINY, kind, store_bf16, cases, tables)
    # when the 40-step call returned, the device tables of its pieces behind the first step - 2 pieces x 2 halves - were still allocated
    # (allocations alive after the call that were not before it)
    assert len(marks) == 4 and marks[1] - marks[0] >= 4, marks


def test_adam_steps_with_feeds_equal_per_step_gathers():
    n = 7
    a, cases, tables, eng = _train(TINY, "f32", False, n, optimizer="Adam")
    b, _, _, eng_b = _train(TINY, "f32", False, n, calls=[(0, n)], optimizer="Adam")
    assert eng.adam_step_count == n and eng_b.adam_step_count == n and "V" in a
    _same_state(a, b, "Adam: parameters, exp_avg, exp_avg_sq, losses, batch")
    _assert_last_batch(b, TINY, "f32", False, cases, tables)
    assert a["M"].ne(0).any() and a["V"].ne(0).any()


# ---- g. what a ta3n_feed is refused for, before anything is launched ----
def test_feed_refusals_precede_every_launch_of_the_call():
    """ta3n_train_steps and ta3n_train_steps_adam with n_steps = 1 and a source feed that breaks one rule per call (more ids than the
    batch half, a null first_row, no labels, sampler 3): TA3N_ERR_INVALID with the text recorded in tests/golden/gather_refusals.json
    before the feed checks were merged, and - the refusal comes before the first launch of step 0 in both entry points (the pipelined
    step checks both feeds before its norm pass; the Adam loop assembles the source half first) - X, both twin planes and P keep their
    bits."""
    with open(mg.JSON_PATH) as f:
        golden = {(e, v): (rc, text) for e, v, rc, text in json.load(f)["feeds"]}
    case = gc.case(TINY[2], TINY[3], seed=1, train=True)
    stores = (case.store(), case.store())
    tables = tuple(gc.id_table(len(case), 1, n, seed=11 + i).cuda() for i, n in enumerate(TINY[:2]))
    for entry in mg.FEED_ENTRIES:
        eng = TrainEngine(*TINY, dropout_i=0.5, dropout_v=0.5, optimizer="Adam" if entry.endswith("adam") else "SGD", **ENGINES["pair"])
        eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
        _preset(eng)
        before = _buffers(eng, "pair") + (_bits(eng.P),)
        for violation in mg.FEED_CASES:
            got = mg.ask_feed(eng, stores, tables, entry, violation)
            print(entry, violation, got)
            assert got[0] == -1 and got == tuple(golden[entry, violation]), (entry, violation)
            after = _buffers(eng, "pair") + (_bits(eng.P),)      # (synchronises)
            for name, a, b in zip(("X", "hi plane", "lo plane", "P"), before, after):
                assert torch.equal(a, b), (entry, violation, name)
