"""The val- and train-mode segment samplers of the device batch assembly: the stand-alone gathers (ta3n_gather_segments_sampled,
ta3n_gather_segments_bf16), gather_into with a sampler, and the batch rows of train_steps(feeds=(store.sampled(...), ids)) - inside the
launch that opens a pipelined step, under Adam, split into pieces and step by step - against the pure-Python restatement of
tests/sampler_reference.py (which shares no code with the library).  Every comparison is on bit patterns, every buffer a gather writes
is preset to a sentinel (tests/test_gpu_gather_widths.py's helpers).  The stores of the stand-alone and gather_into tests hold the
1-frame clip first and the 400-frame clip last, and every id list names both: a draw outside [0, avg) reads another video's rows or
rows past the store, and shows as wrong bits."""
import ctypes as C
import functools

import pytest
import torch

import gather_cases as gc
import sampler_reference as sr
import test_gpu_gather_widths as gw
from ta3n_amd import _lib
from ta3n_amd.engine import TrainEngine
from ta3n_amd.synthetic import synth_state

pytestmark = pytest.mark.gpu

SENT32 = gw.SENT32
TINY, WIDE = gw.TINY, gw.WIDE


@functools.lru_cache(maxsize=None)
def _case(T, D, seed=0, train=False):
    """gather_cases' dozen clips in ascending length: video 0 has one frame, video 11 has 400 (treat as read-only)."""
    counts = sorted(gc.frame_counts(T))
    assert counts[0] == 1 and counts[-1] == 400 and len(counts) == 12
    return gc.Case(T, D, seed, num_frames=counts, **(dict(exps=(-6, -1), specials=False) if train else {}))


def _dev(ids):
    return torch.tensor(ids, dtype=torch.int32).cuda()


# ---- 1. ta3n_gather_segments_sampled ----
@pytest.mark.parametrize("T", [2, 5, 64])
@pytest.mark.parametrize("D", [4, 1028, 37])
def test_sampled_gather_rows_labels_and_frame_numbers(D, T):
    case = _case(T, D)
    store = case.store()
    n = 7
    buf = torch.empty((n * T + 2, D), dtype=torch.float32, device="cuda")      # a guard row in front and behind
    lab = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    seg = torch.empty(n * T + 2, dtype=torch.int32, device="cuda")
    drawn = set()
    for sampler in ("val", "train"):
        for seed in (3, 0xC0FFEE11):
            ids = gc.id_list(len(case), n, seed=seed & 0xFFFF)
            assert ids[0] == ids[-1] == 11 and ids[1] == 0                  # the 400-frame clip in two slots, the 1-frame clip
            for step in (0, 3):
                ref = sr.reference(case, ids, sampler, seed=seed, step=step)
                buf.view(torch.int32).fill_(SENT32)
                lab.fill_(-7)
                seg.fill_(-7)
                x, y = store.gather(_dev(ids), T, out=buf[1:1 + n * T], labels_out=lab[1:1 + n], segment_ids_out=seg[1:1 + n * T],
                                    sampler=sampler, seed=seed, step=step)
                torch.cuda.synchronize()
                what = (sampler, seed, step)
                assert x.shape == (n, T, D) and x.data_ptr() == buf[1].data_ptr()
                got = gw._bits(buf)
                assert torch.equal(seg[1:-1].cpu(), ref["seg"]) and seg[0].item() == -7 and seg[-1].item() == -7, what
                assert torch.equal(got[1:-1], ref["x"].contiguous().view(torch.int32)), what
                assert (got[0] == SENT32).all() and (got[-1] == SENT32).all(), "guard rows"
                assert torch.equal(lab[1:-1].cpu(), ref["labels"]) and lab[0].item() == -7 and lab[-1].item() == -7
                if sampler == "train":
                    drawn.add(tuple(ref["seg"][:T].tolist()))
                    assert ref["seg"][:T].tolist() != ref["seg"][-T:].tolist()      # one video, two slots, two draws
    assert len(drawn) == 4                                                          # the key: seed and step


def test_sampled_gather_refuses_an_unknown_sampler():
    case = _case(2, 4)
    store = case.store()
    out = torch.full((2, 4), 1.5, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().ta3n_gather_segments_sampled(p(store.store), p(store.first_row), p(store.num_frames), p(store.labels), p(_dev([0])), 1, 2, 4,
                                                 p(out), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream), 3, 0, 0)
    torch.cuda.synchronize()
    assert rc != 0 and b"sampler" in _lib.lib().ta3n_last_error() and (out == 1.5).all()


# ---- 2. ta3n_gather_segments_bf16 ----
def _old_bf16_gather(store, ids, T):
    """FeatureStore.gather on a bf16 store before it had a kernel: frames on the host, rows widened by torch."""
    ids = ids.to(torch.int32)
    seg = torch.tensor([[s - 1 for s in _lib.segment_indices(int(nf), T)] for nf in store.num_frames[ids.long()].tolist()],
                       device=store.device, dtype=torch.long)
    rows = store.first_row[ids.long()].unsqueeze(1) + seg
    return store.store[rows.reshape(-1)].view(torch.bfloat16).to(torch.float32).view(ids.numel(), T, store.feature_dim), store.labels[ids.long()]


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("D", [8, 2056])
def test_bf16_store_gather_widens_the_rows_of_every_sampler(D, T):
    case = _case(T, D)
    store = case.store(bf16=True)
    assert store.bf16
    n = 7
    ids = gc.id_list(len(case), n, seed=D + T)
    buf = torch.empty((n * T + 2, D), dtype=torch.float32, device="cuda")
    lab = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    seg = torch.empty(n * T + 2, dtype=torch.int32, device="cuda")
    for sampler in ("test", "val", "train"):
        ref = sr.reference(case, ids, sampler, seed=21, step=2, bf16_store=True)
        assert torch.equal(ref["x"], case.rows[(ref["seg"].long() - 1) + torch.tensor([int(case.first_row[v]) for v in ids for _ in range(T)])]
                           .to(torch.bfloat16).to(torch.float32))
        buf.view(torch.int32).fill_(SENT32)
        lab.fill_(-7)
        seg.fill_(-7)
        x, y = store.gather(_dev(ids), T, out=buf[1:1 + n * T], labels_out=lab[1:1 + n], segment_ids_out=seg[1:1 + n * T],
                            sampler=sampler, seed=21, step=2)
        torch.cuda.synchronize()
        got = gw._bits(buf)
        assert torch.equal(seg[1:-1].cpu(), ref["seg"]) and seg[0].item() == -7 and seg[-1].item() == -7, sampler
        assert torch.equal(got[1:-1], ref["x"].contiguous().view(torch.int32)), sampler
        assert (got[0] == SENT32).all() and (got[-1] == SENT32).all(), "guard rows"
        assert torch.equal(lab[1:-1].cpu(), ref["labels"]) and lab[0].item() == -7 and lab[-1].item() == -7
        if sampler == "test":
            old_x, old_y = _old_bf16_gather(store, _dev(ids), T)
            assert torch.equal(gw._bits(x), gw._bits(old_x)) and torch.equal(y.cpu(), old_y.cpu())
            fresh_x, fresh_y = store.gather(_dev(ids), T)                       # the defaults, buffers of its own
            assert torch.equal(gw._bits(fresh_x), gw._bits(old_x)) and torch.equal(fresh_y.cpu(), old_y.cpu())


# ---- 3. gather_into ----
def _expected(dims, kind, store_bf16, parts, sampler, seed, step):
    """gw._expected for a sampler.  parts: (first_video, Case, ids) per gather."""
    Bs, Bt, T, D = dims[:4]
    rows = (Bs + Bt) * T
    X = torch.full((rows, D), SENT32, dtype=torch.int32)
    hi = torch.full((rows, D), gw.SENT16, dtype=torch.int16)
    lo = torch.full((rows, D), gw.SENT16, dtype=torch.int16)
    twin = kind != "f32"
    for first, case, ids in parts:
        ref = sr.reference(case, ids, sampler, seed=seed, step=step, bf16_store=store_bf16)
        r0, r1 = first * T, (first + len(ids)) * T
        if not (store_bf16 and twin):
            X[r0:r1] = ref["x"].contiguous().view(torch.int32)
        hi[r0:r1], lo[r0:r1] = ref["hi"], ref["lo"]
    return X, hi if twin else None, lo if kind == "pair" else None


@pytest.mark.parametrize("store_bf16", [False, True], ids=["f32_store", "bf16_store"])
@pytest.mark.parametrize("kind", list(gw.ENGINES))
def test_gather_into_with_the_train_sampler(kind, store_bf16):
    Bs, Bt, T, D, F, Cn = TINY
    case = _case(T, D)
    store = case.store(bf16=store_bf16)
    eng = TrainEngine(Bs, Bt, T, D, F, Cn, dropout_i=0.0, dropout_v=0.0, **gw.ENGINES[kind])
    ids = gc.id_list(len(case), Bt, seed=5)
    assert ids[0] == ids[-1] == 11 and ids[1] == 0
    what = f"{kind} engine, {'bf16' if store_bf16 else 'fp32'} store"
    halves = {}
    for first in (0, Bs):
        gw._preset(eng)
        eng._labels.fill_(-7)
        store.gather_into(eng, _dev(ids), first, labels_out=eng._labels[first:first + Bt], sampler="train", seed=77, step=9)
        got = gw._buffers(eng, kind)
        gw._assert_buffers(got, _expected(TINY, kind, store_bf16, [(first, case, ids)], "train", 77, 9), f"{what}, first_video {first}")
        assert torch.equal(eng._labels[first:first + Bt].cpu(), case.labels[torch.tensor(ids)])
        halves[first] = [None if b is None else b[first * T:(first + Bt) * T] for b in got]
    for a, b in zip(halves[0], halves[Bs]):                                     # first_video is no part of the key
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    # sampler="test" is the entry point without a sampler, bit for bit
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw._preset(eng)
    if store_bf16:
        _lib.check(L.ta3n_gather_segments_bf16_into(eng.plan.handle, p(store.store), p(store.first_row), p(store.num_frames), p(store.labels),
                                                    p(_dev(ids)), len(ids), Bs, None if eng.bf16_store else p(eng.X), p(eng.ws), None, stream),
                   "ta3n_gather_segments_bf16_into")
    else:
        _lib.check(L.ta3n_gather_segments_into(eng.plan.handle, p(store.store), p(store.first_row), p(store.num_frames), p(store.labels),
                                               p(_dev(ids)), len(ids), Bs, p(eng.X), p(eng.ws), None, stream), "ta3n_gather_segments_into")
    old = gw._buffers(eng, kind)
    gw._preset(eng)
    store.gather_into(eng, _dev(ids), Bs, sampler="test", seed=77, step=9)
    gw._assert_buffers(gw._buffers(eng, kind), old, f"{what}: sampler test against the entry point without a sampler")
    gw._assert_buffers(old, _expected(TINY, kind, store_bf16, [(Bs, case, ids)], "test", 0, 0), f"{what}: test mode")


# ---- 4 - 7. train_steps(feeds=(store.sampled(...), ids)) ----
SEEDS = (5, 6)      # source, target


def _train(dims, kind, store_bf16, n_steps, calls=None, sampler="train", optimizer="SGD", watch=None):
    """calls None: per step, gather_into(..., sampler, seed, step=eng.step_count) per half + train_step_pipelined.  calls [(lo, hi), ...]:
    train_steps(feeds=((src.sampled(sampler, 5), ids), (tgt.sampled(sampler, 6), ids))) over those step ranges.  watch: a list that receives
    the fp32 rows of slot 0 of the source half after every per-step gather.  Returns (state, cases, id tables, engine)."""
    Bs, Bt, T, D, F, Cn = dims
    cases = (_case(T, D, seed=1, train=True), _case(T, D, seed=2, train=True))
    stores = [c.store(bf16=store_bf16) for c in cases]
    tables = [gc.id_table(len(c), n_steps, half, seed=11 + i) for i, (c, half) in enumerate(zip(cases, (Bs, Bt)))]
    eng = TrainEngine(Bs, Bt, T, D, F, Cn, dropout_i=0.5, dropout_v=0.5, optimizer=optimizer, **gw.ENGINES[kind])
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    gw._preset(eng)
    eng._labels.zero_()
    sched = gw._schedule(n_steps)
    if calls is None:
        for k, (beta, gamma, lr) in enumerate(sched):
            assert eng.step_count == k
            stores[0].gather_into(eng, tables[0][k].cuda(), 0, labels_out=eng._labels[:Bs], sampler=sampler, seed=SEEDS[0], step=eng.step_count)
            stores[1].gather_into(eng, tables[1][k].cuda(), Bs, sampler=sampler, seed=SEEDS[1], step=eng.step_count)
            if watch is not None:
                watch.append(eng.X[:T].clone())
            eng.train_step_pipelined(beta, gamma, lr)
    else:
        views = [st.sampled(sampler, seed) for st, seed in zip(stores, SEEDS)]
        assert views[0].store.data_ptr() == stores[0].store.data_ptr() and (views[1].sampler, views[1].seed) == (sr.CODES[sampler], SEEDS[1])
        for lo, hi in calls:
            eng.train_steps(sched[lo:hi], feeds=tuple((v, t[lo:hi].cuda()) for v, t in zip(views, tables)))
    assert eng.step_count == n_steps
    return gw._state(eng, kind), cases, tables, eng


def _assert_last_batch(state, dims, kind, store_bf16, cases, tables, sampler="train"):
    """X, the twin planes and the labels after the run: the reference's draw for the LAST step, each half with its own seed."""
    Bs, T = dims[0], dims[2]
    step = tables[0].shape[0] - 1
    want = [_expected(dims[:4], kind, store_bf16, [(first, c, t[-1].tolist())], sampler, seed, step)
            for first, c, t, seed in zip((0, Bs), cases, tables, SEEDS)]
    merged = tuple(None if a is None else torch.cat([a[:Bs * T], b[Bs * T:]]) for a, b in zip(*want))
    gw._assert_buffers((state["X"], state["hi"], state["lo"]), merged, "last step's batch")
    assert torch.equal(state["labels"], cases[0].labels[tables[0][-1].long()])


@pytest.mark.parametrize("kind,store_bf16", [("f32", False), ("f32", True), ("bf16", True)])
def test_opening_launch_draws_the_frames_of_per_step_gathers(kind, store_bf16):
    n = 5
    a, cases, tables, _ = _train(WIDE, kind, store_bf16, n)
    b, _, _, eng = _train(WIDE, kind, store_bf16, n, calls=[(0, n)])
    assert eng.can_batch_steps()
    gw._same_state(a, b, f"{kind} engine, {'bf16' if store_bf16 else 'fp32'} store")
    _assert_last_batch(b, WIDE, kind, store_bf16, cases, tables)


def _frames_of(case, video, rows):
    """1-based frame numbers of fp32 rows [T, D] that are rows of `video`."""
    first, nf = int(case.first_row[video]), case.num_frames[video]
    clip = case.rows[first:first + nf].contiguous().view(torch.int32)
    out = []
    for r in rows.contiguous().view(torch.int32):
        hit = (clip == r).all(dim=1).nonzero().view(-1).tolist()
        assert len(hit) == 1
        out.append(hit[0] + 1)
    return out


def test_split_schedules_and_repeated_calls_draw_by_the_absolute_step(monkeypatch):
    """35 steps: one call (pieces of 1, 16 and 18 steps), two calls, and an engine without a single library call for its steps (it runs
    them one by one) against 35 single steps - a step0 counted from the piece, or from the call, draws other frames.  And the draw
    varies: over the 35 steps slot 0 of the source half - always the 400-frame clip - sees more than one frame per segment, and exactly
    one with the test-mode sampler."""
    n, T = 35, TINY[2]
    watch = []
    a, cases, tables, _ = _train(TINY, "f32", False, n, watch=watch)
    assert (tables[0][:, 0] == 11).all() and cases[0].num_frames[11] == 400
    frames = [_frames_of(cases[0], 11, rows.cpu()) for rows in watch]
    assert frames == [sr.frames("train", 400, T, SEEDS[0], k, 0) for k in range(n)]
    for x in range(T):
        assert len({f[x] for f in frames}) > 1, (x, frames)
    b, _, _, _ = _train(TINY, "f32", False, n, calls=[(0, n)])
    gw._same_state(a, b, "one call of 35 steps")
    _assert_last_batch(b, TINY, "f32", False, cases, tables)
    c, _, _, _ = _train(TINY, "f32", False, n, calls=[(0, 20), (20, n)])
    gw._same_state(a, c, "calls of 20 and 15 steps")
    monkeypatch.setenv("TA3N_SIDE_UPDATE", "0")
    d, _, _, eng = _train(TINY, "f32", False, n, calls=[(0, 20), (20, n)])
    assert not eng.can_batch_steps()
    gw._same_state(a, d, "step by step (no single library call)")
    monkeypatch.delenv("TA3N_SIDE_UPDATE")
    watch = []
    _train(TINY, "f32", False, n, sampler="test", watch=watch)
    frames = [_frames_of(cases[0], 11, rows.cpu()) for rows in watch]
    assert all(f == gc.segment_frames(400, T) for f in frames)


def test_adam_steps_with_sampled_feeds_equal_per_step_gathers():
    n = 4
    a, cases, tables, eng = _train(TINY, "f32", False, n, optimizer="Adam")
    b, _, _, eng_b = _train(TINY, "f32", False, n, calls=[(0, n)], optimizer="Adam")
    assert eng.adam_step_count == n and eng_b.adam_step_count == n and "V" in a
    gw._same_state(a, b, "Adam: parameters, exp_avg, exp_avg_sq, losses, batch")
    _assert_last_batch(b, TINY, "f32", False, cases, tables)
