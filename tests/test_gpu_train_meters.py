"""GPU: the training meters (TA3N_FLAG_TRAIN_METERS, include/ta3n_hip.h; ta3n_amd/csrc/ta3n_meters.hip).

  1. the meters launch alone on crafted regions: every count exact, every float64 sum bit for bit against meters_reference.reference_step;
     accumulation, ta3n_meters_reset, the same sequence twice; the launch writes its two regions and nothing else
  2. a non-finite total loss counts the step and adds nothing
  3. the reference's own trajectories (fixtures of tests/golden): Prec@1 / Prec@5 as its log printed them, window values, loss sums
  4. a flagged and an unflagged engine leave the same parameters, momentum and workspace
  5. one K-step call with feeds against K single calls
  6. two ranks sharing the GPU against the single-process global batch
"""
import ctypes as C
import functools
import os
import re
import socket

import numpy as np
import pytest
import torch

import meters_reference as mr
from golden_util import Golden, case_config, step_schedule
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

BETA, GAMMA = [0.75, 0.75, 0.5], 0.003


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Rig:
    """A flagged plan with buffers of its own: crafted regions in, the meters launch alone, the two regions out."""

    def __init__(self, shape):
        self.L = _lib.lib()
        self.plan = p = mr.crafted_plan(shape)
        assert p.has_fused_step
        Bs, Bt, T, C_ = shape
        dev = torch.device("cuda")
        self.ws = torch.zeros(p.ws_floats, device=dev)
        self.X = torch.zeros((Bs + Bt) * T * mr.FEATURE_DIM, device=dev)
        self.P = torch.zeros(p.param_floats, device=dev)
        self.G = torch.zeros(p.param_floats, device=dev)
        _lib.check(self.L.ta3n_init_workspace(p.handle, self.ws.data_ptr(), _stream()), "ta3n_init_workspace")
        self.last = self.L.ta3n_num_phases(p.handle, 4) - 1
        assert p.description["phases"][-2]["kind"] == mr.PH_TRAIN_METERS or p.description["phases"][-1]["kind"] == mr.PH_TRAIN_METERS

    def region(self, name):
        o, n = self.plan.region(name)
        return self.ws[o:o + n]

    def write(self, case):
        for name in ("Y", "Pr", "Pv", "Pf"):
            a = torch.from_numpy(np.ascontiguousarray(case[name]).reshape(-1)).cuda()
            self.region(name)[:a.numel()].copy_(a)
        self.region("labels").view(torch.int32)[:len(case["labels"])].copy_(torch.from_numpy(case["labels"]).cuda())
        self.region("losses")[:6].copy_(torch.from_numpy(case["losses"]).cuda())
        h = _lib.Hyper()
        h.valid_source, h.valid_target, h.train = case["valid_source"], case["valid_target"], 1
        _lib.check(self.L.ta3n_set_hyper(self.plan.handle, self.ws.data_ptr(), C.byref(h), _stream()), "ta3n_set_hyper")

    def launch(self):
        _lib.check(self.L.ta3n_train_step_range(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.ws.data_ptr(),
                                                self.last, 1, _stream()), "ta3n_train_step_range")

    def reset(self):
        _lib.check(self.L.ta3n_meters_reset(self.plan.handle, self.ws.data_ptr(), _stream()), "ta3n_meters_reset")

    def read(self):
        counts, sums = _lib.read_meters(self.plan, self.ws)
        return dict(counts=counts.numpy(), sums=sums.numpy())

    def others(self):
        """Every word of the workspace in front of the two meter regions (they lie behind everything else), as integers."""
        return self.ws[:self.plan.region("meter_counts")[0]].view(torch.int32).cpu()


def _same(got, want):
    assert got["counts"][:20].tolist() == want["counts"][:20].tolist()
    assert not got["counts"][20:].any()                                     # scratch and ticket are zero between launches
    assert got["sums"].tobytes() == want["sums"].tobytes()


# ---- 1. crafted regions, the meters launch alone ----
@pytest.mark.parametrize("shape,valid", mr.CRAFTED, ids=[str(s) for s, _ in mr.CRAFTED])
def test_meters_launch_alone_matches_the_reference(shape, valid):
    rig = Rig(shape)
    levels = mr.counted_levels(rig.plan)
    runs = []
    for rep in range(2):      # the same sequence twice: identical bits
        ref = mr.new_state()
        if rep:
            rig.reset()
            got = rig.read()
            assert not got["counts"].any() and not got["sums"].any()         # ta3n_meters_reset clears
        for step in range(2):      # two launches in a row accumulate
            case = mr.crafted_case(shape, valid, seed=step)
            rig.write(case)
            before = rig.others()
            rig.launch()
            assert torch.equal(rig.others(), before)                         # the launch writes only its two regions
            mr.reference_step(ref, case, levels)
            _same(rig.read(), ref)
        runs.append(rig.read())
    assert runs[0]["counts"].tolist() == runs[1]["counts"].tolist() and runs[0]["sums"].tobytes() == runs[1]["sums"].tobytes()
    c = runs[0]["counts"]
    assert c[mr.STEPS] == 2 and c[mr.ROWS] == 2 * (valid[0] if valid else shape[0]) and c[mr.LAST_ROWS] * 2 == c[mr.ROWS]
    if shape[3] < 6:
        assert c[mr.TOP5] == c[mr.ROWS]


def test_levels_the_plan_does_not_count_stay_zero():
    shape = (6, 4, 5, 12)
    rig = Rig(shape)
    only_video = mr.crafted_plan(shape, flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_TRANS_ATTN)
    assert mr.counted_levels(only_video) == [False, True, False]
    rig2 = Rig.__new__(Rig)
    rig2.__dict__.update(rig.__dict__)
    rig2.plan = only_video
    rig2.ws = torch.zeros(only_video.ws_floats, device="cuda")
    rig2.P, rig2.G = torch.zeros(only_video.param_floats, device="cuda"), torch.zeros(only_video.param_floats, device="cuda")
    _lib.check(rig2.L.ta3n_init_workspace(only_video.handle, rig2.ws.data_ptr(), _stream()), "ta3n_init_workspace")
    rig2.last = rig2.L.ta3n_num_phases(only_video.handle, 4) - 1
    case = mr.crafted_case(shape)
    rig2.write(case)
    rig2.launch()
    ref = mr.new_state()
    mr.reference_step(ref, case, [False, True, False])
    _same(rig2.read(), ref)
    assert not ref["counts"][mr.DOMAIN:mr.DOMAIN + 4].any() and ref["counts"][mr.DOMAIN + 4] == 6


# ---- 2. non-finite step ----
def test_nonfinite_total_loss_counts_the_step_and_adds_nothing():
    shape, valid = mr.CRAFTED[0]
    rig = Rig(shape)
    rig.write(mr.crafted_case(shape, valid))
    rig.launch()
    want = rig.read()
    for bad in (float("nan"), float("inf")):
        case = mr.crafted_case(shape, valid, seed=3)
        case["losses"][0] = bad
        rig.write(case)
        rig.launch()
        want["counts"][mr.STEPS] += 1
        want["counts"][mr.NONFINITE] += 1
        _same(rig.read(), want)
    assert want["counts"][mr.STEPS] == 3 and want["counts"][mr.NONFINITE] == 2


# ---- 3. reference trajectories ----
FIXTURES = ["tiny_T5", "tiny_T9", "tiny_clip", "tiny_T2", "tiny_T3"]
TIE_MARGIN = 10 * tol.LOGIT_ATOL


@functools.lru_cache(maxsize=None)
def _trajectory(name):
    """Per step of the fixture: the batch, the schedule entry, the reference's own log line, and - from the float64 oracle - the source
    rows' hit counts, with the tie guard: the label's logit is at least 10 x LOGIT_ATOL from every other class logit of its row."""
    from oracle import ta3n_oracle as orc
    g = Golden(name)
    c = case_config(g)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0)
    state = orc.TrainState(params={k: v.double() for k, v in synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"]).items()},
                           lr=c["lr"])
    lines = str(g.meta("log")).strip().splitlines()
    steps, smallest = [], float("inf")
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        state.lr = st["lr"]
        res = orc.train_step(state, xs.double(), xt.double(), ys, BETA, GAMMA, cfg, clip=c["clip"], n_src=st["n_src"], n_tgt=st["n_tgt"])
        Y = res["src"]["out"].detach().numpy()[:st["n_src"]]
        lab = ys.numpy()[:st["n_src"]]
        ranks = [mr.rank_of_label(Y[b], lab[b]) for b in range(st["n_src"])]
        for b in range(st["n_src"]):
            others = np.delete(Y[b], lab[b])
            smallest = min(smallest, float(np.abs(others - Y[b, lab[b]]).min()))
        f = lambda key, line=lines[s]: re.search(key + r" ([0-9.]+)", line).group(1)
        steps.append(dict(xs=xs, xt=xt, ys=ys, st=st, rows=st["n_src"], top1=sum(r < 1 for r in ranks), top5=sum(r < 5 for r in ranks),
                          prec1=f("Prec@1"), prec5=f("Prec@5"), loss=float(f("Loss")), loss_c=float(f("loss_c")), loss_a=float(f("loss_a")),
                          loss_e=float(f("loss_e"))))
    assert len(lines) == len(steps)
    assert smallest >= TIE_MARGIN, f"{name}: a label logit lies {smallest:.2e} from another class logit: the comparison below would not be exact"
    return c, steps


def _engine(c, **kw):
    from ta3n_amd.engine import TrainEngine
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], dropout_i=0.0, dropout_v=0.0, clip=c["clip"], train_meters=True, **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    return eng


def _close_to_log(value, logged, what):
    assert abs(value - logged) < 2e-4 * max(1, logged), f"{what}: {value} against the reference's {logged}"      # the bound of test_losses_match_reference_log


@pytest.mark.parametrize("way", ["train_step", "forward_loss_backward", "train_steps"])
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_trajectories(name, way):
    """(a) ta3n_train_step per step, (b) ta3n_forward / ta3n_loss / ta3n_backward per step, (c) TrainEngine.train_steps: ONE call over the
    steps with full batches, fed from a store, and - as train_ddp.py runs it - the short last batch of tiny_T5 as a step of its own."""
    c, steps = _trajectory(name)
    eng = _engine(c, fused=(way != "forward_loss_backward"))
    assert "training meters" in eng.describe()
    rows = top1 = top5 = 0
    loss_sums = np.zeros(6, np.float64)
    if way == "train_steps":
        from ta3n_amd.feature_store import FeatureStore
        full = [s for s in steps if (s["st"]["n_src"], s["st"]["n_tgt"]) == (c["Bs"], c["Bt"])]
        T, D = c["T"], c["D"]
        stores = [FeatureStore.from_tensors(torch.cat([s[k].reshape(-1, D) for s in full]).cuda().contiguous(),
                                            torch.full((len(full) * n,), T), lab.cuda())
                  for k, n, lab in (("xs", c["Bs"], torch.cat([s["ys"] for s in full]).to(torch.int32)),
                                    ("xt", c["Bt"], torch.zeros(len(full) * c["Bt"], dtype=torch.int32)))]
        ids = [torch.arange(len(full) * n, dtype=torch.int32, device="cuda").view(len(full), n) for n in (c["Bs"], c["Bt"])]
        eng.train_steps([(BETA, GAMMA, s["st"]["lr"]) for s in full], feeds=((stores[0], ids[0]), (stores[1], ids[1])))
        for s in steps[len(full):]:
            eng.flush()
            eng.set_batch(s["xs"].cuda(), s["xt"].cuda(), s["ys"].cuda())
            eng.train_step(BETA, GAMMA, s["st"]["lr"], valid_source=s["st"]["n_src"], valid_target=s["st"]["n_tgt"])
        eng.flush()
    for s in steps:
        rows += s["rows"]; top1 += s["top1"]; top5 += s["top5"]
        if way == "train_steps":
            continue
        st = s["st"]
        eng.set_batch(s["xs"].cuda(), s["xt"].cuda(), s["ys"].cuda())
        eng.set_hyper(BETA, GAMMA, st["lr"], train=True, valid_source=st["n_src"], valid_target=st["n_tgt"])
        before = eng.meters()["loss_sums"]
        if way == "train_step":
            eng.fused_step()
            eng.sgd_step_fused()
        else:
            eng.forward(); eng.loss(); eng.backward()
            eng.sgd_step()
        m = eng.meters()
        losses = eng.region("losses")[:6].cpu().numpy()
        loss_sums += losses.astype(np.float64)
        # per-step values: the line's .val
        assert (f"{m['prec1_last']:.3f}", f"{m['prec5_last']:.3f}") == (s["prec1"], s["prec5"])
        assert (m["counts"]["last_source_rows"], m["counts"]["last_top1"], m["counts"]["last_top5"]) == (s["rows"], s["top1"], s["top5"])
        d = {k: m["loss_sums"][k] - before[k] for k in before}
        _close_to_log(d["loss"], s["loss"], "Loss")
        _close_to_log(d["loss_c"], s["loss_c"], "loss_c")
        _close_to_log(d["loss_adv_rel"] + d["loss_adv_vid"] + d["loss_adv_frm"], s["loss_a"], "loss_a")
        _close_to_log(d["loss_e"], s["loss_e"], "loss_e")
    m = eng.meters()
    assert (m["steps"], m["nonfinite_steps"]) == (len(steps), 0)
    # window values: sum of hits / sum of valid source videos
    assert (m["counts"]["source_rows"], m["counts"]["top1"], m["counts"]["top5"]) == (rows, top1, top5)
    assert m["prec1"] == 100.0 * top1 / rows and m["prec5"] == 100.0 * top5 / rows
    last = steps[-1]
    assert (f"{m['prec1_last']:.3f}", f"{m['prec5_last']:.3f}") == (last["prec1"], last["prec5"])
    dom = m["counts"]["domain"]
    n_s, n_t = sum(s["st"]["n_src"] for s in steps), sum(s["st"]["n_tgt"] for s in steps)
    assert [dom[lv]["source"][0] for lv in ("rel", "vid", "frm")] == [n_s * (c["T"] - 1), n_s, n_s * c["T"]]
    assert [dom[lv]["target"][0] for lv in ("rel", "vid", "frm")] == [n_t * (c["T"] - 1), n_t, n_t * c["T"]]
    if way == "train_step":      # bit for bit in float64: the sum of ws["losses"] read after each step
        assert np.array([m["loss_sums"][k] for k in _lib.METER_LOSSES]).tobytes() == loss_sums.tobytes()
    elif way == "train_steps":
        _close_to_log(m["loss"], sum(s["loss"] for s in steps) / len(steps), "mean Loss")
    eng.reset_meters()
    m = eng.meters()
    assert m["steps"] == 0 and m["counts"]["source_rows"] == 0 and m["loss"] == 0.0


# ---- 4. nothing else moves ----
def _small_engine(train_meters, bf16=False, Bs=6, Bt=4, **kw):
    from ta3n_amd.engine import TrainEngine
    eng = TrainEngine(Bs, Bt, 5, 64, 32, 12, dropout_i=0.5, dropout_v=0.5, bf16=bf16, bf16_store=bf16, train_meters=train_meters, **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    return eng


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_flagged_and_unflagged_engines_leave_the_same_bits(bf16):
    xs, xt, ys, _ = synth_batch(12, 5, 64, 6, 4, seed=21)
    out = []
    for flagged in (False, True):
        eng = _small_engine(flagged, bf16)
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_steps([(BETA, GAMMA, 1e-2)] * 7)
        eng.flush()
        torch.cuda.synchronize()
        out.append(eng)
    plain, flagged = out
    n = plain.plan.ws_floats
    assert flagged.plan.region("meter_counts")[0] == n
    assert torch.equal(plain.P.view(torch.int32), flagged.P.view(torch.int32)) and torch.equal(plain.M.view(torch.int32), flagged.M.view(torch.int32))
    assert torch.equal(plain.ws.view(torch.int32), flagged.ws[:n].view(torch.int32))      # every region of the unflagged plan
    m = flagged.meters()
    assert m["steps"] == 7 and m["counts"]["source_rows"] == 42 and m["loss"] > 0
    with pytest.raises(_lib.Ta3nError, match="without train_meters"):
        plain.meters()


def test_meters_under_graph_replay():
    xs, xt, ys, _ = synth_batch(12, 5, 64, 6, 4, seed=21)
    got = []
    for graph in (False, True):
        eng = _small_engine(True)
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        if graph:
            eng.set_hyper(BETA, GAMMA, 1e-2)
            eng.capture()
            eng.reset_meters()      # (capture() runs one warm-up step and restores parameters and momentum, not the window)
        for _ in range(3):
            eng.train_step(BETA, GAMMA, 1e-2)
        got.append(eng.meter_words())
    assert got[0][0].tolist() == got[1][0].tolist() and got[0][1].numpy().tobytes() == got[1][1].numpy().tobytes()
    assert got[0][0][mr.STEPS] == 3


# ---- 5. K-step with feeds ----
def test_one_call_over_seven_steps_with_feeds_equals_seven_calls():
    from ta3n_amd.feature_store import FeatureStore
    Bs, Bt, T, D, K = 6, 4, 5, 64, 7
    gen = torch.Generator().manual_seed(5)
    nf = torch.randint(3, 12, (20,), generator=gen)
    store = FeatureStore.from_tensors(torch.randn(int(nf.sum()), D, generator=gen).cuda().contiguous(), nf.cuda(),
                                      torch.randint(0, 12, (20,), generator=gen).to(torch.int32).cuda())
    ids_s = torch.randint(0, 20, (K, Bs), generator=gen).to(torch.int32).cuda()
    ids_t = torch.randint(0, 20, (K, Bt), generator=gen).to(torch.int32).cuda()
    sched = [(BETA, GAMMA, 1e-2 / (1 + k)) for k in range(K)]
    words = []
    for single in (False, True):
        eng = _small_engine(True)
        if single:
            for k in range(K):
                eng.train_steps(sched[k:k + 1], feeds=((store, ids_s[k:k + 1]), (store, ids_t[k:k + 1])))
        else:
            eng.train_steps(sched, feeds=((store, ids_s), (store, ids_t)))
        eng.flush()
        words.append(eng.meter_words())
    assert words[0][0].tolist() == words[1][0].tolist() and words[0][1].numpy().tobytes() == words[1][1].numpy().tobytes()
    assert words[0][0][mr.STEPS] == K and words[0][0][mr.ROWS] == K * Bs and words[0][1][0] > 0


# ---- 6. two ranks sharing the GPU ----
DDP = dict(C=12, T=5, D=512, fc=128, Bs=12, Bt=8, steps=3)
# Rank-summed float64 loss sums against the single-process engine's, largest relative deviation over the six slots.  Measured on an MI355X
# with this test: 3.3e-07 (each rank adds its shard's rows in fp32 before the ranks are added: another summation order than one process
# over the whole batch, a few fp32 ulps of a sum of three steps).  Asserted with a factor of three for run-to-run summation order (the
# loss slots of the fused step are sums of per-workgroup partials).  For scale: tests/test_gpu_ddp_engine.py holds rank-summed loss
# traces to 2e-6.
DDP_LOSS_SUM_REL = 1e-6


def _ddp_engine(Bs, Bt):
    from ta3n_amd.engine import TrainEngine
    return TrainEngine(Bs, Bt, DDP["T"], DDP["D"], DDP["fc"], DDP["C"], dropout_i=0.0, dropout_v=0.0, train_meters=True)


def _ddp_run(eng, xs, xt, ys, **kw):
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=3))
    for i in range(DDP["steps"]):
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step(BETA, GAMMA, 1e-2, seed=i, **kw)
    eng.flush()
    counts, sums = eng.meter_words()
    return torch.cat((counts.to(torch.float64), sums))


def _ddp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TA3N_DDP_BUCKETS="2", TA3N_DDP_SHARDED="0")      # two buckets: the all-reduce overlaps the step's last launches
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ta3n_amd import parallel
    xs, xt, ys, _ = synth_batch(DDP["C"], DDP["T"], DDP["D"], DDP["Bs"], DDP["Bt"], seed=9)
    lo, hi = parallel.shard_range(DDP["Bs"], world, rank)
    lo_t, hi_t = parallel.shard_range(DDP["Bt"], world, rank)
    eng = _ddp_engine(hi - lo, hi_t - lo_t)
    assert eng.world == world
    words = _ddp_run(eng, xs[lo:hi], xt[lo_t:hi_t], ys[lo:hi], global_source=DDP["Bs"], global_target=DDP["Bt"])
    dist.all_reduce(words)      # what train_ddp.py's log line does with them
    if rank == 0:
        torch.save(words, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_process_meters(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "words.pt")
    mp.spawn(_ddp_worker, args=(2, port, out), nprocs=2, join=True)
    summed = torch.load(out).numpy()
    xs, xt, ys, _ = synth_batch(DDP["C"], DDP["T"], DDP["D"], DDP["Bs"], DDP["Bt"], seed=9)
    one = _ddp_run(_ddp_engine(DDP["Bs"], DDP["Bt"]), xs, xt, ys).numpy()
    want = one[:mr.WORDS].copy()
    want[mr.STEPS] *= 2      # every rank counts every step (_lib.decode_meters(world=2) divides)
    assert np.rint(summed[:mr.WORDS]).astype(np.int64).tolist() == want.astype(np.int64).tolist()      # the counts match exactly
    a, b = summed[mr.WORDS:mr.WORDS + 6], one[mr.WORDS:mr.WORDS + 6]
    rel = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))
    print(f"\n[train meters] rank-summed loss sums against the single process: largest relative deviation {rel:.3e} (sums {b.tolist()})")
    assert rel <= DDP_LOSS_SUM_REL
    m = _lib.decode_meters(np.rint(summed[:mr.WORDS]).astype(np.int64), summed[mr.WORDS:], world=2)
    m1 = _lib.decode_meters(one[:mr.WORDS].astype(np.int64), one[mr.WORDS:])
    assert m["steps"] == DDP["steps"] and m["prec1"] == m1["prec1"] and m["acc_domain"] == m1["acc_domain"]
    assert abs(m["loss"] - m1["loss"]) <= DDP_LOSS_SUM_REL * m1["loss"]
