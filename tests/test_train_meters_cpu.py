"""CPU: the training meters (TA3N_FLAG_TRAIN_METERS, include/ta3n_hip.h) - what the flag does to a plan, what ta3n_plan_create refuses with
it, the numpy statement of the launch (meters_reference.MetersInterp) against the row-by-row float64 reference on the crafted cases the
GPU test runs, the log line's formatter against the reference's own log, and the reduction of the meter words over two ranks."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import meters_reference as mr
from golden_util import Golden, case_config, step_schedule
from ta3n_amd import _lib
from ta3n_amd.synthetic import synth_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METERS = _lib.FLAG_TRAIN_METERS
ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME

# name -> (flags, Plan keywords): one plan of every family the flag is built on
PLANS = {
    "trn-m": (mr.ALL_ADV, {}),
    "trn-m-bf16-twins": (mr.ALL_ADV | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, {}),
    "avgpool-source-only": (0, dict(aggregation=_lib.AGG_AVGPOOL)),
    "avgpool-general": (ADV, dict(aggregation=_lib.AGG_AVGPOOL)),
    "rnn": (ADV, dict(aggregation=_lib.AGG_RNN, rnn_cell=1, n_ts=3)),
    "temconv": (_lib.FLAG_ADV_VIDEO, dict(aggregation=_lib.AGG_TEMCONV)),
}


def _plan(name, extra=0):
    flags, kw = PLANS[name]
    return _lib.Plan(6, 4, 5, 64, 32, 12, flags | extra, **kw)


def _kinds(plan, group):
    return [(ph["kind"], ph["task_begin"], ph["task_count"], ph["tile"]) for ph in plan.description["phases"] if ph["group"] == group]


# ---- 1. plan shape ----
@pytest.mark.parametrize("name", list(PLANS))
def test_the_flag_adds_one_launch_and_two_regions_and_moves_nothing(name):
    plain, flagged = _plan(name), _plan(name, METERS)
    last = (mr.PH_TRAIN_METERS, 0, 0, 0)
    assert _kinds(flagged, 1) == _kinds(plain, 1) + [last]
    assert _kinds(flagged, 4) == (_kinds(plain, 4) + [last] if _kinds(plain, 4) else [])
    for group in (0, 2, 3, 5):
        assert _kinds(flagged, group) == _kinds(plain, group), group
    assert flagged.params == plain.params and flagged.param_floats == plain.param_floats and flagged.live_floats == plain.live_floats
    assert set(flagged.regions) - set(plain.regions) == {"meter_counts", "meter_sums"}
    assert {k: v for k, v in flagged.regions.items() if k in plain.regions} == plain.regions
    o, n = flagged.regions["meter_counts"]
    assert o == plain.ws_floats and n == _lib.METER_WORDS                      # behind everything the plan had
    assert flagged.regions["meter_sums"] == (o + 64, 2 * _lib.METER_SUMS) and (o + 64) % 2 == 0      # float64 words, 8-byte aligned
    assert flagged.ws_floats == o + 128
    assert plain.description["n_tasks"] == flagged.description["n_tasks"] and plain.description["n_segs"] == flagged.description["n_segs"]


def test_levels_follow_the_adv_flags_and_the_rows_the_plan_has():
    assert mr.counted_levels(_plan("trn-m", METERS)) == [True, True, True]
    assert mr.counted_levels(_plan("avgpool-source-only", METERS)) == [False, False, False]
    assert mr.counted_levels(_plan("avgpool-general", METERS)) == [False, True, True]      # no relation rows outside trn-m
    assert mr.counted_levels(_plan("temconv", METERS)) == [False, True, False]
    assert mr.counted_levels(_lib.Plan(6, 4, 5, 64, 32, 12, _lib.FLAG_ADV_VIDEO | METERS)) == [False, True, False]


def test_the_launch_kind_is_the_next_number_and_the_subclass_runs_it():
    """PH_TRAIN_METERS is the last entry of PhaseKind, number 23 (the entries before it are numbered 0..22 in order), and the interpreter of
    meters_reference runs exactly the base interpreter's kinds and this one."""
    import plan_interp
    header = os.path.join(ROOT, "ta3n_amd", "csrc", "ta3n_types.h")
    body = re.search(r"enum PhaseKind : int32_t \{(.*?)\};", open(header).read(), re.S).group(1)
    names = re.findall(r"^\s*(PH_\w+)\b[^,\n]*,", body, re.M)
    assert names[-1] == "PH_TRAIN_METERS" and len(names) == 24 and names.index("PH_TRAIN_METERS") == mr.PH_TRAIN_METERS == 23
    numbered = {name: int(v) for name, v in re.findall(r"^\s*(PH_\w+) = (\d+),", body, re.M)}
    assert [numbered[n] for n in names[:-1]] == list(range(23))
    assert set(mr.MetersInterp.LAUNCH) == set(plan_interp.Interp.LAUNCH) | {23} and 23 not in plan_interp.Interp.LAUNCH
    assert "static_assert(PH_TRAIN_METERS == 23" in open(header).read()


# ---- 2. refusals ----
def test_refusals_name_what_is_refused():
    with pytest.raises(ValueError, match="TA3N_FLAG_TRAIN_METERS with TA3N_FLAG_SCORE_ONLY is not built"):
        _lib.Plan(6, 4, 5, 64, 32, 12, mr.ALL_ADV | METERS | _lib.FLAG_SCORE_ONLY)
    with pytest.raises(ValueError, match="TA3N_FLAG_TRAIN_METERS with chain is not built"):
        _lib.Plan(6, 4, 5, 64, 32, 12, mr.ALL_ADV | METERS, chain=1)
    from ta3n_amd import options
    kind, text = options.refusal("train_meters", dict(chain_arg=True))
    assert kind is NotImplementedError and text.startswith("train_meters together with chained launches (chain) is not built")
    assert options.refusal("train_meters", dict(chain=True, chain_arg=False)) == (None, "")      # TA3N_CHAIN=1 is a default the engine drops
    assert options.refusal("train_meters", {}) == (None, "")


def test_the_reset_is_declared_and_exported():
    assert "ta3n_meters_reset" in _lib.SYMBOLS and hasattr(_lib.lib(), "ta3n_meters_reset")
    plan = _plan("trn-m")
    assert _lib.lib().ta3n_meters_reset(plan.handle, 16, None) == -1      # a plan without the flag: refused before anything is touched
    assert "TA3N_FLAG_TRAIN_METERS" in _lib.lib().ta3n_last_error().decode()


# ---- 3. the numpy statement of the launch against the row-by-row reference ----
def _assert_same(a, b):
    assert a["counts"].tolist() == b["counts"].tolist()
    assert a["sums"].tobytes() == b["sums"].tobytes()


@pytest.mark.parametrize("shape,valid", mr.CRAFTED, ids=[str(s) for s, _ in mr.CRAFTED])
def test_interpreter_matches_reference_on_the_crafted_cases(shape, valid):
    plan = mr.crafted_plan(shape)
    it, ref = mr.MetersInterp(plan), mr.new_state()
    assert it.levels == [shape[2] > 1, True, True]
    for step in range(2):      # two launches in a row accumulate
        case = mr.crafted_case(shape, valid, seed=step)
        mr.load_case(it, case)
        it.run_group(1) if step else mr.MetersInterp.LAUNCH[mr.PH_TRAIN_METERS](it, None, False)      # (the loss list ends with the launch)
        if step:      # run_group(1) ran the loss kernel first, on the crafted logits: the launch read ITS losses
            case = dict(case, losses=it.ws[it.g.o_losses:it.g.o_losses + 6].copy())
        mr.reference_step(ref, case, it.levels)
        _assert_same(it.meters, ref)
    c = ref["counts"]
    assert c[mr.STEPS] == 2 and c[mr.NONFINITE] == 0
    assert c[mr.ROWS] == 2 * (valid[0] if valid else shape[0])
    if shape[3] < 6:
        assert c[mr.TOP5] == c[mr.ROWS]                                        # fewer than six classes: every row is a top-5 hit
    if shape[3] == 1:
        assert c[mr.TOP1] == c[mr.ROWS]
    n_s, n_t = valid if valid else shape[:2]
    for l in range(3):
        per = mr.rows_per_video(l, shape[2])
        assert (c[mr.DOMAIN + 4 * l], c[mr.DOMAIN + 4 * l + 2]) == (2 * n_s * per, 2 * n_t * per)


def test_tie_rules_and_dummy_rows():
    y = np.full(12, -3.0, np.float32)
    y[:5] = 1.5
    assert mr.rank_of_label(y, 4) == 4                     # tied with four lower-index classes: rank 4, a top-5 hit
    y[:6] = 1.5
    assert mr.rank_of_label(y, 5) == 5                     # with five: a miss
    assert mr.rank_of_label(y, 0) == 0                     # with higher-index classes only: top-1
    shape, valid = mr.CRAFTED[0]
    case = mr.crafted_case(shape, valid)
    assert [mr.rank_of_label(case["Y"][b], case["labels"][b]) for b in range(3)] == [4, 5, 0]
    st = mr.new_state()
    mr.reference_step(st, case, [True, True, True])
    full = mr.new_state()
    mr.reference_step(full, dict(case, valid_source=shape[0], valid_target=shape[1]), [True, True, True])
    c, f = st["counts"], full["counts"]
    assert f[mr.ROWS] - c[mr.ROWS] == 1 and f[mr.TOP1] - c[mr.TOP1] == 1      # the dummy row would have been a hit
    for l in range(3):
        per = mr.rows_per_video(l, shape[2])
        for d in (0, 2):
            assert f[mr.DOMAIN + 4 * l + d] - c[mr.DOMAIN + 4 * l + d] == per == f[mr.DOMAIN + 4 * l + d + 1] - c[mr.DOMAIN + 4 * l + d + 1]
    tie = dict(case, Pv=np.zeros_like(case["Pv"]))         # equal domain logits predict source
    st = mr.new_state()
    mr.reference_step(st, tie, [False, True, False])
    assert st["counts"][mr.DOMAIN + 4: mr.DOMAIN + 8].tolist() == [5, 5, 3, 0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_step_counts_and_adds_nothing(bad):
    shape, valid = mr.CRAFTED[0]
    it = mr.MetersInterp(mr.crafted_plan(shape))
    mr.load_case(it, mr.crafted_case(shape, valid))
    it.run_train_meters()
    before = {k: v.copy() for k, v in it.meters.items()}
    case = mr.crafted_case(shape, valid, seed=1)
    case["losses"][0] = bad
    mr.load_case(it, case)
    it.run_train_meters()
    want = before["counts"].copy()
    want[mr.STEPS] += 1; want[mr.NONFINITE] += 1
    assert it.meters["counts"].tolist() == want.tolist() and it.meters["sums"].tobytes() == before["sums"].tobytes()
    ref = mr.new_state()
    mr.reference_step(ref, case, it.levels)
    assert ref["counts"].tolist()[:2] == [1, 1] and not ref["counts"][2:].any() and not ref["sums"].any()


def test_flagged_lists_run_end_to_end_in_the_interpreter():
    """A flagged trn-m plan's forward / loss lists and its fused list on the CPU: both leave the same meters, which are the reference's on
    the logits the lists computed."""
    from ta3n_amd.synthetic import synth_state
    Bs, Bt, T, D, C = 6, 4, 5, 64, 12
    plan = _lib.Plan(Bs, Bt, T, D, 32, C, mr.ALL_ADV | METERS)
    state = synth_state({n: s for n, _, s, _ in plan.params}, seed=3)
    xs, xt, ys, _ = synth_batch(C, T, D, Bs, Bt, seed=5)
    got = []
    for groups in ((0, 1), (4,)):
        it = mr.MetersInterp(plan)
        it.set_params(state)
        it.X = torch.cat((xs.reshape(-1), xt.reshape(-1))).double().numpy()
        it.labels[:Bs] = ys.numpy()
        it.hy = dict(beta=[0.75, 0.75, 0.5], gamma=0.003, p_drop_i=0.0, p_drop_v=0.0, seed_i=1, seed_v=2, train=1, inv_n_cls=1 / 5, inv_n_rel=1 / (8 * (T - 1)),
                     inv_n_vid=1 / 8, inv_n_frm=1 / (8 * T), inv_n_ent=1 / 8, valid_source=5, valid_target=3, lr=1e-3, momentum=0.9, weight_decay=1e-4,
                     clip=20.0)
        for group in groups:
            it.run_group(group)
        g = it.g
        case = dict(Bs=Bs, Bt=Bt, T=T, C=C, valid_source=5, valid_target=3, labels=it.labels, losses=it.ws[g.o_losses:g.o_losses + 6],
                    Y=it.r(g.o_Y, (g.B, C)), Pr=it.r(g.o_Pr, (g.B * (T - 1), 2)), Pv=it.r(g.o_Pv, (g.B, 2)), Pf=it.r(g.o_Pf, (g.B * T, 2)))
        ref = mr.new_state()
        mr.reference_step(ref, case, it.levels)
        _assert_same(it.meters, ref)
        assert ref["counts"][mr.ROWS] == 5 and ref["sums"][0] > 0
        got.append(it.meters)
    assert got[0]["counts"].tolist() == got[1]["counts"].tolist()
    np.testing.assert_allclose(got[0]["sums"], got[1]["sums"], rtol=1e-9)


# ---- 4. the formatter against the reference's own log ----
def _tiny_T5_step0():
    """The reference's own step-0 logits of tiny_T5 (the fixture's fwd/ records), its labels and the losses its log printed."""
    g = Golden("tiny_T5")
    c = case_config(g)
    st = step_schedule(c)[0]
    _, _, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    z = lambda k: np.concatenate((g.z[f"fwd/{k.format('s')}#full"], g.z[f"fwd/{k.format('t')}#full"])).astype(np.float32)
    line = str(g.meta("log")).splitlines()[0]
    f = lambda name: float(re.search(name + r" ([0-9.]+)", line).group(1))
    labels = np.zeros(c["Bs"] + c["Bt"], np.int32)
    labels[:c["Bs"]] = ys.numpy()
    losses = np.array([f("Loss"), f("loss_c"), f("loss_a"), 0.0, 0.0, f("loss_e")], np.float32)
    case = dict(Bs=c["Bs"], Bt=c["Bt"], T=c["T"], C=c["C"], valid_source=st["n_src"], valid_target=st["n_tgt"], labels=labels, losses=losses,
                Y=z("out_{}"), Pr=z("pd_{}_rel").reshape(-1, 2), Pv=z("pd_{}_vid").reshape(-1, 2), Pf=z("pd_{}_frm").reshape(-1, 2))
    return case, line


def test_formatter_reproduces_the_reference_log_line():
    sys.path.insert(0, ROOT)
    import train_ddp
    case, line = _tiny_T5_step0()
    st = mr.new_state()
    mr.reference_step(st, case, [True, True, True])
    m = _lib.decode_meters(st["counts"], st["sums"])
    text = train_ddp.format_train_meters(m, float(case["losses"][0]))
    want = "Prec@1 0.000 (0.000)\tPrec@5 66.667 (66.667)\tLoss 6.5031 (6.5031)   loss_c 3.5068"
    assert want in line and text.startswith(want + "\tloss_a 2.9905\tloss_e 1.9223\tacc_d rel ")
    assert re.search(r"acc_d rel [0-9.]+/[0-9.]+ vid [0-9.]+/[0-9.]+ frm [0-9.]+/[0-9.]+$", text)      # no `nonfinite` field without one
    assert train_ddp.format_train_meters(m, 6.5031, show_a=False, show_e=False).startswith(want + "\tacc_d rel ")
    st["counts"][mr.STEPS] += 2; st["counts"][mr.NONFINITE] += 2      # non-finite steps do not dilute the means
    m2 = _lib.decode_meters(st["counts"], st["sums"])
    assert m2["loss"] == m["loss"] and train_ddp.format_train_meters(m2, 6.5031).endswith("\tnonfinite 2")
    assert m["steps"] == 1 and m["counts"]["source_rows"] == 6 and m["counts"]["top5"] == 4 and set(m["acc_domain"]) == {"rel", "vid", "frm"}


# ---- 5. two ranks: the summed meter words of two half batches are the whole batch's ----
def _rank_main(rank, port, halves, out):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    st = mr.new_state()
    mr.reference_step(st, halves[rank], [True, True, True])
    # what train_ddp.py's log line reduces: the counts and the float64 sums in ONE float64 all-reduce
    words = torch.cat((torch.from_numpy(st["counts"]).to(torch.float64), torch.from_numpy(st["sums"])))
    dist.all_reduce(words)
    if rank == 0:
        torch.save(words, out)
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_whole_batch(tmp_path):
    import socket
    import torch.multiprocessing as mp
    shape = (6, 4, 5, 12)
    whole = mr.crafted_case(shape)
    Bs, Bt, T, _ = shape

    def half(r):      # rank r's contiguous shard of every half; its loss slots are its share of the job's
        s, t = slice(r * Bs // 2, (r + 1) * Bs // 2), slice(Bs + r * Bt // 2, Bs + (r + 1) * Bt // 2)
        rows = lambda P, per: np.concatenate((P[s.start * per:s.stop * per], P[t.start * per:t.stop * per]))
        share = (whole["losses"] * np.float32(0.25 + 0.5 * r)).astype(np.float32)
        return dict(Bs=Bs // 2, Bt=Bt // 2, T=T, C=shape[3], valid_source=Bs // 2, valid_target=Bt // 2, losses=share,
                    Y=np.concatenate((whole["Y"][s], whole["Y"][t])), labels=np.concatenate((whole["labels"][s], whole["labels"][t])),
                    Pr=rows(whole["Pr"], T - 1), Pv=rows(whole["Pv"], 1), Pf=rows(whole["Pf"], T))
    halves = [half(0), half(1)]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "words.pt")
    mp.spawn(_rank_main, args=(port, halves, out), nprocs=2, join=True)
    words = torch.load(out).numpy()
    ref = mr.new_state()
    mr.reference_step(ref, whole, [True, True, True])
    counts = np.rint(words[:mr.WORDS]).astype(np.int64)
    want = ref["counts"].copy()
    want[mr.STEPS] = 2      # (every rank counts its step; decode_meters(world=2) gives the job's one step back)
    assert counts.tolist() == want.tolist()
    m, m_whole = _lib.decode_meters(counts, words[mr.WORDS:], world=2), _lib.decode_meters(ref["counts"], ref["sums"])
    assert m["steps"] == 1 and m["nonfinite_steps"] == 0
    for key in ("prec1", "prec5", "prec1_last", "prec5_last", "acc_domain", "counts"):
        assert m[key] == m_whole[key], key
    assert abs(m["loss"] - m_whole["loss"]) <= 1e-6 * m_whole["loss"]
    sums = halves[0]["losses"].astype(np.float64) + halves[1]["losses"].astype(np.float64)
    assert words[mr.WORDS:mr.WORDS + 6].tobytes() == sums.tobytes()
    np.testing.assert_allclose(words[mr.WORDS:mr.WORDS + 6], whole["losses"].astype(np.float64), rtol=1e-6)
