"""--share_params N (models.py:174-192, 296-305, 565-566, 686-687: the target rows' own first frame layer and video classifier) on the
CPU: the flagged plans executed with numpy (tests/plan_interp.py, unchanged: no phase kind is new) against fixtures the reference
produced (tests/golden/make_golden_unshared.py), the live parameter set, the five specs that are cut at the domain boundary, the
plans without the flag left as they were, and the option handling at the plan, TrainEngine, VideoModel, train_ddp.py and main.py
levels."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from plan_interp import Interp, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import flags_from_options, share_params_refusal
from ta3n_amd.synthetic import synth_batch, synth_state
from test_plan_cpu import make_hyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SP_CASES = ["tiny_sp_T5", "tiny_sp_T2", "tiny_sp_odd", "tiny_sp_one", "tiny_sp_noent", "tiny_sp_sv", "mid_sp"]
R, V, Fr, E, A = (_lib.FLAG_ADV_RELATION, _lib.FLAG_ADV_VIDEO, _lib.FLAG_ADV_FRAME, _lib.FLAG_ATTN_ENTROPY, _lib.FLAG_TRANS_ATTN)
U = _lib.FLAG_UNSHARED
SP = R | V | Fr | E | A | U
TW = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
TINY = dict(Bs=6, Bt=4, T=5, D=512, fc_dim=64, C=12)
LIVE_CAPABLE = ["fc_feature_shared_target", "fc_classifier_video_target"]
NEVER_LIVE = ["fc_feature_target", "fc_classifier_target", "fc_feature_video_target", "fc_feature_video_target_2"]
BASE_X, BASE_P, BASE_G, BASE_WS = 0, 1, 2, 3


def sp_flags(g, c):
    return flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), c["add_loss_DA"] or "attentive_entropy", "TransAttn", "RevGrad",
                              str(g.meta("use_target"))) | U


def _plan(c, flags, **kw):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags, **kw)


def _load_step(it, g, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:c["Bs"]] = ys.numpy()
    it.labels[c["Bs"]:] = yt.numpy()
    it.hy = make_hyper(c, st, c["T"], st["lr"])
    if str(g.meta("use_target")) == "Sv":
        it.hy["inv_n_cls"] = 1.0 / (st["n_src"] + st["n_tgt"])
    it.G[:] = 0


@pytest.mark.parametrize("name", SP_CASES)
def test_plan_reproduces_reference(name):
    """ta3n_forward / ta3n_loss / ta3n_backward / ta3n_sgd_step of the flagged plan against the reference's run of the same command:
    forward tensors, every clipped gradient and every parameter after every step (the last step of the tiny_sp_T5 family with padded
    videos in both halves), with the bounds tests/test_plan_cpu.py uses for the plain lists."""
    g = Golden(name)
    assert str(g.meta("share_params")) == "N"
    c = case_config(g)
    T = c["T"]
    plan = _plan(c, sp_flags(g, c))
    assert not plan.has_fused_step and _lib.lib().ta3n_has_pipelined_step(plan.handle) == 0
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    for s, st in enumerate(step_schedule(c)):
        _load_step(it, g, c, st)
        it.run_group(0)
        if s == 0:
            B, Bs = c["Bs"] + c["Bt"], c["Bs"]
            geo = it.g
            outs = dict(out=it.r(geo.o_Y, (B, c["C"])), attn=it.r(geo.o_attn, (B, T - 1)),
                        rel=it.r(geo.o_Pr, (B, T - 1, 2)), vid=it.r(geo.o_Pv, (B, 2)), frm=it.r(geo.o_Pf, (B, T, 2)),
                        v=it.r(geo.o_V, (B, 256)), f1=it.r(geo.o_F1, (B, T, geo.F)))
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", outs["out"][sl], 5e-5, 2e-5)
                g.check(f"fwd/attn_{dom}", outs["attn"][sl], 5e-5, 2e-5)
                for nm in ("rel", "vid", "frm"):
                    g.check(f"fwd/pd_{dom}_{nm}", outs[nm][sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_v", outs["v"][sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_f1", outs["f1"][sl], 5e-5, 2e-5)
        it.run_group(1)
        it.run_group(2)
        raw = it.get_params(it.G)
        it.run_group(3)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", new[k], 1e-4, 2e-5)


@pytest.mark.parametrize("name", SP_CASES)
def test_live_set_and_state_keys_are_the_references(name):
    """The plan's live set is the reference's (parameters with a gradient after its steps); the four never-live target layers sit
    behind the live prefix, the two live-capable ones inside it exactly when they are live; VideoModel's state_dict has the reference's
    keys in the reference's order."""
    g = Golden(name)
    c = case_config(g)
    plan = _plan(c, sp_flags(g, c))
    ref_live = set(str(k) for k in g.meta("live"))
    assert {n for n, _, _, lv in plan.params if lv} == ref_live
    assert "fc_feature_shared_target.weight" in ref_live
    assert ("fc_classifier_video_target.weight" in ref_live) == (name != "tiny_sp_noent")
    for n, off, shape, lv in plan.params:
        assert lv == (off < plan.live_floats), n
        if n.rsplit(".", 1)[0] in NEVER_LIVE:
            assert not lv, n
    keys = [str(k) for k in g.meta("state_keys")]
    shapes = {n: tuple(s) for n, _, s, _ in plan.params}
    assert set(shapes) == {k for k in keys if "running_" not in k and "num_batches" not in k}
    from ta3n_amd.models import VideoModel
    m = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   verbose=False, share_params="N")
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert {k: tuple(v.shape) for k, v in sd.items() if k in shapes} == shapes
    plain = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18",
                       fc_dim=c["fc_dim"], verbose=False)
    assert len(sd) == len(plain.state_dict()) + 12
    for layer in LIVE_CAPABLE + NEVER_LIVE:      # initialised like their source twins: normal(0, 0.001), zero bias
        w, b = sd[layer + ".weight"], sd[layer + ".bias"]
        assert float(b.abs().max()) == 0 and 0.0005 < float(w.std()) < 0.002, layer


@pytest.mark.parametrize("flags,live", [
    (A | U, set()),                                                      # use_target none: no loss reads a target row
    (V | Fr | A | U, {"fc_feature_shared_target"}),                      # an adversarial level alone
    (Fr | U, {"fc_feature_shared_target"}),
    (A | U | _lib.FLAG_TARGET_ENTROPY, set(LIVE_CAPABLE)),               # each of the three that read the target class logits
    (A | U | _lib.FLAG_TARGET_LABELS, set(LIVE_CAPABLE)),
    (R | V | Fr | E | A | U, set(LIVE_CAPABLE)),
    (R | V | Fr | A | U | _lib.FLAG_FEATURE_GRADS, set(LIVE_CAPABLE))])  # the module path: the caller assembles the loss
def test_live_rule(flags, live):
    plan = _plan(TINY, flags)
    got = {n.rsplit(".", 1)[0] for n, _, _, lv in plan.params if lv and "_target" in n}
    assert got == live
    assert all(not lv for n, _, _, lv in plan.params if n.rsplit(".", 1)[0] in NEVER_LIVE)
    assert sum(1 for n, _, _, _ in plan.params if "_target" in n) == 12


# ---- the five specs that are cut at the domain boundary ----
def _gemm_phases(phases, groups=(0, 2)):
    return [i for i, ph in enumerate(phases) if ph.kind == 0 and ph.group in groups]


def _tasks_of(tasks, ph):
    return [tasks[k] for k in range(ph.task_begin, ph.task_begin + ph.task_count) if tasks[k].seg_count > 0]


def _rows(off, ld, first, n):
    """global (row of the region's first element = 0) range [lo, hi) of n rows behind element offset `off`"""
    assert off % ld == 0
    return off // ld + first, off // ld + first + n


@pytest.mark.parametrize("c", [TINY, dict(Bs=3, Bt=2, T=2, D=512, fc_dim=32, C=5), dict(Bs=5, Bt=4, T=4, D=512, fc_dim=20, C=6),
                               dict(Bs=1, Bt=1, T=3, D=512, fc_dim=32, C=5), dict(Bs=40, Bt=24, T=5, D=512, fc_dim=128, C=12),
                               dict(Bs=128, Bt=74, T=5, D=2048, fc_dim=512, C=12)],
                         ids=["tiny_T5", "tiny_T2", "odd", "one", "mid", "headline"])
@pytest.mark.parametrize("arith", [0, TW], ids=["fp32", "twins"])
def test_split_specs_sit_in_their_parents_launch_and_stay_on_their_side(c, arith):
    """F1, Y, gVt, dWcv / dbcv and dWsh / dbsh appear as a source and a target spec, each pair in the launch the whole spec sits in
    in the plain lists; no task of a source spec reads or writes a row >= Bs T (a video >= Bs), no task of a target spec one below."""
    plan, plain = _plan(c, SP | arith), _plan(c, (SP & ~U) | arith)
    segs, tasks, phases, geo, _, _ = plan_arrays(plan)
    psegs, ptasks, pphases, pgeo, _, _ = plan_arrays(plain)
    assert [(ph.kind, ph.group) for ph in phases] == [(ph.kind, ph.group) for ph in pphases if ph.group < 4]      # launch for launch
    Bs, Bt, T, D, F, C, NB = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], 256
    poff = {n: (off, int(np.prod(s))) for n, off, s, _ in plan.params}
    ppoff = {n: (off, int(np.prod(s))) for n, off, s, _ in plain.params}
    twin_launch = lambda ph: bool(ph.bf16 & 16)      # noqa: E731

    def where(the_tasks, the_phases, pred):
        hit = [k for k, i in enumerate(_gemm_phases(the_phases)) if any(pred(t) for t in _tasks_of(the_tasks, the_phases[i]))]
        assert len(hit) == 1, hit
        return hit[0]

    def ws_out(reg_plan, name):
        lo, n = reg_plan.region(name)
        return lambda t: t.c_base == BASE_WS and lo <= t.c_off < lo + n

    def grad_out(table, name):
        lo, n = table[name]
        return lambda t: t.c_base == BASE_G and lo <= t.c_off < lo + n

    def sides(pred, split_at, unit):
        """tasks matching pred, as (source tasks, target tasks) by the first row of their output"""
        lo = None
        src, tgt = [], []
        for i in _gemm_phases(phases):
            for t in _tasks_of(tasks, phases[i]):
                if pred(t):
                    (src if t.c_off < split_at else tgt).append((phases[i], t))
        assert src and tgt
        return src, tgt

    def a_rows(ph, t, region_off, ld):
        """[lo, hi) rows of the workspace / input region the task's A operands cover (K-contiguous operand: rows m0 ..; its twin likewise)"""
        out = []
        for s in segs[t.seg_begin:t.seg_begin + t.seg_count]:
            if s.a_kmajor:
                continue
            off = s.a_off
            if twin_launch(ph):
                off = (off - (geo.o_x16 if off >= geo.o_x16 else geo.o_ws16)) * 2
            if region_off <= off < region_off + (Bs + Bt) * T * max(D, F, NB) and s.a_ld == ld:
                out.append(_rows(off - region_off, ld, 0, t.m_valid))
        return out

    # F1: output rows and input rows
    f1 = plan.region("F1")[0]
    assert where(tasks, phases, ws_out(plan, "F1")) == where(ptasks, pphases, ws_out(plain, "F1")) == 0
    src, tgt = sides(ws_out(plan, "F1"), f1 + Bs * T * F, F)
    for (ph, t) in src:
        assert _rows(t.c_off - f1, F, 0, t.m_valid) == (0, Bs * T) and t.pad2 == 0 and t.drop_ld == F
        assert a_rows(ph, t, 0, D) == [(0, Bs * T)]
    for (ph, t) in tgt:
        assert _rows(t.c_off - f1, F, 0, t.m_valid) == (Bs * T, (Bs + Bt) * T)
        assert t.pad2 == Bs * T * F and t.drop_ld == F      # the dropout element id stays the GLOBAL row * F + n
        assert a_rows(ph, t, 0, D) == [(Bs * T, (Bs + Bt) * T)]
    bias = lambda pairs: {t.bias_off for _, t in pairs}      # noqa: E731
    assert bias(src) == {poff["fc_feature_shared_source.bias"][0]} and bias(tgt) == {poff["fc_feature_shared_target.bias"][0]}
    # Y
    y = plan.region("Y")[0]
    assert where(tasks, phases, ws_out(plan, "Y")) == where(ptasks, pphases, ws_out(plain, "Y"))
    src, tgt = sides(ws_out(plan, "Y"), y + Bs * C, C)
    vd = plan.region("Vd")[0]
    for (ph, t) in src:
        assert _rows(t.c_off - y, C, 0, t.m_valid) == (0, Bs) and a_rows(ph, t, vd, NB) == [(0, Bs)]
    for (ph, t) in tgt:
        assert _rows(t.c_off - y, C, 0, t.m_valid) == (Bs, Bs + Bt) and a_rows(ph, t, vd, NB) == [(Bs, Bs + Bt)]
    assert bias(src) == {poff["fc_classifier_video_source.bias"][0]} and bias(tgt) == {poff["fc_classifier_video_target.bias"][0]}
    # gVt: both K segments of each side on that side's videos; the shared -beta1 gHv Wdv segment in both
    gv = plan.region("gVt")[0]
    assert where(tasks, phases, ws_out(plan, "gVt")) == where(ptasks, pphases, ws_out(plain, "gVt"))
    src, tgt = sides(ws_out(plan, "gVt"), gv + Bs * NB, NB)
    ghv, gy = plan.region("gHv")[0], plan.region("gY")[0]
    for pairs, lo, hi, wcv in ((src, 0, Bs, "fc_classifier_video_source.weight"), (tgt, Bs, Bs + Bt, "fc_classifier_video_target.weight")):
        for (ph, t) in pairs:
            assert not twin_launch(ph) or C % 8 == 0
            assert _rows(t.c_off - gv, NB, 0, t.m_valid) == (lo, hi) and t.seg_count == 2
            s0, s1 = segs[t.seg_begin], segs[t.seg_begin + 1]
            if not twin_launch(ph):
                assert _rows(s0.a_off - ghv, NB, 0, t.m_valid) == (lo, hi) and s0.scale_kind == 2 and s0.b_off == poff["fc_feature_domain_video.weight"][0]
                assert _rows(s1.a_off - gy, C, 0, t.m_valid) == (lo, hi) and s1.b_off == poff[wcv][0]
            assert t.pad2 == lo * NB and t.drop_ld == NB and t.alpha_kind == 6      # global dropout_v index; SK_REVERSE_MU
    # dWcv / dbcv and dWsh / dbsh: K over the side's rows
    for name, tname, parent, g_reg, g_ld, x_base, x_reg, x_ld, lo_t, n_s, n_t in (
            ("fc_classifier_video_source.weight", "fc_classifier_video_target.weight", "fc_classifier_video_source.weight", "gY", C, BASE_WS, vd, NB, Bs, Bs, Bt),
            ("fc_feature_shared_source.weight", "fc_feature_shared_target.weight", "fc_feature_shared_source.weight", "gZ1", F, BASE_X, 0, D, Bs * T, Bs * T, Bt * T)):
        at = where(tasks, phases, grad_out(poff, name))
        assert at == where(tasks, phases, grad_out(poff, tname)) == where(ptasks, pphases, grad_out(ppoff, parent))
        ph = phases[_gemm_phases(phases)[at]]
        g0 = plan.region(g_reg)[0]
        for which, lo, n in ((name, 0, n_s), (tname, lo_t, n_t)):
            mine = [t for t in _tasks_of(tasks, ph) if grad_out(poff, which)(t)]
            assert mine
            for t in mine:
                assert t.seg_count == 1
                s = segs[t.seg_begin]
                assert s.klen == n and s.a_kmajor and s.b_kmajor
                a_off, b_off = s.a_off, s.b_off
                if twin_launch(ph):
                    a_off = (a_off - geo.o_ws16) * 2
                    b_off = (b_off - (geo.o_x16 if x_base == BASE_X else geo.o_ws16)) * 2
                assert _rows(a_off - g0, g_ld, 0, s.klen) == (lo, lo + n)
                assert _rows(b_off - x_reg, x_ld, 0, s.klen) == (lo, lo + n)
            assert {t.bias_off for t in mine if t.epi & 256} == {poff[which.replace(".weight", ".bias")][0]}      # EPI_ROWSUM_A: the bias gradient


def test_a_dead_target_layer_gets_no_weight_gradient_spec():
    """A spec whose destination is not live is not emitted: use_target none drops both, no loss on the target logits drops dWcv_t."""
    for flags, dead in ((A | U, LIVE_CAPABLE), (R | V | Fr | A | U, ["fc_classifier_video_target"])):
        plan = _plan(TINY, flags)
        _, tasks, _, _, _, _ = plan_arrays(plan)
        for layer in dead:
            for leaf in ("weight", "bias"):
                off, n = next((o, int(np.prod(s))) for nm, o, s, _ in plan.params if nm == f"{layer}.{leaf}")
                assert not any(t.seg_count and ((t.c_base == BASE_G and off <= t.c_off < off + n) or
                                                (t.epi & 256 and t.bias_base == BASE_G and off <= t.bias_off < off + n)) for t in tasks), layer


def test_no_launch_loses_its_twin_reads():
    """bf16 + bf16_store: every GEMM launch of the flagged lists reads twins exactly where the plain unfused lists do."""
    for c in (TINY, dict(TINY, fc_dim=20), dict(TINY, C=16), dict(Bs=40, Bt=24, T=5, D=512, fc_dim=128, C=12), dict(Bs=5, Bt=3, T=5, D=512, fc_dim=64, C=8)):
        mine, plain = _plan(c, SP | TW), _plan(c, (SP & ~U) | TW)      # (kept alive: plan_arrays returns views)
        ours = [bool(ph.bf16 & 16) for ph in plan_arrays(mine)[2] if ph.group in (0, 2) and ph.kind == 0]
        theirs = [bool(ph.bf16 & 16) for ph in plan_arrays(plain)[2] if ph.group in (0, 2) and ph.kind == 0]
        assert ours == theirs and (any(ours) or c["fc_dim"] == 20), c


@pytest.mark.parametrize("store", [False, True])
def test_bf16_plan_on_cpu(store):
    """The flagged lists with bf16 operands (rounded in registers, or read from twins) stay within the bf16 distance of the fp32
    reference that tests/test_plan_cpu.py allows the plain lists (class logits within 0.1 rms)."""
    g = Golden("tiny_sp_T5")
    c = case_config(g)
    plan = _plan(c, sp_flags(g, c) | _lib.FLAG_BF16_MFMA | (_lib.FLAG_BF16_STORE if store else 0))
    it = Interp(plan)
    it.set_params(synth_state({n: s for n, _, s, _ in plan.params}, seed=c["wseed"], scale=c["wscale"]))
    _load_step(it, g, c, step_schedule(c)[0])
    it.run_group(0)
    out = it.r(it.g.o_Y, (c["Bs"] + c["Bt"], c["C"]))
    for dom, sl in (("s", slice(0, c["Bs"])), ("t", slice(c["Bs"], c["Bs"] + c["Bt"]))):
        g.check(f"fwd/out_{dom}", out[sl], 0.0, 0.1 * g.rms(f"fwd/out_{dom}"), "bf16 operands vs fp32 reference")


def test_dropout_masks_stay_keyed_by_the_global_row():
    """dropout_i = 0.5 on the flagged plan: F1 equals its dropout-free value times the mask at the GLOBAL element index
    (tests/plan_interp.keep_mask), for source and target rows alike, exactly (the gradient at the pooled video feature: Task.pad2 in
    test_split_specs_sit_in_their_parents_launch_and_stay_on_their_side)."""
    from plan_interp import keep_mask
    g = Golden("mid_sp")
    c = case_config(g)
    plan = _plan(c, sp_flags(g, c))
    res = []
    for p in (0.0, 0.5):
        it = Interp(plan)
        it.set_params(synth_state({n: s for n, _, s, _ in plan.params}, seed=c["wseed"], scale=c["wscale"]))
        _load_step(it, g, c, step_schedule(c)[0])
        it.hy.update(p_drop_i=p, p_drop_v=p, seed_i=11, seed_v=12)
        it.run_group(0)
        res.append(it.r(it.g.o_F1, ((c["Bs"] + c["Bt"]) * c["T"], it.g.F)).copy())
    BT, F = res[0].shape
    mask = keep_mask(11, np.arange(BT)[:, None] * F + np.arange(F)[None, :], 0.5)
    assert 0.4 < mask[c["Bs"] * c["T"]:].mean() < 0.6
    assert np.array_equal(res[1], res[0] * mask * 2.0)
    restart = keep_mask(11, np.arange(c["Bt"] * c["T"])[:, None] * F + np.arange(F)[None, :], 0.5)      # what a mask that restarts at row 0 would be
    assert not np.array_equal(restart, mask[c["Bs"] * c["T"]:])


@pytest.mark.parametrize("flags", [R | V | Fr | E | A, R | V | Fr | E | A | TW, R | V | Fr | E | A | _lib.FLAG_FEATURE_GRADS, V | Fr,
                                   R | V | Fr | E | A | _lib.FLAG_FRAME_ATTN, R | V | Fr | E | _lib.FLAG_GENERAL_ATTN])
def test_plans_without_the_flag_have_none_of_it(flags):
    plan = _plan(TINY, flags)
    assert not any("_target" in n for n, _, _, _ in plan.params)
    _, tasks, _, _, _, _ = plan_arrays(plan)
    assert all(t.pad2 == 0 for t in tasks if t.epi & (16 | 32))      # no dropout stream offset outside --add_fc


def test_recorded_plans_are_unchanged_to_the_byte():
    """Every configuration of tests/golden/plan_fingerprints.json (none sets the new flag) still builds the recorded plan."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_plan_fingerprints as fp
    fp.clean_env()
    with open(fp.JSON_PATH) as f:
        recorded = json.load(f)["entries"]
    matrix = fp.matrix()
    assert sorted(matrix) == sorted(recorded)
    for name in sorted(recorded):
        assert fp.fingerprint(matrix[name]) == recorded[name], name


# ---- refusals and acceptance ----
@pytest.mark.parametrize("flags,kw,named", [
    (SP, dict(aggregation=_lib.AGG_AVGPOOL), "on avgpool"),
    (SP | _lib.FLAG_MCD, {}, "MCD"), (SP | _lib.FLAG_BN_SHARED, {}, "use_bn"), (SP | _lib.FLAG_FRAME_ATTN, {}, "FRAME_ATTN"),
    ((SP & ~A) | _lib.FLAG_GENERAL_ATTN, {}, "GENERAL_ATTN"), (SP | _lib.FLAG_F32_SPLIT, {}, "F32_SPLIT"),
    (SP, dict(shared_fc_layers=2), "shared_fc_layers"), (SP, dict(chain=1), "chain"), (SP, dict(split_k=2), "split_k"),
    (SP, dict(wgrads_late=1), "wgrads_late"), (SP, dict(phase_tiles=[222]), "phase_tiles")])
def test_plan_refuses_unbuilt_combinations_by_name(flags, kw, named):
    with pytest.raises(ValueError, match="share_params N.*" + named):
        _plan(TINY, flags, **kw)


@pytest.mark.parametrize("Bs,Bt", [(0, 4), (6, 0)])
def test_plan_refuses_an_empty_half_by_name(Bs, Bt):
    with pytest.raises(ValueError, match="share_params N.*batch_source == 0 or batch_target == 0"):
        _plan(dict(TINY, Bs=Bs, Bt=Bt), V | Fr | A | U)


@pytest.mark.parametrize("arith", [0, _lib.FLAG_BF16_MFMA, TW])
def test_plan_accepts_the_supported_combinations(arith):
    for flags in (SP, SP | _lib.FLAG_FEATURE_GRADS, SP | _lib.FLAG_CLASS_WEIGHTS, SP | _lib.FLAG_TARGET_LABELS,
                  (SP & ~E) | _lib.FLAG_TARGET_ENTROPY, V | Fr | U, Fr | U, R | V | Fr | U, U):
        for T in (2, 5, 64):
            plan = _plan(dict(TINY, T=T), flags | arith)
            assert not plan.has_fused_step and _lib.lib().ta3n_has_pipelined_step(plan.handle) == 0


def test_refusal_text_names_the_combination():
    assert share_params_refusal("Y", frame_aggregation="avgpool", use_bn="AdaBN", world=2) == ""
    assert share_params_refusal("N") == "" and share_params_refusal("N", use_attn="none") == ""
    assert "avgpool" in share_params_refusal("N", frame_aggregation="avgpool")
    for kw, named in ((dict(use_attn_frame="TransAttn"), "--use_attn_frame TransAttn"), (dict(use_attn="general"), "--use_attn general"),
                      (dict(add_fc=2), "--add_fc 2"), (dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(dis_DA="JAN"), "--dis_DA JAN"),
                      (dict(ens_DA="MCD"), "--ens_DA MCD"), (dict(f32_split=True), "f32_split"), (dict(chain=True), "chain"),
                      (dict(split_k=2), "split_k"), (dict(wgrads_late=True), "wgrads_late"), (dict(phase_tiles=True), "tuned tile lists"),
                      (dict(world=2), "world size 2"), (dict(process_group=True), "a process group"), (dict(ddp_selftest=True), "TA3N_DDP_SELFTEST"),
                      (dict(sharded_update=True), "sharded update"), (dict(peer_exchange=True), "peer gradient exchange")):
        msg = share_params_refusal("N", **kw)
        assert msg.startswith("--share_params N") and named in msg, (kw, msg)


def test_train_engine_refuses_before_it_needs_a_device(monkeypatch):
    """TrainEngine names the combination (the refusals come first; on a machine without a GPU the supported one then stops at the
    device check, which is how this test tells them apart)."""
    from ta3n_amd.engine import TrainEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    N = dict(share_params="N")
    for kw, named in ((dict(N, aggregation="avgpool", flags=0), "avgpool"), (dict(N, use_bn="AdaBN"), "--use_bn AdaBN"),
                      (dict(N, ens_DA="MCD"), "--ens_DA MCD"), (dict(N, dis_DA="DAN"), "--dis_DA DAN"),
                      (dict(N, f32_split=True), "f32_split"), (dict(N, add_fc=2), "--add_fc 2"),
                      (dict(N, flags=R | V | Fr | E | A | _lib.FLAG_FRAME_ATTN), "--use_attn_frame TransAttn"),
                      (dict(N, flags=R | V | Fr | E | _lib.FLAG_GENERAL_ATTN), "--use_attn general"),
                      (dict(flags=SP | _lib.FLAG_FRAME_ATTN), "--use_attn_frame TransAttn"),      # the flag alone asks for it too
                      (dict(N, chain=True), "chain"), (dict(N, split_k=2), "split_k"), (dict(N, wgrads_late=True), "wgrads_late"),
                      (dict(N, phase_tiles=[222]), "tile lists"),
                      (dict(N, sharded_update=True), "sharded update"), (dict(N, peer_exchange=True), "peer gradient exchange")):
        with pytest.raises(NotImplementedError, match="share_params N.*" + named):
            TrainEngine(6, 4, 5, 512, 64, 12, **kw)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in (dict(), dict(optimizer="Adam"), dict(bf16=True, bf16_store=True), dict(class_weights=[1.0] * 12, domain_weights=(1.0, 2.0)),
               dict(flags=flags_from_options(("N", "Y", "Y"), "target_entropy", "none", "RevGrad", "Sv"))):
        with pytest.raises(_lib.Ta3nError, match="needs a HIP device"):      # the supported combinations get as far as the device check
            TrainEngine(6, 4, 5, 512, 64, 12, share_params="N", **kw)


def _model(**kw):
    from ta3n_amd.models import VideoModel
    return VideoModel(12, "video", kw.pop("agg", "trn-m"), "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64,
                      verbose=False, **kw)


def test_video_model_accepts_unshared_layers():
    plain, m = _model(), _model(share_params="N")
    assert m._flags() == plain._flags() | U and m.share_params == "N"
    assert _model(share_params="N", use_attn="none")._flags() == (plain._flags() & ~A) | U
    plan = m._plan(6, 4)
    assert not plan.has_fused_step
    assert [n for n, _, _, _ in m._named_flat_params(plan)] == [n for n, _, _, _ in plan.params]
    assert {n.rsplit(".", 1)[0] for n, _, _, lv in plan.params if lv and "_target" in n} == set(LIVE_CAPABLE)


@pytest.mark.parametrize("kw,named", [(dict(agg="avgpool", use_attn="none"), "avgpool"),
                                      (dict(use_attn_frame="TransAttn"), "--use_attn_frame TransAttn"),
                                      (dict(use_attn="general"), "--use_attn general"),
                                      (dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(ens_DA="MCD"), "--ens_DA MCD"),
                                      (dict(add_fc=2), "--add_fc 2")])
def test_video_model_refuses_unbuilt_combinations_by_name(kw, named):
    with pytest.raises(NotImplementedError, match="share_params.*" + named):
        _model(share_params="N", **kw)


BASE = ["classInd.txt", "RGB", "s.txt", "t.txt", "v.txt", "--baseline_type", "video", "--frame_aggregation", "trn-m",
        "--use_target", "uSv", "--adv_DA", "RevGrad", "--add_loss_DA", "attentive_entropy", "--lr_adaptive", "dann", "--fc_dim", "512"]


def test_module_path_validation_accepts_the_built_combinations():
    import train_ddp
    from ta3n_amd.opts import parser
    for extra in ([], ["--place_adv", "N", "Y", "Y", "--add_loss_DA", "none"], ["--optimizer", "Adam"], ["--use_target", "Sv"],
                  ["--add_loss_DA", "target_entropy"], ["--use_attn", "none", "--add_loss_DA", "none"],
                  ["--weighted_class_loss", "Y", "--weighted_class_loss_DA", "Y"]):
        train_ddp.validate_options(parser.parse_args(BASE + ["--share_params", "N"] + extra), module_path=True)


def test_train_ddp_refuses_it_and_names_main_py():
    import train_ddp
    from ta3n_amd.opts import parser
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(BASE + ["--share_params", "N"]))
    assert "unsupported option" in str(e.value) and "--share_params N (built on main.py)" in str(e.value)


@pytest.mark.parametrize("extra,named", [
    (["--use_attn_frame", "TransAttn"], "--use_attn_frame TransAttn"), (["--use_bn", "AdaBN"], "--use_bn AdaBN"),
    (["--ens_DA", "MCD", "--mu", "0.5"], "--ens_DA MCD"), (["--dis_DA", "JAN"], "--dis_DA JAN"), (["--add_fc", "2"], "--add_fc 2"),
    (["--use_attn", "general"], "--use_attn general")])
def test_module_path_validation_refuses_unbuilt_combinations_by_name(extra, named):
    import train_ddp
    from ta3n_amd.opts import parser
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(BASE + ["--share_params", "N"] + extra), module_path=True)
    assert "unsupported option" in str(e.value) and "--share_params N together with" in str(e.value) and named in str(e.value)


def test_module_path_validation_refuses_unshared_layers_on_avgpool():
    import train_ddp
    from ta3n_amd.opts import parser
    argv = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "avgpool", "--use_attn", "none", "--add_loss_DA", "none",
            "--share_params", "N"]
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(argv), module_path=True)
    assert "--share_params N on --frame_aggregation avgpool" in str(e.value)


def test_the_flag_is_the_next_free_bit():
    assert U == 1 << 16 and not (U & (flags_from_options(use_target="Sv") | flags_from_options(add_loss_DA="target_entropy") |
                                      flags_from_options(use_attn="general") | flags_from_options(use_attn_frame="TransAttn")))
    header = open(os.path.join(ROOT, "include", "ta3n_hip.h")).read()
    assert "#define TA3N_FLAG_UNSHARED       (1u << 16)" in header
