"""--use_attn general (models.py:320-325, 359-366, 379-388: the relation features weighted by the softmax over the relations of a
learned layer's scores) on the CPU: the new plans executed with numpy (tests/plan_interp.py) against fixtures the
reference produced (tests/golden/make_golden_general_attn.py), the launch order, the plans without the flag left as they were, and
the option handling at the plan, TrainEngine, VideoModel, train_ddp.py and main.py levels."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from plan_interp import PH_GENERAL_ATTN_BWD, PH_GENERAL_ATTN_FWD, Interp, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import flags_from_options, general_attn_refusal
from ta3n_amd.synthetic import synth_batch, synth_state
from test_plan_cpu import make_hyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GA_CASES = ["tiny_ga_T5", "tiny_ga_T2", "tiny_ga_odd", "tiny_ga_relN", "tiny_ga_T9", "mid_ga"]
R, V, Fr, E, A = (_lib.FLAG_ADV_RELATION, _lib.FLAG_ADV_VIDEO, _lib.FLAG_ADV_FRAME, _lib.FLAG_ATTN_ENTROPY, _lib.FLAG_TRANS_ATTN)
GA = R | V | Fr | E | _lib.FLAG_GENERAL_ATTN
TINY = dict(Bs=6, Bt=4, T=5, D=512, fc_dim=64, C=12)
NEW_REGIONS = {"Ua", "gUa", "gs"}
ATTN_PARAMS = {"attn_layer.0.weight": (256, 256), "attn_layer.0.bias": (256,), "attn_layer.2.weight": (1, 256), "attn_layer.2.bias": (1,)}


def ga_flags(c):
    return flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), c["add_loss_DA"] or "attentive_entropy", "general", "RevGrad", "uSv")


def _plan(c, flags, **kw):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags, **kw)


def _load_step(it, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:c["Bs"]] = ys.numpy()
    it.hy = make_hyper(c, st, c["T"], st["lr"])
    it.G[:] = 0


@pytest.mark.parametrize("extra", [0, _lib.FLAG_FEATURE_GRADS], ids=["engine", "module"])
@pytest.mark.parametrize("name", GA_CASES)
def test_plan_reproduces_reference(name, extra):
    """ta3n_forward / ta3n_loss / ta3n_backward / ta3n_sgd_step of the general-attention plan against the reference's run of the same
    command: forward tensors and the attention weights, clipped gradients of step 0 and the parameters after every step (the last step
    of tiny_ga_T5 with padded videos), with the bounds of tests/test_frame_attn_cpu.py.  extra = TA3N_FLAG_FEATURE_GRADS: the plan
    VideoModel builds (no outside gradient: the same numbers)."""
    g = Golden(name)
    assert str(g.meta("use_attn")) == "general"
    c = case_config(g)
    T = c["T"]
    plan = _plan(c, ga_flags(c) | extra)
    assert not plan.has_fused_step
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    assert set(ATTN_PARAMS) <= live
    assert ("relation_domain_classifier_all.0.0.weight" in live) == (name != "tiny_ga_relN")
    for s, st in enumerate(step_schedule(c)):
        _load_step(it, c, st)
        it.run_group(0)
        if s == 0:
            B, Bs = c["Bs"] + c["Bt"], c["Bs"]
            geo = it.g
            outs = dict(out=it.r(geo.o_Y, (B, c["C"])), attn=it.r(geo.o_attn, (B, T - 1)),
                        rel=it.r(geo.o_Pr, (B, T - 1, 2)), vid=it.r(geo.o_Pv, (B, 2)), frm=it.r(geo.o_Pf, (B, T, 2)),
                        v=it.r(geo.o_V, (B, 256)), f1=it.r(geo.o_F1, (B, T, geo.F)))
            assert np.abs(outs["attn"].sum(1) - 1).max() < 1e-12
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
                # attn_layer.2.bias: mathematically zero (the softmax is shift invariant), ~1e-8 from the reference's autograd - the absolute term only
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 0 if k == "attn_layer.2.bias" else 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", new[k], 1e-4, 2e-5)
        if T == 2:      # one relation: w = 1 exactly, every gradient of the attention layer exactly zero - and still live (weight decay moved it)
            assert (it.r(it.g.o_attn, (c["Bs"] + c["Bt"], 1)) == 1).all()
            for k in ATTN_PARAMS:
                assert (raw[k] == 0).all(), k


@pytest.mark.parametrize("name", GA_CASES)
def test_parameter_names_and_shapes_are_the_references(name):
    """The plan holds exactly the reference's parameters (state_dict names of meta/state_keys, BatchNorm buffers aside) in their
    shapes; VideoModel(use_attn='general').state_dict() has the reference's key order, the four attn_layer keys last."""
    g = Golden(name)
    c = case_config(g)
    keys = [str(k) for k in g.meta("state_keys")]
    assert keys[-4:] == list(ATTN_PARAMS)
    plan = _plan(c, ga_flags(c))
    shapes = {n: tuple(s) for n, _, s, _ in plan.params}
    assert set(shapes) == {k for k in keys if "running_" not in k and "num_batches" not in k}
    for k, shp in ATTN_PARAMS.items():
        assert shapes[k] == shp
    from ta3n_amd.models import VideoModel
    m = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   verbose=False, use_attn="general")
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert {k: tuple(v.shape) for k, v in sd.items() if k in shapes} == shapes


def test_padded_rows_contribute_no_gradient():
    """Short last batch of tiny_ga_T5: the padded videos get weights from whatever their features hold, and exactly zero in gs, gUa, gRa."""
    g = Golden("tiny_ga_T5")
    c = case_config(g)
    plan = _plan(c, GA)
    it = Interp(plan)
    it.set_params(synth_state({n: s for n, _, s, _ in plan.params}, seed=c["wseed"], scale=c["wscale"]))
    st = step_schedule(c)[-1]
    assert (st["n_src"], st["n_tgt"]) == (5, 3)
    _load_step(it, c, st)
    for grp in (0, 1, 2):
        it.run_group(grp)
    B, NR = c["Bs"] + c["Bt"], c["T"] - 1
    pad = [5, 9]
    assert (it.r(it.g.o_attn, (B, NR))[pad] > 0).all()
    for name, width in (("gs", 1), ("gUa", 256), ("gRa", 256)):
        assert (it.r(plan.region(name)[0], (B, NR, width))[pad] == 0).all(), name
    assert (it.r(plan.region("gUa")[0], (B, NR, 256))[:5] != 0).any()


def test_launch_order_is_the_plain_one():
    """The plain unfused lists launch for launch, with the two general-attention launches in place of the pooling launches, the Ua
    specs in the launch of Hr and Pf, and gUa / the layer's weight gradients in the relation-level launch."""
    plan, plain = _plan(TINY, GA), _plan(TINY, R | V | Fr | E | A)
    segs, tasks, phases, geo, _, _ = plan_arrays(plan)
    kinds = lambda phs, grp: [ph.kind for ph in phs if ph.group == grp]      # noqa: E731
    pphases = plan_arrays(plain)[2]
    assert kinds(phases, 0) == [PH_GENERAL_ATTN_FWD if k == 1 else k for k in kinds(pphases, 0)] == [0, 0, 0, PH_GENERAL_ATTN_FWD, 0, 0]
    assert kinds(phases, 2) == [PH_GENERAL_ATTN_BWD if k == 3 else k for k in kinds(pphases, 2)] == [0, 0, PH_GENERAL_ATTN_BWD, 0, 0, 0]
    assert kinds(phases, 1) == kinds(pphases, 1) and kinds(phases, 3) == kinds(pphases, 3)
    assert not any(ph.group in (4, 5) for ph in phases)
    Ua, gUa, gs = (plan.region(n) for n in ("Ua", "gUa", "gs"))
    assert Ua[1] == gUa[1] == 10 * 4 * 256 and gs[1] == 40
    poff = {n: off for n, off, _, _ in plan.params}

    def phase_of(pred):
        hit = [i for i, ph in enumerate(phases) if ph.kind == 0 and any(pred(tasks[k]) for k in range(ph.task_begin, ph.task_begin + ph.task_count))]
        assert len(hit) == 1, hit
        return hit[0]

    def reads(t, base, reg):
        return any(b == base and reg[0] <= off < reg[0] + reg[1]
                   for s in segs[t.seg_begin:t.seg_begin + t.seg_count] for b, off in ((s.a_base, s.a_off), (s.b_base, s.b_off)))
    in_ws = lambda t, reg: t.seg_count and t.c_base == 3 and reg[0] <= t.c_off < reg[0] + reg[1]      # noqa: E731
    writes_ua = phase_of(lambda t: in_ws(t, Ua))
    assert writes_ua == phase_of(lambda t: in_ws(t, plan.region("Hr"))) == phase_of(lambda t: in_ws(t, plan.region("Pf")))
    rel_level = phase_of(lambda t: in_ws(t, plan.region("gR")))
    gr = [t for t in tasks if in_ws(t, plan.region("gR"))]
    assert gr and all(t.seg_count == 2 and reads(t, 3, gUa) and t.alpha_kind == 0 and segs[t.seg_begin].scale_kind == 1 for t in gr)
    for name, src in (("attn_layer.0.weight", gUa), ("attn_layer.2.weight", gs)):
        w = (poff[name], int(np.prod(ATTN_PARAMS[name])))
        assert phase_of(lambda t: t.seg_count and t.c_base == 2 and w[0] <= t.c_off < w[0] + w[1] and reads(t, 3, src)) == rel_level


def test_no_launch_loses_its_twin_reads():
    """bf16 + bf16_store: the GEMM launches of the general-attention lists read twins exactly where the TransAttn unfused lists do (the
    relation-level launch reads none in either: what the pooling / attention kernels write has no twin)."""
    tw = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
    for fc_dim in (64, 20):
        mine, plain = _plan(dict(TINY, fc_dim=fc_dim), GA | tw), _plan(dict(TINY, fc_dim=fc_dim), R | V | Fr | E | A | tw)      # (kept alive: plan_arrays returns views)
        ours = [bool(ph.bf16 & 16) for ph in plan_arrays(mine)[2] if ph.group in (0, 2) and ph.kind == 0]
        theirs = [bool(ph.bf16 & 16) for ph in plan_arrays(plain)[2] if ph.group in (0, 2) and ph.kind == 0]
        assert ours == theirs and any(ours)
        assert ours[1] == (fc_dim == 64)      # the tuple products: operands fc_dim wide


@pytest.mark.parametrize("flags", [R | V | Fr | E | A, R | V | Fr | E | A | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE,
                                   R | V | Fr | E | A | _lib.FLAG_FEATURE_GRADS, V | Fr, R | V | Fr | E | A | _lib.FLAG_FRAME_ATTN])
def test_plans_without_the_flag_have_none_of_it(flags):
    plan = _plan(TINY, flags)
    assert not NEW_REGIONS & set(plan.regions)
    assert not any(ph.kind in (PH_GENERAL_ATTN_FWD, PH_GENERAL_ATTN_BWD) for ph in plan_arrays(plan)[2])
    assert not any(n.startswith("attn_layer") for n, _, _, _ in plan.params)


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
    (GA | A, {}, "TRANS_ATTN"), (GA | _lib.FLAG_FRAME_ATTN, {}, "FRAME_ATTN"), (GA | A | _lib.FLAG_FRAME_ATTN, {}, "TRANS_ATTN"),
    (GA, dict(aggregation=_lib.AGG_AVGPOOL), "on avgpool"),
    (GA | _lib.FLAG_F32_SPLIT, {}, "F32_SPLIT"), (GA | _lib.FLAG_MCD, {}, "MCD"), (GA | _lib.FLAG_BN_SHARED, {}, "use_bn"),
    (GA, dict(shared_fc_layers=2), "shared_fc_layers"), (GA, dict(chain=1), "chain"), (GA, dict(split_k=2), "split_k"),
    (GA, dict(wgrads_late=1), "wgrads_late"), (GA, dict(phase_tiles=[222]), "phase_tiles")])
def test_plan_refuses_unbuilt_combinations_by_name(flags, kw, named):
    with pytest.raises(ValueError, match="use_attn general.*" + named):
        _plan(TINY, flags, **kw)


@pytest.mark.parametrize("arith", [0, _lib.FLAG_BF16_MFMA, _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE])
def test_plan_accepts_the_supported_combination(arith):
    for extra in (0, _lib.FLAG_FEATURE_GRADS):
        for T in (2, 5, 64):
            plan = _plan(dict(TINY, T=T), GA | arith | extra)
            assert not plan.has_fused_step and _lib.lib().ta3n_has_pipelined_step(plan.handle) == 0
            assert plan.region("gs")[1] == 10 * (T - 1) and plan.region("Ua")[1] == 10 * (T - 1) * 256


def test_refusal_text_names_the_combination():
    assert general_attn_refusal("none", frame_aggregation="avgpool", use_bn="AdaBN") == ""
    assert general_attn_refusal("TransAttn", use_attn_frame="TransAttn", world=2) == ""
    assert general_attn_refusal("general") == ""
    assert "avgpool" in general_attn_refusal("general", frame_aggregation="avgpool")
    for kw, named in ((dict(use_attn_frame="TransAttn"), "--use_attn_frame TransAttn"), (dict(add_fc=2), "--add_fc 2"),
                      (dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(dis_DA="JAN"), "--dis_DA JAN"), (dict(ens_DA="MCD"), "--ens_DA MCD"),
                      (dict(f32_split=True), "f32_split"), (dict(chain=True), "chain"), (dict(split_k=2), "split_k"),
                      (dict(wgrads_late=True), "wgrads_late"), (dict(phase_tiles=True), "tuned tile lists"),
                      (dict(world=2), "world size 2"), (dict(process_group=True), "a process group"), (dict(ddp_selftest=True), "TA3N_DDP_SELFTEST"),
                      (dict(sharded_update=True), "sharded update"), (dict(peer_exchange=True), "peer gradient exchange")):
        msg = general_attn_refusal("general", **kw)
        assert msg.startswith("--use_attn general") and named in msg, (kw, msg)


def test_train_engine_refuses_before_it_needs_a_device(monkeypatch):
    """TrainEngine names the combination (the refusals come first; on a machine without a GPU the supported one then stops at the
    device check, which is how this test tells them apart)."""
    from ta3n_amd.engine import TrainEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for kw, named in ((dict(flags=GA | A), "--use_attn TransAttn"), (dict(flags=GA | _lib.FLAG_FRAME_ATTN), "use_attn_frame"),
                      (dict(flags=GA, aggregation="avgpool"), "avgpool"), (dict(flags=GA, use_bn="AdaBN"), "--use_bn AdaBN"),
                      (dict(flags=GA, ens_DA="MCD"), "--ens_DA MCD"), (dict(flags=GA, dis_DA="DAN"), "--dis_DA DAN"),
                      (dict(flags=GA, f32_split=True), "f32_split"), (dict(flags=GA, add_fc=2), "--add_fc 2"),
                      (dict(flags=GA, chain=True), "chain"), (dict(flags=GA, split_k=2), "split_k"), (dict(flags=GA, wgrads_late=True), "wgrads_late"),
                      (dict(flags=GA, phase_tiles=[222]), "tile lists"),
                      (dict(flags=GA, sharded_update=True), "sharded update"), (dict(flags=GA, peer_exchange=True), "peer gradient exchange")):
        with pytest.raises(NotImplementedError, match="use_attn.*" + named):
            TrainEngine(6, 4, 5, 512, 64, 12, **kw)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ta3nError, match="needs a HIP device"):      # the supported combination gets as far as the device check
        TrainEngine(6, 4, 5, 512, 64, 12, flags=GA, optimizer="Adam")


def _model(**kw):
    from ta3n_amd.models import VideoModel
    return VideoModel(12, "video", kw.pop("agg", "trn-m"), "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64,
                      verbose=False, **kw)


def test_video_model_accepts_general_attention():
    plain, m = _model(use_attn="TransAttn"), _model(use_attn="general")
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys()) + list(ATTN_PARAMS)
    assert m._flags() == (plain._flags() & ~A) | _lib.FLAG_GENERAL_ATTN and m.use_attn == "general"
    plan = m._plan(6, 4)
    assert NEW_REGIONS <= set(plan.regions) and not plan.has_fused_step
    assert [n for n, _, _, _ in m._named_flat_params(plan)] == [n for n, _, _, _ in plan.params]


@pytest.mark.parametrize("kw,named", [(dict(agg="avgpool", use_attn="general"), "avgpool"),
                                      (dict(use_attn="general", use_attn_frame="TransAttn"), "--use_attn_frame TransAttn"),
                                      (dict(use_attn="general", use_attn_frame="general"), "--use_attn_frame general"),
                                      (dict(use_attn="general", use_bn="AdaBN"), "--use_bn AdaBN"),
                                      (dict(use_attn="general", ens_DA="MCD"), "--ens_DA MCD"),
                                      (dict(use_attn="general", add_fc=2), "--add_fc 2")])
def test_video_model_refuses_unbuilt_combinations_by_name(kw, named):
    with pytest.raises(NotImplementedError, match="use_attn.*" + named):
        _model(**kw)


BASE = ["classInd.txt", "RGB", "s.txt", "t.txt", "v.txt", "--baseline_type", "video", "--frame_aggregation", "trn-m",
        "--use_target", "uSv", "--adv_DA", "RevGrad", "--add_loss_DA", "attentive_entropy", "--lr_adaptive", "dann", "--fc_dim", "512"]


def test_module_path_validation_accepts_the_headline_command_line():
    import train_ddp
    from ta3n_amd.opts import parser
    for extra in ([], ["--place_adv", "N", "Y", "Y", "--add_loss_DA", "none"], ["--optimizer", "Adam"]):
        train_ddp.validate_options(parser.parse_args(BASE + ["--use_attn", "general"] + extra), module_path=True)


def test_train_ddp_refuses_it_and_names_main_py():
    import train_ddp
    from ta3n_amd.opts import parser
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(BASE + ["--use_attn", "general"]))
    assert "unsupported option" in str(e.value) and "--use_attn general (built on main.py)" in str(e.value)


@pytest.mark.parametrize("extra,named", [
    (["--use_attn_frame", "TransAttn"], "--use_attn_frame TransAttn"), (["--use_bn", "AdaBN"], "--use_bn AdaBN"),
    (["--ens_DA", "MCD", "--mu", "0.5"], "--ens_DA MCD"), (["--dis_DA", "JAN"], "--dis_DA JAN"), (["--add_fc", "2"], "--add_fc 2")])
def test_module_path_validation_refuses_unbuilt_combinations_by_name(extra, named):
    import train_ddp
    from ta3n_amd.opts import parser
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(BASE + ["--use_attn", "general"] + extra), module_path=True)
    assert "unsupported option" in str(e.value) and "--use_attn general together with" in str(e.value) and named in str(e.value)


def test_module_path_validation_refuses_general_attention_on_avgpool():
    import train_ddp
    from ta3n_amd.opts import parser
    argv = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "avgpool", "--use_attn", "general", "--add_loss_DA", "none"]
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(argv), module_path=True)
    assert "--use_attn general on --frame_aggregation avgpool" in str(e.value)


def test_flags_from_options_sets_its_own_bit():
    assert flags_from_options(use_attn="general") == R | V | Fr | E | _lib.FLAG_GENERAL_ATTN == 15 | (1 << 15)
    assert flags_from_options(("N", "Y", "Y"), "none", "general", "RevGrad", "uSv") == V | Fr | _lib.FLAG_GENERAL_ATTN
    assert flags_from_options() == 31 and flags_from_options(use_attn="none") == R | V | Fr
