"""--use_target Sv and --add_loss_DA target_entropy without a GPU (reference main.py:439-446, 542-545): options, the two plan flags and their
refusals, the engine's refusals, the loss normalisers, and - on the reference alone - that the cases of tests/target_cases.py cannot be passed
by a kernel that ignored an option or mistook it for its neighbour."""
import ctypes as C

import pytest
import torch

import plan_interp as pi
import target_cases as tc
import train_ddp
from ta3n_amd import _lib, parallel
from ta3n_amd.engine import ALL_FLAGS, TrainEngine, flags_from_options, target_refusal
from ta3n_amd.opts import parser

BASE = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "trn-m"]
SV, TENT = _lib.FLAG_TARGET_LABELS, _lib.FLAG_TARGET_ENTROPY
ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME


@pytest.mark.parametrize("opt,named", [(["--use_target", "Sv"], "--use_target Sv (built on main.py)"),
                                       (["--use_target", "uSv", "--add_loss_DA", "target_entropy"], "--add_loss_DA target_entropy (built: attentive_entropy) (built on main.py)")])
def test_options_are_accepted_on_the_module_path_and_refused_by_train_ddp(opt, named):
    args = parser.parse_args(BASE + opt)
    train_ddp.validate_options(args, module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(args)
    assert "unsupported option" in str(e.value) and named in str(e.value)
    train_ddp.validate_options(parser.parse_args(BASE + ["--use_target", "Sv", "--add_loss_DA", "target_entropy"]), module_path=True)


@pytest.mark.parametrize("module_path", [True, False])
def test_validate_options_names_what_is_not_built(module_path):
    def refused(extra):
        with pytest.raises(SystemExit) as e:
            train_ddp.validate_options(parser.parse_args(BASE + extra), module_path=module_path)
        return str(e.value)
    mcd = ["--ens_DA", "MCD", "--mu", "0.5"]
    if module_path:
        assert "--use_target Sv with --ens_DA MCD" in refused(["--use_target", "Sv"] + mcd)
        assert "--add_loss_DA target_entropy with --ens_DA MCD" in refused(["--use_target", "uSv", "--add_loss_DA", "target_entropy"] + mcd)
    else:
        assert "(built on main.py)" in refused(["--use_target", "Sv"] + mcd)
        assert "(built on main.py)" in refused(["--use_target", "uSv", "--add_loss_DA", "target_entropy"] + mcd)
    # target entropy on TemPooling stays refused, as before
    avg = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "avgpool", "--use_attn", "none"]
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(avg + ["--use_target", "uSv", "--add_loss_DA", "target_entropy"]), module_path=module_path)
    assert "avgpool is built without attention / attentive entropy" in str(e.value)
    # ... and a value the option does not have keeps its refusal
    assert "--pred_normalize Y" in refused(["--use_target", "Sv", "--pred_normalize", "Y"])


def test_flags_from_options_values():
    assert flags_from_options(use_target="uSv") == ALL_FLAGS                                  # as before
    assert flags_from_options(use_target="Sv") == ALL_FLAGS | SV                              # everything else as under uSv
    assert flags_from_options(add_loss_DA="target_entropy") == (ALL_FLAGS & ~_lib.FLAG_ATTN_ENTROPY) | TENT
    assert flags_from_options(add_loss_DA="target_entropy", use_target="Sv") == (ALL_FLAGS & ~_lib.FLAG_ATTN_ENTROPY) | TENT | SV
    assert flags_from_options(add_loss_DA="target_entropy", use_target="none") == _lib.FLAG_TRANS_ATTN      # main.py:542 asks for use_target != none
    # the term needs neither attention nor an adversarial branch
    assert flags_from_options(("N", "N", "N"), "target_entropy", "none", "RevGrad", "uSv") == TENT
    assert flags_from_options(("Y", "Y", "Y"), "target_entropy", "none", "none", "uSv") == TENT
    assert SV == 1 << 13 and TENT == 1 << 14


def test_loss_normalisers_keep_their_values_without_the_new_argument():
    for gs, gt, T in ((6, 4, 5), (5, 3, 5), (128, 74, 5), (0, 0, 2), (3, 0, 3)):
        tot = max(gs + gt, 1)
        today = dict(inv_n_cls=1.0 / max(gs, 1), inv_n_rel=1.0 / (tot * (T - 1)), inv_n_vid=1.0 / tot, inv_n_frm=1.0 / (tot * T), inv_n_ent=1.0 / tot)
        assert parallel.loss_normalisers(gs, gt, T) == today == parallel.loss_normalisers(gs, gt, T, ALL_FLAGS)
        assert parallel.loss_normalisers(gs, gt, T, SV) == dict(today, inv_n_cls=1.0 / tot)
        assert parallel.loss_normalisers(gs, gt, T, TENT) == dict(today, inv_n_ent=1.0 / max(gt, 1))
        assert parallel.loss_normalisers(gs, gt, T, SV | TENT) == dict(today, inv_n_cls=1.0 / tot, inv_n_ent=1.0 / max(gt, 1))


def test_set_hyper_takes_the_normalisers_of_the_flags_and_refuses_a_step_without_target_rows():
    class Stand:
        pass
    s = Stand()
    s._hyper, s.Bs, s.Bt, s.T, s.world, s.rank, s.step_count = _lib.Hyper(), 6, 4, 5, 1, 0, 0
    s.momentum, s.weight_decay, s.clip, s.dropout_i, s.dropout_v = 0.9, 1e-4, 20.0, 0.5, 0.5
    s._flags = ALL_FLAGS
    TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.3, 1e-3, valid_source=5, valid_target=3, upload=False)
    assert s._hyper.inv_n_cls == C.c_float(1 / 5).value and s._hyper.inv_n_ent == C.c_float(1 / 8).value
    s._flags = SV | TENT
    TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.3, 1e-3, valid_source=5, valid_target=3, upload=False)
    assert s._hyper.inv_n_cls == C.c_float(1 / 8).value and s._hyper.inv_n_ent == C.c_float(1 / 3).value
    with pytest.raises(ValueError, match="--add_loss_DA target_entropy"):
        TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.3, 1e-3, valid_source=5, valid_target=0, upload=False)
    s._flags = SV      # Sv alone: a fully padded target half is a step over the source rows
    TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.3, 1e-3, valid_source=5, valid_target=0, upload=False)
    assert s._hyper.inv_n_cls == C.c_float(1 / 5).value


def test_hyper_struct_keeps_its_26_dwords():
    s = C.c_int32()
    _lib.lib().ta3n_debug_struct_sizes(None, None, None, None, C.byref(s))
    assert C.sizeof(_lib.Hyper) == s.value == 26 * 4


def _arrays(plan):
    L = _lib.lib()
    ptrs = [C.c_void_p() for _ in range(6)]
    ns = [C.c_int64() for _ in range(3)]
    L.ta3n_debug_arrays(plan.handle, C.byref(ptrs[0]), C.byref(ns[0]), C.byref(ptrs[1]), C.byref(ns[1]), C.byref(ptrs[2]), C.byref(ns[2]),
                        C.byref(ptrs[3]), C.byref(ptrs[4]), C.byref(ptrs[5]))
    raw = [C.string_at(ptrs[i], ns[i].value * C.sizeof(t)) for i, t in enumerate((pi.Seg, pi.Task, pi.Phase))]
    geom = C.cast(ptrs[3], C.POINTER(pi.Geom)).contents
    return raw, {name: (list(getattr(geom, name)) if hasattr(getattr(geom, name), "__len__") else getattr(geom, name)) for name, _ in pi.Geom._fields_}


NO_ENT = ALL_FLAGS & ~_lib.FLAG_ATTN_ENTROPY
PLANS = [dict(flags=ALL_FLAGS, add=SV), dict(flags=NO_ENT, add=TENT), dict(flags=NO_ENT, add=SV | TENT), dict(flags=0, add=TENT),
         dict(flags=NO_ENT | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, add=SV | TENT), dict(flags=NO_ENT | _lib.FLAG_BN_SHARED, add=SV | TENT),
         dict(flags=ALL_FLAGS | _lib.FLAG_CLASS_WEIGHTS, add=SV), dict(flags=NO_ENT | _lib.FLAG_FEATURE_GRADS, add=SV | TENT),
         dict(flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME, add=SV, aggregation=_lib.AGG_AVGPOOL), dict(flags=NO_ENT, add=SV | TENT, shared_fc_layers=2)]


@pytest.mark.parametrize("kw", PLANS, ids=[str(i) for i in range(len(PLANS))])
def test_flagged_plan_differs_in_its_flags_alone(kw):
    """Same regions, launch lists and tiles: neither flag costs a launch or a workspace float."""
    assert pi.struct_sizes_ok()
    kw = dict(kw)
    flags, add = kw.pop("flags"), kw.pop("add")
    a = _lib.Plan(6, 4, 5, 512, 64, 12, flags, **kw)
    b = _lib.Plan(6, 4, 5, 512, 64, 12, flags | add, **kw)
    assert a.regions == b.regions and a.ws_floats == b.ws_floats and a.params == b.params and a.has_fused_step == b.has_fused_step
    assert a.regions["labels"][1] >= 10      # one label per video of BOTH halves, in every plan
    (raw_a, geom_a), (raw_b, geom_b) = _arrays(a), _arrays(b)
    assert raw_a == raw_b      # Segs, Tasks, Phases byte for byte
    assert geom_b.pop("flags") == geom_a.pop("flags") | add and geom_a == geom_b


def test_plan_refusals_fire_by_name():
    for flags, kw, text in ((ALL_FLAGS | SV | _lib.FLAG_MCD, {}, "TA3N_FLAG_TARGET_LABELS .* with TA3N_FLAG_MCD"),
                            (NO_ENT | TENT | _lib.FLAG_MCD, {}, "TA3N_FLAG_TARGET_ENTROPY .* with TA3N_FLAG_MCD"),
                            (ALL_FLAGS | TENT, {}, "TA3N_FLAG_TARGET_ENTROPY and TA3N_FLAG_ATTN_ENTROPY"),
                            (SV, dict(aggregation=_lib.AGG_AVGPOOL), "TA3N_FLAG_TARGET_LABELS .* source-only avgpool"),
                            (TENT, dict(aggregation=_lib.AGG_AVGPOOL), "avgpool: TA3N_FLAG_TARGET_ENTROPY"),
                            (_lib.FLAG_ADV_VIDEO | TENT, dict(aggregation=_lib.AGG_AVGPOOL), "avgpool: TA3N_FLAG_TARGET_ENTROPY")):
        with pytest.raises(ValueError, match=text):
            _lib.Plan(6, 4, 5, 512, 64, 12, flags, **kw)
    with pytest.raises(ValueError, match="TA3N_FLAG_TARGET_LABELS .* without target rows"):
        _lib.Plan(6, 0, 5, 512, 64, 12, SV)


def test_engine_refusals_fire_by_name_without_a_device(monkeypatch):
    sv, both = flags_from_options(use_target="Sv"), flags_from_options(add_loss_DA="target_entropy", use_target="Sv")
    tent = flags_from_options(add_loss_DA="target_entropy")
    for kw, text in ((dict(flags=sv, process_group=object()), "--use_target Sv together with world size"),
                     (dict(flags=tent, process_group=object()), "--add_loss_DA target_entropy together with world size"),
                     (dict(flags=both, sharded_update=True), "sharded update"),
                     (dict(flags=both, peer_exchange=True), "peer gradient exchange"),
                     (dict(flags=sv, ens_DA="MCD"), "--ens_DA MCD"),
                     (dict(flags=tent, ens_DA="MCD"), "--ens_DA MCD")):
        with pytest.raises(NotImplementedError, match=text):
            TrainEngine(6, 4, 5, 512, 64, 12, **kw)
    monkeypatch.setenv("TA3N_DDP_SELFTEST", "1")
    for flags in (sv, tent):
        with pytest.raises(NotImplementedError, match="TA3N_DDP_SELFTEST"):
            TrainEngine(6, 4, 5, 512, 64, 12, flags=flags)
    assert target_refusal("Sv", "target_entropy") == "" and target_refusal("uSv", "attentive_entropy", world=8, ens_DA="MCD") == ""
    assert target_refusal("none", "target_entropy", world=8) == ""      # (main.py:542: without use_target the term is off)
    assert "world size 2" in target_refusal("Sv", world=2) and "world size 2" in target_refusal("uSv", "target_entropy", world=2)


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_cases_tell_the_options_apart(name):
    """On the reference alone: every block of gY a new option acts on is at least 100 x the GPU test's bound on that block away from the
    block under the option it could be mistaken for."""
    pairs = tc.distinct(name)
    print(f"[target distinct] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in pairs.items()))
    assert pairs or tc.CASES[name]["C"] == 1
    use_target, ent, _ = tc.options(name)
    assert ("Sv|uSv gY_t" in pairs) == (use_target == "Sv" and tc.CASES[name]["C"] > 1)
    assert ("tent|none gY_t" in pairs) == (ent == "target_entropy" and tc.CASES[name]["C"] > 1)
    for k, v in pairs.items():
        assert v >= 100 * tc.LOGIT_GRAD_REL_L2["f32"], (name, k, v)
    if name == "base":      # the pair that rests on gamma, at the reference's value
        assert "tent|attentive gY_s" in pairs
    if tc.CASES[name].get("cw") and use_target == "Sv":
        assert "w both|source gY_t" in pairs


def test_padding_rows_and_the_other_half_get_nothing():
    ref = tc.shared_reference("ragged")["logit_grads"]
    assert (ref["gY_s"][5:] == 0).all() and (ref["gY_t"][3:] == 0).all() and ref["gY_s"][:5].abs().sum() > 0 and ref["gY_t"][:3].abs().sum() > 0
    # target entropy alone: the source rows carry the cross-entropy only, the domain logits nothing from it
    a, b = tc.case_reference("tent_plain")["logit_grads"], tc.case_reference("tent_plain", ent="none")["logit_grads"]
    assert torch.equal(a["gY_s"], b["gY_s"]) and torch.equal(a["gPv"], b["gPv"]) and not torch.equal(a["gY_t"], b["gY_t"])


def test_fp32_restatement_against_float64():
    """The reference's own error: the fp32 restatement of a step against the float64 one - far below the bounds the GPU test applies."""
    cfg, _, params, xs, xt, labels, ns, nt, cw = tc.case_setup("ragged")
    a = tc.reference_step(cfg, params, xs, xt, labels, ns, nt, "Sv", "target_entropy")
    b = tc.reference_step(cfg, params, xs, xt, labels, ns, nt, "Sv", "target_entropy", dtype=torch.float64)
    worst = max(tc.wl.rel_l2(a["grads"][k], b["grads"][k]) for k in b["grads"])
    blocks = max(tc.wl.rel_l2(a["logit_grads"][k], b["logit_grads"][k]) for k in ("gY_s", "gY_t"))
    print(f"[target floor] fp32 vs float64 reference, ragged: worst gradient rel. L2 {worst:.2e}, gY blocks {blocks:.2e}")
    assert worst <= 0.25 * tc.tol.F32_MASKED_GRAD_REL_L2 and blocks <= 0.01 * tc.LOGIT_GRAD_REL_L2["f32"]
    assert abs(a["parts"]["loss"] - b["parts"]["loss"]) <= 1e-5 * max(1.0, abs(b["parts"]["loss"]))


@pytest.mark.parametrize("name", tc.FIXTURES)
def test_restatement_matches_the_reference_fixtures(name):
    """Ties tests/target_cases.py to the reference itself: its loss terms against the log lines main.train printed under --use_target Sv
    (and --add_loss_DA target_entropy), its clipped gradients and updated parameters against the recorded ones, step by step along the
    reference's own trajectory."""
    from golden_util import step_schedule
    from ta3n_amd.synthetic import synth_state
    g, c, cfg, use_target, ent, gamma = tc.fixture_setup(name)
    assert use_target == "Sv" and (ent == "target_entropy") == (name == "tiny_sv_tent") and (gamma == 0.3) == (name == "tiny_sv_tent")
    params = synth_state(tc.wl.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    log = str(g.meta("log")).strip().splitlines()
    mom = None
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = tc.fixture_batch(c, st)
        ref = tc.reference_step(cfg, params, xs, xt, labels, st["n_src"], st["n_tgt"], use_target, ent, gamma=gamma, lr=st["lr"], momentum=mom, clip=c["clip"])
        want = tc.wl.log_numbers(log[s])
        got = dict(Loss=ref["parts"]["loss"], loss_c=ref["parts"]["loss_c"], loss_a=ref["parts"]["loss_a"], loss_e=ref["parts"].get("loss_e"))
        assert set(want) >= {"Loss", "loss_c", "loss_a"} and ("loss_e" in want) == (ent == "target_entropy")
        for k, w in want.items():
            assert abs(got[k] - w) <= 1e-4 * max(1.0, abs(w)), (name, s, k, got[k], w)      # (the log prints four decimals)
        for k, v in ref["grads"].items():
            g.check(f"step{s}/clipped_grad/{k}", v * ref["clip_coef"], 2e-5, 2e-6, rms_atol=2e-5)
        for k, v in ref["params"].items():
            g.check(f"step{s}/param/{k}", v, 2e-5, 2e-6)
        params, mom = ref["params"], ref["momentum"]
    # ... and the options do matter there: under uSv the logged classification loss is missed by far more than the log's resolution
    p0 = synth_state(tc.wl.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    st0 = step_schedule(c)[0]
    xs, xt, labels = tc.fixture_batch(c, st0)
    plain = tc.reference_step(cfg, p0, xs, xt, labels, st0["n_src"], st0["n_tgt"], "uSv", "none", gamma=gamma)
    assert abs(plain["parts"]["loss_c"] - tc.wl.log_numbers(log[0])["loss_c"]) > 100 * 1e-4
