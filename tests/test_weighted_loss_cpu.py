"""The weighted criteria without a GPU (--weighted_class_loss / --weighted_class_loss_DA, reference main.py:156-167, 205-206): options and
helpers, the plan flag and the two ta3n_hyper fields, the engine's refusals, and - on the reference alone - that the cases of
tests/weighted_loss_cases.py cannot be passed by a kernel that ignores the weights."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_interp as pi
import train_ddp
import weighted_loss_cases as wl
from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS, TrainEngine, class_weights_from_list, domain_factors, weights_refusal
from ta3n_amd.opts import parser

BASE = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "trn-m"]


@pytest.mark.parametrize("opt", ["--weighted_class_loss", "--weighted_class_loss_DA"])
def test_options_are_accepted_on_the_module_path_and_refused_by_train_ddp(opt):
    args = parser.parse_args(BASE + [opt, "Y"])
    train_ddp.validate_options(args, module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(args)
    assert f"{opt} Y (built on main.py)" in str(e.value)
    train_ddp.validate_options(parser.parse_args(BASE + ["--weighted_class_loss", "Y", "--weighted_class_loss_DA", "Y"]), module_path=True)


def test_class_weights_from_list_restates_the_reference_formula(tmp_path):
    labels = [0] * 7 + [2] * 1 + [1] * 3 + [3] * 20
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"/data/v{i}/ {5 + i} {c}\n" for i, c in enumerate(labels)))
    # 1 / (share of the class in the list), the division in fp32 as the reference's weights are (main.py:156-164)
    counts = np.array([7, 3, 1, 20], dtype=np.float64)
    want = (np.float32(1) / (counts / counts.sum()).astype(np.float32)).tolist()
    got = class_weights_from_list(str(lst), 4)
    assert torch.equal(torch.Tensor(got), torch.Tensor(want)) and max(got) / min(got) == pytest.approx(20.0)
    with pytest.raises(ValueError, match="class 4"):
        class_weights_from_list(str(lst), 5)
    with pytest.raises(ValueError, match="outside"):
        class_weights_from_list(str(lst), 3)


@pytest.mark.parametrize("ns,nt", [(6, 4), (5, 3), (67, 3), (1, 9), (128, 74)])
@pytest.mark.parametrize("weights", [wl.DOMAIN_W, (3.0, 0.25), (1.0, 1.0)])
def test_domain_factors_reproduce_the_weighted_cross_entropy(ns, nt, weights):
    """k_s, k_t times the unweighted per-row coefficient 1 / (r (n_s + n_t)) IS CrossEntropyLoss(weight=(w_s, w_t)), loss and gradient, at
    the relation (r = T - 1), video (1) and frame (T) level."""
    T = 5
    ks, kt = domain_factors(weights, ns, nt)
    g = torch.Generator().manual_seed(ns * 100 + nt)
    for r in (T - 1, 1, T):
        z = torch.randn((ns + nt) * r, 2, generator=g, dtype=torch.float64).requires_grad_(True)
        lab = torch.cat((torch.zeros(ns * r), torch.ones(nt * r))).long()
        want = F.cross_entropy(z, lab, weight=torch.tensor(weights, dtype=torch.float64))
        gw, = torch.autograd.grad(want, z)
        coef = torch.cat((torch.full((ns * r,), ks, dtype=torch.float64), torch.full((nt * r,), kt, dtype=torch.float64))) / (r * (ns + nt))
        lp = F.log_softmax(z, 1)
        got = -(lp[torch.arange(lab.numel()), lab] * coef).sum()
        gg, = torch.autograd.grad(got, z)
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
        assert torch.allclose(gg, gw, rtol=1e-12, atol=1e-15)
    if weights[0] == weights[1]:
        assert ks == 1.0 and kt == 1.0
    assert domain_factors(None, ns, nt) == (0.0, 0.0)      # read as (1, 1) by the kernels: the unweighted criterion


def _arrays(plan):
    L = _lib.lib()
    ptrs = [C.c_void_p() for _ in range(6)]
    ns = [C.c_int64() for _ in range(3)]
    L.ta3n_debug_arrays(plan.handle, C.byref(ptrs[0]), C.byref(ns[0]), C.byref(ptrs[1]), C.byref(ns[1]), C.byref(ptrs[2]), C.byref(ns[2]),
                        C.byref(ptrs[3]), C.byref(ptrs[4]), C.byref(ptrs[5]))
    raw = [C.string_at(ptrs[i], ns[i].value * C.sizeof(t)) for i, t in enumerate((pi.Seg, pi.Task, pi.Phase))]
    geom = C.cast(ptrs[3], C.POINTER(pi.Geom)).contents
    return raw, {name: (list(getattr(geom, name)) if hasattr(getattr(geom, name), "__len__") else getattr(geom, name)) for name, _ in pi.Geom._fields_}


PLANS = [dict(flags=ALL_FLAGS), dict(flags=ALL_FLAGS | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE), dict(flags=ALL_FLAGS | _lib.FLAG_MCD),
         dict(flags=ALL_FLAGS | _lib.FLAG_BN_SHARED), dict(flags=0, aggregation=_lib.AGG_AVGPOOL),
         dict(flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME, aggregation=_lib.AGG_AVGPOOL), dict(flags=ALL_FLAGS, shared_fc_layers=2)]


@pytest.mark.parametrize("kw", PLANS, ids=[str(i) for i in range(len(PLANS))])
def test_flagged_plan_differs_by_the_trailing_region_only(kw):
    assert pi.struct_sizes_ok()
    kw = dict(kw)
    flags = kw.pop("flags")
    a = _lib.Plan(6, 4, 5, 512, 64, 12, flags, **kw)
    b = _lib.Plan(6, 4, 5, 512, 64, 12, flags | _lib.FLAG_CLASS_WEIGHTS, **kw)
    L = _lib.lib()
    assert L.ta3n_ws_offset(a.handle, b"class_w") == -1 and "class_w" not in a.regions
    off, size = b.regions["class_w"]
    assert size == 64 and off == a.ws_floats and b.ws_floats == a.ws_floats + 64 and L.ta3n_ws_offset(b.handle, b"class_w") == off
    assert off == max(o for o, _ in b.regions.values())      # behind everything else
    assert {k: v for k, v in b.regions.items() if k != "class_w"} == a.regions
    assert a.params == b.params and a.has_fused_step == b.has_fused_step
    (raw_a, geom_a), (raw_b, geom_b) = _arrays(a), _arrays(b)
    assert raw_a == raw_b      # Segs, Tasks, Phases byte for byte
    assert geom_b.pop("flags") == geom_a.pop("flags") | _lib.FLAG_CLASS_WEIGHTS and geom_a == geom_b


def test_flag_is_refused_where_it_cannot_work():
    with pytest.raises(ValueError, match="without source rows"):
        _lib.Plan(0, 4, 5, 512, 64, 12, ALL_FLAGS | _lib.FLAG_CLASS_WEIGHTS)
    with pytest.raises(ValueError, match="num_class > 64"):
        _lib.Plan(6, 4, 5, 512, 64, 65, ALL_FLAGS | _lib.FLAG_CLASS_WEIGHTS)


def test_hyper_struct_fits_its_region_and_matches_the_library():
    s = C.c_int32()
    _lib.lib().ta3n_debug_struct_sizes(None, None, None, None, C.byref(s))
    assert C.sizeof(_lib.Hyper) == s.value == 26 * 4 <= 128
    h = _lib.Hyper()
    assert h.class_w_off == 0 and tuple(h.dom_k) == (0.0, 0.0)      # zero-initialised: unweighted
    assert _lib.Hyper.class_w_off.offset == 23 * 4 and _lib.Hyper.dom_k.offset == 24 * 4      # behind the 24 dwords every caller knows
    a = _lib.Plan(6, 4, 5, 512, 64, 12, ALL_FLAGS)
    assert a.regions["hyper"][1] * 4 >= C.sizeof(_lib.Hyper)


def test_engine_refusals_fire_by_name_without_a_device(monkeypatch):
    ok = [1.0] * 12
    for kw, exc, text in ((dict(class_weights=ok[:11]), ValueError, "11 entries for 12 classes"),
                          (dict(class_weights=ok[:11] + [0.0]), ValueError, "class_weights must be positive"),
                          (dict(class_weights=ok[:11] + [float("nan")]), ValueError, "class_weights must be positive"),
                          (dict(domain_weights=(1.0, -1.0)), ValueError, "domain_weights must be positive"),
                          (dict(domain_weights=(1.0,)), ValueError, "domain_weights has 1 entries"),
                          (dict(class_weights=ok, process_group=object()), NotImplementedError, "class_weights together with world size")):
        with pytest.raises(exc, match=text):
            TrainEngine(6, 4, 5, 512, 64, 12, **kw)
    monkeypatch.setenv("TA3N_DDP_SELFTEST", "1")
    with pytest.raises(NotImplementedError, match="TA3N_DDP_SELFTEST"):
        TrainEngine(6, 4, 5, 512, 64, 12, class_weights=ok)
    assert weights_refusal(ok, wl.DOMAIN_W, num_class=12) == ""
    assert weights_refusal(None, wl.DOMAIN_W, num_class=12, world=8) == ""      # the domain factors are global: any world
    assert "world size 2" in weights_refusal(ok, None, num_class=12, world=2)


def test_set_hyper_forms_the_domain_factors_from_the_global_counts():
    """set_hyper on a stand-in with the attributes it reads: dom_k follows the step's global valid counts; no domain_weights attribute: zeros."""
    class Stand:
        pass
    s = Stand()
    s._hyper, s.Bs, s.Bt, s.T, s.world, s.rank, s.step_count = _lib.Hyper(), 6, 4, 5, 2, 0, 0
    s.momentum, s.weight_decay, s.clip, s.dropout_i, s.dropout_v = 0.9, 1e-4, 20.0, 0.5, 0.5
    TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.003, 1e-3, valid_source=5, valid_target=3, upload=False)
    assert tuple(s._hyper.dom_k) == (0.0, 0.0)
    s.domain_weights = wl.DOMAIN_W
    TrainEngine.set_hyper(s, [0.1, 0.2, 0.3], 0.003, 1e-3, valid_source=5, valid_target=3, upload=False)
    ks, kt = domain_factors(wl.DOMAIN_W, 10, 6)      # world 2: global counts
    assert tuple(s._hyper.dom_k) == (C.c_float(ks).value, C.c_float(kt).value)


def test_class_weights_of_the_cases_are_skewed_twenty_fold():
    for c in (12, 64):
        w = wl.class_weights(c)
        assert 15.0 <= max(w) / min(w) <= 25.0 and len(w) == c
    assert wl.class_weights(1) == [1.0]


@pytest.mark.parametrize("name", sorted(wl.CASES))
def test_cases_tell_weighted_from_unweighted(name):
    """On the reference alone: for each group of logit gradients the case's weights act on, the weighted and the unweighted gradients are
    more than 100 x the bound of the GPU test apart - a kernel that ignored a weight, or divided by n, cannot pass."""
    groups = wl.distinct_from_unweighted(name)
    assert groups
    for grp in groups:
        assert max(grp.values()) > 100 * wl.LOGIT_GRAD_REL_L2, (name, grp)


def test_fp32_restatement_against_float64():
    """The reference-only floor: the fp32 restatement of a weighted step against the float64 one, at the shape of the first case - far below
    the bounds the GPU test applies (ta3n_amd/tolerances.py)."""
    cfg, _, params, xs, xt, ys, ns, nt, cw, dw = wl.case_setup("trn_ragged")
    a = wl.reference_step(cfg, params, xs, xt, ys, ns, nt, cw, dw)
    b = wl.reference_step(cfg, params, xs, xt, ys, ns, nt, cw, dw, dtype=torch.float64)
    worst = max(wl.rel_l2(a["grads"][k], b["grads"][k]) for k in b["grads"])
    print(f"[weighted floor] fp32 vs float64 reference, trn_ragged: worst gradient rel. L2 {worst:.2e}, "
          f"loss {abs(a['parts']['loss'] - b['parts']['loss']):.2e}")
    assert worst <= 0.25 * wl.tol.F32_MASKED_GRAD_REL_L2
    assert abs(a["parts"]["loss"] - b["parts"]["loss"]) <= 1e-5 * max(1.0, abs(b["parts"]["loss"]))


@pytest.mark.parametrize("name", wl.FIXTURES)
def test_weighted_restatement_matches_the_reference_fixtures(name):
    """Ties tests/weighted_loss_cases.py to the reference itself: its weighted loss against the log line main.train printed with the two
    criteria built as main.py:160-167, 205-206 builds them, its clipped gradients and updated parameters against the recorded ones, step by
    step from the reference's own trajectory."""
    from golden_util import step_schedule
    from ta3n_amd.synthetic import synth_batch, synth_state
    g, c, cfg, cw, dw = wl.fixture_setup(name)
    assert cw is not None and max(cw) / min(cw) >= 15.0 and (dw is not None) == (name == "tiny_wcls_wdom")
    params = synth_state(orc_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    log = str(g.meta("log")).strip().splitlines()
    mom = None
    gamma = 0.0 if c["agg"] == "avgpool" else 0.003
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        ref = wl.reference_step(cfg, params, xs, xt, ys, st["n_src"], st["n_tgt"], cw, dw, gamma=gamma, lr=st["lr"], momentum=mom, clip=c["clip"])
        want = wl.log_numbers(log[s])
        got = dict(Loss=ref["parts"]["loss"], loss_c=ref["parts"]["loss_c"], loss_a=ref["parts"]["loss_a"], loss_e=ref["parts"].get("loss_e"))
        assert set(want) >= {"Loss", "loss_c", "loss_a"}
        for k, w in want.items():
            assert abs(got[k] - w) <= 1e-4 * max(1.0, abs(w)), (name, s, k, got[k], w)      # (the log prints four decimals)
        for k, v in ref["grads"].items():
            g.check(f"step{s}/clipped_grad/{k}", v * ref["clip_coef"], 2e-5, 2e-6, rms_atol=2e-5)
        for k, v in ref["params"].items():
            g.check(f"step{s}/param/{k}", v, 2e-5, 2e-6)
        params, mom = ref["params"], ref["momentum"]
    # ... and the weights do matter there: the unweighted criteria miss the logged loss by far more than the log's resolution
    xs, xt, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=c["xseed"])
    p0 = synth_state(orc_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    plain = wl.reference_step(cfg, p0, xs, xt, ys, c["Bs"], c["Bt"], None, None, gamma=gamma)
    assert abs(plain["parts"]["loss_c"] - wl.log_numbers(log[0])["loss_c"]) > 100 * 1e-4


def orc_shapes(cfg):
    return wl.param_shapes(cfg)
