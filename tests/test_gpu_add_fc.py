"""--add_fc 2 / 3 on the MI355X (models.py:145-153, 581-603): the engine's fused step and unfused lists against fixtures the reference
produced (tests/golden/make_golden_add_fc.py), the bf16 arithmetics against the fp32 result, the K-step call, the per-layer dropout
streams, the module path, main.py's fast path and train_ddp.py's checkpoints."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["tiny_addfc2", "tiny_addfc3_clip", "tiny_avgpool_addfc2_da", "tiny_avgpool_addfc2", "headline_addfc2"]
RTOL, ATOL = tol.F32_RTOL, tol.F32_ATOL


def _case(name):
    g = Golden(name)
    c = case_config(g)
    c["add_fc"] = int(g.meta("add_fc"))
    avg = c["agg"] == "avgpool"
    if not avg:
        kw, beta, gamma = {}, [0.75, 0.75, 0.5], 0.003
    elif c["place_adv"] is None:
        kw, beta, gamma = dict(aggregation="avgpool", flags=0), [0.0, 0.0, 0.0], 0.0
    else:
        kw, beta, gamma = dict(aggregation="avgpool", flags=flags_from_options(c["place_adv"], "none", "none", "RevGrad", "uSv")), [0.75, 0.75, 0.5], 0.0
    return g, c, kw, beta, gamma


def _engine(c, kw, **more):
    from ta3n_amd.engine import TrainEngine
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], dropout_i=more.pop("dropout_i", 0.0),
                      dropout_v=more.pop("dropout_v", 0.0), clip=c["clip"], add_fc=c["add_fc"], **kw, **more)
    shapes = {n: s for n, _, s, _ in eng.plan.params}
    eng.load_state(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    return eng


def _layers(eng, c):
    """[F_1, ..., F_L] of the last forward, [B, T, F] each."""
    B, T, F, L = c["Bs"] + c["Bt"], c["T"], eng.F, c["add_fc"]
    return [eng.region(f"F_l{k}", (B, T, F)) for k in range(1, L)] + [eng.region("F1", (B, T, F))]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_train_steps_match_reference_golden(name, fused):
    g, c, kw, beta, gamma = _case(name)
    eng = _engine(c, kw)
    assert eng.add_fc == c["add_fc"] and eng.plan.has_fused_step
    live = set(eng.live_names())
    assert live == set(str(k) for k in g.meta("live"))
    B, Bs, T = c["Bs"] + c["Bt"], c["Bs"], c["T"]
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, yt = synth_batch(c["C"], T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.set_hyper(beta, gamma, st["lr"], train=True, valid_source=st["n_src"], valid_target=st["n_tgt"])
        if fused:
            eng.fused_step()
        else:
            eng.forward()
        if s == 0:
            o = {k: v.detach().cpu() for k, v in eng.outputs().items()}
            layers = [f.detach().cpu() for f in _layers(eng, c)]
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", o["out"][sl], 0, tol.LOGIT_ATOL, "class logits")
                g.check(f"fwd/feat_{dom}_v", o["feat_v"][sl], RTOL, ATOL)
                g.check(f"fwd/feat_{dom}_f1", o["feat_f1"][sl], RTOL, ATOL)
                for k, f in enumerate(layers, 1):
                    g.check(f"fwd/feat_{dom}_l{k}", f[sl], RTOL, ATOL)
                if "pred_frm" in o and g.has(f"fwd/pd_{dom}_frm"):
                    g.check(f"fwd/pd_{dom}_frm", o["pred_frm"][sl], 0, tol.LOGIT_ATOL)
                    g.check(f"fwd/pd_{dom}_vid", o["pred_vid"][sl], 0, tol.LOGIT_ATOL)
        if not fused:
            eng.loss()
            eng.backward()
        raw = {k: v.clone() for k, v in eng.param_views(eng.G).items()}
        eng.sgd_step_fused() if fused else eng.sgd_step()
        torch.cuda.synchronize()
        coef = eng.region("grad_norm")[1].item()
        if name == "tiny_addfc3_clip":
            assert coef < 1.0
        new = eng.param_views()
        l2s = {}
        for k in new:
            if k in live:
                if s == 0:
                    g.check(f"step{s}/clipped_grad/{k}", raw[k].cpu() * coef, 1e-3, 2e-5, rms_atol=1e-2)
                l2s[k] = g.rel_l2(f"step{s}/clipped_grad/{k}", raw[k].cpu() * coef)
            g.check(f"step{s}/param/{k}", new[k].cpu(), RTOL, ATOL)
        bound = tol.F32_GRAD_REL_L2 * (1 if s == 0 else tol.GOLDEN_DRIFT_FACTOR)
        worst = max(l2s, key=l2s.get)
        assert l2s[worst] <= bound, f"step {s} {worst}: relative L2 {l2s[worst]:.3e} > {bound:.1e}"


def _one_step(c, kw, beta, gamma, fused=True, **more):
    eng = _engine(c, kw, **more)
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.set_hyper(beta, gamma, st["lr"], train=True)
    if fused:
        eng.fused_step()
    else:
        eng.forward(); eng.loss(); eng.backward()
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("arith", ["bf16", "bf16_store"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["tiny_addfc2", "tiny_avgpool_addfc2_da", "tiny_avgpool_addfc2", "headline_addfc2"])
def test_bf16_arithmetics_hold_the_bf16_bounds(name, fused, arith):
    """bf16 MFMA operands (and bf16 twins with bf16_store) at add_fc 2.  Small cases: against the SAME plan executed with numpy in the
    same arithmetic (tests/plan_interp.py: bf16-rounded operands, fp64 sums), held to the bf16 contract's bounds (BF16_*).  Headline
    shape: against the fp32 HIP step on the same inputs, held to the bounds on the distance from fp32 (BF16_REF_*)."""
    _, c, kw, beta, gamma = _case(name)
    got = _one_step(c, kw, beta, gamma, fused, bf16=True, bf16_store=(arith == "bf16_store"))
    live = got.live_names()
    b = got.param_views(got.G)
    y16 = got.outputs()["out"].double().cpu()
    if name.startswith("headline"):
        ref = _one_step(c, kw, beta, gamma, fused)
        y = ref.outputs()["out"].double().cpu()
        a = {k: v.double().cpu() for k, v in ref.param_views(ref.G).items()}
        logit_bound, grad_bound, median_bound = tol.BF16_REF_LOGIT_REL_RMS, tol.BF16_REF_GRAD_REL_L2, tol.BF16_REF_GRAD_REL_L2_MEDIAN
    else:
        from plan_interp import Interp
        from test_plan_cpu import make_hyper
        it = Interp(got.plan)
        it.set_params(synth_state({n: s for n, _, s, _ in got.plan.params}, seed=c["wseed"], scale=c["wscale"]))
        st = step_schedule(c)[0]
        xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:c["Bs"]] = ys.numpy()
        it.hy = make_hyper(c, dict(n_src=c["Bs"], n_tgt=c["Bt"]), c["T"], st["lr"])
        it.hy["beta"], it.hy["gamma"] = list(beta), gamma
        it.G[:] = 0
        for grp in ((4,) if fused else (0, 1, 2)):
            it.run_group(grp)
        y = torch.from_numpy(it.r(it.g.o_Y, (c["Bs"] + c["Bt"], c["C"])).copy())
        a = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in it.get_params(it.G).items()}
        logit_bound, grad_bound, median_bound = tol.BF16_LOGIT_REL_RMS, tol.BF16_GRAD_REL_L2, tol.BF16_GRAD_REL_L2_MEDIAN
    assert (y16 - y).abs().max().item() <= logit_bound * y.pow(2).mean().sqrt().item()
    rel = {}
    for k in live:
        r, x = a[k].reshape(-1).double(), b[k].reshape(-1).double().cpu()
        rel[k] = (x - r).norm().item() / max(r.norm().item(), 1e-30)
    worst = max(rel, key=rel.get)
    assert rel[worst] <= grad_bound, (worst, rel[worst])
    assert float(torch.tensor(list(rel.values())).median()) <= median_bound, rel


@pytest.mark.parametrize("arith", ["f32", "bf16"])
def test_k_step_call_is_bit_identical_to_single_steps(arith):
    """ta3n_train_steps with K = 3 against three single fused steps with the whole update in between (train_step), against the
    pipelined single steps (the update opens the next step; W_2 is updated by the side workgroups of its first launch, before the
    second launch reads it) and the deferred ones (side-stream update joined after the first launch): bit for bit."""
    _, c, kw, _, _ = _case("tiny_addfc2")
    more = dict(bf16=True, bf16_store=True) if arith == "bf16" else {}
    sched = [([0.1 * (i + 1), 0.75, 0.5], 0.003, 1e-3 * (i + 1)) for i in range(3)]
    res = []
    for mode in ("plain", "pipelined", "deferred", "one_call"):
        eng = _engine(c, kw, dropout_i=0.5, dropout_v=0.5, **more)
        xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=11)
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        if mode == "one_call":
            eng.train_steps(sched)
        else:
            for i, (b, gm, lr) in enumerate(sched):
                getattr(eng, {"plain": "train_step", "pipelined": "train_step_pipelined", "deferred": "train_step_deferred"}[mode])(b, gm, lr, seed=i)
        eng.flush()
        torch.cuda.synchronize()
        assert eng.step_count == len(sched)
        res.append((mode, eng.P.clone(), eng.M.clone(), eng.region("losses")[:6].clone()))
    for mode, *other in res[1:]:
        assert all(torch.equal(x, y) for x, y in zip(res[0][1:], other)), mode
    assert torch.isfinite(res[0][1]).all()


@pytest.mark.parametrize("fused", [False, True])
def test_each_layer_draws_its_own_dropout_mask(fused):
    """p = 0.5, train mode: every layer keeps ~1 - p of its active units, the masks of layers 1 and 2 agree at the rate of independent
    masks, and the backward zeroes exactly the entries the forward dropped (the masks are re-derived from the stored activations)."""
    _, c, kw, beta, gamma = _case("headline_addfc2")
    eng = _one_step(c, kw, beta, gamma, fused, dropout_i=0.5, dropout_v=0.5)
    B, T = c["Bs"] + c["Bt"], c["T"]
    F1, F2 = (f.reshape(B * T, -1).double() for f in _layers(eng, c))
    P = eng.param_views()
    X = eng.X.double()
    Z1 = X @ P["fc_feature_shared_source.weight"].double().t() + P["fc_feature_shared_source.bias"].double()
    Z2 = F1 @ P["fc_feature_shared_2_source.weight"].double().t() + P["fc_feature_shared_2_source.bias"].double()
    act1, act2 = Z1 > 1e-4, Z2 > 1e-4            # (away from the ReLU kink: fp32 vs fp64 round-off)
    keep1, keep2 = F1 > 0, F2 > 0
    r1 = keep1[act1].double().mean().item()
    r2 = keep2[act2].double().mean().item()
    assert abs(r1 - 0.5) < 0.02 and abs(r2 - 0.5) < 0.02, (r1, r2)
    both = act1 & act2
    agree = (keep1[both] == keep2[both]).double().mean().item()
    assert both.sum().item() > 10000 and abs(agree - 0.5) < 0.02, agree      # a repeated mask would agree everywhere
    # ... and exactly: each layer's pattern is the host's restatement of the stream at that layer's id offset (tests/dropout_masks.py;
    # the seeds of step 0, which set_hyper took) - zero where it drops, nonzero where it keeps an active unit
    from dropout_masks import check_frame_pattern, dropout_masks
    from ta3n_amd.engine import dropout_seeds
    for k, (Fk, Zk) in enumerate(((F1, Z1), (F2, Z2)), 1):
        keep = torch.cat(dropout_masks(*dropout_seeds(0, 0), 0.5, 0.5, c["Bs"], c["Bt"], T, eng.F, 256, layer=k)["keep_i"])
        check_frame_pattern(Fk.cpu(), Zk.cpu(), keep, f"layer {k}")
    # kept units carry the 1 / (1 - p) scale
    assert torch.allclose(F1[act1 & keep1], 2 * Z1[act1 & keep1], rtol=1e-3, atol=1e-5)
    gZ1, gZ2 = eng.region("gZ_l1", (B * T, -1)), eng.region("gZ1", (B * T, -1))
    for F, gZ in ((F1, gZ1), (F2, gZ2)):
        assert torch.all(gZ[F <= 0] == 0)
        assert (gZ[F > 0] != 0).double().mean().item() > 0.99


def _model(c, add_fc):
    from ta3n_amd.models import VideoModel
    arch = "resnet18" if c["D"] == 512 else "resnet101"
    avg = c["agg"] == "avgpool"
    m = VideoModel(c["C"], "video", "avgpool" if avg else "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model=arch,
                   fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0, partial_bn=False, verbose=False, add_fc=add_fc,
                   use_attn="none" if avg else "TransAttn")
    sd = m.state_dict()
    sd.update(synth_state({k: tuple(v.shape) for k, v in sd.items()}, seed=c["wseed"], scale=c["wscale"]))
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("name", ["tiny_addfc2", "tiny_addfc3_clip"])
def test_module_path_matches_the_fused_step(name):
    """VideoModel(add_fc=k) forward + the torch loss assembly (oracle.total_loss, main.py:439-562) + autograd on the unfused lists:
    the feature list is [logits, V, F_k, ..., F_1], and the gradients equal the engine's fused step on the same batch."""
    from oracle import ta3n_oracle as orc
    g, c, kw, beta, gamma = _case(name)
    model = _model(c, c["add_fc"])
    model.train()
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    out = model(xs, xt, beta, 0, True, False)
    feat_s, feat_t = out[4], out[9]
    L = c["add_fc"]
    assert len(feat_s) == len(feat_t) == L + 2
    for k in range(1, L + 1):
        g.check(f"fwd/feat_s_l{k}", feat_s[L + 2 - k], RTOL, ATOL)
        g.check(f"fwd/feat_t_l{k}", feat_t[L + 2 - k], RTOL, ATOL)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"])
    loss, _ = orc.total_loss(dict(out=out[1], pred_domain=out[3]), dict(out=out[6], pred_domain=out[8]), ys.cuda(), gamma, cfg,
                             c["Bs"], c["Bt"])
    loss.backward()
    eng = _one_step(c, kw, beta, gamma, True)
    G = eng.param_views(eng.G)
    live = set(eng.live_names())
    for k, p in model.named_parameters():
        assert (p.grad is not None) == (k in live), k
        if k in live:
            want = G[k].double()
            assert (p.grad.double() - want).norm().item() <= tol.F32_GRAD_REL_L2 * want.norm().item(), k


def test_main_fast_path_logs_what_the_module_path_logs(tmp_path):
    from fixture_t7 import make_dataset
    data = make_dataset(str(tmp_path / "data"))
    TA3N = ["--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
            "--add_loss_DA", "attentive_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.003", "--lr_adaptive", "dann"]
    COMMON = ["--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0.5", "--dropout_v", "0.5", "-b", "8", "6", "8",
              "--lr", "0.03", "--epochs", "2", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn", "--add_fc", "2"]
    outs, cks = [], []
    for fast in ("1", "0"):
        exp = str(tmp_path / f"exp{fast}")
        cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *TA3N, *COMMON,
               "--save_best_log", str(tmp_path / f"best{fast}.log")]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
        cks.append(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False))
    assert len(outs[0]) == len(outs[1]) == 6
    num = re.compile(r"(Loss|loss_c|loss_a|loss_e|lr:) (-?[0-9.]+)")
    for a, b in zip(*outs):
        fa, fb = num.findall(a), num.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb]
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-3 * max(1.0, abs(float(y))), (k, x, y, a, b)
    sa, sb = cks[0]["state_dict"], cks[1]["state_dict"]
    assert set(sa) == set(sb) and "module.fc_feature_shared_2_source.weight" in sa
    for k in sa:
        assert torch.allclose(sa[k].float(), sb[k].float(), rtol=2e-3, atol=2e-5), k


def test_train_ddp_checkpoint_loads_strictly(tmp_path):
    """train_ddp.py --add_fc 2: the checkpoint holds the reference's state_dict keys (fixture) and loads with strict=True into VideoModel;
    the tester (test_models.py --add_fc 2) evaluates it."""
    from ta3n_amd.models import VideoModel
    g = Golden("tiny_addfc2")
    exp = str(tmp_path / "exp") + "/"
    cmd = [sys.executable, os.path.join(ROOT, "train_ddp.py"), "no_class_file", "RGB", "a", "b", "c", "--synthetic", "24", "16",
           "--frame_aggregation", "trn-m", "--baseline_type", "video", "--arch", "resnet18", "--num_segments", "5", "--add_fc", "2",
           "--fc_dim", "64", "-b", "6", "4", "6", "--lr", "0.01", "--lr_adaptive", "dann", "--use_target", "uSv", "--adv_DA", "RevGrad",
           "--use_attn", "TransAttn", "--add_loss_DA", "attentive_entropy", "--place_adv", "Y", "Y", "Y", "--beta", "0.75", "0.75", "0.5",
           "--gamma", "0.003", "--print_freq", "1", "--epochs", "1", "--exp_path", exp, "--save_model"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "nan" not in r.stdout.lower()
    ck = torch.load(exp + "RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False)
    sd = {k[len("module."):]: v for k, v in ck["state_dict"].items()}
    assert set(sd) == set(str(k) for k in g.meta("state_keys"))
    net = VideoModel(12, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, add_fc=2, verbose=False)
    net.load_state_dict(sd, strict=True)
    names = [n for n, _ in net.named_parameters()]
    assert len(ck["optimizer"]["param_groups"][0]["params"]) == len(names) == len(g.meta("param_keys"))
    assert names == [str(k) for k in g.meta("param_keys")]
    net = net.cuda().eval()
    x = torch.randn(4, 5, 512).abs()
    with torch.no_grad():
        out = net(x, x, [0, 0, 0], 0, False, False)
    assert torch.isfinite(out[6]).all() and len(out[9]) == 4
