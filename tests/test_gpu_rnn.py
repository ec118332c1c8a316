"""GPU: --frame_aggregation rnn (reference models.py:202-215, 392-422).  The TA3N_AGG_RNN plan through the C ABI against the fixtures
the reference wrote (tests/golden/make_golden_rnn.py) - forward regions, every stored gradient entry and every parameter after every
step - and, with dropout 0.5 / 0.5 on the kernels' own masks, against the float64 restatement (tests/rnn_reference.py); VideoModel's
forward and autograd backward; main.py and test_models.py end to end.  Every measured figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rnn_reference as rr
from dropout_masks import dropout_masks
from fixture_t7 import make_dataset
from golden_util import step_schedule
from ta3n_amd import _lib, tolerances as tol
from ta3n_amd.models import VideoModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTUM, WEIGHT_DECAY = 0.9, 1e-4


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Raw:
    """The flat buffers of one plan and the C entry points on them (TrainEngine does not take the recurrent aggregation)."""

    def __init__(self, plan, state):
        self.plan, self.L = plan, _lib.lib()
        self.P, self.G, self.M = (torch.zeros(plan.param_floats, device="cuda") for _ in range(3))
        self.ws = torch.zeros(plan.ws_floats, device="cuda")
        _lib.check(self.L.ta3n_init_workspace(plan.handle, self.ws.data_ptr(), _stream()), "ta3n_init_workspace")
        for name, off, shape, _ in plan.params:
            self.P[off:off + state[name].numel()] = state[name].reshape(-1).float().cuda()
        self.X = None

    def region(self, name, shape=None):
        off, n = self.plan.region(name)
        v = self.ws[off:off + n]
        return v if shape is None else v[:int(np.prod(shape))].view(shape)

    def views(self, buf):
        return {name: buf[off:off + int(np.prod(shape))].view(shape) for name, off, shape, _ in self.plan.params}

    def set_step(self, x, labels, c, st, lr, train=1, p_drop=(0.0, 0.0), seeds=(1, 2), norm=None):
        self.X = x.reshape(-1, x.shape[-1]).float().cuda().contiguous()
        self.region("labels").view(torch.int32)[:labels.numel()] = labels.to(torch.int32).cuda()
        if c.get("class_w") is not None:
            self.region("class_w")[:len(c["class_w"])] = torch.tensor(c["class_w"]).cuda()
        h = _lib.Hyper()
        h.beta[0], h.beta[1], h.beta[2] = c["beta"]
        h.gamma, h.lr, h.momentum, h.weight_decay, h.clip = 0.0, float(lr), MOMENTUM, WEIGHT_DECAY, float(c["clip"])
        h.p_drop_i, h.p_drop_v = p_drop
        h.seed_i, h.seed_v = seeds
        for k, v in (norm or rr.normalisers(c, st)).items():
            setattr(h, k, v)
        h.valid_source, h.valid_target, h.train = st["n_src"], st["n_tgt"], train
        _lib.check(self.L.ta3n_set_hyper(self.plan.handle, self.ws.data_ptr(), C.byref(h), _stream()), "ta3n_set_hyper")

    def forward(self):
        _lib.check(self.L.ta3n_forward(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.ws.data_ptr(), _stream()), "ta3n_forward")

    def unfused(self):
        self.forward()
        _lib.check(self.L.ta3n_loss(self.plan.handle, self.ws.data_ptr(), _stream()), "ta3n_loss")
        _lib.check(self.L.ta3n_backward(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.ws.data_ptr(), _stream()),
                   "ta3n_backward")

    def train_step(self):
        _lib.check(self.L.ta3n_train_step(self.plan.handle, self.X.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.ws.data_ptr(), _stream()),
                   "ta3n_train_step")

    def update(self, fused):
        fn = self.L.ta3n_sgd_step_fused if fused else self.L.ta3n_sgd_step
        _lib.check(fn(self.plan.handle, self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.ws.data_ptr(), _stream()), "sgd step")


def _max_scale(g, key, t):
    """max |t - ref| / max |ref| over the stored entries of record `key` (Golden.rel_l2's entries)."""
    a = t.detach().double().cpu().numpy().reshape(-1)
    if key + "#full" in g.z:
        ref = g.z[key + "#full"].astype(np.float64).reshape(-1)
    else:
        from golden_util import N_SAMP, sample_index
        ref = np.concatenate([g.z[key + "#head"], g.z[key + "#samp"]]).astype(np.float64)
        a = np.concatenate([a[:N_SAMP], a[sample_index(a.size)]])
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if ref.size else 0.0


def _rel_l2(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).norm() / max(float(want.norm()), 1e-300))


@pytest.mark.parametrize("name", rr.FIXTURES)
def test_c_abi_matches_reference_golden(name):
    g, c = rr.setup(name)
    T, B, Bs, F = c["T"], c["Bs"] + c["Bt"], c["Bs"], c["fc_dim"]
    plan = rr.make_plan(c)
    shapes = {n: s for n, _, s, _ in plan.params}
    raw = Raw(plan, rr.state_of(shapes, c))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = rr.step_batch(c, st)
        raw.set_step(torch.cat((xs, xt)), labels, c, st, st["lr"])
        if s == 0:
            raw.forward()
            torch.cuda.synchronize()
            o = dict(out=raw.region("Y", (B, c["C"])), v=raw.region("V", (B, F)), f1=raw.region("F1", (B, T, F)), vid=raw.region("Pv", (B, 2)),
                     frm=raw.region("Pf", (B, T, 2)))
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", o["out"][sl], 0, tol.LOGIT_ATOL, "class logits")
                g.check(f"fwd/feat_{dom}_v", o["v"][sl], tol.F32_RTOL, tol.F32_ATOL)
                g.check(f"fwd/feat_{dom}_f1", o["f1"][sl], tol.F32_RTOL, tol.F32_ATOL)
                if c["place_adv"] and (c["place_adv"][1] == "Y" or c["place_adv"][0] == "Y"):
                    g.check(f"fwd/pd_{dom}_vid", o["vid"][sl], 0, tol.LOGIT_ATOL, "video domain logits")
                if c["place_adv"] and c["place_adv"][2] == "Y":
                    g.check(f"fwd/pd_{dom}_frm", o["frm"][sl], 0, tol.LOGIT_ATOL, "frame domain logits")
        fused = s % 2 == 0                       # both launch lists: ta3n_train_step and ta3n_forward / ta3n_loss / ta3n_backward
        raw.G.zero_()
        raw.train_step() if fused else raw.unfused()
        torch.cuda.synchronize()
        grads = {k: v.clone() for k, v in raw.views(raw.G).items()}
        gz1 = raw.region("gZ1", (B, T, F)).clone()
        raw.update(fused)
        torch.cuda.synchronize()
        coef = float(raw.region("grad_norm")[1])
        drift = tol.GOLDEN_DRIFT_FACTOR if s >= 1 else 1.0
        rels = {k: g.rel_l2(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) for k in sorted(live)}
        worst = max(rels, key=rels.get)
        print(f"[rnn golden] {name} step {s} ({'fused' if fused else 'unfused'}): gradient rel. L2 median {np.median(list(rels.values())):.2e}, "
              f"worst {rels[worst]:.2e} ({worst}); rnn.*: " + ", ".join(f"{rels[k]:.1e}" for k in sorted(rels) if k.startswith("rnn.")))
        assert np.median(list(rels.values())) <= tol.F32_GRAD_REL_L2_MEDIAN * drift
        for k, v in rels.items():
            assert v <= tol.F32_GRAD_REL_L2 * drift, (k, v)
            assert _max_scale(g, f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) <= tol.F32_GRAD_MAX_SCALE * drift, k
        for k, v in raw.views(raw.P).items():
            g.check(f"step{s}/param/{k}", v.cpu(), tol.F32_RTOL, tol.F32_ATOL)
        # exact statements
        if name == "tiny_rnn_lstm_ts1":
            assert not bool(grads["rnn.weight_hh_l0"].any()) and "rnn.weight_hh_l0" in live
        if c["rnn_cell"] == "LSTM":
            assert torch.equal(grads["rnn.bias_ih_l0"], grads["rnn.bias_hh_l0"])
        if name == "tiny_rnn_gru_T7":
            assert not bool(gz1[:, 5:, :].any()) and bool(gz1[:, :5, :].any())
    if name == "tiny_rnn_lstm_ts1":
        assert not torch.equal(raw.views(raw.P)["rnn.weight_hh_l0"].cpu(), rr.state_of(shapes, c)["rnn.weight_hh_l0"])


@pytest.mark.parametrize("cell,F,T,n_ts,Bs,Bt,Cn", [("LSTM", 64, 8, 5, 6, 5, 6), ("GRU", 20, 3, 5, 5, 4, 7)])
def test_dropout_on_the_kernels_own_masks_against_float64(cell, F, T, n_ts, Bs, Bt, Cn):
    """dropout 0.5 / 0.5: F1 and Vd carry the masks of tests/dropout_masks.py (dropout_v: element b F + k on the last hidden state);
    forward tensors and every gradient against the float64 restatement on those masks."""
    D, place_adv = 512, ("N", "Y", "Y")
    c = dict(Bs=Bs, Bt=Bt, T=T, D=D, fc_dim=F, C=Cn, rnn_cell=cell, n_ts=n_ts, wseed=71, wscale="trained", clip=0.0, beta=rr.BETA, class_w=None,
             flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME)
    plan = rr.make_plan(c)
    state = rr.state_of({n: s for n, _, s, _ in plan.params}, c)
    raw = Raw(plan, state)
    xs, xt, ys, yt = rr.synth_batch(Cn, T, D, Bs, Bt, seed=72)
    st = dict(n_src=Bs, n_tgt=Bt)
    seeds = (12345, 67890)
    raw.set_step(torch.cat((xs, xt)), torch.cat((ys, yt)), c, st, 1e-3, p_drop=(0.5, 0.5), seeds=seeds)
    raw.train_step()
    torch.cuda.synchronize()
    m = dropout_masks(seeds[0], seeds[1], 0.5, 0.5, Bs, Bt, T, F, F)
    mask_i = torch.cat(m["drop_i"]).view(Bs + Bt, T, F)
    mask_v = torch.cat(m["drop_v"])
    fwd, grads, _ = rr.step(state, torch.cat((xs, xt)), torch.cat((ys, yt)), Bs, Bs, Bt, cell, n_ts, place_adv, mask_i=mask_i, mask_v=mask_v)
    B = Bs + Bt
    got = dict(F1=raw.region("F1", (B, T, F)), V=raw.region("V", (B, F)), Y=raw.region("Y", (B, Cn)), Pv=raw.region("Pv", (B, 2)),
               Pf=raw.region("Pf", (B, T, 2)))
    assert not bool(got["F1"].cpu()[mask_i == 0].any())                       # what dropout_i dropped is exactly zero
    vd = raw.region("Vd", (B, F)).cpu().double()
    assert torch.equal(vd == 0, mask_v == 0) and torch.allclose(vd, fwd["V"] * mask_v, rtol=tol.F32_RTOL, atol=tol.F32_ATOL)
    for k in ("F1", "V"):
        assert torch.allclose(got[k].cpu().double(), fwd[k], rtol=tol.F32_RTOL, atol=tol.F32_ATOL), k
    for k in ("Y", "Pv", "Pf"):
        err = float((got[k].cpu().double() - fwd[k]).abs().max())
        print(f"[rnn dropout] {cell} {k}: max |error| {err:.2e}")
        assert err <= tol.LOGIT_ATOL, k
    gv = raw.views(raw.G)
    rels = {k: _rel_l2(gv[k], w) for k, w in grads.items()}
    print(f"[rnn dropout] {cell} F {F} T {T}: gradient rel. L2 median {np.median(list(rels.values())):.2e}, worst {max(rels.values()):.2e} "
          f"({max(rels, key=rels.get)})")
    assert set(rels) == {n for n, _, _, lv in plan.params if lv}
    assert np.median(list(rels.values())) <= tol.F32_GRAD_REL_L2_MEDIAN and max(rels.values()) <= tol.F32_GRAD_REL_L2


def _module(c, val_T=None):
    m = VideoModel(c["C"], "video", "rnn", "RGB", train_segments=c["T"], val_segments=val_T or c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   dropout_i=0.0, dropout_v=0.0, use_attn="none", verbose=False, rnn_cell=c["rnn_cell"], n_ts=c["n_ts"])
    sd = m.state_dict()
    sd.update(rr.state_of({k: tuple(v.shape) for k, v in sd.items()}, c))
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("name", ["tiny_rnn_lstm_T5", "tiny_rnn_gru_T7"])
def test_module_path_forward_and_autograd_backward(name):
    """VideoModel(frame_aggregation='rnn'): the 10-tuple against the fixture's forward records; the loss assembled by the caller
    (main.py:439-451, 508-538) plus a gradient of the caller's own at feat[1] (gV_ext), every parameter gradient against the float64
    restatement with the same extra term."""
    import torch.nn.functional as Fn
    g, c = rr.setup(name)
    Bs, Bt, T = c["Bs"], c["Bt"], c["T"]
    m = _module(c)
    m.train()
    st = step_schedule(c)[0]
    xs, xt, labels = rr.step_batch(c, st)
    out = m(xs, xt, rr.BETA, 0, True, False)
    attn_s, out_s, _, pd_s, feat_s, attn_t, out_t, _, pd_t, feat_t = out
    g.check("fwd/out_s", out_s, 0, tol.LOGIT_ATOL); g.check("fwd/out_t", out_t, 0, tol.LOGIT_ATOL)
    g.check("fwd/attn_s", attn_s, tol.F32_RTOL, tol.F32_ATOL); g.check("fwd/attn_t", attn_t, tol.F32_RTOL, tol.F32_ATOL)
    for i, nm in enumerate(("rel", "vid", "frm")):      # (the module path computes every discriminator: the caller assembles the loss)
        if True:
            g.check(f"fwd/pd_s_{nm}", pd_s[i], 0, tol.LOGIT_ATOL); g.check(f"fwd/pd_t_{nm}", pd_t[i], 0, tol.LOGIT_ATOL)
    assert torch.equal(pd_s[0], pd_s[1]) and torch.equal(feat_s[0], out_s) and torch.equal(attn_t, feat_t[1][:, 0])
    for i, nm in enumerate(("y", "v", "f1")):
        g.check(f"fwd/feat_s_{nm}", feat_s[i], tol.F32_RTOL, tol.LOGIT_ATOL if i == 0 else tol.F32_ATOL)
        g.check(f"fwd/feat_t_{nm}", feat_t[i], tol.F32_RTOL, tol.LOGIT_ATOL if i == 0 else tol.F32_ATOL)
    place = ("N", "Y", "Y")                                     # the caller decides: video and frame level here, whatever the fixture trained
    wv = torch.linspace(-1, 1, c["fc_dim"]).cuda()              # the caller's own term on feat[1]
    loss = Fn.cross_entropy(out_s, labels[:Bs].cuda())
    for lvl in (1, 2):
        ps, pt = pd_s[lvl].reshape(-1, 2), pd_t[lvl].reshape(-1, 2)
        lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long().cuda()
        loss = loss + Fn.cross_entropy(torch.cat((ps, pt)), lab)
    loss = loss + 0.1 * ((feat_s[1] * wv).sum() + (feat_t[1] * wv).sum())
    loss.backward()
    P = {k: v.detach().double() for k, v in rr.state_of({k: tuple(v.shape) for k, v in m.state_dict().items()}, c).items()}
    x = torch.cat((xs, xt))
    _, grads, _ = _step_with_extra(P, x, labels, Bs, Bt, c, place, wv.cpu().double())
    named = dict(m.named_parameters())
    assert {k for k, v in named.items() if v.grad is not None} == set(grads)
    rels = {k: _rel_l2(named[k].grad, w) for k, w in grads.items()}
    print(f"[rnn module] {name}: gradient rel. L2 median {np.median(list(rels.values())):.2e}, worst {max(rels.values()):.2e} ({max(rels, key=rels.get)})")
    assert np.median(list(rels.values())) <= tol.F32_GRAD_REL_L2_MEDIAN and max(rels.values()) <= tol.F32_GRAD_REL_L2
    assert named["bn_before_rnn.weight"].grad is None and named["bn_after_rnn.bias"].grad is None


def _step_with_extra(P, x, labels, Bs, Bt, c, place, wv):
    """rr.step with 0.1 <V, wv> summed over all videos added to the loss: by linearity, the gradients of the two parts add."""
    import torch.nn.functional as Fn
    fwd, grads, _ = rr.step(P, x, labels, Bs, Bs, Bt, c["rnn_cell"], c["n_ts"], place)
    Q = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    F1 = torch.relu(x.double() @ Q["fc_feature_shared_source.weight"].t() + Q["fc_feature_shared_source.bias"])
    Xp = F1[:, rr.slot_windows(c["T"], c["n_ts"]), :].max(2).values
    F_ = F1.shape[-1]
    rnn = (torch.nn.LSTM if c["rnn_cell"] == "LSTM" else torch.nn.GRU)(F_, F_, 1, batch_first=True).double()
    V = torch.func.functional_call(rnn, {k[4:]: v for k, v in Q.items() if k.startswith("rnn.")}, (Xp,))[0][:, -1, :]
    (0.1 * (V * wv).sum()).backward()
    for k, v in Q.items():
        if v.grad is not None:
            grads[k] = grads[k] + v.grad if k in grads else v.grad
    return fwd, grads, None


def test_module_path_validates_on_another_segment_count():
    """tiny_rnn_eval: trained on 5 segments, validated on 25 (len_ts 5) - a second plan; main.validate's call (main.py:707)."""
    g, c = rr.setup("tiny_rnn_eval")
    val_T = int(g.meta("val_T"))
    m = _module(c, val_T)
    m.eval()
    xv, _, _, _ = rr.synth_batch(c["C"], val_T, c["D"], c["Bs"], c["Bt"], seed=c["xseed"] + 7)
    with torch.no_grad():
        ev = m(xv, xv, [0, 0, 0], 0, False, False)
    g.check("eval/out_t", ev[6], 0, tol.LOGIT_ATOL)
    g.check("eval/feat_t_v", ev[9][1], tol.F32_RTOL, tol.F32_ATOL)
    assert ev[9][2].shape == (c["Bs"], val_T, c["fc_dim"]) and len(m._plans) == 1
    m.train()
    xs, xt, _ = rr.step_batch(c, step_schedule(c)[0])
    g.check("fwd/out_s", m(xs, xt, rr.BETA, 0, True, False)[1], 0, tol.LOGIT_ATOL)
    assert len(m._plans) == 2


def test_main_trains_validates_checkpoints_and_the_tester_reads_it(tmp_path):
    """main.py --frame_aggregation rnn --rnn_cell GRU --use_attn none for two epochs on the tests/fixture_t7.py dataset: logs, validation,
    best checkpoint; the loss is finite and falls; test_models.py on the checkpoint reproduces the validation accuracy."""
    data = make_dataset(str(tmp_path / "data"))
    exp = str(tmp_path / "exp")
    opts = ["--baseline_type", "video", "--frame_aggregation", "rnn", "--rnn_cell", "GRU", "--n_ts", "5", "--use_target", "uSv", "--adv_DA", "RevGrad",
            "--use_attn", "none", "--add_loss_DA", "none", "--beta", "0.75", "0.75", "0.5", "--place_adv", "N", "Y", "Y", "--lr_adaptive", "dann",
            "--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0", "--dropout_v", "0", "-b", "8", "6", "8",
            "--lr", "0.03", "--epochs", "2", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn", "--save_best_log", str(tmp_path / "best.log")]
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *opts]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = exp + "/RGB/"
    for f in ("train.log", "val.log", "checkpoint.pth.tar", "model_best.pth.tar"):
        assert os.path.exists(out + f), f
    lines = [ln for ln in open(out + "train.log") if ln.startswith("Train:")]
    assert len(lines) == 6
    # the running average of the total loss at the end of each epoch (the figure in parentheses): the same three batches both times
    first, last = (float(ln.split("Loss")[1].split("(")[1].split(")")[0]) for ln in (lines[2], lines[5]))
    print("".join(lines))
    assert all(np.isfinite(float(ln.split("loss_c")[1].split()[0])) for ln in lines) and last < first, (first, last)
    assert "Testing Results: Prec@1" in open(out + "val.log").read()
    ck = torch.load(out + "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert any(k == "module.rnn.weight_hh_l0" for k in ck["state_dict"]) and "module.bn_after_rnn.running_var" in ck["state_dict"]
    tm = [sys.executable, os.path.join(ROOT, "test_models.py"), data[0], "RGB", data[3], out + "checkpoint.pth.tar", "--arch", "resnet18",
          "--test_segments", "5", "--fc_dim", "64", "--baseline_type", "video", "--frame_aggregation", "rnn", "--rnn_cell", "GRU", "--n_ts", "5",
          "--use_attn", "none", "--bS", "8", "-j", "0", "--top", "1", "3"]
    rt = subprocess.run(tm, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert rt.returncode == 0, rt.stdout[-2000:] + rt.stderr[-3000:]
    pred = [ln for ln in rt.stdout.splitlines() if ln.startswith("Pred@1 ") and "%" in ln][-1]
    assert abs(float(pred.split()[1].rstrip("%")) - float(ck["prec1"])) < 1e-2, (pred, ck["prec1"])
