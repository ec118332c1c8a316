"""GPU: --frame_aggregation temconv (reference models.py:44-56, 228-243, 654-672).  The TA3N_AGG_TEMCONV plan through the C ABI against
the fixtures the reference's own layers wrote (tests/golden/make_golden_temconv.py) - forward regions, every stored gradient entry and
every parameter after every step - and against the float64 restatement (tests/temconv_reference.py) at the shapes where the three
kernels branch, with dropout 0.5 / 0.5 on the kernels' own masks, and twice for determinism; VideoModel's forward and autograd
backward; main.py and test_models.py end to end.  Every measured figure is printed before it is asserted.
(T = 1 is not among the shapes: ta3n_plan_create refuses num_segments < 2 for every aggregation.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import temconv_reference as tr
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
    """The flat buffers of one plan and the C entry points on them (TrainEngine does not take the temporal-convolution aggregation)."""

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
        for k, v in (norm or tr.normalisers(c, st)).items():
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
    return float((got.reshape(want.shape) - want).norm() / max(float(want.norm()), 1e-300))      # (tcl_3_1.conv2d.weight: 3 floats here, [1, 1, 3, 1] there)


def _like(g, key, t):
    """t in the shape of the fixture's record `key`."""
    return t.reshape(tuple(g.z[key + "#full"].shape)) if key + "#full" in g.z else t


def _print_and_bound(tag, rels, drift=1.0):
    worst = max(rels, key=rels.get)
    print(f"[temconv {tag}] gradient rel. L2 median {np.median(list(rels.values())):.2e}, worst {rels[worst]:.2e} ({worst}); "
          f"tcl_3_1: weight {rels[tr.W]:.1e}, bias {rels[tr.C0]:.1e}")
    assert np.median(list(rels.values())) <= tol.F32_GRAD_REL_L2_MEDIAN * drift
    for k, v in rels.items():
        assert v <= tol.F32_GRAD_REL_L2 * drift, (k, v)


@pytest.mark.parametrize("name", tr.FIXTURES)
def test_c_abi_matches_reference_golden(name):
    g, c = tr.setup(name)
    T, B, Bs, F = c["T"], c["Bs"] + c["Bt"], c["Bs"], c["fc_dim"]
    plan = tr.make_plan(c)
    shapes = {n: s for n, _, s, _ in plan.params}
    raw = Raw(plan, tr.state_of(shapes, c))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = tr.step_batch(c, st)
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
        raw.update(fused)
        torch.cuda.synchronize()
        coef = float(raw.region("grad_norm")[1])
        drift = tol.GOLDEN_DRIFT_FACTOR if s >= 1 else 1.0
        rels = {k: g.rel_l2(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) for k in sorted(live)}
        _print_and_bound(f"golden {name} step {s} ({'fused' if fused else 'unfused'})", rels, drift)
        for k in rels:
            assert _max_scale(g, f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) <= tol.F32_GRAD_MAX_SCALE * drift, k
        for k, v in raw.views(raw.P).items():
            g.check(f"step{s}/param/{k}", _like(g, f"step{s}/param/{k}", v.cpu()), tol.F32_RTOL, tol.F32_ATOL)
        assert bool(grads[tr.W].any()) and bool(grads[tr.C0].any())


def _case(F, T, Bs, Bt, Cn=5, seed=81):
    # (D: the plan's F is min(fc_dim, feature_dim), models.py:129)
    c = dict(Bs=Bs, Bt=Bt, T=T, D=512 if F <= 512 else 2048, fc_dim=F, C=Cn, wseed=seed, wscale="trained", clip=0.0, beta=tr.BETA, class_w=None,
             flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME)
    plan = tr.make_plan(c)
    state = tr.state_of({n: s for n, _, s, _ in plan.params}, c)
    # taps of both signs and a small bias: F1 >= 0, so the ReLU cuts a share of Z that is neither nothing nor everything (asserted below)
    state[tr.W] = torch.tensor([0.9, -1.3, 0.7])
    state[tr.C0] = torch.tensor([0.01])
    return c, plan, state


def _cut_share(F1, state):
    pad = torch.nn.functional.pad(F1, (0, 0, 1, 1))
    w = state[tr.W].double().reshape(-1)
    z = w[0] * pad[:, :-2] + w[1] * pad[:, 1:-1] + w[2] * pad[:, 2:] + state[tr.C0].double()
    return float((z > 0).double().mean())


# one case per value of T {2, 3, 64}, fc_dim {4: one lane, 20, 1028: a thread's channel loop wraps past 1024} and videos {1 + 1, 3 + 2,
# 150 + 150: 300 partial rows - more than one wave, more than the final sum's workgroup is wide}, the others small
@pytest.mark.parametrize("F,T,Bs,Bt", [(20, 2, 3, 2), (4, 3, 1, 1), (20, 64, 3, 2), (1028, 3, 3, 2), (20, 2, 150, 150)])
def test_shapes_against_float64(F, T, Bs, Bt):
    c, plan, state = _case(F, T, Bs, Bt)
    raw = Raw(plan, state)
    xs, xt, ys, yt = tr.synth_batch(c["C"], T, c["D"], Bs, Bt, seed=82)
    x, labels, B = torch.cat((xs, xt)), torch.cat((ys, yt)), Bs + Bt
    raw.set_step(x, labels, c, dict(n_src=Bs, n_tgt=Bt), 1e-3)
    raw.train_step()
    torch.cuda.synchronize()
    fwd, grads, _ = tr.step(state, x, labels, Bs, Bs, Bt, ("N", "Y", "Y"))
    share = _cut_share(fwd["F1"], state)
    print(f"[temconv shapes] F {F} T {T} videos {Bs}+{Bt}: {100 * share:.1f} % of Z positive")
    assert 0.1 <= share <= 0.9
    got = dict(F1=raw.region("F1", (B, T, F)), V=raw.region("V", (B, F)), Y=raw.region("Y", (B, c["C"])), Pv=raw.region("Pv", (B, 2)),
               Pf=raw.region("Pf", (B, T, 2)))
    for k in ("F1", "V"):
        assert torch.allclose(got[k].cpu().double(), fwd[k], rtol=tol.F32_RTOL, atol=tol.F32_ATOL), k
    for k in ("Y", "Pv", "Pf"):
        err = float((got[k].cpu().double() - fwd[k]).abs().max())
        print(f"[temconv shapes] {k}: max |error| {err:.2e}")
        assert err <= tol.LOGIT_ATOL, k
    gv = raw.views(raw.G)
    assert set(grads) == {n for n, _, _, lv in plan.params if lv}
    _print_and_bound(f"shapes F {F} T {T} videos {Bs}+{Bt}", {k: _rel_l2(gv[k], w) for k, w in grads.items()})
    # the unfused lists leave the same gradients, and the fused optimiser's norm counts the four temconv entries
    fused = {k: v.clone() for k, v in gv.items()}
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in fused.values())))
    raw.update(True)
    torch.cuda.synchronize()
    assert abs(float(raw.region("grad_norm")[0]) - total) <= 1e-5 * total
    raw2 = Raw(plan, state)
    raw2.set_step(x, labels, c, dict(n_src=Bs, n_tgt=Bt), 1e-3)
    raw2.unfused()
    torch.cuda.synchronize()
    for k, v in raw2.views(raw2.G).items():
        if k in grads:
            assert _rel_l2(v, fused[k]) <= tol.F32_GRAD_REL_L2, k


def test_direct_mode_against_float64():
    """No frame discriminator (place_adv N Y N): the kernel writes gZ1 = gF1 [F1 > 0] / keep_i itself, here with dropout_i on."""
    c, plan, state = _case(20, 3, 3, 2)
    c["flags"] = _lib.FLAG_ADV_VIDEO
    plan = tr.make_plan(c)
    raw = Raw(plan, state)
    xs, xt, ys, yt = tr.synth_batch(c["C"], 3, c["D"], 3, 2, seed=83)
    x, labels = torch.cat((xs, xt)), torch.cat((ys, yt))
    seeds = (2468, 1357)
    raw.set_step(x, labels, c, dict(n_src=3, n_tgt=2), 1e-3, p_drop=(0.5, 0.0), seeds=seeds)
    raw.train_step()
    torch.cuda.synchronize()
    m = dropout_masks(seeds[0], seeds[1], 0.5, 0.0, 3, 2, 3, 20, 20)
    mask_i = torch.cat(m["drop_i"]).view(5, 3, 20)
    _, grads, _ = tr.step(state, x, labels, 3, 3, 2, ("N", "Y", "N"), mask_i=mask_i)
    gv = raw.views(raw.G)
    assert set(grads) == {n for n, _, _, lv in plan.params if lv} and "fc_feature_domain.weight" not in grads
    _print_and_bound("direct", {k: _rel_l2(gv[k], w) for k, w in grads.items()})


@pytest.mark.parametrize("F,T,Bs,Bt,Cn", [(64, 5, 6, 5, 6), (20, 7, 5, 4, 7)])
def test_dropout_on_the_kernels_own_masks_against_float64(F, T, Bs, Bt, Cn):
    """dropout 0.5 / 0.5: F1 and Vd carry the masks of tests/dropout_masks.py (dropout_v: element b F + k on the video feature);
    forward tensors and every gradient against the float64 restatement on those masks.  Dropped entries are exactly zero."""
    c, plan, state = _case(F, T, Bs, Bt, Cn=Cn, seed=71)
    raw = Raw(plan, state)
    xs, xt, ys, yt = tr.synth_batch(Cn, T, c["D"], Bs, Bt, seed=72)
    x, labels, B = torch.cat((xs, xt)), torch.cat((ys, yt)), Bs + Bt
    seeds = (12345, 67890)
    raw.set_step(x, labels, c, dict(n_src=Bs, n_tgt=Bt), 1e-3, p_drop=(0.5, 0.5), seeds=seeds)
    raw.train_step()
    torch.cuda.synchronize()
    m = dropout_masks(seeds[0], seeds[1], 0.5, 0.5, Bs, Bt, T, F, F)
    mask_i = torch.cat(m["drop_i"]).view(B, T, F)
    mask_v = torch.cat(m["drop_v"])
    fwd, grads, _ = tr.step(state, x, labels, Bs, Bs, Bt, ("N", "Y", "Y"), mask_i=mask_i, mask_v=mask_v)
    assert 0.1 <= _cut_share(fwd["F1"], state) <= 0.9
    got = dict(F1=raw.region("F1", (B, T, F)), V=raw.region("V", (B, F)), Y=raw.region("Y", (B, Cn)), Pv=raw.region("Pv", (B, 2)),
               Pf=raw.region("Pf", (B, T, 2)))
    assert not bool(got["F1"].cpu()[mask_i == 0].any())                       # what dropout_i dropped is exactly zero
    vd = raw.region("Vd", (B, F)).cpu().double()
    assert not bool(vd[mask_v == 0].any()) and torch.allclose(vd, fwd["Vd"], rtol=tol.F32_RTOL, atol=tol.F32_ATOL)
    for k in ("F1", "V"):
        assert torch.allclose(got[k].cpu().double(), fwd[k], rtol=tol.F32_RTOL, atol=tol.F32_ATOL), k
    for k in ("Y", "Pv", "Pf"):
        err = float((got[k].cpu().double() - fwd[k]).abs().max())
        print(f"[temconv dropout] {k}: max |error| {err:.2e}")
        assert err <= tol.LOGIT_ATOL, k
    gv = raw.views(raw.G)
    assert set(grads) == {n for n, _, _, lv in plan.params if lv}
    _print_and_bound(f"dropout F {F} T {T}", {k: _rel_l2(gv[k], w) for k, w in grads.items()})


@pytest.mark.parametrize("fused", [True, False])
def test_the_same_step_twice_gives_the_same_bits(fused):
    """No floating-point atomics: 300 partial rows summed in a fixed order."""
    c, plan, state = _case(64, 5, 150, 150)
    raw = Raw(plan, state)
    xs, xt, ys, yt = tr.synth_batch(c["C"], 5, c["D"], 150, 150, seed=84)
    raw.set_step(torch.cat((xs, xt)), torch.cat((ys, yt)), c, dict(n_src=150, n_tgt=150), 1e-3, p_drop=(0.5, 0.5), seeds=(5, 6))
    runs = []
    for _ in range(2):
        raw.G.zero_()
        raw.region("tc_part").zero_()
        raw.train_step() if fused else raw.unfused()
        torch.cuda.synchronize()
        runs.append({k: v.clone() for k, v in raw.views(raw.G).items()})
    assert bool(runs[0][tr.W].any()) and bool(runs[0][tr.C0].any())
    assert torch.equal(runs[0][tr.W], runs[1][tr.W]) and torch.equal(runs[0][tr.C0], runs[1][tr.C0])
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def _module(c, val_T=None):
    m = VideoModel(c["C"], "video", "temconv", "RGB", train_segments=c["T"], val_segments=val_T or c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   dropout_i=0.0, dropout_v=0.0, use_attn="none", verbose=False)
    sd = m.state_dict()
    sd.update(tr.state_of({k: tuple(v.shape) for k, v in sd.items()}, c))
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("name", ["tiny_tc_T5", "tiny_tc_odd"])
def test_module_path_forward_and_autograd_backward(name):
    """VideoModel(frame_aggregation='temconv'): the 10-tuple against the fixture's forward records; the loss assembled by the caller
    (main.py:439-451, 508-538) plus a gradient of the caller's own at feat[1] (gV_ext, the route DAN / JAN take), every parameter
    gradient against the float64 restatement with the same extra term; the layers the forward never calls keep grad None."""
    import torch.nn.functional as Fn
    g, c = tr.setup(name)
    Bs, Bt = c["Bs"], c["Bt"]
    m = _module(c)
    m.train()
    st = step_schedule(c)[0]
    xs, xt, labels = tr.step_batch(c, st)
    out = m(xs, xt, tr.BETA, 0, True, False)
    attn_s, out_s, _, pd_s, feat_s, attn_t, out_t, _, pd_t, feat_t = out
    g.check("fwd/out_s", out_s, 0, tol.LOGIT_ATOL); g.check("fwd/out_t", out_t, 0, tol.LOGIT_ATOL)
    g.check("fwd/attn_s", attn_s, tol.F32_RTOL, tol.F32_ATOL); g.check("fwd/attn_t", attn_t, tol.F32_RTOL, tol.F32_ATOL)
    for i, nm in enumerate(("rel", "vid", "frm")):      # (the module path computes every discriminator: the caller assembles the loss)
        g.check(f"fwd/pd_s_{nm}", pd_s[i], 0, tol.LOGIT_ATOL); g.check(f"fwd/pd_t_{nm}", pd_t[i], 0, tol.LOGIT_ATOL)
    assert torch.equal(pd_s[0], pd_s[1]) and torch.equal(feat_s[0], out_s) and torch.equal(attn_t, feat_t[1][:, 0])
    for i, nm in enumerate(("y", "v", "f1")):
        g.check(f"fwd/feat_s_{nm}", feat_s[i], tol.F32_RTOL, tol.LOGIT_ATOL if i == 0 else tol.F32_ATOL)
        g.check(f"fwd/feat_t_{nm}", feat_t[i], tol.F32_RTOL, tol.LOGIT_ATOL if i == 0 else tol.F32_ATOL)
    wv = torch.linspace(-1, 1, c["fc_dim"]).cuda()              # the caller's own term on feat[1]
    loss = Fn.cross_entropy(out_s, labels[:Bs].cuda())
    for lvl in (1, 2):
        ps, pt = pd_s[lvl].reshape(-1, 2), pd_t[lvl].reshape(-1, 2)
        lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long().cuda()
        loss = loss + Fn.cross_entropy(torch.cat((ps, pt)), lab)
    loss = loss + 0.1 * ((feat_s[1] * wv).sum() + (feat_t[1] * wv).sum())
    loss.backward()
    P = tr.state_of({k: tuple(v.shape) for k, v in m.state_dict().items()}, c)
    _, grads, _ = tr.step(P, torch.cat((xs, xt)), labels, Bs, Bs, Bt, ("N", "Y", "Y"), extra_v=wv.cpu())
    named = dict(m.named_parameters())
    assert {k for k, v in named.items() if v.grad is not None} == set(grads)
    assert named[tr.W].grad.shape == (1, 1, 3, 1) and named[tr.C0].grad.shape == (1,)
    _print_and_bound(f"module {name}", {k: _rel_l2(named[k].grad, w) for k, w in grads.items()})
    for dead in ("tcl_5_1.conv2d.weight", "tcl_3_2.conv2d.bias", "tcl_5_2.conv2d.weight", "bn_1_S.weight", "bn_2_T.bias", "conv_fusion.0.weight"):
        assert named[dead].grad is None, dead


def test_module_path_validates_on_another_segment_count():
    """tiny_tc_eval: trained on 5 segments, validated on 25 - a second plan, the same parameters; main.validate's call (main.py:707)."""
    g, c = tr.setup("tiny_tc_eval")
    val_T = int(g.meta("val_T"))
    m = _module(c, val_T)
    m.eval()
    xv, _, _, _ = tr.synth_batch(c["C"], val_T, c["D"], c["Bs"], c["Bt"], seed=c["xseed"] + 7)
    with torch.no_grad():
        ev = m(xv, xv, [0, 0, 0], 0, False, False)
    g.check("eval/out_t", ev[6], 0, tol.LOGIT_ATOL)
    g.check("eval/feat_t_v", ev[9][1], tol.F32_RTOL, tol.F32_ATOL)
    assert ev[9][2].shape == (c["Bs"], val_T, c["fc_dim"]) and len(m._plans) == 1
    m.train()
    xs, xt, _ = tr.step_batch(c, step_schedule(c)[0])
    g.check("fwd/out_s", m(xs, xt, tr.BETA, 0, True, False)[1], 0, tol.LOGIT_ATOL)
    assert len(m._plans) == 2


def test_main_trains_validates_checkpoints_and_the_tester_reads_it(tmp_path):
    """main.py --frame_aggregation temconv --use_attn none for one epoch on the tests/fixture_t7.py dataset: logs, validation, checkpoint;
    the losses are finite; test_models.py on the checkpoint reproduces the validation accuracy."""
    data = make_dataset(str(tmp_path / "data"))
    exp = str(tmp_path / "exp")
    opts = ["--baseline_type", "video", "--frame_aggregation", "temconv", "--use_target", "uSv", "--adv_DA", "RevGrad",
            "--use_attn", "none", "--add_loss_DA", "none", "--beta", "0.75", "0.75", "0.5", "--place_adv", "N", "Y", "Y", "--lr_adaptive", "dann",
            "--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0", "--dropout_v", "0", "-b", "8", "6", "8",
            "--lr", "0.03", "--epochs", "1", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn", "--save_best_log", str(tmp_path / "best.log")]
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *opts]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = exp + "/RGB/"
    for f in ("train.log", "val.log", "checkpoint.pth.tar", "model_best.pth.tar"):
        assert os.path.exists(out + f), f
    lines = [ln for ln in open(out + "train.log") if ln.startswith("Train:")]
    print("".join(lines))
    assert len(lines) == 3 and all(np.isfinite(float(ln.split("loss_c")[1].split()[0])) for ln in lines)
    assert "Testing Results: Prec@1" in open(out + "val.log").read()
    ck = torch.load(out + "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert ck["state_dict"]["module.tcl_3_1.conv2d.weight"].shape == (1, 1, 3, 1) and "module.conv_fusion.0.bias" in ck["state_dict"]
    fresh = VideoModel(ck["state_dict"]["module.fc_classifier_video_source.weight"].shape[0], "video", "temconv", "RGB", train_segments=5, val_segments=5,
                       base_model="resnet18", fc_dim=64, use_attn="none", verbose=False)
    assert not torch.equal(fresh.state_dict()["tcl_3_1.conv2d.weight"], ck["state_dict"]["module.tcl_3_1.conv2d.weight"])
    tm = [sys.executable, os.path.join(ROOT, "test_models.py"), data[0], "RGB", data[3], out + "checkpoint.pth.tar", "--arch", "resnet18",
          "--test_segments", "5", "--fc_dim", "64", "--baseline_type", "video", "--frame_aggregation", "temconv",
          "--use_attn", "none", "--bS", "8", "-j", "0", "--top", "1", "3"]
    rt = subprocess.run(tm, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert rt.returncode == 0, rt.stdout[-2000:] + rt.stderr[-3000:]
    pred = [ln for ln in rt.stdout.splitlines() if ln.startswith("Pred@1 ") and "%" in ln][-1]
    assert abs(float(pred.split()[1].rstrip("%")) - float(ck["prec1"])) < 1e-2, (pred, ck["prec1"])


