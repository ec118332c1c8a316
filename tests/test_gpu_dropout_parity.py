"""Dropout ON against the oracle, on the kernels' own masks.  Every real run trains with dropout (0.5 / 0.5 is the reference's default),
yet the other GPU tests that compare numbers with a reference run with dropout off, "because the oracle and the kernels draw different
masks".  They need not: the stream is stateless, tests/dropout_masks.py rebuilds every mask on the host from the element-id formulas
alone ("Dropout element ids"), and oracle.train_step takes explicit masks.  Per case, after one or two eng.train_step(seed=s):

 (a) exact pattern: F1 is zero exactly where the host stream drops and - outside the entries whose float64 pre-activation lies within
     1e-4 of its largest magnitude of the ReLU kink (at most 1 % of a tensor; tests/test_dropout_cpu.py checks that condition from the
     oracle alone) - nonzero exactly where it keeps an active unit; Vd is 0 / V / (1 - p_v) by the host's dropout_v pattern, and the
     gradient that leaves dropout_v (gVt) is zero exactly where it drops.  First, because (b) synchronises ReLU patterns and would hide one
     direction of a mask disagreement.
 (b) mask-synchronised gradient parity (the recipe of tests/test_gpu_masked_gradients.py): ReLU patterns from the workspace, DROPOUT
     MASKS FROM THE HELPER, never from the workspace; hidden activations, losses and every element of every gradient tensor, fp32 MFMA,
     within F32_MASKED_GRAD_REL_L2 per tensor and F32_MASKED_GRAD_REL_L2_MEDIAN in the median - the dropout-off bounds, unchanged.
 (c) negative controls (tiny case): the oracle on masks of seed + 1, with drop_v missing its 1 / (1 - p_v), with target rows counted
     from 0 must each land above 100 x F32_MASKED_GRAD_REL_L2 - the comparator sees the bugs this file is for.

Excluded shares of (a), float64 oracle, at the seeds below (tests/test_dropout_cpu.py::test_excluded_shares_of_the_gpu_cases asserts
them <= 1 % on the CPU and prints them): 0.03 % in both steps of trn-m tiny, avgpool + RevGrad and MCD, 0.00 % / 0.09 % for source-only avgpool, 0.00 % / 0.03 % for AdaBN, 0.03 % / 0.48 % for
the ragged case (the second step's dummy rows), 0.00 % for both layers of add_fc 2, 0.09 % for frame attention.

--ens_DA MCD: both passes - the reversed second forward draws its own seeds (ta3n_amd/engine.py: mcd_second_forward) and runs in a second
workspace, whose masks and ReLU patterns the oracle takes through train_step(drop_rev=, masks_rev=)."""
import numpy as np
import pytest
import torch

from dropout_masks import (BETA, GAMMA, LR, TINY, batch, check_frame_pattern, check_video_pattern, dropout_masks, oracle_cases, preactivation,
                           rel_l2, summary)
from golden_util import Golden, case_config
from oracle import ta3n_oracle as orc
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, dropout_seeds, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

def _dev(t):
    return t.cuda()


def _sync():
    torch.cuda.synchronize()


def _hidden_spec(eng, avg):
    B, T, F = eng.B, eng.T, eng.F
    if avg and "Hf" not in eng.plan.regions:      # source-only TemPooling: no discriminators
        return dict(F1=("F1", (B * T, F)))
    if avg:
        return dict(F1=("F1", (B * T, F)), Hf=("Hf", (B * T, F)), Hv=("Hv", (B, F)))
    n_tuples = sum(len(s) for s in orc.selected_relations(T))
    return dict(F1=("F1", (B * T, F)), Hf=("Hf", (B * T, F)), Z=("Zr", (B, n_tuples, 256)), Hr=("Hr", (B, T - 1, 256)), Hv=("Hv", (B, 256)))


def _engine_masks(eng, avg):
    T = eng.T
    full = {k: eng.region(r, sh).detach().cpu() for k, (r, sh) in _hidden_spec(eng, avg).items()}
    rows = lambda k, lo, hi: full[k][lo * T:hi * T] if k in ("F1", "Hf") else full[k][lo:hi]
    act = tuple({k: rows(k, lo, hi) for k in full} for lo, hi in ((0, eng.Bs), (eng.Bs, eng.B)))
    return tuple({k: v > 0 for k, v in a.items()} for a in act), act


def _oracle(cfg, state, xs, xt, ys, gamma, ns, nt, mk, masks, dtype=torch.float64):
    st = orc.TrainState(params={k: v.to(dtype).clone() for k, v in state.params.items()}, lr=LR)
    st.momentum = {k: v.to(dtype).clone() for k, v in state.momentum.items()}
    return orc.train_step(st, xs.to(dtype), xt.to(dtype), ys, BETA, gamma, cfg, clip=20.0, n_src=ns, n_tgt=nt, masks=masks,
                          drop_i=tuple(m.to(dtype) for m in mk["drop_i"]), drop_v=tuple(m.to(dtype) for m in mk["drop_v"]))


def _grad_parity(eng, res, tag, lines, exempt=()):
    """Every element of every gradient tensor against the oracle's: per tensor <= F32_MASKED_GRAD_REL_L2, median <=
    F32_MASKED_GRAD_REL_L2_MEDIAN.  A tensor whose reference norm is below 1e-5 of the step's largest gradient norm is held to that
    absolute size instead, as tests/test_gpu_engine_bn.py does - but only if the CASE names it in `exempt` (None: only those whose
    reference is exactly zero); any other tensor that small fails, and the exempt ones are printed."""
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res["grads"]}
    assert set(eng.live_names()) == set(res["grads"])
    top = max(w.double().norm().item() for w in res["grads"].values())
    per = rel_l2(got, res["grads"])
    rel, small = {}, []
    for k, w in res["grads"].items():
        assert torch.isfinite(got[k]).all(), (tag, k)
        if w.double().norm().item() < 1e-5 * top:
            assert (w.double().norm().item() == 0.0) if exempt is None else (k in exempt), (tag, k, "a tensor this small must be named by the case")
            assert (got[k].double().reshape(w.shape) - w.double()).norm().item() < 1e-5 * top, (tag, k)
            small.append(k)
        else:
            rel[k] = per[k]
    med, worst, line = summary(rel, tag)
    lines.append(line)
    if small:
        lines.append(f"[dropout parity] {tag}: held to 1e-5 of the largest gradient norm instead ({len(small)} of {len(res['grads'])}): " + ", ".join(sorted(small)))
    for k, v in rel.items():
        assert v <= tol.F32_MASKED_GRAD_REL_L2, (tag, k, v)
    assert med <= tol.F32_MASKED_GRAD_REL_L2_MEDIAN, (tag, med)
    return got


def _run(case, p_i, p_v, fused, capsys, steps=2, controls=False, engine_kw=None, gamma=GAMMA, exempt=()):
    mkcfg, shape, wseed, wscale, xseed, _, valid = oracle_cases()[case]
    Bs, Bt, T, D, Fc, Cn = (shape[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    cfg = mkcfg(p_i, p_v)
    avg = cfg.frame_aggregation == "avgpool"
    NV = Fc if avg else 256
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=p_i, dropout_v=p_v, clip=20.0, fused=fused, **(engine_kw or {}))
    assert eng.fused == fused
    eng.load_state(synth_state(orc.param_shapes(cfg), seed=wseed, scale=wscale))
    lines = []
    for s in range(steps):
        ns, nt = valid[s]
        xs, xt, ys = batch(shape, xseed, s, ns, nt)
        state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
        state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
        eng.set_batch(_dev(xs), _dev(xt), _dev(ys))
        eng.train_step(BETA, gamma, LR, valid_source=ns, valid_target=nt, seed=s)
        _sync()
        tag = f"{case} p {p_i}/{p_v} {'fused' if fused else 'unfused'} step {s}"
        seeds = dropout_seeds(s, 0)
        mk = dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, NV)
        # (a) exact patterns
        B = Bs + Bt
        share = check_frame_pattern(eng.region("F1", (B * T, Fc)).cpu(), preactivation(cfg, state.params, xs, xt), torch.cat(mk["keep_i"]), tag)
        # (source-only TemPooling has no gVt: pool_cls_kernel goes from the logit gradient to gZ1 [B, T, F] at once - its largest
        # magnitude over the segments stands in: zero wherever dropout_v dropped the column)
        gVt = eng.region("gVt", (B, NV)).cpu() if "gVt" in eng.plan.regions else eng.region("gZ1", (B, T, Fc)).cpu().abs().amax(1)
        check_video_pattern(eng.region("V", (B, NV)).cpu(), eng.region("Vd", (B, NV)).cpu(), gVt, torch.cat(mk["keep_v"]), p_v, tag)
        lines.append(f"[dropout parity] {tag}: excluded share of the pattern check {share:.2%}")
        # (b) mask-synchronised parity
        masks, act = _engine_masks(eng, avg)
        res = _oracle(cfg, state, xs, xt, ys, gamma, ns, nt, mk, masks)
        for d, (dom, nv) in enumerate((("src", ns), ("tgt", nt))):
            for k, a in act[d].items():
                want = res[dom]["hidden"][k].detach()
                rows = nv * T if k in ("F1", "Hf") else nv
                err = (a[:rows].double() - want[:rows]).abs().max().item()
                assert err <= 2e-4 * max(1.0, want[:rows].abs().max().item()), (tag, dom, k, err)
        loss = eng.losses()["loss"]
        assert abs(loss - res["loss"].item()) <= 2e-4 * max(1.0, abs(res["loss"].item())), (tag, loss, res["loss"].item())
        got = _grad_parity(eng, res, tag, lines, exempt)
        # (c) negative controls
        if controls and s == 0:
            ratios = []
            for name, bad in (("seed + 1", dropout_masks(seeds[0] + 1, seeds[1] + 1, p_i, p_v, Bs, Bt, T, Fc, NV)),
                              ("drop_v unscaled", dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, NV, scale_v=False)),
                              ("target rows from 0", dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, NV, target_row0=0))):
                worst = max(rel_l2(got, _oracle(cfg, state, xs, xt, ys, gamma, ns, nt, bad, masks)["grads"]).values())
                ratios.append(f"{name} {worst / tol.F32_MASKED_GRAD_REL_L2:.0f} x")
                assert worst > 100 * tol.F32_MASKED_GRAD_REL_L2, (tag, name, worst)
            lines.append(f"[dropout parity] {tag}: negative controls, worst rel. L2 over the bound: " + ", ".join(ratios))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    return eng


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("p_i,p_v", [(0.5, 0.5), (0.3, 0.8)])
def test_trn_m(p_i, p_v, fused, capsys):
    """GEMM epilogue EPI_DROP_I, heads kernel forward / backward (fused), pool_fwd_kernel and the unfused backward through dropout_v
    (unfused); the negative controls ride on the fused 0.5 / 0.5 run.  Excluded shares: <= 0.05 %."""
    _run("trn-m", p_i, p_v, fused, capsys, controls=(fused and p_i == 0.5))


def test_trn_m_ragged(capsys):
    """F = 128, three tiles of rows, and in the second step dummy rows in both domains (valid 37 / 25 of 40 / 30): the target rows' ids
    still start at Bs T.  Excluded share 0.48 % in the second step (the dummy rows' biases, see RAGGED_WSEED in tests/dropout_masks.py)."""
    _run("ragged", 0.3, 0.8, True, capsys)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_avgpool_revgrad(fused, capsys):
    """TemPooling + RevGrad (config of tiny_avgpool_da): dropout_v on the F-wide mean feature - pool_avg_fwd_kernel, NV = F = 64."""
    _run("avgpool_da", 0.3, 0.8, fused, capsys, gamma=0.0,
         engine_kw=dict(aggregation="avgpool", flags=flags_from_options(("N", "Y", "Y"), "none", "none", "RevGrad", "uSv")))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_avgpool_source_only(fused, capsys):
    """TemPooling, source-only (config of tiny_avgpool, BASELINE configs[0]; no adversarial flag): pool_cls_kernel - its own dropout_v
    id b F + k, its own 1 / (1 - p_v), and its own way back gvd mask / T / (1 - p_i) to gZ1 - at p 0.3 / 0.8, so that a p_i / p_v
    mix-up in it cannot pass.  Excluded shares 0.00 % / 0.09 %."""
    _run("avgpool_src", 0.3, 0.8, fused, capsys, gamma=0.0, engine_kw=dict(aggregation="avgpool", flags=0))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("p_i,p_v", [(0.5, 0.5), (0.3, 0.8)])
def test_adabn(p_i, p_v, fused, capsys):
    """use_bn AdaBN (config of tiny_adabn): dropout_i moves out of the GEMM into bn_shared_fwd_kernel; the pattern is checked on the
    post-BatchNorm pre-activation.  Fused: the 10-launch step."""
    _run("adabn", p_i, p_v, fused, capsys, engine_kw=dict(use_bn="AdaBN"), exempt=ADABN_SMALL)


# use_bn: the shared FC's bias sits in front of a BatchNorm, its gradient is zero in exact arithmetic (tests/test_gpu_engine_bn.py); and the
# frame discriminator's 2-wide output bias, whose two entries are sums over all rows that cancel (+x, -x), falls below 1e-5 of the largest
# gradient norm in the 0.3 / 0.8 run.  No other tensor of any case may be that small.
ADABN_SMALL = ("fc_feature_shared_source.bias", "fc_classifier_domain.bias")


def test_p_one_drops_everything(capsys):
    """p = 1 / 1: F1 and Vd are all zero (not NaN: 1 / (1 - p) is 0 there), every gradient is finite, and the gradients equal the
    oracle's on all-zero masks: where the oracle's gradient is exactly zero (the weights behind the dropped features) the engine's is
    zero up to 1e-5 of the largest gradient norm, every other tensor meets the relative bound."""
    eng = _run("trn-m", 1.0, 1.0, True, capsys, steps=1, exempt=None)
    assert not eng.region("F1").any() and not eng.region("Vd").any()
    assert torch.isfinite(eng.G).all() and torch.isfinite(eng.P).all()


def test_bf16_twins_carry_the_dropped_zeros(capsys):
    """bf16 MFMA operands from bf16 twins, trn-m tiny, 0.5 / 0.5: the twin of F1 is round_bf16(F1) bit for bit and zero wherever the
    host stream drops; gradients and logits against the oracle's bf16-operand mode on the SAME masks (ReLU patterns synchronised), held
    to the BF16_REF_* bounds the way tests/test_gpu_gradients.py applies them: tensors of >= 4096 elements within min(cap, factor x the
    contract's own distance from fp32 on these inputs + floor), the median over all tensors, logits against their rms."""
    Bs, Bt, T, D, Fc, Cn = (TINY[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    p_i = p_v = 0.5
    cfg32 = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=p_i, dropout_v=p_v)
    cfg16 = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=p_i, dropout_v=p_v, arithmetic="bf16", bf16_twins=True)
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=p_i, dropout_v=p_v, clip=20.0, bf16=True, bf16_store=True)
    assert eng.fused and eng.bf16_store
    eng.load_state(synth_state(orc.param_shapes(cfg32), seed=11, scale="trained"))
    xs, xt, ys = batch(TINY, 21, 0, Bs, Bt)
    state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
    state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
    eng.set_batch(_dev(xs), _dev(xt), _dev(ys))
    eng.train_step(BETA, GAMMA, LR, seed=0)
    _sync()
    mk = dropout_masks(*dropout_seeds(0, 0), p_i, p_v, Bs, Bt, T, Fc, 256)
    B = Bs + Bt
    keep = torch.cat(mk["keep_i"])
    F1 = eng.region("F1", (B * T, Fc))
    o16, _ = eng.plan.region("ws16")
    oF, n = eng.plan.region("F1")
    twin = eng.ws[o16:].view(torch.int16)[oF:oF + n].view(B * T, Fc)
    assert torch.equal(twin, F1.to(torch.bfloat16).view(torch.int16))
    assert bool((twin.cpu()[keep == 0] == 0).all()) and bool((F1.cpu()[keep == 0] == 0).all())
    assert 0.2 < (twin != 0).double().mean().item() < 0.5          # (about half of the active half survives)
    check_video_pattern(eng.region("V", (B, 256)).cpu(), eng.region("Vd", (B, 256)).cpu(), eng.region("gVt", (B, 256)).cpu(),
                        torch.cat(mk["keep_v"]), p_v, "bf16")
    masks, _ = _engine_masks(eng, False)
    res16 = _oracle(cfg16, state, xs, xt, ys, GAMMA, Bs, Bt, mk, masks, dtype=torch.float32)
    res32 = _oracle(cfg32, state, xs, xt, ys, GAMMA, Bs, Bt, mk, masks, dtype=torch.float32)
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res16["grads"]}
    per, contract = rel_l2(got, res16["grads"]), rel_l2(res16["grads"], res32["grads"])
    med, worst, line = summary(per, "bf16 twins p 0.5/0.5 vs the bf16-operand oracle")
    with capsys.disabled():
        print("\n" + line)
    for k, v in per.items():
        if res16["grads"][k].numel() >= 4096:
            bound = min(tol.BF16_REF_GRAD_REL_L2, tol.BF16_REF_GRAD_CONTRACT_FACTOR * contract[k] + tol.BF16_REF_GRAD_FLOOR)
            assert v <= bound, (k, v, bound)
    assert med <= tol.BF16_REF_GRAD_REL_L2_MEDIAN, med
    o = eng.outputs()
    for key, pick in (("out", lambda r: r["out"]), ("pred_rel", lambda r: r["pred_domain"][0]), ("pred_vid", lambda r: r["pred_domain"][1]),
                      ("pred_frm", lambda r: r["pred_domain"][2])):
        want = torch.cat((pick(res16["src"]), pick(res16["tgt"])), 0).detach()
        err = (o[key].cpu().reshape(want.shape) - want).abs().max().item()
        assert err <= tol.BF16_REF_LOGIT_REL_RMS * want.pow(2).mean().sqrt().item() + 1e-7, (key, err)


def _interp_hyper(Bs, Bt, T, p_i, p_v, step):
    si, sv = dropout_seeds(step, 0)
    return dict(beta=list(BETA), gamma=GAMMA, lr=LR, momentum=0.9, weight_decay=1e-4, clip=20.0, p_drop_i=p_i, p_drop_v=p_v, seed_i=si, seed_v=sv,
                inv_n_cls=1.0 / Bs, inv_n_rel=1.0 / ((Bs + Bt) * (T - 1)), inv_n_vid=1.0 / (Bs + Bt), inv_n_frm=1.0 / ((Bs + Bt) * T),
                inv_n_ent=1.0 / (Bs + Bt), valid_source=Bs, valid_target=Bt, train=1)


def _against_interpreter(eng, it, state, xs, xt, ys, hy, fused, tag, capsys):
    """Gradients of an fp32 engine step against the float64 numpy execution of the SAME plan on the same seeds: max |error| <=
    (2e-3 + 2e-4) x max |want| per tensor, the bound of tests/test_gpu_bf16.py's kernels-vs-interpreter comparisons."""
    it.set_params(state)
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:xs.size(0)] = ys.numpy()
    it.hy = hy
    it.G[:] = 0
    for grp in ((4,) if fused else (0, 1, 2)):
        it.run_group(grp)
    want = it.get_params(it.G)
    got = {k: v.detach().cpu().double().numpy() for k, v in eng.param_views(eng.G).items()}
    worst = {}
    for k in eng.live_names():
        scale = np.abs(want[k]).max() + 1e-30
        worst[k] = np.abs(got[k] - want[k].reshape(got[k].shape)).max() / scale
        assert worst[k] <= 2e-3 + 2e-4, (tag, k, worst[k])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    with capsys.disabled():
        print(f"\n[dropout parity] {tag} vs the float64 interpreter: worst max/scale " + ", ".join(f"{k} {v:.2e}" for k, v in top))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_add_fc_2_layers_draw_the_offset_streams(fused, capsys):
    """--add_fc 2 (tiny_addfc2), p 0.5 / 0.3: the pattern check per layer against the helper's streams - layer 2 at the pad2 offset
    B T F - and, the oracle having no stacked layers, the gradients against the float64 interpreter of the same plan."""
    from plan_interp import Interp
    c = case_config(Golden("tiny_addfc2"))
    Bs, Bt, T, D, Fc, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], 0.5, 0.3
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=p_i, dropout_v=p_v, clip=20.0, add_fc=2, fused=fused)
    state = synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"])
    eng.load_state(state)
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    eng.set_batch(_dev(xs), _dev(xt), _dev(ys))
    eng.train_step(BETA, GAMMA, LR, seed=0)
    _sync()
    B = Bs + Bt
    seeds = dropout_seeds(0, 0)
    k1 = torch.cat(dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, 256, layer=1)["keep_i"])
    m2 = dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, 256, layer=2)
    k2 = torch.cat(m2["keep_i"])
    P = {k: v.double() for k, v in state.items()}
    X = torch.cat((xs, xt), 0).double().reshape(B * T, D)
    Fl1, F2 = eng.region("F_l1", (B * T, Fc)).cpu().double(), eng.region("F1", (B * T, Fc)).cpu().double()
    pre1 = X @ P["fc_feature_shared_source.weight"].t() + P["fc_feature_shared_source.bias"]
    pre2 = Fl1 @ P["fc_feature_shared_2_source.weight"].t() + P["fc_feature_shared_2_source.bias"]
    s1, s2 = check_frame_pattern(Fl1, pre1, k1, "layer 1"), check_frame_pattern(F2, pre2, k2, "layer 2")
    assert not torch.equal(k1, k2)
    check_video_pattern(eng.region("V", (B, 256)).cpu(), eng.region("Vd", (B, 256)).cpu(), eng.region("gVt", (B, 256)).cpu(),
                        torch.cat(m2["keep_v"]), p_v, "add_fc 2")
    with capsys.disabled():
        print(f"\n[dropout parity] add_fc 2 {'fused' if fused else 'unfused'}: excluded shares {s1:.2%} (layer 1), {s2:.2%} (layer 2)")
    _against_interpreter(eng, Interp(eng.plan), state, xs, xt, ys, _interp_hyper(Bs, Bt, T, p_i, p_v, 0), fused,
                         f"add_fc 2 {'fused' if fused else 'unfused'}", capsys)


def test_frame_attention_lists(capsys):
    """--use_attn_frame TransAttn (tiny_faf_T5; the option's unfused lists), p 0.5 / 0.5: pattern check on F1 (the un-attended frame
    features) and Vd, gradients against the float64 interpreter with the two frame-attention phases."""
    from plan_interp import Interp
    c = case_config(Golden("tiny_faf_T5"))
    Bs, Bt, T, D, Fc, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], 0.5, 0.5
    flags = flags_from_options(("Y", "Y", "Y"), "attentive_entropy", "TransAttn", "RevGrad", "uSv", use_attn_frame="TransAttn")
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, flags=flags, dropout_i=p_i, dropout_v=p_v, clip=20.0)
    assert eng.frame_attn and not eng.fused
    state = synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"])
    eng.load_state(state)
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    eng.set_batch(_dev(xs), _dev(xt), _dev(ys))
    eng.train_step(BETA, GAMMA, LR, seed=0)
    _sync()
    B = Bs + Bt
    mk = dropout_masks(*dropout_seeds(0, 0), p_i, p_v, Bs, Bt, T, Fc, 256)
    P = {k: v.double() for k, v in state.items()}
    pre = torch.cat((xs, xt), 0).double().reshape(B * T, D) @ P["fc_feature_shared_source.weight"].t() + P["fc_feature_shared_source.bias"]
    share = check_frame_pattern(eng.region("F1", (B * T, Fc)).cpu(), pre, torch.cat(mk["keep_i"]), "frame attention")
    check_video_pattern(eng.region("V", (B, 256)).cpu(), eng.region("Vd", (B, 256)).cpu(), eng.region("gVt", (B, 256)).cpu(),
                        torch.cat(mk["keep_v"]), p_v, "frame attention")
    with capsys.disabled():
        print(f"\n[dropout parity] frame attention: excluded share {share:.2%}")
    _against_interpreter(eng, Interp(eng.plan), state, xs, xt, ys, _interp_hyper(Bs, Bt, T, p_i, p_v, 0), False, "frame attention", capsys)


def test_module_path_forward_uses_the_drawn_seeds():
    """VideoModel (trn-m tiny, train mode, 0.5 / 0.5), forward only: the two stream seeds are the torch.randint draw of the forward
    (ta3n_amd/models.py) - replayed here after torch.manual_seed - and the class logits and domain predictions equal the oracle's
    forward on the helper's masks to LOGIT_ATOL."""
    from ta3n_amd.models import VideoModel
    Bs, Bt, T, D, Fc, Cn = (TINY[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=0.5, dropout_v=0.5)
    params = synth_state(orc.param_shapes(cfg), seed=11, scale="trained")
    m = VideoModel(Cn, "video", "trn-m", "RGB", train_segments=T, val_segments=T, base_model="resnet18", fc_dim=Fc, dropout_i=0.5,
                   dropout_v=0.5, partial_bn=False, verbose=False, use_attn="TransAttn")
    sd = m.state_dict(); sd.update(params); m.load_state_dict(sd)
    m = m.cuda(); m.train()
    xs, xt, ys = batch(TINY, 21, 0, Bs, Bt)
    torch.manual_seed(5)
    seeds = [int(v) for v in torch.randint(0, 2 ** 31 - 1, (2,))]
    torch.manual_seed(5)
    with torch.no_grad():
        out = m(xs, xt, BETA, 0, True, False)
    mk = dropout_masks(seeds[0], seeds[1], 0.5, 0.5, Bs, Bt, T, Fc, 256)
    p = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        want = [orc.forward_domain(p, x.double(), BETA, cfg, mk["drop_i"][d], mk["drop_v"][d], domain="ST"[d]) for d, x in enumerate((xs, xt))]
    for d, (y, pd) in enumerate(((out[1], out[3]), (out[6], out[8]))):
        assert (y.cpu().double() - want[d]["out"]).abs().max().item() <= tol.LOGIT_ATOL, d
        for l in range(3):
            w = want[d]["pred_domain"][l]
            assert (pd[l].cpu().double().reshape(w.shape) - w).abs().max().item() <= tol.LOGIT_ATOL, (d, l)
    # ... and another draw gives other masks: the logits move
    torch.manual_seed(6)
    with torch.no_grad():
        other = m(xs, xt, BETA, 0, True, False)
    assert (other[1] - out[1]).abs().max().item() > 10 * tol.LOGIT_ATOL


def test_mcd_both_passes(capsys):
    """--ens_DA MCD (config of tiny_mcd, mu 0.5), p 0.5 / 0.5, one step: the first pass on dropout_seeds(step), the reversed second pass
    on the seeds the engine derives for it, each in its own workspace - pattern checks on both, then losses (with the second classifier's
    cross-entropy, loss_s and the entropy term moved to the second pass) and every gradient of the summed two passes against the oracle
    on the helper's masks for both passes."""
    c = case_config(Golden("tiny_mcd"))
    Bs, Bt, T, D, Fc, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], 0.5, 0.5
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=p_i, dropout_v=p_v, ens_DA="MCD")
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=p_i, dropout_v=p_v, clip=20.0, ens_DA="MCD", mu=c["mu"])
    assert not eng.fused
    eng.load_state(synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"]))
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
    state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
    eng.set_batch(_dev(xs), _dev(xt), _dev(ys))
    eng.train_step(BETA, GAMMA, LR, seed=0)
    _sync()
    B = Bs + Bt
    seeds1 = dropout_seeds(0, 0)
    seeds2 = dropout_seeds(seeds1[0] ^ 0x5bd1e995, 0)          # engine.py: mcd_second_forward
    mk1, mk2 = (dropout_masks(*sd, p_i, p_v, Bs, Bt, T, Fc, 256) for sd in (seeds1, seeds2))
    assert not torch.equal(mk1["keep_i"][1], mk2["keep_i"][1])
    pre = preactivation(cfg, state.params, xs, xt)
    lines = []
    for what, reg, mk in (("first pass", eng.region, mk1), ("second pass", eng._region2, mk2)):
        share = check_frame_pattern(reg("F1", (B * T, Fc)).cpu(), pre, torch.cat(mk["keep_i"]), what)
        check_video_pattern(reg("V", (B, 256)).cpu(), reg("Vd", (B, 256)).cpu(), reg("gVt", (B, 256)).cpu(), torch.cat(mk["keep_v"]), p_v, what)
        lines.append(f"[dropout parity] mcd {what}: excluded share of the pattern check {share:.2%}")
    masks, act = _engine_masks(eng, False)
    full2 = {k: eng._region2(r, sh).detach().cpu() for k, (r, sh) in _hidden_spec(eng, False).items()}
    act2 = {k: (v[Bs * T:] if k in ("F1", "Hf") else v[Bs:]) for k, v in full2.items()}
    st = orc.TrainState(params={k: v.double() for k, v in state.params.items()}, lr=LR)
    st.momentum = {k: v.double() for k, v in state.momentum.items()}
    res = orc.train_step(st, xs.double(), xt.double(), ys, BETA, GAMMA, cfg, clip=20.0, n_src=Bs, n_tgt=Bt, mu=c["mu"], masks=masks,
                         drop_i=mk1["drop_i"], drop_v=mk1["drop_v"], drop_rev=(mk2["drop_i"][1], mk2["drop_v"][1]),
                         masks_rev={k: v > 0 for k, v in act2.items()})
    for d, dom in enumerate(("src", "tgt")):
        for k, a in act[d].items():
            want = res[dom]["hidden"][k].detach()
            assert (a.double() - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item()), ("first pass", dom, k)
    for k, a in act2.items():
        want = res["tgt_rev"]["hidden"][k].detach()
        assert (a.double() - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item()), ("second pass", k)
    loss = eng.losses()["loss"] + float(eng.loss_c2) + float(eng.loss_s) + (float(eng.loss_e_shift[0]) if eng.loss_e_shift is not None else 0.0)
    assert abs(loss - res["loss"].item()) <= 2e-4 * max(1.0, abs(res["loss"].item())), (loss, res["loss"].item())
    assert abs(float(eng.loss_s) - res["parts"]["loss_s"].item()) <= 2e-4, (float(eng.loss_s), res["parts"]["loss_s"].item())
    _grad_parity(eng, res, "mcd p 0.5/0.5 step 0", lines)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
