"""The eight-wave video workgroups of the heads kernel (ta3n_heads.hip, NW == 8: one video per workgroup, at most 4 relations, fc_dim
<= 512) against the four-wave kernel in the same process (ta3n_set_heads_waves) and against the float64 oracle.

Cases (Bs, Bt, T, D, F, C), NB = 256: the MID shape of tests/golden/make_plan_fingerprints.py (four relations, eight waves) and
one change at a time - 1 / 2 relations (seven / six waves without one), 5 relations (must stay on the untouched PIPE kernel), 1 / 13 /
64 classes (class lanes; the predicate of the classifier-weight loads, no multiple of the thread count), one video and no target,
the largest one-video-per-workgroup batch and the first two-per-workgroup one (must stay on VPW == 2), fc_dim 20 (k < F guards beside
idle frame waves) and 96 (FQ 2; on D = 96, the plan's fc_dim being min(F, D)).  Every test first asserts from the library which
kernel the plan gets (ta3n_get_heads_waves).

 (a) four against eight waves, fp32 with dropout 0.5 / 0.5 and bf16 twins: BIT-IDENTICAL in every region of the forward and of the
     frame workgroups (Y, Pr, attn, R, V, Vd, Hv, Pv, Pf, gY, gPv, gHv, gPr, gPf, gHf and its bf16 twin, the frame partials); the regions
     behind stage F (gVt, gRa, gPrT, gHr) and the loss partials within F32_RTOL / F32_ATOL elementwise - and, since the eight-wave
     kernel runs stage F's chain over an srow's 16 rows in the four-wave order (two halves handed over through LDS), the four
     gradient regions bit-identical as well (a step on eight waves then IS the step on four: tests/test_gpu_training_equivalence.py
     follows 300 of them).  Where both settings must select the same four-wave kernel, everything is bit-identical.
 (b) the eight-wave step against the float64 oracle on the kernels' own dropout masks and ReLU patterns (the recipe and bounds of
     tests/test_gpu_dropout_parity.py: F32_MASKED_GRAD_REL_L2 per tensor and its median, hidden activations, loss, plus the logits at
     limit_shapes.logit_bound), dropout off and 0.5 / 0.5; and on bf16 twins against the bf16-operand oracle with
     tests/test_gpu_bf16.py's gate and bounds."""
import pytest
import torch

import limit_shapes as ls
from dropout_masks import BETA, GAMMA, LR, dropout_masks
from oracle import ta3n_oracle as orc
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, dropout_seeds
from ta3n_amd.synthetic import synth_batch, synth_state
from test_gpu_bf16 import _oracle_gate, _print_report
from test_gpu_dropout_parity import _engine_masks, _grad_parity, _oracle

pytestmark = pytest.mark.gpu

MID = (6, 5, 5, 64, 32, 8)
# name: ((Bs, Bt, T, D, F, C), waves the automatic choice must give)
CASES = {
    "mid_four_relations": (MID, 8),
    "T2_one_relation": ((6, 5, 2, 64, 32, 8), 8),
    "T3_two_relations": ((6, 5, 3, 64, 32, 8), 8),
    "T6_pipe_kernel": ((6, 5, 6, 64, 32, 8), 4),
    "C1": ((6, 5, 5, 64, 32, 1), 8),
    "C13": ((6, 5, 5, 64, 32, 13), 8),
    "C64": ((6, 5, 5, 64, 32, 64), 8),
    "one_video_no_target": ((1, 0, 5, 64, 32, 8), 8),
    "b224_largest_one_per_wg": ((112, 112, 5, 64, 32, 8), 8),
    "b225_two_per_wg": ((113, 112, 5, 64, 32, 8), 4),
    "F20": ((6, 5, 5, 64, 20, 8), 8),
    "F96_fq2": ((6, 5, 5, 96, 96, 8), 8),
}
WSEED, XSEED, CLIP = 11, 21, 20.0

EXACT = ("Y", "Pr", "attn", "R", "V", "Vd", "Hv", "Pv", "Pf", "gY", "gPv", "gHv", "gPr", "gPf", "gHf", "fh_part", "fh_bpart")
BEHIND_F = ("gVt", "gRa", "gPrT", "gHr", "loss_part")


@pytest.fixture(autouse=True)
def _automatic_choice_afterwards():
    yield
    _lib.check(_lib.lib().ta3n_set_heads_waves(0), "ta3n_set_heads_waves")


def _set_waves(w):
    _lib.check(_lib.lib().ta3n_set_heads_waves(w), "ta3n_set_heads_waves")


def _waves_of(eng):
    return _lib.lib().ta3n_get_heads_waves(eng.plan.handle)


def _cfg(shape, p_i, p_v):
    Bs, Bt, T, D, F, C = shape
    return orc.Config(num_class=C, num_segments=T, feature_dim=D, fc_dim=F, dropout_i=p_i, dropout_v=p_v)


def _stepped_engine(shape, waves, p, bf16):
    """An engine of `shape` after one train step on the fixed inputs, run with ta3n_set_heads_waves(waves)."""
    Bs, Bt, T, D, F, C = shape
    _set_waves(waves)
    eng = TrainEngine(Bs, Bt, T, D, F, C, dropout_i=p, dropout_v=p, clip=CLIP, **(dict(bf16=True, bf16_store=True) if bf16 else {}))
    assert eng.fused and eng.plan.has_fused_step
    eng.load_state(synth_state(orc.param_shapes(_cfg(shape, p, p)), seed=WSEED, scale="trained"))
    xs, xt, ys, _ = synth_batch(C, T, D, Bs, Bt, seed=XSEED)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(BETA, GAMMA, LR, seed=0)
    torch.cuda.synchronize()
    return eng


def _trim(v):
    if torch.is_tensor(v):
        return v[:0]
    if isinstance(v, dict):
        return {k: _trim(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_trim(x) for x in v)
    return v


@pytest.fixture
def oracle_without_target(monkeypatch):
    """The oracle reshapes an empty target batch to [0, T, -1] and stops there.  For the one-video case it gets ONE dummy target row of
    zeros with n_tgt = 0 (dummy rows take part in no loss: the ragged steps of tests/limit_shapes.py), all-on patterns and masks for that
    row, and the row is cut from what it returns - so the helpers of the other test files see the engine's shapes."""
    real = orc.train_step

    def step(state, xs, xt, *args, **kw):
        if xt.shape[0] != 0:
            return real(state, xs, xt, *args, **kw)
        assert xs.shape[0] == 1
        kw = dict(kw, n_tgt=0)
        if kw.get("masks") is not None:
            kw["masks"] = (kw["masks"][0], {k: torch.ones_like(v) for k, v in kw["masks"][0].items()})
        for key in ("drop_i", "drop_v"):
            if kw.get(key) is not None:
                kw[key] = (kw[key][0], torch.ones_like(kw[key][0]))
        res = real(state, xs, xt.new_zeros((1,) + tuple(xt.shape[1:])), *args, **kw)
        res["tgt"] = _trim(res["tgt"])
        return res
    monkeypatch.setattr(orc, "train_step", step)


def test_the_setting_takes_0_4_8_and_nothing_else():
    L = _lib.lib()
    for w in (4, 8, 0):
        assert L.ta3n_set_heads_waves(w) == 0
    for w in (-1, 1, 2, 6, 16):
        assert L.ta3n_set_heads_waves(w) == -1 and b"heads waves" in L.ta3n_last_error()


@pytest.mark.parametrize("arith", ["fp32_dropout", "bf16_twins"])
@pytest.mark.parametrize("name", list(CASES))
def test_eight_waves_against_four_waves(name, arith, capsys):
    shape, auto = CASES[name]
    bf16 = arith == "bf16_twins"
    runs = {}
    for w in (4, 8):
        eng = _stepped_engine(shape, w, 0.0 if bf16 else 0.5, bf16)
        assert _waves_of(eng) == (w if auto == 8 else 4), (name, w, _waves_of(eng))
        runs[w] = (eng, eng.ws.detach().cpu().clone())
        _set_waves(0)
        assert _waves_of(eng) == auto, (name, "automatic", _waves_of(eng))
    (e4, ws4), (e8, ws8) = runs[4], runs[8]
    assert e4.plan.regions == e8.plan.regions and e4.plan.description == e8.plan.description      # the setting is not a plan's business
    cut = lambda ws, r: ws[e4.plan.region(r)[0]:e4.plan.region(r)[0] + e4.plan.region(r)[1]]
    for r in EXACT:
        assert torch.equal(cut(ws4, r).view(torch.int32), cut(ws8, r).view(torch.int32)), (name, arith, r)
    if bf16:      # the bf16 twin of gHf: 16-bit elements at the region's element offset behind ws16
        o16, (oH, nH) = e4.plan.region("ws16")[0], e4.plan.region("gHf")
        twin = lambda ws: ws[o16:].view(torch.int16)[oH:oH + nH]
        assert torch.equal(twin(ws4), twin(ws8)), (name, "gHf twin")
        assert bool((twin(ws8) != 0).any())
    worst = {}
    for r in BEHIND_F:
        a, b = cut(ws8, r), cut(ws4, r)
        if auto == 4 or r != "loss_part":
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, arith, r, "one kernel, two results")
        err = (a.double() - b.double()).abs()
        assert bool((err <= tol.F32_ATOL + tol.F32_RTOL * b.double().abs()).all()), (name, arith, r, float(err.max()))
        worst[r] = float(err.max() / (b.double().abs().max() + 1e-30))
    assert bool(cut(ws8, "gVt").any()) and bool(cut(ws8, "gHr").any())
    with capsys.disabled():
        print(f"\n[heads waves 8 vs 4] {name} {arith}: max |difference| / max |value| " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["dropout_off", "dropout_on"])
@pytest.mark.parametrize("name", list(CASES))
def test_eight_wave_step_against_the_float64_oracle(name, p, capsys, oracle_without_target):
    shape, auto = CASES[name]
    Bs, Bt, T, D, F, C = shape
    cfg = _cfg(shape, p, p)
    _set_waves(8)
    eng = TrainEngine(Bs, Bt, T, D, F, C, dropout_i=p, dropout_v=p, clip=CLIP)
    assert eng.fused and _waves_of(eng) == auto
    eng.load_state(synth_state(orc.param_shapes(cfg), seed=WSEED, scale="trained"))
    xs, xt, ys, _ = synth_batch(C, T, D, Bs, Bt, seed=XSEED)
    state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
    state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(BETA, GAMMA, LR, seed=0)
    torch.cuda.synchronize()
    tag = f"heads waves {_waves_of(eng)}, {name} p {p}"
    mk = dropout_masks(*dropout_seeds(0, 0), p, p, Bs, Bt, T, F, 256)
    masks, act = _engine_masks(eng, False)
    res = _oracle(cfg, state, xs, xt, ys, GAMMA, Bs, Bt, mk, masks)
    for d, (dom, nv) in enumerate((("src", Bs), ("tgt", Bt))):
        for k, a in act[d].items():
            want = res[dom]["hidden"][k].detach()
            err = (a.double() - want).abs().max().item() if nv else 0.0
            assert err <= 2e-4 * max(1.0, want.abs().max().item() if nv else 0.0), (tag, dom, k, err)
    o, lerr = eng.outputs(), 0.0
    for k, w in ls.oracle_logits(res, Bs, Bt).items():
        err = float((o[k].detach().cpu().double().reshape(w.shape) - w).abs().max())
        lerr = max(lerr, err)
        assert err <= ls.logit_bound(w), (tag, k, err)
    loss = eng.losses()["loss"]
    assert abs(loss - res["loss"].item()) <= 2e-4 * max(1.0, abs(res["loss"].item())), (tag, loss, res["loss"].item())
    lines = [f"[heads waves vs float64] {tag}: logits max error {lerr:.1e}, loss {loss:.6f} (oracle {res['loss'].item():.6f})"]
    _grad_parity(eng, res, tag, lines, exempt=None)      # (a tensor may be tiny only where the oracle's is exactly zero: one class)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", list(CASES))
def test_eight_wave_bf16_step_matches_the_bf16_operand_oracle(name, capsys, oracle_without_target):
    shape, auto = CASES[name]
    _set_waves(8)
    rep, bad = _oracle_gate(dict(zip(("Bs", "Bt", "T", "D", "F", "C"), shape)), wseed=WSEED, wscale="trained", xseed=XSEED, lr=1e-3, clip=CLIP)
    with capsys.disabled():
        _print_report(f"heads waves, {name}", rep)
    assert not bad, bad
