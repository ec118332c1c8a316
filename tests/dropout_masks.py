"""The kernels' dropout masks, rebuilt on the host (test infrastructure; a plain helper module).

The dropout stream is stateless: keep(seed, element id, p) (ta3n_amd/csrc/ta3n_kernels.h: keep_mask; tests/plan_interp.py: keep_mask is its
bit-exact numpy twin, u >= p compared in fp32).  Every site that applies dropout recomputes the element id on its own, picks its seed
and its p, and multiplies by 1 / (1 - p) on its own.  The ids, per stream ("Dropout element ids"):
  * dropout_i (seed_i, p_drop_i), on the shared frame features [B T, F]:  id = row F + col, row counted over the COMBINED
    [source; target] batch - target rows start at Bs T.  The k-th stacked shared layer of --add_fc k (k = 1 the first) adds
    (k - 1) (Bs + Bt) T F, in uint32 arithmetic.
  * dropout_v (seed_v, p_drop_v), on the video feature [B, NV]:  id = b NV + col, b over the combined batch; NV = 256 on trn-m, F on
    avgpool.
This module derives the masks from those formulas and NOTHING of the kernels' output, so that a test can hand them to the oracle
(oracle.train_step(drop_i=, drop_v=)) and compare numbers with dropout ON: a site that forgets 1 / (1 - p), takes the other stream's p
or seed, or counts target rows from 0 then disagrees with the oracle (tests/test_dropout_cpu.py on the launch plans executed with
numpy, tests/test_gpu_dropout_parity.py on the kernels).  Also here: the comparators those two test files share."""
import numpy as np
import torch

from golden_util import Golden, case_config
from oracle import ta3n_oracle as orc
from plan_interp import keep_mask
from ta3n_amd.synthetic import synth_batch

U32 = 0xFFFFFFFF


def keep_rows(seed, p, row0, rows, cols, offset=0):
    """0/1 float64 [rows, cols]: the keep pattern of the elements (row0 + r) cols + c + offset of stream `seed`.  p >= 1 drops everything
    (the stream's u < 1 always), p <= 0 keeps everything."""
    if p >= 1.0:
        return np.zeros((rows, cols))
    idx = ((np.arange(row0, row0 + rows, dtype=np.uint64)[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]
            + np.uint64(offset & U32)) & np.uint64(U32))
    return keep_mask(int(seed) & U32, idx, p)


def inv_keep(p):
    """1 / (1 - p); 0 at p >= 1 (everything is dropped: the kernels' hyper_scale gives 0 there, not inf)."""
    return 0.0 if p >= 1.0 else 1.0 / (1.0 - p)


def dropout_masks(seed_i, seed_v, p_i, p_v, Bs, Bt, T, F, NV, layer=1, target_row0=None, scale_v=True):
    """Per-domain multiplicative masks of one forward pass, already scaled by 1 / (1 - p), as float64 torch tensors:
    dict(drop_i=(src [Bs T, F], tgt [Bt T, F]), drop_v=(src [Bs, NV], tgt [Bt, NV]), keep_i=(...), keep_v=(...)) - keep_*: the 0/1 patterns.
    layer: which stacked shared layer of --add_fc (1 = the first / only one).
    target_row0 / scale_v exist for NEGATIVE CONTROLS only (what a wrong kernel would do): target_row0 = 0 counts the target rows from 0
    instead of from Bs, scale_v = False leaves drop_v without its 1 / (1 - p_v)."""
    t0 = Bs if target_row0 is None else target_row0
    off = ((layer - 1) * (Bs + Bt) * T * F) & U32
    ki = (keep_rows(seed_i, p_i, 0, Bs * T, F, off), keep_rows(seed_i, p_i, t0 * T, Bt * T, F, off))
    kv = (keep_rows(seed_v, p_v, 0, Bs, NV), keep_rows(seed_v, p_v, t0, Bt, NV))
    sv = inv_keep(p_v) if scale_v else 1.0
    tt = torch.from_numpy
    return dict(keep_i=tuple(tt(k) for k in ki), keep_v=tuple(tt(k) for k in kv),
                drop_i=tuple(tt(k * inv_keep(p_i)) for k in ki), drop_v=tuple(tt(k * sv) for k in kv))


# ---- comparators shared by tests/test_dropout_cpu.py (launch plans executed with numpy) and tests/test_gpu_dropout_parity.py (kernels) ----
EXCLUDE_REL = 1e-4       # pattern check: entries with |pre-activation| <= EXCLUDE_REL * max |pre-activation| may sit on either side of the ReLU
EXCLUDE_SHARE = 0.01     # ... and must be at most this share of the tensor (a condition on the test's data, checked from the float64 oracle alone)


def excluded(pre):
    """(bool mask of the entries too close to the ReLU kink to be compared, their share) of a float64 pre-activation tensor."""
    pre = torch.as_tensor(pre).double()
    ex = pre.abs() <= EXCLUDE_REL * pre.abs().max()
    return ex, ex.double().mean().item()


def check_frame_pattern(F1, pre, keep_i, what=""):
    """Exact pattern of one shared frame layer's output F1 (all rows of the combined batch) against the host mask: zero exactly wherever
    the host stream drops, and - away from the ReLU kink - nonzero exactly where the host stream keeps an active unit.  Returns the
    excluded share (asserted <= EXCLUDE_SHARE)."""
    F1, pre, keep = torch.as_tensor(F1).double(), torch.as_tensor(pre).double(), torch.as_tensor(keep_i).double()
    assert F1.shape == pre.shape == keep.shape, (what, F1.shape, pre.shape, keep.shape)
    ex, share = excluded(pre)
    assert share <= EXCLUDE_SHARE, (what, "excluded share", share)
    assert bool((F1[keep == 0] == 0).all()), (what, "a dropped entry is not zero", int((F1[keep == 0] != 0).sum()))
    want = (keep == 1) & (pre > 0)
    bad = ((F1 != 0) != want) & ~ex
    assert not bool(bad.any()), (what, "nonzero pattern differs from host keep & active", int(bad.sum()), F1.numel())
    return share


def check_video_pattern(V, Vd, gVt, keep_v, p_v, what=""):
    """dropout_v forward and backward: Vd = 0 exactly where the host stream drops and V / (1 - p_v) where it keeps; the gradient that
    leaves dropout_v towards V (gVt; None: the plan has no such region) is 0 exactly where the host stream drops."""
    V, Vd, keep = torch.as_tensor(V).double(), torch.as_tensor(Vd).double(), torch.as_tensor(keep_v).double()
    assert V.shape == Vd.shape == keep.shape, (what, V.shape, Vd.shape, keep.shape)
    assert bool((Vd[keep == 0] == 0).all()), (what, "a dropped video feature is not zero")
    on = keep == 1
    assert torch.allclose(Vd[on], V[on] * inv_keep(p_v), rtol=1e-6, atol=0.0), (what, "kept video features are not V / (1 - p_v)")
    if gVt is not None:
        gVt = torch.as_tensor(gVt).double()
        assert bool((gVt[keep == 0] == 0).all()), (what, "the gradient behind a dropped video feature is not zero")


def rel_l2(got, want):
    """{name: ||got - want|| / ||want||} over the tensors of `want` (every element)."""
    out = {}
    for k, w in want.items():
        w = torch.as_tensor(w).detach().double().cpu()
        d = torch.as_tensor(got[k]).detach().double().cpu().reshape(w.shape) - w
        out[k] = (d.pow(2).sum().sqrt() / (w.pow(2).sum().sqrt() + 1e-300)).item()
    return out


def summary(per, tag):
    """(median, worst, line) of a rel_l2 result, the line in the format tests/test_gpu_masked_gradients.py prints."""
    med = float(np.median(list(per.values())))
    top = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    return med, top[0][1], f"[dropout parity] {tag}: median rel. L2 {med:.2e}; worst " + ", ".join(f"{k} {v:.2e}" for k, v in top)


# ---- the cases of tests/test_gpu_dropout_parity.py (their excluded-share condition is checked on the CPU by tests/test_dropout_cpu.py) ----
BETA, GAMMA, LR = [0.75, 0.75, 0.5], 0.003, 2e-3
TINY = dict(Bs=6, Bt=4, T=5, D=512, F=64, C=12)
RAGGED = dict(Bs=40, Bt=30, T=3, D=256, F=128, C=7)


def _golden_case(name):
    c = case_config(Golden(name))
    return dict(Bs=c["Bs"], Bt=c["Bt"], T=c["T"], D=c["D"], F=c["fc_dim"], C=c["C"]), c


def oracle_cases():
    """{case: (oracle Config factory(p_i, p_v), shape, weight seed, weight scale, data seed, [(p_i, p_v)], [(n_src, n_tgt) per step])} of
    the cases of tests/test_gpu_dropout_parity.py whose pattern check reads the oracle's pre-activation - tests/test_dropout_cpu.py checks
    their excluded-share condition on the CPU."""
    def trn(shape, **kw):
        return lambda p_i, p_v: orc.Config(num_class=shape["C"], num_segments=shape["T"], feature_dim=shape["D"], fc_dim=shape["F"],
                                           dropout_i=p_i, dropout_v=p_v, **kw)
    avg_shape, avg = _golden_case("tiny_avgpool_da")
    src_shape, src = _golden_case("tiny_avgpool")
    bn_shape, bn = _golden_case("tiny_adabn")
    return {
        "trn-m": (trn(TINY), TINY, 11, "trained", 21, [(0.5, 0.5), (0.3, 0.8)], [(6, 4), (6, 4)]),
        "ragged": (trn(RAGGED), RAGGED, RAGGED_WSEED, "trained", 21, [(0.3, 0.8)], [(40, 30), (37, 25)]),
        "avgpool_da": (trn(avg_shape, place_adv=avg["place_adv"], add_loss_DA="none", use_attn="none", frame_aggregation="avgpool"),
                       avg_shape, avg["wseed"], avg["wscale"], avg["xseed"], [(0.3, 0.8)], [(avg["Bs"], avg["Bt"])] * 2),
        "avgpool_src": (trn(src_shape, place_adv=("N", "N", "N"), add_loss_DA="none", use_attn="none", frame_aggregation="avgpool"),
                        src_shape, src["wseed"], src["wscale"], src["xseed"], [(0.3, 0.8)], [(src["Bs"], src["Bt"])] * 2),
        "adabn": (trn(bn_shape, use_bn=bn["use_bn"]), bn_shape, bn["wseed"], bn["wscale"], bn["xseed"], [(0.5, 0.5), (0.3, 0.8)],
                  [(bn["Bs"], bn["Bt"])] * 2),
    }


# The ragged case's second step zeroes 8 of its 70 videos; a zero row's pre-activation IS the bias, and ~10 % of a trained-scale bias
# vector lies within 1e-4 of the tensor's largest pre-activation - 1.2 % of the tensor at weight seed 11, whatever the data seed.  The
# excluded-share condition is met by the weight seed instead (0.48 % at 12; tests/test_dropout_cpu.py asserts it).
RAGGED_WSEED = 12


def batch(shape, xseed, s, ns, nt):
    xs, xt, ys, yt = synth_batch(shape["C"], shape["T"], shape["D"], shape["Bs"], shape["Bt"], seed=xseed + 7 * s)
    xs[ns:] = 0; xt[nt:] = 0
    return xs, xt, ys


def preactivation(cfg, params, xs, xt):
    """The oracle's own float64 pre-activation of the shared frame layer (post-BatchNorm with use_bn), combined batch [B T, F]."""
    p = {k: v.detach().double().cpu() for k, v in params.items()}
    with torch.no_grad():
        s = orc.forward_domain(p, xs.double(), BETA, cfg, domain="S")
        t = orc.forward_domain(p, xt.double(), BETA, cfg, domain="T")
    return torch.cat((s["pre_f1"], t["pre_f1"]))
