"""Training meters (TA3N_FLAG_TRAIN_METERS, include/ta3n_hip.h): what one meters launch adds to regions "meter_counts" / "meter_sums".

Two independent statements of the launch, and the crafted cases both the CPU and the GPU tests run them on:
  - reference_step: the specification row by row in plain Python, float64 sums - the reference everything is compared with;
  - MetersInterp: plan_interp.Interp with the new launch kind (23) wired in, vectorised numpy over the interpreter's workspace, so a
    flagged plan's launch lists run end to end on the CPU.
"""
import math

import numpy as np

import plan_interp
from ta3n_amd import _lib

PH_TRAIN_METERS = 23
WORDS, SUMS = _lib.METER_WORDS, _lib.METER_SUMS
STEPS, NONFINITE, ROWS, TOP1, TOP5, LAST_ROWS, LAST_TOP1, LAST_TOP5, DOMAIN = 0, 1, 2, 3, 4, 5, 6, 7, 8
LEVEL_REGION = ("Pr", "Pv", "Pf")
LEVEL_FLAG = (_lib.FLAG_ADV_RELATION, _lib.FLAG_ADV_VIDEO, _lib.FLAG_ADV_FRAME)


def rows_per_video(level, T):
    return (T - 1, 1, T)[level]


def counted_levels(plan):
    """The levels a flagged plan counts: the ADV flag is set and the plan holds the level's logits row by row."""
    Bs, Bt, T = plan.cfg.batch_source, plan.cfg.batch_target, plan.cfg.num_segments
    trn = plan.cfg.aggregation == _lib.AGG_TRN_M
    out = []
    for l in range(3):
        per = rows_per_video(l, T) if (l or trn) else 0
        size = plan.regions.get(LEVEL_REGION[l], (0, 0))[1]
        out.append(bool(plan.cfg.flags & LEVEL_FLAG[l]) and per > 0 and size == (Bs + Bt) * per * 2)
    return out


def new_state():
    return dict(counts=np.zeros(WORDS, np.int64), sums=np.zeros(SUMS, np.float64))


def rank_of_label(y, label):
    """Classes ahead of the label in torch.topk order: a larger logit, or an equal one with a lower class index."""
    return sum(1 for c, v in enumerate(y) if v > y[label] or (v == y[label] and c < label))


def reference_step(state, case, levels):
    """One launch on `case` (crafted_case / any dict with the same keys), row by row."""
    c, s = state["counts"], state["sums"]
    Bs, Bt, T = case["Bs"], case["Bt"], case["T"]
    vs, vt = case["valid_source"], case["valid_target"]
    c[STEPS] += 1
    if not math.isfinite(float(case["losses"][0])):
        c[NONFINITE] += 1
        return
    for i in range(6):
        s[i] += float(case["losses"][i])      # (fp32 -> float64 is exact)
    rows = top1 = top5 = 0
    for b in range(min(vs, Bs)):
        r = rank_of_label(case["Y"][b], int(case["labels"][b]))
        rows += 1; top1 += r < 1; top5 += r < 5
    c[ROWS] += rows; c[TOP1] += top1; c[TOP5] += top5
    c[LAST_ROWS], c[LAST_TOP1], c[LAST_TOP5] = rows, top1, top5
    for l in range(3):
        if not levels[l]:
            continue
        per, P = rows_per_video(l, T), case[LEVEL_REGION[l]]
        for row in range((Bs + Bt) * per):
            b = row // per
            src = b < Bs
            if not (b < vs if src else b - Bs < vt):
                continue
            predicts_target = bool(P[row, 1] > P[row, 0])      # a tie predicts source
            w = DOMAIN + 4 * l + (0 if src else 2)
            c[w] += 1
            c[w + 1] += predicts_target != src


class MetersInterp(plan_interp.Interp):
    """The interpreter of the plan's launch lists with the meters launch; the two regions are kept beside the float workspace."""
    LAUNCH = dict(plan_interp.Interp.LAUNCH)
    LAUNCH[PH_TRAIN_METERS] = lambda it, ph, fused_norm: it.run_train_meters()

    def __init__(self, plan, dtype=np.float64):
        super().__init__(plan, dtype)
        self.meters = new_state()
        self.levels = counted_levels(plan)

    def run_train_meters(self):
        g, h, c = self.g, self.hy, self.meters["counts"]
        L = self.ws[g.o_losses:g.o_losses + 6].astype(np.float64)
        c[STEPS] += 1
        if not np.isfinite(L[0]):
            c[NONFINITE] += 1
            return
        self.meters["sums"][:6] += L
        n = min(h["valid_source"], g.Bs)
        Y, lab = self.r(g.o_Y, (g.B, g.C))[:n], self.labels[:n]
        ylab = Y[np.arange(n), lab][:, None]
        ahead = ((Y > ylab) | ((Y == ylab) & (np.arange(g.C)[None, :] < lab[:, None]))).sum(1)
        now = np.array([n, (ahead < 1).sum(), (ahead < 5).sum()])
        c[ROWS:ROWS + 3] += now
        c[LAST_ROWS:LAST_ROWS + 3] = now
        b = np.arange(g.B)
        valid = np.where(b < g.Bs, b < h["valid_source"], b - g.Bs < h["valid_target"])
        for l, (off, per) in enumerate(((g.o_Pr, g.n_rel), (g.o_Pv, 1), (g.o_Pf, g.T))):
            if not self.levels[l]:
                continue
            P = self.r(off, (g.B * per, 2))
            v, src, tgt_pred = np.repeat(valid, per), np.repeat(b < g.Bs, per), P[:, 1] > P[:, 0]
            for d, dom in enumerate((src, ~src)):
                c[DOMAIN + 4 * l + 2 * d] += (v & dom).sum()
                c[DOMAIN + 4 * l + 2 * d + 1] += (v & dom & (tgt_pred == bool(d))).sum()


# (Bs, Bt, T, C), (valid_source, valid_target) or None: include/ta3n_hip.h's launch at every size at which it takes another path
CRAFTED = [
    ((6, 4, 5, 12), (5, 3)),      # dummy rows written as would-be hits must not count
    ((3, 70, 2, 1), None),        # one class, one relation, more target than source
    ((70, 3, 3, 64), None),       # 64 classes (every lane a class), more wave items than one workgroup holds
    ((1, 0, 5, 7), None),         # one video, no target
    ((2, 2, 64, 5), None),        # 256 frame rows, fewer than six classes: every row a top-5 hit
]
FEATURE_DIM, FC_DIM = 64, 32     # (the meters never read a feature: the smallest plan)
ALL_ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN


def crafted_plan(shape, flags=ALL_ADV):
    Bs, Bt, T, C = shape
    return _lib.Plan(Bs, Bt, T, FEATURE_DIM, FC_DIM, C, flags | _lib.FLAG_TRAIN_METERS)


def crafted_case(shape, valid=None, seed=0):
    """fp32 logits, labels and loss slots of one step.  Logits are multiples of 1/8 in a small range, so ties are frequent and exact.
    Rows 0..2 (where the shape has them and at least seven classes) are the tie rules: the label tied with four lower classes (rank 4: a top-5
    hit), with five lower classes (rank 5: a miss), with higher classes only (rank 0: top-1).  Dummy rows carry their label as the clear
    maximum and domain logits that would be correct.  Every fourth domain row has equal logits (predicts source)."""
    Bs, Bt, T, C = shape
    B = Bs + Bt
    vs, vt = valid if valid is not None else (Bs, Bt)
    rng = np.random.default_rng(1000 + seed)
    Y = (rng.integers(-16, 17, size=(B, C)) / 8.0).astype(np.float32)
    labels = rng.integers(0, C, size=B).astype(np.int32)
    if Bs >= 3 and C >= 7:
        for row, (lab, lower, higher) in enumerate(((4, 4, 0), (5, 5, 0), (0, 0, 3))):
            Y[row] = -3.0
            labels[row] = lab
            Y[row, lab - lower:lab + higher + 1] = 1.5
    for b in range(vs, Bs):
        Y[b, labels[b]] = 9.0
    case = dict(Bs=Bs, Bt=Bt, T=T, C=C, valid_source=vs, valid_target=vt, Y=Y, labels=labels)
    for l, name in enumerate(LEVEL_REGION):
        per = rows_per_video(l, T)
        P = (rng.integers(-8, 9, size=(B * per, 2)) / 8.0).astype(np.float32)
        P[::4, 1] = P[::4, 0]
        for b in list(range(vs, Bs)) + list(range(Bs + vt, B)):
            P[b * per:(b + 1) * per] = (2.0, -2.0) if b < Bs else (-2.0, 2.0)
        case[name] = P
    parts = (rng.integers(1, 4000, size=5) / 1024.0).astype(np.float32)
    gamma = np.float32(0.003)
    total = np.float32(parts[0] + parts[1] + parts[2] + parts[3] + gamma * parts[4])
    case["losses"] = np.array([total, *parts], np.float32)
    return case


def load_case(it, case):
    """A crafted case into a MetersInterp's workspace."""
    g = it.g
    n = max(case["valid_source"] + case["valid_target"], 1)      # (the loss kernel's scalars too: the loss list can run on the case)
    it.hy = dict(valid_source=case["valid_source"], valid_target=case["valid_target"], beta=[0.75, 0.75, 0.5], gamma=0.003,
                 inv_n_cls=1.0 / max(case["valid_source"], 1), inv_n_rel=1.0 / (n * max(g.n_rel, 1)), inv_n_vid=1.0 / n, inv_n_frm=1.0 / (n * g.T),
                 inv_n_ent=1.0 / n)
    it.labels[:] = case["labels"]
    it.r(g.o_Y, (g.B, g.C))[:] = case["Y"]
    it.r(g.o_Pr, (g.B * g.n_rel, 2))[:] = case["Pr"]
    it.r(g.o_Pv, (g.B, 2))[:] = case["Pv"]
    it.r(g.o_Pf, (g.B * g.T, 2))[:] = case["Pf"]
    it.ws[g.o_losses:g.o_losses + 6] = case["losses"]
