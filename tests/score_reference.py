"""Score-only plans (TA3N_FLAG_SCORE_ONLY) restated for the tests: the score kernel's rules in float64 numpy with the explicit tie rule
(the lower class index is ahead), the launch list of a score plan executed with tests/plan_interp.py, and the fixtures' inputs.
Test infrastructure: nothing here is used by the product."""
import numpy as np
import torch

import rnn_reference as rr
import temconv_reference as tr
from golden_util import Golden, case_config, step_schedule
from plan_interp import (PH_GEMM, PH_POOL_AVG_FWD, PH_RNN_CELL_FWD, PH_RNN_POOL_FWD, PH_TEMCONV_FWD, Interp, sigmoid)
from ta3n_amd import _lib
from ta3n_amd.synthetic import synth_batch, synth_state

ALL_FLAGS = (_lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN)
EVAL_HYPER = dict(beta=[0.0, 0.0, 0.0], gamma=0.0, p_drop_i=0.0, p_drop_v=0.0, seed_i=0, seed_v=0, train=0, reverse=0, mu=0.0)
AGG = {"trn-m": _lib.AGG_TRN_M, "avgpool": _lib.AGG_AVGPOOL, "rnn": _lib.AGG_RNN, "temconv": _lib.AGG_TEMCONV}


# ---- the score kernel's rules ---------------------------------------------------------------------------------------------------
def score_rows(Y, labels):
    """Per-video outputs of the score kernel from the logits Y [n, C] (float64): dict(prob, ce, rank, pred)."""
    y = np.asarray(Y, np.float64)
    lab = np.asarray(labels, np.int64)
    n, C = y.shape
    if n == 0:
        return dict(prob=np.zeros((0, C)), ce=np.zeros(0), rank=np.zeros(0, np.int64), pred=np.zeros(0, np.int64))
    m = y.max(1, keepdims=True)
    e = np.exp(y - m)
    s = e.sum(1, keepdims=True)
    ylab = y[np.arange(n), lab]
    idx = np.arange(C)[None, :]
    rank = ((y > ylab[:, None]) | ((y == ylab[:, None]) & (idx < lab[:, None]))).sum(1)      # classes ahead of the label, torch.topk order
    return dict(prob=e / s, ce=(m[:, 0] + np.log(s[:, 0])) - ylab, rank=rank, pred=y.argmax(1))      # numpy's argmax: the FIRST maximum


def score_metrics(Y, labels):
    """What ta3n_score accumulates over the videos: dict(ce_sum, hits1, hits5, n, confusion [C, C] rows = label, cols = pred)."""
    r = score_rows(Y, labels)
    C = np.asarray(Y).shape[1]
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (np.asarray(labels, np.int64), r["pred"]), 1)
    return dict(ce_sum=float(r["ce"].sum()), hits1=int((r["rank"] < 1).sum()), hits5=int((r["rank"] < 5).sum()), n=len(r["rank"]), confusion=conf)


def classify(V, Wcv, bcv):
    return np.asarray(V, np.float64) @ np.asarray(Wcv, np.float64).T + np.asarray(bcv, np.float64)


def trn_front_end(Zr, tuple_first, Hr, W2, b2, attn_on):
    """The trn-m front end: Zr [B, NT, NB], Hr [B, NR, NB] (read only with attn_on), W2 [NR, 2, NB], b2 [NR, 2] -> (V [B, NB], attn [B, NR])."""
    B, _, NB = Zr.shape
    NR = len(tuple_first) - 1
    V = np.zeros((B, NB)); attn = np.zeros((B, NR))
    for j in range(NR):
        R = Zr[:, tuple_first[j]:tuple_first[j + 1], :].sum(1)
        if attn_on:
            z = Hr[:, j, :] @ W2[j].T + b2[j]
            _, _, H = Interp.soft2(z)
            attn[:, j] = 1 - H
        V += (1 + attn[:, j])[:, None] * R
    return V, attn


# ---- a score plan on the host ---------------------------------------------------------------------------------------------------
def run_group0(it):
    """Group 0 of a score plan through the interpreter.  The recurrent launches are restated here: Interp's own look up the backward
    regions ("rnn_gGx", ...) a score plan does not have."""
    g = it.g
    for ph in it.phases:
        assert ph.group == 0
        if ph.kind == PH_RNN_POOL_FWD:
            F1 = it.r(g.o_F1, (g.B, g.T, g.F))
            Xp, h = it.reg("rnn_Xp", (it.n_ts, g.B, g.F)), it.reg("rnn_h", (it.n_ts + 1, g.B, g.F))
            for j in range(it.n_ts):
                Xp[j] = F1[:, it.frames[j * it.len_ts:(j + 1) * it.len_ts], :].max(1)
            h[0] = 0
            if it.lstm:
                it.reg("rnn_c", (it.n_ts + 1, g.B, g.F))[0] = 0
        elif ph.kind == PH_RNN_CELL_FWD:
            s, G = ph.task_begin, 4 if it.lstm else 3
            x, r = it.reg("rnn_Gx", (it.n_ts, g.B, G, g.F))[s], it.reg("rnn_Gh", (it.n_ts, g.B, G, g.F))[s]
            h = it.reg("rnn_h", (it.n_ts + 1, g.B, g.F))
            if it.lstm:
                c = it.reg("rnn_c", (it.n_ts + 1, g.B, g.F))
                pre = x + r
                c[s + 1] = sigmoid(pre[:, 1]) * c[s] + sigmoid(pre[:, 0]) * np.tanh(pre[:, 2])
                h[s + 1] = sigmoid(pre[:, 3]) * np.tanh(c[s + 1])
            else:
                z = sigmoid(x[:, 1] + r[:, 1])
                h[s + 1] = (1 - z) * np.tanh(x[:, 2] + sigmoid(x[:, 0] + r[:, 0]) * r[:, 2]) + z * h[s]
            if s == it.n_ts - 1:
                it.r(g.o_V, (g.B, g.F))[:] = h[s + 1]
        else:
            assert ph.kind in (PH_GEMM, PH_POOL_AVG_FWD, PH_TEMCONV_FWD), ph.kind
            Interp.LAUNCH[ph.kind](it, ph, False)


def run_plan(plan, state, x, labels):
    """A score plan on the host in float64: group 0, then the score kernel's rules.  x [B, T, D] (torch), labels [B].
    Returns dict(Y, V, attn (trn-m) | None, prob, ce, rank, pred)."""
    it = Interp(plan)
    it.set_params(state)
    it.X = x.double().numpy().reshape(-1)
    it.hy = dict(EVAL_HYPER)
    run_group0(it)
    g = it.g
    attn = None
    if plan.cfg.aggregation == _lib.AGG_TRN_M:
        NR, NB = g.n_rel, g.NB
        attn_on = bool(g.flags & _lib.FLAG_TRANS_ATTN)
        Hr = it.r(g.o_Hr, (g.B, NR, NB)) if attn_on else None
        W2 = np.stack([it.w2(j)[0] for j in range(NR)]); b2 = np.stack([it.w2(j)[1] for j in range(NR)])
        V, attn = trn_front_end(it.r(g.o_Zr, (g.B, g.n_tuples, NB)), it.tf, Hr, W2, b2, attn_on)
    else:
        V = it.r(g.o_V, (g.B, g.F)).copy()
    width = V.shape[1]
    Y = classify(V, it.P[g.p_Wcv:g.p_Wcv + g.C * width].reshape(g.C, width), it.P[g.p_bcv:g.p_bcv + g.C])
    out = dict(Y=Y, V=V, attn=attn)
    out.update(score_rows(Y, labels))
    return out


# ---- the fixtures' configurations and inputs ------------------------------------------------------------------------------------
def case(name):
    """(Golden, config dict, plan keywords, state maker) of a fixture the score tests use; the flags are the training configuration's."""
    g = Golden(name)
    agg = str(g.meta("agg")) if g.has_meta("agg") else "trn-m"
    if agg == "rnn":
        g, c = rr.setup(name)
        kw = dict(aggregation=_lib.AGG_RNN, rnn_cell=_lib.RNN_CELLS[c["rnn_cell"]], n_ts=c["n_ts"])
        return g, c, kw, lambda shapes: rr.state_of(shapes, c)
    if agg == "temconv":
        g, c = tr.setup(name)
        return g, c, dict(aggregation=_lib.AGG_TEMCONV), lambda shapes: tr.state_of(shapes, c)
    c = case_config(g)
    c["flags"] = ALL_FLAGS if agg == "trn-m" else 0
    return g, c, dict(aggregation=AGG[agg]), lambda shapes: synth_state(shapes, seed=c["wseed"], scale=c["wscale"])


def score_plan(c, kw, T=None, capacity=None, flags=None):
    return _lib.Plan(c["Bs"] + c["Bt"] if capacity is None else capacity, 0, c["T"] if T is None else T, c["D"], c["fc_dim"], c["C"],
                     (c["flags"] if flags is None else flags) | _lib.FLAG_SCORE_ONLY, **kw)


def train_plan(c, kw, T=None, flags=None):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"] if T is None else T, c["D"], c["fc_dim"], c["C"], c["flags"] if flags is None else flags, **kw)


def first_batch(c):
    """The batch of the fixture's recorded forward (step 0): x [Bs + Bt, T, D], labels [Bs + Bt]."""
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    return torch.cat((xs, xt), 0), torch.cat((ys, yt))


def eval_batch(g, c):
    """The clips of the fixture's recorded validation pass (eval/out_t): x [Bs, val_T, D], labels [Bs]."""
    val_T = int(g.meta("val_T"))
    xv, _, yv, _ = synth_batch(c["C"], val_T, c["D"], c["Bs"], c["Bt"], seed=c["xseed"] + 7)
    return xv, yv, val_T
