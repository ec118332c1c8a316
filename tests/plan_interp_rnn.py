"""plan_interp.Interp with the four launches of the recurrent aggregator (TA3N_AGG_RNN; ta3n_amd/csrc/ta3n_rnn.hip), executed from their
specification: slot max-pooling, one LSTM / GRU cell step, and both ways back.  The GEMM launches between them run through Interp
like every other.  Test infrastructure."""
import numpy as np

from plan_interp import Interp
from ta3n_amd import _lib

PH_RNN_POOL_FWD, PH_RNN_CELL_FWD, PH_RNN_CELL_BWD, PH_RNN_POOL_BWD = 16, 17, 18, 19


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class RnnInterp(Interp):
    """cell: 'LSTM' / 'GRU', n_ts: as given to the plan.  The regions are found by name ("rnn_*"); a cell phase's step is its task_begin."""

    def __init__(self, plan, cell, n_ts, dtype=np.float64):
        super().__init__(plan, dtype)
        self.cell, self.n_ts = cell, n_ts
        self.len_ts, self.frames = _lib.rnn_slots(self.g.T, n_ts)
        self.G_ = 4 if cell == "LSTM" else 3

    def reg(self, name, shape):
        return self.r(self.plan.region(name)[0], shape)

    def _tensors(self):
        g, n, G = self.g, self.n_ts, self.G_
        B, F = g.B, g.F
        return dict(Xp=self.reg("rnn_Xp", (n, B, F)), Gx=self.reg("rnn_Gx", (n, B, G, F)), Gh=self.reg("rnn_Gh", (n, B, G, F)),
                    act=self.reg("rnn_gates", (n, B, G, F)), c=self.reg("rnn_c", (n + 1, B, F)), h=self.reg("rnn_h", (n + 1, B, F)),
                    gGx=self.reg("rnn_gGx", (n, B, G, F)), gGh=self.reg("rnn_gGh", (n, B, G, F)), gc=self.reg("rnn_gc", (n, B, F)),
                    gh=self.reg("rnn_gh", (B, F)), ghd=self.reg("rnn_ghd", (B, F)), gXp=self.reg("rnn_gXp", (n, B, F)))

    def run_rnn_pool_fwd(self):
        g, t = self.g, self._tensors()
        F1 = self.r(g.o_F1, (g.B, g.T, g.F))
        for j in range(self.n_ts):
            t["Xp"][j] = F1[:, self.frames[j * self.len_ts:(j + 1) * self.len_ts], :].max(1)
        t["h"][0] = 0
        if self.cell == "LSTM":
            t["c"][0] = 0

    def run_rnn_cell_fwd(self, s):
        g, h, t = self.g, self.hy, self._tensors()
        B, F = g.B, g.F
        x, r, act = t["Gx"][s], t["Gh"][s], t["act"][s]
        if self.cell == "LSTM":
            pre = x + r
            act[:, 0], act[:, 1], act[:, 2], act[:, 3] = sigmoid(pre[:, 0]), sigmoid(pre[:, 1]), np.tanh(pre[:, 2]), sigmoid(pre[:, 3])
            t["c"][s + 1] = act[:, 1] * t["c"][s] + act[:, 0] * act[:, 2]
            t["h"][s + 1] = act[:, 3] * np.tanh(t["c"][s + 1])
        else:
            act[:, 0], act[:, 1] = sigmoid(x[:, 0] + r[:, 0]), sigmoid(x[:, 1] + r[:, 1])
            act[:, 2] = np.tanh(x[:, 2] + act[:, 0] * r[:, 2])
            t["h"][s + 1] = (1 - act[:, 1]) * act[:, 2] + act[:, 1] * t["h"][s]
        if s == self.n_ts - 1:
            V = t["h"][s + 1]
            mk = np.ones((B, F), self.dtype)
            if h["train"] and h["p_drop_v"] > 0:
                from plan_interp import keep_mask
                mk = keep_mask(h["seed_v"], np.arange(B)[:, None] * F + np.arange(F)[None, :], h["p_drop_v"]) * self.scale(5)
            self.r(g.o_V, (B, F))[:] = V
            self.r(g.o_Vd, (B, F))[:] = V * mk
            self.ws[g.o_losses:g.o_losses + 8] = 0

    def run_rnn_cell_bwd(self, s):
        g, t = self.g, self._tensors()
        B, F = g.B, g.F
        last = s == self.n_ts - 1
        if last:
            gh = self.r(g.o_gVt, (B, F)).copy()
            if g.o_gV_ext > 0:
                gh = gh + self.r(g.o_gV_ext, (B, F))
        else:
            gh = t["gh"].copy()
        act, gGx, gGh = t["act"][s], t["gGx"][s], t["gGh"][s]
        if self.cell == "LSTM":
            i, f, gg, o = act[:, 0], act[:, 1], act[:, 2], act[:, 3]
            tc = np.tanh(t["c"][s + 1])
            gc = gh * o * (1 - tc * tc) + (0 if last else t["gc"][s + 1])
            gGx[:, 0] = gc * gg * i * (1 - i); gGx[:, 1] = gc * t["c"][s] * f * (1 - f)
            gGx[:, 2] = gc * i * (1 - gg * gg); gGx[:, 3] = gh * tc * o * (1 - o)
            gGh[:] = gGx
            t["gc"][s] = gc * f
            t["ghd"][:] = 0
        else:
            r, z, n = act[:, 0], act[:, 1], act[:, 2]
            dn = gh * (1 - z) * (1 - n * n)
            gGx[:, 2] = dn; gGh[:, 2] = dn * r
            gGx[:, 1] = gGh[:, 1] = gh * (t["h"][s] - n) * z * (1 - z)
            gGx[:, 0] = gGh[:, 0] = dn * t["Gh"][s][:, 2] * r * (1 - r)
            t["ghd"][:] = gh * z

    def run_rnn_pool_bwd(self):
        """The lowest frame index among equal candidates takes the window's gradient; frames in no window get zero."""
        g, t = self.g, self._tensors()
        B, T, F = g.B, g.T, g.F
        F1 = self.r(g.o_F1, (B, T, F))
        out = np.zeros((B, T, F), self.dtype)
        for j in range(self.n_ts):
            fr = np.asarray(self.frames[j * self.len_ts:(j + 1) * self.len_ts])
            first = F1[:, fr, :].argmax(1)                      # numpy's argmax returns the first maximum
            b, k = np.meshgrid(np.arange(B), np.arange(F), indexing="ij")
            np.add.at(out, (b, fr[first], k), t["gXp"][j])
        if g.o_gHf < 0:
            self.r(g.o_gZ1, (B, T, F))[:] = np.where(F1 > 0, out * self.scale(4), 0.0)
        else:
            self.r(g.o_gRa, (B, T, F))[:] = out

    def run_group(self, group, fused_norm=False):
        """Interp.run_group skips the kinds it does not know: it runs the stretches between two recurrent phases (as
        tests/plan_interp_general_attn.py does)."""
        kept = self.phases
        try:
            run = []
            for ph in kept:
                if ph.group != group:
                    continue
                if ph.kind in (PH_RNN_POOL_FWD, PH_RNN_CELL_FWD, PH_RNN_CELL_BWD, PH_RNN_POOL_BWD):
                    self.phases = run
                    Interp.run_group(self, group, fused_norm)
                    run = []
                    if ph.kind == PH_RNN_POOL_FWD: self.run_rnn_pool_fwd()
                    elif ph.kind == PH_RNN_CELL_FWD: self.run_rnn_cell_fwd(ph.task_begin)
                    elif ph.kind == PH_RNN_CELL_BWD: self.run_rnn_cell_bwd(ph.task_begin)
                    else: self.run_rnn_pool_bwd()
                else:
                    run.append(ph)
            self.phases = run
            Interp.run_group(self, group, fused_norm)
        finally:
            self.phases = kept
