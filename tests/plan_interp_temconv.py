"""plan_interp.Interp with the three launches of the temporal-convolution aggregator (TA3N_AGG_TEMCONV; ta3n_amd/csrc/ta3n_temconv.hip),
executed from their specification: the 3-tap filter over the segments + ReLU + mean, its way back, and the sum of the per-video parts
of the four parameter gradients.  The GEMM launches around them run through Interp like every other.  Test infrastructure."""
import numpy as np

from plan_interp import Interp, keep_mask

PH_TEMCONV_FWD, PH_TEMCONV_BWD, PH_TEMCONV_WGRAD = 20, 21, 22


class TemconvInterp(Interp):
    """The parameters are found by name (tcl_3_1.conv2d.weight / .bias), the partial sums in region "tc_part"."""

    def __init__(self, plan, dtype=np.float64):
        super().__init__(plan, dtype)
        off = {name: o for name, o, _, _ in plan.params}
        self.p_w, self.p_b = off["tcl_3_1.conv2d.weight"], off["tcl_3_1.conv2d.bias"]

    def _z(self):
        """(F1 padded with one zero row on either side [B, T + 2, F], Z [B, T, F])."""
        g = self.g
        F1 = self.r(g.o_F1, (g.B, g.T, g.F))
        pad = np.zeros((g.B, g.T + 2, g.F), self.dtype)
        pad[:, 1:-1] = F1
        w, c = self.P[self.p_w:self.p_w + 3], self.P[self.p_b]
        return pad, w[0] * pad[:, :-2] + w[1] * pad[:, 1:-1] + w[2] * pad[:, 2:] + c

    def run_temconv_fwd(self):
        g, h = self.g, self.hy
        B, F = g.B, g.F
        V = np.maximum(self._z()[1], 0).mean(1)
        mk = np.ones((B, F), self.dtype)
        if h["train"] and h["p_drop_v"] > 0:
            mk = keep_mask(h["seed_v"], np.arange(B)[:, None] * F + np.arange(F)[None, :], h["p_drop_v"]) * self.scale(5)
        self.r(g.o_V, (B, F))[:] = V
        self.r(g.o_Vd, (B, F))[:] = V * mk
        self.ws[g.o_losses:g.o_losses + 8] = 0

    def run_temconv_bwd(self):
        g = self.g
        B, T, F = g.B, g.T, g.F
        gv = self.r(g.o_gVt, (B, F))
        if g.o_gV_ext > 0:
            gv = gv + self.r(g.o_gV_ext, (B, F))
        pad, Z = self._z()
        gR = np.where(Z > 0, gv[:, None, :] / T, 0.0)
        gRp = np.zeros((B, T + 2, F), self.dtype)
        gRp[:, 1:-1] = gR
        w = self.P[self.p_w:self.p_w + 3]
        gF1 = w[0] * gRp[:, 2:] + w[1] * gRp[:, 1:-1] + w[2] * gRp[:, :-2]      # gF1[t] = w0 gR[t+1] + w1 gR[t] + w2 gR[t-1]
        if g.o_gHf < 0:
            self.r(g.o_gZ1, (B, T, F))[:] = np.where(pad[:, 1:-1] > 0, gF1 * self.scale(4), 0.0)
        else:
            self.r(g.o_gRa, (B, T, F))[:] = gF1
        part = self.r(self.plan.region("tc_part")[0], (B, 4))
        for j in range(3):
            part[:, j] = (gR * pad[:, j:j + T]).sum((1, 2))
        part[:, 3] = gR.sum((1, 2))

    def run_temconv_wgrad(self):
        g = self.g
        d = self.r(self.plan.region("tc_part")[0], (g.B, 4)).sum(0)
        self.G[self.p_w:self.p_w + 3] = d[:3]
        self.G[self.p_b] = d[3]
        self.ws[g.o_sumsq + g.n_sumsq - 1] = (d * d).sum()

    def run_group(self, group, fused_norm=False):
        """Interp.run_group skips the kinds it does not know: it runs the stretches between two temconv phases (as
        tests/plan_interp_rnn.py does)."""
        kept = self.phases
        try:
            run = []
            for ph in kept:
                if ph.group != group:
                    continue
                if ph.kind in (PH_TEMCONV_FWD, PH_TEMCONV_BWD, PH_TEMCONV_WGRAD):
                    self.phases = run
                    Interp.run_group(self, group, fused_norm)
                    run = []
                    if ph.kind == PH_TEMCONV_FWD: self.run_temconv_fwd()
                    elif ph.kind == PH_TEMCONV_BWD: self.run_temconv_bwd()
                    else: self.run_temconv_wgrad()
                else:
                    run.append(ph)
            self.phases = run
            Interp.run_group(self, group, fused_norm)
        finally:
            self.phases = kept
