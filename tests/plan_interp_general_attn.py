"""plan_interp.Interp with the two general-attention phases (TA3N_FLAG_GENERAL_ATTN; ta3n_pointwise.hip: general_attn_fwd_kernel /
general_attn_bwd_kernel) executed with numpy from their specification.  Like the kernels, the phases find their regions and the
attention layer's second Linear by name (the Geom has no field for them).  Test infrastructure only."""
import numpy as np

from plan_interp import Interp, keep_mask

PH_GENERAL_ATTN_FWD, PH_GENERAL_ATTN_BWD = 14, 15


class GeneralAttnInterp(Interp):
    def _off(self, name):
        return self.plan.region(name)[0]

    def _wa2(self):
        poff = {n: (off, shape) for n, off, shape, _ in self.plan.params}
        NB = self.g.NB
        return self.P[poff["attn_layer.2.weight"][0]:][:NB], self.P[poff["attn_layer.2.bias"][0]]

    def run_general_attn_fwd(self):
        """Pr and R as pool_fwd; A = tanh(U) in place; w = softmax_j(<A_j, wa2> + ba2); V = sum_j (1 + w_j) R_j; Vd; losses cleared."""
        g, h = self.g, self.hy
        B, NR, NB, NT = g.B, g.n_rel, g.NB, g.n_tuples
        Hr = self.r(g.o_Hr, (B, NR, NB)); Zr = self.r(g.o_Zr, (B, NT, NB))
        R = self.r(g.o_R, (B, NR, NB)); Pr = self.r(g.o_Pr, (B, NR, 2))
        for j in range(NR):
            W2 = self.P[g.p_W2_0 + j * g.p_W2_stride:][:2 * NB].reshape(2, NB)
            b2 = self.P[g.p_b2_0 + j * g.p_b2_stride:][:2]
            Pr[:, j, :] = Hr[:, j, :] @ W2.T + b2
            R[:, j, :] = Zr[:, self.tf[j]:self.tf[j + 1], :].sum(1)
        Ua = self.r(self._off("Ua"), (B, NR, NB))
        Ua[:] = np.tanh(Ua)
        wa2, ba2 = self._wa2()
        s = Ua @ wa2 + ba2
        e = np.exp(s - s.max(1, keepdims=True))
        w = e / e.sum(1, keepdims=True)
        self.r(g.o_attn, (B, NR))[:] = w
        V = ((1 + w)[:, :, None] * R).sum(1)
        self.r(g.o_V, (B, NB))[:] = V
        Vd = V
        if h["train"] and h["p_drop_v"] > 0:
            idx = np.arange(B)[:, None] * NB + np.arange(NB)[None, :]
            Vd = V * keep_mask(h["seed_v"], idx, h["p_drop_v"]) * self.scale(5)
        self.r(g.o_Vd, (B, NB))[:] = Vd
        self.ws[g.o_losses:g.o_losses + 8] = 0

    def run_general_attn_bwd(self):
        """d_j = <R_j, gv> + g_attn; gs = w (d - sum_k w_k d_k); gUa = gs wa2 (1 - A^2); gRa = (1 + w) gv; gPrT = gPr; gHr from gPr."""
        g = self.g
        B, NR, NB = g.B, g.n_rel, g.NB
        gv = self.r(g.o_gVt, (B, NB))
        if g.o_gV_ext > 0:
            gv = gv + self.r(g.o_gV_ext, (B, NB))
        R = self.r(g.o_R, (B, NR, NB)); w = self.r(g.o_attn, (B, NR)); A = self.r(self._off("Ua"), (B, NR, NB))
        d = (R * gv[:, None, :]).sum(2) + self.r(g.o_gattn, (B, NR))
        gs = w * (d - (w * d).sum(1, keepdims=True))
        self.r(self._off("gs"), (B, NR))[:] = gs
        wa2, _ = self._wa2()
        self.r(self._off("gUa"), (B, NR, NB))[:] = gs[:, :, None] * wa2[None, None, :] * (1 - A * A)
        self.r(g.o_gRa, (B, NR, NB))[:] = (1 + w)[:, :, None] * gv[:, None, :]
        gPr = self.r(g.o_gPr, (B, NR, 2)); Hr = self.r(g.o_Hr, (B, NR, NB))
        self.r(g.o_gPrT, (B, NR, 2))[:] = gPr
        gHr = self.r(g.o_gHr, (B, NR, NB))
        for j in range(NR):
            W2 = self.P[g.p_W2_0 + j * g.p_W2_stride:][:2 * NB].reshape(2, NB)
            gHr[:, j, :] = np.where(Hr[:, j, :] > 0, gPr[:, j, :] @ W2, 0)

    def run_group(self, group, fused_norm=False):
        """Interp.run_group is a plain loop over self.phases that dispatches on the phase kind and skips kinds it does not know; it
        does nothing once per group.  On that assumption it is called here once per stretch of phases between two general-attention
        phases, with self.phases narrowed to the stretch (as tests/plan_interp_frame_attn.py does)."""
        mine = {PH_GENERAL_ATTN_FWD: self.run_general_attn_fwd, PH_GENERAL_ATTN_BWD: self.run_general_attn_bwd}
        kept = self.phases
        try:
            run = []
            for ph in kept:
                if ph.group != group:
                    continue
                if ph.kind in mine:
                    self.phases = run
                    Interp.run_group(self, group, fused_norm)
                    run = []
                    mine[ph.kind]()
                else:
                    run.append(ph)
            self.phases = run
            Interp.run_group(self, group, fused_norm)
        finally:
            self.phases = kept
