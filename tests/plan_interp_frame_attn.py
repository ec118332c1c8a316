"""plan_interp.Interp with the two frame-attention phases (TA3N_FLAG_FRAME_ATTN; ta3n_pointwise.hip: frame_attn_fwd_kernel /
frame_attn_bwd_kernel) executed with numpy from their specification.  Like the kernels, the phases find their regions by name
(the Geom has no field for them).  Test infrastructure only."""
import numpy as np

from plan_interp import Interp

PH_FRAME_ATTN_FWD, PH_FRAME_ATTN_BWD = 12, 13


class FrameAttnInterp(Interp):
    def _off(self, name):
        return self.plan.region(name)[0]

    def _grad_base(self):
        """(1 + w) gF1a goes to a region of its own, or into gRa where that is large enough."""
        return self._off("gF1s") if "gF1s" in self.plan.regions else self.g.o_gRa

    def run_frame_attn_fwd(self):
        g = self.g
        BT, F = g.B * g.T, g.F
        _, _, H = self.soft2(self.r(g.o_Pf, (BT, 2)))
        w = 1 - H
        self.r(self._off("attn_frame"), (BT,))[:] = w
        self.r(self._off("F1a"), (BT, F))[:] = (1 + w)[:, None] * self.r(g.o_F1, (BT, F))

    def run_frame_attn_bwd(self):
        g = self.g
        BT, F = g.B * g.T, g.F
        p, lp, H = self.soft2(self.r(g.o_Pf, (BT, 2)))
        gin = self.r(self._off("gF1a"), (BT, F)).copy()
        d = (gin * self.r(g.o_F1, (BT, F))).sum(1)
        self.r(self._off("gPfT"), (BT, 2))[:] = self.r(g.o_gPf, (BT, 2)) + d[:, None] * p * (lp + H[:, None])
        self.r(self._grad_base(), (BT, F))[:] = (1 + (1 - H))[:, None] * gin

    def run_group(self, group, fused_norm=False):
        """Interp.run_group is a plain loop over self.phases that dispatches on the phase kind and skips kinds it does not know; it
        does nothing once per group.  On that assumption it is called here once per stretch of phases between two frame-attention
        phases, with self.phases narrowed to the stretch.  Should it ever gain per-group work (a prologue, a counter), this override
        must become a loop of its own over the phases."""
        mine = {PH_FRAME_ATTN_FWD: self.run_frame_attn_fwd, PH_FRAME_ATTN_BWD: self.run_frame_attn_bwd}
        kept = self.phases
        try:      # the base class runs the stretches between the new phases
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
