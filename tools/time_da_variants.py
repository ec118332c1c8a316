"""Step time of the options that run as unfused launch lists (ens_DA MCD, dis_DA DAN / JAN, use_attn_frame TransAttn, use_attn general) beside
the fused step, headline shape, bf16 twins and fp32: wall clock with the host included and HIP events around the same loop, best of 3; for
use_attn_frame and use_attn general also their two pointwise kernels' own times (ta3n_time_phases).
usage (GPU box): python tools/time_da_variants.py [steps] [substrings of the variants to run, comma-separated]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ta3n_amd.engine import TrainEngine, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
only = sys.argv[2].split(",") if len(sys.argv) > 2 else []
Bs, Bt, T, D, F, C = 128, 74, 5, 2048, 512, 12
xs, xt, ys, yt = synth_batch(C, T, D, Bs, Bt, seed=1234)
for bf16 in (True, False):
    for name, kw in (("fused step", {}), ("unfused lists", dict(fused=False)), ("ens_DA MCD", dict(ens_DA="MCD", mu=0.5)),
                     ("dis_DA DAN", dict(dis_DA="DAN", alpha=0.5)), ("dis_DA JAN", dict(dis_DA="JAN", alpha=0.5, place_dis=("Y", "Y", "N"))),
                     ("use_attn_frame", dict(flags=flags_from_options(use_attn_frame="TransAttn"))),
                     ("use_attn general", dict(flags=flags_from_options(use_attn="general")))):
        if only and not any(o in name for o in only):
            continue
        try:
            eng = TrainEngine(Bs, Bt, T, D, F, C, dropout_i=0.5, dropout_v=0.5, clip=20.0, bf16=bf16, bf16_store=bf16, **kw)
        except Exception as ex:      # noqa: BLE001
            print(f"{name}: {type(ex).__name__}: {ex}"[:200]); continue
        eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7, scale="init"))
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        for _ in range(30):
            eng.train_step([0.75, 0.75, 0.5], 0.003, 0.03)
        best, best_ev = 1e9, 1e9
        for rep in range(3):      # best of three runs: the first run of a configuration also pays one-time costs (code objects, allocator)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                eng.train_step([0.75, 0.75, 0.5], 0.003, 0.03)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, 1e6 * (time.perf_counter() - t0) / steps)
            best_ev = min(best_ev, 1e3 * e0.elapsed_time(e1) / steps)
        print(f"{'bf16' if bf16 else 'f32 '} {name:16s} fused={eng.fused}: {best:.0f} us/step host included, {best_ev:.0f} us/step between HIP events "
              f"(one library call per launch group; best of 3 x {steps})")
        if name == "use_attn_frame":      # kinds 12 / 13: frame_attn_fwd_kernel / frame_attn_bwd_kernel
            ph = eng.time_phases(reps=50)
            print("    launches (kind:us): " + " ".join(f"{k}:{1e3 * ms:.1f}" for k, _, _, ms in ph))
            print("    frame_attn_fwd %.1f us, frame_attn_bwd %.1f us, all launches %.0f us" %
                  (1e3 * sum(ms for k, _, _, ms in ph if k == 12), 1e3 * sum(ms for k, _, _, ms in ph if k == 13), 1e3 * sum(ms for _, _, _, ms in ph)))
        if name == "use_attn general":      # kinds 14 / 15: general_attn_fwd_kernel / general_attn_bwd_kernel (in place of kinds 1 / 3, the pooling launches)
            ph = eng.time_phases(reps=50)
            print("    launches (kind:us): " + " ".join(f"{k}:{1e3 * ms:.1f}" for k, _, _, ms in ph))
            print("    general_attn_fwd %.1f us, general_attn_bwd %.1f us, all launches %.0f us" %
                  (1e3 * sum(ms for k, _, _, ms in ph if k == 14), 1e3 * sum(ms for k, _, _, ms in ph if k == 15), 1e3 * sum(ms for _, _, _, ms in ph)))
        if name == "unfused lists":         # ... and the pooling launches they stand in for
            ph = eng.time_phases(reps=50)
            print("    pool_fwd %.1f us, pool_bwd %.1f us, all launches %.0f us" %
                  (1e3 * sum(ms for k, _, _, ms in ph if k == 1), 1e3 * sum(ms for k, _, _, ms in ph if k == 3), 1e3 * sum(ms for _, _, _, ms in ph)))
