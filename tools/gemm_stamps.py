"""Debug aid (needs a library built with -DTA3N_GEMM_STAMPS in a directory of its own:
    TA3N_LIBDIR=$PWD/ta3n_amd/lib_stamps TA3N_EXTRA_FLAGS=-DTA3N_GEMM_STAMPS python -m ta3n_amd.build
    TA3N_LIBDIR=$PWD/ta3n_amd/lib_stamps python tools/gemm_stamps.py [bf16|f32] [config 2|4|5]
): per-workgroup s_memtime stamps of every GEMM launch of the fused step - entry / descriptors loaded / K loop done / epilogue done,
and inside the K loop the time thread 0 spends WAITING for a stage (s_waitcnt + s_barrier) against the time it spends issuing the next
stage's DMA, LDS reads and MFMAs - printed per launch and per tile length: where a launch's time goes; and around a Seg boundary: from the
barrier to the stage's DMAs issued on chunks that start a Seg's stream against chunks inside a Seg, and the LDS reads + MFMAs of a Seg's last
chunk against an interior one (-DTA3N_SEG_FAST=0 beside -DTA3N_GEMM_STAMPS builds the old boundary sequence).  TA3N_KIND_KERNELS=0 runs the
general kernels, which request a tile's residual and mask inside the store loop; the default runs the kind-specialised ones.
The front of a tile ("desc", entry -> descriptors / bias loaded) is split into its stretches - first Task word there, per-step scalars there, bias
requested, first stage's DMAs issued: each as thread 0's time since entry, in the order the kernel reaches them - and the store pass into "Task fields
of the store loop in registers" and the LDS sum behind it (-DTA3N_TASK_FAST=0 beside -DTA3N_GEMM_STAMPS builds the old descriptor reads)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from ta3n_amd import _lib
from ta3n_amd.engine import TrainEngine
from ta3n_amd.synthetic import synth_batch, synth_state
sys.path.insert(0, ROOT)
import bench
CFG = bench.CONFIGS[int(sys.argv[2]) if len(sys.argv) > 2 else 2]["shape"]
bf16 = (sys.argv[1] if len(sys.argv) > 1 else "bf16") == "bf16"
print(f"## {'bf16 (twins)' if bf16 else 'fp32'} shape {CFG}")
eng = TrainEngine(CFG["Bs"], CFG["Bt"], CFG["T"], CFG["D"], CFG["F"], CFG["C"], 
                  bf16=bf16, bf16_store=bf16)
eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7, scale="init"))
xs, xt, ys, yt = synth_batch(CFG["C"], CFG["T"], CFG["D"], CFG["Bs"], CFG["Bt"], seed=1234)
eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
eng.set_hyper([0.75, 0.75, 0.5], 0.003, 0.03)
for _ in range(3):
    eng.fused_step()
torch.cuda.synchronize()
L = _lib.lib()
n_ph = L.ta3n_num_phases(eng.plan.handle, 4)
phases = [ph for ph in eng.plan.description["phases"] if ph["group"] == 4]
args = (eng.plan.handle, eng.X.data_ptr(), eng.P.data_ptr(), eng.G.data_ptr(), eng.ws.data_ptr())
SL = 16
stamps = eng.region("stamps").view(torch.int64)
for i, ph in enumerate(phases):
    if ph["kind"] != 0:
        L.ta3n_train_step_range(*args, i, 1, eng._stream()); continue
    torch.cuda.synchronize()
    L.ta3n_train_step_range(*args, i, 1, eng._stream())     # warm: code and operands in cache, as inside a running step
    torch.cuda.synchronize()
    stamps.zero_()
    L.ta3n_train_step_range(*args, i, 1, eng._stream())
    torch.cuda.synchronize()
    n = min(ph["task_count"], 8192)
    st = stamps[: n * SL].cpu().numpy().reshape(n, SL).astype(np.int64)
    # the front stamps share slots 6 / 7 with the cost and the Seg count, the store-pass stamp slot 11 with the old one (ta3n_gemm_kernel.h: FSTAMP)
    front = np.stack([(st[:, 6] >> 24) & 0xFFFF, (st[:, 6] >> 40) & 0xFFFF, (st[:, 7] >> 16) & 0xFFFF, (st[:, 7] >> 32) & 0xFFFF], 1)
    st[:, 6] &= (1 << 24) - 1
    st[:, 7] &= (1 << 16) - 1
    M48 = (1 << 48) - 1
    sum_lds = (st[:, 11] >> 48) & 0xFFFF
    st[:, 11] &= M48
    st[:, 4] = np.where(st[:, 11] > 0, st[:, 4] & M48, st[:, 4])      # (only the difference [11] - [4] is printed)
    real = st[:, 7] > 0
    if not real.any():
        print(f"launch {i}: no stamps"); continue
    t0 = st[real, 0].min()
    TICK = 1.0 / 2400      # s_memtime counts shader clocks; us at the nominal 2.4 GHz (a launch timed with HIP events calibrates it: span ~ duration)
    print(f"launch {i} tile {ph['tile']} tasks {n} (real {real.sum()}): span {(st[real, 5].max() - t0) * TICK:.2f} us, last entry {(st[real, 0].max() - t0) * TICK:.2f} us after the first")
    for cst in np.unique(st[real, 6])[-5:]:
        m = real & (st[:, 6] == cst)
        d = lambda a, b: np.mean(st[m, a] - st[m, b]) * TICK
        ns = np.maximum(st[m, 10], 1)
        print(f"    K {cst:5d} x{m.sum():4d}: desc {d(1, 0):5.2f}  kloop {d(2, 1):6.2f} (thread 0: waiting for stage+barrier {np.mean(st[m, 8]) * TICK:6.2f}, issue+compute {np.mean(st[m, 9]) * TICK:6.2f}, "
              f"{np.mean(ns):.1f} stages -> {np.mean(st[m, 8] / ns) * TICK * 1e3:5.0f} + {np.mean(st[m, 9] / ns) * TICK * 1e3:5.0f} ns per stage)  wait-waves {d(3, 2):5.2f}  to-lds {d(4, 3):5.2f}  "
              f"combine+store {d(5, 4):5.2f} (second wave, first pass: LDS sum and global operands there {d(11, 4):5.2f} after [4])"
              f"  | finish {np.mean(st[m, 5] - t0) * TICK:6.2f} us")
        f = front[m].mean(0) * TICK
        print(f"          front, us since entry: first Task word {f[0]:4.2f}  per-step scalars {f[1]:4.2f}  bias requested {f[2]:4.2f}  first stage's DMAs issued {f[3]:4.2f}"
              f" | store pass: [4] -> Task fields in registers {d(11, 4) - np.mean(sum_lds[m]) * TICK:4.2f}, -> LDS sum and global operands there {np.mean(sum_lds[m]) * TICK:4.2f}")
        # Seg boundary stamps (slots 12 - 15: cycles in the low 40 bits, stretches counted above them): ns per stretch over the class
        def per(slot):
            cyc, cnt = (st[m, slot] & ((1 << 40) - 1)).sum(), (st[m, slot] >> 40).sum()
            return f"{cyc / cnt * TICK * 1e3:4.0f} ns x{cnt / m.sum():4.1f}" if cnt else "   - "
        print(f"          {np.mean(st[m, 7]):4.1f} Segs | barrier -> stage's DMAs issued: starting a Seg {per(12)}, inside a Seg {per(13)} | LDS reads + MFMAs: "
              f"FULL chunk {per(14)}, a Seg's last chunk that holds a whole chunk {per(15)}")
