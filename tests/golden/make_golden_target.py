#!/usr/bin/env python
"""Generate the fixtures of --use_target Sv / --add_loss_DA target_entropy (tests/golden/tiny_sv_tent.npz, tiny_avgpool_da_sv.npz) by running
the REFERENCE ITSELF on CPU.

Run in the build container only (needs the reference checkout, like make_golden.py):
    python tests/golden/make_golden_target.py [case ...]
Same recipe and record names as make_golden.run_case - the reference's VideoModel.forward and main.train, weights and batches (the target
videos' labels included) from ta3n_amd.synthetic - with args.use_target / args.add_loss_DA of the case in place of run_case's uSv /
attentive_entropy (main.py:442-446, 542-545).  On top of run_case's records every fixture holds
  meta/use_target     the value of --use_target the reference ran with
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)


def run_case(name, case):
    use_target = case["use_target"]
    plain = {k: v for k, v in case.items() if k != "use_target"}
    orig = mg.make_args

    def make_args(c):
        a = orig(c)      # (takes the case's add_loss_DA itself)
        a.use_target = use_target
        return a
    mg.make_args = make_args
    try:
        mg.run_case(name, plain)
    finally:
        mg.make_args = orig
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    store["meta/use_target"] = np.array(use_target)
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path) // 1024, "KiB (use_target", use_target + ")")


CASES = {
    # trn-m with the TA3N options of the headline command but Sv and the plain target entropy at the reference's H->U gamma
    # (script_train_val.sh:90), the tiny_T5 case: two steps, the last one short
    "tiny_sv_tent": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=2,
                         short_last=(5, 3), lr=2e-3, gamma=0.3, add_loss_DA="target_entropy", use_target="Sv"),
    # TemPooling + RevGrad (video and frame level) under Sv
    "tiny_avgpool_da_sv": dict(agg="avgpool", place_adv=("N", "Y", "Y"), arch="resnet18", fc_dim=64, T=5, C=5, Bs=6, Bt=4, wseed=15,
                               wscale="trained", xseed=57, steps=2, short_last=(5, 3), lr=2e-3, use_target="Sv"),
}

if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES):
        run_case(nm, CASES[nm])
