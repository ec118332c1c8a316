#!/usr/bin/env python
"""Generate the weighted-criteria fixtures (tests/golden/tiny_wcls_wdom.npz, tiny_avgpool_da_wcls.npz) by running the REFERENCE ITSELF on CPU.

Run in the build container only (needs the reference checkout, like make_golden.py):
    python tests/golden/make_golden_weighted.py [case ...]
Same recipe and record names as make_golden.run_case - the reference's VideoModel.forward and main.train, weights from
ta3n_amd.synthetic - with the two criteria built the way the reference's main builds them under --weighted_class_loss Y /
--weighted_class_loss_DA Y (main.py:160-167, 205-206):
    criterion        = CrossEntropyLoss(weight = 1 / class_freq)                       class_freq of a made-up, skewed source list
    criterion_domain = CrossEntropyLoss(weight = [1 / num_source_train, 1 / num_target_train])
On top of run_case's records every fixture holds
  meta/class_w     the class weights (fp32, as torch.Tensor(class_freq) makes them), all 1 when the class criterion is unweighted
  meta/domain_w    the two domain weights, (1, 1) when the domain criterion is unweighted
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)


def class_weights(counts):
    """The weights the reference's main forms from a source list with counts[c] videos of class c (main.py:156-164): one over the class's
    share of the list, divided in fp32."""
    share = np.asarray(counts, dtype=np.float64) / float(sum(counts))
    return 1 / torch.Tensor(share.tolist())


class weighted_criteria:
    """While active, the two CrossEntropyLoss() that run_case builds - the class criterion first, the domain criterion second - carry
    the case's weights (main.py:205-206)."""

    def __init__(self, class_w, domain_w):
        self.weights = [class_w, domain_w]

    def __enter__(self):
        self.orig = torch.nn.CrossEntropyLoss
        pending = list(self.weights)
        orig = self.orig

        def make(*a, **k):
            return orig(*a, weight=pending.pop(0), **k) if pending and not a and not k else orig(*a, **k)
        torch.nn.CrossEntropyLoss = make
        self.pending = pending
        return self

    def __exit__(self, *exc):
        torch.nn.CrossEntropyLoss = self.orig
        assert exc[0] is not None or not self.pending, "run_case built fewer criteria than expected"


def run_case(name, case):
    class_w = class_weights(case["class_counts"]) if case.get("class_counts") else torch.ones(case["C"])
    domain_w = torch.Tensor(list(case["domain_w"])) if case.get("domain_w") else torch.Tensor([1, 1])
    plain = {k: v for k, v in case.items() if k not in ("class_counts", "domain_w")}
    with weighted_criteria(class_w, domain_w):
        mg.run_case(name, plain)
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    store["meta/class_w"] = class_w.numpy().astype(np.float32)
    store["meta/domain_w"] = domain_w.numpy().astype(np.float32)
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path) // 1024, "KiB (with the weights)")


CASES = {
    # trn-m with the TA3N options of the headline command, the tiny_T5 case: both criteria weighted, two steps, the last one short.
    # 12 classes with 3 .. 60 videos (weights 20 x apart), domain weights of a 37-video source and a 1438-video target list
    "tiny_wcls_wdom": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=2,
                           short_last=(5, 3), lr=2e-3, class_counts=(13, 3, 46, 8, 27, 5, 60, 10, 35, 4, 20, 6),
                           domain_w=(1 / 37, 1 / 1438)),
    # TemPooling + RevGrad (video and frame level), the class criterion weighted
    "tiny_avgpool_da_wcls": dict(agg="avgpool", place_adv=("N", "Y", "Y"), arch="resnet18", fc_dim=64, T=5, C=5, Bs=6, Bt=4, wseed=15,
                                 wscale="trained", xseed=57, steps=2, short_last=(5, 3), lr=2e-3, class_counts=(40, 2, 9, 21, 4)),
}

if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES):
        run_case(nm, CASES[nm])
