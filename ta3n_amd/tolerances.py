"""Parity bounds of the HIP train step, in ONE place: the GPU tests assert them (tests/test_gpu_parity.py, test_gpu_gradients.py,
test_gpu_bf16.py) and bench.py quotes them in its `config.workload` strings, so what the benchmark line says is what the tests
check.  Floors measured on MI355X are recorded in profiles/r03_parity_floors.txt (tests/test_gpu_gradients.py prints them).

Metrics: "max" = max |got - want|; "rel. L2" = ||got - want||_2 / ||want||_2 per tensor, every element of every tensor;
"max/scale" = max |got - want| / max |want| per tensor."""

# ---- fp32 MFMA: against the reference's fp32 CPU path (oracle pinned to it; re-synchronised to the engine's parameters each step) ----
LOGIT_ATOL = 1e-3            # north_star: class and domain logits within 1e-3 absolute at trained-scale (O(1..10)) logits
F32_RTOL, F32_ATOL = 2e-4, 5e-5     # parameters after a step, features, attention weights (elementwise)
# Gradients, every element of every tensor of every step.  Typical tensors agree to 1e-6 .. 2e-5 (fp32 summation order); a tensor
# behind a ReLU mask moves by ~1/rows of its norm for every hidden unit whose pre-activation sits within round-off of zero and
# lands on the other side (measured worst: 2.2e-3, the video discriminator's hidden layer at 1024 videos) - hence a tight bound
# on the MEDIAN over the step's tensors and a looser one on each tensor.
F32_GRAD_REL_L2_MEDIAN = 2e-5      # measured <= 3.1e-6
F32_GRAD_REL_L2 = 5e-3             # measured worst 2.2e-3
F32_GRAD_MAX_SCALE = 3e-2          # measured worst 7.7e-3
# ... and with the oracle forced to the engine's ReLU on/off patterns (tests/test_gpu_masked_gradients.py: no unit can land on different
# sides in the two computations, what is left is fp32 summation order): EVERY gradient tensor, not just the median
# (measured worst: 5.7e-5, the shared-FC weight at 128+128 videos x 12 segments - three dependent contractions with K up to 6 144 in
# front of a 3 072-row weight gradient whose adversarial and classification parts cancel; 25 x tighter than the free-running bound)
F32_MASKED_GRAD_REL_L2 = 2e-4
F32_MASKED_GRAD_REL_L2_MEDIAN = 2e-5
# (at the limits of the accepted shapes - 64 segments, 1 / 64 classes, fc_dim up to 2048 and past it, dimensions that are no multiples
# of 4 - the same two bounds hold against the float64 oracle, and the logits are held to LOGIT_ATOL x max(1, max |logit| / 10): they
# grow with the relation count, ~230 at 64 segments.  tests/test_gpu_limit_shapes.py; floors in profiles/limit_shapes_parity_floors.txt)
# Against the reference's RECORDED multi-step trajectories (golden vectors): from the second step on the two sides stand on
# parameters that differ by round-off, more ReLU units switch sides; the per-tensor bound is scaled by this factor there.
GOLDEN_DRIFT_FACTOR = 2.0         # measured worst later-step tensor: 1.1e-3 (fp32), 1.6e-3 (f32x3)
# ---- fp32-grade split arithmetic (f32x3: 16 mantissa bits per operand, ~2^-16 per product): same reference, its own bounds ----
# logits stay within LOGIT_ATOL (measured <= 1.5e-4); gradients are 30-100x further from the reference than the fp32 MFMA's
F32X3_GRAD_REL_L2_MEDIAN = 2e-4    # measured <= 2.0e-5
# ... except in a step where a hidden unit of the TRN bottleneck sits within round-off of zero and lands on the other side of the ReLU
# than in the oracle: its whole gradient row then differs, and with it every tensor upstream.  Measured once (headline shape, third step,
# stored hi / lo planes): ONE element of Zr is 6.8e-7 instead of 0.0, 442 elements of gZ1 follow, the step's median is 4.3e-4
# (profiles/r03_parity_floors.txt).  At most ONE step of a case may exceed the median bound, and only up to this:
F32X3_GRAD_REL_L2_MEDIAN_TIE = 1e-3
F32X3_GRAD_REL_L2 = 1.5e-2   # measured worst 5.3e-3
F32X3_GRAD_MAX_SCALE = 6e-2  # measured worst 2.2e-2

# ---- bf16 arithmetic: against the independent bf16-operand oracle (same arithmetic contract, fp64 accumulation) ----
BF16_LOGIT_REL_RMS = 5e-3    # max |error| / rms(reference tensor)
BF16_GRAD_REL_L2 = 2e-2      # per gradient / update tensor
BF16_GRAD_REL_L2_MEDIAN = 1e-3
BF16_GRAD_MAX_SCALE = 1e-1
# loss terms (means of cross-entropies / entropies of those logits), relative to max(1, |term|): a cross-entropy moves by at most twice the largest
# logit error of its row, so 2 x BF16_LOGIT_REL_RMS x rms(logits) with logits of rms O(1); tests/test_gpu_weighted_loss.py (measured there: below 1e-6 at 6 + 4 videos, profiles/weighted_loss_parity_floors.txt)
BF16_LOSS_REL = 2e-2
# ---- bf16 arithmetic: distance from the fp32 REFERENCE (what rounding the contraction operands to bf16 costs) ----
BF16_REF_LOGIT_REL_RMS = 2.5e-2          # measured 1.1e-2 .. 1.7e-2 of rms at the three benchmarked shapes
BF16_REF_GRAD_REL_L2_MEDIAN = 2e-2       # measured 3.4e-3 .. 6.4e-3
BF16_REF_GRAD_REL_L2 = 0.25              # absolute cap per weight-gradient tensor; measured 0.8 - 1.3 % at the headline shape, up to 15 % for single
                                         # relation-discriminator hidden layers at 1024 videos / 12 segments (ReLU-masked, few active rows)
# ... and, per tensor, relative to what the bf16 CONTRACT costs on the very same inputs (the oracle's bf16-operand mode against its fp32
# mode, computed in the test): rel. L2(HIP bf16, fp32 reference) <= FACTOR x rel. L2(oracle bf16, fp32 reference) + FLOOR.  The contract's
# cost is the ReLU on/off pattern (0.08 % of the hidden units land on the other side of zero; profiles/r04_bf16_gradient_deviation_attribution.txt):
# two implementations of the contract flip different units of the same population, hence a factor and not equality.
BF16_REF_GRAD_CONTRACT_FACTOR = 1.5      # measured: the HIP path's distances ARE the contract's to two digits (ratio 0.98 .. 1.02 at the three shapes,
BF16_REF_GRAD_FLOOR = 5e-3                # profiles/r04_parity_floors.txt), e.g. 6.5e-2 / 6.5e-2 and 1.5e-1 / 1.5e-1 for relation_domain_classifier_all.6.0.weight

# ---- training equivalence over 300 steps on a learnable synthetic task (tests/test_gpu_training_equivalence.py) ----
# early: total loss step by step over the first 20 steps, relative (the trajectories coincide up to the arithmetic's rounding; from
# ~step 25 on ReLU flips decorrelate ANY two arithmetics - the oracle's own bf16-operand mode is 3.1e-2 from its fp32 mode there);
# late: medians over the last 100 steps; accuracy: held-out top-1, points, both domains.
# Measured (profiles/r04_training_equivalence.json; one MI355X run): early 9.4e-7 (fp32 MFMA), 4.2e-3 (f32x3), 1.2e-2 (bf16); late medians
# within 1.3e-2 (total), 1.1e-2 (adversarial) of the oracle's; classification-loss medians <= 4.6e-3, entropy <= 4.7e-2; accuracies
# 98.5-100 % against the oracle's 99.5 / 98.5 %.
TRAIN_EARLY_REL_F32 = 0.01
TRAIN_EARLY_REL_BF16 = 0.05
TRAIN_LATE_REL = 0.05           # total and adversarial loss medians
TRAIN_LATE_LOSS_C = 0.05        # classification loss median (learnt task: -> 0)
TRAIN_LATE_LOSS_E = 0.15        # attentive-entropy median
TRAIN_ACC_POINTS = 3.0
# with dropout 0.5 / 0.5 (bf16 engine against the fp32 engine on identical masks): classification loss and entropy stay well above zero
TRAIN_ACC_POINTS_DROPOUT = 5.0
TRAIN_LATE_REL_DROPOUT = 0.10    # total / adversarial loss medians (measured 5.4e-2 / 3.6e-3)
TRAIN_LATE_DROPOUT_REL = 0.5
TRAIN_LATE_DROPOUT_ABS = 0.05
