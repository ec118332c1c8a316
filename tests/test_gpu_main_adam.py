"""GPU: main.py --optimizer Adam (reference main.py:84-86) on the fused step (TrainEngine's Adam update) against the module path
(TA3N_MAIN_FAST=0: VideoModel.forward + torch loss assembly + autograd + clip_grad_norm_ + torch.optim.Adam.step), in the pattern of
test_main_dropin.py::test_own_main_fused_fast_path_logs_what_the_module_path_logs.  Parameters are not compared element by element:
Adam's first steps move every element by about lr * sign(g), so an element whose gradient is below the fp32 summation-order floor
differs by 2 lr between any two correct implementations; exp_avg and exp_avg_sq are linear and quadratic in the gradients, so Adam's
normalisation does not amplify round-off in them."""
import os
import re
import subprocess
import sys

import pytest
import torch

from fixture_t7 import make_dataset
from ta3n_amd import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TA3N = ["--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
        "--add_loss_DA", "attentive_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.003", "--lr_adaptive", "dann"]
COMMON = ["--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0.5", "--dropout_v", "0.5", "-b", "8", "6", "8",
          "--optimizer", "Adam", "--lr", "1e-3", "--epochs", "2", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn"]


def _main(data, exp, tmp_path, fast, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *TA3N, *COMMON,
           "--save_best_log", str(tmp_path / f"best{fast}.log"), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def _adam_state(ck, n_steps):
    """The checkpoint's optimizer entry loaded into a torch.optim.Adam over a fresh model (main.py:104): {index: state}, every live step == n_steps."""
    from ta3n_amd.models import VideoModel
    net = VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, use_attn="TransAttn", verbose=False)
    opt = torch.optim.Adam(net.parameters(), 0.1)
    opt.load_state_dict(ck["optimizer"])
    g = opt.param_groups[0]
    assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and not g["amsgrad"]
    state = ck["optimizer"]["state"]
    assert state and all(float(st["step"]) == float(n_steps) for st in state.values()), {k: float(st["step"]) for k, st in state.items()}
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in state.values())
    return state


def test_own_main_adam_fast_path_logs_what_the_module_path_logs(tmp_path):
    data = make_dataset(str(tmp_path / "data"))
    outs, cks = [], []
    for fast in ("1", "0"):
        exp = str(tmp_path / f"exp{fast}")
        r = _main(data, exp, tmp_path, fast)
        assert "using Adam" in r.stdout
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
        cks.append(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False))
    print("# train.log of main.py --optimizer Adam with the fused step (TA3N_MAIN_FAST=1), then with the module path (=0); dropout 0.5 / 0.5\n" +
          "".join(outs[0]) + "# ----\n" + "".join(outs[1]))
    assert len(outs[0]) == len(outs[1]) == 6      # 2 epochs x ceil(24 / 8) steps, print_freq 1
    num = re.compile(r"(Loss|loss_c|loss_a|loss_e|lr:) (-?[0-9.]+)")
    for a, b in zip(*outs):
        fa, fb = num.findall(a), num.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb] and fa
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-3 * max(1.0, abs(float(y))), (k, x, y, a, b)
    sa, sb = _adam_state(cks[0], 6), _adam_state(cks[1], 6)
    assert set(sa) == set(sb), (sorted(sa), sorted(sb))
    bound = tol.F32_GRAD_REL_L2 * tol.GOLDEN_DRIFT_FACTOR
    worst = {}
    for k in sa:
        for key in ("exp_avg", "exp_avg_sq"):
            a_, b_ = sa[k][key].double(), sb[k][key].double()
            worst[key] = max(worst.get(key, 0.0), (a_ - b_).norm().item() / max(b_.norm().item(), 1e-30))
    print(f"[main adam] worst per-tensor rel. L2, fused step vs module path: {worst} (bound {bound})")
    for k in sa:
        for key in ("exp_avg", "exp_avg_sq"):
            a_, b_ = sa[k][key].double(), sb[k][key].double()
            assert (a_ - b_).norm().item() <= bound * b_.norm().item(), (k, key, (a_ - b_).norm().item(), b_.norm().item())
    # --resume --resume_hp: the third epoch starts from the saved step count (6) and learning rate
    exp = str(tmp_path / "exp1")
    r2 = _main(data, exp, tmp_path, "1", ["--resume", exp + "/RGB/checkpoint.pth.tar", "--resume_hp", "--epochs", "3"])
    assert "(epoch 2)" in r2.stdout and "Train: [3][0/3]" in r2.stdout and "Train: [2]" not in r2.stdout
    _adam_state(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False), 9)
