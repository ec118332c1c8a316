"""GPU: main.py --use_target Sv --add_loss_DA target_entropy (reference main.py:439-446, 542-545, 565-571) on the fused step (TrainEngine
with TA3N_FLAG_TARGET_LABELS / TA3N_FLAG_TARGET_ENTROPY) against the module path (TA3N_MAIN_FAST=0: VideoModel.forward + the torch loss
assembly with the concatenation of :442-444 and cross_entropy_soft + autograd + clip_grad_norm_ + SGD.step), in the pattern of
tests/test_gpu_main_adam.py: tiny synthetic lists, dropout 0.5 / 0.5 on the same masks, the Train: lines under that test's bound."""
import os
import re
import subprocess
import sys

import pytest
import torch

from fixture_t7 import make_dataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "Sv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
        "--add_loss_DA", "target_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.3", "--lr_adaptive", "dann"]
COMMON = ["--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0.5", "--dropout_v", "0.5", "-b", "8", "6", "8",
          "--lr", "0.03", "--epochs", "2", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn"]


def _main(data, exp, tmp_path, fast):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *OPTS, *COMMON,
           "--save_best_log", str(tmp_path / f"best{fast}.log")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_own_main_sv_target_entropy_fast_path_logs_what_the_module_path_logs(tmp_path):
    from ta3n_amd.models import VideoModel
    data = make_dataset(str(tmp_path / "data"))
    outs, cks = [], []
    for fast in ("1", "0"):
        exp = str(tmp_path / f"exp{fast}")
        r = _main(data, exp, tmp_path, fast)
        said = [ln for ln in r.stdout.splitlines() if ln.startswith("[ta3n]") and "target labels" in ln and "target entropy" in ln]
        assert bool(said) == (fast == "1"), r.stdout[-2000:]
        if said:
            assert "fused step" in said[0]
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
        cks.append(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False))
    print("# train.log of main.py --use_target Sv --add_loss_DA target_entropy with the fused step (TA3N_MAIN_FAST=1), then with the module path (=0)\n" +
          "".join(outs[0]) + "# ----\n" + "".join(outs[1]))
    assert len(outs[0]) == len(outs[1]) == 6      # 2 epochs x ceil(24 / 8) steps, print_freq 1
    num = re.compile(r"(Prec@1|Prec@5|Loss|loss_c|loss_a|loss_e|lr:) (-?[0-9.]+)")
    for a, b in zip(*outs):
        fa, fb = num.findall(a), num.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb] and {"Prec@1", "Loss", "loss_c", "loss_a", "loss_e"} <= {k for k, _ in fa}
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-3 * max(1.0, abs(float(y))), (k, x, y, a, b)
    assert all(float(dict(num.findall(ln))["loss_e"]) > 0 for ln in outs[0])      # the target entropy is logged, and it is not zero
    # the checkpoints load: model and optimiser state
    sds = []
    for ck in cks:
        net = torch.nn.DataParallel(VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64,
                                               use_attn="TransAttn", verbose=False))
        net.load_state_dict(ck["state_dict"])
        sds.append({k: v.double() for k, v in ck["state_dict"].items() if v.dtype.is_floating_point})
        opt = torch.optim.SGD(net.parameters(), 0.1, momentum=0.9, nesterov=True)
        opt.load_state_dict(ck["optimizer"])
    assert set(sds[0]) == set(sds[1])
    worst = max(((sds[0][k] - sds[1][k]).norm().item() / max(sds[1][k].norm().item(), 1e-30)) for k in sds[0])
    print(f"[main target] worst per-tensor rel. L2 of the saved parameters, fused step vs module path: {worst:.2e}")      # (reported: the log lines above are the comparison)
