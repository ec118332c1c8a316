"""--optimizer Adam, host side (no GPU): the bias corrections of ta3n_adam_scalars against Python's own, the option gate
(main.py accepts Adam, train_ddp.py names main.py), the torch.optim.Adam checkpoint form, argument checks of ta3n_adam_range
that must answer before any device is touched, and the schedules TrainEngine refuses by name under Adam."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import train_ddp  # noqa: E402
from ta3n_amd import _lib  # noqa: E402
from ta3n_amd.opts import parser  # noqa: E402

BASE = ["classInd.txt", "RGB", "s.txt", "t.txt", "v.txt", "--baseline_type", "video", "--frame_aggregation", "trn-m",
        "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn", "--add_loss_DA", "attentive_entropy",
        "--lr_adaptive", "dann", "--fc_dim", "512"]
TA3N_ERR_INVALID = -1      # include/ta3n_hip.h


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
@pytest.mark.parametrize("lr,b1,b2", [(1e-3, 0.9, 0.999), (3e-2, 0.5, 0.99)])
def test_adam_scalars_equal_pythons_bias_corrections(t, lr, b1, b2):
    # torch/optim/adam.py forms both in Python floats from the 1-based step; the learning rate crosses the C ABI as fp32
    lr32 = float(np.float32(lr))
    ss, bc = C.c_float(), C.c_float()
    assert _lib.lib().ta3n_adam_scalars(t, lr32, b1, b2, C.byref(ss), C.byref(bc)) == 0
    assert np.float32(ss.value) == np.float32(lr32 / (1 - b1 ** t))
    assert np.float32(bc.value) == np.float32((1 - b2 ** t) ** 0.5)


def test_adam_scalars_refuse_step_zero_and_bad_betas():
    L = _lib.lib()
    ss, bc = C.c_float(), C.c_float()
    assert L.ta3n_adam_scalars(0, 1e-3, 0.9, 0.999, C.byref(ss), C.byref(bc)) == TA3N_ERR_INVALID
    assert L.ta3n_adam_scalars(1, 1e-3, 1.0, 0.999, C.byref(ss), C.byref(bc)) == TA3N_ERR_INVALID
    assert b"step" in L.ta3n_last_error() or b"beta" in L.ta3n_last_error()


def test_main_accepts_adam_and_train_ddp_names_main():
    args = parser.parse_args(BASE + ["--optimizer", "Adam"])
    train_ddp.validate_options(args, module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(args)
    assert "unsupported option" in str(e.value) and "--optimizer Adam" in str(e.value) and "main.py" in str(e.value)
    assert "train_ddp.py trains with SGD" in str(e.value)
    with pytest.raises(SystemExit):      # no other optimiser slips in with Adam
        train_ddp.validate_options(argparse.Namespace(**{**vars(args), "optimizer": "RMSprop"}), module_path=True)


def _small():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2), torch.nn.Linear(5, 1))      # the last layer is dead: no gradient
    return net, [n for n, _ in net.named_parameters()]


def test_adam_optimizer_entry_loads_into_torch_adam():
    from ta3n_amd.checkpoint import adam_optimizer_state_dict, optimizer_kind
    net, names = _small()
    live = names[:4]
    moments = {n: (torch.full_like(p, 0.25), torch.full_like(p, 0.5)) for n, p in net.named_parameters() if n in live}
    sd = adam_optimizer_state_dict(names, moments, step=7, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    assert optimizer_kind(sd) == "Adam"
    opt = torch.optim.Adam(net.parameters(), 1e-3, weight_decay=1e-4)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 2.5e-4 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 1e-4 and not g["amsgrad"]
    params = list(net.parameters())
    for i, p in enumerate(params):
        if names[i] in live:
            st = opt.state[p]
            assert float(st["step"]) == 7.0 and st["step"].dtype == torch.float32
            assert torch.equal(st["exp_avg"], torch.full_like(p, 0.25)) and torch.equal(st["exp_avg_sq"], torch.full_like(p, 0.5))
        else:
            assert p not in opt.state or len(opt.state[p]) == 0      # a dead parameter has no state
    # the keys torch itself writes after one step on the same module (dead layer: no gradient, no state)
    ref = torch.optim.Adam(net.parameters(), 1e-3, weight_decay=1e-4)
    net[1](net[0](torch.ones(2, 4))).sum().backward()
    ref.step()
    want = ref.state_dict()
    assert set(sd) == set(want)
    assert set(sd["param_groups"][0]) == set(want["param_groups"][0])
    assert set(sd["state"]) == set(want["state"]) == {0, 1, 2, 3}
    for i in want["state"]:
        assert set(sd["state"][i]) == set(want["state"][i])
        assert sd["state"][i]["step"].dtype == want["state"][i]["step"].dtype and sd["state"][i]["step"].shape == want["state"][i]["step"].shape
    # the loaded state steps on: torch accepts it as its own
    opt.zero_grad()
    net[1](net[0](torch.ones(2, 4))).sum().backward()
    opt.step()
    assert float(opt.state[params[0]]["step"]) == 8.0


class _FakeEngine:
    """What load_into_engine touches before it decides whether the optimiser entry fits."""
    def __init__(self, optimizer):
        self.optimizer, self.loaded = optimizer, False

    def load_state(self, sd):
        self.loaded = True


@pytest.mark.parametrize("eng_opt,ckpt_opt", [("Adam", "SGD"), ("SGD", "Adam")])
def test_checkpoint_of_the_other_optimizer_is_refused_before_anything_is_loaded(eng_opt, ckpt_opt):
    from ta3n_amd.checkpoint import adam_optimizer_state_dict, load_into_engine, optimizer_state_dict
    net, names = _small()
    entry = (adam_optimizer_state_dict(names, {}, 0, 1e-3, (0.9, 0.999), 1e-8, 0.0) if ckpt_opt == "Adam"
             else optimizer_state_dict(names, {}, lr=0.01, mu=0.9, weight_decay=1e-4))
    eng = _FakeEngine(eng_opt)
    with pytest.raises(ValueError, match=ckpt_opt):
        load_into_engine(eng, net, {"epoch": 1, "state_dict": {}, "optimizer": entry}, resume_hp=True)
    assert not eng.loaded


def _plan():
    return _lib.Plan(12, 8, 5, 512, 128, 12, 0x1F)


def test_adam_range_argument_checks_answer_without_a_device():
    L, plan = _lib.lib(), _plan()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16

    def call(params=a, m=a, begin=0, end=4, step=1):
        return L.ta3n_adam_range(plan.handle, params, a, m, a, a, begin, end, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, step, None)
    assert call(params=None) == TA3N_ERR_INVALID and b"null" in L.ta3n_last_error()
    assert call(m=None) == TA3N_ERR_INVALID
    assert call(step=0) == TA3N_ERR_INVALID and b"step" in L.ta3n_last_error()
    assert call(begin=2) == TA3N_ERR_INVALID and b"4-float aligned" in L.ta3n_last_error()
    assert call(end=plan.live_floats + 4) == TA3N_ERR_INVALID
    assert call(params=a + 4) == TA3N_ERR_INVALID and b"aligned" in L.ta3n_last_error()
    hy = _lib.Hyper()
    assert L.ta3n_adam_step_next(plan.handle, a, a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, 0, C.byref(hy), None) == TA3N_ERR_INVALID
    assert L.ta3n_adam_step_next(plan.handle, a, a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, 1, None, None) == TA3N_ERR_INVALID
    assert L.ta3n_train_steps_adam(plan.handle, a, a, a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, 0, C.byref(hy), 1, None, None,
                                   None) == TA3N_ERR_INVALID
    assert L.ta3n_train_steps_adam(plan.handle, a, a, a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, 1, None, 1, None, None,
                                   None) == TA3N_ERR_INVALID


def test_engine_refuses_sgd_only_schedules_under_adam_by_name(monkeypatch):
    """The refusals that are decided before the engine asks for a device."""
    from ta3n_amd.engine import TrainEngine, adam_refusal
    with pytest.raises(NotImplementedError, match="Adam.*sharded update"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="Adam", sharded_update=True)
    with pytest.raises(NotImplementedError, match="Adam.*peer"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="Adam", peer_exchange=True)
    with pytest.raises(NotImplementedError, match="Adam.*process group"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="Adam", process_group=object())
    monkeypatch.setenv("TA3N_DDP_SELFTEST", "1")
    with pytest.raises(NotImplementedError, match="Adam.*TA3N_DDP_SELFTEST"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="Adam")
    monkeypatch.delenv("TA3N_DDP_SELFTEST")
    with pytest.raises(NotImplementedError, match="RMSprop"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="RMSprop")
    with pytest.raises(ValueError, match="betas"):
        TrainEngine(12, 8, 5, 512, 128, 12, optimizer="Adam", betas=(1.0, 0.999))
    assert adam_refusal() == ""
    for kw, word in ((dict(world=2), "world size 2"), (dict(fused_update=True), "fused_update"), (dict(capture=True), "capture()"),
                     (dict(two_stream=True), "two-stream"), (dict(side_update=True), "TA3N_SIDE_UPDATE")):
        assert word in adam_refusal(**kw) and "Adam" in adam_refusal(**kw)
