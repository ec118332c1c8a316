"""TrainEngine's argument / environment switches are settled in one place (ta3n_amd.engine._resolve_switches): for each switch the four
inputs - argument None with the variable unset, None with it set, argument True, argument False - give the value the constructor's
own expressions gave when each site read the environment itself.  The expected values are written out by hand from those expressions;
the two places that see a switch in another form than the engine runs with (documented at the resolver) are covered through
TrainEngine(...) itself."""
import pytest
import torch

from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS, TrainEngine, _resolve_switches

# field, argument, variable, the value that sets it, (None + unset, None + set, on, off), the argument's (on, off)
ARG_SWITCHES = [
    ("sharded_update", "sharded_update", "TA3N_DDP_SHARDED", "1", (False, True, True, False), (True, False)),
    ("peer_exchange", "peer_exchange", "TA3N_DDP_PEER", "1", (False, True, True, False), (True, False)),
    ("grad_bf16", "grad_transport", "TA3N_DDP_BF16", "1", (False, True, True, False), ("bf16", "fp32")),
    ("ddp_buckets", "ddp_buckets", "TA3N_DDP_BUCKETS", "2", (1, 2, 2, 1), (2, 1)),
    ("split_k", "split_k", "TA3N_SPLIT_K", "4", (0, 4, 6, 0), (6, 0)),
]
# field, variable, value, (unset, set)
ENV_SWITCHES = [
    ("ddp_selftest", "TA3N_DDP_SELFTEST", "1", (False, True)),
    ("ddp_native", "TA3N_DDP_NATIVE", "0", (True, False)),
    ("phase_tiles_env", "TA3N_PHASE_TILES", "3:222,5:114", ("", "3:222,5:114")),
    ("cost_model", "TA3N_COST_MODEL", "1", (0, 1)),
    ("side_update", "TA3N_SIDE_UPDATE", "0", (True, False)),
    ("native_mcd", "TA3N_NATIVE_MCD", "0", (True, False)),
    ("native_discrepancy", "TA3N_NATIVE_DISCREPANCY", "0", (True, False)),
    ("fused_update", "TA3N_FUSED_UPDATE", "1", (False, True)),
    ("sharded_two_streams", "TA3N_DDP_SHARDED_STREAMS", "2", (False, True)),
]


@pytest.mark.parametrize("field,arg,var,value,want,on_off", ARG_SWITCHES, ids=[s[0] for s in ARG_SWITCHES])
def test_argument_wins_over_the_variable_when_not_none(field, arg, var, value, want, on_off):
    assert getattr(_resolve_switches(env={}), field) == want[0]
    assert getattr(_resolve_switches(env={var: value}), field) == want[1]
    for env in ({}, {var: value}, {var: "0"}):      # an argument that is not None: the variable is not looked at
        assert getattr(_resolve_switches(env=env, **{arg: on_off[0]}), field) == want[2]
        assert getattr(_resolve_switches(env=env, **{arg: on_off[1]}), field) == want[3]
    assert type(getattr(_resolve_switches(env={var: value}), field)) is type(want[1])


@pytest.mark.parametrize("field,var,value,want", ENV_SWITCHES, ids=[s[0] for s in ENV_SWITCHES])
def test_switches_without_an_argument(field, var, value, want):
    assert getattr(_resolve_switches(env={}), field) == want[0]
    assert getattr(_resolve_switches(env={var: value}), field) == want[1]
    for arg, on_off in (("sharded_update", (True, False)), ("chain", (True, False))):      # no argument reaches them
        for v in on_off:
            assert getattr(_resolve_switches(env={var: value}, **{arg: v}), field) == want[1]


def test_values_that_are_not_the_switch_leave_the_default():
    """== "1" switches: any other text is off; != "0" switches (native MCD / discrepancy): any other text is on; the streams: only "2"."""
    sw = _resolve_switches(env={"TA3N_DDP_SELFTEST": "yes", "TA3N_DDP_SHARDED": "true", "TA3N_DDP_PEER": "2", "TA3N_DDP_BF16": "",
                                "TA3N_DDP_NATIVE": "yes", "TA3N_CHAIN": "on", "TA3N_SIDE_UPDATE": "yes", "TA3N_NATIVE_MCD": "no",
                                "TA3N_NATIVE_DISCREPANCY": "", "TA3N_FUSED_UPDATE": "2", "TA3N_DDP_SHARDED_STREAMS": "3", "TA3N_PHASE_TILES": ""})
    assert not (sw.ddp_selftest or sw.sharded_update or sw.peer_exchange or sw.grad_bf16 or sw.ddp_native or sw.chain_env or sw.side_update
                or sw.fused_update or sw.sharded_two_streams or sw.phase_tiles_env)
    assert sw.native_mcd and sw.native_discrepancy


def test_chain_keeps_the_argument_and_the_default_apart():
    """chain: as an argument it is taken as given; TA3N_CHAIN=1 is a default that holds only where chained launches are built.  The record
    keeps the two apart, and the refusals see the argument alone (None: off)."""
    for env, chain, want in (({}, None, (False, False, False)), ({"TA3N_CHAIN": "1"}, None, (False, False, True)),
                             ({}, True, (True, True, False)), ({"TA3N_CHAIN": "1"}, False, (True, False, True)),
                             ({}, False, (True, False, False))):
        sw = _resolve_switches(env=env, chain=chain)
        assert (sw.chain_given, sw.chain_arg, sw.chain_env) == want


def test_peer_exchange_as_passed_is_kept_beside_the_resolved_one():
    for env, arg, want in (({}, None, (False, False)), ({"TA3N_DDP_PEER": "1"}, None, (True, False)), ({}, True, (True, True)),
                           ({"TA3N_DDP_PEER": "1"}, False, (False, False))):
        sw = _resolve_switches(env=env, peer_exchange=arg)
        assert (sw.peer_exchange, sw.peer_exchange_arg) == want


def test_the_record_is_immutable_and_reads_os_environ_by_default(monkeypatch):
    monkeypatch.setenv("TA3N_SPLIT_K", "2")
    sw = _resolve_switches()
    assert sw.split_k == 2
    with pytest.raises(AttributeError):
        sw.split_k = 0


def _stops_at_the_device_check(**kw):
    """The options are accepted: on a machine without a GPU the constructor then stops where it needs the device."""
    with pytest.raises(_lib.Ta3nError, match="needs a HIP device"):
        TrainEngine(6, 4, 5, 512, 64, 12, **kw)


def test_adam_refusal_sees_the_peer_argument_only(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("TA3N_DDP_PEER", "1")
    _stops_at_the_device_check(optimizer="Adam")
    with pytest.raises(NotImplementedError, match="optimizer Adam together with the peer gradient exchange"):
        TrainEngine(6, 4, 5, 512, 64, 12, optimizer="Adam", peer_exchange=True)
    # ... while the target options see the resolved switch
    with pytest.raises(NotImplementedError, match="--use_target Sv together with the peer gradient exchange"):
        TrainEngine(6, 4, 5, 512, 64, 12, flags=ALL_FLAGS | _lib.FLAG_TARGET_LABELS)


def test_add_fc_and_frame_attention_see_chain_as_passed(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("TA3N_CHAIN", "1")
    _stops_at_the_device_check(add_fc=2)
    _stops_at_the_device_check(flags=ALL_FLAGS | _lib.FLAG_FRAME_ATTN)
    with pytest.raises(NotImplementedError, match=r"--add_fc 2 together with chained launches \(chain\)"):
        TrainEngine(6, 4, 5, 512, 64, 12, add_fc=2, chain=True)
    with pytest.raises(NotImplementedError, match=r"--use_attn_frame TransAttn together with chained launches \(chain\)"):
        TrainEngine(6, 4, 5, 512, 64, 12, flags=ALL_FLAGS | _lib.FLAG_FRAME_ATTN, chain=True)


def test_option_errors_win_in_the_order_they_always_did(monkeypatch):
    """weights -> target -> optimiser -> add_fc -> frame attention -> dis_DA -> use_bn -> ens_DA -> arithmetic -> aggregation, all before
    the device is asked for."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    bad = dict(class_weights=[1.0], optimizer="RMSprop", add_fc=4, dis_DA="CORAL", use_bn="GN", ens_DA="co", f32_split=True, bf16=True,
               aggregation="rnn")
    for key, err, named in (("class_weights", ValueError, "class_weights has 1 entries"), ("optimizer", NotImplementedError, "optimizer 'RMSprop'"),
                            ("add_fc", NotImplementedError, "--add_fc 4"), ("dis_DA", NotImplementedError, "dis_DA 'CORAL'"),
                            ("use_bn", NotImplementedError, "use_bn 'GN'"), ("ens_DA", NotImplementedError, "ens_DA 'co'"),
                            ("f32_split", ValueError, "different arithmetics"), ("aggregation", NotImplementedError, "frame_aggregation 'rnn'")):
        with pytest.raises(err, match=named):
            TrainEngine(6, 4, 5, 512, 64, 12, **bad)
        bad.pop(key)
        if key == "f32_split":
            bad.pop("bf16")
    _stops_at_the_device_check()
