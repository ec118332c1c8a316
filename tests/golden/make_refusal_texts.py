"""What the option refusals of ta3n_amd/engine.py say, and what TrainEngine and main._fast_engine decide from them, for a fixed set of
inputs: what "every message, exception type, precedence and engine-or-module-path decision stays" means for a restructuring of them.

    python tests/golden/make_refusal_texts.py        # writes tests/golden/refusal_texts.json

Run it on the commit whose behaviour is the REFERENCE (the parent of a refactor of the refusals), never on the code under test: the
JSON is the evidence, tests/test_refusal_table_cpu.py computes every entry again and compares for equality.  Host-only: no GPU (the
engine's constructor is run with torch.cuda.is_available patched to False, so an accepted combination ends at "needs a HIP device").
Deterministic: the file holds no commit, date or path, so running it on a tree that behaves the same reproduces it byte for byte.

The file has three parts; every distinct message is stored once in "messages" and named by its index.
  "functions": per public refusal function [keywords, result]: the result is a message index, for weights_refusal_kind
               [exception type name or null, message index].  Inputs: the feature on and nothing else (and the bare defaults), every
               keyword at a refused value, every pair of them (the order of the joined labels is part of the message), the early exits.
  "engine":    per case [case, [[exception type name, message index] per environment of "envs"]] of TrainEngine(6, 4, 5, 512, 64, 12,
               **case): every feature alone, with every other option a refusal looks at, and every pair of features (which refusal wins).
               A case is the constructor's keywords, with "flags_on" / "flags_off" (names of _lib.FLAG_*) standing for
               flags=(ALL_FLAGS | on) & ~off and "process_group": true for an object that is not None.
  "fast_engine": main._fast_engine over the grid "axes" (last axis fastest): "grid" indexes "outcomes", each "module path" or the
               [positional, keyword] arguments TrainEngine would have been built with.
"""
import argparse
import contextlib
import io
import itertools
import json
import os
import sys
from unittest import mock

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

JSON_PATH = os.path.join(HERE, "refusal_texts.json")

# ---- (a) the refusal functions: the keywords that turn the feature on, the refused value of every other keyword, the early exits
ON = dict(use_bn="AdaBN", dis_DA="DAN", ens_DA="MCD", chain=True, split_k=2, wgrads_late=True, phase_tiles=True, f32_split=True, add_fc=2,
          use_attn_frame="TransAttn", use_attn="general", frame_aggregation="avgpool", world=2, process_group=True, ddp_selftest=True,
          sharded_update=True, peer_exchange=True, fused_update=True, side_update=True, capture=True, two_stream=True, feeds=True,
          multi_step=True, optimizer="Adam", share_params="N")
RANKS = ("world", "process_group", "ddp_selftest", "sharded_update", "peer_exchange")
FUNCTIONS = {
    "add_fc_refusal": dict(
        base=dict(add_fc=2), keys=("use_bn", "dis_DA", "ens_DA", "chain", "split_k", "wgrads_late", "phase_tiles"),
        exits=[dict(add_fc=0), dict(add_fc=4), dict(add_fc=1), dict(add_fc=1, use_bn="AdaBN"), dict(add_fc=3), dict(add_fc=3, dis_DA="JAN"),
               dict(add_fc=4, use_bn="AdaBN"), dict(add_fc=-1, chain=True)]),
    "frame_attn_refusal": dict(
        base=dict(use_attn_frame="TransAttn"),
        keys=("use_attn", "frame_aggregation", "add_fc", "use_bn", "dis_DA", "ens_DA", "f32_split", "chain", "split_k", "wgrads_late"),
        values=dict(use_attn="none"),
        exits=[dict(use_attn_frame="none"), dict(use_attn_frame="none", use_bn="AdaBN"), dict(use_attn_frame="general"),
               dict(use_attn_frame="general", frame_aggregation="avgpool"), dict(use_attn_frame="TransAttn", use_attn="general"),
               dict(use_attn_frame="TransAttn", use_attn="general", frame_aggregation="avgpool", use_bn="AdaBN"), dict(use_attn_frame="TransAttn", add_fc=3)]),
    "general_attn_refusal": dict(
        base=dict(),
        keys=("frame_aggregation", "use_attn_frame", "add_fc", "use_bn", "dis_DA", "ens_DA", "f32_split", "chain", "split_k", "wgrads_late",
              "phase_tiles") + RANKS,
        exits=[dict(use_attn="TransAttn"), dict(use_attn="none", use_bn="AdaBN", world=2), dict(use_attn="general", use_attn_frame="general"),
               dict(use_attn="general", frame_aggregation="avgpool", world=2)]),
    "share_params_refusal": dict(
        base=dict(),
        keys=("frame_aggregation", "use_attn", "use_attn_frame", "add_fc", "use_bn", "dis_DA", "ens_DA", "f32_split", "chain", "split_k",
              "wgrads_late", "phase_tiles") + RANKS,
        exits=[dict(share_params="Y"), dict(share_params="Y", use_bn="AdaBN", world=2), dict(share_params="X"),
               dict(share_params="X", frame_aggregation="avgpool"), dict(share_params="N", use_attn="none"),
               dict(share_params="N", frame_aggregation="avgpool", world=2)]),
    "adam_refusal": dict(base=dict(), keys=RANKS + ("fused_update", "side_update", "capture", "two_stream"), exits=[]),
    "target_refusal": dict(
        base=dict(use_target="Sv"), keys=RANKS + ("ens_DA",),
        exits=[dict(use_target="none"), dict(use_target="uSv", world=2), dict(use_target="none", add_loss_DA="target_entropy", world=2),
               dict(use_target="uSv", add_loss_DA="target_entropy"), dict(use_target="uSv", add_loss_DA="target_entropy", world=2),
               dict(use_target="uSv", add_loss_DA="target_entropy", ens_DA="MCD"), dict(use_target="Sv", add_loss_DA="target_entropy"),
               dict(use_target="Sv", add_loss_DA="target_entropy", world=2, ens_DA="MCD"), dict(use_target="Sv", add_loss_DA="attentive_entropy", world=2),
               dict(use_target="Sv", ens_DA="co")]),
    "weights_refusal": dict(
        base=dict(class_weights=[1.0, 2.0, 0.5], num_class=3), keys=("world", "process_group", "ddp_selftest"),
        exits=[dict(class_weights=[1.0, 2.0], num_class=3), dict(class_weights=[1.0, 0.0, 1.0], num_class=3, world=2),
               dict(class_weights=[1.0, float("inf"), 1.0], num_class=3), dict(domain_weights=[1.0, 2.0]), dict(domain_weights=[1.0, 2.0], world=2),
               dict(domain_weights=[1.0]), dict(domain_weights=[1.0, -1.0]), dict(class_weights=[1.0, 2.0, 0.5], num_class=3, domain_weights=[1.0]),
               dict(class_weights=[1.0, 2.0, 0.5], num_class=3, domain_weights=[1.0], world=2),
               dict(class_weights=[1.0], num_class=3, domain_weights=[1.0])]),
    "pretrain_refusal": dict(
        base=dict(),
        keys=("optimizer", "dis_DA", "ens_DA", "use_attn", "use_attn_frame", "share_params", "add_fc", "use_bn", "f32_split", "feeds", "capture",
              "fused_update", "multi_step") + RANKS,
        exits=[dict(use_attn="none"), dict(use_attn="TransAttn"), dict(share_params="Y"), dict(optimizer="SGD"), dict(add_fc=3)]),
}
FUNCTIONS["weights_refusal_kind"] = FUNCTIONS["weights_refusal"]


def function_inputs(name):
    """The keyword sets one refusal function is asked with, in a fixed order."""
    spec = FUNCTIONS[name]
    base, values = spec["base"], dict(ON, **spec.get("values", {}))
    out = [dict(), dict(base)] if base else [dict()]
    out += [dict(base, **{k: values[k]}) for k in spec["keys"]]
    out += [dict(base, **{a: values[a], b: values[b]}) for a, b in itertools.combinations(spec["keys"], 2)]
    return out + [dict(e) for e in spec["exits"]]


def ask_function(name, kw):
    """(exception type name or None, message) of one call; a function that takes no such call (a required argument left out) is an
    outcome too."""
    from ta3n_amd import engine
    try:
        got = getattr(engine, name)(**kw)
    except TypeError:
        return "TypeError", "TypeError"
    if name == "weights_refusal_kind":
        return (None if got[0] is None else got[0].__name__), got[1]
    return None, got


# ---- (b) the constructor
ENVS = [{}, {"TA3N_CHAIN": "1"}, {"TA3N_DDP_PEER": "1"}, {"TA3N_DDP_SHARDED": "1"}, {"TA3N_DDP_SELFTEST": "1"}, {"TA3N_PHASE_TILES": "3:222"}]
FEATURES = [
    ("add_fc", dict(add_fc=2)),
    ("frame_attn", dict(flags_on=["FLAG_FRAME_ATTN"])),
    ("general_attn", dict(flags_on=["FLAG_GENERAL_ATTN"], flags_off=["FLAG_TRANS_ATTN"])),
    ("share_params", dict(share_params="N")),
    ("adam", dict(optimizer="Adam")),
    ("target_labels", dict(flags_on=["FLAG_TARGET_LABELS"])),
    ("target_entropy", dict(flags_on=["FLAG_TARGET_ENTROPY"])),
    ("class_weights", dict(class_weights=[1.0 + 0.25 * c for c in range(12)])),
    ("pretrain", dict(pretrain_source=True)),
]
OPTIONS = [
    dict(use_bn="AdaBN"), dict(use_bn="AutoDIAL"), dict(dis_DA="DAN"), dict(dis_DA="JAN"), dict(ens_DA="MCD"), dict(add_fc=3), dict(add_fc=0),
    dict(add_fc=4), dict(f32_split=True), dict(bf16=True), dict(chain=True), dict(chain=False), dict(split_k=2), dict(wgrads_late=True),
    dict(phase_tiles=[0, 0, 0, 222]), dict(phase_tiles=[0, 0]), dict(process_group=True), dict(sharded_update=True), dict(sharded_update=False),
    dict(peer_exchange=True), dict(peer_exchange=False), dict(aggregation="avgpool"), dict(fused=False), dict(share_params="X"),
    dict(flags_off=["FLAG_TRANS_ATTN"]), dict(flags_on=["FLAG_GENERAL_ATTN"]), dict(flags_on=["FLAG_UNSHARED"]),
    dict(domain_weights=[0.5, 2.0]), dict(class_weights=[1.0, 2.0]), dict(optimizer="RMSprop"), dict(betas=(1.0, 0.999)),
]


def merged(*cases):
    out = {}
    for c in cases:
        for k, v in c.items():
            if k in ("flags_on", "flags_off"):
                out[k] = sorted(set(out.get(k, [])) | set(v))
            else:
                out[k] = v
    return out


def engine_cases():
    cases = [dict()] + [dict(o) for o in OPTIONS] + [dict(f) for _, f in FEATURES]
    cases += [merged(f, o) for _, f in FEATURES for o in OPTIONS]
    cases += [merged(a, b) for (_, a), (_, b) in itertools.combinations(FEATURES, 2)]
    cases += [merged(a, b, dict(process_group=True)) for (_, a), (_, b) in itertools.combinations(FEATURES, 2)]
    return cases


def engine_keywords(case):
    from ta3n_amd import _lib
    from ta3n_amd.engine import ALL_FLAGS
    kw = {k: v for k, v in case.items() if k not in ("flags_on", "flags_off")}
    if "flags_on" in case or "flags_off" in case:
        flags = ALL_FLAGS
        for n in case.get("flags_on", ()):
            flags |= getattr(_lib, n)
        for n in case.get("flags_off", ()):
            flags &= ~getattr(_lib, n)
        kw["flags"] = flags
    if kw.get("process_group"):
        kw["process_group"] = object()
    else:
        kw.pop("process_group", None)
    return kw


@contextlib.contextmanager
def environment(env):
    """os.environ without any TA3N_* variable but those of env."""
    import torch
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TA3N_")}
    with mock.patch.dict(os.environ, dict(clean, **env), clear=True), mock.patch.object(torch.cuda, "is_available", lambda: False):
        yield


def ask_engine(case, env):
    from ta3n_amd.engine import TrainEngine
    with environment(env):
        try:
            TrainEngine(6, 4, 5, 512, 64, 12, **engine_keywords(case))
        except Exception as ex:      # noqa: BLE001 - the type is what is recorded
            return type(ex).__name__, str(ex)
    return None, ""


# ---- (c) main._fast_engine
AXES = [("add_fc", [1, 2, 3, 4]), ("use_attn_frame", ["none", "TransAttn"]), ("use_attn", ["TransAttn", "none", "general"]),
        ("share_params", ["Y", "N"]), ("dis_DA", ["none", "DAN"]), ("ens_DA", ["none", "MCD"]), ("use_bn", ["none", "AdaBN"]),
        ("use_target", ["none", "uSv", "Sv"]), ("pretrain_source", [False, True])]


class _Model:
    """What _fast_engine reads of model / model.module."""

    def __init__(self):
        import torch
        self.module, self.feature_dim, self._p = self, 512, torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self._p])


class _Built:
    fused = True

    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw

    def describe(self):
        return ""


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v if isinstance(v, (int, float, str, bool, type(None))) else str(v)


def ask_fast_engine(point, optimizer):
    """'module path', or [positional, keyword] arguments of the engine _fast_engine builds at one grid point."""
    import main
    from ta3n_amd import engine
    ns = argparse.Namespace(
        frame_aggregation="trn-m", save_attention=-1, add_loss_DA="attentive_entropy", place_adv=["Y", "Y", "Y"], adv_DA="RevGrad",
        batch_size=[6, 4, 4], num_segments=5, fc_dim=64, dropout_i=0.5, dropout_v=0.5, clip_gradient=20.0, no_partialbn=True, print_freq=1,
        lr_adaptive="dann", epochs=2, place_dis=["N", "Y", "N"], **point)
    with environment({}), mock.patch.object(main, "args", ns), mock.patch.object(engine, "TrainEngine", _Built), \
            contextlib.redirect_stdout(io.StringIO()):
        eng = main._fast_engine(_Model(), optimizer, 12, None, None)
    if eng is None:
        return "module path"
    return [_plain(eng.args), {k: _plain(v) for k, v in sorted(eng.kw.items())}]


def fast_engine_grid():
    import torch
    optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.03, momentum=0.9, weight_decay=1e-4, nesterov=True)
    for values in itertools.product(*(v for _, v in AXES)):
        yield ask_fast_engine(dict(zip((k for k, _ in AXES), values)), optimizer)


class Index:
    """Distinct values in the order they first appear; add() gives the index."""

    def __init__(self):
        self.items, self._at = [], {}

    def add(self, v):
        key = json.dumps(v, sort_keys=True)
        if key not in self._at:
            self._at[key] = len(self.items)
            self.items.append(v)
        return self._at[key]


def record():
    """The whole fixture as the object that is written."""
    messages = Index()
    functions = {}
    for name in sorted(FUNCTIONS):
        rows = []
        for kw in function_inputs(name):
            kind, text = ask_function(name, kw)
            rows.append([kw, [kind, messages.add(text)] if name == "weights_refusal_kind" or kind else messages.add(text)])
        functions[name] = rows
    engine = []
    for case in engine_cases():
        engine.append([case, [[kind, messages.add(text)] for kind, text in (ask_engine(case, env) for env in ENVS)]])
    outcomes = Index()
    grid = [outcomes.add(o) for o in fast_engine_grid()]
    return {"messages": messages.items, "functions": functions, "engine": {"envs": ENVS, "cases": engine},
            "fast_engine": {"axes": [[k, v] for k, v in AXES], "outcomes": outcomes.items, "grid": grid}}


def dumps(rec):
    """One line per message, input and case."""
    def lines(rows):
        return "[\n" + ",\n".join(json.dumps(r) for r in rows) + "]"
    parts = ['"messages": ' + lines(rec["messages"]),
             '"functions": {\n' + ",\n".join("%s: %s" % (json.dumps(k), lines(v)) for k, v in sorted(rec["functions"].items())) + "}",
             '"engine": {"envs": %s,\n"cases": %s}' % (json.dumps(rec["engine"]["envs"]), lines(rec["engine"]["cases"])),
             '"fast_engine": {"axes": %s,\n"outcomes": %s,\n"grid": %s}' % (json.dumps(rec["fast_engine"]["axes"]), lines(rec["fast_engine"]["outcomes"]),
                                                                          json.dumps(rec["fast_engine"]["grid"], separators=(",", ":")))]
    return "{" + ",\n".join(parts) + "}\n"


def main():
    rec = record()
    with open(JSON_PATH, "w") as f:
        f.write(dumps(rec))
    print("wrote", JSON_PATH, os.path.getsize(JSON_PATH), "bytes;", len(rec["messages"]), "messages,",
          sum(len(v) for v in rec["functions"].values()), "function calls,", len(rec["engine"]["cases"]), "engine cases x", len(ENVS),
          "environments,", len(rec["fast_engine"]["grid"]), "grid points,", len(rec["fast_engine"]["outcomes"]), "outcomes")


if __name__ == "__main__":
    main()
