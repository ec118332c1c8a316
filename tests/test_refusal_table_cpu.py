"""Which options are built together is one table (ta3n_amd/options.py: CONTEXT, FEATURES, refusal).  tests/golden/refusal_texts.json
holds what the refusal functions returned, what TrainEngine(...) raised and what main._fast_engine decided on the commit before the
table existed (tests/golden/make_refusal_texts.py wrote it there and is never rerun on the code under test): every entry is computed
again here and compared for equality - texts, exception types, which refusal wins, engine or module path.  No case is left out."""
import inspect
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refusal_texts as mr  # noqa: E402

from ta3n_amd import engine, options  # noqa: E402

PUBLIC = ("add_fc_refusal", "frame_attn_refusal", "general_attn_refusal", "share_params_refusal", "adam_refusal", "target_refusal",
          "weights_refusal", "weights_refusal_kind", "pretrain_refusal")


@pytest.fixture(scope="module")
def golden():
    with open(mr.JSON_PATH) as f:
        return json.load(f)


def test_the_fixture_holds_every_input_of_its_generator(golden):
    assert sorted(golden["functions"]) == sorted(PUBLIC) == sorted(mr.FUNCTIONS)
    for name in PUBLIC:
        assert [kw for kw, _ in golden["functions"][name]] == json.loads(json.dumps(mr.function_inputs(name))), name
    assert golden["engine"]["envs"] == mr.ENVS
    assert [case for case, _ in golden["engine"]["cases"]] == json.loads(json.dumps(mr.engine_cases()))
    assert golden["fast_engine"]["axes"] == [[k, v] for k, v in mr.AXES]
    n = 1
    for _, values in mr.AXES:
        n *= len(values)
    assert len(golden["fast_engine"]["grid"]) == n == 2304


@pytest.mark.parametrize("name", PUBLIC)
def test_the_public_functions_return_what_they_returned(golden, name):
    rows = golden["functions"][name]
    assert len(rows) > 10
    for kw, want in rows:
        kind, text = mr.ask_function(name, kw)
        want_kind, want_text = want if isinstance(want, list) else (None, want)
        assert (kind, text) == (want_kind, golden["messages"][want_text]), (name, kw)


@pytest.mark.parametrize("env", range(len(mr.ENVS)), ids=["none"] + [next(iter(e)) for e in mr.ENVS[1:]])
def test_the_constructor_raises_what_it_raised(golden, env):
    accepted = 0
    for case, results in golden["engine"]["cases"]:
        want_kind, want_text = results[env]
        kind, text = mr.ask_engine(case, mr.ENVS[env])
        assert (kind, text) == (want_kind, golden["messages"][want_text]), (case, mr.ENVS[env])
        accepted += kind == "Ta3nError" and "needs a HIP device" in text
    assert accepted >= 20      # (the accepted combinations end where the constructor asks for the device)


def test_main_takes_the_engine_where_it_took_it(golden):
    outcomes, grid = golden["fast_engine"]["outcomes"], golden["fast_engine"]["grid"]
    assert "module path" in outcomes and len(outcomes) > 40
    keys = [k for k, _ in mr.AXES]
    for want, got in zip(grid, mr.fast_engine_grid(), strict=True):
        assert json.loads(json.dumps(got)) == outcomes[want], (keys, want)


# ---- the world size, asked again
SINGLE_RANK = {"adam": ("adam_refusal", {}), "class_weights": ("weights_refusal", dict(class_weights=[1.0, 2.0, 0.5], num_class=3)),
               "target": ("target_refusal", dict(use_target="Sv")), "share_params": ("share_params_refusal", {}),
               "general_attn": ("general_attn_refusal", {}), "pretrain": ("pretrain_refusal", {})}


def _world2_message(golden, feature):
    name, base = SINGLE_RANK[feature]
    (want,) = [w for kw, w in golden["functions"][name] if kw == dict(base, world=2)]
    return golden["messages"][want]


@pytest.mark.parametrize("feature", sorted(SINGLE_RANK))
def test_world_two_refuses_every_single_rank_feature(golden, feature):
    assert set(SINGLE_RANK) == set(options.WORLD_ORDER)
    context = dict(SINGLE_RANK[feature][1], use_attn="general" if feature == "general_attn" else "TransAttn",
                   share_params="N" if feature == "share_params" else "Y")
    want = _world2_message(golden, feature)
    assert "world size 2" in want
    assert options.world_refusal([feature], context, 1) == (None, "")
    assert options.world_refusal([feature], context, 2) == (NotImplementedError, want)
    assert options.world_refusal(["add_fc", "frame_attn"], dict(context, add_fc=2, use_attn_frame="TransAttn"), 2) == (None, "")      # not asked again
    if feature != "adam":      # Adam's wins, wherever it stands among the active features
        for features in (["adam", feature], [feature, "adam"]):
            assert options.world_refusal(features, context, 2) == (NotImplementedError, _world2_message(golden, "adam"))


def test_the_others_win_in_the_order_the_constructor_asks_them(golden):
    context = dict(class_weights=[1.0, 2.0, 0.5], num_class=3, use_target="Sv", share_params="N")
    order = [f for f in options.WORLD_ORDER if f != "adam" and f != "general_attn"]
    for i, feature in enumerate(order):
        kind, text = options.world_refusal(list(reversed(order[i:])), context, 2)
        assert kind is NotImplementedError and text.startswith(options.FEATURES[feature].head if feature != "target" else "--use_target Sv"), feature


# ---- a new option cannot be half-added
def test_every_row_names_context_keys_only():
    keys = [item.key for item in options.CONTEXT]
    assert len(keys) == len(set(keys)) and set(options.RANKS) <= set(keys)
    for name, row in options.FEATURES.items():
        assert set(row.without) <= set(keys), name
        assert all(options.ITEMS[k].label for k in row.without), name      # what a row lists has a name to list it by
        assert set(row.labels) <= set(row.without), name
        assert set(row.reads) <= set(keys) and set(row.reads.values()) <= set(keys), name
        assert {p.rstrip("!") for p in row.params.split()} <= set(keys), name
        assert set(row.defaults) <= {p.rstrip("!") for p in row.params.split()}, name
    assert set(options.WORLD_ORDER) <= set(options.FEATURES)
    labels = [item.label for item in options.CONTEXT if item.label]
    assert len(labels) == len(set(labels))      # one copy of every label


@pytest.mark.parametrize("name", PUBLIC)
def test_every_public_keyword_is_a_context_key(name):
    keys = {item.key for item in options.CONTEXT}
    fn = getattr(engine, name)
    assert fn is getattr(options, name)      # engine.py re-exports the bindings, it has no body of its own
    params = inspect.signature(fn).parameters
    assert params and set(params) <= keys


def test_the_generator_reproduces_the_committed_file(golden):
    """Deterministic, and the tree behaves as the commit the file was written on: byte for byte."""
    with open(mr.JSON_PATH) as f:
        assert mr.dumps(mr.record()) == f.read()
