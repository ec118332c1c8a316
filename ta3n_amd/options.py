"""Which options of the train step are built together: one ordered list of what a refusal can name (CONTEXT), one table with a row per
feature (FEATURES), one function that evaluates a row against a context (refusal).  TrainEngine, main.py, train_ddp.py and VideoModel
build a context - a mapping from CONTEXT keys to values, missing keys at their defaults - and ask through it; the *_refusal functions
are bindings of the same rows with keyword arguments.  A new option is a new row (and a CONTEXT entry for what it adds to the other
rows' `without`): tests/test_refusal_table_cpu.py checks that no row names a key the list does not have.  No torch, no device."""
import inspect
import math
from collections import namedtuple

# key of the context; its value when nobody says otherwise; how a refusal names it when it is on (None: read by the rows, named by none);
# on(context) where "on" is something else than "not the default"
Item = namedtuple("Item", "key default label on", defaults=(None, None))

CONTEXT = (
    Item("use_bn", "none", "--use_bn {use_bn}"),
    Item("dis_DA", "none", "--dis_DA {dis_DA}"),
    Item("ens_DA", "none", "--ens_DA {ens_DA}"),
    Item("add_fc", 1, "--add_fc {add_fc}"),
    Item("use_attn_frame", "none", "--use_attn_frame {use_attn_frame}"),
    Item("use_attn", "TransAttn", "--use_attn {use_attn}", lambda c: c["use_attn"] not in ("TransAttn", "none")),
    Item("share_params", "Y", "--share_params N", lambda c: c["share_params"] == "N"),
    Item("optimizer", "SGD", "optimizer Adam (torch keeps a step count per parameter - the parameters the pass does not reach fall behind; the "
                              "engine keeps one)", lambda c: c["optimizer"] == "Adam"),
    Item("f32_split", False, "f32_split"),
    Item("chain", False, "chained launches (chain)"),
    Item("split_k", 0, "split_k"),
    Item("wgrads_late", False, "wgrads_late"),
    Item("phase_tiles", False, "explicit phase_tiles / tuned tile lists"),
    # the multi-rank schedules, as every refusal of a single-rank option lists them (RANKS)
    Item("world", 1, "world size {world} (a process group)", lambda c: c["world"] > 1 or bool(c["process_group"])),
    Item("ddp_selftest", False, "the 1-rank self-test of the data-parallel path (TA3N_DDP_SELFTEST)"),
    Item("sharded_update", False, "the sharded update (sharded_update / TA3N_DDP_SHARDED)"),
    Item("peer_exchange", False, "the peer gradient exchange (peer_exchange / TA3N_DDP_PEER)"),
    # ways of running the step or its update
    Item("fused_update", False, "fused_update"),
    Item("side_update", False, "the side-stream / side-workgroup update (TA3N_SIDE_UPDATE)"),
    Item("capture", False, "capture()"),
    Item("two_stream", False, "the two-stream multi-job call (ta3n_train_steps_multi)"),
    Item("feeds", False, "train_steps(feeds=...)"),
    Item("multi_step", False, "train_steps / the deferred and pipelined steps (the pass is not part of the multi-step calls)"),
    # read by the rows, named by none.  process_group: whether there is one (part of "world").  peer_exchange_arg / chain_arg: the
    # switch as it was passed (engine._resolve_switches), for the rows whose `reads` asks for that form; None where nobody tells them apart
    Item("process_group", False), Item("peer_exchange_arg", None), Item("chain_arg", None),
    Item("frame_aggregation", "trn-m"), Item("use_target", "none"), Item("add_loss_DA", "none"),
    Item("class_weights", None), Item("domain_weights", None), Item("num_class", 0),
)
ITEMS = {item.key: item for item in CONTEXT}
DEFAULTS = {item.key: item.default for item in CONTEXT}
RANKS = ("world", "ddp_selftest", "sharded_update", "peer_exchange")

# One feature: on(c) - is it asked for; exits - (exception type, when(c), sentence) of its own, in order, in front of the list;
# without - the CONTEXT keys it is not built with, in the order the message names them; labels - where this row names (or judges) a key
# otherwise than CONTEXT does: a label, or (on, label); the message is "{head} together with {the labels that are on} is not built{tail}";
# reads - {key: the context key this row sees it through, where the context has that one}; params - the keyword arguments of the public
# binding in their order ("!": required), defaults - where its default is not CONTEXT's
Row = namedtuple("Row", "on exits without head tail labels reads params defaults", defaults=((), (), "", "", {}, {}, "", {}))

_CHAIN_AS_PASSED = {"chain": "chain_arg"}      # TA3N_CHAIN=1 is a default that is itself off where chained launches are not built: only a chain asked for by argument is refused


def _target_options(c):
    return [o for o, on in (("--use_target Sv", c["use_target"] == "Sv"),
                            ("--add_loss_DA target_entropy", c["add_loss_DA"] == "target_entropy" and c["use_target"] != "none")) if on]


def _positive(key):
    return lambda c: any(not (float(v) > 0.0 and math.isfinite(float(v))) for v in c[key])


FEATURES = {
    # --weighted_class_loss: the kernels take the normaliser sum_j w[y_j] over the rank's own rows - single rank
    "class_weights": Row(
        on=lambda c: c["class_weights"] is not None,
        exits=((ValueError, lambda c: len(c["class_weights"]) != c["num_class"], "class_weights has {n_class_weights} entries for {num_class} classes"),
               (ValueError, _positive("class_weights"), "class_weights must be positive and finite (1 / class_freq, main.py:164)")),
        without=("world", "ddp_selftest"), head="class_weights",
        tail=" (the weighted mean divides by the sum of the weights of the rank's own labels: single rank)",
        params="class_weights domain_weights num_class world process_group ddp_selftest"),
    # --weighted_class_loss_DA: the domain factors are formed from the global counts - any world
    "domain_weights": Row(
        on=lambda c: c["domain_weights"] is not None,
        exits=((ValueError, lambda c: len(c["domain_weights"]) != 2, "domain_weights has {n_domain_weights} entries, takes (w_source, w_target)"),
               (ValueError, _positive("domain_weights"),
                "domain_weights must be positive and finite (1 / num_source_train, 1 / num_target_train; main.py:167)"))),
    # --use_target Sv / --add_loss_DA target_entropy: means over this rank's rows with labels this rank holds - single rank
    "target": Row(
        on=lambda c: bool(_target_options(c)), without=RANKS + ("ens_DA",), head=lambda c: " / ".join(_target_options(c)),
        tail=" (target labels and target entropy: single rank)",
        labels={"ens_DA": (lambda c: c["ens_DA"] == "MCD", "--ens_DA MCD (under Sv the reference itself fails at main.py:448; target entropy on "
                                                            "MCD's rebound out_target is not built)")},
        params="use_target add_loss_DA world process_group ddp_selftest sharded_update peer_exchange ens_DA"),
    # optimizer="Adam": one launch over the flat prefix behind the step's gradients on one rank; every schedule it lists is a way of
    # splitting or moving the SGD update.  Sees the peer exchange as passed: TA3N_DDP_PEER=1 in the environment does not refuse a
    # single-rank Adam engine (on one rank without the self-test no exchange is set up at all), peer_exchange=True does
    "adam": Row(
        on=lambda c: True, without=RANKS + ("fused_update", "side_update", "capture", "two_stream"), head="optimizer Adam",
        tail=" (Adam: single rank, the update as one launch behind the step)",
        labels={"fused_update": "fused_update=True (the Nesterov update inside the gradient tiles, TA3N_FUSED_UPDATE)",
                "capture": "capture() (a hipGraph would freeze the step count of the bias corrections)"},
        reads={"peer_exchange": "peer_exchange_arg"},
        params="world sharded_update process_group ddp_selftest peer_exchange fused_update side_update capture two_stream"),
    # --add_fc 2 / 3: TA3N / trn-m and TemPooling with use_bn none, no dis_DA / ens_DA, the default launch shapes
    "add_fc": Row(
        on=lambda c: c["add_fc"] != 1,
        exits=((ValueError, lambda c: c["add_fc"] < 1, "add at least one fc layer (models.py:137-138)"),
               (NotImplementedError, lambda c: c["add_fc"] > 3, "--add_fc {add_fc}: built for 1, 2 and 3 (the reference builds no fourth layer, "
                "models.py:145-153, but shifts the place_dis slicing with add_fc, main.py:368-378)")),
        without=("use_bn", "dis_DA", "ens_DA", "chain", "split_k", "wgrads_late", "phase_tiles"), head="--add_fc {add_fc}",
        reads=_CHAIN_AS_PASSED, params="add_fc! use_bn dis_DA ens_DA chain split_k wgrads_late phase_tiles"),
    # --share_params N: the target rows' own first frame layer and video classifier on trn-m, use_attn TransAttn or none, on one rank
    "share_params": Row(
        on=lambda c: c["share_params"] != "Y",
        exits=((NotImplementedError, lambda c: c["share_params"] != "N", "--share_params {share_params} (built: Y, N)"),
               (NotImplementedError, lambda c: c["frame_aggregation"] != "trn-m",
                "--share_params N on --frame_aggregation {frame_aggregation}: built for trn-m (the unfused launch lists)")),
        without=("use_bn", "dis_DA", "ens_DA", "add_fc", "use_attn_frame", "use_attn", "f32_split", "chain", "split_k", "wgrads_late",
                 "phase_tiles") + RANKS,
        head="--share_params N", tail=" (single rank, the unfused launch lists)", reads=_CHAIN_AS_PASSED,
        params="share_params frame_aggregation use_attn use_attn_frame add_fc use_bn dis_DA ens_DA f32_split chain split_k wgrads_late "
               "phase_tiles world process_group ddp_selftest sharded_update peer_exchange", defaults={"share_params": "N"}),
    # --use_attn general: conventional attention over the relation features of trn-m (models.py:320-325, 359-366, 379-388), on one rank
    "general_attn": Row(
        on=lambda c: c["use_attn"] == "general",
        exits=((NotImplementedError, lambda c: c["frame_aggregation"] != "trn-m", "--use_attn general on --frame_aggregation {frame_aggregation}: "
                "built for trn-m (the reference's aggregate_frames ignores use_attn on avgpool)"),),
        without=("use_attn_frame", "add_fc", "use_bn", "dis_DA", "ens_DA", "f32_split", "chain", "split_k", "wgrads_late", "phase_tiles") + RANKS,
        head="--use_attn general", tail=" (single rank, the unfused launch lists)",
        labels={"use_attn_frame": "--use_attn_frame {use_attn_frame} (the reference sends 'general' frame attention to a 256-wide layer on "
                                  "fc_dim-wide rows)"},
        reads=_CHAIN_AS_PASSED,
        params="use_attn frame_aggregation use_attn_frame add_fc use_bn dis_DA ens_DA f32_split chain split_k wgrads_late phase_tiles world "
               "process_group ddp_selftest sharded_update peer_exchange", defaults={"use_attn": "general"}),
    # --use_attn_frame TransAttn together with --use_attn TransAttn on trn-m (models.py:368-377, 612-614), fp32 and bf16
    "frame_attn": Row(
        on=lambda c: c["use_attn_frame"] != "none",
        exits=((NotImplementedError, lambda c: c["use_attn_frame"] != "TransAttn", "--use_attn_frame {use_attn_frame}: built for TransAttn (the "
                "reference's 'general' frame attention needs an attn_layer its model never creates for frames)"),
               (NotImplementedError, lambda c: c["frame_aggregation"] != "trn-m", "--use_attn_frame TransAttn on --frame_aggregation "
                "{frame_aggregation}: built for trn-m (frame attention in front of the TRN)"),
               (NotImplementedError, lambda c: c["use_attn"] != "TransAttn", "--use_attn_frame TransAttn with --use_attn {use_attn}: the reference "
                "takes the kind of frame attention from --use_attn (models.py:369-372; with use_attn none it raises UnboundLocalError) - built "
                "with --use_attn TransAttn")),
        without=("add_fc", "use_bn", "dis_DA", "ens_DA", "f32_split", "chain", "split_k", "wgrads_late"), head="--use_attn_frame TransAttn",
        reads=_CHAIN_AS_PASSED,
        params="use_attn_frame! use_attn frame_aggregation add_fc use_bn dis_DA ens_DA f32_split chain split_k wgrads_late"),
    # TrainEngine(pretrain_source=True): the source-only pass of --pretrain_source in front of every step (a second plan, ta3n_sgd_live)
    "pretrain": Row(
        on=lambda c: True,
        without=("optimizer", "dis_DA", "ens_DA", "use_attn_frame", "use_attn", "share_params", "add_fc", "use_bn", "f32_split", "feeds",
                 "multi_step", "capture", "fused_update") + RANKS,
        head="pretrain_source", tail=" (the source-only pass: trn-m with use_attn TransAttn / none or avgpool, fp32 or bf16, SGD, add_fc 1, "
                                     "use_bn none, single rank, one step per call)",
        labels={"f32_split": "f32_split (f32x3)"},
        params="optimizer dis_DA ens_DA use_attn use_attn_frame share_params add_fc use_bn f32_split feeds capture fused_update multi_step world "
               "process_group ddp_selftest sharded_update peer_exchange"),
    # TrainEngine(train_meters=True): TA3N_FLAG_TRAIN_METERS - one more launch behind the step's launch list keeps loss sums, Prec@1/5 and the
    # domain discriminators' accuracy on the device; every aggregation, arithmetic, optimiser, schedule and world size, chained launches excepted
    "train_meters": Row(
        on=lambda c: True, without=("chain",), head="train_meters", tail=" (the meters launch stands behind the plain launch lists)",
        reads=_CHAIN_AS_PASSED, params="chain"),
}


def refusal(feature, context):
    """(exception type, message) that refuses `feature` in `context`, (None, "") where it is off or built together with everything the
    context has on."""
    row = FEATURES[feature]
    c = dict(DEFAULTS, **context)
    for key, seen_through in row.reads.items():
        if c[seen_through] is not None:
            c[key] = c[seen_through]
    if not row.on(c):
        return None, ""
    for name in ("class_weights", "domain_weights"):      # (for the sentences that count them)
        c["n_" + name] = len(c[name]) if c[name] is not None else 0
    for kind, when, sentence in row.exits:
        if when(c):
            return kind, sentence.format(**c)
    named = []
    for key in row.without:
        item = ITEMS[key]
        label = row.labels.get(key, item.label)
        on, label = label if isinstance(label, tuple) else (item.on, label)
        if on is None:      # not the default (a switch that defaults to off: any true value)
            is_on = c[key] != item.default if item.default else bool(c[key])
        else:
            is_on = on(c)
        if is_on:
            named.append(label.format(**c))
    if not named:
        return None, ""
    head = row.head(c) if callable(row.head) else row.head.format(**c)
    return NotImplementedError, f"{head} together with {', '.join(named)} is not built{row.tail}"


def first_refusal(features, context):
    """The first (exception type, message) among `features`, asked in that order."""
    for feature in features:
        kind, refused = refusal(feature, context)
        if refused:
            return kind, refused
    return None, ""


# the single-rank features in the order they are asked again once the world size is known: Adam first, then the order TrainEngine asks them
WORLD_ORDER = ("adam", "class_weights", "target", "share_params", "general_attn", "pretrain")


def world_refusal(features, context, world):
    """What refuses the active `features` of an engine on `world` ranks: (exception type, message) of the first of WORLD_ORDER that does."""
    return first_refusal([f for f in WORLD_ORDER if f in features], dict(context, world=world))


def binding(*features, kind=False):
    """The rows of `features` as a function of the first row's keyword arguments that returns the message ('' when nothing is refused),
    with kind=True (exception type or None, message)."""
    row = FEATURES[features[0]]
    names = row.params.split()
    sig = inspect.Signature([inspect.Parameter(
        n.rstrip("!"), inspect.Parameter.POSITIONAL_OR_KEYWORD,
        default=inspect.Parameter.empty if n.endswith("!") else row.defaults.get(n, DEFAULTS[n])) for n in names])

    def asked(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        got = first_refusal(features, bound.arguments)
        return got if kind else got[1]
    asked.__signature__ = sig
    return asked


add_fc_refusal = binding("add_fc")
frame_attn_refusal = binding("frame_attn")
general_attn_refusal = binding("general_attn")
share_params_refusal = binding("share_params")
adam_refusal = binding("adam")
target_refusal = binding("target")
pretrain_refusal = binding("pretrain")
# ValueError: a value that no configuration accepts; NotImplementedError: a combination that is not built
weights_refusal = binding("class_weights", "domain_weights")
weights_refusal_kind = binding("class_weights", "domain_weights", kind=True)
