#!/usr/bin/env python
"""Video-level testing of a trained checkpoint on a score-only plan: test_models.py's command line, output lines and files, computed by
ta3n_amd.Scorer (TA3N_FLAG_SCORE_ONLY, ta3n_score) - the launches the class logits depend on, on the model's own parameters, and the
softmax, the label's rank, the top-k hits and the confusion matrix on the device - instead of VideoModel.forward on the clip fed to both
halves with the bookkeeping in torch.

    python score_models.py data/classInd_hmdb_ucf.txt RGB <test_list> <exp>/RGB/model_best.pth.tar \\
        --arch resnet101 --test_segments 5 --baseline_type video --frame_aggregation trn-m --use_attn TransAttn --bS 128 \\
        [--save_confusion <prefix>] [--save_scores <prefix>] [--save_attention <prefix>]

A program of its own beside test_models.py, which stays the reference's tester as it is: it takes that file's parser, so the two command
lines cannot drift apart, and tests/test_gpu_score.py holds its output lines and files to test_models.py's.

A configuration the scorer does not build (use_bn, share_params N, frame / general attention, add_fc 2 / 3) exits and names it; nothing
falls back to test_models.py's path.  Lines cited as :N are this repository's test_models.py."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from ta3n_amd import Scorer  # noqa: E402
from ta3n_amd.dataset import TSNDataSet  # noqa: E402
from ta3n_amd.models import VideoModel  # noqa: E402
from ta3n_amd.utils.utils import plot_confusion_matrix  # noqa: E402
from test_models import build_parser  # noqa: E402


def main(argv=None):
    args = build_parser().parse_args(argv)
    class_names = [line.strip().split(' ', 1)[1] for line in open(args.class_file)]        # :66-69
    num_class = len(class_names)
    top = sorted(args.top)
    kmax = min(max(top), num_class)
    print('preparing the model......')                                                       # :70-79
    seg = args.test_segments if args.baseline_type == 'video' else 1
    net = VideoModel(num_class, args.baseline_type, args.frame_aggregation, args.modality, train_segments=seg, val_segments=seg,
                     base_model=args.arch, add_fc=args.add_fc, fc_dim=args.fc_dim, share_params=args.share_params,
                     dropout_i=args.dropout_i, dropout_v=args.dropout_v, use_bn=args.use_bn, ens_DA=args.ens_DA, partial_bn=False,
                     n_rnn=args.n_rnn, rnn_cell=args.rnn_cell, n_directions=args.n_directions, n_ts=args.n_ts, use_attn=args.use_attn,
                     n_attn=args.n_attn, use_attn_frame=args.use_attn_frame, verbose=args.verbose)
    checkpoint = torch.load(args.weights, map_location="cpu", weights_only=False)
    print("model epoch {} prec@1: {}".format(checkpoint['epoch'], checkpoint['prec1']))
    net.load_state_dict({'.'.join(k.split('.')[1:]): v for k, v in list(checkpoint['state_dict'].items())})
    try:
        scorer = Scorer.from_model(net.cuda(), capacity=args.bS, num_segments=args.test_segments)
    except NotImplementedError as e:
        raise SystemExit(f"score_models.py: {e}")
    print('loading data......')                                                              # :80-86
    data_length = 1 if args.modality == "RGB" else 5
    num_test = sum(1 for _ in open(args.test_list))
    tmpl = "img_{:05d}.t7" if args.modality in ['RGB', 'RGBDiff', 'RGBDiff2', 'RGBDiffplus'] else args.flow_prefix + "{}_{:05d}.t7"
    data_set = TSNDataSet("", args.test_list, num_dataload=num_test, num_segments=args.test_segments, new_length=data_length,
                          modality=args.modality, image_tmpl=tmpl, test_mode=True)
    loader = torch.utils.data.DataLoader(data_set, batch_size=args.bS, shuffle=False, num_workers=args.workers, pin_memory=True)
    max_num = args.max_num if args.max_num > 0 else len(loader.dataset)
    labels, total = [], 0
    print('start testing......')
    t0 = time.time()
    for i, (data, label) in enumerate(loader):                                               # :96-116; no padding: every row of the plan is alike
        if i >= max_num:
            break
        scorer.score(data, label, reset=(i == 0))
        labels.append(label)
        total += data.size(0)
        if args.verbose or i == len(loader) - 1:
            rank = scorer.per_video()["rank"].cpu()
            # a video is a top-t hit when fewer than t classes are ahead of its label (torch.topk order)
            line = ''.join('Pred@%d %f, ' % (t, float((rank < min(t, kmax)).sum()) / total) for t in top)
            print(line + 'average %f sec/video' % ((time.time() - t0) / total))
    out = scorer.per_video()
    labels = torch.cat(labels).numpy() if labels else np.zeros(0, np.int64)
    rank = out["rank"].cpu().numpy()
    if args.save_attention:                                                                  # :117-120
        attn = out["attn"] if out["attn"] is not None else out["feat_v"][:, :1]      # (elsewhere the model returns the placeholder V[:, 0], models.py:627-628)
        np.savetxt(args.save_attention + '.txt', attn.cpu().reshape(total, -1).numpy(), fmt="%s")
    if args.save_scores:
        np.save(args.save_scores + '.npy', out["prob"].cpu().numpy())
    cls_cnt = np.bincount(labels, minlength=num_class)                                       # :121-135
    cls_hit = [np.bincount(labels[rank < min(t, kmax)], minlength=num_class) for t in top]      # videos of class c with fewer than t classes ahead of the label
    cls_acc_topK = [h / np.maximum(cls_cnt, 1) for h in cls_hit]
    if args.save_confusion:
        cf0 = scorer.results()["confusion"].numpy()
        plot_confusion_matrix(args.save_confusion + '.png', cf0, classes=class_names, normalize=True, title='Normalized confusion matrix')
        with open(args.save_confusion + '-top' + str(top) + '.txt', 'w') as f:
            for c in range(num_class):
                f.write(' '.join(str(a[c]) for a in cls_acc_topK) + ' \n')
    if args.verbose:
        for c in range(num_class):
            print(' '.join(str(a[c]) for a in cls_acc_topK))
    print(''.join('Pred@{:d} {:.02f}% '.format(t, h.sum() / max(cls_cnt.sum(), 1) * 100) for t, h in zip(top, cls_hit)))
    return {t: float(h.sum() / max(cls_cnt.sum(), 1) * 100) for t, h in zip(top, cls_hit)}


if __name__ == "__main__":
    main()
