#!/usr/bin/env python3
"""Label-free collapse metrics of a pre-trained encoder on MI355X: is the feature distribution still spread out?

    python health.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --health_t 2.0

Single process, single device, shaped like knn.py and reading the same videos: a video's feature is the mean of the encoder's
pooled feature over the clips of its test plan.  The train-list videos and the test-list videos are evaluated SEPARATELY and no
label is read: std_ratio, erank, rankme, top1_share, uniformity and nn_sim (cstp_amd.health: ops.l2_normalize, ops.feat_gram,
ops.pair_potential, ops.sim_topk, then fp64 host arithmetic).  ``Health train: ...``, ``Health test: ...`` and a final JSON line
go to the terminal and to health_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.
--dataset synthetic_video builds --retrieval_gallery_len "train" and --synthetic_len / 4 "test" videos; --dataset UcfFineTune
reads UCF-style frame folders (cstp_amd.frame_folder); any other data set is refused.  The figures are monitors: no accuracy is
claimed to follow from them and no run on real data exists.
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import health, retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import health_opts, parse_opts


def build_sets(opts):
    """-> (train-list loader, test-list loader): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts, what="health")


def run(opts):
    if opts.dataset not in ("synthetic_video", "UcfFineTune"):
        raise NotImplementedError("dataset %r: health.py serves --dataset synthetic_video and UcfFineTune" % (opts.dataset,))
    if not torch.cuda.is_available():
        raise RuntimeError("health.py needs a HIP device: cstp_amd has no CPU execution path")
    opts.cuda = True
    opts.distributed = False
    opts.local_rank = 0
    opts.device = torch.device("cuda:0")
    opts.task = "retrieval"          # the model factory's encoder-only task: the pre-training wrapper in eval mode
    print(opts)
    opts.arch = "{}-{}".format(opts.model_name, opts.model_depth)
    t = health_opts(opts)[1]
    train_loader, test_loader = build_sets(opts)
    print("Train videos = {}, test videos = {}".format(len(train_loader), len(test_loader)))
    model = generate_model(opts)
    res = {"train": health.evaluate(model, train_loader, t), "test": health.evaluate(model, test_loader, t)}
    retrieval.close_video_sets(train_loader, test_loader)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "health_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split, opts.sample_duration)
    summary = {"task": "health", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split), "t": t,
               "train": res["train"], "test": res["test"]}
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        for line in ("Health train: " + health.format_line(res["train"]), "Health test: " + health.format_line(res["test"]),
                     json.dumps(summary)):
            print(line)
            f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
