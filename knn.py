#!/usr/bin/env python3
"""Weighted k-nearest-neighbour classification with a pre-trained encoder on MI355X: an accuracy without fine-tuning.

    python knn.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --knn_k 20 --knn_t 0.07

Single process, single device, shaped like retrieval.py and reading the same videos: the test list is the queries, the train list
the gallery, a video's feature is the mean of the encoder's pooled feature over the clips of its test plan.  Every query takes the
classes its --knn_k most similar gallery videos vote for, neighbour j weighing exp((sim_j - sim_0) / --knn_t)
(cstp_amd.knn: ops.l2_normalize, ops.sim_topk, ops.knn_vote).  ``kNN top-1 = ...``, ``kNN top-5 = ...`` and a final JSON line go to
the terminal and to knn_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.
--dataset synthetic_video builds --retrieval_gallery_len gallery and --synthetic_len / 4 query videos whose patterns depend on
the class; --dataset UcfFineTune reads UCF-style frame folders (cstp_amd.frame_folder); any other data set is refused.
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import knn, retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import parse_opts


def build_sets(opts):
    """-> (gallery loader, query loader): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts, what="knn")


def run(opts):
    if opts.dataset not in ("synthetic_video", "UcfFineTune"):
        raise NotImplementedError("dataset %r: knn.py serves --dataset synthetic_video and UcfFineTune" % (opts.dataset,))
    if not torch.cuda.is_available():
        raise RuntimeError("knn.py needs a HIP device: cstp_amd has no CPU execution path")
    opts.cuda = True
    opts.distributed = False
    opts.local_rank = 0
    opts.device = torch.device("cuda:0")
    opts.task = "retrieval"          # the model factory's encoder-only task: the pre-training wrapper in eval mode
    print(opts)
    opts.arch = "{}-{}".format(opts.model_name, opts.model_depth)
    gallery_loader, query_loader = build_sets(opts)
    print("Gallery videos = {}, query videos = {}".format(len(gallery_loader), len(query_loader)))
    model = generate_model(opts)
    res = knn.evaluate(model, gallery_loader, query_loader, opts.knn_k, opts.knn_t)
    retrieval.close_video_sets(gallery_loader, query_loader)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "knn_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split, opts.sample_duration)
    summary = {"task": "knn", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split), "n_query": res["n_query"],
               "n_gallery": res["n_gallery"], "feature_dim": res["feature_dim"], "k": res["k"],
               "temperature": res["temperature"], "top1": res["top1"], "top5": res["top5"]}
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        for line in ("kNN top-1 = {:.4f}".format(res["top1"]), "kNN top-5 = {:.4f}".format(res["top5"]), json.dumps(summary)):
            print(line)
            f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
