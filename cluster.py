#!/usr/bin/env python3
"""k-means clustering evaluation of a pre-trained encoder on MI355X: the one frozen-feature measurement that forms its answer
without labels.

    python cluster.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --n_finetune_classes 101 --cluster_iters 50 --cluster_restarts 10

Single process, single device, shaped like knn.py and reading the same videos: a video's feature is the mean of the encoder's
pooled feature over the clips of its test plan.  The train list is clustered by spherical k-means into --cluster_k clusters (0 =
--n_finetune_classes), --cluster_restarts restarts side by side for exactly --cluster_iters iterations, the best final score
winning (cstp_amd.cluster: ops.l2_normalize, ops.kmeans_assign, ops.kmeans_update); the test list is assigned to the fitted
centroids.  Both partitions are scored against the labels: ``Cluster NMI = ...``, ``Cluster ARI = ...``, ``Cluster purity = ...``
and ``Cluster acc = ...`` (Hungarian-matched) for train and test and a final JSON line go to the terminal and to
cluster_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.  The seed is --manual_seed.
--dataset synthetic_video builds --retrieval_gallery_len gallery and --synthetic_len / 4 query videos whose patterns depend on
the class; --dataset UcfFineTune reads UCF-style frame folders (cstp_amd.frame_folder); any other data set is refused.
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import cluster, retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import parse_opts


def build_sets(opts):
    """-> (gallery loader, query loader): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts, what="cluster")


def run(opts):
    if opts.dataset not in ("synthetic_video", "UcfFineTune"):
        raise NotImplementedError("dataset %r: cluster.py serves --dataset synthetic_video and UcfFineTune" % (opts.dataset,))
    if opts.transform_mode != "img_test":            # the loaders' own refusal, before any device work
        build_sets(opts)
    if not torch.cuda.is_available():
        raise RuntimeError("cluster.py needs a HIP device: cstp_amd has no CPU execution path")
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
    k = opts.cluster_k if opts.cluster_k > 0 else opts.n_finetune_classes
    res = cluster.evaluate(model, gallery_loader, query_loader, k, opts.cluster_iters, opts.cluster_restarts, opts.manual_seed)
    retrieval.close_video_sets(gallery_loader, query_loader)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "cluster_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split, opts.sample_duration)
    summary = {"task": "cluster", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split)}
    summary.update(res)
    lines = []
    for part in ("train", "test"):
        lines += ["Cluster NMI = {:.4f} ({})".format(res[part + "_nmi"], part), "Cluster ARI = {:.4f} ({})".format(res[part + "_ari"], part),
                  "Cluster purity = {:.4f} ({})".format(res[part + "_purity"], part),
                  "Cluster acc = {:.4f} ({})".format(res[part + "_acc"], part)]
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        for line in lines + [json.dumps(summary)]:
            print(line)
            f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
