#!/usr/bin/env python3
"""Nearest-neighbour video retrieval with a pre-trained encoder on MI355X: no fine-tuning, minutes instead of hours.

    python retrieval.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --retrieval_k 1 5 10 20 50

Single process, single device, shaped like test.py.  The videos of the test list are the queries, the videos of the train list
the gallery; every video is cut into the clips of its test plan, a video's feature is the mean of the encoder's pooled feature
over them (cstp_amd.retrieval.extract_features), the features are L2-normalised and ops.sim_topk finds each query's nearest
gallery videos.  One line per k and a final JSON line go to the terminal and to
retrieval_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.
--dataset synthetic_video builds --retrieval_gallery_len gallery and --synthetic_len / 4 query videos whose patterns depend on
the class; --dataset UcfFineTune reads UCF-style frame folders (cstp_amd.frame_folder).
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import parse_opts


def build_sets(opts):
    """-> (gallery loader, query loader): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts)


def run(opts):
    if not torch.cuda.is_available():
        raise RuntimeError("retrieval.py needs a HIP device: cstp_amd has no CPU execution path")
    opts.cuda = True
    opts.distributed = False
    opts.local_rank = 0
    opts.device = torch.device("cuda:0")
    opts.task = "retrieval"
    print(opts)
    opts.arch = "{}-{}".format(opts.model_name, opts.model_depth)
    ks = sorted(set(opts.retrieval_k))
    gallery_loader, query_loader = build_sets(opts)
    print("Gallery videos = {}, query videos = {}".format(len(gallery_loader), len(query_loader)))
    model = generate_model(opts)
    g_feat, g_labels = retrieval.extract_features(model, gallery_loader)
    q_feat, q_labels = retrieval.extract_features(model, query_loader)
    for loader in (gallery_loader, query_loader):
        close = getattr(loader.dataset, "close", None)
        if close is not None:
            close()
    recall, _, _, _, _ = retrieval.retrieve(q_feat, q_labels, g_feat, g_labels, ks)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "retrieval_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split,
                                                    opts.sample_duration)
    summary = {"task": "retrieval", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split),
               "n_query": int(q_feat.shape[0]), "n_gallery": int(g_feat.shape[0]), "feature_dim": int(q_feat.shape[1]),
               "recall": {str(k): recall[k] for k in ks}}
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        for k in ks:
            line = "R@{} = {:.4f}".format(k, recall[k])
            print(line)
            f.write(line + "\n")
        line = json.dumps(summary)
        print(line)
        f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
