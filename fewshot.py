#!/usr/bin/env python3
"""Few-shot episodic evaluation of a pre-trained encoder on MI355X: N-way K-shot accuracy without fine-tuning.

    python fewshot.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --fewshot_way 5 --fewshot_shot 1 5 --fewshot_query 15 --fewshot_episodes 10000

Single process, single device, shaped like knn.py and reading the same videos: a video's feature is the mean of the encoder's
pooled feature over the clips of its test plan.  An episode draws --fewshot_way classes, for each the support videos from the
TRAIN list and --fewshot_query query videos from the TEST list; a query takes the class of the most similar prototype by cosine,
the K-shot prototype being the sum of the class's first K support features, so the shot counts of --fewshot_shot are paired on
the same episodes (cstp_amd.fewshot: ops.l2_normalize, ops.fewshot_episodes -- one launch for all episodes).  One
``Few-shot N-way K-shot: acc ± ci95 (E episodes)`` line per shot count and a final JSON line go to the terminal and to
fewshot_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.  Classes with fewer than max(--fewshot_shot) train
videos or --fewshot_query test videos are left out, with a line that counts them.
--dataset synthetic_video builds --retrieval_gallery_len "train" and --synthetic_len / 4 "test" videos whose patterns depend on
the class; --dataset UcfFineTune reads UCF-style frame folders (cstp_amd.frame_folder); any other data set is refused.
The defaults are the literature's conventions (5-way, 1- and 5-shot, 15 queries, 10 000 episodes, mean ± 95 % confidence interval).
They are not tuned, and no few-shot accuracy of a trained encoder on real data has been measured with this code.
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import fewshot, retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import fewshot_opts, parse_opts


def build_sets(opts):
    """-> (support loader: the train list, query loader: the test list): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts, what="fewshot")


def run(opts):
    if opts.dataset not in ("synthetic_video", "UcfFineTune"):
        raise NotImplementedError("dataset %r: fewshot.py serves --dataset synthetic_video and UcfFineTune" % (opts.dataset,))
    if not torch.cuda.is_available():
        raise RuntimeError("fewshot.py needs a HIP device: cstp_amd has no CPU execution path")
    opts.cuda = True
    opts.distributed = False
    opts.local_rank = 0
    opts.device = torch.device("cuda:0")
    opts.task = "retrieval"          # the model factory's encoder-only task: the pre-training wrapper in eval mode
    print(opts)
    opts.arch = "{}-{}".format(opts.model_name, opts.model_depth)
    way, shots, query, episodes, seed = fewshot_opts(opts)
    support_loader, query_loader = build_sets(opts)
    print("Support videos = {}, query videos = {}".format(len(support_loader), len(query_loader)))
    model = generate_model(opts)
    res = fewshot.evaluate(model, support_loader, query_loader, way, shots, query, episodes, seed)
    retrieval.close_video_sets(support_loader, query_loader)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "fewshot_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split, opts.sample_duration)
    summary = {"task": "fewshot", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split), "n_way": res["n_way"],
               "shots": res["shots"], "n_query": res["n_query"], "episodes": res["episodes"], "seed": res["seed"],
               "n_support": res["n_support"], "n_queries": res["n_queries"], "feature_dim": res["feature_dim"],
               "acc": {str(k): v for k, v in res["acc"].items()}, "ci95": {str(k): v for k, v in res["ci95"].items()}}
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        for line in [fewshot.format_line(res, k) for k in res["shots"]] + [json.dumps(summary)]:
            print(line)
            f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
