#!/usr/bin/env python3
"""Linear-probe evaluation of a pre-trained encoder on MI355X: a linear classifier trained on frozen, cached features.

    python linear_probe.py --dataset UcfFineTune --transform_mode img_test --frame_dir ... --annotation_path ... --split 1 \
        --model_name r21d_byol --model_depth 18 --pretrained_path results/.../save_200.pth --result_path results \
        --sample_duration 16 --sample_size 112 --n_finetune_classes 101 --probe_epochs 100 --probe_batch 1024 --probe_lr 1e-3

Single process, single device, shaped like knn.py and reading the same videos: the train list is the training set of the
classifier, the test list is scored; a video's feature is the mean of the encoder's pooled feature over the clips of its test plan,
extracted once.  The classifier (--n_finetune_classes outputs, from zero) is trained on the standardised features for
--probe_epochs passes with --probe_optimizer and a cosine learning rate from --probe_lr (cstp_amd.probe: ops.probe_step, the
flat-arena optimizer kernels, ops.probe_predict).  ``Linear probe top-1 = ...``, ``Linear probe top-5 = ...`` and a final JSON line
go to the terminal and to probe_{model}{depth}_{dataset}_{split}_{T}.txt under result_path/dataset/.
With --probe_lrs (and optionally --probe_wds, --probe_val_fraction) the learning rate and weight decay are selected first: the
grid is trained side by side on a stratified part of the train list and scored on the held-out rest (cstp_amd.probe.sweep), one
``Probe sweep lr = ..`` line per grid point and a ``Probe sweep selected lr = .., wd = ..`` line are printed, the selected point is
refitted on the whole train list by the same single-classifier path, and the JSON line gains sweep, selected_lr, selected_wd,
val_fraction and n_val.  The test list takes no part in the selection.
--dataset synthetic_video builds --retrieval_gallery_len gallery and --synthetic_len / 4 query videos whose patterns depend on
the class; --dataset UcfFineTune reads UCF-style frame folders (cstp_amd.frame_folder); any other data set is refused.
"""
from __future__ import annotations

import json
import os

import torch

from cstp_amd import probe, retrieval
from cstp_amd.model import generate_model
from cstp_amd.opts import parse_opts, probe_grid


def build_sets(opts):
    """-> (gallery loader, query loader): one whole video per item, as the video test reads them."""
    return retrieval.build_video_sets(opts, what="linear_probe")


def run(opts):
    if opts.dataset not in ("synthetic_video", "UcfFineTune"):
        raise NotImplementedError("dataset %r: linear_probe.py serves --dataset synthetic_video and UcfFineTune" % (opts.dataset,))
    if opts.transform_mode != "img_test":
        build_sets(opts)                 # raises the loaders' own refusal of other transform modes, before any device work
    grid = probe_grid(opts)
    sweep_args = {}
    if grid is not None:
        probe.grid_points(grid[0], grid[1])      # the refusals of a hand-built namespace, before any device work
        sweep_args = dict(lrs=grid[0], wds=grid[1], val_fraction=grid[2])
    if not torch.cuda.is_available():
        raise RuntimeError("linear_probe.py needs a HIP device: cstp_amd has no CPU execution path")
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
    res = probe.evaluate(model, gallery_loader, query_loader, opts.n_finetune_classes, epochs=opts.probe_epochs,
                         batch=opts.probe_batch, lr=opts.probe_lr, weight_decay=opts.probe_wd, optimizer=opts.probe_optimizer,
                         seed=opts.manual_seed, **sweep_args)
    retrieval.close_video_sets(gallery_loader, query_loader)
    result_path = "{}/{}/".format(opts.result_path, opts.dataset)
    os.makedirs(result_path, exist_ok=True)
    out_name = "probe_{}{}_{}_{}_{}.txt".format(opts.model_name, opts.model_depth, opts.dataset, opts.split, opts.sample_duration)
    summary = {"task": "linear_probe", "arch": opts.arch, "dataset": opts.dataset, "split": str(opts.split)}
    summary.update(res)
    with open(os.path.join(result_path, out_name), "w+") as f:
        f.write(str(opts) + "\n")
        lines = []
        if grid is not None:
            lines = ["Probe sweep lr = {:g}, wd = {:g}: val top-1 = {:.4f}, val loss = {:.4f}, last-epoch train loss = {:.4f}".format(
                p["lr"], p["wd"], p["val_top1"], p["val_loss"], p["last_epoch_loss"]) for p in res["sweep"]]
            lines.append("Probe sweep selected lr = {:g}, wd = {:g}".format(res["selected_lr"], res["selected_wd"]))
        for line in lines + ["Linear probe top-1 = {:.4f}".format(res["top1"]), "Linear probe top-5 = {:.4f}".format(res["top5"]),
                     json.dumps(summary)]:
            print(line)
            f.write(line + "\n")
    return summary


if __name__ == "__main__":
    run(parse_opts())
