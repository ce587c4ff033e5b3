#!/usr/bin/env python3
"""CSTP BYOL pre-training driver for MI355X -- drop-in for the reference's main_byol.py.

Launch exactly like the reference (README.md:41-50), one process per GPU over RCCL:

    python -m torch.distributed.run --nproc_per_node=8 --master-addr 127.0.0.1 main_byol.py \
        --dataset synthetic --batch_size 128 --sample_duration 16 --model_name r21d_byol \
        --model_depth 18 --n_epochs 300 --learning_rate 0.09 --weight_decay 5e-4 --sample_size 112 \
        --task loss_com --optimizer sgd --loss_weight 0.1 1 1 1 1 --result_path results

What is kept from /root/reference/main_byol.py: seeding (:144-146), env:// process group on
--dist_backend (:171-174), rank-0-only printing (:166-169), global --batch_size split over ranks
(utils.py:111), generate_model -> DDP (:211), SGD(momentum, wd) (:228-232), the per-epoch
cosine/warm-up schedule starting at 1e-5 (:252-258,269), the per-step loss composition, clip at 18
and optimiser step (:60-91), the per-iteration print columns (:96-117), the per-epoch TSV row
(:119-130) and the save_{epoch}.pth checkpoint dict every 100 epochs (:132-140).
What differs: --dataset synthetic feeds random clips through a DataLoader; --dataset synthetic_video keeps decoded
uint8 videos in HBM and samples / rotates / crops / resizes / flips / normalises the clip pairs on the GPU
(cstp_amd.sampler + cstp_clip_assemble) in place of the reference's PIL worker pipeline; --dataset UcfRepreBYOLSpPre
reads UCF-style frame folders (--frame_dir, --annotation_path, --split; --n_workers decode threads) and runs everything
after the JPEG decode on the GPU (cstp_amd.frame_folder); the LMDB data sets are out of scope; the log scalars reach the host through one pinned-memory copy per iteration, read one step late
(cstp_amd.train.LaggedScalars), instead of seven .item() syncs and a blocking all-reduce per iteration.
New: --knn_every E (default 0 = off) fills the ``acc`` column of the epoch log, which the reference leaves empty: after every E-th
epoch and after the last one rank 0 classifies labelled test videos by weighted k-NN on the ONLINE encoder (cstp_amd.knn, --knn_k,
--knn_t) under model.eval() + no_grad, the other ranks wait in a barrier, and training goes on unchanged (KnnMonitor).
New: --ntxent_queue K (default 0 = off) gives the NT-Xent term (--ntxent_weight) K extra negatives per row: a FIFO queue of past
online projections, normalised, identical on every rank, not checkpointed (cstp_amd.ntxent, csrc/ntxq.h).
New: --health_every E (default 0 = off) watches for collapse without labels: after every E-th epoch and after the last one rank 0
computes std_ratio, erank, rankme, top1_share, uniformity and nn_sim of the ONLINE encoder's features of the test-list videos
(cstp_amd.health, --health_t), prints ``Health epoch N: ...`` and appends a JSON line to health.jsonl beside the epoch log; the
epoch log and every other output line stay as they are (HealthMonitor).
"""
from __future__ import annotations

import argparse
import builtins
import json
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from cstp_amd import health, knn, retrieval, sampler as clip_sampler
from cstp_amd.model import generate_model
from cstp_amd.ntxent import NTXentLoss
from cstp_amd.optim import build_optimizer
from cstp_amd.opts import health_opts, parse_opts
from cstp_amd.scheduler import CosineAnnealingWarmupRestarts
from cstp_amd.synthetic import SyntheticClips
from cstp_amd.train import LaggedScalars, PretrainStep
from cstp_amd.utils import LOG_COLUMNS, AverageMeter, Logger


def build_dataset(opts):
    if opts.dataset == "synthetic_video":
        from cstp_amd.clip_ops import GpuVideoClips
        return GpuVideoClips(torch.device("cuda", opts.local_rank), sample_duration=opts.sample_duration,
                             sample_size=opts.sample_size, length=opts.synthetic_len, seed=opts.manual_seed)
    if opts.dataset == "UcfRepreBYOLSpPre":
        # frame folders listed under --annotation_path: JPEGs decoded on CPU threads, everything after the decode on the GPU
        from cstp_amd.frame_folder import build_pretrain
        return build_pretrain(opts, torch.device("cuda", opts.local_rank))
    if opts.dataset != "synthetic":
        raise NotImplementedError("dataset %r: --dataset synthetic, synthetic_video and UcfRepreBYOLSpPre (UCF-style frame "
                                  "folders) are built in; the reference's LMDB data sets are outside this package's scope"
                                  % opts.dataset)
    return SyntheticClips(opts.synthetic_len, opts.sample_duration, opts.sample_size, opts.manual_seed)


def check_knn_opts(opts):
    """Refuses what the --knn_every monitor cannot serve; called before any device work.  0 = off: nothing to check."""
    every = getattr(opts, "knn_every", 0)
    if every < 0:
        raise ValueError("--knn_every takes 0 (off) or a positive number of epochs, got %d" % every)
    if every == 0:
        return
    if opts.dataset not in KnnMonitor.SETS:
        raise ValueError("--knn_every %d with --dataset %s: the k-NN monitor needs labelled videos, which --dataset "
                         "synthetic_video and UcfRepreBYOLSpPre have (--dataset synthetic is unlabelled random clips)"
                         % (every, opts.dataset))
    try:
        clip_sampler.short_side(opts.sample_size)
    except ValueError:
        raise ValueError("--knn_every %d with --sample_size %d: the monitor reads whole videos as the video test does, and its "
                         "ClipScale serves --sample_size 112 and 224 only" % (every, opts.sample_size)) from None


def check_health_opts(opts):
    """Refuses what the --health_every monitor cannot serve -- what check_knn_opts refuses: it reads the same whole-video sets;
    called before any device work.  0 = off: nothing to check."""
    every, _ = health_opts(opts)
    if every < 0:
        raise ValueError("--health_every takes 0 (off) or a positive number of epochs, got %d" % every)
    if every == 0:
        return
    if opts.dataset not in KnnMonitor.SETS:
        raise ValueError("--health_every %d with --dataset %s: the health monitor reads the whole test-list videos of --dataset "
                         "synthetic_video and UcfRepreBYOLSpPre, the labelled sets of the k-NN monitor (their labels are "
                         "ignored; --dataset synthetic is random clips without videos)" % (every, opts.dataset))
    try:
        clip_sampler.short_side(opts.sample_size)
    except ValueError:
        raise ValueError("--health_every %d with --sample_size %d: the monitor reads whole videos as the video test does, and "
                         "its ClipScale serves --sample_size 112 and 224 only" % (every, opts.sample_size)) from None


def check_ntxent_queue_opts(opts):
    """Refuses a --ntxent_queue the NT-Xent term cannot use; called before any device work.  0 = off: nothing to check."""
    k = getattr(opts, "ntxent_queue", 0)
    if k < 0:
        raise ValueError("--ntxent_queue takes 0 (off) or a positive number of rows, got %d" % k)
    if k > 0 and opts.ntxent_weight == 0.0:
        raise ValueError("--ntxent_queue %d with --ntxent_weight 0: the queue feeds a term that is switched off" % k)
    if k % (2 * opts.batch_size) != 0:
        raise ValueError("--ntxent_queue %d must be a multiple of 2 * batch_size = %d: a step pushes that many rows and a push "
                         "never wraps" % (k, 2 * opts.batch_size))


class KnnMonitor:
    """--knn_every: ``monitor(epoch)`` -> the k-NN top-1 of the online encoder after every E-th epoch and after the last, else
    None.  Rank 0 evaluates (cstp_amd.knn.evaluate: eval mode, no_grad, the mode restored) and prints; under DDP every rank then
    meets in a barrier, so the evaluation has to finish inside the collective timeout.  The evaluation draws from no random
    generator and updates no buffer: the training that follows is the training without it."""

    # the pre-training data set -> the labelled whole-video sets of the same flags (retrieval.build_video_sets)
    SETS = {"synthetic_video": "synthetic_video", "UcfRepreBYOLSpPre": "UcfFineTune"}

    def __init__(self, opts, model, local_rank):
        check_knn_opts(opts)
        self.every, self.last, self.k, self.t = opts.knn_every, opts.n_epochs, opts.knn_k, opts.knn_t
        self.model, self.distributed, self.loaders = model, opts.distributed, None
        if max(opts.rank, 0) == 0:
            sets_opts = argparse.Namespace(**vars(opts))
            sets_opts.device = torch.device("cuda", local_rank)
            self.loaders = retrieval.build_video_sets(sets_opts, self.SETS[opts.dataset])
            print("kNN monitor: {} gallery videos, {} query videos, k = {}, T = {}".format(
                len(self.loaders[0]), len(self.loaders[1]), self.k, self.t))

    def __call__(self, epoch):
        if epoch % self.every != 0 and epoch != self.last:
            return None
        top1 = None
        if self.loaders is not None:
            res = knn.evaluate(self.model, self.loaders[0], self.loaders[1], self.k, self.t)
            print("Epoch {}: kNN top-1 = {:.4f}".format(epoch, res["top1"]))
            print("Epoch {}: kNN top-5 = {:.4f}".format(epoch, res["top5"]))
            top1 = res["top1"]
        if self.distributed:
            dist.barrier()
        return top1

    def close(self):
        if self.loaders is not None:
            retrieval.close_video_sets(*self.loaders)


class HealthMonitor:
    """--health_every: ``monitor(epoch)`` after every E-th epoch and after the last.  Rank 0 computes the label-free collapse
    metrics of the online encoder on the test-list videos (cstp_amd.health.evaluate: eval mode, no_grad, the mode restored),
    prints ``Health epoch N: ...`` and appends the JSON line to ``path``; under DDP every rank then meets in a barrier.  It
    extracts its own features also where KnnMonitor fires in the same epoch.  Like that monitor it draws from no random generator
    and updates no buffer."""

    def __init__(self, opts, model, local_rank, path):
        check_health_opts(opts)
        self.every, self.t = health_opts(opts)
        self.last, self.model, self.distributed, self.loader, self.path = opts.n_epochs, model, opts.distributed, None, path
        if max(opts.rank, 0) == 0:
            sets_opts = argparse.Namespace(**vars(opts))
            sets_opts.device = torch.device("cuda", local_rank)
            train_list, self.loader = retrieval.build_video_sets(sets_opts, KnnMonitor.SETS[opts.dataset])
            retrieval.close_video_sets(train_list)          # only the test list is watched
            del train_list
            print("Health monitor: {} videos, t = {}".format(len(self.loader), self.t))

    def __call__(self, epoch):
        if epoch % self.every != 0 and epoch != self.last:
            return None
        res = None
        if self.loader is not None:
            res = dict(health.evaluate(self.model, self.loader, self.t), epoch=epoch)
            print("Health epoch {}: {}".format(epoch, health.format_line(res)))
            with open(self.path, "a") as f:
                f.write(json.dumps(res) + "\n")
        if self.distributed:
            dist.barrier()
        return res

    def close(self):
        if self.loader is not None:
            retrieval.close_video_sets(self.loader)


def train_BYOL(epoch, loader, step_fn, optimizer, opts, train_logger, knn_monitor=None, health_monitor=None):
    meters = {k: AverageMeter() for k in ("batch", "data", "loss", "loss_byol", "loss_pred_spa", "loss_pred_tem",
                                          "loss_pred_pb", "loss_pred_rot")}
    dev = torch.device("cuda", opts.local_rank)
    # The log scalars (and the rank-mean of the total loss, main_byol.py:22-26,75) lag ONE step behind the launches: no
    # host sync and no blocking collective between two steps; the columns are the reference's.
    lagged = LaggedScalars(dev, opts.world_size)

    def log_line(rec):
        (it, n, t_batch, t_data), host = rec
        for k in LaggedScalars.KEYS:
            meters[k].update(host[k], n)
        meters["batch"].update(t_batch)
        meters["data"].update(t_data)
        m = meters
        print("Epoch: [{0}][{1}/{2}]\tTime {3:.3f} ({4:.3f})\tData {5:.3f} ({6:.3f})\t"
              "Loss_byol {7:.4f} ({8:.4f})\tLoss_pred_spa {9:.4f} ({10:.4f})\tLoss_pred_tem {11:.4f} ({12:.4f})\t"
              "Loss_pred_pb {13:.4f} ({14:.4f})\tLoss_pred_rot {15:4f} ({16:.4f})Loss_total {17:.4f} ({18:.4f})\t"
              "Lr {19:.4}".format(epoch, it, len(loader), m["batch"].val, m["batch"].avg, m["data"].val, m["data"].avg,
                                  m["loss_byol"].val, m["loss_byol"].avg, m["loss_pred_spa"].val, m["loss_pred_spa"].avg,
                                  m["loss_pred_tem"].val, m["loss_pred_tem"].avg, m["loss_pred_pb"].val,
                                  m["loss_pred_pb"].avg, m["loss_pred_rot"].val, m["loss_pred_rot"].avg, m["loss"].val,
                                  m["loss"].avg, optimizer.param_groups[-1]["lr"]))

    end = time.time()
    for i, (inputs, targets) in enumerate(loader):
        if opts.max_steps and i >= opts.max_steps:
            break
        t_data = time.time() - end
        clip_1 = inputs[0].to(dev, non_blocking=True)
        clip_2 = inputs[1].to(dev, non_blocking=True)
        spa, tem, pb = (targets[j].to(dev, non_blocking=True) for j in range(3))
        rot_1, rot_2 = targets[3][0].to(dev, non_blocking=True), targets[3][1].to(dev, non_blocking=True)
        out = step_fn(clip_1, clip_2, spa, tem, pb, rot_1, rot_2)
        t_batch = time.time() - end
        end = time.time()
        prev = lagged.push(out, (i + 1, clip_1.size(0), t_batch, t_data))
        if prev is not None:
            log_line(prev)
    last = lagged.flush()
    if last is not None:
        log_line(last)
    acc = knn_monitor(epoch) if knn_monitor is not None else None      # every rank calls it: it ends in a barrier under DDP
    if health_monitor is not None:
        health_monitor(epoch)
    if opts.local_rank == 0:
        row = {k: meters[k].avg for k in LOG_COLUMNS if k in meters}
        row.update({"epoch": epoch, "acc": acc, "lr": float("{:.5f}".format(optimizer.param_groups[-1]["lr"]))})
        train_logger.log(row)
        if opts.rank == 0 and epoch % 100 == 0:     # rank 0 writes its own state: what DDP's broadcast hands every rank
            path = os.path.join(opts.result_path, opts.dataset, opts.task, "save_{}.pth".format(epoch))
            torch.save({"epoch": epoch + 1, "arch": opts.arch, "state_dict": step_fn.model.state_dict(),
                        "optimizer": optimizer.state_dict()}, path)


def main_worker(local_rank, opts):
    opts.device = local_rank
    if opts.distributed:
        if local_rank != 0:
            builtins.print = lambda *a, **k: None   # only the master prints
        opts.rank = local_rank                      # single-node assumption, as in the reference
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=opts.dist_backend, init_method=opts.dist_url, world_size=opts.world_size,
                                rank=opts.rank)
    log_path = os.path.join(opts.result_path, opts.dataset, opts.task)
    if local_rank == 0:
        os.makedirs(log_path, exist_ok=True)
    print(opts)
    opts.arch = "{}-{}".format(opts.model_name, opts.model_depth)

    check_ntxent_queue_opts(opts)
    criterion_ctr = NTXentLoss(device=local_rank, batch_size=opts.batch_size, temperature=opts.temperature,
                               use_cosine_similarity=True, queue_size=getattr(opts, "ntxent_queue", 0))
    train_data = build_dataset(opts)
    print("Length of training data = ", len(train_data))
    per_rank = int(opts.batch_size / opts.world_size)
    if opts.dataset == "synthetic_video":
        from cstp_amd.clip_ops import GpuClipLoader
        loader = sampler = GpuClipLoader(train_data, per_rank, rank=max(opts.rank, 0), world_size=opts.world_size,
                                         seed=opts.manual_seed)
    elif opts.dataset == "UcfRepreBYOLSpPre":
        from cstp_amd.frame_folder import FramePairLoader
        loader = sampler = FramePairLoader(train_data, per_rank, rank=max(opts.rank, 0), world_size=opts.world_size,
                                           seed=opts.manual_seed)
    else:
        sampler = DistributedSampler(train_data, num_replicas=opts.world_size, rank=max(opts.rank, 0), shuffle=True) \
            if opts.distributed else None
        loader = DataLoader(train_data, batch_size=per_rank, shuffle=sampler is None, num_workers=opts.n_workers,
                            pin_memory=True, sampler=sampler, drop_last=True)

    print("Loading model... ", opts.model_name, opts.model_depth)
    model, parameters = generate_model(opts)
    print("Model is loaded successfully!")
    inner = model.module if hasattr(model, "module") else model
    train_logger = Logger(os.path.join(log_path, "{}_train_clip{}model{}{}.log".format(
        opts.dataset, opts.sample_duration, opts.model_name, opts.model_depth)), LOG_COLUMNS,
        overlay=not opts.resume_md_path) \
        if local_rank == 0 else None

    optimizer = build_optimizer(opts, parameters, inner.flatten_parameters())   # sgd | adamw | adam (main_byol.py:227-244) | lars
    begin_epoch = 1
    if opts.resume_md_path:
        # The reference only reloads the optimizer for --task resume and then trains nothing (main_byol.py:246-247,
        # 260).  Here --resume_md_path continues a loss_com run: weights (online, target, heads, BN buffers), momentum
        # buffers, the epoch counter (checkpoints store epoch + 1) and the schedule position.
        md = torch.load(opts.resume_md_path, map_location=torch.device("cuda", local_rank))
        assert opts.arch == md["arch"]
        model.load_state_dict(md["state_dict"])
        optimizer.load_state_dict(md["optimizer"])
        begin_epoch = int(md["epoch"])
        print("Resume model {} at epoch {}".format(opts.resume_md_path, begin_epoch))
    scheduler = CosineAnnealingWarmupRestarts(optimizer, first_cycle_steps=opts.n_epochs, cycle_mult=1.0,
                                              max_lr=opts.learning_rate, min_lr=0.00001,
                                              warmup_steps=0.5 * opts.n_epochs, gamma=0.5)
    for _ in range(1, begin_epoch):
        scheduler.step()
    step_fn = PretrainStep(model, optimizer, opts.loss_weight, task=opts.task, clip_grad_norm=opts.clip_grad_norm,
                           ntxent=criterion_ctr, ntxent_weight=opts.ntxent_weight)
    knn_monitor = KnnMonitor(opts, model, local_rank) if getattr(opts, "knn_every", 0) > 0 else None
    health_monitor = HealthMonitor(opts, model, local_rank, os.path.join(log_path, "health.jsonl")) \
        if health_opts(opts)[0] > 0 else None
    if opts.task in ("r_byol", "loss_com"):
        print("Start to train BYOL CoCLR data augmentation pre-trained model!")
        for epoch in range(begin_epoch, opts.n_epochs + 1):
            print("Training BYOL at epoch {}".format(epoch))
            if sampler is not None:
                sampler.set_epoch(epoch)
            model.train()
            train_BYOL(epoch, loader, step_fn, optimizer, opts, train_logger, knn_monitor, health_monitor)
            scheduler.step()
    if knn_monitor is not None:
        knn_monitor.close()
    if health_monitor is not None:
        health_monitor.close()
    if opts.distributed:
        dist.barrier()
        dist.destroy_process_group()


def main(opts):
    check_knn_opts(opts)
    check_health_opts(opts)
    check_ntxent_queue_opts(opts)
    torch.manual_seed(opts.manual_seed)
    np.random.seed(opts.manual_seed)
    random.seed(opts.manual_seed)
    if not torch.cuda.is_available():
        raise NotImplementedError("Only DistributedDataParallel on HIP devices is supported.")
    opts.cuda = True
    if opts.local_rank != -1:
        opts.world_size = int(os.environ["WORLD_SIZE"])
        opts.distributed = True
        opts.nprocs = torch.cuda.device_count()
        main_worker(opts.local_rank, opts)
    else:
        opts.distributed = False
        opts.world_size = 1
        opts.local_rank = 0
        opts.rank = 0
        main_worker(0, opts)


if __name__ == "__main__":
    main(parse_opts())
