#!/usr/bin/env python3
"""CSTP fine-tune / train-from-scratch driver for MI355X -- drop-in for the reference's main_ft_mp.py.

    python -m torch.distributed.run --nproc_per_node=8 --master-addr 127.0.0.1 main_ft_mp.py \
        --dataset synthetic --n_classes 101 --batch_size 64 --sample_duration 16 --sample_size 112 \
        --model_name r21d_byol --model_depth 18 --task ft_all --pretrained_path results/synthetic/loss_com/save_300.pth \
        --learning_rate 0.01 --weight_decay 5e-4 --n_epochs 30 --result_path results

What is kept from /root/reference/main_ft_mp.py: seeding (:29-31), env:// process group and rank-0-only printing
(:51-62), train/val loaders with the global batch split over ranks (:75-102, utils.py:91-163), generate_model incl. the
checkpoint handling per task (:106), sgd / adamw(betas 0.9,0.99) / adam (:133-147), ReduceLROnPlateau('min',
patience=--lr_patience) stepped with the epoch's validation loss (:153,279), the train loop (:178-242: forward with
o_type=task, CrossEntropy, accuracy, loss all-reduce for the meter, zero_grad/backward/step, the print columns, the TSV row),
the validation loop under model.eval() + no_grad (:245-310) with the best-accuracy checkpoint ``save_{epoch}_max.pth``
replacing the previous best, and the side-stream host-to-HBM batch overlap (:313-352; cstp_amd.device_batches).
What differs (each a fix of something that cannot work in the reference, none changes the arithmetic):
  * ``--task scratch`` forwards with o_type 'ft_all' (the reference passes o_type='scratch', which R21DBYOL.forward
    rejects, r21d_byol.py:400-401); ``--task resume`` continues an ft_all run (undefined model in the reference);
  * the validation loss is averaged over ranks and EVERY rank steps the plateau scheduler (the reference steps it on
    rank 0 only, :278-279, so after the first reduction the ranks train with different learning rates);
  * --dataset synthetic (class-patterned clips) stands in for the out-of-scope UCF/Kinetics readers; --dataset synthetic_video
    keeps labelled uint8 videos in HBM and runs UcfFineTune's frame selection and the 'img' / 'img_val' transforms on the GPU
    (cstp_amd.sampler + cstp_clip_batch_forward: a whole batch in two launches) in place of the PIL worker pipeline;
    --dataset UcfFineTune feeds the same path from UCF-style frame folders (--frame_dir, --annotation_path, --split;
    --n_workers JPEG decode threads; cstp_amd.frame_folder).
What is added (off by default, then the step is the one above): --label_smoothing, --mixup_alpha, --cutmix_alpha, --mix_prob,
--mix_switch_prob regularise TRAINING with smoothed / mixed targets and blended clips (cstp_amd.mix, cstp_clip_mix,
cstp_soft_cross_entropy_*); training accuracy is then taken against the target that carried the larger weight.  --dropout and
--drop_path add dropout in front of the classifier and stochastic depth on the residual blocks (cstp_amd.regularize, cstp_dropout,
cstp_droppath_add_relu_*), in training forwards only.  --randaug_n / --randaug_m / --randaug_mstd and --random_erase augment the
TRAINING clips of --dataset synthetic_video | UcfFineTune under --transform_mode img with RandAugment and random erasing on the
8-bit frames of the whole batch (cstp_amd.randaug, cstp_randaug_layer / cstp_randaug_finish); validation clips never are.
--layer_decay, --wd_skip_1d, --model_ema, --lr_schedule cosine (--warmup_epochs, --min_lr) are the optimisation half of that recipe
(cstp_amd.recipe): per-tensor learning-rate scales and weight decays in ONE optimiser launch (optim.TableSGD / TableAdam,
cstp_tab_sgd_step / cstp_tab_adam_step), a weight EMA updated in that same launch -- validation, the plateau metric and the best
checkpoint then use the EMA weights, and the checkpoint gains ``state_dict_ema`` beside the unchanged ``state_dict`` -- and a
warm-up + cosine schedule stepped per iteration in place of the plateau scheduler.
"""
from __future__ import annotations

import builtins
import contextlib
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from cstp_amd import ops, randaug, recipe
from cstp_amd.mix import build_mixer
from cstp_amd.model import generate_model
from cstp_amd.regularize import build_regularizer
from cstp_amd.opts import parse_opts
from cstp_amd.device_batches import DeviceBatches
from cstp_amd.synthetic import SyntheticLabelledClips
from cstp_amd.train import FineTuneStep, sync_buffers
from cstp_amd.utils import AverageMeter, Logger, calculate_accuracy, get_dataloader

TRAIN_TASKS = ("ft_fc", "ft_all", "scratch", "resume")


def reduce_mean(tensor, world_size):
    rt = tensor.clone()
    if dist.is_initialized():
        dist.all_reduce(rt, op=dist.ReduceOp.SUM)
    rt /= world_size
    return rt


def build_dataset(opts, data_type, augment=None):
    """``augment``: the randaug.Settings of --randaug_* / --random_erase (None = off); training clips only."""
    if data_type != "train":
        augment = None
    if opts.dataset == "synthetic_video":
        # labelled uint8 videos in HBM; train clips take --transform_mode ('img'), validation '{}_val'.format(mode) (:80,93)
        from cstp_amd.clip_ops import GpuLabelledVideos
        mode = opts.transform_mode if data_type == "train" else "{}_val".format(opts.transform_mode)
        length = opts.synthetic_len if data_type == "train" else max(opts.synthetic_len // 4, 1)
        return GpuLabelledVideos(torch.device("cuda", opts.device), data_type, mode, n_classes=opts.n_classes,
                                 sample_duration=opts.sample_duration, sample_size=opts.sample_size, pb_rate=opts.pb_rate,
                                 length=length, seed=opts.manual_seed,
                                 randaug=None if augment is None else (augment.n, augment.m, augment.mstd),
                                 random_erase=0.0 if augment is None else augment.erase)
    if opts.dataset == "UcfFineTune":
        # frame folders listed under --annotation_path; the same modes, the JPEGs decoded on CPU threads
        from cstp_amd.frame_folder import build_finetune
        mode = opts.transform_mode if data_type == "train" else "{}_val".format(opts.transform_mode)
        return build_finetune(opts, torch.device("cuda", opts.device), data_type, mode, augment=augment)
    if opts.dataset != "synthetic":
        raise NotImplementedError("dataset %r: --dataset synthetic, synthetic_video and UcfFineTune (UCF-style frame folders) are "
                                  "built in (the reference's Kinetics / LMDB readers are outside this package's scope)"
                                  % opts.dataset)
    length = opts.synthetic_len if data_type == "train" else max(opts.synthetic_len // 4, 1)
    return SyntheticLabelledClips(data_type, length, opts.sample_duration, opts.sample_size, opts.n_classes,
                                  opts.manual_seed)


def build_dataloader(dataset, opts, data_type):
    """get_dataloader for the host datasets; the HBM-resident video set brings its own loader (same split of the GLOBAL batch
    over ranks, same shuffle / drop_last rules) whose batches are assembled on the device."""
    if opts.dataset in ("synthetic_video", "UcfFineTune"):
        from cstp_amd.clip_ops import GpuLabelledLoader
        if opts.dataset == "UcfFineTune":
            from cstp_amd.frame_folder import FrameLabelledLoader as GpuLabelledLoader      # + the decode prefetch
        world = opts.world_size if opts.distributed else 1
        loader = GpuLabelledLoader(dataset, max(int(opts.batch_size / world), 1), rank=max(opts.rank, 0) if opts.distributed else 0,
                                   world_size=world, seed=opts.manual_seed)
        return loader, (loader if data_type == "train" else None)
    return get_dataloader(dataset, opts=opts, data_type=data_type)


def o_type_for(task):
    return "ft_all" if task in ("scratch", "resume") else task


def train(epoch, train_dataloader, step_fn, optimizer, opts, train_logger, len_train_data, schedule=None):
    """``schedule``: the per-iteration recipe.WarmupCosine of --lr_schedule cosine (None: the rate changes per epoch at most)."""
    step_fn.model.train()
    batch_time, data_time, losses, accuracies = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    end_time = time.time()
    n_iter = int(len_train_data / opts.batch_size)
    i = 0
    for inputs, targets in DeviceBatches(train_dataloader, opts.device):
        i += 1
        data_time.update(time.time() - end_time)
        if schedule is not None:
            schedule.step()
        loss, outputs = step_fn(inputs, targets)
        acc = calculate_accuracy(outputs, step_fn.accuracy_targets(targets))   # under mixing: the heavier target
        reduced_loss = reduce_mean(loss, opts.world_size)
        losses.update(reduced_loss.item(), inputs.size(0))
        accuracies.update(acc, inputs.size(0))
        batch_time.update(time.time() - end_time)
        end_time = time.time()
        print("Epoch: [{0}][{1}/{2}]\t"
              "Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
              "Data {data_time.val:.3f} ({data_time.avg:.3f})\t"
              "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
              "Acc {acc.val:.3f} ({acc.avg:.3f})\t"
              "Lr {lr:.6f}\t"
              "Left {left:.1f}d".format(epoch, i, n_iter, batch_time=batch_time, data_time=data_time, loss=losses,
                                        acc=accuracies, lr=optimizer.param_groups[-1]["lr"],
                                        left=(batch_time.avg * ((opts.n_epochs - epoch) * n_iter + n_iter - i)) / 3600 / 24))
        if opts.max_steps and i >= opts.max_steps:
            break
    if opts.rank == 0 and opts.local_rank == 0:
        train_logger.log({"epoch": epoch, "loss": losses.avg, "acc": accuracies.avg,
                          "lr": float("{:.5f}".format(optimizer.param_groups[-1]["lr"]))})
    return losses.avg, accuracies.avg


def validation(epoch, val_dataloader, model, optimizer, opts, val_logger, len_val_data, scheduler, ema=False):
    """``scheduler``: the plateau scheduler, or None under --lr_schedule cosine.  ``ema`` (--model_ema): the loop below runs on the EMA
    weights and EMA BatchNorm statistics, so the plateau metric and the best-checkpoint choice are theirs; the checkpoint keeps the
    raw weights under ``state_dict`` and gains ``state_dict_ema`` with the same keys."""
    batch_time, data_time, losses, accuracies = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    o_type = o_type_for(opts.task)
    n_iter = int(len_val_data / opts.batch_size)
    model.eval()     # BatchNorm switches to its running statistics (cstp_bn_forward_eval)
    # DDP(broadcast_buffers=True) hands rank 0's running statistics to every rank at the first eval forward too
    # (models/model.py:97-103): every rank validates -- and rank 0 checkpoints -- the same statistics
    sync_buffers(model)
    state_dict_ema = None
    with (recipe.ema_applied(model.module, optimizer) if ema else contextlib.nullcontext()), torch.no_grad():
        if ema and opts.rank == 0 and opts.local_rank == 0:
            state_dict_ema = {k: v.clone() for k, v in model.state_dict().items()}
        i = 0
        for inputs, targets in DeviceBatches(val_dataloader, opts.device):
            end_time = time.time()
            outputs = model(inputs, o_type=o_type)
            loss = ops.cross_entropy(outputs, targets)
            acc = calculate_accuracy(outputs, targets)
            losses.update(loss.item(), inputs.size(0))
            accuracies.update(acc, inputs.size(0))
            batch_time.update(time.time() - end_time)
            print("Val_Epoch: [{0}][{1}/{2}]\t"
                  "Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
                  "Data {data_time.val:.3f} ({data_time.avg:.3f})\t"
                  "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                  "Acc {acc.val:.3f} ({acc.avg:.3f})".format(epoch, i + 1, n_iter, batch_time=batch_time,
                                                             data_time=data_time, loss=losses, acc=accuracies))
            i += 1
    # every rank sees the same plateau metric and takes the same lr decision (see the module docstring)
    val_loss = losses.avg
    if opts.distributed:
        t = torch.tensor([losses.sum, float(losses.count)], dtype=torch.float64, device=torch.device("cuda", opts.device))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        val_loss = float(t[0] / t[1].clamp(min=1))
    if scheduler is not None:
        scheduler.step(val_loss)
    if opts.rank == 0 and opts.local_rank == 0:
        val_logger.log({"epoch": epoch, "loss": losses.avg, "acc": accuracies.avg})
        accuracy_val = accuracies.avg
        if accuracy_val > list(opts.highest_val.values())[0]:
            old_key = list(opts.highest_val.keys())[0]
            file_path = os.path.join(opts.result_path, opts.dataset, opts.task, old_key)
            if os.path.exists(file_path):
                os.remove(file_path)
            opts.highest_val.pop(old_key)
            opts.highest_val["save_{}_max.pth".format(epoch)] = accuracy_val
            save_file_path = os.path.join(opts.result_path, opts.dataset, opts.task, "save_{}_max.pth".format(epoch))
            checkpoint = {"epoch": epoch + 1, "arch": opts.arch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}
            if ema:
                checkpoint["state_dict_ema"] = state_dict_ema
            torch.save(checkpoint, save_file_path)
    return val_loss, accuracies.avg


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
    if opts.task not in TRAIN_TASKS:
        raise ValueError("main_ft_mp.py serves --task %s, got %r" % ("/".join(TRAIN_TASKS), opts.task))
    regularizer = build_regularizer(opts)        # --dropout / --drop_path: refused here, before any data or model is built
    augment = randaug.from_opts(opts)            # --randaug_* / --random_erase likewise; None at the defaults
    plan = recipe.check_flags(opts)              # --layer_decay / --wd_skip_1d / --model_ema / --lr_schedule ... likewise

    print("Preprocessing train data ...")
    train_data = build_dataset(opts, "train", augment)
    len_train_data = len(train_data)
    print("Length of training data = ", len_train_data)
    train_dataloader, train_sampler = build_dataloader(train_data, opts, "train")
    print("Preprocessing validation data ...")
    val_data = build_dataset(opts, "val")
    len_val_data = len(val_data)
    print("Length of validation data = ", len_val_data)
    val_dataloader, _ = build_dataloader(val_data, opts, "val")

    print("Loading model... ", opts.model_name, opts.model_depth)
    model, parameters = generate_model(opts)
    inner = model.module

    resume = opts.task == "resume"
    begin_epoch = int(opts.resume_md_path.split("/")[-1].split("_")[1]) if resume else 1
    name = "{}_{}_clip{}model{}{}.log"
    train_logger = val_logger = None
    if local_rank == 0:
        train_logger = Logger(os.path.join(log_path, name.format(opts.dataset, "train", opts.sample_duration, opts.model_name,
                                                                 opts.model_depth)),
                              ["epoch", "loss", "acc", "lr"], overlay=not resume)
        val_logger = Logger(os.path.join(log_path, name.format(opts.dataset, "val", opts.sample_duration, opts.model_name,
                                                               opts.model_depth)),
                            ["epoch", "loss", "acc"], overlay=not resume)

    # at the defaults: optim.build_optimizer's FlatSGD / FlatAdam / FlatLARS and the plateau scheduler, as before these flags
    optimizer = recipe.build_optimizer(opts, inner, parameters, inner.flatten_parameters())
    print("Optimizer:", type(optimizer).__name__)
    resume_md = torch.load(opts.resume_md_path, map_location=torch.device("cuda", local_rank)) if resume else None
    if resume:
        optimizer.load_state_dict(resume_md["optimizer"])
    ema = plan.model_ema > 0.0
    if ema:                                      # the shadows start from the loaded weights ...
        optimizer.enable_ema(plan.model_ema)
        if resume and "state_dict_ema" in resume_md:         # ... or continue the checkpoint's
            recipe.load_ema_state_dict(model, inner, optimizer, resume_md["state_dict_ema"])
    resume_md = None
    iters_per_epoch = len(train_dataloader)
    if opts.max_steps:
        iters_per_epoch = min(iters_per_epoch, opts.max_steps)
    scheduler = recipe.build_scheduler(opts, optimizer, iters_per_epoch, begin_epoch)
    cosine = plan.lr_schedule == "cosine"        # stepped per iteration in train(); the plateau scheduler is then not built
    # --label_smoothing / --mixup_alpha / --cutmix_alpha (all tasks served here); None at the defaults.  Training only:
    # validation below keeps the plain cross-entropy, so the plateau scheduler's metric stays comparable between runs
    # --dropout / --drop_path likewise: None at the defaults, training forwards only
    step_fn = FineTuneStep(model, optimizer, o_type_for(opts.task), mixer=build_mixer(opts), regularizer=regularizer)

    for epoch in range(begin_epoch, opts.n_epochs + 1):
        print("Start to fine-tune")
        print("Start training epoch {}".format(epoch))
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        step_fn.set_epoch(epoch)
        train(epoch, train_dataloader, step_fn, optimizer, opts, train_logger, len_train_data, scheduler if cosine else None)
        print("Start validating epoch {}".format(epoch))
        validation(epoch, val_dataloader, model, optimizer, opts, val_logger, len_val_data, None if cosine else scheduler, ema)
    if opts.distributed:
        dist.barrier()
        dist.destroy_process_group()


def main(opts):
    torch.manual_seed(opts.manual_seed)
    np.random.seed(opts.manual_seed)
    random.seed(opts.manual_seed)
    if not torch.cuda.is_available():
        raise RuntimeError("main_ft_mp.py needs a HIP device: cstp_amd has no CPU execution path")
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
