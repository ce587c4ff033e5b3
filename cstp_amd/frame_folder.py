"""UCF-style frame folders as a data source of the GPU clip pipeline: ``--dataset UcfRepreBYOLSpPre`` (pre-training pairs,
reference data_process/datasets.py:812-948) and ``--dataset UcfFineTune`` (fine-tune / validation / video test, :951-1097).

What the reference does per sample in a DataLoader worker -- Image.open of every frame of a clip, then the PIL transform chain --
is split here: the host decides (cstp_amd.sampler: a plan per sample, a pure function of (seed, epoch, index) and the video's
length and frame size), CPU threads decode with Pillow (the reference's decoder, hence the parity definition; it releases the GIL
while decoding), and everything after the decode runs on the GPU (cstp_amd.clip_ops.assemble_pairs / assemble_batch), bit for
bit what the PIL chain gives on the same decoded frames.

Per batch the frames that its clips name are decoded ONCE each -- the union of (video, frame) over all clips: the two clips of
a pair overlap in time more often than not -- into one pinned uint8 arena, uploaded with one asynchronous copy, and every sample
gets a ``[n_unique, h, w, 3]`` view of the device arena with its plan's frame indices remapped to positions in that view.

Prefetch: while step k runs, batch k + 1 is being decoded.  The rules that keep that safe:
  * worker threads do host work only (file read, JPEG decode, a memcpy into pinned memory) and make no HIP call;
  * the main thread enqueues the copy on a side stream;
  * a pinned arena is decoded into again only after the event behind its last copy has completed;
  * a device arena is overwritten only after the assembly kernels that read it: the copy stream waits on the event recorded
    behind them;
  * there are two arenas of each kind, used in turn, and they only grow.
"""
from __future__ import annotations

import dataclasses
import os
import random
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import sampler
from . import randaug as randaug_draws
from .clip_ops import GpuClipLoader, GpuLabelledLoader, assemble_batch, assemble_pairs, augment_settings

MAX_DECODE_THREADS = 16


class FrameError(RuntimeError):
    """A frame file that is missing, unreadable or of another size than its video's first planned frame."""


# ---- lists and paths ---------------------------------------------------------------------------------------------------------
def list_name(data_type: str, split) -> str:
    """'train' reads trainlist0{split}_nframe.txt, 'val' and 'test' testlist0{split}_nframe.txt (datasets.py:827-830)."""
    if data_type not in ("train", "val", "test"):
        raise ValueError("data_type %r" % (data_type,))
    return ("trainlist0{}_nframe.txt" if data_type == "train" else "testlist0{}_nframe.txt").format(split)


def read_list(annotation_path: str, frame_dir: str, data_type: str, split) -> List[Tuple[str, int, int]]:
    """-> [(video folder, label, n_frames)] in file order.  Lines are ``Class/v_name.avi <label> <n_frames>``; the folder is
    frame_dir/<first field up to its first '.'>; n_frames comes from the list; a folder that does not exist is reported and
    skipped (datasets.py:831-840, 970-979)."""
    data = []
    with open(os.path.join(annotation_path, list_name(data_type, split)), "r") as f:
        for line in f:
            fields = line.strip().split(" ")
            if len(fields) < 3:
                continue
            folder = os.path.join(frame_dir, fields[0].split(".")[0])
            if os.path.exists(folder):
                data.append((folder, int(fields[1]), int(fields[2])))
            else:
                print("{} does not exist".format(folder))
    return data


def frame_path(folder: str, index: int) -> str:
    """File of the 0-based frame ``index``: frames are '%05d.jpg', 1-based."""
    return os.path.join(folder, "%05d.jpg" % (index + 1))


def frame_size(path: str) -> Tuple[int, int]:
    """(width, height) from the JPEG header: Image.open is lazy, nothing is decoded."""
    try:
        with Image.open(path) as im:
            return im.size
    except OSError as e:
        raise FrameError("cannot read frame %s: %s" % (path, e)) from e


def union_remap(clips: Sequence[Sequence[int]]):
    """The frames a sample's clips name, each once: -> (sorted unique frame indices, the clips with every index replaced by its
    position in that list)."""
    unique = sorted({int(i) for c in clips for i in c})
    pos = {f: k for k, f in enumerate(unique)}
    return unique, [[pos[int(i)] for i in c] for c in clips]


def decode_into(path: str, dst: np.ndarray) -> None:
    """One frame through Pillow into dst (uint8 [h][w][3]).  Host work only: runs on the decode threads."""
    try:
        with Image.open(path) as im:
            if im.mode != "RGB":
                im = im.convert("RGB")
            if (im.size[1], im.size[0]) != dst.shape[:2]:
                raise FrameError("frame %s is %d x %d, its video's first planned frame %d x %d"
                                 % (path, im.size[0], im.size[1], dst.shape[1], dst.shape[0]))
            dst[...] = np.asarray(im)
    except OSError as e:                                     # FileNotFoundError, truncated or broken JPEG
        raise FrameError("cannot read frame %s: %s" % (path, e)) from e


def decode_threads(n_workers: int) -> int:
    """--n_workers decode threads, at least one, never more than 16 (and never sized by the machine's CPU count)."""
    return max(1, min(int(n_workers), MAX_DECODE_THREADS))


# ---- staging: decode -> pinned arena -> device arena ---------------------------------------------------------------------------
class _Ticket:
    def __init__(self, slot, total, layout, futures):
        self.slot, self.total, self.layout, self.futures = slot, total, layout, futures


class FrameStager:
    """Two pinned and two device arenas used in turn.  ``begin`` hands the decode jobs of one batch to the thread pool and
    returns at once; ``finish`` waits for them, enqueues the one upload on the side stream and returns the per-sample device
    views; ``release`` marks the point behind the kernels that read them."""

    def __init__(self, device, threads: int):
        self.device = torch.device(device)
        self.threads = threads
        self.pool = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="cstp-decode")
        self.pinned, self.dev = [None, None], [None, None]
        self.copied, self.consumed = [None, None], [None, None]      # events: behind the last copy / the last reading kernels
        self.copy_stream = None
        self.turn = 0

    def begin(self, samples) -> _Ticket:
        """samples: [(paths, h, w)].  Main thread; the only wait is for the copy that last read this slot's pinned arena."""
        slot = self.turn
        self.turn ^= 1
        total = sum(len(paths) * h * w * 3 for paths, h, w in samples)
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()
        if self.pinned[slot] is None or self.pinned[slot].numel() < total:
            self.pinned[slot] = torch.empty(_grown(total), dtype=torch.uint8, pin_memory=True)
        host = self.pinned[slot].numpy()
        layout, futures, off = [], [], 0
        for paths, h, w in samples:
            layout.append((off, len(paths), h, w))
            for path in paths:
                futures.append(self.pool.submit(decode_into, path, host[off:off + h * w * 3].reshape(h, w, 3)))
                off += h * w * 3
        return _Ticket(slot, total, layout, futures)

    @staticmethod
    def wait(ticket: _Ticket) -> None:
        """Every job of the ticket has ended when this returns or raises (nothing still writes into the arena)."""
        first = None
        for f in ticket.futures:
            try:
                f.result()
            except Exception as e:          # noqa: BLE001 -- kept, re-raised below once every job has ended
                first = first or e
        if first is not None:
            raise first

    def finish(self, ticket: _Ticket) -> List[torch.Tensor]:
        self.wait(ticket)
        slot, total = ticket.slot, ticket.total
        consumer = torch.cuda.current_stream(self.device)
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(device=self.device)
        cs = self.copy_stream
        if self.dev[slot] is None or self.dev[slot].numel() < total:
            new = torch.empty(_grown(total), dtype=torch.uint8, device=self.device)
            new.record_stream(cs)           # written on the copy stream: the allocator must not recycle it under that copy
            born = torch.cuda.Event()
            born.record(consumer)           # ... nor may the copy overtake what last used this memory on the consumer stream
            cs.wait_event(born)
            self.dev[slot] = new
        elif self.consumed[slot] is not None:
            cs.wait_event(self.consumed[slot])
        arena = self.dev[slot]
        with torch.cuda.stream(cs):
            arena[:total].copy_(self.pinned[slot][:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        self.copied[slot] = ev
        consumer.wait_event(ev)
        arena.record_stream(consumer)
        return [arena[off:off + n * h * w * 3].view(n, h, w, 3) for off, n, h, w in ticket.layout]

    def release(self, ticket: _Ticket) -> None:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.consumed[ticket.slot] = ev

    def close(self) -> None:
        self.pool.shutdown(wait=True)


def _grown(nbytes: int) -> int:
    """Arena capacities are whole multiples of 64 KiB."""
    return max((nbytes + (1 << 16) - 1) >> 16 << 16, 1 << 16)


class _FolderSource:
    """What the two sources share: the list, per-sample seeding, staging with a one-batch prefetch."""

    _SALT = {"train": 11, "val": 23, "test": 37}

    def __init__(self, device, frame_dir, annotation_path, split, data_type, sample_duration, sample_size, seed, n_workers,
                 list_from=None):
        if data_type not in self._SALT:
            raise ValueError("data_type %r" % (data_type,))
        self.device, self.data_type = torch.device(device), data_type
        self.t, self.size, self.seed = sample_duration, sample_size, seed
        self.threads = decode_threads(n_workers)
        self.frame_dir, self.annotation_path, self.split = frame_dir, annotation_path, split
        self.list_from = data_type if list_from is None else list_from
        self.data = read_list(annotation_path, frame_dir, self.list_from, split)
        self._stager = None
        self._pending = None          # (key, staged request) of the prefetched batch

    def __len__(self):
        return len(self.data)

    def _seed(self, index: int, epoch: int) -> int:
        return ((self.seed * 1000003 + epoch) * 1000003 + index) * 101 + self._SALT[self.data_type]

    def _rngs(self, index: int, epoch: int):
        s = self._seed(index, epoch)
        return random.Random(s), np.random.RandomState(s & 0x7fffffff)

    # -- staging ----------------------------------------------------------------------------------------------------------
    def stager(self) -> FrameStager:
        if self._stager is None:
            self._stager = FrameStager(self.device, self.threads)
        return self._stager

    def _request(self, key):
        """-> (plans, samples [(paths, h, w)], whatever ``_assemble`` needs): host work only."""
        raise NotImplementedError

    def _begin(self, key):
        req = self._request(key)
        return req, self.stager().begin(req[1])

    def prefetch(self, key) -> None:
        """Start decoding the batch ``key`` names; the next ``_staged(key)`` picks it up."""
        if self._pending is not None and self._pending[0] == key:
            return
        self._drop_pending()
        self._pending = (key, self._begin(key))

    def _drop_pending(self):
        if self._pending is not None:
            _, (_, ticket) = self._pending
            self._pending = None
            try:
                FrameStager.wait(ticket)
            except Exception:               # noqa: BLE001 -- a batch nobody asked for
                pass

    def _staged(self, key, then=None):
        """The request and device views of batch ``key`` (prefetched or prepared now); ``then`` is started decoding before
        the caller's kernels are enqueued."""
        if self._pending is not None and self._pending[0] == key:
            req, ticket = self._pending[1]
            self._pending = None
        else:
            self._drop_pending()
            req, ticket = self._begin(key)
        views = self.stager().finish(ticket)
        if then is not None:
            try:
                self.prefetch(then)
            except FrameError:              # it belongs to the batch after this one: raised when that batch is asked for
                self._pending = None
        return req, ticket, views

    def close(self):
        self._drop_pending()
        if self._stager is not None:
            self._stager.close()
            self._stager = None


class FramePairFolder(_FolderSource):
    """UcfRepreBYOLSpPre on the GPU clip pipeline: ``batch(indices, epoch)`` returns what ``GpuVideoClips.batch`` returns, from
    the JPEG frames of the listed videos.  Plans come from ``sampler.sample_pair`` with a ``random.Random`` / ``RandomState``
    per sample seeded from (seed, epoch, index); the frame size is that of the first planned frame (the reference takes the
    image size from the first frame of each clip list)."""

    def __init__(self, device, frame_dir, annotation_path, split=1, data_type="train", sample_duration=16, sample_size=112, seed=1,
                 n_workers=4):
        super().__init__(device, frame_dir, annotation_path, split, data_type, sample_duration, sample_size, seed, n_workers)

    def plan_sized(self, index: int, epoch: int = 0):
        """-> (PairPlan, frame width, frame height)."""
        folder, _, n_frames = self.data[index]
        rng, np_rng = self._rngs(index, epoch)
        state = rng.getstate()
        first = sampler.sample_frames(n_frames, self.t, rng)[0][0]          # the frame draws do not depend on the frame size
        rng.setstate(state)
        w, h = frame_size(frame_path(folder, first))
        return sampler.sample_pair(n_frames, w, h, self.t, rng, np_rng=np_rng), w, h

    def plan(self, index: int, epoch: int = 0) -> "sampler.PairPlan":
        return self.plan_sized(index, epoch)[0]

    def _request(self, key):
        indices, epoch = key
        plans, samples = [], []
        for i in indices:
            folder = self.data[i][0]
            plan, w, h = self.plan_sized(i, epoch)
            unique, (f1, f2) = union_remap([plan.clip_1.frames, plan.clip_2.frames])
            plans.append(dataclasses.replace(plan, clip_1=dataclasses.replace(plan.clip_1, frames=f1),
                                             clip_2=dataclasses.replace(plan.clip_2, frames=f2)))
            samples.append(([frame_path(folder, f) for f in unique], h, w))
        return plans, samples

    def batch(self, indices: List[int], epoch: int = 0, prefetch: List[int] = None):
        """-> (clip_1 [B,3,T,S,S], clip_2, spa, tem, pb, rot_1, rot_2) on the device, labels int64.  ``prefetch``: the indices
        of the batch that follows in the same epoch; its frames are decoded while this one is consumed."""
        then = (tuple(prefetch), epoch) if prefetch else None
        (plans, _), ticket, views = self._staged((tuple(indices), epoch), then)
        c1, c2 = assemble_pairs(views, plans, self.size)
        self.stager().release(ticket)
        lab = torch.tensor([[p.spa_label for p in plans], [p.tem_label for p in plans], [p.pb_label for p in plans],
                            [p.rot_labels[0] for p in plans], [p.rot_labels[1] for p in plans]], dtype=torch.int64)
        lab = lab.pin_memory().to(self.device, non_blocking=True)
        return c1, c2, lab[0], lab[1], lab[2], lab[3], lab[4]


class FrameLabelledFolder(_FolderSource):
    """UcfFineTune on the GPU clip pipeline: ``batch(indices, epoch)`` and ``video(index)`` behave as ``GpuLabelledVideos``'
    do, from the JPEG frames of the listed videos, under the PIL transform modes 'img' / 'img_val' / 'img_test' (the ``numpy*``
    modes resize with cv2 and stay refused).  The label is the list's second column as it stands (datasets.py:977).
    ``list_from="train"`` with data_type 'test' / mode 'img_test' reads the TRAIN list as whole-video test items: the gallery of
    nearest-neighbour retrieval (cstp_amd.retrieval); by default the list follows data_type.  ``randaug=(n, m, mstd)`` and
    ``random_erase=P`` augment 'train' clips (cstp_amd.randaug), from a generator of their own per clip."""

    augment = None

    def __init__(self, device, frame_dir, annotation_path, split=1, data_type="train", mode="img", sample_duration=16,
                 sample_size=112, pb_rate=4, seed=1, n_workers=4, list_from=None, randaug=None, random_erase=0.0):
        sampler._check_ft_mode(mode)
        self.augment = augment_settings(randaug, random_erase, data_type, mode)      # training clips only
        if (data_type == "test") != (mode == "img_test"):
            raise ValueError("data_type %r with transform mode %r: the video test takes 'img_test', train / val take 'img' / "
                             "'img_val'" % (data_type, mode))
        if mode != "img":
            sampler.short_side(sample_size)
        if list_from is not None and (list_from not in ("train", "test") or data_type != "test"):
            raise ValueError("list_from %r with data_type %r: only the video test reads another list ('train' | 'test')"
                             % (list_from, data_type))
        super().__init__(device, frame_dir, annotation_path, split, data_type, sample_duration, sample_size, seed, n_workers,
                         list_from)
        self.mode, self.pb_rate = mode, pb_rate
        self.labels = [lab for _, lab, _ in self.data]

    def plan_sized(self, index: int, epoch: int = 0):
        """-> (FtClipPlan for 'train' / 'val', [FtClipPlan] -- every clip of the video -- for 'test'; frame width; height)."""
        folder, _, n_frames = self.data[index]
        if self.data_type == "test":
            first = sampler.ft_test_frames(n_frames, self.t, self.pb_rate)[0][0]
            w, h = frame_size(frame_path(folder, first))
            return sampler.plan_test_video(n_frames, w, h, self.t, self.size, self.pb_rate, self.mode), w, h
        rng, _ = self._rngs(index, epoch)
        state = rng.getstate()
        first = sampler.ft_clip_frames(n_frames, self.t, self.pb_rate, rng)[0]
        rng.setstate(state)
        w, h = frame_size(frame_path(folder, first))
        plan = sampler.sample_ft_clip(n_frames, w, h, self.t, self.size, self.pb_rate, self.mode, rng)
        if self.augment is not None:      # a generator of its own: the draws above keep their values
            plan.randaug, plan.erase = randaug_draws.draw(self.augment, self.size, randaug_draws.clip_rng(self._seed(index, epoch)))
        return plan, w, h

    def plan(self, index: int, epoch: int = 0):
        return self.plan_sized(index, epoch)[0]

    def _request(self, key):
        indices, epoch = key
        plans, samples, owner = [], [], []
        for k, i in enumerate(indices):
            folder = self.data[i][0]
            mine, w, h = self.plan_sized(i, epoch)
            mine = mine if isinstance(mine, list) else [mine]
            unique, remapped = union_remap([p.frames for p in mine])
            plans += [dataclasses.replace(p, frames=f) for p, f in zip(mine, remapped)]
            owner += [k] * len(mine)
            samples.append(([frame_path(folder, f) for f in unique], h, w))
        return plans, samples, owner

    def _labels(self, indices):
        return torch.tensor([self.labels[i] for i in indices], dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)

    def _clips(self, key, then):
        (plans, _, owner), ticket, views = self._staged(key, then)
        clips = assemble_batch([views[k] for k in owner], plans, self.size)
        self.stager().release(ticket)
        return clips

    def batch(self, indices: List[int], epoch: int = 0, prefetch: List[int] = None):
        """-> (clips [B,3,T,S,S] fp32, labels [B] int64) on the device."""
        if self.data_type == "test":
            raise ValueError("batch() serves data_type 'train' / 'val'; a 'test' item is a whole video()")
        then = (tuple(prefetch), epoch) if prefetch else None
        return self._clips((tuple(indices), epoch), then), self._labels(indices)

    def video(self, index: int, prefetch: int = None):
        """A 'test' item: (clips [n_clips,3,T,S,S] fp32, label [1] int64) on the device (datasets.py:999-1001)."""
        if self.data_type != "test":
            raise ValueError("video() serves data_type 'test'")
        then = ((prefetch,), 0) if prefetch is not None else None
        return self._clips(((index,), 0), then), self._labels([index])


# ---- loaders: the sharding of GpuClipLoader / GpuLabelledLoader, plus the epoch and the hint for the prefetch ------------------
class FramePairLoader(GpuClipLoader):
    """GpuClipLoader over a FramePairFolder: same shuffle, stride and drop_last; passes the epoch (so the augmentation of a
    video changes from epoch to epoch) and names the next batch so that it is decoded while this one trains."""

    def __iter__(self):
        idx = self.indices()
        bs, n = self.batch_size, len(self)
        for b in range(n):
            nxt = idx[(b + 1) * bs:(b + 2) * bs] if b + 1 < n else None
            c1, c2, spa, tem, pb, r1, r2 = self.dataset.batch(idx[b * bs:(b + 1) * bs], self.epoch, prefetch=nxt)
            yield [c1, c2], [spa, tem, pb, [r1, r2]]


class FrameLabelledLoader(GpuLabelledLoader):
    """GpuLabelledLoader over a FrameLabelledFolder: 'train' shuffled with full batches only, 'val' in order with the partial
    batch kept, 'test' one video per item; the next batch or video is decoded while this one is consumed."""

    def __iter__(self):
        idx = self.indices()
        if self.data_type == "test":
            for k, i in enumerate(idx):
                clips, label = self.dataset.video(i, prefetch=idx[k + 1] if k + 1 < len(idx) else None)
                yield clips.unsqueeze(0), label
            return
        bs, n = self.batch_size, len(self)
        for b in range(n):
            nxt = idx[(b + 1) * bs:(b + 2) * bs] if b + 1 < n else None
            yield self.dataset.batch(idx[b * bs:(b + 1) * bs], self.epoch, prefetch=nxt)


def build_pretrain(opts, device) -> FramePairFolder:
    """--dataset UcfRepreBYOLSpPre from the reference's flags (--frame_dir, --annotation_path, --split, --n_workers)."""
    return FramePairFolder(device, opts.frame_dir, opts.annotation_path, opts.split, "train", opts.sample_duration,
                           opts.sample_size, opts.manual_seed, opts.n_workers)


def build_finetune(opts, device, data_type: str, mode: str, list_from=None, augment=None) -> FrameLabelledFolder:
    """--dataset UcfFineTune from the reference's flags, for 'train' / 'val' / 'test' under ``mode``.  ``augment``: the
    ``randaug.Settings`` of --randaug_* / --random_erase, honoured for 'train' only."""
    if data_type != "train":
        augment = None
    return FrameLabelledFolder(device, opts.frame_dir, opts.annotation_path, opts.split, data_type, mode, opts.sample_duration,
                               opts.sample_size, opts.pb_rate, opts.manual_seed, opts.n_workers, list_from,
                               randaug=None if augment is None else (augment.n, augment.m, augment.mstd),
                               random_erase=0.0 if augment is None else augment.erase)
