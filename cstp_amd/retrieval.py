"""Nearest-neighbour video retrieval: the evaluation of a pre-trained encoder that needs no training.

Features of the query videos (the test split) are compared with features of the gallery videos (the train split) by cosine
similarity; R@k is the share of queries whose k nearest gallery videos include one of the query's class.  A video's feature is
the mean, over the clips of its test plan (sampler.plan_test_video), of the pooled backbone feature ``ByolBase.encode``.
The search runs in ops.sim_topk (csrc/retrieve.hip), which streams the gallery and keeps k candidates per query: the
[queries x gallery] similarity matrix is never built.
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple

import torch

from . import ops


def _inner(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "encode") else model


def build_video_sets(opts, dataset=None, what="retrieval"):
    """-> (gallery loader, query loader): one whole video per item, as the video test reads them; the train list is the gallery,
    the test list the queries.  ``dataset`` None: opts.dataset under --transform_mode img_test (the retrieval.py / knn.py
    drivers); named ("synthetic_video" | "UcfFineTune"): that kind of set from the same flags, whatever opts.dataset and
    opts.transform_mode say (the k-NN monitor of main_byol.py, whose own data set is the unlabelled pre-training one)."""
    if dataset is None:
        if opts.transform_mode != "img_test":
            raise ValueError("%s reads whole videos: --transform_mode img_test, got %r" % (what, opts.transform_mode,))
        dataset = opts.dataset
    if dataset == "synthetic_video":
        from .clip_ops import GpuLabelledLoader, GpuLabelledVideos
        kw = dict(n_classes=opts.n_classes, sample_duration=opts.sample_duration, sample_size=opts.sample_size,
                  pb_rate=opts.pb_rate)
        # two instances: other noise, other lengths, the same class-dependent patterns
        gallery = GpuLabelledVideos(opts.device, "test", "img_test", n_videos=max(opts.retrieval_gallery_len, 1),
                                    seed=opts.manual_seed + 1, **kw)
        queries = GpuLabelledVideos(opts.device, "test", "img_test", n_videos=max(opts.synthetic_len // 4, 1),
                                    seed=opts.manual_seed, **kw)
        return GpuLabelledLoader(gallery), GpuLabelledLoader(queries)
    if dataset == "UcfFineTune":
        from .frame_folder import FrameLabelledLoader, build_finetune
        gallery = build_finetune(opts, opts.device, "test", "img_test", list_from="train")
        queries = build_finetune(opts, opts.device, "test", "img_test")
        return FrameLabelledLoader(gallery), FrameLabelledLoader(queries)
    raise NotImplementedError("dataset %r: %s serves --dataset synthetic_video and UcfFineTune" % (dataset, what))


def close_video_sets(*loaders) -> None:
    """Stops the decode threads of frame-folder loaders (the synthetic ones have none)."""
    for loader in loaders:
        close = getattr(loader.dataset, "close", None)
        if close is not None:
            close()


def extract_features(model, loader) -> Tuple[torch.Tensor, torch.Tensor]:
    """``loader`` yields one video per item as the video-test loaders do: (clips [1, n_clips, 3, T, S, S], label [1]).
    -> (features [n, d] fp32, labels [n] int64) on the device of the clips; row v is the mean of encode() over video v's clips.
    The model is put in eval mode (running BatchNorm statistics) and nothing records a graph."""
    net = _inner(model)
    net.eval()
    feats, labels = [], []
    with torch.no_grad():
        for clips, label in loader:
            clips = torch.squeeze(clips, 0)
            f = net.encode(clips)
            if f.dim() != 2 or f.dtype != torch.float32:
                raise ValueError("encode() must give [clips, d] fp32, got %s %s" % (tuple(f.shape), f.dtype))
            feats.append(f.mean(dim=0))
            labels.append(label.reshape(1).to(f.device))
    if not feats:
        raise ValueError("extract_features: the loader gave no video")
    return torch.stack(feats).contiguous(), torch.cat(labels).to(torch.int64)


def recall_at_k(idx: torch.Tensor, q_labels: torch.Tensor, g_labels: torch.Tensor, ks: Iterable[int]) -> Dict[int, float]:
    """R@k for every k of ``ks`` from idx [nq, K] (gallery rows by rank, -1 where the list ran out): the share of queries with a
    gallery item of their own class among the first k.  Plain tensor ops; CPU or device tensors alike."""
    ks = [int(k) for k in ks]
    if idx.dim() != 2 or idx.shape[0] != q_labels.shape[0]:
        raise ValueError("idx %s does not match %d queries" % (tuple(idx.shape), q_labels.shape[0]))
    if not ks or min(ks) < 1 or max(ks) > idx.shape[1]:
        raise ValueError("ks %r must lie in 1..%d (the width of idx)" % (ks, idx.shape[1]))
    idx = idx.to(torch.int64)
    found = idx >= 0
    same = (g_labels.to(idx.device)[idx.clamp(min=0)] == q_labels.to(idx.device).reshape(-1, 1)) & found
    first = torch.where(same.any(dim=1), same.to(torch.int64).argmax(dim=1), torch.full_like(idx[:, 0], idx.shape[1]))
    return {k: float((first < k).to(torch.float64).mean()) for k in ks}


def retrieve(q_feat: torch.Tensor, q_labels: torch.Tensor, g_feat: torch.Tensor, g_labels: torch.Tensor, ks: Sequence[int],
             exclude_self: bool = False):
    """L2-normalise, search, score: -> (recall {k: R@k}, val [nq, K], idx [nq, K], normalised queries, normalised gallery) with
    K = max(ks).  ``exclude_self``: the queries ARE the gallery (leave-one-out), a video never retrieves itself."""
    ks = [int(k) for k in ks]
    qn, gn = ops.l2_normalize(q_feat), ops.l2_normalize(g_feat)
    val, idx = ops.sim_topk(qn, gn, max(ks), exclude_self)
    return recall_at_k(idx, q_labels, g_labels, ks), val, idx, qn, gn
