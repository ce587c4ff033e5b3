#!/usr/bin/env python3
"""The frame-folder data path (cstp_amd.frame_folder) timed on its own and against what it replaces, in one process on one box.
Writes a temporary tree of 340 x 256 JPEG frames (the UCF_101_1f_256 size; smooth pattern plus noise, quality 90, 4:2:0) and
prints one JSON line per case:
  * decoded frames / s with 1, 4, 8 and 16 Pillow threads (decode_into: open, decode, copy into a pinned arena);
  * ms to prepare a 16-pair, T = 16 batch: decode (thread pool, --threads) and upload (one async copy), and its unique frames;
  * assemble_pairs (2B descriptors, two launches) against the per-clip assemble_pair loop on the SAME plans and device frames,
    alternating repeats, outputs compared first;
  * the batched horizontal + vertical pass under each rotation code on the same centred box (what the column walk of 90 / 270 costs);
  * --step: ms / step of the R(2+1)D-18 pre-training step (bench.py's workload: B = 16 pairs, 3 x 16 x 112 x 112, fp32) fed from
    the folder through FramePairLoader against the same step fed by --dataset synthetic_video (GpuVideoClips through
    GpuClipLoader, the per-clip path), alternating, plus the step on a resident batch."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import clip_ops, frame_folder, sampler  # noqa: E402

H, W, T, SIZE, PAIRS = 256, 340, 16, 112, 16


def write_tree(root, n_videos, n_frames, repeat):
    frame_dir, ann = os.path.join(root, "frames"), os.path.join(root, "labels")
    os.makedirs(ann)
    ys, xs = np.mgrid[0:H, 0:W]
    lines = []
    for v in range(n_videos):
        entry = "Class%02d/v_Class%02d_g01_c01" % (v % 4, v)
        os.makedirs(os.path.join(frame_dir, entry))
        rs = np.random.RandomState(v)
        for f in range(n_frames):
            base = 127 + 80 * np.sin(xs / (17.0 + v) + ys / 23.0 + f / 5.0)[:, :, None] * np.array([1.0, 0.7, -0.8])
            img = np.clip(base + rs.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img, "RGB").save(os.path.join(frame_dir, entry, "%05d.jpg" % (f + 1)), quality=90)
        lines.append("%s.avi %d %d" % (entry, v % 4, n_frames))
    with open(os.path.join(ann, "trainlist01_nframe.txt"), "w") as f:
        f.write("\n".join(lines * repeat) + "\n")
    return frame_dir, ann


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed(fn, inner):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(inner):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, ev0.elapsed_time(ev1) / inner


def decode_rates(paths, repeats):
    arena = torch.empty(len(paths) * H * W * 3, dtype=torch.uint8, pin_memory=True).numpy().reshape(len(paths), H, W, 3)
    for threads in (1, 4, 8, 16):
        rates = []
        with ThreadPoolExecutor(max_workers=threads) as pool:
            for _ in range(repeats + 1):
                t0 = time.perf_counter()
                list(pool.map(frame_folder.decode_into, paths, arena))
                rates.append(len(paths) / (time.perf_counter() - t0))
        print(json.dumps({"case": "decode %d x %d JPEG, %d files per pass" % (W, H, len(paths)), "threads": threads,
                          "frames_per_s": summary(rates[1:])}), flush=True)


def prepare_batch(ds, repeats):
    st = ds.stager()
    dec, up, uniq = [], [], []
    for r in range(repeats + 2):
        key = (tuple(range(r * PAIRS % len(ds), r * PAIRS % len(ds) + PAIRS)), r)
        req = ds._request(key)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ticket = st.begin(req[1])
        st.wait(ticket)
        t1 = time.perf_counter()
        st.finish(ticket)
        st.copied[ticket.slot].synchronize()
        t2 = time.perf_counter()
        st.release(ticket)
        dec.append((t1 - t0) * 1e3)
        up.append((t2 - t1) * 1e3)
        uniq.append(sum(len(p) for p, _, _ in req[1]))
    print(json.dumps({"case": "prepare a %d-pair T = %d batch" % (PAIRS, T), "threads": ds.threads, "unique_frames": summary(uniq[2:]),
                      "of_frames_named": 2 * PAIRS * T, "decode_ms": summary(dec[2:]), "upload_ms": summary(up[2:]),
                      "megabytes": round(statistics.median(uniq[2:]) * H * W * 3 / 1e6, 1)}), flush=True)


def assemble_cases(ds, repeats, inner):
    (plans, samples), ticket, views = ds._staged((tuple(range(PAIRS)), 0))
    ds.stager().release(ticket)

    def batched():
        return clip_ops.assemble_pairs(views, plans, SIZE)

    def per_clip():
        got = [clip_ops.assemble_pair(v, p, SIZE)[0] for v, p in zip(views, plans)]
        return torch.stack([g[0] for g in got]), torch.stack([g[1] for g in got])

    a, b = batched(), per_clip()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for fn in (batched, per_clip):
        for _ in range(3):
            fn()
    res = {"batched": ([], []), "per_clip": ([], [])}
    for _ in range(repeats):                    # alternating: every repeat times both back to back
        for name, fn in (("batched", batched), ("per_clip", per_clip)):
            wall, dev = timed(fn, inner)
            res[name][0].append(wall)
            res[name][1].append(dev)
    clips = [c for p in plans for c in (p.clip_1, p.clip_2)]
    out = {"case": "%d pairs of %d x %d x %d clips from %d x %d frames" % (PAIRS, T, SIZE, SIZE, W, H), "repeats": repeats,
           "inner": inner, "base_clips": sum(c.base is not None for c in clips),
           "rotations": {str(r): sum(c.rotate == r for c in clips) for r in (0, 90, 180, 270)}}
    for name, label in (("batched", "assemble_pairs"), ("per_clip", "assemble_pair_loop")):
        out[label + "_wall_ms"], out[label + "_gpu_ms"] = summary(res[name][0]), summary(res[name][1])
    out["speedup_wall_median"] = round(out["assemble_pair_loop_wall_ms"]["median"] / out["assemble_pairs_wall_ms"]["median"], 2)
    print(json.dumps(out), flush=True)
    # the two passes under each rotation code: the same 224 x 224 box (inside the frame in either orientation), 32 clips
    video = views[0]
    n = video.shape[0]
    per_rot = {}
    fns = {}
    for rot in (0, 90, 180, 270):
        rp = [sampler.ClipPlan([(i + j) % n for j in range(T)], rot, (16, 16, 240, 240), False, False) for i in range(2 * PAIRS)]
        fns[rot] = (lambda rp=rp: clip_ops._batch_forward(video, rp, SIZE, None, []))
        fns[rot]()
        per_rot[rot] = []
    for _ in range(repeats):
        for rot, fn in fns.items():
            per_rot[rot].append(timed(fn, inner)[1])
    print(json.dumps({"case": "batched passes, %d clips, box 224 x 224 of %d x %d frames, by rotation code" % (2 * PAIRS, W, H),
                      "gpu_ms": {str(r): summary(v) for r, v in per_rot.items()}}), flush=True)


def step_cases(ds, steps, repeats):
    from cstp_amd.ntxent import NTXentLoss
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.train import PretrainStep
    torch.manual_seed(1)
    model = R21DBYOL(pretrain=True, layer_sizes=layer_sizes_for_depth(18)).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.09, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    ntx = NTXentLoss(device=torch.device("cuda", 0), batch_size=PAIRS, temperature=0.5, use_cosine_similarity=True)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 0.0, 0.0), clip_grad_norm=True, ntxent=ntx, ntxent_weight=1.0)
    folder = frame_folder.FramePairLoader(ds, PAIRS, seed=1)
    synth = clip_ops.GpuClipLoader(clip_ops.GpuVideoClips("cuda:0", sample_duration=T, sample_size=SIZE, length=PAIRS * steps),
                                   PAIRS, seed=1)
    epoch = [0]

    def fed(loader):
        def run():
            done = 0
            while done < steps:
                epoch[0] += 1
                loader.set_epoch(epoch[0])
                for (c1, c2), (spa, tem, pb, (r1, r2)) in loader:
                    step(c1, c2, spa, tem, pb, r1, r2)
                    done += 1
                    if done == steps:
                        break
        return run
    (c1, c2), (spa, tem, pb, (r1, r2)) = next(iter(synth))

    def resident():
        for _ in range(steps):
            step(c1, c2, spa, tem, pb, r1, r2)
    cases = (("frame_folder", fed(folder)), ("synthetic_video", fed(synth)), ("resident_batch", resident))
    for _, fn in cases:
        fn()
    res = {name: [] for name, _ in cases}
    for _ in range(repeats):
        for name, fn in cases:
            res[name].append(timed(fn, 1)[0] / steps)
    out = {"case": "R(2+1)D-18 pre-training step, B = %d pairs, 3 x %d x %d x %d fp32, ms / step over %d steps" % (PAIRS, T, SIZE, SIZE, steps),
           "threads": ds.threads, "repeats": repeats}
    for name in res:
        out[name + "_ms"] = summary(res[name])
    out["frame_folder_over_synthetic_video"] = round(out["frame_folder_ms"]["median"] / out["synthetic_video_ms"]["median"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--frames", type=int, default=120, help="frames per video")
    ap.add_argument("--threads", type=int, default=16, help="decode threads (--n_workers)")
    ap.add_argument("--step", action="store_true", help="also time the R(2+1)D-18 pre-training step fed from the folder")
    ap.add_argument("--steps", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py needs a HIP device")
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        frame_dir, ann = write_tree(root, args.videos, args.frames, repeat=8)
        print(json.dumps({"case": "wrote %d JPEG frames" % (args.videos * args.frames), "seconds": round(time.perf_counter() - t0, 1),
                          "pillow": Image.__version__}), flush=True)
        ds = frame_folder.FramePairFolder("cuda:0", frame_dir, ann, 1, "train", T, SIZE, seed=1, n_workers=args.threads)
        paths = [frame_folder.frame_path(ds.data[v][0], f) for v in range(min(args.videos, 8)) for f in range(64)]
        decode_rates(paths, args.repeats)
        prepare_batch(ds, args.repeats)
        assemble_cases(ds, args.repeats, args.inner)
        if args.step:
            step_cases(ds, args.steps, args.repeats)
        ds.close()


if __name__ == "__main__":
    main()
