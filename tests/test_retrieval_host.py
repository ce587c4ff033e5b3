"""Video retrieval, the parts that need no GPU: the C ABI of the similarity top-k (declared, bound, exported, refusing bad
arguments before any HIP call, workspace bounded by nq * k), the refusals of ops.sim_topk, the new flags, the retrieval task of the
model factory, R@k against a hand-written answer, the acceptance rule tests/retrieval_spec.check_topk (it accepts the stable fp32
answer and bites on a wrong member and on a wrong tie order), and the train list read as whole-video test items."""
import ctypes
import os

import pytest
import torch

from retrieval_spec import _stable_from_scores, check_topk, stable_reference, tau_for, unit_rows
from test_abi import header_symbols
from test_frame_folder_host import PB, T, VIDEOS, write_tree


def test_simtopk_is_declared_bound_and_exported():
    from cstp_amd import _lib
    names = ("cstp_simtopk", "cstp_simtopk_workspace_bytes")
    syms = header_symbols()
    for n in names:
        assert n in syms and n in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # added without a bump, as the S3D-G and I3D entry points were
    assert "#define CSTP_ABI_VERSION 18" in open(os.path.join(os.path.dirname(_lib._HERE), "include", "cstp_hip.h")).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n)
    assert lib.cstp_abi_version() == 18


def test_simtopk_refuses_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks fail first
    big = 1 << 30
    calls = [
        ((None, one, one, 8, 100, 16, 0, 0, one, one, one, big), b"k must be in 1..64"),
        ((None, one, one, 8, 100, 16, 65, 0, one, one, one, big), b"k must be in 1..64"),
        ((None, one, one, 0, 100, 16, 5, 0, one, one, one, big), b"bad shape"),
        ((None, one, one, 8, 0, 16, 5, 0, one, one, one, big), b"bad shape"),
        ((None, one, one, 8, 100, 0, 5, 0, one, one, one, big), b"bad shape"),
        ((None, None, one, 8, 100, 16, 5, 0, one, one, one, big), b"null argument"),
        ((None, one, None, 8, 100, 16, 5, 0, one, one, one, big), b"null argument"),
        ((None, one, one, 8, 100, 16, 5, 0, None, one, one, big), b"null argument"),
        ((None, one, one, 8, 100, 16, 5, 0, one, None, one, big), b"null argument"),
        ((None, one, one, 8, 100, 16, 5, 0, one, one, None, big), b"null argument"),
        ((None, one, one, 7, 20000, 512, 64, 0, one, one, one, 1024), b"workspace too small"),
    ]
    for args, needle in calls:
        rc = lib.cstp_simtopk(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"line" in msg, (args, rc, msg)
    for bad in ((0, 5, 8, 1), (5, 0, 8, 1), (5, 5, 0, 1), (5, 5, 8, 0), (5, 5, 8, 65), (-1, 5, 8, 1)):
        assert lib.cstp_simtopk_workspace_bytes(*bad) == 0


def test_workspace_grows_with_queries_times_k_not_with_the_matrix():
    from cstp_amd import _lib
    lib = _lib.load()
    const = 4096
    nq, ng, d, k = 4096, 65536, 128, 50
    b = lib.cstp_simtopk_workspace_bytes(nq, ng, d, k)
    assert 0 < b <= 32 * nq * k * 8 + const
    assert b < 0.01 * nq * ng * 4                                            # the fp32 matrix would be 1 GiB
    for nq2, ng2, k2 in ((1, 1, 1), (7, 20000, 64), (1500, 1300, 20), (20000, 240000, 50), (3, 2 ** 31 - 200, 64)):
        b2 = lib.cstp_simtopk_workspace_bytes(nq2, ng2, 512, k2)
        assert 0 < b2 <= 32 * nq2 * k2 * 8 + const, (nq2, ng2, k2, b2)
    # ten times the gallery: not one byte more once the split count has reached its cap
    assert lib.cstp_simtopk_workspace_bytes(7, 200000, 512, 64) == lib.cstp_simtopk_workspace_bytes(7, 2000000, 512, 64)


def test_sim_topk_refusals_on_cpu_tensors():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    q, g = torch.zeros(3, 8), torch.zeros(5, 8)
    with pytest.raises(CstpError, match="HIP device"):
        ops.sim_topk(q, g, 2)
    with pytest.raises(CstpError, match="float32"):
        ops.sim_topk(q.double(), g, 2)
    with pytest.raises(CstpError, match="float32"):
        ops.sim_topk(q, g.to(torch.bfloat16), 2)
    with pytest.raises(CstpError, match="features"):
        ops.sim_topk(q, torch.zeros(5, 9), 2)
    for k in (0, 65, -1, 2.0):
        with pytest.raises(CstpError, match="k must be"):
            ops.sim_topk(q, g, k)
    with pytest.raises(CstpError, match="rows, features"):
        ops.sim_topk(q[0], g, 1)


def test_opts_carry_the_retrieval_flags():
    from cstp_amd.opts import parse_opts
    d = parse_opts([])
    assert d.retrieval_k == [1, 5, 10, 20, 50] and d.retrieval_gallery_len > 0
    o = parse_opts(["--retrieval_k", "3", "64", "1", "--retrieval_gallery_len", "12"])
    assert o.retrieval_k == [3, 64, 1] and o.retrieval_gallery_len == 12
    for bad in ("65", "0"):
        with pytest.raises(SystemExit):
            parse_opts(["--retrieval_k", "5", bad])


def test_retrieval_task_is_known_to_the_model_factory():
    from cstp_amd import model
    from cstp_amd.model import generate_model
    from cstp_amd.opts import parse_opts
    assert "retrieval" in model.RETRIEVAL_TASKS
    if torch.cuda.is_available():
        return                                          # the refusal below is what a machine without a GPU sees
    for name, depth in (("r21d_byol", 18), ("r3d_byol", 18), ("s3d_byol", 1), ("i3d_byol", 1)):
        o = parse_opts(["--model_name", name, "--model_depth", str(depth), "--task", "retrieval"])
        with pytest.raises(RuntimeError, match="HIP device"):        # not the ValueError an unknown task gets
            generate_model(o)


def test_retrieval_driver_refuses_without_a_gpu_and_names_its_datasets():
    import retrieval as driver
    from cstp_amd.opts import parse_opts
    o = parse_opts(["--dataset", "Kin400RepreLMDB", "--transform_mode", "img_test"])
    o.device = "cpu"
    with pytest.raises(NotImplementedError):
        driver.build_sets(o)
    o = parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img"])
    with pytest.raises(ValueError, match="img_test"):
        driver.build_sets(o)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img_test"]))


def test_recall_at_k_against_a_hand_written_answer():
    from cstp_amd.retrieval import recall_at_k
    g_labels = torch.tensor([0, 0, 1, 2, 1, 3])
    q_labels = torch.tensor([1, 0, 2, 7, 3])            # class 7 has no gallery item
    idx = torch.tensor([[0, 2, 4, 1],                   # first hit at rank 2
                        [1, 0, 5, 3],                   # rank 1
                        [0, 1, 2, 3],                   # rank 4
                        [3, 2, 1, 0],                   # never
                        [0, 1, -1, -1]], dtype=torch.int32)     # the list ran out before class 3 (row 5): never; -1 is no row
    r = recall_at_k(idx, q_labels, g_labels, [4, 1, 2])          # ks not sorted
    assert list(r) == [4, 1, 2]
    assert r[1] == pytest.approx(1 / 5) and r[2] == pytest.approx(2 / 5) and r[4] == pytest.approx(3 / 5)
    full = recall_at_k(idx, q_labels, g_labels, [1, 2, 3, 4])
    assert [full[k] for k in (1, 2, 3, 4)] == sorted(full.values())          # R@k never decreases with k
    assert full[3] == pytest.approx(2 / 5)
    # -1 must not be read as "the last gallery row": with the last row of class 3 the padded query still misses
    assert recall_at_k(torch.tensor([[-1, -1]]), torch.tensor([3]), g_labels, [2])[2] == 0.0
    with pytest.raises(ValueError):
        recall_at_k(idx, q_labels, g_labels, [5])
    with pytest.raises(ValueError):
        recall_at_k(idx, q_labels[:3], g_labels, [1])


SHAPES = [(3, 5, 7, 5), (65, 257, 512, 50), (33, 4097, 2048, 10)]


@pytest.mark.parametrize("nq,ng,d,k", SHAPES)
def test_check_topk_accepts_the_stable_fp32_answer_and_bites(nq, ng, d, k):
    q, g = unit_rows(nq, d, 11), unit_rows(ng, d, 12)
    tau = tau_for(d)
    val, idx = stable_reference(q, g, k)
    check_topk(val, idx, q, g, k, False, tau)
    # one far-away element swapped in: the least similar gallery row of query 0 takes the place of its best match
    s = q.double() @ g.double().T
    worst = int(s[0].argmin())
    assert float(s[0].max() - s[0].min()) > 100 * tau
    v2, i2 = val.clone(), idx.clone()
    v2[0, 0], i2[0, 0] = float(s[0, worst]), worst
    with pytest.raises(AssertionError):
        check_topk(v2, i2, q, g, k, False, tau)
    # a wrong value at a right index
    v3 = val.clone()
    v3[0, 0] += 4 * tau
    with pytest.raises(AssertionError):
        check_topk(v3, idx, q, g, k, False, tau)
    # a duplicate
    if k > 1:
        i4 = idx.clone()
        i4[0, 1] = i4[0, 0]
        with pytest.raises(AssertionError):
            check_topk(val, i4, q, g, k, False, tau)


def test_check_topk_pins_the_tie_order_and_the_padding():
    nq, ng, d, k = 4, 9, 16, 5
    q, g = unit_rows(nq, d, 3), unit_rows(ng, d, 4)
    g[6] = g[2]                                                              # rows 2 and 6 are the same vector
    s = q @ g.T
    s[:, 6] = s[:, 2]                                                        # and their fp32 similarities the same bits
    val, idx = _stable_from_scores(s, ng, False)
    check_topk(val, idx, q, g, ng, False, tau_for(d))
    pos2 = (idx == 2).nonzero()
    assert bool((idx[pos2[:, 0], pos2[:, 1] + 1] == 6).all())                # the stable sort put 2 right before 6
    bad = idx.clone()
    bad[pos2[:, 0], pos2[:, 1]] = 6
    bad[pos2[:, 0], pos2[:, 1] + 1] = 2
    with pytest.raises(AssertionError, match="ascending index"):
        check_topk(val, bad, q, g, ng, False, tau_for(d))
    # ng < k: the tail is (-inf, -1), no more and no less
    val, idx = stable_reference(q, g[:3], k)
    assert bool((idx[:, 3:] == -1).all()) and bool((val[:, 3:] == float("-inf")).all())
    check_topk(val, idx, q, g[:3], k, False, tau_for(d))
    short = idx.clone()
    short[:, 2] = -1
    with pytest.raises(AssertionError):
        check_topk(val, short, q, g[:3], k, False, tau_for(d))
    # exclude_self: q is g; i is never returned and one candidate fewer exists
    val, idx = stable_reference(g[:4], g[:4], k, exclude_self=True)
    assert bool((idx[:, 3:] == -1).all())
    check_topk(val, idx, g[:4], g[:4], k, True, tau_for(d))
    val, idx = stable_reference(g[:4], g[:4], k)
    with pytest.raises(AssertionError, match="itself"):
        check_topk(val, idx, g[:4], g[:4], k, True, tau_for(d))


def test_train_list_as_whole_video_test_items(tmp_path):
    from cstp_amd import sampler
    from cstp_amd.frame_folder import FrameLabelledFolder
    frame_dir, ann = write_tree(tmp_path)
    size = 112                                          # the video test's ClipScale knows 112 and 224 only
    kw = dict(sample_duration=T, sample_size=size, pb_rate=PB)
    gallery = FrameLabelledFolder("cpu", frame_dir, ann, 1, "test", "img_test", list_from="train", **kw)
    queries = FrameLabelledFolder("cpu", frame_dir, ann, 1, "test", "img_test", **kw)
    assert len(gallery) == len(VIDEOS) and len(queries) == len(VIDEOS[::2])              # the missing folder is skipped in both
    assert gallery.labels == [lab for _, lab, _, _, _, _ in VIDEOS]
    assert [f for f, _, _ in queries.data] == [f for f, _, _ in gallery.data][::2]
    for i, (_, _, n, h, w, _) in enumerate(VIDEOS):
        plans = gallery.plan(i)
        want = sampler.plan_test_video(n, w, h, T, size, PB, "img_test")
        assert isinstance(plans, list) and len(plans) == len(want) >= 1
        assert [p.frames for p in plans] == [p.frames for p in want]
    # the pinned refusals stand, and list_from belongs to the video test alone
    for args in (("train", "img_test"), ("test", "img"), ("test", "img_val")):
        with pytest.raises(ValueError):
            FrameLabelledFolder("cpu", frame_dir, ann, 1, *args, **kw)
    with pytest.raises(ValueError):
        FrameLabelledFolder("cpu", frame_dir, ann, 1, "train", "img", list_from="train", **kw)
    with pytest.raises(ValueError):
        FrameLabelledFolder("cpu", frame_dir, ann, 1, "test", "img_test", list_from="training", **kw)
