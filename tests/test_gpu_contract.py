"""GPU tests of the host-side mirrors and of the engine's clip/streaming
interface, all through the C ABI."""
import os

import numpy as np
import pytest
import torch
import yaml

from playaid_core_amd import synth
from playaid_core_amd.anim_ontology import ACTIONS, MOVE_TO_CLASS_ID

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_crops_on_gpu(engine):
    z = np.load(os.path.join(GOLD, "crop_kats.npz"))
    for (h, w, seed, idx, pad), box, ok, crop in zip(z["cases"], z["boxes"], z["ok"], z["crops"]):
        frame = synth.make_frame(int(idx), int(h), int(w), int(seed))
        got, status = engine.square_crops(frame[None], np.array([[box, box]]), padding=int(pad))
        assert (status[0, 0] == 0) == bool(ok)
        assert np.array_equal(got[0, 0], crop)
        assert np.array_equal(got[0, 1], crop)


def test_golden_clip720_on_gpu(engine):
    z = np.load(os.path.join(GOLD, "clip720_golden.npz"))
    n, h, w = int(z["n"]), int(z["height"]), int(z["width"])
    got = engine.infer_clip(synth.make_frames(n, h, w), synth.make_boxes(n, h, w))
    assert np.abs(got["logp"] - z["logp"]).max() <= 1e-4
    assert np.array_equal(got["action_id"], z["action_id"])
    assert np.allclose(got["prob"] * 100.0, z["confidence"], atol=1e-2)


def test_detector_and_runner_mirrors(tmp_path, state_dict):
    from oracle import cnn
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.timeline import load_timeline_from_ai_output

    ckpt = str(tmp_path / "seeded.ckpt")
    synth.save_checkpoint(ckpt, seed=1234)
    model = CNNActionDetector.load_from_checkpoint(
        ckpt, actions=list(MOVE_TO_CLASS_ID.keys()), max_batch_frames=32, max_clip_frames=64,
        max_frame_height=720, max_frame_width=1280,
    )
    assert model.eval() is model and model.sequence_length == 7 and model.actions == ACTIONS
    # b1: model(x)
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 7, 3, 128, 128)).astype(np.float32) / np.float32(255))
    logp = model(x)
    assert not logp.is_cuda and logp.shape == (2, 63)
    assert (logp - cnn.forward(x, state_dict)).abs().max() <= 1e-4
    with pytest.raises(ValueError):
        model(x[:, :5])
    # b2: runner
    clip = ClipSource.synthetic(30, 720, 1280)
    runner = AIRunner(clip, model=model, output_dir=str(tmp_path / "ai_cache"))
    assert runner.fighters == ["Pikachu", "Joker"] and runner.max_frames == 30
    inp, char_id, action_id, data = runner.action_recognition(14, "Joker")
    assert inp.shape == (1, 7, 3, 128, 128) and char_id == 3 and len(data["frames"]) == 7
    assert data["frames"][0].shape == (128, 128, 3) and data["predicted_action"] == ACTIONS[int(action_id)]
    # the reference's own call shape: model(input_frames) on the window reproduces the cached-path answer
    lp = model(inp)
    assert int(torch.argmax(lp)) == int(action_id)
    assert float(torch.exp(lp)[0][int(action_id)]) * 100.0 == pytest.approx(data["confidence"], abs=1e-2)
    assert str(data["crop"]).startswith("3 ") and data["crop"].confidence == 1.0
    with pytest.raises(IndexError):
        runner.action_recognition(30, "Joker")
    runner.run_action_recognition()
    runner.write_output()
    out = yaml.safe_load(open(runner.ai_output_file))
    assert sorted(out) == ["Joker", "Pikachu"] and sorted(out["Joker"]) == list(range(29))
    assert out["Joker"][13]["action"] == data["predicted_action"]
    tl = load_timeline_from_ai_output(runner.ai_output_file, max_frames=29)
    assert tl[13][0]["action"] == data["predicted_action"]
    # resume: a second runner finds the cached output and skips the work (ai_runner.py:503-505)
    again = AIRunner(clip, model=model, output_dir=str(tmp_path / "ai_cache"))
    assert again.ai_output_data["Joker"][0].action


def test_runner_repairs_label_gaps(tmp_path, state_dict):
    """Row a3: a fighter the detector lost for three frames (and lost for good near the end) is
    repaired as clean_yolo_crops does (ai_runner.py:361-424, 270-289): interpolated boxes measured
    from the END frame, pixels from VideoCapture position j (one frame late), tail image duplicated;
    the labels then match the CPU oracle run on exactly those (frame, box) pairs."""
    from oracle import jpeg, pipeline
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.fighter import YoloCrop

    n, h, w = 36, 720, 1280
    clip = ClipSource.synthetic(n, h, w)
    full = [[YoloCrop.from_string(l) for l in t.splitlines()] for t in clip.labels]
    drop = {12, 13, 14, 35, 36}  # Joker (second line) missing in these 1-indexed frames
    clip.labels = ["".join(str(c) + "\n" for k, c in enumerate(cs) if not (k == 1 and i + 1 in drop)) for i, cs in enumerate(full)]
    ckpt = str(tmp_path / "seeded.ckpt")
    synth.save_checkpoint(ckpt, seed=1234)
    model = CNNActionDetector.load_from_checkpoint(
        ckpt, actions=list(MOVE_TO_CLASS_ID.keys()), max_batch_frames=64, max_clip_frames=64,
        max_frame_height=h, max_frame_width=w,
    )
    runner = AIRunner(clip, model=model, output_dir=str(tmp_path / "ai_cache"), crop_mode="square")
    assert runner.max_frames == n
    runner.run_action_recognition()
    # expected (frame index, box) per entry, written out independently of label_cleaning.py
    src = np.arange(n)[:, None].repeat(2, 1)
    boxes = np.array([[c.yolo_crop() for c in cs] for cs in full])
    s11, e15 = full[10][1], full[14][1]
    for j in (12, 13, 14):
        it = s11.interp(e15, (15 - j) / (15 - 11))
        boxes[j - 1, 1] = it.yolo_crop()
        src[j - 1, 1] = j
        assert runner.ai_output_data["Joker"][j - 1].crop == str(it)
    boxes[34, 1], src[34, 1] = boxes[33, 1], 33  # frame 35 <- frame 34's image; frame 36 has no crop, never needed
    assert runner.ai_output_data["Joker"][34].crop == "None"
    crops = np.zeros((n, 2, 128, 128, 3), np.uint8)
    for p in range(2):
        cp, ok = pipeline.crops_for_clip(clip.frames[src[:, p]], boxes)
        assert ok.all()
        # the runner's default: every crop through the reference's JPEG write + read (ai_runner.py:420,446)
        crops[:, p] = np.stack([jpeg.roundtrip(c, 95) for c in cp[:, p]])
    want = pipeline.run_action_recognition(clip.frames, boxes, state_dict, mode="cached", crops_rgb=crops)
    res = runner._results
    assert np.array_equal(res["crops_rgb"][:35], crops[:35]) and np.array_equal(res["crops_rgb"][35, 0], crops[35, 0])
    assert np.abs(res["logp"] - want["logp"]).max() <= 1e-4
    assert np.array_equal(res["action_id"], want["action_id"])
    for f in range(1, n):
        assert runner.ai_output_data["Joker"][f - 1].action == ACTIONS[int(want["action_id"][f - 1, 1])]


def test_capacity_and_argument_errors(state_dict):
    """The reference's asserts / exit()s become status codes: nothing is silently truncated."""
    from playaid_core_amd import _lib
    from playaid_core_amd.engine import Engine, EngineError

    eng = Engine(state_dict, max_batch_frames=4, max_clip_frames=16, max_frame_height=360, max_frame_width=640)
    try:
        h, w = 360, 640
        frames, boxes = synth.make_frames(20, h, w), synth.make_boxes(20, h, w)
        with pytest.raises(EngineError) as ei:  # clip longer than the feature cache
            eng.infer_clip(frames, boxes)
        assert ei.value.code == _lib.PA_ERR_CAPACITY
        with pytest.raises(EngineError) as ei:  # frame larger than the resampler scratch
            eng.infer_clip(synth.make_frames(4, 720, 1280), synth.make_boxes(4, 720, 1280))
        assert ei.value.code == _lib.PA_ERR_CAPACITY
        with pytest.raises(EngineError) as ei:  # a window needs at least two frames (max_frames - 1 >= 1)
            eng.infer_clip(frames[:1], boxes[:1])
        assert ei.value.code == _lib.PA_ERR_INVALID_ARG
        with pytest.raises(EngineError) as ei:  # more frames in one backbone call than max_batch_frames
            eng.clip_begin(16)
            eng.backbone_frames(torch.from_numpy(frames[:8]).cuda(), torch.from_numpy(boxes[:8]).cuda(), 0)
        assert ei.value.code == _lib.PA_ERR_CAPACITY
        # the longest clip that fits, fed in the largest chunks that fit, still works
        out = eng.infer_clip(frames[:16], boxes[:16])
        assert out["logp"].shape == (15, 2, 63) and np.isfinite(out["logp"]).all()
    finally:
        eng.close()


def test_im2col_engine_still_agrees(engine, tmp_path):
    """PA_PATCH=0 (read once per process) sends the fp32 stride-1 3x3 convs that would run on conv3x3_patch_kernel
    back through the im2col engine, which stays the fallback for geometries the patch kernel rejects. At the
    default PA_WINO=1 all thirteen of them run as Winograd and PA_PATCH changes no launch of this engine
    (tests/test_engine_plan.py): the two processes must then agree like two runs of one build, and to fp32
    rounding (different summation order) wherever the patch kernel does run."""
    import subprocess
    import sys

    n, h, w = 24, 720, 1280
    frames, boxes = synth.make_frames(n, h, w, seed=31), synth.make_boxes(n, h, w)
    ours = engine.infer_clip(frames, boxes)
    out = tmp_path / "igemm_logp.npy"
    code = (
        "import numpy as np, sys\n"
        "sys.path.insert(0, %r)\n"
        "from playaid_core_amd import synth\n"
        "from playaid_core_amd.engine import Engine\n"
        "e = Engine(synth.make_state_dict(seed=1234), max_batch_frames=64, max_clip_frames=512)\n"
        "r = e.infer_clip(synth.make_frames(%d, %d, %d, seed=31), synth.make_boxes(%d, %d, %d))\n"
        "np.save(%r, r['logp'])\n" % (str(ROOT), n, h, w, n, h, w, str(out))
    )
    env = dict(os.environ, PA_PATCH="0", PA_STEM_IGEMM="1")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
    other = np.load(out)
    assert np.abs(other - ours["logp"]).max() <= 1e-5


BF16_LOGP_TOL = 5e-2  # bf16 conv path (configs[2]); measured 1.8e-2 on this clip. The fp32 path's bar is 1e-4.


def test_bf16_conv_path_against_oracle(state_dict):
    """BASELINE.json configs[2]: 3x3 convolutions on bf16 activations / weights (8 mantissa bits),
    fp32 accumulation, everything else fp32. Not within the north-star's 1e-4 (that bar is for the
    default fp32 path): log-probs within 5e-2 of the fp32 CPU oracle, the same argmax wherever the
    oracle's top-2 margin exceeds that, crops bit-exact (the crop stage does not change)."""
    from oracle import pipeline
    from playaid_core_amd.engine import Engine

    n, h, w = 40, 720, 1280
    frames, boxes = synth.make_frames(n, h, w), synth.make_boxes(n, h, w)
    ref = pipeline.run_action_recognition(frames, boxes, state_dict, mode="cached")
    eng = Engine(state_dict, max_batch_frames=32, max_clip_frames=64, max_frame_height=h, max_frame_width=w,
                 compute_dtype="bf16")
    try:
        got = eng.infer_clip(frames, boxes, want_crops=True)
        # chunked (two backbone calls, different tile / split-K choices) vs one shot: same bf16 roundings
        eng.clip_begin(n)
        fd, bd = torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda()
        eng.backbone_frames(fd[:24], bd[:24], 0)
        eng.backbone_frames(fd[24:], bd[24:], 24)
        lp2 = eng.alloc_logp(n - 1)
        eng.head_frames(1, n, eng.alloc_records(n - 1), lp2)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert np.array_equal(got["crops_rgb"], ref["crops_rgb"]) and (got["crop_status"] == 0).all()
    d = np.abs(got["logp"].astype(np.float64) - ref["logp"])
    assert d.max() <= BF16_LOGP_TOL, d.max()
    assert d.max() > 1e-4  # the test would be vacuous if this engine silently ran the fp32 kernels
    top2 = np.sort(ref["logp"], axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > BF16_LOGP_TOL * 2
    assert clear.any() and np.array_equal(got["action_id"][clear], ref["action_id"][clear])
    assert np.abs(lp2.cpu().numpy() - got["logp"]).max() <= 2e-2


_BF16_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from playaid_core_amd import synth
from playaid_core_amd.engine import Engine
e = Engine(synth.make_state_dict(seed=1234), max_batch_frames=32, max_clip_frames=64, max_frame_height=720,
           max_frame_width=1280, compute_dtype="bf16")
np.save(sys.argv[1], e.infer_clip(synth.make_frames(40, 720, 1280), synth.make_boxes(40, 720, 1280))["logp"])
e.close()
"""


def test_bf16_downsample_on_the_openers_centre_tap_is_bit_identical(tmp_path):
    """igemm_bf16.hip DS: the 1x1/2 downsample branch computed on the centre tap of the block's stride-2 opener (second
    accumulator set, second store) against the same branch as its own GEMM, the opener launched with the same tile and K
    split (PA_BF16_DS_FUSE=2): same products in the same order, so the log-probs are BIT-IDENTICAL -- partial tiles
    included (40 frames in backbone batches of 32 and 8). The knob is read once per process: two children."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for mode in ("2", "1"):
        f = str(tmp_path / f"logp_{mode}.npy")
        subprocess.run([sys.executable, "-c", _BF16_CHILD % root, f], check=True, timeout=300,
                       env=dict(os.environ, PA_BF16_DS_FUSE=mode))
        out[mode] = np.load(f)
    assert np.isfinite(out["1"]).all() and np.array_equal(out["1"], out["2"])


def test_streaming_chunks_and_feature_exchange(engine):
    """Chunked backbone + deferred head equals the one-shot clip; exported
    features re-imported into a fresh clip give the same records."""
    n, h, w = 48, 720, 1280
    frames = torch.from_numpy(synth.make_frames(n, h, w)).cuda()
    boxes = torch.from_numpy(synth.make_boxes(n, h, w)).cuda()
    ref = engine.infer_clip(frames, boxes)
    engine.clip_begin(n)
    from playaid_core_amd.engine import EngineError

    rec = engine.alloc_records(n - 1)
    lp = engine.alloc_logp(n - 1)
    engine.backbone_frames(frames[:20], boxes[:20], 0)
    with pytest.raises(EngineError) as ei:  # frame 21.. not cached yet
        engine.head_frames(1, 10, rec, lp)
    assert ei.value.code == -6
    engine.backbone_frames(frames[20:], boxes[20:], 20)
    engine.head_frames(1, 25, rec[:24], lp[:24])
    engine.head_frames(25, n, rec[24:], lp[24:])
    torch.cuda.synchronize()
    # tile / split-K are chosen per launch from the batch size, so a different chunking may
    # sum in a different order: equal to fp32 rounding, not bitwise
    assert (lp.cpu() - torch.from_numpy(ref["logp"])).abs().max() <= 1e-5
    feats = engine.features_export(0, n)
    engine.clip_begin(n)
    engine.features_import(0, feats)
    lp2 = engine.alloc_logp(n - 1)
    engine.head_frames(1, n, engine.alloc_records(n - 1), lp2)
    torch.cuda.synchronize()
    assert torch.equal(lp2.cpu(), lp.cpu())  # same features, same head launches: bitwise


def test_full_size_batch_properties(engine, state_dict):
    """BASELINE.json configs[1] size (64 x 1080p): determinism, per-crop
    independence, and oracle parity on a sampled subset of windows."""
    from oracle import cnn

    n, h, w = 64, 1080, 1920
    frames = synth.make_frames(n, h, w)
    boxes = synth.make_boxes(n, h, w)
    a = engine.infer_clip(frames, boxes, want_crops=True)
    b = engine.infer_clip(frames, boxes)
    assert np.array_equal(a["logp"], b["logp"])  # bitwise run-to-run (no atomics in reductions)
    assert (a["crop_status"] == 0).all() and np.isfinite(a["logp"]).all()
    assert np.allclose(np.exp(a["logp"]).sum(-1), 1.0, atol=1e-5)
    # a window's answer does not depend on what else is in the batch: run the first 40 frames alone
    c = engine.infer_clip(frames[:40], boxes[:40])
    assert np.abs(c["logp"][:12] - a["logp"][:12]).max() <= 1e-5  # frames 1..12 never reach past frame 39
    # oracle on three windows built from the GPU's own (bit-exact-tested) crops
    from playaid_core_amd.dataset_utils import action_sample_from_frame_middle_out

    for f, p in [(1, 0), (31, 1), (63, 0)]:
        idx = action_sample_from_frame_middle_out(f, 7, 3, n, min_frame=1)
        x = torch.from_numpy(np.stack([a["crops_rgb"][j - 1, p] for j in idx])).permute(0, 3, 1, 2)[None].float() / 255.0
        ref = cnn.forward(x, state_dict)[0].numpy()
        assert np.abs(ref - a["logp"][f - 1, p]).max() <= 1e-4


def test_profile_rows(engine):
    frames = synth.make_frames(8, 720, 1280)
    boxes = synth.make_boxes(8, 720, 1280)
    engine.profile_enable(True)
    engine.infer_clip(frames, boxes)
    rows = engine.profile_read()
    engine.profile_enable(False)
    names = {r["name"] for r in rows}
    assert {"preprocess_crops", "igemm_conv3x3", "stem_conv7x7_pool", "head_mlp_logsoftmax"} <= names
    conv = next(r for r in rows if r["name"] == "igemm_conv3x3")
    # sixteen convolutions + the three 1x1/2 branch GEMMs of layers 2-4 (whose 3x3 runs as Winograd since round 5); thirteen of
    # the launches execute 4/9 of their algorithmic multiply-adds
    assert conv["launches"] == 19 and conv["total_ms"] > 0 and conv["flops"] > 1e9
    assert 0.45 * conv["flops"] < conv["flops_executed"] < 0.60 * conv["flops"]


def test_two_stream_pipeline_equals_serial(engine):
    """Crop stage on a second stream into alternating slots (parallel.FrameParallelClip,
    pipeline=True): several back-to-back clips give bitwise the serial results."""
    from playaid_core_amd.parallel import FrameParallelClip

    runner = FrameParallelClip(engine, 7, 3)
    clips = []
    for seed in (7, 8, 9):
        n = 40
        f = torch.from_numpy(synth.make_frames(n, 720, 1280, seed=seed)).cuda()
        b = torch.from_numpy(synth.make_boxes(n, 720, 1280, first_frame=seed)).cuda()
        clips.append((f, b, n))
    torch.cuda.synchronize()
    serial = [runner.run(f, b, n, pipeline=False)[1].clone() for f, b, n in clips]
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):  # reuse of both slots across calls
        for f, b, n in clips:
            outs.append(runner.run(f, b, n, pipeline=True)[1].clone())
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert torch.equal(o, serial[i % 3])


def test_mixed_resolution_stream_with_hipgraph(engine, state_dict):
    """BASELINE.json configs[4]: 1080p/720p interleaved, bucketed batches, hipGraph replay."""
    from oracle import pipeline, yolo_crop
    from playaid_core_amd.stream_runner import MixedResolutionRunner

    n = 40
    res = [(1080, 1920) if (i % 3) != 1 else (720, 1280) for i in range(n)]
    frames = [synth.make_frame(i, h, w) for i, (h, w) in enumerate(res)]
    boxes = np.stack([[synth.fighter_box(i, p, *res[i]) for p in range(2)] for i in range(n)]).astype(np.float64)
    crops_ref = np.zeros((n, 2, 128, 128, 3), np.uint8)
    for i in range(n):
        for p in range(2):
            ok, c = yolo_crop.square_crop(frames[i], boxes[i, p], 128, padding=30)
            assert ok
            crops_ref[i, p] = yolo_crop.runner_input_from_crop(c)
    ref = pipeline.run_action_recognition(np.zeros((n, 1, 1, 3), np.uint8), boxes, state_dict, mode="cached", crops_rgb=crops_ref)
    # 32 frames = 64 crops per captured batch (the size from which the engine used to fork a side stream inside
    # the backbone; stem and max-pool are one kernel now, the captured sequence is a single stream)
    runner = MixedResolutionRunner(engine, batch_frames=32, use_graphs=True)
    got = runner.run(frames, boxes, want_crops=True)
    assert runner.captures == 2 and runner.replays == 1 + 1  # 27 frames @1080p -> 1 padded batch, 13 @720p -> 1
    assert np.array_equal(got["crops_rgb"], crops_ref)
    assert np.abs(got["logp"] - ref["logp"]).max() <= 1e-4
    assert np.array_equal(got["action_id"], ref["action_id"])
    # the second clip lands in each bucket's other staging slot (one more capture each); from the third
    # clip on only replays happen; eager mode agrees bitwise
    again = runner.run(frames, boxes)
    assert runner.captures == 4 and np.array_equal(again["logp"], got["logp"])
    third = runner.run(frames, boxes)
    assert runner.captures == 4 and runner.replays == 6 and np.array_equal(third["logp"], got["logp"])
    eager = MixedResolutionRunner(engine, batch_frames=32, use_graphs=False).run(frames, boxes)
    assert np.array_equal(eager["logp"], got["logp"])
    # steady-state form with the frames resident in HBM: same results, no host synchronisation inside
    by_shape = {}
    for i, (h, w) in enumerate(res):
        by_shape.setdefault((h, w), []).append(i)
    resident = {}
    for shape, idx in by_shape.items():
        idx = idx + [idx[-1]] * (-len(idx) % 32)
        resident[shape] = (torch.from_numpy(np.stack([frames[i] for i in idx])).cuda(),
                           torch.from_numpy(boxes[idx]).cuda(), torch.tensor(idx, dtype=torch.int32).cuda())
    rec, lp = engine.alloc_records(n - 1), engine.alloc_logp(n - 1)
    runner.run_resident(resident, n, rec, lp)
    torch.cuda.synchronize()
    assert runner.captures == 4 and np.array_equal(lp.cpu().numpy(), got["logp"])


@pytest.mark.parametrize("n_total", [40, 90])
def test_frame_parallel_hip_engine_two_ranks(engine, tmp_path, n_total):
    """BASELINE.json configs[3] in miniature on the real HIP engine: two ranks (sharing this box's one
    GPU, gloo transport) shard one clip, exchange the 27-frame feature halo and gather the records;
    compared with single-process infer_clip. n_total = 40: shards (20 frames) shorter than the reach,
    no interior frames at all; n_total = 90: 45-frame shards with interior frames whose head runs under
    the halo exchange. Rank 1 builds its engine from rank 0's broadcast weight arena."""
    import socket
    import subprocess
    import sys

    h, w = 720, 1280
    out = str(tmp_path / "two_rank.npz")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "two_rank_worker.py"), str(n_total), str(h), str(w), out]
    subprocess.run(cmd, check=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4"))
    got = np.load(out)
    single = engine.infer_clip(synth.make_frames(n_total, h, w), synth.make_boxes(n_total, h, w))
    assert got["logp"].shape == (n_total - 1, 2, 63)
    # the batch a crop travels in differs (shards of 20 / 45 in chunks of 16 vs one 64-chunked clip), so tiles
    # and split-K may differ: fp32 rounding, not bitwise
    assert np.abs(got["logp"] - single["logp"]).max() <= 1e-5
    assert np.array_equal(got["rec"][..., 1], single["action_id"])
    assert np.array_equal(got["rec"][..., 0], single["char_id"])
    assert np.array_equal(got["logp_p"], got["logp"]) and np.array_equal(got["rec_p"], got["rec"])  # pipelined == serial
    has_interior = (got["interior"][:, 1] > got["interior"][:, 0]).any()
    assert has_interior == (n_total == 90)


def test_rccl_world_size_one_runs_the_device_collectives(tmp_path):
    """RCCL itself, once: a FRESH child process (torch.distributed.run, one rank -- RCCL wants one GPU per rank and this box
    has one) calls init_process_group("nccl", device_id=...), parallel.broadcast_engine (the uint8 weight arena broadcast as a
    DEVICE tensor: the `_host_staged() == False` branch every gloo test skips) and FrameParallelClip.run (device
    all_gather_into_tensor of records and log-probabilities, the device barrier), serial and pipelined. The clip goes through
    the same 16-frame batches single-process infer_clip uses below, so the labels must be equal bit for bit. No scaling claim:
    none can be measured on one GPU."""
    import socket
    import subprocess
    import sys

    n_total, h, w = 48, 720, 1280
    out = str(tmp_path / "rccl_one_rank.npz")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "two_rank_worker.py"), str(n_total), str(h), str(w), out, "nccl"]
    env = dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    assert str(got["backend"]) == "nccl" and bool(got["arena_on_device"])
    from playaid_core_amd.engine import Engine

    eng16 = Engine(synth.make_state_dict(seed=1234), max_batch_frames=16, max_clip_frames=64, max_frame_height=h, max_frame_width=w)
    try:
        single = eng16.infer_clip(synth.make_frames(n_total, h, w), synth.make_boxes(n_total, h, w))
    finally:
        eng16.close()
    assert got["logp"].shape == (n_total - 1, 2, 63)
    assert np.array_equal(got["logp"], single["logp"]), np.abs(got["logp"] - single["logp"]).max()
    assert np.array_equal(got["rec"][..., 1], single["action_id"]) and np.array_equal(got["rec"][..., 0], single["char_id"])
    assert np.array_equal(got["logp_p"], got["logp"]) and np.array_equal(got["rec_p"], got["rec"])  # pipelined == serial


def test_indexed_backbone_rejects_frame_ids_outside_the_clip(engine):
    """a bad id must not become an out-of-bounds device write. The host path refuses it
    (pa_clip_mark_ready -> PA_ERR_CAPACITY); ids that only exist on the device are skipped by the
    scatter kernel and reported by pa_device_errors."""
    from playaid_core_amd import _lib
    from playaid_core_amd.engine import EngineError

    n, h, w = 4, 720, 1280
    fr = torch.from_numpy(synth.make_frames(n, h, w)).cuda()
    bx = torch.from_numpy(synth.make_boxes(n, h, w)).cuda()
    engine.clip_begin(8)
    with pytest.raises(EngineError) as ei:
        engine.clip_mark_ready([0, 1, 8])
    assert ei.value.code == _lib.PA_ERR_CAPACITY
    guard = engine.features_buffer(1)  # the row a wild id 8 would have hit first: cache rows 16, 17
    engine.clip_mark_ready(list(range(8)))
    before = engine.features_export(7, 1).clone()
    engine.backbone_frames_indexed(fr, bx, torch.tensor([0, 1, 8, -3], dtype=torch.int32).cuda())
    with pytest.raises(EngineError) as ei:
        engine.check_device_errors()
    assert ei.value.code == _lib.PA_ERR_CAPACITY and "2 frame id" in str(ei.value)
    engine.check_device_errors()  # the counter was cleared
    assert torch.equal(engine.features_export(7, 1), before)  # nothing was written for the bad ids
    # a caller's buffer for the export is checked before the library writes through its pointer
    with pytest.raises(ValueError):
        engine.features_export(0, 2, out=torch.empty((1, engine.F, 1024), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        engine.features_export(0, 1, out=torch.empty((1, engine.F, 1024), dtype=torch.float16, device="cuda"))
    mine = torch.empty((2, engine.F, 1024), dtype=torch.float32, device="cuda")
    assert engine.features_export(0, 2, out=mine) is mine and torch.equal(mine, engine.features_export(0, 2))
    assert engine.features_export(0, 2).abs().sum() > 0
    # features of a frame that is not cached in this clip cannot be exported (stale rows of an earlier clip)
    engine.clip_begin(8)
    with pytest.raises(EngineError) as ei:
        engine.features_export(0, 1)
    assert ei.value.code == _lib.PA_ERR_NOT_READY
    del guard


def test_repaired_gap_crops_come_from_their_source_frames(engine, state_dict):
    """pa_backbone_frames_src: crop (i, p) cut from frames[src[i, p]] in ONE pass == cutting each
    fighter column from its own re-indexed frame stack (what the runner did in two passes before)."""
    n, h, w = 12, 720, 1280
    frames = synth.make_frames(n, h, w)
    boxes = synth.make_boxes(n, h, w)
    src = np.tile(np.arange(n, dtype=np.int32)[:, None], (1, 2))
    src[4, 0], src[5, 0], src[9, 1] = 5, 6, 10  # repaired gaps read VideoCapture position j (one frame late)
    got = engine.infer_clip(frames, boxes, want_crops=True, src=src)
    for p in range(2):
        ref = engine.infer_clip(frames[src[:, p]], boxes, want_crops=True)
        assert np.array_equal(got["crops_rgb"][:, p], ref["crops_rgb"][:, p])
        assert np.array_equal(got["logp"][:, p], ref["logp"][:, p])
    bad = src.copy()
    bad[3, 1] = n  # outside the frame buffer: never dereferenced, reported per crop
    st = engine.infer_clip(frames, boxes, want_crops=True, src=bad)["crop_status"]
    assert st[3, 1] == 5 and (np.delete(st.ravel(), 3 * 2 + 1) == 0).all()


def test_log_projection_boxes(engine, tmp_path):
    """boxes from the game log on the device vs the literal numpy oracle."""
    from oracle import projection as oproj
    from playaid_core_amd import projection, timeline

    rng = np.random.default_rng(5)
    n = 400
    rows = np.zeros((n, 2, 9))
    rows[..., 0] = rng.uniform(-70, 70, (n, 2))          # pos_x
    rows[..., 1] = rng.uniform(-5, 45, (n, 2))           # pos_y
    rows[..., 2:5] = np.array([0.0, 15.8, 148.5]) + rng.normal(0, [8, 4, 25], (n, 1, 3))
    rows[..., 5:8] = np.array([0.0, 11.2, 0.0]) + rng.normal(0, [8, 4, 0], (n, 1, 3))
    rows[..., 8] = rng.choice([30.0, 50.0], (n, 1))
    got = engine.project_boxes(rows).cpu().numpy()
    for i in range(n):
        for p in range(2):
            r = rows[i, p]
            ref = oproj.project_box(r[0], r[1], list(r[2:5]), list(r[5:8]), r[8])
            assert tuple(got[i, p]) == ref, (i, p, got[i, p], ref)
    # the stub log of the plumbing config goes through the same path
    log = str(tmp_path / "stub.log")
    synth.make_stub_log(log, 16)
    tl = timeline.load_ground_truth_from_path(log)
    lr = projection.log_rows_from_timeline(tl)
    assert lr.shape == (16, 2, 9) and (lr[..., 8] == 50).all()
    boxes = engine.project_boxes(lr).cpu().numpy()
    d0 = tl[3][1]
    assert tuple(boxes[3, 1]) == oproj.project_box(d0["pos_x"], d0["pos_y"], list(d0["camera_position"].values()),
                                                    list(d0["camera_target_position"].values()), 50)


def test_fighter_kat_box_on_gpu(engine):
    """The camera / position of the reference-held fixture (fighter_test.py:9-28) through
    pa_project_boxes == the literal numpy oracle == the host Fighter mirror."""
    import json

    from oracle import projection as oproj
    from playaid_core_amd import projection
    from playaid_core_amd.fighter import Fighter

    k = json.load(open(os.path.join(GOLD, "fighter_kat.json")))
    data = dict(k["data"], **k["added_keys"])
    rows = projection.log_rows_from_timeline([[data]])
    got = tuple(engine.project_boxes(rows).cpu().numpy()[0, 0])
    want = oproj.project_box(data["pos_x"], data["pos_y"], list(data["camera_position"].values()),
                             list(data["camera_target_position"].values()), 50)
    assert got == want
    assert Fighter(frame_num=0, data=data).crop.yolo_crop() == want


def test_bf16_full_size_configs2_properties(state_dict):
    """BASELINE.json configs[2] at its full size (256 x 720p frames = 512 crops per backbone batch) -- far
    beyond what the CPU oracle finishes in seconds, so checked through properties: the bf16 path's crops are
    bit-identical to the fp32 engine's (whose parity with the oracle the small tests pin), its log-probs stay
    within the bf16 tolerance of the fp32 engine's on every one of the 510 windows, the run is bitwise
    repeatable (no atomics, fixed tile order), and chunking the clip into 4 x 64 frames changes nothing beyond
    that tolerance."""
    from playaid_core_amd.engine import Engine

    n, h, w = 256, 720, 1280
    frames = synth.make_frames_torch(n, h, w, device="cuda")
    boxes = torch.from_numpy(synth.make_boxes(n, h, w)).cuda()
    outs = {}
    for dt, mb in (("f32", 64), ("bf16", 256), ("bf16", 64)):
        eng = Engine(state_dict, max_batch_frames=mb, max_clip_frames=n, max_frame_height=h, max_frame_width=w, compute_dtype=dt)
        try:
            rec, lp = eng.alloc_records(n - 1), eng.alloc_logp(n - 1)
            crops = torch.empty((n, 2, 128, 128, 3), dtype=torch.uint8, device="cuda")
            st = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            eng.infer_clip_device(frames, boxes, rec, lp, crops, st)
            torch.cuda.synchronize()
            first = lp.clone()
            eng.infer_clip_device(frames, boxes, rec, lp, crops, st)
            torch.cuda.synchronize()
            assert torch.equal(first, lp), "not bitwise repeatable"
            assert (st == 0).all() and torch.isfinite(lp).all()
            outs[(dt, mb)] = (lp.cpu().numpy(), crops.cpu().numpy(), eng.decode_records(rec)["action_id"])
        finally:
            eng.close()
    ref_lp, ref_crops, ref_act = outs[("f32", 64)]
    for key in (("bf16", 256), ("bf16", 64)):
        lp, crops, act = outs[key]
        assert np.array_equal(crops, ref_crops)
        d = np.abs(lp - ref_lp)
        assert d.max() <= BF16_LOGP_TOL and d.max() > 1e-4, d.max()
        top2 = np.sort(ref_lp, axis=-1)[..., -2:]
        clear = (top2[..., 1] - top2[..., 0]) > 2 * BF16_LOGP_TOL
        assert clear.sum() > 100 and np.array_equal(act[clear], ref_act[clear])
    assert np.abs(outs[("bf16", 256)][0] - outs[("bf16", 64)][0]).max() <= BF16_LOGP_TOL


def test_clip_lanes_equal_single_engine(engine):
    """ClipLanes (independent clips alternating over two engines / streams, the second engine cloned from the
    first one's weight arena) returns bitwise what the single engine returns for every clip, whatever the lane,
    with clips of both lanes in flight at the same time."""
    from playaid_core_amd.parallel import ClipLanes

    n, h, w = 24, 720, 1280
    clips = []
    for seed in (3, 4, 5, 6, 7):
        f = torch.from_numpy(synth.make_frames(n, h, w, seed=seed)).cuda()
        b = torch.from_numpy(synth.make_boxes(n, h, w, first_frame=10 * seed)).cuda()
        clips.append((f, b))
    torch.cuda.synchronize()
    want = [engine.infer_clip(f, b)["logp"] for f, b in clips]
    lanes = ClipLanes(engine, 7, 3, lanes=2)
    try:
        assert len(lanes.engines) == 2 and lanes.engines[1] is not engine
        assert lanes.streams[0] is not lanes.streams[1]
        for rounds in range(2):
            if rounds == 1:
                # the second round on streams picked by measurement; a calibration leaves results unchanged
                rates = lanes.calibrate(clips[0][0], clips[0][1], n, clips=4)
                if rates:
                    assert lanes.calibration["picked"] == list(max(rates, key=rates.get))
                    assert all(v > 0 for v in rates.values())
                lanes.synchronize()
            pending = []
            for i, (f, b) in enumerate(clips):
                lane, rec, lp = lanes.submit(f, b, n)
                pending.append((i, lane, lp))
                if len(pending) == 2:  # both lanes busy: drain the older one before its lane is reused
                    j, lj, lpj = pending.pop(0)
                    lanes.streams[lj].synchronize()
                    assert np.array_equal(lpj.cpu().numpy(), want[j]), (rounds, j, lj)
            lanes.synchronize()
            for j, lj, lpj in pending:
                assert np.array_equal(lpj.cpu().numpy(), want[j])
    finally:
        lanes.close()


def test_clip_batch_equals_separate_clips(engine):
    """pa_clip_begin_batch: k independent clips run as ONE long clip through the backbone (more crops per launch)
    give every clip the records it gets alone (to fp32 rounding) -- windows are clamped to the clip's own frame
    numbers, never into a neighbour -- for clip lengths below and above the 27-frame reach of the window."""
    from playaid_core_amd.parallel import FrameParallelClip

    h, w = 720, 1280
    for L, k in ((20, 3), (40, 2)):
        clips = []
        for c in range(k):
            f = torch.from_numpy(synth.make_frames(L, h, w, seed=11 + c)).cuda()
            b = torch.from_numpy(synth.make_boxes(L, h, w, first_frame=7 * c)).cuda()
            clips.append((f, b))
        torch.cuda.synchronize()
        want = [engine.infer_clip(f, b) for f, b in clips]
        runner = FrameParallelClip(engine, 7, 3)
        frames = torch.cat([f for f, _ in clips])
        boxes = torch.cat([b for _, b in clips])
        rec, lp = runner.run(frames, boxes, L * k, gather=False, batch_of=k)
        torch.cuda.synchronize()
        lp = lp.cpu().numpy()
        assert lp.shape[0] == L * k - 1
        for c in range(k):
            got = lp[c * L: c * L + L - 1]
            # same windows, same weights; a launch over more crops picks other tiles / split-K factors, so the
            # sums differ in the last bits only (2e-6 here against the 1e-4 bar)
            assert np.abs(got - want[c]["logp"]).max() <= 1e-5, (L, k, c, np.abs(got - want[c]["logp"]).max())
            assert np.array_equal(got.argmax(-1), want[c]["logp"].argmax(-1))
        # the same frames as ONE clip differ near the seams: the batch flag is what keeps the clips apart
        rec1, lp1 = runner.run(frames, boxes, L * k, gather=False)
        torch.cuda.synchronize()
        assert np.abs(lp1.cpu().numpy()[L - 4: L - 1] - want[0]["logp"][L - 4: L - 1]).max() > 1e-3
    with pytest.raises(ValueError):
        engine.clip_begin(50, batch_of=3)


def test_runner_with_the_references_jpeg_round_trip(tmp_path, state_dict):
    """AIRunner's default (crop_jpeg_quality=95): the crops cut from frames take the reference's cv2.imwrite / cv2.imread
    round trip (ai_runner.py:420,446) before the CNN; labels equal the oracle pipeline fed with libjpeg-exact crops, and
    differ from the opt-out (crop_jpeg_quality=0) somewhere on the log-probabilities (the codec's loss is real)."""
    from oracle import jpeg, pipeline
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    n, h, w = 30, 720, 1280
    clip = ClipSource.synthetic(n, h, w)
    ckpt = str(tmp_path / "seeded.ckpt")
    synth.save_checkpoint(ckpt, seed=1234)
    model = CNNActionDetector.load_from_checkpoint(ckpt, actions=list(MOVE_TO_CLASS_ID.keys()), max_batch_frames=32,
                                                   max_clip_frames=64, max_frame_height=h, max_frame_width=w)
    plain = AIRunner(clip, model=model, output_dir=str(tmp_path / "plain"), crop_jpeg_quality=0, crop_mode="square")
    plain.run_action_recognition()
    lp_plain = plain._results["logp"].copy()
    runner = AIRunner(clip, model=model, output_dir=str(tmp_path / "jpeg"), crop_mode="square")
    assert runner.crop_jpeg_quality == 95
    runner.run_action_recognition()
    boxes = synth.make_boxes(n, h, w)
    crops, ok = pipeline.crops_for_clip(clip.frames, boxes)
    assert ok.all()
    crops_jpeg = np.stack([[jpeg.roundtrip(crops[i, f], 95) for f in range(2)] for i in range(n)])
    want = pipeline.run_action_recognition(clip.frames, boxes, state_dict, mode="cached", crops_rgb=crops_jpeg)
    res = runner._results
    assert np.array_equal(res["crops_rgb"], crops_jpeg)
    assert np.abs(res["logp"] - want["logp"]).max() <= 1e-4
    assert np.array_equal(res["action_id"], want["action_id"])
    assert np.abs(res["logp"] - lp_plain).max() > 1e-3
    # the option belongs to the runner's clip, not to the shared engine
    again, _ = model.engine.square_crops(clip.frames[:2], boxes[:2])
    assert np.array_equal(again[..., ::-1], crops[:2])


def test_golden_clip1080_on_gpu(engine):
    """BASELINE.json configs[0]/[1] data at full length: every one of the 254 windows of the committed 128-frame
    1080p golden clip (oracle output, tests/golden/make_golden.py) within 1e-4, identical labels; the backbone sees
    the clip in 64-frame batches (the engine's max_batch_frames), the head the whole clip."""
    z = np.load(os.path.join(GOLD, "clip1080_128_logp.npz"))
    n, h, w = 128, 1080, 1920
    assert engine.max_batch_frames == 64
    got = engine.infer_clip(synth.make_frames_torch(n, h, w, device="cuda"), synth.make_boxes(n, h, w))
    assert got["logp"].shape == z["logp"].shape == (127, 2, 63)
    assert (got["crop_status"] == 0).all()
    assert np.abs(got["logp"] - z["logp"]).max() <= 1e-4
    assert np.array_equal(got["action_id"], z["action_id"])
    want = yaml.safe_load(open(os.path.join(GOLD, "ai_output_128.yaml")))
    for p, fighter in enumerate(synth.FIGHTER_NAMES):
        for k in range(n - 1):
            assert want[fighter][k]["action"] == ACTIONS[int(got["action_id"][k, p])]
            assert want[fighter][k]["predicted_action_confidence"] == pytest.approx(float(got["prob"][k, p]) * 100.0, abs=1e-2)


def test_configs3_full_size_eight_virtual_ranks(state_dict):
    """BASELINE.json configs[3] at its full size on ONE GPU: the 8192-frame 1080p clip (device generator) processed as
    8 virtual ranks in one process -- shard_range / halo_plan / interior_frame_nums / owned_frame_nums exactly as
    FrameParallelClip.run uses them, the halo rows moved with features_export / features_import in place of the
    point-to-point transfers -- is bitwise repeatable, equals the one-shot clip to 1e-5 on every window, and agrees with
    the CPU oracle (<= 1e-4) on windows that straddle every one of the seven shard edges."""
    from oracle import cnn
    from playaid_core_amd.dataset_utils import action_sample_from_frame_middle_out
    from playaid_core_amd.engine import Engine
    from playaid_core_amd.parallel import halo_plan, interior_frame_nums, owned_frame_nums, shard_range

    N, h, w, world, S, delta = 8192, 1080, 1920, 8, 7, 3
    reach = delta * (S // 2) ** 2
    step = 256
    eng = Engine(state_dict, max_batch_frames=step, max_clip_frames=N, max_frame_height=h, max_frame_width=w)
    boxes = torch.from_numpy(synth.make_boxes(N, h, w)).cuda()
    buf = torch.empty((step, h, w, 3), dtype=torch.uint8, device="cuda")
    try:
        def backbone(lo, hi):
            for f0 in range(lo, hi, step):
                cnt = min(step, hi - f0)
                synth.make_frames_torch(cnt, h, w, first_frame=f0, device="cuda", out=buf[:cnt])
                eng.backbone_frames(buf[:cnt], boxes[f0:f0 + cnt], f0)

        # one shot: the whole clip on one engine (what `bench.py --clip-frames 8192` times)
        eng.clip_begin(N)
        backbone(0, N)
        rec1, lp1 = eng.alloc_records(N - 1), eng.alloc_logp(N - 1)
        eng.head_frames(1, N, rec1, lp1)
        torch.cuda.synchronize()

        def virtual_ranks():
            own = []
            for r in range(world):  # every rank: crops + backbone of its own shard only
                lo, hi = shard_range(N, world, r)
                eng.clip_begin(N)
                backbone(lo, hi)
                own.append(eng.features_export(lo, hi - lo))
            rec, lp = eng.alloc_records(N - 1), eng.alloc_logp(N - 1)
            for r in range(world):
                lo, hi = shard_range(N, world, r)
                eng.clip_begin(N)
                eng.features_import(lo, own[r])
                f_lo, f_hi = owned_frame_nums(N, world, r)
                i_lo, i_hi = interior_frame_nums(N, world, r, reach)
                assert i_hi - i_lo >= (hi - lo) - 2 * reach
                if i_hi > i_lo:  # the interior head runs before the halo has arrived
                    eng.head_frames(i_lo, i_hi, rec[i_lo - 1:], lp[i_lo - 1:])
                recvs, sends = halo_plan(N, world, r, reach)
                assert sorted(p for p, _, _ in recvs) == [q for q in (r - 1, r + 1) if 0 <= q < world]
                for peer, f0, cnt in recvs:
                    p_lo, _ = shard_range(N, world, peer)
                    assert (r, f0, cnt) in [(q, a, c) for q, a, c in halo_plan(N, world, peer, reach)[1]]  # the peer sends it
                    eng.features_import(f0, own[peer][f0 - p_lo: f0 - p_lo + cnt])
                for a, b in ((f_lo, i_lo), (i_hi, f_hi)):
                    if b > a:
                        eng.head_frames(a, b, rec[a - 1:], lp[a - 1:])
            torch.cuda.synchronize()
            return rec.cpu().numpy(), lp.cpu().numpy()

        rec_a, lp_a = virtual_ranks()
        rec_b, lp_b = virtual_ranks()
        assert np.array_equal(lp_a, lp_b) and np.array_equal(rec_a, rec_b)  # bitwise repeatable
        one = lp1.cpu().numpy()
        assert np.isfinite(one).all()
        # a shard's last backbone batch and the one-shot clip's batches differ in nothing here (both 256-frame
        # batches on 1024-frame shards), but the bar is the fp32-rounding one of the other chunking tests
        assert np.abs(lp_a - one).max() <= 1e-5
        assert np.array_equal(rec_a[..., 1], rec1.cpu().numpy()[..., 1])
        # oracle on windows that straddle each shard edge, built from the engine's (bit-exact-tested) crops
        for r in range(1, world):
            edge = shard_range(N, world, r)[0]  # first frame index of rank r; frame numbers edge, edge + 1 meet here
            for f, p in ((edge - 1, 0), (edge + 1, 1), (edge + 13, 0)):
                idx = action_sample_from_frame_middle_out(f, S, delta, N, min_frame=1)
                assert min(idx) <= edge < max(idx)  # the window reads both shards
                fr = torch.stack([synth.make_frames_torch(1, h, w, first_frame=j - 1, device="cuda")[0] for j in idx])
                crops, st = eng.square_crops(fr, boxes[[j - 1 for j in idx]], swap_rb=True)
                assert (st == 0).all()
                x = torch.from_numpy(crops[:, p]).permute(0, 3, 1, 2)[None].float() / 255.0
                ref = cnn.forward(x, state_dict)[0].numpy()
                assert np.abs(ref - lp_a[f - 1, p]).max() <= 1e-4, (r, f, p)
                assert int(ref.argmax()) == int(rec_a[f - 1, p, 1])
    finally:
        eng.close()
