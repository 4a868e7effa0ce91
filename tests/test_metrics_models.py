"""Scoring through the reference-shaped surface: ``validation_step`` / ``test_step`` / ``metrics`` of the three detector
mirrors, ``Engine.evaluate_clip`` / ``Engine.agreement`` and ``AIRunner.evaluate``, against the same figures computed on the
host from the very log-probabilities the device scored. Runs under both fp32 arithmetics (the shared ``engine`` fixture).

Tolerances: integers (rows, correct, ignored, confusion) are exact. The device's loss is a float64 sum of ``rows`` terms
(error <= rows * 2**-53 * sum|term|, tests/test_metrics.py) divided once; ``F.nll_loss`` on float32 rounds its mean in fp32,
hence ``rows * 2**-24 * max|logp|`` where torch is the other side."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from playaid_core_amd import synth
from playaid_core_amd.anim_ontology import ACTIONS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "ground_truth_sample.csv")
A = len(ACTIONS)


def _inputs(b, s, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(b, s, 3, 128, 128)).astype(np.float32) / 255.0)


def _host_figures(logp, y):
    """logp float32[rows, A], y int[rows] (-100 = ignored) -> what metrics.finish must say, in float64."""
    logp, y = np.asarray(logp, np.float32).reshape(-1, logp.shape[-1]), np.asarray(y).reshape(-1)
    ok = y != -100
    pred = logp.argmax(axis=1)
    terms = -logp[ok, y[ok]].astype(np.float64)
    cm = np.zeros((logp.shape[1], logp.shape[1]), np.int64)
    np.add.at(cm, (y[ok], pred[ok]), 1)
    rows = int(ok.sum())
    return dict(rows=rows, ignored=int((~ok).sum()), correct=int((pred[ok] == y[ok]).sum()), cm=cm, loss=math.fsum(terms) / rows,
                loss_bar=2.0 ** -53 * math.fsum(np.abs(terms)) + 2.0 ** -52 * abs(math.fsum(terms) / rows),
                conf=100.0 * math.fsum(np.exp(logp[ok, pred[ok]].astype(np.float64))) / rows)


def _same(out, want, where):
    print(f"{where}: rows={out['rows']} loss={out['loss']!r} want={want['loss']!r} bar={want['loss_bar']:.3e}")
    assert out["rows"] == want["rows"] and out["ignored"] == want["ignored"], where
    assert np.array_equal(out["confusion"], want["cm"]), where
    assert out["accuracy"] == want["correct"] / want["rows"], where
    assert abs(out["loss"] - want["loss"]) <= want["loss_bar"], where
    # one ulp for each side's exp on top of the summation bound, times the 100 / rows of the finishing step
    assert abs(out["mean_confidence"] - want["conf"]) <= (want["rows"] + 6) * 2.0 ** -52 * want["conf"], where


def _labels_with_centre(centre, s, num_actions):
    """[B, S] labels whose centre column is `centre` and every other column another value: only the centre may be scored."""
    centre = torch.as_tensor(centre, dtype=torch.int64)
    lab = ((centre + 1) % num_actions)[:, None].repeat(1, s)
    lab[:, s // 2] = centre
    return lab


def test_cnn_detector_steps_score_the_centre_label(engine, state_dict):
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    model = CNNActionDetector(ACTIONS, state_dict=state_dict, max_batch_frames=32, max_clip_frames=64, compute_dtype=engine.compute_dtype).eval()
    try:
        s = model.sequence_length
        assert s == 7
        x1, x2 = _inputs(3, s, seed=31), _inputs(3, s, seed=32)
        lp1, lp2 = model(x1), model(x2)
        assert not lp1.is_cuda and lp1.shape == (3, A)
        y1 = torch.tensor([int(lp1[0].argmax()), (int(lp1[1].argmax()) + 5) % A, 17])   # a hit, a miss, whatever 17 is
        y2 = torch.tensor([int(lp2[0].argmax()), int(lp2[1].argmax()), (int(lp2[2].argmax()) + 1) % A])
        b1 = (x1, torch.full((3,), 2), _labels_with_centre(y1, s, A), [{}] * 3)
        b2 = (x2, torch.full((3,), 3), _labels_with_centre(y2, s, A), [{}] * 3)
        assert model.test_step(b1, 0) is None                    # as the reference: nothing returned, nothing read back
        out = model.metrics("test")
        want = float(F.nll_loss(lp1, y1))
        bar = 3 * 2.0 ** -24 * float(lp1.abs().max())
        print(f"cnn test_step: loss={out['test_action_loss']!r} torch={want!r} bar={bar:.3e}")
        assert abs(out["test_action_loss"] - want) <= bar
        assert out["test_action_acc"] == (lp1.argmax(1) == y1).numpy().mean()
        assert out["loss"] == out["test_action_loss"] and out["accuracy"] == out["test_action_acc"]
        _same(out, _host_figures(lp1.numpy(), y1.numpy()), "cnn one step")
        # a second step accumulates: the epoch's figures are those of the six rows (Lightning's batch-weighted mean)
        model.test_step(b2, 1)
        out = model.metrics("test")
        both_lp, both_y = torch.cat([lp1, lp2]), torch.cat([y1, y2])
        assert abs(out["test_action_loss"] - float(F.nll_loss(both_lp, both_y))) <= 6 * 2.0 ** -24 * float(both_lp.abs().max())
        assert out["test_action_acc"] == int((both_lp.argmax(1) == both_y).sum()) / 6 and out["rows"] == 6
        _same(out, _host_figures(both_lp.numpy(), both_y.numpy()), "cnn two steps")
        # the splits are separate states; a device batch is taken as well
        assert model.metrics("val")["rows"] == 0 and math.isnan(model.metrics("val")["val_action_loss"])
        model.validation_step((x1.cuda(), b1[1], b1[2].cuda(), b1[3]), 0)
        val = model.metrics("val")
        assert val["rows"] == 3 and val["val_action_acc"] == int((lp1.argmax(1) == y1).sum()) / 3
        assert model.metrics("test")["rows"] == 6
        model.reset_metrics("test")
        assert model.metrics("test")["rows"] == 0 and model.metrics("val")["rows"] == 3
        model.reset_metrics()
        assert model.metrics("val")["rows"] == 0
        with pytest.raises(ValueError):
            model.metrics("train")
    finally:
        model.engine.close()


def _flat_model_steps(model, s, where):
    """RNNActionDetector / ResnetTransformerDetector: the reference scores every (window, frame) row against the flattened
    labels (rnn_action_detector.py:132-160, resnet_transformer_detector.py:179-205)."""
    x = _inputs(2, s, seed=41)
    lp = model(x).reshape(-1, A)
    assert not lp.is_cuda and lp.shape == (2 * s, A)
    pred = lp.argmax(1)
    y = (pred + torch.arange(2 * s) % 3) % A          # every third row a hit, the others one or two classes off
    batch = (x, torch.zeros(2, dtype=torch.int64), y.reshape(2, s), [{}] * 2)
    assert model.test_step(batch, 0) is None
    out = model.metrics("test")
    want = float(F.nll_loss(lp, y))
    bar = 2 * s * 2.0 ** -24 * float(lp.abs().max())
    print(f"{where} test_step: loss={out['test_action_loss']!r} torch={want!r} bar={bar:.3e}")
    assert abs(out["test_action_loss"] - want) <= bar
    assert out["test_action_acc"] == int((pred == y).sum()) / (2 * s)
    _same(out, _host_figures(lp.numpy(), y.numpy()), where + " one step")
    model.validation_step(batch, 0)
    model.test_step(batch, 1)
    out = model.metrics("test")
    assert out["rows"] == 4 * s and out["test_action_acc"] == int((pred == y).sum()) / (2 * s)
    _same(out, _host_figures(torch.cat([lp, lp]).numpy(), torch.cat([y, y]).numpy()), where + " two steps")
    assert model.metrics("val")["rows"] == 2 * s
    model.reset_metrics("test")
    assert model.metrics("test")["rows"] == 0 and model.metrics("val")["rows"] == 2 * s


def test_rnn_detector_steps(engine):
    from playaid_core_amd.rnn_action_detector import RNNActionDetector

    sd = synth.make_rnn_state_dict(seed=4321, num_actions=A)
    model = RNNActionDetector("byleth", [f"a{i}" for i in range(A)], state_dict=sd, max_rows=64, compute_dtype=engine.compute_dtype).eval()
    try:
        _flat_model_steps(model, 7, "rnn")
    finally:
        model.close()


def test_resformer_detector_steps(engine):
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    sd = synth.make_resformer_state_dict(seed=2468, num_actions=A, sequence_length=7)
    model = ResnetTransformerDetector([f"a{i}" for i in range(A)], sequence_length=7, state_dict=sd, max_rows=70,
                                      compute_dtype=engine.compute_dtype).eval()
    try:
        _flat_model_steps(model, 7, "resformer")
    finally:
        model.close()


def test_engine_evaluate_clip_and_agreement(engine):
    from playaid_core_amd.ai_runner import ClipSource
    from playaid_core_amd.metrics import EvalState

    n, h, w = 24, 270, 480
    clip = ClipSource.synthetic(n, h, w)
    boxes = synth.make_boxes(n, h, w)
    base = engine.infer_clip(clip.frames, boxes)
    assert np.array_equal(base["logp"].argmax(2), base["action_id"])
    labels = base["action_id"].astype(np.int32).copy()
    flat = labels.reshape(-1)
    flat[::5] = (flat[::5] + 1) % A
    flat[[3, 40]] = -100
    out = engine.evaluate_clip(clip.frames, boxes, labels)
    want = _host_figures(base["logp"], labels)
    assert want["rows"] == (n - 1) * 2 - 2 and want["ignored"] == 2 and 0 < want["correct"] < want["rows"]
    _same(out, want, "evaluate_clip")
    for k in ("char_id", "action_id", "prob", "status", "crop_status"):   # the records are bitwise infer_clip's
        assert np.array_equal(out["records"][k], base[k]), k
    # a state handed in keeps accumulating across clips
    with EvalState(A, engine.device) as st:
        engine.evaluate_clip(clip.frames, boxes, labels, state=st)
        twice = engine.evaluate_clip(clip.frames, boxes, labels, state=st)
    assert twice["rows"] == 2 * want["rows"] and np.array_equal(twice["confusion"], 2 * want["cm"])
    with pytest.raises(ValueError):
        engine.evaluate_clip(clip.frames, boxes, labels[:-1])
    # agreement of a run with itself: its own action_id, read in place from the records, as the labels
    fd = torch.from_numpy(clip.frames).to(engine.device)
    bd = torch.from_numpy(boxes).double().to(engine.device)
    records, logp = engine.alloc_records(n - 1), engine.alloc_logp(n - 1)
    engine.infer_clip_device(fd, bd, records, logp)
    agree = engine.agreement(records, logp)
    assert agree["accuracy"] == 1.0 and agree["rows"] == (n - 1) * 2 and agree["ignored"] == 0
    assert np.array_equal(agree["confusion"], np.diag(np.bincount(base["action_id"].reshape(-1), minlength=A)))
    # ... and against labels shifted by one class nothing agrees, every count one column to the right of the diagonal
    shifted = records.clone()
    shifted[..., 1] = (shifted[..., 1] + A - 1) % A
    off = engine.agreement(shifted, logp)
    assert off["accuracy"] == 0.0 and np.array_equal(off["confusion"], np.roll(agree["confusion"], -1, axis=0))


def _runner_figures(runner, table):
    """The same figures from run_action_recognition's outputs (ai_output_data: action names and confidences) + the clip's logp."""
    runner.run_action_recognition(overwrite=True)
    names = runner.model.actions
    rows = correct = 0
    conf = []
    cm = np.zeros((len(names), len(names)), np.int64)
    for p, fighter in enumerate(runner.fighters):
        for f in range(1, runner.max_frames):
            rec = runner.ai_output_data[fighter][f - 1]
            y = int(table[f - 1, p])
            if y == -100:
                continue
            rows += 1
            correct += names.index(rec.action) == y
            cm[y, names.index(rec.action)] += 1
            conf.append(rec.predicted_action_confidence)
    return rows, correct, cm, math.fsum(conf) / rows


def test_runner_evaluate_with_action_strings_and_with_a_ground_truth_csv(engine, state_dict, tmp_path):
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.ult_action_dataset import label_table

    names = ACTIONS[:-1] + ["Unknown"]   # a list with the dataset's fall-back class in it
    model = CNNActionDetector(names, state_dict=state_dict, max_batch_frames=32, max_clip_frames=64, max_frame_height=270,
                              max_frame_width=480, compute_dtype=engine.compute_dtype).eval()
    try:
        # per-fighter action strings, the shape ClipWindowDataset takes; the square-crop mode
        runner = AIRunner(ClipSource.synthetic(24, 270, 480), model=model, output_dir=str(tmp_path / "a"), crop_mode="square")
        res = runner._run_clip()
        gt = [[names[int(res["action_id"][f, p])] if (f + p) % 3 else names[(f * 7 + p) % A] for f in range(runner.max_frames - 1)]
              for p in range(2)]
        gt[1][4] = None                    # an unlabelled frame
        gt[0][9] = "NotAMove"              # outside the list -> "Unknown"
        out = runner.evaluate(actions=gt)
        table = label_table(runner, gt, names)
        assert np.array_equal(out["labels"], table) and table[4, 1] == -100 and table[9, 0] == A - 1
        want = _host_figures(res["logp"][: runner.max_frames - 1], table)
        _same(out, want, "runner actions=")
        rows, correct, cm, conf = _runner_figures(runner, table)
        assert (out["rows"], out["ignored"]) == (rows, 1) and out["accuracy"] == correct / rows and np.array_equal(out["confusion"], cm)
        # (the runner's confidence is the record's float32 exp: <= 2.5 ulp of fp32 away from the float64 one, times 100)
        assert abs(out["mean_confidence"] - conf) <= 100 * 2.5 * 2.0 ** -24
        with pytest.raises(ValueError):
            runner.evaluate()              # this clip carries no ground truth of its own
        with pytest.raises(ValueError):
            runner.evaluate(actions=gt, ground_truth_csv=CSV)

        # a hand-labelled clip: boxes from the CSV (no detector), the runner's default crop mode, Joker's frame 4 unlabelled
        clip = ClipSource.from_ground_truth(synth.make_frames(6, 270, 480), CSV, name="gt")
        runner = AIRunner(clip, model=model, output_dir=str(tmp_path / "b"))
        assert runner.fighters == ["Pikachu", "Joker"] and runner.max_frames == 6
        out = runner.evaluate()
        table = out["labels"]
        assert table.shape == (5, 2) and table[4, 1] == -100 and table[2, 1] == A - 1 and table[0, 0] == names.index("Jab")
        want = _host_figures(runner._run_clip()["logp"][:5], table)
        _same(out, want, "runner csv")
        rows, correct, cm, conf = _runner_figures(runner, table)
        assert (out["rows"], out["ignored"]) == (rows, 1) == (9, 1)
        assert out["accuracy"] == correct / rows and np.array_equal(out["confusion"], cm)
        assert abs(out["mean_confidence"] - conf) <= 100 * 2.5 * 2.0 ** -24
        again = runner.evaluate(ground_truth_csv=CSV)
        assert np.array_equal(again["labels"], table) and again["loss"] == out["loss"] and np.array_equal(again["confusion"], cm)
    finally:
        model.engine.close()
