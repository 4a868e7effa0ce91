"""Scoring without a GPU: the ``pa_eval_*`` bindings and their argument checks, the float64 finishing arithmetic
(``metrics.finish`` / ``metrics.merge``) on hand-written totals, and the ground-truth CSV -> label table path."""
import ctypes
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "ground_truth_sample.csv")


@pytest.fixture(scope="module")
def lib():
    from playaid_core_amd import _build, _lib

    _build.build()
    return _lib.load()


def test_eval_symbols_are_bound_and_the_struct_matches_the_header(lib):
    from playaid_core_amd import _lib

    for name in ("pa_eval_create", "pa_eval_destroy", "pa_eval_reset", "pa_eval_update", "pa_eval_read"):
        assert hasattr(lib, name) and name in {s[0] for s in _lib.SYMBOLS}
    assert ctypes.sizeof(_lib.pa_eval_totals) == 48
    assert [f[0] for f in _lib.pa_eval_totals._fields_] == ["rows", "correct", "ignored", "bad_labels", "nll_sum", "conf_sum"]
    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    assert "#define PA_ABI_VERSION 15" in hdr and lib.pa_abi_version() == 15   # append only: nothing existing changed layout
    assert "#define PA_EVAL_IGNORE (-100)" in hdr and _lib.PA_EVAL_IGNORE == -100
    assert "PA_ERR_BAD_LABELS = %d" % _lib.PA_ERR_BAD_LABELS in hdr
    assert b"labels" in lib.pa_status_string(_lib.PA_ERR_BAD_LABELS)
    assert lib.pa_status_string(_lib.PA_ERR_BAD_LABELS) != lib.pa_status_string(-99)


def test_eval_handle_rejects_bad_arguments_without_gpu(lib):
    """pa_eval_create / pa_eval_update check their arguments before any device call; a create that stops at the device (none
    here) still hands back a handle that carries num_actions, so every rejection of pa_eval_update is reachable."""
    from playaid_core_amd import _lib

    bad = _lib.PA_ERR_INVALID_ARG
    h = ctypes.c_void_p(0)
    assert lib.pa_eval_create(0, 5, None) == bad
    for a in (0, -3):
        assert lib.pa_eval_create(0, a, ctypes.byref(h)) == bad and not h
    assert lib.pa_eval_create(-1, 5, ctypes.byref(h)) == bad and not h
    x = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused first
    z = ctypes.c_void_p(0)
    tot = _lib.pa_eval_totals()
    assert lib.pa_eval_update(None, x, 5, 1, x, 1, None) == bad
    assert lib.pa_eval_reset(None, None) == bad
    assert lib.pa_eval_read(None, ctypes.byref(tot), None, None) == bad
    lib.pa_eval_destroy(None)   # a null handle is ignored
    rc = lib.pa_eval_create(0, 5, ctypes.byref(h))
    assert rc in (_lib.PA_OK, _lib.PA_ERR_NO_DEVICE, _lib.PA_ERR_HIP) and h, rc
    try:
        assert lib.pa_eval_update(h, z, 5, 1, x, 1, None) == bad       # null logp
        assert lib.pa_eval_update(h, x, 5, 1, z, 1, None) == bad       # null labels
        assert lib.pa_eval_update(h, x, 4, 1, x, 1, None) == bad       # ld < A
        assert lib.pa_eval_update(h, x, 5, -1, x, 1, None) == bad      # n < 0
        assert lib.pa_eval_update(h, x, 5, 1, x, 0, None) == bad       # label_stride < 1
        assert lib.pa_eval_update(h, x, 5, 1, x, -4, None) == bad
        assert lib.pa_eval_read(h, None, None, None) == bad            # null totals
        if rc != _lib.PA_OK:   # no device: what passes the checks stops there, before anything is launched
            assert lib.pa_eval_update(h, x, 5, 1, x, 1, None) == _lib.PA_ERR_NO_DEVICE
            assert lib.pa_eval_reset(h, None) == _lib.PA_ERR_NO_DEVICE
            assert lib.pa_eval_read(h, ctypes.byref(tot), None, None) == _lib.PA_ERR_NO_DEVICE
    finally:
        lib.pa_eval_destroy(h)


def _totals(rows, correct, ignored, nll, conf, bad=0):
    return dict(rows=rows, correct=correct, ignored=ignored, bad_labels=bad, nll_sum=nll, conf_sum=conf)


def test_finish_on_hand_written_totals():
    from playaid_core_amd import _lib, metrics

    # 3 x 3 by hand: class 0 has 4 rows (3 right, 1 taken for class 2), class 1 has none, class 2 has 2 rows (1 right, 1 for class 0)
    cm = np.array([[3, 0, 1], [0, 0, 0], [1, 0, 1]], dtype=np.int64)
    out = metrics.finish(_totals(6, 4, 2, 3.0, 4.5), cm)
    assert out["loss"] == 0.5 and out["accuracy"] == 4 / 6 and out["mean_confidence"] == 75.0
    assert out["rows"] == 6 and out["ignored"] == 2
    np.testing.assert_array_equal(out["confusion"], cm)
    np.testing.assert_array_equal(out["confusion_normalized"], np.array([[0.75, 0, 0.25], [0, 0, 0], [0.5, 0, 0.5]]))
    assert out["confusion_normalized"].dtype == np.float64
    pc = out["per_class_accuracy"]
    assert pc[0] == 0.75 and math.isnan(pc[1]) and pc[2] == 0.5          # a class with no rows: NaN, its matrix row all zero
    # the ctypes struct is taken as well as a dict
    t = _lib.pa_eval_totals(6, 4, 2, 0, 3.0, 4.5)
    again = metrics.finish(t, cm)
    assert again["loss"] == 0.5 and again["accuracy"] == 4 / 6
    # every row ignored: NaN figures, no exception, no warning turned error
    with np.errstate(all="raise"):
        out = metrics.finish(_totals(0, 0, 9, 0.0, 0.0), np.zeros((3, 3), np.int64))
    assert math.isnan(out["loss"]) and math.isnan(out["accuracy"]) and math.isnan(out["mean_confidence"])
    assert out["rows"] == 0 and out["ignored"] == 9 and not out["confusion_normalized"].any()
    assert np.isnan(out["per_class_accuracy"]).all()


def test_merge_of_a_split_equals_the_whole():
    from playaid_core_amd import metrics

    rng = np.random.default_rng(5)
    a_cm, b_cm, c_cm = (rng.integers(0, 50, (4, 4)).astype(np.int64) for _ in range(3))
    # (dyadic sums: adding the parts is exact whatever the order)
    a = _totals(int(a_cm.sum()), int(np.trace(a_cm)), 3, 10.25, 7.5)
    b = _totals(int(b_cm.sum()), int(np.trace(b_cm)), 0, 0.125, 2.0, bad=1)
    c = _totals(int(c_cm.sum()), int(np.trace(c_cm)), 5, 4.0, 0.5)
    tot, cm = metrics.merge([(a, a_cm), (b, b_cm), (c, c_cm)])
    whole_cm = a_cm + b_cm + c_cm
    assert tot == _totals(int(whole_cm.sum()), int(np.trace(whole_cm)), 8, 14.375, 10.0, bad=1)
    np.testing.assert_array_equal(cm, whole_cm)
    whole = metrics.finish(tot, cm)
    assert whole["accuracy"] == np.trace(whole_cm) / whole_cm.sum() and whole["loss"] == 14.375 / whole_cm.sum()
    one, one_cm = metrics.merge([(a, a_cm)])
    assert one == a and np.array_equal(one_cm, a_cm) and one_cm is not a_cm
    with pytest.raises(ValueError):
        metrics.merge([])
    with pytest.raises(ValueError):
        metrics.merge([(a, a_cm), (b, np.zeros((3, 3), np.int64))])


def test_ground_truth_csv_and_label_table():
    from playaid_core_amd.ai_runner import ClipSource
    from playaid_core_amd.anim_ontology import ACTIONS
    from playaid_core_amd.ult_action_dataset import label_table, load_ground_truth_labels

    labels, action_to_frames = load_ground_truth_labels(CSV)
    assert sorted(labels) == ["Joker", "Pikachu"]
    assert sorted(labels["Pikachu"]) == [0, 1, 2, 3, 4, 5] and sorted(labels["Joker"]) == [0, 1, 2, 3, 5]   # Joker has no frame 4
    assert labels["Joker"][3] == (3, "Joker", "DownTilt", 0.878584, 0.443256, 0.153290, 0.294113)
    assert dict(action_to_frames["Pikachu"]) == {"Jab": [0, 1], "DashAttack": [2, 3], "ForwardTilt": [4, 5]}
    assert dict(action_to_frames["Joker"]) == {"UpSmash": [0, 1], "NotAMove": [2], "DownTilt": [3], "Jab": [5]}
    # lines=: 1-based file lines, the header never counts (ult_action_dataset.py:525)
    some, a2f = load_ground_truth_labels(CSV, lines={1, 2, 3, 7})
    assert {k: sorted(v) for k, v in some.items()} == {"Pikachu": [0], "Joker": [0, 2]} and dict(a2f["Joker"]) == {"UpSmash": [0], "NotAMove": [2]}
    assert load_ground_truth_labels(CSV, lines=set()) == ({}, {})

    animations = ACTIONS[:-1] + ["Unknown"]
    jab, dash, ftilt, dtilt, usmash = (animations.index(a) for a in ("Jab", "DashAttack", "ForwardTilt", "DownTilt", "UpSmash"))
    tab = label_table(["Pikachu", "Joker"], labels, animations)
    assert tab.dtype == np.int32 and tab.shape == (6, 2)
    assert tab[:, 0].tolist() == [jab, jab, dash, dash, ftilt, ftilt]
    assert tab[:, 1].tolist() == [usmash, usmash, 62, dtilt, -100, jab]     # outside the list -> "Unknown"; a missing frame -> -100
    assert label_table(["Joker", "Pikachu"], labels, animations)[:, 0].tolist() == tab[:, 1].tolist()   # columns follow the slot order
    assert label_table(["Pikachu", "Joker"], labels, animations, n_rows=4).tolist() == tab[:4].tolist()
    shifted = label_table(["Pikachu", "Joker"], labels, animations, first_frame=2)
    assert shifted.tolist() == tab[2:].tolist()
    with pytest.raises(ValueError):
        label_table(["Pikachu", "Joker"], labels, ACTIONS)    # the 63-class ontology has no "Unknown" to fall back on

    # per-fighter strings, the shape ClipWindowDataset takes, through a runner-like object (fighters, max_frames)
    class R:
        fighters = ["Pikachu", "Joker"]
        max_frames = 5

    strings = [["Jab", "Jab", None, "Nope"], ["UpSmash"] * 4]
    got = label_table(R, strings, animations)
    assert got.tolist() == [[jab, usmash], [jab, usmash], [-100, usmash], [62, usmash]]
    assert label_table(R, labels, animations).tolist() == tab[:4].tolist()

    # the clip with boxes given: label text per frame from the CSV's boxes, nothing for what the CSV does not list
    clip = ClipSource.from_ground_truth(np.zeros((7, 8, 8, 3), np.uint8), CSV, name="gt")
    assert clip.name == "gt" and len(clip.labels) == 7
    assert clip.labels[0] == "2 0.163299 0.637705 0.128906 0.278391 1.0\n3 0.609912 0.271628 0.13757 0.267016 1.0\n"
    assert clip.labels[4] == "2 0.428866 0.906557 0.140519 0.294483 1.0\n" and clip.labels[6] == ""
    assert clip.ground_truth["Joker"] == {0: "UpSmash", 1: "UpSmash", 2: "NotAMove", 3: "DownTilt", 5: "Jab"}
    assert label_table(["Pikachu", "Joker"], clip.ground_truth, animations).tolist() == tab.tolist()


def test_models_and_engine_expose_the_scoring_surface():
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.engine import Engine
    from playaid_core_amd.metrics import EvalState
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector
    from playaid_core_amd.rnn_action_detector import RNNActionDetector

    for cls in (CNNActionDetector, RNNActionDetector, ResnetTransformerDetector):
        for name in ("validation_step", "test_step", "metrics", "reset_metrics"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert callable(Engine.evaluate_clip) and callable(Engine.agreement)
    assert callable(AIRunner.evaluate) and callable(ClipSource.from_ground_truth)
    for name in ("update", "reset", "totals", "compute", "__enter__", "__exit__"):
        assert callable(getattr(EvalState, name))
