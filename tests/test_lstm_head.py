"""The recurrent head (``pa_lstm_create`` / ``pa_lstm_forward``, csrc/lstm.hip) against a float64 recurrence, on device
features the test supplies (rows of LD = 1024 floats, NaN past input_dim, as the mirror's feature stride), so the head is
checked apart from the backbone. Weights, bar and its derivation: tests/helpers/lstm_head.py.

What the cases reach: the served shape (64 windows x 7 frames, 448 rows) runs the input projections of layers 1-2 on the
matrix-core GEMM (rows >= 64, K = 512) and the persistent kernel's granule hand-off for 64 steps; rows 63 / 64 / 65 sit on
the projection's switch; input 512 takes layer 0 onto the matrix cores too; H 200 and H 8 run the vector U = 4 kernel
(H % 64 != 0); 520 steps of batch 1 run the hand-off past 512 steps. The knob children force the per-step kernel
(PA_LSTM_STEPS=1), the vector form at H 512 (PA_LSTM_MFMA=0) and 1 / 2 / 8 units per workgroup (PA_LSTM_UNITS), each
against float64 and each with its forms asserted from ``pa_lstm_layer_forms``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import lstm_head as lh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# forms at the default knobs: matrix-core recurrence where H % 64 == 0, the vector U = 4 kernel elsewhere
DEFAULT_FORM = {512: "mfma", 200: "u4", 8: "u4"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(lh.CASES))
def test_lstm_head_against_float64(name):
    r, forms, _ = lh.run_case(name)
    hidden, layers = lh.CASES[name][1], lh.CASES[name][2]
    assert forms == [DEFAULT_FORM[hidden]] * layers, f"{name}: forms {forms}"
    print(f"lstm {name}: {r:.3f} of the {lh.BAR:g} bar, forms {forms}")


KNOB_CASES = "served 64x7,batch 16,rows 65,H 200,1 window"


@pytest.mark.gpu
@pytest.mark.parametrize("knob, want", [
    ({"PA_LSTM_STEPS": "1"}, {512: "steps", 200: "steps"}),
    ({"PA_LSTM_MFMA": "0"}, {512: "u4", 200: "u4"}),
    ({"PA_LSTM_UNITS": "1"}, {512: "u1", 200: "u1"}),
    ({"PA_LSTM_UNITS": "2"}, {512: "u2", 200: "u2"}),
    ({"PA_LSTM_UNITS": "8"}, {512: "u8", 200: "u8"}),
], ids=["steps", "mfma0", "units1", "units2", "units8"])
def test_lstm_knob_forms_against_float64(knob, want):
    env = dict(os.environ, **knob)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "lstm_knob_worker.py"), KNOB_CASES],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"{knob}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for name, v in res.items():
        hidden, layers = lh.CASES[name][1], lh.CASES[name][2]
        assert v["forms"] == [want[hidden]] * layers, f"{knob} {name}: forms {v['forms']}"
        assert v["ratio"] <= 1.0
    print(f"{knob}: " + ", ".join(f"{k} {v['ratio']:.3f}" for k, v in res.items()))


@pytest.mark.gpu
def test_second_call_equals_a_fresh_handle():
    """No h or c state leaks from one call into the next: a call after another on the same handle (with a different batch
    and more steps first) gives the same bits as the same call on a fresh handle."""
    input_dim, hidden, layers, actions = 300, 512, 3, 63
    w = lh.make_weights(input_dim, hidden, layers, actions, 5)
    first = lh.make_features(20, 9, input_dim, 6)
    second = lh.make_features(12, 7, input_dim, 7)
    a = lh.Head(input_dim, hidden, layers, actions, 256, w)
    b = lh.Head(input_dim, hidden, layers, actions, 256, w)
    try:
        a.forward(first)
        got = a.forward(second)
        fresh = b.forward(second)
    finally:
        a.close()
        b.close()
    assert np.array_equal(got, fresh)
    assert lh.ratio(fresh, lh.reference(second, w, input_dim, layers)) <= 1.0


# -- the comparator itself (CPU) ------------------------------------------------------------------------
def test_lstm_bar_rejects_named_faults():
    """On the served case's own weights and features, every named fault moves the log-probabilities by at least 3x the
    bar. Faults computed in float64."""
    input_dim, hidden, layers, actions, seq, batch = lh.CASES["served 64x7"]
    w = lh.make_weights(input_dim, hidden, layers, actions, 77)
    x = lh.make_features(seq, batch, input_dim, 78)
    ref = lh.reference(x, w, input_dim, layers)
    _, c_prev = lh.lstm_ref(lh.make_features(seq, batch, input_dim, 5)[..., :input_dim], w, layers)
    faults = {
        "stale granule (layer 1, step 5 reads h(t-2))": dict(fault={"stale": (1, 5)}),
        "c carried over from the previous call": dict(c0=c_prev),
        "one unit's recurrent rows rounded to bf16": dict(fault={"bf16_unit": lh.BF16_UNIT}),
        "gates f and g swapped": dict(fault={"swap_fg": True}),
        "b_hh dropped": dict(fault={"no_bhh": True}),
    }
    for what, kw in faults.items():
        r = lh.ratio(lh.reference(x, w, input_dim, layers, **kw), ref)
        print(f"{what}: {r:.2f} x the bar")
        assert r >= 3.0, f"{what}: only {r:.2f} x the bar"


def test_lstm_reference_matches_the_oracle_literal():
    """At the reference's own dimensions the generalised recurrence is oracle.rnn.lstm_literal."""
    from oracle import rnn
    from playaid_core_amd import synth

    sd = synth.make_rnn_state_dict(seed=3, num_actions=9)
    w = {}
    for l in range(3):
        for a, b in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            w[f"{a}{l}"] = sd[f"lstm.{b}_l{l}"]
    x = np.random.default_rng(1).uniform(-1, 1, (5, 3, 300))
    h, _ = lh.lstm_ref(x, w, 3)
    np.testing.assert_allclose(h, rnn.lstm_literal(x, sd), rtol=0, atol=1e-12)  # (summation order only)
