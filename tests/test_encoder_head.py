"""The transformer head (``pa_encoder_create`` / ``pa_encoder_forward``, csrc/transformer.hip) against a float64
restatement (a generalised ``oracle.resformer.encoder_literal`` plus the front projection, the time encoding, the
classifier and log_softmax), on device features the test supplies: rows of ``in_dim + 64`` floats, NaN past in_dim, so a
read past the row's features poisons the result.

Bar (log-probabilities, absolute): ``BAR = 2e-5``. Derivation from the fp32 arithmetic, u = 2^-24, at the served shape
(in 2048, d_model 256, 8 heads of 32, 3 post-norm layers, ff 2048, 63 actions):
  * every dense layer is an fp32 dot product of K = 2048 / 256 terms in chains split over 32-wide MFMA k-steps or 16-wide
    VALU tiles; with random-sign roundings its error is ~ sqrt(K) u sum|w a| / sqrt(K) ~ u * |a|_2 |w|_2 ~ 1e-7 relative.
  * attention: 32-term scores, an online softmax whose rescaling by exp(m_old - m_new) is exact up to expf's few ulp, and
    a <= 300-term weighted mean: ~ 3e-7 relative. At scores of +-40 expf(s - m) stays within [e^-80, 1] and the running
    sum l >= 1, so nothing overflows or flushes that matters; the scaled case checks that.
  * LayerNorm renormalises every row: it does not amplify the error (its Jacobian has norm g / std <= 1 here: gains
    U(0.3, 0.6), small enough that the eps of the next LayerNorm shows), but each layer's rows carry the relative error of
    its products: after three layers ~ 6e-7 relative (measured on an MI355X with a classifier of twice this gain: 1.9e-5
    at |logit| ~ 30).
  * classifier: 256 terms with |w| <= 4 sqrt(3 / 256) = 0.43 on a LayerNorm'd row (|x|_2 <= 16 * 0.6): |logit| <= 15, and
    the relative error above becomes <= 15 * 6e-7 ~ 9e-6 absolute; log_softmax adds a few ulp of |logit| (9.5e-7 each
    at 8..16).
  Total ~1e-5 in the worst row: the error is proportional to the logits' scale, so BAR = 2e-5 holds for logits up to
  ~15 (the synthetic checkpoint's classifier gain) and is 5x tighter than the end-to-end bar of 1e-4.

Cases: the served shape (64 windows x 7 slots, the padded front projection 247 -> 256); 1 window; 65 and 130 windows
(attention_kernel's lane loop wraps); 300 windows x 7 (2100 rows: launch_linear_f32's 128 x 64 tile on the 2048-wide
feed-forward); rows 63 / 64 / 65 around the matrix-core switch; hidden % 64 == 0 (the unpadded front projection on the
matrix cores); enc_dim = 0; 1 head; ff_dim = 200 (vector tiles); 100 actions (log-softmax loop wraps); inputs scaled so
that the first layer's attention scores reach about +-40.
"""
import ctypes as C
import math

import numpy as np
import pytest

BAR = 2e-5
PAD = 64  # extra floats per feature row


def make_weights(in_dim, hidden, slots, enc_dim, layers, ff, actions, seed):
    from playaid_core_amd.resnet_transformer_detector import time_encoding

    rng = np.random.default_rng([seed, in_dim, hidden, slots, enc_dim, layers, ff, actions])
    D = hidden + enc_dim

    def dense(shape, gain=1.0):
        a = gain * math.sqrt(3.0 / shape[1])
        return rng.uniform(-a, a, shape).astype(np.float32)

    def small(n, a=0.05):
        return rng.uniform(-a, a, n).astype(np.float32)

    w = {"ffn_w": dense((hidden, in_dim)), "ffn_b": small(hidden)}
    if enc_dim == 9 and slots > 1:
        w["enc"] = time_encoding(slots)
    else:
        w["enc"] = rng.uniform(-1, 1, (slots, enc_dim)).astype(np.float32)
    for l in range(layers):
        w[f"{l}.in_w"], w[f"{l}.in_b"] = dense((3 * D, D)), small(3 * D)
        w[f"{l}.out_w"], w[f"{l}.out_b"] = dense((D, D)), small(D)
        w[f"{l}.l1_w"], w[f"{l}.l1_b"] = dense((ff, D)), small(ff)
        w[f"{l}.l2_w"], w[f"{l}.l2_b"] = dense((D, ff)), small(D)
        for nm in ("n1", "n2"):
            w[f"{l}.{nm}_g"] = rng.uniform(0.3, 0.6, D).astype(np.float32)
            w[f"{l}.{nm}_b"] = small(D, 0.1)
    w["cls_w"], w["cls_b"] = dense((actions, D), gain=4.0), small(actions, 0.5)   # (synth.make_resformer_state_dict's gain)
    return w


def pack_blob(w, in_dim, hidden, slots, enc_dim, heads, layers, ff, actions):
    from playaid_core_amd import _lib

    hdr = np.zeros(16, np.int32)
    hdr[:10] = [_lib.PA_ENCODER_MAGIC, 1, in_dim, hidden, slots, enc_dim, heads, layers, ff, actions]
    keys = ["ffn_w", "ffn_b", "enc"]
    for l in range(layers):
        keys += [f"{l}.{k}" for k in ("in_w", "in_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "n1_g", "n1_b", "n2_g", "n2_b")]
    keys += ["cls_w", "cls_b"]
    return np.concatenate([hdr.view(np.uint8)] + [np.ascontiguousarray(w[k], np.float32).reshape(-1).view(np.uint8) for k in keys])


def encoder_ref(feats, w, heads, layers, fault=None):
    """feats [L, N, in] -> float64[L * N, A]. fault (sensitivity tests only): "slots" attention over the N slots instead of
    the L windows; "first64" only windows j < 64 attended; "noscale" no 1/sqrt(32); "eps" LayerNorm eps 1e-6; "stale"
    the encoding columns left as the padded projection writes them (0) instead of the time encoding."""
    f64 = lambda k: np.asarray(w[k], np.float64)  # noqa: E731
    x = np.asarray(feats, np.float64) @ f64("ffn_w").T + f64("ffn_b")
    L, N, _ = x.shape
    enc = f64("enc")
    if fault == "stale":
        enc = np.zeros_like(enc)
    x = np.concatenate([x, np.broadcast_to(enc[None], (L, N, enc.shape[1]))], axis=2)
    D = x.shape[2]
    hd = D // heads
    eps = 1e-6 if fault == "eps" else 1e-5

    def ln(v, g, b):
        mu = v.mean(-1, keepdims=True)
        var = ((v - mu) ** 2).mean(-1, keepdims=True)
        return (v - mu) / np.sqrt(var + eps) * g + b

    for l in range(layers):
        qkv = x @ f64(f"{l}.in_w").T + f64(f"{l}.in_b")
        q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(L, N, heads, hd) for i in range(3))
        scale = 1.0 if fault == "noscale" else 1.0 / np.sqrt(hd)
        if fault == "slots":
            s = np.einsum("lihd,ljhd->lhij", q, k) * scale
            s = np.exp(s - s.max(-1, keepdims=True))
            o = np.einsum("lhij,ljhd->lihd", s / s.sum(-1, keepdims=True), v).reshape(L, N, D)
        else:
            s = np.einsum("inhd,jnhd->nhij", q, k) * scale
            if fault == "first64":
                s[..., 64:] = -np.inf
            s = np.exp(s - s.max(-1, keepdims=True))
            o = np.einsum("nhij,jnhd->inhd", s / s.sum(-1, keepdims=True), v).reshape(L, N, D)
        o = o @ f64(f"{l}.out_w").T + f64(f"{l}.out_b")
        x = ln(x + o, f64(f"{l}.n1_g"), f64(f"{l}.n1_b"))
        f = np.maximum(x @ f64(f"{l}.l1_w").T + f64(f"{l}.l1_b"), 0.0)
        x = ln(x + f @ f64(f"{l}.l2_w").T + f64(f"{l}.l2_b"), f64(f"{l}.n2_g"), f64(f"{l}.n2_b"))
    y = (x @ f64("cls_w").T + f64("cls_b")).reshape(L * N, -1)
    y = y - y.max(1, keepdims=True)
    return y - np.log(np.exp(y).sum(1, keepdims=True))


def max_score(feats, w, heads):
    """The largest |attention score| of the first layer, float64."""
    x = np.asarray(feats, np.float64) @ np.asarray(w["ffn_w"], np.float64).T + w["ffn_b"]
    L, N, _ = x.shape
    x = np.concatenate([x, np.broadcast_to(np.asarray(w["enc"], np.float64)[None], (L, N, w["enc"].shape[1]))], axis=2)
    D = x.shape[2]
    qkv = x @ np.asarray(w["0.in_w"], np.float64).T + w["0.in_b"]
    q, k = (qkv[..., i * D:(i + 1) * D].reshape(L, N, heads, D // heads) for i in range(2))
    return float(np.abs(np.einsum("inhd,jnhd->nhij", q, k)).max() / np.sqrt(D // heads))


def make_features(windows, slots, in_dim, seed, scale=1.0):
    rng = np.random.default_rng([seed, windows, slots, in_dim])
    x = np.full((windows, slots, in_dim + PAD), np.nan, np.float32)
    x[..., :in_dim] = (rng.uniform(0.0, 1.0, (windows, slots, in_dim)) * scale).astype(np.float32)
    return x


# name -> (in_dim, hidden, slots, enc_dim, heads, layers, ff, actions, windows, feature scale)
SERVED = (2048, 247, 7, 9, 8, 3, 2048, 63)
CASES = {
    "served 64x7": SERVED + (64, 1.0),
    "1 window": SERVED + (1, 1.0),
    "65 windows": SERVED + (65, 1.0),
    "130 windows": SERVED + (130, 1.0),
    "300x7 rows": SERVED + (300, 1.0),
    "rows 63": SERVED + (9, 1.0),
    "rows 64": (2048, 247, 4, 9, 8, 3, 2048, 63, 16, 1.0),
    "rows 65": (2048, 247, 5, 9, 8, 3, 2048, 63, 13, 1.0),
    "hidden 192": (2048, 192, 7, 64, 8, 3, 2048, 63, 10, 1.0),
    "enc_dim 0": (2048, 256, 7, 0, 8, 3, 2048, 63, 10, 1.0),
    "1 head": (300, 23, 7, 9, 1, 2, 64, 63, 10, 1.0),
    "ff 200": (2048, 247, 7, 9, 8, 2, 200, 63, 10, 1.0),
    "100 actions": (2048, 247, 7, 9, 8, 3, 2048, 100, 10, 1.0),
    "scores 40": SERVED + (20, 6.0),
}


def run(name, seed=11):
    import torch

    from playaid_core_amd import _lib
    from playaid_core_amd.engine import _ptr

    in_dim, hidden, slots, enc_dim, heads, layers, ff, actions, windows, scale = CASES[name]
    lib = _lib.load()
    w = make_weights(in_dim, hidden, slots, enc_dim, layers, ff, actions, seed)
    blob = pack_blob(w, in_dim, hidden, slots, enc_dim, heads, layers, ff, actions)
    assert blob.nbytes == lib.pa_encoder_blob_bytes(in_dim, hidden, slots, enc_dim, layers, ff, actions)
    x = make_features(windows, slots, in_dim, seed + 1, scale)
    h = C.c_void_p()
    rc = lib.pa_encoder_create(0, in_dim, hidden, slots, enc_dim, heads, layers, ff, actions, windows * slots,
                               blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(h))
    try:
        assert rc == 0, lib.pa_encoder_last_error(h).decode() if h else rc
        xd = torch.from_numpy(x).cuda()
        out = torch.full((windows * slots, actions), float("nan"), device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.pa_encoder_forward(h, _ptr(xd), in_dim + PAD, windows, slots, _ptr(out), stream)
        assert rc == 0, lib.pa_encoder_last_error(h).decode()
        got = out.cpu().numpy()
    finally:
        if h:
            lib.pa_encoder_destroy(h)
    ref = encoder_ref(x[..., :in_dim], w, heads, layers)
    return float(np.abs(got.astype(np.float64) - ref).max() / BAR), got, x, w


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_encoder_head_against_float64(name):
    r, got, x, w = run(name)
    assert np.isfinite(got).all() and r <= 1.0, f"{name}: max |dlogp| = {r:.3g} x the {BAR:g} bar"
    line = f"encoder {name}: {r:.3f} of the bar"
    if name == "scores 40":
        line += f", first-layer scores up to {max_score(x[..., :CASES[name][0]], w, CASES[name][4]):.1f}"
    print(line)


# -- the comparator itself (CPU) ------------------------------------------------------------------------
def test_scaled_case_reaches_scores_of_40():
    in_dim, hidden, slots, enc_dim, heads, layers, ff, actions, windows, scale = CASES["scores 40"]
    w = make_weights(in_dim, hidden, slots, enc_dim, layers, ff, actions, 11)
    s = max_score(make_features(windows, slots, in_dim, 12, scale)[..., :in_dim], w, heads)
    assert 30.0 <= s <= 60.0, s


@pytest.mark.parametrize("case, fault", [
    ("served 64x7", "slots"), ("130 windows", "first64"), ("served 64x7", "noscale"), ("served 64x7", "eps"),
    ("served 64x7", "stale")])
def test_encoder_bar_rejects_named_faults(case, fault):
    """On the case's own weights and features every named fault moves the log-probabilities by >= 3x the bar (float64)."""
    in_dim, hidden, slots, enc_dim, heads, layers, ff, actions, windows, scale = CASES[case]
    w = make_weights(in_dim, hidden, slots, enc_dim, layers, ff, actions, 11)
    x = make_features(windows, slots, in_dim, 12, scale)[..., :in_dim]
    r = float(np.abs(encoder_ref(x, w, heads, layers, fault=fault) - encoder_ref(x, w, heads, layers)).max() / BAR)
    print(f"{case} {fault}: {r:.2f} x the bar")
    assert r >= 3.0, f"{fault}: only {r:.2f} x the bar"


def test_encoder_reference_matches_the_oracle_literal():
    """The generalised restatement is oracle.resformer.encoder_literal on the reference's dimensions."""
    from oracle import resformer
    from playaid_core_amd import synth

    sd = synth.make_resformer_state_dict(seed=3, num_actions=5, sequence_length=7)
    p = "model.transformer.layers."
    w = {"ffn_w": np.eye(256, dtype=np.float32), "ffn_b": np.zeros(256, np.float32), "enc": np.zeros((7, 0), np.float32),
         "cls_w": np.eye(256, dtype=np.float32), "cls_b": np.zeros(256, np.float32)}
    names = {"in_w": "self_attn.in_proj_weight", "in_b": "self_attn.in_proj_bias", "out_w": "self_attn.out_proj.weight",
             "out_b": "self_attn.out_proj.bias", "l1_w": "linear1.weight", "l1_b": "linear1.bias", "l2_w": "linear2.weight",
             "l2_b": "linear2.bias", "n1_g": "norm1.weight", "n1_b": "norm1.bias", "n2_g": "norm2.weight", "n2_b": "norm2.bias"}
    for l in range(3):
        for k, v in names.items():
            w[f"{l}.{k}"] = sd[p + f"{l}." + v]
    x = np.random.default_rng(2).standard_normal((5, 7, 256))
    lit = resformer.encoder_literal(x, sd).reshape(35, 256)
    lit = lit - lit.max(1, keepdims=True)
    lit = lit - np.log(np.exp(lit).sum(1, keepdims=True))
    np.testing.assert_allclose(encoder_ref(x, w, 8, 3), lit, rtol=0, atol=1e-10)
