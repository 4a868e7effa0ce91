"""Shared pieces of tests/test_head_windows.py and its child tests/helpers/head_splitk_worker.py: the temporal head's inference
path (``pa_head_frames``: ``window_gather_kernel`` -> the gathered split-K igemm -> ``head_mlp_kernel``) on features the test
imports, against a float64 reference on the CPU.

Reference: the windows are ``oracle.window.action_sample_from_frame_middle_out`` per frame number (cache row
``(fn - 1) * F + fighter``; in a batch of k clips of L frames, frame number f belongs to clip ``c = (f - 1) // L``, has the local
number ``j = f - c * L`` -- ``j = L`` on the seam rows -- and its window is the sampler's at ``(j, S, D, L)`` shifted by ``c * L``);
the head is ``oracle.cnn.head_logits`` + ``log_softmax`` in float64 from the state dict.

Features are ``standard_normal * 0.25`` in columns 0..999 and exact zeros in the padding, every (frame, fighter) row its own draw.
At that scale torch's fp32 head is within 1e-6 of float64, so the project's head bar applies to every case: |logp - ref| <= 1e-5
absolute (``BAR``). Nothing here is changed by a test.
"""
import functools
import hashlib

import numpy as np
import torch
import torch.nn.functional as F_

from oracle import cnn
from oracle.window import action_sample_from_frame_middle_out
from playaid_core_amd import synth

BAR = 1e-5        # |dlogp|, absolute: the head bar of test_head_from_imported_features
PROB_BAR = 1e-5   # |prob - exp(max ref logp)|
TIE_GAP = 2e-5    # action_id is compared where the reference's top two log-probabilities differ by more than 2 x BAR
TIE_CAP = 0.02    # ... and at most this share of the windows may be left out for that reason
CLASS_IDS = (11, 5, 29, 17)   # four distinct character ids, none equal to its fighter index
SD_SEED = 1234
FEAT_SCALE = 0.25

# name: S, A, F, frame_delta, max_batch_frames, clip, ranges [lo, hi), feature seed
GRID = {
    "S1 A1 F1": (1, 1, 1, 3, 4, 6, ((1, 6),), 101),
    "S3 A2 F2": (3, 2, 2, 1, 4, 11, ((1, 11), (2, 3)), 102),
    "S5 A37 F3": (5, 37, 3, 2, 5, 23, ((1, 23), (9, 10)), 103),
    "S7 A63 F2": (7, 63, 2, 3, 8, 64, ((1, 64), (30, 33)), 104),
    "S9 A64 F4": (9, 64, 4, 1, 16, 40, ((1, 40),), 105),
    "S15 A64 F1": (15, 64, 1, 1, 65, 70, ((1, 70),), 106),
}
SERVED = "S7 A63 F2"
# the knob child's second engine: 4 K splits by default (one tap of 32 k-steps)
SPLITK_S1 = (1, 5, 1, 3, 4, 40, ((1, 40),), 107)


@functools.lru_cache(maxsize=None)
def state_dict(S, A, seed=SD_SEED):
    return synth.make_state_dict(seed=seed, num_actions=A, sequence_length=S)


def make_feats(n_frames, F, seed):
    """float32[n_frames, F, 1024]."""
    rng = np.random.default_rng(seed)
    feats = np.zeros((n_frames, F, 1024), np.float32)
    feats[..., :1000] = (rng.standard_normal((n_frames, F, 1000)) * FEAT_SCALE).astype(np.float32)
    return feats


# -- windows ----------------------------------------------------------------------------------------
def window_frames(f, S, D, clip, batch_of=0):
    """Frame numbers of the window around frame number f: the reference sampler, per clip of a batch."""
    if not batch_of:
        return np.array(action_sample_from_frame_middle_out(f, S, D, clip, min_frame=1), dtype=np.int64)
    L = clip // batch_of
    c = (f - 1) // L
    return np.array(action_sample_from_frame_middle_out(f - c * L, S, D, L, min_frame=1), dtype=np.int64) + c * L


def window_rows(lo, hi, S, D, clip, F, batch_of=0):
    """int64[hi - lo, F, S]: the feature-cache rows of every window of frame numbers [lo, hi)."""
    fn = np.stack([window_frames(f, S, D, clip, batch_of) for f in range(lo, hi)])       # [n, S]
    return (fn[:, None, :] - 1) * F + np.arange(F)[None, :, None]


def kernel_rows(f0, cnt, F, S, D, clip_frames, sub_frames=0):
    """``window_gather_kernel`` (csrc/misc.hip) line by line, one loop turn per thread: int64[cnt * F * S]."""
    out = np.empty(cnt * F * S, np.int64)
    for i in range(cnt * F * S):
        min_frame, max_frames = 1, clip_frames
        t = i % S
        w = i // S
        fighter = w % F
        f = f0 + w // F
        if sub_frames > 0:
            c = (f - 1) // sub_frames
            min_frame = c * sub_frames + 1
            max_frames = (c + 1) * sub_frames
        mid = S // 2
        off = abs(D * (mid - t) * (mid - t))
        if t <= mid:
            fn = max(f - off, min_frame)
        else:
            fn = min(f + off, max_frames - 1)
        out[i] = (fn - 1) * F + fighter
    return out


# -- the head in float64 ----------------------------------------------------------------------------
def gather_x(feats, rows):
    """feats [n_frames, F, 1024], rows [n, F, S] -> float64 tensor [n * F, S, 1000]. A row outside the cache (only a fault
    model asks for one) reads zeros."""
    flat = np.concatenate([feats.reshape(-1, feats.shape[-1])[:, :1000].astype(np.float64), np.zeros((1, 1000))])
    r = np.asarray(rows).reshape(-1, rows.shape[-1])
    r = np.where((r >= 0) & (r < flat.shape[0] - 1), r, flat.shape[0] - 1)
    return torch.from_numpy(flat[r])


def logp_of_x(x, sd):
    """x float64[B, S, 1000] -> log-probabilities float64[B, A]."""
    with torch.no_grad():
        return F_.log_softmax(cnn.head_logits(x, sd), dim=1).numpy()


def reference(sd, feats, rows):
    """-> float64[n, F, A]."""
    n, F, _ = rows.shape
    return logp_of_x(gather_x(feats, rows), sd).reshape(n, F, -1)


def first_argmax(logp):
    """The head's rule (``torch.argmax``): the FIRST index among equal maxima, along the last axis."""
    logp = np.asarray(logp)
    mx = logp.max(axis=-1, keepdims=True)
    idx = np.broadcast_to(np.arange(logp.shape[-1]), logp.shape)
    return np.where(logp == mx, idx, logp.shape[-1]).min(axis=-1)


def decided(ref):
    """bool[...]: windows whose reference argmax an error of BAR per log-probability cannot turn."""
    if ref.shape[-1] == 1:
        return np.ones(ref.shape[:-1], bool)
    top = np.sort(ref, axis=-1)
    return (top[..., -1] - top[..., -2]) > TIE_GAP


# -- comparison -------------------------------------------------------------------------------------
def measure(logp, rec, ref, class_ids=CLASS_IDS):
    """Device results (logp float32[n, F, A], the ``decode_records`` dict) against ``reference``'s -> dict of figures."""
    n, F, A = ref.shape
    ok = decided(ref)
    want = first_argmax(ref)
    return {
        "err": float(np.abs(logp.astype(np.float64) - ref).max()),
        "prob_err": float(np.abs(rec["prob"].astype(np.float64) - np.exp(ref.max(axis=-1))).max()),
        "skipped": float(1.0 - ok.mean()),
        "action_wrong": int((rec["action_id"] != want)[ok].sum()),
        "char_wrong": int((rec["char_id"] != np.asarray(class_ids[:F])[None, :]).sum()),
        "status_nonzero": int((rec["status"] != 0).sum()),
        "windows": n * F,
    }


def check(m, what):
    """Print the figures, then assert every one of them."""
    print(f"{what}: {m['windows']} windows, max |dlogp| = {m['err']:.3g}, max |dprob| = {m['prob_err']:.3g}, "
          f"near-ties left out {m['skipped']:.4f}")
    assert m["err"] <= BAR, f"{what}: max |dlogp| = {m['err']:.3g} > {BAR:g}"
    assert m["action_wrong"] == 0, f"{what}: {m['action_wrong']} action_id differ from the reference's first argmax"
    assert m["skipped"] <= TIE_CAP, f"{what}: {m['skipped']:.4f} of the windows are near-ties"
    assert m["char_wrong"] == 0, f"{what}: {m['char_wrong']} char_id are not class_ids[fighter]"
    assert m["prob_err"] <= PROB_BAR, f"{what}: max |prob - exp(max ref logp)| = {m['prob_err']:.3g}"
    assert m["status_nonzero"] == 0, f"{what}: {m['status_nonzero']} records with a non-zero status"


# -- the device -------------------------------------------------------------------------------------
def make_engine(case, dtype="f32", sd=None, max_clip_frames=None):
    from playaid_core_amd.engine import Engine

    S, A, F, D, mbf, clip = case[:6]
    return Engine(sd if sd is not None else state_dict(S, A), num_fighters=F, frame_delta=D, max_batch_frames=mbf,
                  max_clip_frames=max_clip_frames or clip, max_frame_height=128, max_frame_width=128,
                  fighter_class_ids=CLASS_IDS, compute_dtype=dtype)


def head_range(eng, lo, hi):
    """``head_frames(lo, hi)`` on whatever the engine's cache holds -> (logp float32[n, F, A], records dict) on the host."""
    lp = eng.alloc_logp(hi - lo)
    rec = eng.alloc_records(hi - lo)
    eng.head_frames(lo, hi, rec, lp)
    torch.cuda.synchronize()
    return lp.cpu().numpy(), eng.decode_records(rec)


def import_and_run(eng, feats, lo, hi, batch_of=0):
    """``clip_begin`` (+ batch) + ``features_import`` of the whole clip + ``head_frames(lo, hi)``."""
    eng.clip_begin(feats.shape[0], batch_of=batch_of)
    eng.features_import(0, torch.from_numpy(feats))
    return head_range(eng, lo, hi)


def run_case(case, dtype="f32", what=""):
    """One engine for ``case``, every range against float64 -> (list of ``measure`` dicts, sha256 of all logp bytes)."""
    S, A, F, D, mbf, clip, ranges, seed = case
    sd = state_dict(S, A)
    feats = make_feats(clip, F, seed)
    eng = make_engine(case, dtype)
    out, sha = [], hashlib.sha256()
    try:
        for lo, hi in ranges:
            lp, rec = import_and_run(eng, feats, lo, hi)
            sha.update(np.ascontiguousarray(lp).tobytes())
            m = measure(lp, rec, reference(sd, feats, window_rows(lo, hi, S, D, clip, F)))
            m["logp_max"] = float(lp.max())
            m["logp_min"] = float(lp.min())
            m["prob_min"], m["prob_max"] = float(rec["prob"].min()), float(rec["prob"].max())
            m["action_max"] = int(rec["action_id"].max())
            check(m, f"{what}{dtype} S={S} A={A} F={F} D={D} [{lo}, {hi})")
            out.append(m)
    finally:
        eng.close()
    return out, sha.hexdigest()
