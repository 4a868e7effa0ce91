"""Every backbone stage of the engine against float64, one layer at a time (``pa_backbone_trace``), on all three compute
dtypes, plus the temporal head from imported features.

Each stage's reference is computed in float64 from the PREVIOUS stage's stored output -- its interior only, with a zero
border of our own -- so errors do not add up from layer to layer and a corrupted border shows up in the next layer. The
weights are folded exactly as ``fold_conv`` (csrc/pa_api.hip) folds them: ``scale = gamma / sqrt(var + 1e-5)`` in
float64, ``w * scale`` and ``beta - mean * scale`` each rounded to fp32, the block-0 conv2 bias of layers 2-4
``fp32(double(b2) + double(bd))``. That is the engine's folded weights bit for bit.

Bars:
  * f32 / emulated_f32: every conv and the fc ``max|got - ref| <= 2e-5 * max|ref|`` (the bar of test_wino.py /
    test_psgemm.py); stem + pool the same; avgpool at the fp32 rounding of a 16-term mean; fc columns 1000..1023 exactly 0.
  * bf16, rounding model (misc.hip nchw_to_padded, stem_pool.hip's store, the patchconv_bf16.hip / igemm_bf16.hip
    epilogues): the model input is RNE to bf16; the weights are the folded fp32 values RNE to bf16; bias, residual add
    and ReLU are fp32; one RNE rounding at the store. The 1x1/2 downsample branch is stored as bf16 without bias and the
    block's conv2 adds it as its residual. With ``ref`` = the float64 result on those bf16-exact operands, every element
    satisfies ``|got - ref| <= half a bf16 ulp of ref + 2e-5 * max|ref|`` and ``got == RNE_bf16(ref)`` holds for at
    least 99.9 % of the elements of each stage. Measured on an MI355X: the lowest fraction of any stage in any case is
    99.988 %, the worst element sits at 0.993 of its bar.
  * every stage: the border is exactly zero, and so is channel 3 of the model input.

Cases (one engine per dtype and capacity, created and closed one after another). What each reaches, from
``choose_tile`` and the launchers at the default knobs (the plan's side of it is pinned by tests/test_engine_plan.py):
  * 1 of 136 crops: every tile is partial; at M = 16..1024 rows choose_tile takes 64x64 tiles and the deepest split K,
    the Winograd layers their split-K tickets.
  * 35 of 136 (5 windows x 7): the bf16 patch kernel's 8-image tiles (8x8 maps) and 16-image tiles (4x4 maps) both end
    ragged (35 % 8 = 35 % 16 = 3).
  * 136 of 136: the bf16 layer-2 opener (fused downsample) takes the 128x128 tile (272 tiles >= 256); 136 % 16 = 8 leaves
    the 4x4 maps' last 16-image tile half full (the 8x8 maps' tiles are all whole here).
  * 18 of 18 (max_batch_frames=9): ragged last tiles (18 % 8 = 18 % 16 = 2) at the very end of the layer buffers.
For more than 20 crops the float64 reference covers a sample: the first and last crop and both sides of every 8- (and so
16-) image boundary. Convolution is per image, so a sampled crop is still checked exactly; the border checks cover all.
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

P = "model.cnn2d."
U32 = 2.0 ** -24
F32_BAR = 2e-5
MIN_EXACT = 0.999
DTYPES = ["f32", "emulated_f32", "bf16"]
BRANCH_STAGES = (7, 11, 15)


# -- rounding model --------------------------------------------------------------------------------
def rne_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64 (finite values of bf16's normal range)."""
    m, e = np.frexp(np.asarray(x, np.float64))  # x = m * 2**e, 0.5 <= |m| < 1
    return np.ldexp(np.round(np.ldexp(m, 8)), e - 8)  # 8 significant bits; np.round rounds half to even


def half_ulp_bf16(x):
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 9))


def bf16_verdict(got, ref, min_exact=MIN_EXACT):
    """(passes, worst ratio of |got - ref| to its element bar, fraction of got == RNE_bf16(ref))."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    bar = half_ulp_bf16(ref) + F32_BAR * np.abs(ref).max()
    ratio = float((np.abs(got - ref) / np.maximum(bar, 1e-300)).max())
    exact = float((got == rne_bf16(ref)).mean())
    return ratio <= 1.0 and exact >= min_exact, ratio, exact


def f32_ratio(got, ref):
    """max|got - ref| over the bar 2e-5 * max|ref|."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (F32_BAR * np.abs(ref).max()))


# -- the engine's folded weights ---------------------------------------------------------------------
def fold(sd, conv, bn):
    """fold_conv: float64 scale, weights and bias each rounded to fp32 (as float64 arrays)."""
    w = np.asarray(sd[P + conv + ".weight"], np.float64)
    g, b, m, v = (np.asarray(sd[P + bn + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = g / np.sqrt(v + 1e-5)
    wf = (w * scale[:, None, None, None]).astype(np.float32).astype(np.float64)
    bf = (b - m * scale).astype(np.float32).astype(np.float64)
    return wf, bf


def conv_table():
    """(stage, name, cin, cout, stride, input stage, residual) of the sixteen 3x3 convs in engine order; residual is a
    stage, "branch" (the stored 1x1/2 downsample of the block input) or None."""
    out = []
    for li in range(4):
        co = (64, 128, 256, 512)[li]
        ci = 64 if li == 0 else co // 2
        s, blk = 2 + 4 * li, 1 + 4 * li
        q = f"layer{li + 1}"
        out += [(s, q + ".0.conv1", ci, co, 1 if li == 0 else 2, blk, None),
                (s + 1, q + ".0.conv2", co, co, 1, s, blk if li == 0 else "branch"),
                (s + 2, q + ".1.conv1", co, co, 1, s + 1, None),
                (s + 3, q + ".1.conv2", co, co, 1, s + 2, s + 1)]
    return out


def folded_weights(sd, bf16):
    """stage -> (w [cout][cin][k][k], b) as the engine holds them; 'stem', 'fc' and ('ds', stage) likewise."""
    cast = rne_bf16 if bf16 else (lambda a: a)
    wts = {}
    w, b = fold(sd, "conv1", "bn1")
    wts["stem"] = (cast(w), b)   # the bf16 stem multiplies the RNE'd folded weights too (stem_wgt_bf16)
    for s, name, *_ in conv_table():
        blk = name[:-len(".conv1")]
        w, b = fold(sd, name, blk + (".bn1" if name.endswith("conv1") else ".bn2"))
        if s in BRANCH_STAGES:
            wd, bd = fold(sd, blk + ".downsample.0", blk + ".downsample.1")
            b = (b + bd).astype(np.float32).astype(np.float64)
            wts[("ds", s)] = (cast(wd), None)
        wts[s] = (cast(w), b)
    wts["fc"] = (np.asarray(sd[P + "fc.weight"], np.float64), np.asarray(sd[P + "fc.bias"], np.float64))
    return wts


# -- float64 references from stored NHWC buffers ---------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def interior(a, pad=1):
    return a[:, pad:-pad, pad:-pad, :]


def ref_stem(x0, w, b):
    y = F.conv2d(_nchw(interior(x0, 3)[..., :3]), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=3)
    return _nhwc(F.max_pool2d(F.relu(y), 3, 2, 1))


def ref_conv(xin, w, b, stride, residual=None, relu=True):
    y = F.conv2d(_nchw(interior(xin)), torch.from_numpy(w), None if b is None else torch.from_numpy(b), stride=stride,
                 padding=w.shape[-1] // 2)
    y = _nhwc(y)
    if residual is not None:
        y = y + residual
    return np.maximum(y, 0.0) if relu else y


def ref_branch(xin, wd):
    return _nhwc(F.conv2d(_nchw(interior(xin)), torch.from_numpy(wd), None, stride=2))


def border_is_zero(a, pad):
    return (not a[:, :pad].any() and not a[:, -pad:].any() and not a[:, :, :pad].any() and not a[:, :, -pad:].any())


def sample_crops(n):
    if n <= 20:
        return np.arange(n)
    s = {0, n - 1}
    for edge in range(8, n, 8):
        s |= {edge - 1, edge}
    return np.array(sorted(s))


def _host(t):
    return t.float().cpu().numpy()  # bf16 -> fp32 is exact


def run_case(eng, sd, n, seed):
    """Traces every stage of one batch and checks it; returns {stage: (worst ratio, bf16 exact fraction or None)}."""
    bf16 = eng.compute_dtype == "bf16"
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255))
    xd = torch.from_numpy(x).cuda()
    st, aux = {}, {}
    for s in range(20):
        if s in BRANCH_STAGES:
            o, a = eng.backbone_trace(xd, s, aux=True)
            aux[s] = _host(a)
        else:
            o = eng.backbone_trace(xd, s)
        st[s] = _host(o)
    torch.cuda.synchronize()
    idx = sample_crops(n)
    wts = folded_weights(sd, bf16)
    res = {}
    tag = f"{eng.compute_dtype} n={n}"

    def check(s, got, ref, what):
        assert (ref != 0).mean() > 0.2, f"{tag} stage {s} ({what}): the reference is mostly zero, the check would be idle"
        if bf16:
            ok, ratio, exact = bf16_verdict(got, ref)
            assert ok, f"{tag} stage {s} ({what}): worst |err| / bar = {ratio:.3g}, exact fraction {exact:.5f}"
            res[s if what != "branch" else ("ds", s)] = (ratio, exact)
        else:
            ratio = f32_ratio(got, ref)
            assert ratio <= 1.0, f"{tag} stage {s} ({what}): max|err| = {ratio:.3g} x the 2e-5 bar"
            res[s if what != "branch" else ("ds", s)] = (ratio, None)

    # 0: the model input as stored
    x0 = st[0]
    assert border_is_zero(x0, 3) and not x0[..., 3].any(), tag
    xin = np.ascontiguousarray(x.transpose(0, 2, 3, 1), np.float64)
    assert np.array_equal(interior(x0, 3)[..., :3], rne_bf16(xin) if bf16 else xin), tag
    # 1: stem + BatchNorm + ReLU + max-pool
    assert border_is_zero(st[1], 1), tag
    w, b = wts["stem"]
    check(1, interior(st[1])[idx], ref_stem(x0[idx], w, b), "stem+pool")
    # 2..17: the 3x3 convolutions (and the stored downsample branches)
    for s, name, ci, co, stride, src, resid in conv_table():
        got = st[s]
        assert border_is_zero(got, 1), f"{tag} stage {s} {name}: non-zero border"
        w, b = wts[s]
        r = None
        if resid == "branch":
            a = aux[s]
            assert border_is_zero(a, 1), f"{tag} stage {s} {name}: non-zero border in the stored branch"
            # the branch reads the block input: the input of the block's opener, stage s - 2
            check(s, interior(a)[idx], ref_branch(st[s - 2][idx], wts[("ds", s)][0]), "branch")
            r = interior(a)[idx].astype(np.float64)
        elif resid is not None:
            r = interior(st[resid])[idx].astype(np.float64)
        check(s, interior(got)[idx], ref_conv(st[src][idx], w, b, stride, r), name)
    # 18: avgpool (fp32 for every dtype): a 16-term fp32 sum times 1/16
    l4 = interior(st[17])[idx].astype(np.float64)
    ref = l4.mean(axis=(1, 2))
    bar = 16 * U32 * np.abs(l4).mean(axis=(1, 2))
    err = np.abs(st[18][idx] - ref)
    assert (err <= bar).all(), f"{tag} avgpool: worst |err| / bar = {(err / np.maximum(bar, 1e-300)).max():.3g}"
    res[18] = (float((err / np.maximum(bar, 1e-300)).max()), None)
    # 19: fc, fp32 for every dtype; the 24 padding columns are exactly zero
    fc = st[19]
    assert not fc[:, 1000:].any(), tag
    w, b = wts["fc"]
    ratio = f32_ratio(fc[idx, :1000], st[18][idx].astype(np.float64) @ w.T + b)
    assert ratio <= 1.0, f"{tag} fc: max|err| = {ratio:.3g} x the 2e-5 bar"
    res[19] = (ratio, None)
    if bf16:
        # sensitivity: the same bar must tell the engine's bf16 weights from the unrounded fp32 ones (layer3.1.conv1)
        s, name, ci, co, stride, src, resid = conv_table()[10]
        w32, b32 = fold(sd, name, name[:-len(".conv1")] + ".bn1")
        ok, ratio, exact = bf16_verdict(interior(st[s])[idx], ref_conv(st[src][idx], w32, b32, stride))
        assert not ok, f"{tag}: the bf16 bar cannot tell bf16 weights from fp32 ones (ratio {ratio:.3g}, exact {exact:.5f})"
    return res


CASES = {136: [1, 3, 35, 136], 18: [5, 18]}   # 3 and 5 crops: layer 4 has 48 and 80 pixels -- a last tile partly out of range, tile counts that are no multiple of 8


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [136, 18])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backbone_stages_against_float64(state_dict, dtype, capacity):
    from playaid_core_amd.engine import Engine

    t0 = time.time()
    eng = Engine(state_dict, max_batch_frames=capacity // 2, max_clip_frames=16, max_frame_height=128, max_frame_width=128,
                 compute_dtype=dtype)
    try:
        for n in CASES[capacity]:
            res = run_case(eng, state_dict, n, seed=1000 + n)
            worst = max(res.items(), key=lambda kv: kv[1][0])
            conv = max((v[0], k) for k, v in res.items() if k not in (18, 19))
            line = (f"{dtype} capacity {capacity} n={n}: worst stage {worst[0]} at {worst[1][0]:.3f} of its bar, "
                    f"worst conv stage {conv[1]} at {conv[0]:.3f}")
            if dtype == "bf16":
                low = min((v[1], k) for k, v in res.items() if v[1] is not None)
                line += f", lowest exact fraction {low[0]:.5f} (stage {low[1]})"
            print(line)
    finally:
        eng.close()
    print(f"{dtype} capacity {capacity}: {time.time() - t0:.1f} s")


@pytest.mark.gpu
def test_trace_refuses_bad_arguments(state_dict):
    from playaid_core_amd import _lib
    from playaid_core_amd.engine import Engine, EngineError, _ptr

    eng = Engine(state_dict, max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    try:
        x = torch.zeros((9, 3, 128, 128), device="cuda")
        out = torch.empty(eng.trace_shape(9, 1), device="cuda")
        nb = out.numel() * 4 // 9 * 8  # stage 1 of 8 crops
        lib, s = eng._lib, eng._stream()
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 9, 1, _ptr(out), nb, None, 0, s) == _lib.PA_ERR_INVALID_ARG  # > max_crops
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 0, 1, _ptr(out), nb, None, 0, s) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 8, 20, _ptr(out), nb, None, 0, s) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 8, -1, _ptr(out), nb, None, 0, s) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 8, 1, _ptr(out), nb - 4, None, 0, s) == _lib.PA_ERR_INVALID_ARG  # too small
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 8, 7, _ptr(out), nb, _ptr(out), 16, s) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_backbone_trace(eng._h, _ptr(x), 8, 1, _ptr(out), nb, None, 0, s) == _lib.PA_OK
        with pytest.raises(EngineError):
            eng.backbone_trace(x, 3)
        torch.cuda.synchronize()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_from_imported_features(state_dict, dtype):
    """features_import + head_frames: the temporal Conv1d (igemm split K with the reduce deferred to the MLP kernel) +
    MLP + log-softmax (misc.hip) on exact fp32 features, against oracle.cnn.head_logits in float64 + log-softmax.
    Bar 1e-5 absolute on log-probabilities; measured on an MI355X: 7.4e-6 at most, the same on all three dtypes (the
    head is fp32 on every one)."""
    from oracle import cnn
    from oracle.window import action_sample_from_frame_middle_out
    from playaid_core_amd import constants
    from playaid_core_amd.engine import Engine

    clip = 40
    eng = Engine(state_dict, num_fighters=1, max_batch_frames=16, max_clip_frames=clip, max_frame_height=128,
                 max_frame_width=128, compute_dtype=dtype)
    try:
        S = eng.S
        rng = np.random.default_rng(5)
        feats = np.zeros((clip, 1, 1024), np.float32)
        feats[..., :1000] = (rng.standard_normal((clip, 1, 1000)) * 2.0).astype(np.float32)
        worst = 0.0
        # 1 window, an odd count, max_clip_frames - 1 windows (16 per pass: 16 + 16 + 7)
        for lo, hi in ((7, 8), (3, 16), (1, clip)):
            eng.clip_begin(clip)
            eng.features_import(0, torch.from_numpy(feats))
            lp = eng.alloc_logp(hi - lo)
            eng.head_frames(lo, hi, eng.alloc_records(hi - lo), lp)
            torch.cuda.synchronize()
            rows = [np.array(action_sample_from_frame_middle_out(f, S, constants.FRAME_DELTA, clip, min_frame=1)) - 1
                    for f in range(lo, hi)]
            win = torch.from_numpy(np.stack([feats[r, 0, :1000] for r in rows]).astype(np.float64))
            ref = F.log_softmax(cnn.head_logits(win, state_dict), dim=1).numpy()
            err = float(np.abs(lp.cpu().numpy()[:, 0].astype(np.float64) - ref).max())
            assert err <= 1e-5, f"{dtype}: {hi - lo} windows, max |dlogp| = {err:.3g}"
            worst = max(worst, err)
        print(f"{dtype} head: max |dlogp| = {worst:.3g}")
    finally:
        eng.close()


# -- the comparator itself (CPU) --------------------------------------------------------------------
def _taps_conv(xpad, w, drop=None, shift=None, acc_dtype=np.float64):
    """3x3 stride-1 conv of a zero-bordered NHWC x by w [co][ci][3][3], summed per (tap, 32-channel chunk) piece in the
    kernel's k order. drop = (tap, chunk): leave that piece out; shift = tap: that tap reads one pixel to the right."""
    n, hp, wp, ci = xpad.shape
    h, wd = hp - 2, wp - 2
    acc = np.zeros((n, h, wd, w.shape[0]), acc_dtype)
    for c0 in range(0, ci, 32):
        for t in range(9):
            if drop == (t, c0 // 32):
                continue
            ky, kx = divmod(t, 3)
            dx = 1 if shift == t else 0
            xs = np.pad(xpad, ((0, 0), (0, 0), (0, 1), (0, 0)))[:, ky:ky + h, kx + dx:kx + dx + wd, c0:c0 + 32]
            piece = np.einsum("nyxc,oc->nyxo", xs, w[:, c0:c0 + 32, ky, kx])
            acc = acc + piece.astype(acc_dtype)
    return acc


def test_bf16_comparator_accepts_rne_and_rejects_known_faults():
    """The bf16 checker accepts an fp32-order sum rounded RNE and rejects a result missing one 32-channel K chunk, a tap
    shifted by a pixel, and a residual added before its bf16 rounding."""
    rng = np.random.default_rng(11)
    n, hw, ci, co = 4, 8, 64, 64
    xpad = np.zeros((n, hw + 2, hw + 2, ci))
    xpad[:, 1:-1, 1:-1] = rne_bf16(np.abs(rng.standard_normal((n, hw, hw, ci))))
    w = rne_bf16(rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci))
    b = rng.standard_normal(co).astype(np.float32).astype(np.float64) * 0.5
    res32 = rng.standard_normal((n, hw, hw, co)).astype(np.float32)
    res = rne_bf16(res32)
    ref = np.maximum(_taps_conv(xpad, w) + b + res, 0.0)
    # the engine's arithmetic: fp32 accumulation piece by piece, fp32 epilogue, one RNE
    acc = _taps_conv(xpad, w, acc_dtype=np.float32)
    good = np.maximum(acc + b.astype(np.float32) + res.astype(np.float32), np.float32(0))
    ok, ratio, exact = bf16_verdict(rne_bf16(good.astype(np.float64)), ref)
    assert ok, (ratio, exact)
    faults = {
        "missing K chunk": np.maximum(_taps_conv(xpad, w, drop=(4, 1)) + b + res, 0.0),
        "shifted tap": np.maximum(_taps_conv(xpad, w, shift=5) + b + res, 0.0),
        "unrounded residual": np.maximum(_taps_conv(xpad, w) + b + res32.astype(np.float64), 0.0),
    }
    for what, bad in faults.items():
        ok, ratio, exact = bf16_verdict(rne_bf16(bad), ref)
        assert not ok, f"{what} passed: ratio {ratio:.3g}, exact {exact:.5f}"


def test_rne_bf16_matches_the_kernels_bit_trick():
    """rne_bf16 on fp32 inputs equals the kernels' ``(u + 0x7fff + ((u >> 16) & 1)) >> 16``."""
    rng = np.random.default_rng(2)
    v = np.concatenate([rng.standard_normal(100000).astype(np.float32) * 10.0,
                        np.float32([0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-30])])
    u = v.view(np.uint32).astype(np.uint64)
    trick = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    assert np.array_equal(rne_bf16(v.astype(np.float64)), trick.astype(np.float64))
