"""ResnetTransformerDetector's 64-window call (64 x 7 = 448 crops, 63 actions, seeded weights) under each compute dtype, and the
bf16 ResNet-50's per-row times.

  python scripts/resformer_dtypes.py               the call under f32, emulated_f32 and bf16, alternated twice in one process:
                                                   median ms of 10 calls after 3 warm-up calls each, windows/s
  python scripts/resformer_dtypes.py --rows OUT    per-row times of the bf16 table at 64 crops (one served group), JSON to OUT;
                                                   run once per setting of PA_CONVNET_BG_SPLIT (read once per process): unset
                                                   (the rule), 0 (no split-K), 4 and 8 (S forced on every row whose unsplit grid
                                                   is below half the CUs)
  python scripts/resformer_dtypes.py --compare REF A [B ...]
                                                   the --rows files side by side: every row where a file's form differs from
                                                   REF's (REF: the PA_CONVNET_BG_SPLIT=0 run), its time and the ratio to REF's

A row's time is the difference of two prefixes, rows 0..i against rows 0..i-1 (pa_convnet_trace, copying the 512 KiB pooled buffer
of 64 crops x 2048 fp32, which the difference cancels), median of 31 HIP-event timings each."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.resnet_transformer_detector import ConvNet, ResnetTransformerDetector, build_resnet50_table  # noqa: E402

WINDOWS, SEQ, ACTIONS = 64, 7, 63
DTYPES = ("f32", "emulated_f32", "bf16")


def _time(fn, reps, warm):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def calls():
    sd = synth.make_resformer_state_dict(seed=2468, num_actions=ACTIONS, sequence_length=SEQ)
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (WINDOWS, SEQ, 3, 128, 128)).astype(np.float32) / 255).cuda()
    models = {dt: ResnetTransformerDetector([f"a{i}" for i in range(ACTIONS)], sequence_length=SEQ, state_dict=sd, max_rows=WINDOWS * SEQ,
                                            compute_dtype=dt).eval() for dt in DTYPES}
    ref = models["f32"](x)
    res = {dt: [] for dt in DTYPES}
    for rnd in range(2):
        for dt in DTYPES:
            ms = _time(lambda: models[dt](x), 10, 3)
            res[dt].append(ms)
            d = float((models[dt](x) - ref).abs().max())
            print(f"round {rnd} {dt:13s} {ms:7.3f} ms per 64-window call ({WINDOWS * SEQ} crops) = {WINDOWS / ms * 1e3:7.0f} windows/s; "
                  f"max |d log p| vs f32 {d:.3g}")
    best = {dt: min(v) for dt, v in res.items()}
    for dt in DTYPES:
        print(f"{dt:13s} best {best[dt]:7.3f} ms = {WINDOWS / best[dt] * 1e3:7.0f} windows/s, x{best['f32'] / best[dt]:.2f} f32")
    for m in models.values():
        m.close()


def rows(out):
    sd = synth.make_resformer_state_dict(seed=2468, num_actions=ACTIONS, sequence_length=SEQ)
    descs, bufs, weights, dim = build_resnet50_table(sd)
    net = ConvNet(descs, bufs, weights, dim, max_crops=64, compute_dtype="bf16")
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (64, 3, 128, 128)).astype(np.float32) / 255).cuda()
    pooled = descs[-1]["out_buf"]
    prefix = [_time(lambda li=li: net.trace(x, li, pooled), 31, 3) for li in range(-1, len(descs))]
    forms = net.layer_forms()
    res = []
    for i, d in enumerate(descs):
        us = (prefix[i + 1] - prefix[i]) * 1e3
        hw = d["in_hw"] // d["stride"] if d["kind"] == 0 else (32 if d["kind"] == 1 else 1)
        gf = 2.0 * 64 * hw * hw * d["cout"] * d["ksize"] ** 2 * d["cin"] / 1e9 if d["kind"] == 0 else (2.0 * 64 * 64 * 64 * 64 * 147 / 1e9 if d["kind"] == 1 else 0.0)
        res.append(dict(row=i, kind=d["kind"], k=d["ksize"], s=d["stride"], hw=hw, cin=d["cin"], cout=d["cout"], form=forms[i], us=us, gflop=gf))
        print(f"{i:3d} kind {d['kind']} k{d['ksize']} s{d['stride']} out {hw:2d}x{hw:<2d} cin {d['cin']:4d} cout {d['cout']:4d} "
              f"{forms[i]:13s} {us:8.1f} us {gf / us * 1e3 if us > 0 and gf else 0:6.1f} TF")
    print(f"knob PA_CONVNET_BG_SPLIT={os.environ.get('PA_CONVNET_BG_SPLIT', '(unset)')}; whole table {prefix[-1] * 1e3:.1f} us "
          f"(input conversion {prefix[0] * 1e3:.1f} us)")
    json.dump(dict(knob=os.environ.get("PA_CONVNET_BG_SPLIT"), total_us=prefix[-1] * 1e3, rows=res), open(out, "w"))
    net.close()


def compare(ref, *others):
    R = json.load(open(ref))
    O = [json.load(open(f)) for f in others]
    knob = lambda J: "unset (the rule)" if J["knob"] is None else J["knob"]
    print("per-row split-K A/B at 64 crops, us (ratio to the unsplit row); columns: PA_CONVNET_BG_SPLIT = "
          + " | ".join(knob(J) for J in [R] + O))
    for i, r in enumerate(R["rows"]):
        if all(J["rows"][i]["form"] == r["form"] for J in O):
            continue
        cells = [f"{r['form']:6s} {r['us']:6.1f}"]
        for J in O:
            o = J["rows"][i]
            cells.append(f"{'split' if o['form'] == 'bgemm_splitk' else 'whole':6s} {o['us']:6.1f} ({o['us'] / r['us']:.2f})")
        print(f"{i:3d} k{r['k']} s{r['s']} out {r['hw']:2d}x{r['hw']:<2d} cin {r['cin']:4d} cout {r['cout']:4d}: " + " | ".join(cells))
    print("whole table: " + " | ".join(f"{J['total_us']:.1f} us" for J in [R] + O))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows")
    ap.add_argument("--compare", nargs="+")
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    elif args.rows:
        rows(args.rows)
    else:
        calls()
