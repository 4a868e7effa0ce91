"""Digests of the ResNet-18 engine's weight arena and backbone stages, one line each, for comparing two builds of the library
(``PA_LIB_PATH`` selects the build; knobs come from the environment, so one process per knob setting). Modes:

  arena   SHA-256 of the ``pa_weights_export`` bytes and ``pa_weights_arena_bytes`` for {f32, emulated_f32, bf16} x {8, 64, 128
          crops} x S in {1, 5} (``--dtypes`` narrows it), from one seeded state dict per S
  trace   SHA-256 of every ``pa_backbone_trace`` stage 1..19 (and the stored branch of stages 7, 11, 15 where the engine has one)
          at 1, 35, 64 and 128 of 128 crops per dtype, seeded integer pixels / 255
  time    engine creation, f32 at 128 crops: median of five ``pa_create`` (fold) and of five ``pa_create_from_arena`` (adopt)
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.engine import Engine, EngineError  # noqa: E402
from playaid_core_amd.weights import pack_state_dict  # noqa: E402

GEOM = dict(max_clip_frames=8, max_frame_height=128, max_frame_width=128)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def arena(dtypes):
    for S in (1, 5):
        sd = synth.make_state_dict(seed=1234, num_actions=7, sequence_length=S)
        for dt in dtypes:
            for frames in (4, 32, 64):
                eng = Engine(sd, max_batch_frames=frames, compute_dtype=dt, **GEOM)
                a = eng.weights_arena().data
                print(f"arena dtype={dt} crops={2 * frames} S={S} bytes={a.numel()} sha256={sha(a)}", flush=True)
                eng.close()


def trace(dtypes):
    sd = synth.make_state_dict(seed=1234)
    pixels = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (128, 3, 128, 128)).astype(np.float32) / np.float32(255))
    for dt in dtypes:
        eng = Engine(sd, max_batch_frames=64, compute_dtype=dt, **GEOM)
        x = pixels.to(eng.device)
        for n in (1, 35, 64, 128):
            for stage in range(1, 20):
                print(f"trace dtype={dt} crops={n} stage={stage} sha256={sha(eng.backbone_trace(x[:n], stage))}", flush=True)
                if stage in Engine.TRACE_BRANCH_STAGES:
                    try:
                        branch = sha(eng.backbone_trace(x[:n], stage, aux=True)[1])
                    except EngineError:
                        branch = "none"   # block-0 conv2 takes the branch as its second K source
                    print(f"trace dtype={dt} crops={n} stage={stage} branch sha256={branch}", flush=True)
        eng.close()


def create_time():
    sd = pack_state_dict(synth.make_state_dict(seed=1234), 7, 63)   # the packed blob: pa_create's own time, without the packing
    keep = Engine(sd, max_batch_frames=64, **GEOM)
    prepared = keep.weights_arena()
    for mode, src in (("fold", sd), ("adopt", prepared)):
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng = Engine(src, max_batch_frames=64, **GEOM)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            eng.close()
        print(f"create mode={mode} dtype=f32 crops=128 ms={' '.join(f'{m:.0f}' for m in ms)} median={sorted(ms)[2]:.0f}", flush=True)
    keep.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["arena", "trace", "time"])
    ap.add_argument("--dtypes", default="f32,emulated_f32,bf16")
    args = ap.parse_args()
    if args.mode == "time":
        create_time()
    else:
        {"arena": arena, "trace": trace}[args.mode](args.dtypes.split(","))
