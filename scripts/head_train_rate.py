"""Time of one training step of the temporal head (pa_head_train_step, apply = 1) on one GPU at S = 7, A = 63 and B = 64 / 256,
against the same step written in eager torch-ROCm fp32 (gather, conv1d, two linears, log_softmax, nll_loss, backward,
torch.optim.Adam) in the same process. HIP events around groups of --steps steps after warm-up, the two arms alternated
--rounds times; median and min-max of the per-step time. The achieved bytes/s is the 86.0 MB of optimiser state a step must
move (w, m, v of cnn1d.0.weight read and written: 6 x 512 x 1000 x 7 x 4 bytes) over the step time -- a figure for the WHOLE
step, five launches, not a kernel's; the device arm is the pa_head_train_step call alone (HeadTrainer.step adds three small
torch launches for its running statistics). Feature rows are seeded random; the numbers say nothing about the backbone.
usage: python scripts/head_train_rate.py [--steps 50] [--rounds 7] [--out profiles/head_train_rate.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402
from playaid_core_amd.head_trainer import TENSOR_KEYS, HeadTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("head_train_rate.py needs a GPU: nothing here can be measured on a CPU")

S, A, N_ROWS, LR = 7, 63, 4096, 2e-4
STATE_MB = 6 * 512 * 1000 * S * 4 / 1e6
sd = synth.make_state_dict(seed=5, num_actions=A, sequence_length=S)
eng = Engine(sd, max_batch_frames=8, max_clip_frames=64)
trainer = HeadTrainer(eng, lr=LR, max_batch=256)
g = torch.Generator().manual_seed(1)
feats = torch.zeros(N_ROWS, 1024)
feats[:, :1000] = 0.5 * torch.clamp(torch.randn(N_ROWS, 1000, generator=g), min=-0.5)
feats = feats.cuda()
params = [torch.tensor(np.asarray(sd[k]), device="cuda", requires_grad=True) for k in TENSOR_KEYS]
opt = torch.optim.Adam(params, lr=LR)


def eager_step(gather, labels):
    w1, b1, w2, b2, w3, b3 = params
    opt.zero_grad(set_to_none=True)
    x = feats[:, :1000][gather.long()]
    h1 = torch.relu(F.conv1d(x.permute(0, 2, 1), w1, b1)).flatten(1)
    logp = F.log_softmax(F.linear(torch.relu(F.linear(h1, w2, b2)), w3, b3), dim=1)
    F.nll_loss(logp, labels.long(), ignore_index=-100).backward()
    opt.step()


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # us per step


lines = [f"head training step, S={S} A={A}, {args.steps} steps per group, {args.rounds} rounds, arms alternated; {torch.cuda.get_device_name(0)}"]
rng = np.random.default_rng(2)
for B in (64, 256):
    gather = torch.from_numpy(rng.integers(0, N_ROWS, size=(B, S)).astype(np.int32)).cuda()
    labels = rng.integers(0, A, size=B).astype(np.int32)
    labels[::5] = -100
    labels = torch.from_numpy(labels).cuda()
    dev = lambda: trainer._run(feats, gather, labels, True, None)   # noqa: E731  (the ABI call alone, without step()'s running statistics)
    eag = lambda: eager_step(gather, labels)            # noqa: E731
    for fn in (dev, eag):
        timed(fn, 10)                                   # warm-up: code objects, allocator, library algorithm choice
    t_dev, t_eag = [], []
    for _ in range(args.rounds):
        t_dev.append(timed(dev, args.steps))
        t_eag.append(timed(eag, args.steps))
    md, me = statistics.median(t_dev), statistics.median(t_eag)
    lines.append(f"B={B:3d}: device step {md:8.1f} us (min {min(t_dev):.1f}, max {max(t_dev):.1f}) = {STATE_MB / md:.3f} TB/s of the "
                 f"{STATE_MB:.1f} MB optimiser state; eager torch fp32 {me:8.1f} us (min {min(t_eag):.1f}, max {max(t_eag):.1f}); ratio {me / md:.2f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
