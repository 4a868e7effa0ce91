"""Time of one training step of the LSTM head (pa_lstm_train_step, apply = 1) on one GPU at the served dimensions (input 300,
H 512, 3 layers, A 63) for (T, N) = (8, 4) and (64, 7), against the same step written in eager torch-ROCm fp32 (nn.LSTM, the
decoder, log_softmax, nll_loss, backward, torch.optim.Adam) in the same process. HIP events around groups of --steps steps after
warm-up, the two arms alternated --rounds times; median and min-max of the per-step time. The device arm is the
pa_lstm_train_step call alone (LSTMTrainer.step adds three small torch launches for its running statistics). Feature rows are
seeded random; the numbers say nothing about the backbone. --device-only leaves the eager arm out (for a kernel trace of the
device step alone).
usage: python scripts/lstm_train_rate.py [--steps 20] [--rounds 7] [--device-only] [--shape 64x7] [--out profiles/lstm_train_rate.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from playaid_core_amd import _lib, synth  # noqa: E402
from playaid_core_amd.lstm_trainer import LSTMTrainer  # noqa: E402
from playaid_core_amd.rnn_action_detector import HIDDEN_DIM, INPUT_DIM, NUM_LAYERS, pack_lstm_blob  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--shape", default=None, help="TxN: that shape alone, e.g. 64x7")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("lstm_train_rate.py needs a GPU: nothing here can be measured on a CPU")

A, LR, LD, MAX_ROWS = 63, 2e-4, _lib.PA_FEATURE_STRIDE, 64 * 7
sd = synth.make_rnn_state_dict(seed=5, num_actions=A)
lib = _lib.load()
blob = pack_lstm_blob(sd, A)
handle = C.c_void_p()
rc = lib.pa_lstm_create(0, INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, A, MAX_ROWS, blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(handle))
if rc != 0:
    sys.exit(f"pa_lstm_create: {rc} {lib.pa_lstm_last_error(handle).decode() if handle else ''}")
trainer = LSTMTrainer(handle, lr=LR, dims=(INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, A), max_rows=MAX_ROWS)


class Eager(nn.Module):
    def __init__(self):
        super().__init__()
        self.lstm = nn.LSTM(INPUT_DIM, HIDDEN_DIM, num_layers=NUM_LAYERS)
        self.action_decoder = nn.Sequential(nn.Linear(HIDDEN_DIM, 128), nn.ReLU(), nn.Linear(128, A))

    def forward(self, x):
        h, _ = self.lstm(x)
        return F.log_softmax(self.action_decoder(h.reshape(-1, HIDDEN_DIM)), dim=1)


eager = None
if not args.device_only:
    eager = Eager()
    eager.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith(("lstm.", "action_decoder."))})
    eager = eager.cuda()
    opt = torch.optim.Adam(eager.parameters(), lr=LR)


def eager_step(x, labels):
    opt.zero_grad(set_to_none=True)
    F.nll_loss(eager(x), labels, ignore_index=-100).backward()
    opt.step()


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # us per step


lines = [f"LSTM head training step, input {INPUT_DIM} H {HIDDEN_DIM} layers {NUM_LAYERS} A {A}, {args.steps} steps per group, {args.rounds} rounds, "
         f"arms alternated; {torch.cuda.get_device_name(0)}"]
SHAPES = ((8, 4), (64, 7)) if args.shape is None else (tuple(int(v) for v in args.shape.split("x")),)
rng = np.random.default_rng(2)
for T, N in SHAPES:
    x = torch.zeros(T, N, LD)
    x[..., :INPUT_DIM] = torch.from_numpy(rng.uniform(-1.0, 1.0, (T, N, INPUT_DIM)).astype(np.float32))
    x = x.cuda()
    labels = rng.integers(0, A, size=T * N).astype(np.int32)
    labels[::5] = -100
    labels = torch.from_numpy(labels).cuda()
    xe, le = x[..., :INPUT_DIM].contiguous(), labels.long()
    launches = NUM_LAYERS * (2 * T + 5) + 3
    dev = lambda: trainer._run(x, T, N, labels, True, None)   # noqa: E731  (the ABI call alone, without step()'s running statistics)
    eag = lambda: eager_step(xe, le)                          # noqa: E731
    arms = (dev,) if args.device_only else (dev, eag)
    for fn in arms:
        timed(fn, 5)                                          # warm-up: code objects, allocator, library algorithm choice
    t_dev, t_eag = [], []
    for _ in range(args.rounds):
        t_dev.append(timed(dev, args.steps))
        if not args.device_only:
            t_eag.append(timed(eag, args.steps))
    md = statistics.median(t_dev)
    line = f"T={T:2d} N={N}: device step {md:9.1f} us (min {min(t_dev):.1f}, max {max(t_dev):.1f}), {launches} launches"
    if t_eag:
        me = statistics.median(t_eag)
        line += f"; eager torch fp32 {me:9.1f} us (min {min(t_eag):.1f}, max {max(t_eag):.1f}); eager / device {me / md:.2f}"
    lines.append(line)
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
trainer.close()
lib.pa_lstm_destroy(handle)
