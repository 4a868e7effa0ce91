"""Time of one training step of the encoder head (pa_encoder_train_step, apply = 1, dropout 0.1) on one GPU at the served
dimensions (in 2048, hidden 247 + 9, 8 heads, 3 layers, ff 2048, A 63) for (L windows, N slots) = (8, 7) and (64, 7), against the
same step written in eager torch-ROCm fp32 (Linear, the encoding appended, nn.TransformerEncoder in train mode, Linear,
log_softmax, nll_loss, backward, torch.optim.Adam) in the same process. HIP events around groups of --steps steps after warm-up,
the two arms alternated --rounds times; median and min-max of the per-step time. The device arm is the pa_encoder_train_step
call alone (EncoderTrainer.step adds three small torch launches for its running statistics). Feature rows are seeded random; the
numbers say nothing about the backbone. --device-only leaves the eager arm out (for a kernel trace of the device step alone);
--shape runs one shape, so that a caller can give each its own time limit.
usage: python scripts/encoder_train_rate.py [--steps 20] [--rounds 7] [--device-only] [--shape 64x7] [--out FILE]"""
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
from playaid_core_amd.encoder_trainer import EncoderTrainer  # noqa: E402
from playaid_core_amd.resnet_transformer_detector import D_MODEL, FF_DIM, HIDDEN_DIM, NUM_HEADS, NUM_LAYERS, pack_encoder_blob  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--shape", default=None, help="LxN: that shape alone, e.g. 64x7")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("encoder_train_rate.py needs a GPU: nothing here can be measured on a CPU")

A, S, LR, P, IN, ENC, LD, MAX_ROWS = 63, 7, 2e-4, 0.1, 2048, 9, 2048, 64 * 7
sd = {k: v for k, v in synth.make_resformer_state_dict(seed=5, num_actions=A, sequence_length=S).items() if not k.startswith("model.resnet.")}
lib = _lib.load()
blob = pack_encoder_blob(sd, A, S)
handle = C.c_void_p()
rc = lib.pa_encoder_create(0, IN, HIDDEN_DIM, S, ENC, NUM_HEADS, NUM_LAYERS, FF_DIM, A, MAX_ROWS, blob.ctypes.data_as(C.c_void_p), blob.nbytes,
                           C.byref(handle))
if rc != 0:
    sys.exit(f"pa_encoder_create: {rc} {lib.pa_encoder_last_error(handle).decode() if handle else ''}")
trainer = EncoderTrainer(handle, lr=LR, dropout=P, dims=(IN, HIDDEN_DIM, S, ENC, NUM_HEADS, NUM_LAYERS, FF_DIM, A))


class Eager(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet_ffn = nn.Linear(IN, HIDDEN_DIM)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(D_MODEL, NUM_HEADS, FF_DIM, dropout=P), NUM_LAYERS,
                                                 enable_nested_tensor=False)
        self.classifier = nn.Linear(D_MODEL, A)
        self.register_buffer("freq_encoding", torch.zeros(S, ENC))

    def forward(self, x):   # [L, N, in] -> [L * N, A]
        h = self.resnet_ffn(x)
        h = torch.cat([h, self.freq_encoding[None].expand(h.shape[0], -1, -1)], dim=2)
        return F.log_softmax(self.classifier(self.transformer(h)).reshape(-1, A), dim=1)


eager = None
if not args.device_only:
    eager = Eager()
    eager.load_state_dict({k[len("model."):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items()
                           if k.startswith(("model.resnet_ffn.", "model.transformer.", "model.classifier.", "model.freq_encoding"))})
    eager = eager.cuda().train()
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


lines = [f"encoder head training step, in {IN} hidden {HIDDEN_DIM} + {ENC} heads {NUM_HEADS} layers {NUM_LAYERS} ff {FF_DIM} A {A} dropout {P}, "
         f"{args.steps} steps per group, {args.rounds} rounds, arms alternated; {torch.cuda.get_device_name(0)}"]
SHAPES = ((8, S), (64, S)) if args.shape is None else (tuple(int(v) for v in args.shape.split("x")),)
rng = np.random.default_rng(2)
for L, N in SHAPES:
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (L, N, LD)).astype(np.float32)).cuda()
    labels = rng.integers(0, A, size=L * N).astype(np.int32)
    labels[::5] = -100
    labels = torch.from_numpy(labels).cuda()
    le = labels.long()
    dev = lambda: trainer._run(x, L, N, labels, True, None)   # noqa: E731  (the ABI call alone, without step()'s running statistics)
    eag = lambda: eager_step(x, le)                           # noqa: E731
    arms = (dev,) if args.device_only else (dev, eag)
    for fn in arms:
        timed(fn, 5)                                          # warm-up: code objects, allocator, library algorithm choice
    t_dev, t_eag = [], []
    for _ in range(args.rounds):
        t_dev.append(timed(dev, args.steps))
        if not args.device_only:
            t_eag.append(timed(eag, args.steps))
    md = statistics.median(t_dev)
    line = f"L={L:2d} N={N}: device step {md:9.1f} us (min {min(t_dev):.1f}, max {max(t_dev):.1f})"
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
lib.pa_encoder_destroy(handle)
