"""SHA-256 digests of what the two device trainers compute (pa_head_train_step, pa_lstm_train_step), for comparing two builds
of the library bit for bit: run once per build in a fresh process (PA_LIB_PATH selects the library) with --out, then a third
time with --compare A B, which lists every line that differs and exits 1 if there is one. No tolerance applies.

For each shape: seeded weights, features and labels (every fifth label -100 where there are more than four); one
gradient-only call, then three applied steps on different batches, the second of them with no labelled row at all. Digests:
the gradients; the four pa_train_stats words of every call; read("weights"), read("m"), read("v") after the third step; for
the head also read_raw of the three sets, so that the padding columns count. Shapes: head (S, A, B) = (3, 5, 1), (3, 5, 7),
(7, 63, 37), (7, 63, 256); LSTM (input, H, layers, A) x (T, N) = (21, 32, 2, 5) x (9, 1) and (37, 7), (33, 64, 1, 3) x (1, 7)
and (5, 16), (300, 512, 3, 63) x (8, 4) -- B = 1 and T = 1, odd B, A < 64 and A = 63, N = 16, an input width that is no
multiple of 4 (the element-wise edge of lt_dw_kernel), B = 256.
usage: python scripts/train_bits.py --out FILE | --compare FILE_A FILE_B"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD_SHAPES = ((3, 5, 1), (3, 5, 7), (7, 63, 37), (7, 63, 256))
LSTM_CASES = (((21, 32, 2, 5), (9, 1)), ((21, 32, 2, 5), (37, 7)), ((33, 64, 1, 3), (1, 7)), ((33, 64, 1, 3), (5, 16)),
              ((300, 512, 3, 63), (8, 4)))
N_ROWS, LR, IGNORE = 300, 1e-3, -100

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--compare", nargs=2, default=None)
args = ap.parse_args()

if args.compare:
    a, b = (open(p).read().splitlines() for p in args.compare)
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in bad:
        print(f"DIFFERS\n  {x}\n  {y}")
    print(f"{len(a)} / {len(b)} digests, {len(bad)} differ")
    sys.exit(1 if bad or len(a) != len(b) or not a else 0)

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("train_bits.py needs a GPU")
from playaid_core_amd import _lib, synth  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402
from playaid_core_amd.head_trainer import HeadTrainer  # noqa: E402
from playaid_core_amd.lstm_trainer import LSTMTrainer, tensor_shapes  # noqa: E402

lines = []


def digest(name, tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    lines.append(f"{name} {h.hexdigest()}")


def words(name, stats):
    lines.append(f"{name} stats " + " ".join(f"{int(w) & 0xffffffff:08x}" for w in stats.cpu().tolist()))


def labels_for(rng, n, A, call):
    """Call 2 (the second applied step) has no labelled row."""
    if call == 2:
        return np.full(n, IGNORE, np.int32)
    l = rng.integers(0, A, size=n).astype(np.int32)
    if n > 4:
        l[::5] = IGNORE
    return l


def finish(name, tr, raw):
    for which in ("weights", "m", "v"):
        d = tr.read(which)
        digest(f"{name} {which}", [d[k] for k in tr.keys])
        if raw:
            digest(f"{name} raw {which}", tr.read_raw(which))


for S, A, B in HEAD_SHAPES:
    name = f"head S={S} A={A} B={B}"
    rng = np.random.default_rng([1, S, A, B])
    eng = Engine(synth.make_state_dict(seed=5, num_actions=A, sequence_length=S), max_batch_frames=8, max_clip_frames=64)
    tr = HeadTrainer(eng, lr=LR, max_batch=256)
    feats = torch.zeros(N_ROWS, _lib.PA_FEATURE_STRIDE)
    feats[:, :1000] = torch.from_numpy(0.5 * np.maximum(rng.standard_normal((N_ROWS, 1000)), -0.5).astype(np.float32))
    feats = feats.cuda()
    for call in range(4):
        gather = rng.integers(0, N_ROWS, size=(B, S)).astype(np.int32)
        labels = labels_for(rng, B, A, call)
        if call == 0:
            g, stats = tr.grads(feats, gather, labels)
            digest(f"{name} grads", [g[k] for k in tr.keys])
        else:
            stats = tr.step(feats, gather, labels)
        words(f"{name} call {call}", stats)
    finish(name, tr, raw=True)
    tr.close()
    eng.close()

lib = _lib.load()
for dims, (T, N) in LSTM_CASES:
    input_dim, H, L, A = dims
    name = f"lstm in={input_dim} H={H} L={L} A={A} T={T} N={N}"
    rng = np.random.default_rng([2, *dims, T, N])
    k = 1.5 / np.sqrt(H)
    parts = [np.array([_lib.PA_LSTM_MAGIC, 1, input_dim, H, L, A, 0, 0], np.int32).view(np.uint8)]   # the blob: header, tensors in blob order
    for shape in tensor_shapes(*dims):
        parts.append(rng.uniform(-k, k, shape).astype(np.float32).reshape(-1).view(np.uint8))
    blob = np.concatenate(parts)
    handle = C.c_void_p()
    rc = lib.pa_lstm_create(0, *dims, T * N, blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(handle))
    if rc != 0:
        sys.exit(f"pa_lstm_create: {rc} {lib.pa_lstm_last_error(handle).decode() if handle else ''}")
    tr = LSTMTrainer(handle, lr=LR, dims=dims, max_rows=T * N)
    for call in range(4):
        x = torch.zeros(T, N, _lib.PA_FEATURE_STRIDE)
        x[..., :input_dim] = torch.from_numpy(rng.uniform(-1.0, 1.0, (T, N, input_dim)).astype(np.float32))
        x = x.cuda()
        labels = labels_for(rng, T * N, A, call)
        if call == 0:
            g, stats = tr.grads(x, T, N, labels)
            digest(f"{name} grads", [g[k] for k in tr.keys])
        else:
            stats = tr.step(x, T, N, labels)
        words(f"{name} call {call}", stats)
    finish(name, tr, raw=False)
    tr.close()
    lib.pa_lstm_destroy(handle)

text = "\n".join(lines)
print(text)
print(f"library: {_lib.LIB_PATH}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
