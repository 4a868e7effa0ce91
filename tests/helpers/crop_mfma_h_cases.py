"""Cases of tests/test_crop_mfma_h.py, shared with its child (crop_mfma_h_worker.py), a CPU copy of the crop plan's choice
of forms (csrc/preprocess.hip: crop_plan_kernel, band_rows, band_lds -- vector, matrix vertical pass, matrix horizontal pass)
and a numpy restatement of the horizontal matrix form's operand (crop_hop_kernel) and of the pass itself."""
import numpy as np

from helpers import crop_mfma_cases as cm
from playaid_core_amd import synth

FUSED_LDS = cm.FUSED_LDS
HOP_PIXELS, HOP_WINDOW, HOP_BLOCKS_MAX = 10, 64, 48   # pa_kernels.h: PA_HOP_*
HOP_BLOCK_BYTES = 6 * 1024 + 32 * 4 + 16


def box(cx, cy, w, h, height, width):
    """Normalised box whose yolo_pixels (int(v * size)) are exactly these pixels."""
    return ((cx + 0.5) / width, (cy + 0.5) / height, (w + 0.5) / width, (h + 0.5) / height)


# ---------------------------------------------------------------------------------------------------------------------
# frame sets: (height, width, frames). "main" is crop_mfma_cases' size; "odd" has rows of 1914 bytes (not a multiple of 4);
# "tall" is high enough for a sub-band of more than 32 source rows at 7 taps.
# ---------------------------------------------------------------------------------------------------------------------
SETS = {"main": (cm.H, cm.W, 2), "odd": (360, 638, 2), "tall": (560, 400, 1)}


def frames(name):
    h, w, n = SETS[name]
    return synth.make_frames(n, h, w, seed=37 + len(name))


def _b(name, cx, cy, w, h):
    hh, ww, _ = SETS[name]
    return box(cx, cy, w, h, hh, ww)


# (case, frame set, frame, box); padding 30 throughout. Slice start x = cx - d // 2 - 30: its byte misalignment is (3 x) & 3.
CASES = [
    ("d128_m0", "main", 0, _b("main", 194, 180, 128, 100)),    # x = 100: aligned; d = 128 is INTER_AREA's copy path
    ("d129_m3", "main", 0, _b("main", 195, 170, 129, 100)),    # x = 101: misaligned by 3; 13 blocks, the last of 9 pixels
    ("d130_m2", "main", 1, _b("main", 197, 175, 130, 90)),     # x = 102: by 2; rw = 130: 13 whole blocks
    ("d131_m1", "main", 1, _b("main", 198, 172, 100, 131)),    # x = 103: by 1
    ("d160_m1", "main", 0, _b("main", 201, 170, 120, 160)),    # x = 91: by 1; 16 whole blocks
    ("d191_m0", "main", 1, _b("main", 301, 200, 191, 150)),    # x = 176: aligned; last block of 1 pixel
    ("d240_m2", "main", 0, _b("main", 320, 180, 240, 240)),    # x = 170: by 2; 24 blocks
    ("clip_left", "main", 1, _b("main", 60, 180, 200, 180)),   # slice starts at x = 0: 190 x 260 -> 146 x 200
    ("clip_right", "main", 0, _b("main", 585, 170, 190, 170)),  # slice ends at x = 640: 180 x 250 -> 137 x 190
    ("odd_pitch", "odd", 1, _b("odd", 201, 170, 120, 160)),    # rows of 1914 bytes: the misalignment changes row by row
    ("odd_pitch_b", "odd", 0, _b("odd", 300, 190, 191, 150)),
    ("over_32_rows", "tall", 0, _b("tall", 50, 280, 380, 500)),  # 330 x 560 slice -> 295 x 500: 40 source rows a sub-band
]


def by_set(name):
    return [i for i, c in enumerate(CASES) if c[1] == name]


# calls of several crop counts on the "main" frames (frame f of a call = main frame f & 1): (frames, fighter slots used)
COUNTS = [(1, 1), (3, 2), (6, 2), (40, 2)]   # 1 crop; 6 slots, 5 compared; 12; 80 -- ten whole groups of 8 rows of the grid
CLIP_FRAMES, CLIP_BATCH = 20, 8              # infer_clip: three backbone batches on one engine


def mixed_boxes(n, slots):
    """boxes float64[n, slots, 4]: the "main" cases in turn, and the case index of every slot."""
    main = by_set("main")
    bx = np.zeros((n, slots, 4), np.float64)
    idx = np.zeros((n, slots), np.int64)
    for f in range(n):
        for s in range(slots):
            i = main[(f * slots + s) % len(main)]
            bx[f, s] = CASES[i][3]
            idx[f, s] = i
    return bx, idx


def mixed_frames(n):
    fr = frames("main")
    return np.stack([fr[f & 1] for f in range(n)])


# ---------------------------------------------------------------------------------------------------------------------
# the plan on the host
# ---------------------------------------------------------------------------------------------------------------------
def _al(v, a):
    return (v + a - 1) // a * a


def _band_lds(pl, n0, n2, mfma_v, mfma_h, mis):
    sw, rw = pl["sw"], pl["rw"]
    p0 = _al(sw * 3, 4) + 4
    if mfma_h:
        p0 = _al(mis + sw * 3, 4) | 4
    p1 = _al(rw * 3, 4) + 4
    s1 = _al(n0 * p1, 16)
    if mfma_v:
        pt4, nblk = (n0 + 3) >> 2, (rw * 3 + 31) >> 5
        p1 = max(p1, nblk * 32)
        while ((p1 >> 2) & 3) != 2:
            p1 += 4
        skew = 0 if pt4 & 1 else 4
        s1 = _al(nblk * 32 * pt4 * 4 + nblk * 4 * skew + 32, 16)
    s0, s2 = _al(n0 * p0, 16), _al(n2 * p1, 16)
    if pl["need_h"] and pl["need_v"]:
        total = s0 + s1 + (s2 if s2 > s0 else 0)
    elif pl["need_h"]:
        total = s0 + s1
    elif pl["need_v"]:
        total = s0 + s2
    else:
        total = s0
    return total + (3 * 32 * 32 if mfma_v else 0), p0


def _bands(pl, rb):
    """(n0, n2) of every sub-band of rb output rows."""
    d, rh, sh, py = pl["d"], pl["rh"], pl["sh"], pl["py"]
    out_h = int(d * (128.0 / d))
    scale_y = 1.0 / (out_h / d)
    mode = 0 if d == 128 else None
    res = []
    for r0 in range(0, 128, rb):
        r1 = min(r0 + rb, out_h)
        if r0 >= r1:
            res.append((0, 0))
            continue
        if mode == 0:
            dy0, dy1 = r0, r1
        else:
            assert abs(scale_y - round(scale_y)) > 1e-9, "integer INTER_AREA scales are not mirrored here"
            a, _ = cm._area_tab(r0, scale_y, d)
            s, n = cm._area_tab(r1 - 1, scale_y, d)
            dy0, dy1 = a, s + n
        ry0, ry1 = min(max(dy0 - py, 0), rh), min(max(dy1 - py, 0), rh)
        if ry1 <= ry0:
            res.append((0, 0))
            continue
        if pl["need_v"]:
            ty0 = cm._bounds(sh, rh, ry0)[0]
            m, c = cm._bounds(sh, rh, ry1 - 1)
            ty1 = m + c
        else:
            ty0, ty1 = ry0, ry1
        res.append((ty1 - ty0, ry1 - ry0))
    return res


def block_windows(sw, rw, mis):
    """Per block of HOP_PIXELS output pixels of the pass sw -> rw: (first tap pixel, bytes from the aligned dword that holds
    the first tap to the end of the last tap)."""
    out = []
    for x0 in range(0, rw, HOP_PIXELS):
        x1 = min(x0 + HOP_PIXELS - 1, rw - 1)
        lo, _ = cm._bounds(sw, rw, x0)
        lo1, c1 = cm._bounds(sw, rw, x1)
        out.append((lo, ((mis + 3 * lo) & 3) + 3 * (lo1 + c1 - lo)))
    return out


def plan(bx, height, width, pad=30, frame=0, base_mis=0, mfma=1, mfma_h=1):
    """The geometry of cm.plan plus the plan kernel's choice: rb, mfma_v, mfma_h, h_mis, and the sub-bands' row counts."""
    pl = cm.plan(bx, height, width, pad)
    d, sw, sh, rw, rh = pl["d"], pl["sw"], pl["sh"], pl["rw"], pl["rh"]
    pl["py"] = int(np.rint((d - rh) * 0.5)) if (rw == d and rh != d) else 0
    mis = (base_mis + ((frame * height + pl["sy0"]) * width + pl["sx0"]) * 3) & 3
    mfma_ok = bool(mfma) and pl["need_h"] and pl["need_v"] and pl["ksize_v"] <= 7
    nb = (rw + HOP_PIXELS - 1) // HOP_PIXELS
    wins = block_windows(sw, rw, mis) if pl["need_h"] else []
    h_ok = mfma_ok and bool(mfma_h) and pl["ksize_h"] <= 7 and (width * 3) % 4 == 0 and nb <= HOP_BLOCKS_MAX and \
        all(w <= HOP_WINDOW for _, w in wins)
    pl.update(mis=mis, windows=wins, window_fits=all(w <= HOP_WINDOW for _, w in wins), rb=None, mfma_v=False, mfma_h=False, h_mis=0)
    for rb in (8, 4, 2, 1):
        bands = _bands(pl, rb)
        for m in ([2] if h_ok else []) + ([1] if mfma_ok else []) + [0]:
            worst = 0
            for n0, n2 in bands:
                need, _ = _band_lds(pl, n0, n2, m >= 1, m == 2, mis if m == 2 else 0)
                if m and (n0 > 32 or n2 > 32):
                    need = 1 << 30
                worst = max(worst, need)
            if worst <= FUSED_LDS:
                pl.update(rb=rb, mfma_v=m >= 1, mfma_h=m == 2, h_mis=mis if m == 2 else 0, bands=bands,
                          bands8=_bands(pl, 8))
                return pl
    pl.update(bands=[], bands8=_bands(pl, 8))
    return pl


def plan_of(i, **kw):
    name, fs, fr, bx = CASES[i]
    h, w, _ = SETS[fs]
    return plan(bx, h, w, frame=fr, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the operand and the pass in numpy
# ---------------------------------------------------------------------------------------------------------------------
def digits(k):
    """k = d0 + 256 d1 + 65536 d2 with d0, d1 in [-128, 127] (int64 arrays)."""
    d0 = ((k & 0xFF) ^ 0x80) - 0x80
    k1 = (k - d0) >> 8
    d1 = ((k1 & 0xFF) ^ 0x80) - 0x80
    d2 = (k1 - d1) >> 8
    return d0, d1, d2


def build_operand(bounds, kk, rw, mis):
    """crop_hop_kernel: per block a HOP_BLOCK_BYTES record -- six 1 KB fragments (digit 2, 1, 0 x the window's two 32-byte
    halves; lane l = 32 * (byte's 16-byte quarter & 1) + column holds 16 window bytes), 32 int32 constants, the window's
    first byte inside the staged row. ``bounds`` / ``kk``: oracle.resample.pil_bicubic_coeffs of the pass."""
    nb = (rw + HOP_PIXELS - 1) // HOP_PIXELS
    op = np.zeros((nb, HOP_BLOCK_BYTES), np.uint8)
    for blk in range(nb):
        x0 = blk * HOP_PIXELS
        first = mis + 3 * int(bounds[x0, 0])
        tail = op[blk, 6 * 1024:].view(np.int32)
        tail[32] = first & ~3
        for n in range(3 * HOP_PIXELS):
            px, c = divmod(n, 3)
            xx = x0 + px
            if xx >= rw:
                continue
            cnt = int(bounds[xx, 1])
            assert cnt <= 7
            k = kk[xx, :cnt].astype(np.int64)
            tail[n] = 128 * int(k.sum()) + (1 << 21)
            for t in range(cnt):
                kidx = (first & 3) + 3 * (int(bounds[xx, 0]) + t - int(bounds[x0, 0])) + c
                assert 0 <= kidx < HOP_WINDOW, (blk, n, t, kidx)
                dg = digits(k[t:t + 1])
                off = (kidx >> 5) * 1024 + (((kidx >> 4) & 1) * 32 + n) * 16 + (kidx & 15)
                for j, dj in enumerate((dg[2], dg[1], dg[0])):
                    op[blk, j * 2048 + off] = np.uint8(int(dj[0]) & 0xFF)
    return op


def run_operand(op, rows, rw):
    """The pass as the kernel runs it, on staged rows (uint8 [m][bytes], the slice's bytes behind ``mis`` bytes of whatever
    the frame holds there): int8 digit planes x (pixels - 128), per instruction step an exact int32 sum, Horner in wrapping
    int32 with the constant beside the middle digit. Returns (accumulators int64 [m][rw * 3], largest |partial sum|)."""
    m = rows.shape[0]
    acc_out = np.zeros((m, rw * 3), np.int64)
    padded = np.concatenate([rows, np.zeros((m, HOP_WINDOW + 4), np.uint8)], axis=1)
    biggest = 0
    for blk in range(op.shape[0]):
        tail = op[blk, 6 * 1024:].view(np.int32)
        wbase = int(tail[32])
        assert wbase % 4 == 0
        win = padded[:, wbase:wbase + HOP_WINDOW].astype(np.int64) - 128          # A: [m][64]
        acc = np.zeros((m, 32), np.uint32)
        for j in range(3):
            for step in range(2):
                frag = op[blk, (2 * j + step) * 1024:(2 * j + step + 1) * 1024].view(np.int8).reshape(64, 16).astype(np.int64)
                # B[k][n]: lane l holds column l & 31, window bytes 32 step + 16 (l >> 5) .. + 15
                b = np.zeros((HOP_WINDOW, 32), np.int64)
                b[32 * step:32 * step + 32] = frag.reshape(2, 32, 16).transpose(0, 2, 1).reshape(32, 32)
                part = win @ b
                biggest = max(biggest, int(np.abs(part).max()))
                acc = (acc + part.astype(np.int32).astype(np.uint32)).astype(np.uint32)
            if j < 2:
                acc = (acc << np.uint32(8)).astype(np.uint32)
                if j == 1:
                    acc = (acc + tail[:32].astype(np.uint32)[None, :]).astype(np.uint32)
        cols = min(3 * HOP_PIXELS, rw * 3 - blk * 3 * HOP_PIXELS)
        acc_out[:, blk * 3 * HOP_PIXELS:blk * 3 * HOP_PIXELS + cols] = acc.astype(np.int32).astype(np.int64)[:, :cols]
    return acc_out, biggest
