"""The cases the host and the device tests of ``playaid_core_amd.detect_composite`` share: renders, resize targets, stages,
sprites and scene records."""
import numpy as np

from playaid_core_amd import detect_composite as dc

ALPHAS = ["zero", "full", "random", "one", "254"]


def make_render(h, w, alpha, seed=0):
    """As tests/test_sprite_augment.py: seeded noise, the alpha plane zero / full / random / 1 / 254."""
    rng = np.random.default_rng([h, w, ALPHAS.index(alpha), seed])
    s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha != "random":
        s[..., 3] = {"zero": 0, "full": 255, "one": 1, "254": 254}[alpha]
    return s


# (source h x w, target (ow, oh)): the issue's table
RESIZE_CASES = [
    ((100, 100), (50, 50)),
    ((128, 128), (128, 128)),      # the copy case
    ((300, 175), (50, 85)),
    ((300, 1024), (50, 14)),       # the 83-tap pass
    ((350, 100), (150, 525)),      # enlarging and tall
    ((120, 110), (60, 65)),
    ((101, 257), (149, 58)),
]
# ... and one pass alone: the width stays, the height stays
ONE_PASS_CASES = [((120, 110), (110, 65)), ((120, 110), (60, 120))]


def resize_renders():
    """One render per (case, alpha plane), and the records that resize each to its case's target."""
    renders, targets = [], []
    for (h, w), (ow, oh) in RESIZE_CASES + ONE_PASS_CASES:
        for a in ALPHAS:
            renders.append(make_render(h, w, a))
            targets.append((ow, oh))
    params = dc.resize_params(np.arange(len(renders)), [t[0] for t in targets], [t[1] for t in targets])
    return renders, params


STAGE_SHAPES = [(150, 200), (77, 131), (100, 100)]   # (h, w): 200 x 150, 131 x 77 (odd width, lower than a sprite), 100 x 100


def make_stages(shapes=STAGE_SHAPES):
    return [np.random.default_rng([7, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def make_slots(n=6):
    """128 x 128 RGBA sprites whose alpha planes are zero, full, random, 1, 254 and random again."""
    return np.stack([make_render(128, 128, a, seed=k) for k, a in enumerate((ALPHAS + ["random"])[:n])])


def scene(stage, sprites):
    r = np.zeros(1, dtype=dc.SCENE_DTYPE)
    r["stage"] = stage
    r["n_sprites"] = len(sprites)
    for k, s in enumerate(sprites):
        r["sprites"][0, k] = s
    return r


def scene_records(stage_shapes=STAGE_SHAPES):
    """Per stage: no sprite; one inside (or as far inside as the stage allows); one over each edge; one over each corner; one
    wholly outside on each side; four sprites, two of them overlapping, in both orders."""
    recs = []
    for g, (H, W) in enumerate(stage_shapes):
        recs.append(scene(g, []))
        recs.append(scene(g, [(2, (W - 128) // 2, (H - 128) // 2)]))
        for x, y in ((-40, 5), (W - 70, 5), (10, -50), (10, H - 60)):                      # the four edges
            recs.append(scene(g, [(2, x, y)]))
        for x, y in ((-33, -21), (W - 90, -21), (-33, H - 77), (W - 90, H - 77)):          # the four corners
            recs.append(scene(g, [(5, x, y)]))
        for x, y in ((-128, 0), (W, 0), (0, -128), (0, H), (-4096, 4096)):                 # wholly outside
            recs.append(scene(g, [(1, x, y)]))
        recs.append(scene(g, [(1, 3, 2), (5, 40, 30), (3, -20, H - 100), (4, W - 100, -30)]))
        recs.append(scene(g, [(5, 40, 30), (1, 3, 2), (4, W - 100, -30), (3, -20, H - 100)]))
    return np.concatenate(recs)


# A bank for the sampler: names of CHAR_LIST and of the ontology; Pikachu's Jab renders are below the reference's 100-pixel
# rule (one in width, one in height), so characters drawn from them are skipped.
def sampler_tree():
    big = [make_render(120, 110, "random"), make_render(300, 175, "full"), make_render(350, 100, "254")]
    small = [make_render(99, 150, "random"), make_render(150, 99, "random")]
    return {
        "Pikachu": {"Jab": {"c00": {"c05attack11": {"0": small}}},
                    "Grabbed": {"c00": {"c05capture": {"0": big[:1], "1": big[1:2]}}}},
        "Joker": {"UpSmash": {"c00": {"c05attackhi4": {"0": big}}}},
    }
