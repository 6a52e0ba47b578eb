"""The cases of the history-clipping tests, shared by tests/test_clip_cpu.py (the reference alone:
teeth and premises) and tests/test_gpu_clip.py (the library against the reference): frames of
test_gpu_temporal's synthetic three-patch scene with seeded random colours and two speck pixels
(clip_ref.speck: no similar neighbour, so no box), the cameras they are seen from, the clip's
settings, and the real cases of the three other entry points, which are their own tests' cases."""
import numpy as np

from tests import clip_ref as CR
from tests import temporal_ref as TR
from tests import test_gpu_temporal as G

PARAMS = G.PARAMS                   # alpha 0.1, depth_tol 0.1, normal_min 0.9, max_history 32
CLIP = dict(radius=3, gamma=1.0, max_history=4)
TILES = 0x2                         # TPT_TEMPORAL_TILES
FOURTH = dict(yaw_deg=4.5, translate=(0.39, 0.15, 0.06))

# name -> (W, H, second camera's arguments, radius, demodulate, launch flags).  37 x 29: the odd
# size of the other temporal tests; 131 x 9: three 64-pixel row segments; 5 x 3: a frame smaller
# than a radius-3 window (and than a radius-1 window's rows: every window is cut by the frame);
# 70 x 70 in 16 x 16 tiles: 5 x 5 tiles, the last ones partial.  Both radii, both demodulate
# settings and both launch shapes occur; radius 2 is the loose-box test's.
TWO_FRAME = {
    "static_r3": (37, 29, {}, 3, True, 0),
    "static_r1_plain": (37, 29, {}, 1, False, 0),
    "translate_r1": (37, 29, dict(translate=G.MOVE), 1, True, 0),
    "translate_r3_plain_tiles": (37, 29, dict(translate=G.MOVE), 3, False, TILES),
    "pitch_roll_r3": (37, 29, G.PITCH_ROLL, 3, True, 0),
    "pitch_roll_r1_tiles": (37, 29, G.PITCH_ROLL, 1, True, TILES),
    "131x9_r3": (131, 9, G.PITCH_ROLL, 3, True, 0),
    "131x9_r1_plain": (131, 9, G.PITCH_ROLL, 1, False, 0),
    "5x3_r3": (5, 3, dict(translate=(0.05, 0.02, 0.0)), 3, True, 0),
    "5x3_r1_tiles": (5, 3, {}, 1, False, TILES),
    "70x70_r3_tiles": (70, 70, G.PITCH_ROLL, 3, True, TILES),
}
# The four-frame chain at 37 x 29 (test_gpu_temporal's chain cameras and one more): history lengths
# above the cap, so the cap acts from frame 3 on (clip max_history 1) and the moments' shift
# is carried through blended histories.
CHAIN_CAMERAS = (dict(), dict(yaw_deg=1.5, translate=G.MOVE), dict(yaw_deg=3.0, translate=(0.26, 0.10, 0.04)), FOURTH)
CHAIN_CLIP = dict(radius=3, gamma=1.0, max_history=1)
# Frames of at least 1,000 pixels must show at least 20 reprojected pixels on either side of the
# clip; the 5 x 3 frame has 15 pixels in all and must show one on either side.
MIN_SIDE = lambda w, h: 20 if w * h >= 1000 else 1


def frame(cam, seed, w, h):
    """test_gpu_temporal.frame on the three-material scene (black = None: the middle hit pixel
    has albedo 0, so demodulation divides by the floor) with the two specks."""
    rad, aov = G.frame(cam, seed, w, h, (0, 1, 2), black=None)
    return rad, CR.speck(aov)


def two_frames(name):
    """The case's cameras, frames, temporal parameters, clip setting and launch flags."""
    w, h, cam2, radius, demodulate, flags = TWO_FRAME[name]
    cams = (TR.camera(aspect=w / h), TR.camera(aspect=w / h, **cam2))
    frames = (frame(cams[0], 101, w, h), frame(cams[1], 202, w, h))
    return cams, frames, dict(PARAMS, demodulate=demodulate), dict(CLIP, radius=radius), flags


def chain():
    w, h = G.W, G.H
    cams = tuple(TR.camera(aspect=w / h, **kw) for kw in CHAIN_CAMERAS)
    frames = tuple(frame(c, 101 * (k + 1), w, h) for k, c in enumerate(cams))
    return cams, frames, dict(PARAMS, demodulate=True), CHAIN_CLIP, 0


def reference(cams, frames, params, clip, _without=None):
    """The chain of clipped tpt_temporal calls through temporal_ref; one result per frame."""
    refs, state = [], None
    for cam, (rad, aov) in zip(cams, frames):
        refs.append(TR.temporal_ref(state, cam, rad, aov, clip=clip, _without=_without, **params))
        state = refs[-1]["state"]
    return refs


def premises(tag, ref, w, h):
    """What a clipped case's frame must show for the GPU comparison to mean something; returns the counts."""
    dec, rep, cl = ref["decidable"], ref["reprojected"], ref["clipped"]
    counts = dict(clipped=int((rep & cl & dec).sum()), kept=int((rep & ~cl & dec).sum()), few=int((ref["n"] < 4).sum()),
                  undecidable=int((~dec).sum()))
    print(f"{tag}: {counts}")
    assert counts["clipped"] >= MIN_SIDE(w, h), tag
    assert counts["kept"] >= MIN_SIDE(w, h), tag
    assert counts["few"] >= 1, tag
    assert counts["undecidable"] <= 0.01 * w * h, tag
    return counts
