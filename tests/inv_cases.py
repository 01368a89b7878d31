"""The matrix of the inverse-transform dispatch: one geometry per class of tests/inv_plan.py, three contents each.

Each geometry is the smallest of its class (by area, over every even size up to 1300x760 in all four formats) that the oracle
codes; tests/test_inv_plan_host.py checks that the classes here are exactly the ones the sweep finds.  The class each case is
there for is spelled out beside it (inv_plan.describe); the GPU module checks on the device that the plan's kernels ran.
"""
import numpy as np

import _cabi as A

F444, F422, F420, F411 = A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411

GEOMETRIES = [
    # w, h, fmt                 luma | chroma (patch kernel / part4 / strips) | fused border
    (32, 32, F444),           # general/l1a | patch | fb 1x1
    (32, 32, F422),           # general/l1a | patch | fb 2x1
    (32, 32, F420),           # general/l1a | patch | fb 2x2
    (32, 32, F411),           # general/l1a | patch | no fb
    (32, 34, F444),           # general/l1a | no-patch | no fb
    (32, 36, F444),           # general/l1a | patch, part4 | fb 1x1
    (32, 36, F422),           # general/l1a | patch, part4 | fb 2x1
    (32, 36, F411),           # general/l1a | patch, part4 | no fb
    (32, 40, F420),           # general/l1a | patch, part4 | fb 2x2
    (32, 66, F444),           # general/l1a | patch, bottom | no fb
    (34, 32, F444),           # general/no-l1a | no-patch | no fb
    (40, 36, F444),           # general/no-l1a | patch, part4 | no fb
    (40, 66, F444),           # general/no-l1a | patch, bottom | no fb
    (62, 32, F411),           # general/no-l1a | patch | no fb
    (64, 32, F411),           # general/l1a | patch | fb 4x1
    (64, 36, F411),           # general/l1a | patch, part4 | fb 4x1
    (130, 32, F444),          # general/no-l1a | patch, right | no fb
    (130, 36, F444),          # general/no-l1a | patch, part4, right | no fb
    (130, 66, F444),          # general/no-l1a | patch, right, bottom | no fb
    (144, 74, F444),          # fast, strips | patch, bottom | no fb
    (144, 74, F420),          # fast, strips | no-patch | no fb
    (144, 76, F444),          # fast, strips | patch, part4 | fb 1x1
    (144, 76, F422),          # fast, strips | patch, part4 | no fb
    (144, 80, F444),          # fast eb, strips | patch | fb 1x1
    (144, 80, F422),          # fast eb, strips | patch | no fb
    (144, 80, F411),          # fast eb, strips | no-patch | no fb
    (144, 88, F420),          # fast eb, strips | patch, part4 | no fb
    (144, 136, F444),         # fast, strips | patch | fb 1x1
    (144, 136, F422),         # fast, strips | patch | no fb
    (160, 76, F422),          # fast, strips | patch, part4 | fb 2x1
    (160, 80, F422),          # fast eb, strips | patch | fb 2x1
    (160, 80, F420),          # fast eb, strips | patch | fb 2x2
    (160, 88, F420),          # fast eb, strips | patch, part4 | fb 2x2
    (160, 136, F422),         # fast, strips | patch | fb 2x1
    (160, 136, F420),         # fast, strips | patch, part4 | fb 2x2
    (192, 76, F411),          # fast, strips | patch, part4 | fb 4x1
    (192, 80, F411),          # fast eb, strips | patch | fb 4x1
    (192, 136, F411),         # fast, strips | patch | fb 4x1
    (256, 74, F444),          # fast er, strips | patch, bottom | no fb
    (256, 74, F420),          # fast er, strips | no-patch | no fb
    (256, 76, F444),          # fast er, strips | patch, part4 | fb 1x1
    (256, 76, F422),          # fast er, strips | patch, part4 | fb 2x1
    (256, 76, F411),          # fast er, strips | patch, part4 | fb 4x1
    (256, 80, F444),          # fast er eb | patch | fb 1x1
    (256, 80, F422),          # fast er eb | patch | fb 2x1
    (256, 80, F420),          # fast er eb | patch | fb 2x2
    (256, 80, F411),          # fast er eb | patch | fb 4x1
    (256, 88, F420),          # fast er eb | patch, part4 | fb 2x2
    (256, 136, F444),         # fast er, strips | patch | fb 1x1
    (256, 136, F422),         # fast er, strips | patch | fb 2x1
    (256, 136, F420),         # fast er, strips | patch, part4 | fb 2x2
    (256, 136, F411),         # fast er, strips | patch | fb 4x1
    (264, 32, F422),          # general/l1a | patch, right | no fb
    (264, 40, F420),          # general/l1a | patch, part4, right | no fb
    (264, 70, F422),          # general/l1a | patch, right, bottom | no fb
    (264, 78, F422),          # fast, strips | patch, right, bottom | no fb
    (264, 80, F422),          # fast eb, strips | patch, right | no fb
    (264, 88, F420),          # fast eb, strips | patch, part4, right | no fb
    (264, 136, F422),         # fast, strips | patch, right | no fb
    (264, 136, F420),         # fast, strips | patch, part4, right | no fb
]

NFRAMES = 4
# every inter candidate stays a P picture: no scene cuts, no intra decision (intra share above 100 %), one GOP
CODING = dict(gop=12, rc_mode_cli=1, scd=0, ipct=101)
CONTENTS = {
    # strong per-pixel noise, new in every frame: every patch of every tile has a residual -- the general path everywhere
    "dense": dict(style=7, qp=95),
    # a static scene with a small square moving over it: empty tiles next to tiles with a residual
    "sparse": dict(style=11, qp=85),
    # pan + texture at a coarse quantiser: the luma smoothing filter changes pixels (tests/test_inv_plan_host.py shows it)
    "coarse": dict(style=0, qp=35),
}


def cli(content):
    return dict(CODING, qp=CONTENTS[content]["qp"])


def make_content(w, h, fmt, content, seed):
    """the clip (NFRAMES, frame bytes) of one content at one geometry"""
    style = CONTENTS[content]["style"]
    if style != 11:
        return A.gen_clip(w, h, fmt, seed, NFRAMES, style=style)
    # style 11 of test_gpu_recon.make_clip, with the square scaled down to half the picture's short side where 40 does not fit
    s = 40 if min(w, h) >= 64 else min(w, h) // 2
    clip = np.repeat(A.gen_clip(w, h, fmt, seed, 1, style=0), NFRAMES, axis=0)
    for t in range(NFRAMES):
        y = clip[t, :w * h].reshape(h, w)
        x0, y0 = (40 + 23 * t) % (w - s - 8), (24 + 9 * t) % (h - s - 8)
        y[y0:y0 + s, x0:x0 + s] = (37 * t + np.arange(s)[None, :] * 5 + np.arange(s)[:, None] * 3) % 256
    return clip


def case_id(g):
    w, h, fmt = g
    return "%dx%d_%s" % (w, h, {F444: "444", F422: "422", F420: "420", F411: "411"}[fmt])
