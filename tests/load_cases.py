"""The matrix of the source load: one geometry per class of tests/load_plan.py at each pyramid depth, three contents each.

Each case (w, h, fmt, pyramid_levels) is the smallest geometry of the classes listed beside it -- by area over every even size from
32x32 to 300x300 in all four formats, ties to the earlier format of load_plan.FORMATS, then the narrower picture -- at the default
switches and a 16-byte aligned source.  tests/test_load_plan_host.py checks that the classes here are exactly the ones the sweep finds
and that every value of every plan field occurs; tests/test_gpu_load_paths.py loads every case and compares every byte of every level
with the oracle.  A class is spelled as load_plan.classes() returns it: ("level0", (sides, fuse1, fuse2, sides1, sides2, bodies, level
0's border kernel, its tb_only)), ("upper", (border kernel, tb_only, ds2x, ds2x_sides, ds2x_tail, src_odd_w, src_odd_h)) of one level
above 0, ("sum", (luma_sum_dword,)).
"""
import numpy as np

import _cabi as A

F444, F422, F420, F411 = A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411

CASES = {
    # pyramid_levels = 0 (the encoder's own depth: 3 at these sizes)
    (32, 32, F444, 0): [
        ('level0', (1, 1, 1, 1, 0, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 110 | k_extend16 tb
        ('upper', ('k_extend', 0, 0, 0, 0, 0, 0)),                                     # upper: k_extend | fused
        ('upper', ('k_extend', 0, 1, 0, 0, 0, 0)),                                     # upper: k_extend | ds2x
        ('upper', ('k_extend16', 1, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 tb | fused
        ('sum', (1,)),                                                                 # sum: dword
    ],
    (32, 32, F411, 0): [
        ('level0', (0, 1, 1, 0, 0, ('fused2', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: fused2/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend16', 0, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 | fused
    ],
    (32, 34, F444, 0): [
        ('level0', (1, 1, 0, 1, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 110 | k_extend16 tb
        ('upper', ('k_extend', 0, 1, 0, 0, 0, 1)),                                     # upper: k_extend | ds2x oddh
    ],
    (34, 32, F444, 0): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: scalar/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend', 0, 1, 0, 1, 0, 0)),                                     # upper: k_extend | ds2x tail
        ('upper', ('k_extend', 0, 1, 0, 1, 1, 0)),                                     # upper: k_extend | ds2x tail oddw
        ('sum', (0,)),                                                                 # sum: scalar
    ],
    (32, 34, F411, 0): [
        ('level0', (0, 1, 0, 0, 0, ('fused1', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: fused1/scalar/scalar | sides 000 | k_extend
    ],
    (34, 34, F444, 0): [
        ('upper', ('k_extend', 0, 1, 0, 1, 1, 1)),                                     # upper: k_extend | ds2x tail oddw oddh
    ],
    (36, 34, F444, 0): [
        ('upper', ('k_extend', 0, 1, 0, 1, 0, 1)),                                     # upper: k_extend | ds2x tail oddh
    ],
    (46, 32, F444, 0): [
        ('upper', ('k_extend', 0, 1, 0, 0, 1, 0)),                                     # upper: k_extend | ds2x oddw
    ],
    (48, 32, F444, 0): [
        ('level0', (1, 1, 1, 0, 0, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 100 | k_extend16 tb
    ],
    (46, 34, F444, 0): [
        ('upper', ('k_extend', 0, 1, 0, 0, 1, 1)),                                     # upper: k_extend | ds2x oddw oddh
    ],
    (48, 34, F444, 0): [
        ('level0', (1, 1, 0, 0, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 100 | k_extend16 tb
    ],
    (62, 32, F444, 0): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 1, 0)),                                   # upper: k_extend16 tb | ds2x sides oddw
    ],
    (62, 32, F411, 0): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'v16', 'v16'), 'k_extend', 0)),          # level0: scalar/v16/v16 | sides 000 | k_extend
    ],
    (64, 32, F444, 0): [
        ('level0', (1, 1, 1, 1, 1, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 111 | k_extend16 tb
    ],
    (62, 34, F444, 0): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 1, 1)),                                   # upper: k_extend16 tb | ds2x sides oddw oddh
    ],
    (64, 34, F444, 0): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 0, 1)),                                   # upper: k_extend16 tb | ds2x sides oddh
    ],
    (126, 32, F444, 0): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 0, 0)),                                   # upper: k_extend16 tb | ds2x sides
    ],
    # pyramid_levels = 1
    (32, 32, F444, 1): [
        ('level0', (1, 1, 0, 1, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 110 | k_extend16 tb
        ('upper', ('k_extend16', 1, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 tb | fused
        ('sum', (1,)),                                                                 # sum: dword
    ],
    (32, 32, F411, 1): [
        ('level0', (0, 1, 0, 0, 0, ('fused1', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: fused1/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend16', 0, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 | fused
    ],
    (34, 32, F444, 1): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: scalar/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend', 0, 1, 0, 1, 0, 0)),                                     # upper: k_extend | ds2x tail
        ('sum', (0,)),                                                                 # sum: scalar
    ],
    (40, 32, F444, 1): [
        ('upper', ('k_extend', 0, 1, 0, 0, 0, 0)),                                     # upper: k_extend | ds2x
    ],
    (48, 32, F444, 1): [
        ('level0', (1, 1, 0, 0, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 100 | k_extend16 tb
        ('upper', ('k_extend', 0, 0, 0, 0, 0, 0)),                                     # upper: k_extend | fused
    ],
    (62, 32, F411, 1): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'v16', 'v16'), 'k_extend', 0)),          # level0: scalar/v16/v16 | sides 000 | k_extend
    ],
    # pyramid_levels = 2
    (32, 32, F444, 2): [
        ('level0', (1, 1, 1, 1, 0, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 110 | k_extend16 tb
        ('upper', ('k_extend', 0, 0, 0, 0, 0, 0)),                                     # upper: k_extend | fused
        ('upper', ('k_extend16', 1, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 tb | fused
        ('sum', (1,)),                                                                 # sum: dword
    ],
    (32, 32, F411, 2): [
        ('level0', (0, 1, 1, 0, 0, ('fused2', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: fused2/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend16', 0, 0, 0, 0, 0, 0)),                                   # upper: k_extend16 | fused
    ],
    (32, 34, F444, 2): [
        ('level0', (1, 1, 0, 1, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 110 | k_extend16 tb
        ('upper', ('k_extend', 0, 1, 0, 0, 0, 1)),                                     # upper: k_extend | ds2x oddh
    ],
    (34, 32, F444, 2): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: scalar/scalar/scalar | sides 000 | k_extend
        ('upper', ('k_extend', 0, 1, 0, 1, 0, 0)),                                     # upper: k_extend | ds2x tail
        ('upper', ('k_extend', 0, 1, 0, 1, 1, 0)),                                     # upper: k_extend | ds2x tail oddw
        ('sum', (0,)),                                                                 # sum: scalar
    ],
    (32, 34, F411, 2): [
        ('level0', (0, 1, 0, 0, 0, ('fused1', 'scalar', 'scalar'), 'k_extend', 0)),    # level0: fused1/scalar/scalar | sides 000 | k_extend
    ],
    (34, 34, F444, 2): [
        ('upper', ('k_extend', 0, 1, 0, 1, 1, 1)),                                     # upper: k_extend | ds2x tail oddw oddh
    ],
    (36, 34, F444, 2): [
        ('upper', ('k_extend', 0, 1, 0, 1, 0, 1)),                                     # upper: k_extend | ds2x tail oddh
    ],
    (40, 32, F444, 2): [
        ('upper', ('k_extend', 0, 1, 0, 0, 0, 0)),                                     # upper: k_extend | ds2x
    ],
    (46, 32, F444, 2): [
        ('upper', ('k_extend', 0, 1, 0, 0, 1, 0)),                                     # upper: k_extend | ds2x oddw
    ],
    (48, 32, F444, 2): [
        ('level0', (1, 1, 1, 0, 0, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 100 | k_extend16 tb
    ],
    (46, 34, F444, 2): [
        ('upper', ('k_extend', 0, 1, 0, 0, 1, 1)),                                     # upper: k_extend | ds2x oddw oddh
    ],
    (48, 34, F444, 2): [
        ('level0', (1, 1, 0, 0, 0, ('fused1', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused1/v16/v16 | sides 100 | k_extend16 tb
    ],
    (62, 32, F444, 2): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 1, 0)),                                   # upper: k_extend16 tb | ds2x sides oddw
    ],
    (62, 32, F411, 2): [
        ('level0', (0, 0, 0, 0, 0, ('scalar', 'v16', 'v16'), 'k_extend', 0)),          # level0: scalar/v16/v16 | sides 000 | k_extend
    ],
    (64, 32, F444, 2): [
        ('level0', (1, 1, 1, 1, 1, ('fused2', 'v16', 'v16'), 'k_extend16', 1)),        # level0: fused2/v16/v16 | sides 111 | k_extend16 tb
    ],
    (62, 34, F444, 2): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 1, 1)),                                   # upper: k_extend16 tb | ds2x sides oddw oddh
    ],
    (64, 34, F444, 2): [
        ('upper', ('k_extend16', 1, 1, 1, 0, 0, 1)),                                   # upper: k_extend16 tb | ds2x sides oddh
    ],
}

# the flag cases of dsvg_load_frames_map_ex (4:2:0, the encoder's own pyramid): a small geometry that takes chroma in place, the
# smallest that refuses it (odd chroma height), the smallest that takes luma in place (a ring of 4 x 16 columns and 16 x 4 rows, which
# leaves 64 x 64 inside)
CHROMA_IN_PLACE = (64, 32, F420, 0)
CHROMA_REFUSED = (32, 34, F420, 0)
LUMA_IN_PLACE = (192, 192, F420, 0)

NFRAMES = 3          # frames per clip: slots 0..2 of a context of 4 source slots


def case_id(c):
    w, h, fmt, pyramid = c
    return "%dx%d_%s_p%d" % (w, h, {F444: "444", F422: "422", F420: "420", F411: "411"}[fmt], pyramid)


def _planes(w, h, fmt, luma, chroma):
    """a packed planar frame from a luma picture and one chroma picture (both chroma planes alike but for an offset of 1 in x)"""
    return np.concatenate([luma.reshape(-1), chroma.reshape(-1), np.roll(chroma, 1, axis=1).reshape(-1)]).astype(np.uint8)


def make_content(w, h, fmt, content, seed):
    """the clip (NFRAMES, frame bytes) of one content at one geometry, chosen so that a wrong byte cannot hide:
      noise    uniform over 1..255: every neighbour differs (a border taken from column 1 shows) and nothing is 0 (an unwritten byte
               of the zeroed slab shows);
      checker  0 / 255: the one-pixel checkerboard, its other phase, and a lattice of lines three pixels apart, whose 2x2 means (with
               its complement's) are 0, 64, 128, 191 and 255 side by side -- carries between the lanes of the packed means, and level 2 rounded
               from the ROUNDED level 1;
      flat     255 everywhere (its complement, loaded second: 0 everywhere)."""
    cw, ch = A.chroma_dims(w, h, fmt)
    rng = np.random.default_rng(seed)
    frames = []
    for t in range(NFRAMES):
        def pic(pw, ph):
            y, x = np.mgrid[0:ph, 0:pw]
            if content == "noise":
                return rng.integers(1, 256, size=(ph, pw))
            if content == "checker":
                return (((x + y + t) & 1) if t < 2 else ((x % 3 == 0) | (y % 3 == 0))) * 255
            assert content == "flat"
            return np.full((ph, pw), 255)
        frames.append(_planes(w, h, fmt, pic(w, h), pic(cw, ch)))
    return np.stack(frames)


CONTENTS = ("noise", "checker", "flat")
