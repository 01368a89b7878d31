"""What the debug-overlay tests share: the stream fixtures (tests/test_drawinfo_host.py pins the definition to the reference on them,
tests/test_gpu_drawinfo.py decodes them on the GPU; tests/golden/drawinfo.json holds the reference's -drawinfo7 hashes, made by
tools/make_drawinfo_goldens.py) and the synthetic block tables of the kernel test (also walked on the host under a sanitizer:
tools/drawvec_host.cpp, tools/drawvec_dump.py)."""
import json
import os

import numpy as np

import _cabi as A
import _drawinfo as DI

GOLDEN = os.path.join(A.ROOT, "tests", "golden", "drawinfo.json")
FRAMES = 6
CLI = ["-gop12", "-qp85", "-rc_mode1"]
KW = dict(qp=85, gop=12, rc_mode_cli=1)
# name -> (w, h, clipgen seed): 4:2:0, clipgen style 1, dimensions that are multiples of the block size the encoder picks
STREAMS = {
    "96x64": (96, 64, 0xD1A001),
    "352x288": (352, 288, 0xD1A002),
    "384x240": (384, 240, 0xD1A003),
    "768x384": (768, 384, 0xD1A004),
}
# the first frame taken from the generator's clip.  At 352x288 the first frames of a style-1 clip give intra blocks with full
# submasks only (480 seeds tried); from frame 21 on the flat objects have moved far enough for partial ones.
START = {"352x288": 21}


def stream_clip(name, fmt=A.SUBSAMP_420, frames=FRAMES):
    w, h, seed = STREAMS[name]
    return A.gen_clip(w, h, fmt, seed, frames, style=1, start=START.get(name, 0))


def goldens():
    with open(GOLDEN) as f:
        return json.load(f)


def picture_packets(stream):
    return [p for p in A.split_packets(stream) if p[5] & 4]


def define(pkg, stream, plain, w, h, mode):
    """the definition applied to the plain decode [frames][frame_bytes] of `stream`, picture by picture, from packet_blockinfo"""
    out = np.array(plain, dtype=np.uint8, copy=True).reshape(len(plain), -1)
    pics = picture_packets(stream)
    assert len(pics) == out.shape[0]
    for t, p in enumerate(pics):
        bw, bh, has_ref, info = pkg.packet_blockinfo(p, w, h)
        if has_ref and mode:
            DI.draw_info(out[t, :w * h].reshape(h, w), bw, bh, info, mode)
    return out


# ---- synthetic tables of the kernel test: n = 3 pictures with different tables ----
KERNEL_GEOMS = [(96, 64, 16, 16), (100, 70, 16, 16), (120, 80, 24, 16), (130, 100, 64, 48)]
# what every case's traces must show at mode 7, over its three pictures together
CONFLICTS = ["later_vec_over_dot", "later_vec_over_dash", "dot_over_earlier_vec", "dash_over_earlier_vec", "own_vec_over_dash",
             "leaves_left", "leaves_right", "leaves_top", "leaves_bottom", "zero_vec"]


def _dot(i, j, bw, bh, bit):
    return i * bw + bw * (3 if bit & 1 else 1) // 4, j * bh + bh * (3 if bit & 2 else 1) // 4


def _centre(i, j, bw, bh):
    return i * bw + bw // 2, j * bh + bh // 2


def kernel_tables(w, h, bw, bh):
    """three tables [3][nblk] of BLOCKINFO.
    Picture 0, the conflicts: blocks 0 = (0, 0) and (1, 1) are intra with all four dots and stable; their neighbours' vectors are aimed
    from their block centres through a dot and through an odd dash pixel of each (twice the way there, so the pixel lies well inside the
    walk): blocks (1, 0) and (2, 1) come after block 0 -- a later vector over an earlier dot / dash --, blocks (0, 1) and (2, 0) come
    before block (1, 1) -- a later dot / dash over an earlier vector.  Every other block is intra without a dash.
    Picture 1, the walks: a block's own horizontal vector over its own dash, exits through the four sides, a zero vector, +-2048 and
    (32767, -32768); the other blocks a fixed mixture.  Picture 2: a seeded random table with vectors up to +-3000."""
    nbh, nbv = DI.nblocks(w, h, bw, bh)
    nblk = nbh * nbv
    assert nbh >= 3 and nbv >= 2 and nblk >= 9 and 2 * bw <= w and 2 * bh <= h
    T = np.zeros((3, nblk), dtype=DI.BLOCKINFO)

    def aim(src, tx, ty):
        cx, cy = _centre(src % nbh, src // nbh, bw, bh)
        return 2 * (tx - cx), 2 * (ty - cy), 0, 0, 0, 0

    for b in range(nblk):
        T[0][b] = (0, 0, 1, (b * 7 + 3) & 0xF, 0, 0)
    tb = nbh + 1
    T[0][0] = T[0][tb] = (0, 0, 1, 0xF, 1, 0)
    c0, c1 = _centre(0, 0, bw, bh), _centre(1, 1, bw, bh)
    T[0][1] = aim(1, *_dot(0, 0, bw, bh, 3))
    T[0][nbh + 2] = aim(nbh + 2, c0[0] + 1, c0[1])
    T[0][nbh] = aim(nbh, *_dot(1, 1, bw, bh, 0))
    T[0][2] = aim(2, c1[0] - 1, c1[1])
    walks = [(bw, 0, 1), (-4 * w, 0, 0), (4 * w, 3, 0), (0, -4 * h, 0), (-3, 4 * h, 0), (0, 0, 0), (2048, -2048, 1), (-2048, 2048, 0),
             (32767, -32768, 0)]
    for b in range(nblk):
        if b < len(walks):
            T[1][b] = (walks[b][0], walks[b][1], 0, 0, walks[b][2], 0)
        elif b % 3 == 0:
            T[1][b] = (0, 0, 1, (b * 5 + 1) & 0xF, b & 1, 0)
        else:
            T[1][b] = ((b * 5) % 23 - 11, (b * 3) % 17 - 8, 0, 0, (b >> 1) & 1, 0)
    rng = np.random.default_rng(w * 1000 + h)
    for b in range(nblk):
        if rng.integers(0, 3) == 0:
            T[2][b] = (0, 0, 1, int(rng.integers(0, 16)), int(rng.integers(0, 2)), 0)
        else:
            T[2][b] = (int(rng.integers(-3000, 3001)), int(rng.integers(-3000, 3001)), 0, 0, int(rng.integers(0, 2)), 0)
    return T
