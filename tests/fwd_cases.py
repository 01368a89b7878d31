"""The matrix of the forward and motion-search dispatch: per value of each independent axis of tests/fwd_plan.py one geometry,
four contents each.

Luma, the chroma pair and the motion search are launched independently, so the list holds every VALUE of each axis (luma branch,
chroma branch, fusable x format, motion-search class), not their product.  Each geometry is the smallest of its value (by area,
over fwd_plan's sweep in all four formats) that the oracle codes as one I picture followed by P pictures;
tests/test_fwd_plan_host.py checks that the values here are exactly the ones the sweep finds.  The I path (k_fwd_b4t<true> +
k_fwd_haar_mid<2, true>) has one value; every case's first picture takes it.
"""
import ctypes as C
import json
import os

import numpy as np

import _cabi as A
import fwd_plan as P
import inv_cases as IC

F444, F422, F420, F411 = A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411

GEOMETRIES = [
    (32, 32, F444),           # chroma -|-; fusable yes 444; hme (0, '0', '0', 'none'); luma -|-
    (32, 32, F422),           # fusable yes 422
    (32, 32, F420),           # fusable yes 420
    (32, 32, F411),           # fusable no 411
    (32, 34, F444),           # chroma T+B|-; luma T+B|-
    (32, 34, F420),           # chroma row1|-
    (34, 32, F444),           # chroma whole; luma whole
    (42, 32, F422),           # chroma -|col1
    (42, 34, F422),           # chroma T+B|col1
    (42, 34, F420),           # chroma row1|col1
    (46, 32, F444),           # luma -|col1
    (46, 34, F444),           # luma T+B|col1
    (32, 78, F420),           # chroma B|-
    (42, 78, F420),           # chroma B|col1
    (32, 354, F420),          # fusable no 420
    (354, 32, F422),          # fusable no 422
    (708, 32, F411),          # fusable yes 411 (706x32: the oracle dies)
    (734, 32, F444),          # chroma -|L+R; luma -|L+R
    (734, 34, F444),          # chroma T+B|L+R; luma T+B|L+R
    (1342, 32, F422),         # chroma -|R
    (1338, 34, F420),         # chroma row1|L+R
    (1342, 34, F422),         # chroma T+B|R
    (1342, 34, F420),         # chroma row1|R
    (1338, 78, F420),         # chroma B|L+R
    (1342, 78, F420),         # chroma B|R
    (1282, 706, F444),        # hme (8, '1+2', '3', 'table')
    (1344, 736, F444),        # hme (8, '1', '3', 'table')
    (1282, 994, F444),        # hme (8, '1+2', '0/3', 'table')
    (1282, 1026, F444),       # hme (12, '1+2', '3', 'table')
    (1344, 1024, F444),       # hme (8, '1', '0/3', 'table')
    (1344, 1056, F444),       # hme (12, '1', '3', 'table')
    (1282, 1282, F444),       # hme (16, '1+2', '3', 'table')
    (1344, 1344, F444),       # hme (16, '1', '3', 'table')
    (4160, 706, F444),        # hme (8, '1+2', '0/3', 'early-out')
    (4160, 736, F444),        # hme (8, '1', '0/3', 'early-out')
]

# Smaller geometries of a value that were left out when the cases were selected, because the oracle and the compiled reference die
# on them (signal 8 while coding the first P picture: the 1-pixel-wide chroma edge block of DESIGN.md section 3);
# tests/test_fwd_plan_host.py shows both in child processes.  (tests/golden/ref_crash_skips.json is written by
# tools/make_goldens.py from the fuzz and extreme cases and parametrises tests/test_gpu_robustness.py by their ids, so this
# geometry, which is neither, is kept here.)
ORACLE_DIES = [(706, 32, F411)]

NFRAMES = IC.NFRAMES
CODING = IC.CODING
CONTENTS = {
    # the lean kernel's H.sparse test (k_sbt.hip:879) needs both outcomes: a residual in every patch / empty patches beside them
    "dense": IC.CONTENTS["dense"],
    "sparse": IC.CONTENTS["sparse"],
    # true motion in half-pel units, the halves of the picture moving apart and together again: vectors of all four phases, and
    # at every edge blocks whose vector points out of the picture
    "motion": dict(style="halfpel", qp=85),
    # a share of the P blocks intra (clip style 4): k_mc by list, the general kernel's intra patches
    "intra": dict(style=4, qp=85),
}
# The motion content: a smooth texture synthesised at twice the picture's resolution and sampled at a per-frame offset, as
# halfpel_cases does, but with the four QUADRANTS of the picture moving apart in the first P picture, together again in the
# second and apart the other way round in the third.  Per quadrant (left / right, top / bottom) the step in half-pel units (x, y)
# away from the centre: all four half-pel phases side by side in ONE picture, and in the diverging or in the converging picture
# (whichever way the search's vectors point) a vector that leaves the picture at every edge.
MOTION_OUT = {(0, 0): (-3, -2), (1, 0): (2, -3), (0, 1): (-3, 3), (1, 1): (2, 2)}        # phases (1,0) (0,1) (1,1) (0,0)
MOTION_SIGNS = [1, -1, -1]                                                                # frame t's step = sign * MOTION_OUT


def _field(rng, W2, H2):
    """halfpel_cases._field's texture (ten sinusoids + a little noise) by outer products: sin(a + b) = sin a cos b + cos a sin b"""
    xx, yy = np.arange(W2, dtype=np.float64), np.arange(H2, dtype=np.float64)
    f = np.zeros((H2, W2))
    for _ in range(10):
        fx, fy = rng.uniform(0.004, 0.09, 2) * rng.choice([-1, 1], 2)
        amp, a, b = rng.uniform(10, 30), 2 * np.pi * fx * xx + rng.uniform(0, 6.28), 2 * np.pi * fy * yy
        f += amp * (np.outer(np.cos(b), np.sin(a)) + np.outer(np.sin(b), np.cos(a)))
    f += rng.normal(0, 2.0, f.shape)
    return np.clip(128 + f, 0, 255)


def motion_clip(w, h, fmt, seed, nframes=None):
    n = NFRAMES if nframes is None else nframes
    rng = np.random.default_rng(seed)
    offs = {q: np.cumsum(np.array([(0, 0)] + [(sg * d[0], sg * d[1]) for sg in MOTION_SIGNS[:n - 1]]), axis=0) for q, d in MOTION_OUT.items()}
    pad = 16
    cw, ch = A.chroma_dims(w, h, fmt)
    sx, sy = w // cw, h // ch
    dims = [(w, h), (cw, ch), (cw, ch)]
    fields = [_field(rng, 2 * pw + 2 * pad, 2 * ph + 2 * pad) for pw, ph in dims]
    out = np.empty((n, A.frame_bytes(w, h, fmt)), np.uint8)
    for t in range(n):
        planes = []
        for c, (pw, ph) in enumerate(dims):
            img = np.empty((ph, pw))
            for (qx, qy), o in offs.items():
                ox, oy = o[t]
                if c:
                    ox, oy = int(round(ox / sx)), int(round(oy / sy))
                full = fields[c][pad + oy:pad + oy + 2 * ph:2, pad + ox:pad + ox + 2 * pw:2]
                x0, x1 = (0, pw // 2) if qx == 0 else (pw // 2, pw)
                y0, y1 = (0, ph // 2) if qy == 0 else (ph // 2, ph)
                img[y0:y1, x0:x1] = full[y0:y1, x0:x1]
            planes.append(np.rint(img).astype(np.uint8).ravel())
        out[t] = np.concatenate(planes)
    return out


def contents_of(g):
    """the contents a geometry is run with: all four where the strip axes live; the pictures of 64-wide blocks (about a megapixel
    and more: there for the motion search's classes, and the oracle's time) take the motion content and the dense one"""
    return ["dense", "motion"] if g[0] > 1280 and g[1] > 704 else list(CONTENTS)


def cli(content):
    return dict(CODING, qp=CONTENTS[content]["qp"])


def make_content(w, h, fmt, content, seed):
    """the clip (NFRAMES, frame bytes) of one content at one geometry"""
    if content in IC.CONTENTS:
        return IC.make_content(w, h, fmt, content, seed)
    if content == "motion":
        return motion_clip(w, h, fmt, seed)
    return A.gen_clip(w, h, fmt, seed, NFRAMES, style=CONTENTS[content]["style"])


def seed_of(g):
    return 0x1A7 + 7 * g[0] + g[1]


def case_id(g):
    return IC.case_id(g)


def crash_listed(g):
    """the geometry is one on which the reference itself dies (tests/golden/ref_crash_skips.json, the fuzz entries): such
    geometries are left out when the cases are selected"""
    with open(os.path.join(A.ROOT, "tests", "golden", "ref_crash_skips.json")) as f:
        keys = json.load(f)
    return any(k.startswith("fuzz:%dx%d_f%d_" % g) for k in keys)


def oracle_fields(clip, w, h, fmt, **kw):
    """the oracle encoder's final motion field of every picture after the first: [(nbv, nbh) array of A.MV_DTYPE]"""
    L = A.load_orc()
    cfg = A.orc_cfg(w, h, fmt, **kw)
    e = L.orc_enc_open(C.byref(cfg))
    L.orc_enc_set_next_fnum(e, 0)
    out, n, cap = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
    nbh, nbv = P.block_dims(w, h)[2:]
    fields = []
    for t in range(clip.shape[0]):
        L.orc_enc_frame(e, clip[t].ctypes.data, C.byref(out), C.byref(n), C.byref(cap), None)
        cnt = C.c_int(0)
        p = L.orc_enc_last_mvs(e, C.byref(cnt))
        if t == 0:
            continue
        assert p and cnt.value == nbh * nbv, (t, cnt.value, nbh, nbv)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cnt.value * 12,)).copy().view(A.MV_DTYPE)
        fields.append(a.reshape(nbv, nbh))
    C.CDLL(None).free(out)
    L.orc_enc_close(e)
    return fields


def field_facts(f, w, h):
    """of one picture's motion field: (luma half-pel phases present {(xh, yh)}, edges {'L','R','T','B'} with an inter block
    whose vector points out of the picture, edges with an inter block whose vector is not zero, intra blocks)"""
    bw, bh, nbh, nbv = P.block_dims(w, h)
    inter = f["mode"] == 0
    x, y = f["x"].astype(int), f["y"].astype(int)
    phases = {(int(a) & 1, int(b) & 1) for a, b in zip(x[inter], y[inter])}
    nz = inter & ((x != 0) | (y != 0))
    # the predicted block's first / last column and row (bmc.c: the reference position is the block's plus the vector's full-pel part,
    # the half-pel part reads one sample further)
    x0, y0 = np.arange(nbh)[None, :] * bw + (x >> 1), np.arange(nbv)[:, None] * bh + (y >> 1)
    out = {"L": inter[:, 0] & (x0[:, 0] < 0), "R": inter[:, -1] & (x[:, -1] > 0) & (x0[:, -1] + bw + (x[:, -1] & 1) > w),
           "T": inter[0, :] & (y0[0, :] < 0), "B": inter[-1, :] & (y[-1, :] > 0) & (y0[-1, :] + bh + (y[-1, :] & 1) > h)}
    edge_nz = {"L": nz[:, 0], "R": nz[:, -1], "T": nz[0, :], "B": nz[-1, :]}
    return phases, {k for k, v in out.items() if v.any()}, {k for k, v in edge_nz.items() if v.any()}, int((~inter).sum())
