"""The cases of the entropy pack stage's branches (tests/hz_plan.py), found on the CPU, and how the oracle's entries are taken.

Two seams, two lists; each case names the labels of hz_plan.LABELS it is there for, and tests/test_hz_plan_host.py re-derives them
from the oracle on every run.

  * OP_CASES -- dsvg_op_encode_plane against orc_encode_plane: k_hz_quant<false>, the scan and the emit kernel with every chunk
    unpacked, on int32 coefficients built so that the oracle's symbols land where the labels need them (isolated values far apart,
    values of tens of thousands times the quantiser, long stretches of short codes, single entries in late chunks).  This seam
    owns the three tiers of emit_round64, the word-sharing labels and the plane labels.
  * PIPE_CASES -- pkg.Batch frame by frame: collect, the packed chunks' rounds, the list kernels.
  * TILE -- 33 streams of 2048x2080 on one coding stream: the 256-thread scan's second tile.

The entries come from the oracle's recorder (orc_hz_rec_*, oracle/orc_hzcc.c), never from the product.
"""
import ctypes as C

import numpy as np

import _cabi as A
import hz_plan as H
import inv_cases as IC

F444, F422, F420, F411 = A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's entries
def recorded(fn):
    """run fn() with the oracle's entry recorder armed: (fn's result, [plane record]) -- a record is a dict of w, h, isP, cur_plane,
    at (byte offset of the payload in the bit stream it was written to), bits, entries (n x 2 int32: scan position, value)"""
    L = A.load_orc()
    L.orc_hz_rec_arm.argtypes = [C.c_int]
    L.orc_hz_rec_read.restype = C.c_size_t
    L.orc_hz_rec_read.argtypes = [C.c_void_p, C.c_size_t]
    L.orc_hz_rec_arm(1)
    try:
        res = fn()
        n = L.orc_hz_rec_read(None, 0)
        words = np.zeros(max(n, 1), dtype=np.int32)
        assert L.orc_hz_rec_read(words.ctypes.data, n) == n
    finally:
        L.orc_hz_rec_arm(0)
    out, o = [], 0
    while o < n:
        w, h, isP, c, cnt, at, bits = (int(x) for x in words[o:o + 7])
        out.append(dict(w=w, h=h, isP=isP, cur_plane=c, at=at, bits=bits, entries=words[o + 7:o + 7 + 2 * cnt].reshape(-1, 2).copy()))
        o += 7 + 2 * cnt
    assert o == n
    return res, out


# ---------------------------------------------------------------------------------------------------------------------------
# operator seam
OP_Q = 16           # MINQUANT on an I plane with no stable block: symbol s = coefficient / 16 (levels 0, 1, LL) or >> 5 (level 2)


def op_coefs(w, h, entries):
    """int32 coefficient plane whose symbols under OP_Q are `entries` [(scan position, symbol)] (planes without region overlap)"""
    assert not H.overlaps(w, h)
    co = np.zeros((h, w), dtype=np.int32)
    for p, s in entries:
        x, y, level = H.cell_of(w, h, p)
        co[y, x] = s * 32 if level == 2 else s * 16
    return co.reshape(-1)


def _short(n0, n1):
    return [(p, ((p * 7) % 199) - 99 or 1) for p in range(n0, n1)]


def _phase(k, tail=3):
    """k entries of 1 at the end of chunk 0, one entry on the first cell of chunk 1, `tail` at the head of chunk 2: the bit phase
    of chunks 1 and 2 moves by three bits per k"""
    return [(p, 1) for p in range(2048 - k, 2048)] + [(2048, 1)] + [(4096 + 5 * i, -2) for i in range(tail)]


def _op_random(w, h, seed):
    rng = np.random.default_rng(seed)
    co = rng.laplace(0, 40, size=(h, w)).astype(np.int32)
    co[: h // 8, : w // 8] *= 16
    return co.reshape(-1)


# name -> (w, h, coefficients, labels).  128x128: 8 chunks; 64x64: 2; 8x8: 1 (64 cells); 256x160: 20 (40960 cells)
def op_cases():
    big = lambda e: op_coefs(256, 160, e)
    return {
        "empty": (8, 8, op_coefs(8, 8, []), ["pl.empty"]),
        "one": (8, 8, op_coefs(8, 8, [(5, 3)]), ["pl.one", "r64.nfull0", "w.single", "w.bit0", "un.one", "sc.1024"]),
        "short-codes": (64, 64, op_coefs(64, 64, _short(1, 4096)), ["r64.tier8", "un.many", "w.first_shared", "w.last_shared"]),
        # chunk 0: six entries 300 cells apart (second tier by the run alone); chunk 2: 128 entries of 20000, 15 cells apart -- its
        # second round has the values alone at 37 bits an entry: 74 words, the stage's second half
        "tier15": (128, 128, op_coefs(128, 128, [(300 * (i + 1), 1) for i in range(6)] + [(4096 + 15 * i, 20000 if i & 1 else -20000) for i in range(128)]),
                   ["r64.tier15.run", "r64.tier15.mag", "r64.tier15.half2"]),
        # one entry in chunk 0, the next 36889 cells on in chunk 18 (third tier by the run alone, 17 empty chunks crossed), then
        # -40000 in chunk 19 and an entry after it (third tier by the value alone)
        "tier31": (256, 160, big([(10, 5), (36900, 7), (38950, -40000), (38951, 1)]), ["r64.tier31.run", "r64.tier31.mag", "pl.run_gt16"]),
        "late-single": (128, 128, op_coefs(128, 128, [(5 * 2048 + 77, -9)]), ["pl.one", "pl.first_ne_not_0", "pl.last_ne_not_last"]),
        # the phase family (search_phases below found the k): chunk 1's single entry is 3 bits
        "phase-single-both": (128, 128, op_coefs(128, 128, _phase(PHASE_K["w.single_both"])), ["w.single_both", "w.single", "w.first_shared", "w.last_shared"]),
        "phase-endword": (128, 128, op_coefs(128, 128, _phase(PHASE_K["w.endword"])), ["w.endword", "w.bit0"]),
        "phase-endword-single": (128, 128, op_coefs(128, 128, _phase(PHASE_K["w.endword+w.single..."])), ["w.endword", "w.bit0", "w.first_shared"]),
        # region overlap (36 = 4 mod 8, 20 = 4 mod 8), random coefficients
        "overlap": (36, 20, _op_random(36, 20, 11), ["un.many"]),
        "random-100x52": (100, 52, _op_random(100, 52, 12), ["un.many", "r64.tier8"]),
    }


# k of _phase(k) for the labels that depend on the bit phase: chunk 0 holds len_ueg(2047 - k) + 3 (k - 1) bits, chunk 1 three.
#   w.single_both          chunk 1 (3 bits) starts past bit 0 of a word and ends inside it
#   w.endword              chunk 0 ends on a word boundary (chunk 1 then starts at bit 0)
#   w.endword+w.single...  chunk 1 ends on a word boundary: it fills the last 3 bits of a word (nfull == 1, carry 0)
PHASE_K = {"w.single_both": 1, "w.endword": 26, "w.endword+w.single...": 25}


def search_phases(kmax=64):
    """(not called by the tests) the smallest k of _phase(k) per PHASE_K key, from the oracle's entries and the model"""
    found = {}
    for k in range(1, kmax):
        pl = op_plane(128, 128, op_coefs(128, 128, _phase(k)))[0]
        c0, c1 = pl.chunks[0], pl.chunks[1]
        for key, hit in (("w.single_both", "w.single_both" in c1.labels), ("w.endword", "w.endword" in c0.labels),
                         ("w.endword+w.single...", "w.endword" in c1.labels and "w.first_shared" in c1.labels)):
            if hit:
                found.setdefault(key, k)
    return found


def op_stab(w, h):
    """the stability argument of the operator cases: an I plane 0 with no stable block"""
    bw, bh, nbh, nbv = A.block_dims(w, h)
    meta = A.Meta(w, h, A.SUBSAMP_420, 30, 1, 1, 1)
    prm = A.Params(C.pointer(meta), 1, 0, bw, bh, nbh, nbv)
    sb = np.zeros(nbh * nbv, dtype=np.uint8)
    return A.Stability(C.pointer(prm), A.u8p(sb), 0, 0), (meta, prm, sb)


def op_encode(L, fn, w, h, coefs):
    """fn = 'orc_encode_plane' | 'dsvg_op_encode_plane' on a copy of coefs: (packed bytes, coefficients after)"""
    st, keep = op_stab(w, h)
    co = coefs.copy()
    buf = np.zeros(w * h * 8 + 64, dtype=np.uint8)
    bs = A.BS(A.u8p(buf), 0)
    rc = getattr(L, fn)(C.byref(bs), C.byref(A.Coefs(A.i32p(co), w, h)), OP_Q, C.byref(st))
    if fn.startswith("dsvg"):
        A.chk(L, rc)
    assert bs.pos % 8 == 0
    return buf[:bs.pos // 8].tobytes(), co


def op_plane(w, h, coefs):
    """(model of the plane, oracle's packed bytes, oracle's coefficients after, the plane's record)"""
    (buf, co), recs = recorded(lambda: op_encode(A.load_orc(), "orc_encode_plane", w, h, coefs))
    assert len(recs) == 1
    return H.Plane(w, h, recs[0]["entries"], "I", "op", 1), buf, co, recs[0]


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline seam
CODING = IC.CODING          # one I picture, then P pictures only


def _planes(w, h, fmt, y, c=None):
    cw, ch = A.chroma_dims(w, h, fmt)
    c = np.full((2, ch, cw), 128, dtype=np.uint8) if c is None else c
    return np.concatenate([y.astype(np.uint8).ravel(), c.astype(np.uint8).ravel()])


def make_content(w, h, fmt, content, seed, n):
    """the clip (n, frame bytes) of one content"""
    rng = np.random.default_rng(seed)
    cw, ch = A.chroma_dims(w, h, fmt)
    out = np.empty((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    if content == "static2":
        # a static textured scene with two small changed spots far apart (top left, bottom right), new in every P picture
        base = A.gen_clip(w, h, fmt, seed, 1, style=0)[0]
        for t in range(n):
            out[t] = base
            y = out[t, :w * h].reshape(h, w)
            if t:
                for x0, y0 in ((8, 4), (w - 24, h - 18)):
                    y[y0:y0 + 10, x0:x0 + 10] = rng.integers(0, 256, size=(10, 10))
        return out
    for t in range(n):
        if content == "noise":                               # full-range noise, new in every frame
            y, c = rng.integers(0, 256, size=(h, w)), rng.integers(0, 256, size=(2, ch, cw))
        elif content == "halfnoise":                         # ... in the left half, flat beside it (full-range noise all over does not fit the
            y, c = np.full((h, w), 128 + 8 * t), np.full((2, ch, cw), 128)      # oracle's packet bound of 2 bytes a pixel at top quality)
            y[:, :w // 2], c[:, :, :cw // 2] = rng.integers(0, 256, size=(h, w // 2)), rng.integers(0, 256, size=(2, ch, cw // 2))
        elif content == "soft":                              # noise of +-12: every chunk dense, every code short
            y, c = 128 + rng.integers(-12, 13, size=(h, w)), 128 + rng.integers(-12, 13, size=(2, ch, cw))
        elif content == "leftnoise":                         # soft noise in the left 192 columns, flat beside it: runs of 256 in the finest subbands' rows
            y, c = np.full((h, w), 128 + 8 * t), np.full((2, ch, cw), 128)
            y[:, :192] = 128 + rng.integers(-12, 13, size=(h, 192))
        elif content == "flat":
            y, c = np.full((h, w), 90 + 30 * t), np.full((2, ch, cw), 128 + t)
        elif content == "blocks":                            # coarse full-contrast structure: 32-pixel checkerboard, moved by a block per frame
            yy, xx = np.mgrid[0:h, 0:w]
            y = np.where((((xx // 32) + (yy // 32) + t) & 1) == 1, 255, 0)
            c = np.stack([y[::h // ch, ::w // cw][:ch, :cw]] * 2)
        else:
            raise ValueError(content)
        out[t] = _planes(w, h, fmt, y, c)
    return out


# (name, geometry, content, qp, frames, labels).  32x32 4:2:0: every plane one chunk (LL and all detail share it);
# 360x200: ll_end = 45 x 25 = 1125 (not a multiple of 4), chroma 180x100 with overlapping scan regions; 704x480: ll_end = 5280, two
# whole LL chunks before the straddling one; 704x64: leftnoise's runs
PIPE_CASES = [
    ("tiny-noise", (32, 32, F420), "noise", 100, 3, ["co.straddle.dense.detail", "co.straddle.sparse.flag", "co.short_last", "co.ll_end.8"]),
    ("tiny-flat", (32, 32, F420), "flat", 85, 3, ["co.straddle.dense.nodetail", "co.straddle.sparse.noflag"]),
    ("odd-ll-noise", (360, 200, F420), "halfnoise", 100, 3, ["co.ll_end.n4", "co.ll_end.n8", "co.dense", "co.sparse.flag", "pk.256s_tail", "pk.detour.mag", "pk.detour.first", "r64.tier15.mag"]),
    ("odd-ll-soft", (360, 200, F420), "soft", 100, 3, ["pk.r256", "pk.256s_tail", "pk.256s", "pk.129_256", "co.dense"]),
    ("odd-ll-static2", (360, 200, F420), "static2", 98, 3, ["co.sparse.noflag", "co.sparse.flag", "pk.le64", "pk.65_128", "co.straddle.sparse.noflag"]),
    ("ll-chunks-static2", (704, 480, F420), "static2", 98, 3, ["co.ll.whole", "pl.run_gt16", "pk.r64.tier31.run", "co.sparse.noflag"]),
    ("ll-chunks-blocks", (704, 480, F420), "blocks", 100, 2, ["co.ll.whole", "r64.tier15.mag"]),
    ("leftnoise", (704, 64, F420), "leftnoise", 100, 3, ["pk.detour.run", "pk.r256"]),
]
NOLLQ_CASES = ["tiny-noise", "odd-ll-noise"]                 # also under DSV1_NO_LLQ=1
NOLIST_CASES = ["odd-ll-static2", "odd-ll-noise"]            # also under DSV1_NO_LIST_PACK=1

_pipe = {}


def pipe_case(name):
    return next(c for c in PIPE_CASES if c[0] == name)


def seed_of(name):
    return 0x42C + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def pipe_oracle(name, clip=None, geometry=None, qp=None, kw=None):
    """(clip, stream, reconstructions, pictures) of the oracle encoder on a pipeline case; pictures = [dict(kind, packet (index into
    split_packets(stream)), planes [record + 'model' (hz_plan.Plane, one job)] x 3)]"""
    if name not in _pipe:
        if clip is None:
            _, g, content, qp, n, _ = pipe_case(name)
            clip = make_content(g[0], g[1], g[2], content, seed_of(name), n)
        else:
            g = geometry
        (stream, recs), planes = recorded(lambda: A.orc_encode(clip, A.orc_cfg(g[0], g[1], g[2], **dict(kw or CODING, qp=qp)), want_recon=True, eos=False))
        pics = [i for i, p in enumerate(A.split_packets(stream)) if p[5] & 4]
        assert len(planes) == 3 * len(pics) == 3 * clip.shape[0]
        pictures = []
        for t, pk in enumerate(pics):
            pl = planes[3 * t:3 * t + 3]
            assert [p["cur_plane"] for p in pl] == [0, 1, 2]
            pictures.append(dict(kind="P" if pl[0]["isP"] else "I", packet=pk, planes=pl))
        _pipe[name] = (clip, stream, recs, pictures)
    return _pipe[name]


def model_of(rec, seam="pipe", njobs=1):
    return H.Plane(rec["w"], rec["h"], rec["entries"], "P" if rec["isP"] else "I", seam, njobs)


# two streams, one with a scene cut: the second frame step holds a P job (stream 0) and an I job (stream 1), so launch_hz_pack
# has ndense > 0 and nsparse > 0 in one call
CUT_G, CUT_QP = (360, 200, F420), 98
CUT_CODING = dict(CODING, scd=1)
CUT_NAMES = ["cut-0", "cut-1"]


def cut_oracle():
    """[pipe_oracle's tuple per stream]: stream 0 static2, stream 1 a dark soft-noise picture followed by static2 of another scene"""
    w, h, fmt = CUT_G
    a = make_content(w, h, fmt, "static2", 0xC07, 3)
    b = make_content(w, h, fmt, "static2", 0xC08, 3)
    b[0] = _planes(w, h, fmt, 40 + np.random.default_rng(5).integers(-12, 13, size=(h, w)))
    return [pipe_oracle(n, c, CUT_G, CUT_QP, CUT_CODING) for n, c in zip(CUT_NAMES, (a, b))]


# ---------------------------------------------------------------------------------------------------------------------------
# the scan's second tile: 2048x2080 luma = 66560 x 64 = 4 259 840 scan cells = 2080 chunks; chunks 2048..2079 are the last 64 rows
# of the finest diagonal subband, i.e. the bottom 128 picture rows
TILE_G = (2048, 2080, F420)
TILE_STREAMS = 33
TILE_QP = 90
TILE_AMP = 90


def tile_clips():
    """{'A': fine diagonal detail in isolated spots over the whole frame, bottom rows included; its P picture changes only in the
    bottom rows.  'B': the same detail in the top half only; its P picture changes one spot near the top}"""
    w, h, fmt = TILE_G
    out = {}
    for name in ("A", "B"):
        y0 = np.full((h, w), 128, dtype=np.uint8)
        rows = range(16, h - 8, 96) if name == "A" else range(16, h // 2, 96)
        for r in list(rows) + ([h - 40] if name == "A" else []):
            for x in range(32, w - 8, 160):
                y0[r:r + 8, x:x + 8] = np.where((np.add.outer(np.arange(8), np.arange(8)) & 1) == 1, 250, 6)   # one-pixel checkerboard: the finest HH
        y1 = y0.copy()
        ry = h - 24 if name == "A" else 40
        # a one-pixel checkerboard of the background's mean on a flat spot: the finest diagonal subband alone, and too weak for a
        # motion vector to one of the strong spots to predict it
        y1[ry:ry + 8, 96:112] = np.where((np.add.outer(np.arange(8), np.arange(16)) & 1) == 1, 128 + TILE_AMP, 128 - TILE_AMP)
        out[name] = np.stack([_planes(w, h, fmt, y0), _planes(w, h, fmt, y1)])
    return out


def tile_oracle():
    """{'A' | 'B': pipe_oracle's tuple}"""
    clips = tile_clips()
    return {k: pipe_oracle("tile-" + k, clips[k], TILE_G, TILE_QP) for k in clips}
