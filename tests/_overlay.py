"""The overlay pass (include/dsv1_api.h, Overlays) stated in numpy and plain Python integers: the definition the library is held to.
A placement is a dict (ov()); its bitmap the four planes Y, U, V, A one after the other (bitmap() / planes_of()).  valid(), opacity_at()
and plan() are the host-only rules; chroma_alpha(), blend() and composite() the arithmetic; from_rgba() the RGBA helper from the RGB
section's pieces (tests/_rgb.py).  Written from the definition, with none of the library's tricks: the blend divides by 65280."""
from fractions import Fraction
from math import floor

import numpy as np

import _cabi as A
import _pixout as PO
import _rgb as RG

FORMATS = (A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411)
MAX_OVERLAYS = 4096


def r(a, b):
    """the exact rational a / b rounded half up"""
    return floor(Fraction(a, b) + Fraction(1, 2))


def ov(planes, w, h, x=0, y=0, source=-1, t0=0, dur=0, fade_in=0, fade_out=0, opacity=256, reserved=0):
    return dict(planes=planes, w=w, h=h, x=x, y=y, source=source, t0=t0, dur=dur, fade_in=fade_in, fade_out=fade_out, opacity=opacity,
                reserved=reserved)


def bitmap_bytes(w, h, fmt):
    return A.frame_bytes(w, h, fmt) + w * h


def planes_of(o, fmt):
    """Y, U, V, A as 2-D views of the placement's bitmap"""
    w, h = o["w"], o["h"]
    cw, ch = A.chroma_dims(w, h, fmt)
    p = np.asarray(o["planes"], dtype=np.uint8).reshape(-1)
    assert p.size == bitmap_bytes(w, h, fmt)
    e = np.cumsum([0, w * h, cw * ch, cw * ch, w * h])
    return (p[e[0]:e[1]].reshape(h, w), p[e[1]:e[2]].reshape(ch, cw), p[e[2]:e[3]].reshape(ch, cw), p[e[3]:e[4]].reshape(h, w))


def bitmap(w, h, fmt, seed, alpha="random"):
    """a random bitmap; alpha: "random", 0 or 255"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, bitmap_bytes(w, h, fmt), dtype=np.uint8)
    if alpha != "random":
        p[p.size - w * h:] = alpha
    return p


def valid(o, W, H, fmt, S):
    if fmt not in FORMATS:
        return False
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    return (o["planes"] is not None and o["reserved"] == 0 and o["w"] >= 1 and o["h"] >= 1 and 0 <= o["x"] and o["x"] + o["w"] <= W
            and 0 <= o["y"] and o["y"] + o["h"] <= H and o["x"] % (1 << hs) == 0 and o["y"] % (1 << vs) == 0 and 0 <= o["opacity"] <= 256
            and -1 <= o["source"] <= S - 1 and 0 <= o["fade_in"] <= 65535 and 0 <= o["fade_out"] <= 65535)


def opacity_at(o, t):
    t0, dur, fi, fo = o["t0"], o["dur"], o["fade_in"], o["fade_out"]
    if t < t0 or (dur > 0 and t >= t0 + dur):
        return 0
    a = min(t - t0 + 1, fi + 1)
    b = fo + 1 if dur == 0 else min(t0 + dur - t, fo + 1)
    return r(o["opacity"] * a * b, (fi + 1) * (fo + 1))


def intersects(a, b):
    return a["x"] < b["x"] + b["w"] and b["x"] < a["x"] + a["w"] and a["y"] < b["y"] + b["h"] and b["y"] < a["y"] + a["h"]


def plan(ovs, S, F, counters):
    """([(overlay, source, frame, op, layer)] in the order source, frame, overlay; the number of layers)"""
    items = []
    for s in range(S):
        for f in range(F):
            here = []
            for i, o in enumerate(ovs):
                if o["source"] not in (-1, s):
                    continue
                op = opacity_at(o, counters[s] + f)
                if op == 0:
                    continue
                layer = 1 + max([l for j, l in here if intersects(ovs[j], o)], default=0)
                here.append((i, layer))
                items.append((i, s, f, op, layer))
    return items, max([it[4] for it in items], default=0)


def chroma_alpha(Aa, fmt):
    """A_c[Y][X] = r(sum / count) over the alpha samples the chroma sample covers"""
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    h, w = Aa.shape
    cw, ch = A.chroma_dims(w, h, fmt)
    out = np.zeros((ch, cw), dtype=np.uint8)
    for Y in range(ch):
        for X in range(cw):
            blk = Aa[Y << vs:min(h, (Y + 1) << vs), X << hs:min(w, (X + 1) << hs)].astype(np.int64)
            out[Y, X] = r(int(blk.sum()), blk.size)
    return out


def blend(inp, ovl, alpha, op):
    """out = floor((in (65280 - k) + ov k + 32640) / 65280), k = alpha op; arrays or integers"""
    inp, ovl, k = np.asarray(inp).astype(np.int64), np.asarray(ovl).astype(np.int64), np.asarray(alpha).astype(np.int64) * int(op)
    num = inp * (65280 - k) + ovl * k + 32640
    assert num.max(initial=0) < 1 << 24
    return num // 65280


def blend_shift(inp, ovl, alpha, op):
    """the same as a shift by 8 and then a division by 255"""
    inp, ovl, k = np.asarray(inp).astype(np.int64), np.asarray(ovl).astype(np.int64), np.asarray(alpha).astype(np.int64) * int(op)
    return ((inp * (65280 - k) + ovl * k + 32640) >> 8) // 255


def blend_frame(frame, o, op, W, H, fmt):
    """one placement onto one packed planar frame (uint8, flat), in place"""
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    cw, ch = A.chroma_dims(W, H, fmt)
    Yp, Up, Vp, Ap = planes_of(o, fmt)
    Ac = chroma_alpha(Ap, fmt)
    dst = (frame[:W * H].reshape(H, W), frame[W * H:W * H + cw * ch].reshape(ch, cw), frame[W * H + cw * ch:].reshape(ch, cw))
    for k, (d, src, al) in enumerate(zip(dst, (Yp, Up, Vp), (Ap, Ac, Ac))):
        x, y = (o["x"] >> hs, o["y"] >> vs) if k else (o["x"], o["y"])
        ph, pw = src.shape
        d[y:y + ph, x:x + pw] = blend(d[y:y + ph, x:x + pw], src, al, op).astype(np.uint8)


def composite(clip, W, H, fmt, ovs, t_first=0, source=0):
    """frames [n][frame bytes] of one source, frame i picture t_first + i: the overlays in list order, later on top"""
    out = np.array(clip, dtype=np.uint8).reshape(-1, A.frame_bytes(W, H, fmt))
    for i in range(out.shape[0]):
        for o in ovs:
            if o["source"] in (-1, source):
                op = opacity_at(o, t_first + i)
                if op:
                    blend_frame(out[i], o, op, W, H, fmt)
    return out


def composite_call(clip, W, H, fmt, ovs, S, F, counters):
    """a session's call, [source][F frames]: source s's first frame is picture counters[s]"""
    c = np.asarray(clip, dtype=np.uint8).reshape(S, F, -1)
    return np.stack([composite(c[s], W, H, fmt, ovs, counters[s], s) for s in range(S)]).reshape(S * F, -1)


def from_rgba(img, w, h, order, matrix, full, fmt):
    """img: the image's bytes in memory order `order`, tight.  Y, U, V are tests/_rgb.py's import_ of the colour bytes (its to_ycc and
    the output pass's halving; at 4:1:1, which import_ does not take, the horizontal halving twice), A the alpha bytes or 255"""
    f = RG.rf(order=order, matrix=matrix, full=full)
    img = np.asarray(img, dtype=np.uint8).reshape(-1)
    if fmt in RG.SUBSAMPS:
        yuv = RG.import_(img, f, w, h, fmt, 1)[0]
    else:
        R, G, B = RG.unpack(img, f, w, h, 1)
        Y, Cb, Cr = RG.to_ycc(R[0], G[0], B[0], matrix, full)
        u, v = (PO.halve_h(PO.halve_h(c.astype(np.uint8))) for c in (Cb, Cr))
        assert u.shape == A.chroma_dims(w, h, fmt)[::-1]
        yuv = np.concatenate([Y.astype(np.uint8).reshape(-1), u.reshape(-1), v.reshape(-1)])
    a = img.reshape(h, w, 4)[:, :, RG.ALPHA[order]].reshape(-1) if order in RG.ALPHA else np.full(w * h, 255, dtype=np.uint8)
    return np.concatenate([yuv, a])
