"""The reframe pass, the line sums and the bars rule (include/dsv1_api.h, Reframe) stated in numpy, and the case lists the reframe
tests share.  A reframe is a dict with the fields of dsv1_reframe: in_w, in_h, x, y, w, h, out_w, out_h, dst_x, dst_y, fill (Y, U, V),
reserved."""
import numpy as np

import _cabi as A

FORMATS = (A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411)
FILL = (16, 128, 128)


def rf(in_w, in_h, window, out, dst=(0, 0), fill=FILL, reserved=0):
    x, y, w, h = window
    return dict(in_w=in_w, in_h=in_h, x=x, y=y, w=w, h=h, out_w=out[0], out_h=out[1], dst_x=dst[0], dst_y=dst[1], fill=tuple(fill), reserved=reserved)


def valid(r, fmt):
    """the predicate of include/dsv1_api.h, rule by rule"""
    if fmt not in FORMATS or r["reserved"] != 0:
        return False
    if min(r["in_w"], r["in_h"], r["w"], r["h"], r["out_w"], r["out_h"]) < 1:
        return False
    if r["x"] < 0 or r["x"] + r["w"] > r["in_w"] or r["y"] < 0 or r["y"] + r["h"] > r["in_h"]:
        return False
    if r["dst_x"] < 0 or r["dst_x"] + r["w"] > r["out_w"] or r["dst_y"] < 0 or r["dst_y"] + r["h"] > r["out_h"]:
        return False
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    return r["x"] % (1 << hs) == 0 and r["dst_x"] % (1 << hs) == 0 and r["y"] % (1 << vs) == 0 and r["dst_y"] % (1 << vs) == 0


def planes(frame, w, h, fmt):
    """the three planes of one packed planar frame as 2-D views"""
    cw, ch = A.chroma_dims(w, h, fmt)
    f = np.asarray(frame).reshape(-1)
    return [f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)]


def reframe_clip(clip, r, fmt):
    """[n][frame bytes of in_w x in_h] -> [n][frame bytes of out_w x out_h], every plane on its own"""
    assert valid(r, fmt)
    ifb, ofb = A.frame_bytes(r["in_w"], r["in_h"], fmt), A.frame_bytes(r["out_w"], r["out_h"], fmt)
    clip = np.asarray(clip, dtype=np.uint8).reshape(-1, ifb)
    out = np.zeros((clip.shape[0], ofb), dtype=np.uint8)
    for t in range(clip.shape[0]):
        for p, (i, o) in enumerate(zip(planes(clip[t], r["in_w"], r["in_h"], fmt), planes(out[t], r["out_w"], r["out_h"], fmt))):
            hs, vs = (A.hshift(fmt), A.vshift(fmt)) if p else (0, 0)
            X0, W, DX = r["x"] >> hs, A.rshift_up(r["w"], hs), r["dst_x"] >> hs
            Y0, H, DY = r["y"] >> vs, A.rshift_up(r["h"], vs), r["dst_y"] >> vs
            o[...] = r["fill"][p]
            o[DY:DY + H, DX:DX + W] = i[Y0:Y0 + H, X0:X0 + W]
    return out


def line_sums(clip, w, h, fmt):
    """(row_sum [n][h], col_sum [n][w]) of the luma, uint32"""
    clip = np.asarray(clip, dtype=np.uint8).reshape(-1, A.frame_bytes(w, h, fmt))
    y = clip[:, :w * h].reshape(-1, h, w).astype(np.uint64)
    return y.sum(axis=2).astype(np.uint32), y.sum(axis=1).astype(np.uint32)


def bars_ok(thresh, align):
    return 0 <= thresh <= 254 and align in (1, 2, 4, 8, 16, 32, 64)


def bars_from_sums(row_sum, col_sum, thresh, align):
    """(x, y, w, h) or None: a line is content if its sum exceeds thresh x its length in any frame; rounded inward to align"""
    assert bars_ok(thresh, align)
    row_sum, col_sum = np.asarray(row_sum, dtype=np.uint64), np.asarray(col_sum, dtype=np.uint64)
    h, w = row_sum.shape[-1], col_sum.shape[-1]
    rows = np.flatnonzero((row_sum.reshape(-1, h) > thresh * w).any(axis=0))
    cols = np.flatnonzero((col_sum.reshape(-1, w) > thresh * h).any(axis=0))
    if not rows.size or not cols.size:
        return None
    x0, x1, y0, y1 = int(cols[0]), int(cols[-1]), int(rows[0]), int(rows[-1])
    x = -(-x0 // align) * align
    y = -(-y0 // align) * align
    rw, rh = (x1 + 1) // align * align - x, (y1 + 1) // align * align - y
    return (x, y, rw, rh) if rw > 0 and rh > 0 else None


def noise(n, w, h, fmt, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)


def boxed(n, w, h, fmt, rect, seed, level=16):
    """n noisy frames whose luma outside rect (x, y, w, h) is `level`, chroma 128 there"""
    clip = noise(n, w, h, fmt, seed)
    clip[:, :w * h] = np.maximum(clip[:, :w * h], 64)    # (content well above any threshold the tests use)
    full = rf(w, h, rect, (w, h), (rect[0], rect[1]), (level, 128, 128))
    return reframe_clip(clip, full, fmt)


# ---- the validity table: (name, reframe, expected at every subsampling or {fmt: expected}) ----
def validity_table():
    ok = rf(64, 48, (8, 4, 32, 24), (96, 64), (16, 8))
    t = [("valid", ok, True)]
    for k in ("in_w", "in_h", "w", "h", "out_w", "out_h"):
        for v in (0, -1):
            t.append(("%s = %d" % (k, v), dict(ok, **{k: v}), False))
    t += [("x < 0", dict(ok, x=-4), False), ("x + w > in_w", dict(ok, x=36), False), ("y < 0", dict(ok, y=-4), False),
          ("y + h > in_h", dict(ok, y=28), False), ("dst_x < 0", dict(ok, dst_x=-4), False), ("dst_x + w > out_w", dict(ok, dst_x=68), False),
          ("dst_y < 0", dict(ok, dst_y=-4), False), ("dst_y + h > out_h", dict(ok, dst_y=44), False), ("reserved", dict(ok, reserved=1), False),
          ("huge x", dict(ok, x=2 ** 31 - 4), False), ("huge w", dict(ok, w=2 ** 31 - 1), False)]
    # alignment: per subsampling
    al = lambda hs, vs: {f: (A.hshift(f) <= hs and A.vshift(f) <= vs) for f in FORMATS}
    t += [("x odd", dict(ok, x=9), al(0, 2)), ("dst_x odd", dict(ok, dst_x=17), al(0, 2)), ("y odd", dict(ok, y=5), al(2, 0)),
          ("dst_y odd", dict(ok, dst_y=9), al(2, 0)), ("x = 2 mod 4", dict(ok, x=10), al(1, 2)), ("dst_x = 2 mod 4", dict(ok, dst_x=18), al(1, 2))]
    # valid corners
    t += [("odd w and h", dict(ok, w=31, h=23), True), ("window touches left / top", dict(ok, x=0, y=0), True),
          ("window touches right / bottom", dict(ok, x=32, y=24), True), ("canvas edge right / bottom", dict(ok, dst_x=64, dst_y=40), True),
          ("canvas edge left / top", dict(ok, dst_x=0, dst_y=0), True), ("1x1 window", dict(ok, w=1, h=1), True),
          ("1x1 everything", rf(1, 1, (0, 0, 1, 1), (1, 1)), True), ("identity", rf(64, 48, (0, 0, 64, 48), (64, 48)), True),
          ("odd window at the odd input's end", rf(71, 51, (8, 4, 63, 47), (96, 64), (16, 8)), True)]
    return t


# ---- GPU cases: (name, reframe, frames); each runs at every subsampling at which it is valid (formats_of) ----
def gpu_cases():
    c = [("odd everything", rf(70, 50, (6, 4, 51, 33), (96, 64), (10, 8)), 3),          # (x = 6: not 4:1:1, whose case is below)
         ("pure pad", rf(64, 48, (0, 0, 64, 48), (96, 64), (16, 8)), 3),
         ("pure crop", rf(96, 64, (16, 8, 64, 48), (64, 48)), 3),
         ("last column and row", rf(70, 50, (36, 20, 34, 30), (49, 41), (8, 4)), 3),
         ("4:1:1 with x = 4", rf(73, 41, (4, 2, 61, 37), (81, 47), (8, 4), (235, 90, 240)), 3),
         ("1080p 2.39:1", rf(1920, 1080, (0, 140, 1920, 800), (1920, 800)), 2)]
    for w in (1, 3, 15, 17):
        c.append(("window %dx1" % w, rf(70, 50, (12, 8, w, 1), (45, 9), (4, 4)), 3))
    return c


def formats_of(r):
    return [f for f in FORMATS if valid(r, f)]


LINE_SUM_GEOMS = ((33, 7), (64, 1), (1, 64), (250, 130), (1920, 1080))
