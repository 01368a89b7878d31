"""The decoders' debug overlay, stated sequentially (include/dsv1_api.h, debug overlays; the reference's -drawinfo, dsv_decoder.c:147-243).

Blocks are visited in raster order and a pixel keeps what its last writer left.  A block at (x, y) = (i * bw, j * bh) draws, in order:
  grid    luma row y is cleared once per block row, before its blocks; then column x over the rows of the block;
  dash    (bit 1, stable blocks) 2 * (bw // 4) + 1 pixels centred on the block's centre row: 255 at odd offsets, 0 at even ones;
  vector  (bit 2, inter blocks) the line walk from the block's centre towards centre + (mvx, mvy): 0 on every point short of the end;
  dots    (bit 4, intra blocks) a 255 per set submask bit, at the quarter points of the block.
Everything is clipped to the plane -- the dots too, which is where this definition deliberately leaves the reference.

`trace` (a dict) collects what happened, so that a test can assert that its tables really make the writers collide.
"""
import numpy as np

STABHQ, MOVECS, IBLOCK = 1, 2, 4

BLOCKINFO = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mode", "u1"), ("submask", "u1"), ("stable", "u1"), ("reserved", "u1")])


def block_size(dim):
    """the block size the encoder picks for a dimension (per axis)"""
    for above, size in ((1280, 64), (1024, 48), (704, 32), (352, 24)):
        if dim > above:
            return size
    return 16


def nblocks(w, h, bw, bh):
    return -(-w // bw), -(-h // bh)


def line_points(x0, y0, mvx, mvy):
    """the points the vector of a block centred at (x0, y0) visits: from the centre up to, not including, the end; a zero vector
    visits the centre"""
    x1, y1 = x0 + mvx, y0 + mvy
    dx, dy = abs(mvx), abs(mvy)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err = dx - dy
    yield x0, y0
    x, y = x0, y0
    first = True
    while (x, y) != (x1, y1):
        if not first:
            yield x, y
        first = False
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += sy


def draw_info(luma, bw, bh, info, mode, trace=None):
    """draw the overlay of `mode` (non-zero) onto luma, a (h, w) uint8 array, in place; info: one BLOCKINFO entry per block, raster order"""
    h, w = luma.shape
    nbh, nbv = nblocks(w, h, bw, bh)
    info = np.asarray(info).reshape(-1)
    assert info.size >= nbh * nbv and mode
    owner = {}                           # (x, y) -> (what, block) of the last writer, for the trace
    tr = trace if trace is not None else {}

    def note(tag):
        tr[tag] = tr.get(tag, 0) + 1

    def put(x, y, v, what, b):
        if not (0 <= x < w and 0 <= y < h):
            return False
        if trace is not None:
            old = owner.get((x, y))
            if old is not None:
                ow, ob = old
                if what == "vec" and ow in ("dash255", "dot"):
                    note("own_vec_over_dash" if ob == b else "later_vec_over_" + ("dash" if ow == "dash255" else "dot"))
                elif what in ("dash255", "dot") and ow == "vec":
                    note(("dash" if what == "dash255" else "dot") + "_over_earlier_vec")
            owner[(x, y)] = (what, b)
        luma[y, x] = v
        return True

    for j in range(nbv):
        y = j * bh
        luma[y, :] = 0
        for i in range(nbh):
            b = j * nbh + i
            e = info[b]
            x = i * bw
            for k in range(y, min(y + bh, h)):
                put(x, k, 0, "grid", b)
            if (mode & STABHQ) and (int(e["stable"]) & 1):
                q = bw // 4
                for k in range(-q, q + 1):
                    odd = k % 2                     # (Python's % is never negative: odd for -1, -3, ... as k & 1 is in C)
                    if put(x + bw // 2 + k, y + bh // 2, 255 * odd, "dash255" if odd else "dash0", b):
                        note("dash_pixels")
            if (mode & MOVECS) and int(e["mode"]) == 0:
                mvx, mvy = int(e["mvx"]), int(e["mvy"])
                inside = 0
                for px, py in line_points(x + bw // 2, y + bh // 2, mvx, mvy):
                    if put(px, py, 0, "vec", b):
                        inside += 1
                        continue
                    note("leaves_" + ("left" if px < 0 else "right" if px >= w else "top" if py < 0 else "bottom"))
                    # outside, and moving away or not at all on that axis: nothing more of this walk lies inside
                    if (px < 0 and mvx <= 0) or (px >= w and mvx >= 0) or (py < 0 and mvy <= 0) or (py >= h and mvy >= 0):
                        break
                if inside:
                    note("vec_pixels")
                if mvx == 0 and mvy == 0:
                    note("zero_vec")
            if (mode & IBLOCK) and int(e["mode"]) == 1:
                for bit in range(4):
                    if (int(e["submask"]) >> bit) & 1:
                        px = x + bw * (3 if bit & 1 else 1) // 4
                        py = y + bh * (3 if bit & 2 else 1) // 4
                        if put(px, py, 255, "dot", b):
                            note("dots")
                        else:
                            note("dots_clipped")
    return luma


def draw_frames(frames, w, h, bw, bh, infos, mode, traces=None):
    """the overlay on packed planar frames [n][frame_bytes] (a copy is returned); infos: [n][nblk] BLOCKINFO; luma only"""
    out = np.array(frames, dtype=np.uint8, copy=True)
    nbh, nbv = nblocks(w, h, bw, bh)
    infos = np.asarray(infos).reshape(out.shape[0], -1)
    for t in range(out.shape[0]):
        luma = out[t, :w * h].reshape(h, w)
        draw_info(luma, bw, bh, infos[t][:nbh * nbv], mode, None if traces is None else traces[t])
    return out
