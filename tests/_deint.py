"""The deinterlacer's definition in numpy (include/dsv1_api.h, Deinterlacing; csrc/k_deint.hip computes the same bytes).

Every plane of a tightly packed planar 8-bit frame is treated on its own, at its own dimensions.  Line y belongs to field y & 1
(0 = top); tff says which field of a frame is earlier in time, the first field's parity is p = 0 if tff else 1.  An output picture
keeps the lines of one parity q and makes the others from the lines above and below (edge-directed, five directions) bounded by what
the frame before allows (motion-adaptive).  FRAME mode: output t keeps q = p.  FIELD mode: output 2t keeps q = p (first-field
output), output 2t + 1 keeps q = 1 - p (second-field output)."""
import numpy as np

import _cabi as A

FRAME, FIELD = 0, 1
DIRS = (0, -1, -2, 1, 2)                                 # the order the statistics count the winning direction in


def planes_of(frame, w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    o = 0
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        yield frame[o:o + pw * ph].reshape(ph, pw)
        o += pw * ph


def deint_plane(cur, prv, q, second, stats=None):
    """one plane [H, W] uint8 of frame t; prv: the same plane of frame t - 1 or None; q: the parity kept; second: the second-field
    output of FIELD mode.  stats (dict) collects: made samples, winners per direction, clamp outcomes (prv present only)."""
    H, W = cur.shape
    out = cur.copy()
    if H == 1:
        return out
    rows = np.arange(H)
    ys = rows[(rows & 1) != q]
    up = np.where(ys - 1 >= 0, ys - 1, ys + 1)
    dn = np.where(ys + 1 <= H - 1, ys + 1, ys - 1)
    C = np.pad(cur[up].astype(np.int32), ((0, 0), (3, 3)), mode="edge")     # c[i] = C[:, i + 3], columns clamped
    E = np.pad(cur[dn].astype(np.int32), ((0, 0), (3, 3)), mode="edge")

    def c(o):
        return C[:, 3 + o:3 + o + W]

    def e(o):
        return E[:, 3 + o:3 + o + W]

    def S(j):
        return sum(np.abs(c(k + j) - e(k - j)) for k in (-1, 0, 1))

    def P(j):
        return (c(j) + e(-j)) >> 1

    best, sp, win = S(0) - 1, P(0), np.zeros(C[:, 3:3 + W].shape, dtype=np.int32)
    for first, then in ((-1, -2), (1, 2)):
        t1 = S(first) < best
        best, sp, win = np.where(t1, S(first), best), np.where(t1, P(first), sp), np.where(t1, first, win)
        t2 = t1 & (S(then) < best)
        best, sp, win = np.where(t2, S(then), best), np.where(t2, P(then), sp), np.where(t2, then, win)
    if stats is not None:
        stats["made"] = stats.get("made", 0) + int(sp.size)
        for j in DIRS:
            stats[("dir", j)] = stats.get(("dir", j), 0) + int((win == j).sum())
    if prv is None:
        res = sp
    else:
        a, b = prv[ys].astype(np.int32), cur[ys].astype(np.int32)
        if second:
            tp, td0 = b, np.abs(b - a) >> 1
        else:
            tp, td0 = (a + b) >> 1, np.abs(a - b) >> 1
        td1 = (np.abs(prv[up].astype(np.int32) - c(0)) + np.abs(prv[dn].astype(np.int32) - e(0))) >> 1
        d = np.maximum(td0, td1)
        res = np.minimum(np.maximum(sp, tp - d), tp + d)
        if stats is not None:
            stats["clamped"] = stats.get("clamped", 0) + int(sp.size)
            stats["below"] = stats.get("below", 0) + int((sp < tp - d).sum())
            stats["above"] = stats.get("above", 0) + int((sp > tp + d).sum())
            stats["inside"] = stats.get("inside", 0) + int(((sp >= tp - d) & (sp <= tp + d)).sum())
    out[ys] = res.astype(np.uint8)
    return out


def deint_frame(cur, prv, w, h, fmt, q, second, stats=None):
    pp = [None] * 3 if prv is None else list(planes_of(prv, w, h, fmt))
    return np.concatenate([deint_plane(c, p, q, second, stats).reshape(-1) for c, p in zip(planes_of(cur, w, h, fmt), pp)])


def out_frames(mode, n):
    return 2 * n if mode == FIELD else n


def deint_clip(clip, w, h, fmt, mode, tff, prev=None, stats=None):
    """clip [n, frame_bytes] uint8 (one stream) -> [n or 2n, frame_bytes]; prev: the frame before clip[0] or None"""
    p = 0 if tff else 1
    out = []
    for t in range(clip.shape[0]):
        prv = clip[t - 1] if t else prev
        out.append(deint_frame(clip[t], prv, w, h, fmt, p, False, stats))
        if mode == FIELD:
            out.append(deint_frame(clip[t], prv, w, h, fmt, 1 - p, True, stats))
    return np.stack(out)


def gen_interlaced(w, h, fmt, n, seed, tff=1):
    """an interlaced test clip [n, frame_bytes]: every frame weaves two fields taken at consecutive instants (first field parity from
    tff) of a scene of tilted bars of several slopes that move, a static textured region (the left quarter) and low noise"""
    rng = np.random.default_rng(seed)
    p = 0 if tff else 1
    cw, ch = A.chroma_dims(w, h, fmt)
    frames = np.empty((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    slopes = (0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5)

    def scene(pw, ph, tau, k):
        """the scene of plane k at instant tau (field units), progressive, [ph, pw]"""
        y, x = np.mgrid[0:ph, 0:pw].astype(np.float64)
        band = np.minimum((y * len(slopes) // max(ph, 1)).astype(np.int64), len(slopes) - 1)
        sl = np.asarray(slopes)[band]
        period = 9.0 + 2.0 * band + 3 * k
        speed = 1.5 + 0.75 * band
        moving = x >= pw // 4
        ph_ = x + sl * y + np.where(moving, speed * tau, 0.0)
        v = 128 + 100 * np.sin(2 * np.pi * ph_ / period)
        return v

    texture = [np.random.default_rng(seed + 1 + k).integers(-24, 25, (ph, pw)) for k, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch)))]
    for t in range(n):
        parts = []
        for k, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
            first, second = scene(pw, ph, 2 * t, k), scene(pw, ph, 2 * t + 1, k)
            rows = np.arange(ph)
            pl = np.where(((rows & 1) == p)[:, None], first, second)
            noise = rng.integers(-2, 3, pl.shape)
            noise[:, :pw // 4] = texture[k][:, :pw // 4]  # (the static region is static to the bit, and no interpolation guesses it)
            parts.append(np.clip(np.rint(pl) + noise, 0, 255).astype(np.uint8).reshape(-1))
        frames[t] = np.concatenate(parts)
    return frames


# the standalone cases of tests/test_gpu_deint.py (tests/test_deint_host.py checks what their clips reach): all rows aligned; none;
# tails; odd (both row rules, both column clamps); chroma of one row; three rows; one sample
GPU_GEOMS = [(352, 288, A.SUBSAMP_420), (250, 130, A.SUBSAMP_422), (36, 20, A.SUBSAMP_411), (48, 18, A.SUBSAMP_420), (35, 19, A.SUBSAMP_444),
             (16, 2, A.SUBSAMP_420), (64, 3, A.SUBSAMP_422), (1, 1, A.SUBSAMP_444)]
GPU_FRAMES, GPU_SEED = 3, 0xD1


def gpu_case(w, h, fmt, tff):
    """the standalone GPU test's input for a geometry: (the GPU_FRAMES frames it deinterlaces, the frame before them)"""
    clip = gen_interlaced(w, h, fmt, GPU_FRAMES + 1, GPU_SEED, tff)
    return clip[1:], clip[0]


def planes_fast(w, h, fmt):
    """per plane: is every row 16-byte aligned in buffers that start aligned (and is there more than one row) -- the kernel's rule for
    its 16-byte path (csrc/k_deint.hip: di_launch)"""
    cw, ch = A.chroma_dims(w, h, fmt)
    fb = A.frame_bytes(w, h, fmt)
    return [ph > 1 and (fb | off | pw) % 16 == 0 for pw, ph, off in ((w, h, 0), (cw, ch, w * h), (cw, ch, w * h + cw * ch))]
