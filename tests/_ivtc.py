"""Inverse telecine and field order detection, defined in numpy (include/dsv1_api.h, Inverse telecine; csrc/k_ivtc.hip computes the same
integers and bytes).

All decisions read luma only.  Line y belongs to field y & 1; p = 0 if tff else 1 is the parity of the field first in time.  Per frame
four comb sums (mc0 mc1 mp0 mp1); a causal match P / C; the woven picture; per cycle of 5 the picture with the smallest luma SAD
against the woven picture before it is dropped.  The state a stream carries: its last input frame, then its last woven luma."""
import numpy as np

import _cabi as A
from _deint import planes_of

C, P = 0, 1
U32MAX = 0xFFFFFFFF


def comb(K, q, O, nt):
    """kept lines of parity q from luma K, the others from luma O ([H, W] uint8): the sum of e > nt over the interior lines"""
    H = K.shape[0]
    ys = np.array([y for y in range(1, H - 1) if (y & 1) == 1 - q], dtype=np.int64)
    if ys.size == 0:
        return 0
    a, b, o = K[ys - 1].astype(np.int64), K[ys + 1].astype(np.int64), O[ys].astype(np.int64)
    e = np.maximum(np.maximum(np.minimum(a, b) - o, o - np.maximum(a, b)), 0)
    return int(e[e > nt].sum())


def luma(frame, w, h):
    return frame[:w * h].reshape(h, w)


def field_metrics(clip, w, h, prev=None, nt=0):
    """clip [n, frame_bytes] -> uint32 [n, 4]: mc0 mc1 mp0 mp1; prev: the frame before clip[0] or None"""
    m = np.zeros((clip.shape[0], 4), dtype=np.uint32)
    for t in range(clip.shape[0]):
        cur = luma(clip[t], w, h)
        prv = luma(clip[t - 1], w, h) if t else (luma(prev, w, h) if prev is not None else None)
        for q in (0, 1):
            m[t, q] = comb(cur, q, cur, nt)
            m[t, 2 + q] = comb(cur, q, prv, nt) if prv is not None else 0
    return m


def match_of(metrics, first_has_prev, tff):
    p = 0 if tff else 1
    return np.array([P if (t > 0 or first_has_prev) and int(m[2 + p]) < int(m[p]) else C for t, m in enumerate(np.asarray(metrics).reshape(-1, 4))],
                    dtype=np.uint8)


def pick_of(D):
    """D [n] -> drop [n / 5]: the smallest of each cycle, on ties the earliest"""
    D = np.asarray(D, dtype=np.uint64).reshape(-1, 5)
    return np.argmin(D, axis=1).astype(np.uint8)           # (numpy's argmin returns the first of equal minima)


def field_order_of(metrics, first_has_prev=False):
    m = np.asarray(metrics).reshape(-1, 4)[0 if first_has_prev else 1:]
    tv, bv = int((m[:, 2] < m[:, 3]).sum()), int((m[:, 3] < m[:, 2]).sum())
    return 1 if tv > 2 * bv else 0 if bv > 2 * tv else -1


def votes_of(metrics, first_has_prev=False):
    m = np.asarray(metrics).reshape(-1, 4)[0 if first_has_prev else 1:]
    return int((m[:, 2] < m[:, 3]).sum()), int((m[:, 3] < m[:, 2]).sum())


def weave(cur, prv, w, h, fmt, p, match):
    """the woven picture: every plane's lines of parity p from cur, the others from prv under P; a plane of one line is cur's"""
    if match == C:
        return cur.copy()
    out = []
    for c, q in zip(planes_of(cur, w, h, fmt), planes_of(prv, w, h, fmt)):
        o = c.copy()
        if c.shape[0] > 1:
            rows = np.arange(c.shape[0])
            o[(rows & 1) != p] = q[(rows & 1) != p]
        out.append(o.reshape(-1))
    return np.concatenate(out)


def state_bytes(w, h, fmt):
    return A.frame_bytes(w, h, fmt) + w * h


def ivtc_clip(clip, w, h, fmt, tff, nt=0, state=None):
    """clip [n, frame_bytes] (n a multiple of 5), state: what the call before returned or None -> (pictures [4n / 5, frame_bytes],
    match [n], drop [n / 5], state [frame_bytes + w * h], D [n])"""
    n = clip.shape[0]
    assert n % 5 == 0 and n >= 5
    fb = A.frame_bytes(w, h, fmt)
    p = 0 if tff else 1
    prev = state[:fb] if state is not None else None
    last = state[fb:].reshape(h, w) if state is not None else None
    met = field_metrics(clip, w, h, prev, nt)
    match = match_of(met, state is not None, tff)
    V, D = [], np.zeros(n, dtype=np.uint64)
    for t in range(n):
        V.append(weave(clip[t], clip[t - 1] if t else prev, w, h, fmt, p, match[t]))
        before = luma(V[t - 1], w, h) if t else last
        D[t] = U32MAX if before is None else int(np.abs(luma(V[t], w, h).astype(np.int64) - before.astype(np.int64)).sum())
    drop = pick_of(D)
    keep = [t for t in range(n) if t % 5 != drop[t // 5]]
    new = np.concatenate([clip[n - 1], V[n - 1][:w * h]])
    return np.stack([V[t] for t in keep]), match, drop, new, D.astype(np.uint32)


# ---- test material ----
def smooth_noise(hh, ww, seed, passes=3):
    """pre-smoothed noise: correlated over a few samples, so that a pan of 1 .. 2 samples per field stays smooth against the motion"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (hh, ww)).astype(np.float64)
    for _ in range(passes):
        a = (np.roll(a, 1, 0) + 2 * a + np.roll(a, -1, 0)) / 4
        a = (np.roll(a, 1, 1) + 2 * a + np.roll(a, -1, 1)) / 4
    a = (a - a.mean()) / max(a.std(), 1e-9)
    return np.clip(np.rint(128 + 50 * a), 0, 255).astype(np.uint8)


def film_frames(w, h, fmt, n, seed, speed=3):
    """n progressive film frames [n, frame_bytes]: a horizontal pan (speed samples per frame) over pre-smoothed noise, every plane"""
    cw, ch = A.chroma_dims(w, h, fmt)
    out = np.empty((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    for k, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
        sp = speed if k == 0 or pw == w else max(speed // 2, 1)
        tex = smooth_noise(ph, pw + sp * n + 1, seed + k)
        o = 0 if k == 0 else w * h + (k - 1) * cw * ch
        for t in range(n):
            out[t, o:o + pw * ph] = tex[:, sp * t:sp * t + pw].reshape(-1)
    return out


def fields_to_frame(top_src, bot_src, w, h, fmt):
    """a frame whose top-field lines (even) come from top_src and whose bottom-field lines from bot_src, every plane"""
    out = []
    for a, b in zip(planes_of(top_src, w, h, fmt), planes_of(bot_src, w, h, fmt)):
        o = a.copy()
        o[1::2] = b[1::2]
        out.append(o.reshape(-1))
    return np.concatenate(out)


def telecine(film, w, h, fmt, tff, phase=0):
    """3:2 pulldown of film frames [4k, frame_bytes] -> [5k, frame_bytes].  In field time a cycle's four film frames last 2, 3, 2, 3
    fields; `phase` (0 .. 3) rotates which film frame of the cycle takes the first slot.  The first field in time has parity p."""
    n = film.shape[0]
    assert n % 4 == 0
    seq = []                                               # the film frame shown in every field time
    for i in range(n):
        seq += [i] * (2 if (i + phase) % 2 == 0 else 3)
    frames = []
    for t in range(len(seq) // 2):
        first, second = film[seq[2 * t]], film[seq[2 * t + 1]]
        top, bot = (first, second) if tff else (second, first)
        frames.append(fields_to_frame(top, bot, w, h, fmt))
    return np.stack(frames), seq


def kept_film(seq, match, drop, first_has_prev=False):
    """which film frame every kept picture shows, or None for a picture that mixes two: from the field sequence and the decisions"""
    out = []
    for t in range(len(match)):
        if t % 5 == drop[t // 5]:
            continue
        a = seq[2 * t]                                     # the first field in time is always cur's
        b = seq[2 * t - 1] if match[t] == P else seq[2 * t + 1]
        out.append(a if a == b else None)
    return out


def interlaced_pan(w, h, fmt, n, seed, tff, speed):
    """true interlaced video [n, frame_bytes]: every field is its own instant of a pan of `speed` samples per field"""
    film = film_frames(w, h, fmt, 2 * n, seed, speed)
    return np.stack([fields_to_frame(*((film[2 * t], film[2 * t + 1]) if tff else (film[2 * t + 1], film[2 * t])), w, h, fmt) for t in range(n)])


def static_columns(w, h, fmt, n, seed):
    """a static clip [n, frame_bytes] whose rows are all alike (columns of pre-smoothed noise): no sample lies outside its vertical
    neighbours, every metric is 0 and no frame votes.  (A static picture WITH vertical detail has mp == mc, and its frames vote by
    which of its own fields combs more: that says nothing about time, and the vote is not meant for such material.)"""
    cw, ch = A.chroma_dims(w, h, fmt)
    parts = [np.repeat(smooth_noise(4, pw, seed + k)[:1], ph, axis=0).reshape(-1) for k, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch)))]
    return np.repeat(np.concatenate(parts)[None], n, axis=0)


def add_noise(clip, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(clip.astype(np.float64) + rng.normal(0, sigma, clip.shape)), 0, 255).astype(np.uint8)
