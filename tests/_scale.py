"""The resampler of resolution ladders stated in numpy (include/dsv1_api.h dsv1_scale_weights / dsv1_scale_clip, csrc/k_scale.hip).
Integer arithmetic from integer weight tables built in binary64 in a fixed order, so the device must equal it to the byte.

Per axis and plane, S source samples -> D destination samples (1 <= S / D <= 8), centre-aligned grids:
  c = ((2i+1) S - D) / (2 D),  inv = D / S,  taps j = floor(c) - r .. floor(c) + r + 1 with r = ceil(support S / D), T = 2r + 2;
  t = (j - c) inv, x = |t|, w = K(x);  sum = sum w (ascending j);  q = rint(w 16384 / sum);  16384 - sum q goes to the first largest q.
Horizontal pass first: H = sum qh P (int32), Hs = (H + 128) >> 8; V = sum qv Hs (int32); out = clamp((V + 2^19) >> 20, 0, 255).
Source indices are clamped to [0, S-1]."""
import numpy as np

import _cabi as A

TENT, CUBIC = 0, 1
SUPPORT = {TENT: 1, CUBIC: 2}
ONE = 16384


def taps(S, D, filt):
    r = (SUPPORT[filt] * S + D - 1) // D
    return 2 * r + 2


def kernel(x, filt):
    x = np.asarray(x, dtype=np.float64)
    if filt == TENT:
        return np.maximum(0.0, 1.0 - x)
    near = ((1.5 * x - 2.5) * x) * x + 1.0
    far = ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def weights(S, D, filt):
    """(start int32 [D], q int16 [D, T]): the taps of output sample i are start[i] .. start[i] + T - 1 (before clamping)"""
    assert 1 <= D <= S <= 8 * D, (S, D)
    T = taps(S, D, filt)
    r = (T - 2) // 2
    i = np.arange(D, dtype=np.int64)
    c = ((2 * i + 1) * S - D).astype(np.float64) / float(2 * D)
    inv = float(D) / float(S)
    start = np.floor(c).astype(np.int64) - r
    j = start[:, None] + np.arange(T, dtype=np.int64)[None, :]
    w = kernel(np.abs((j.astype(np.float64) - c[:, None]) * inv), filt)
    s = np.zeros(D, dtype=np.float64)
    for t in range(T):                      # ascending j, one addition at a time
        s = s + w[:, t]
    q = np.rint(w * float(ONE) / s[:, None]).astype(np.int64)
    first = np.argmax(q, axis=1)            # the first largest
    q[i, first] += ONE - q.sum(axis=1)
    return start.astype(np.int32), q.astype(np.int16)


def scale_plane(P, dw, dh, filt):
    """uint8 [h, w] -> uint8 [dh, dw]"""
    h, w = P.shape
    sx, qh = weights(w, dw, filt)
    sy, qv = weights(h, dh, filt)
    P = P.astype(np.int64)
    H = np.zeros((h, dw), dtype=np.int64)
    for t in range(qh.shape[1]):
        H += qh[:, t].astype(np.int64)[None, :] * P[:, np.clip(sx.astype(np.int64) + t, 0, w - 1)]
    assert np.abs(H).max() < 2 ** 31
    Hs = (H + 128) >> 8
    V = np.zeros((dh, dw), dtype=np.int64)
    for t in range(qv.shape[1]):
        V += qv[:, t].astype(np.int64)[:, None] * Hs[np.clip(sy.astype(np.int64) + t, 0, h - 1), :]
    assert np.abs(V).max() < 2 ** 31
    return np.clip((V + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def scale_frame(frame, sw, sh, fmt, dw, dh, filt):
    """one packed planar frame (Y, U, V) of sw x sh -> dw x dh, each plane from the source's chroma dims to the rung's"""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    out, o = [], 0
    scw, sch = A.chroma_dims(sw, sh, fmt)
    dcw, dch = A.chroma_dims(dw, dh, fmt)
    for (pw, ph), (qw, qh) in zip([(sw, sh), (scw, sch), (scw, sch)], [(dw, dh), (dcw, dch), (dcw, dch)]):
        out.append(scale_plane(frame[o:o + pw * ph].reshape(ph, pw), qw, qh, filt).reshape(-1))
        o += pw * ph
    return np.concatenate(out)


def scale_clip(clip, sw, sh, fmt, dw, dh, filt):
    """[frames, frame_bytes] -> [frames, scaled frame_bytes]"""
    clip = np.asarray(clip, dtype=np.uint8)
    n = clip.shape[0]
    return np.stack([scale_frame(clip[t], sw, sh, fmt, dw, dh, filt) for t in range(n)]) if n else \
        np.zeros((0, A.frame_bytes(dw, dh, fmt)), dtype=np.uint8)
