"""The resampler in both directions stated in numpy (include/dsv1_api.h dsv1_resample_weights / dsv1_resample_clip, csrc/k_scale.hip,
and the upscale inside csrc/k_quality.hip k_xres_quality).  Integer arithmetic from integer weight tables built in binary64 in a
fixed order, so the device must equal it to the byte.

Per axis and plane, S source samples -> D destination samples (1/8 <= S / D <= 8), centre-aligned grids:
  c = ((2i+1) S - D) / (2 D),  inv = min(1, D / S),  r = ceil(support max(1, S / D)),  T = 2r + 2,
  taps j = floor(c) - r .. floor(c) + r + 1,  w = K(|j - c| inv);  then exactly tests/_scale.py's rint / remainder rule and passes.
Where S >= D this is tests/_scale.py itself."""
import numpy as np

import _cabi as A
import _scale as Z
import _ssim as Q

TENT, CUBIC, ONE = Z.TENT, Z.CUBIC, Z.ONE


def taps(S, D, filt):
    r = (Z.SUPPORT[filt] * S + D - 1) // D if S >= D else Z.SUPPORT[filt]
    return 2 * r + 2


def weights(S, D, filt):
    """(start int32 [D], q int16 [D, T]): the taps of output sample i are start[i] .. start[i] + T - 1 (before clamping)"""
    assert S >= 1 and D >= 1 and S <= 8 * D and D <= 8 * S, (S, D)
    T = taps(S, D, filt)
    r = (T - 2) // 2
    i = np.arange(D, dtype=np.int64)
    c = ((2 * i + 1) * S - D).astype(np.float64) / float(2 * D)
    inv = float(D) / float(S) if S >= D else 1.0
    start = np.floor(c).astype(np.int64) - r
    j = start[:, None] + np.arange(T, dtype=np.int64)[None, :]
    w = Z.kernel(np.abs((j.astype(np.float64) - c[:, None]) * inv), filt)
    s = np.zeros(D, dtype=np.float64)
    for t in range(T):                      # ascending j, one addition at a time
        s = s + w[:, t]
    q = np.rint(w * float(ONE) / s[:, None]).astype(np.int64)
    first = np.argmax(q, axis=1)            # the first largest
    q[i, first] += ONE - q.sum(axis=1)
    return start.astype(np.int32), q.astype(np.int16)


def resample_plane(P, dw, dh, filt):
    """uint8 [h, w] -> uint8 [dh, dw], each axis either way"""
    h, w = P.shape
    sx, qh = weights(w, dw, filt)
    sy, qv = weights(h, dh, filt)
    P = P.astype(np.int64)
    H = np.zeros((h, dw), dtype=np.int64)
    for t in range(qh.shape[1]):
        H += qh[:, t].astype(np.int64)[None, :] * P[:, np.clip(sx.astype(np.int64) + t, 0, w - 1)]
    assert np.abs(H).max() < 2 ** 23
    Hs = (H + 128) >> 8
    V = np.zeros((dh, dw), dtype=np.int64)
    for t in range(qv.shape[1]):
        V += qv[:, t].astype(np.int64)[:, None] * Hs[np.clip(sy.astype(np.int64) + t, 0, h - 1), :]
    assert np.abs(V).max() < 2 ** 31
    return np.clip((V + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def planes(frame, w, h, fmt):
    """the Y, U, V planes of one packed frame as 2-D arrays"""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    cw, ch = A.chroma_dims(w, h, fmt)
    out, o = [], 0
    for pw, ph in [(w, h), (cw, ch), (cw, ch)]:
        out.append(frame[o:o + pw * ph].reshape(ph, pw))
        o += pw * ph
    return out


def resample_frame(frame, sw, sh, fmt, dw, dh, filt):
    dcw, dch = A.chroma_dims(dw, dh, fmt)
    return np.concatenate([resample_plane(P, qw, qh, filt).reshape(-1)
                           for P, (qw, qh) in zip(planes(frame, sw, sh, fmt), [(dw, dh), (dcw, dch), (dcw, dch)])])


def resample_clip(clip, sw, sh, fmt, dw, dh, filt):
    """[frames, frame_bytes] -> [frames, resampled frame_bytes]"""
    clip = np.asarray(clip, dtype=np.uint8)
    return np.stack([resample_frame(clip[t], sw, sh, fmt, dw, dh, filt) for t in range(clip.shape[0])])


def src_quality(src_frame, rec_frame, sw, sh, rw, rh, fmt, filt):
    """([3] SSE, [3] SSIM_FX) of a w x h reconstruction upscaled to the source's sw x sh and compared with the source frame"""
    up = resample_frame(rec_frame, rw, rh, fmt, sw, sh, filt)
    sse = np.zeros(3, dtype=np.uint64)
    for p, (a, b) in enumerate(zip(planes(src_frame, sw, sh, fmt), planes(up, sw, sh, fmt))):
        d = a.astype(np.int64) - b.astype(np.int64)
        sse[p] = int((d * d).sum())
    return sse, Q.picture_fx(np.asarray(src_frame).reshape(-1), up, sw, sh, fmt)
