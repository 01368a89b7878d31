"""The temporal noise filter's definition in numpy (include/dsv1_api.h, Temporal noise reduction; csrc/k_denoise.hip computes the same
bytes).

Every plane of a tightly packed planar 8-bit frame is treated on its own, at its own dimensions W x H, with the strength T = luma for
plane 0 and chroma for planes 1 and 2; a plane with T == 0 is copied and keeps no state.  The filter is causal and recursive: per
plane and stream it carries pin, the previous INPUT picture, and S, the filtered value times 16 (uint16, 0..4080).  A stream's state
is 3 * frame_bytes bytes: pin in the frame's layout, then S in the frame's layout as little-endian uint16."""
import numpy as np

import _cabi as A

T_MAX = 512


def valid(luma, chroma):
    return 0 <= luma <= T_MAX and 0 <= chroma <= T_MAX and (luma or chroma) != 0


def state_bytes(w, h, fmt):
    return 3 * A.frame_bytes(w, h, fmt)


def plane_dims(w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    return [(w, h), (cw, ch), (cw, ch)]


def gain(m, T):
    """k of the definition, 4..16, for motion measures m (int array) at strength T >= 1"""
    mid = 4 + (12 * (m - T) + T // 2) // T
    return np.where(m <= T, 4, np.where(m >= 2 * T, 16, mid))


def denoise_plane(cur, pin, S, T, stats=None):
    """one plane [H, W] uint8 of picture t; pin: the same plane of picture t - 1 and S its filter state [H, W] (ints), or both None
    for a stream's first picture -> (out uint8, S' int32).  stats (dict) counts the branches taken."""
    c = cur.astype(np.int32)
    if pin is None:
        S2 = 16 * c
    else:
        d = np.pad(np.abs(c - pin.astype(np.int32)), 1, mode="edge")        # (|cl(cur) - cl(pin)| is the clamped |cur - pin|)
        H, W = cur.shape
        m0 = sum(d[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        S = S.astype(np.int32)
        pout = (S + 8) >> 4
        m1 = 3 * np.abs(c - pout)
        m = np.maximum(m0, m1)
        k = gain(m, T)
        S2 = S + (((16 * c - S) * k + 8) >> 4)
        if stats is not None:
            stats["filtered"] = stats.get("filtered", 0) + m.size
            stats["still"] = stats.get("still", 0) + int((m <= T).sum())
            stats["between"] = stats.get("between", 0) + int(((m > T) & (m < 2 * T)).sum())
            stats["moving"] = stats.get("moving", 0) + int((m >= 2 * T).sum())
            stats["recursive"] = stats.get("recursive", 0) + int((m1 > m0).sum())
            stats["smin"] = min(stats.get("smin", 4080), int(S2.min()))
            stats["smax"] = max(stats.get("smax", 0), int(S2.max()))
    return ((S2 + 8) >> 4).astype(np.uint8), S2


def denoise_clip(clip, w, h, fmt, luma, chroma, state=None, stats=None):
    """clip [n, frame_bytes] uint8 (one stream) -> (out [n, frame_bytes] uint8, state uint8 [3 * frame_bytes]); state: what the call
    before returned, or None where the stream starts"""
    assert valid(luma, chroma)
    fb = A.frame_bytes(w, h, fmt)
    clip = np.ascontiguousarray(clip, dtype=np.uint8).reshape(-1, fb)
    out = np.empty_like(clip)
    new = np.zeros(3 * fb, dtype=np.uint8)
    o = 0
    for p, (pw, ph) in enumerate(plane_dims(w, h, fmt)):
        T, n = (luma if p == 0 else chroma), pw * ph
        if T == 0:
            out[:, o:o + n] = clip[:, o:o + n]
        else:
            pin = S = None
            if state is not None:
                pin = state[o:o + n].reshape(ph, pw)
                S = state[fb + 2 * o:fb + 2 * (o + n)].view("<u2").reshape(ph, pw)
            for t in range(clip.shape[0]):
                cur = clip[t, o:o + n].reshape(ph, pw)
                res, S = denoise_plane(cur, pin, S, T, stats)
                out[t, o:o + n] = res.reshape(-1)
                pin = cur
            assert S.min() >= 0 and S.max() <= 4080
            new[o:o + n] = pin.reshape(-1)
            new[fb + 2 * o:fb + 2 * (o + n)] = S.astype("<u2").reshape(-1).view(np.uint8)
        o += n
    return out, new


def gen_noisy(w, h, fmt, n, seed, sigma=2.0):
    """a noisy test clip [n, frame_bytes]: a static textured left quarter, bars of several slopes and speeds that move, and Gaussian
    noise whose sigma grows from sigma / 4 at the top row to sigma at the bottom, so that every branch of the filter is taken"""
    rng = np.random.default_rng(seed)
    frames = np.empty((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    slopes = (0.0, 1.0, -1.0, 2.0, -0.5)
    dims = plane_dims(w, h, fmt)
    texture = [np.random.default_rng(seed + 1 + k).integers(-24, 25, (ph, pw)) for k, (pw, ph) in enumerate(dims)]
    for t in range(n):
        parts = []
        for k, (pw, ph) in enumerate(dims):
            y, x = np.mgrid[0:ph, 0:pw].astype(np.float64)
            band = np.minimum((y * len(slopes) // max(ph, 1)).astype(np.int64), len(slopes) - 1)
            period = 23.0 + 6.0 * band + 5 * k
            speed = 0.25 + 0.5 * band
            v = 128 + 90 * np.sin(2 * np.pi * (x + np.asarray(slopes)[band] * y + speed * t) / period)
            still = x < pw // 4
            v = np.where(still, 128 + texture[k], v)
            sg = sigma * (0.25 + 0.75 * y / max(ph - 1, 1))
            parts.append(np.clip(np.rint(v + sg * rng.standard_normal(v.shape)), 0, 255).astype(np.uint8).reshape(-1))
        frames[t] = np.concatenate(parts)
    return frames


def gen_scene(w, h, fmt, n, seed, sigma, speed):
    """(clean, noisy) clips [n, frame_bytes] of a sine plus checkerboard scene that moves `speed` samples per picture along x"""
    rng = np.random.default_rng(seed)
    clean = np.empty((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    noisy = np.empty_like(clean)
    for t in range(n):
        a, b = [], []
        for k, (pw, ph) in enumerate(plane_dims(w, h, fmt)):
            y, x = np.mgrid[0:ph, 0:pw].astype(np.float64)
            xs = x + speed * t
            v = 128 + 50 * np.sin(2 * np.pi * (xs + 0.5 * y) / 13.0) + 40 * (((np.floor(xs / 6) + np.floor(y / 6)) % 2) - 0.5)
            a.append(np.clip(np.rint(v), 0, 255).astype(np.uint8).reshape(-1))
            b.append(np.clip(np.rint(v + sigma * rng.standard_normal(v.shape)), 0, 255).astype(np.uint8).reshape(-1))
        clean[t], noisy[t] = np.concatenate(a), np.concatenate(b)
    return clean, noisy


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max((d * d).mean(), 1e-12))


# the standalone cases of tests/test_gpu_denoise.py (tests/test_denoise_host.py checks what their clips reach): all rows aligned; none;
# tails; odd sizes (both clamps); a chroma plane of one row; three rows; one sample
GPU_GEOMS = [(352, 288, A.SUBSAMP_420), (250, 130, A.SUBSAMP_422), (36, 20, A.SUBSAMP_411), (35, 19, A.SUBSAMP_444),
             (16, 2, A.SUBSAMP_420), (64, 3, A.SUBSAMP_422), (1, 1, A.SUBSAMP_444)]
GPU_STRENGTHS = [(24, 24), (40, 0), (0, 16), (512, 1)]
GPU_FRAMES, GPU_SEED = 4, 0xD7


def gpu_case(w, h, fmt):
    """the standalone GPU test's input for a geometry: (the GPU_FRAMES pictures it filters, the picture before them)"""
    clip = gen_noisy(w, h, fmt, GPU_FRAMES + 1, GPU_SEED)
    return clip[1:], clip[0]


def planes_fast(w, h, fmt):
    """per plane: is every row 16-byte aligned in buffers that start aligned -- the kernel's rule for its 16-byte path
    (csrc/k_denoise.hip: dn_launch)"""
    fb = A.frame_bytes(w, h, fmt)
    o, res = 0, []
    for pw, ph in plane_dims(w, h, fmt):
        res.append((fb | o | pw) % 16 == 0)
        o += pw * ph
    return res
