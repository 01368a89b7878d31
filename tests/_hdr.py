"""HDR sources (include/dsv1_api.h, HDR sources; csrc/k_hdr.hip) stated in numpy: the definition the GPU is held to.  Written from the
definition, not from the kernel.  Two layers, as the header has them: build() makes the tables of settings in float64 and exact
rationals (what dsv1_hdr_build is compared with, entry by entry); import_() is the pixel path, a pure integer function of (tables,
layout, upsample) in int64 -- steps a to i.  float_pixels() is a float64 model of the same chain with no table and no rounding
anywhere, against which the integer definition itself is measured."""
from fractions import Fraction as Fr

import numpy as np

import _cabi as A
import _pixfmt as PF
import _rgb as RG

PQ, HLG = 0, 1
CLIP, REINHARD, BT2390 = 0, 1, 2
CURVES = [CLIP, REINHARD, BT2390]
ONE = 1 << 20
NBUCKETS = 3329
SUBSAMPS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420]
PAIRS = [(A.SUBSAMP_420, A.SUBSAMP_420), (A.SUBSAMP_422, A.SUBSAMP_422), (A.SUBSAMP_444, A.SUBSAMP_444), (A.SUBSAMP_422, A.SUBSAMP_420),
         (A.SUBSAMP_444, A.SUBSAMP_420), (A.SUBSAMP_444, A.SUBSAMP_422)]
# BT.2087, BT.2020 -> BT.709 primaries, in 1 / 10000; the diagonal is the remainder of its row
G2087 = [[None, -5876, -728], [-1246, None, -83], [-182, -1006, None]]
TABLE_KEYS = ("ycc", "in_oy", "in_oc", "eotf", "gamut", "gain", "oetf", "fwd", "ybias", "cbias")


def hd(transfer=PQ, matrix=RG.BT2020, full=0, gamut=1, curve=BT2390, peak=1000, white=203, out_matrix=RG.BT709, out_full=0):
    return dict(transfer=transfer, matrix=matrix, full=full, gamut=gamut, curve=curve, peak=peak, white=white, out_matrix=out_matrix,
                out_full=out_full)


def valid(h):
    return (h["transfer"] in (PQ, HLG) and h["matrix"] in RG.MATRICES and h["out_matrix"] in RG.MATRICES and h["full"] in (0, 1) and
            h["out_full"] in (0, 1) and h["gamut"] in (0, 1) and h["curve"] in CURVES and 100 <= h["peak"] <= 10000 and
            (h["white"] == 0 or 48 <= h["white"] <= 1000) and (h["white"] or 203) <= h["peak"])


# ---- buckets ----
def cidx(v):
    """v <= 2^20 (array) -> its bucket"""
    v = np.asarray(v, dtype=np.int64)
    e = np.floor(np.log2(np.maximum(v, 1))).astype(np.int64)      # exact: v < 2^53
    e = np.where((1 << e) > v, e - 1, e)
    big = ((e - 7) << 8) | ((v >> np.maximum(e - 8, 0)) & 255)
    return np.where(v < 256, v, big)


def bucket_rep(i):
    i = np.asarray(i, dtype=np.int64)
    e = (i >> 8) + 7
    sh = np.maximum(e - 8, 0)
    r = ((256 + (i & 255)) << sh) + ((1 << sh) >> 1)
    return np.where(i < 256, i, np.minimum(r, ONE))


# ---- settings -> tables ----
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


def pq_nits(e):
    p = np.power(np.asarray(e, dtype=np.float64), 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def pq_signal(nits):
    yp = np.power(np.asarray(nits, dtype=np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * yp) / (1.0 + C3 * yp), M2)


def hlg_scene(e):
    e = np.asarray(e, dtype=np.float64)
    a = 0.17883277
    b, c = 1.0 - 4.0 * a, 0.5 - a * np.log(4.0 * a)
    return np.where(e <= 0.5, e * e / 3.0, (np.exp((np.maximum(e, 0.5) - c) / a) + b) / 12.0)


def tonemap(h, m):
    """nits -> SDR linear 0..1"""
    m = np.asarray(m, dtype=np.float64)
    peak, white = float(h["peak"]), float(h["white"] or 203)
    if h["curve"] == CLIP:
        t = m / white
    elif h["curve"] == REINHARD:
        x, l = m / white, peak / white
        t = x * (1.0 + x / (l * l)) / (1.0 + x)
    else:
        pw = pq_signal(peak)
        e1, maxl = pq_signal(m) / pw, pq_signal(white) / pw
        ks = 1.5 * maxl - 0.5
        e2 = e1
        if ks < 1.0:
            s = (e1 - ks) / (1.0 - ks)
            s2, s3 = s * s, s * s * s
            p = (2.0 * s3 - 3.0 * s2 + 1.0) * ks + (s3 - 2.0 * s2 + s) * (1.0 - ks) + (-2.0 * s3 + 3.0 * s2) * maxl
            e2 = np.where(e1 >= ks, p, e1)
        t = pq_nits(e2 * pw) / white
    return np.minimum(t, 1.0)


def rnd(x):
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5)


def ycc_rows(matrix, full):
    """IY, RV, GU, GV, BU in Q14 from the 10-bit signal to 0..4095 (exact)"""
    kr, kb = RG.K[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fr(4095, 1023), Fr(4095, 1023)) if full else (Fr(4095, 876), Fr(4095, 896))
    return [RG.r(16384 * sy), RG.r(16384 * 2 * (1 - kr) * sc), -RG.r(16384 * 2 * (1 - kb) * kb / kg * sc), -RG.r(16384 * 2 * (1 - kr) * kr / kg * sc),
            RG.r(16384 * 2 * (1 - kb) * sc)]


def fwd_rows(matrix, full):
    """Q20 rows Y, Cb, Cr from E' 0..4095 to the 8-bit signal (exact): the RGB section's rules with 4095 in the place of 255"""
    kr, kb = RG.K[matrix]
    sy, sc = (Fr(255, 4095), Fr(255, 4095)) if full else (Fr(219, 4095), Fr(224, 4095))
    q = 1 << 20
    yr, yb = RG.r(q * sy * kr), RG.r(q * sy * kb)
    hf = RG.r(q * sc / 2)
    cbr = -RG.r(q * sc * kr / (2 * (1 - kb)))
    crb = -RG.r(q * sc * kb / (2 * (1 - kr)))
    return [yr, RG.r(q * sy) - yr - yb, yb, cbr, -(hf + cbr), hf, hf, -(hf + crb), crb]


def gamut_rows(on):
    g = []
    for i in range(3):
        row = [0 if (i == j or not on) else -RG.r(Fr(16384 * -G2087[i][j], 10000)) for j in range(3)]
        row[i] = 16384 - sum(row)
        g += row
    return g


def build(h):
    """the tables of settings h: dict of python ints and int64 arrays"""
    assert valid(h)
    peak, white = float(h["peak"]), float(h["white"] or 203)
    e = np.arange(4096) / 4095.0
    lin = np.minimum(pq_nits(e), peak) / peak if h["transfer"] == PQ else hlg_scene(e)
    f = bucket_rep(np.arange(NBUCKETS)) / float(ONE)
    fs = np.where(f == 0.0, 1.0, f)
    gain = rnd(65536.0 * tonemap(h, fs * peak if h["transfer"] == PQ else peak * np.power(fs, 1.2)) / fs)
    gain[0] = rnd(65536.0 * peak / white) if h["transfer"] == PQ else 0.0
    return dict(ycc=ycc_rows(h["matrix"], h["full"]), in_oy=0 if h["full"] else 64, in_oc=512,
                eotf=np.minimum(rnd(ONE * lin), ONE).astype(np.int64), gamut=gamut_rows(h["gamut"]),
                gain=np.minimum(gain, 4294967295.0).astype(np.int64), oetf=rnd(4095.0 * np.power(f, 1.0 / 2.4)).astype(np.int64),
                fwd=fwd_rows(h["out_matrix"], h["out_full"]), ybias=((0 if h["out_full"] else 16) << 20) + (1 << 19), cbias=(128 << 20) + (1 << 19))


def tables_valid(T):
    return (all(abs(int(x)) <= 1 << 19 for x in T["ycc"]) and 0 <= T["in_oy"] <= 1023 and 0 <= T["in_oc"] <= 1023 and
            int(np.max(T["eotf"])) <= ONE and int(np.min(T["eotf"])) >= 0 and all(abs(int(x)) <= 1 << 18 for x in T["gamut"]) and
            0 <= int(np.min(T["gain"])) and int(np.max(T["gain"])) < 1 << 32 and 0 <= int(np.min(T["oetf"])) and int(np.max(T["oetf"])) <= 4095 and
            all(abs(int(x)) <= 1 << 16 for x in T["fwd"]) and abs(T["ybias"]) <= 1 << 30 and abs(T["cbias"]) <= 1 << 30)


def random_tables(rng):
    """entries anywhere inside the valid bounds: every lookup and every rounding shows"""
    return dict(ycc=[int(x) for x in rng.integers(-(1 << 19), (1 << 19) + 1, 5)], in_oy=int(rng.integers(0, 1024)), in_oc=int(rng.integers(0, 1024)),
                eotf=rng.integers(0, ONE + 1, 4096), gamut=[int(x) for x in rng.integers(-(1 << 18), (1 << 18) + 1, 9)],
                gain=rng.integers(0, 1 << 32, NBUCKETS), oetf=rng.integers(0, 4096, NBUCKETS),
                fwd=[int(x) for x in rng.integers(-(1 << 16), (1 << 16) + 1, 9)], ybias=int(rng.integers(-(1 << 30), (1 << 30) + 1)),
                cbias=int(rng.integers(-(1 << 30), (1 << 30) + 1)))


# ---- tables -> pixels ----
def sample10(x, depth, msb):
    """step a: 16-bit words -> 10-bit samples"""
    x = np.asarray(x, dtype=np.uint16).astype(np.int64)
    v = (x >> (16 - depth)) if msb else (x & ((1 << depth) - 1))
    return v if depth == 10 else np.minimum(1023, (v + (1 << (depth - 11))) >> (depth - 10))


def pixels(T, Y, U, V):
    """steps c to h on 4:4:4 10-bit samples: the 8-bit Y, Cb, Cr as int64 arrays"""
    IY, RV, GU, GV, BU = (int(x) for x in T["ycc"])
    eotf, gain, oetf = (np.asarray(T[k], dtype=np.int64) for k in ("eotf", "gain", "oetf"))
    G, F = [int(x) for x in T["gamut"]], [int(x) for x in T["fwd"]]
    y, u, v = np.asarray(Y, dtype=np.int64) - T["in_oy"], np.asarray(U, dtype=np.int64) - T["in_oc"], np.asarray(V, dtype=np.int64) - T["in_oc"]
    idx = [np.clip((IY * y + RV * v + 8192) >> 14, 0, 4095), np.clip((IY * y + GU * u + GV * v + 8192) >> 14, 0, 4095),
           np.clip((IY * y + BU * u + 8192) >> 14, 0, 4095)]
    lin = [eotf[i] for i in idx]
    c = [np.clip((G[3 * k] * lin[0] + G[3 * k + 1] * lin[1] + G[3 * k + 2] * lin[2] + 8192) >> 14, 0, ONE) for k in range(3)]
    g = gain[cidx(np.maximum(np.maximum(c[0], c[1]), c[2]))]
    assert int(g.max(initial=0)) < 1 << 32                      # (c g + 32768 < 2^53: int64 holds it)
    E = [oetf[cidx(np.minimum((x * g + 32768) >> 16, ONE))] for x in c]
    return [np.clip((F[3 * k] * E[0] + F[3 * k + 1] * E[1] + F[3 * k + 2] * E[2] + (T["ybias"] if k == 0 else T["cbias"])) >> 20, 0, 255) for k in range(3)]


def unpack(buf, f, w, h, sub, n):
    """the raw clip -> 10-bit Y [n, h, w], U and V [n, ch, cw]: only the bytes of samples are looked at"""
    lay, _, fb = PF.plane_layout(f, w, h, sub)
    buf = np.asarray(buf).view(np.uint8).reshape(-1)
    cw, ch = A.chroma_dims(w, h, sub)

    def plane(t, k):
        off, pitch, rb, nr = lay[k]
        r = np.stack([buf[t * fb + off + y * pitch: t * fb + off + y * pitch + rb] for y in range(nr)])
        return sample10(np.ascontiguousarray(r).view("<u2"), f["depth"], f["msb"])

    Y, U, V = [], [], []
    for t in range(n):
        Y.append(plane(t, 0))
        if f["layout"] == PF.PLANAR:
            U.append(plane(t, 1))
            V.append(plane(t, 2))
        else:
            c2 = plane(t, 1).reshape(ch, cw, 2)
            a, b = (0, 1) if f["layout"] == PF.SEMI_UV else (1, 0)
            U.append(c2[:, :, a])
            V.append(c2[:, :, b])
    return np.stack(Y), np.stack(U), np.stack(V)


def layout_valid(f, w, h, src_sub, sub):
    return (f["depth"] in (10, 12, 16) and f["layout"] in (PF.PLANAR, PF.SEMI_UV, PF.SEMI_VU) and (src_sub, sub) in PAIRS and
            PF.plane_layout(f, w, h, src_sub) is not None)


def import_(buf, f, w, h, src_sub, sub, n, T, upsample):
    """raw HDR clip -> uint8 [n, frame_bytes(w, h, sub)] packed planar SDR"""
    assert layout_valid(f, w, h, src_sub, sub) and upsample in (RG.REPLICATE, RG.LINEAR)
    Y, U, V = unpack(buf, f, w, h, src_sub, n)
    out = np.zeros((n, A.frame_bytes(w, h, sub)), dtype=np.uint8)
    for t in range(n):
        u, v = RG.upsample(U[t], w, h, src_sub, upsample), RG.upsample(V[t], w, h, src_sub, upsample)       # step b, on 10-bit values
        Yo, Cb, Cr = pixels(T, Y[t], u, v)
        cb, cr = RG.halve(Cb.astype(np.uint8), sub), RG.halve(Cr.astype(np.uint8), sub)                     # step i
        assert cb.shape == A.chroma_dims(w, h, sub)[::-1]
        out[t] = np.concatenate([Yo.astype(np.uint8).reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    return out


# ---- the float64 model of the same chain: no table, no rounding ----
def float_pixels(h, Y, U, V):
    """10-bit limited- or full-range samples (4:4:4) -> the SDR signal Y, Cb, Cr as float64, unrounded and clipped to 0..255"""
    kr, kb = (float(x) for x in RG.K[h["matrix"]])
    kg = 1.0 - kr - kb
    Y, U, V = (np.asarray(x, dtype=np.float64) for x in (Y, U, V))
    if h["full"]:
        y, u, v = Y / 1023.0, (U - 512.0) / 1023.0, (V - 512.0) / 1023.0
    else:
        y, u, v = (Y - 64.0) / 876.0, (U - 512.0) / 896.0, (V - 512.0) / 896.0
    sig = [y + 2.0 * (1.0 - kr) * v, y - 2.0 * (1.0 - kb) * kb / kg * u - 2.0 * (1.0 - kr) * kr / kg * v, y + 2.0 * (1.0 - kb) * u]
    sig = [np.clip(x, 0.0, 1.0) for x in sig]
    peak = float(h["peak"])
    lin = [np.minimum(pq_nits(x), peak) / peak if h["transfer"] == PQ else hlg_scene(x) for x in sig]
    G = np.array(gamut_rows(h["gamut"]), dtype=np.float64).reshape(3, 3) / 16384.0
    c = [np.clip(G[k, 0] * lin[0] + G[k, 1] * lin[1] + G[k, 2] * lin[2], 0.0, 1.0) for k in range(3)]
    m = np.maximum(np.maximum(c[0], c[1]), c[2])
    ms = np.where(m == 0.0, 1.0, m)
    gain = tonemap(h, ms * peak if h["transfer"] == PQ else peak * np.power(ms, 1.2)) / ms
    E = [np.power(np.minimum(x * gain, 1.0), 1.0 / 2.4) for x in c]
    kr, kb = (float(x) for x in RG.K[h["out_matrix"]])
    kg = 1.0 - kr - kb
    sy, sc, oy = (255.0, 255.0, 0.0) if h["out_full"] else (219.0, 224.0, 16.0)
    yl = kr * E[0] + kg * E[1] + kb * E[2]
    return [np.clip(oy + sy * yl, 0.0, 255.0), np.clip(128.0 + sc * (E[2] - yl) / (2.0 * (1.0 - kb)), 0.0, 255.0),
            np.clip(128.0 + sc * (E[0] - yl) / (2.0 * (1.0 - kr)), 0.0, 255.0)]
