"""The cases of the decoder output scale (include/dsv1_api.h, decoder output scale), shared by tests/test_gpu_outscale.py and the host
test that keeps them honest without a GPU (tests/test_outscale_host.py): the geometries, the targets that must be taken and the ones
that must be refused, and the numpy definition's own ratio rule (tests/_resample.py weights(): 1/8 <= S / D <= 8 on every axis of
every plane, each plane scaled on its own at the stream's subsampling)."""
import _cabi as A

S420, S422, S444 = A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444

# context level, hostile borders: (w, h, subsampling) -> targets.  250x130: an exact half (odd chroma 125x65 -> 63x33); 63x17: the last
# quad of a row is three samples (the byte stores) and the height ratio is near 8; doubled; anamorphic, up and down; the identity tables.
# 100x36 at 4:4:4: a half, 13x288 (near 8 down across, exactly 8 up the rows), the identity
CTX_TARGETS = {
    (250, 130, S420): [(125, 65), (63, 17), (500, 260), (333, 40), (250, 130)],
    (100, 36, S444): [(50, 18), (13, 288), (100, 36)],
}

# batched decoder: the streams of tests/test_gpu_pixout.py streams_of() -> targets (44x36 and 45x25: ratio 8)
DEC_TARGETS = {
    (352, 288, S420): [(176, 144), (44, 36), (704, 576)],
    (360, 200, S422): [(45, 25), (641, 75)],
    (320, 240, S444): [(321, 239), (100, 36)],
}

# refused from 352x288 4:2:0: luma 352 / 43 > 8; 8x up is 2816 across and 2304 down; 288 / 35 > 8; sizes that are not positive.
# From 250x130: 250 / 31 and 130 / 16 are just above 8.  ACCEPTED_EDGE: their neighbours on the allowed side of the bound
REFUSED = {
    (352, 288, S420): [(43, 36), (2817, 288), (352, 35), (352, 2305), (0, 144), (176, 0), (-176, -144)],
    (250, 130, S420): [(31, 65), (250, 16)],
}
ACCEPTED_EDGE = {
    (352, 288, S420): [(44, 36), (2816, 288), (352, 2304)],
    (250, 130, S420): [(32, 65), (250, 17)],
}


def plane_dims(w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    return [(w, h), (cw, ch), (cw, ch)]


def ratio_ok(sw, sh, fmt, dw, dh):
    """the numpy definition's rule (tests/_resample.py weights(): its assertion), per plane and axis"""
    if dw < 1 or dh < 1:
        return False
    for (pw, ph), (qw, qh) in zip(plane_dims(sw, sh, fmt), plane_dims(dw, dh, fmt)):
        for S, D in ((pw, qw), (ph, qh)):
            if not (S >= 1 and D >= 1 and S <= 8 * D and D <= 8 * S):
                return False
    return True
