"""Bit-level helpers shared by the decoder tests: a writer and a reader of the reference's codes (bs.c:129-219), the plane
framing (hzcc.c:449-476) and the splicing of hand-built plane payloads into real picture packets (dsv_decoder.c:335-400)."""
import numpy as np


class BW:
    """MSB-first bit writer with the interleaved exp-Golomb codes (bs.c:129-206)"""

    def __init__(self):
        self.bits = []

    def put(self, n, v):
        for i in range(n - 1, -1, -1):
            self.bits.append((v >> i) & 1)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def ueg(self, v):
        m = v + 1
        k = m.bit_length() - 1
        for i in range(k - 1, -1, -1):
            self.bits.append(0)
            self.bits.append((m >> i) & 1)
        self.bits.append(1)

    def seg(self, v):
        self.ueg(abs(v))
        if v:
            self.bits.append(1 if v < 0 else 0)

    def neg(self, v):
        self.ueg(abs(v) - 1)
        self.bits.append(1 if v < 0 else 0)

    @property
    def nbits(self):
        return len(self.bits)

    def bytes(self):
        self.align()
        a = np.packbits(np.array(self.bits, dtype=np.uint8))
        return a.tobytes()


def plane_payload(dc, entries):
    """bytes that follow a plane's 32-bit length: SEG(DC), run count, UEG(run) / NEG(value) chain, end-of-plane symbol.
    entries: (scan position, symbol) pairs, positions increasing, position 0 is the DC's cell and never coded"""
    w = BW()
    w.seg(dc)
    w.align()
    w.put(32, len(entries))
    w.align()
    prev, stored = 0, 0
    for pos, v in entries:
        assert pos > prev - 1 and v != 0
        w.ueg(pos - prev)          # zeros skipped since the cell after the previous non-zero (run restarts at 0 there)
        if stored:
            w.neg(stored)
        stored = v
        prev = pos + 1
    if stored:
        w.neg(stored)
    w.align()
    w.put(8, 0x55)
    w.align()
    return w.bytes()


class BR:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bit(self):
        b = (self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7

    def ueg(self):
        m = 1
        while not self.bit():
            m = (m << 1) | self.bit()
        return m - 1


def plane_offsets(pkt):
    """byte offsets of the three planes' 32-bit length fields in a picture packet (dsv_decoder.c:335-400)"""
    r = BR(pkt)
    r.pos = 14 * 8
    r.align(); r.bits(32); r.align(); r.ueg(); r.ueg(); r.align()
    r.align(); n = r.ueg(); r.align(); r.pos += 8 * n
    if pkt[5] & 1:
        r.align()
        for _ in range(4):
            n = r.ueg(); r.align(); r.pos += 8 * n
    r.align()
    r.bits(11)
    offs = []
    for _ in range(3):
        r.align()
        offs.append(r.pos >> 3)
        plen = r.bits(32)
        r.align()
        r.pos += 8 * plen
    assert (r.pos >> 3) == len(pkt)
    return offs


def splice(pkt, planes):
    """the packet with planes {index: payload bytes} replaced; next-link word updated"""
    offs = plane_offsets(pkt)
    out = bytearray(pkt[:offs[0]])
    for p in range(3):
        if p in planes:
            pay = planes[p]
        else:
            ln = int.from_bytes(pkt[offs[p]:offs[p] + 4], "big")
            pay = pkt[offs[p] + 4:offs[p] + 4 + ln]
        out += len(pay).to_bytes(4, "big") + pay
    out[10:14] = len(out).to_bytes(4, "big")
    return bytes(out)


def region_base(w, h, l, s):
    """first scan position of sub-band s (1 LH, 2 HL, 3 HH) of scan level l (hzcc.c:30-48: round-up dimensions per level)"""
    dim = lambda v, lv: (v + (1 << (3 - lv)) - 1) >> (3 - lv)
    base = dim(w, 0) * dim(h, 0)
    for lv in range(l):
        base += 3 * dim(w, lv) * dim(h, lv)
    return base + (s - 1) * dim(w, l) * dim(h, l), dim(w, l)
