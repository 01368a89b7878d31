"""A model of the branches of the entropy decoder (csrc/k_hzcc.hip: k_hz_parse, k_hz_codes, k_hz_positions, k_hz_scatter_lv,
k_hz_dec_resolve, k_hz_unscatter, k_dec_clear and their launchers).

Pure Python and numpy; nothing of the product is loaded.  The input is ONE plane: width, height, the bytes that follow the
plane's 32-bit length (with whatever lies behind them in the buffer) and the `len` handed to the decoder.

Two restatements, both in Python integers:

  * read_entries / coef_plane -- the reference's reader, the high-precision reference of the stage: the bit reader
    (bs.c:148-219), the entry walk (hzcc.c:295-435: U(run_1), then per entry the next run, the value, and "stop at the first
    value after which bytepos >= len"), the dequantiser (hzcc.c:77-92, 121-135) and the DC that dsv_decode_plane writes last
    (hzcc.c:495).  Three of its rules can be flipped (RULES) so that a test can show they matter.
  * Plane -- the kernels' decomposition of the same bits: the device sees `len` bytes and zeros behind them; S0 is the first
    bit after U(run_1); from S0 the bits are cut into chunks of PARSE_BITS, PARSE_THREADS chunks a pass, 64 chunks a wave; per
    chunk the machine state it is entered with, the code ends per 64-bit word, cbase (codes that ended before it) and prev_end
    (the bit after the last of them); per code what k_hz_codes decodes from those facts; then k_hz_positions' 64-bit prefix sum
    and the prefix of entries inside the scan.  Plane.entries must be read_entries' list: tests/test_hzdec_plan_host.py checks
    that on every case, so the decomposition itself is verified on the CPU before anything runs on a device.

Out of the decomposition comes a set of LABELS, one per branch; LABELS says which kernel and which condition each names.
tests/hzdec_cases.py lists the cases with the labels each is there for, tests/test_hzdec_plan_host.py proves that every label
outside UNREACHABLE is reached, tests/test_gpu_hzdec_paths.py runs the cases on the device.
"""
import numpy as np

import hz_plan as H

PARSE_THREADS = 1024              # chunks per pass of k_hz_parse
PARSE_BITS = 128                  # bits per chunk
HZ_CHUNK = 2048                   # scan cells per chunk of the pack stage: the entry arrays hold nchunks * HZ_CHUNK
POS_ITEMS = 8                     # entries per thread and pass of k_hz_positions
WAVE = 64
PASS_BITS = PARSE_THREADS * PARSE_BITS
INT_MAX = 0x7fffffff
MINQ = 16

# the machine of parse_step: state x bit -> (state, a code ends with this bit).  0 U flag, 1 U data, 2 N flag, 3 N data, 4 sign
STEP = {0: ((1, False), (2, True)), 1: ((0, False), (0, False)), 2: ((3, False), (4, False)), 3: ((2, False), (2, False)),
        4: ((0, True), (0, True))}
STATE_NAMES = ["U flag", "U data", "N flag", "N data", "sign"]

RULES = dict(trunc_ge=True, later_wins=True, plus1=True)      # the reader's rules a test may flip (never the kernels' model)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's reader
class Bits:
    """MSB-first reader over a byte buffer (bs.c:65-74, 148-219); reading past the buffer is an error of the CASE: the reference
    would read out of bounds"""

    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8)).tolist()
        self.pos = 0

    def bit(self):
        assert self.pos < len(self.b), "the reference reads past the buffer: not a payload it defines"
        v = self.b[self.pos]
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7

    def ueg(self):
        v = 1
        while not self.bit():
            v = (v << 1) | self.bit()
        return v - 1

    def seg(self):
        v = self.ueg()
        return -v if v and self.bit() else v

    def neg(self):
        v = self.ueg() + 1
        return -v if self.bit() else v


def read_header(rd):
    """(DC, announced count as the reference's int, bit position of U(run_1)): dsv_decode_plane hzcc.c:479-487, hzcc_dec :309-311"""
    dc = rd.seg()
    rd.align()
    runs = rd.bits(32)
    rd.align()
    return dc, runs - (1 << 32) if runs >= 1 << 31 else runs, rd.pos


def read_entries(buf, length, nscan, rules=RULES):
    """(DC, [(scan position, value)]) as hzcc_dec walks them.  The reference steps cell by cell and counts `run` down; jumping
    by run + 1 is the same walk as long as a run is at most INT_MAX (the cases keep them at or below 2^31 - 2)"""
    rd = Bits(buf)
    dc, runs, _ = read_header(rd)

    def next_run():
        nonlocal runs
        runs -= 1
        return rd.ueg() if runs >= 0 else INT_MAX
    out, p = [], next_run()
    while p < nscan:
        nxt = next_run()
        v = rd.neg()
        if (rd.pos >> 3) >= length if rules["trunc_ge"] else (rd.pos >> 3) > length:       # hzcc.c:337-339
            break
        out.append((p, v))
        p += nxt + (1 if rules["plus1"] else 0)
    return dc, out


def lb2(n):
    i, l = 1, 0
    while i < n:
        i, l = i << 1, l + 1
    return l


def level_quant(q, isP, level):
    """dsv_get_quant hzcc.c:77-92 of a plane without stable blocks; level -1 is the LL region (level 0's quantiser); level 2 is
    the shift of dequantH"""
    qq = q * 3 // 2 if isP else q
    if level == 1:
        qq = qq * 2 // 3
    elif level == 2:
        qq = qq * 3 // 2
    qq = max(qq, MINQ)
    return lb2(qq) if level == 2 else qq


def dequant(v, level, q=16, isP=0):
    """dequant / dequantH hzcc.c:121-135, no stable block (tmq4pos leaves the quantiser as it is)"""
    t = level_quant(q, isP, level)
    if level == 2:
        r = (v << t) & 0xffffffff
        return r - (1 << 32) if r >= 1 << 31 else r
    m = (abs(v) * 2 * t + t) >> 1
    assert m <= INT_MAX, "value x quantiser leaves the reference's int"
    return -m if v < 0 else m


def coef_plane(w, h, dc, entries, q=16, isP=0, rules=RULES):
    """the int32 coefficient plane hzcc_dec leaves (zeros where it wrote nothing): entries in scan order, so a cell two regions
    share ends with the later region's value; the DC last"""
    out = np.zeros((h, w), dtype=np.int64)
    for p, v in (entries if rules["later_wins"] else reversed(entries)):
        x, y, level = H.cell_of(w, h, p)
        out[y, x] = dequant(v, level, q, isP)
    out[0, 0] = dc
    return out.astype(np.int32).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# LABELS: name -> kernel: condition
LABELS = {
    # k_hz_parse: the head
    "pa.runs0": "k_hz_parse: n <= 0 by an announced count of 0: the workgroup leaves after writing entry 0",
    "pa.runs_neg": "k_hz_parse: an announced count of 2^31 or more is negative as int: n <= 0",
    "pa.runs_clamped": "k_hz_parse: announced count above cap = nchunks * HZ_CHUNK - 1: n = cap",
    "pa.u1.len1": "k_hz_parse, tid 0: U(run_1) of one bit (k = 0)",
    "pa.u1.gt31": "k_hz_parse, tid 0: U(run_1) of more than 31 bits (ueg_value's 64-bit body)",
    "pa.u1.w0": "k_hz_parse, tid 0: the 64 bits at U(run_1) are all zero (w == 0, k = 31): on data the reference defines only where len ends before U(run_1)",
    "pa.u1.cut": "k_hz_parse: the data ends inside U(run_1) or with it: S0 >= endbits, no pass runs",
    # the pass loop
    "pa.pass1": "k_hz_parse: one pass",
    "pa.pass2": "k_hz_parse: two passes",
    "pa.pass3": "k_hz_parse: three or more passes",
    **{"pa.chunk.s%d" % s: "k_hz_parse: a chunk entered in state %d (%s): st_in through the wave scan" % (s, STATE_NAMES[s]) for s in range(5)},
    **{"pa.wave.s%d" % s: "k_hz_parse: thread 64k, k >= 1, entered in state %d (%s): st_in through s_wmap alone" % (s, STATE_NAMES[s]) for s in range(5)},
    **{"pa.pass.s%d" % s: "k_hz_parse: a pass after the first entered in state %d (%s): the carried s_state" % (s, STATE_NAMES[s]) for s in range(5)},
    "pa.straddle.chunk": "k_hz_parse: a decoded code straddles a chunk boundary inside a wave: prev_end through the lane scan",
    "pa.straddle.wave": "k_hz_parse: a decoded code straddles a wave boundary: prev_end through s_wlast",
    "pa.straddle.pass": "k_hz_parse: a decoded code straddles a pass boundary: prev_end is the carried s_lastend",
    "pa.lbefore_neg": "k_hz_parse: a chunk other than a pass's first, with codes to decode, takes prev_end from s_lastend (lbefore < 0)",
    "pa.m0_empty": "k_hz_parse / k_hz_codes: a chunk with codes to decode has no code end in its first word (m0 == 0, m1 != 0)",
    "pa.m1_empty": "k_hz_parse / k_hz_codes: a chunk with codes to decode has no code end in its second word (m1 == 0)",
    "pa.m_none": "k_hz_codes: a chunk inside the data without any code end: leaves at !(m0 | m1)",
    "pa.end.keep_lt64": "parse_chunk_bits: the data ends in a chunk's first word (0 < keep < 64)",
    "pa.end.keep_64": "parse_chunk_bits: the data ends between a chunk's words (keep == 64)",
    "pa.end.keep_gt64": "parse_chunk_bits: the data ends in a chunk's second word (64 < keep < 128)",
    "pa.end.past": "parse_chunk_bits: a chunk of a running pass lies wholly past the data (keep <= 0)",
    "pa.all_found": "k_hz_parse / k_hz_codes: all announced codes end before the data does; the ends that follow are ignored (j >= ncodes)",
    "pa.short.even": "k_hz_positions: the data ends first, ncode < ncodes, ncode even",
    "pa.short.odd": "k_hz_positions: the data ends first, ncode < ncodes, ncode odd: the run without its value is dropped",
    # k_hz_codes
    "cd.run.u31": "k_hz_codes: a run code of at most 31 bits (ueg_value32)",
    "cd.run.u63": "k_hz_codes: a run code of more than 31 bits (ueg_value)",
    "cd.val.u31": "k_hz_codes: a value code whose U part has at most 31 bits (ueg_value32)",
    "cd.val.u63": "k_hz_codes: a value code whose U part has more than 31 bits (ueg_value)",
    "cd.start.prev.al": "k_hz_codes: a code that starts in the previous chunk's second word at its bit 0 (idx 0, sh 0)",
    "cd.start.prev.un": "k_hz_codes: a code that starts inside the previous chunk's second word (idx 0, sh != 0)",
    "cd.start.w0.al": "k_hz_codes: a code that starts at the chunk's bit 0 (idx 1, sh 0)",
    "cd.start.w0.un": "k_hz_codes: a code that starts inside the chunk's first word (idx 1, sh != 0)",
    "cd.start.w1.al": "k_hz_codes: a code that starts at the chunk's bit 64 (idx 2, sh 0)",
    "cd.start.w1.un": "k_hz_codes: a code that starts inside the chunk's second word (idx 2, sh != 0)",
    "cd.rel_neg": "k_hz_codes: a code that starts before the previous chunk's second word (rel < 0): the reload",
    "cd.last.n1": "k_hz_codes: the final code is the only one (n == 1): it starts at S0",
    "cd.last.sign.same": "k_hz_codes: the final code's sign bit lies in the chunk its U part ends in",
    "cd.last.sign.chunk": "k_hz_codes: the final code's sign bit is the next chunk's first bit",
    "cd.last.sign.pass": "k_hz_codes: the final code's sign bit is the first bit of the next pass's range",
    "cd.cut.val.kept": "k_hz_codes: a value whose last bit is bit 6 of byte len-1: bytepos == len-1 after it, the last that can be kept",
    "cd.cut.val.flush": "k_hz_codes: a value whose last bit is the last bit of byte len-1: bytepos == len, dropped with all after it",
    "cd.cut.val.next": "k_hz_codes: a value whose last bit (its sign) is the first bit of byte len: dropped",
    "cd.cut.last.kept": "k_hz_codes: the final code's sign bit is bit 6 of byte len-1: kept",
    "cd.cut.last.flush": "k_hz_codes: the final code's sign bit is the last bit of byte len-1: dropped",
    "cd.cut.last.next": "k_hz_codes: the final code's sign bit is the first bit of byte len: dropped",
    # k_hz_positions
    "po.pass1": "k_hz_positions: at most PARSE_THREADS * POS_ITEMS - 1 entries: one pass",
    "po.pass2": "k_hz_positions: more entries: s_q carries the position into the next pass",
    "po.vec": "k_hz_positions: a thread with eight entries: the two 16-byte stores",
    "po.tail": "k_hz_positions: the thread with the last entries and fewer than eight: the tail store",
    "po.last_cell": "k_hz_positions: an entry at nscan-1, kept",
    "po.nscan": "k_hz_positions: an entry at nscan, dropped: dec_cnt counts the prefix",
    "po.sum64": "k_hz_positions: a running position of 2^32 or more (the 64-bit accumulator)",
    # scatter
    "sc.pos0": "k_hz_scatter_lv: an entry i >= 1 at position 0, the DC's cell: it stores nothing, the DC stands (hzcc.c:495)",
    "sc.ll": "k_hz_scatter_lv: an entry in the LL region past cell 0",
    "sc.lv0": "k_hz_scatter_lv: an entry in level group 0",
    "sc.lv1": "k_hz_scatter_lv: an entry in level group 1",
    "sc.lv2": "k_hz_scatter_lv: an entry in level group 2 (dequantH)",
    # (the int32 path's ordered phases; on the symbol path the same cells are k_hz_dec_resolve's, which tests/test_gpu_decode_escape.py
    # runs at 250x130)
    **{"sc.shared.%d%d.both" % (l, l + 1): "k_hz_scatter_lv, int32 path: a cell of a level-%d and a level-%d region with both symbols present: the later one wins (phase %d stores after phase %d)" % (l, l + 1, l + 1, l) for l in (0, 1)},
    **{"sc.shared.%d%d.earlier" % (l, l + 1): "k_hz_scatter_lv, int32 path: a cell of a level-%d and a level-%d region with only the earlier symbol: its value stays" % (l, l + 1) for l in (0, 1)},
    # seams and launchers (declared by the call, see call_labels)
    "sc.i32": "k_hz_scatter_lv: the int32 path (dec_sym == 0): dequantised coefficient into the plane",
    "sc.sym": "k_hz_scatter_lv / k_hz_unscatter: the int16 symbol path (dec_sym == 1)",
    "cl.sym": "k_dec_clear: a symbol-path plane: LL region and patch flags",
    "cl.vec": "k_dec_clear: an int32 plane, 16-byte stores",
    "cl.scalar": "k_dec_clear: an int32 plane's scalar stores (plane not 16-byte aligned or w*h not a multiple of 4)",
    "la.scatter1": "launch_hz_parse_scatter: every plane of the call on the symbol path: one scatter launch",
    "la.scatter3": "launch_hz_parse_scatter: a plane of the call keeps int32 coefficients: three scatter launches",
    "la.ip": "launch_hz_parse_scatter: a call with an I and a P picture",
    "la.mixed": "k_hz_scatter_lv: I pictures on int32 coefficients beside P pictures on the symbol path in one call (DSV1_NO_DEC_SYM_I): the first launch serves every entry of the symbol planes and level group 0 of the others, launches 1 and 2 skip the symbol planes (dec_sym || ph != phase)",
    "la.unequal": "launchers: jobs of unequal payload in one call: grids sized by the largest, the small job's threads leave early",
}

# Labels no payload the reference defines can reach, with the derivation.  A run is an int (hzcc.c:303), so a run code holds at
# most 2^31 - 1 + 1 -> 61 bits; a value times its quantiser (>= 16, or a shift >= 4) must fit an int, so a value code has at
# most 2 * 26 + 2 = 54 bits.  Every code the reference defines is therefore at most 61 bits long.
UNREACHABLE = {
    "cd.rel_neg": "rel < 0 needs a code that starts more than 64 bits before the chunk it ends in: longer than 64 bits; a run of 2^32 or more overflows the reference's int",
    "cd.start.prev.al": "a code from bit 0 of the previous chunk's second word that ends in this chunk has at least 65 bits: a run beyond the reference's int",
    "pa.m0_empty": "64 bits without a code end, with one behind them, need a code of at least 65 bits: a run beyond the reference's int",
    "pa.lbefore_neg": "128 bits of a pass without a code end, with one behind them, need a code of at least 129 bits: a run beyond the reference's int",
    "cl.scalar": "the pipeline refuses odd luma sides and rounds chroma sides up to even: every plane holds a multiple of 4 coefficients and starts 16-byte aligned (the operator never clears); no geometry reaches it",
    "pa.end.keep_64": "keep = 8 * len - S0 - 128 i is odd for every input: the header ends byte-aligned (hzcc.c:309-311) and U(run_1) has an odd number of bits; no payload at all reaches it",
}


def scatter_launches(kinds, sym=True, sym_i=True):
    """k_hz_scatter_lv launches of one decoder call (dsvg_decode_pictures' all_sparse argument of launch_hz_parse_scatter): one
    where every plane of every job is on the symbol path -- the P pictures unless DSV1_NO_DEC_SYM (sym False), the I pictures
    unless that or DSV1_NO_DEC_SYM_I (sym_i False) --, else three.  For geometries whose planes all qualify for the symbol path"""
    return 1 if sym and (sym_i or "I" not in kinds) else 3


def call_labels(kinds, sym=True, lens=None, sym_i=True):
    """labels of one decoder call of the pipeline: kinds 'I' / 'P' per job, the switches as in scatter_launches, lens the payload
    bytes of the jobs' planes"""
    one = scatter_launches(kinds, sym, sym_i) == 1
    out = {"la.scatter1" if one else "la.scatter3"}
    out |= {"sc.sym", "cl.sym"} if sym and (sym_i or "P" in kinds) else set()
    out |= {"sc.i32", "cl.vec"} if not one else set()
    if "I" in kinds and "P" in kinds:
        out.add("la.ip")
        if sym and not sym_i:
            out.add("la.mixed")
    if lens and max(lens) >= 16 * max(min(lens), 1):
        out.add("la.unequal")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
class Chunk:
    """one 128-bit chunk of k_hz_parse: pass, thread, first bit B, entering state, code ends (chunk bit offsets), cbase, prev_end"""

    def __init__(self, npass, tid, B, st_in, ends, cbase, prev_end, keep, from_carry):
        self.npass, self.tid, self.B, self.st_in, self.ends, self.cbase, self.prev_end, self.keep = npass, tid, B, st_in, ends, cbase, prev_end, keep
        self.from_carry = from_carry                      # prev_end is the carried s_lastend (lbefore < 0)
        self.labels = set()
        self.codes = []                                   # (code index j, kind 'run' | 'val' | 'last', entry, start bit, bits)

    def describe(self):
        return "pass %d thread %d (wave %d, chunk %d of the chain, bits %d..%d), entered in state %d (%s), %d code ends, cbase %d, prev_end %d; labels %s" % (
            self.npass, self.tid, self.tid // WAVE, self.npass * PARSE_THREADS + self.tid, self.B, self.B + PARSE_BITS - 1, self.st_in,
            STATE_NAMES[self.st_in], len(self.ends), self.cbase, self.prev_end, sorted(self.labels))


class Plane:
    """the decoder's facts of one plane: buf = the bytes behind the plane's length word (guard bytes included), length = `len`"""

    def __init__(self, w, h, buf, length):
        self.w, self.h, self.length = w, h, length
        self.ll_end, self.nscan, self.nchunks = H.geometry(w, h)
        rd = Bits(buf)
        self.dc, self.runs, self.start0 = read_header(rd)
        self.endbits = 8 * length
        # what the device holds: `len` bytes, zeros behind them
        self.dev = rd.b[:self.endbits] + [0] * (3 * 64 + 64)
        self.labels, self.chunks = set(), []
        self.R, self.V = {}, {}                           # run_m, value_m as k_hz_codes leaves them
        self.entry_chunk = {}                             # entry m -> the chunk its value was decoded in
        self.first_bad, self.ncode, self.npass = INT_MAX, 0, 0
        self._parse()
        self._positions()
        self._scatter_labels()
        for c in self.chunks:
            self.labels |= c.labels

    def bit(self, i):
        return self.dev[i] if i < len(self.dev) else 0

    def ueg_at(self, start, nbits):
        """value of the U code in bits [start, start + nbits), nbits = 2k + 1"""
        k, m = (nbits - 1) >> 1, 1
        for i in range(k):
            m = (m << 1) | self.bit(start + 2 * i + 1)
        return m - 1

    # -----------------------------------------------------------------------------------------------------------------------
    def _parse(self):
        L = self.labels
        cap = self.nchunks * HZ_CHUNK - 1
        self.n = n = min(self.runs, cap)
        if n <= 0:
            L.add("pa.runs0" if self.runs == 0 else "pa.runs_neg")
            return
        if self.runs > cap:
            L.add("pa.runs_clamped")
        # U(run_1), thread 0: the first '1' at an even offset of the 64 bits is the stop flag
        w = [self.bit(self.start0 + i) for i in range(64)]
        flags = [i for i in range(0, 64, 2) if w[i]]
        k = flags[0] >> 1 if flags else (32 if any(w) else 31)       # (no flag in sight: only where the data ends inside the code)
        ulen = 2 * k + 1
        if not any(w):
            L.add("pa.u1.w0")
        self.S0 = S0 = self.start0 + ulen
        if S0 >= self.endbits:
            L.add("pa.u1.cut")
        else:
            self.R[1] = self.ueg_at(self.start0, ulen)
            if ulen == 1 or ulen > 31:
                L.add("pa.u1.len1" if ulen == 1 else "pa.u1.gt31")
        self.ncodes = ncodes = 2 * n - 1
        state, ncode, lastend, pbase = 0, 0, S0, S0
        while pbase < self.endbits and ncode < ncodes:
            if self.npass:
                L.add("pa.pass.s%d" % state)
            pass_lastend, lbefore = lastend, -1
            for tid in range(PARSE_THREADS):
                B = pbase + tid * PARSE_BITS
                keep = self.endbits - B
                st_in, ends = state, []
                if keep <= 0:                              # 128 zero bits: a pending sign ends at once, the rest toggles in pairs
                    if state == 4:
                        ends, state = [0], 1
                else:
                    for i in range(PARSE_BITS):
                        state, e = STEP[state][self.bit(B + i) if i < keep else 0]
                        if e:
                            ends.append(i)
                prev_end = pbase + lbefore + 1 if lbefore >= 0 else pass_lastend
                if keep > 0:
                    c = Chunk(self.npass, tid, B, st_in, ends, ncode, prev_end, keep, lbefore < 0)
                    self.chunks.append(c)
                    c.labels.add("pa.chunk.s%d" % st_in)
                    if tid and tid % WAVE == 0:
                        c.labels.add("pa.wave.s%d" % st_in)
                    if keep < PARSE_BITS:
                        c.labels.add("pa.end.keep_lt64" if keep < 64 else "pa.end.keep_64" if keep == 64 else "pa.end.keep_gt64")
                    self._codes(c, pbase)
                else:
                    L.add("pa.end.past")
                ncode += len(ends)
                if ends:
                    lbefore = tid * PARSE_BITS + ends[-1]
            if lbefore >= 0:
                lastend = pbase + lbefore + 1
            pbase += PASS_BITS
            self.npass += 1
        self.ncode = ncode
        if self.npass:
            L.add("pa.pass%d" % min(self.npass, 3))
        if ncode >= ncodes:
            if ncode > ncodes:
                L.add("pa.all_found")
        else:
            L.add("pa.short.odd" if ncode & 1 else "pa.short.even")

    def _codes(self, c, pbase):
        """k_hz_codes on one chunk"""
        n, ncodes, dlen = self.n, self.ncodes, self.length
        j = c.cbase
        if not c.ends:
            c.labels.add("pa.m_none")
            return
        if j >= ncodes:
            return
        lo = [e for e in c.ends if e < 64]
        if not lo:
            c.labels.add("pa.m0_empty")
        if len(lo) == len(c.ends):
            c.labels.add("pa.m1_empty")
        prev_end = c.prev_end
        for e in c.ends:
            if j >= ncodes:
                break
            endp = c.B + e + 1
            nbits = min(endp - prev_end, 63)
            rel = prev_end - (c.B - 64)
            if rel < 0:
                c.labels.add("cd.rel_neg")
            else:
                c.labels.add("cd.start.%s.%s" % (("prev", "w0", "w1")[rel >> 6], "un" if rel & 63 else "al"))
            if prev_end < c.B:
                if c.tid == 0 and c.npass:
                    c.labels.add("pa.straddle.pass")
                elif c.tid % WAVE == 0 and c.tid:
                    c.labels.add("pa.straddle.wave")
                elif c.tid:
                    c.labels.add("pa.straddle.chunk")
                if c.tid and c.from_carry:
                    c.labels.add("pa.lbefore_neg")
            last, isN = j == ncodes - 1, bool(j & 1)
            ulen = nbits - 1 if isN else nbits
            mag = self.ueg_at(prev_end, ulen)
            sign = self.bit(prev_end + nbits - 1)
            if last:
                sign = self.bit(endp)
                c.labels.add("cd.last.sign.pass" if endp == pbase + PASS_BITS else "cd.last.sign.chunk" if endp == c.B + PARSE_BITS else "cd.last.sign.same")
                if n == 1:
                    c.labels.add("cd.last.n1")
            mi = n if last else (j + 1) >> 1
            if isN or last:
                self.V[mi] = -(mag + 1) if sign else mag + 1
                self.entry_chunk[mi] = c
                c.labels.add("cd.val.u31" if ulen <= 31 else "cd.val.u63")
                after = endp + (1 if last else 0)            # the bit after the value: the reference's pos
                if (after >> 3) >= dlen:
                    self.first_bad = min(self.first_bad, mi)
                kind = "last" if last else "val"
                if after == 8 * dlen - 1:
                    c.labels.add("cd.cut.%s.kept" % kind)
                elif after == 8 * dlen:
                    c.labels.add("cd.cut.%s.flush" % kind)
                elif after == 8 * dlen + 1:
                    c.labels.add("cd.cut.%s.next" % kind)
                c.codes.append((j, kind, mi, prev_end, nbits + (1 if last else 0)))
            else:
                self.R[(j >> 1) + 2] = mag
                c.labels.add("cd.run.u31" if ulen <= 31 else "cd.run.u63")
                c.codes.append((j, "run", (j >> 1) + 2, prev_end, nbits))
            prev_end = endp
            j += 1

    # -----------------------------------------------------------------------------------------------------------------------
    def _positions(self):
        """k_hz_positions: nent usable entries, their positions by a 64-bit sum, the prefix inside the scan"""
        L = self.labels
        self.entries, self.nent = [], 0
        if self.n <= 0:
            return
        if self.ncode >= self.ncodes:
            nent = min(self.n, self.first_bad - 1)
        else:
            nent = min(self.ncode // 2, self.first_bad - 1)
        self.nent = nent
        L.add("po.pass1" if nent < PARSE_THREADS * POS_ITEMS else "po.pass2")
        if nent >= POS_ITEMS - 1:
            L.add("po.vec")
        if nent % POS_ITEMS != POS_ITEMS - 1 and nent >= 1:
            L.add("po.tail")
        q, prefix = 0, True
        for m in range(1, nent + 1):
            q += self.R[m] + (1 if m > 1 else 0)
            if q >= 1 << 32:
                L.add("po.sum64")
            if q < self.nscan and prefix:
                self.entries.append((q, self.V[m]))
                if q == self.nscan - 1:
                    L.add("po.last_cell")
            else:
                if q == self.nscan and prefix:
                    L.add("po.nscan")
                prefix = False                             # positions increase: what follows is outside as well

    def _scatter_labels(self):
        L = self.labels
        if not self.entries:
            return
        seen = {}
        shared = self._shared_cells() if H.overlaps(self.w, self.h) else set()
        r1, r4, r7 = (H.regions(self.w, self.h)[i][0] for i in (1, 4, 7))
        for p, v in self.entries:
            L.add("sc.pos0" if p == 0 else "sc.ll" if p < r1 else "sc.lv0" if p < r4 else "sc.lv1" if p < r7 else "sc.lv2")
            if shared:
                x, y, _ = H.cell_of(self.w, self.h, p)
                if (x, y) in shared:
                    seen.setdefault((x, y), []).append(p)
        for cell, ps in seen.items():
            first = shared_first(self.w, self.h, cell)
            lv = H.cell_of(self.w, self.h, first)[2]
            if len(ps) > 1:
                L.add("sc.shared.%d%d.both" % (lv, lv + 1))
            elif ps[0] == first:
                L.add("sc.shared.%d%d.earlier" % (lv, lv + 1))

    def _shared_cells(self):
        cnt = np.zeros((self.h + 8, self.w + 8), dtype=np.int32)
        for base, x0, y0, sw, sh, level in H.regions(self.w, self.h):
            cnt[y0:y0 + sh, x0:x0 + sw] += 1
        ys, xs = np.nonzero(cnt > 1)
        return {(int(x), int(y)) for x, y in zip(xs, ys)} - {(x, y) for x in range(H.rsu(self.w, 3)) for y in range(H.rsu(self.h, 3))}

    # -----------------------------------------------------------------------------------------------------------------------
    def explain(self, got, want):
        """where a decoded plane first differs from the expected one (int32, h x w), in the model's words"""
        bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
        if not bad.size:
            return "planes equal"
        cells = {}
        for m, (p, v) in enumerate(self.entries, 1):
            x, y, _ = H.cell_of(self.w, self.h, p)
            cells.setdefault(y * self.w + x, m)
        i = int(bad[0])
        msg = "%d cells differ, first (%d, %d): got %d want %d" % (bad.size, i % self.w, i // self.w, int(np.asarray(got).reshape(-1)[i]), int(np.asarray(want).reshape(-1)[i]))
        hit = [(m, cells[int(b)]) for m, b in enumerate(bad) if int(b) in cells]
        if i == 0:
            return msg + "; the DC's cell (dc %d, entries at position 0: %d)" % (self.dc, sum(p == 0 for p, _ in self.entries))
        if not hit:
            return msg + "; no entry of the %d expected ones lands there (nent %d, first_bad %d, ncode %d of %d)" % (len(self.entries), self.nent, self.first_bad, self.ncode, getattr(self, "ncodes", 0))
        m = hit[0][1]
        c = self.entry_chunk[m]
        return msg + "; first differing entry %d of %d (position %d, value %d), its value decoded in %s" % (m, len(self.entries), self.entries[m - 1][0], self.entries[m - 1][1], c.describe())


def shared_first(w, h, cell):
    """the scan position of a shared cell in the EARLIER of its regions"""
    for base, x0, y0, sw, sh, level in H.regions(w, h)[1:]:
        if x0 <= cell[0] < x0 + sw and y0 <= cell[1] < y0 + sh:
            return base + (cell[1] - y0) * sw + (cell[0] - x0)
    raise ValueError(cell)
