"""A model of the branches of the entropy pack stage (csrc/k_hzcc.hip: k_hz_quant, k_hz_collect(_list), k_hz_scan, k_hz_emit(_list)).

Pure Python and numpy; nothing of the product is loaded.  For ONE plane of ONE picture -- width, height, the picture kind, the
seam it came through and its entry list in scan order, (scan position, value), taken from the oracle -- the model restates

  * make_hz_plane (csrc/dsvg_common.hip): ll_end = rsu(w,3) * rsu(h,3), nscan, nchunks of HZ_CHUNK = 2048 scan cells;
  * which chunks are packed (one word per entry, collect_round_pk): in the pipeline the chunks whose base is at or past ll_end,
    through the operator (k_hz_quant<false>) none;
  * per chunk the entry count, the predecessor entry, the bit offset of its first code counted from the plane's first code
    (k_hz_scan starts s_c_bits at 0), and the rounds emit_chunk_t will run with the tier each takes in emit_round64;
  * the bits themselves, by a plain writer of the reference's rule (hzcc.c:137-293, bs.c:129-206): per entry UEG(run), then NEG
    of the previous value, and a trailing NEG of the last.  This is the high-precision reference of the stage: Python integers.

Out of those facts comes a set of LABELS, one per branch the kernels can take on the plane (LABELS below says which line each one
names).  tests/hz_cases.py lists the cases with the labels each is there for; tests/test_hz_plan_host.py proves on the CPU, from
the oracle alone, that every label is reached and that the writer's bytes are the oracle's; tests/test_gpu_hz_paths.py runs the
cases on the device and names chunk, rounds and labels where the bytes differ.
"""
import numpy as np

HZ_CHUNK = 2048
SCAN_ITEMS = 8                    # chunks per thread and tile of k_hz_scan


def rsu(x, s):
    return (x + (1 << s) - 1) >> s


def regions(w, h):
    """the ten scan regions of a w x h coefficient plane: [(base, x0, y0, sw, sh, level)] (make_hz_plane)"""
    out = [(0, 0, 0, rsu(w, 3), rsu(h, 3), -1)]
    base = rsu(w, 3) * rsu(h, 3)
    for l in range(3):
        sw, sh = rsu(w, 3 - l), rsu(h, 3 - l)
        for s in (1, 2, 3):
            out.append((base, sw if s & 1 else 0, sh if s & 2 else 0, sw, sh, l))
            base += sw * sh
    return out


def geometry(w, h):
    """(ll_end, nscan, nchunks)"""
    r = regions(w, h)
    nscan = r[-1][0] + r[-1][3] * r[-1][4]
    return r[1][0], nscan, (nscan + HZ_CHUNK - 1) // HZ_CHUNK


def overlaps(w, h):
    """some scan regions of the plane share cells (a side that is 1..4 modulo 8)"""
    return any(2 * rsu(d, 3 - l) > rsu(d, 2 - l) for d in (w, h) for l in (0, 1))


def cell_of(w, h, p):
    """(x, y, level) in the coefficient plane of scan cell p"""
    for base, x0, y0, sw, sh, level in reversed(regions(w, h)):
        if p >= base:
            return x0 + (p - base) % sw, y0 + (p - base) // sw, level
    raise ValueError(p)


def scan_threads(njobs):
    """launch_hz_pack: 1024 threads per plane for up to 32 jobs of three planes in the frame step, 256 beyond"""
    return 1024 if 3 * njobs <= 96 else 256


K_QUANT, K_QUANT_LL = "void k_hz_quant<false>", "void k_hz_quant<true>"
K_COLLECT, K_COLLECT_LIST, K_SCAN, K_EMIT, K_EMIT_LIST = "k_hz_collect", "k_hz_collect_list", "k_hz_scan", "k_hz_emit", "k_hz_emit_list"
ENTROPY_KERNELS = [K_QUANT, K_QUANT_LL, K_COLLECT, K_COLLECT_LIST, K_SCAN, K_EMIT, K_EMIT_LIST]


def step_kernels(kinds, llq=True, list_pack=True):
    """launches per entropy kernel of one frame step of the pipeline whose jobs are pictures of `kinds` ('I' / 'P')
    (launch_hz_quant, launch_hz_pack): dense jobs take the wave-per-chunk pair, sparse ones the list pair -- all of them the
    dense pair without list_pack (DSV1_NO_LIST_PACK) --, one scan, and k_hz_quant<true> only without llq (DSV1_NO_LLQ)"""
    dense = sum(k == "I" for k in kinds) if list_pack else len(kinds)
    sparse = len(kinds) - dense
    out = {K_SCAN: 1}
    if dense:
        out[K_COLLECT] = out[K_EMIT] = 1
    if sparse:
        out[K_COLLECT_LIST] = out[K_EMIT_LIST] = 1
    if not llq:
        out[K_QUANT_LL] = 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the codes (bs.c:129-206)
def len_ueg(v):
    return 2 * ((v + 1).bit_length() - 1) + 1


def len_neg(v):
    return len_ueg(abs(v) - 1) + 1


def code_ueg(v):
    """(pattern, length), MSB first: k x ('0', data bit) then '1'"""
    m = v + 1
    k = m.bit_length() - 1
    pat = 0
    for i in range(k - 1, -1, -1):
        pat = (pat << 2) | ((m >> i) & 1)
    return (pat << 1) | 1, 2 * k + 1


def code_neg(v):
    pat, n = code_ueg(abs(v) - 1)
    return (pat << 1) | (1 if v < 0 else 0), n + 1


def write_plane(entries):
    """the plane's payload by the reference's rule: (bytes zero-padded to a whole byte, bits)"""
    out, acc, fill, nbits, prev, held = bytearray(), 0, 0, 0, -1, 0

    def put(code):
        nonlocal acc, fill, nbits
        acc, fill, nbits = (acc << code[1]) | code[0], fill + code[1], nbits + code[1]
        while fill >= 8:                                  # whole bytes leave: the accumulator stays a small integer
            fill -= 8
            out.append(acc >> fill)
            acc &= (1 << fill) - 1
    for pos, val in entries:
        put(code_ueg(pos - prev - 1))
        if held:
            put(code_neg(held))
        prev, held = pos, val
    if held:
        put(code_neg(held))
    if fill:
        out.append(acc << (8 - fill))
    return bytes(out), nbits


# ---------------------------------------------------------------------------------------------------------------------------
# LABELS: name -> the code it stands for (k_hzcc.hip)
LABELS = {
    # emit_round64, one round of 64 entries (lane = entry; m = run + 1, mag = |previous value|)
    "r64.tier8": "every m and mag of the round below 256: both codes in one 32-bit pattern",
    "r64.tier15.run": "second tier (all below 32768) entered by m >= 256",
    "r64.tier15.mag": "second tier entered by mag >= 256",
    "r64.tier31.run": "third tier entered by m >= 32768",
    "r64.tier31.mag": "third tier entered by mag >= 32768",
    "r64.nfull0": "a round that completes no word: nfull == 0, everything stays in the carry",
    "r64.tier15.half2": "second tier, 64 + lane < nfull: the words of the stage's second half leave too",
    # emit_chunk_t<true>
    "pk.le64": "packed chunk of at most 64 entries: one round of 64",
    "pk.65_128": "packed chunk of 65..128 entries: two rounds of 64",
    "pk.129_256": "packed chunk of 129..256 entries: one round of 256 with idle lanes",
    "pk.256s_tail": "packed chunk of rounds of 256 followed by a tail of 64s",
    "pk.256s": "packed chunk of more than 256 entries whose last round is one of 256 (129..256 left)",
    "pk.r256": "a round of 256 entries assembled as one (no run or value of 256 or more in it)",
    "pk.detour.run": "a round of 256 done as four rounds of 64 because of m >= 256",
    "pk.detour.mag": "a round of 256 done as four rounds of 64 because of mag >= 256",
    "pk.detour.first": "the detour in the chunk's first round: lane 0's predecessor is the carried-in one",
    "pk.r64.tier31.run": "third tier entered by a run inside a packed chunk's rounds of 64",
    "pk.r64.tier31.mag": "third tier entered by the magnitude of a packed chunk's own entry",
    # emit_chunk_t<false>
    "un.one": "unpacked chunk, one round",
    "un.many": "unpacked chunk, several rounds",
    # a chunk's first and last word (first_pending / firstv / carry and the closing atomicOr's)
    "w.single": "all of the chunk's bits inside one word that they do not complete: first_pending still set at the close",
    "w.bit0": "the chunk begins at bit 0 of a word",
    "w.endword": "the chunk ends on a word boundary: the final carry is 0",
    "w.first_shared": "the chunk's first word also holds bits of the chunk before",
    "w.last_shared": "the chunk's last word also holds bits of the chunk after",
    "w.single_both": "first and last word are one word, shared with both neighbours",
    # the plane
    "pl.empty": "no entries",
    "pl.one": "one entry",
    "pl.last_ne_not_last": "the last non-empty chunk is not the plane's last chunk",
    "pl.first_ne_not_0": "the first non-empty chunk is not chunk 0",
    "pl.run_gt16": "a run that crosses more than 16 empty chunks",
    # collect (pipeline seam)
    "co.dense": "dense chunk (I picture, chunk past the LL region): collect_chunk's plain loads",
    "co.sparse.flag": "sparse chunk, flagged: symbols fetched where the group flags are up",
    "co.sparse.noflag": "sparse chunk, unflagged: the empty summary",
    "co.ll.whole": "LL chunk wholly inside the LL region: collect_chunk_ll's 32-byte loads only",
    "co.straddle.dense.detail": "the chunk that straddles ll_end, dense picture, detail entries in it",
    "co.straddle.dense.nodetail": "the chunk that straddles ll_end, dense picture, no detail entry",
    "co.straddle.sparse.flag": "the chunk that straddles ll_end, sparse picture, its flag raised (detail entries)",
    "co.straddle.sparse.noflag": "the chunk that straddles ll_end, sparse picture, no flag",
    "co.ll_end.8": "ll_end a multiple of 8: no lane's eight cells straddle it",
    "co.ll_end.n8": "ll_end not a multiple of 8",
    "co.ll_end.n4": "ll_end not a multiple of 4: a flag byte's four cells straddle it",
    "co.short_last": "the plane's last chunk cut short by nscan",
    # k_hz_scan
    "sc.1024": "the 1024-thread variant",
    "sc.256": "the 256-thread variant",
    "sc.tile2.entries": "a second tile with entries whose first non-empty chunk takes its predecessor from the first tile",
    "sc.tile2.empty": "a second tile with no entries: the plane's last chunk is found through the carry",
    "sc.tile2.first": "the plane's first non-empty chunk lies in the second tile",
}

# Labels no input reaches, with the derivation.  Each is either reached through the other seam under another name, or its code is
# shown dead.
UNREACHABLE = {
    # A packed chunk's entries are (symbol << 16) | position words (collect_round_pk), the symbol an int16 of jb.sym.  The packed
    # chunks hold detail cells of transform levels 1..3 only, whose coefficients are at most 26212 in magnitude
    # (tests/test_symbol_range.py derives the bound from the filter gains and checks it against the oracle), and a symbol is
    # never larger than its coefficient (quantisers >= 16, shifts >= 1).  So no entry of a packed chunk has |v| >= 32768, and
    # the ballot of emit_round64's third tier is never raised by the value of a packed chunk's own entry: that is what this
    # label names, and the model raises it for own entries only.  The one value such a round takes from outside the chunk is
    # lane 0's carried-in predecessor (cs.prev_val, an int32 that may come from an LL chunk); a round it sends to the third tier is
    # labelled "r64.tier31.mag" like any other, the same lines of emit_round64 that the operator seam runs on int32 symbols.
    "pk.r64.tier31.mag": "int16 symbols, |v| <= 26212 in a packed chunk; the tier's code is reached at the operator seam (r64.tier31.mag)",
}


class Round:
    """one pass of the emit loop: kind 'r64' (emit_round64) or 'r256'; first entry, entries, bits, tier (r64: 8, 15, 31), why the
    tier was entered, complete words nfull, and whether it is part of a detour"""

    def __init__(self, kind, first, n, bits, o0, tier=8, by=(), detour=()):
        self.kind, self.first, self.n, self.bits, self.o0, self.tier, self.by, self.detour = kind, first, n, bits, o0, tier, tuple(by), tuple(detour)
        self.nfull = (o0 + bits) >> 5

    def __repr__(self):
        if self.kind == "r256":
            return "round of 256 (%d entries, %d bits, %d words)" % (self.n, self.bits, self.nfull)
        s = "round of 64 (%d entries, %d bits, %d words, tier <2^%d%s)" % (self.n, self.bits, self.nfull, self.tier, " by " + "+".join(self.by) if self.by else "")
        return s + (" in a round of 256 detoured by " + "+".join(self.detour) if self.detour else "")


class Chunk:
    def __init__(self, index, packed, lo, hi, prev, bit_off):
        self.index, self.packed, self.lo, self.hi, self.prev, self.bit_off = index, packed, lo, hi, prev, bit_off
        self.nnz = hi - lo
        self.rounds, self.bits, self.labels = [], 0, set()

    def describe(self):
        return "chunk %d, %s, %d entries at bit %d: %s; labels %s" % (
            self.index, "packed" if self.packed else "unpacked", self.nnz, self.bit_off,
            ", ".join(map(repr, self.rounds)) or "no rounds", sorted(self.labels))


def _round64(pos, val, lo, hi, j0, prev, o0, detour=()):
    """emit_round64 on entries [j0, min(j0 + 64, hi)) of the chunk [lo, hi); prev = the plane's entry before the chunk or None"""
    ms, mags, bits = [], [], 0
    for j in range(j0, min(j0 + 64, hi)):
        pp, pv = (pos[j - 1], val[j - 1]) if j > lo else (prev if prev else (-1, 0))
        m = pos[j] - pp                                   # UEG codes run + 1
        bits += 2 * (m.bit_length() - 1) + 1
        ms.append(m)
        if j > lo or prev:
            mags.append(abs(pv))
            bits += len_neg(pv)
    big = max(ms + mags)
    tier = 8 if big < 256 else (15 if big < 32768 else 31)
    lim = {8: 0, 15: 256, 31: 32768}[tier]
    by = [k for k, v in (("run", ms), ("mag", mags)) if tier > 8 and v and max(v) >= lim]
    return Round("r64", j0 - lo, min(j0 + 64, hi) - j0, bits, o0, tier, by, detour)


class Plane:
    """the pack stage's facts of one plane.  kind: 'I' (dense) or 'P' (sparse); seam: 'pipe' (fused: the chunks past ll_end packed)
    or 'op' (k_hz_quant<false>: nothing packed); njobs: jobs of the frame step on the coding stream.  The pipeline's two A/B switches
    leave these facts as they are: without llq the LL chunks are compacted by k_hz_quant<true>, unpacked as before, and without the
    list kernels a P picture's chunks still go by their flags (collect_chunk<false> reads the chunk flag itself), so 'sparse,
    flagged / unflagged' describes them under either launch"""

    def __init__(self, w, h, entries, kind="I", seam="op", njobs=1):
        self.w, self.h, self.kind, self.seam, self.njobs = w, h, kind, seam, njobs
        self.ll_end, self.nscan, self.nchunks = geometry(w, h)
        e = np.asarray(entries, dtype=np.int64).reshape(-1, 2)
        self.pos, self.val = [int(x) for x in e[:, 0]], [int(x) for x in e[:, 1]]
        assert all(a < b for a, b in zip(self.pos, self.pos[1:])) and all(self.val), "entries are in scan order and not zero"
        assert not self.pos or (0 < self.pos[0] and self.pos[-1] < self.nscan), "entry outside the scan"
        self.labels = set()
        self.chunks = []
        self._build()

    def packed(self, chunk):
        return self.seam != "op" and chunk * HZ_CHUNK >= self.ll_end

    def _build(self):
        pos, val = self.pos, self.val
        cut = np.searchsorted(np.asarray(pos, dtype=np.int64), np.arange(self.nchunks + 1) * HZ_CHUNK)
        bit = 0
        for k in range(self.nchunks):
            lo, hi = int(cut[k]), int(cut[k + 1])
            ch = Chunk(k, self.packed(k), lo, hi, (pos[lo - 1], val[lo - 1]) if lo else None, bit)
            if hi > lo:
                self._rounds(ch)
            bit += ch.bits
            self.chunks.append(ch)
        self.bits_chunks = bit
        self.total_bits = bit + (len_neg(val[-1]) if val else 0)
        self._chunk_labels()
        self._plane_labels()

    def _rounds(self, ch):
        pos, val, lo, hi = self.pos, self.val, ch.lo, ch.hi
        at = ch.bit_off & 31

        def add(r):
            nonlocal at
            ch.rounds.append(r)
            at += r.bits
        if not ch.packed:
            for j0 in range(lo, hi, 64):
                add(_round64(pos, val, lo, hi, j0, ch.prev, at & 31))
            ch.labels.add("un.one" if len(ch.rounds) == 1 else "un.many")
        else:
            base, tail = lo, False
            while base < hi:
                if hi - base <= 128:
                    tail = base > lo
                    add(_round64(pos, val, lo, hi, base, ch.prev, at & 31))
                    base += 64
                    continue
                top = min(base + 256, hi)
                ms, mags, bits = [], [], 0
                for j in range(base, top):
                    pp, pv = (pos[j - 1], val[j - 1]) if j > lo else (ch.prev if ch.prev else (-1, 0))
                    ms.append(pos[j] - pp)
                    bits += 2 * (ms[-1].bit_length() - 1) + 1
                    if j > lo or ch.prev:
                        mags.append(abs(pv))
                        bits += len_neg(pv)
                why = [k for k, v in (("run", ms), ("mag", mags)) if v and max(v) >= 256]
                if why:
                    for r in range(4):
                        if base + 64 * r < hi:
                            add(_round64(pos, val, lo, hi, base + 64 * r, ch.prev, at & 31, detour=why))
                    if len(why) == 1:                     # (a label names ONE cause: a round with both proves neither)
                        ch.labels.add("pk.detour." + why[0])
                    if base == lo:
                        ch.labels.add("pk.detour.first")
                else:
                    add(Round("r256", base - lo, top - base, bits, at & 31))
                    ch.labels.add("pk.r256")
                base += 256
            n = ch.nnz
            ch.labels.add("pk.le64" if n <= 64 else "pk.65_128" if n <= 128 else "pk.129_256" if n <= 256 else "pk.256s_tail" if tail else "pk.256s")
        for r in ch.rounds:
            if r.kind != "r64":
                continue
            if r.tier == 8:
                ch.labels.add("r64.tier8")
            if len(r.by) == 1:                            # (one cause, as above)
                ch.labels.add("r64.tier%d.%s" % (r.tier, r.by[0]))
                # (in a packed chunk the value label counts the chunk's OWN entries: lane 0's carried-in predecessor may come from
                # an LL chunk, see UNREACHABLE)
                if ch.packed and r.tier == 31 and (r.by[0] == "run" or max(abs(v) for v in val[lo:hi]) >= 32768):
                    ch.labels.add("pk.r64.tier31." + r.by[0])
            if r.nfull == 0:
                ch.labels.add("r64.nfull0")
            if r.tier == 15 and r.nfull > 64:
                ch.labels.add("r64.tier15.half2")
        ch.bits = sum(r.bits for r in ch.rounds)
        assert sum(r.n for r in ch.rounds) == ch.nnz

    def _chunk_labels(self):
        ne = [c for c in self.chunks if c.nnz]
        for i, c in enumerate(ne):
            o0, end = c.bit_off & 31, c.bit_off + c.bits
            single = o0 + c.bits < 32                     # no round ever has nfull > 0
            after = i + 1 < len(ne)
            if single:
                c.labels.add("w.single")
            if o0 == 0:
                c.labels.add("w.bit0")
            else:
                c.labels.add("w.first_shared")            # (bit_off > 0: the bits before it are an earlier chunk's)
            if end & 31 == 0:
                c.labels.add("w.endword")
            elif after:
                c.labels.add("w.last_shared")
            if single and o0 and after:
                c.labels.add("w.single_both")
        for c in self.chunks:
            self.labels |= c.labels

    def _plane_labels(self):
        L, ne = self.labels, [c.index for c in self.chunks if c.nnz]
        if not ne:
            L.add("pl.empty")
        else:
            if len(self.pos) == 1:
                L.add("pl.one")
            if ne[-1] != self.nchunks - 1:
                L.add("pl.last_ne_not_last")
            if ne[0] != 0:
                L.add("pl.first_ne_not_0")
            if any(b - a - 1 > 16 for a, b in zip(ne, ne[1:])) or ne[0] > 16:
                L.add("pl.run_gt16")
        nt = scan_threads(self.njobs)
        L.add("sc.%d" % nt)
        tile = nt * SCAN_ITEMS
        if self.nchunks > tile:
            in2 = [k for k in ne if k >= tile]
            if in2 and ne[0] < tile:
                L.add("sc.tile2.entries")
            if in2 and ne[0] >= tile:
                L.add("sc.tile2.first")
            if not in2 and ne:
                L.add("sc.tile2.empty")
        if self.seam == "op":
            return
        le = self.ll_end
        L.add("co.ll_end.8" if le % 8 == 0 else "co.ll_end.n8")
        if le % 4:
            L.add("co.ll_end.n4")
        if self.nscan % HZ_CHUNK:
            L.add("co.short_last")
        for c in self.chunks:
            cb = c.index * HZ_CHUNK
            if cb >= le:
                L.add("co.dense" if self.kind == "I" else ("co.sparse.flag" if c.nnz else "co.sparse.noflag"))
            elif cb + HZ_CHUNK <= le:
                L.add("co.ll.whole")
            else:
                detail = any(p >= le for p in self.pos[c.lo:c.hi])
                if self.kind == "I":
                    L.add("co.straddle.dense.detail" if detail else "co.straddle.dense.nodetail")
                else:
                    L.add("co.straddle.sparse.flag" if detail else "co.straddle.sparse.noflag")

    # -----------------------------------------------------------------------------------------------------------------------
    def chunk_of_bit(self, bit):
        """the chunk whose codes hold payload bit `bit` (None: the trailing value or past the end)"""
        for c in self.chunks:
            if c.nnz and c.bit_off <= bit < c.bit_off + c.bits:
                return c
        return None

    def explain(self, got, want):
        """where two payloads of this plane (bytes) first differ, in the model's words"""
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        if first == n and len(got) == len(want):
            return "payloads equal"
        x = (got[first] ^ want[first]) if first < n else 0x80
        bit = 8 * first + (8 - x.bit_length())
        c = self.chunk_of_bit(bit)
        if c is None:
            return "first differing bit %d of %d: past the chunks' codes (the trailing value, %d bits)" % (bit, self.total_bits, self.total_bits - self.bits_chunks)
        at, where = c.bit_off, "?"
        for r in c.rounds:
            if bit < at + r.bits:
                where = repr(r)
                break
            at += r.bits
        return "first differing bit %d (word %d): %s; the bit is in its %s" % (bit, bit >> 5, c.describe(), where)
